"""rows_retire: at a tile's end conv3x3_rows<16> finishes and stores output rows 0 and 1 (and their 2x2 pool) between
the last step's two barriers, waves 0-3 before and waves 4-7 behind their MFMAs of input rows 4 and 5, and rows 2 and 3
after the step.  It must write, bit for bit, what the tail epilogue (rows_retire=0) and the streaming patch kernel
(rows_kernel=0) write: y and the fused pool.

Every output buffer is pre-filled with a bf16 NaN pattern no conv of finite inputs stores, so an output nobody wrote
and a store outside the view both show.  The shapes are the smallest that reach each path: one granule (every step is a
tile end), two and three granules (a tile end on either step parity), partial tiles, the pool on odd and even sizes,
channel-slice views, one tile per block, three tiles per resident block, a captured graph, and the f16x3 form, which
keeps its tail epilogue.  All are forced onto the row-stationary kernel (rows_kernel=16)."""

import numpy as np
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

DEV = "cuda"
SENT = 0x7FC1  # a bf16 / fp16 NaN pattern
DEFAULTS = {"rows_retire": 1, "rows_kernel": 1}
ROWS16 = "vm::conv3x3_rows<16>"

# (n, h, w, cin, cout, pool, view offset, act)
CASES = [
    (1, 16, 32, 32, 64, False, 0, "relu"),     # one tile, one granule: its first step is its last
    (1, 16, 32, 64, 64, False, 0, "relu"),     # two granules: the tile ends on the odd step
    (1, 16, 32, 96, 64, False, 0, "relu"),     # three: on the even step
    (1, 17, 33, 64, 64, False, 0, "relu"),     # partial tile row and column (early and late rows masked alike)
    (1, 31, 40, 96, 64, False, 0, "none"),     # ... and no activation
    (1, 17, 35, 64, 64, True, 0, "relu"),      # pool, odd sizes: the last window holds one row / column
    (1, 32, 64, 64, 64, True, 0, "relu"),      # pool, even sizes
    (1, 17, 35, 32, 64, True, 0, "relu"),      # pool with one granule
    (1, 32, 64, 96, 128, True, 0, "none"),     # pool, three granules, two channel tiles
    (1, 17, 33, 64, 64, False, 64, "relu"),    # [..., 64:128] of a 128-channel tensor
    (1, 17, 33, 64, 128, True, 64, "relu"),    # [..., 64:192] of a 256-channel tensor, with the pool
    (2, 64, 64, 64, 256, True, 0, "relu"),     # 64 tiles: a batch, four channel tiles per patch
    (1, 384, 256, 64, 256, True, 0, "relu"),   # 768 tiles: three per resident block (accumulator restart, DMA stream)
]


class options:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        from vmatting import _lib
        for k, v in self.kv.items():
            _lib.set_option(k, v)

    def __exit__(self, *exc):
        from vmatting import _lib
        for k in self.kv:
            _lib.set_option(k, DEFAULTS[k])


def bits(t):
    return t.contiguous().view(torch.int16)


def sentinel(shape, dtype=torch.bfloat16):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.int16).fill_(SENT)
    return t


class Case:
    """One conv: its operands (made once) and run() -> (y buffer, pool buffer or None, kernel name)."""

    def __init__(self, case):
        from vmatting import ops
        self.n, self.h, self.w, self.cin, self.cout, self.pool, self.off, self.act = case
        n, h, w, cin, cout = case[:5]
        rs = np.random.RandomState(h * 131 + w * 7 + cin + cout + n)
        self.x = torch.from_numpy(rs.normal(size=(n, h, w, cin)).astype(np.float32)).to(torch.bfloat16).to(DEV)
        wt = (rs.normal(size=(3, 3, cin, cout)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
        # bias and a folded-BN affine: every constant of the epilogue differs per channel
        self.pc = ops.PackedConv(wt, (rs.normal(size=cout) * 0.1).astype(np.float32), torch.bfloat16, DEV,
                                 scale=(1.0 + 0.1 * rs.normal(size=cout)).astype(np.float32),
                                 shift=(0.1 * rs.normal(size=cout)).astype(np.float32))

    def buffers(self):
        n, h, w, cout = self.n, self.h, self.w, self.cout
        ybuf = sentinel((n, h, w, 2 * self.off + cout))
        pbuf = sentinel((n, (h + 1) // 2, (w + 1) // 2, cout)) if self.pool else None
        return ybuf, pbuf

    def view(self, ybuf):
        return ybuf[..., self.off:self.off + self.cout]

    def call(self, ybuf, pbuf):
        from vmatting import ops
        ops.conv3x3(self.x, self.pc, self.act, out=self.view(ybuf), pool_out=pbuf)

    def run(self):
        from vmatting import _lib
        ybuf, pbuf = self.buffers()
        self.call(ybuf, pbuf)
        torch.cuda.synchronize()
        return ybuf, pbuf, _lib.last_conv_kernel()

    def check_written(self, ybuf, pbuf):
        """Every output of the view and of the pool was written, nothing outside the view."""
        y = bits(ybuf)
        assert not bool((y[..., self.off:self.off + self.cout] == SENT).any()), "an output kept its sentinel"
        if self.off:
            assert bool((y[..., :self.off] == SENT).all()) and bool((y[..., self.off + self.cout:] == SENT).all()), \
                "a store outside the channel slice"
        if pbuf is not None:
            assert not bool((bits(pbuf) == SENT).any()), "a pooled output kept its sentinel"


def same(a, b):
    return a is None and b is None or torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_retired_rows_bit_identical(case):
    c = Case(case)
    with options(rows_kernel=16, rows_retire=1):
        y1, p1, k1 = c.run()
    with options(rows_kernel=16, rows_retire=0):
        y0, p0, k0 = c.run()
    with options(rows_kernel=0):
        ys, ps, ks = c.run()
    assert k1 == ROWS16 and k0 == ROWS16 and ks.startswith("vm::conv3x3_patch"), (k1, k0, ks)
    for y, p in ((y1, p1), (y0, p0), (ys, ps)):
        c.check_written(y, p)
    assert same(y1, y0), "y differs from the tail epilogue's"
    assert same(p1, p0), "the pool differs from the tail epilogue's"
    assert same(y1, ys), "y differs from the streaming patch kernel's"
    assert same(p1, ps), "the pool differs from the streaming patch kernel's"


def test_retired_rows_in_a_captured_graph():
    """The 17 x 35 pool case captured in a HIP graph and replayed twice, the outputs reset to the sentinel in between."""
    from vmatting import _lib
    c = Case(CASES[5])
    assert c.pool and (c.h, c.w) == (17, 35)
    with options(rows_kernel=16, rows_retire=1):
        y0, p0, k0 = c.run()  # eager
        assert k0 == ROWS16
        ybuf, pbuf = c.buffers()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            c.call(ybuf, pbuf)  # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            c.call(ybuf, pbuf)
        assert _lib.last_conv_kernel() == ROWS16
    fresh_y, fresh_p = c.buffers()
    for _ in range(2):
        ybuf.copy_(fresh_y)
        pbuf.copy_(fresh_p)
        graph.replay()
        torch.cuda.synchronize()
        assert same(ybuf, y0) and same(pbuf, p0)


def test_f16x3_form_keeps_its_bits():
    """conv3x3_rows<16, true> (the split-fp16 x3 form) keeps the tail epilogue: rows_retire does not reach it."""
    from vmatting import _lib, ops, split3
    n, h, w, cin, cout = 1, 32, 64, 64, 64
    rs = np.random.RandomState(11)
    x = (rs.randn(n, h, w, cin) * 300).astype(np.float32)
    wt = (rs.randn(3, 3, cin, cout) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    t = split3.filter_scale(wt)
    pc = ops.PackedConv(split3.split3_filter(wt, cin, cout, t), None, "f16", DEV,
                        scale=np.full(cout, 1.0 / t, np.float32), shift=rs.randn(cout).astype(np.float32))
    xs = torch.zeros((n, h, w, 2 * cin), dtype=torch.float16, device=DEV)
    split3.split3h(torch.from_numpy(x).to(DEV), xs[..., :cin])
    out = []
    for retire in (1, 0):
        buf = sentinel((n, h, w, 2 * cout), torch.float16)
        with options(rows_kernel=16, rows_retire=retire):
            split3.conv_split(xs, pc, buf[..., :cout], "relu", splitk=False)
            assert _lib.last_conv_kernel() == "vm::conv3x3_rows<16, true>", _lib.last_conv_kernel()
        torch.cuda.synchronize()
        assert not bool((bits(buf) == SENT).any())
        out.append(buf)
    assert same(out[0], out[1])
