"""border_fuse: the folded upconv's border pass run by extra blocks of the folded kernel's own launch (1 = the
streaming kernel, 2 = the persistent one too) writes, bit for bit, what the separate border launch (0) writes: y, and
with the head split the per-tap partials, with y left alone under store_y = 0.

Every output buffer is pre-filled with a sentinel no kernel can produce (y: negative values under a relu; partials:
1e30 and up), so a pixel that nobody wrote, or that the main blocks wrote where the border blocks should have, shows.
The shapes are the smallest that reach each path: one tile, partial tile rows / columns, two phases per channel tile,
a frame that is almost all ring, a batch, a channel-slice output view, the head split; plus the smallest grids that
put the 8-wave streaming and persistent kernels (two border groups per block) to work."""

import numpy as np
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

DEV = "cuda"
DEFAULTS = {"border_fuse": 2, "patch_cfg": 0, "persist_up_rounds": 6}

# (n, h, w, cin, cout, kind): kind "plain", "view" (channel-slice output, coff > 0, cstride > cout) or "head"
CASES = [
    (1, 8, 32, 32, 64, "plain"),    # exactly one tile
    (1, 9, 40, 32, 64, "plain"),    # partial tile row and column
    (1, 17, 33, 64, 128, "plain"),  # odd sizes, two phases per channel tile
    (1, 3, 5, 32, 64, "plain"),     # almost all ring
    (2, 9, 40, 32, 64, "plain"),    # batch
    (1, 9, 40, 32, 64, "view"),     # cat-buffer style view
    (1, 9, 40, 64, 64, "head"),     # partials path
]
# grids of >= 512 blocks of 64 channels: the 8-wave kernels, whose border blocks hold two 4-wave groups
BIG = [(1, 100, 300, 64, 64, "head"), (1, 60, 250, 32, 128, "view")]
# several tiles, more than one round of border groups
MID = [(1, 33, 70, 32, 64, "plain"), (2, 17, 60, 64, 64, "head")]


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


def sentinel_y(shape):
    i = torch.arange(int(np.prod(shape)), device=DEV) % 13
    return (-(1.0 + i.float())).to(torch.bfloat16).reshape(shape)


def sentinel_part(shape):
    i = torch.arange(int(np.prod(shape)), device=DEV) % 7
    return ((1.0 + i.float()) * 1e30).reshape(shape)


class Case:
    """One folded upconv: its operands (made once), and run() -> (y buffer, partials or None, kernel, fused)."""

    def __init__(self, case):
        from vmatting import ops
        self.n, self.h, self.w, self.cin, self.cout, self.kind = case
        n, h, w, cin, cout = case[:5]
        rs = np.random.RandomState(h * 131 + w * 7 + cin + cout + n)
        self.x = torch.from_numpy(rs.normal(size=(n, h, w, cin)).astype(np.float32)).to(torch.bfloat16).to(DEV)
        wt = (rs.normal(size=(3, 3, cin, cout)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
        self.pc = ops.PackedConv(wt, (rs.normal(size=cout) * 0.1).astype(np.float32), torch.bfloat16, DEV)
        self.whd = torch.from_numpy((rs.normal(size=(3, 3, 128, 1)) * 0.05).astype(np.float32)).to(DEV)

    def buffers(self):
        n, h, w, cout = self.n, self.h, self.w, self.cout
        ybuf = sentinel_y((n, 2 * h, 2 * w, cout + 48 if self.kind == "view" else cout))
        part = sentinel_part((n, 2 * h, 2 * w, 12)) if self.kind == "head" else None
        return ybuf, part

    def view(self, ybuf):
        return ybuf[..., 16:16 + self.cout] if self.kind == "view" else ybuf

    def call(self, ybuf, part, store_y=True):
        from vmatting import ops
        if self.kind == "head":
            assert ops.upconv3x3_head(self.x, self.pc, self.whd, 64, part, "relu", out=ybuf, store_y=store_y) is not None
        else:
            ops.upconv3x3(self.x, self.pc, "relu", out=self.view(ybuf))

    def run(self, store_y=True):
        from vmatting import _lib
        ybuf, part = self.buffers()
        self.call(ybuf, part, store_y)
        torch.cuda.synchronize()
        return ybuf, part, _lib.last_conv_kernel(), _lib.last_border_fused()

    def check_written(self, ybuf, part, store_y=True):
        """Every output of the view was written (relu: >= 0), nothing outside it; every partial was written."""
        ref, _ = self.buffers()
        if store_y:
            assert bool((self.view(ybuf).float() >= 0).all()), "an output pixel kept its sentinel"
            if self.kind == "view":
                assert torch.equal(ybuf[..., :16], ref[..., :16]) and torch.equal(ybuf[..., 16 + self.cout:],
                                                                                  ref[..., 16 + self.cout:])
        else:
            assert torch.equal(ybuf, ref), "store_y = 0 wrote y"
        if part is not None:
            assert bool((part.abs() < 1e20).all()), "a partial kept its sentinel"


def compare(case, level, want_kernel, **opts):
    c = Case(case)
    stores = (True, False) if c.kind == "head" else (True,)
    for store_y in stores:
        with options(border_fuse=0, **opts):
            y0, p0, k0, f0 = c.run(store_y)
        with options(border_fuse=level, **opts):
            y1, p1, k1, f1 = c.run(store_y)
        assert not f0 and f1, (k0, f0, k1, f1)
        assert k0 == k1 and want_kernel in k1, (k0, k1)
        c.check_written(y0, p0, store_y)
        c.check_written(y1, p1, store_y)
        assert torch.equal(y0, y1), "y differs from the separate border pass"
        if p0 is not None:
            assert torch.equal(p0, p1), "the head partials differ from the separate border pass"


@pytest.mark.parametrize("case", CASES + MID)
def test_streaming_4wave_fused_border_bit_identical(case):
    compare(case, 1, "conv3x3_patch<64, 4, 1, 2, 4, 2,")


@pytest.mark.parametrize("case", [c for c in CASES + BIG if c[5] != "head"])
@pytest.mark.parametrize("cfg", [19, 22])
def test_streaming_8wave_fused_border_bit_identical(case, cfg):
    """(the head split needs patch_cfg 0: its 8-wave case is the BIG grid below)"""
    compare(case, 1, "conv3x3_patch<64, 8, 1, %d, 8, 1," % (3 if cfg == 19 else 2), patch_cfg=cfg)


@pytest.mark.parametrize("case", BIG)
def test_streaming_8wave_fused_border_on_its_own_grid(case):
    compare(case, 1, "conv3x3_patch<64, 8, 1, 3, 8, 1,")


@pytest.mark.parametrize("case", CASES + MID + BIG)
def test_persistent_fused_border_bit_identical(case):
    """border_fuse 2 with persist_up_rounds 0: the persistent kernel on the grids of >= 512 blocks (BIG; a folded
    upconv's per-block constants do not fit beside the 4-wave tiling's LDS, so smaller grids stay on the streaming
    kernel, fused as under 1)."""
    n, h, w, _, cout, _ = case
    tiles8 = n * ((h + 7) // 8) * ((w + 31) // 32)
    if tiles8 * (cout // 64) * 4 >= 512:
        want = "conv3x3_patch_persist<64, 8, 1, 2, 8, 1, true>"
    else:
        want = "conv3x3_patch<64, 4, 1, 2, 4, 2,"
    compare(case, 2, want, persist_up_rounds=0)


def test_level_1_leaves_the_persistent_kernel_its_separate_pass():
    c = Case(BIG[1])
    with options(border_fuse=1, persist_up_rounds=0):
        _, _, k, f = c.run()
    assert "conv3x3_patch_persist" in k and not f, (k, f)


@pytest.mark.parametrize("level,opts", [(1, {}), (2, {"persist_up_rounds": 0})])
def test_fused_border_in_a_captured_graph(level, opts):
    """One fused call captured in a HIP graph and replayed twice, the outputs reset to the sentinel in between."""
    c = Case(BIG[0])
    with options(border_fuse=0, **opts):
        y0, p0, _, _ = c.run()
    with options(border_fuse=level, **opts):
        ybuf, part = c.buffers()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            c.call(ybuf, part)  # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            c.call(ybuf, part)
        from vmatting import _lib
        assert _lib.last_border_fused()
    fresh_y, fresh_p = c.buffers()
    for _ in range(2):
        ybuf.copy_(fresh_y)
        part.copy_(fresh_p)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(ybuf, y0) and torch.equal(part, p0)
