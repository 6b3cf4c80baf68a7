"""Every kernel that writes a split-fp16 x3 activation (vmatting/split3.py), each on its own at the smallest shapes that
reach its edges: the values it stores and the range flag it raises.

  producers      the patch kernel's f32-staged split epilogue (tilings 0 / 19 / 22 / 25 / 30, packed frames, fused
                 pool), conv3x3_rows<8 | 16, true>'s register epilogue (fused pool), splitk_reduce_kernel, the folded
                 upconv (patch kernel + conv3x3_up2x_border<.., true>) and resize_split3h_kernel (exact-2x, general)
  A  values      every [l, h(, h)] slab bit-equal to the f32 output split afterwards (split3.conv_f32 + split3.split3h,
                 same split-K setting), over shapes whose tiles overhang both frame edges and the channel count, both
                 activations, a concat segment and a whole buffer, with and without the third slab; a NaN-pattern
                 sentinel shows that every output and nothing else is written; the fused pool against the split of
                 the oracle's max_pool_2x2_same of the f32 output; h + l against a float64 conv (2e-6 of max |y|, the
                 bound of test_f16x3_conv_matches_float64)
  B  range flag  exact convs (one filter tap of value 2 on the channel diagonal: filter scale 2^11, Wh = 4096, Wl = 0;
                 integer inputs below 65520 split exactly, so y = 2 x(tap) exactly in f32): one hot input 32760 gives
                 y = 65520 and flag 1, 32759 gives 65518, flag 0 and h = 65504; by position (first pixel, last pixel
                 of an overhanging tile, first / last channel of cout 24, second image), by sign and activation; the
                 input split's own flag (a separate tensor) stays 0; a tile lane past the frame edge that computes
                 65520 raises nothing, never wins the fused pool and stores nothing
"""

import contextlib
import functools

import numpy as np
import pytest
import torch

from conftest import gpu_available
from oracle import ops as oo

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

DEV = "cuda"
SENT = 0x7E01  # an fp16 NaN pattern: no conv or resize of finite inputs stores it
DEFAULTS = {"patch_cfg": 0, "rows_kernel": 1, "pack_frames": 1, "splitk_tiles": 512, "border_ks": 1}

# producer -> (options, split-K, the kernel vm_conv3x3_last_kernel must name, takes a fused pool)
PATCH = {0: "vm::conv3x3_patch<64, ", 19: "vm::conv3x3_patch<64, 8, 1, 3, 8, 1, ",
         22: "vm::conv3x3_patch<64, 8, 1, 2, 8, 1, ", 25: "vm::conv3x3_patch<64, 4, 1, 2, 4, 2, ",
         30: "vm::conv3x3_patch<128, 4, 2, 3, 8, 2, "}
PRODUCERS = {"patch%d" % k: (dict(patch_cfg=k, rows_kernel=0, pack_frames=0), False, v, True) for k, v in PATCH.items()}
PRODUCERS.update({
    "packed": (dict(patch_cfg=0, rows_kernel=0, pack_frames=1), False, PATCH[0], True),
    "rows8": (dict(patch_cfg=0, rows_kernel=8), False, "vm::conv3x3_rows<8, true>", True),
    "rows16": (dict(patch_cfg=0, rows_kernel=16), False, "vm::conv3x3_rows<16, true>", True),
    # the 4 x 32 px split-K tiling, then splitk_reduce_kernel (ysplit > 0); no fused pool on this path
    "splitk": (dict(patch_cfg=0, rows_kernel=0, pack_frames=0), True, PATCH[25], False)})

SHAPES = [(1, 9, 33, 64, 64), (2, 17, 70, 128, 128), (1, 20, 45, 96, 192), (1, 3, 5, 256, 128), (1, 1, 1, 64, 64),
          (1, 33, 66, 64, 24), (3, 16, 32, 160, 64)]
# packed frames: n >= 2 narrow frames whose packing saves >= 10 % of the column tiles (plan_packed_frames: 4 x 10 px
# frames: 4 column tiles -> 2; 2 x 70 px: 6 -> 5); an even width where a pool is fused
PACKED_SHAPES = [(4, 9, 10, 64, 64), (2, 17, 70, 128, 128), (5, 3, 6, 64, 24)]
F64_SHAPE = {"packed": (4, 9, 10, 64, 64)}  # (the others: (1, 20, 45, 96, 192))


@contextlib.contextmanager
def options(**kw):
    from vmatting import _lib
    try:
        for k, v in kw.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k in kw:
            _lib.set_option(k, DEFAULTS[k])


def bits(t):
    return t.contiguous().view(torch.int16)


def split_buffer(n, h, w, cout, seg, third):
    """A sentinel-filled split buffer and the producer's view of it: ``seg``: channels [cout, 2 cout) of a 2-cout-wide
    concat (S = 2 cout), else the whole buffer (S = cout); ``third``: the pixel row holds 3 S channels (the slab width
    is then passed explicitly), else 2 S.  -> (buf, view, S, off, slabs written, the slab argument)"""
    S, off = (2 * cout, cout) if seg else (cout, 0)
    nsl = 3 if third else 2
    buf = torch.empty((n, h, w, nsl * S), dtype=torch.float16, device=DEV)
    buf.view(torch.int16).fill_(SENT)
    return buf, buf[..., off:off + cout], S, off, nsl, (S if third else 0)


def check_slabs(got, ref, S, off, cout, nsl, what):
    """``got`` (the producer's buffer) against ``ref`` (same layout, the split of the f32 output): written slabs
    bit-equal and free of the sentinel, everything else still the sentinel."""
    g, r = bits(got.cpu()), bits(ref.cpu())
    written = torch.zeros(g.shape[-1], dtype=torch.bool)
    for p in range(nsl):
        sl = slice(p * S + off, p * S + off + cout)
        written[sl] = True
        assert torch.equal(g[..., sl], r[..., sl]), "%s: slab %d differs from the split of the f32 output" % (what, p)
        assert not (g[..., sl] == SENT).any(), "%s: slab %d has unwritten outputs" % (what, p)
    assert (g[..., ~written] == SENT).all(), "%s: stores outside the view's slabs" % what


@functools.lru_cache(maxsize=None)
def conv_case(shape):
    """The inputs of test_f16x3_conv_matches_float64 (randn * 300, He-scaled filter, a bias) for one shape: the f32
    arrays, the split input [l, h] on the device and the packed split filter."""
    from vmatting import ops
    from vmatting.split3 import filter_scale, split3_filter, split3h
    n, h, w, cin, cout = shape
    rs = np.random.RandomState(cin + cout + h)
    x = (rs.randn(n, h, w, cin) * 300).astype(np.float32)
    wt = (rs.randn(3, 3, cin, cout) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    b = rs.randn(cout).astype(np.float32)
    t = filter_scale(wt)
    pc = ops.PackedConv(split3_filter(wt, cin, cout, t), None, "f16", DEV, scale=np.full(cout, 1.0 / t, np.float32),
                        shift=b)
    xs = torch.zeros((n, h, w, 2 * cin), dtype=torch.float16, device=DEV)  # [l, h], read as [l, h, h]
    split3h(torch.from_numpy(x).to(DEV), xs[..., :cin])
    return x, wt, b, xs, pc


@functools.lru_cache(maxsize=None)
def conv_f64(shape):
    x, wt, b, _, _ = conv_case(shape)
    return oo.conv3x3_same(x.astype(np.float64), wt.astype(np.float64), b.astype(np.float64))


def f32_output(xs, pc, n, h, w, cout, act, splitk):
    from vmatting import split3
    y = torch.empty((n, h, w, cout), dtype=torch.float32, device=DEV)
    return split3.conv_f32(xs, pc, y, act, splitk=splitk)


def split_of(f32, n, h, w, cout, seg, third):
    """split3.split3h of an f32 tensor into a zero buffer of split_buffer's layout."""
    from vmatting import split3
    S, off = (2 * cout, cout) if seg else (cout, 0)
    ref = torch.zeros((n, h, w, (3 if third else 2) * S), dtype=torch.float16, device=DEV)
    split3.split3h(f32, ref[..., off:off + cout], slab=S)
    return ref


def splitk_planned(xs, pc):
    from vmatting import ops
    xv = ops.nhwc(xs)
    return ops.lib().vm_conv3x3_workspace_bytes(ops.ctypes.byref(xv), pc.cin, pc.cout) > 0


# (activation, concat segment, third slab): both activations, both layouts, both slab counts, each pair once
LAYOUTS = [("relu", True, True), ("none", False, False), ("none", True, False), ("relu", False, True)]


def _producer_shapes():
    out = []
    for prod in PRODUCERS:
        for shape in (PACKED_SHAPES if prod == "packed" else SHAPES):
            out.append(pytest.param(prod, shape, id="%s-%s" % (prod, "x".join(map(str, shape)))))
    return out


# ------------------------------------------------------------------------------------------------ A: values

@pytest.mark.parametrize("prod,shape", _producer_shapes())
def test_conv_split_epilogue_equals_split_of_f32_output(prod, shape):
    from vmatting import _lib, split3
    opts, splitk, kernel, _ = PRODUCERS[prod]
    n, h, w, cin, cout = shape
    _, _, _, xs, pc = conv_case(shape)
    with options(**opts):
        if splitk:
            assert splitk_planned(xs, pc), "no split-K plan at %s" % (shape,)
        for act, seg, third in LAYOUTS:
            what = "%s %s act=%s seg=%s third=%s" % (prod, shape, act, seg, third)
            buf, view, S, off, nsl, slab = split_buffer(n, h, w, cout, seg, third)
            split3.conv_split(xs, pc, view, act, y_slab=slab, splitk=splitk)
            assert _lib.last_conv_kernel().startswith(kernel), (what, _lib.last_conv_kernel())
            # (the f32 output comes from the patch kernel on the same tiling and split-K plan: the same sums)
            yf = f32_output(xs, pc, n, h, w, cout, act, splitk)
            torch.cuda.synchronize()
            check_slabs(buf, split_of(yf, n, h, w, cout, seg, third), S, off, cout, nsl, what)


def _pool_cases():
    out = []
    for prod, (_, _, _, pool) in PRODUCERS.items():
        if pool:
            for shape in ([s for s in PACKED_SHAPES if s[2] % 2 == 0] if prod == "packed" else SHAPES):
                out.append(pytest.param(prod, shape, id="%s-%s" % (prod, "x".join(map(str, shape)))))
    return out


@pytest.mark.parametrize("prod,shape", _pool_cases())
def test_conv_split_fused_pool_equals_split_of_pooled_f32_output(prod, shape):
    """The fused 2x2 SAME pool (odd sizes: the last window holds one row / column): its slabs equal the split of the
    oracle's max_pool_2x2_same of the f32 output; the full-resolution slabs are checked again beside it."""
    from vmatting import _lib, split3
    opts, _, kernel, _ = PRODUCERS[prod]
    n, h, w, cin, cout = shape
    ph, pw = (h + 1) // 2, (w + 1) // 2
    _, _, _, xs, pc = conv_case(shape)
    with options(**opts):
        for act, seg, third in LAYOUTS[:2]:
            what = "%s %s pool act=%s seg=%s third=%s" % (prod, shape, act, seg, third)
            buf, view, S, off, nsl, slab = split_buffer(n, h, w, cout, seg, third)
            pbuf, pview, _, _, _, pslab = split_buffer(n, ph, pw, cout, seg, third)
            split3.conv_split(xs, pc, view, act, pool=pview, y_slab=slab, pool_slab=pslab)
            assert _lib.last_conv_kernel().startswith(kernel), (what, _lib.last_conv_kernel())
            yf = f32_output(xs, pc, n, h, w, cout, act, False)  # (no split-K under a pool)
            torch.cuda.synchronize()
            check_slabs(buf, split_of(yf, n, h, w, cout, seg, third), S, off, cout, nsl, what)
            pooled = torch.from_numpy(oo.max_pool_2x2_same(yf.cpu().numpy())).to(DEV)
            check_slabs(pbuf, split_of(pooled, n, ph, pw, cout, seg, third), S, off, cout, nsl, what + " (pool)")


@pytest.mark.parametrize("prod", list(PRODUCERS))
def test_conv_split_epilogue_matches_float64(prod):
    """h + l of the stored split against the float64 conv of the f32 operands: within 2e-6 of max |y|."""
    from vmatting import _lib, split3
    opts, splitk, kernel, _ = PRODUCERS[prod]
    shape = F64_SHAPE.get(prod, (1, 20, 45, 96, 192))
    n, h, w, cin, cout = shape
    _, _, _, xs, pc = conv_case(shape)
    ref = conv_f64(shape)
    buf, view, S, off, nsl, slab = split_buffer(n, h, w, cout, False, False)
    with options(**opts):
        assert not splitk or splitk_planned(xs, pc)
        split3.conv_split(xs, pc, view, "none", splitk=splitk)
        assert _lib.last_conv_kernel().startswith(kernel), _lib.last_conv_kernel()
    torch.cuda.synchronize()
    got = buf.cpu().double().numpy()
    got = got[..., :cout] + got[..., S:S + cout]
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("f16x3 split epilogue %s %s: max err %.3e of max |y|" % (prod, shape, err))
    assert err <= 2e-6


RESIZES = [((5, 6), (9, 12)), ((3, 4), (3, 4)), ((7, 9), (14, 18)), ((1, 1), (2, 2)), ((68, 120), (135, 240))]


@pytest.mark.parametrize("src,dst", RESIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("c", [8, 64])
def test_resize_split3h_equals_resize_then_split(src, dst, c):
    """vm_resize_split3h_nhwc (the exact-2x quad form at 7x9 -> 14x18 and 1x1 -> 2x2, the general one elsewhere) from
    an f32 channel-slice view into a concat segment and a whole buffer: bit-equal to ops.resize_bilinear + split3h."""
    from vmatting import ops, split3
    n = 2
    torch.manual_seed(c + src[0])
    x = (torch.randn(n, src[0], src[1], c + 8) * torch.logspace(-6, 4, c + 8)).float().to(DEV)
    xv = x[..., 4:4 + c]  # (16-byte aligned: channel offset 4)
    rr = ops.resize_bilinear(xv.contiguous(), dst)
    for seg, third in ((True, True), (False, False)):
        buf, view, S, off, nsl, slab = split_buffer(n, dst[0], dst[1], c, seg, third)
        ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
        split3.resize_split3h(xv, view, slab=slab, overflow=ovf)
        torch.cuda.synchronize()
        assert int(ovf.item()) == 0
        check_slabs(buf, split_of(rr, n, dst[0], dst[1], c, seg, third), S, off, c, nsl,
                    "resize %s -> %s c=%d seg=%s" % (src, dst, c, seg))


def up_case(shape, w):
    """The packed filters of one folded 2x upconv as Split3Forward packs them (one scale for the folded filter and
    the plain one of the border pass, no bias) -> (pc_up, pc, t)."""
    from vmatting import ops
    from vmatting.split3 import filter_scale, fold_up2x, split3_filter
    _, _, _, cin, cout = shape
    wu = fold_up2x(w)
    t = min(filter_scale(w), filter_scale(wu))
    aff = dict(scale=np.full(cout, 1.0 / t, np.float32), shift=np.zeros(cout, np.float32))
    pc_up = ops.PackedConv(split3_filter(wu, cin, 4 * cout, t), None, "f16", DEV, **aff)
    pc = ops.PackedConv(split3_filter(w, cin, cout, t), None, "f16", DEV, **aff)
    return pc_up, pc, t


@pytest.mark.parametrize("shape", [(1, 9, 13, 128, 64), (2, 7, 33, 256, 128), (1, 1, 1, 64, 64)],
                         ids=lambda s: "x".join(map(str, s)))
def test_up_split_writes_its_view_only_and_border_ks_is_bit_identical(shape):
    """vm_conv3x3_up2x_split3_nhwc (interior phases on the patch kernel + the split border pass) into a concat
    segment with the third slab: every output and nothing else is written, and border_ks 1 / 2 / 4 give the same
    bits (the arithmetic is test_f16x3_folded_upconvs_match_the_resize_path's; today the split border pass always
    launches its 4-group form, so the option must simply be harmless here)."""
    from vmatting import _lib, split3
    n, h, w, cin, cout = shape
    rs = np.random.RandomState(cin + h)
    x = (rs.randn(n, h, w, cin) * 300).astype(np.float32)
    wt = (rs.randn(3, 3, cin, cout) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    pc_up, pc, _ = up_case(shape, wt)
    xs = torch.zeros((n, h, w, 2 * cin), dtype=torch.float16, device=DEV)
    split3.split3h(torch.from_numpy(x).to(DEV), xs[..., :cin])
    outs = []
    for ks in (1, 2, 4):
        with options(border_ks=ks):
            buf, view, S, off, nsl, slab = split_buffer(n, 2 * h, 2 * w, cout, True, True)
            ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
            split3.up_split(xs, pc_up, pc, view, ovf, y_slab=slab)
            assert _lib.last_conv_kernel().startswith("vm::conv3x3_patch<"), _lib.last_conv_kernel()
            torch.cuda.synchronize()
            assert int(ovf.item()) == 0
            outs.append(buf.cpu())
    check_slabs(outs[0], outs[1], S, off, cout, nsl, "up_split %s border_ks 1 vs 2" % (shape,))
    check_slabs(outs[0], outs[2], S, off, cout, nsl, "up_split %s border_ks 1 vs 4" % (shape,))
    lo, hi = outs[0][..., off:off + cout], outs[0][..., S + off:S + off + cout]
    assert torch.isfinite(lo).all() and torch.isfinite(hi).all()
    assert torch.equal(bits(hi), bits(outs[0][..., 2 * S + off:2 * S + off + cout]))  # the third slab: h again


# ------------------------------------------------------------------------------------------------ B: range flag

CENTRE, UP, LEFT = (1, 1), (0, 1), (1, 0)  # filter taps (kh, kw): y(r, c) = 2 x(r + kh - 1, c + kw - 1)


def tap_filter(cin, cout, taps):
    """[3,3,cin,cout] filter with ``taps`` {(kh, kw): value} on the channel diagonal."""
    w = np.zeros((3, 3, cin, cout), np.float32)
    for (kh, kw), g in taps.items():
        for c in range(min(cin, cout)):
            w[kh, kw, c, c] = g
    return w


def test_exact_threshold_arithmetic_on_the_host():
    """The premises of the flag tests, from filter_scale / split3_filter / split2h alone: the one-tap filter of value
    2 scales by 2^11 into Wh = 4096, Wl = 0; integers below 65520 split exactly into h (fp16) + l (an integer, |l| <=
    16); so (l Wh + h Wl + h Wh) 2^-11 = 2 x in f32 whatever the order of the sums; 32760 -> 65520, 32759 -> 65518
    (h = 65504, finite)."""
    from vmatting.split3 import filter_scale, split2h, split3_filter
    w = tap_filter(32, 24, {CENTRE: 2.0})
    t = filter_scale(w)
    assert t == 2.0 ** 11
    wf = split3_filter(w, 32, 24, t)  # slabs [Wh, Wl, Wh]
    assert float(wf[1, 1, 0, 0]) == 4096.0 and float(wf[1, 1, 64, 0]) == 4096.0 and not wf[:, :, 32:64].any()
    assert float(wf.abs().sum()) == 2 * 24 * 4096.0
    x = torch.arange(-65519, 65520, dtype=torch.float32)
    h, lo = split2h(x)
    assert torch.equal(h + lo, x) and float(lo.abs().max()) <= 16 and torch.equal(lo, lo.round())
    # the products l Wh and h Wh and their sum 4096 x: multiples of 2^12 below 2^29, so exact f32 in any order
    acc = lo * 4096 + h * 4096
    assert torch.equal(acc.double(), 4096 * x.double()) and torch.equal(acc / 2048, 2 * x)
    h1, l1 = split2h(torch.tensor([32760.0, 32759.0]))
    assert h1.tolist() == [32768.0, 32752.0] and l1.tolist() == [-8.0, 7.0]
    assert (l1 * 4096 + h1 * 4096).tolist() == [32760 * 4096.0, 32759 * 4096.0]
    h2, l2 = split2h(torch.tensor([65520.0, 65518.0]))
    assert h2.tolist() == [float("inf"), 65504.0] and float(l2[1]) == 14.0


def exact_conv(n, h, w, cin, cout, taps, hot, prod, act="none", pool=False, seg=False):
    """One exact conv on producer ``prod``: integer background in +-100, the ``hot`` elements {(n, r, c, ch): value}
    placed, the input split with a flag of its own.  -> (the producer's flag, the input split's flag, the expected f32
    output, buf / its layout, pool buf or None, the f32 output of conv_f32)."""
    from vmatting import _lib, ops, split3
    from vmatting.split3 import filter_scale, split3_filter
    opts, splitk, kernel, _ = PRODUCERS[prod]
    rs = np.random.RandomState(n * 1000 + h * 10 + w)
    x = rs.randint(-100, 101, (n, h, w, cin)).astype(np.float32)
    for k, v in hot.items():
        x[k] = v
    wt = tap_filter(cin, cout, taps)
    t = filter_scale(wt)
    pc = ops.PackedConv(split3_filter(wt, cin, cout, t), None, "f16", DEV, scale=np.full(cout, 1.0 / t, np.float32),
                        shift=np.zeros(cout, np.float32))
    xs = torch.zeros((n, h, w, 2 * cin), dtype=torch.float16, device=DEV)
    in_flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    split3.split3h(torch.from_numpy(x).to(DEV), xs[..., :cin], overflow=in_flag)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    buf, view, S, off, nsl, slab = split_buffer(n, h, w, cout, seg, seg)
    pbuf = pview = None
    if pool:
        pbuf, pview, _, _, _, pslab = split_buffer(n, (h + 1) // 2, (w + 1) // 2, cout, seg, seg)
    with options(**opts):
        if splitk:
            assert splitk_planned(xs, pc)
        split3.conv_split(xs, pc, view, act, pool=pview, overflow=flag, y_slab=slab, pool_slab=slab if pool else 0,
                          splitk=splitk)
        assert _lib.last_conv_kernel().startswith(kernel), _lib.last_conv_kernel()
        yf = f32_output(xs, pc, n, h, w, cout, act, splitk and not pool)
    torch.cuda.synchronize()
    want = np.zeros((n, h, w, cout), np.float64)  # y = sum over taps of g x(r + kh - 1, c + kw - 1), zero padding
    xp = np.pad(x.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    cc = min(cin, cout)
    for (kh, kw), g in taps.items():
        want[..., :cc] += g * xp[:, kh:kh + h, kw:kw + w, :cc]
    if act == "relu":
        want = np.maximum(want, 0.0)
    return dict(flag=int(flag.item()), in_flag=int(in_flag.item()), want=want, buf=buf, layout=(S, off, nsl), pbuf=pbuf,
                yf=yf, seg=seg)


def stored(r, cout):
    """(l, h) of the producer's stored output as float64 numpy (the view's channels)."""
    S, off, _ = r["layout"]
    g = r["buf"].cpu().double().numpy()
    return g[..., off:off + cout], g[..., S + off:S + off + cout]


# (n, h, w, cin, cout, the hot element (n, r, c, ch)): 9 rows overhang the 8- and 16-row tiles (and the 4-row ones),
# 33 columns the 32-px tiles; cout 24 leaves 40 of a 64-channel tile's lanes past the channel count
POSITIONS = {"first-pixel-ch0": (1, 9, 33, 64, 64, (0, 0, 0, 0)),
             "last-pixel-overhang": (1, 9, 33, 64, 64, (0, 8, 32, 63)),
             "cout24-ch0": (1, 9, 33, 64, 24, (0, 4, 20, 0)),
             "cout24-last-ch": (1, 9, 33, 64, 24, (0, 8, 32, 23)),
             "second-image": (2, 9, 33, 64, 64, (1, 3, 7, 5))}
PACKED_POSITIONS = {"first-pixel-ch0": (4, 9, 10, 64, 64, (0, 0, 0, 0)),
                    "last-pixel-overhang": (4, 9, 10, 64, 64, (3, 8, 9, 63)),
                    "cout24-ch0": (4, 9, 10, 64, 24, (1, 4, 2, 0)),
                    "cout24-last-ch": (4, 9, 10, 64, 24, (2, 8, 9, 23)),
                    "second-image": (4, 9, 10, 64, 64, (1, 3, 7, 5))}
# two patch tilings + packed frames, the rows kernel at both heights without and with its pool, the split-K reduction
FLAG_PRODUCERS = [("patch22", False), ("patch25", False), ("patch25", True), ("packed", False), ("packed", True),
                  ("rows8", False), ("rows8", True), ("rows16", False), ("rows16", True), ("splitk", False)]
FLAG_IDS = ["%s%s" % (p, "-pool" if q else "") for p, q in FLAG_PRODUCERS]


@pytest.mark.parametrize("where", list(POSITIONS))
@pytest.mark.parametrize("prod,pool", FLAG_PRODUCERS, ids=FLAG_IDS)
def test_conv_split_flag_exactly_at_the_threshold(prod, pool, where):
    n, h, w, cin, cout, at = (PACKED_POSITIONS if prod == "packed" else POSITIONS)[where]
    r = exact_conv(n, h, w, cin, cout, {CENTRE: 2.0}, {at: 32760.0}, prod, pool=pool)
    assert r["in_flag"] == 0
    assert r["flag"] == 1, "y = 65520 at %s raised no flag" % (at,)
    r = exact_conv(n, h, w, cin, cout, {CENTRE: 2.0}, {at: 32759.0}, prod, pool=pool)
    assert r["in_flag"] == 0
    assert r["flag"] == 0, "y = 65518 at %s raised the flag" % (at,)
    lo, hi = stored(r, cout)
    assert np.isfinite(lo).all() and np.isfinite(hi).all()
    assert hi[at] == 65504.0 and lo[at] == 14.0
    assert np.array_equal(lo + hi, r["want"])  # y = 2 x exactly, everywhere
    assert np.array_equal(r["yf"].cpu().double().numpy(), r["want"])


@pytest.mark.parametrize("prod,pool", FLAG_PRODUCERS, ids=FLAG_IDS)
def test_conv_split_flag_sign_and_activation(prod, pool):
    n, h, w, cin, cout, at = (PACKED_POSITIONS if prod == "packed" else POSITIONS)["second-image"]
    r = exact_conv(n, h, w, cin, cout, {CENTRE: 2.0}, {at: -32760.0}, prod, act="none", pool=pool)
    assert (r["in_flag"], r["flag"]) == (0, 1)  # y = -65520
    r = exact_conv(n, h, w, cin, cout, {CENTRE: 2.0}, {at: -32760.0}, prod, act="relu", pool=pool)
    assert (r["in_flag"], r["flag"]) == (0, 0)  # clipped to 0 before the split
    lo, hi = stored(r, cout)
    assert hi[at] == 0.0 and lo[at] == 0.0 and np.array_equal(lo + hi, r["want"])


@pytest.mark.parametrize("edge", ["row", "column"])
@pytest.mark.parametrize("prod,pool", FLAG_PRODUCERS, ids=FLAG_IDS)
def test_conv_split_lanes_past_the_frame_raise_no_flag(prod, pool, edge):
    """A false flag moves a model onto the 2x slower path for good (UNet.build).  The 'look up' filter (tap kh 0, kw 1:
    y(r, c) = 2 x(r - 1, c)) with the hot input in the frame's last row: every in-frame output is small and the
    tile's overhang row r = H computes 65520; likewise the 'look left' filter and the last column.  No flag, the
    overhang value never wins the fused pool, nothing is stored outside the view."""
    n, h, w, cin, cout = (4, 9, 10, 64, 64) if prod == "packed" else (2, 9, 33, 64, 64)
    taps, at = ({UP: 2.0}, (1, h - 1, 3, 5)) if edge == "row" else ({LEFT: 2.0}, (1, 2, w - 1, 5))
    r = exact_conv(n, h, w, cin, cout, taps, {at: 32760.0}, prod, pool=pool, seg=True)
    assert r["in_flag"] == 0
    assert r["flag"] == 0, "an output past the frame's last %s raised the flag" % edge
    S, off, nsl = r["layout"]
    assert np.abs(r["want"]).max() <= 200.0
    assert np.array_equal(r["yf"].cpu().double().numpy(), r["want"])
    check_slabs(r["buf"], split_of(r["yf"], n, h, w, cout, True, True), S, off, cout, nsl,
                "%s overhang %s" % (prod, edge))
    if pool:
        pooled = torch.from_numpy(oo.max_pool_2x2_same(r["yf"].cpu().numpy())).to(DEV)
        check_slabs(r["pbuf"], split_of(pooled, n, (h + 1) // 2, (w + 1) // 2, cout, True, True), S, off, cout, nsl,
                    "%s overhang %s (pool)" % (prod, edge))
    # the same frame does raise it once the hot output is inside: the tap moved onto the hot pixel
    r = exact_conv(n, h, w, cin, cout, {CENTRE: 2.0}, {at: 32760.0}, prod, pool=pool, seg=True)
    assert (r["in_flag"], r["flag"]) == (0, 1)


def exact_up(h, w, c, taps, hot, border_ks):
    """One exact folded upconv of a [1, h, w, c] integer frame -> (flag, input flag, (l, h) of the stored output)."""
    from vmatting import split3
    rs = np.random.RandomState(h * 10 + w)
    x = rs.randint(-100, 101, (1, h, w, c)).astype(np.float32)
    for k, v in hot.items():
        x[k] = v
    pc_up, pc, t = up_case((1, h, w, c, c), tap_filter(c, c, taps))
    assert t == 2.0 ** 11
    xs = torch.zeros((1, h, w, 2 * c), dtype=torch.float16, device=DEV)
    in_flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    split3.split3h(torch.from_numpy(x).to(DEV), xs[..., :c], overflow=in_flag)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    buf, view, S, off, nsl, slab = split_buffer(1, 2 * h, 2 * w, c, False, False)
    with options(border_ks=border_ks):
        split3.up_split(xs, pc_up, pc, view, flag)
    torch.cuda.synchronize()
    g = buf.cpu().double().numpy()
    return int(flag.item()), int(in_flag.item()), g[..., :c], g[..., S:S + c]


@pytest.mark.parametrize("border_ks", [1, 4])
def test_up_split_flag_from_the_interior_and_from_the_border_pass(border_ks):
    """The TF-1 2x resize copies low-res pixel (i, j) to output (2i, 2j), so with the centre tap of value 2 a hot
    low-res pixel (2, 3) of a 5 x 7 frame puts 65520 at the interior output (4, 6) only: the patch kernel's flag.
    With the taps {centre: 2, up: -2}, y(r, c) = 2 (u(r, c) - u(r - 1, c)) of the resized u: a hot low-res pixel (0, 3)
    gives 65520 at output (0, 6) — its row above is the zero padding — and 2 (u(r) - u(r - 1)) = x(1, 3) - 32760 on
    rows 1 and 2: only a frame-border pixel, which the border pass writes, is out of range."""
    h, w, c = 5, 7, 64
    for taps, at, out in (({CENTRE: 2.0}, (0, 2, 3, 9), (0, 4, 6, 9)),
                          ({CENTRE: 2.0, UP: -2.0}, (0, 0, 3, 9), (0, 0, 6, 9))):
        flag, in_flag, lo, hi = exact_up(h, w, c, taps, {at: 32760.0}, border_ks)
        assert (in_flag, flag) == (0, 1), (taps, flag)
        assert hi[out] == float("inf")
        flag, in_flag, lo, hi = exact_up(h, w, c, taps, {at: 32759.0}, border_ks)
        assert (in_flag, flag) == (0, 0), (taps, flag)
        assert np.isfinite(lo).all() and np.isfinite(hi).all()
        assert hi[out] == 65504.0 and lo[out] == 14.0
        assert np.abs(lo + hi).max() == 65518.0


@pytest.mark.parametrize("src,dst", [((7, 9), (14, 18)), ((5, 6), (9, 12))], ids=["exact2x", "general"])
@pytest.mark.parametrize("last", [False, True], ids=["first-pixel", "last-pixel"])
def test_resize_split3h_flag(src, dst, last):
    """The resize copies its first and last input pixels to the first and last output pixels (interpolation weight
    0), so a hot f32 input 65520 there must raise the flag, 65519 (every output <= 65519) must not; a NaN input does,
    as the kernel's comment promises."""
    from vmatting import split3
    c = 16
    at = (1, src[0] - 1, src[1] - 1, c - 1) if last else (0, 0, 0, 0)
    out = (1, dst[0] - 1, dst[1] - 1, c - 1) if last else (0, 0, 0, 0)
    x = torch.from_numpy(np.random.RandomState(5).randint(-100, 101, (2,) + src + (c,)).astype(np.float32)).to(DEV)
    for hot, want in ((65520.0, 1), (65519.0, 0), (float("nan"), 1)):
        x[at] = hot
        buf, view, S, off, nsl, slab = split_buffer(2, dst[0], dst[1], c, False, False)
        ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
        split3.resize_split3h(x, view, overflow=ovf)
        torch.cuda.synchronize()
        assert int(ovf.item()) == want, hot
        hi = buf[..., S:S + c].cpu()
        if want == 0:
            assert torch.isfinite(buf.cpu()).all() and float(hi[out]) == 65504.0
        elif hot == 65520.0:
            assert float(hi[out]) == float("inf")
