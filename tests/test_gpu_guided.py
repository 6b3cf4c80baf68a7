"""The guided matte upsampling on the GPU against the numpy restatement (tests/guided_ref.py): the reductions and the
apply bit for bit, the coefficients within their two f32 roundings.  Every result is written into the middle of a
sentinel-filled buffer and the inputs are verified unchanged."""

import numpy as np
import pytest
import torch

import guided_ref as gr
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

SCALES = (2, 3, 4)
COEFF_TILE_H, COEFF_TILE_W = 8, 32   # csrc/guided.hip CTH, CTW
APPLY_TILE_H, APPLY_TILE_W = 64, 256  # csrc/guided.hip ATH, ATW (a wave walks 16 rows, a lane owns 4 pixels)


def ragged_shapes(s):
    """One pixel; less than a block by more than a block; one block; a ragged thread at the end of a row of 64 reduced
    pixels; rows of whole threads; one more pixel than that; and an ordinary ragged frame."""
    return [(1, 1), (s - 1, s + 1), (s, s), (2 * s + 1, 64 * s - 1), (5, 64 * s), (7, 64 * s + 1), (37, 70)]


def placed(a, lead):
    """``a`` on the device as a contiguous view that starts ``lead`` elements into a larger buffer."""
    a = np.ascontiguousarray(a)
    buf = torch.zeros(a.size + lead + 8, dtype=torch.from_numpy(a[:0].reshape(-1)).dtype, device="cuda")
    view = buf[lead:lead + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


class Sentinel:
    """An output view of ``shape`` that starts ``lead`` elements into a sentinel-filled buffer."""

    def __init__(self, shape, dtype, fill, lead):
        self.size, self.lead, self.fill = int(np.prod(shape)), lead, fill
        self.buf = torch.full((self.size + lead + 64,), fill, dtype=dtype, device="cuda")
        self.view = self.buf[lead:lead + self.size].view(shape)

    def result(self):
        b = self.buf.cpu().numpy()
        assert (b[:self.lead] == self.fill).all() and (b[self.lead + self.size:] == self.fill).all(), "wrote outside"
        return b[self.lead:self.lead + self.size].reshape(tuple(self.view.shape))


def unchanged(t, a):
    assert t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes(), "an input was written"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def trimaps(rs, n, h, w, s):
    """0 / 128 / 255 in regions a few blocks wide (so whole blocks agree), with single pixels flipped."""
    hm, wm = gr.reduced_size(h, w, 2 * s)
    lab = rs.choice(np.array([0, 128, 255], np.uint8), (n, hm, wm))
    t = np.repeat(np.repeat(lab, 2 * s, 1), 2 * s, 2)[:, :h, :w].copy()
    flip = rs.random((n, h, w)) < 0.03
    t[flip] = rs.choice(np.array([0, 128, 255], np.uint8), int(flip.sum()))
    return t


# ---------------------------------------------------------------- reduce: bit for bit
@pytest.mark.parametrize("kind", ["mean", "trimap"])
@pytest.mark.parametrize("s", SCALES)
def test_reduce_equals_the_restatement(s, kind):
    from vmatting import ops
    rs = np.random.default_rng(100 + s)
    for n in (1, 2):
        for h, w in ragged_shapes(s):
            if kind == "mean":
                src = rs.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
                want = gr.reduce_mean(src, s)
            else:
                src = trimaps(rs, n, h, w, s)
                want = gr.reduce_trimap(src, s)
                if h * w > 1000:
                    assert all((want == v).any() for v in (0, 128, 255))
            # the source 16-byte aligned and at an odd address (every row load is shifted into place); the output
            # 4-byte aligned (dword stores) and at an odd address (byte stores)
            for src_lead, out_lead in ((0, 32), (13, 7)):
                d = placed(src, src_lead)
                out = Sentinel(want.shape, torch.uint8, 201, out_lead)
                res = ops.frames_reduce_u8(d, s, kind, out=out.view)
                assert res.data_ptr() == out.view.data_ptr()
                got = out.result()
                unchanged(d, src)
                assert np.array_equal(got, want), (n, h, w, src_lead, np.argwhere(got != want)[:4])
    if kind == "trimap":  # other values: agreement is what counts
        src = np.repeat(np.repeat(rs.integers(0, 256, (1, 9, 40), dtype=np.uint8), s, 1), s, 2)
        src[0, 2 * s, 3 * s] ^= 1
        got = ops.frames_reduce_u8(placed(src, 3), s, kind).cpu().numpy()
        want = gr.reduce_trimap(src, s)
        assert np.array_equal(got, want) and got[0, 2, 3] == 128 and (got != 128).sum() > 300


# ---------------------------------------------------------------- coeffs: against the f64 restatement
def guides(rs, n, hm, wm):
    two = np.where(rs.random((n, hm, wm, 1)) < 0.5, np.array([[[[20, 30, 40]]]]), np.array([[[[220, 10, 130]]]]))
    return {"constant": np.full((n, hm, wm, 3), 93, np.uint8), "random": rs.integers(0, 256, (n, hm, wm, 3), dtype=np.uint8),
            "two-valued": two.astype(np.uint8)}


@pytest.mark.parametrize("r", [1, 2, 8])
def test_coeffs_within_two_f32_roundings(r):
    """|got - want| <= 4 * 2^-24 * max(1, M), M the largest |a| or |b| of the restatement's unaveraged coefficients in
    the pixel's window: the rounding of (a, b) to f32 and that of their mean, each of which may fall the other way in
    the kernel (its f64 sums run in another order), doubled; the f64 terms are below 1e-9 of it."""
    from vmatting import ops
    rs = np.random.default_rng(200 + r)
    th, tw = COEFF_TILE_H, COEFF_TILE_W
    shapes = [(1, 1, 1), (2, 2, 3), (1, r, 2 * r + 1), (1, th - 1, tw - 1), (1, th, tw), (2, th + 1, tw + 1), (2, 37, 70)]
    worst = 0.0
    for n, hm, wm in shapes:
        p = (rs.random((n, hm, wm)) ** 2).astype(np.float32)
        for gname, g in guides(rs, n, hm, wm).items():
            dg, dp = placed(g, 5), placed(p, 3)
            for eps in (1e-5, 1e-3, 1.0):
                want, raw = gr.coeffs(g, p, r, eps)
                out = Sentinel((n, hm, wm, 4), torch.float32, -7.25, 8)
                work = torch.full((ops.guided_workspace_bytes(n, hm, wm) + 32,), 77, dtype=torch.uint8, device="cuda")
                res = ops.guided_coeffs(dg, dp, r, eps, out=out.view, work=work[:-32])
                assert res.data_ptr() == out.view.data_ptr()
                got = out.result()
                assert (work[-32:] == 77).all()
                M = gr.box_max(np.abs(raw).max(-1).astype(np.float64), r)
                bound = 4 * 2.0 ** -24 * np.maximum(1.0, M)[..., None]
                ratio = float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / bound).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (n, hm, wm, gname, eps, ratio)
            unchanged(dg, g)
            unchanged(dp, p)
    print("r = %d: largest |got - want| / bound = %.3f" % (r, worst))


# ---------------------------------------------------------------- apply: bit for bit
@pytest.mark.parametrize("s", SCALES)
def test_apply_equals_the_restatement(s):
    from vmatting import ops
    rs = np.random.default_rng(300 + s)
    # the ragged shapes; hm = 1 and wm = 1 (the clamped interpolation in one direction only); one row and one column of
    # pixels past a block's tile in both directions
    shapes = ragged_shapes(s) + [(s, 41), (41, s), (APPLY_TILE_H + 1, APPLY_TILE_W + 1)]
    for n in (1, 2):
        for h, w in shapes:
            hm, wm = gr.reduced_size(h, w, s)
            ab = (rs.normal(0.0, 1.5, (n, hm, wm, 4))).astype(np.float32)
            cmp = rs.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
            want = gr.apply(ab, cmp, s)
            if h * w > 1000:
                assert (want == 0).any() and (want == 1).any() and ((want > 0) & (want < 1)).any()
            for cmp_lead, out_lead in ((0, 32), (13, 1)):  # aligned; an odd frame address and a 4-byte aligned output
                dab, dcmp = placed(ab, 4), placed(cmp, cmp_lead)
                out = Sentinel((n, h, w, 1), torch.float32, -3.5, out_lead)
                res = ops.guided_apply(dab, dcmp, s, out=out.view)
                assert res.data_ptr() == out.view.data_ptr()
                got = out.result()[..., 0]
                unchanged(dab, ab)
                unchanged(dcmp, cmp)
                assert np.array_equal(bits(got), bits(want)), (n, h, w, cmp_lead, np.argwhere(got != want)[:4])
    # every byte value in every channel
    cmp = (np.arange(4 * 64 * 3) % 256).astype(np.uint8).reshape(1, 4, 64, 3)
    hm, wm = gr.reduced_size(4, 64, s)
    ab = np.broadcast_to(np.array([0.3, 0.5, 0.2, 0.0], np.float32), (1, hm, wm, 4)).copy()
    got = ops.guided_apply(placed(ab, 0), placed(cmp, 0), s).cpu().numpy()[..., 0]
    assert np.array_equal(bits(got), bits(gr.apply(ab, cmp, s)))


# ---------------------------------------------------------------- the chain
@pytest.mark.parametrize("s", SCALES)
def test_upsample_is_the_three_ops_and_does_its_job(s):
    from vmatting import ops, reader
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    rs = np.random.default_rng(400 + s)
    n, h, w = 2, 37, 70
    hm, wm = gr.reduced_size(h, w, s)
    cmp, p = rs.integers(0, 256, (n, h, w, 3), dtype=np.uint8), rs.random((n, hm, wm)).astype(np.float32)
    dcmp, dp = dev(cmp), dev(p)
    lo = ops.frames_reduce_u8(dcmp, s)
    step = ops.guided_apply(ops.guided_coeffs(lo, dp, 3, 1e-2), dcmp, s)
    assert torch.equal(ops.guided_upsample(dp, dcmp, s, r=3, eps=1e-2), step)
    assert torch.equal(ops.guided_upsample(dp[..., None], dcmp, s, r=3, eps=1e-2, guide_lo=lo), step)
    assert tuple(step.shape) == (n, h, w, 1)
    one = reader.upsample_matte(p[0].astype(np.float64), cmp[0], s, r=3, eps=1e-2)
    assert one.dtype == np.float32 and np.array_equal(bits(one), bits(step[0, :, :, 0].cpu().numpy()))

    def upsample(p_lo, frames, **kw):
        return ops.guided_upsample(dev(p_lo), dev(frames), s, **kw)[..., 0].cpu().numpy()

    # the host test's two conditions, on the kernels
    for hh, ww in ((33, 50), (64, 96)):
        frames, guide_lo, p_lo, want = gr.affine_case(hh, ww, s)
        assert np.array_equal(ops.frames_reduce_u8(dev(frames), s).cpu().numpy(), guide_lo)
        err = np.abs(upsample(p_lo, frames, r=2, eps=1e-5)[0].astype(np.float64) - want).max()
        print("affine %dx%d s=%d: max err %.3e" % (hh, ww, s, err))
        assert err <= 5e-3
    for hh, ww in ((96, 160), (97, 161)):
        ratio = gr.edge_scene_ratio(hh, ww, s, upsample)
        print("edge scene %dx%d s=%d: SAD ratio to bilinear %.3f" % (hh, ww, s, ratio))
        assert ratio <= 0.5
