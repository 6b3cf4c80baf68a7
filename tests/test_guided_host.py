"""CPU checks of the guided matte upsampling: the numpy restatement (tests/guided_ref.py) does what the method is for,
and every argument check of the C calls, ops, reader.upsample_matte and FrameStream(scale=...) happens on the host."""

import numpy as np
import pytest
import torch

import guided_ref as gr

SCALES = (2, 3, 4)


# ---------------------------------------------------------------- exact cases of the restatement
@pytest.mark.parametrize("s", SCALES)
def test_constant_guide_and_matte_give_back_the_constant(s):
    cmp = np.full((1, 11, 14, 3), 77, np.uint8)
    hm, wm = gr.reduced_size(11, 14, s)
    p = np.full((1, hm, wm), 0.375, np.float32)
    guide_lo = gr.reduce_mean(cmp, s)
    assert (guide_lo == 77).all()
    ab, raw = gr.coeffs(guide_lo, p, 2, 1e-3)
    assert (raw[..., :3] == 0).all() and (raw[..., 3] == np.float32(0.375)).all()
    assert np.array_equal(ab, raw)
    assert (gr.apply(ab, cmp, s) == np.float32(0.375)).all()


def test_one_reduced_pixel_works():
    rs = np.random.default_rng(0)
    cmp = rs.integers(0, 256, (2, 3, 4, 3), dtype=np.uint8)
    guide_lo = gr.reduce_mean(cmp, 4)
    assert guide_lo.shape == (2, 1, 1, 3)
    p = np.array([0.25, 0.75], np.float32).reshape(2, 1, 1)
    ab, _ = gr.coeffs(guide_lo, p, 8, 1e-5)
    assert (ab[..., :3] == 0).all() and np.array_equal(ab[..., 3], p)  # one pixel: no covariance, b = p
    out = gr.apply(ab, cmp, 4)
    assert out.shape == (2, 3, 4) and (out[0] == 0.25).all() and (out[1] == 0.75).all()


@pytest.mark.parametrize("s", SCALES)
def test_reductions_are_the_integer_definitions(s):
    rs = np.random.default_rng(1)
    h, w = 2 * s + 1, 3 * s + 2
    cmp = rs.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    tri = rs.choice(np.array([0, 128, 255], np.uint8), (2, h, w), p=(0.45, 0.1, 0.45))
    tri[:, :s, :2 * s] = 255
    tri[:, s:2 * s, :s] = 0
    mean, lab = gr.reduce_mean(cmp, s), gr.reduce_trimap(tri, s)
    hm, wm = gr.reduced_size(h, w, s)
    assert mean.shape == (2, hm, wm, 3) and lab.shape == (2, hm, wm)
    for Y in range(hm):
        for X in range(wm):
            blk = cmp[:, s * Y:s * Y + s, s * X:s * X + s].astype(np.int64)
            cnt = blk.shape[1] * blk.shape[2]
            assert np.array_equal(mean[:, Y, X], (2 * blk.sum((1, 2)) + cnt) // (2 * cnt))
            assert np.array_equal(mean[:, Y, X], np.floor(blk.mean((1, 2)) + 0.5))  # the mean, halves rounded up
            for f in range(2):
                t = tri[f, s * Y:s * Y + s, s * X:s * X + s]
                mixed = t.min() != t.max()
                # a mixed block never becomes a hard label; an agreeing one keeps its own
                assert lab[f, Y, X] == (128 if mixed else t.flat[0])
    assert lab[0, 0, 0] == 255 and lab[0, 1, 0] == 0
    odd = rs.integers(0, 256, (1, h, w), dtype=np.uint8)  # other values: agreement, not membership of {0, 128, 255}
    odd[0, :s, :s] = 77
    assert gr.reduce_trimap(odd, s)[0, 0, 0] == 77


# ---------------------------------------------------------------- affine recovery
@pytest.mark.parametrize("h,w", [(33, 50), (64, 96)])
@pytest.mark.parametrize("s", SCALES)
def test_affine_matte_is_recovered(h, w, s):
    """A matte that is affine in the guide is what the filter's model is exact for: the full-resolution result follows
    the full-resolution guide, which bilinear upsampling cannot (it is off by about 0.3 here)."""
    cmp, guide_lo, p_lo, want = gr.affine_case(h, w, s)
    got = gr.upsample(p_lo, cmp, s, r=2, eps=1e-5, guide_lo=guide_lo)[0]
    err = np.abs(got.astype(np.float64) - want).max()
    bil = np.abs(gr.bilinear(p_lo[..., None], h, w, s)[0, ..., 0].astype(np.float64) - want).max()
    print("affine %dx%d s=%d: guided max err %.3e, bilinear %.3f" % (h, w, s, err, bil))
    assert err <= 5e-3
    assert bil > 0.2


# ---------------------------------------------------------------- the edge scene
@pytest.mark.parametrize("h,w", [(96, 160), (97, 161)])
@pytest.mark.parametrize("s", SCALES)
def test_edge_scene_beats_bilinear(h, w, s):
    ratio = gr.edge_scene_ratio(h, w, s, lambda p, c: gr.upsample(p, c, s))
    print("edge scene %dx%d s=%d: SAD ratio to bilinear %.3f" % (h, w, s, ratio))
    assert ratio <= 0.5


# ---------------------------------------------------------------- argument checks, no device
def test_c_calls_reject_bad_arguments():
    from vmatting import _lib
    lib = _lib.lib()
    P, Q, W = 4096, 1 << 20, 1 << 21  # non-null, aligned, far apart: validation never dereferences them
    for args in [(None, 1, 4, 4, 3, 2, 0, Q), (P, 1, 4, 4, 3, 2, 0, None), (P, 0, 4, 4, 3, 2, 0, Q),
                 (P, 1, 0, 4, 3, 2, 0, Q), (P, 1, 4, 0, 3, 2, 0, Q), (P, 1, 4, 4, 3, 1, 0, Q), (P, 1, 4, 4, 3, 5, 0, Q),
                 (P, 1, 4, 4, 3, 2, 2, Q), (P, 1, 4, 4, 1, 2, 0, Q), (P, 1, 4, 4, 3, 2, 1, Q), (P, 1, 4, 4, 3, 2, 0, P + 8),
                 (P, 1 << 15, 1 << 10, 1 << 10, 3, 2, 0, Q)]:
        assert lib.vm_frames_reduce_u8(*args, None) == _lib.VM_EINVAL, args
        assert b"frames_reduce_u8" in lib.vm_last_error()
    ok = (P, Q, 1, 4, 4, 2, 1e-3, W, W + (1 << 16))
    for i, v in [(0, None), (1, None), (7, None), (8, None), (2, 0), (3, 0), (4, 0), (5, 0), (5, 9), (6, 0.0),
                 (6, 9e-6), (6, 1.5), (6, float("nan")), (1, Q + 2), (7, W + 4), (8, W + (1 << 16) + 8), (8, W + 16),
                 (7, Q)]:
        args = ok[:i] + (v,) + ok[i + 1:]
        assert lib.vm_guided_coeffs(*args, None) == _lib.VM_EINVAL, args
        assert b"guided_coeffs" in lib.vm_last_error()
    assert lib.vm_guided_workspace_bytes(2, 5, 7) == 2 * 5 * 7 * 16
    assert lib.vm_guided_workspace_bytes(0, 5, 7) == 0 and lib.vm_guided_workspace_bytes(1, 1 << 20, 1 << 10) == 0
    ok = (W, P, 1, 4, 4, 2, Q)
    for i, v in [(0, None), (1, None), (6, None), (2, 0), (3, 0), (4, 0), (5, 1), (5, 5), (0, W + 4), (6, Q + 2),
                 (6, P + 16), (6, W)]:
        args = ok[:i] + (v,) + ok[i + 1:]
        assert lib.vm_guided_apply(*args, None) == _lib.VM_EINVAL, args
        assert b"guided_apply" in lib.vm_last_error()


def test_option_checks():
    from vmatting import ops
    assert ops.GUIDED_DEFAULTS == {"r": 2, "eps": 1e-3}
    assert ops.check_guided_options("t") == (2, 1e-3)
    assert ops.check_guided_options("t", r=np.int64(8), eps=1) == (8, 1.0)
    assert ops.check_guided_options("t", r=1, eps=1e-5) == (1, 1e-5)
    for kw in (dict(r=0), dict(r=9), dict(eps=9e-6), dict(eps=1.01), dict(eps=float("nan")), dict(eps=-1.0)):
        with pytest.raises(ValueError):
            ops.check_guided_options("t", **kw)
    for kw in (dict(r=2.0), dict(r=True), dict(r="2"), dict(eps="1e-3"), dict(eps=None), dict(eps=True)):
        with pytest.raises(TypeError):
            ops.check_guided_options("t", **kw)
    assert ops.guided_options("t", None) == ops.GUIDED_DEFAULTS
    assert ops.guided_options("t", {"eps": 0.5}) == {"r": 2, "eps": 0.5}
    with pytest.raises(ValueError):
        ops.guided_options("t", {"radius": 2})
    for v in (1, 5, 0, -2):
        with pytest.raises(ValueError):
            ops.check_scale("t", v)
    for v in (2.0, "2", True, None):
        with pytest.raises(TypeError):
            ops.check_scale("t", v)
    assert ops.check_scale("t", 1, smallest=1) == 1 and ops.check_scale("t", np.int32(4)) == 4
    assert ops.reduced_size(2160, 3840, 2) == (1080, 1920) and ops.reduced_size(7, 10, 3) == (3, 4)


def test_ops_refuse_bad_arguments_before_the_device():
    from vmatting import ops
    u8, f32 = torch.uint8, torch.float32
    cmp, tri = torch.zeros((2, 5, 7, 3), dtype=u8), torch.zeros((2, 5, 7), dtype=u8)
    g, p, ab = torch.zeros((2, 3, 4, 3), dtype=u8), torch.zeros((2, 3, 4), dtype=f32), torch.zeros((2, 3, 4, 4), dtype=f32)
    V, T = ValueError, TypeError
    cases = [
        (V, lambda: ops.frames_reduce_u8(cmp, 1)), (V, lambda: ops.frames_reduce_u8(cmp, 5)),
        (T, lambda: ops.frames_reduce_u8(cmp, 2.0)), (V, lambda: ops.frames_reduce_u8(cmp, 2, kind="max")),
        (V, lambda: ops.frames_reduce_u8(tri, 2)), (V, lambda: ops.frames_reduce_u8(cmp, 2, kind="trimap")),
        (V, lambda: ops.frames_reduce_u8(cmp[..., :2], 2)), (T, lambda: ops.frames_reduce_u8(cmp.float(), 2)),
        (T, lambda: ops.frames_reduce_u8(cmp.numpy(), 2)), (V, lambda: ops.frames_reduce_u8(cmp[:, :, ::2], 2)),
        (V, lambda: ops.frames_reduce_u8(cmp, 2, out=torch.zeros((2, 3, 3, 3), dtype=u8))),
        (T, lambda: ops.frames_reduce_u8(cmp, 2, out=torch.zeros((2, 3, 4, 3), dtype=f32))),
        (V, lambda: ops.guided_coeffs(g, p, r=0)), (V, lambda: ops.guided_coeffs(g, p, r=9)),
        (V, lambda: ops.guided_coeffs(g, p, eps=1e-6)), (V, lambda: ops.guided_coeffs(g, p, eps=2.0)),
        (T, lambda: ops.guided_coeffs(g, p, r=1.5)), (V, lambda: ops.guided_coeffs(g[..., :2], p)),
        (T, lambda: ops.guided_coeffs(g.float(), p)), (T, lambda: ops.guided_coeffs(g, p.double())),
        (V, lambda: ops.guided_coeffs(g, p[:, :2])), (V, lambda: ops.guided_coeffs(g, p[:1])),
        (T, lambda: ops.guided_coeffs(g.numpy(), p)), (T, lambda: ops.guided_coeffs(g, p.numpy())),
        (V, lambda: ops.guided_coeffs(g, p, out=torch.zeros((2, 3, 4, 3), dtype=f32))),
        (V, lambda: ops.guided_coeffs(g, p, out=torch.zeros((2, 3, 4), dtype=f32))),
        (V, lambda: ops.guided_apply(ab, cmp, 1)), (V, lambda: ops.guided_apply(ab, cmp, 5)),
        (V, lambda: ops.guided_apply(ab, cmp, 3)),                 # 5 x 7 at scale 3 is 2 x 3, not 3 x 4
        (V, lambda: ops.guided_apply(ab[..., :3], cmp, 2)), (T, lambda: ops.guided_apply(ab.double(), cmp, 2)),
        (T, lambda: ops.guided_apply(ab, cmp.float(), 2)), (V, lambda: ops.guided_apply(ab, cmp[0], 2)),
        (T, lambda: ops.guided_apply(ab.numpy(), cmp, 2)),
        (V, lambda: ops.guided_apply(ab, cmp, 2, out=torch.zeros((2, 5, 7, 2), dtype=f32))),
        (T, lambda: ops.guided_apply(ab, cmp, 2, out=torch.zeros((2, 5, 7, 1), dtype=torch.float64))),
        (V, lambda: ops.guided_upsample(p, cmp, 6)), (V, lambda: ops.guided_upsample(p, cmp, 2, r=0)),
        (V, lambda: ops.guided_upsample(p, cmp, 2, eps=0.0)),
        (V, lambda: ops.guided_upsample(p, cmp, 2, guide_lo=g[:, :2])),
        # and the right arguments on the host are refused last: nothing computes on the CPU
        (T, lambda: ops.frames_reduce_u8(cmp, 2)), (T, lambda: ops.frames_reduce_u8(tri, 3, kind="trimap")),
        (T, lambda: ops.guided_coeffs(g, p)), (T, lambda: ops.guided_apply(ab, cmp, 2)),
        (T, lambda: ops.guided_upsample(p, cmp, 2)),
    ]
    for i, (exc, call) in enumerate(cases):
        with pytest.raises(exc):
            call()
            pytest.fail("case %d raised nothing" % i)


def test_upsample_matte_rejects_bad_arguments():
    from vmatting import reader
    cmp, lo = np.zeros((5, 7, 3), np.uint8), np.zeros((3, 4), np.float32)
    for exc, args, kw in [(ValueError, (lo, cmp, 1), {}), (ValueError, (lo, cmp, 5), {}), (TypeError, (lo, cmp, 2.0), {}),
                          (ValueError, (lo, cmp, 2), dict(radius=2)), (ValueError, (lo, cmp, 2), dict(r=0)),
                          (ValueError, (lo, cmp, 2), dict(eps=1e-6)), (TypeError, (lo, cmp, 2), dict(r=2.5)),
                          (TypeError, (lo.astype(np.float16), cmp, 2), {}), (TypeError, (lo, cmp.astype(np.int16), 2), {}),
                          (ValueError, (lo, cmp[..., :2], 2), {}), (ValueError, (lo, cmp[None], 2), {}),
                          (ValueError, (lo[:2], cmp, 2), {}), (ValueError, (lo, cmp, 3), {})]:
        with pytest.raises(exc):
            reader.upsample_matte(*args, **kw)


@pytest.fixture(scope="module")
def models(vgg0):
    from vmatting import unet
    np.random.seed(0)  # (the constructors do not touch the device)
    return unet.UNetVideo(vgg0, dtype="bf16", device="cuda"), unet.UNetImage(vgg0, dtype="bf16", device="cuda")


def test_frame_stream_scale_arguments(models):
    from vmatting import FrameStream
    mv, mi = models
    for kw in (dict(scale=0), dict(scale=5), dict(scale=-1), dict(scale=1, guided_options={}),
               dict(guided_options={"r": 2}), dict(scale=2, guided_options={"radius": 2}),
               dict(scale=2, guided_options={"r": 0}), dict(scale=2, guided_options={"r": 9}),
               dict(scale=3, guided_options={"eps": 1e-6}), dict(scale=3, guided_options={"eps": 1.5}),
               dict(scale=4, guided_options={"eps": float("nan")})):
        with pytest.raises(ValueError):
            FrameStream(mv, 9, 14, **kw)
    for kw in (dict(scale=2.0), dict(scale="2"), dict(scale=True), dict(scale=2, guided_options={"r": 2.0}),
               dict(scale=2, guided_options={"eps": "1e-3"})):
        with pytest.raises(TypeError):
            FrameStream(mv, 9, 14, **kw)
    fs = FrameStream(mv, 9, 14, scale=1)
    assert fs.scale == 1 and not hasattr(fs, "guided")
    fs = FrameStream(mv, 9, 14, scale=4, guided_options={"eps": 0.01})
    assert (fs.scale, fs.h, fs.w, fs.hm, fs.wm) == (4, 9, 14, 3, 4) and fs.guided == {"r": 2, "eps": 0.01}
    fs = FrameStream(mi, 9, 14, trimap=False, scale=3)
    assert (fs.hm, fs.wm) == (3, 5) and fs.guided == {"r": 2, "eps": 1e-3}
    # items stay full-resolution: a reduced frame is the wrong shape
    fs = FrameStream(mv, 9, 14, chunk=2, scale=2)
    z = lambda *s: np.zeros(s, np.uint8)  # noqa: E731
    with pytest.raises(ValueError):
        next(fs.run(iter([(z(2, 5, 7, 3), z(2, 5, 7, 3), z(2, 5, 7))])))
    assert fs.check_item((z(2, 9, 14, 3), z(2, 9, 14, 3), z(2, 9, 14)))[3] == 2
