"""The plate alignment on the CPU: the numpy restatement (tests/plate_align_ref.py) recovers known motions, brings the
plate trimap back, and falls back to the identity where there is nothing to fit; the argument checks of the C calls,
ops, reader and FrameStream, none of which touches a device."""

import numpy as np
import pytest
import torch

import flow_est_ref as fe
import plate_align_ref as ref
import trimap_plate_ref as tp

SEEDS = (0, 1, 2)
# The largest corner error of the restatement over motions x gains x seeds, measured, and the bound: twice that (at most
# 0.25 px: half a pixel is the failure the alignment exists to remove).
#   96 x 160 (4 levels), all seven motions: 0.0525 px (the issue's prototype: 0.049)
#   64 x 96 (3 levels), id / sub / rot / zoom: 0.1051 px (the prototype: 0.091 with `one`)
# 64 x 96 leaves out `big` and `shift`, which are outside its basin (the guards test below), and `one`, which the
# restatement itself fails in one of its nine cases: at gain 1.25, seed 2 it ends 0.69 px off with 41 % support.
WORST = {(96, 160): 0.0525, (64, 96): 0.1051}
BOUND = {k: 2 * v for k, v in WORST.items()}
MOTIONS = {(96, 160): tuple(ref.MOTIONS), (64, 96): ("id", "sub", "rot", "zoom")}
assert all(b <= 0.25 for b in BOUND.values())


@pytest.fixture(scope="module")
def fits():
    """{(h, w, motion, gain, seed): (frame, plate, alpha, true, params, support)}, made once."""
    out = {}
    for (h, w), motions in MOTIONS.items():
        for m in motions:
            for g in ref.GAINS:
                for seed in SEEDS:
                    scene = ref.scene(h, w, m, g, seed)
                    out[h, w, m, g, seed] = scene + ref.fit_frames(scene[0], scene[1])
    return out


@pytest.mark.parametrize("h,w", list(MOTIONS))
def test_restatement_recovers_the_motion(fits, h, w):
    worst = {}
    for (hh, ww, m, g, seed), (_, _, _, true, prm, sup) in fits.items():
        if (hh, ww) == (h, w):
            worst[m, g, seed] = ref.corner_error(prm, true, h, w)
            assert sup * 4 >= h * w
            assert m == "id" or not np.array_equal(prm, ref.identity())
            assert abs(float(prm[6]) / g - 1) <= 0.02 and prm[7] == 0
    print("corner error %d x %d: worst %.4f px (bound %.4f)" % (h, w, max(worst.values()), BOUND[h, w]))
    assert max(worst.values()) <= BOUND[h, w], sorted(worst.items(), key=lambda kv: -kv[1])[:3]


@pytest.mark.parametrize("motion", ref.TABLE)
def test_the_trimap_comes_back(fits, motion):
    h, w = 96, 160
    frame, plate, alpha, true, prm, _ = fits[h, w, motion, 1.0, 0]
    share = lambda p: float((tp.trimap(frame, p, **tp.DEFAULTS) == 0)[alpha == 0].mean())  # noqa: E731
    fitted = ref.apply(plate, prm)
    given, got, want = share(plate), share(fitted), share(ref.apply(plate, true))
    print("%s: background labelled 0: plate as given %.3f, fitted %.3f, true map %.3f" % (motion, given, got, want))
    assert abs(got - want) <= 0.02
    assert want >= 0.7
    if motion in ("sub", "one", "shift"):
        assert given <= 0.1
    assert not ((tp.trimap(frame, fitted, **tp.DEFAULTS) == 0) & (alpha == 1)).any()


@pytest.mark.parametrize("h,w", [(96, 160), (64, 96)])
@pytest.mark.parametrize("name", list(ref.DEGENERATE))
def test_nothing_to_fit_is_the_identity(name, h, w):
    for seed in SEEDS:
        frame, plate = ref.DEGENERATE[name](h, w, seed)
        prm, sup = ref.fit_frames(frame, plate)
        assert np.array_equal(prm, ref.identity()), (seed, prm)
        # the support shows why: none for a plate without texture, well under the share for unrelated images
        assert sup == 0 if name == "constant" else 0 < sup * 6 < h * w, (seed, sup)


def test_outside_the_basin_is_the_identity_or_right():
    """`big` and `shift` at 64 x 96 (a 4-pixel coarsest level): the identity or a map within the bound, never one beyond
    ``reach``."""
    h, w = 64, 96
    seen = set()
    for m in ("big", "shift"):
        for g in ref.GAINS:
            for seed in SEEDS:
                frame, plate, _, true = ref.scene(h, w, m, g, seed)
                prm, _ = ref.fit_frames(frame, plate)
                ident = np.array_equal(prm, ref.identity())
                seen.add(ident)
                assert ident or ref.corner_error(prm, true, h, w) <= BOUND[h, w], (m, g, seed, prm)
                assert ref.corner_error(prm, ref.identity(), h, w) <= min(h, w) / 6
    assert seen == {True, False}


def test_a_tiny_coarsest_level_misleads_the_fit():
    """128 x 192 at 6 levels starts on 8 x 12 pixels: `one` at gain 0.8 (seed 4) leaves there by tens of pixels and the
    guards return the identity; at 4 levels (16 x 24) it is found.  Recorded, not wanted: ``levels`` is the knob."""
    h, w = 128, 192
    frame, plate, _, true = ref.scene(h, w, "one", 0.8, 4)
    prm, sup = ref.fit_frames(frame, plate)
    assert np.array_equal(prm, ref.identity()) and sup * 4 < h * w
    prm, sup = ref.fit_frames(frame, plate, levels=4)
    assert ref.corner_error(prm, true, h, w) <= 0.05 and sup * 4 >= h * w


def test_reach_and_share_guards():
    h, w = 96, 160
    frame, plate, _, true = ref.scene(h, w, "big", 1.0, 0)
    prm, sup = ref.fit_frames(frame, plate)
    assert ref.corner_error(prm, true, h, w) <= BOUND[h, w]
    far, sup2 = ref.fit_frames(frame, plate, reach=8)  # 12 px: 15.4 px is beyond it
    assert np.array_equal(far, ref.identity()) and sup2 == sup
    none, sup3 = ref.fit_frames(frame, plate, min_share=1)  # every pixel would have to agree: the disc does not
    assert np.array_equal(none, ref.identity()) and 0 < sup3 < h * w


def test_apply_identity_and_border():
    rs = np.random.RandomState(3)
    bg = rs.randint(0, 256, (17, 23, 3)).astype(np.uint8)
    assert np.array_equal(ref.apply(bg, ref.identity()), bg)
    shifted = ref.apply(bg, np.array([0, 0, 2, 0, 0, -1, 1, 0], np.float32))
    assert np.array_equal(shifted[1:, :-2], bg[:-1, 2:])
    assert np.array_equal(shifted[0, :-2], bg[0, 2:]) and (shifted[:, -2:] == shifted[:, -3:-2]).all()  # replicated
    half = ref.apply(bg, np.array([0, 0, .5, 0, 0, 0, 1, 0], np.float32)).astype(np.int64)
    mean = (bg[:, :-1].astype(np.int64) + bg[:, 1:]) / 2
    assert (np.abs(half[:, :-1] - mean) <= 0.5).all()
    far = ref.apply(bg, np.array([0, 0, 1e6, 0, 0, -1e6, 1, 0], np.float32))
    assert (far == bg[0, -1]).all()


def test_solve_is_the_linear_solve():
    rs = np.random.RandomState(5)
    M = rs.normal(size=(40, 7))
    A, b = M.T @ M, rs.normal(size=7)
    assert np.allclose(ref.solve(A, b), np.linalg.solve(A, b), rtol=1e-10)
    assert ref.solve(np.zeros((7, 7)), b) is None
    A[3, 3] = np.nan
    assert ref.solve(A, b) is None


def test_pyramids_are_the_flow_estimate_s():
    assert ref.fe is fe and not hasattr(ref, "pyramid") and not hasattr(ref, "bilinear")
    assert ref.DEFAULTS == {"iters": 4, "tol": 16.0, "min_share": 4, "reach": 6, "levels": 6}


# ---------------------------------------------------------------- argument checks, no device
def test_c_calls_reject_bad_arguments():
    from vmatting import _lib
    lib = _lib.lib()
    for args in ref.bad_fit_arguments():
        assert lib.vm_plate_align_fit(*args, None) == _lib.VM_EINVAL, args
        assert b"plate_align_fit" in lib.vm_last_error()
    for args in ref.bad_apply_arguments():
        assert lib.vm_plate_align_apply(*args, None) == _lib.VM_EINVAL, args
        assert b"plate_align_apply" in lib.vm_last_error()
    size = lib.vm_plate_align_workspace_bytes
    assert size(1, 16, 16, 6) > 0 and size(5, 1080, 1920, 6) == 5 * size(1, 1080, 1920, 6) and size(3, 17, 23, 1) % 16 == 0
    assert size(1, 1080, 1920, 6) <= 1 << 17
    for shape in ((0, 16, 16, 6), (-1, 16, 16, 6), (1, 15, 16, 6), (1, 16, 15, 6), (1, 16, 16, 0), (1, 40000, 16, 6)):
        assert size(*shape) == 0


def test_option_checks():
    from vmatting import ops
    assert ops.ALIGN_DEFAULTS == ref.DEFAULTS and list(ops.ALIGN_DEFAULTS) == ["iters", "tol", "min_share", "reach", "levels"]
    assert ops.check_align_options("t") == (4, 16.0, 4, 6, 6)
    assert ops.check_align_options("t", np.int64(64), 3, 4096, 1024, 1) == (64, 3.0, 4096, 1024, 1)
    for kw in (dict(iters=0), dict(iters=65), dict(tol=0), dict(tol=-1.0), dict(tol=float("nan")), dict(tol=float("inf")),
               dict(min_share=0), dict(min_share=4097), dict(reach=0), dict(reach=1025), dict(levels=0)):
        with pytest.raises(ValueError):
            ops.check_align_options("t", **kw)
    for kw in (dict(iters=4.0), dict(iters=True), dict(tol="16"), dict(tol=None), dict(tol=True), dict(min_share=4.0),
               dict(reach="6"), dict(levels=6.0)):
        with pytest.raises(TypeError):
            ops.check_align_options("t", **kw)
    assert ops.align_options("t", None) == ops.ALIGN_DEFAULTS
    assert ops.align_options("t", {"tol": 8}) == dict(ops.ALIGN_DEFAULTS, tol=8.0)
    with pytest.raises(ValueError):
        ops.align_options("t", {"tolerance": 8})
    assert ops.ALIGN_FIT == "fit"
    assert ops.check_align_mode("t", None, None) is None
    assert ops.check_align_mode("t", "fit", None) == ops.ALIGN_DEFAULTS
    assert ops.check_align_mode("t", "fit", {"reach": 8}) == dict(ops.ALIGN_DEFAULTS, reach=8)
    for align, options in [("auto", None), (True, None), (1, None), ("", None), ("Fit", None), (None, {}),
                           (None, {"tol": 8}), ("fit", {"tols": 8}), ("fit", {"iters": 0})]:
        with pytest.raises(ValueError):
            ops.check_align_mode("t", align, options)
    with pytest.raises(TypeError):
        ops.check_align_mode("t", "fit", {"iters": 2.5})


def test_ops_refuse_bad_arguments_before_the_device():
    from vmatting import ops
    u8, f32, i32 = torch.uint8, torch.float32, torch.int32
    pyr, one = torch.zeros((2, 400), dtype=f32), torch.zeros((1, 400), dtype=f32)  # 16 x 23 at one level: 368 floats
    bg, plate, prm = torch.zeros((2, 16, 23, 3), dtype=u8), torch.zeros((16, 23, 3), dtype=u8), torch.zeros((2, 8), dtype=f32)
    V, T = ValueError, TypeError
    fit = lambda *a, **k: ops.plate_align_fit(*a, **dict(dict(levels=1), **k))  # noqa: E731
    cases = [
        (V, lambda: fit(pyr, pyr, 16, 23, iters=0)), (V, lambda: fit(pyr, pyr, 16, 23, tol=0.0)),
        (V, lambda: fit(pyr, pyr, 16, 23, min_share=0)), (V, lambda: fit(pyr, pyr, 16, 23, reach=0)),
        (V, lambda: fit(pyr, pyr, 16, 23, levels=0)), (T, lambda: fit(pyr, pyr, 16, 23, iters=4.0)),
        (V, lambda: fit(pyr, pyr, 15, 23)), (V, lambda: fit(pyr, pyr, 16, 15)), (T, lambda: fit(pyr, pyr, 16.0, 23)),
        (V, lambda: fit(pyr[0], pyr, 16, 23)), (V, lambda: fit(pyr, torch.zeros((3, 400), dtype=f32), 16, 23)),
        (T, lambda: fit(pyr.double(), pyr, 16, 23)), (T, lambda: fit(pyr, one.half(), 16, 23)),
        (T, lambda: fit(pyr.numpy(), pyr, 16, 23)), (V, lambda: fit(pyr[:, ::2], one, 16, 23)),
        (V, lambda: fit(pyr, one, 16, 23, out=torch.zeros((2, 7), dtype=f32))),
        (V, lambda: fit(pyr, one, 16, 23, out=torch.zeros((2, 8), dtype=torch.float64))),
        (V, lambda: fit(pyr, one, 16, 23, support=torch.zeros((2, 1), dtype=i32))),
        (V, lambda: fit(pyr, one, 16, 23, support=torch.zeros(2, dtype=torch.int64))),
        (V, lambda: ops.plate_align_apply(bg, prm[:, :7])), (V, lambda: ops.plate_align_apply(bg, prm[0])),
        (T, lambda: ops.plate_align_apply(bg, prm.double())), (T, lambda: ops.plate_align_apply(bg, prm.numpy())),
        (T, lambda: ops.plate_align_apply(bg.float(), prm)), (V, lambda: ops.plate_align_apply(bg[..., :2], prm)),
        (V, lambda: ops.plate_align_apply(torch.zeros((3, 16, 23, 3), dtype=u8), prm)),
        (V, lambda: ops.plate_align_apply(plate, prm, out=torch.zeros((1, 16, 23, 3), dtype=u8))),
        (V, lambda: ops.plate_align_apply(plate, prm, out=torch.zeros((2, 16, 23, 3), dtype=i32))),
        # and the right arguments on the host are refused last: nothing computes on the CPU
        (T, lambda: fit(pyr, pyr, 16, 23)), (T, lambda: fit(pyr, one, 16, 23)), (T, lambda: fit(pyr, one[0], 16, 23)),
        (T, lambda: ops.plate_align_apply(bg, prm)), (T, lambda: ops.plate_align_apply(plate, prm)),
    ]
    for i, (exc, call) in enumerate(cases):
        with pytest.raises(exc):
            call()
            pytest.fail("case %d raised nothing" % i)


def test_reader_rejects_bad_arguments():
    from vmatting import reader
    cmp, bg = np.zeros((16, 23, 3), np.uint8), np.zeros((16, 23, 3), np.uint8)
    for exc, args, kw in [(ValueError, (cmp, bg), dict(tols=8)), (ValueError, (cmp, bg), dict(tol=0)),
                          (ValueError, (cmp, bg), dict(reach=2000)), (TypeError, (cmp, bg), dict(iters=2.5)),
                          (TypeError, (cmp.astype(np.int16), bg), {}), (TypeError, (cmp, bg.astype(np.float32)), {}),
                          (ValueError, (cmp[..., :2], bg[..., :2]), {}), (ValueError, (cmp[None], bg[None]), {}),
                          (ValueError, (cmp, bg[:, :20]), {}), (ValueError, (cmp[:15], bg[:15]), {})]:
        with pytest.raises(exc):
            reader.align_plate(*args, **kw)
    for kw in (dict(align="auto"), dict(align=True), dict(align_options={}), dict(align="fit", align_options={"tols": 1}),
               dict(align="fit", align_options={"iters": 65})):
        with pytest.raises(ValueError):
            reader.trimap_from_plate(cmp, bg, **kw)
    with pytest.raises(ValueError):
        reader.trimap_from_plate(cmp[:15], bg[:15], align="fit")
    with pytest.raises(TypeError):
        reader.trimap_from_plate(cmp, bg, align="fit", align_options={"min_share": 1.5})
    with pytest.raises(TypeError):
        reader.trimap_from_plate(cmp, bg, None, None, None, None, None, None, None, "fit")  # keyword-only


@pytest.fixture(scope="module")
def model(vgg0):
    from vmatting import unet
    np.random.seed(0)  # (the constructor does not touch the device)
    return unet.UNetVideo(vgg0, dtype="bf16", device="cuda")


def test_frame_stream_align_arguments(model):
    from vmatting import FrameStream
    for kw in (dict(align="auto"), dict(align=True), dict(align=1), dict(align="Fit"), dict(align_options={}),
               dict(align_options={"tol": 8}), dict(align="fit", align_options={"tols": 8}),
               dict(align="fit", align_options={"iters": 0}), dict(align="fit", align_options={"reach": 1025})):
        with pytest.raises(ValueError):
            FrameStream(model, 32, 48, **kw)
    with pytest.raises(TypeError):
        FrameStream(model, 32, 48, align="fit", align_options={"iters": 4.0})
    with pytest.raises(ValueError):
        FrameStream(model, 15, 48, align="fit")  # the pyramid's own limit
    fs = FrameStream(model, 15, 48)
    assert fs.align is None
    with pytest.raises(ValueError):
        fs.last_alignment()
    fs = FrameStream(model, 32, 48, align="fit", align_options={"tol": 8})
    assert fs.align == dict(ref.DEFAULTS, tol=8.0)
    with pytest.raises(RuntimeError):
        fs.last_alignment()
