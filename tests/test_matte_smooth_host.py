"""CPU checks of the flow-compensated temporal matte filter (include/vmatting.h): the numpy restatement on exact cases,
what the filter is worth on the synthetic noisy clip, and every refusal of the C call, ops, reader and FrameStream - all
checked before any device work."""

import numpy as np
import pytest
import torch

import matte_smooth_ref as ref
import score_ref

F = np.float32


# ---------------------------------------------------------------- the restatement
@pytest.fixture(scope="module")
def material():
    n, h, w = 4, 23, 35
    return {"alpha": score_ref.mattes(n, h, w, 1, wild=True), "cmp": ref.frames(n, h, w, 2),
            "flow": ref.moderate_flow(n, h, w, 3), "wild": score_ref.wild_flow(n, h, w, 4)}


def test_strength_zero_is_the_clamp(material):
    for flow in (material["flow"], material["wild"]):
        out, _ = ref.smooth(material["alpha"], material["cmp"], flow, strength=0.0)
        assert np.array_equal(out, score_ref.unit(material["alpha"]))


def test_a_still_clip_of_equal_mattes_is_unchanged(material):
    alpha = np.repeat(score_ref.unit(material["alpha"][:1]), 4, 0)
    cmp = np.repeat(material["cmp"][:1], 4, 0)
    out, weight = ref.smooth(alpha, cmp, np.zeros((4, 23, 35, 2), F))
    assert np.array_equal(out, alpha)
    assert (weight[0] == 0).all() and (weight[1:] == 1).all()  # both gates wide open, and nothing to pull


def test_a_still_clip_with_the_jump_gate_open_is_the_exponential_recurrence(material):
    """Zero flow, identical frames (the colour gate is 1), a huge jump (the other gate is 1 - |a - p| / jump = 1 in f32):
    s[j] = unit(a + strength (s[j - 1] - a)) exactly."""
    alpha = material["alpha"]
    cmp = np.repeat(material["cmp"][:1], 4, 0)
    for strength in (0.5, 0.8):
        out, weight = ref.smooth(alpha, cmp, np.zeros((4, 23, 35, 2), F), strength=strength, jump=1e30)
        a = score_ref.unit(alpha)
        want = a[0]
        for j in range(1, 4):
            want = score_ref.unit(a[j] + F(strength) * (want - a[j]))
            assert np.array_equal(out[j], want)
        assert (weight[1:] == 1).all()
    prev = (alpha[3], cmp[0])  # and frame 0 follows ``prev``
    out, weight = ref.smooth(alpha[:1], cmp[:1], np.zeros((1, 23, 35, 2), F), prev=prev, jump=1e30)
    assert np.array_equal(out[0], score_ref.unit(a[0] + F(0.5) * (a[3] - a[0]))) and (weight == 1).all()


def test_a_flow_that_leaves_the_frame_keeps_the_matte():
    h, w = 9, 11
    alpha = score_ref.mattes(2, h, w, 5, wild=True)
    cmp = np.repeat(ref.frames(1, h, w, 6), 2, 0)
    a = score_ref.unit(alpha)
    for u, v in ((np.nan, 0), (0, np.nan), (np.inf, 0), (0, -np.inf), (1e6, 0), (0, -3e4), (-0.001 - (w - 1), 0),
                 (0, h)):
        flow = np.zeros((2, h, w, 2), F)
        flow[..., 0], flow[..., 1] = u, v
        out, weight = ref.smooth(alpha, cmp, flow)
        gone = ~ref.targets(flow[1])[0]
        assert gone.any() and np.array_equal(out[1][gone], a[1][gone]) and (weight[1][gone] == 0).all()
    flow = np.zeros((2, h, w, 2), F)
    flow[1, :, :, 0] = (w - 1) - np.arange(w)  # exactly onto the last column: inside, x1 clamped
    out, weight = ref.smooth(alpha, cmp, flow, jump=1e30, tol=1e30)
    assert ref.targets(flow[1])[0].all()
    assert np.array_equal(out[1], score_ref.unit(a[1] + F(0.5) * (a[0][:, -1:] - a[1])))


def test_the_result_is_always_within_the_unit_interval(material):
    for flow in (material["flow"], material["wild"]):
        for opts in ({}, {"strength": 0.99, "tol": 1e-3, "jump": 1e-3}, {"strength": 0.9, "tol": 1e30, "jump": 1e30}):
            out, weight = ref.smooth(material["alpha"], material["cmp"], flow,
                                     prev=(material["alpha"][2], material["cmp"][3]), **opts)
            for v in (out, weight):
                assert np.isfinite(v).all() and v.min() >= 0 and v.max() <= 1
    assert (ref.smooth(material["alpha"], material["cmp"], material["flow"])[1][1:] > 0).any()  # the gates do open


# ---------------------------------------------------------------- what the filter is worth on the synthetic clip
SIZES = ((48, 64), (96, 128))


@pytest.mark.parametrize("h,w", SIZES)
def test_exact_flow_lowers_dtssd_and_keeps_sad(h, w):
    """ref.noisy_clip (8 frames, a soft-edged textured disc moving 1.5 x 0.7 px/frame over a textured plate, matte noise
    of sigma 0.08 within 8 px of the edge), exact flows, the defaults, filtered over raw, seeds 0..2.  Measured with this
    restatement: dtSSD 0.756 - 0.767 and SAD 0.974 - 0.993 over both sizes (the issue's prototype, on its own scene:
    0.74 - 0.76 and 0.995 - 1.000).  The bounds guard against a broken gate; they are no tuning targets."""
    for seed in range(3):
        c = ref.noisy_clip(8, h, w, seed)
        out, _ = ref.smooth(c["alpha"], c["cmp"], c["backward"])
        d, s = ref.dtssd(out, c["gt"]) / ref.dtssd(c["alpha"], c["gt"]), ref.sad(out, c["gt"]) / ref.sad(c["alpha"], c["gt"])
        print("%d x %d seed %d: dtSSD ratio %.3f, SAD ratio %.4f" % (h, w, seed, d, s))
        assert d <= 0.85 and s <= 1.02


@pytest.mark.parametrize("h,w", SIZES)
def test_a_wrong_flow_does_not_smear(h, w):
    """The subject at 3 px/frame under a zero flow.  Measured: SAD 1.011 - 1.027 of raw with the gates at their
    defaults; with both gates off (tol = jump = 1e30) SAD 2.88 - 3.03 and dtSSD 1.76 - 1.80 of raw (the prototype: 3.2 and
    1.95)."""
    for seed in range(3):
        c = ref.noisy_clip(8, h, w, seed, speed=(3.0, 0.0))
        zero = np.zeros_like(c["backward"])
        raw = ref.sad(c["alpha"], c["gt"])
        gated = ref.sad(ref.smooth(c["alpha"], c["cmp"], zero)[0], c["gt"]) / raw
        print("%d x %d seed %d: wrong-flow SAD ratio %.4f" % (h, w, seed, gated))
        assert gated <= 1.05
        if seed == 0:  # and it is the gates that do it
            assert ref.sad(ref.smooth(c["alpha"], c["cmp"], zero, tol=1e30, jump=1e30)[0], c["gt"]) / raw >= 2.0


# ---------------------------------------------------------------- argument checks, no device
def test_signature_table_has_the_symbol():
    from vmatting import _lib
    rows = [r for r in _lib.SIGNATURES if r[0] == "vm_matte_smooth"]
    assert len(rows) == 1 and len(rows[0][2]) == 14 and rows[0][2][8:11] == [_lib.c_float] * 3
    assert _lib.ABI_VERSION == 1 and _lib.lib().vm_abi_version() == 1  # additive: the version stays


def test_c_call_rejects_bad_arguments():
    """Pointers that are never dereferenced: 2 frames of 4 x 4, so alpha / out / weight are 128 bytes, cmp 96, backward
    256, prev_alpha 64, prev_cmp 48."""
    from vmatting import _lib
    lib = _lib.lib()
    A, C, B, PA, PC, O, W = (i << 20 for i in range(1, 8))
    ok = (A, C, B, PA, PC, 2, 4, 4, 0.5, 24.0, 0.3, O, W)
    nan, inf = float("nan"), float("inf")
    bad = [(0, None), (1, None), (2, None), (11, None),                           # a null pointer
           (3, None), (4, None),                                                  # one prev pointer alone
           (5, 0), (6, 0), (7, 0), (5, -1), (6, 1 << 30),                         # shapes; 2 x 2^30 x 4 x 3 bytes
           (8, 1.0), (8, -0.01), (8, nan), (8, 1.5),                              # strength in [0, 1)
           (9, 0.0), (9, -1.0), (9, nan), (9, inf), (10, 0.0), (10, -0.3), (10, nan), (10, inf),
           (0, A + 2), (2, B + 1), (3, PA + 2), (11, O + 3), (12, W + 2),         # f32 pointers off 4 bytes
           (11, A + 4), (11, A - 4), (11, A + 124), (11, A - 124),                # out overlaps alpha but is not alpha
           (11, C + 92), (11, C - 124), (11, B + 252), (11, PA + 60), (11, PC + 44), (11, PC - 124),
           (12, A), (12, A + 124), (12, C + 92), (12, B - 124), (12, PA), (12, PC + 44), (12, O), (12, O + 124),
           (12, O - 124)]
    for i, v in bad:
        args = ok[:i] + (v,) + ok[i + 1:]
        assert lib.vm_matte_smooth(*args, None) == _lib.VM_EINVAL, args
        assert b"matte_smooth" in lib.vm_last_error()
    assert lib.vm_matte_smooth(*(ok[:11] + (A, A)), None) == _lib.VM_EINVAL     # in place, but weight on top of it
    assert b"weight" in lib.vm_last_error()
    assert lib.vm_matte_smooth(A, C, B, None, PC, 2, 4, 4, 0.5, 24.0, 0.3, O, None, None) == _lib.VM_EINVAL
    assert b"go together" in lib.vm_last_error()
    # n h w 3 beyond 2^31 - 1: 715827883 pixels are, 715827882 are not (the next check, a null pointer, refuses those)
    assert lib.vm_matte_smooth(A, C, B, None, None, 1, 715827883, 1, 0.5, 24.0, 0.3, O, None, None) == _lib.VM_EINVAL
    assert b"exceed" in lib.vm_last_error()
    assert lib.vm_matte_smooth(None, C, B, None, None, 1, 715827882, 1, 0.5, 24.0, 0.3, O, None, None) == _lib.VM_EINVAL
    assert b"null" in lib.vm_last_error()


def test_smooth_options():
    from vmatting import ops
    assert ops.SMOOTH_DEFAULTS == {"strength": 0.5, "tol": 24.0, "jump": 0.3} == ref.DEFAULTS
    face = lambda o: ops.smooth_options("t", o)  # noqa: E731
    assert face(None) == ops.SMOOTH_DEFAULTS and face({}) == ops.SMOOTH_DEFAULTS and face(None) is not ops.SMOOTH_DEFAULTS
    got = face({"tol": 12, "strength": np.float32(0.25)})
    assert got == {"strength": 0.25, "tol": 12.0, "jump": 0.3} and list(got) == list(ops.SMOOTH_DEFAULTS)
    assert all(type(v) is float for v in got.values())
    with pytest.raises(ValueError) as e:
        face({"tol": 12, "sigma": 3})
    assert "t takes" in str(e.value) and "'sigma'" in str(e.value)
    assert all(repr(k) in str(e.value) for k in ops.SMOOTH_DEFAULTS)
    for options in ({"strength": 1.0}, {"strength": -0.1}, {"strength": float("nan")}, {"tol": 0}, {"tol": -1.0},
                    {"tol": float("inf")}, {"tol": float("nan")}, {"jump": 0.0}, {"jump": float("nan")}, {"jump": 1e39}):
        with pytest.raises(ValueError, match="t: "):
            face(options)
    for options in ({"strength": "0.5"}, {"tol": None}, {"jump": True}, {"tol": [24.0]}):
        with pytest.raises(TypeError, match="t: "):
            face(options)
    assert ops.check_smooth_options("t", 0.0, 1e-3, 1e30) == (0.0, 1e-3, 1e30)
    assert ops.check_smooth_mode("t", None, None) is None
    assert ops.check_smooth_mode("t", "flow", None) == ops.SMOOTH_DEFAULTS
    assert ops.check_smooth_mode("t", "flow", {"jump": 1}) == {"strength": 0.5, "tol": 24.0, "jump": 1.0}
    for smooth, options in [("Flow", None), (True, None), (1, None), ("", None), ("median", None), (None, {}),
                            (None, {"tol": 24.0}), ("flow", {"tols": 8}), ("flow", {"strength": 1})]:
        with pytest.raises(ValueError):
            ops.check_smooth_mode("t", smooth, options)
    with pytest.raises(TypeError):
        ops.check_smooth_mode("t", "flow", {"tol": "24"})


def test_ops_refuse_bad_arguments_before_the_device():
    from vmatting import ops
    f32, u8 = torch.float32, torch.uint8
    alpha, cmp, bw = torch.zeros((2, 5, 7), dtype=f32), torch.zeros((2, 5, 7, 3), dtype=u8), torch.zeros((2, 5, 7, 2), dtype=f32)
    pa, pc = torch.zeros((5, 7), dtype=f32), torch.zeros((5, 7, 3), dtype=u8)
    V, T = ValueError, TypeError
    cases = [
        (V, lambda: ops.matte_smooth(alpha, cmp, bw, strength=1.0)), (V, lambda: ops.matte_smooth(alpha, cmp, bw, tol=0)),
        (V, lambda: ops.matte_smooth(alpha, cmp, bw, jump=float("nan"))), (T, lambda: ops.matte_smooth(alpha, cmp, bw, tol="24")),
        (V, lambda: ops.matte_smooth(alpha[0], cmp, bw)), (V, lambda: ops.matte_smooth(alpha, cmp[:1], bw)),
        (V, lambda: ops.matte_smooth(alpha, cmp, bw[..., :1])), (V, lambda: ops.matte_smooth(alpha, cmp[:, :4], bw)),
        (V, lambda: ops.matte_smooth(alpha[:, :, ::2], cmp[:, :, ::2], bw[:, :, ::2])),
        (T, lambda: ops.matte_smooth(alpha.double(), cmp, bw)), (T, lambda: ops.matte_smooth(alpha, cmp.float(), bw)),
        (T, lambda: ops.matte_smooth(alpha, cmp, bw.double())), (T, lambda: ops.matte_smooth(alpha.numpy(), cmp, bw)),
        (T, lambda: ops.matte_smooth(alpha, cmp, bw, prev=pa)), (T, lambda: ops.matte_smooth(alpha, cmp, bw, prev=(pa,))),
        (T, lambda: ops.matte_smooth(alpha, cmp, bw, prev=(pa, None))), (T, lambda: ops.matte_smooth(alpha, cmp, bw, prev=(pa, pc.float()))),
        (V, lambda: ops.matte_smooth(alpha, cmp, bw, prev=(pa[:4], pc))), (V, lambda: ops.matte_smooth(alpha, cmp, bw, prev=(pa, pc[None]))),
        (V, lambda: ops.matte_smooth(alpha, cmp, bw, out=torch.zeros((1, 5, 7), dtype=f32))),
        (V, lambda: ops.matte_smooth(alpha, cmp, bw, out=torch.zeros((2, 5, 7), dtype=torch.float64))),
        (V, lambda: ops.matte_smooth(alpha, cmp, bw, weight=torch.zeros((2, 5, 8), dtype=f32))),
        (V, lambda: ops.matte_smooth(alpha, cmp, bw, weight=torch.zeros((2, 5, 7), dtype=u8))),
        # and the right arguments on the host are refused last: nothing computes on the CPU
        (T, lambda: ops.matte_smooth(alpha, cmp, bw)), (T, lambda: ops.matte_smooth(alpha[..., None], cmp, bw, prev=(pa, pc))),
        (T, lambda: ops.matte_smooth(alpha, cmp, bw, prev=(pa[..., None], pc), out=alpha, weight=torch.zeros((2, 5, 7, 1), dtype=f32))),
    ]
    for i, (exc, call) in enumerate(cases):
        with pytest.raises(exc):
            call()
            pytest.fail("case %d raised nothing" % i)


def test_reader_rejects_bad_arguments():
    from vmatting import reader
    m, f, fl = np.zeros((2, 16, 20), F), np.zeros((2, 16, 20, 3), np.uint8), np.zeros((2, 16, 20, 2), F)
    for exc, args, kw in [(ValueError, (m, f, fl), dict(tols=8)), (ValueError, (m, f, fl), dict(strength=1.0)),
                          (TypeError, (m, f, fl), dict(jump="0.3")), (TypeError, (m.astype(np.float64), f, fl), {}),
                          (TypeError, (m, f.astype(np.int16), fl), {}), (TypeError, (m, f, fl.astype(np.float64)), {}),
                          (ValueError, (m[0], f, fl), {}), (ValueError, (m, f[:1], fl), {}), (ValueError, (m, f, fl[..., :1]), {}),
                          (ValueError, (m[:, :15], f[:, :15], None), {}),  # the estimator's 16 x 16
                          (ValueError, (m[:0], f[:0], fl[:0]), {})]:
        with pytest.raises(exc):
            reader.smooth_mattes(*args, **kw)


@pytest.fixture(scope="module")
def models(vgg0):
    from vmatting import unet
    np.random.seed(0)  # (the constructors do not touch the device)
    return (unet.UNetVideo(vgg0, dtype="bf16", device="cuda"), unet.UNetImage(vgg0, dtype="bf16", device="cuda"),
            unet.UNetVideo(vgg0, dtype="f16x3", device="cuda"))


def test_frame_stream_smooth_arguments(models):
    from vmatting import FrameStream, ops
    mv, mi, mx = models
    for kw in (dict(smooth="Flow"), dict(smooth=True), dict(smooth=1), dict(smooth="median"),
               dict(smooth_options={}), dict(smooth_options={"tol": 24.0}),           # smooth_options without smooth
               dict(smooth="flow", smooth_options={"tols": 8}), dict(smooth="flow", smooth_options={"strength": 1.0}),
               dict(smooth="flow", flow="given"),                                      # given flows go with propagate
               dict(smooth="flow", flow="files"), dict(smooth="flow", flow_options={"sweeps": 3}),
               dict(smooth="flow", flow_options={"iters": 0})):
        with pytest.raises(ValueError):
            FrameStream(mv, 32, 48, **kw)
    with pytest.raises(TypeError):
        FrameStream(mv, 32, 48, smooth="flow", smooth_options={"tol": "24"})
    for h, w in ((15, 48), (32, 15)):
        with pytest.raises(ValueError, match="16 x 16"):
            FrameStream(mv, h, w, smooth="flow")                                       # the estimator's smallest frame
    FrameStream(mv, 15, 48, smooth="flow", trimap="propagate", flow="given")           # given flows need none
    with pytest.raises(ValueError, match="f16x3"):
        FrameStream(mx, 32, 48, smooth="flow")
    assert FrameStream(mx, 32, 48).smooth is None
    # without the filter (and without "propagate") flow and flow_options are refused as ever
    for kw in (dict(flow="estimate"), dict(flow_options={"iters": 5})):
        with pytest.raises(ValueError, match="propagate"):
            FrameStream(mv, 32, 48, **kw)
    fs = FrameStream(mv, 32, 48)
    assert fs.smooth is None and not fs.estimate and fs._smooth_last is None and fs._smooth_weight is None
    with pytest.raises(ValueError):
        fs.last_weight()
    fs = FrameStream(mv, 32, 48, smooth="flow")
    assert fs.smooth == ops.SMOOTH_DEFAULTS and fs.estimate and fs.flow_options == ops.FLOW_DEFAULTS
    assert fs._slots is None
    with pytest.raises(RuntimeError):
        fs.last_weight()
    fs = FrameStream(mi, 32, 48, trimap=False, static_bg=np.zeros((32, 48, 3), np.uint8), scale=2, gain="fit",
                     smooth="flow", smooth_options={"tol": 12}, flow="estimate", flow_options={"iters": 5})
    assert fs.smooth == {"strength": 0.5, "tol": 12.0, "jump": 0.3} and fs.flow_options["iters"] == 5
    both = FrameStream(mv, 32, 48, trimap="propagate", flow="given", smooth="flow")
    assert both.smooth == ops.SMOOTH_DEFAULTS and not both.estimate
    # the items are those of the stream without the filter
    z = lambda *s: np.zeros(s, np.uint8)  # noqa: E731
    assert fs.check_item((z(2, 32, 48, 3), None, None))[3] == 2
    with pytest.raises(ValueError):
        fs.check_item((z(2, 32, 48, 3), None, None, np.zeros((2, 32, 48, 2), F)))
