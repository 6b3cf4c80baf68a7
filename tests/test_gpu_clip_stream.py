"""vmatting.clip.ClipStream on the GPU: the video model's recurrence over a clip,

    alpha[t] = UNetSimple(cmp[t], bg[t], warp_img(alpha[t-1], backward[t]) [corrected by correct_alpha]),

against the same recurrence stepped with calls that existed before it (flow.warp_img, flow.correct_alpha,
UNetSimple.forward on numpy-built frames), frame by frame and bit for bit on the f32 alpha, and against the float64
oracle one step at a time."""

import numpy as np
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

VGG_MEAN = np.array([103.939, 116.779, 123.68], np.float64)
H, W, F = 24, 40, 5
THRESH = 6.0  # the default 15 zeroes nothing at this size (tests/test_gpu_clip_feed.py)
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731


def feed(u8):
    return (u8.astype(np.float64) - VGG_MEAN).astype(np.float32)


def quantize_ref(a, m):
    return np.clip(np.rint(a.astype(np.float32) * np.float32(m)), 0, m).astype(np.uint8 if m == 255 else np.uint16)


class Clip:
    def __init__(self):
        from oracle import flow as oflow
        from oracle import models as om
        rs = np.random.RandomState(42)
        self.cmp = rs.randint(0, 256, (F, H, W, 3)).astype(np.uint8)
        self.bg = rs.randint(0, 256, (F, H, W, 3)).astype(np.uint8)
        assert len({self.cmp[i].tobytes() for i in range(F)}) == F and len({self.bg[i].tobytes() for i in range(F)}) == F
        self.bw = np.stack([oflow.smooth_flow(H, W, seed=100 + t, amp=6.0) for t in range(F)])
        self.fw = np.stack([oflow.smooth_flow(H, W, seed=200 + t, amp=6.0) for t in range(F)])
        self.alpha0 = rs.uniform(0.0, 1.0, (H, W)).astype(np.float32)
        # the oracle's draws, the output conv scaled by 2^-6 (exact): unscaled, the logits' std is ~36, the sigmoid
        # saturates and the matte barely shows its third input
        p = om.unet_simple_params(np.random.RandomState(1))
        w, b = p["output"]
        p["output"] = (w * np.float32(2.0 ** -6), b * np.float32(2.0 ** -6))
        self.params = p
        self.bn = {"conv4": (rs.uniform(0.5, 1.5, 48).astype(np.float32), rs.normal(size=48).astype(np.float32) * 0.1),
                   "upconv2": (rs.uniform(0.5, 1.5, 32).astype(np.float32), rs.normal(size=32).astype(np.float32) * 0.1)}
        self.models, self._ref = {}, {}

    def model(self, dtype, vgg0):
        from vmatting import unet_simple
        if dtype not in self.models:
            np.random.seed(0)
            m = unet_simple.UNetSimple(unet_simple.Vgg16(vgg0, dtype), False, dtype)
            self.models[dtype] = m.load_params(self.params, self.bn)
        return self.models[dtype]

    def source(self, plate=False, occlusion=False, frames=F):
        """One set of arrays, overwritten after every yield (a decoder's ring)."""
        c, b, bw, fw = (np.empty_like(a[0]) for a in (self.cmp, self.bg, self.bw, self.fw))
        for t in range(frames):
            c[...], b[...], bw[...], fw[...] = self.cmp[t], self.bg[t], self.bw[t], self.fw[t]
            yield c, (None if plate else b), bw, (fw if occlusion else None)
            c[...], b[...], bw[...], fw[...] = 0xA5, 0x5A, 1e3, -1e3

    def stepwise(self, dtype, vgg0, plate=False, occlusion=False, alpha0=None, bw=None):
        """[F,H,W] f32: the recurrence from calls that exist without ClipStream (computed once per configuration)."""
        from vmatting import flow
        key = (dtype, plate, occlusion) if alpha0 is None and bw is None else None
        if key in self._ref:
            return self._ref[key]
        m = self.model(dtype, vgg0)
        prev = T(self.alpha0 if alpha0 is None else alpha0)[None]
        bws = self.bw if bw is None else bw
        out = []
        for t in range(F):
            warped = flow.warp_img(prev, T(bws[t])[None])
            if occlusion:
                flow.correct_alpha(T(bws[t]), T(self.fw[t]), warped[0], thresh=THRESH)
            bg = self.bg[2] if plate else self.bg[t]
            a = m.forward(T(feed(self.cmp[t]))[None], T(feed(bg))[None], warped[..., None].repeat(1, 1, 1, 3))
            prev = a[:, :, :, 0].clone()
            out.append(prev[0].cpu().numpy())
        out = np.stack(out)
        if key is not None:
            self._ref[key] = out
        return out


@pytest.fixture(scope="module")
def clip():
    return Clip()


def stream(clip, vgg0, dtype, plate=False, occlusion=False, **kw):
    from vmatting import ClipStream
    kw.setdefault("out", "f32")
    return ClipStream(clip.model(dtype, vgg0), H, W, static_bg=clip.bg[2] if plate else None, occlusion=occlusion,
                      thresh=THRESH, **kw)


def run(cs, clip, alpha0=None, frames=F):
    plate, occ = cs.static_bg is not None, cs.occlusion
    return np.stack(list(cs.run(clip.source(plate, occ, frames), clip.alpha0 if alpha0 is None else alpha0)))


def test_reference_recurrence_shows_its_third_input(clip, vgg0):
    """Preconditions on the step-wise route: the matte depends on the previous matte (swapping alpha0 for 1 - alpha0
    moves most of frame 0) and on the occlusion mask (every frame moves), and the frames differ from each other, so a
    feed that ignored the third tower, a stale matte or a swapped frame could not pass the checks below."""
    for dtype in ("bf16", "fp32"):
        a = clip.stepwise(dtype, vgg0)
        assert (a > 0.01).all() and (a < 0.99).all()  # no saturated sigmoid (the float64 oracle: 0.034 .. 0.74)
        assert len({a[i].tobytes() for i in range(F)}) == F
        swapped = clip.stepwise(dtype, vgg0, alpha0=(1 - clip.alpha0).astype(np.float32))
        assert (np.abs(swapped[0] - a[0]) > 1e-5).mean() > 0.5
        occ = clip.stepwise(dtype, vgg0, occlusion=True)
        for t in range(F):
            assert (np.abs(occ[t] - a[t]) > 1e-5).mean() > 0.5, t
        assert not np.array_equal(clip.stepwise(dtype, vgg0, plate=True)[0], a[0])  # the plate is not frame 0's bg


@pytest.mark.parametrize("occlusion", [False, True], ids=["warp", "occ"])
@pytest.mark.parametrize("bgmode", ["per-frame", "plate-reuse", "plate-full"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_clip_stream_equals_stepwise_recurrence(clip, vgg0, dtype, bgmode, occlusion):
    plate = bgmode != "per-frame"
    want = clip.stepwise(dtype, vgg0, plate, occlusion)
    cs = stream(clip, vgg0, dtype, plate, occlusion, reuse_bg_tower=bgmode == "plate-reuse")
    graphs = None
    for _ in range(2):  # a second run on the same object: the same mattes from the same graphs
        got = run(cs, clip)
        assert got.dtype == np.float32 and got.shape == (F, H, W)
        for t in range(F):
            assert np.array_equal(got[t], want[t]), "frame %d" % t
        assert cs.stats["bg_tower_evals"] == (1 if bgmode == "plate-reuse" else F) and cs.stats["frames"] == F
        ids = [id(g) for s in cs._slots for g in s.graphs.values()]
        assert graphs is None or ids == graphs
        graphs = ids
    assert len(graphs) == (3 if bgmode == "plate-reuse" else 2)


@pytest.mark.parametrize("depth,graph", [(1, True), (3, True), (2, False), (1, False)])
@pytest.mark.parametrize("bgmode", ["per-frame", "plate-reuse"])
def test_clip_stream_depths_and_eager_give_the_same_mattes(clip, vgg0, bgmode, depth, graph):
    plate = bgmode != "per-frame"
    want = clip.stepwise("bf16", vgg0, plate, True)
    cs = stream(clip, vgg0, "bf16", plate, True, depth=depth, graph=graph)
    got = run(cs, clip)
    assert np.array_equal(got, want)
    assert cs.stats["bg_tower_evals"] == (1 if plate else F)
    assert all(bool(s.graphs) == graph for s in cs._slots)


def test_clip_stream_lag_is_depth_minus_one(clip, vgg0):
    taken = []

    def source():
        for t, item in enumerate(clip.source()):
            taken.append(t)
            yield item
    for depth in (1, 2, 3):
        del taken[:]
        cs = stream(clip, vgg0, "bf16", depth=depth, graph=False)
        seen = [len(taken) for _ in cs.run(source(), clip.alpha0)]
        assert seen == [min(i + depth, F) for i in range(F)], (depth, seen)


@pytest.mark.parametrize("out", ["u8", "u16"])
def test_clip_stream_quantised_output(clip, vgg0, out):
    """The quantised mattes are quantize_ref of the f32 recurrence (the recurrence itself stays f32 on the device)."""
    m = 255 if out == "u8" else 65535
    want = clip.stepwise("bf16", vgg0, True, False)
    got = run(stream(clip, vgg0, "bf16", True, False, out=out), clip)
    assert got.dtype == (np.uint8 if out == "u8" else np.uint16)
    assert np.array_equal(got, quantize_ref(want, m))


def test_clip_stream_uint8_alpha0(clip, vgg0):
    u = np.rint(clip.alpha0 * 255).astype(np.uint8)
    f = (u.astype(np.float64) / 255.0).astype(np.float32)
    cs = stream(clip, vgg0, "bf16")
    a, b = run(cs, clip, alpha0=u), run(cs, clip, alpha0=f)
    assert np.array_equal(a, b)
    assert np.array_equal(b, clip.stepwise("bf16", vgg0, alpha0=f))
    assert not np.array_equal(b[0], clip.stepwise("bf16", vgg0)[0])


def test_clip_stream_matches_float64_oracle_teacher_forced(clip, vgg0):
    """fp32: each frame's matte is within 1e-4 (the bound of test_unet_simple_fp32_matches_reference_golden) of the
    float64 oracle evaluated on the stream's own previous matte warped by the oracle's warp_img."""
    from oracle import flow as oflow
    from oracle import models as om
    got = run(stream(clip, vgg0, "fp32"), clip)
    prev = clip.alpha0
    for t in range(F):
        warped = oflow.warp_img(prev, clip.bw[t])
        ref = om.unet_simple_forward(feed(clip.cmp[t])[None], feed(clip.bg[t])[None],
                                     np.repeat(warped[None, :, :, None], 3, -1), False, vgg0, clip.params, bn=clip.bn)
        err = np.abs(got[t] - ref["output"][0, :, :, 0]).max()
        print("frame %d: max |stream - oracle| = %.3g" % (t, err))
        assert err <= 1e-4, (t, err)
        prev = got[t]


def test_clip_stream_index_error_names_the_frame(clip, vgg0):
    """A frame whose backward flow trips the reference's IndexError: the earlier mattes are yielded, then IndexError
    names the frame; the object runs again afterwards."""
    want = clip.stepwise("bf16", vgg0, False, True)
    cs = stream(clip, vgg0, "bf16", False, True)
    bad = clip.bw.copy()
    bad[2, 3, 4, 1] = -40.0  # i0 = 3 - 40 < -H

    def source():
        for t, (c, b, bw, fw) in enumerate(clip.source(False, True)):
            if t == 2:
                bw[...] = bad[2]
            yield c, b, bw, fw
    got = []
    with pytest.raises(IndexError, match="frame 2"):
        for m in cs.run(source(), clip.alpha0):
            got.append(m)
    assert len(got) == 2 and np.array_equal(np.stack(got), want[:2])
    assert np.array_equal(run(cs, clip), want)


def test_clip_stream_failing_source(clip, vgg0):
    """A source that raises on its fourth item: the three frames it did produce are delivered, in order, then the
    exception propagates; a wrong-shape item behaves the same; the object runs again afterwards."""
    want = clip.stepwise("bf16", vgg0)
    cs = stream(clip, vgg0, "bf16")

    def failing(bad_item):
        for t, item in enumerate(clip.source()):
            if t == 3:
                if bad_item:
                    yield item[0][:, :W - 1], item[1], item[2], item[3]
                raise OSError("decoder lost the file")
            yield item
    for bad_item, exc in ((False, OSError), (True, ValueError)):
        got = []
        with pytest.raises(exc):
            for m in cs.run(failing(bad_item), clip.alpha0):
                got.append(m)
        assert len(got) == 3 and np.array_equal(np.stack(got), want[:3])
    assert np.array_equal(run(cs, clip), want)
    # abandoning the generator leaves nothing queued, and the next run starts clean
    g = cs.run(clip.source(), clip.alpha0)
    next(g)
    g.close()
    assert cs._compute.query() and cs._upload.query()
    assert np.array_equal(run(cs, clip), want)


def test_load_params_hands_trained_parameters_to_inference(clip, vgg0):
    """load_params takes what VideoTrainer.params_numpy() returns: after it the model's forward is the float64
    oracle's on those parameters (fp32, 1e-4), and before it it is not."""
    from oracle import models as om
    from vmatting import unet_simple
    np.random.seed(5)
    m = unet_simple.UNetSimple(unet_simple.Vgg16(vgg0, "fp32"), False, "fp32")
    c, b = feed(clip.cmp[:1]), feed(clip.bg[:1])
    d = np.repeat(clip.alpha0[None, :, :, None], 3, -1)
    ref = om.unet_simple_forward(c, b, d, False, vgg0, clip.params, bn=clip.bn)["output"]
    before = m.forward(c, b, d).cpu().numpy()
    assert np.abs(before - ref).max() > 1e-2
    assert m.load_params(clip.params, clip.bn) is m
    assert np.abs(m.forward(c, b, d).cpu().numpy() - ref).max() <= 1e-4
    with pytest.raises(ValueError):
        m.load_params({k: v for k, v in clip.params.items() if k != "conv2"})
    with pytest.raises(ValueError):
        m.load_params(clip.params, {"conv9": (np.ones(3), np.zeros(3))})
