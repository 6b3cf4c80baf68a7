"""FrameStream(scale=...) on the GPU: the stream's results equal the eager chain (reduce -> FrameStream at the model's
size on the reduced frames -> ops.guided_upsample -> quantise | compose) byte for byte, in every trimap and out mode, and
scale=1 is the stream as it was."""

import numpy as np
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

H, W, CHUNK, DEPTH, FRAMES = 46, 70, 2, 2, 5  # a short last chunk
GROW = 1
NEW_BUFFERS = ("r_cmp", "r_bg", "r_tri", "alpha_lo", "ab")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def models(vgg0):
    from vmatting import unet
    np.random.seed(0)
    return {7: unet.UNetVideo(vgg0, dtype="bf16", device="cuda").prepare(),
            6: unet.UNetImage(vgg0, dtype="bf16", device="cuda").prepare()}


@pytest.fixture(scope="module")
def clip():
    """A subject (a textured block that drifts) over a smooth plate, so that the automatic trimaps have all three
    labels; per-frame backgrounds that differ slightly from the plate; painted trimaps; small smooth flows; new plates."""
    from oracle.flow import smooth_flow
    rs = np.random.RandomState(7)
    yy, xx = np.mgrid[0:H, 0:W]
    plate = np.stack([120 + 60 * np.sin(xx / 9.0 + c) + 40 * np.cos(yy / 7.0 + 2 * c) for c in range(3)], -1)
    plate = np.clip(np.rint(plate), 0, 255).astype(np.uint8)
    cmp = np.repeat(plate[None], FRAMES, 0).copy()
    tri = np.zeros((FRAMES, H, W), np.uint8)
    for j in range(FRAMES):
        y, x = 8 + j, 14 + 2 * j
        cmp[j, y:y + 26, x:x + 30] = rs.randint(0, 256, (26, 30, 3))
        tri[j, y - 3:y + 29, x - 3:x + 33] = 128
        tri[j, y + 3:y + 23, x + 3:x + 27] = 255
    bg = np.clip(plate[None].astype(np.int64) + rs.randint(-2, 3, (FRAMES, H, W, 3)), 0, 255).astype(np.uint8)
    flows = np.stack([smooth_flow(H, W, seed=j, amp=1.5) for j in range(FRAMES)]).astype(np.float32)
    new = rs.randint(0, 256, (FRAMES, H, W, 3)).astype(np.uint8)
    return {"cmp": cmp, "plate": plate, "bg": bg, "tri": tri, "flows": flows, "new": new}


def chunks():
    return [(i, min(i + CHUNK, FRAMES)) for i in range(0, FRAMES, CHUNK)]


def source(clip, static, trimap, new_per_frame=False):
    """The clip as FrameStream items for the trimap mode."""
    for a, b in chunks():
        bg = None if static else clip["bg"][a:b]
        if trimap == "propagate":
            item = (clip["cmp"][a:b], bg, clip["tri"][0] if a == 0 else None, clip["flows"][a:b])
        else:
            item = (clip["cmp"][a:b], bg, clip["tri"][a:b] if trimap is True else None)
        yield item + ((clip["new"][a:b],) if new_per_frame else ())


def full_trimaps(clip, static, trimap):
    """The full-resolution trimaps the stream makes or is given, as the eager ops make them -> uint8 [F,H,W] | None."""
    from vmatting import ops
    if trimap is True:
        return clip["tri"]
    if trimap is False:
        return None
    if trimap == "auto":
        bg = dev(clip["plate"]) if static else dev(clip["bg"])
        return ops.trimap_from_plate(dev(clip["cmp"]), bg, **ops.PLATE_DEFAULTS).cpu().numpy()
    tris = [dev(clip["tri"][0])]
    for j in range(1, FRAMES):
        tris.append(ops.trimap_propagate(tris[-1], dev(clip["flows"][j]), GROW))
    return torch.stack(tris).cpu().numpy()


_ALPHA = {}


def eager_alpha(models, clip, s, static, trimap, options=None):
    """reduce -> FrameStream at hm x wm with out="f32" on the reduced frames -> guided_upsample: f32 [F,H,W,1] on the
    device, computed once per configuration."""
    from vmatting import FrameStream, ops
    key = (s, static, trimap, None if options is None else tuple(sorted(options.items())))
    if key not in _ALPHA:
        tri = full_trimaps(clip, static, trimap)
        cmp_lo = ops.frames_reduce_u8(dev(clip["cmp"]), s).cpu().numpy()
        bg_lo = ops.frames_reduce_u8(dev(clip["plate"][None] if static else clip["bg"]), s).cpu().numpy()
        tri_lo = None if tri is None else ops.frames_reduce_u8(dev(tri), s, "trimap").cpu().numpy()
        hm, wm = cmp_lo.shape[1:3]
        assert (hm, wm) == (-(-H // s), -(-W // s))
        model = models[7 if trimap else 6]
        fs = FrameStream(model, hm, wm, chunk=CHUNK, depth=DEPTH, trimap=tri is not None, out="f32", graph=False,
                         static_bg=bg_lo[0] if static else None)
        items = [(cmp_lo[a:b], None if static else bg_lo[a:b], None if tri_lo is None else tri_lo[a:b])
                 for a, b in chunks()]
        lo = np.concatenate(list(fs.run(items)))
        assert lo.shape == (FRAMES, hm, wm) and lo.dtype == np.float32 and fs.overflowed_chunks == []
        _ALPHA[key] = ops.guided_upsample(dev(lo), dev(clip["cmp"]), s, **(options or {}))
        if trimap is True:  # the reduced trimaps keep hard labels only where the whole block has them
            assert all((tri_lo == v).any() for v in (0, 128, 255))
    return _ALPHA[key]


def stream(models, clip, s, static, trimap, out, graph, **kw):
    from vmatting import FrameStream
    fs = FrameStream(models[7 if trimap else 6], H, W, chunk=CHUNK, depth=DEPTH, trimap=trimap, out=out, graph=graph,
                     static_bg=clip["plate"] if static else None, scale=s, **kw)
    per_frame = kw.get("new_bg") == "per_frame"
    got = list(fs.run(source(clip, static, trimap, per_frame)))
    assert [g.shape[0] for g in got] == [b - a for a, b in chunks()]
    assert fs.overflowed_chunks == []
    return np.concatenate(got), fs


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("out", ["u8", "f32"])
@pytest.mark.parametrize("s,static", [(2, False), (3, True)], ids=["s2-bg-per-frame", "s3-static-plate"])
def test_stream_equals_the_eager_chain(models, clip, s, static, out, graph):
    from vmatting import ops
    alpha = eager_alpha(models, clip, s, static, True)
    want = (alpha[..., 0] if out == "f32" else ops.matte_quantize(alpha[..., 0].contiguous())).cpu().numpy()
    got, fs = stream(models, clip, s, static, True, out, graph)
    assert got.shape == (FRAMES, H, W) and got.dtype == want.dtype
    assert np.array_equal(got.view(np.uint32) if out == "f32" else got, want.view(np.uint32) if out == "f32" else want)
    slot = fs._slots[0]
    assert tuple(slot.alpha.shape) == (CHUNK, H, W, 1) and tuple(slot.alpha_lo.shape) == (CHUNK, fs.hm, fs.wm, 1)
    assert tuple(slot.frames.shape[:3]) == (CHUNK, fs.hm, fs.wm) and (slot.r_bg is None) == static
    if out == "u8" and graph:  # the object runs again, over the same graphs
        again = np.concatenate(list(fs.run(source(clip, static, True))))
        assert np.array_equal(again, want)


@pytest.mark.parametrize("s,static,trimap,graph", [(2, True, False, True), (3, False, False, False), (3, True, "auto", True),
                                                   (2, False, "auto", False), (2, False, "propagate", True),
                                                   (2, True, "propagate", False)])
def test_stream_trimap_modes(models, clip, s, static, trimap, graph):
    from vmatting import ops
    alpha = eager_alpha(models, clip, s, static, trimap)
    want = ops.matte_quantize(alpha[..., 0].contiguous()).cpu().numpy()
    kw = dict(flow="given", grow=GROW) if trimap == "propagate" else {}
    got, fs = stream(models, clip, s, static, trimap, "u8", graph, **kw)
    assert np.array_equal(got, want)
    assert (fs._slots[0].r_tri is None) == (trimap is False)


def test_stream_guided_options_reach_the_kernels(models, clip):
    options = {"r": 4, "eps": 0.05}
    alpha = eager_alpha(models, clip, 2, True, True, options)
    got, _ = stream(models, clip, 2, True, True, "f32", True, guided_options=options)
    assert np.array_equal(got.view(np.uint32), alpha[..., 0].cpu().numpy().view(np.uint32))
    assert not torch.equal(alpha, eager_alpha(models, clip, 2, True, True))


def test_stream_composes_at_full_resolution(models, clip):
    from vmatting import ops
    cmp, plate, bg, new = (dev(clip[k]) for k in ("cmp", "plate", "bg", "new"))
    alpha = eager_alpha(models, clip, 2, False, True)
    want = ops.matte_compose(alpha, cmp, bg, new, mode="over").cpu().numpy()
    got, _ = stream(models, clip, 2, False, True, "over", True, new_bg="per_frame")
    assert got.shape == (FRAMES, H, W, 3) and np.array_equal(got, want)
    alpha = eager_alpha(models, clip, 3, True, True)
    want = ops.matte_compose(alpha, cmp, plate, mode="bgra").cpu().numpy()
    got, _ = stream(models, clip, 3, True, True, "bgra", False)
    assert got.shape == (FRAMES, H, W, 4) and np.array_equal(got, want)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_scale_one_is_the_stream_as_it_was(models, clip, graph):
    from vmatting import FrameStream
    res = []
    for kw in ({}, {"scale": 1}):
        fs = FrameStream(models[7], H, W, chunk=CHUNK, depth=DEPTH, out="u16", graph=graph, **kw)
        res.append(np.concatenate(list(fs.run(source(clip, False, True)))))
        assert fs.scale == 1 and fs._plate_lo is None and fs._guided_work is None
        for s in fs._slots:
            assert not any(hasattr(s, name) for name in NEW_BUFFERS)
            assert tuple(s.frames.shape[:3]) == (CHUNK, H, W)
    assert np.array_equal(res[0], res[1])
