"""FrameStream(trimap="auto", shadow="chroma") on the GPU: its mattes equal those of FrameStream(trimap=True) fed the
numpy restatement's shadow-tolerant trimaps (tests/plate_shadow_ref.py), bit for bit, with the graph on and off, and in
one combination each with auto_fill, gain="fit" and scale=2 against the reference chains of those options' own tests."""

import numpy as np
import pytest
import torch

import plate_gain_ref as gain_ref
import plate_shadow_ref as ref
import trimap_fill_ref as fill_ref
import trimap_plate_ref as plain
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

H, W, F, CHUNK = 70, 90, 7, 3    # items of 3, 3 and 1 frames: two full chunks and a short, eager one
AUTO = {"lo": 12, "hi": 40, "r_bg": 2, "r_fg": 3}
SHADOW = {"floor": 140, "ceil": 256, "dark": 90}   # (the darker part of the plate gets no tolerance: not the defaults)
FRAME_GAINS = (0.8, 1.2, 1.0, 0.9, 1.1, 0.85, 1.15)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def items(cmp, bg, tris=None):
    for a in range(0, len(cmp), CHUNK):
        b = min(a + CHUNK, len(cmp))
        yield (cmp[a:b], None if bg is None else bg[a:b], None if tris is None else tris[a:b])


def shadowed_pair(seed):
    """trimap_plate_ref.blob_pair's plate (within 20..130: no gain clips it) and disc, with a soft shadow keeping 0.7 of
    the light over the lower right of the frame only -> (frame u8, plate u8)."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[:H, :W].astype(np.float64)
    plate = np.stack([60 + 40 * np.sin(x / 9), 90 + 30 * np.cos(y / 7), 120 + 0 * x], -1)
    fg = np.stack([200 + 20 * np.sin(y / 5), 40 + 20 * np.cos(x / 6), 30 + 0 * x], -1)
    a = np.clip((14 - np.hypot(x - 30 - seed % 5, y - 28)) / 4 + 0.5, 0, 1)[..., None]
    light = 1 - 0.3 * np.clip((1 - np.hypot((x - 62) / 24, (y - 50) / 14)) * 6 + 0.5, 0, 1)[..., None]
    u8 = lambda v: np.clip(np.rint(v + rs.normal(0, 2, v.shape)), 0, 255).astype(np.uint8)  # noqa: E731
    return u8(a * fg + (1 - a) * plate * light), u8(plate)


@pytest.fixture(scope="module")
def clip(vgg0):
    """7 shadowed frames over per-frame plates, a bf16 model whose mattes depend on the trimap, and the restatement's
    trimaps, with the shadow test and without, over the per-frame plates and over plate 0 alone."""
    from vmatting import unet
    pairs = [shadowed_pair(30 + t) for t in range(F)]
    cmp, bg = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    np.random.seed(0)
    params = dict(unet.UNetVideo(vgg0, dtype="bf16", device="cuda").prepare().params)
    # a fresh UNetVideo's conv1_1 is [VGG, VGG, 0]: its mattes do not depend on the trimap.  As test_gpu_trimap_fill
    # does, stand in for a trained one with weights on the trimap channel that weigh -0.5 .. 0.5 like a colour
    w, b = params["conv1_1"]
    w = w.copy()
    w[:, :, 6, :] = np.random.RandomState(5).normal(0, 20.0, w[:, :, 6, :].shape)
    params["conv1_1"] = (w, b)
    model = unet.UNetVideo(vgg0, dtype="bf16", device="cuda").load_params(params).prepare()
    tris = {(k, s is not None): ref.trimaps(cmp, p, shadow=s, **AUTO)
            for k, p in (("frames", bg), ("static", bg[0])) for s in (SHADOW, None)}
    for k in ("frames", "static"):
        assert np.array_equal(tris[k, False], plain.trimaps(cmp, bg if k == "frames" else bg[0], **AUTO))
        for i in range(F):
            assert set(np.unique(tris[k, True][i]).tolist()) == {0, 128, 255}
            assert ((tris[k, True][i] == 0) & (tris[k, False][i] != 0)).sum() > 300    # the shadow, held
    return model, cmp, bg, tris


def run(model, cmp, bg, static, tris=None, h=H, w=W, **kw):
    """The clip through a FrameStream: ``bg`` per frame, or with ``static`` the one plate."""
    from vmatting import FrameStream
    kw.setdefault("out", "u16")
    fs = FrameStream(model, h, w, chunk=CHUNK, static_bg=bg if static else None, **kw)
    got = list(fs.run(items(cmp, None if static else bg, tris)))
    assert [g.shape[0] for g in got] == [3, 3, 1] and fs.overflowed_chunks == []
    return fs, np.concatenate(got)


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("plate", ["frames", "static"])
def test_stream_shadow_equals_per_frame_trimaps(clip, plate, graph):
    model, cmp, bg, tris = clip
    static = plate == "static"
    feed = bg[0] if static else bg
    _, want = run(model, cmp, feed, static, tris[plate, True])
    _, unshadowed = run(model, cmp, feed, static, tris[plate, False])
    assert not np.array_equal(want, unshadowed)                                        # it reaches the mattes
    fs, got = run(model, cmp, feed, static, trimap="auto", auto_options=AUTO, shadow="chroma", shadow_options=SHADOW,
                  graph=graph)
    assert fs.shadow == SHADOW and got.shape == (F, H, W) and np.array_equal(got, want)
    assert np.array_equal(np.concatenate(list(fs.run(items(cmp, None if static else bg)))), want)   # it runs again
    assert all((s.graph is not None) == graph for s in fs._slots)
    # and without the option the stream is what it was
    _, got = run(model, cmp, feed, static, trimap="auto", auto_options=AUTO, graph=graph)
    assert np.array_equal(got, unshadowed)
    # what the stream fed the model is what reader.trimap_from_plate shows
    from vmatting import reader
    assert np.array_equal(reader.trimap_from_plate(cmp, feed, shadow="chroma", shadow_options=SHADOW, **AUTO),
                          tris[plate, True])


def test_stream_shadow_defaults(clip):
    """shadow_options reach the kernel: the defaults give other trimaps on these frames, and the stream follows them."""
    model, cmp, bg, tris = clip
    tri = ref.trimaps(cmp, bg, shadow=ref.DEFAULTS, **AUTO)
    assert not np.array_equal(tri, tris["frames", True])
    _, want = run(model, cmp, bg, False, tri)
    _, got = run(model, cmp, bg, False, trimap="auto", auto_options=AUTO, shadow="chroma")
    assert np.array_equal(got, want)


def test_stream_shadow_with_auto_fill(clip):
    """The fill works on the shadow-tolerant trimap.  A plate-coloured patch inside the disc is the hole."""
    model, cmp, bg, _ = clip
    cmp = cmp.copy()
    cmp[:, 22:34, 26:38] = bg[:, 22:34, 26:38]
    tri = ref.trimaps(cmp, bg, shadow=SHADOW, **AUTO)
    filled = fill_ref.fills(tri)
    assert all((filled[i] != tri[i]).sum() > 20 for i in range(F))
    _, want = run(model, cmp, bg, False, filled)
    _, unfilled = run(model, cmp, bg, False, tri)
    assert not np.array_equal(want, unfilled)
    _, got = run(model, cmp, bg, False, trimap="auto", auto_options=AUTO, auto_fill=True, shadow="chroma",
                 shadow_options=SHADOW)
    assert np.array_equal(got, want)


def test_stream_shadow_with_gain(clip):
    """The shadow test sees the gained plate: frames under gains of their own against one static plate, out="over"."""
    model, cmp, bg, _ = clip
    cmp = np.clip(np.rint(cmp * np.array(FRAME_GAINS)[:, None, None, None]), 0, 255).astype(np.uint8)
    new = np.random.RandomState(3).randint(0, 256, (H, W, 3)).astype(np.uint8)
    G, S = gain_ref.fits(cmp, bg[0])
    assert (S * 16 >= H * W).all() and (np.abs(G / 4096 / np.array(FRAME_GAINS)[:, None] - 1) <= 0.05).all()
    gained = gain_ref.applies(bg[0], G)
    tri = ref.trimaps(cmp, gained, shadow=SHADOW, **AUTO)
    assert not np.array_equal(tri, ref.trimaps(cmp, bg[0], shadow=SHADOW, **AUTO))
    assert not np.array_equal(tri, plain.trimaps(cmp, gained, **AUTO))
    _, want = run(model, cmp, gained, False, tri, out="over", new_bg=new)
    fs, got = run(model, cmp, bg[0], True, trimap="auto", auto_options=AUTO, gain="fit", shadow="chroma",
                  shadow_options=SHADOW, out="over", new_bg=new)
    assert got.shape == (F, H, W, 3) and np.array_equal(got, want)
    assert np.array_equal(fs.last_gains()[0], G[-1:].astype(np.float32) / np.float32(4096))


def test_stream_shadow_with_scale(clip):
    """scale=2: the trimap is made at full resolution, shadow test included, then reduced; the chain of
    test_gpu_stream_scale (reduce -> the stream at the model's size, out="f32" -> guided_upsample -> quantise)."""
    from vmatting import ops
    model, cmp, bg, tris = clip
    s = 2
    cmp_lo = ops.frames_reduce_u8(dev(cmp), s).cpu().numpy()
    bg_lo = ops.frames_reduce_u8(dev(bg), s).cpu().numpy()
    want = {}
    for shadow in (True, False):
        tri_lo = ops.frames_reduce_u8(dev(tris["frames", shadow]), s, "trimap").cpu().numpy()
        hm, wm = cmp_lo.shape[1:3]
        assert (hm, wm) == (-(-H // s), -(-W // s))
        _, lo = run(model, cmp_lo, bg_lo, False, tri_lo, h=hm, w=wm, out="f32", graph=False)
        alpha = ops.guided_upsample(dev(lo), dev(cmp), s)
        want[shadow] = ops.matte_quantize(alpha[..., 0].contiguous()).cpu().numpy()
    assert not np.array_equal(want[True], want[False])
    _, got = run(model, cmp, bg, False, trimap="auto", auto_options=AUTO, shadow="chroma", shadow_options=SHADOW, scale=s,
                 out="u8")
    assert got.shape == (F, H, W) and np.array_equal(got, want[True])
