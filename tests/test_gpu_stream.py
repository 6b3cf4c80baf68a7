"""vmatting.stream.FrameStream on the GPU: uint8 chunks from a host source through upload / ingest / forward / quantise /
download slots, against ``model.forward`` of the numpy-built frames, frame by frame and bit for bit."""

import numpy as np
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

VGG_MEAN = np.array([103.939, 116.779, 123.68], np.float64)
H, W, F, CHUNK = 24, 40, 19, 8  # spans of 8, 8 and 3: slot 0's graph is reused, the last chunk is short (eager)


def feed(cmp, bg, tri):
    return np.concatenate([(cmp.astype(np.float64) - VGG_MEAN).astype(np.float32),
                           (bg.astype(np.float64) - VGG_MEAN).astype(np.float32),
                           (tri.astype(np.float64) / 255.0 - 0.5).astype(np.float32)[..., None]], -1)


def quantize_ref(a, m):
    return np.clip(np.rint(a.astype(np.float32) * np.float32(m)), 0, m).astype(np.uint8 if m == 255 else np.uint16)


def reusing_source(cmp, bg, tri, chunk, static=False):
    """Yields the clip in chunks out of ONE set of arrays that it overwrites after every yield (a decoder's ring)."""
    n = cmp.shape[0]
    bc, bb, bt = np.empty_like(cmp[:chunk]), np.empty_like(cmp[:chunk]), np.empty_like(tri[:chunk])
    for a in range(0, n, chunk):
        k = min(chunk, n - a)
        bc[:k], bt[:k] = cmp[a:a + k], tri[a:a + k]
        if not static:
            bb[:k] = bg[a:a + k]
        yield bc[:k], (None if static else bb[:k]), bt[:k]
        bc[...], bb[...], bt[...] = 0xA5, 0x5A, 0x33


@pytest.fixture(scope="module")
def clip_and_reference(vgg0):
    """19 distinct frames, the bf16 model, and model.forward of every numpy-built frame on its own (computed once)."""
    from vmatting import unet
    rs = np.random.RandomState(42)
    cmp = rs.randint(0, 256, (F, H, W, 3)).astype(np.uint8)
    bg = rs.randint(0, 256, (F, H, W, 3)).astype(np.uint8)
    tri = rs.choice(np.array([0, 128, 255], np.uint8), (F, H, W))
    assert len({cmp[i].tobytes() for i in range(F)}) == F
    np.random.seed(0)
    model = unet.UNetVideo(vgg0, dtype="bf16", device="cuda").prepare()

    def reference(bgs):
        x = feed(cmp, bgs, tri)
        return np.stack([model.forward(torch.from_numpy(x[i:i + 1]).cuda())[0, :, :, 0].cpu().numpy() for i in range(F)])
    alpha = reference(bg)
    assert len({alpha[i].tobytes() for i in range(F)}) == F  # distinct mattes: a swapped or stale frame would show
    alpha_plate = reference(np.broadcast_to(bg[3], bg.shape))
    return model, cmp, bg, tri, alpha, alpha_plate


@pytest.mark.parametrize("out", ["f32", "u8", "u16"])
def test_stream_equals_forward_frame_by_frame(clip_and_reference, out):
    from vmatting import FrameStream
    model, cmp, bg, tri, alpha, _ = clip_and_reference
    want = {"f32": alpha, "u8": quantize_ref(alpha, 255), "u16": quantize_ref(alpha, 65535)}[out]
    fs = FrameStream(model, H, W, chunk=CHUNK, depth=2, out=out)
    for _ in range(2):  # the call repeats with the same result (the slots' graphs are reused)
        got = list(fs.run(reusing_source(cmp, bg, tri, CHUNK)))
        assert [g.shape for g in got] == [(8, H, W), (8, H, W), (3, H, W)]
        assert all(g.dtype == want.dtype for g in got)
        got = np.concatenate(got)
        for i in range(F):  # in order, frame by frame
            assert np.array_equal(got[i], want[i]), "frame %d" % i
    assert fs.overflowed_chunks == []
    assert sum(s.graph is not None for s in fs._slots) == 2


@pytest.mark.parametrize("depth,graph", [(1, True), (3, True), (2, False)])
def test_stream_depths_and_eager_give_the_same_mattes(clip_and_reference, depth, graph):
    from vmatting import FrameStream
    model, cmp, bg, tri, alpha, _ = clip_and_reference
    fs = FrameStream(model, H, W, chunk=CHUNK, depth=depth, out="u16", graph=graph)
    got = np.concatenate(list(fs.run(reusing_source(cmp, bg, tri, CHUNK))))
    assert np.array_equal(got, quantize_ref(alpha, 65535))


def test_stream_lag_is_depth_minus_one(clip_and_reference):
    """Chunk i is yielded once chunk i + depth - 1 has been taken from the source (and the rest at its end)."""
    from vmatting import FrameStream
    model, cmp, bg, tri, _, _ = clip_and_reference
    taken = []

    def source():
        for i, item in enumerate(reusing_source(cmp, bg, tri, 4)):
            taken.append(i)
            yield item
    for depth in (1, 2, 3):
        del taken[:]
        seen = [len(taken) for _ in FrameStream(model, H, W, chunk=4, depth=depth, graph=False).run(source())]
        assert seen == [min(i + depth, 5) for i in range(5)], (depth, seen)


def test_stream_static_plate_equals_per_frame_plate(clip_and_reference):
    from vmatting import FrameStream
    model, cmp, bg, tri, _, alpha_plate = clip_and_reference
    want = quantize_ref(alpha_plate, 255)
    per_frame = np.broadcast_to(bg[3], bg.shape)
    a = np.concatenate(list(FrameStream(model, H, W, chunk=CHUNK).run(reusing_source(cmp, per_frame, tri, CHUNK))))
    fs = FrameStream(model, H, W, chunk=CHUNK, static_bg=bg[3])
    b = np.concatenate(list(fs.run(reusing_source(cmp, None, tri, CHUNK, static=True))))
    assert np.array_equal(a, want) and np.array_equal(b, want)


def test_stream_failing_source(clip_and_reference):
    """A source that raises on its third item: the two chunks it did produce are delivered, in order, then the
    exception propagates; a bad item behaves the same; the object runs again afterwards."""
    from vmatting import FrameStream
    model, cmp, bg, tri, alpha, _ = clip_and_reference
    want = quantize_ref(alpha, 255)
    fs = FrameStream(model, H, W, chunk=CHUNK, depth=2)

    def failing(bad_item):
        for i, item in enumerate(reusing_source(cmp, bg, tri, CHUNK)):
            if i == 2:
                if bad_item:
                    yield item[0].astype(np.float32), item[1], item[2]
                raise OSError("decoder lost the file")
            yield item
    for bad_item, exc in ((False, OSError), (True, TypeError)):
        got = []
        with pytest.raises(exc):
            for m in fs.run(failing(bad_item)):
                got.append(m)
        assert len(got) == 2
        assert np.array_equal(np.concatenate(got), want[:16])
    again = np.concatenate(list(fs.run(reusing_source(cmp, bg, tri, CHUNK))))
    assert np.array_equal(again, want)


# ---------------------------------------------------------------------------------------------- f16x3 overflow
# The overflow fixture's recipe of tests/test_gpu_video.py, restated for uint8 input.  A uint8 frame cannot exceed
# +-152 after the mean subtraction, and with the vgg0 weights such frames peak near 1.3e3, far inside fp16's range, so
# no uint8 frame overflows on its own.  The recipe therefore scales conv1_1's filter by 300 (activations scale with it)
# and uses frames of two kinds: cool ones within 3 counts of the mean (|input| <= 4: peak ~1e4, below 65520 / 4) and
# hot ones over the whole byte range (peak ~3.8e5, above 2 * 65520).

SPLIT_LAYERS = ("conv1_1", "conv1_2", "pool1", "conv2_1", "conv2_2", "pool2", "conv3_1", "conv3_2", "conv3_3", "pool3",
                "conv4_1", "conv4_2", "conv4_3", "pool4", "conv5_1", "upconv1", "upconv2", "upconv3", "upconv4")
SCALE = 300.0


def test_stream_f16x3_middle_chunk_overflow(vgg0):
    from oracle import models as om
    from vmatting import FrameStream, unet
    rs = np.random.RandomState(7)
    near = np.array([104, 117, 124])
    n, chunk = 5, 2  # chunks (0, 1), (2, 3), (4): the middle one holds the hot frame
    cmp = (near + rs.randint(-3, 4, (n, H, W, 3))).astype(np.uint8)
    bg = (near + rs.randint(-3, 4, (n, H, W, 3))).astype(np.uint8)
    tri = rs.choice(np.array([0, 128, 255], np.uint8), (n, H, W))
    cmp[3] = rs.randint(0, 256, (H, W, 3))
    bg[3] = rs.randint(0, 256, (H, W, 3))
    frames = feed(cmp, bg, tri)
    np.random.seed(0)
    model = unet.UNetVideo(vgg0, dtype="f16x3", device="cuda")
    model.params = model._make_params()
    w11, b11 = model.params["conv1_1"]
    model.load_params(dict(model.params, conv1_1=(w11 * np.float32(SCALE), b11))).prepare()
    # precondition, by the float64 oracle: only frame 3 leaves fp16's range, and clearly
    peak = [max(np.abs(v).max() for k, v in om.unet_forward(frames[i:i + 1], model.params, dtype=np.float64).items()
                if k in SPLIT_LAYERS) for i in range(n)]
    assert peak[3] >= 2 * 65520 and all(peak[i] <= 65520 / 4 for i in range(n) if i != 3), peak
    alone = {}
    for i in (0, 1, 4):
        alone[i] = model.forward(torch.from_numpy(frames[i:i + 1]).cuda())[0, :, :, 0].cpu().numpy()
        assert not model.overflowed()
    for graph in (True, False):
        fs = FrameStream(model, H, W, chunk=chunk, depth=2, out="f32", graph=graph)
        got = np.concatenate(list(fs.run(reusing_source(cmp, bg, tri, chunk))))
        assert fs.overflowed_chunks == [1], graph
        assert model.split_mode == "f16x3"
        assert np.isfinite(got).all()
        for i in (0, 1, 4):
            assert np.array_equal(got[i], alone[i]), "frame %d differs from its standalone f16x3 forward" % i
        # the re-run chunk is the bf16x6 forward of the same frames
        x6 = fs._x6.forward(torch.from_numpy(frames[2:4]).cuda())[:, :, :, 0].cpu().numpy()
        assert np.array_equal(got[2:4], x6)
        # a second run over the same slots: the flag does not stick to the slot
        cool = np.concatenate(list(fs.run(reusing_source(cmp[[0, 1, 4]], bg[[0, 1, 4]], tri[[0, 1, 4]], chunk))))
        assert fs.overflowed_chunks == []
        for j, i in enumerate((0, 1, 4)):
            assert np.array_equal(cool[j], alone[i])
