"""csrc/ingest.hip on the GPU: uint8 frames -> network input and alpha -> quantised mattes, bit for bit against numpy,
and VideoMatter.from_uint8 against VideoMatter on the numpy-built f32 frames.

The reference values are the reference's inference feed restated in numpy (loader.py:45,75-78): the mean and the 0.5
are subtracted in float64 and the result becomes float32 once; bf16 is torch's round-to-nearest-even of that f32.
"""

import numpy as np
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

VGG_MEAN = np.array([103.939, 116.779, 123.68], np.float64)


def feed(cmp, bg, tri=None):
    """numpy reference: [n,h,w,7] (6 without a trimap) f32."""
    n = cmp.shape[0]
    bg = np.broadcast_to(bg.reshape((-1,) + cmp.shape[1:]), cmp.shape)
    parts = [(cmp.astype(np.float64) - VGG_MEAN).astype(np.float32), (bg.astype(np.float64) - VGG_MEAN).astype(np.float32)]
    if tri is not None:
        parts.append((tri.astype(np.float64) / 255.0 - 0.5).astype(np.float32)[..., None])
    out = np.concatenate(parts, -1)
    assert out.shape[0] == n
    return out


def clip(n, h, w, seed=0):
    """Random uint8 frames whose every channel holds all 256 byte values when the frame has room for them."""
    rs = np.random.RandomState(seed)
    cmp = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    bg = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    tri = rs.randint(0, 256, (n, h, w)).astype(np.uint8)
    if n * h * w >= 256:
        ramp = np.arange(256, dtype=np.uint8)
        for c in range(3):
            cmp.reshape(-1, 3)[c:c + 256, c] = ramp
            bg.reshape(-1, 3)[7 + c:7 + c + 256, c] = ramp[::-1]
        tri.reshape(-1)[5:261] = ramp
    return cmp, bg, tri


SHAPES = [(3, 5, 7), (2, 16, 24), (1, 1, 1)]


def test_reference_distinguishes_f64_from_f32_subtraction():
    """The float64-then-f32 values differ from the f32 subtraction's somewhere, so the bit-exact checks below can tell
    the reference's arithmetic from the obvious torch preprocessing."""
    u = np.arange(256, dtype=np.uint8)
    a = (u[:, None].astype(np.float64) - VGG_MEAN).astype(np.float32)
    b = u[:, None].astype(np.float32) - VGG_MEAN.astype(np.float32)
    assert (a != b).any()
    t64 = (u.astype(np.float64) / 255.0 - 0.5).astype(np.float32)
    t32 = u.astype(np.float32) / np.float32(255.0) - np.float32(0.5)
    assert (t64 != t32).any()


@pytest.mark.parametrize("trimap", [True, False], ids=["c7", "c6"])
@pytest.mark.parametrize("static", [False, True], ids=["nb=n", "nb=1"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_frames_from_u8_bit_exact(shape, static, trimap):
    from vmatting import ops
    n, h, w = shape
    cmp, bg, tri = clip(n, h, w, seed=n * h)
    if n * h * w >= 256:
        assert all(len(np.unique(p.reshape(-1, 3)[:, c])) == 256 for p in (cmp, bg) for c in range(3))
        assert len(np.unique(tri)) == 256
    if static:
        bg = bg[0]
    if not trimap:
        tri = None
    want = feed(cmp, bg, tri)
    c = want.shape[-1]
    dc, db = torch.from_numpy(cmp).cuda(), torch.from_numpy(bg).cuda()
    dt = None if tri is None else torch.from_numpy(tri).cuda()
    # f32 into a dense tensor
    got = ops.frames_from_u8(dc, db, dt)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, h, w, c)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # f32 into channels 2.. of a wider tensor: the channel offset and the pixel stride; the rest is untouched
    wide = torch.full((n, h, w, 11), -7.0, dtype=torch.float32, device="cuda")
    ops.frames_from_u8(dc, db, dt, out=wide[..., 2:2 + c])
    wn = wide.cpu().numpy()
    assert np.array_equal(wn[..., 2:2 + c].view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    assert (wn[..., :2] == -7.0).all() and (wn[..., 2 + c:] == -7.0).all()
    # bf16 x 8: RNE bf16 of the f32 values, zero pad channels, nothing outside the view's frames written
    SENT = 0x7B7B
    buf = torch.full((n + 2, h, w, 8), SENT, dtype=torch.int16, device="cuda")
    view = buf.view(torch.bfloat16)[1:n + 1, :, :, :c]
    ops.frames_from_u8(dc, db, dt, out=view)
    bits = buf.cpu().numpy()
    wb = torch.from_numpy(want).to(torch.bfloat16).view(torch.int16).numpy()
    assert np.array_equal(bits[1:n + 1, :, :, :c], wb)
    assert (bits[1:n + 1, :, :, c:] == 0).all()
    assert (bits[0] == SENT).all() and (bits[n + 1] == SENT).all()
    # the allocated bf16 form is the [..., :C] view of an 8-channel buffer
    g16 = ops.frames_from_u8(dc, db, dt, dtype=torch.bfloat16)
    assert g16.stride(2) == 8 and np.array_equal(g16.contiguous().view(torch.int16).cpu().numpy(), wb)


def test_frames_from_u8_unaligned_planes():
    """Planes that start at an odd byte take the one-pixel-per-thread path: the same values."""
    from vmatting import ops
    n, h, w = 2, 9, 13
    cmp, bg, tri = clip(n, h, w, seed=5)
    want = feed(cmp, bg, tri)

    def odd(a):
        raw = torch.zeros(a.size + 1, dtype=torch.uint8, device="cuda")
        raw[1:] = torch.from_numpy(a.reshape(-1)).cuda()
        return raw[1:].view(a.shape)
    dc, db, dt = odd(cmp), odd(bg), odd(tri)
    assert dc.data_ptr() % 4 == 1
    got = ops.frames_from_u8(dc, db, dt)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    g16 = ops.frames_from_u8(dc, db, dt, dtype=torch.bfloat16)
    assert torch.equal(g16.cpu(), torch.from_numpy(want).to(torch.bfloat16))


def quantize_ref(a, m):
    with np.errstate(invalid="ignore"):
        r = np.rint(a.astype(np.float32) * np.float32(m))
    r = np.where(np.isnan(r), np.float32(0), r)  # NaN gives 0
    return np.clip(r, 0, m).astype(np.uint8 if m == 255 else np.uint16)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("size", [1, 7, 4099])
def test_matte_quantize_bit_exact(size, bits):
    from vmatting import ops
    m = 255 if bits == 8 else 65535
    special = np.array([0.0, 1.0, np.nextafter(np.float32(0), np.float32(-1)), np.nextafter(np.float32(1), np.float32(2)),
                        -0.25, 1.5, -0.0, np.inf, -np.inf, np.nan, 0.5, 1e-9], np.float32)
    # exact ties: products k + 0.5 that f32 represents exactly (rint rounds them to even), and their neighbours
    k = np.arange(0, 64, dtype=np.float32)
    ties = ((k + np.float32(0.5)) / np.float32(m)).astype(np.float32)
    ties = np.concatenate([ties, np.nextafter(ties, np.float32(2)), np.nextafter(ties, np.float32(-1)),
                           np.float32(m - 0.5) / np.float32(m) * np.ones(1, np.float32)])
    rs = np.random.RandomState(size + bits)
    pool = np.concatenate([special, ties, rs.uniform(-0.05, 1.05, 4099).astype(np.float32)])
    a = pool[:size] if size >= len(special) else pool[[1, 9, 0, 7, 5, 3, 8][:size]]
    if size == 4099:
        prod = a[np.isfinite(a)] * np.float32(m)
        assert ((prod - np.floor(prod)) == 0.5).sum() >= 8  # the ties are really ties in f32
        assert np.isnan(a).any() and np.isinf(a).any()
    want = quantize_ref(a, m)
    got = ops.matte_quantize(torch.from_numpy(a).cuda(), bits=bits)
    assert got.dtype == (torch.uint8 if bits == 8 else torch.uint16)
    assert np.array_equal(got.cpu().numpy(), want)
    # an unaligned alpha (offset by one float) takes the scalar path: the same values
    if size > 1:
        base = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), a])).cuda()
        got = ops.matte_quantize(base[1:], bits=bits)
        assert np.array_equal(got.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------- model

SIZES = [(24, 40), (70, 90)]  # the second: odd sizes at every pooling level


def _model(vgg0, cls, dtype):
    from vmatting import unet
    np.random.seed(0)
    return getattr(unet, cls)(vgg0, dtype=dtype, device="cuda").prepare()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dtype", ["bf16", "fp32", "f16x3"])
def test_from_uint8_equals_video_matter_on_numpy_frames(vgg0, dtype, size):
    """VideoMatter.from_uint8 (ingest kernel inside each chunk's graph; bf16: the bf16 x 8 frame straight into the first
    pair kernel) gives the alpha of VideoMatter on the numpy-built f32 frames, bit for bit; graph and eager agree."""
    from vmatting import video
    h, w = size
    n = 3
    cmp, bg, tri = clip(n, h, w, seed=h)
    model = _model(vgg0, "UNetVideo", dtype)
    frames = torch.from_numpy(feed(cmp, bg, tri)).cuda().contiguous()
    want = video.VideoMatter(model, frames, chunk=2, graph=False).run().clone()
    dc, db, dt = (torch.from_numpy(a).cuda() for a in (cmp, bg, tri))
    for graph in (True, False):
        vm = video.VideoMatter.from_uint8(model, dc, db, dt, chunk=2, graph=graph)
        assert vm.frames.dtype == (torch.bfloat16 if dtype == "bf16" else torch.float32)
        got = vm.run().clone()
        torch.cuda.synchronize()
        assert vm.overflowed_chunks == []
        assert torch.equal(got, want), "graph=%s" % graph
    # the graphs read the uint8 tensors when they run: new bytes in place, new mattes
    dc.copy_(torch.from_numpy(cmp[::-1].copy()).cuda())
    dt.copy_(torch.from_numpy(tri[::-1].copy()).cuda())
    f2 = torch.from_numpy(feed(cmp[::-1], bg, tri[::-1])).cuda().contiguous()
    want2 = video.VideoMatter(model, f2, chunk=2, graph=False).run().clone()
    vm = video.VideoMatter.from_uint8(model, dc, db, dt, chunk=2, graph=True)
    assert torch.equal(vm.run(), want2)
    # one static plate for the whole clip
    plate = torch.from_numpy(bg[0]).cuda()
    f3 = torch.from_numpy(feed(cmp[::-1], bg[0], tri[::-1])).cuda().contiguous()
    want3 = video.VideoMatter(model, f3, chunk=2, graph=False).run().clone()
    assert torch.equal(video.VideoMatter.from_uint8(model, dc, plate, dt, chunk=2).run(), want3)


@pytest.mark.parametrize("dtype", ["bf16", "fp32", "f16x3"])
def test_from_uint8_image_model_without_trimap(vgg0, dtype):
    from vmatting import video
    h, w = SIZES[1]
    cmp, bg, _ = clip(2, h, w, seed=11)
    model = _model(vgg0, "UNetImage", dtype)
    frames = torch.from_numpy(feed(cmp, bg)).cuda().contiguous()
    want = video.VideoMatter(model, frames, chunk=2, graph=False).run().clone()
    dc, db = torch.from_numpy(cmp).cuda(), torch.from_numpy(bg).cuda()
    for graph in (True, False):
        got = video.VideoMatter.from_uint8(model, dc, db, None, chunk=2, graph=graph).run()
        assert torch.equal(got, want), "graph=%s" % graph


def test_bf16_frame_through_forward_and_capture(vgg0):
    """UNet.forward / capture on a bf16 x 8 frame: the f32 frame's alpha bit for bit, also on the unfused first pair
    (the frame is in8 itself) and through a copying (non-static) graph; .conv1_1 is evaluated from the bf16 frame."""
    from vmatting import ops
    h, w = SIZES[0]
    cmp, bg, tri = clip(2, h, w, seed=2)
    model = _model(vgg0, "UNetVideo", "bf16")
    f32 = torch.from_numpy(feed(cmp, bg, tri)).cuda()
    x16 = ops.frames_from_u8(*(torch.from_numpy(a).cuda() for a in (cmp, bg, tri)), dtype=torch.bfloat16)
    want = model.forward(f32).clone()
    c11 = model.conv1_1.clone()
    assert torch.equal(model.forward(x16), want)
    assert torch.equal(model.conv1_1, c11)
    g = model.capture(x16)
    assert g.input.dtype == torch.bfloat16 and g.input.stride(2) == 8
    assert torch.equal(g(x16), want)
    model.fuse_first = False
    try:
        unfused = model.forward(f32).clone()
        assert torch.equal(model.forward(x16), unfused)
    finally:
        del model.fuse_first
