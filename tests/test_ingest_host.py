"""CPU checks of the clip ends (csrc/ingest.hip, vmatting/stream.py, video.VideoMatter.from_uint8): every argument
check happens on the host, before any GPU call, so none of this needs a device."""

import ctypes

import numpy as np
import pytest
import torch


def _view(n=2, h=3, w=5, c=7, cstride=7, coff=0, dtype=0, ptr=64):
    from vmatting import _lib
    return _lib.VmTensor(ptr, n, h, w, c, cstride, coff, dtype)


def test_frames_from_u8_rejects_bad_arguments():
    from vmatting import _lib
    lib = _lib.lib()
    P = 64  # a non-null address: validation never dereferences it
    ok = _view()
    cases = [
        (None, P, P, 1, ok), (P, None, P, 1, ok), (P, P, P, 1, None), (P, P, P, 1, _view(ptr=None)),  # NULLs
        (P, P, P, 3, ok), (P, P, P, 0, ok),                       # nb outside {1, n}
        (P, P, None, 1, ok), (P, P, P, 1, _view(c=6, cstride=6)),  # C against the trimap pointer
        (P, P, None, 1, _view(c=5, cstride=8)),
        (P, P, P, 1, _view(dtype=_lib.VM_F16)), (P, P, P, 1, _view(dtype=_lib.VM_U8)),  # unsupported dtypes
        (P, P, P, 1, _view(n=0)), (P, P, P, 1, _view(cstride=6)), (P, P, P, 1, _view(coff=2, cstride=8)),
    ]
    for cmp, bg, tri, nb, out in cases:
        rc = lib.vm_frames_from_u8(cmp, bg, tri, nb, None if out is None else ctypes.byref(out), None)
        assert rc == _lib.VM_EINVAL, (cmp, bg, tri, nb)
        assert b"frames_from_u8" in lib.vm_last_error()
        with pytest.raises(ValueError):
            _lib.check(rc, "frames_from_u8")
    # a bf16 frame is whole 8-channel pixels: another layout is valid but not supported
    rc = lib.vm_frames_from_u8(P, P, P, 1, ctypes.byref(_view(cstride=16, dtype=_lib.VM_BF16)), None)
    assert rc == _lib.VM_EUNSUPPORTED and b"8-channel" in lib.vm_last_error()


def test_matte_quantize_rejects_bad_arguments():
    from vmatting import _lib
    lib = _lib.lib()
    for alpha, pixels, bits, out in [(None, 4, 8, 64), (64, 4, 8, None), (64, 0, 8, 64), (64, -1, 16, 64),
                                     (64, 4, 12, 64), (64, 4, 0, 64)]:
        rc = lib.vm_matte_quantize(alpha, pixels, bits, out, None)
        assert rc == _lib.VM_EINVAL, (alpha, pixels, bits, out)
        assert b"matte_quantize" in lib.vm_last_error()


def test_ops_wrappers_refuse_cpu_tensors():
    from vmatting import ops
    cmp, bg, tri = (torch.zeros(s, dtype=torch.uint8) for s in ((2, 4, 6, 3), (4, 6, 3), (2, 4, 6)))
    with pytest.raises(TypeError):
        ops.frames_from_u8(cmp, bg, tri)
    with pytest.raises(TypeError):
        ops.frames_from_u8(cmp, bg)
    with pytest.raises(TypeError):
        ops.matte_quantize(torch.zeros(8))
    # dtype and shape errors come first (no device needed to see them)
    with pytest.raises(TypeError):
        ops.frames_from_u8(cmp.float(), bg, tri)
    with pytest.raises(ValueError):
        ops.frames_from_u8(cmp, bg[:3], tri)
    with pytest.raises(ValueError):
        ops.frames_from_u8(cmp, bg, tri[:1])
    with pytest.raises(ValueError):
        ops.frames_from_u8(cmp[..., :2], bg, tri)


@pytest.fixture(scope="module")
def models(vgg0):
    from vmatting import unet
    np.random.seed(0)  # (the constructors do not touch the device)
    return unet.UNetVideo(vgg0, dtype="bf16", device="cuda"), unet.UNetImage(vgg0, dtype="bf16", device="cuda")


def test_from_uint8_rejects_bad_frames(models):
    from vmatting import video
    mv, mi = models
    cmp, bg, tri = (torch.zeros(s, dtype=torch.uint8) for s in ((2, 4, 6, 3), (2, 4, 6, 3), (2, 4, 6)))
    with pytest.raises(TypeError):
        video.VideoMatter.from_uint8(mv, cmp.float(), bg, tri)
    with pytest.raises(TypeError):
        video.VideoMatter.from_uint8(mv, cmp, bg, tri.to(torch.int16))
    with pytest.raises(ValueError):
        video.VideoMatter.from_uint8(mv, cmp, bg[:, :3], tri)
    with pytest.raises(ValueError):
        video.VideoMatter.from_uint8(mv, cmp[0], bg, tri)
    with pytest.raises(ValueError):
        video.VideoMatter.from_uint8(mv, cmp, bg)            # a 7-channel model needs the trimap
    with pytest.raises(ValueError):
        video.VideoMatter.from_uint8(mi, cmp, bg, tri)       # a 6-channel model takes none
    with pytest.raises(TypeError):
        video.VideoMatter.from_uint8(mv, cmp, bg, tri)       # right frames, but on the host


def test_frame_stream_rejects_bad_arguments_and_items(models):
    from vmatting import FrameStream, stream
    assert stream.FrameStream is FrameStream
    mv, mi = models
    plate = np.zeros((4, 6, 3), np.uint8)
    for kw in (dict(chunk=0), dict(depth=0), dict(out="u4"), dict(trimap=False), dict(static_bg=plate[:3]),
               dict(static_bg=plate.astype(np.float32))):
        with pytest.raises((ValueError, TypeError)):
            FrameStream(mv, 4, 6, **kw)
    with pytest.raises(ValueError):
        FrameStream(mi, 4, 6, trimap=True)

    def first(fs, item):
        return next(fs.run(iter([item])))

    cmp, bg, tri = np.zeros((2, 4, 6, 3), np.uint8), np.zeros((2, 4, 6, 3), np.uint8), np.zeros((2, 4, 6), np.uint8)
    fs = FrameStream(mv, 4, 6, chunk=2)
    bad = [(cmp.astype(np.float32), bg, tri), (cmp, bg.astype(np.int8), tri), (cmp, bg, tri.astype(np.uint16)),  # dtypes
           (cmp[:, :3], bg[:, :3], tri[:, :3]), (cmp, bg[:1], tri), (cmp, bg, tri[:, :, :5]), (cmp[0], bg[0], tri[0]),
           (np.zeros((3, 4, 6, 3), np.uint8), np.zeros((3, 4, 6, 3), np.uint8), np.zeros((3, 4, 6), np.uint8)),  # k > chunk
           (cmp, None, tri),   # bg=None without a static_bg
           (cmp, bg, None), (cmp, bg), torch.zeros(2, 4, 6, 3, dtype=torch.uint8)]
    for item in bad:
        with pytest.raises((ValueError, TypeError)):
            first(fs, item)
        assert fs._slots is None  # rejected before anything was allocated on the device
    with pytest.raises(ValueError):
        first(FrameStream(mv, 4, 6, chunk=2, static_bg=plate), (cmp, bg, tri))  # a plate AND per-frame backgrounds
    with pytest.raises(ValueError):
        first(FrameStream(mi, 4, 6, chunk=2, trimap=False), (cmp, bg, tri))
    # a failing source propagates as it is, and an empty one yields nothing; neither touches the device
    def boom():
        raise KeyError("decoder")
        yield
    with pytest.raises(KeyError):
        list(fs.run(boom()))
    assert list(fs.run(iter([]))) == [] and fs._slots is None
