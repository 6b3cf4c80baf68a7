"""CPU checks of the video model's clip path (vm_clip_feed in csrc/flow.hip, ops.clip_feed, vmatting/clip.py): every
argument check happens on the host, before any GPU call, so none of this needs a device."""

import ctypes

import numpy as np
import pytest
import torch

P = 64  # a non-null, 16-byte aligned address: validation never dereferences it


def _towers(n=6, h=3, w=5, c=3, cstride=8, coff=0, dtype=1, ptr=P):
    from vmatting import _lib
    return _lib.VmTensor(ptr, n, h, w, c, cstride, coff, dtype)


def _cat(n=2, h=3, w=5, c=9, cstride=32, coff=0, dtype=1, ptr=P):
    from vmatting import _lib
    return _lib.VmTensor(ptr, n, h, w, c, cstride, coff, dtype)


def _call(cmp=P, bg=P, nb=2, prev=P, bw=P, fw=None, thresh=15.0, promote=0, towers="ok", cat="ok", warped=None,
          err=None):
    from vmatting import _lib
    towers = _towers() if towers == "ok" else towers
    cat = _cat() if cat == "ok" else cat
    rc = _lib.lib().vm_clip_feed(cmp, bg, nb, prev, bw, fw, thresh, promote,
                                 None if towers is None else ctypes.byref(towers),
                                 None if cat is None else ctypes.byref(cat), warped, err, None)
    return rc, _lib.lib().vm_last_error()


def test_clip_feed_rejects_bad_arguments():
    from vmatting import _lib
    F32, BF16 = _lib.VM_F32, _lib.VM_BF16
    invalid = [
        dict(cmp=None), dict(bg=None), dict(prev=None), dict(bw=None), dict(towers=None), dict(cat=None),  # NULLs
        dict(towers=_towers(ptr=None)), dict(cat=_cat(ptr=None)),
        dict(nb=3), dict(nb=0),                                                # nb outside {1, n}
        dict(towers=_towers(n=5)), dict(towers=_towers(n=2)),                  # towers.n != 3 * cat.n
        dict(towers=_towers(h=4)), dict(cat=_cat(w=6)),                        # mismatched h / w
        dict(cat=_cat(n=0)),
        dict(towers=_towers(c=8)), dict(cat=_cat(c=6)), dict(cat=_cat(c=16)),  # wrong channel counts
        dict(towers=_towers(dtype=_lib.VM_F16), cat=_cat(dtype=_lib.VM_F16)),  # a dtype other than f32 / bf16
        dict(towers=_towers(dtype=_lib.VM_U8), cat=_cat(dtype=_lib.VM_U8)),
        dict(towers=_towers(dtype=F32)), dict(cat=_cat(dtype=F32)),            # differing dtypes
        dict(promote=2), dict(promote=-1),
        dict(fw=P),                                                            # a forward flow without its flag
    ]
    for kw in invalid:
        rc, msg = _call(**kw)
        assert rc == _lib.VM_EINVAL, (kw, rc, msg)
        assert b"clip_feed" in msg
        with pytest.raises(ValueError):
            _lib.check(rc, "clip_feed")
    # valid descriptions of layouts the kernel does not take
    unsupported = [
        dict(towers=_towers(cstride=16)), dict(towers=_towers(cstride=4)), dict(towers=_towers(coff=1)),
        dict(towers=_towers(ptr=P + 8)),
        dict(cat=_cat(cstride=9)), dict(cat=_cat(cstride=12)), dict(cat=_cat(cstride=20)), dict(cat=_cat(coff=8)),
        dict(cat=_cat(ptr=P + 2)),
        dict(towers=_towers(dtype=F32), cat=_cat(dtype=F32, cstride=18)),
        dict(bw=P + 4), dict(fw=P + 4, err=P),                                 # flows are read as float2
    ]
    for kw in unsupported:
        rc, msg = _call(**kw)
        assert rc == _lib.VM_EUNSUPPORTED, (kw, rc, msg)
        assert b"clip_feed" in msg
        with pytest.raises(NotImplementedError):
            _lib.check(rc, "clip_feed")
    assert BF16 == 1  # (the views above default to bf16)


def _host_feed_args(n=2, h=4, w=6):
    cmp = torch.zeros((n, h, w, 3), dtype=torch.uint8)
    bg = torch.zeros((n, h, w, 3), dtype=torch.uint8)
    prev = torch.zeros((n, h, w), dtype=torch.float32)
    bw = torch.zeros((n, h, w, 2), dtype=torch.float32)
    towers = torch.zeros((3 * n, h, w, 8), dtype=torch.bfloat16)[..., :3]
    cat = torch.zeros((n, h, w, 32), dtype=torch.bfloat16)[..., :9]
    return cmp, bg, prev, bw, towers, cat


def test_ops_clip_feed_refuses_cpu_tensors_and_bad_shapes():
    from vmatting import ops
    cmp, bg, prev, bw, towers, cat = _host_feed_args()
    with pytest.raises(TypeError):  # everything is right but the device
        ops.clip_feed(cmp, bg, prev, bw, towers=towers, cat=cat)
    with pytest.raises(TypeError):
        ops.clip_feed(cmp, bg[0], prev, bw, forward=bw.clone(), towers=towers, cat=cat)
    # dtype and shape errors come first (no device needed to see them)
    for kw in (dict(cmp=cmp.float()), dict(bg=bg.to(torch.int8)), dict(prev=prev.double()), dict(bw=bw.half()),
               dict(forward=bw.double()), dict(towers=towers.float()), dict(cat=cat.half(), towers=towers.half()),
               dict(warped=prev.double()), dict(err=torch.zeros(1))):
        a = dict(cmp=cmp, bg=bg, prev=prev, bw=bw, forward=None, towers=towers, cat=cat, warped=None, err=None)
        a.update(kw)
        with pytest.raises(TypeError):
            ops.clip_feed(a["cmp"], a["bg"], a["prev"], a["bw"], forward=a["forward"], towers=a["towers"], cat=a["cat"],
                          warped=a["warped"], err=a["err"])
    for kw in (dict(cmp=cmp[..., :2]), dict(bg=bg[:, :3]), dict(prev=prev[:1]), dict(bw=bw[..., :1]),
               dict(forward=bw[:, :3]), dict(towers=towers[:4]), dict(cat=cat[..., :8]), dict(towers=None),
               dict(warped=prev[:, :2]), dict(promote="numpy3")):
        a = dict(cmp=cmp, bg=bg, prev=prev, bw=bw, forward=None, towers=towers, cat=cat, warped=None, promote="numpy1")
        a.update(kw)
        with pytest.raises(ValueError):
            ops.clip_feed(a["cmp"], a["bg"], a["prev"], a["bw"], forward=a["forward"], promote=a["promote"],
                          towers=a["towers"], cat=a["cat"], warped=a["warped"])


def _stub_model(dtype=torch.bfloat16):
    """A UNetSimple without its constructor (which packs weights on the device): ClipStream's host-side checks read
    only its type, dtype and device."""
    from vmatting.unet_simple import UNetSimple
    m = UNetSimple.__new__(UNetSimple)
    m.dtype, m.device = dtype, torch.device("cuda")
    return m


def test_clip_stream_rejects_bad_arguments(vgg0):
    from vmatting import ClipStream, clip, unet
    assert clip.ClipStream is ClipStream
    m = _stub_model()
    plate = np.zeros((4, 6, 3), np.uint8)
    for kw in (dict(depth=0), dict(out="u4"), dict(promote="numpy3"), dict(thresh=-1.0), dict(thresh=float("nan")),
               dict(static_bg=plate[:3]), dict(static_bg=plate.astype(np.float32))):
        with pytest.raises((ValueError, TypeError)):
            ClipStream(m, 4, 6, **kw)
    with pytest.raises(ValueError):
        ClipStream(m, 0, 6)
    # the per-frame models are not the video model, and fp16 is not one of its dtypes
    np.random.seed(0)
    with pytest.raises(TypeError):
        ClipStream(unet.UNetVideo(vgg0, dtype="bf16", device="cuda"), 4, 6)
    with pytest.raises(TypeError):
        ClipStream(object(), 4, 6)
    with pytest.raises(TypeError):
        ClipStream(_stub_model(torch.float16), 4, 6)
    cs = ClipStream(m, 4, 6, static_bg=plate, reuse_bg_tower=True)
    assert cs.reuse_bg_tower and not ClipStream(m, 4, 6).reuse_bg_tower  # reuse needs a plate
    assert not cs.occlusion and cs.thresh == 15.0 and cs.promote == "numpy1" and cs.out == "u8" and cs.depth == 2


def test_clip_stream_rejects_bad_items_before_touching_the_device():
    from vmatting import ClipStream
    m = _stub_model(torch.float32)
    h, w = 4, 6
    cmp, bg = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.uint8)
    bw, fw = np.zeros((h, w, 2), np.float32), np.zeros((h, w, 2), np.float32)
    a0 = np.zeros((h, w), np.float32)

    def first(cs, item, alpha0=a0):
        return next(cs.run(iter([item]), alpha0))

    cs = ClipStream(m, h, w)
    assert cs.check_item((cmp, bg, bw, None)) == (cmp, bg, bw, None)
    bad = [(cmp, bg, bw), (cmp, bg, bw, None, None), cmp,                      # not a 4-tuple
           (cmp, None, bw, None),                                              # bg=None without a static_bg
           (cmp, bg, bw, fw),                                                  # a forward flow without occlusion
           (cmp.astype(np.float32), bg, bw, None), (cmp, bg.astype(np.int8), bw, None),
           (cmp, bg, bw.astype(np.float64), None),                             # dtypes
           (cmp[:3], bg[:3], bw[:3], None), (cmp, bg[:, :5], bw, None), (cmp, bg, bw[..., :1], None),
           (cmp[None], bg[None], bw[None], None), (cmp, bg, None, None),
           (torch.zeros(h, w, 3, dtype=torch.uint8), bg, bw, None), (cmp, bg, bw.tolist(), None)]
    for item in bad:
        with pytest.raises((ValueError, TypeError)):
            first(cs, item)
        assert cs._slots is None  # rejected before anything was allocated on the device
    occ = ClipStream(m, h, w, occlusion=True, static_bg=bg)
    assert occ.check_item((cmp, None, bw, fw))[3] is fw
    for item in [(cmp, None, bw, None), (cmp, bg, bw, fw), (cmp, None, bw, fw.astype(np.float64)),
                 (cmp, None, bw, fw[:, :5])]:
        with pytest.raises((ValueError, TypeError)):
            first(occ, item)
        assert occ._slots is None
    # alpha0: f32 or uint8 [h,w]; uint8 is converted as f32(u / 255.0)
    for alpha0 in (a0[:3], a0.astype(np.float64), a0[None], None, a0.tolist()):
        with pytest.raises((ValueError, TypeError)):
            first(cs, (cmp, bg, bw, None), alpha0)
        assert cs._slots is None
    u = np.arange(h * w, dtype=np.uint8).reshape(h, w) * 10
    got = cs.check_alpha0(u)
    assert got.dtype == np.float32 and np.array_equal(got, (u.astype(np.float64) / 255.0).astype(np.float32))
    # a failing source propagates as it is, and an empty one yields nothing; neither touches the device

    def boom():
        raise KeyError("decoder")
        yield
    with pytest.raises(KeyError):
        list(cs.run(boom(), a0))
    assert list(cs.run(iter([]), a0)) == [] and cs._slots is None
