"""CPU checks of the matte applied (vm_matte_compose in csrc/ingest.hip, ops.matte_compose, out="over" / "bgra" /
"premul" of FrameStream and ClipStream): every argument check happens on the host, before any GPU call, and the numpy
restatement the GPU tests compare against (tests/compose_ref.py) has the properties the definition promises."""

import numpy as np
import pytest
import torch

import compose_ref as cr


# ---------------------------------------------------------------------------------------------- C entry point
def test_matte_compose_rejects_bad_arguments():
    from vmatting import _lib
    lib = _lib.lib()
    assert (_lib.VM_COMPOSE_OVER, _lib.VM_COMPOSE_STRAIGHT, _lib.VM_COMPOSE_PREMUL) == (0, 1, 2)
    P = 64  # a non-null address: validation never dereferences it
    OVER, STRAIGHT, PREMUL = 0, 1, 2
    #        alpha cmp  bg    nb new_bg nn n  h  w  mode     out
    cases = [(None, P, P, 2, P, 2, 2, 3, 5, OVER, P), (P, None, P, 2, P, 2, 2, 3, 5, OVER, P),  # NULLs
             (P, P, None, 2, P, 2, 2, 3, 5, OVER, P), (P, P, P, 2, P, 2, 2, 3, 5, OVER, None),
             (P, P, None, 2, None, 0, 2, 3, 5, PREMUL, P), (P, P, P, 2, None, 0, 2, 3, 5, STRAIGHT, None),
             (P, P, P, 0, P, 0, 0, 3, 5, OVER, P), (P, P, P, 2, P, 2, 2, 0, 5, OVER, P),  # n, h, w <= 0
             (P, P, P, 2, P, 2, 2, 3, -1, OVER, P), (P, P, P, 1, None, 0, -2, 3, 5, PREMUL, P),
             (P, P, P, 3, P, 2, 2, 3, 5, OVER, P), (P, P, P, 0, P, 2, 2, 3, 5, OVER, P),  # nb outside {1, n}
             (P, P, P, 4, None, 0, 3, 3, 5, STRAIGHT, P),
             (P, P, P, 2, P, 2, 2, 3, 5, 3, P), (P, P, P, 2, P, 2, 2, 3, 5, -1, P),  # mode outside 0..2
             (P, P, P, 2, None, 0, 2, 3, 5, 7, P),
             (P, P, P, 2, None, 2, 2, 3, 5, OVER, P), (P, P, P, 2, None, 0, 2, 3, 5, OVER, P),  # OVER without a plate
             (P, P, P, 2, P, 0, 2, 3, 5, OVER, P), (P, P, P, 2, P, 3, 2, 3, 5, OVER, P),  # OVER, nn outside {1, n}
             (P, P, P, 2, P, 0, 2, 3, 5, STRAIGHT, P), (P, P, P, 2, P, 0, 2, 3, 5, PREMUL, P),  # a layer with a plate
             (P, P, P, 2, None, 1, 2, 3, 5, STRAIGHT, P), (P, P, P, 2, None, 2, 2, 3, 5, PREMUL, P),  # a layer with nn != 0
             (P, P, P, 2, P, 2, 2, 3, 5, PREMUL, P)]
    for case in cases:
        rc = lib.vm_matte_compose(*case, None)
        assert rc == _lib.VM_EINVAL, case
        assert b"matte_compose" in lib.vm_last_error(), case
        with pytest.raises(ValueError):
            _lib.check(rc, "matte_compose")


# ---------------------------------------------------------------------------------------------- ops wrapper
def test_ops_matte_compose_checks_before_the_device():
    from vmatting import ops
    n, h, w = 2, 4, 6
    alpha = torch.zeros((n, h, w), dtype=torch.float32)
    cmp, bg, plate = (torch.zeros(s, dtype=torch.uint8) for s in ((n, h, w, 3), (n, h, w, 3), (h, w, 3)))
    for bad_alpha in (alpha.double(), alpha.half(), alpha.to(torch.uint8), alpha.numpy()):  # dtypes
        with pytest.raises(TypeError):
            ops.matte_compose(bad_alpha, cmp, bg, mode="bgra")
    with pytest.raises(TypeError):
        ops.matte_compose(alpha, cmp.float(), bg, mode="bgra")
    with pytest.raises(TypeError):
        ops.matte_compose(alpha, cmp, bg.to(torch.int8), mode="premul")
    with pytest.raises(TypeError):
        ops.matte_compose(alpha, cmp, bg, new_bg=plate.float(), mode="over")
    for kw in (dict(alpha=alpha[:1]), dict(alpha=alpha[:, :3]), dict(alpha=alpha[..., None, None]),  # shapes
               dict(cmp=cmp[..., :2]), dict(cmp=cmp[0]), dict(bg=bg[:, :3]), dict(bg=plate[:3]),
               dict(out=torch.zeros((n, h, w, 3), dtype=torch.uint8)),           # a BGRA layer has 4 channels
               dict(out=torch.zeros((n, h, w, 4), dtype=torch.float32))):
        a = dict(alpha=alpha, cmp=cmp, bg=bg, out=None)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.matte_compose(a["alpha"], a["cmp"], a["bg"], mode="bgra", out=a["out"])
    with pytest.raises(ValueError):
        ops.matte_compose(alpha, cmp, bg, new_bg=plate[:3], mode="over")
    with pytest.raises(ValueError):
        ops.matte_compose(alpha, cmp, bg, new_bg=plate, mode="over", out=torch.zeros((n, h, w, 4), dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.matte_compose(alpha, cmp, bg, mode="straight")
    # a plate with a layer mode, a missing plate with "over"
    for mode in ("bgra", "premul"):
        with pytest.raises(ValueError):
            ops.matte_compose(alpha, cmp, bg, new_bg=plate, mode=mode)
    with pytest.raises(ValueError):
        ops.matte_compose(alpha, cmp, bg, mode="over")
    # right tensors, but on the host
    for args, kw in (((alpha, cmp, bg), dict(mode="bgra")), ((alpha[..., None], cmp, plate), dict(mode="premul")),
                     ((alpha, cmp, bg), dict(new_bg=plate, mode="over"))):
        with pytest.raises(TypeError):
            ops.matte_compose(*args, **kw)


# ---------------------------------------------------------------------------------------------- the streams
@pytest.fixture(scope="module")
def video_model(vgg0):
    from vmatting import unet
    np.random.seed(0)  # (the constructor does not touch the device)
    return unet.UNetVideo(vgg0, dtype="bf16", device="cuda")


def _simple_model():
    """A UNetSimple without its constructor (which packs weights on the device): ClipStream's host-side checks read
    only its type, dtype and device."""
    from vmatting.unet_simple import UNetSimple
    m = UNetSimple.__new__(UNetSimple)
    m.dtype, m.device = torch.bfloat16, torch.device("cuda")
    return m


H, W = 4, 6
PLATE = np.zeros((H, W, 3), np.uint8)


def _constructor_errors(make):
    with pytest.raises(ValueError):
        make(out="over")                                   # "over" without its plate
    for out in ("u8", "u16", "f32", "bgra", "premul"):     # a plate with anything else
        with pytest.raises(ValueError):
            make(out=out, new_bg=PLATE)
        with pytest.raises(ValueError):
            make(out=out, new_bg="per_frame")
    with pytest.raises(ValueError):
        make(new_bg=PLATE)                                 # (out defaults to "u8")
    for bad in (PLATE[:3], PLATE[None], PLATE[..., :2]):   # a wrong plate shape
        with pytest.raises(ValueError):
            make(out="over", new_bg=bad)
    with pytest.raises(ValueError):
        make(out="over", new_bg="each_frame")
    for bad in (PLATE.astype(np.float32), PLATE.astype(np.int8)):  # a wrong plate dtype
        with pytest.raises(TypeError):
            make(out="over", new_bg=bad)
    for out in ("bgra", "premul"):
        assert make(out=out).new_bg is None
    assert make(out="over", new_bg="per_frame").new_bg == "per_frame"
    s = make(out="over", new_bg=PLATE[:, ::-1])
    assert s.new_bg.flags.c_contiguous and s._slots is None


def test_frame_stream_compose_arguments_and_items(video_model):
    from vmatting import FrameStream
    _constructor_errors(lambda **kw: FrameStream(video_model, H, W, chunk=2, **kw))

    def first(fs, item):
        return next(fs.run(iter([item])))

    cmp, bg, tri = np.zeros((2, H, W, 3), np.uint8), np.zeros((2, H, W, 3), np.uint8), np.zeros((2, H, W), np.uint8)
    nw = np.zeros((2, H, W, 3), np.uint8)
    fs = FrameStream(video_model, H, W, chunk=2, out="over", new_bg="per_frame")
    got = fs.check_item((cmp, bg, tri, nw))
    assert len(got) == 5 and got[3] == 2 and got[4] is nw
    bad = [(cmp, bg, tri),                                            # the old arity
           (cmp, bg, tri, nw, nw), (cmp, bg, tri, None),
           (cmp, bg, tri, nw[:1]),                                    # a per-frame plate with wrong k
           (cmp[:1], bg[:1], tri[:1], nw),
           (cmp, bg, tri, nw[0]), (cmp, bg, tri, nw[:, :3]), (cmp, bg, tri, nw[..., :2]),
           (cmp, bg, tri, nw.astype(np.float32)), (cmp, bg, tri, torch.zeros(2, H, W, 3, dtype=torch.uint8)),
           (cmp, bg, tri.astype(np.uint16), nw)]                      # the old checks still run
    for item in bad:
        with pytest.raises((ValueError, TypeError)):
            first(fs, item)
        assert fs._slots is None  # rejected before anything was allocated on the device
    # a static new plate, and the layer modes, keep the old arity
    for kw in (dict(out="over", new_bg=PLATE), dict(out="bgra"), dict(out="premul")):
        fs = FrameStream(video_model, H, W, chunk=2, **kw)
        assert len(fs.check_item((cmp, bg, tri))) == 4
        with pytest.raises(ValueError):
            first(fs, (cmp, bg, tri, nw))
        assert fs._slots is None


def test_clip_stream_compose_arguments_and_items():
    from vmatting import ClipStream
    m = _simple_model()
    _constructor_errors(lambda **kw: ClipStream(m, H, W, **kw))

    def first(cs, item):
        return next(cs.run(iter([item]), np.zeros((H, W), np.float32)))

    cmp, bg, nw = (np.zeros((H, W, 3), np.uint8) for _ in range(3))
    bw = np.zeros((H, W, 2), np.float32)
    cs = ClipStream(m, H, W, out="over", new_bg="per_frame")
    got = cs.check_item((cmp, bg, bw, None, nw))
    assert len(got) == 5 and got[4] is nw
    bad = [(cmp, bg, bw, None),                                        # the old arity
           (cmp, bg, bw, None, nw, nw), (cmp, bg, bw, None, None),
           (cmp, bg, bw, None, nw[None]), (cmp, bg, bw, None, nw[:3]), (cmp, bg, bw, None, nw[..., :2]),
           (cmp, bg, bw, None, nw.astype(np.float32)), (cmp, bg, bw, None, torch.zeros(H, W, 3, dtype=torch.uint8)),
           (cmp, bg, bw.astype(np.float64), None, nw)]                 # the old checks still run
    for item in bad:
        with pytest.raises((ValueError, TypeError)):
            first(cs, item)
        assert cs._slots is None
    for kw in (dict(out="over", new_bg=PLATE), dict(out="bgra"), dict(out="premul")):
        cs = ClipStream(m, H, W, **kw)
        assert cs.check_item((cmp, bg, bw, None)) == (cmp, bg, bw, None)
        with pytest.raises(ValueError):
            first(cs, (cmp, bg, bw, None, nw))
        assert cs._slots is None


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.fixture(scope="module")
def pixels():
    rs = np.random.RandomState(11)
    n = 200000
    alpha = rs.uniform(0.0, 1.0, (1, 1, n)).astype(np.float32)
    special = cr.special_alphas()
    alpha[0, 0, :special.size] = special
    fg, bg, nw = (rs.randint(0, 256, (1, 1, n, 3)).astype(np.uint8) for _ in range(3))
    a = np.clip(np.nan_to_num(alpha.astype(np.float64)), 0.0, 1.0)[..., None]
    cmp = np.rint(a * fg + (1.0 - a) * bg).astype(np.uint8)  # composites made from a known foreground
    return alpha, cmp, bg, nw


def test_restatement_over_identities(pixels):
    alpha, cmp, bg, nw = pixels
    assert np.array_equal(cr.compose(alpha, cmp, bg, bg, "over"), cmp)          # the same plate back: cmp exactly
    assert np.array_equal(cr.compose(np.ones_like(alpha), cmp, bg, nw, "over"), cmp)  # all foreground: cmp
    assert np.array_equal(cr.compose(np.zeros_like(alpha), bg, bg, nw, "over"), nw)   # all background: the new plate
    out = cr.compose(alpha, cmp, bg, nw, "over")
    assert out.shape == cmp.shape and out.dtype == np.uint8 and not np.array_equal(out, cmp)
    # both clamps fire
    z, f = np.zeros_like(cmp), np.full_like(cmp, 255)
    assert (cr.compose(np.zeros_like(alpha), z, f, z, "over") == 0).all()       # 0 + (0 - 255) -> 0
    assert (cr.compose(np.zeros_like(alpha), f, z, f, "over") == 255).all()     # 255 + (255 - 0) -> 255


def test_restatement_layers(pixels):
    alpha, cmp, bg, _ = pixels
    q = cr.quantize8(alpha)
    assert q[0, 0, :6].tolist() == [0, 255, 0, 255, 0, 0]  # 0, 1, -0.25, 1.5, NaN, a denormal
    for mode in ("bgra", "premul"):
        out = cr.compose(alpha, cmp, bg, mode=mode)
        assert out.shape == cmp.shape[:3] + (4,) and out.dtype == np.uint8
        assert np.array_equal(out[..., 3], q)               # the alpha channel is the u8 matte
        assert np.array_equal(out[q == 255][:, :3], cmp[q == 255])  # opaque: the composite itself
    straight = cr.compose(alpha, cmp, bg, mode="bgra")
    assert (q == 0).sum() >= 4 and (straight[q == 0] == 0).all()  # transparent: zeros
    assert np.array_equal(cr.compose(alpha, cmp, bg, mode="premul")[q == 0][:, :3],  # premultiplied there: c - b
                          np.clip(cmp[q == 0].astype(int) - bg[q == 0], 0, 255))
    # both clamps of the straight layer: c = 255 over b = 0 at a small q, and the reverse
    small = np.full_like(alpha, 3.0 / 255.0)
    z, f = np.zeros_like(cmp), np.full_like(cmp, 255)
    assert (cr.compose(small, f, z, mode="bgra")[..., :3] == 255).all()
    assert (cr.compose(small, z, f, mode="bgra")[..., :3] == 0).all()


def test_premultiplied_layer_recomposes_within_one_level(pixels):
    """A condition on the definition: for composites made from a known foreground, the premultiplied layer put back
    over the original plate with its stored alpha, rint(P + (255 - q) b / 255), is within 1 level of cmp."""
    alpha, cmp, bg, _ = pixels
    out = cr.compose(alpha, cmp, bg, mode="premul")
    p, q = out[..., :3].astype(np.float64), out[..., 3:].astype(np.float64)
    back = np.rint(p + (255.0 - q) * bg.astype(np.float64) / 255.0)
    err = np.abs(back - cmp.astype(np.float64))
    print("recomposed premultiplied layer: max |err| = %d, %.3f %% of values off" % (err.max(), 100.0 * (err > 0).mean()))
    assert err.max() <= 1
