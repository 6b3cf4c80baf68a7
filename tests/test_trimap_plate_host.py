"""CPU checks of the trimap from the background plate: the numpy restatement (tests/trimap_plate_ref.py) against the
definition read pixel by pixel, its threshold edges, what the defaults give on a synthetic composite, and the host-side
argument checks of the C entry, the wrappers and FrameStream(trimap="auto"), which all happen before any GPU call."""

import numpy as np
import pytest
import torch

import trimap_plate_ref as ref


def brute(cmp, bg, lo, hi, r_bg, r_fg):
    """include/vmatting.h's definition, one pixel at a time."""
    h, w = cmp.shape[:2]
    c, b = cmp.astype(int), bg.astype(int)
    D = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)
                    D[y, x] += sum((int(c[yy, xx, k]) - int(b[yy, xx, k])) ** 2 for k in range(3))
    out = np.empty((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            def every(cond, r):
                return all(cond(D[yy, xx]) for yy in range(max(y - r, 0), min(y + r, h - 1) + 1)
                           for xx in range(max(x - r, 0), min(x + r, w - 1) + 1))
            fore = every(lambda v: v >= 9 * hi * hi, r_fg)
            back = every(lambda v: v <= 9 * lo * lo, r_bg)
            assert not (fore and back)
            out[y, x] = 255 if fore else 0 if back else 128
    return out


@pytest.mark.parametrize("shape", [(9, 11), (1, 7)])
@pytest.mark.parametrize("radii", [(0, 0), (1, 2), (2, 0), (12, 1)])   # 12: larger than either image
def test_restatement_equals_the_definition(shape, radii):
    h, w = shape
    for name, make in ref.PAIRS.items():
        cmp, bg = make(h, w, seed=3)
        for lo, hi in ((0, 1), (16, 48), (120, 200), (441, 442)):
            want = brute(cmp, bg, lo, hi, *radii)
            assert np.array_equal(ref.trimap(cmp, bg, lo, hi, *radii), want), (name, lo, hi)


def test_inputs_cover_what_they_claim():
    cmp, bg = ref.noise_pair(70, 90)
    assert set(np.unique(ref.trimap(cmp, bg, 120, 200, 0, 0)).tolist()) == {0, 128, 255}
    cmp, bg = ref.blob_pair(70, 90)
    assert set(np.unique(ref.trimap(cmp, bg, 16, 48, 1, 3)).tolist()) == {0, 128, 255}
    assert (ref.box_sum(*ref.equal_pair(9, 11)) == 0).all()
    assert (ref.box_sum(*ref.extreme_pair(9, 11)) == 27 * 255 * 255).all()
    assert 27 * 255 * 255 < 9 * 442 * 442 < 2 ** 31


def test_labels_exclude_each_other_and_shrink_with_the_radii():
    cmp, bg = ref.noise_pair(40, 60, seed=2)
    D = ref.box_sum(cmp, bg)
    for lo, hi in ((0, 1), (100, 101), (150, 250)):
        assert not ((D <= 9 * lo * lo) & (D >= 9 * hi * hi)).any()
    cmp, bg = ref.blob_pair(40, 60, seed=2)
    prev = ref.trimap(cmp, bg, 16, 48, 0, 0)
    for r in (1, 2, 5):
        cur = ref.trimap(cmp, bg, 16, 48, r, r)
        assert ((cur == 0) <= (prev == 0)).all() and ((cur == 255) <= (prev == 255)).all()
        prev = cur


def test_threshold_edges_are_exact():
    h, w = 7, 9
    bg = np.full((h, w, 3), 100, np.uint8)
    # D == 9 lo^2 is background, D == 9 lo^2 + 1 is not
    cmp = bg.copy()
    cmp[..., 0] += 5                      # d = 25 everywhere: D = 9 * 5^2
    assert (ref.trimap(cmp, bg, 5, 6, 0, 0) == 0).all()
    cmp[3, 4, 1] += 1                     # d = 26 there: D = 9 * 25 + 1 in its 3 x 3 neighbourhood
    out = ref.trimap(cmp, bg, 5, 6, 0, 0)
    assert (ref.box_sum(cmp, bg)[2:5, 3:6] == 226).all()
    assert (out[2:5, 3:6] == 128).all() and (out == 0).sum() == h * w - 9
    # D == 9 hi^2 is foreground, D == 9 hi^2 - 1 is not
    cmp = bg.copy()
    cmp[..., 2] += 3                      # d = 9: D = 9 * 3^2
    assert (ref.trimap(cmp, bg, 2, 3, 0, 0) == 255).all()
    cmp[3, 4] = bg[3, 4] + np.array([2, 2, 0], np.uint8)   # d = 8 there: D = 80
    out = ref.trimap(cmp, bg, 2, 3, 0, 0)
    assert (ref.box_sum(cmp, bg)[2:5, 3:6] == 80).all()
    assert (out[2:5, 3:6] == 128).all() and (out == 255).sum() == h * w - 9
    # the replicated border: a corner pixel counts four times in its own box sum
    cmp = bg.copy()
    cmp[0, 0, 0] += 1
    assert ref.box_sum(cmp, bg)[0, 0] == 4 and ref.box_sum(cmp, bg)[0, 1] == 2 and ref.box_sum(cmp, bg)[1, 1] == 1


def test_windows_are_clipped_not_padded():
    """Pixels outside the image do not erode: an all-background frame stays all background at any radius."""
    cmp, bg = ref.equal_pair(5, 40)
    assert (ref.trimap(cmp, bg, 16, 48, 32, 32) == 0).all()
    cmp, bg = ref.extreme_pair(5, 40)
    assert (ref.trimap(cmp, bg, 16, 48, 32, 32) == 255).all()


@pytest.mark.parametrize("seed", range(20))
def test_defaults_are_sound_on_a_synthetic_composite(seed):
    """No wrong certain label, and caps on how much stays unknown.  A numpy prototype gave, over these seeds: unknown
    share <= 0.21, >= 0.54 of the opaque pixels labelled 255, >= 0.88 of the background pixels labelled 0."""
    frame, plate, alpha = ref.scene(seed)
    assert frame.shape == (96, 160, 3)
    out = ref.trimap(frame, plate, **ref.DEFAULTS)
    assert not ((out == 0) & (alpha > 0)).any()
    assert not ((out == 255) & (alpha < 1)).any()
    assert (out == 128).mean() <= 0.30
    assert (out[alpha == 1] == 255).mean() >= 0.45
    assert (out[alpha == 0] == 0).mean() >= 0.80


# ---------------------------------------------------------------- the C entry point and the wrappers, on the host

def test_c_entry_rejects_bad_arguments():
    from vmatting import _lib
    lib = _lib.lib()
    P, Q, W = 4096, 8192, 64  # non-null addresses: validation never dereferences them
    ok = dict(cmp=P, bg=Q, nb=1, n=2, h=5, w=5, lo=16, hi=48, r_bg=4, r_fg=8, out=16384, work=W)
    bad = [dict(cmp=None), dict(bg=None), dict(out=None), dict(work=None),
           dict(n=0), dict(h=0), dict(w=0), dict(h=-1), dict(n=1 << 15, h=1 << 8, w=1 << 8),   # 2^31 pixels
           dict(nb=0), dict(nb=3),
           dict(lo=-1), dict(lo=48), dict(lo=49), dict(hi=443), dict(lo=442, hi=443),
           dict(r_bg=-1), dict(r_bg=33), dict(r_fg=-1), dict(r_fg=33),
           dict(out=P), dict(out=Q), dict(out=P + 149), dict(out=Q + 74), dict(out=P - 1),      # out overlaps cmp / bg
           dict(work=72)]
    order = ("cmp", "bg", "nb", "n", "h", "w", "lo", "hi", "r_bg", "r_fg", "out", "work")
    for change in bad:
        args = dict(ok, **change)
        rc = lib.vm_trimap_from_plate(*[args[k] for k in order], None)
        assert rc == _lib.VM_EINVAL, change
        assert b"trimap_from_plate" in lib.vm_last_error()
    for shape in ((0, 5, 5), (1, 0, 5), (1, 5, -1), (1 << 15, 1 << 8, 1 << 8)):
        assert lib.vm_trimap_from_plate_workspace_bytes(*shape) == 0
    # bit rows: one {background, foreground} pair of 64-bit words per 64 pixels of a row
    assert lib.vm_trimap_from_plate_workspace_bytes(1, 1080, 1920) == 1080 * 30 * 16
    assert lib.vm_trimap_from_plate_workspace_bytes(8, 3, 65) == 8 * 3 * 2 * 16
    assert lib.vm_abi_version() == 1


def test_check_plate_options():
    from vmatting import ops
    assert ops.PLATE_DEFAULTS == ref.DEFAULTS
    assert ops.check_plate_options("t", **ops.PLATE_DEFAULTS) == (16, 48, 4, 8)
    assert ops.check_plate_options("t", np.int32(0), np.int64(442), 0, 32) == (0, 442, 0, 32)
    good = dict(ops.PLATE_DEFAULTS)
    for key in good:
        for v in (1.0, "1", None, True):
            with pytest.raises(TypeError, match="t: %s must be an integer" % key):
                ops.check_plate_options("t", **dict(good, **{key: v}))
    for change in (dict(lo=-1), dict(lo=48), dict(lo=60), dict(hi=443), dict(hi=16), dict(r_bg=-1), dict(r_bg=33),
                   dict(r_fg=-1), dict(r_fg=33)):
        with pytest.raises(ValueError):
            ops.check_plate_options("t", **dict(good, **change))


def test_wrappers_check_on_the_host():
    from vmatting import ops, reader
    cmp, bg = torch.zeros((2, 4, 6, 3), dtype=torch.uint8), torch.zeros((4, 6, 3), dtype=torch.uint8)
    with pytest.raises(TypeError):
        ops.trimap_from_plate(cmp, bg)                       # right tensors, but on the host
    with pytest.raises(TypeError):
        ops.trimap_from_plate(cmp.float(), bg)
    with pytest.raises(TypeError):
        ops.trimap_from_plate(cmp.numpy(), bg)
    with pytest.raises(ValueError):
        ops.trimap_from_plate(cmp, bg[:3])
    with pytest.raises(ValueError):
        ops.trimap_from_plate(cmp[0], bg)
    with pytest.raises(ValueError):
        ops.trimap_from_plate(cmp, bg, lo=48)
    with pytest.raises(TypeError):
        ops.trimap_from_plate(cmp, bg, r_fg=2.0)
    with pytest.raises(TypeError):
        reader.trimap_from_plate(cmp.numpy(), bg)            # numpy and torch mixed
    with pytest.raises(TypeError):
        reader.trimap_from_plate(cmp.numpy().astype(np.int8), bg.numpy())
    with pytest.raises(ValueError):
        reader.trimap_from_plate(cmp.numpy(), bg.numpy()[:3])
    with pytest.raises(ValueError):
        reader.trimap_from_plate(cmp.numpy()[0], cmp.numpy())   # one frame takes one plate
    with pytest.raises(ValueError):
        reader.trimap_from_plate(cmp.numpy(), bg.numpy(), hi=3)
    with pytest.raises(TypeError):
        reader.trimap_from_plate(cmp.numpy(), bg.numpy(), r_bg=1.5)


# ---------------------------------------------------------------- FrameStream(trimap="auto"), host side

@pytest.fixture(scope="module")
def models(vgg0):
    from vmatting import unet
    np.random.seed(0)  # (the constructors do not touch the device)
    return unet.UNetVideo(vgg0, dtype="bf16", device="cuda"), unet.UNetImage(vgg0, dtype="bf16", device="cuda")


def test_frame_stream_auto_constructs(models):
    from vmatting import FrameStream, ops
    mv, _ = models
    fs = FrameStream(mv, 32, 48, trimap="auto")
    assert fs.auto and not fs.propagate and fs.trimap and fs.auto_options == ops.PLATE_DEFAULTS
    assert fs._slots is None
    fs = FrameStream(mv, 32, 48, trimap="auto", auto_options={"hi": 60, "r_fg": 0}, out="over", new_bg="per_frame")
    assert fs.auto_options == {"lo": 16, "hi": 60, "r_bg": 4, "r_fg": 0}
    with pytest.raises(ValueError, match="propagate"):
        fs.last_trimap()
    assert not FrameStream(mv, 32, 48).auto and not FrameStream(mv, 32, 48, trimap="propagate").auto


def test_frame_stream_auto_constructor_errors(models):
    from vmatting import FrameStream
    mv, mi = models
    with pytest.raises(ValueError, match="takes 6 channels"):
        FrameStream(mi, 32, 48, trimap="auto")                           # a 6-channel model takes no trimap
    with pytest.raises(ValueError, match="'auto'"):
        FrameStream(mv, 32, 48, trimap="automatic")
    for kw in (dict(), dict(trimap="propagate")):
        with pytest.raises(ValueError, match="auto_options go with"):
            FrameStream(mv, 32, 48, auto_options={"lo": 8}, **kw)        # auto_options without "auto"
    with pytest.raises(ValueError, match="auto_options go with"):
        FrameStream(mi, 32, 48, trimap=False, auto_options={})
    with pytest.raises(ValueError, match="auto_options takes"):
        FrameStream(mv, 32, 48, trimap="auto", auto_options={"low": 8})  # an unknown key
    with pytest.raises(ValueError):
        FrameStream(mv, 32, 48, trimap="auto", auto_options={"lo": 48})
    with pytest.raises(ValueError):
        FrameStream(mv, 32, 48, trimap="auto", auto_options={"r_bg": 33})
    with pytest.raises(TypeError):
        FrameStream(mv, 32, 48, trimap="auto", auto_options={"hi": 48.0})
    for kw in (dict(flow="estimate"), dict(flow="given"), dict(flow_options={"iters": 5})):
        with pytest.raises(ValueError, match="propagate"):
            FrameStream(mv, 32, 48, trimap="auto", **kw)                 # flow / flow_options stay with "propagate"
    with pytest.raises(ValueError):
        FrameStream(mv, 32, 48, trimap="auto", grow=9)                   # grow is checked as ever


def test_frame_stream_auto_check_item(models):
    from vmatting import FrameStream
    mv, _ = models
    h, w, k = 16, 24, 2
    cmp, bg, tri = np.zeros((k, h, w, 3), np.uint8), np.zeros((k, h, w, 3), np.uint8), np.zeros((k, h, w), np.uint8)
    fs = FrameStream(mv, h, w, chunk=2, trimap="auto")
    item = fs.check_item((cmp, bg, None))
    assert item[0] is cmp and item[1] is bg and item[2] is None and item[3] == k
    bad = [(cmp, bg, tri),                                               # a trimap although they are made from the plate
           (cmp, bg), (cmp, bg, None, None),                             # not three entries
           (cmp.astype(np.float32), bg, None), (cmp, None, None), (cmp, bg[:1], None), (cmp[0], bg[0], None),
           (np.zeros((3, h, w, 3), np.uint8), np.zeros((3, h, w, 3), np.uint8), None)]
    for item in bad:
        with pytest.raises((ValueError, TypeError)):
            fs.check_item(item)
        with pytest.raises((ValueError, TypeError)):
            next(fs.run(iter([item])))
        assert fs._slots is None                                         # rejected before anything was allocated
    with pytest.raises(ValueError, match="made from the plate"):
        fs.check_item((cmp, bg, tri))

    plate = FrameStream(mv, h, w, chunk=2, trimap="auto", static_bg=bg[0])
    assert plate.check_item((cmp, None, None))[3] == k
    with pytest.raises(ValueError):
        plate.check_item((cmp, bg, None))

    per_frame = FrameStream(mv, h, w, chunk=2, trimap="auto", out="over", new_bg="per_frame")
    with pytest.raises(ValueError):
        per_frame.check_item((cmp, bg, None))                            # new_bg comes last
    with pytest.raises(ValueError, match="made from the plate"):
        per_frame.check_item((cmp, bg, tri, cmp))
    assert per_frame.check_item((cmp, bg, None, cmp))[4] is cmp
