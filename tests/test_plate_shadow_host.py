"""CPU checks of the shadow-tolerant trimap from the background plate: the numpy restatement (tests/plate_shadow_ref.py)
against the definition read pixel by pixel in Python integers, what the defaults give on a synthetic shadow, the
documented grey-on-grey limit, and the host-side argument checks of the C entry, the wrappers and
FrameStream(shadow="chroma"), which all happen before any GPU call."""

import os
import re

import numpy as np
import pytest
import torch

import plate_shadow_ref as ref
import trimap_plate_ref as plain

SEEDS = range(20)


def brute_distance(cmp, bg, floor, ceil, dark):
    """include/vmatting.h's d', d and cross, one pixel at a time, in Python integers."""
    h, w = cmp.shape[:2]
    dp, d, cross = (np.zeros((h, w), object) for _ in range(3))
    for y in range(h):
        for x in range(w):
            i, e = [int(v) for v in cmp[y, x]], [int(v) for v in bg[y, x]]
            d[y, x] = sum((a - b) ** 2 for a, b in zip(i, e))
            ee, ie, ii = sum(b * b for b in e), sum(a * b for a, b in zip(i, e)), sum(a * a for a in i)
            cross[y, x] = ii * ee - ie * ie
            ok = ee >= max(3 * dark * dark, 1) and floor * ee <= 256 * ie <= ceil * ee
            dp[y, x] = cross[y, x] // ee if ok else d[y, x]
    return dp, d, cross


@pytest.mark.parametrize("kind", sorted(ref.PAIRS))
def test_restatement_equals_the_definition(kind):
    h, w = 9, 13
    cmp, bg = ref.PAIRS[kind](h, w, seed=3)
    for triple in ref.TRIPLES:
        want, d, cross = brute_distance(cmp, bg, *triple)
        got = ref.distance_shadow(cmp, bg, *triple)
        assert got.dtype == np.int64 and (got == want).all(), triple
        assert (got <= d).all() and (got >= 0).all()                      # d' <= d everywhere
        assert (cross >= 0).all() and (ref.terms(cmp, bg)[4] == cross).all()
        D = np.zeros((h, w), np.int64)                                    # the box sum with clamped coordinates
        for y in range(h):
            for x in range(w):
                D[y, x] = sum(int(want[min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)])
                              for dy in (-1, 0, 1) for dx in (-1, 0, 1))
        opts = dict(zip(ref.DEFAULTS, triple))
        assert np.array_equal(ref.box_sum(cmp, bg, opts), D)
        for lo, hi, r_bg, r_fg in ((16, 48, 1, 2), (8, 30, 0, 0)):
            assert np.array_equal(ref.trimap(cmp, bg, lo, hi, r_bg, r_fg, shadow=opts),
                                  ref.from_box_sum(D, lo, hi, r_bg, r_fg))


def test_distance_bounds_on_larger_inputs():
    """d' <= d and cross >= 0 where cross passes 2^32, and a quotient at the top of its range."""
    for kind in ref.PAIRS:
        cmp, bg = ref.PAIRS[kind](70, 90, seed=11)
        d, ee, ie, ii, cross = ref.terms(cmp, bg)
        assert (cross >= 0).all()
        for triple in ref.TRIPLES:
            assert (ref.distance_shadow(cmp, bg, *triple) <= d).all()
    assert ref.terms(*plain.noise_pair(70, 90, seed=11))[4].max() > 2 ** 32
    cmp, bg = np.array([[[255, 255, 0]]], np.uint8), np.array([[[0, 1, 255]]], np.uint8)
    assert ref.distance_shadow(cmp, bg, 1, 512, 0)[0, 0] == (2 * 255 ** 2 * 65026 - 255 ** 2) // 65026 == 130049
    cmp, bg = np.full((1, 1, 3), 255, np.uint8), np.full((1, 1, 3), 255, np.uint8)
    assert ref.distance_shadow(cmp, bg, 256, 256, 255)[0, 0] == 0         # the one plate (256, 256, 255) trusts
    assert ref.in_range(*ref.terms(cmp, bg)[1:3], 256, 256, 255).all()


def test_inputs_cover_what_they_claim():
    """Both branches of d' on the inputs of the GPU tests, at their smallest full-size shape."""
    share = {kind: [ref.in_range(*ref.terms(*ref.PAIRS[kind](70, 90, seed=11))[1:3], *t).mean() for t in ref.TRIPLES]
             for kind in ref.PAIRS}
    assert 0.45 <= share["noise"][0] <= 0.60 and 0.45 <= share["ratio"][0] <= 0.60
    assert any(0.05 <= v <= 0.95 for v in share["dark"])
    cmp, bg = ref.dark_pair(70, 90, seed=11)
    assert (bg.reshape(-1, 3).max(1) == 0).sum() > 100 and bg.max() == 40 and cmp.max() == 40
    cmp, bg = ref.ratio_pair(70, 90, seed=11)
    assert set(np.unique(ref.trimap(cmp, bg, 8, 30, 0, 0, shadow={})).tolist()) == {0, 128, 255}


def test_no_shadow_is_the_plain_trimap():
    for kind in ref.PAIRS:
        cmp, bg = ref.PAIRS[kind](40, 60, seed=2)
        assert np.array_equal(ref.trimap(cmp, bg, **plain.DEFAULTS), plain.trimap(cmp, bg, **plain.DEFAULTS))
        assert np.array_equal(ref.trimap(cmp, bg, 8, 30, 1, 2, shadow=None), plain.trimap(cmp, bg, 8, 30, 1, 2))
    cmp, bg = np.stack([plain.noise_pair(9, 13, s)[0] for s in range(2)]), plain.noise_pair(9, 13, 5)[1]
    assert np.array_equal(ref.trimaps(cmp, bg, lo=100, hi=200), plain.trimaps(cmp, bg, lo=100, hi=200))


# ---------------------------------------------------------------- the synthetic claims

@pytest.fixture(scope="module")
def shadowed():
    """Per strength s and seed: (alpha, the shadow's core, the plain trimap, the shadow trimap), all with the defaults."""
    out = {}
    for s in (0.8, 0.6):
        for seed in SEEDS:
            frame, plate, alpha, m = ref.shadow_scene(seed, s)
            assert frame.shape == (96, 160, 3)
            out[s, seed] = (alpha, (m >= 1) & (alpha == 0), plain.trimap(frame, plate, **plain.DEFAULTS),
                            ref.trimap(frame, plate, shadow=ref.DEFAULTS, **plain.DEFAULTS))
    return out


@pytest.mark.parametrize("s", [0.8, 0.6])
def test_defaults_hold_a_synthetic_shadow(shadowed, s):
    """The plain trimap labels none of the shadow's core background, the shadow trimap at least 0.6 of it in every seed
    (a numpy prototype measured 0.72-0.84: the 0.6 is a floor under the worst seed), and no certain label is wrong."""
    for seed in SEEDS:
        alpha, core, t_plain, t_shadow = shadowed[s, seed]
        assert core.sum() > 500
        assert (t_plain[core] == 0).mean() == 0.0, seed
        assert (t_shadow[core] == 0).mean() >= 0.6, seed
        assert not ((t_shadow == 0) & (alpha > 0)).any(), seed
        assert not ((t_shadow == 255) & (alpha < 1)).any(), seed


def test_plain_mode_calls_a_deep_shadow_foreground(shadowed):
    """At s = 0.6 the plain distance passes hi: background pixels become sure foreground in some seed."""
    assert max(((shadowed[0.6, seed][2] == 255) & (shadowed[0.6, seed][0] == 0)).sum() for seed in SEEDS) >= 1


def test_scene_is_the_plain_scene_without_a_shadow():
    frame, plate, alpha, m = ref.shadow_scene(4, 1.0)
    f0, p0, a0 = plain.scene(4)
    assert np.array_equal(frame, f0) and np.array_equal(plate, p0) and np.array_equal(alpha, a0)
    assert 0 < (m >= 1).sum() < m.size and m.min() == 0


@pytest.mark.parametrize("seed", SEEDS)
def test_defaults_stay_sound_without_a_shadow(seed):
    """The five conditions test_trimap_plate_host pins for the plain mode on the unshadowed composite."""
    frame, plate, alpha = plain.scene(seed)
    out = ref.trimap(frame, plate, shadow=ref.DEFAULTS, **plain.DEFAULTS)
    assert not ((out == 0) & (alpha > 0)).any()
    assert not ((out == 255) & (alpha < 1)).any()
    assert (out == 128).mean() <= 0.30
    assert (out[alpha == 1] == 255).mean() >= 0.45
    assert (out[alpha == 0] == 0).mean() >= 0.80


def test_grey_on_grey_passes_as_shadow():
    """The documented limit: a per-pixel colour test cannot tell a darker grey subject from the plate in shadow."""
    frame, plate, square = ref.grey_scene()
    assert (ref.trimap(frame, plate, shadow=ref.DEFAULTS, **plain.DEFAULTS)[square] == 0).all()
    assert not (plain.trimap(frame, plate, **plain.DEFAULTS)[square] == 0).any()


# ---------------------------------------------------------------- options

def test_check_shadow_options():
    from vmatting import ops
    assert ops.SHADOW_DEFAULTS == ref.DEFAULTS and list(ops.SHADOW_DEFAULTS) == ["floor", "ceil", "dark"]
    assert list(ops.PLATE_DEFAULTS) == ["lo", "hi", "r_bg", "r_fg"]
    assert ops.SHADOW_CHROMA == "chroma"
    assert ops.check_shadow_options("t") == (128, 256, 32)
    for triple in ref.TRIPLES + [(1, 256, 0), (256, 512, 255)]:
        assert ops.check_shadow_options("t", *triple) == triple
    assert ops.check_shadow_options("t", np.int32(5), np.int64(300), np.uint8(7)) == (5, 300, 7)
    good = dict(ops.SHADOW_DEFAULTS)
    for key in good:
        for v in (1.0, "1", None, True):
            with pytest.raises(TypeError, match="t: %s must be an integer" % key):
                ops.check_shadow_options("t", **dict(good, **{key: v}))
    for change in (dict(floor=0), dict(floor=257), dict(floor=-1), dict(ceil=255), dict(ceil=513), dict(dark=-1),
                   dict(dark=256), dict(floor=300, ceil=280), dict(floor=200, ceil=100)):
        with pytest.raises(ValueError):
            ops.check_shadow_options("t", **dict(good, **change))
    with pytest.raises(ValueError, match="floor <= ceil"):
        ops.check_shadow_options("t", floor=300, ceil=280)
    assert ops.shadow_options("t", None) == ref.DEFAULTS
    assert ops.shadow_options("t", {"dark": 0}) == {"floor": 128, "ceil": 256, "dark": 0}
    with pytest.raises(ValueError, match="t takes"):
        ops.shadow_options("t", {"flor": 100})
    assert ops.check_shadow_mode("t", None, None) is None
    assert ops.check_shadow_mode("t", "chroma", None) == ref.DEFAULTS
    assert ops.check_shadow_mode("t", "chroma", {"floor": 100}) == {"floor": 100, "ceil": 256, "dark": 32}
    for mode in ("Chroma", "fit", True, 1):
        with pytest.raises(ValueError, match="shadow must be None or 'chroma'"):
            ops.check_shadow_mode("t", mode, None)
    with pytest.raises(ValueError, match="shadow_options go with shadow='chroma'"):
        ops.check_shadow_mode("t", None, {})
    with pytest.raises(ValueError, match="t: shadow_options takes"):
        ops.check_shadow_mode("t", "chroma", {"level": 3})


def test_wrappers_check_on_the_host():
    from vmatting import ops, reader
    cmp, bg = torch.zeros((2, 4, 6, 3), dtype=torch.uint8), torch.zeros((4, 6, 3), dtype=torch.uint8)
    with pytest.raises(TypeError):
        ops.trimap_from_plate(cmp, bg, shadow={})                          # right tensors, but on the host
    with pytest.raises(ValueError, match="floor"):
        ops.trimap_from_plate(cmp, bg, shadow={"floor": 0})
    with pytest.raises(ValueError, match="takes"):
        ops.trimap_from_plate(cmp, bg, shadow={"light": 1})
    with pytest.raises(TypeError, match="dark must be an integer"):
        ops.trimap_from_plate(cmp, bg, shadow={"dark": 1.5})
    with pytest.raises((TypeError, ValueError)):
        ops.trimap_from_plate(cmp, bg, shadow="chroma")                    # ops takes the options, not the mode
    c, b = cmp.numpy(), bg.numpy()
    with pytest.raises(ValueError, match="shadow must be None or 'chroma'"):
        reader.trimap_from_plate(c, b, shadow="luma")
    with pytest.raises(ValueError, match="shadow_options go with"):
        reader.trimap_from_plate(c, b, shadow_options={"floor": 100})
    with pytest.raises(ValueError, match="shadow_options takes"):
        reader.trimap_from_plate(c, b, shadow="chroma", shadow_options={"low": 1})
    with pytest.raises(ValueError):
        reader.trimap_from_plate(c, b, shadow="chroma", shadow_options={"ceil": 200})
    with pytest.raises(TypeError):
        reader.trimap_from_plate(c, b, shadow="chroma", shadow_options={"floor": 100.0})
    with pytest.raises(ValueError):
        reader.trimap_from_plate(c, b[:3], shadow="chroma")                # the shapes are checked as ever


@pytest.fixture(scope="module")
def models(vgg0):
    from vmatting import unet
    np.random.seed(0)  # (the constructors do not touch the device)
    return unet.UNetVideo(vgg0, dtype="bf16", device="cuda"), unet.UNetImage(vgg0, dtype="bf16", device="cuda")


def test_frame_stream_shadow_constructs(models):
    from vmatting import FrameStream, ops
    mv, _ = models
    assert FrameStream(mv, 32, 48, trimap="auto").shadow is None and FrameStream(mv, 32, 48).shadow is None
    fs = FrameStream(mv, 32, 48, trimap="auto", shadow="chroma")
    assert fs.auto and fs.shadow == ops.SHADOW_DEFAULTS and fs.auto_options == ops.PLATE_DEFAULTS and fs._slots is None
    fs = FrameStream(mv, 32, 48, trimap="auto", shadow="chroma", shadow_options={"floor": 100, "dark": 0},
                     auto_fill=True, gain="fit", align="fit", smooth="flow", scale=2, out="over", new_bg="per_frame")
    assert fs.shadow == {"floor": 100, "ceil": 256, "dark": 0}


def test_frame_stream_shadow_constructor_errors(models):
    from vmatting import FrameStream
    mv, mi = models
    for kw in (dict(), dict(trimap="propagate"), dict(trimap=True)):
        with pytest.raises(ValueError, match="shadow and shadow_options go with trimap='auto'"):
            FrameStream(mv, 32, 48, shadow="chroma", **kw)
        with pytest.raises(ValueError, match="shadow and shadow_options go with trimap='auto'"):
            FrameStream(mv, 32, 48, shadow_options={}, **kw)
    with pytest.raises(ValueError, match="go with trimap='auto'"):
        FrameStream(mi, 32, 48, trimap=False, shadow="chroma")
    with pytest.raises(ValueError, match="shadow_options go with shadow='chroma'"):
        FrameStream(mv, 32, 48, trimap="auto", shadow_options={"floor": 100})
    with pytest.raises(ValueError, match="shadow must be None or 'chroma'"):
        FrameStream(mv, 32, 48, trimap="auto", shadow="fit")
    with pytest.raises(ValueError, match="shadow_options takes"):
        FrameStream(mv, 32, 48, trimap="auto", shadow="chroma", shadow_options={"lo": 8})
    with pytest.raises(ValueError):
        FrameStream(mv, 32, 48, trimap="auto", shadow="chroma", shadow_options={"floor": 257})
    with pytest.raises(ValueError):
        FrameStream(mv, 32, 48, trimap="auto", shadow="chroma", shadow_options={"ceil": 255})
    with pytest.raises(ValueError):
        FrameStream(mv, 32, 48, trimap="auto", shadow="chroma", shadow_options={"dark": 256})
    with pytest.raises(TypeError):
        FrameStream(mv, 32, 48, trimap="auto", shadow="chroma", shadow_options={"dark": 3.0})


def test_other_streams_do_not_take_it():
    import inspect

    from vmatting import ClipStream, PlateEstimator
    from vmatting.video import VideoMatter
    for cls in (ClipStream, VideoMatter, PlateEstimator):
        assert "shadow" not in inspect.signature(cls.__init__).parameters


# ---------------------------------------------------------------- the C entry point, on the host

ORDER = ("cmp", "bg", "nb", "n", "h", "w", "lo", "hi", "r_bg", "r_fg", "floor", "ceil", "dark", "out", "work")


def test_symbol_is_in_the_table_and_the_header():
    from vmatting import _lib
    rows = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    res, args = rows["vm_trimap_from_plate_shadow"]
    plain_args = rows["vm_trimap_from_plate"][1]
    assert res is rows["vm_trimap_from_plate"][0] and len(args) == len(ORDER) + 1 == len(plain_args) + 3
    assert args[:10] == plain_args[:10] and args[13:] == plain_args[10:] and len(set(args[10:13])) == 1
    assert hasattr(_lib.lib(), "vm_trimap_from_plate_shadow")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vmatting.h")).read()
    decl = re.search(r"int vm_trimap_from_plate_shadow\(([^;]*)\);", header).group(1)
    names = [p.split()[-1].lstrip("*") for p in decl.replace("\n", " ").split(",")]
    assert names == list(ORDER) + ["stream"]
    assert _lib.ABI_VERSION == 1 and _lib.lib().vm_abi_version() == 1


def test_c_entry_rejects_bad_arguments():
    from vmatting import _lib
    lib = _lib.lib()
    P, Q, W = 4096, 8192, 64  # non-null addresses: validation never dereferences them
    ok = dict(cmp=P, bg=Q, nb=1, n=2, h=5, w=5, lo=16, hi=48, r_bg=4, r_fg=8, floor=128, ceil=256, dark=32, out=16384,
              work=W)
    bad = [dict(floor=0), dict(floor=-1), dict(floor=257), dict(ceil=255), dict(ceil=513), dict(floor=300, ceil=300),
           dict(floor=300, ceil=280), dict(dark=-1), dict(dark=256),
           dict(cmp=None), dict(bg=None), dict(out=None), dict(work=None),
           dict(n=0), dict(h=0), dict(w=0), dict(h=-1), dict(n=1 << 15, h=1 << 8, w=1 << 8),   # 2^31 pixels
           dict(nb=0), dict(nb=3),
           dict(lo=-1), dict(lo=48), dict(hi=443), dict(r_bg=-1), dict(r_bg=33), dict(r_fg=-1), dict(r_fg=33),
           dict(out=P), dict(out=Q), dict(out=P + 149), dict(out=Q + 74), dict(out=P - 1),      # out overlaps cmp / bg
           dict(work=72)]
    for change in bad:
        args = dict(ok, **change)
        rc = lib.vm_trimap_from_plate_shadow(*[args[k] for k in ORDER], None)
        assert rc == _lib.VM_EINVAL, change
        assert b"trimap_from_plate_shadow" in lib.vm_last_error()
    for change, word in ((dict(floor=0), b"floor 0"), (dict(ceil=513), b"ceil 513"), (dict(dark=256), b"dark 256")):
        args = dict(ok, **change)
        assert lib.vm_trimap_from_plate_shadow(*[args[k] for k in ORDER], None) == _lib.VM_EINVAL
        assert word in lib.vm_last_error()
