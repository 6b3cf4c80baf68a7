"""FrameStream(align="fit") on the GPU: the stream equals the stream fed reader.align_plate's plates as per-frame
backgrounds, byte for byte, alone and together with gain="fit", trimap="auto", scale=2, out="over" and smooth="flow"
(which shares its frame pyramids), captured or eager; last_alignment() returns the last chunk's maps; align=None
allocates nothing new."""

import numpy as np
import pytest

import plate_align_ref as ref
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

CHUNK, DEPTH, FRAMES = 3, 2, 5  # two chunks, the last one short
MOVES = (("sub", 1.0), ("one", 0.8), ("id", 1.0), ("rot", 1.25), ("zoom", 1.0))
NEW_BUFFERS = ("a_bg", "align", "align_support")
SIZES = {1: (64, 96), 2: (128, 192)}  # by scale
# 128 x 192 at the default 6 levels has a coarsest level of 8 x 12 pixels, at which the fit of `one` goes astray and ends at
# the identity (tests/test_plate_align_host.py); four levels (16 x 24) fit every frame of the clip
OPTIONS = {(64, 96): {}, (128, 192): {"levels": 4}}


@pytest.fixture(scope="module")
def models(vgg0):
    from vmatting import unet
    np.random.seed(0)
    return unet.UNetVideo(vgg0, dtype="bf16", device="cuda").prepare()


@pytest.fixture(scope="module")
def clips():
    """Per size: one textured plate, five frames that see it through a motion and under a gain of their own behind the
    scenes' disc, painted trimaps, a new plate; and reader.align_plate's plates, maps and supports, frame by frame."""
    from vmatting import reader
    out = {}
    for h, w in SIZES.values():
        scenes = [ref.scene(h, w, m, g, 4) for m, g in MOVES]  # (one seed: one plate)
        plate = scenes[0][1]
        cmp = np.stack([s[0] for s in scenes])
        tri = np.stack([np.where(s[2] == 1, 255, np.where(s[2] == 0, 0, 128)).astype(np.uint8) for s in scenes])
        res = [reader.align_plate(cmp[j], plate, **OPTIONS[h, w]) for j in range(FRAMES)]
        aligned, params = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
        support = np.array([r[2] for r in res], np.int64)
        # the fits are fits: every moved frame's map is within a quarter pixel of the truth, and moves the plate
        for j, (m, _) in enumerate(MOVES):
            full = np.concatenate([params[j], [0]]).astype(np.float32)
            assert ref.corner_error(full, scenes[j][3], h, w) <= 0.25 and support[j] * 4 >= h * w
            assert (m == "id") == np.array_equal(aligned[j], plate) or m == "id"
        new = np.random.RandomState(5).randint(0, 256, (h, w, 3)).astype(np.uint8)
        out[h, w] = {"cmp": cmp, "plate": plate, "tri": tri, "new": new, "aligned": aligned, "params": params,
                     "support": support}
    return out


def chunks():
    return [(i, min(i + CHUNK, FRAMES)) for i in range(0, FRAMES, CHUNK)]


def run_stream(model, clip, bg, static, trimap="auto", out="u8", graph=False, scale=1, **kw):
    """The clip through a FrameStream: ``bg`` is the static plate ([h,w,3]) or the per-frame backgrounds."""
    from vmatting import FrameStream
    h, w = clip["plate"].shape[:2]
    if out == "over":
        kw["new_bg"] = clip["new"]
    fs = FrameStream(model, h, w, chunk=CHUNK, depth=DEPTH, trimap=trimap, out=out, graph=graph,
                     static_bg=bg if static else None, scale=scale, **kw)
    items = [(clip["cmp"][a:b], None if static else bg[a:b], clip["tri"][a:b] if trimap is True else None)
             for a, b in chunks()]
    got = list(fs.run(items))
    assert [g.shape[0] for g in got] == [b - a for a, b in chunks()] and fs.overflowed_chunks == []
    return np.concatenate(got), fs


@pytest.mark.parametrize("graph,trimap,out,scale,extra", [
    (True, True, "u8", 1, {}), (False, True, "u8", 1, {}), (True, True, "u16", 1, {"gain": "fit"}),
    (False, "auto", "u8", 1, {}), (True, "auto", "bgra", 1, {"gain": "fit", "auto_fill": True}),
    (True, True, "u8", 2, {}), (False, "auto", "over", 1, {}), (True, True, "over", 1, {}),
    (True, True, "f32", 1, {"smooth": "flow"}), (False, "auto", "u8", 1, {"smooth": "flow"}),
    (True, True, "u8", 1, {"smooth": "flow", "flow_options": {"levels": 3}})])
def test_stream_equals_the_stream_fed_aligned_plates(models, clips, graph, trimap, out, scale, extra):
    clip = clips[SIZES[scale]]
    want, _ = run_stream(models, clip, clip["aligned"], False, trimap, out, False, scale, **extra)
    got, fs = run_stream(models, clip, clip["plate"], True, trimap, out, graph, scale, align="fit",
                         align_options=OPTIONS[SIZES[scale]] or None, **extra)
    assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)
    # and the alignment matters: the stream on the plate as given differs
    plain, _ = run_stream(models, clip, clip["plate"], True, trimap, out, False, scale, **extra)
    assert not np.array_equal(plain, want)
    params, support = fs.last_alignment()
    a, b = chunks()[-1]
    assert params.dtype == np.float32 and params.shape == (b - a, 7) and support.shape == (b - a,)
    assert np.array_equal(params, clip["params"][a:b]) and np.array_equal(support, clip["support"][a:b])
    slot = fs._slots[0]
    h, w = SIZES[scale]
    assert tuple(slot.a_bg.shape) == (CHUNK, h, w, 3) and tuple(slot.align.shape) == (CHUNK, 8)
    assert fs._plate_lo is None and tuple(fs._align_bg_rows.shape)[0] == 1
    # the flow estimate's pyramids are the alignment's where the levels agree, and only there
    shared = "smooth" in extra and extra.get("flow_options", {}).get("levels", 6) == 6
    assert (fs._align_rows is None) == shared
    if graph and out == "u8" and scale == 1 and not extra:  # the object runs again, over the same graphs
        again = np.concatenate(list(fs.run([(clip["cmp"][a:b], None, clip["tri"][a:b]) for a, b in chunks()])))
        assert np.array_equal(again, want)


def test_per_frame_backgrounds_are_aligned_frame_by_frame(models, clips):
    """Per-frame ``bg`` items get a pyramid each; here every frame's background is the plate moved once more."""
    from vmatting import reader
    clip = clips[SIZES[1]]
    bgs = np.stack([np.roll(clip["plate"], (j % 2, -(j % 3)), (0, 1)) for j in range(FRAMES)])
    aligned = np.stack([reader.align_plate(clip["cmp"][j], bgs[j])[0] for j in range(FRAMES)])
    want, _ = run_stream(models, clip, aligned, False, True, "u8", False)
    for graph in (True, False):
        got, fs = run_stream(models, clip, bgs, False, True, "u8", graph, align="fit", align_options={"iters": 4})
        assert np.array_equal(got, want) and tuple(fs._align_bg_rows.shape)[0] == CHUNK


def test_align_options_reach_the_kernels(models, clips):
    from vmatting import reader
    clip, opts = clips[SIZES[1]], {"tol": 8.0, "levels": 2, "iters": 2}
    res = [reader.align_plate(clip["cmp"][j], clip["plate"], **opts) for j in range(FRAMES)]
    assert not np.array_equal(np.stack([r[1] for r in res]), clip["params"])
    want, _ = run_stream(models, clip, np.stack([r[0] for r in res]), False, True, "u8", False)
    got, fs = run_stream(models, clip, clip["plate"], True, True, "u8", True, align="fit", align_options=opts)
    assert np.array_equal(got, want) and np.array_equal(fs.last_alignment()[0], np.stack([r[1] for r in res])[3:])


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_no_align_is_the_stream_as_it_was(models, clips, graph):
    clip, res = clips[SIZES[1]], []
    for kw in ({}, {"align": None}):
        got, fs = run_stream(models, clip, clip["plate"], True, "auto", "u16", graph, **kw)
        res.append(got)
        assert fs.align is None and fs._align_work is None and fs._align_rows is None and fs._align_bg_rows is None
        assert fs._align_pyr_work is None and fs._align_last is None
        for s in fs._slots:
            assert not any(hasattr(s, name) for name in NEW_BUFFERS)
    assert np.array_equal(res[0], res[1])


def test_reader_helpers(clips):
    """reader.align_plate is the restatement's resampling of its own map, and close to the restatement's map;
    reader.trimap_from_plate(align="fit") is the plate trimap of the aligned plates."""
    import trimap_plate_ref as tp
    from vmatting import reader
    clip = clips[SIZES[1]]
    h, w = SIZES[1]
    for j in (0, 3):
        plate, params, support = reader.align_plate(clip["cmp"][j], clip["plate"])
        assert params.dtype == np.float32 and params.shape == (7,) and isinstance(support, int)
        full = np.concatenate([params, [0]]).astype(np.float32)
        assert np.array_equal(plate, ref.apply(clip["plate"], full))
        want, wsup = ref.fit_frames(clip["cmp"][j], clip["plate"])
        assert ref.corner_error(full, want, h, w) <= 1.0 / 1024 and abs(support - wsup) <= 2
    got = reader.trimap_from_plate(clip["cmp"], clip["plate"], align="fit")
    assert np.array_equal(got, tp.trimaps(clip["cmp"], clip["aligned"], **tp.DEFAULTS))
    assert not np.array_equal(got, reader.trimap_from_plate(clip["cmp"], clip["plate"]))
    one = reader.trimap_from_plate(clip["cmp"][1], clip["plate"], align="fit", gain="fit", fill=True)
    gained = reader.match_plate(clip["cmp"][1], clip["aligned"][1])[0]
    assert np.array_equal(one, reader.fill_enclosed(tp.trimap(clip["cmp"][1], gained, **tp.DEFAULTS)))
