"""CPU checks of the component labelling and the enclosed-background fill: the numpy restatement
(tests/trimap_fill_ref.py, a breadth-first flood) against scipy.ndimage.label and against a per-pixel loop, what the fill
buys on the synthetic composite the plate defaults are pinned on, and the host-side argument checks of the two C
entries, the wrappers and FrameStream(auto_fill=...), which all happen before any GPU call."""

import numpy as np
import pytest
import torch

import trimap_fill_ref as ref
import trimap_plate_ref as plate_ref


# ---------------------------------------------------------------- the restatement

@pytest.mark.parametrize("connectivity", [4, 8])
def test_restatement_equals_scipy(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)
    for h, w in ((40, 60), (33, 7), (1, 9), (9, 1), (3, 3)):
        for p in ref.P_ZERO:
            for tri in ref.random_trimaps(2, h, w, p, seed=h + w):
                lab, count = ndimage.label(tri == 0, structure=structure)
                want = np.full((h, w), -1, np.int32)
                index = np.arange(h * w).reshape(h, w)
                for c in range(1, count + 1):                 # every scipy label -> its component's smallest index
                    want[lab == c] = index[lab == c].min()
                got = ref.label(tri, 0, connectivity)
                assert np.array_equal(got, want), (h, w, p)
                if connectivity == 4:
                    # the fill from scipy's labels: bincount areas, and the labels met on the four border lines
                    area = np.bincount(lab.ravel(), minlength=count + 1)
                    edge = np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))
                    for cap in (0, 3):
                        fill = np.ones(count + 1, bool)
                        fill[0] = False
                        fill[edge] = False
                        if cap:
                            fill &= area <= cap
                        expect = tri.copy()
                        if h >= 3 and w >= 3:
                            expect[fill[lab]] = 128
                        assert np.array_equal(ref.fill(tri, cap), expect), (h, w, p, cap)


def brute_labels(mask, value, connectivity):
    """Relabel to a fixpoint, one pixel at a time: every set pixel takes the smallest label among itself and its set
    neighbours."""
    h, w = mask.shape
    steps = ref.N4 if connectivity == 4 else ref.N8
    lab = [[y * w + x if mask[y, x] == value else -1 for x in range(w)] for y in range(h)]
    changed = True
    while changed:
        changed = False
        for y in range(h):
            for x in range(w):
                if lab[y][x] < 0:
                    continue
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w and 0 <= lab[yy][xx] < lab[y][x]:
                        lab[y][x] = lab[yy][xx]
                        changed = True
    return np.array(lab, np.int32).reshape(h, w)


def brute_fill(tri, max_area):
    h, w = tri.shape
    lab = brute_labels(tri, 0, 4)
    out = tri.copy()
    for y in range(h):
        for x in range(w):
            if lab[y, x] < 0:
                continue
            members = [(yy, xx) for yy in range(h) for xx in range(w) if lab[yy, xx] == lab[y, x]]
            enclosed = all(0 < yy < h - 1 and 0 < xx < w - 1 for yy, xx in members)
            if enclosed and (max_area == 0 or len(members) <= max_area):
                out[y, x] = 128
    return out


@pytest.mark.parametrize("shape", [(7, 9), (3, 3), (2, 5), (1, 6), (5, 1), (1, 1)])
def test_restatement_equals_the_definition(shape):
    h, w = shape
    for p in ref.P_ZERO:
        for tri in ref.random_trimaps(3, h, w, p, seed=7):
            for connectivity in (4, 8):
                for value in (0, 128):
                    assert np.array_equal(ref.label(tri, value, connectivity), brute_labels(tri, value, connectivity))
            for cap in (0, 1, 2):
                assert np.array_equal(ref.fill(tri, cap), brute_fill(tri, cap)), (p, cap)


def test_patterns_are_what_they_claim():
    h, w = 133, 261
    for make in (ref.serpentine, ref.spiral):
        closed, opened = make(h, w), make(h, w, open_end=True)
        assert ref.census(closed)[:2] == (1, 1) and ref.census(opened)[:2] == (1, 0)
        assert (closed == 0).sum() + 1 == (opened == 0).sum() > h * w // 3
        assert (ref.fill(closed) != 0).all() and np.array_equal(ref.fill(opened), opened)
    assert ref.census(ref.comb(h, w))[:2] == (1, 1)
    board = ref.checkerboard(70, 90)
    assert len(np.unique(ref.label(board, 0, 4))) == 1 + (board == 0).sum()
    assert len(np.unique(ref.label(board, 0, 8))) == 2
    squares = ref.corner_squares(70, 90)
    assert ref.census(squares)[:2] == (2, 1) and len(np.unique(ref.label(squares, 0, 8))) == 2
    filled = ref.fill(squares)
    assert (filled[5:10, 5:10] == 128).all() and (filled[0:5, 0:5] == 0).all()
    assert ref.census(ref.rings(70, 90))[:2] == (3, 3)
    zero = np.zeros((70, 90), np.uint8)
    assert np.array_equal(ref.fill(zero), zero)
    assert (ref.fill(ref.framed_zero(70, 90)) == 128).all()
    for where in ("tl", "tr", "bl", "br", "mid"):
        t = ref.one_pixel_touch(70, 90, where)
        border = np.ones((70, 90), bool)
        border[1:-1, 1:-1] = False
        assert ((t == 0) & border).sum() == 1 and ref.census(t)[:2] == (1, 0)
        assert np.array_equal(ref.fill(t), t)
        if where != "mid":
            t = ref.one_pixel_touch(70, 90, where, diagonal=True)
            assert ref.census(t)[:2] == (2, 1) and (ref.fill(t)[1:-1, 1:-1] == 128).all()
    odd = ref.odd_bytes(70, 90)
    assert len(np.unique(odd)) == 256 and ((ref.fill(odd) != odd) == ((odd == 0) & (ref.fill(odd) == 128))).all()
    areas = ref.area_squares(70, 90)
    lab = ref.label(areas, 0, 4)
    assert sorted(np.bincount(lab[lab >= 0])[np.unique(lab[lab >= 0])].tolist()) == [1, 1, 1, 24, 25, 26]
    assert (ref.fill(areas, 25) == 0).sum() == 26 and (ref.fill(areas, 1) == 0).sum() == 75
    assert (ref.fill(areas) == 0).sum() == 0


def patched_scene(seed, patch=25):
    """trimap_plate_ref.scene with a patch x patch square at the disc's centre overwritten by plate colour plus
    sigma = 4 noise: opaque foreground that matches the plate."""
    frame, plate, alpha = plate_ref.scene(seed)
    h, w = alpha.shape
    y, x = np.mgrid[:h, :w].astype(np.float64)
    clean = np.stack([60 + 40 * np.sin(x / 9), 90 + 30 * np.cos(y / 7), 120 + 0 * x], -1)
    noise = np.random.default_rng(1000 + seed).normal(0, 4.0, (patch, patch, 3))
    y0, x0 = 48 - patch // 2, 80 - patch // 2
    frame = frame.copy()
    frame[y0:y0 + patch, x0:x0 + patch] = np.clip(np.rint(clean[y0:y0 + patch, x0:x0 + patch] + noise), 0, 255)
    return frame, plate, alpha


@pytest.mark.parametrize("seed", range(20))
def test_fill_is_sound_on_a_synthetic_composite(seed):
    """The defaults label a plate-coloured patch of opaque foreground sure background; the fill turns all of it unknown
    and nothing else wrong.  The restatement gave, over these seeds: 4500 such pixels without the fill, none with it,
    and an unknown share of at most 0.292."""
    frame, plate, alpha = patched_scene(seed)
    plain = plate_ref.trimap(frame, plate, **plate_ref.DEFAULTS)
    wrong = ((plain == 0) & (alpha == 1)).sum()
    assert wrong > 0
    out = ref.fill(plain)
    assert not ((out == 0) & (alpha > 0)).any()
    assert not ((out == 255) & (alpha < 1)).any()
    assert (out == 128).mean() <= 0.30
    assert ((out != plain) <= (plain == 0)).all()


# ---------------------------------------------------------------- the C entry points and the wrappers, on the host

def test_check_fill():
    from vmatting import ops
    assert ops.check_fill("t", None) is None and ops.check_fill("t", False) is None
    assert ops.check_fill("t", True) == 0 and ops.check_fill("t", True) is not True
    assert ops.check_fill("t", 1) == 1 and ops.check_fill("t", np.int64(4096)) == 4096
    assert type(ops.check_fill("t", np.int32(7))) is int
    for bad in (0, -1, -4096, 1.0, 2.5, "1", (1,)):
        with pytest.raises(ValueError, match="t: fill"):
            ops.check_fill("t", bad)


def test_label_entry_rejects_bad_arguments():
    from vmatting import _lib
    lib = _lib.lib()
    M, L = 4096, 65536  # non-null addresses: validation never dereferences them
    ok = dict(mask=M, n=2, h=5, w=7, value=0, connectivity=4, labels=L)
    bad = [dict(mask=None), dict(labels=None), dict(n=0), dict(h=0), dict(w=0), dict(w=-3),
           dict(n=1 << 15, h=1 << 8, w=1 << 8),                                   # 2^31 pixels
           dict(value=-1), dict(value=256), dict(connectivity=0), dict(connectivity=6), dict(connectivity=-4),
           dict(labels=L + 1), dict(labels=L + 2),                                # misaligned
           dict(labels=M), dict(labels=M + 68), dict(labels=M - 276), dict(mask=L + 279)]   # labels overlap mask
    order = ("mask", "n", "h", "w", "value", "connectivity", "labels")
    for change in bad:
        args = dict(ok, **change)
        assert lib.vm_components_label(*[args[k] for k in order], None) == _lib.VM_EINVAL, change
        assert b"components_label" in lib.vm_last_error()
    assert lib.vm_abi_version() == 1


def test_fill_entry_rejects_bad_arguments():
    from vmatting import _lib
    lib = _lib.lib()
    T, O, W = 4096, 8192, 65536
    ok = dict(trimap=T, n=2, h=5, w=7, max_area=0, out=O, work=W)      # 70 pixels, 560 bytes of workspace
    bad = [dict(trimap=None), dict(out=None), dict(work=None), dict(n=0), dict(h=0), dict(w=0), dict(h=-1),
           dict(n=1 << 15, h=1 << 8, w=1 << 8), dict(max_area=-1), dict(max_area=-4096),
           dict(work=W + 8), dict(work=W + 4), dict(work=W + 1),                  # misaligned
           dict(out=T + 1), dict(out=T + 69), dict(out=T - 69),                   # out overlaps trimap without being it
           dict(work=T - 544), dict(work=O + 64), dict(trimap=W + 559, out=W + 559), dict(out=W + 16)]
    order = ("trimap", "n", "h", "w", "max_area", "out", "work")
    for change in bad:
        args = dict(ok, **change)
        assert lib.vm_trimap_fill_enclosed(*[args[k] for k in order], None) == _lib.VM_EINVAL, change
        assert b"trimap_fill_enclosed" in lib.vm_last_error()
    for shape in ((0, 5, 5), (1, 0, 5), (1, 5, -1), (1 << 15, 1 << 8, 1 << 8)):
        assert lib.vm_trimap_fill_enclosed_workspace_bytes(*shape) == 0
    # labels, and an int32 per pixel for the border flag and the area at the roots
    assert lib.vm_trimap_fill_enclosed_workspace_bytes(1, 1080, 1920) == 8 * 1080 * 1920
    assert lib.vm_trimap_fill_enclosed_workspace_bytes(8, 3, 65) == 8 * 8 * 3 * 65
    assert lib.vm_trimap_fill_enclosed_workspace_bytes(2, 1, 1) == 16
    assert lib.vm_trimap_fill_enclosed_workspace_bytes(1 << 11, 1 << 10, (1 << 10) - 1) == 8 * (2 ** 31 - 2 ** 21)
    assert lib.vm_abi_version() == 1


def test_wrappers_check_on_the_host():
    from vmatting import ops, reader
    tri = torch.zeros((2, 4, 6), dtype=torch.uint8)
    for call in (ops.label_components, ops.trimap_fill_enclosed):
        with pytest.raises(TypeError):
            call(tri)                                         # the right tensor, but on the host
        with pytest.raises(TypeError):
            call(tri.float())
        with pytest.raises(TypeError):
            call(tri.numpy())
        with pytest.raises(ValueError):
            call(tri[0])
        with pytest.raises(ValueError):
            call(tri.permute(0, 2, 1))
    with pytest.raises(TypeError):
        reader.fill_enclosed(tri.numpy().astype(np.int32))
    with pytest.raises(TypeError):
        reader.fill_enclosed(tri.float())
    with pytest.raises(ValueError):
        reader.fill_enclosed(tri.numpy()[0, 0])
    with pytest.raises(ValueError):
        reader.fill_enclosed(tri.numpy()[None])
    with pytest.raises(ValueError):
        reader.fill_enclosed(tri.numpy(), max_area=-1)
    with pytest.raises(TypeError):
        reader.fill_enclosed(tri.numpy(), max_area=2.0)
    with pytest.raises(TypeError):
        reader.fill_enclosed(tri.numpy(), max_area=True)
    cmp, bg = np.zeros((2, 4, 6, 3), np.uint8), np.zeros((4, 6, 3), np.uint8)
    for fill in (0, -2, 1.0, "yes"):
        with pytest.raises(ValueError, match="trimap_from_plate: fill"):
            reader.trimap_from_plate(cmp, bg, fill=fill)
    with pytest.raises(TypeError):
        reader.trimap_from_plate(cmp, bg, 16, 48, 4, 8, True)    # fill is keyword-only


# ---------------------------------------------------------------- FrameStream(auto_fill=...), host side

@pytest.fixture(scope="module")
def models(vgg0):
    from vmatting import unet
    np.random.seed(0)  # (the constructors do not touch the device)
    return unet.UNetVideo(vgg0, dtype="bf16", device="cuda"), unet.UNetImage(vgg0, dtype="bf16", device="cuda")


def test_frame_stream_auto_fill_constructs(models):
    from vmatting import FrameStream, ops
    mv, _ = models
    assert FrameStream(mv, 32, 48, trimap="auto").auto_fill is None
    assert FrameStream(mv, 32, 48, trimap="auto", auto_fill=False).auto_fill is None
    fs = FrameStream(mv, 32, 48, trimap="auto", auto_fill=True)
    assert fs.auto_fill == 0 and fs.auto_fill is not True and fs.auto_options == ops.PLATE_DEFAULTS
    assert fs._slots is None
    fs = FrameStream(mv, 32, 48, trimap="auto", auto_fill=4096, auto_options={"hi": 60})
    assert fs.auto_fill == 4096 and fs.auto_options == dict(ops.PLATE_DEFAULTS, hi=60)
    assert set(ops.PLATE_DEFAULTS) == {"lo", "hi", "r_bg", "r_fg"}


def test_frame_stream_auto_fill_errors(models):
    from vmatting import FrameStream
    mv, mi = models
    for kw in (dict(), dict(trimap="propagate"), dict(trimap=True)):
        for fill in (True, False, 50):
            with pytest.raises(ValueError, match="auto_fill"):
                FrameStream(mv, 32, 48, auto_fill=fill, **kw)           # auto_fill without "auto"
    with pytest.raises(ValueError, match="auto_fill"):
        FrameStream(mi, 32, 48, trimap=False, auto_fill=True)
    for fill in (0, -1, 1.0, 2.5, "all"):
        with pytest.raises(ValueError, match="auto_fill"):
            FrameStream(mv, 32, 48, trimap="auto", auto_fill=fill)
    with pytest.raises(ValueError, match="auto_options takes"):
        FrameStream(mv, 32, 48, trimap="auto", auto_fill=True, auto_options={"fill": True})
