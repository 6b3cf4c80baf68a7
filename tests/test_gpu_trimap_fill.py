"""The fill of enclosed background on the GPU: ops.trimap_fill_enclosed against the breadth-first restatement
(tests/trimap_fill_ref.py), byte for byte, and FrameStream(trimap="auto", auto_fill=...) against FrameStream(trimap=True)
fed the restatement's filled trimaps, bit for bit."""

import numpy as np
import pytest
import torch

import trimap_fill_ref as ref
import trimap_plate_ref as plate_ref
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

# the smallest first (below 3 x 3 the call is a copy); then as tests/test_gpu_components.py
SHAPES = [(1, 1), (2, 2), (3, 3), (1, 17), (19, 1), (64, 64), (70, 90), (65, 129), (133, 261)]
LARGE = SHAPES[5:]
N = 3
SENTINEL = 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(nbytes, fill, lead=0):
    """A uint8 device buffer of ``nbytes`` with SENTINEL bytes of ``fill`` behind it (and ``lead`` in front)."""
    buf = torch.full((lead + nbytes + SENTINEL,), fill, dtype=torch.uint8, device="cuda")
    return buf, buf[lead:lead + nbytes]


def intact(buf, nbytes, fill, lead=0):
    b = buf.cpu().numpy()
    return (b[:lead] == fill).all() and (b[lead + nbytes:] == fill).all()


def check(tris, caps=(0,), case=None):
    """Out of place into a guarded buffer, over a guarded workspace full of 0xFF; the input stays as it was."""
    from vmatting import ops
    n, h, w = tris.shape
    nwork = ops.trimap_fill_enclosed_workspace_bytes(n, h, w)
    assert nwork == 8 * n * h * w
    d_tri = dev(tris)
    for cap in caps:
        obuf, out = guarded(n * h * w, 0xA5)
        wbuf, work = guarded(nwork, 0xFF)
        got = ops.trimap_fill_enclosed(d_tri, cap, out=out.view(n, h, w), work=work)
        assert got.data_ptr() == out.data_ptr()
        assert np.array_equal(got.cpu().numpy(), ref.shared_fills(tris, cap)), (case, cap)
        assert intact(obuf, n * h * w, 0xA5) and intact(wbuf, nwork, 0xFF), (case, cap)
    assert np.array_equal(d_tri.cpu().numpy(), tris)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_random_trimaps_equal_the_restatement(shape):
    h, w = shape
    changed = 0
    for p in ref.P_ZERO:
        tris = ref.random_trimaps(N, h, w, p)
        if shape in LARGE and p <= 0.7:
            for t in tris:                                    # both kinds of component occur in every frame
                count, enclosed, _ = ref.census(t)
                assert 0 < enclosed < count, (shape, p)
        check(tris, caps=(0, 1, 7, 4096), case=p)
        changed += (ref.shared_fills(tris) != tris).sum()
    assert (changed > 0) == (shape in LARGE)
    if h < 3 or w < 3:
        tris = np.zeros((N, h, w), np.uint8)
        assert np.array_equal(ref.shared_fills(tris), tris)
        check(tris, case="a copy")


def patterns():
    h, w = 133, 261
    yield "serpentine", ref.serpentine(h, w), (0, 4096)
    yield "serpentine, open", ref.serpentine(h, w, open_end=True), (0,)
    yield "spiral", ref.spiral(h, w), (0,)
    yield "spiral, open", ref.spiral(h, w, open_end=True), (0,)
    yield "comb", ref.comb(h, w), (0, 17159, 17158)
    yield "checkerboard", ref.checkerboard(h, w), (0, 1)
    yield "corner squares", ref.corner_squares(h, w), (0, 24)
    yield "rings", ref.rings(h, w), (0, 100)
    yield "all zero", np.zeros((h, w), np.uint8), (0, 1)
    yield "framed zero", ref.framed_zero(h, w), (0,)
    for where in ("tl", "tr", "bl", "br", "mid"):
        yield "touch " + where, ref.one_pixel_touch(h, w, where), (0,)
    for where in ("tl", "tr", "bl", "br"):
        yield "diagonal " + where, ref.one_pixel_touch(70, 90, where, diagonal=True), (0,)
    yield "odd bytes", ref.odd_bytes(h, w), (0, 3)
    yield "areas", ref.area_squares(70, 90), (0, 25, 1)
    yield "areas, two tiles", np.roll(ref.area_squares(70, 90), (27, 55), (0, 1)), (0, 25, 1)


@pytest.mark.parametrize("name", [p[0] for p in patterns()])
def test_patterns_equal_the_restatement(name):
    tri, caps = next(p[1:] for p in patterns() if p[0] == name)
    tris = np.stack([tri, tri[::-1, ::-1], tri[::-1]])
    check(tris, caps=caps, case=name)
    want = ref.shared_fills(tris)
    if name in ("serpentine", "spiral", "comb", "framed zero"):
        assert (want != 0).all()                              # everything is filled
    if name in ("serpentine, open", "spiral, open", "all zero") or name.startswith("touch"):
        assert np.array_equal(want, tris)                     # nothing changes
    if name.startswith("diagonal"):
        assert (want == 0).sum() == N                         # the corner pixel alone stays
    if name == "corner squares":
        assert (want[0][5:10, 5:10] == 128).all() and (want[0][0:5, 0:5] == 0).all()
    if name == "odd bytes":
        assert len(np.unique(want)) == 256
    if name.startswith("areas"):
        assert [(ref.shared_fills(tris, cap)[0] == 0).sum() for cap in (0, 25, 1)] == [0, 26, 75]


def test_in_place_offsets_and_workspace_reuse():
    from vmatting import ops
    h, w = 133, 261
    a = ref.random_trimaps(N, h, w, 0.6)
    b = np.stack([ref.serpentine(h, w), ref.comb(h, w), ref.rings(h, w)])
    nwork = ops.trimap_fill_enclosed_workspace_bytes(N, h, w)
    wbuf, work = guarded(nwork, 0xFF)
    # in place, at byte offsets 1 and 3, one workspace for every call and both inputs
    for lead in (1, 3, 0):
        for tris in (a, b):
            for cap in (0, 7):
                buf, t = guarded(tris.size, 0xA5, lead=lead)
                t.copy_(dev(tris).view(-1))
                assert t.data_ptr() % 16 == lead
                got = ops.trimap_fill_enclosed(t.view(N, h, w), cap, out=t.view(N, h, w), work=work)
                assert got.data_ptr() == t.data_ptr()
                assert np.array_equal(got.cpu().numpy(), ref.shared_fills(tris, cap)), (lead, cap)
                assert intact(buf, tris.size, 0xA5, lead=lead) and intact(wbuf, nwork, 0xFF)
    # out of place with trimap and out at different offsets
    for lead_t, lead_o in ((1, 3), (3, 0), (0, 1)):
        _, t = guarded(a.size, 0, lead=lead_t)
        t.copy_(dev(a).view(-1))
        obuf, o = guarded(a.size, 0xA5, lead=lead_o)
        got = ops.trimap_fill_enclosed(t.view(N, h, w), out=o.view(N, h, w), work=work)
        assert np.array_equal(got.cpu().numpy(), ref.shared_fills(a)) and np.array_equal(t.cpu().numpy(), a.ravel())
        assert intact(obuf, a.size, 0xA5, lead=lead_o)
    # three calls on one input: identical bytes
    d = dev(a)
    runs = [ops.trimap_fill_enclosed(d, 4096, work=work).cpu().numpy() for _ in range(3)]
    assert all(np.array_equal(r, ref.shared_fills(a, 4096)) for r in runs)


def test_allocated_buffers_and_reader_wrappers():
    from vmatting import ops, reader
    h, w = 70, 90
    tris = ref.random_trimaps(N, h, w, 0.6)
    want = ref.shared_fills(tris)
    got = ops.trimap_fill_enclosed(dev(tris))
    assert got.shape == (N, h, w) and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    # reader.fill_enclosed: numpy in, numpy out; device tensors stay on the device; one frame or a stack
    got = reader.fill_enclosed(tris)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    d = dev(tris)
    got = reader.fill_enclosed(d)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want) and np.array_equal(d.cpu().numpy(), tris)
    got = reader.fill_enclosed(tris[1], max_area=7)
    assert got.shape == (h, w) and np.array_equal(got, ref.shared_fills(tris, 7)[1])
    got = reader.fill_enclosed(dev(tris[2]))
    assert got.is_cuda and got.shape == (h, w) and np.array_equal(got.cpu().numpy(), want[2])
    # reader.trimap_from_plate(fill=...)
    pairs = [ref.holed_blob_pair(h, w, seed=30 + i) for i in range(N)]
    cmp, bg = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    plain = plate_ref.trimaps(cmp, bg, **AUTO)
    assert np.array_equal(reader.trimap_from_plate(cmp, bg, **AUTO), plain)
    assert np.array_equal(reader.trimap_from_plate(cmp, bg, fill=False, **AUTO), plain)
    assert np.array_equal(reader.trimap_from_plate(cmp, bg, fill=True, **AUTO), ref.fills(plain))
    assert np.array_equal(reader.trimap_from_plate(cmp, bg, fill=20, **AUTO), plain)
    assert np.array_equal(reader.trimap_from_plate(cmp[0], bg[0], fill=81, **AUTO), ref.fill(plain[0]))
    got = reader.trimap_from_plate(dev(cmp), dev(bg[0]), fill=True, **AUTO)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), ref.fills(plate_ref.trimaps(cmp, bg[0], **AUTO)))


def test_captured_call_replays_on_new_inputs():
    from vmatting import ops
    h, w = 133, 261
    d_tri = torch.zeros((N, h, w), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((N, h, w), dtype=torch.uint8, device="cuda")
    work = torch.zeros(ops.trimap_fill_enclosed_workspace_bytes(N, h, w), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.trimap_fill_enclosed(d_tri, 7, out=d_out, work=work)
        ops.trimap_fill_enclosed(d_tri, out=d_tri, work=work)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.trimap_fill_enclosed(d_tri, 7, out=d_out, work=work)     # with the area sums, out of place
        ops.trimap_fill_enclosed(d_tri, out=d_tri, work=work)        # then any area, in place: as the stream calls it
    a = ref.random_trimaps(N, h, w, 0.6)
    b = np.stack([ref.serpentine(h, w), ref.comb(h, w), ref.rings(h, w)])
    for tris in (a, b, a):
        d_tri.copy_(dev(tris))
        d_out.zero_()
        g.replay()
        assert np.array_equal(d_out.cpu().numpy(), ref.shared_fills(tris, 7))
        assert np.array_equal(d_tri.cpu().numpy(), ref.shared_fills(tris))


def test_wrapper_errors():
    from vmatting import ops
    n, h, w = 2, 8, 12
    tri = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    big = torch.zeros(n * h * w * 10, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="out must be trimap itself"):
        ops.trimap_fill_enclosed(big[:n * h * w].view(n, h, w), out=big[8:8 + n * h * w].view(n, h, w))
    with pytest.raises(ValueError, match="work must not overlap"):
        ops.trimap_fill_enclosed(big[:n * h * w].view(n, h, w), work=big[:n * h * w * 8])
    with pytest.raises(ValueError):
        ops.trimap_fill_enclosed(tri, out=torch.zeros((n, h, 11), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ops.trimap_fill_enclosed(tri, work=torch.zeros(8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ops.trimap_fill_enclosed(tri, max_area=-1)
    with pytest.raises(TypeError):
        ops.trimap_fill_enclosed(tri, max_area=1.5)
    assert (tri == 0).all() and (big == 0).all()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- FrameStream(trimap="auto", auto_fill=...)

H, W, F, CHUNK = 70, 90, 7, 3    # items of 3, 3 and 1 frames: two full chunks and a short, eager one
AUTO = {"lo": 12, "hi": 40, "r_bg": 2, "r_fg": 3}


def items(cmp, bg, tris=None):
    for a in range(0, len(cmp), CHUNK):
        b = min(a + CHUNK, len(cmp))
        yield (cmp[a:b], None if bg is None else bg[a:b], None if tris is None else tris[a:b])


@pytest.fixture(scope="module")
def clip(vgg0):
    """7 frames of a disc with a plate-coloured patch inside it over per-frame plates, the bf16 model, and the
    restatement's trimaps, plain and filled, over the per-frame plates and over plate 0 alone."""
    from vmatting import unet
    pairs = [ref.holed_blob_pair(H, W, seed=30 + t) for t in range(F)]
    cmp, bg = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    np.random.seed(0)
    params = dict(unet.UNetVideo(vgg0, dtype="bf16", device="cuda").prepare().params)
    # a fresh UNetVideo's conv1_1 is [VGG, VGG, 0], as the reference's: its mattes do not depend on the trimap at all.
    # A trained one's do; stand in for it with weights on the trimap channel that weigh -0.5 .. 0.5 like a colour
    w, b = params["conv1_1"]
    w = w.copy()
    w[:, :, 6, :] = np.random.RandomState(5).normal(0, 20.0, w[:, :, 6, :].shape)
    params["conv1_1"] = (w, b)
    model = unet.UNetVideo(vgg0, dtype="bf16", device="cuda").load_params(params).prepare()
    plain = {"frames": plate_ref.trimaps(cmp, bg, **AUTO), "static": plate_ref.trimaps(cmp, bg[0], **AUTO)}
    filled = {k: ref.fills(t) for k, t in plain.items()}
    for k in plain:
        for i in range(F):
            count, enclosed, _ = ref.census(plain[k][i])
            assert count >= 2 and enclosed >= 1
            assert 20 < (filled[k][i] != plain[k][i]).sum()
            assert np.array_equal(ref.fill(plain[k][i], 20), plain[k][i])     # every hole is larger than 20 pixels
    return model, cmp, bg, plain, filled


def run(model, cmp, bg, plate, tris=None, **kw):
    from vmatting import FrameStream
    static = bg[0] if plate == "static" else None
    feed = None if plate == "static" else bg
    fs = FrameStream(model, H, W, chunk=CHUNK, out="u16", static_bg=static, **kw)
    return fs, list(fs.run(items(cmp, feed, tris)))


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("plate", ["frames", "static"])
def test_stream_auto_fill_equals_filled_trimaps(clip, plate, graph):
    model, cmp, bg, plain, filled = clip
    want = np.concatenate(run(model, cmp, bg, plate, filled[plate])[1])
    unfilled = np.concatenate(run(model, cmp, bg, plate, plain[plate])[1])
    assert not np.array_equal(filled[plate], plain[plate]) and not np.array_equal(want, unfilled)   # it reaches the mattes
    fs, got = run(model, cmp, bg, plate, trimap="auto", auto_options=AUTO, auto_fill=True, graph=graph)
    assert fs.auto_fill == 0 and fs.auto_options == AUTO
    assert [g.shape for g in got] == [(3, H, W), (3, H, W), (1, H, W)]
    assert np.array_equal(np.concatenate(got), want)
    assert np.array_equal(np.concatenate(list(fs.run(items(cmp, None if plate == "static" else bg)))), want)
    assert fs.overflowed_chunks == []
    assert all((s.graph is not None) == graph for s in fs._slots)
    # a cap below every hole's area: the unfilled stream's mattes
    _, got = run(model, cmp, bg, plate, trimap="auto", auto_options=AUTO, auto_fill=20, graph=graph)
    assert np.array_equal(np.concatenate(got), unfilled)
    # ... and without auto_fill the stream is what it was
    _, got = run(model, cmp, bg, plate, trimap="auto", auto_options=AUTO, graph=graph)
    assert np.array_equal(np.concatenate(got), unfilled)
