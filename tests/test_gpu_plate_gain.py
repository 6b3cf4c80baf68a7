"""vm_plate_gain_fit / vm_plate_gain_apply on the GPU: gain, support and every byte of the gained plate equal the numpy
restatement (tests/plate_gain_ref.py) exactly, at every pointer alignment and with nothing written outside the results;
FrameStream(gain="fit") equals the stream fed the restatement's gained plates as per-frame backgrounds, byte for byte."""

import gc

import numpy as np
import pytest
import torch

import plate_gain_ref as ref
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

SENTINEL, FILL = -7777, 0xA5
OFFSETS = ((0, 0, 0), (1, 2, 3), (2, 3, 1), (3, 1, 2))  # byte offsets of cmp, bg and out from a 16-byte boundary
OPTIONS = ({}, {"band": 3, "min_share": 200})


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def at_offset(a, off):
    """``a`` (uint8 numpy) on the device at byte 32 + ``off`` of a buffer (the allocator's blocks start on 512 bytes) with
    FILL bytes before and after it -> (the whole buffer, the view of a's shape)."""
    buf = torch.full((32 + 4 + a.size + 32,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[32 + off:32 + off + a.size].view(a.shape)
    view.copy_(dev(a))
    return buf, view


def guarded_i32(n):
    """An int32 [n,3] result with four sentinel words on either side -> (the whole buffer, the view)."""
    buf = torch.full((3 * n + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    return buf, buf[4:4 + 3 * n].view(n, 3)


def fit_and_apply(cmp, bg, offs=(0, 0, 0), **opts):
    """Both calls through ops on ``cmp`` [n,h,w,3] and ``bg`` [nb,h,w,3] placed at the byte offsets, the workspace
    pre-filled with 0xFF; checks that nothing around the results was written -> (gain, support, out) as numpy."""
    from vmatting import ops
    n = cmp.shape[0]
    _, d_cmp = at_offset(cmp, offs[0])
    _, d_bg = at_offset(bg, offs[1])
    gbuf, gain = guarded_i32(n)
    sbuf, sup = guarded_i32(n)
    work = torch.full((ops.plate_gain_workspace_bytes(n),), 0xFF, dtype=torch.uint8, device="cuda")
    ops.plate_gain_fit(d_cmp, d_bg, out=gain, support=sup, work=work, **opts)
    obuf, out = at_offset(np.zeros(cmp.shape, np.uint8), offs[2])
    out.fill_(FILL)
    ops.plate_gain_apply(d_bg, gain, out=out)
    for buf in (gbuf, sbuf):
        edge = buf.cpu().numpy()
        assert (edge[:4] == SENTINEL).all() and (edge[-4:] == SENTINEL).all()
    edge, size = obuf.cpu().numpy(), cmp.size
    assert (edge[:32 + offs[2]] == FILL).all() and (edge[32 + offs[2] + size:] == FILL).all()
    return gain.cpu().numpy(), sup.cpu().numpy(), out.cpu().numpy()


def check(cmp, bg, offs=(0, 0, 0), **opts):
    G, S = ref.fits(cmp, bg, **opts)
    gain, sup, out = fit_and_apply(cmp, bg, offs, **opts)
    assert np.array_equal(gain, G), (gain, G)
    assert np.array_equal(sup, S), (sup, S)
    assert np.array_equal(out, ref.applies(bg, G))
    return G, S


def stacks(n, h, w):
    """Input stacks of n frames: uniform noise, and the scene under a different gain per frame."""
    noise = [ref.noise_pair(h, w, 10 + i) for i in range(n)]
    scenes = [ref.scene(20 + i, ref.GAINS[(i + 1) % len(ref.GAINS)], 0.3 * min(h, w), h, w)[:2] for i in range(n)]
    for pairs in (noise, scenes):
        yield np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (23, 35), (46, 70)])
def test_fit_and_apply_equal_the_restatement(h, w, n):
    """Odd row bytes and ragged last units, nb = 1 and nb = n, every alignment of the three byte planes.  (These frames
    are one block each; the 256 x 256 and 300 x 300 cases below take several.)"""
    k = 0
    for cmp, bg in stacks(n, h, w):
        for nb in sorted({1, n}):
            for opts in OPTIONS:
                check(cmp, bg[:nb], OFFSETS[k % 4], **opts)
                k += 1
    for offs in OFFSETS:  # every alignment on one input as well
        check(cmp, bg, offs, min_share=64)


def test_scene_gains_are_fitted_not_the_identity():
    """The scene stack at 46 x 70 takes the division path (the identity would pass a lazy kernel)."""
    cmp, bg = list(stacks(5, 46, 70))[1]
    G, S = check(cmp, bg, (1, 3, 2))
    assert (G != ref.ONE).sum() >= 12 and (S * 16 >= 46 * 70).all()


@pytest.mark.parametrize("offs", [(0, 0, 0), (1, 3, 2)])
def test_all_pairs(offs):
    """Every (a, b) of the division, at a different place per channel (a channel mix-up shows), several blocks."""
    cmp, bg = ref.all_pairs()
    for opts in ({"min_share": 1}, {"band": 16, "min_share": 1}, {"band": 1, "min_share": 4096}):
        G, S = check(cmp[None], bg[None], offs, **opts)
    assert len({tuple(r) for r in np.stack([G[0], S[0]], -1)}) == 1  # the same multiset of pairs in every channel
    two = np.stack([cmp, np.roll(cmp, 1, -1)])  # a second frame with its channels rotated, against the one plate
    check(two, bg[None], offs, band=2, min_share=1)


def test_constant_frames_need_64_bit_sums():
    """300 x 300 of 250 / 250: every pixel in one bin, sum b b = 5.6e9."""
    cmp, bg = ref.constant_pair(300, 300)
    G, S = check(cmp[None], bg[None], (3, 2, 1))
    assert G.tolist() == [[4096] * 3] and S.tolist() == [[90000] * 3]
    G, S = check(np.stack([cmp, cmp // 2]), bg[None], (2, 0, 3))
    assert G.tolist() == [[4096] * 3, [2048] * 3]


def test_zero_plate_falls_back_to_the_identity():
    cmp = ref.noise_pair(23, 35, 4)[0]
    G, S = check(np.stack([cmp, cmp]), np.zeros((1, 23, 35, 3), np.uint8), (1, 1, 1))
    assert (G == ref.ONE).all() and (S == 0).all()


def test_apply_on_every_byte():
    """G in {0, 1, 4095, 4096, 4097, 17281} on all 256 bytes in every channel; gains outside 0 .. 2^20 act as the
    nearer end."""
    from vmatting import ops
    bg = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, -1)
    gains = np.array([0, 1, 4095, 4096, 4097, 17281], np.int64)
    G = np.stack([np.roll(gains, i)[:3] for i in range(6)])
    for off in range(4):
        _, d_bg = at_offset(bg[None], off)
        obuf, out = at_offset(np.zeros((6, 16, 16, 3), np.uint8), (off + 1) % 4)
        ops.plate_gain_apply(d_bg, dev(G.astype(np.int32)), out=out)
        assert np.array_equal(out.cpu().numpy(), ref.applies(bg, G))
        edge = obuf.cpu().numpy()
        assert (edge[:32 + (off + 1) % 4] == FILL).all() and (edge[32 + (off + 1) % 4 + 6 * 768:] == FILL).all()
    wild = np.array([[-5, 1 << 20, (1 << 31) - 1], [-(1 << 31), (1 << 20) + 1, 1 << 30]], np.int64)
    got = ops.plate_gain_apply(dev(bg), dev(wild.astype(np.int32))).cpu().numpy()
    assert np.array_equal(got, ref.applies(bg, np.maximum(wild, 0)))


def test_captured_graph_follows_its_inputs():
    from vmatting import ops
    n, h, w = 2, 23, 35
    inputs = list(stacks(n, h, w))
    d_cmp, d_bg = dev(inputs[0][0]), dev(inputs[0][1])
    gain, sup = (torch.zeros((n, 3), dtype=torch.int32, device="cuda") for _ in range(2))
    out = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    work = torch.full((ops.plate_gain_workspace_bytes(n),), 0xFF, dtype=torch.uint8, device="cuda")

    def chain():
        ops.plate_gain_fit(d_cmp, d_bg, out=gain, support=sup, work=work, min_share=64)
        ops.plate_gain_apply(d_bg, gain, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gc.collect()  # (no dead cycle holding an earlier graph is left to be collected inside the capture: vmatting/graphs.py)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    for cmp, bg in (inputs[1], inputs[0]):
        d_cmp.copy_(dev(cmp))
        d_bg.copy_(dev(bg))
        for t in (gain, sup, out):
            t.zero_()
        g.replay()
        G, S = ref.fits(cmp, bg, min_share=64)
        assert np.array_equal(gain.cpu().numpy(), G) and np.array_equal(sup.cpu().numpy(), S)
        assert np.array_equal(out.cpu().numpy(), ref.applies(bg, G))


# ---------------------------------------------------------------- FrameStream(gain="fit")
H, W, CHUNK, DEPTH, FRAMES = 46, 70, 2, 2, 5  # a short last chunk
FRAME_GAINS = ((.8, .8, .8), (1.25, 1.1, .9), (1, 1, 1), (.7, .85, 1.1), (1.2, 1.2, 1.2))
NEW_BUFFERS = ("g_bg", "gain", "support")


@pytest.fixture(scope="module")
def models(vgg0):
    from vmatting import unet
    np.random.seed(0)
    return {7: unet.UNetVideo(vgg0, dtype="bf16", device="cuda").prepare(),
            6: unet.UNetImage(vgg0, dtype="bf16", device="cuda").prepare()}


@pytest.fixture(scope="module")
def clip():
    """test_gpu_stream_scale's clip (a textured block drifting over a smooth plate that stays within 20..220) with every
    frame under a gain of its own; per-frame backgrounds that differ slightly from the plate; painted trimaps; one new
    plate.  The restatement's gains and gained backgrounds for the static plate and for the per-frame backgrounds."""
    rs = np.random.RandomState(7)
    yy, xx = np.mgrid[0:H, 0:W]
    plate = np.stack([120 + 60 * np.sin(xx / 9.0 + c) + 40 * np.cos(yy / 7.0 + 2 * c) for c in range(3)], -1)
    plate = np.clip(np.rint(plate), 0, 255).astype(np.uint8)
    cmp = np.repeat(plate[None], FRAMES, 0).copy()
    tri = np.zeros((FRAMES, H, W), np.uint8)
    for j in range(FRAMES):
        y, x = 8 + j, 14 + 2 * j
        cmp[j, y:y + 26, x:x + 30] = rs.randint(0, 256, (26, 30, 3))
        tri[j, y - 3:y + 29, x - 3:x + 33] = 128
        tri[j, y + 3:y + 23, x + 3:x + 27] = 255
    cmp = np.clip(np.rint(cmp * np.array(FRAME_GAINS)[:, None, None, :]), 0, 255).astype(np.uint8)
    bg = np.clip(plate[None].astype(np.int64) + rs.randint(-2, 3, (FRAMES, H, W, 3)), 0, 255).astype(np.uint8)
    new = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    out = {"cmp": cmp, "plate": plate, "bg": bg, "tri": tri, "new": new}
    for key, src in (("static", plate), ("per_frame", bg)):
        G, S = ref.fits(cmp, src)
        assert (S * 16 >= H * W).all() and (np.abs(G / 4096 / np.array(FRAME_GAINS) - 1) <= 0.03).all()
        out[key] = (G, S, ref.applies(src, G))
    return out


def chunks():
    return [(i, min(i + CHUNK, FRAMES)) for i in range(0, FRAMES, CHUNK)]


def run_stream(models, clip, bg, static, trimap, out, graph, scale, **kw):
    """The clip through a FrameStream: ``bg`` is the static plate ([H,W,3]) or the per-frame backgrounds."""
    from vmatting import FrameStream
    if trimap == "auto":
        kw["auto_fill"] = True
    if out == "over":
        kw["new_bg"] = clip["new"]
    fs = FrameStream(models[7 if trimap else 6], H, W, chunk=CHUNK, depth=DEPTH, trimap=trimap, out=out, graph=graph,
                     static_bg=bg if static else None, scale=scale, **kw)
    items = [(clip["cmp"][a:b], None if static else bg[a:b], clip["tri"][a:b] if trimap is True else None)
             for a, b in chunks()]
    got = list(fs.run(items))
    assert [g.shape[0] for g in got] == [b - a for a, b in chunks()] and fs.overflowed_chunks == []
    return np.concatenate(got), fs


@pytest.mark.parametrize("graph,trimap,out,scale,static", [
    (True, True, "u8", 1, True), (False, "auto", "over", 1, True), (True, "auto", "bgra", 2, True),
    (False, True, "u8", 2, True), (True, True, "over", 1, False), (False, False, "bgra", 1, False)])
def test_stream_equals_the_stream_fed_gained_plates(models, clip, graph, trimap, out, scale, static):
    G, S, gained = clip["static" if static else "per_frame"]
    want, _ = run_stream(models, clip, gained, False, trimap, out, False, scale)
    got, fs = run_stream(models, clip, clip["plate"] if static else clip["bg"], static, trimap, out, graph, scale,
                         gain="fit")
    assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)
    # and the gain matters: the ungained stream differs
    plain, _ = run_stream(models, clip, clip["plate"] if static else clip["bg"], static, trimap, out, False, scale)
    assert not np.array_equal(plain, want)
    gains, support = fs.last_gains()
    a, b = chunks()[-1]
    assert gains.dtype == np.float32 and gains.shape == (b - a, 3) == support.shape
    assert np.array_equal(gains, G[a:b].astype(np.float32) / np.float32(4096)) and np.array_equal(support, S[a:b])
    slot = fs._slots[0]
    assert tuple(slot.g_bg.shape) == (CHUNK, H, W, 3) and tuple(slot.gain.shape) == (CHUNK, 3) == tuple(slot.support.shape)
    assert fs._plate_lo is None and (scale == 1 or tuple(slot.r_bg.shape) == (CHUNK, fs.hm, fs.wm, 3))
    if graph and out == "u8":  # the object runs again, over the same graphs
        again = np.concatenate(list(fs.run([(clip["cmp"][a:b], None, clip["tri"][a:b]) for a, b in chunks()])))
        assert np.array_equal(again, want)


def test_gain_options_reach_the_kernels(models, clip):
    """min_share 1 at band 1 is another fit: the stream's gains are the restatement's for those options."""
    opts = {"band": 1, "min_share": 1}
    G, S = ref.fits(clip["cmp"], clip["plate"], **opts)
    assert not np.array_equal(G, clip["static"][0])
    want, _ = run_stream(models, clip, ref.applies(clip["plate"], G), False, True, "u8", False, 1)
    got, fs = run_stream(models, clip, clip["plate"], True, True, "u8", True, 1, gain="fit", gain_options=opts)
    assert np.array_equal(got, want)
    assert np.array_equal(fs.last_gains()[1], S[-1:])


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_no_gain_is_the_stream_as_it_was(models, clip, graph):
    res = []
    for kw in ({}, {"gain": None}):
        got, fs = run_stream(models, clip, clip["plate"], True, "auto", "u16", graph, 1, **kw)
        res.append(got)
        assert fs.gain is None and fs._gain_work is None and fs._gain_last is None
        for s in fs._slots:
            assert not any(hasattr(s, name) for name in NEW_BUFFERS)
    assert np.array_equal(res[0], res[1])


def test_reader_helpers(clip):
    """reader.match_plate and reader.trimap_from_plate(gain="fit") are the restatement's, through the kernels."""
    import trimap_plate_ref as tp
    from vmatting import reader
    G, S, gained = clip["static"]
    plate, gains, support = reader.match_plate(clip["cmp"][0], clip["plate"])
    assert np.array_equal(plate, gained[0]) and np.array_equal(support, S[0])
    assert gains.dtype == np.float32 and np.array_equal(gains, G[0].astype(np.float32) / np.float32(4096))
    got = reader.trimap_from_plate(clip["cmp"], clip["plate"], gain="fit")
    assert np.array_equal(got, tp.trimaps(clip["cmp"], gained, **tp.DEFAULTS))
    assert not np.array_equal(got, reader.trimap_from_plate(clip["cmp"], clip["plate"]))
    G2, _ = ref.fits(clip["cmp"][:1], clip["plate"], band=2)
    got = reader.trimap_from_plate(clip["cmp"][0], clip["plate"], gain="fit", gain_options={"band": 2}, fill=True)
    assert got.shape == (H, W)
    assert np.array_equal(got, reader.fill_enclosed(tp.trimap(clip["cmp"][0], ref.apply(clip["plate"], G2[0]),
                                                              **tp.DEFAULTS)))
