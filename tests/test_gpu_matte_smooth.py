"""vm_matte_smooth on the GPU: out and weight equal the numpy restatement (tests/matte_smooth_ref.py) bit for bit, at
every pointer alignment, in place and apart, with nothing written outside the results; FrameStream(smooth="flow") equals
the restatement run over the whole clip on the unsmoothed stream's mattes, bit for bit, in every configuration."""

import numpy as np
import pytest
import torch

import matte_smooth_ref as ref
import score_ref
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

F = np.float32
SENTINEL, FILL = -7777.0, 0xA5
SHAPES = [(1, 1), (1, 9), (7, 1), (5, 7), (16, 16), (37, 53), (46, 70)]  # 37 x 53: odd h w, so unaligned frame bases
OPTIONS = ({}, {"strength": 0.9, "tol": 60.0, "jump": 0.75}, {"strength": 0.25, "tol": 9.0, "jump": 0.15})


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def at_offset(a, off):
    """``a`` (uint8 numpy) on the device at byte 32 + ``off`` of a buffer (the allocator's blocks start on 512 bytes) with
    FILL bytes before and after it -> (the whole buffer, the view of a's shape)."""
    buf = torch.full((32 + 4 + a.size + 32,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[32 + off:32 + off + a.size].view(a.shape)
    view.copy_(dev(a))
    return buf, view


def guarded_f32(a, pad):
    """``a`` (f32 numpy) on the device behind ``pad`` sentinel floats and before 4 more (pad 4: the array starts on 16
    bytes; pad 5: on 4 only) -> (the whole buffer, the view of a's shape)."""
    buf = torch.full((pad + a.size + 4,), SENTINEL, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[pad:pad + a.size].view(a.shape)
    view.copy_(dev(a))
    return buf, view


def guards_intact(buf, pad):
    edge = buf.cpu().numpy()
    return (edge[:pad] == SENTINEL).all() and (edge[-4:] == SENTINEL).all()


def run_kernel(alpha, cmp, flow, prev, in_place, pads, off, **opts):
    """ops.matte_smooth on the inputs placed at the given alignments -> (out, weight) as numpy, after checking that
    nothing around them was written."""
    from vmatting import ops
    abuf, d_alpha = guarded_f32(alpha, pads[0])
    _, d_flow = guarded_f32(flow, pads[1])
    _, d_cmp = at_offset(cmp, off)
    d_prev = None
    if prev is not None:
        d_prev = (guarded_f32(prev[0], pads[2])[1], at_offset(prev[1], (off + 1) % 4)[1])
    wbuf, d_weight = guarded_f32(np.full(alpha.shape, SENTINEL, F), pads[2])
    if in_place:
        obuf, d_out = abuf, d_alpha
    else:
        obuf, d_out = guarded_f32(np.full(alpha.shape, SENTINEL, F), pads[0])
    got = ops.matte_smooth(d_alpha, d_cmp, d_flow, d_prev, out=d_out, weight=d_weight, **opts)
    assert got is d_out
    assert guards_intact(obuf, pads[0]) and guards_intact(wbuf, pads[2])
    if not in_place:
        assert np.array_equal(bits(d_alpha.cpu().numpy()), bits(alpha))  # the input is left alone
    return d_out.cpu().numpy(), d_weight.cpu().numpy()


@pytest.mark.parametrize("with_prev", [False, True], ids=["start", "prev"])
@pytest.mark.parametrize("h,w", SHAPES)
def test_kernel_equals_the_restatement(h, w, with_prev):
    """n = 3: frame 0 with or without ``prev``, frames 1 and 2 against the kernel's own previous result.  Wild mattes
    (NaN, below 0, above 1), wild flows (NaN, +-inf, far outside, exactly on the last column) and moderate ones, every
    byte offset of cmp, f32 arrays on 16 bytes and on 4 only, in place and apart, three sets of options."""
    n = 3
    alpha = score_ref.mattes(n, h, w, 11, wild=True)
    cmp = ref.frames(n, h, w, 12)
    prev = (score_ref.mattes(1, h, w, 13, wild=True)[0], ref.frames(1, h, w, 14)[0]) if with_prev else None
    k, shares = 0, []
    for flow in (score_ref.wild_flow(n, h, w, 15), ref.moderate_flow(n, h, w, 16)):
        for in_place in (False, True):
            for pads in ((4, 4, 4), (5, 4, 4), (4, 6, 5)):
                opts = OPTIONS[k % 3]
                want, want_w = ref.smooth(alpha, cmp, flow, prev, **opts)
                out, weight = run_kernel(alpha, cmp, flow, prev, in_place, pads, k % 4, **opts)
                assert np.array_equal(bits(out), bits(want)), (k, in_place, pads)
                assert np.array_equal(bits(weight), bits(want_w)), (k, in_place, pads)
                shares.append(((want_w[1:] > 0).mean(), (want[1:] != score_ref.unit(alpha[1:])).mean()))
                k += 1
    if h * w >= 256:  # the filter does something on these inputs: the comparison is not one of clamps alone
        assert max(s[0] for s in shares) > 0.4 and max(s[1] for s in shares) > 0.4 and min(s[0] for s in shares) > 0.02


def test_shapes_with_a_trailing_axis_and_no_weight():
    """alpha [n,h,w,1] gives out [n,h,w,1]; without ``out`` and ``weight`` the result is new and alpha untouched."""
    from vmatting import ops
    n, h, w = 2, 16, 20
    alpha, cmp, flow = score_ref.mattes(n, h, w, 1, wild=True), ref.frames(n, h, w, 2), ref.moderate_flow(n, h, w, 3)
    d_alpha = dev(alpha[..., None])
    out = ops.matte_smooth(d_alpha, dev(cmp), dev(flow))
    assert tuple(out.shape) == (n, h, w, 1) and out.data_ptr() != d_alpha.data_ptr()
    assert np.array_equal(bits(out.cpu().numpy()[..., 0]), bits(ref.smooth(alpha, cmp, flow)[0]))
    assert np.array_equal(bits(d_alpha.cpu().numpy()[..., 0]), bits(alpha))
    with pytest.raises(ValueError, match="matte_smooth"):  # a partial overlap is the library's refusal
        buf = torch.zeros(n * h * w + 8, dtype=torch.float32, device="cuda")
        ops.matte_smooth(buf[:n * h * w].view(n, h, w), dev(cmp), dev(flow), out=buf[8:].view(n, h, w))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- FrameStream(smooth="flow")
H, W, CHUNK, DEPTH, FRAMES = 46, 70, 2, 2, 5  # test_gpu_plate_gain's clip shape: a short last chunk
FLOW_OPTIONS = {"levels": 3, "iters": 8}
KEYS = (0, 2)  # trimap="propagate": the frames that carry a key (the second one restarts the filter mid-clip)


@pytest.fixture(scope="module")
def models(vgg0):
    from vmatting import unet
    np.random.seed(0)
    return {7: unet.UNetVideo(vgg0, dtype="bf16", device="cuda").prepare(),
            6: unet.UNetImage(vgg0, dtype="bf16", device="cuda").prepare()}


@pytest.fixture(scope="module")
def clip():
    """A smooth plate, one textured block drifting 2 x 1 px/frame over it (the same texture in every frame, so the flow
    has something to follow), painted trimaps, a new plate, and the device's flow estimates between consecutive
    frames."""
    from vmatting import ops
    rs = np.random.RandomState(7)
    yy, xx = np.mgrid[0:H, 0:W]
    plate = np.stack([120 + 60 * np.sin(xx / 9.0 + c) + 40 * np.cos(yy / 7.0 + 2 * c) for c in range(3)], -1)
    plate = np.clip(np.rint(plate), 0, 255).astype(np.uint8)
    block = rs.randint(0, 256, (26, 30, 3))
    block = ((block + np.roll(block, 1, 0) + np.roll(block, 1, 1) + np.roll(block, (1, 1), (0, 1))) // 4).astype(np.uint8)
    cmp = np.repeat(plate[None], FRAMES, 0).copy()
    tri = np.zeros((FRAMES, H, W), np.uint8)
    for j in range(FRAMES):
        y, x = 8 + j, 14 + 2 * j
        cmp[j, y:y + 26, x:x + 30] = block
        tri[j, y - 3:y + 29, x - 3:x + 33] = 128
        tri[j, y + 3:y + 23, x + 3:x + 27] = 255
    flows = np.zeros((FRAMES, H, W, 2), F)
    for j in range(1, FRAMES):
        flows[j] = ops.estimate_flow(dev(cmp[j]), dev(cmp[j - 1]), **FLOW_OPTIONS).cpu().numpy()
    assert np.abs(flows[1:]).max() > 0.5  # the estimator saw the block move
    return {"cmp": cmp, "plate": plate, "tri": tri, "flows": flows,
            "new": rs.randint(0, 256, (H, W, 3)).astype(np.uint8), "plain": {}}


def chunks():
    return [(i, min(i + CHUNK, FRAMES)) for i in range(0, FRAMES, CHUNK)]


def make_stream(models, clip, trimap, out, graph, **kw):
    from vmatting import FrameStream
    if trimap == "auto":
        kw["auto_fill"] = True
    if out == "over":
        kw["new_bg"] = clip["new"]
    return FrameStream(models[7 if trimap else 6], H, W, chunk=CHUNK, depth=DEPTH, trimap=trimap, out=out, graph=graph,
                       static_bg=clip["plate"], **kw)


def items(clip, trimap):
    for a, b in chunks():
        if trimap == "propagate":
            yield clip["cmp"][a:b], None, clip["tri"][a] if a in KEYS else None, None
        else:
            yield clip["cmp"][a:b], None, clip["tri"][a:b] if trimap is True else None


def run(fs, clip, trimap):
    got = list(fs.run(items(clip, trimap)))
    assert [g.shape[0] for g in got] == [b - a for a, b in chunks()] and fs.overflowed_chunks == []
    return np.concatenate(got)


def oracle(models, clip, trimap, **kw):
    """The unsmoothed stream's f32 mattes of this configuration (computed once, eagerly), and the restatement run over
    the whole clip on them with the estimated flows, restarted where the stream restarts -> (plain, out, weight)."""
    name = repr((trimap, sorted(kw.items())))
    if name not in clip["plain"]:
        more = {"flow_options": FLOW_OPTIONS} if trimap == "propagate" else {}
        plain = run(make_stream(models, clip, trimap, "f32", False, **kw, **more), clip, trimap)
        assert plain.dtype == np.float32 and plain.shape == (FRAMES, H, W)
        starts = list(KEYS if trimap == "propagate" else (0,)) + [FRAMES]
        parts = [ref.smooth(plain[a:b], clip["cmp"][a:b], clip["flows"][a:b]) for a, b in zip(starts, starts[1:])]
        clip["plain"][name] = (plain, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
    return clip["plain"][name]


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_stream_equals_the_restatement_over_the_whole_clip(models, clip, graph):
    plain, want, want_w = oracle(models, clip, True)
    fs = make_stream(models, clip, True, "f32", graph, smooth="flow", flow_options=FLOW_OPTIONS)
    got = run(fs, clip, True)
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    assert not np.array_equal(got, plain) and np.array_equal(got[0], plain[0])  # it filters; frame 0 starts the run
    assert np.array_equal(bits(fs.last_weight()), bits(want_w[-1])) and (want_w[-1] > 0).any()
    # the object runs again to the same bytes: the state restarts, and the graphs captured at setup are reused
    graphs = [dict(s.graphs) for s in fs._slots]
    assert all(sorted(g) == ([False, True] if graph else []) for g in graphs) and len(graphs) == DEPTH
    assert np.array_equal(bits(run(fs, clip, True)), bits(want))
    assert all(s.graphs[k] is g[k] for s, g in zip(fs._slots, graphs) for k in g)
    assert tuple(fs._smooth_last.shape) == (H, W, 1) and tuple(fs._smooth_cmp.shape) == (H, W, 3)
    assert tuple(fs._smooth_weight.shape) == (CHUNK, H, W, 1) and all(tuple(s.d_bw.shape) == (CHUNK, H, W, 2) for s in fs._slots)


@pytest.mark.parametrize("graph,out", [(True, "u8"), (False, "over")])
def test_quantised_and_composed_results_come_from_the_filtered_matte(models, clip, graph, out):
    from vmatting import ops
    _, want, _ = oracle(models, clip, True)
    got = run(make_stream(models, clip, True, out, graph, smooth="flow", flow_options=FLOW_OPTIONS), clip, True)
    if out == "u8":
        through = ops.matte_quantize(dev(want), bits=8)
    else:
        through = ops.matte_compose(dev(want), dev(clip["cmp"]), dev(clip["plate"]), dev(clip["new"]), mode="over")
    assert got.dtype == np.uint8 and np.array_equal(got, through.cpu().numpy())


@pytest.mark.parametrize("graph,trimap,kw", [
    (True, True, {"scale": 2}), (False, "auto", {}), (True, False, {"gain": "fit"}), (True, "propagate", {}),
    (False, "propagate", {})], ids=["scale2", "auto", "gain", "propagate-graph", "propagate-eager"])
def test_stream_in_every_configuration(models, clip, graph, trimap, kw):
    """With scale the filter runs on the full-resolution matte; with "propagate" the second key restarts it."""
    plain, want, _ = oracle(models, clip, trimap, **kw)
    fs = make_stream(models, clip, trimap, "f32", graph, smooth="flow", flow_options=FLOW_OPTIONS, **kw)
    got = run(fs, clip, trimap)
    assert np.array_equal(bits(got), bits(want)) and not np.array_equal(got, plain)
    if trimap == "propagate":
        assert all(np.array_equal(got[k], plain[k]) for k in KEYS) and not np.array_equal(got[3], plain[3])


def test_propagate_shares_its_flows_with_the_filter(models, clip, monkeypatch):
    """One flow per frame with a predecessor (frames 1, 3 and 4: 0 and 2 carry keys), not two."""
    from vmatting import ops
    calls = []
    real = ops.flow_from_pyramids
    monkeypatch.setattr(ops, "flow_from_pyramids", lambda *a, **k: calls.append(1) or real(*a, **k))
    fs = make_stream(models, clip, "propagate", "f32", False, smooth="flow", flow_options=FLOW_OPTIONS)
    run(fs, clip, "propagate")
    assert len(calls) == 3
    del calls[:]
    run(make_stream(models, clip, True, "f32", False, smooth="flow", flow_options=FLOW_OPTIONS), clip, True)
    assert len(calls) == 4  # without "propagate" only the first frame of the run has no predecessor


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_no_smooth_is_the_stream_as_it_was(models, clip, graph):
    res = []
    for kw in ({}, {"smooth": None}):
        fs = make_stream(models, clip, True, "u16", graph, **kw)
        res.append(run(fs, clip, True))
        assert fs.smooth is None and not fs.estimate and not hasattr(fs, "_flow")
        assert fs._smooth_last is None and fs._smooth_cmp is None and fs._smooth_weight is None
        assert all(s.d_bw is None and s.graphs == {} for s in fs._slots)
    assert np.array_equal(res[0], res[1])


def test_reader_smooth_mattes(clip):
    """The inspection helper estimates its flows at the estimator's defaults; given flows are taken as they are; uint8
    mattes are q / 255."""
    from vmatting import ops, reader
    cmp = clip["cmp"]
    mattes = score_ref.mattes(FRAMES, H, W, 3, wild=True)
    flows = np.zeros((FRAMES, H, W, 2), F)
    for j in range(1, FRAMES):
        flows[j] = ops.estimate_flow(dev(cmp[j]), dev(cmp[j - 1])).cpu().numpy()
    got = reader.smooth_mattes(mattes, cmp)
    assert got.dtype == np.float32 and got.shape == (FRAMES, H, W)
    assert np.array_equal(bits(got), bits(ref.smooth(mattes, cmp, flows)[0]))
    got = reader.smooth_mattes(mattes, cmp, clip["flows"], tol=60.0)
    assert np.array_equal(bits(got), bits(ref.smooth(mattes, cmp, clip["flows"], tol=60.0)[0]))
    q = score_ref.mattes(FRAMES, H, W, 4, dtype=np.uint8)
    got = reader.smooth_mattes(q, cmp, clip["flows"])
    assert np.array_equal(bits(got), bits(ref.smooth(score_ref.unit(q), cmp, clip["flows"])[0]))
