"""The flow estimator on the GPU (csrc/flow_est.hip): vm_flow_estimate equals the numpy f32 restatement
(tests/flow_est_ref.py) bit for bit, through the blocked sweep kernel (FT sweeps per launch on LDS tiles) and through
the one-sweep-per-launch kernel; it can be captured in a graph; and ClipStream(flow="estimate") gives the mattes of
ClipStream(flow="given") fed with ops.estimate_flow's flows of the same frame pairs."""

import numpy as np
import pytest
import torch

import flow_est_ref as ref
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

FT, TILE = 4, (32, 56)  # sweeps per blocked launch and the tile (rows, columns) of csrc/flow_est.hip
ODD = (133, 261)        # no multiple of the tile either way, five tiles each way
SENTINEL = 64
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

_pairs, _want = {}, {}


def frames(h, w, name):
    if (h, w, name) not in _pairs:
        _pairs[h, w, name] = ref.pair(h, w, name)[:2]
    return _pairs[h, w, name]


def want(h, w, name, **opts):
    """The restatement's flow, computed once per case."""
    key = (h, w, name, tuple(sorted(opts.items())))
    if key not in _want:
        _want[key] = ref.estimate(*frames(h, w, name), **opts)
        _want[key].setflags(write=False)
    return _want[key]


def set_blocked(on):
    from vmatting import _lib
    _lib.set_option("flow_blocked", int(on))


def device_flow(cur, prev, blocked, **opts):
    """ops.estimate_flow into a buffer with sentinel floats behind the flow, which must survive."""
    from vmatting import ops
    h, w = cur.shape[:2]
    buf = torch.full((h * w * 2 + SENTINEL,), -7.25, dtype=torch.float32, device="cuda")
    set_blocked(blocked)
    try:
        out = ops.estimate_flow(T(cur), T(prev), out=buf[:h * w * 2].view(h, w, 2), **opts)
        torch.cuda.synchronize()
    finally:
        set_blocked(True)
    assert out.data_ptr() == buf.data_ptr()
    assert (buf[h * w * 2:] == -7.25).all(), "wrote past the flow"
    return out.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_shapes_cover_the_tile():
    assert ODD[0] % TILE[0] and ODD[1] % TILE[1] and ODD[0] // TILE[0] >= 3 and ODD[1] // TILE[1] >= 3
    assert ref.level_shapes(70, 90, 6) == [(70, 90), (35, 45), (18, 23), (9, 12)]  # odd halving


@pytest.mark.parametrize("blocked", [True, False], ids=["blocked", "per-sweep"])
@pytest.mark.parametrize("h,w,name", [(70, 90, "small"), (96, 128, "small"), (96, 128, "large"), (96, 128, "zoom"),
                                      ODD + ("small",)])
def test_estimate_equals_restatement_bit_for_bit(h, w, name, blocked):
    cur, prev = frames(h, w, name)
    got = device_flow(cur, prev, blocked)
    exp = want(h, w, name)
    print("max |device - restatement| = %.3g" % np.abs(got - exp).max())
    assert same_bits(got, exp)


@pytest.mark.parametrize("blocked", [True, False], ids=["blocked", "per-sweep"])
@pytest.mark.parametrize("iters", [1, FT - 1, FT, FT + 1])
def test_sweep_counts_around_the_block_length(iters, blocked):
    h, w = ODD
    cur, prev = frames(h, w, "small")
    got = device_flow(cur, prev, blocked, warps=1, iters=iters)
    exp = want(h, w, "small", warps=1, iters=iters)
    print("max |device - restatement| = %.3g" % np.abs(got - exp).max())
    assert same_bits(got, exp)


@pytest.mark.parametrize("h,w", [(70, 90), ODD])
def test_pyramid_equals_restatement(h, w):
    """The stage that is callable on its own: ops.flow_pyramid's smoothed levels, finest first, each level's start
    padded to 4 floats."""
    from vmatting import ops
    cur, _ = frames(h, w, "small")
    got = ops.flow_pyramid(T(cur)).cpu().numpy()
    off = 0
    for level in ref.pyramid(cur, 6):
        n = level.size
        assert same_bits(got[off:off + n].reshape(level.shape), level), level.shape
        off += (n + 3) // 4 * 4
    assert off == got.size == ops.flow_pyramid_floats(h, w, 6)


def test_split_form_and_public_wrapper_equal_the_one_call():
    from vmatting import flow, ops
    h, w = 70, 90
    cur, prev = frames(h, w, "small")
    pc, pp = ops.flow_pyramid(T(cur)), ops.flow_pyramid(T(prev))
    assert same_bits(ops.flow_from_pyramids(pc, pp, h, w).cpu().numpy(), want(h, w, "small"))
    got = flow.estimate_flow(cur, prev)
    assert isinstance(got, np.ndarray) and same_bits(got, want(h, w, "small"))
    dev = flow.estimate_flow(T(cur), T(prev))
    assert dev.is_cuda and same_bits(dev.cpu().numpy(), got)
    # the convention: warping the previous frame's grey by the flow gives the current frame's
    g_cur, g_prev = ref.grey(cur), ref.grey(prev)
    warped = flow.warp_img(g_prev, got, mode="exact")
    inner = (slice(20, -20),) * 2
    assert np.abs(warped - g_cur)[inner].mean() < 0.25 * np.abs(g_prev - g_cur)[inner].mean()


def test_graph_capture_replays_on_new_frames():
    from vmatting import ops
    h, w = 70, 90
    pairs = [frames(h, w, "small"), frames(h, w, "zoom")[::-1]]
    cur, prev = (torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
    out = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
    work = torch.zeros(ops.flow_workspace_bytes(h, w), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.estimate_flow(cur, prev, out=out, work=work)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.estimate_flow(cur, prev, out=out, work=work)
    for c, p in pairs + pairs[:1]:
        cur.copy_(T(c))
        prev.copy_(T(p))
        graph.replay()
        torch.cuda.synchronize()
        eager = ops.estimate_flow(T(c), T(p))
        assert same_bits(out.cpu().numpy(), eager.cpu().numpy())
        assert out.abs().max().item() > 1.0


# ---------------------------------------------------------------- ClipStream(flow="estimate")
H, W, F = 24, 40, 5
THRESH = 2.0  # zeroes part of every warped matte of this clip (the default 15 zeroes nothing at this size)


class Clip:
    """A texture shifting by (1.5, -1) px per frame over random backgrounds, and the tiny seeded UNetSimple of
    tests/test_gpu_clip_stream.py."""

    def __init__(self):
        from oracle import models as om
        rs = np.random.RandomState(42)
        tex = ref.texture(H, W, 11)
        self.cmp0 = ref.render(tex, H, W, ref.shift_flow(H, W, -1.5, 1.0))
        self.cmp = np.stack([ref.render(tex, H, W, ref.shift_flow(H, W, 1.5 * t, -1.0 * t)) for t in range(F)])
        self.bg = rs.randint(0, 256, (F, H, W, 3)).astype(np.uint8)
        self.alpha0 = rs.uniform(0.0, 1.0, (H, W)).astype(np.float32)
        # the oracle's draws, the output conv scaled by 2^-6 (exact): unscaled, the sigmoid saturates and the matte
        # barely shows its third input
        p = om.unet_simple_params(np.random.RandomState(1))
        w, b = p["output"]
        p["output"] = (w * np.float32(2.0 ** -6), b * np.float32(2.0 ** -6))
        self.params = p
        self.bn = {"conv4": (rs.uniform(0.5, 1.5, 48).astype(np.float32), rs.normal(size=48).astype(np.float32) * 0.1),
                   "upconv2": (rs.uniform(0.5, 1.5, 32).astype(np.float32), rs.normal(size=32).astype(np.float32) * 0.1)}
        self._model, self._flows = None, {}

    def model(self, vgg0):
        from vmatting import unet_simple
        if self._model is None:
            np.random.seed(0)
            m = unet_simple.UNetSimple(unet_simple.Vgg16(vgg0, "bf16"), False, "bf16")
            self._model = m.load_params(self.params, self.bn)
        return self._model

    def flows(self, with_cmp0):
        """(backward [F,H,W,2], forward [F,H,W,2]) by ops.estimate_flow on each frame pair, downloaded; frame 0
        against cmp0, or zeros without it."""
        from vmatting import ops
        if with_cmp0 not in self._flows:
            bw, fw = np.zeros((F, H, W, 2), np.float32), np.zeros((F, H, W, 2), np.float32)
            for t in range(F):
                prev = self.cmp[t - 1] if t else (self.cmp0 if with_cmp0 else None)
                if prev is not None:
                    bw[t] = ops.estimate_flow(T(self.cmp[t]), T(prev)).cpu().numpy()
                    fw[t] = ops.estimate_flow(T(prev), T(self.cmp[t])).cpu().numpy()
            self._flows[with_cmp0] = bw, fw
        return self._flows[with_cmp0]

    def source(self, plate, flows=None, occlusion=False):
        """One set of arrays, overwritten after every yield (a decoder's ring)."""
        c, b = np.empty_like(self.cmp[0]), np.empty_like(self.bg[0])
        bw, fw = np.empty((H, W, 2), np.float32), np.empty((H, W, 2), np.float32)
        for t in range(F):
            c[...], b[...] = self.cmp[t], self.bg[t]
            if flows is None:
                yield c, (None if plate else b), None, None
            else:
                bw[...], fw[...] = flows[0][t], flows[1][t]
                yield c, (None if plate else b), bw, (fw if occlusion else None)
            c[...], b[...], bw[...], fw[...] = 0xA5, 0x5A, 1e3, -1e3


@pytest.fixture(scope="module")
def clip():
    return Clip()


def test_clip_flows_are_a_real_input(clip):
    """Preconditions: the estimated flows are the clip's shift, frame 0's flows against cmp0 are not zero, and the
    occlusion mask at THRESH zeroes some but not all of a warped matte."""
    from vmatting import flow
    bw, fw = clip.flows(True)
    for t in range(F):
        assert np.abs(bw[t][6:-6, 6:-6] - np.float32([1.5, -1.0])).max() < 0.75, t
        a = np.ones((H, W), np.float32)
        flow.correct_alpha(bw[t], fw[t], a, thresh=THRESH)
        assert 0 < (a == 0).sum() < H * W, t
    assert not clip.flows(False)[0][0].any() and same_bits(clip.flows(False)[0][1:], bw[1:])


def test_flow_tracker_equals_pairwise_estimates(clip, monkeypatch):
    """FlowTracker, the one running estimate behind ClipStream and FrameStream: every flow it writes is
    ops.estimate_flow of that frame pair, however the clip is cut; a flow it skips, and the bytes around its outputs
    and its pyramids, stay as they were; the last pyramid is carried, and a second pass finds nothing stale."""
    from vmatting import ops
    from vmatting.flow_track import FlowTracker
    opts, guard, mark = ops.flow_options("t", H, W, None), SENTINEL, -7.25
    cmp, cmp0 = T(clip.cmp), T(clip.cmp0)
    bw_want, fw_want = clip.flows(True)
    self0 = ops.estimate_flow(cmp[0], cmp[0]).cpu().numpy()  # frame 0 against itself
    # the library's count is a multiple of 4 floats at this size (and every other), so the tracker's round-up of a row
    # is a guard that real sizes never exercise: it is shown on a count that needs it
    count = ops.flow_pyramid_floats
    assert count(H, W, 6) % 4 == 0
    monkeypatch.setattr(ops, "flow_pyramid_floats", lambda h, w, levels=6: count(h, w, levels) + 1)
    odd = FlowTracker(H, W, opts, "cuda", frames=3)
    monkeypatch.undo()
    assert odd.rows.shape == (4, count(H, W, 6) + 4) and all(odd.rows[j].data_ptr() % 16 == 0 for j in range(4))

    def guarded(shape):
        """A tensor of ``shape`` between ``guard`` floats, everything holding the mark -> (the whole buffer, the view)."""
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * guard,), mark, dtype=torch.float32, device="cuda")
        return buf, buf[guard:guard + n].view(shape)

    def run(frames, cuts, seed, forward):
        """Two passes over the clip on one tracker -> the pass's (backward, forward | None) on the host, checked equal."""
        tr = FlowTracker(H, W, opts, "cuda", frames=frames)
        floats = tr.rows.shape[1]
        assert tr.rows.shape[0] == frames + 1 and floats % 4 == 0 and floats >= ops.flow_pyramid_floats(H, W, 6)
        assert all(tr.rows[j].data_ptr() % 16 == 0 for j in range(frames + 1)) and tr.rows.is_contiguous()
        pyr, tr.rows = guarded(tr.rows.shape)  # the same rows between guards (256 bytes: the alignment stays)
        assert all(tr.rows[j].data_ptr() % 16 == 0 for j in range(frames + 1))
        passes = []
        for _ in range(2):
            (b_buf, bw), (f_buf, fw) = guarded((F, H, W, 2)), guarded((F, H, W, 2))
            if seed is not None:
                tr.seed(seed)
            a = 0
            for k in cuts:
                tr.advance(cmp[a:a + k], bw[a:a + k], fw[a:a + k] if forward else None,
                           has_previous=a > 0 or seed is not None)
                a += k
            assert a == F
            torch.cuda.synchronize()
            for buf in (b_buf, f_buf, pyr):
                assert (buf[:guard] == mark).all() and (buf[-guard:] == mark).all(), "wrote outside its buffer"
            assert forward or (fw == mark).all()
            passes.append((bw.cpu().numpy(), fw.cpu().numpy() if forward else None))
        assert same_bits(passes[0][0], passes[1][0]) and (not forward or same_bits(passes[0][1], passes[1][1]))
        return passes[0]

    # frames=1, one frame per call, both directions: seeded with the frame before the clip, and with frame 0 itself
    bw, fw = run(1, (1,) * F, cmp0, True)
    assert same_bits(bw, bw_want) and same_bits(fw, fw_want)
    bw, fw = run(1, (1,) * F, cmp[0], True)
    assert same_bits(bw[1:], bw_want[1:]) and same_bits(fw[1:], fw_want[1:])
    assert same_bits(bw[0], self0) and same_bits(fw[0], self0)
    # frames=3 in two cuttings, nothing before the clip: frame 0's flows are skipped and keep the mark
    for cuts, forward in (((3, 2), True), ((1, 3, 1), False)):
        bw, fw = run(3, cuts, None, forward)
        assert (bw[0] == mark).all() and same_bits(bw[1:], bw_want[1:]), cuts
        assert not forward or ((fw[0] == mark).all() and same_bits(fw[1:], fw_want[1:])), cuts


@pytest.mark.parametrize("depth,graph,plate,occlusion,with_cmp0", [
    (1, True, False, False, False), (2, True, True, True, True), (3, True, True, False, True),
    (1, False, True, True, False), (2, False, False, True, True), (3, False, False, False, False),
    (1, True, True, True, True), (2, True, False, True, False)])
def test_clip_stream_estimate_equals_given_flows(clip, vgg0, depth, graph, plate, occlusion, with_cmp0):
    from vmatting import ClipStream
    m = clip.model(vgg0)
    kw = dict(depth=depth, static_bg=clip.bg[2] if plate else None, occlusion=occlusion, thresh=THRESH, out="f32",
              graph=graph, reuse_bg_tower=True)
    given = ClipStream(m, H, W, **kw)
    exp = np.stack(list(given.run(clip.source(plate, clip.flows(with_cmp0), occlusion), clip.alpha0)))
    assert len({exp[t].tobytes() for t in range(F)}) == F
    est = ClipStream(m, H, W, flow="estimate", **kw)
    for _ in range(2):  # a second run on the same object: no stale previous-frame pyramid
        got = np.stack(list(est.run(clip.source(plate), clip.alpha0, cmp0=clip.cmp0 if with_cmp0 else None)))
        for t in range(F):
            assert same_bits(got[t], exp[t]), "frame %d" % t
    assert est.stats["bg_tower_evals"] == (1 if plate else F) and est.stats["frames"] == F
    assert all(bool(s.graphs) == graph for s in est._slots)
    assert all(s.h_bw is None and s.d_bw is None and s.h_fw is None and s.d_fw is None for s in est._slots)


def test_clip_stream_estimate_depends_on_cmp0_and_runs_repeat(clip, vgg0):
    """cmp0 moves frame 0's matte (its flow is no longer zero), and runs with and without it alternate on one object
    without either leaving its previous frame behind."""
    from vmatting import ClipStream
    est = ClipStream(clip.model(vgg0), H, W, flow="estimate", out="f32")
    run = lambda cmp0: np.stack(list(est.run(clip.source(False), clip.alpha0, cmp0=cmp0)))  # noqa: E731
    a, b, a2, b2 = run(None), run(clip.cmp0), run(None), run(clip.cmp0)
    assert same_bits(a, a2) and same_bits(b, b2)
    assert not np.array_equal(a[0], b[0])
