"""The matte scorer on the GPU: ops.matte_score against the numpy restatement (tests/score_ref.py) — counts equal,
grad_map bit for bit, every sum within the reach of its own f64 additions — and MatteScorer's carry of the previous
frame across chunks, bit for bit."""

import numpy as np
import pytest
import torch

import flow_est_ref as fer
import score_ref as ref
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

TILE_H, TILE_W = 16, 64  # csrc/score.hip TH, TW
# 1 pixel; smaller than the halo; one below, equal to and one above the tile in both dimensions; several tiles each way
SHAPES = [(1, 1, 1), (2, 3, 5), (1, TILE_H - 1, TILE_W - 1), (1, TILE_H, TILE_W), (2, TILE_H + 1, TILE_W + 1), (3, 37, 70)]
DTYPES = [(np.float32, np.float32), (np.float32, np.uint8), (np.uint8, np.float32), (np.uint8, np.uint8)]
STAT_FILL, MAP_FILL = -7.25, -3.5


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def run(pred, gt, trimap=None, prev=None, backward=None):
    """ops.matte_score with stats and grad_map in the middle of sentinel-filled buffers, twice: (stats, grad_map) as
    numpy, after checking that the sentinels are intact and that both runs gave the same bits."""
    from vmatting import ops
    n, h, w = pred.shape
    args = [dev(pred), dev(gt), dev(trimap), None if prev is None else (dev(prev[0]), dev(prev[1])), dev(backward)]
    got = []
    for _ in range(2):
        sbuf = torch.full((n * 8 + 16,), STAT_FILL, dtype=torch.float64, device="cuda")
        mbuf = torch.full((n * h * w + 64,), MAP_FILL, dtype=torch.float32, device="cuda")
        out, gmap = sbuf[8:8 + n * 8].view(n, 8), mbuf[32:32 + n * h * w].view(n, h, w)
        res = ops.matte_score(*args, out=out, grad_map=gmap)
        assert res.data_ptr() == out.data_ptr()
        s, m = sbuf.cpu().numpy(), mbuf.cpu().numpy()
        assert (s[:8] == STAT_FILL).all() and (s[8 + n * 8:] == STAT_FILL).all()
        assert (m[:32] == MAP_FILL).all() and (m[32 + n * h * w:] == MAP_FILL).all()
        got.append((s[8:8 + n * 8].reshape(n, 8), m[32:32 + n * h * w].reshape(n, h, w)))
    assert np.array_equal(bits(got[0][0]), bits(got[1][0])) and np.array_equal(bits(got[0][1]), bits(got[1][1]))
    for a, b in zip(args[:3], (pred, gt, trimap)):  # the inputs are only read
        assert b is None or a.cpu().numpy().tobytes() == np.ascontiguousarray(b).tobytes()
    return got[0]


def compare(got, pred, gt, trimap=None, prev=None, backward=None, what=""):
    """The kernel's (stats, grad_map) against the restatement: counts equal, grad_map the same bits, every sum within
    relative N * 2^-52 of the exactly rounded sum of the restatement's N f32 terms.  Returns the restatement's frames."""
    stats, gmap = got
    frames = ref.terms(pred, gt, trimap, prev, backward)
    want = ref.stats(pred, gt, trimap, prev, backward, frames=frames)
    assert np.array_equal(bits(gmap), bits(ref.grad_map(pred, gt))), what
    assert np.array_equal(stats[:, [0, 6, 7]], want[:, [0, 6, 7]]), what
    for j in range(len(frames)):
        for e in (1, 2, 3, 4, 5):
            terms = want[j, 6] if e == 5 else want[j, 0]
            tol = terms * 2.0 ** -52 * want[j, e]
            print("%s frame %d entry %d: %r against %r, %d terms, |diff| %.3g, bound %.3g" %
                  (what, j, e, stats[j, e], want[j, e], terms, abs(stats[j, e] - want[j, e]), tol))
            assert abs(stats[j, e] - want[j, e]) <= tol, (what, j, e)
    return frames


def make(n, h, w, dtypes, seed):
    pred = ref.mattes(n, h, w, seed, dtypes[0], wild=True)  # f32: NaN, values below 0 and above 1
    gt = ref.mattes(n, h, w, seed + 1, dtypes[1])
    prev = (ref.mattes(1, h, w, seed + 2, dtypes[0], wild=True)[0], ref.mattes(1, h, w, seed + 3, dtypes[1])[0])
    return pred, gt, prev


@pytest.mark.parametrize("dtypes", DTYPES, ids=lambda d: "%s-%s" % (d[0].__name__, d[1].__name__))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_restatement(shape, dtypes):
    n, h, w = shape
    pred, gt, prev = make(n, h, w, dtypes, seed=17)
    if dtypes[0] == np.float32 and pred.size > 100:
        assert np.isnan(pred).any() and (pred < 0).any() and (pred > 1).any()
    flows = {"none": None, "zero": np.zeros((n, h, w, 2), np.float32), "wild": ref.wild_flow(n, h, w, 23)}
    tris = {"none": None, "random": ref.trimaps(n, h, w, 29), "known": ref.trimaps(n, h, w, 31, "known")}
    for tname, tri in tris.items():
        for fname, fl in flows.items():
            for pv in (None, prev):
                what = "trimap %s, flow %s, prev %s" % (tname, fname, pv is not None)
                compare(run(pred, gt, tri, pv, fl), pred, gt, tri, pv, fl, what)


def test_a_smooth_flow_keeps_most_pixels_in_frame():
    from oracle.flow import smooth_flow
    n, h, w = 3, 37, 70
    pred, gt, prev = make(n, h, w, (np.float32, np.float32), seed=41)
    fl = np.stack([smooth_flow(h, w, seed=3, amp=3.0)] * n)
    assert fl.dtype == np.float32
    frames = compare(run(pred, gt, None, prev, fl), pred, gt, None, prev, fl, "smooth flow")
    share = sum(t["take"].sum() for t in frames) / float(n * h * w)
    print("the restatement keeps %.1f %% of the pixels in frame" % (100 * share))
    assert share >= 0.8
    assert all((t["me"][t["take"]] > 0).any() for t in frames)


def offset(a, lead):
    """``a`` on the device as a contiguous view that starts ``lead`` elements into a larger buffer."""
    src = dev(a)
    buf = torch.zeros(a.size + lead + 8, dtype=src.dtype, device="cuda")
    view = buf[lead:lead + a.size].view(a.shape)
    view.copy_(src)
    return view


@pytest.mark.parametrize("dtypes", DTYPES, ids=lambda d: "%s-%s" % (d[0].__name__, d[1].__name__))
def test_offset_slices_take_the_scalar_form_and_give_the_same_bits(dtypes):
    from vmatting import ops
    n, h, w = 2, 36, 68  # w is a multiple of 4: the aligned call stages with wide loads
    pred, gt, prev = make(n, h, w, dtypes, seed=47)
    tri, fl = ref.trimaps(n, h, w, 53), ref.wild_flow(n, h, w, 59)
    aligned = run(pred, gt, tri, prev, fl)
    compare(aligned, pred, gt, tri, prev, fl, "aligned")
    d_pred, d_gt, d_tri = offset(pred, 1), offset(gt, 1), offset(tri, 1)
    d_prev = (offset(prev[0], 1), offset(prev[1], 1))
    d_fl = offset(fl, 2)  # (one flow vector: backward stays 8-byte aligned)
    wide = lambda dt: 16 if dt == np.float32 else 4
    assert d_pred.data_ptr() % wide(dtypes[0]) and d_gt.data_ptr() % wide(dtypes[1])
    sbuf = torch.full((n * 8 + 2,), STAT_FILL, dtype=torch.float64, device="cuda")
    mbuf = torch.full((n * h * w + 2,), MAP_FILL, dtype=torch.float32, device="cuda")
    out, gmap = sbuf[1:1 + n * 8].view(n, 8), mbuf[1:1 + n * h * w].view(n, h, w)
    ops.matte_score(d_pred, d_gt, d_tri, d_prev, d_fl, out=out, grad_map=gmap)
    assert np.array_equal(bits(out.cpu().numpy()), bits(aligned[0]))
    assert np.array_equal(bits(gmap.cpu().numpy()), bits(aligned[1]))
    s, m = sbuf.cpu().numpy(), mbuf.cpu().numpy()
    assert s[0] == STAT_FILL and s[-1] == STAT_FILL and m[0] == MAP_FILL and m[-1] == MAP_FILL
    # and one operand at a time
    for k in range(2):
        a = [dev(pred), dev(gt)]
        a[k] = (d_pred, d_gt)[k]
        got = ops.matte_score(a[0], a[1], dev(tri), (dev(prev[0]), dev(prev[1])), dev(fl))
        assert np.array_equal(bits(got.cpu().numpy()), bits(aligned[0]))


def test_allocated_buffers_and_the_librarys_refusals():
    from vmatting import ops
    n, h, w = 2, 9, 12
    pred, gt, _ = make(n, h, w, (np.float32, np.uint8), seed=61)
    got = ops.matte_score(dev(pred), dev(gt))
    assert got.dtype == torch.float64 and tuple(got.shape) == (n, 8)
    want = ref.stats(pred, gt)
    assert np.array_equal(got.cpu().numpy()[:, 0], want[:, 0]) and np.allclose(got.cpu().numpy(), want, rtol=1e-12)
    with pytest.raises(ValueError, match="work"):
        ops.matte_score(dev(pred), dev(gt), work=torch.zeros(8, dtype=torch.uint8, device="cuda"))
    fl = torch.zeros(n * h * w * 2 + 1, dtype=torch.float32, device="cuda")[1:].view(n, h, w, 2)
    with pytest.raises(ValueError, match="matte_score: matte_score: backward must be 8-byte aligned"):
        ops.matte_score(dev(pred), dev(gt), backward=fl)
    torch.cuda.synchronize()


def test_captured_call_replays_on_new_inputs():
    from vmatting import ops
    n, h, w = 3, 37, 70
    d_pred = torch.zeros((n, h, w), dtype=torch.float32, device="cuda")
    d_gt = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    d_tri = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    d_prev = (torch.zeros((h, w), dtype=torch.float32, device="cuda"), torch.zeros((h, w), dtype=torch.uint8, device="cuda"))
    d_fl = torch.zeros((n, h, w, 2), dtype=torch.float32, device="cuda")
    out = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    gmap = torch.zeros((n, h, w), dtype=torch.float32, device="cuda")
    work = torch.zeros(ops.matte_score_workspace_bytes(n, h, w), dtype=torch.uint8, device="cuda")
    call = lambda o, m: ops.matte_score(d_pred, d_gt, d_tri, d_prev, d_fl, out=o, grad_map=m, work=work)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(out, gmap)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(out, gmap)
    for seed in (1, 2, 3):
        pred, gt, prev = make(n, h, w, (np.float32, np.uint8), seed)
        tri, fl = ref.trimaps(n, h, w, seed + 5), ref.wild_flow(n, h, w, seed + 9)
        for d, a in ((d_pred, pred), (d_gt, gt), (d_tri, tri), (d_prev[0], prev[0]), (d_prev[1], prev[1]), (d_fl, fl)):
            d.copy_(dev(a))
        g.replay()
        replayed = (out.cpu().numpy(), gmap.cpu().numpy())
        eager = call(None, None).cpu().numpy()
        assert np.array_equal(bits(replayed[0]), bits(eager))
        compare(replayed, pred, gt, tri, prev, fl, "replay %d" % seed)


# ---------------------------------------------------------------- MatteScorer
H, W, F = 24, 40, 19


@pytest.fixture(scope="module")
def clip():
    """19 frames of f32 mattes, uint8 ground truth, trimaps and flows, and the restatement's table for the clip."""
    pred, gt, _ = make(F, H, W, (np.float32, np.uint8), seed=71)
    tri, fl = ref.trimaps(F, H, W, 73), ref.wild_flow(F, H, W, 79)
    return pred, gt, tri, fl, ref.stats(pred, gt, tri, None, fl)


def chunks(sizes):
    a = 0
    for k in sizes:
        yield a, a + k
        a += k


def test_scorer_chunking_does_not_change_a_bit(clip):
    from vmatting import MatteScorer, ops
    pred, gt, tri, fl, want = clip
    tables = []
    for sizes in ((8, 8, 3), (1,) * F, (F,)):
        sc = MatteScorer(H, W, flow="given")
        for a, b in chunks(sizes):
            assert sc.add(pred[a:b], gt[a:b], tri[a:b], fl[a:b]) is sc
        assert sc.frames == F
        tables.append(sc.stats())
    one = ops.matte_score(dev(pred), dev(gt), dev(tri), None, dev(fl)).cpu().numpy()
    for t in tables:
        assert t.shape == (F, 8) and np.array_equal(bits(t), bits(one))
    assert np.array_equal(one[:, [0, 6]], want[:, [0, 6]]) and np.allclose(one, want, rtol=1e-12, atol=0)
    assert (one[0, 4:] == 0).all() and (one[1:, 4] > 0).all() and (one[1:, 6] > 0).all()
    # the figures are score_summary of the table
    r, s = sc.result(), ops.score_summary(one, False, True)
    assert all(np.array_equal(r[k], s[k], equal_nan=True) for k in ops.SCORE_FIGURES) and r["clip"] == s["clip"]
    assert np.isnan(r["dtssd"][0]) and not np.isnan(r["dtssd"][1:]).any() and r["clip"]["messddt"] > 0


def test_scorer_device_tensors_and_reset(clip):
    from vmatting import MatteScorer
    pred, gt, tri, fl, _ = clip
    host, device = MatteScorer(H, W, flow="given"), MatteScorer(H, W, flow="given")
    d = [dev(a) for a in (pred, gt, tri, fl)]
    for a, b in chunks((8, 8, 3)):
        host.add(pred[a:b], gt[a:b], tri[a:b], fl[a:b])
        device.add(*(t[a:b] for t in d))
    assert np.array_equal(bits(host.stats()), bits(device.stats()))
    for t, a in zip(d, (pred, gt, tri, fl)):  # used in place, and only read
        assert np.array_equal(t.cpu().numpy(), a, equal_nan=True)
    # reset() forgets the clip: the same frames again give the same table, not a continuation
    first = host.stats()
    host.reset()
    assert host.frames == 0 and host.stats().shape == (0, 8)
    host.add(gt[:5], gt[:5], None, fl[:5])  # (other dtypes than before)
    with pytest.raises(TypeError, match="reset"):
        host.add(pred[5:8], gt[5:8], None, fl[5:8])
    host.reset()
    for a, b in chunks((F,)):
        host.add(pred[a:b], gt[a:b], tri[a:b], fl[a:b])
    assert np.array_equal(bits(host.stats()), bits(first)) and (host.stats()[0, 4:] == 0).all()
    # without a flow: no MESSDdt entries, the rest unchanged
    plain = MatteScorer(H, W)
    plain.add(pred, gt, tri)
    t = plain.stats()
    assert (t[:, 5:] == 0).all() and np.array_equal(bits(t[:, :5]), bits(first[:, :5]))
    assert np.isnan(plain.result()["clip"]["messddt"])


def test_scorer_estimated_flows_equal_given_estimates(monkeypatch):
    from vmatting import MatteScorer, ops
    n, opts = 5, {"warps": 2, "iters": 4}
    tex = fer.texture(H, W, 7)
    cmp = np.stack([fer.render(tex, H, W, None if t == 0 else fer.shift_flow(H, W, 1.5 * t, -1.0 * t)) for t in range(n)])
    pred, gt, _ = make(n, H, W, (np.uint8, np.float32), seed=83)
    flows = np.zeros((n, H, W, 2), np.float32)
    for t in range(1, n):
        flows[t] = ops.estimate_flow(dev(cmp[t]), dev(cmp[t - 1]), **opts).cpu().numpy()
    assert np.abs(flows[1:]).max() > 0.5
    given = MatteScorer(H, W, flow="given").add(pred, gt, None, flows).stats()
    assert (given[1:, 5] > 0).all()
    pairs, from_pyramids = [], ops.flow_from_pyramids  # the pairs a scorer estimates: frame 0 of a clip has none
    monkeypatch.setattr(ops, "flow_from_pyramids", lambda *a, **kw: pairs.append(1) or from_pyramids(*a, **kw))
    for sizes in ((n,), (2, 1, 2)):
        est = MatteScorer(H, W, flow="estimate", flow_options=opts)
        for clip in range(2):  # the second after reset(): frame 0 has no previous frame again, and its row no flow
            del pairs[:]
            for a, b in chunks(sizes):
                est.add(pred[a:b], gt[a:b], None, None, cmp[a:b])
            assert np.array_equal(bits(est.stats()), bits(given)), (sizes, clip)
            assert len(pairs) == n - 1, (sizes, clip)
            est.reset()


def test_frame_stream_u8_mattes_feed_the_scorer(vgg0):
    from vmatting import FrameStream, MatteScorer, unet
    h, w, n, chunk = 64, 96, 6, 4
    rs = np.random.RandomState(5)
    cmp, bg = (rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8) for _ in range(2))
    tri = ref.trimaps(n, h, w, 89)
    gt = ref.mattes(n, h, w, 97, np.uint8)
    np.random.seed(0)
    model = unet.UNetVideo(vgg0, dtype="bf16", device="cuda").prepare()
    sc = MatteScorer(h, w)
    mattes = []
    source = ((cmp[a:b], bg[a:b], tri[a:b]) for a, b in chunks((4, 2)))
    for (a, b), m in zip(chunks((4, 2)), FrameStream(model, h, w, chunk=chunk, out="u8").run(source)):
        assert m.dtype == np.uint8 and m.shape == (b - a, h, w)
        sc.add(m, gt[a:b], tri[a:b])
        mattes.append(m.copy())
    mattes = np.concatenate(mattes)
    got, want = sc.stats(), ref.stats(mattes, gt, tri)
    assert np.array_equal(got[:, 0], want[:, 0]) and (got[:, 0] > 0).all() and np.allclose(got, want, rtol=1e-12, atol=0)
    assert sc.result()["clip"]["sad"] > 0


def test_reader_score_matte_equals_the_restatement():
    from vmatting import ops, reader
    h, w = 37, 70
    pred, gt, _ = make(1, h, w, (np.float32, np.uint8), seed=101)
    tri = ref.trimaps(1, h, w, 103)
    for t in (None, tri):
        want = ops.score_summary(ref.stats(pred, gt, t))
        got = reader.score_matte(pred[0], gt[0], None if t is None else t[0])
        assert sorted(got) == ["count", "grad", "mse", "sad"] and got["count"] == want["count"][0] > 0
        for k in ("sad", "mse", "grad"):
            assert isinstance(got[k], float) and abs(got[k] - want[k][0]) <= got["count"] * 2.0 ** -52 * want[k][0], k
    # float64 mattes are rounded to f32 first
    assert reader.score_matte(pred[0].astype(np.float64), gt[0]) == reader.score_matte(pred[0], gt[0])
    empty = reader.score_matte(pred[0], gt[0], ref.trimaps(1, h, w, 1, "known")[0])
    assert empty["count"] == 0 and all(np.isnan(empty[k]) for k in ("sad", "mse", "grad"))
