"""CPU checks of the matte scorer (vm_matte_score in csrc/score.hip, ops.matte_score / ops.score_summary, MatteScorer,
reader.score_matte): the numpy restatement the GPU tests compare against (tests/score_ref.py) has the taps and the
properties the definition promises, score_summary's arithmetic, and every argument check happens on the host, before
any GPU call."""

import numpy as np
import pytest
import torch

import score_ref as ref


# ---------------------------------------------------------------------------------------------- the restatement
def test_tap_literals_are_the_formula_rounded_to_f32():
    g64, d64 = ref.taps64()
    assert np.array_equal(ref.G, g64.astype(np.float32))
    d32 = d64.astype(np.float32)
    assert d32[4] == 0 and np.signbit(d32[4])          # the formula gives -0 for the centre tap ...
    d32[4] = 0.0
    assert np.array_equal(ref.D, d32) and not np.signbit(ref.D[4])  # ... and the definition takes +0
    assert np.array_equal(ref.D, -ref.D[::-1]) and np.array_equal(ref.G, ref.G[::-1])
    # the literals of the header and of the kernel are these
    import os
    from conftest import PKG, REPO
    want_g = " ".join("%sf" % v for v in ref.G)
    want_d = " ".join(("+0.0f" if i == 4 else "%sf" % v) for i, v in enumerate(ref.D))
    header = " ".join(open(os.path.join(REPO, "include", "vmatting.h")).read().replace("*", " ").split())
    assert want_g in header and want_d in header
    kernel = " ".join(open(os.path.join(PKG, "csrc", "score.hip")).read().split())
    assert ", ".join("%sf" % v for v in ref.G) in kernel
    assert ", ".join(("0.0f" if i == 4 else "%sf" % v) for i, v in enumerate(ref.D)) in kernel


def test_gx_matches_a_float64_9x9_correlation():
    """The separable f32 passes against an independent, non-separable float64 correlation with edge padding: two 9-term
    f32 accumulations (a product and an add per term, (1 + 2^-24)^20 - 1 ~ 20 * 2^-24 in all) on values bounded by
    sum|G| * sum|D| * max|x|."""
    h, w = 20, 23
    x = np.random.RandomState(4).uniform(0, 1, (h, w)).astype(np.float32)
    g64, d64 = ref.G.astype(np.float64), ref.D.astype(np.float64)
    p = np.pad(x.astype(np.float64), 4, mode="edge")
    kx, ky = np.outer(g64, d64), np.outer(d64, g64)  # [dy, dx]
    want_gx, want_gy = np.zeros((h, w)), np.zeros((h, w))
    for y in range(h):
        for xx in range(w):
            win = p[y:y + 9, xx:xx + 9]
            want_gx[y, xx], want_gy[y, xx] = (kx * win).sum(), (ky * win).sum()
    gx, gy = ref.gradients(x)
    assert gx.dtype == np.float32 and gy.dtype == np.float32
    bound = 20 * 2.0 ** -24 * np.abs(g64).sum() * np.abs(d64).sum() * float(np.abs(x).max())
    ex, ey = np.abs(gx - want_gx).max(), np.abs(gy - want_gy).max()
    print("gx: %.3g, gy: %.3g from float64, bound %.3g" % (ex, ey, bound))
    assert ex <= bound and ey <= bound
    assert np.abs(want_gx).max() > 0.05


def test_equal_mattes_score_zero():
    for dt in (np.float32, np.uint8):
        m = ref.mattes(3, 9, 14, 1, dt)
        fl = np.zeros((3, 9, 14, 2), np.float32)
        s = ref.stats(m, m.copy(), ref.trimaps(3, 9, 14, 2), None, fl)
        assert (s[:, 0] > 0).all() and (s[:, 1:6] == 0).all() and (s[1:, 6] == s[1:, 0]).all() and s[0, 6] == 0


def test_constant_offset_gives_sad_c_times_count():
    n, h, w, c = 2, 12, 17, 0.25
    gt = np.full((n, h, w), 0.5, np.float32)
    pred = gt + np.float32(c)
    tri = ref.trimaps(n, h, w, 3)
    s = ref.stats(pred, gt, tri)
    count = ((tri != 0) & (tri != 255)).sum((1, 2))
    assert np.array_equal(s[:, 0], count) and np.array_equal(s[:, 1], c * count)
    assert np.array_equal(s[:, 2], c * c * count)
    # uint8 against f32: 51 / 255 is 0.2 in f32
    s = ref.stats(np.full((1, 4, 5), 51, np.uint8), np.zeros((1, 4, 5), np.float32))
    assert s[0, 0] == 20 and s[0, 1] == 20 * float(np.float32(0.2))


def test_a_still_clip_with_zero_flow_has_no_temporal_error():
    pred, gt = ref.mattes(1, 10, 13, 5), ref.mattes(1, 10, 13, 6, np.uint8)
    pred, gt = np.repeat(pred, 4, 0), np.repeat(gt, 4, 0)
    s = ref.stats(pred, gt, None, (pred[0], gt[0]), np.zeros((4, 10, 13, 2), np.float32))
    assert (s[:, 2] > 0).all() and (s[:, 4] == 0).all() and (s[:, 5] == 0).all() and (s[:, 6] == 130).all()


def test_a_whole_pixel_translation_with_its_flow_has_no_messddt():
    n, h, w, dx, dy = 3, 16, 21, 3, -2
    pred0, gt0 = ref.mattes(1, h + 8 * n, w + 8 * n, 7)[0], ref.mattes(1, h + 8 * n, w + 8 * n, 8)[0]
    # frame j shows the planes shifted by j * (dx, dy): frame j at (x, y) is frame j - 1 at (x + dx, y + dy)
    crop = lambda p, j: p[12 + j * dy:12 + j * dy + h, 4 + j * dx:4 + j * dx + w]
    pred, gt = (np.stack([crop(p, j) for j in range(n)]) for p in (pred0, gt0))
    flow = np.zeros((n, h, w, 2), np.float32)
    flow[..., 0], flow[..., 1] = dx, dy
    s = ref.stats(pred, gt, None, None, flow)
    assert (s[1:, 6] == (h - abs(dy)) * (w - abs(dx))).all() and (s[1:, 5] == 0).all() and (s[1:, 4] > 0).all()
    assert (s[0, 4:] == 0).all()
    # the other way round the error does not follow the flow
    flow[..., 0], flow[..., 1] = -dx, -dy
    assert (ref.stats(pred, gt, None, None, flow)[1:, 5] > 0).all()


def test_an_all_known_trimap_gives_nan_figures_left_out_of_the_means():
    from vmatting import ops
    n, h, w = 3, 8, 11
    pred, gt = ref.mattes(n, h, w, 9), ref.mattes(n, h, w, 10)
    tri = ref.trimaps(n, h, w, 11)
    tri[1] = ref.trimaps(1, h, w, 12, "known")[0]
    s = ref.stats(pred, gt, tri, None, np.zeros((n, h, w, 2), np.float32))
    assert s[1, 0] == 0 and (s[1] == 0).all()
    r = ops.score_summary(s, False, True)
    for k in ops.SCORE_FIGURES:
        assert np.isnan(r[k][1]), k
    assert np.isnan(r["dtssd"][0]) and np.isnan(r["messddt"][0]) and not np.isnan(r["sad"][0])
    assert r["clip"]["sad"] == (s[0, 1] + s[2, 1]) / 2 and r["clip"]["dtssd"] == np.sqrt(s[2, 4] / s[2, 0])
    # every frame empty: the clip figures are NaN too
    r = ops.score_summary(ref.stats(pred, gt, ref.trimaps(n, h, w, 1, "known")))
    assert all(np.isnan(v) for v in r["clip"].values())


# ---------------------------------------------------------------------------------------------- score_summary
def test_score_summary_arithmetic():
    from vmatting import ops
    s = np.array([[10, 5.0, 2.5, 7.0, 0.0, 0.0, 0, 0],
                  [20, 8.0, 5.0, 3.0, 1.8, 4.0, 16, 0],
                  [4, 1.0, 1.0, 2.0, 0.36, 9.0, 0, 0]], np.float64)
    r = ops.score_summary(s, first_has_prev=False, has_flow=True)
    assert np.array_equal(r["count"], [10, 20, 4]) and np.array_equal(r["taking_part"], [0, 16, 0])
    assert np.array_equal(r["sad"], [5, 8, 1]) and np.array_equal(r["grad"], [7, 3, 2])
    assert np.array_equal(r["mse"], [0.25, 0.25, 0.25])
    assert np.isnan(r["dtssd"][0]) and np.array_equal(r["dtssd"][1:], np.sqrt(np.array([1.8 / 20, 0.36 / 4])))
    assert np.isnan(r["messddt"][0]) and r["messddt"][1] == 0.25 and np.isnan(r["messddt"][2])  # nobody took part
    assert r["clip"] == {"sad": 14 / 3, "mse": 0.25, "grad": 4.0, "dtssd": float(np.mean(r["dtssd"][1:])), "messddt": 0.25}
    # with prev the first frame has its temporal figures; without a flow there is no messddt
    r = ops.score_summary(torch.from_numpy(s), first_has_prev=True)
    assert r["dtssd"][0] == 0 and np.isnan(r["messddt"]).all() and np.isnan(r["clip"]["messddt"])
    assert ops.score_summary(np.zeros((0, 8)))["sad"].shape == (0,)
    with pytest.raises(ValueError):
        ops.score_summary(np.zeros((3, 7)))
    with pytest.raises(ValueError):
        ops.score_summary(np.zeros(8))
    with pytest.raises(TypeError):
        ops.score_summary(np.zeros((3, 8), np.float32))


# ---------------------------------------------------------------------------------------------- C entry point
def test_matte_score_rejects_bad_arguments():
    from vmatting import _lib
    lib = _lib.lib()
    P, Q = 64, 68  # non-null addresses (validation never dereferences them); Q is 4-byte but not 8-byte aligned
    F32, U8 = _lib.VM_F32, _lib.VM_U8
    #        pred dt  gt dt  trimap prev_pred prev_gt backward n h w stats grad_map work
    cases = [(None, F32, P, F32, P, None, None, None, 2, 3, 5, P, None, P),  # NULLs
             (P, F32, None, U8, None, None, None, None, 2, 3, 5, P, None, P),
             (P, U8, P, F32, None, None, None, None, 2, 3, 5, None, P, P),
             (P, U8, P, U8, None, P, P, P, 2, 3, 5, P, P, None),
             (P, F32, P, F32, None, None, None, None, 0, 3, 5, P, None, P),  # n, h, w < 1
             (P, F32, P, F32, None, None, None, None, 2, 0, 5, P, None, P),
             (P, F32, P, F32, None, None, None, None, 2, 3, -1, P, None, P),
             (P, _lib.VM_BF16, P, F32, None, None, None, None, 2, 3, 5, P, None, P),  # dtypes
             (P, F32, P, _lib.VM_F64, None, None, None, None, 2, 3, 5, P, None, P),
             (P, 7, P, U8, None, None, None, None, 2, 3, 5, P, None, P),
             (P, U8, P, -1, None, None, None, None, 2, 3, 5, P, None, P),
             (P, F32, P, F32, None, P, None, None, 2, 3, 5, P, None, P),  # one of prev_pred / prev_gt
             (P, F32, P, U8, P, None, P, P, 2, 3, 5, P, None, P),
             (P, F32, P, F32, None, None, None, Q, 2, 3, 5, P, None, P),  # misaligned backward, stats, work
             (P, F32, P, F32, None, None, None, None, 2, 3, 5, Q, None, P),
             (P, U8, P, U8, None, None, None, None, 2, 3, 5, P, None, Q)]
    for case in cases:
        rc = lib.vm_matte_score(*case, None)
        assert rc == _lib.VM_EINVAL, case
        assert b"matte_score" in lib.vm_last_error(), case
        with pytest.raises(ValueError):
            _lib.check(rc, "matte_score")
    for shape in ((0, 3, 5), (2, 0, 5), (2, 3, 0), (-1, 3, 5)):
        assert lib.vm_matte_score_workspace_bytes(*shape) == 0
    nbytes = lib.vm_matte_score_workspace_bytes(2, 3, 5)
    assert nbytes > 0 and nbytes % 8 == 0
    assert lib.vm_matte_score_workspace_bytes(4, 3, 5) == 2 * nbytes
    assert _lib.ABI_VERSION == 1


# ---------------------------------------------------------------------------------------------- ops wrapper
def test_ops_matte_score_checks_before_the_device():
    from vmatting import ops
    n, h, w = 2, 4, 6
    pf, pu = torch.zeros((n, h, w), dtype=torch.float32), torch.zeros((n, h, w), dtype=torch.uint8)
    fl = torch.zeros((n, h, w, 2), dtype=torch.float32)
    for bad in (pf.double(), pf.half(), pf.to(torch.int8), pf.numpy()):  # dtypes and types
        with pytest.raises(TypeError):
            ops.matte_score(bad, pf)
        with pytest.raises(TypeError):
            ops.matte_score(pu, bad)
    for kw in (dict(trimap=pf), dict(trimap=pu.numpy()), dict(backward=fl.double()), dict(prev=pf[0]),
               dict(prev=(pf[0],)), dict(prev=(pu[0], pf[0])),           # prev carries the dtypes of pred and gt
               dict(prev=(pf[0], pu[0].to(torch.int8))), dict(out=torch.zeros((n, 8), dtype=torch.float32)),
               dict(grad_map=torch.zeros((n, h, w), dtype=torch.float64))):
        with pytest.raises(TypeError):
            ops.matte_score(pf, pu, **kw)
    for args, kw in (((pf[0], pu[0]), {}), ((pf[None], pu[None]), {}), ((pf[:, :0], pu[:, :0]), {}),  # shapes
                     ((pf, pu[:1]), {}), ((pf, pu[:, :3]), {}), ((pf, pu), dict(trimap=pu[..., :5])),
                     ((pf, pu), dict(prev=(pf[0, :3], pu[0, :3]))), ((pf, pu), dict(prev=(pf, pu))),
                     ((pf, pu), dict(backward=fl[:1])), ((pf, pu), dict(backward=fl[..., 0])),
                     ((pf, pu), dict(out=torch.zeros((n, 7), dtype=torch.float64))),
                     ((pf, pu), dict(out=torch.zeros((n + 1, 8), dtype=torch.float64))),
                     ((pf, pu), dict(grad_map=torch.zeros((n, h), dtype=torch.float32))),
                     ((pf.transpose(1, 2), pu.transpose(1, 2).contiguous()), {}),       # not contiguous
                     ((pf, pu), dict(backward=torch.zeros((n, h, w, 4), dtype=torch.float32)[..., :2]))):
        with pytest.raises(ValueError):
            ops.matte_score(*args, **kw)
    # right tensors, but on the host
    for args, kw in (((pf, pu), {}), ((pu, pf), dict(trimap=pu, prev=(pu[0], pf[0]), backward=fl))):
        with pytest.raises(TypeError, match="ROCm device tensors"):
            ops.matte_score(*args, **kw)


# ---------------------------------------------------------------------------------------------- MatteScorer
def test_matte_scorer_arguments():
    from vmatting import MatteScorer
    for bad in (dict(h=0), dict(w=-3), dict(flow="forward"), dict(flow=True), dict(flow="given", flow_options={}),
                dict(flow_options={"levels": 3}), dict(device="cpu"), dict(flow="estimate", flow_options={"sweeps": 3}),
                dict(flow="estimate", flow_options={"iters": 0}), dict(h=8, flow="estimate")):  # the estimator's 16 x 16
        kw = dict(h=24, w=40)
        kw.update(bad)
        with pytest.raises(ValueError):
            MatteScorer(**kw)
    for bad in (dict(h=2.0), dict(w="40"), dict(h=True), dict(flow="estimate", flow_options={"warps": 2.5})):
        kw = dict(h=24, w=40)
        kw.update(bad)
        with pytest.raises(TypeError):
            MatteScorer(**kw)
    h, w = 24, 40
    pf, pu = np.zeros((3, h, w), np.float32), np.zeros((3, h, w), np.uint8)
    fl, cmp = np.zeros((3, h, w, 2), np.float32), np.zeros((3, h, w, 3), np.uint8)
    plain, given, est = MatteScorer(h, w), MatteScorer(h, w, flow="given"), MatteScorer(h, w, flow="estimate")
    assert est.flow_options == {"levels": 6, "warps": 3, "iters": 20, "alpha": 15.0} and plain.flow_options is None
    assert MatteScorer(h, w, flow="estimate", flow_options={"levels": 2, "alpha": 4}).flow_options["alpha"] == 4.0
    assert plain.check_chunk(pf, pu, pu) == 3 and given.check_chunk(pu[:1], pf[:1], None, fl[:1]) == 1
    assert est.check_chunk(pf, pf, pu, None, cmp) == 3
    bad = [(plain, (pf, pu, None, fl)), (plain, (pf, pu, None, None, cmp)),  # flows with the wrong mode, or missing
           (given, (pf, pu)), (given, (pf, pu, None, None, cmp)), (given, (pf, pu, None, fl, cmp)),
           (est, (pf, pu)), (est, (pf, pu, None, fl)),
           (plain, (pf[0], pu[0])), (plain, (pf[:, :5], pu[:, :5])), (plain, (pf[:0], pu[:0])),  # shapes
           (plain, (pf, pu[:2])), (plain, (pf, pu, pu[:, :, :7])), (given, (pf, pu, None, fl[..., :1])),
           (given, (pf, pu, None, fl[:2])), (est, (pf, pu, None, None, cmp[..., :2])), (est, (pf, pu, None, None, cmp[1:])),
           (plain, (pf.astype(np.float64), pu)), (plain, (pf, pu.astype(np.int8))), (plain, (pf, pu, pf)),  # dtypes
           (given, (pf, pu, None, fl.astype(np.float64))), (est, (pf, pu, None, None, cmp.astype(np.float32))),
           (plain, (pf.tolist(), pu)), (plain, (pf, None)),                                      # types
           (plain, (torch.from_numpy(pf), pu)), (plain, (pf, pu, torch.from_numpy(pu)))]         # host tensors
    for scorer, args in bad:
        with pytest.raises((ValueError, TypeError)):
            scorer.add(*args)
        assert scorer.frames == 0 and scorer._prev is None and scorer._work is None  # nothing reached the device
    # a dtype change between calls
    plain._dtypes = (torch.float32, torch.uint8)
    assert plain.check_chunk(pf, pu) == 3
    for args in ((pu, pu), (pf, pf), (pu, pf)):
        with pytest.raises(TypeError, match="reset"):
            plain.add(*args)
    plain.reset()
    assert plain.check_chunk(pu, pf) == 3
    assert plain.stats().shape == (0, 8) and np.isnan(plain.result()["clip"]["sad"])


# ---------------------------------------------------------------------------------------------- reader.score_matte
def test_reader_score_matte_checks_before_the_device():
    from vmatting import reader
    pf, pu = np.zeros((4, 6), np.float32), np.zeros((4, 6), np.uint8)
    for args in ((pf.astype(np.float16), pu), (pf, pu.astype(np.int32)), (pf, pu, pf), (pf, pu, pu.astype(bool))):
        with pytest.raises(TypeError):
            reader.score_matte(*args)
    for args in ((pf[None], pu[None]), (pf, pu[:3]), (pf[0], pu[0]), (pf, pu, pu[:, :5]), (pf[:0], pu[:0]),
                 (pf, pu, pu[None])):
        with pytest.raises(ValueError):
            reader.score_matte(*args)
    import reader as top
    assert top.score_matte is reader.score_matte
