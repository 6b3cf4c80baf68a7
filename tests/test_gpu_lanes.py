"""Every lane packing of the per-channel passes against the float64 references of tests/lane_ref.py:
csrc/elementwise.hip bn_partial / bn_apply / softmax (CP 1..64), their 8-channels-per-lane forms (TPG 1..64) and the
2-channel f32 pair kernel; csrc/train.hip bn_bwd_partial / bn_bwd_apply / relu_bwd / maxpool_bwd / relu_bwd_bias, their
8-channel forms and bn_bwd_apply2_f32; vm_common.h fold_columns.

Two tiers of pixel counts.  Small ([1,1,1], [1,7,9], [2,7,9], [2,19,33]): every channel count on each side of every
packing boundary, every dtype, every argument in turn (and all together) a channel slice of a wider buffer, both
settings of the A/B options for the 8-channel widths.  Seam (one case per CP, M just above 5 * 4096 * (256 / CP)): the
grid cap is passed, so the four-loads-in-flight bodies and their tails both run (and fold_columns' unrolled body where
the partial passes reach 4096 blocks, M >= 2^20).

What reaches which loop (per = 4096 * (256 / CP) pixels, the capped grid's one trip):
  * bn_apply_kernel, bn_bwd_apply, relu_bwd_kernel: the small tier runs the tail loop only (M <= 1254 < 3 per); the
    seam's M in (5 per, 5.13 per) gives one trip of the four-in-flight body and one or two of the tail.
  * bn_partial_kernel, bn_bwd_partial: their step is nblk * 4 * (64 / CP) pixels with nblk = M / 256 blocks at most, so
    M = 1254 already takes the unrolled body and the tail at CP >= 4; the seam does at every CP, with nblk = 4096
    (CP <= 4) down to 321 (CP 64).
  * fold_columns: its unrolled body needs nblk > 768, M >= 196 864: the seam cases of CP <= 16 (nblk 1281 .. 4096).
  * relu_bwd_bias_kernel, maxpool_bwd_kernel: one loop; the seam takes it past one trip of 4096 blocks.
  * the 8-channel forms: TPG = 1, 2, 4, 8, 16, 32, 64 from C = 8, 16, 24 | 32, 40 | 64, 72 | 128, 136 | 256, 264 | 512;
    C = 520 falls back to nine groups of CP 64; test_vec8_apply_kernels_past_their_grid_cap wraps their pixel loops.
  * bn_apply2_f32_kernel / bn_bwd_apply2_f32: C = 2 f32 contiguous, "al" and "pair"; "off1" is bn_apply_kernel<2>.

Views (PAD): "al" keeps every 16-byte predicate true; "off1" breaks the pixel stride and the base; "ptr" (channels
4..4+C of a C+8 buffer) keeps the stride a multiple of 8 elements and only moves a bf16 base 8 bytes off — the one
case that tells the `% 16` pointer test of the 8-channel predicates from the stride test; "pair" is the 2-channel f32
kernels' own 8-byte case.  Outputs are NaN inside their slice and 7.0 outside before every call.

Bounds (from the formats and the kernels' arithmetic, not from what the kernels return):
  * bn_stats, random data: the kernel folds f64 sums and rounds m = S/M, v = SS/M - m*m to f32 once, so
    |mean - ref| <= 2^-24 |ref| + 1e-12 max|x| and |var - ref| <= 2^-24 ref + 1e-12 max x^2 (M <= 1254 f64 roundings of
    at most 2^-53 each are below 1.4e-13 of the largest term); exact-sum data: one f32 ulp of the three-operation value.
  * bn_apply f32: 1e-6 (|xhat gamma| + |beta| + 1) with the kernel's own statistics; sigmoid 1e-6; bf16 adds 2^-8 |ref|.
  * relu / max-pool adjoints: equality with the reference rounded to the output's dtype.
  * bn_backward dx, dgamma, dbeta: scaled_err <= 1e-4; channel sums of dy alone 1e-5; dbias 1e-5 of sum |dx|.
  * relu_backward_bias dbias, random data: 1e-5 of the channel mean of sum |dz| (tests/test_gpu_train.py's bound).
  * softmax: 1e-6 (f32), 2^-8 |ref| + 1e-6 (bf16), also for each row's sum against 1.

Not run, because the API rejects them by contract: dx2 without dx, dx or dbias without x (bn_backward); a dy or dx
of bn_backward / bn_backward_apply that is not f32; relu_backward's dx_lo with a split outside (0, C), so no split at
C = 1."""

import contextlib

import numpy as np
import pytest
import torch

import lane_ref as lr
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

DEV = "cuda"
EPS = 1e-3
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
PAD = {"tight": (0, 0), "al": (8, 8), "off1": (1, 2), "ptr": (4, 4), "pair": (2, 2)}
OPTION_DEFAULT = {"bn_vec_fwd": 0, "bn_vec": 1, "relu_bias_vec": 1}

C_ALL = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 130]
C_VEC = [8, 16, 24, 32, 40, 64, 72, 128, 136, 256, 264, 512, 520]  # TPG 1..64 at both ends; 520: nine groups of CP 64
# (channels, option value): the widths the 8-channel forms take run under both settings, the others as they come
CH = [(c, None) for c in C_ALL if c not in C_VEC] + [(c, v) for c in C_VEC for v in (0, 1)]
CH_IDS = ["c%d" % c if v is None else "c%d-vec%d" % (c, v) for c, v in CH]
SMALL = [(1, 1, 1), (1, 7, 9), (2, 7, 9), (2, 19, 33)]  # M = 1, 63, 126, 1254
SMALL_IDS = ["m1", "m63", "m126", "m1254"]
SEAM_C = {1: 1, 2: 2, 4: 3, 8: 5, 16: 9, 32: 17, 64: 33}  # the smallest width of each packing
SEAM = [(cp, "f32") for cp in SEAM_C] + [(2, "bf16"), (64, "bf16")]
SEAM_IDS = ["cp%d-%s" % s for s in SEAM]
# (CP, relu mask dtype or None) of the BN backward seam cases
SEAM_BWD = [(cp, None) for cp in SEAM_C] + SEAM
SEAM_BWD_IDS = ["cp%d-%s" % (cp, dt or "plain") for cp, dt in SEAM_BWD]


def seam_modes(cp):
    """Seam cases run on misaligned slices; 2 channels also contiguous, which is what the f32 pair kernels take."""
    return ("tight", "off1") if cp == 2 else ("off1",)


def H(t):
    return t.detach().to(torch.float64).cpu().numpy()


def q(a, dt):
    """Host values as the device tensor of dtype ``dt`` holds them (float64)."""
    return lr.to_bf16(a) if dt == "bf16" else lr.to_f32(a)


def chan(a):
    return None if a is None else torch.from_numpy(np.asarray(a, np.float32)).to(DEV)


def scaled_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


class Slot:
    """A tensor argument as channels [lo, lo + c) of a wider buffer that is 7.0 elsewhere: an input holding ``host``, or
    an output pre-filled with NaN."""

    def __init__(self, shape, dt, mode="tight", host=None):
        self.lo, hi = PAD[mode]
        self.c = shape[3]
        self.buf = torch.full(tuple(shape[:3]) + (self.lo + self.c + hi,), 7.0, dtype=TDT[dt], device=DEV)
        self.v = self.buf[..., self.lo:self.lo + self.c]
        if host is None:
            self.v.fill_(float("nan"))
        else:
            self.v.copy_(torch.from_numpy(np.ascontiguousarray(host)).to(DEV))

    def result(self):
        """The slice's values, after checking that all of it was written and nothing beside it."""
        assert bool((self.buf[..., :self.lo] == 7.0).all()) and bool((self.buf[..., self.lo + self.c:] == 7.0).all()), \
            "wrote outside the channel slice"
        got = H(self.v)
        assert not np.isnan(got).any(), "%d elements of the slice not written" % int(np.isnan(got).sum())
        return got


class Inputs:
    """Input slots of one test case, built once per (name, dtype, view)."""

    def __init__(self):
        self.slots = {}

    def __call__(self, name, host, dt, mode):
        key = (name, dt, mode)
        if key not in self.slots:
            self.slots[key] = Slot(host.shape, dt, mode, host)
        return self.slots[key].v

    def untouched(self):
        for s in self.slots.values():
            assert bool((s.buf[..., :s.lo] == 7.0).all()) and bool((s.buf[..., s.lo + s.c:] == 7.0).all())


def positions(names, c):
    """Which arguments are slices: none; each in turn (aligned, misaligned); all of them in every view."""
    pos = [{}]
    for nm in names:
        pos += [{nm: "al"}, {nm: "off1"}]
    for m in ("al", "off1", "ptr") + (("pair",) if c == 2 else ()):
        pos.append({nm: m for nm in names})
    return pos


def plan(names, c, combos, has=lambda combo, name: True):
    """(position, combo) pairs: the full cross where no argument or every argument is a slice (both sides of every
    alignment predicate with every dtype); where a single argument is, two combos in rotation out of those that have
    that argument."""
    out, k = [], 0
    for pos in positions(names, c):
        if len(pos) != 1:
            out += [(pos, cb) for cb in combos]
            continue
        cands = [cb for cb in combos if all(has(cb, nm) for nm in pos)]
        for _ in range(min(2, len(cands))):
            out.append((pos, cands[k % len(cands)]))
            k += 1
    return out


@contextlib.contextmanager
def option(key, value):
    from vmatting import _lib
    try:
        if value is not None:
            _lib.set_option(key, value)
        yield
    finally:
        _lib.set_option(key, OPTION_DEFAULT[key])


def seam_shape(cp):
    """[2, h, w] with odd h, w and 2*h*w just above 5 * 4096 * (256 / cp), not a multiple of 4096 * (256 / cp)."""
    per = 4096 * (256 // cp)
    w = 2 * (int(np.sqrt(5 * per / 2.0)) // 2) + 1
    h = 5 * per // (2 * w) + 1
    h += 1 - h % 2
    m = 2 * h * w
    assert 5 * per < m < 5 * per + per // 8 and m % per and h % 2 and w % 2
    return 2, h, w


def kernel_stats(x_host, dt="f32"):
    """The kernels' own f32 statistics of ``x_host`` (the default forms), as device tensors and float64 host arrays."""
    from vmatting import ops
    mean, var = ops.bn_stats(Slot(x_host.shape, dt, "tight", x_host).v)
    return mean, var, H(mean), H(var)


def stats_bounds(x):
    return 1e-12 * np.abs(x).max(), 1e-12 * (x * x).max()


# ------------------------------------------------------------------------------------------------ bn_stats

def check_stats_random(mean, var, x):
    rm, rv = lr.bn_stats(x)
    am, av = stats_bounds(x)
    assert np.all(np.abs(H(mean) - rm) <= 2.0 ** -24 * np.abs(rm) + am), np.abs(H(mean) - rm).max()
    assert np.all(np.abs(H(var) - rv) <= 2.0 ** -24 * rv + av), np.abs(H(var) - rv).max()


def run_stats(xv):
    from vmatting import ops
    c = xv.shape[-1]
    mean = torch.full((c,), float("nan"), device=DEV)
    var = torch.full((c,), float("nan"), device=DEV)
    ops.bn_stats(xv, mean, var)
    return mean, var


@pytest.mark.parametrize("nhw", SMALL, ids=SMALL_IDS)
@pytest.mark.parametrize("c,vec", CH, ids=CH_IDS)
def test_bn_stats(c, vec, nhw):
    rs = np.random.RandomState(c + nhw[1])
    x = rs.normal(size=nhw + (c,)) * 3 + 1
    inp = Inputs()
    with option("bn_vec_fwd", vec):
        for pos in positions(["x"], c):
            for xdt in ("f32", "bf16"):
                hx = q(x, xdt)
                mean, var = run_stats(inp("x", hx, xdt, pos.get("x", "tight")))
                check_stats_random(mean, var, hx)
    inp.untouched()


@pytest.mark.parametrize("c,vec", [(5, None), (40, 0), (40, 1)], ids=["c5", "c40-vec0", "c40-vec1"])
def test_bn_numerical_edges(c, vec):
    """A channel of mean 100 and deviation 0.1: E[x^2] - m^2 cancels four digits, which f64 sums carry (about 3e-6 of
    the variance at worst) and f32 sums would not (1e-2); a constant channel: variance 0 up to f64 rounding, the apply
    returns beta, and the backward stays finite."""
    from vmatting import ops
    rs = np.random.RandomState(c)
    shape = (2, 19, 33, c)
    x = rs.normal(size=shape) * 3 + 1
    x[..., 1] = 100.0 + 0.1 * rs.normal(size=shape[:3])
    x[..., 2] = np.float32(0.1)
    x = lr.to_f32(x)
    gamma, beta = rs.uniform(0.5, 1.5, c), rs.normal(size=c)
    dy = lr.to_f32(rs.normal(size=shape))
    with option("bn_vec_fwd", vec), option("bn_vec", vec):
        for mode in ("tight", "al", "off1"):
            xv = Slot(shape, "f32", mode, x).v
            mean, var = run_stats(xv)
            check_stats_random(mean, var, x)
            rv = lr.bn_stats(x)[1]
            hv = H(var)
            assert abs(hv[1] - rv[1]) <= 1e-5 * rv[1], (hv[1], rv[1])
            assert 0.0 <= hv[2] <= 1e-12, hv[2]
            out = Slot(shape, "f32", mode)
            ops.bn_apply(xv, mean, var, chan(gamma), chan(beta), EPS, "none", out=out.v)
            assert np.abs(out.result()[..., 2] - np.float32(beta[2])).max() <= 1e-6
            dx = Slot(shape, "f32", mode)
            sums = [torch.full((c,), float("nan"), device=DEV) for _ in range(3)]
            ops.bn_backward(xv, Slot(shape, "f32", mode, dy).v, None, mean, var, chan(gamma), EPS, dx=dx.v,
                            dgamma=sums[0], dbeta=sums[1], dbias=sums[2])
            assert np.isfinite(dx.result()).all() and all(np.isfinite(H(s)).all() for s in sums)


@pytest.mark.parametrize("cp,dt", SEAM, ids=SEAM_IDS)
def test_bn_stats_seam(cp, dt):
    """Exact sums (integers from +-1..4): a lost or repeated pixel moves the mean by at least 1/M, hundreds of ulps."""
    c, shape = SEAM_C[cp], seam_shape(cp) + (SEAM_C[cp],)
    x = lr.exact_ints(np.random.RandomState(cp), shape)
    lr.check_exact_precondition(x)
    m3, v3 = lr.bn_stats_3op(x)
    for mode in seam_modes(cp):
        mean, var = run_stats(Slot(shape, dt, mode, x).v)
        assert np.all(np.abs(H(mean) - lr.to_f32(m3)) <= lr.ulp32(m3)), (H(mean), m3)
        assert np.all(np.abs(H(var) - lr.to_f32(v3)) <= lr.ulp32(v3)), (H(var), v3)


# ------------------------------------------------------------------------------------------------ bn_apply

ACTS = ("none", "relu", "sigmoid")
ABSENT = ((), ("mean", "var", "gamma", "beta"), ("mean",), ("var",), ("gamma",), ("beta",))


def check_apply(got, x, stats, act, ydt):
    """``stats``: float64 mean, var, gamma, beta or None each."""
    ref = lr.bn_apply(x, *stats, EPS, act)
    if act == "sigmoid":
        tol = np.full(ref.shape, 1e-6)
    else:
        pre = lr.bn_preact(x, stats[0], stats[1], stats[2], None, EPS)
        tol = 1e-6 * (np.abs(pre) + (0.0 if stats[3] is None else np.abs(stats[3])) + 1.0)
    if ydt == "bf16":
        tol = tol + 2.0 ** -8 * np.abs(ref)
    bad = np.abs(got - ref) > tol
    assert not bad.any(), (int(bad.sum()), float((np.abs(got - ref) / tol).max()))


@pytest.mark.parametrize("nhw", SMALL, ids=SMALL_IDS)
@pytest.mark.parametrize("c,vec", CH, ids=CH_IDS)
def test_bn_apply(c, vec, nhw):
    from vmatting import ops
    rs = np.random.RandomState(100 + c + nhw[1])
    shape = nhw + (c,)
    x = rs.normal(size=shape) * 3 + 1
    mean, var, hm, hv = kernel_stats(lr.to_f32(x))
    full = {"mean": hm, "var": hv, "gamma": lr.to_f32(rs.uniform(0.5, 1.5, c)), "beta": lr.to_f32(rs.normal(size=c))}
    dev = {"mean": mean, "var": var, "gamma": chan(full["gamma"]), "beta": chan(full["beta"])}
    combos = [(a, b) for a in ("f32", "bf16") for b in ("f32", "bf16")]
    inp = Inputs()
    with option("bn_vec_fwd", vec):
        for i, (pos, (xdt, ydt)) in enumerate(plan(["x", "y"], c, combos)):
            act, absent = ACTS[i % 3], ABSENT[(i // 3) % 6]
            hx = q(x, xdt)
            out = Slot(shape, ydt, pos.get("y", "tight"))
            args = [None if k in absent else dev[k] for k in ("mean", "var", "gamma", "beta")]
            ops.bn_apply(inp("x", hx, xdt, pos.get("x", "tight")), *args, EPS, act, out=out.v)
            stats = [None if k in absent else full[k] for k in ("mean", "var", "gamma", "beta")]
            check_apply(out.result(), hx, stats, act, ydt)
        # in place: out aliases x
        hx = lr.to_f32(x)
        for i, mode in enumerate(("tight", "al", "off1", "ptr") + (("pair",) if c == 2 else ())):
            s = Slot(shape, "f32", mode, hx)
            assert ops.bn_apply(s.v, mean, var, dev["gamma"], dev["beta"], EPS, ACTS[i % 3]) is s.v
            check_apply(s.result(), hx, [full[k] for k in ("mean", "var", "gamma", "beta")], ACTS[i % 3], "f32")
    inp.untouched()


@pytest.mark.parametrize("cp,dt", SEAM, ids=SEAM_IDS)
def test_bn_apply_seam(cp, dt):
    """The four-in-flight body and the tail of bn_apply_kernel<CP> (2 channels: also the pair kernel, contiguous)."""
    from vmatting import ops
    rs = np.random.RandomState(10 + cp)
    c, shape = SEAM_C[cp], seam_shape(cp) + (SEAM_C[cp],)
    x = lr.exact_ints(rs, shape)
    mean, var, hm, hv = kernel_stats(x, dt)
    gamma, beta = lr.to_f32(rs.uniform(0.5, 1.5, c)), lr.to_f32(rs.normal(size=c))
    for mode in seam_modes(cp):
        out = Slot(shape, "f32", mode)
        ops.bn_apply(Slot(shape, dt, mode, x).v, mean, var, chan(gamma), chan(beta), EPS, "relu", out=out.v)
        check_apply(out.result(), x, [hm, hv, gamma, beta], "relu", "f32")
    if cp == 64 and dt == "f32":  # in place
        s = Slot(shape, "f32", "off1", x)
        ops.bn_apply(s.v, mean, var, chan(gamma), chan(beta), EPS, "none")
        check_apply(s.result(), x, [hm, hv, gamma, beta], "none", "f32")


# ------------------------------------------------------------------------------------------------ bn_backward

def check_bn_backward(got, ref, dx2=None):
    dx, dgamma, dbeta, dbias = got
    rdx, rdgamma, rdbeta, _ = ref
    assert scaled_err(dx, rdx) <= 1e-4, scaled_err(dx, rdx)
    assert scaled_err(dgamma, rdgamma) <= 1e-4, scaled_err(dgamma, rdgamma)
    assert scaled_err(dbeta, rdbeta) <= 1e-4, scaled_err(dbeta, rdbeta)
    lim = 1e-5 * np.abs(rdx).sum(axis=lr.AX)
    miss = np.abs(dbias - rdx.sum(axis=lr.AX))
    assert np.all(miss <= lim), (miss / (lim + 1e-300)).max()
    if dx2 is not None:
        assert np.array_equal(dx2, lr.to_bf16(dx))


def run_bn_backward(xv, dyv, yv, mean, var, gamma, shape, dx_mode, dx2_mode):
    from vmatting import ops
    c = shape[3]
    dx = Slot(shape, "f32", dx_mode)
    dx2 = None if dx2_mode is None else Slot(shape, "bf16", dx2_mode)
    sums = [torch.full((c,), float("nan"), device=DEV) for _ in range(3)]
    ops.bn_backward(xv, dyv, yv, mean, var, gamma, EPS, dx=dx.v, dgamma=sums[0], dbeta=sums[1],
                    dx2=None if dx2 is None else dx2.v, dbias=sums[2])
    return (dx.result(), H(sums[0]), H(sums[1]), H(sums[2])), None if dx2 is None else dx2.result()


def bias_sum(dyv):
    from vmatting import ops
    s = torch.full((dyv.shape[-1],), float("nan"), device=DEV)
    ops.bn_backward(None, dyv, None, None, None, None, dbeta=s)
    return H(s)


@pytest.mark.parametrize("nhw", SMALL, ids=SMALL_IDS)
@pytest.mark.parametrize("c,vec", CH, ids=CH_IDS)
def test_bn_backward(c, vec, nhw):
    rs = np.random.RandomState(200 + c + nhw[1])
    shape = nhw + (c,)
    x, dy = lr.to_f32(rs.normal(size=shape) * 3 + 1), lr.to_f32(rs.normal(size=shape))
    y = np.maximum(rs.normal(size=shape), 0)
    gamma = lr.to_f32(rs.uniform(0.5, 1.5, c))
    mean, var, hm, hv = kernel_stats(x)
    combos = [(ydt, with2) for ydt in (None, "f32", "bf16") for with2 in (False, True)]
    has = lambda cb, nm: (nm != "y" or cb[0] is not None) and (nm != "dx2" or cb[1])  # noqa: E731
    refs = {ydt: lr.bn_backward(x, dy, None if ydt is None else q(y, ydt), hm, hv, gamma, EPS)
            for ydt in (None, "f32", "bf16")}
    inp = Inputs()
    with option("bn_vec", vec):
        for pos, (ydt, with2) in plan(["x", "dy", "y", "dx", "dx2"], c, combos, has):
            yv = None if ydt is None else inp("y", q(y, ydt), ydt, pos.get("y", "tight"))
            got, dx2 = run_bn_backward(inp("x", x, "f32", pos.get("x", "tight")),
                                       inp("dy", dy, "f32", pos.get("dy", "tight")), yv, mean, var, chan(gamma), shape,
                                       pos.get("dx", "tight"),
                                       pos.get("dx2", "tight") if with2 else None)
            check_bn_backward(got, refs[ydt], dx2)
        # x = None: the channel sums of dy alone (a bias gradient)
        for mode in ("tight", "al", "off1"):
            assert scaled_err(bias_sum(inp("dy", dy, "f32", mode)), dy.sum(axis=lr.AX)) <= 1e-5
    inp.untouched()


@pytest.mark.parametrize("cp,dt", SEAM_BWD, ids=SEAM_BWD_IDS)
def test_bn_backward_seam(cp, dt):
    """bn_bwd_partial<MASK, CP> and bn_bwd_apply<MASK, CP> (2 channels unmasked and contiguous: bn_bwd_apply2_f32) past
    the grid cap; integer gradients, so dbeta and the bias sum are exact.  ``dt`` is the relu mask's dtype."""
    mask = dt is not None
    rs = np.random.RandomState(20 + cp)
    c, shape = SEAM_C[cp], seam_shape(cp) + (SEAM_C[cp],)
    x = lr.to_f32(rs.normal(size=shape) * 3 + 1)
    dy = lr.exact_ints(rs, shape)
    y = np.maximum(lr.exact_ints(rs, shape), 0) if mask else None
    gamma = lr.to_f32(rs.uniform(0.5, 1.5, c))
    mean, var, hm, hv = kernel_stats(x)
    ref = lr.bn_backward(x, dy, y, hm, hv, gamma, EPS)
    lr.check_exact_precondition(dy)
    lr.check_exact_precondition(dy * (y > 0) if mask else dy)
    for mode in seam_modes(cp):
        yv = Slot(shape, dt, mode, y).v if mask else None
        dyv = Slot(shape, "f32", mode, dy).v
        got, dx2 = run_bn_backward(Slot(shape, "f32", mode, x).v, dyv, yv, mean, var, chan(gamma), shape, mode,
                                   mode if mask else None)
        check_bn_backward(got, ref, dx2)
        assert np.array_equal(got[2], ref[2]), np.abs(got[2] - ref[2]).max()
        assert np.array_equal(bias_sum(dyv), dy.sum(axis=lr.AX))


@pytest.mark.parametrize("mask", [False, True], ids=["plain", "mask"])
@pytest.mark.parametrize("with_dx2", [False, True], ids=["dx", "dx2"])
@pytest.mark.parametrize("c", [2, 20, 64])
def test_bn_backward_apply_syncbn(c, with_dx2, mask):
    """vm_bn_backward_apply_nhwc: a [4,9,11,C] batch as replicas of 1 and 3 samples, their channel sums added on the
    host and applied with count = the whole batch's pixels, against the whole-batch reference."""
    from vmatting import ops
    rs = np.random.RandomState(300 + c)
    shape = (4, 9, 11, c)
    x, dy = lr.to_f32(rs.normal(size=shape) * 3 + 1), lr.to_f32(rs.normal(size=shape))
    y = lr.to_bf16(np.maximum(rs.normal(size=shape), 0)) if mask else None
    gamma = lr.to_f32(rs.uniform(0.5, 1.5, c))
    mean, var, hm, hv = kernel_stats(x)
    ref = lr.bn_backward(x, dy, y, hm, hv, gamma, EPS)
    for mode in ("tight", "al", "off1") + (("pair",) if c == 2 else ()):
        halves, sg, sgx = [], np.zeros(c), np.zeros(c)
        for s in (slice(0, 1), slice(1, 4)):
            sh = x[s].shape
            args = (Slot(sh, "f32", mode, x[s]).v, Slot(sh, "f32", mode, dy[s]).v,
                    Slot(sh, "bf16", mode, y[s]).v if mask else None)
            db, dg = (torch.full((c,), float("nan"), device=DEV) for _ in range(2))
            ops.bn_backward(*args, mean, var, chan(gamma), EPS, dx=None, dgamma=dg, dbeta=db)
            sg, sgx = sg + H(db), sgx + H(dg)
            halves.append((sh, args))
        assert scaled_err(sg, ref[2]) <= 1e-4 and scaled_err(sgx, ref[1]) <= 1e-4
        dxs, dx2s = [], []
        for sh, args in halves:
            dx, dx2 = Slot(sh, "f32", mode), Slot(sh, "bf16", mode) if with_dx2 else None
            ops.bn_backward_apply(*args, mean, var, chan(gamma), chan(sg), chan(sgx), 4 * 9 * 11, dx.v, EPS,
                                  dx2=dx2.v if with_dx2 else None)
            dxs.append(dx.result())
            if with_dx2:
                dx2s.append(dx2.result())
        dx = np.concatenate(dxs, 0)
        assert scaled_err(dx, ref[0]) <= 1e-4, scaled_err(dx, ref[0])
        if with_dx2:
            assert np.array_equal(np.concatenate(dx2s, 0), lr.to_bf16(dx))


def test_vec8_apply_kernels_past_their_grid_cap():
    """bn_apply8 and bn_bwd_apply8 cap their grids at 4096 blocks of 256 / TPG pixels like the per-channel forms; at
    64 channels (TPG 8) 2 * 257 * 257 = 132098 pixels is just past 4096 * 32, so their pixel loops take a second trip
    for the first 1026 pixels only.  Integer data: dbeta is exact."""
    from vmatting import ops
    rs = np.random.RandomState(64)
    c, shape = 64, (2, 257, 257, 64)
    assert 4096 * 32 < 2 * 257 * 257 < 4096 * 33
    x, dy = lr.exact_ints(rs, shape), lr.exact_ints(rs, shape)
    y = np.maximum(lr.exact_ints(rs, shape), 0)
    lr.check_exact_precondition(x)
    lr.check_exact_precondition(dy * (y > 0))
    gamma, beta = lr.to_f32(rs.uniform(0.5, 1.5, c)), lr.to_f32(rs.normal(size=c))
    xv, yv = Slot(shape, "f32", "al", x).v, Slot(shape, "bf16", "al", y).v
    with option("bn_vec_fwd", 1), option("bn_vec", 1):
        mean, var = run_stats(xv)
        hm, hv = H(mean), H(var)
        m3, v3 = lr.bn_stats_3op(x)
        assert np.all(np.abs(hm - lr.to_f32(m3)) <= lr.ulp32(m3)) and np.all(np.abs(hv - lr.to_f32(v3)) <= lr.ulp32(v3))
        out = Slot(shape, "bf16", "al")
        ops.bn_apply(xv, mean, var, chan(gamma), chan(beta), EPS, "relu", out=out.v)
        check_apply(out.result(), x, [hm, hv, gamma, beta], "relu", "bf16")
        got, dx2 = run_bn_backward(xv, Slot(shape, "f32", "al", dy).v, yv, mean, var, chan(gamma), shape, "al", "al")
    ref = lr.bn_backward(x, dy, y, hm, hv, gamma, EPS)
    check_bn_backward(got, ref, dx2)
    assert np.array_equal(got[2], ref[2])


# ------------------------------------------------------------------------------------------------ relu_backward

def run_relu_backward(dyv, yv, shape, split, odt, modes, with2):
    """-> the gradient reassembled over all channels, and its bf16 copy of channels [split, C) or None."""
    from vmatting import ops
    hi_shape, lo_shape = shape[:3] + (shape[3] - split,), shape[:3] + (split,)
    dx = Slot(hi_shape, odt, modes.get("dx", "tight"))
    dx2 = Slot(hi_shape, "bf16", modes.get("dx2", "tight")) if with2 else None
    lo = Slot(lo_shape, odt, modes.get("dx_lo", "tight")) if split else None
    ops.relu_backward(dyv, yv, dx.v, dx2=dx2.v if with2 else None, dx_lo=lo.v if split else None)
    whole = np.concatenate([lo.result(), dx.result()], -1) if split else dx.result()
    return whole, dx2.result() if with2 else None


@pytest.mark.parametrize("nhw", SMALL, ids=SMALL_IDS)
@pytest.mark.parametrize("c", C_ALL + [520])
def test_relu_backward(c, nhw):
    rs = np.random.RandomState(400 + c + nhw[1])
    shape = nhw + (c,)
    dy, y = rs.normal(size=shape), np.maximum(rs.normal(size=shape), 0)
    splits = (0,) if c == 1 else (0, max(1, c // 3))
    # (dy and dx dtype, mask dtype, bf16 copy, split)
    combos = [(gdt, ydt, with2, sp) for gdt in ("f32", "bf16") for ydt in ("f32", "bf16") for with2 in (False, True)
              for sp in splits]
    has = lambda cb, nm: (nm != "dx2" or cb[2]) and (nm != "dx_lo" or cb[3] > 0)  # noqa: E731
    inp = Inputs()
    for pos, (gdt, ydt, with2, sp) in plan(["dy", "y", "dx", "dx2", "dx_lo"], c, combos, has):
        hdy, hy = q(dy, gdt), q(y, ydt)
        got, got2 = run_relu_backward(inp("dy", hdy, gdt, pos.get("dy", "tight")),
                                      inp("y", hy, ydt, pos.get("y", "tight")), shape, sp, gdt, pos, with2)
        ref = lr.relu_backward(hdy, hy)
        assert np.array_equal(got, ref)  # (dy's own dtype: exact)
        if with2:
            assert np.array_equal(got2, lr.to_bf16(ref[..., sp:]))
    inp.untouched()


@pytest.mark.parametrize("cp,dt", SEAM, ids=SEAM_IDS)
def test_relu_backward_seam(cp, dt):
    """relu_bwd_kernel<CP>'s four-in-flight body and tail, with the bf16 copy and (C > 1) the split."""
    rs = np.random.RandomState(30 + cp)
    c, shape = SEAM_C[cp], seam_shape(cp) + (SEAM_C[cp],)
    dy, y = lr.to_f32(rs.normal(size=shape)), q(np.maximum(rs.normal(size=shape), 0), dt)
    ref = lr.relu_backward(dy, y)
    for mode, sp in zip(("off1", "tight"), (c // 2, 0) if cp == 2 else (c // 2,)):
        modes = {k: mode for k in ("dx", "dx2", "dx_lo")}
        got, got2 = run_relu_backward(Slot(shape, "f32", mode, dy).v, Slot(shape, dt, mode, y).v, shape, sp, "f32",
                                      modes, True)
        assert np.array_equal(got, ref)
        assert np.array_equal(got2, lr.to_bf16(ref[..., sp:]))


# ------------------------------------------------------------------------------------------------ relu_backward_bias

def pooled(shape):
    return (shape[0], (shape[1] + 1) // 2, (shape[2] + 1) // 2, shape[3])


def tie_heavy(rs, shape):
    return np.maximum(rs.randint(-2, 4, size=shape), 0) * 0.5  # a few levels and relu zeros: ties in most windows


def run_relu_backward_bias(dyv, yv, addv, shape, zdt, mode):
    from vmatting import ops
    dz = Slot(shape, zdt, mode)
    db = torch.full((shape[3],), float("nan"), device=DEV)
    ops.relu_backward_bias(dyv, yv, dz.v, db, add=addv)
    return dz.result(), H(db)


@pytest.mark.parametrize("nhw", SMALL, ids=SMALL_IDS)
@pytest.mark.parametrize("c,vec", CH, ids=CH_IDS)
def test_relu_backward_bias(c, vec, nhw):
    rs = np.random.RandomState(500 + c + nhw[1])
    shape = nhw + (c,)
    y = tie_heavy(rs, shape)
    dy = {False: rs.normal(size=shape), True: rs.normal(size=pooled(shape))}
    add = rs.normal(size=shape)
    # (dy, y, dz dtypes): the 8-channel form's (bf16 y and dz, either dy) and the per-channel form's others
    trip = [("f32", "bf16", "bf16"), ("bf16", "bf16", "bf16"), ("f32", "f32", "f32"), ("bf16", "f32", "bf16")]
    combos = [(pool, adt) + t for pool in (False, True) for adt in (None, "f32", "bf16") for t in trip]
    has = lambda cb, nm: nm != "add" or cb[1] is not None  # noqa: E731
    inp, refs = Inputs(), {}
    with option("relu_bias_vec", vec):
        for pos, (pool, adt, gdt, ydt, zdt) in plan(["dy", "y", "add", "dz"], c, combos, has):
            hdy, hy, hadd = q(dy[pool], gdt), q(y, ydt), None if adt is None else q(add, adt)
            key = (pool, adt, gdt, ydt)
            if key not in refs:
                refs[key] = lr.relu_backward_bias(hdy, hy, hadd, pool)
            rdz, rdb = refs[key]
            got, db = run_relu_backward_bias(inp("dy%d" % pool, hdy, gdt, pos.get("dy", "tight")),
                                             inp("y", hy, ydt, pos.get("y", "tight")),
                                             None if adt is None else inp("add", hadd, adt, pos.get("add", "tight")),
                                             shape, zdt, pos.get("dz", "tight"))
            assert np.array_equal(got, lr.to_bf16(rdz) if zdt == "bf16" else rdz)
            assert np.abs(db - rdb).max() <= 1e-5 * np.abs(rdz).sum() / c
    inp.untouched()


@pytest.mark.parametrize("pool", [False, True], ids=["plain", "pool"])
@pytest.mark.parametrize("cp,dt", SEAM, ids=SEAM_IDS)
def test_relu_backward_bias_seam(cp, dt, pool):
    """relu_bwd_bias_kernel<POOL, CP> over more pixels than its 4096 blocks hold at once, and fold_sum_kernel's
    unrolled fold; integer dy and add (``dt``), so the bias gradient is the exact integer sum."""
    rs = np.random.RandomState(40 + cp)
    c, shape = SEAM_C[cp], seam_shape(cp) + (SEAM_C[cp],)
    y = tie_heavy(rs, shape)
    dy, add = lr.exact_ints(rs, pooled(shape) if pool else shape), lr.exact_ints(rs, shape)
    rdz, rdb = lr.relu_backward_bias(dy, y, add, pool)
    lr.check_exact_precondition(rdz)
    for mode in seam_modes(cp):
        got, db = run_relu_backward_bias(Slot(dy.shape, dt, mode, dy).v, Slot(shape, "f32", mode, y).v,
                                         Slot(shape, dt, mode, add).v, shape, "f32", mode)
        assert np.array_equal(got, rdz)
        assert np.array_equal(db, rdb), np.abs(db - rdb).max()


# ------------------------------------------------------------------------------------------------ maxpool_backward

@pytest.mark.parametrize("nhw", SMALL, ids=SMALL_IDS)
@pytest.mark.parametrize("c", C_ALL + [520])
def test_maxpool_backward(c, nhw):
    from vmatting import ops
    rs = np.random.RandomState(600 + c + nhw[1])
    shape = nhw + (c,)
    x = tie_heavy(rs, shape)
    dy, add = lr.to_f32(rs.normal(size=pooled(shape))), lr.to_f32(rs.normal(size=shape))
    combos = [(xdt, how) for xdt in ("f32", "bf16") for how in (None, "separate", "inplace")]
    has = lambda cb, nm: nm != "add" or cb[1] == "separate"  # noqa: E731
    refs = {with_add: lr.to_f32(lr.maxpool_backward(x, dy, add if with_add else None)) for with_add in (False, True)}
    inp = Inputs()
    for pos, (xdt, how) in plan(["x", "dy", "add", "dx"], c, combos, has):
        xv, dyv = inp("x", x, xdt, pos.get("x", "tight")), inp("dy", dy, "f32", pos.get("dy", "tight"))
        if how == "inplace":
            dx = Slot(shape, "f32", pos.get("dx", "tight"), add)
            ops.maxpool_backward(xv, dyv, dx.v, add=dx.v)
        else:
            dx = Slot(shape, "f32", pos.get("dx", "tight"))
            ops.maxpool_backward(xv, dyv, dx.v, add=inp("add", add, "f32", pos.get("add", "tight")) if how else None)
        assert np.array_equal(dx.result(), refs[how is not None])
    inp.untouched()


# ------------------------------------------------------------------------------------------------ softmax

@pytest.mark.parametrize("nhw", [(1, 1, 1), (2, 7, 9)], ids=["m1", "m126"])
@pytest.mark.parametrize("c", [1, 2, 3, 4, 64])
def test_softmax_lastdim(c, nhw):
    """Rows of +-1e4 (the maximum must be subtracted), of moderate values, and of equal values (exactly 1/C in f32)."""
    from vmatting import ops
    rs = np.random.RandomState(700 + c + nhw[1])
    shape = nhw + (c,)
    x = rs.uniform(-1e4, 1e4, size=shape)
    if nhw[0] > 1:
        x[0, ::2] = rs.normal(size=x[0, ::2].shape) * 3
        x[1, 1::2] = rs.normal(size=(x[1, 1::2].shape[:2] + (1,))) * 50  # equal within a row
    else:
        x[...] = -37.5
    combos = [(a, b) for a in ("f32", "bf16") for b in ("f32", "bf16")]
    inp = Inputs()
    for pos, (xdt, ydt) in plan(["x", "y"], c, combos):
        hx = q(x, xdt)
        out = Slot(shape, ydt, pos.get("y", "tight"))
        ops.softmax_lastdim(inp("x", hx, xdt, pos.get("x", "tight")), out=out.v)
        got, ref = out.result(), lr.softmax(hx)
        scale = 2.0 ** -8 if ydt == "bf16" else 0.0
        assert np.all(np.abs(got - ref) <= scale * ref + 1e-6), np.abs(got - ref).max()
        assert np.all(np.abs(got.sum(-1) - 1.0) <= scale + 1e-6), np.abs(got.sum(-1) - 1.0).max()
        equal = np.ptp(hx, axis=-1) == 0
        assert equal.any()
        if ydt == "f32":
            assert np.all(got[equal] == np.float64(np.float32(1.0) / np.float32(c)))
    inp.untouched()
