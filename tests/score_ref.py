"""numpy restatement of vm_matte_score (include/vmatting.h), the comparison of the kernel tests: every per-pixel term in
f32, operation for operation as the header states it (numpy contracts nothing), and the sums with math.fsum, i.e. exactly
rounded, so that a kernel sum may differ from them only by its own f64 additions.

Conventions: pred / gt [n,h,w] f32 or uint8, trimap uint8 [n,h,w] or None, prev = (prev_pred, prev_gt) [h,w] or None,
backward f32 [n,h,w,2] or None."""

import math

import numpy as np

F = np.float32
SIGMA, RADIUS = 1.4, 4
# G = g / sqrt(sum g^2), D = d / sqrt(sum d^2) of g_i = exp(-i^2 / (2 sigma^2)), d_i = -i g_i, i = -4..4, rounded to f32
G = np.array([0.010715649, 0.0639064, 0.22881863, 0.4918805, 0.63481766, 0.4918805, 0.22881863, 0.0639064, 0.010715649],
             np.float32)
D = np.array([0.04329901, 0.19367121, 0.46229678, 0.49688867, 0.0, -0.49688867, -0.46229678, -0.19367121, -0.04329901],
             np.float32)


def taps64():
    """The taps by their formula, in float64."""
    i = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    g = np.exp(-i * i / (2.0 * SIGMA * SIGMA))
    d = -i * g
    return g / np.sqrt((g * g).sum()), d / np.sqrt((d * d).sum())


def unit(v):
    """The unit value of stored matte values: q / 255 of a uint8, the clamp to [0,1] with NaN -> 0 of an f32."""
    v = np.asarray(v)
    if v.dtype == np.uint8:
        return v.astype(F) / F(255.0)
    assert v.dtype == np.float32, v.dtype
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, np.minimum(v, F(1.0)), F(0.0)).astype(F)


def pass_1d(v, tap, axis):
    """acc = 0; for k = -4..4 ascending: acc = acc + tap[k] * v[clamped index + k], along ``axis`` of an f32 array."""
    n = v.shape[axis]
    pad = [(0, 0)] * v.ndim
    pad[axis] = (RADIUS, RADIUS)
    p = np.pad(v, pad, mode="edge")
    acc = np.zeros(v.shape, F)
    for k in range(2 * RADIUS + 1):
        acc = acc + tap[k] * np.take(p, np.arange(k, k + n), axis=axis)
    return acc


def gradients(x):
    """(gx, gy) of unit planes [..., h, w]: gx = vertical_G(horizontal_D(x)), gy = vertical_D(horizontal_G(x))."""
    return pass_1d(pass_1d(x, D, -1), G, -2), pass_1d(pass_1d(x, G, -1), D, -2)


def magnitude(x):
    gx, gy = gradients(x)
    return np.sqrt(gx * gx + gy * gy)


def region(trimap, shape):
    if trimap is None:
        return np.ones(shape, bool)
    assert trimap.dtype == np.uint8 and trimap.shape == tuple(shape)
    return (trimap != 0) & (trimap != 255)


def warped_error(e_prev, flow):
    """(e^, takes part) of one frame: the previous frame's squared error [h,w] sampled bilinearly at (x, y) + flow."""
    h, w = e_prev.shape
    xs = np.arange(w, dtype=F)[None, :] + flow[..., 0]
    ys = np.arange(h, dtype=F)[:, None] + flow[..., 1]
    with np.errstate(invalid="ignore"):
        inside = (xs >= 0) & (xs <= F(w - 1)) & (ys >= 0) & (ys <= F(h - 1))  # (False for NaN)
    xc, yc = np.where(inside, xs, F(0)), np.where(inside, ys, F(0))
    xf, yf = np.floor(xc), np.floor(yc)
    fx, fy = xc - xf, yc - yf
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    top = e_prev[y0, x0] + fx * (e_prev[y0, x1] - e_prev[y0, x0])
    bot = e_prev[y1, x0] + fx * (e_prev[y1, x1] - e_prev[y1, x0])
    return top + fy * (bot - top), inside


def terms(pred, gt, trimap=None, prev=None, backward=None):
    """Per frame a dict of [h,w] arrays: "region" (bool), f32 "sad", "sse", "grad", and, where the frame has a frame
    before it, "dt" and (with a flow) "me" and "take" (bool: in the region and in frame); else None for those."""
    n, h, w = pred.shape
    a, g = unit(pred), unit(gt)
    assert a.dtype == F and g.dtype == F
    d = a - g
    dm = magnitude(a) - magnitude(g)
    grad = dm * dm
    out = []
    for j in range(n):
        r = region(None if trimap is None else trimap[j], (h, w))
        t = {"region": r, "sad": np.abs(d[j]), "sse": d[j] * d[j], "grad": grad[j], "dt": None, "me": None, "take": None}
        if j or prev is not None:
            a1, g1 = (a[j - 1], g[j - 1]) if j else (unit(prev[0]), unit(prev[1]))
            dd = (a[j] - a1) - (g[j] - g1)
            t["dt"] = dd * dd
            if backward is not None:
                d1 = a1 - g1
                e, inside = warped_error(d1 * d1, backward[j])
                t["me"], t["take"] = np.abs(t["sse"] - e), r & inside
        assert all(v is None or v.dtype in (F, bool) for v in t.values())
        out.append(t)
    return out


def fsum(values):
    return math.fsum(float(v) for v in values)


def stats(pred, gt, trimap=None, prev=None, backward=None, frames=None):
    """The f64 [n,8] table of vm_matte_score with exactly rounded sums (``frames``: the result of terms(), if the
    caller has it already)."""
    frames = terms(pred, gt, trimap, prev, backward) if frames is None else frames
    s = np.zeros((len(frames), 8), np.float64)
    for j, t in enumerate(frames):
        r = t["region"]
        s[j, 0] = r.sum()
        s[j, 1], s[j, 2], s[j, 3] = fsum(t["sad"][r]), fsum(t["sse"][r]), fsum(t["grad"][r])
        if t["dt"] is not None:
            s[j, 4] = fsum(t["dt"][r])
        if t["me"] is not None:
            s[j, 5], s[j, 6] = fsum(t["me"][t["take"]]), t["take"].sum()
    return s


def grad_map(pred, gt):
    dm = magnitude(unit(pred)) - magnitude(unit(gt))
    return dm * dm


# ---------------------------------------------------------------- test material
def mattes(n, h, w, seed, dtype=np.float32, wild=False):
    """Smooth-ish random mattes: blurred noise stretched over [0,1], with flat 0 and 1 areas; ``wild`` (f32 only) adds
    NaN and values below 0 and above 1."""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-0.4, 1.4, (n, h, w))
    x = (x + np.roll(x, 1, 1) + np.roll(x, 1, 2) + np.roll(x, (1, 1), (1, 2))) / 4.0
    x = np.clip((x - 0.5) * 2.0 + 0.5, 0.0, 1.0)
    if dtype == np.uint8:
        return np.rint(x * 255.0).astype(np.uint8)
    x = x.astype(np.float32)
    if wild:
        m = rs.uniform(size=x.shape)
        x[m < 0.03] = np.nan
        x[(m >= 0.03) & (m < 0.06)] = -0.75
        x[(m >= 0.06) & (m < 0.09)] = 1.5
        x[(m >= 0.09) & (m < 0.10)] = -0.0
    return x


def trimaps(n, h, w, seed, kind="random"):
    """"random": 0 / 128 / 255 plus other byte values; "known": only 0 and 255 (an empty region)."""
    rs = np.random.RandomState(seed)
    if kind == "known":
        return rs.choice(np.array([0, 255], np.uint8), size=(n, h, w))
    assert kind == "random"
    return rs.choice(np.array([0, 128, 255, 1, 254, 77], np.uint8), size=(n, h, w), p=[0.3, 0.3, 0.25, 0.05, 0.05, 0.05])


def wild_flow(n, h, w, seed):
    """Flows with NaN, +-inf, out-of-frame and exactly-on-the-border targets among moderate random ones."""
    rs = np.random.RandomState(seed)
    f = rs.uniform(-4.0, 4.0, (n, h, w, 2)).astype(np.float32)
    m = rs.uniform(size=(n, h, w))
    f[m < 0.04] = np.nan
    f[(m >= 0.04) & (m < 0.07), 0] = np.inf
    f[(m >= 0.07) & (m < 0.10), 1] = -np.inf
    f[(m >= 0.10) & (m < 0.14)] = 1e6
    f[(m >= 0.14) & (m < 0.18)] = -3.0e4
    f[(m >= 0.18) & (m < 0.25)] = np.float32(2.0)  # whole-pixel targets: one neighbour, weight 0
    x = np.arange(w, dtype=np.float32)
    f[:, 0, :, 0] = (w - 1) - x  # the first row lands exactly on the last column: x1 is clamped
    f[:, 0, :, 1] = 0.0
    return f
