"""The arithmetic of vm_flow_estimate (csrc/flow_est.hip) restated in numpy, shared by
tests/test_flow_est_host.py and tests/test_gpu_flow_est.py: coarse-to-fine Horn-Schunck with warping and Jacobi
sweeps.  Every intermediate has the dtype ``dt`` (np.float32: the kernels' arithmetic, operation for operation;
np.float64: the same formulas at higher precision), and every expression is parenthesised as the kernels evaluate it.

    estimate(cur, prev) -> f [h,w,2] with cur(x, y) ~ prev(x + f[...,0], y + f[...,1])

Also the test inputs: a seeded smooth texture with a margin, and a sampler that renders the current frame from it under
a known flow, so the flow the estimator should find is known exactly.
"""

import numpy as np

MARGIN = 20


def grey(bgr, dt=np.float32):
    b = bgr.astype(np.int32)
    return (29 * b[..., 0] + 150 * b[..., 1] + 77 * b[..., 2]).astype(dt) / dt(256)


def down(a):
    """2x2 box mean, ceil sizes, the last row / column replicated."""
    dt = a.dtype.type
    h, w = a.shape
    y0, x0 = np.arange((h + 1) // 2) * 2, np.arange((w + 1) // 2) * 2
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    g = lambda ys, xs: a[ys][:, xs]  # noqa: E731
    return ((g(y0, x0) + g(y0, x1)) + (g(y1, x0) + g(y1, x1))) * dt(0.25)


def smooth(a):
    """Separable [1/4, 1/2, 1/4], horizontal then vertical, replicate borders."""
    dt = a.dtype.type
    h, w = a.shape
    xs, ys = np.arange(w), np.arange(h)
    hz = (a[:, np.maximum(xs - 1, 0)] + a[:, np.minimum(xs + 1, w - 1)]) * dt(0.25) + a * dt(0.5)
    return (hz[np.maximum(ys - 1, 0)] + hz[np.minimum(ys + 1, h - 1)]) * dt(0.25) + hz * dt(0.5)


def level_shapes(h, w, levels):
    shapes = [(h, w)]
    while len(shapes) < levels and min(shapes[-1]) // 2 >= 8:
        hk, wk = shapes[-1]
        shapes.append(((hk + 1) // 2, (wk + 1) // 2))
    return shapes


def pyramid(bgr, levels, dt=np.float32):
    """The smoothed levels, finest first.  Levels are built from the unsmoothed level below and smoothed afterwards."""
    raw = [grey(bgr, dt)]
    for _ in level_shapes(bgr.shape[0], bgr.shape[1], levels)[1:]:
        raw.append(down(raw[-1]))
    return [smooth(a) for a in raw]


def bilinear(p, x, y):
    """p [h,w] or [h,w,c] sampled at (x, y), coordinates clamped to the image."""
    dt = x.dtype.type
    h, w = p.shape[:2]
    x = np.minimum(np.maximum(x, dt(0)), dt(w - 1))
    y = np.minimum(np.maximum(y, dt(0)), dt(h - 1))
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = x - xf, y - yf
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    if p.ndim == 3:
        fx, fy = fx[..., None], fy[..., None]
    top = p[y0, x0] + fx * (p[y0, x1] - p[y0, x0])
    bot = p[y1, x0] + fx * (p[y1, x1] - p[y1, x0])
    return top + fy * (bot - top)


def grid(h, w, dt):
    return np.arange(w, dtype=dt)[None, :].repeat(h, 0), np.arange(h, dtype=dt)[:, None].repeat(w, 1)


def upsample(flow, h, w):
    dt = flow.dtype.type
    x, y = grid(h, w, dt)
    return dt(2) * bilinear(flow, (x - dt(0.5)) * dt(0.5), (y - dt(0.5)) * dt(0.5))


def coefficients(cur, prev, flow, alpha):
    """(Ix, Iy, It, den) of one warp at flow = (u0, v0)."""
    dt = cur.dtype.type
    h, w = cur.shape
    x, y = grid(h, w, dt)
    iw = bilinear(prev, x + flow[..., 0], y + flow[..., 1])
    xs, ys = np.arange(w), np.arange(h)
    ix = (iw[:, np.minimum(xs + 1, w - 1)] - iw[:, np.maximum(xs - 1, 0)]) * dt(0.5)
    iy = (iw[np.minimum(ys + 1, h - 1)] - iw[np.maximum(ys - 1, 0)]) * dt(0.5)
    it = iw - cur
    a2 = dt(alpha) * dt(alpha)
    return ix, iy, it, (a2 + ix * ix) + iy * iy


def neighbour_mean(u):
    dt = u.dtype.type
    p = np.pad(u, 1, mode="edge")
    e = (p[:-2, 1:-1] + p[2:, 1:-1]) + (p[1:-1, :-2] + p[1:-1, 2:])
    d = (p[:-2, :-2] + p[:-2, 2:]) + (p[2:, :-2] + p[2:, 2:])
    return e * (dt(1) / dt(6)) + d * (dt(1) / dt(12))


def sweep(flow, flow0, coef):
    """One Jacobi sweep: both components from the previous iterate."""
    ix, iy, it, den = coef
    ub, vb = neighbour_mean(flow[..., 0]), neighbour_mean(flow[..., 1])
    r = (ix * (ub - flow0[..., 0]) + iy * (vb - flow0[..., 1])) + it
    q = r / den
    return np.stack([ub - ix * q, vb - iy * q], -1)


def estimate_from_pyramids(cur, prev, warps=3, iters=20, alpha=15.0, debug=None):
    dt = cur[0].dtype.type
    flow = None
    for k in range(len(cur) - 1, -1, -1):
        h, w = cur[k].shape
        flow = np.zeros((h, w, 2), dt) if flow is None else upsample(flow, h, w)
        for _ in range(warps):
            flow0 = flow
            coef = coefficients(cur[k], prev[k], flow0, alpha)
            for _ in range(iters):
                flow = sweep(flow, flow0, coef)
            assert flow.dtype == dt
        if debug is not None:
            debug.append(coef)
    return flow


def estimate(cur, prev, levels=6, warps=3, iters=20, alpha=15.0, dt=np.float32):
    """cur, prev: uint8 [h,w,3] BGR -> the backward flow [h,w,2] in ``dt``."""
    return estimate_from_pyramids(pyramid(cur, levels, dt), pyramid(prev, levels, dt), warps, iters, alpha)


# ---------------------------------------------------------------- inputs with a known flow

def _box(a, times):
    for _ in range(times):
        p = np.pad(a, 1, mode="edge")
        a = sum(p[i:i + a.shape[0], j:j + a.shape[1]] for i in range(3) for j in range(3)) / 9.0
    return a


def texture(h, w, seed, channels=3):
    """float64 [h + 2 MARGIN, w + 2 MARGIN, channels] in 0..255: uniform noise box-blurred a few times plus a blurred
    8x-upsampled low-frequency term, stretched to the full range."""
    rs = np.random.RandomState(seed)
    H, W = h + 2 * MARGIN, w + 2 * MARGIN
    out = []
    for _ in range(channels):
        fine = _box(rs.uniform(0.0, 1.0, (H, W)), 3)
        low = rs.uniform(0.0, 1.0, ((H + 7) // 8, (W + 7) // 8))
        low = _box(np.kron(low, np.ones((8, 8)))[:H, :W], 4)
        t = (fine - fine.mean()) / fine.std() + 1.5 * (low - low.mean()) / low.std()
        out.append(255.0 * (t - t.min()) / (t.max() - t.min()))
    return np.stack(out, -1)


def render(tex, h, w, flow=None):
    """The uint8 [h,w,3] frame seen through ``flow`` (None: the texture itself, the previous frame):
    frame(x, y) = tex(x + flow_x + MARGIN, y + flow_y + MARGIN), bilinear in float64, rounded once."""
    x, y = grid(h, w, np.float64)
    if flow is not None:
        x, y = x + flow[..., 0], y + flow[..., 1]
    assert x.min() >= -MARGIN and y.min() >= -MARGIN and x.max() <= w - 1 + MARGIN and y.max() <= h - 1 + MARGIN
    return np.rint(bilinear(tex, x + MARGIN, y + MARGIN)).astype(np.uint8)


def shift_flow(h, w, dx, dy):
    return np.broadcast_to(np.array([dx, dy], np.float64), (h, w, 2)).copy()


def zoom_flow(h, w):
    """4 % zoom + rotation: u = 0.04 (x - w/2) - 0.03 (y - h/2) + 1, v = 0.03 (x - w/2) + 0.04 (y - h/2) - 0.5."""
    x, y = grid(h, w, np.float64)
    x, y = x - w / 2, y - h / 2
    return np.stack([0.04 * x - 0.03 * y + 1.0, 0.03 * x + 0.04 * y - 0.5], -1)


FLOWS = {"small": lambda h, w: shift_flow(h, w, 3.5, -2.25), "large": lambda h, w: shift_flow(h, w, 12.5, -9.0),
         "zoom": zoom_flow}


def pair(h, w, name, seed=7):
    """(cur, prev, flow): two uint8 frames and the exact backward flow between them."""
    tex = texture(h, w, seed)
    flow = FLOWS[name](h, w)
    return render(tex, h, w, flow), render(tex, h, w), flow


def endpoint_error(got, want, border=MARGIN):
    d = got.astype(np.float64) - want
    e = np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)
    return float(e[border:-border, border:-border].mean())
