"""numpy restatement of vm_plate_align_fit / vm_plate_align_apply (include/vmatting.h), and the inputs their tests share.

fit(cmp_pyr, bg_pyr, h, w, ...): one affine map and one photometric gain per frame between the grey pyramids
(flow_est_ref.pyramid) of a frame and of its background plate, coarse to fine, Gauss-Newton over the pixels within
``tol`` grey levels.  Every per-pixel quantity is f32 and parenthesised as the kernels evaluate it; the sums over the
inliers and the 7 x 7 solve are f64 (the sums in numpy's order, the kernels' in theirs: that is all the two differ in).
apply(bg, params): the plate seen through the map, bilinear, rounded once.

The scenes: a textured plate (flow_est_ref.texture, so the moved background comes from real texture and not from a
clamped border), seen through a known affine map, under a gain, behind a textured disc, with sensor noise.
"""

import numpy as np

import flow_est_ref as fe

DEFAULTS = {"iters": 4, "tol": 16.0, "min_share": 4, "reach": 6, "levels": 6}
F = np.float32
NP = 7  # six affine deviations and the gain


def identity():
    return np.array([0, 0, 0, 0, 0, 0, 1, 0], F)


def centred(hk, wk, k, h, w):
    """The level-0 position of every pixel of a level-k grid, and the same relative to the frame's centre."""
    x, y = fe.grid(hk, wk, F)
    s = F(2 ** k)
    X0, Y0 = (x + F(0.5)) * s - F(0.5), (y + F(0.5)) * s - F(0.5)
    return X0, Y0, X0 - F(w - 1) * F(0.5), Y0 - F(h - 1) * F(0.5)


def mapped(p, X0, Y0, xc, yc):
    """Where the frame's pixel sees the plate, in level-0 pixels."""
    return X0 + ((p[0] * xc + p[1] * yc) + p[2]), Y0 + ((p[3] * xc + p[4] * yc) + p[5])


def step_terms(I, P, k, h, w, prm, tol):
    """One Gauss-Newton step's per-pixel terms at level k: (J [7] of f32 arrays, r, the inlier mask)."""
    hk, wk = I.shape
    inv = F(1) / F(2 ** k)
    X0, Y0, xc, yc = centred(hk, wk, k, h, w)
    X, Y = mapped(prm, X0, Y0, xc, yc)
    xl, yl = (X + F(0.5)) * inv - F(0.5), (Y + F(0.5)) * inv - F(0.5)
    inside = (xl >= 0) & (xl <= F(wk - 1)) & (yl >= 0) & (yl <= F(hk - 1))
    pw = fe.bilinear(P, xl, yl)
    gx = ((fe.bilinear(P, xl + F(1), yl) - fe.bilinear(P, xl - F(1), yl)) * F(0.5)) * inv
    gy = ((fe.bilinear(P, xl, yl + F(1)) - fe.bilinear(P, xl, yl - F(1))) * F(0.5)) * inv
    g = prm[6]
    r = I - g * pw
    a, b = g * gx, g * gy
    J = [a * xc, a * yc, a, b * xc, b * yc, b, pw]
    assert all(t.dtype == F for t in J + [r])
    return J, r, inside & (np.abs(r) <= F(tol)), inside & (np.abs(r) <= F(tol) * F(0.25))


def step_sums(I, P, k, h, w, prm, tol):
    """(A f64 [7,7], b f64 [7], count, close) over the inliers; nothing where a parameter is not finite."""
    if not np.isfinite(prm).all():
        return np.zeros((NP, NP)), np.zeros(NP), 0, 0
    J, r, m, close = step_terms(I, P, k, h, w, prm, tol)
    A, b = np.zeros((NP, NP)), np.zeros(NP)
    for i in range(NP):
        for j in range(i, NP):
            A[i, j] = A[j, i] = (J[i] * J[j])[m].astype(np.float64).sum()
        b[i] = (J[i] * r)[m].astype(np.float64).sum()
    return A, b, int(m.sum()), int(close.sum())


def solve(A, b):
    """Gaussian elimination without pivoting in f64, one rounding per operation -> the solution as a list, or None at
    a pivot that is not positive."""
    A, b = [[float(v) for v in row] for row in A], [float(v) for v in b]
    for i in range(NP):
        piv = A[i][i]
        if not piv > 0.0:
            return None
        for j in range(i + 1, NP):
            f = A[j][i] / piv
            for k in range(i, NP):
                A[j][k] = A[j][k] - f * A[i][k]
            b[j] = b[j] - f * b[i]
    x = [0.0] * NP
    for i in range(NP - 1, -1, -1):
        s = b[i]
        for k in range(i + 1, NP):
            s = s - A[i][k] * x[k]
        x[i] = s / A[i][i]
    return x


def corners(h, w):
    cx, cy = F(w - 1) * F(0.5), F(h - 1) * F(0.5)
    return [(-cx, -cy), (cx, -cy), (-cx, cy), (cx, cy)]


def displacement(prm, h, w):
    """The displacement (dx, dy) of the frame's four corners under the map, f32 [4,2]."""
    return np.array([[(prm[0] * x + prm[1] * y) + prm[2], (prm[3] * x + prm[4] * y) + prm[5]] for x, y in corners(h, w)], F)


def fit(cmp_pyr, bg_pyr, h, w, iters=4, tol=16.0, min_share=4, reach=6, trace=None):
    """Two flow_est_ref.pyramid results (f32, finest first) of [h,w] frames -> (params f32 [8], support int).  ``trace``
    (a list) receives every step's (level, residuals, mask)."""
    top = len(cmp_pyr) - 1
    sp = float(bg_pyr[top].astype(np.float64).sum())
    prm = identity()
    if sp > 0.0:
        prm[6] = F(float(cmp_pyr[top].astype(np.float64).sum()) / sp)
    support = 0
    for k in range(top, -1, -1):
        hk, wk = cmp_pyr[k].shape
        for _ in range(iters):
            A, b, count, close = step_sums(cmp_pyr[k], bg_pyr[k], k, h, w, prm[:NP], tol)
            if trace is not None and np.isfinite(prm).all():
                trace.append((k,) + step_terms(cmp_pyr[k], bg_pyr[k], k, h, w, prm[:NP], tol)[1:])
            d = solve(A, b) if count * min_share >= hk * wk else None
            support = close if d is not None or count * min_share < hk * wk else 0
            if d is not None:
                prm[:NP] = [F(float(prm[i]) + d[i]) for i in range(NP)]
    lim = F(min(h, w)) / F(reach)
    far = any(not (dx * dx + dy * dy <= lim * lim) for dx, dy in displacement(prm, h, w))
    if support * min_share < h * w or not np.isfinite(prm).all() or far:
        prm = identity()
    return prm, support


def apply(bg, prm):
    """bg uint8 [h,w,3], params f32 [8] -> uint8 [h,w,3]: the plate at every pixel's mapped position."""
    h, w, _ = bg.shape
    X0, Y0, xc, yc = centred(h, w, 0, h, w)
    X, Y = mapped(np.asarray(prm, F), X0, Y0, xc, yc)
    v = fe.bilinear(bg.astype(F), X, Y)
    assert v.dtype == F
    return np.minimum(np.maximum(np.rint(v), F(0)), F(255)).astype(np.uint8)


def fit_frames(cmp, bg, levels=6, **opts):
    """uint8 frames: cmp [h,w,3], bg [h,w,3] -> (params, support)."""
    h, w, _ = cmp.shape
    return fit(fe.pyramid(cmp, levels), fe.pyramid(bg, levels), h, w, **opts)


def fits(cmp, bg, **opts):
    """A stack: cmp uint8 [n,h,w,3]; bg [n,h,w,3], [1,h,w,3] or one plate [h,w,3] -> (params f32 [n,8], support int64
    [n])."""
    bg = bg[None] if bg.ndim == 3 else bg
    res = [fit_frames(cmp[i], bg[i if len(bg) > 1 else 0], **opts) for i in range(len(cmp))]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res], np.int64)


def applies(bg, params):
    bg = bg[None] if bg.ndim == 3 else bg
    return np.stack([apply(bg[i if len(bg) > 1 else 0], params[i]) for i in range(len(params))])


def corner_error(prm, true, h, w):
    """The largest distance over the four corners between two maps' displacements, in pixels (f64)."""
    d = displacement(prm, h, w).astype(np.float64) - displacement(true, h, w).astype(np.float64)
    return float(np.sqrt((d ** 2).sum(-1)).max())


# ---------------------------------------------------------------- inputs

def _affine(a, b, c, d, tx, ty):
    return np.array([a, b, tx, c, d, ty, 1, 0], F)


MOTIONS = {
    "id": _affine(0, 0, 0, 0, 0, 0),
    "sub": _affine(0, 0, 0, 0, 0.5, 0.5),
    "one": _affine(0, 0, 0, 0, 1, -1),
    "shift": _affine(0, 0, 0, 0, 3.5, -2.25),
    "big": _affine(0, 0, 0, 0, 12.5, -9),
    "rot": _affine(np.cos(0.01) - 1, -np.sin(0.01), np.sin(0.01), np.cos(0.01) - 1, 1.2, -0.8),
    "zoom": _affine(0.02, 0.004, -0.003, 0.02, -1.5, -1),
}
GAINS = (1.0, 0.8, 1.25)
TABLE = ("id", "sub", "one", "shift", "rot", "zoom")  # the motions of the trimap study


def scene(h, w, motion, gain=1.0, seed=0, sigma=2.0):
    """-> (frame u8, plate u8, alpha f64, the true params).  The plate is a texture; the frame's background is that
    texture seen through MOTIONS[motion] (rendered from the texture's margin, not from a clamped border) under ``gain``;
    the subject is a disc of another texture, radius 0.3 min(h, w), soft over 4 pixels; sensor noise on both."""
    true = MOTIONS[motion]
    tex, sub = fe.texture(h, w, seed), fe.texture(h, w, seed + 1000)
    rng = np.random.default_rng(seed)
    X0, Y0, xc, yc = (a.astype(np.float64) for a in centred(h, w, 0, h, w))
    X, Y = mapped(true.astype(np.float64), X0, Y0, xc, yc)
    assert X.min() >= -fe.MARGIN and Y.min() >= -fe.MARGIN and X.max() <= w - 1 + fe.MARGIN and Y.max() <= h - 1 + fe.MARGIN
    back = fe.bilinear(tex, X + fe.MARGIN, Y + fe.MARGIN) * gain
    fg = sub[fe.MARGIN:fe.MARGIN + h, fe.MARGIN:fe.MARGIN + w]
    alpha = np.clip((0.3 * min(h, w) - np.hypot(X0 - (w - 1) / 2, Y0 - (h - 1) / 2)) / 4 + 0.5, 0, 1)
    frame = alpha[..., None] * fg + (1 - alpha[..., None]) * back
    plate = tex[fe.MARGIN:fe.MARGIN + h, fe.MARGIN:fe.MARGIN + w]
    u8 = lambda v: np.clip(np.rint(v + rng.normal(0, sigma, v.shape)), 0, 255).astype(np.uint8)  # noqa: E731
    return u8(frame), u8(plate), alpha, true


def constant_plate(h, w, seed=0):
    """A textured frame against a plate of one colour: nothing to fit."""
    frame = scene(h, w, "id", seed=seed)[0]
    return frame, np.full((h, w, 3), 128, np.uint8)


def noise_pair(h, w, seed=0):
    """Independent uniform noise in frame and plate."""
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (h, w, 3)).astype(np.uint8), rs.randint(0, 256, (h, w, 3)).astype(np.uint8)


def covered(h, w, seed=0):
    """A subject that covers the whole frame: two unrelated textures."""
    m = fe.MARGIN
    u8 = lambda v: np.rint(v[m:m + h, m:m + w]).astype(np.uint8)  # noqa: E731
    return u8(fe.texture(h, w, seed + 1000)), u8(fe.texture(h, w, seed))


DEGENERATE = {"constant": constant_plate, "noise": noise_pair, "covered": covered}


# ---------------------------------------------------------------- arguments the C calls refuse (never dereferenced)

def _vary(ok, cases):
    return [ok[:i] + (v,) + ok[i + 1:] for i, v in cases]


def bad_fit_arguments():
    """vm_plate_align_fit(cmp_pyr, cmp_stride, bg_pyr, bg_stride, nb, n, h, w, levels, iters, tol, min_share, reach,
    params, support, work) without the stream: each differs in one place from a valid call on two 16 x 16 frames."""
    P, Q, G, S, W = 4096, 1 << 20, 1 << 21, (1 << 21) + 4096, 1 << 22  # non-null, aligned, far apart
    ok = (P, 4096, Q, 4096, 1, 2, 16, 16, 6, 4, 16.0, 4, 6, G, S, W)
    bad = _vary(ok, [(0, None), (2, None), (13, None), (14, None), (15, None), (5, 0), (5, -1), (6, 15), (7, 15), (6, 40000),
                     (8, 0), (4, 0), (4, 3), (9, 0), (9, 65), (10, 0.0), (10, -1.0), (10, float("nan")),
                     (10, float("inf")), (11, 0), (11, 4097), (12, 0), (12, 1025), (1, 255), (0, P + 2), (2, Q + 1),
                     (13, G + 2), (14, S + 1), (15, W + 8)])
    return bad + [(P, 4096, Q, 255, 2, 2, 16, 16, 6, 4, 16.0, 4, 6, G, S, W),  # nb == n: bg_stride is read
                  (P, 4096, Q, 4096, 1, 1 << 20, 1024, 1024, 6, 4, 16.0, 4, 6, G, S, W)]  # n h w 3 beyond 2^31 - 1


def bad_apply_arguments():
    """vm_plate_align_apply(bg, nb, params, n, h, w, out) without the stream, likewise."""
    P, Q, G = 4096, 1 << 20, 1 << 21
    ok = (P, 1, G, 2, 16, 16, Q)
    return _vary(ok, [(0, None), (2, None), (6, None), (3, 0), (4, 0), (5, 0), (1, 0), (1, 3), (2, G + 2), (6, P + 100),
                      (6, P), (6, P - 1000), (6, G + 16), (6, G - 95), (4, 1 << 30), (4, 40000)])
