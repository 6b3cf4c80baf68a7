"""numpy restatement of vm_matte_smooth (include/vmatting.h), and the inputs its tests share: every step in f32,
operation for operation as the header states it (numpy contracts nothing).

Conventions: alpha f32 [n,h,w], cmp uint8 [n,h,w,3], backward f32 [n,h,w,2], prev = (prev_alpha f32 [h,w], prev_cmp uint8
[h,w,3]) or None."""

import numpy as np

from score_ref import unit

F = np.float32
DEFAULTS = {"strength": 0.5, "tol": 24.0, "jump": 0.3}


def targets(flow):
    """The bilinear taps of one frame's flow [h,w,2], tests/score_ref.py:warped_error's convention -> (inside, y0, x0,
    y1, x1, fx, fy); outside, the target is (0, 0)."""
    h, w = flow.shape[:2]
    xs = np.arange(w, dtype=F)[None, :] + flow[..., 0]
    ys = np.arange(h, dtype=F)[:, None] + flow[..., 1]
    with np.errstate(invalid="ignore"):
        inside = (xs >= 0) & (xs <= F(w - 1)) & (ys >= 0) & (ys <= F(h - 1))  # (False for NaN)
    xc, yc = np.where(inside, xs, F(0)), np.where(inside, ys, F(0))
    xf, yf = np.floor(xc), np.floor(yc)
    fx, fy = xc - xf, yc - yf
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    assert fx.dtype == F and fy.dtype == F
    return inside, y0, x0, y1, x1, fx, fy


def sample(v, taps):
    """top + fy (bot - top) of an f32 plane [h,w] or [h,w,c] at the taps."""
    _, y0, x0, y1, x1, fx, fy = taps
    if v.ndim == 3:
        fx, fy = fx[..., None], fy[..., None]
    top = v[y0, x0] + fx * (v[y0, x1] - v[y0, x0])
    bot = v[y1, x0] + fx * (v[y1, x1] - v[y1, x0])
    out = top + fy * (bot - top)
    assert out.dtype == F
    return out


def smooth_frame(alpha, cmp, flow, prev_s, prev_cmp, strength, tol, jump):
    """One frame with a predecessor -> (s, weight), both f32 [h,w]."""
    inv_tol, inv_jump = F(1.0) / F(tol), F(1.0) / F(jump)
    a = unit(alpha)
    taps = targets(flow)
    with np.errstate(invalid="ignore", over="ignore"):
        p = sample(unit(prev_s), taps)
        c = sample(prev_cmp.astype(F), taps)
        d = np.abs(cmp.astype(F) - c).max(-1)
        k = unit(F(1.0) - d * inv_tol) * unit(F(1.0) - np.abs(a - p) * inv_jump)
        k = np.where(taps[0], k, F(0.0))
        s = unit(a + (F(strength) * k) * (p - a))
    assert s.dtype == F and k.dtype == F
    return s, k


def smooth(alpha, cmp, backward, prev=None, strength=DEFAULTS["strength"], tol=DEFAULTS["tol"], jump=DEFAULTS["jump"]):
    """The clip in order -> (out, weight), f32 [n,h,w]: a frame with nothing before it keeps its clamped matte at weight
    0; frame j >= 1 follows (out[j - 1], cmp[j - 1])."""
    assert alpha.dtype == F and cmp.dtype == np.uint8 and backward.dtype == F
    out, weight = np.zeros(alpha.shape, F), np.zeros(alpha.shape, F)
    for j in range(alpha.shape[0]):
        before = (out[j - 1], cmp[j - 1]) if j else prev
        if before is None:
            out[j] = unit(alpha[j])
        else:
            out[j], weight[j] = smooth_frame(alpha[j], cmp[j], backward[j], before[0], before[1], strength, tol, jump)
    return out, weight


# ---------------------------------------------------------------- test material
def frames(n, h, w, seed):
    """uint8 frames that share their content, so that the photometric gate is open, half open and shut in places: smooth
    waves (a few levels per pixel) that drift from frame to frame, a little noise, and a sprinkle of changed pixels."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((n, h, w, 3), np.uint8)
    for j in range(n):
        f = np.stack([128 + 60 * np.sin((xx + 0.6 * j) / 13.0 + c) + 50 * np.cos((yy - 0.4 * j) / 11.0 + 2 * c)
                      for c in range(3)], -1) + rs.uniform(-2.0, 2.0, (h, w, 3))
        f = np.clip(np.rint(f), 0, 255).astype(np.uint8)
        m = rs.uniform(size=(h, w)) < 0.1
        f[m] = rs.randint(0, 256, (int(m.sum()), 3))
        out[j] = f
    return out


def moderate_flow(n, h, w, seed):
    return np.random.RandomState(seed).uniform(-2.5, 2.5, (n, h, w, 2)).astype(F)


def _texture(h, w, rs, lo, hi):
    """A smooth texture within lo..hi (float64 [h,w,3]), defined on a canvas larger than the frame so that it can move."""
    t = rs.uniform(lo, hi, (h, w, 3))
    for _ in range(6):
        t = (t + np.roll(t, 1, 0) + np.roll(t, 1, 1) + np.roll(t, (1, 1), (0, 1))) / 4.0
    return (t - t.min()) / (t.max() - t.min()) * (hi - lo) + lo


def noisy_clip(n=8, h=48, w=64, seed=0, speed=(1.5, 0.7), sigma=0.08, band=8.0):
    """The issue's synthetic clip: a soft-edged textured disc moving ``speed`` px/frame over a textured plate, and a
    "model" matte equal to the truth plus blurred noise of ``sigma`` within ``band`` px of the disc's edge -> a dict:
    "cmp" uint8 [n,h,w,3], "gt" and "alpha" f32 [n,h,w], "backward" f32 [n,h,w,2] (the exact flow: the disc's motion
    on the disc and its rim, zero on the plate: frame j at (x, y) ~ frame j - 1 at (x - vx, y - vy))."""
    rs = np.random.RandomState(seed)
    plate = _texture(h, w, rs, 30.0, 140.0)
    pad = int(np.ceil(n * max(abs(speed[0]), abs(speed[1])))) + 2
    skin = _texture(h + 2 * pad, w + 2 * pad, rs, 120.0, 240.0)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    radius, soft = 0.28 * min(h, w), 4.0
    cx0, cy0 = 0.35 * w, 0.4 * h
    cmp, gt, alpha = np.empty((n, h, w, 3), np.uint8), np.empty((n, h, w), F), np.empty((n, h, w), F)
    backward = np.zeros((n, h, w, 2), F)
    for j in range(n):
        dx, dy = speed[0] * j, speed[1] * j
        r = np.hypot(xx - (cx0 + dx), yy - (cy0 + dy))
        a = np.clip((radius - r) / soft + 0.5, 0.0, 1.0)
        a = a * a * (3.0 - 2.0 * a)  # a smooth profile: a bilinear sample of the previous matte follows it closely
        # the disc's texture moves with it: bilinear sample of the canvas at (x - dx, y - dy)
        sx, sy = xx - dx + pad, yy - dy + pad
        x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
        fx, fy = (sx - x0)[..., None], (sy - y0)[..., None]
        fg = ((1 - fy) * ((1 - fx) * skin[y0, x0] + fx * skin[y0, x0 + 1]) +
              fy * ((1 - fx) * skin[y0 + 1, x0] + fx * skin[y0 + 1, x0 + 1]))
        cmp[j] = np.clip(np.rint(a[..., None] * fg + (1 - a[..., None]) * plate), 0, 255).astype(np.uint8)
        gt[j] = a.astype(F)
        noise = rs.normal(0.0, 1.0, (h, w))
        for _ in range(2):
            noise = (noise + np.roll(noise, 1, 0) + np.roll(noise, 1, 1) + np.roll(noise, (1, 1), (0, 1))) / 4.0
        noise *= sigma / noise.std()
        near = np.abs(r - radius) <= band
        alpha[j] = np.clip(a + np.where(near, noise, 0.0), 0.0, 1.0).astype(F)
        moving = r <= radius + soft / 2 + 1.0  # the disc and its soft rim move; the plate around them stands still
        backward[j, ..., 0] = np.where(moving, -speed[0], 0.0)
        backward[j, ..., 1] = np.where(moving, -speed[1], 0.0)
    return {"cmp": cmp, "gt": gt, "alpha": alpha, "backward": backward}


def dtssd(pred, gt):
    """The clip's mean dtSSD over all pixels (score_summary's figure without a trimap), in float64."""
    p, g = pred.astype(np.float64), gt.astype(np.float64)
    d = (p[1:] - p[:-1]) - (g[1:] - g[:-1])
    return float(np.sqrt((d * d).mean((1, 2))).mean())


def sad(pred, gt):
    return float(np.abs(pred.astype(np.float64) - gt.astype(np.float64)).sum())
