"""numpy restatement of the guided matte upsampling (include/vmatting.h, csrc/guided.hip): the integer reductions, the
f64 coefficients with their two f32 roundings, the apply in f32 operation by operation, plain bilinear upsampling with
the same half-pixel geometry as the thing to beat, and the synthetic edge scene the tests measure on."""

import numpy as np

F = np.float32


def reduced_size(h, w, s):
    return -(-h // s), -(-w // s)


def _blocks(a, s, fill):
    """The s * s members of every block of ``a`` [n,h,w,c] as [n,hm,wm,c] planes, with their validity [hm,wm]."""
    n, h, w, c = a.shape
    hm, wm = reduced_size(h, w, s)
    pad = np.full((n, hm * s, wm * s, c), fill, dtype=np.int64)
    pad[:, :h, :w] = a
    valid = np.zeros((hm * s, wm * s), dtype=bool)
    valid[:h, :w] = True
    for i in range(s):
        for j in range(s):
            yield pad[:, i::s, j::s], valid[i::s, j::s]


def reduce_mean(frames, s):
    """uint8 [n,h,w,3] -> [n,hm,wm,3]: (2 sum + cnt) / (2 cnt) in integers over each block, ragged edge blocks smaller."""
    total, cnt = 0, 0
    for plane, valid in _blocks(frames, s, 0):
        total = total + plane
        cnt = cnt + valid.astype(np.int64)
    cnt = cnt[None, :, :, None]
    return ((2 * total + cnt) // (2 * cnt)).astype(np.uint8)


def reduce_trimap(tri, s):
    """uint8 [n,h,w] -> [n,hm,wm]: the block's byte if all its pixels agree, else 128."""
    lo = hi = None  # pixels past the ragged edge count as 255 for the smallest byte and as 0 for the largest
    for plane, _ in _blocks(tri[..., None], s, 255):
        lo = plane if lo is None else np.minimum(lo, plane)
    for plane, _ in _blocks(tri[..., None], s, 0):
        hi = plane if hi is None else np.maximum(hi, plane)
    return np.where(lo == hi, lo, 128).astype(np.uint8)[..., 0]


def box_sum(a, r):
    """The sum of ``a`` [n,h,w,...] over the (2 r + 1)^2 window of every pixel, clipped to the image, term by term."""
    n, h, w = a.shape[:3]
    pad = np.zeros((n, h + 2 * r, w + 2 * r) + a.shape[3:], dtype=a.dtype)
    pad[:, r:r + h, r:r + w] = a
    out = np.zeros_like(a)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out += pad[:, dy:dy + h, dx:dx + w]
    return out


def box_max(a, r):
    n, h, w = a.shape[:3]
    pad = np.zeros((n, h + 2 * r, w + 2 * r), dtype=a.dtype)
    pad[:, r:r + h, r:r + w] = a
    out = np.zeros_like(a)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out = np.maximum(out, pad[:, dy:dy + h, dx:dx + w])
    return out


def coeffs(g, p, r, eps):
    """g uint8 [n,hm,wm,3], p f32 [n,hm,wm] -> (ab, raw), f32 [n,hm,wm,4] each: raw = (a, b) of every pixel's clipped
    window rounded to f32 once, ab = its mean over the same window, summed in f64 and rounded to f32 once.  The guide's
    moments are exact integers, everything with p and the solve is f64."""
    n, hm, wm, _ = g.shape
    gi = g.astype(np.int64)
    N = box_sum(np.ones((n, hm, wm), dtype=np.int64), r)
    s1 = box_sum(gi, r)
    s2 = box_sum(gi[..., :, None] * gi[..., None, :], r)
    M = N[..., None, None] * s2 - s1[..., :, None] * s1[..., None, :]
    dn = N.astype(np.float64)
    sigma = M.astype(np.float64) / (dn * dn * 65025.0)[..., None, None] + eps * np.eye(3)
    pd = p.astype(np.float64)
    sp = box_sum(pd, r)
    sip = box_sum(gi.astype(np.float64) * pd[..., None], r)
    c = (dn[..., None] * sip - s1.astype(np.float64) * sp[..., None]) / (dn * dn * 255.0)[..., None]
    a = np.linalg.solve(sigma, c[..., None])[..., 0]
    b = sp / dn - (a * (s1.astype(np.float64) / (255.0 * dn)[..., None])).sum(-1)
    raw = np.concatenate([a, b[..., None]], -1).astype(F)
    ab = (box_sum(raw.astype(np.float64), r) / dn[..., None]).astype(F)
    return ab, raw


def texel(size, s, lim):
    """Per full-resolution coordinate 0..size-1: the texel below it, the next one (clamped) and its f32 weight."""
    f = (np.arange(size).astype(F) + F(0.5)) / F(s) - F(0.5)
    f = np.minimum(np.maximum(f, F(0)), F(lim - 1))
    fl = np.floor(f)
    i0 = fl.astype(np.int64)
    t = f - fl
    assert f.dtype == F and t.dtype == F
    return i0, np.minimum(i0 + 1, lim - 1), t


def _lerp(u, v, t):
    return u + t * (v - u)


def bilinear(lo, h, w, s):
    """lo f32 [n,hm,wm,c] -> [n,h,w,c] in f32: horizontally first, then vertically."""
    y0, y1, ty = texel(h, s, lo.shape[1])
    x0, x1, tx = texel(w, s, lo.shape[2])
    tx, ty = tx[None, None, :, None], ty[None, :, None, None]
    top = _lerp(lo[:, y0][:, :, x0], lo[:, y0][:, :, x1], tx)
    bot = _lerp(lo[:, y1][:, :, x0], lo[:, y1][:, :, x1], tx)
    out = _lerp(top, bot, ty)
    assert out.dtype == F
    return out


def apply(ab, cmp, s):
    """ab f32 [n,hm,wm,4], cmp uint8 [n,h,w,3] -> f32 [n,h,w]: q = ((a0 I0 + a1 I1) + a2 I2) + b clamped to [0, 1]."""
    n, h, w, _ = cmp.shape
    m = bilinear(ab, h, w, s)
    i = cmp.astype(F) / F(255.0)
    q = ((m[..., 0] * i[..., 0] + m[..., 1] * i[..., 1]) + m[..., 2] * i[..., 2]) + m[..., 3]
    assert q.dtype == F
    return np.minimum(np.maximum(q, F(0)), F(1))


def upsample(p_lo, cmp, s, r=2, eps=1e-3, guide_lo=None):
    """The three in a row: p_lo f32 [n,hm,wm], cmp uint8 [n,h,w,3] -> f32 [n,h,w]."""
    if guide_lo is None:
        guide_lo = reduce_mean(cmp, s)
    return apply(coeffs(guide_lo, p_lo, r, eps)[0], cmp, s)


def block_mean(a, s):
    """f64 [h,w] -> the mean of every s x s block (ragged edge blocks smaller), f32 [hm,wm]."""
    h, w = a.shape
    hm, wm = reduced_size(h, w, s)
    pad = np.zeros((hm * s, wm * s))
    pad[:h, :w] = a
    cnt = np.zeros((hm * s, wm * s))
    cnt[:h, :w] = 1.0
    fold = lambda v: v.reshape(hm, s, wm, s).sum((1, 3))  # noqa: E731
    return (fold(pad) / fold(cnt)).astype(F)


def edge_scene(h, w):
    """A subject with a 3-pixel soft edge and thin strands over a smooth background -> (alpha f64 [h,w], cmp uint8
    [h,w,3])."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    bg = np.stack([120 + 60 * np.sin(xx / 37 + c) + 30 * np.cos(yy / 23 + 2 * c) for c in range(3)], -1)
    fg = np.array([40.0, 200.0, 90.0]) + (25 * np.sin(xx / 5) * np.cos(yy / 7))[..., None]
    cy, cx = (h - 1) / 2.0, (w - 1) / 2.0
    d, ang = np.hypot(yy - cy, xx - cx), np.arctan2(yy - cy, xx - cx)
    R = 0.3 * min(h, w) * (1 + 0.25 * np.sin(9 * ang) + 0.1 * np.sin(31 * ang))
    alpha = np.clip((R - d) / 3 + 0.5, 0, 1)
    noise = np.random.default_rng(3).normal(0.0, 1.0, (h, w, 3))
    cmp = np.rint(alpha[..., None] * fg + (1 - alpha[..., None]) * bg + noise)
    return alpha, np.clip(cmp, 0, 255).astype(np.uint8)


def edge_band(alpha, s):
    """The pixels within 2 s (in both coordinates) of an unknown pixel of ``alpha`` [h,w]."""
    unknown = ((alpha > 0) & (alpha < 1)).astype(np.int64)[None]
    return box_max(unknown, 2 * s)[0] > 0


def edge_scene_ratio(h, w, s, upsample):
    """SAD of ``upsample(p_lo [1,hm,wm], cmp [1,h,w,3])`` over SAD of bilinear upsampling, near the scene's edge."""
    alpha, cmp = edge_scene(h, w)
    p_lo = block_mean(alpha, s)[None]
    band = edge_band(alpha, s)
    got = upsample(p_lo, cmp[None])[0].astype(np.float64)
    bil = bilinear(p_lo[..., None], h, w, s)[0, ..., 0].astype(np.float64)
    return np.abs(got - alpha)[band].sum() / np.abs(bil - alpha)[band].sum()


def affine_case(h, w, s):
    """Uniform random guide bytes and a matte that is affine in the reduced guide -> (cmp [1,h,w,3], guide_lo, p_lo
    [1,hm,wm], want f64 [h,w])."""
    cmp = np.random.default_rng(5).integers(0, 256, (1, h, w, 3), dtype=np.uint8)
    guide_lo = reduce_mean(cmp, s)
    p_lo = (0.2 + 0.5 * guide_lo[..., 0].astype(np.float64) / 255).astype(F)
    return cmp, guide_lo, p_lo, 0.2 + 0.5 * cmp[0, ..., 0].astype(np.float64) / 255
