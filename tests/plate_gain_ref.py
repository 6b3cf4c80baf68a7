"""numpy restatement of vm_plate_gain_fit / vm_plate_gain_apply (include/vmatting.h), and the inputs their tests share.

fit(cmp, bg, band, min_share): per channel the histogram of the ratio's bins over the valid pixels, its 3-bin mode, and
the least-squares ratio over the inliers as a Q12 integer; int64 throughout.  apply(bg, G): the plate under the gains."""

import numpy as np

DEFAULTS = {"band": 8, "min_share": 16}
ONE = 4096


def fit(cmp, bg, band=8, min_share=16):
    """One frame: cmp, bg uint8 [h,w,3] -> (G int[3], support int[3])."""
    assert 1 <= band <= 16 and 1 <= min_share <= 4096
    h, w, _ = cmp.shape
    G, sup = [], []
    for c in range(3):
        a = cmp[..., c].astype(np.int64).ravel()
        b = bg[..., c].astype(np.int64).ravel()
        v = (b >= 16) & (b <= 250) & (a <= 250) & (64 * a + b // 2 < 255 * b)
        a, b = a[v], b[v]
        H = np.bincount((64 * a + b // 2) // np.maximum(b, 1), minlength=256)[:256]
        S = H.copy()
        S[1:] += H[:-1]
        S[:-1] += H[1:]
        q0 = 16 + int(np.argmax(S[16:255]))
        inl = np.abs(64 * a - q0 * b) <= band * b
        n, N, D = int(inl.sum()), int((a[inl] * b[inl]).sum()), int((b[inl] ** 2).sum())
        G.append((4096 * N + D // 2) // D if n * min_share >= h * w else 4096)
        sup.append(n)
    return G, sup


def apply(bg, G):
    """bg uint8 [h,w,3], G int[3] -> uint8 [h,w,3]."""
    return np.minimum(255, (bg.astype(np.int64) * np.array(G) + 2048) >> 12).astype(np.uint8)


def fits(cmp, bg, **opts):
    """A stack: cmp uint8 [n,h,w,3]; bg [n,h,w,3], [1,h,w,3] or one plate [h,w,3] -> (G int64 [n,3], support int64
    [n,3])."""
    bg = bg[None] if bg.ndim == 3 else bg
    res = [fit(cmp[i], bg[i if len(bg) > 1 else 0], **opts) for i in range(len(cmp))]
    return np.array([r[0] for r in res], np.int64), np.array([r[1] for r in res], np.int64)


def applies(bg, G):
    """bg [n,h,w,3], [1,h,w,3] or one plate [h,w,3], G int [n,3] -> uint8 [n,h,w,3]."""
    bg = bg[None] if bg.ndim == 3 else bg
    return np.stack([apply(bg[i if len(bg) > 1 else 0], G[i]) for i in range(len(G))])


def fit_loops(cmp, bg, band=8, min_share=16):
    """fit, pixel by pixel over Python ints: the definition read off the header line by line."""
    h, w, _ = cmp.shape
    G, sup = [], []
    for c in range(3):
        pairs = []
        H = [0] * 256
        for y in range(h):
            for x in range(w):
                a, b = int(cmp[y, x, c]), int(bg[y, x, c])
                if not (16 <= b <= 250 and a <= 250):
                    continue
                t = 64 * a + (b >> 1)
                if not t < 255 * b:
                    continue
                H[t // b] += 1
                pairs.append((a, b))
        q0, best = 16, -1
        for q in range(16, 255):
            s = H[q - 1] + H[q] + (H[q + 1] if q + 1 <= 254 else 0)
            if s > best:
                q0, best = q, s
        cnt = N = D = 0
        for a, b in pairs:
            if abs(64 * a - q0 * b) <= band * b:
                cnt, N, D = cnt + 1, N + a * b, D + b * b
        G.append((4096 * N + (D >> 1)) // D if cnt * min_share >= h * w else 4096)
        sup.append(cnt)
    return G, sup


# ---------------------------------------------------------------- inputs

GAINS = ((1, 1, 1), (.8, .8, .8), (1.25, 1.25, 1.25), (.7, .85, 1.1), (1.5, 1.3, .6), (.5, .5, .5))


def scene(seed, gain=(1, 1, 1), radius=30, h=96, w=160, sigma=4.0):
    """trimap_plate_ref.scene with the frame's light scaled per channel by ``gain`` before the noise and the rounding,
    and the disc's radius free -> (frame u8, plate u8, alpha f64).  gain (1, 1, 1) and radius 30 give that scene."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:h, :w].astype(np.float64)
    plate = np.stack([60 + 40 * np.sin(x / 9), 90 + 30 * np.cos(y / 7), 120 + 0 * x], -1)
    fg = np.stack([200 + 20 * np.sin(y / 5), 40 + 20 * np.cos(x / 6), 30 + 0 * x], -1)
    alpha = np.clip((radius - np.hypot(x - 80, y - 48)) / 4 + 0.5, 0, 1)
    frame = (alpha[..., None] * fg + (1 - alpha[..., None]) * plate) * np.asarray(gain, np.float64)
    u8 = lambda v: np.clip(np.rint(v + rng.normal(0, sigma, v.shape)), 0, 255).astype(np.uint8)  # noqa: E731
    return u8(frame), u8(plate), alpha


def noise_pair(h, w, seed=0):
    """Independent uniform noise: the bins spread over the whole histogram."""
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (h, w, 3)).astype(np.uint8), rs.randint(0, 256, (h, w, 3)).astype(np.uint8)


def all_pairs():
    """256 x 256: cmp is the row index and bg the column index, rolled by 0, 85 and 170 per channel: every (a, b) pair
    of the division, at a different place in every channel."""
    a, b = np.mgrid[:256, :256]
    cmp = np.stack([np.roll(a, s, 0) for s in (0, 85, 170)], -1).astype(np.uint8)
    bg = np.stack([np.roll(b, s, 1) for s in (0, 85, 170)], -1).astype(np.uint8)
    return cmp, bg


def constant_pair(h, w, a=250, b=250):
    """Every pixel in one bin, and the largest sums there are."""
    return np.full((h, w, 3), a, np.uint8), np.full((h, w, 3), b, np.uint8)
