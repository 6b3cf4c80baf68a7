"""numpy restatement of vm_trimap_from_plate (include/vmatting.h), and the inputs its tests share.

trimap(cmp, bg, lo, hi, r_bg, r_fg): int64 throughout; the 3 x 3 box sum over an edge-padded array (the replicated
border), the erosions over windows clipped to the image."""

import numpy as np

DEFAULTS = {"lo": 16, "hi": 48, "r_bg": 4, "r_fg": 8}


def distance(cmp, bg):
    """d = sum over channels of (cmp - bg)^2: uint8 [h,w,3] twice -> int64 [h,w]."""
    q = cmp.astype(np.int64) - bg.astype(np.int64)
    return (q * q).sum(-1)


def box3(d):
    """The 3 x 3 sum with coordinates clamped to the image: always 9 terms."""
    h, w = d.shape
    p = np.pad(d, 1, mode="edge")
    return sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))


def erode(mask, r):
    """mask[y, x] and every pixel of its (2 r + 1)^2 window that lies in the image."""
    h, w = mask.shape
    rows = np.empty_like(mask)
    for x in range(w):
        rows[:, x] = mask[:, max(x - r, 0):x + r + 1].all(1)
    out = np.empty_like(mask)
    for y in range(h):
        out[y] = rows[max(y - r, 0):y + r + 1].all(0)
    return out


def box_sum(cmp, bg):
    return box3(distance(cmp, bg))


def trimap(cmp, bg, lo=16, hi=48, r_bg=4, r_fg=8):
    """One frame: cmp, bg uint8 [h,w,3] -> uint8 [h,w] of 0 / 128 / 255."""
    assert 0 <= lo < hi <= 442 and 0 <= r_bg <= 32 and 0 <= r_fg <= 32
    D = box_sum(cmp, bg)
    back, fore = erode(D <= 9 * lo * lo, r_bg), erode(D >= 9 * hi * hi, r_fg)
    out = np.full(D.shape, 128, np.uint8)
    out[back] = 0
    out[fore] = 255
    return out


def trimaps(cmp, bg, **opts):
    """A stack: cmp uint8 [n,h,w,3]; bg [n,h,w,3], [1,h,w,3] or one plate [h,w,3] -> uint8 [n,h,w]."""
    bg = bg[None] if bg.ndim == 3 else bg
    return np.stack([trimap(cmp[i], bg[i if len(bg) > 1 else 0], **opts) for i in range(len(cmp))])


# ---------------------------------------------------------------- inputs

def noise_pair(h, w, seed=0):
    """Independent uniform noise frames: D spreads over its whole range, so with mid thresholds every label occurs."""
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (h, w, 3)).astype(np.uint8), rs.randint(0, 256, (h, w, 3)).astype(np.uint8)


def blob_pair(h, w, seed=0):
    """A smooth plate with little noise and a soft-edged disc of another colour composited on it: large regions of every
    label, with borders that cross tile and word boundaries."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[:h, :w].astype(np.float64)
    plate = np.stack([60 + 40 * np.sin(x / 9), 90 + 30 * np.cos(y / 7), 120 + 0 * x], -1)
    fg = np.stack([200 + 20 * np.sin(y / 5), 40 + 20 * np.cos(x / 6), 30 + 0 * x], -1)
    cx, cy = rs.uniform(0.3, 0.7) * w, rs.uniform(0.3, 0.7) * h
    rad = 0.3 * max(min(h, w), 8)
    a = np.clip((rad - np.hypot(x - cx, y - cy)) / 4 + 0.5, 0, 1)[..., None]
    frame = a * fg + (1 - a) * plate
    u8 = lambda v: np.clip(np.rint(v + rs.normal(0, 2, v.shape)), 0, 255).astype(np.uint8)  # noqa: E731
    return u8(frame), u8(plate)


def equal_pair(h, w, seed=0):
    """Frame == plate everywhere: D = 0."""
    bg = np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    return bg.copy(), bg


def extreme_pair(h, w, seed=0):
    """The largest difference there is: D = 9 * 3 * 255^2 everywhere."""
    return np.full((h, w, 3), 255, np.uint8), np.zeros((h, w, 3), np.uint8)


PAIRS = {"noise": noise_pair, "blob": blob_pair, "equal": equal_pair, "extreme": extreme_pair}


def scene(seed, h=96, w=160, sigma=4.0):
    """The synthetic composite the defaults are pinned on: a disc of radius 30 with a 4-pixel soft edge at (80, 48) over
    a smooth plate, Gaussian noise added to frame and plate independently -> (frame u8, plate u8, alpha f64)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:h, :w].astype(np.float64)
    plate = np.stack([60 + 40 * np.sin(x / 9), 90 + 30 * np.cos(y / 7), 120 + 0 * x], -1)
    fg = np.stack([200 + 20 * np.sin(y / 5), 40 + 20 * np.cos(x / 6), 30 + 0 * x], -1)
    alpha = np.clip((30 - np.hypot(x - 80, y - 48)) / 4 + 0.5, 0, 1)
    frame = alpha[..., None] * fg + (1 - alpha[..., None]) * plate
    u8 = lambda v: np.clip(np.rint(v + rng.normal(0, sigma, v.shape)), 0, 255).astype(np.uint8)  # noqa: E731
    return u8(frame), u8(plate), alpha
