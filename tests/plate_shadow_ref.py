"""numpy restatement of vm_trimap_from_plate_shadow (include/vmatting.h), and the inputs its tests share.

trimap(cmp, bg, lo, hi, r_bg, r_fg, shadow): trimap_plate_ref.trimap with the shadow-tolerant distance d' in place of d;
int64 throughout.  shadow: None (the plain distance) or a dict over DEFAULTS."""

import numpy as np

import trimap_plate_ref as plain

DEFAULTS = {"floor": 128, "ceil": 256, "dark": 32}
# the option triples (floor, ceil, dark) the tests cross their inputs with: the defaults, everything in range, nothing
# but a pixel of exactly the plate's brightness on a plate of level 255, and a highlight passing on any plate but black
TRIPLES = [(128, 256, 32), (1, 512, 0), (256, 256, 255), (200, 300, 1)]


def terms(cmp, bg):
    """uint8 [h,w,3] twice -> int64 [h,w] each: d, ee, ie, ii, cross."""
    i, e = cmp.astype(np.int64), bg.astype(np.int64)
    ee, ie, ii = (e * e).sum(-1), (i * e).sum(-1), (i * i).sum(-1)
    return plain.distance(cmp, bg), ee, ie, ii, ii * ee - ie * ie


def in_range(ee, ie, floor=128, ceil=256, dark=32):
    """Where the plate's chromaticity is trusted and the light ratio ie / ee is one a shadow may have."""
    return (ee >= max(3 * dark * dark, 1)) & (floor * ee <= 256 * ie) & (256 * ie <= ceil * ee)


def distance_shadow(cmp, bg, floor=128, ceil=256, dark=32):
    """d' = cross // ee where in range, d elsewhere: uint8 [h,w,3] twice -> int64 [h,w]."""
    assert 1 <= floor <= 256 <= ceil <= 512 and 0 <= dark <= 255
    d, ee, ie, ii, cross = terms(cmp, bg)
    return np.where(in_range(ee, ie, floor, ceil, dark), cross // np.maximum(ee, 1), d)


def box_sum(cmp, bg, shadow=None):
    return plain.box3(plain.distance(cmp, bg) if shadow is None else distance_shadow(cmp, bg, **shadow))


def from_box_sum(D, lo=16, hi=48, r_bg=4, r_fg=8):
    """The thresholds, the erosions and the labels: D int64 [h,w] -> uint8 [h,w]."""
    assert 0 <= lo < hi <= 442 and 0 <= r_bg <= 32 and 0 <= r_fg <= 32
    out = np.full(D.shape, 128, np.uint8)
    out[plain.erode(D <= 9 * lo * lo, r_bg)] = 0
    out[plain.erode(D >= 9 * hi * hi, r_fg)] = 255
    return out


def trimap(cmp, bg, lo=16, hi=48, r_bg=4, r_fg=8, shadow=None):
    """One frame: cmp, bg uint8 [h,w,3] -> uint8 [h,w] of 0 / 128 / 255."""
    if shadow is not None:
        shadow = dict(DEFAULTS, **shadow)
    return from_box_sum(box_sum(cmp, bg, shadow), lo, hi, r_bg, r_fg)


def trimaps(cmp, bg, shadow=None, **opts):
    """A stack: cmp uint8 [n,h,w,3]; bg [n,h,w,3], [1,h,w,3] or one plate [h,w,3] -> uint8 [n,h,w]."""
    bg = bg[None] if bg.ndim == 3 else bg
    return np.stack([trimap(cmp[i], bg[i if len(bg) > 1 else 0], shadow=shadow, **opts) for i in range(len(cmp))])


# ---------------------------------------------------------------- inputs

def ratio_pair(h, w, seed=0):
    """The plate is uniform noise; the frame is the plate times one factor per pixel, uniform in 0.3..1.2, plus N(0, 6):
    light ratios on both sides of any floor and ceil, and small distances to the plate's line."""
    rs = np.random.RandomState(seed)
    plate = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    frame = plate * rs.uniform(0.3, 1.2, (h, w, 1)) + rs.normal(0, 6, (h, w, 3))
    return np.clip(np.rint(frame), 0, 255).astype(np.uint8), plate


def dark_pair(h, w, seed=0):
    """A plate of levels 0..40 with all-zero pixels (ee = 0) among them, under a frame of levels 0..40: ee on both sides
    of 3 dark^2 for the dark thresholds in use."""
    rs = np.random.RandomState(seed)
    plate = rs.randint(0, 41, (h, w, 3)).astype(np.uint8)
    plate[rs.uniform(size=(h, w)) < 0.1] = 0
    plate[0, 0] = 0
    return rs.randint(0, 41, (h, w, 3)).astype(np.uint8), plate


PAIRS = dict(plain.PAIRS, ratio=ratio_pair, dark=dark_pair)


def shadow_scene(seed, s, h=96, w=160, sigma=4.0):
    """trimap_plate_ref.scene with a soft elliptical shadow that keeps ``s`` of the light on the floor beside the disc,
    on the background only -> (frame u8, plate u8, alpha f64, m f64): m is the shadow's matte, 1 in its core."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:h, :w].astype(np.float64)
    plate = np.stack([60 + 40 * np.sin(x / 9), 90 + 30 * np.cos(y / 7), 120 + 0 * x], -1)
    fg = np.stack([200 + 20 * np.sin(y / 5), 40 + 20 * np.cos(x / 6), 30 + 0 * x], -1)
    alpha = np.clip((30 - np.hypot(x - 80, y - 48)) / 4 + 0.5, 0, 1)
    m = np.clip((1 - np.hypot((x - 118) / 34, (y - 70) / 18)) * 6 + 0.5, 0, 1)
    light = 1 - (1 - s) * m
    frame = alpha[..., None] * fg + (1 - alpha[..., None]) * plate * light[..., None]
    u8 = lambda v: np.clip(np.rint(v + rng.normal(0, sigma, v.shape)), 0, 255).astype(np.uint8)  # noqa: E731
    return u8(frame), u8(plate), alpha, m


def grey_scene(h=64, w=96):
    """The documented limit: a 110-grey square on a flat 180-grey plate -> (frame u8, plate u8, the square's mask)."""
    plate = np.full((h, w, 3), 180, np.uint8)
    frame = plate.copy()
    square = np.zeros((h, w), bool)
    square[16:48, 32:64] = True
    frame[square] = 110
    return frame, plate, square
