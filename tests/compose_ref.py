"""The arithmetic of vm_matte_compose restated in numpy (include/vmatting.h), shared by tests/test_compose_host.py and
tests/test_gpu_compose.py.  Everything is float64, each value is rounded once at the end:

    fin(v)   = (uint8) rint(min(max(v, 0), 255)), ties to even
    q        = the 8-bit matte of vm_matte_quantize: min(max(rintf(alpha * 255.f), 0), 255), NaN -> 0
    over     a = (double)alpha clamped to [0,1], NaN -> 0;  fin(c + (1 - a) * (nw - b))
    premul   fin(c - ((255 - q) * b) / 255), A = q
    bgra     q == 0: 0, else fin(b + ((c - b) * 255) / q), A = q
"""

import numpy as np

MODES = ("over", "bgra", "premul")


def fin(v):
    return np.rint(np.minimum(np.maximum(v, 0.0), 255.0)).astype(np.uint8)


def quantize8(alpha):
    with np.errstate(invalid="ignore"):
        r = np.rint(np.asarray(alpha, np.float32) * np.float32(255.0))
        r = np.where(r >= 0, r, np.float32(0.0))  # NaN and negatives -> 0
    return np.minimum(r, np.float32(255.0)).astype(np.uint8)


def _frames(plate, n):
    """[n,h,w,3] float64 of a per-frame [n,h,w,3] or static [h,w,3] / [1,h,w,3] uint8 plane."""
    plate = np.asarray(plate)
    if plate.ndim == 3:
        plate = plate[None]
    return np.broadcast_to(plate, (n,) + plate.shape[1:]).astype(np.float64)


def compose(alpha, cmp, bg, new_bg=None, mode="over"):
    """alpha f32 [n,h,w], cmp u8 [n,h,w,3], bg / new_bg u8 [n,h,w,3] | [1,h,w,3] | [h,w,3] -> u8 [n,h,w,3] ("over") or
    [n,h,w,4] BGRA ("bgra" straight, "premul" premultiplied)."""
    alpha = np.asarray(alpha)
    assert alpha.dtype == np.float32 and mode in MODES and (new_bg is not None) == (mode == "over")
    n = cmp.shape[0]
    c, b = cmp.astype(np.float64), _frames(bg, n)
    if mode == "over":
        with np.errstate(invalid="ignore"):
            a = alpha.astype(np.float64)
            a = np.where(a >= 0.0, a, 0.0)  # NaN and negatives -> 0
        a = np.minimum(a, 1.0)[..., None]
        return fin(c + (1.0 - a) * (_frames(new_bg, n) - b))
    q8 = quantize8(alpha)
    q = q8.astype(np.float64)[..., None]
    if mode == "premul":
        bgr = fin(c - ((255.0 - q) * b) / 255.0)
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            bgr = np.where(q == 0.0, np.uint8(0), fin(np.where(q == 0.0, 0.0, b + ((c - b) * 255.0) / q)))
    return np.concatenate([bgr, q8[..., None]], -1).astype(np.uint8)


def special_alphas():
    """The alpha values every kernel test carries besides random ones: the clamps, NaN, a denormal, every rounding
    tie of the 8-bit matte, and the first and last non-trivial levels."""
    ties = (np.arange(255, dtype=np.float64) + 0.5) / 255.0
    return np.concatenate([np.array([0.0, 1.0, -0.25, 1.5, np.nan, 1e-40, 1.0 / 255.0, 254.0 / 255.0]),
                           ties]).astype(np.float32)
