"""numpy restatement of vm_plate_from_samples (include/vmatting.h), and the inputs its tests share.

plate(samples): the samples sorted along the first axis; the plate is row (n - 1) // 2 of that, the spread the largest
difference over a pixel's three bytes between rows n - 1 - (n - 1) // 4 and (n - 1) // 4."""

import numpy as np

MAX_SAMPLES = 64


def ranks(n):
    """(lo, m, hi): the sorted positions the spread's lower end, the plate and the spread's upper end read."""
    lo = (n - 1) // 4
    return lo, (n - 1) // 2, n - 1 - lo


def plate(samples):
    """samples uint8 [n,h,w,3] -> (plate uint8 [h,w,3], spread uint8 [h,w])."""
    assert samples.dtype == np.uint8 and samples.ndim == 4 and samples.shape[3] == 3
    assert 1 <= len(samples) <= MAX_SAMPLES
    lo, m, hi = ranks(len(samples))
    s = np.sort(samples, 0)
    return s[m], (s[hi].astype(np.int16) - s[lo].astype(np.int16)).max(-1).astype(np.uint8)


# ---------------------------------------------------------------- inputs

def noise(n, h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)


def binary(n, h, w, seed=0):
    """Only 0 and 255: every comparison is a tie or the largest difference there is."""
    return (np.random.RandomState(seed).randint(0, 2, (n, h, w, 3)) * 255).astype(np.uint8)


def constant(n, h, w, seed=0):
    """One frame n times: all ties."""
    return np.repeat(noise(1, h, w, seed), n, 0)


def ascending(n, h, w, seed=0):
    return np.sort(noise(n, h, w, seed), 0)


def descending(n, h, w, seed=0):
    return ascending(n, h, w, seed)[::-1].copy()


def lanes(n, h, w, seed=0):
    """Byte k (mod 4) of a frame gets the ascending stack rolled by k along n: the four bytes of a dword hold values of
    four different ranks in every sample, so a packed implementation that lets one byte's order leak into its neighbour
    gets them wrong."""
    flat = ascending(n, h, w, seed).reshape(n, -1).copy()
    for k in range(1, 4):
        flat[:, k::4] = np.roll(flat[:, k::4], k, 0)
    return flat.reshape(n, h, w, 3)


STACKS = {"noise": noise, "binary": binary, "constant": constant, "ascending": ascending, "descending": descending,
          "lanes": lanes}

BRIGHT, DARK, RADIUS = (250, 240, 230), (5, 10, 15), 4


def true_plate(h, w):
    """A noise-free plate with no two neighbouring pixels alike, every value well between DARK and BRIGHT."""
    y, x = np.mgrid[:h, :w]
    return np.stack([60 + (x * 2 + y) % 100, 70 + (x + y * 3) % 90, 80 + (x * 5 + y * 2) % 70], -1).astype(np.uint8)


def recovery_clip(n, h=40, w=56, park=False):
    """n frames of true_plate(h, w) with a bright disc crossing it along the row 0.3 h and a dark one along 0.7 h, left
    to right, at (w - 7) / (n - 1) pixels a frame.  With ``park`` the dark disc stays at its start for the first
    (n - 1) // 2 + 2 frames, more than half, and crosses in what is left.
    -> (frames uint8 [n,h,w,3], plate uint8 [h,w,3], cover int [h,w]: in how many frames a disc covers the pixel,
    parked bool [h,w]: the pixels under the parked disc)."""
    bg = true_plate(h, w)
    y, x = np.mgrid[:h, :w]
    frames = np.repeat(bg[None], n, 0)
    cover = np.zeros((h, w), int)
    parked = np.zeros((h, w), bool)
    stay = (n - 1) // 2 + 2 if park else 0
    for t in range(n):
        at = 3 + (w - 7) * t / max(n - 1, 1)
        dark_at = 3 + (w - 7) * max(t - stay + 1, 0) / max(n - stay, 1)
        for colour, cy, cx in ((BRIGHT, int(0.3 * h), at), (DARK, int(0.7 * h), dark_at)):
            disc = np.hypot(x - cx, y - cy) <= RADIUS
            frames[t][disc] = colour
            cover += disc
            if colour is DARK and t < stay:
                parked |= disc
    return frames, bg, cover, parked
