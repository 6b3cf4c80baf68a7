"""numpy restatement of vm_trimap_propagate (include/vmatting.h), and the inputs its tests share.

propagate(prev, flow, grow): output pixel (x, y) looks at (xs, ys) = (f32(x) + flow_x, f32(y) + flow_y).  Outside the
image (or NaN) it is 128.  Else the window is the pixels the bilinear warp would touch, x0 = floor(xs) .. x1 = x0 +
(xs > x0) and the same in y, grown by ``grow`` and clipped to the image; the output is 255 if all of prev in it is 255,
0 if all of it is 0, else 128.  Vectorised: the window is the union of the symmetric (2 grow + 1)^2 windows at the up
to four touched pixels, so per class one map "my symmetric window is all of this class" (a minimum over shifted
copies, rows then columns) and then a gather of four entries.
"""

import numpy as np

import flow_est_ref as fer


def _all_in_window(mask, grow):
    """mask [h,w] bool -> whether every pixel within ``grow`` (Chebyshev, clipped to the image) is set."""
    h, w = mask.shape
    p = np.pad(mask, grow, mode="constant", constant_values=True)
    rows = np.minimum.reduce([p[:, s:s + w] for s in range(2 * grow + 1)])
    return np.minimum.reduce([rows[s:s + h] for s in range(2 * grow + 1)])


def propagate(prev, flow, grow):
    assert prev.dtype == np.uint8 and flow.dtype == np.float32 and flow.shape == prev.shape + (2,)
    h, w = prev.shape
    x, y = fer.grid(h, w, np.float32)
    with np.errstate(invalid="ignore"):
        xs, ys = x + flow[..., 0], y + flow[..., 1]
        inside = (xs >= 0) & (xs <= np.float32(w - 1)) & (ys >= 0) & (ys <= np.float32(h - 1))
    xs, ys = np.where(inside, xs, np.float32(0)), np.where(inside, ys, np.float32(0))
    x0, y0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    x1, y1 = x0 + (xs > x0), y0 + (ys > y0)
    out = np.full((h, w), 128, np.uint8)
    for value in (255, 0):
        m = _all_in_window(prev == value, grow)
        out[inside & m[y0, x0] & m[y0, x1] & m[y1, x0] & m[y1, x1]] = value
    return out


def chain(key, flows, grow):
    """The trimaps of len(flows) frames: the key itself for frame 0 (flows[0] is unused), then frame by frame."""
    tris = [key]
    for f in flows[1:]:
        tris.append(propagate(tris[-1], f, grow))
    return np.stack(tris)


def canonical(tri):
    return np.where(tri == 255, 255, np.where(tri == 0, 0, 128)).astype(np.uint8)


# ---------------------------------------------------------------- inputs

def blob_trimap(h, w, seed=0):
    """A foreground blob with a 128 band around it on a background of 0."""
    rs = np.random.RandomState(seed)
    x, y = fer.grid(h, w, np.float64)
    cx, cy = w * rs.uniform(0.4, 0.6), h * rs.uniform(0.4, 0.6)
    r = np.hypot((x - cx) / max(0.33 * w, 1.0), (y - cy) / max(0.33 * h, 1.0))
    r = r + 0.1 * np.sin(0.37 * x + 0.23 * y)
    return np.where(r < 0.7, 255, np.where(r < 1.0, 128, 0)).astype(np.uint8)


def noise_trimap(h, w, seed=0):
    """Blocks of 0 / 128 / 255 a few pixels wide, sprinkled with 1, 127 and 254, which all count as unknown."""
    rs = np.random.RandomState(seed)
    cell = 7
    coarse = rs.choice(np.array([0, 255, 255, 0, 128], np.uint8), ((h + cell - 1) // cell, (w + cell - 1) // cell))
    tri = np.kron(coarse, np.ones((cell, cell), np.uint8))[:h, :w].copy()
    odd = rs.uniform(size=(h, w)) < 0.01
    tri[odd] = rs.choice(np.array([1, 127, 254], np.uint8), int(odd.sum()))
    return tri


TRIMAPS = {"blob": blob_trimap, "noise": noise_trimap}


def edge_flow(h, w, seed=0):
    """Small random flows with, scattered over the image: NaN, +inf and -inf in either component, targets exactly on the
    last column / row and on column / row 0, and targets just outside the image on every side."""
    rs = np.random.RandomState(seed)
    f = rs.uniform(-2, 2, (h, w, 2)).astype(np.float32)
    x, y = fer.grid(h, w, np.float32)
    pos = (x, y)
    last = (np.float32(w - 1), np.float32(h - 1))
    kind = rs.randint(0, 24, (h, w))
    for c in (0, 1):
        specials = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), last[c] - pos[c], -pos[c],
                    last[c] - pos[c] + np.float32(0.01), -pos[c] - np.float32(0.01), last[c] - pos[c] + np.float32(1)]
        for i, v in enumerate(specials):
            f[..., c] = np.where(kind == 8 * c + i, v, f[..., c])
    # the exact targets are exact: f32(x) + f32(last - x) is last, f32(x) + f32(-x) is 0
    return f


def flow_fields(h, w, seed=0):
    """name -> f32 [h,w,2]."""
    rs = np.random.RandomState(seed + 100)
    return {
        "zero": np.zeros((h, w, 2), np.float32),
        "shift_int": fer.shift_flow(h, w, 3.0, -2.0).astype(np.float32),
        "shift": fer.shift_flow(h, w, 3.5, -2.25).astype(np.float32),
        "zoom": fer.zoom_flow(h, w).astype(np.float32),
        "random": rs.uniform(-12, 12, (h, w, 2)).astype(np.float32),
        "edge": edge_flow(h, w, seed),
    }
