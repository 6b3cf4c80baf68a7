"""numpy restatement of vm_components_label and vm_trimap_fill_enclosed (include/vmatting.h), and the inputs their tests
share.

The algorithm is not the kernels': a breadth-first flood per component, seeded in row-major order, so a component's
seed is its smallest index.  No union-find, no scipy."""

import numpy as np

N4 = ((-1, 0), (0, -1), (0, 1), (1, 0))
N8 = N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def label(mask, value=0, connectivity=4):
    """One frame: uint8 [h,w] -> int32 [h,w]: the smallest row-major index of the component of every pixel that equals
    ``value``, -1 elsewhere."""
    assert connectivity in (4, 8)
    steps = N4 if connectivity == 4 else N8
    h, w = mask.shape
    todo = (mask == value)
    out = np.full((h, w), -1, np.int32)
    for seed in np.flatnonzero(todo):
        y, x = divmod(int(seed), w)
        if not todo[y, x]:
            continue
        todo[y, x] = False
        out[y, x] = seed
        front = [(y, x)]
        while front:
            nxt = []
            for cy, cx in front:
                for dy, dx in steps:
                    yy, xx = cy + dy, cx + dx
                    if 0 <= yy < h and 0 <= xx < w and todo[yy, xx]:
                        todo[yy, xx] = False
                        out[yy, xx] = seed
                        nxt.append((yy, xx))
            front = nxt
    return out


def labels(masks, value=0, connectivity=4):
    return np.stack([label(m, value, connectivity) for m in masks])


def fill_from_labels(tri, lab, max_area=0):
    """One frame's fill from its 4-connected labels of the zero bytes."""
    h, w = tri.shape
    out = tri.copy()
    if h < 3 or w < 3:
        return out
    ids = lab[lab >= 0]
    area = np.bincount(ids, minlength=h * w)
    edge = np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]])
    open_ = np.zeros(h * w, bool)
    open_[edge[edge >= 0]] = True
    fill = (area > 0) & ~open_
    if max_area:
        fill &= area <= max_area
    out[(lab >= 0) & fill[np.maximum(lab, 0)]] = 128
    return out


def fill(tri, max_area=0):
    """One frame: uint8 [h,w] -> uint8 [h,w], 128 on every enclosed 4-connected component of zero bytes of at most
    ``max_area`` pixels (0: any area)."""
    return fill_from_labels(tri, label(tri, 0, 4), max_area)


def fills(tris, max_area=0):
    return np.stack([fill(t, max_area) for t in tris])


_LABELS = {}


def shared_labels(masks, value=0, connectivity=4):
    """labels() computed once per input and shared among the tests of a run; the result is not to be written."""
    key = (masks.shape, masks.tobytes(), value, connectivity)
    if key not in _LABELS:
        _LABELS[key] = labels(masks, value, connectivity)
        _LABELS[key].setflags(write=False)
    return _LABELS[key]


def shared_fills(tris, max_area=0):
    lab = shared_labels(tris, 0, 4)
    return np.stack([fill_from_labels(t, l, max_area) for t, l in zip(tris, lab)])


def census(tri):
    """(components, enclosed components, largest area) of a frame's zero bytes."""
    lab = label(tri, 0, 4)
    roots = np.unique(lab[lab >= 0])
    edge = np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]])
    open_roots = np.unique(edge[edge >= 0])
    area = np.bincount(lab[lab >= 0], minlength=1)
    return len(roots), len(roots) - len(open_roots), int(area.max()) if len(roots) else 0


# ---------------------------------------------------------------- inputs

P_ZERO = (0.3, 0.5, 0.6, 0.7, 0.9)


def random_trimaps(n, h, w, p, seed=3):
    """A pixel is 0 with probability p, else 128 or 255."""
    rs = np.random.RandomState(seed)
    zero = rs.random_sample((n, h, w)) < p
    other = np.where(rs.randint(0, 2, (n, h, w)) == 1, 255, 128)
    return np.where(zero, 0, other).astype(np.uint8)


def serpentine(h, w, open_end=False):
    """A one-pixel-wide corridor of zeros that runs along every other row inside a one-pixel frame of 128, joined at
    alternating ends: one component with the longest chain a frame can hold.  ``open_end``: its last pixel is joined to
    the frame's border."""
    t = np.full((h, w), 128, np.uint8)
    rows = list(range(1, h - 1, 2))
    for k, y in enumerate(rows):
        t[y, 1:w - 1] = 0
        if k + 1 < len(rows):
            t[y + 1, w - 2 if k % 2 == 0 else 1] = 0
    if open_end:
        y = rows[-1]
        if (len(rows) - 1) % 2 == 0:
            t[y, w - 1] = 0
        else:
            t[y, 0] = 0
    return t


def spiral(h, w, open_end=False):
    """A one-pixel-wide corridor of zeros that winds inwards from (1, 1) with one-pixel walls of 128, inside a frame of
    128: walk ahead while the cell ahead is free and the one beyond it is no corridor, else turn right.  ``open_end``:
    its first pixel is joined to the border."""
    t = np.full((h, w), 128, np.uint8)

    def inside(yy, xx):
        return 1 <= yy <= h - 2 and 1 <= xx <= w - 2

    y, x, dy, dx, turns = 1, 1, 0, 1, 0
    t[y, x] = 0
    while turns < 2:
        ny, nx = y + dy, x + dx
        if inside(ny, nx) and t[ny, nx] and not (inside(ny + dy, nx + dx) and t[ny + dy, nx + dx] == 0):
            y, x, turns = ny, nx, 0
            t[y, x] = 0
        else:
            dy, dx, turns = dx, -dy, turns + 1
    if open_end:
        t[1, 0] = 0
    return t


def comb(h, w):
    """Teeth of zeros in every other column, pointing up from a joining bottom row, inside a frame of 128: the smallest
    index lies in the first tooth and reaches the others only through the last row."""
    t = np.full((h, w), 128, np.uint8)
    t[1:h - 1, 1:w - 1:2] = 0
    t[h - 2, 1:w - 1] = 0
    return t


def checkerboard(h, w):
    y, x = np.mgrid[:h, :w]
    return np.where((y + x) % 2 == 0, 0, 255).astype(np.uint8)


def corner_squares(h, w):
    """Two 5 x 5 squares of zeros that touch only at a corner, one of them on the frame's border."""
    t = np.full((h, w), 255, np.uint8)
    t[0:5, 0:5] = 0
    t[5:10, 5:10] = 0
    return t


def rings(h, w):
    """Nested rings 0 / 255 / 0 / 255 / 0 outwards from the centre, 3 pixels wide each, in a frame of 128."""
    y, x = np.mgrid[:h, :w]
    d = np.maximum(np.abs(y - h // 2), np.abs(x - w // 2)) // 3
    t = np.where(d % 2 == 0, 0, 255).astype(np.uint8)
    t[d > 4] = 128
    return t


def framed_zero(h, w):
    t = np.zeros((h, w), np.uint8)
    t[0], t[-1], t[:, 0], t[:, -1] = 128, 128, 128, 128
    return t


def one_pixel_touch(h, w, where, diagonal=False):
    """The whole interior zero in a frame of 255, and one zero pixel on the border: beside the corner "tl" / "tr" / "bl"
    / "br" (a corner pixel itself has no 4-neighbour off the border), or "mid": the middle of the left edge.  The
    component touches the border at exactly that pixel.  ``diagonal``: the corner pixel itself instead, which meets the
    interior only diagonally: under 4-connectivity the interior stays enclosed."""
    t = np.full((h, w), 255, np.uint8)
    t[1:h - 1, 1:w - 1] = 0
    if where == "mid":
        t[h // 2, 0] = 0
        return t
    y = 0 if where[0] == "t" else h - 1
    x = 0 if where[1] == "l" else w - 1
    if diagonal:
        t[y, x] = 0
    else:
        t[y, 1 if x == 0 else w - 2] = 0
    return t


def odd_bytes(h, w, seed=1):
    """Every byte value occurs, zeros enclosed and not."""
    rs = np.random.RandomState(seed)
    t = rs.randint(0, 256, (h, w)).astype(np.uint8)
    t[rs.random_sample((h, w)) < 0.4] = 0
    return t


def area_squares(h, w):
    """Enclosed blocks of 24, 25 and 26 zeros and three isolated zero pixels, in a frame of 255."""
    t = np.full((h, w), 255, np.uint8)
    t[2:6, 2:8] = 0           # 24
    t[8:13, 2:7] = 0          # 25
    t[2:7, 10:15] = 0         # 25 + 1
    t[7, 10] = 0
    t[15, 3], t[15, 5], t[17, 9] = 0, 0, 0
    return t


def holed_blob_pair(h, w, seed=0, patch=15):
    """trimap_plate_ref.blob_pair with a patch x patch square at the disc's centre overwritten by plate colour plus
    noise: foreground that matches the plate."""
    import trimap_plate_ref as plate_ref
    frame, plate = plate_ref.blob_pair(h, w, seed)
    rs = np.random.RandomState(seed)
    cx, cy = int(rs.uniform(0.3, 0.7) * w), int(rs.uniform(0.3, 0.7) * h)   # blob_pair's first two draws
    y0, x0 = cy - patch // 2, cx - patch // 2
    noise = np.random.RandomState(seed + 1000).normal(0, 2, (patch, patch, 3))
    frame = frame.copy()
    frame[y0:y0 + patch, x0:x0 + patch] = np.clip(np.rint(plate[y0:y0 + patch, x0:x0 + patch] + noise), 0, 255)
    return frame, plate
