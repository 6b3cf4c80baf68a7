"""Connected-component labelling on the GPU: ops.label_components against the breadth-first restatement
(tests/trimap_fill_ref.py), exactly: the labels are canonical, so every run gives the same integers."""

import numpy as np
import pytest
import torch

import trimap_fill_ref as ref
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

# the smallest first.  64 x 64: one tile column, two tile rows exactly; 65 x 129: one pixel into a third tile row and a
# third tile column; 70 x 90 and 133 x 261: ragged in both axes (3 x 5 = 15 tiles per frame of 64 x 32)
SHAPES = [(1, 1), (2, 2), (3, 3), (1, 17), (19, 1), (64, 64), (70, 90), (65, 129), (133, 261)]
N = 3
SENTINEL = 16            # int32 entries behind labels
MARK = 0x5A5A5A5A


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded_labels(count):
    buf = torch.full((count + SENTINEL,), MARK, dtype=torch.int32, device="cuda")
    return buf, buf[:count]


def check(masks, value=0, connectivities=(4, 8), case=None):
    from vmatting import ops
    n, h, w = masks.shape
    d_mask = dev(masks)
    for c in connectivities:
        buf, out = guarded_labels(n * h * w)
        got = ops.label_components(d_mask, value, c, out=out.view(n, h, w))
        assert got.data_ptr() == out.data_ptr() and got.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy(), ref.shared_labels(masks, value, c)), (case, c)
        assert (buf[n * h * w:] == MARK).all(), (case, c)
    assert np.array_equal(d_mask.cpu().numpy(), masks)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_random_masks_equal_the_restatement(shape):
    h, w = shape
    for p in ref.P_ZERO:
        masks = ref.random_trimaps(N, h, w, p)
        check(masks, case=p)
    check(ref.random_trimaps(N, h, w, 0.5), value=255, case="value 255")
    check(np.full((N, h, w), 7, np.uint8), value=7, case="all set")
    check(np.full((N, h, w), 7, np.uint8), value=8, case="none set")


def patterns():
    h, w = 133, 261
    yield "serpentine", ref.serpentine(h, w)
    yield "serpentine, open", ref.serpentine(h, w, open_end=True)
    yield "spiral", ref.spiral(h, w)
    yield "spiral, open", ref.spiral(h, w, open_end=True)
    yield "comb", ref.comb(h, w)
    yield "checkerboard", ref.checkerboard(h, w)
    yield "corner squares", ref.corner_squares(h, w)
    yield "rings", ref.rings(h, w)
    yield "framed zero", ref.framed_zero(h, w)
    for where in ("tl", "tr", "bl", "br"):
        yield "diagonal " + where, ref.one_pixel_touch(70, 90, where, diagonal=True)


@pytest.mark.parametrize("name", [name for name, _ in patterns()])
def test_patterns_equal_the_restatement(name):
    """One component with the longest chains a frame holds (serpentine, spiral, comb), every pixel its own component
    under 4 and all one under 8 (checkerboard), components that 8-connectivity joins and 4 does not."""
    tri = dict(patterns())[name]
    masks = np.stack([tri, tri[::-1, ::-1], tri[::-1]])
    check(masks, case=name)
    if name == "checkerboard":
        lab4, lab8 = ref.shared_labels(masks, 0, 4), ref.shared_labels(masks, 0, 8)
        assert (lab4[0][tri == 0] == np.flatnonzero(tri == 0)).all() and (lab8[0][tri == 0] == 0).all()
    if name == "corner squares":
        assert len(np.unique(ref.shared_labels(masks, 0, 4)[0])) == 3
        assert len(np.unique(ref.shared_labels(masks, 0, 8)[0])) == 2


def test_mask_at_any_byte_address_and_allocated_output():
    from vmatting import ops
    h, w = 70, 90
    masks = ref.random_trimaps(N, h, w, 0.6)
    want = ref.shared_labels(masks, 0, 4)
    for lead in (1, 3):
        buf = torch.zeros(lead + masks.size, dtype=torch.uint8, device="cuda")
        buf[lead:].copy_(dev(masks).view(-1))
        m = buf[lead:].view(N, h, w)
        assert m.data_ptr() % 4 == lead
        got = ops.label_components(m)
        assert got.shape == (N, h, w) and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(ops.label_components(dev(masks), connectivity=8).cpu().numpy(),
                          ref.shared_labels(masks, 0, 8))


def test_repeated_and_captured_calls():
    """Three calls on one input give identical labels (over labels left by another input), and a captured call replays
    on two new inputs of different structure."""
    from vmatting import ops
    h, w = 133, 261
    a = ref.random_trimaps(N, h, w, 0.6)
    b = np.stack([ref.serpentine(h, w), ref.comb(h, w), ref.checkerboard(h, w)])
    d_mask = dev(a)
    out = torch.zeros((N, h, w), dtype=torch.int32, device="cuda")
    ops.label_components(dev(b), out=out)
    runs = [ops.label_components(d_mask, out=out).cpu().numpy() for _ in range(3)]
    assert all(np.array_equal(r, ref.shared_labels(a, 0, 4)) for r in runs)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.label_components(d_mask, out=out)
    for masks in (b, a):
        d_mask.copy_(dev(masks))
        out.fill_(-7)
        g.replay()
        assert np.array_equal(out.cpu().numpy(), ref.shared_labels(masks, 0, 4))


def test_invalid_arguments():
    from vmatting import _lib, ops
    lib = _lib.lib()
    n, h, w = 2, 8, 12
    mask = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    labels = torch.full((n * h * w + 4,), 5, dtype=torch.int32, device="cuda")
    ok = dict(mask=mask.data_ptr(), n=n, h=h, w=w, value=0, connectivity=4, labels=labels.data_ptr())
    order = ("mask", "n", "h", "w", "value", "connectivity", "labels")
    bad = [dict(mask=None), dict(labels=None), dict(n=0), dict(h=0), dict(w=0), dict(value=256), dict(value=-1),
           dict(connectivity=5), dict(labels=labels.data_ptr() + 2), dict(mask=labels.data_ptr() + 8)]
    for change in bad:
        args = dict(ok, **change)
        assert lib.vm_components_label(*[args[k] for k in order], None) == _lib.VM_EINVAL, change
    assert (labels == 5).all()
    assert lib.vm_components_label(*[ok[k] for k in order], None) == _lib.VM_OK
    torch.cuda.synchronize()
    assert (labels[:n * h * w] == 0).all() and (labels[n * h * w:] == 5).all()
    for kw in (dict(value=256), dict(connectivity=6), dict(out=torch.zeros((n, h, 11), dtype=torch.int32, device="cuda")),
               dict(out=torch.zeros((n, h, w), dtype=torch.int64, device="cuda"))):
        with pytest.raises(ValueError):
            ops.label_components(mask, **kw)
    with pytest.raises(TypeError):
        ops.label_components(mask, value=1.0)
