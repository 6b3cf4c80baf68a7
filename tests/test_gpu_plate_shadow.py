"""The shadow-tolerant trimap from the background plate on the GPU: ops.trimap_from_plate(shadow=...) against the numpy
restatement (tests/plate_shadow_ref.py), byte for byte, with nothing written outside the results."""

import numpy as np
import pytest
import torch

import plate_shadow_ref as ref
import trimap_plate_ref as plain
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

# test_gpu_trimap_plate's shapes: 133 x 261 is 2 x 9 candidate tiles per frame, ragged in both axes; 40 x 200 a row of 4
# words whose last is ragged; 70 x 90 and the two one-pixel-wide shapes a row shorter than any tile
SHAPES = [(70, 90), (133, 261), (40, 200), (1, 17), (19, 1)]
# (lo, hi, r_bg, r_fg): the ordinary thresholds, low ones without erosion (d' is small where it applies: every label on
# `ratio`), high ones with the largest radius (every label on `noise`)
SETTINGS = [(16, 48, 1, 3), (8, 30, 0, 0), (120, 200, 2, 32)]
N = 3
SENTINEL = 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(nbytes, fill, lead=0):
    """A uint8 device buffer of ``nbytes`` with SENTINEL bytes of ``fill`` behind it (and ``lead`` in front)."""
    buf = torch.full((lead + nbytes + SENTINEL,), fill, dtype=torch.uint8, device="cuda")
    return buf, buf[lead:lead + nbytes]


def intact(buf, nbytes, fill, lead=0):
    b = buf.cpu().numpy()
    return (b[:lead] == fill).all() and (b[lead + nbytes:] == fill).all()


def stack(kind, h, w, seed):
    pairs = [ref.PAIRS[kind](h, w, seed + i) for i in range(N)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def options(triple):
    return dict(zip(ref.DEFAULTS, triple))


@pytest.mark.parametrize("shape", SHAPES)
def test_equals_the_restatement(shape):
    from vmatting import ops
    h, w = shape
    nwork = ops.trimap_from_plate_workspace_bytes(N, h, w)
    labels, shares = set(), []
    for kind in ref.PAIRS:
        cmp, bgs = stack(kind, h, w, seed=11)
        d_cmp = dev(cmp)
        for bg in (bgs, bgs[:1]):                             # nb = 3 and nb = 1
            d_bg = dev(bg)
            for triple in ref.TRIPLES:
                opts = options(triple)
                pick = [bg[i if len(bg) > 1 else 0] for i in range(N)]
                D = [ref.box_sum(cmp[i], pick[i], opts) for i in range(N)]
                shares.append(np.mean([ref.in_range(*ref.terms(cmp[i], pick[i])[1:3], *triple) for i in range(N)]))
                for lo, hi, r_bg, r_fg in SETTINGS:
                    obuf, out = guarded(N * h * w, 0xA5)
                    wbuf, work = guarded(nwork, 0x5A)
                    got = ops.trimap_from_plate(d_cmp, d_bg, lo, hi, r_bg, r_fg, out=out.view(N, h, w), work=work,
                                                shadow=opts)
                    assert got.data_ptr() == out.data_ptr()
                    want = np.stack([ref.from_box_sum(D[i], lo, hi, r_bg, r_fg) for i in range(N)])
                    case = (kind, len(bg), triple, lo, hi, r_bg, r_fg)
                    assert np.array_equal(got.cpu().numpy(), want), case
                    assert intact(obuf, N * h * w, 0xA5) and intact(wbuf, nwork, 0x5A), case
                    labels |= set(np.unique(want).tolist())
            assert np.array_equal(d_bg.cpu().numpy(), bg)
        assert np.array_equal(d_cmp.cpu().numpy(), cmp)
    # what the cases covered, on the restatement: every label, and on some input each branch of d' on >= 5 % of the pixels
    assert labels == {0, 128, 255}
    assert any(0.05 <= s <= 0.95 for s in shares) and min(shares) == 0.0 and max(shares) >= 0.95
    # the restatement itself, through its own entry, once
    cmp, bgs = stack("ratio", h, w, seed=11)
    assert np.array_equal(ops.trimap_from_plate(dev(cmp), dev(bgs), 8, 30, 0, 0, shadow={}).cpu().numpy(),
                          ref.trimaps(cmp, bgs, lo=8, hi=30, r_bg=0, r_fg=0, shadow={}))


def test_coverage_of_the_inputs():
    """At 70 x 90: `ratio` at (8, 30, 0, 0) shows all three labels, `noise` and `ratio` are about half in range under the
    defaults, and `dark` has both branches on >= 5 % of its pixels where dark is 0 or 1."""
    h, w = 70, 90
    cmp, bg = stack("ratio", h, w, seed=11)
    assert set(np.unique(ref.trimaps(cmp, bg, lo=8, hi=30, r_bg=0, r_fg=0, shadow={})).tolist()) == {0, 128, 255}
    share = {}
    for kind in ("noise", "ratio", "dark"):
        cmp, bg = stack(kind, h, w, seed=11)
        share[kind] = [np.mean([ref.in_range(*ref.terms(cmp[i], bg[i])[1:3], *t) for i in range(N)]) for t in ref.TRIPLES]
    assert 0.45 <= share["noise"][0] <= 0.60 and 0.45 <= share["ratio"][0] <= 0.60
    assert 0.05 <= share["dark"][1] <= 0.95 and 0.05 <= share["dark"][3] <= 0.95


def test_planes_off_four_bytes_are_read_bytewise():
    """cmp and bg that do not start on 4 bytes take the bytewise loads: the same bytes."""
    from vmatting import ops
    h, w = 70, 90
    cmp, bg = stack("ratio", h, w, seed=5)
    want = ref.trimaps(cmp, bg[0], lo=8, hi=30, r_bg=0, r_fg=0, shadow={})
    assert set(np.unique(want).tolist()) == {0, 128, 255}
    for lead_c, lead_b in ((1, 0), (0, 3), (2, 2)):
        _, c = guarded(cmp.size, 0, lead=lead_c)
        _, b = guarded(bg[0].size, 0, lead=lead_b)
        c.copy_(dev(cmp).view(-1))
        b.copy_(dev(bg[0]).view(-1))
        assert c.data_ptr() % 4 == lead_c and b.data_ptr() % 4 == lead_b
        got = ops.trimap_from_plate(c.view(N, h, w, 3), b.view(h, w, 3), 8, 30, 0, 0, shadow={})
        assert np.array_equal(got.cpu().numpy(), want), (lead_c, lead_b)


def test_unaligned_output_and_the_reader():
    """An output that does not start on 16 bytes is stored bytewise, nothing before or behind it is touched; the call
    allocates what it is not given; reader.trimap_from_plate(shadow="chroma") returns what it was given."""
    from vmatting import ops, reader
    h, w = 133, 261
    cmp, bg = stack("blob", h, w, seed=2)
    cmp = (cmp * np.linspace(0.55, 1.0, w)[None, None, :, None]).astype(np.uint8)   # the light falls off to the left
    want = ref.trimaps(cmp, bg, shadow={}, **plain.DEFAULTS)
    assert set(np.unique(want).tolist()) == {0, 128, 255}
    assert not np.array_equal(want, plain.trimaps(cmp, bg, **plain.DEFAULTS))
    obuf, out = guarded(N * h * w, 0xA5, lead=3)
    assert out.data_ptr() % 16 == 3
    got = ops.trimap_from_plate(dev(cmp), dev(bg), out=out.view(N, h, w), shadow={})
    assert np.array_equal(got.cpu().numpy(), want) and intact(obuf, N * h * w, 0xA5, lead=3)
    got = ops.trimap_from_plate(dev(cmp), dev(bg), shadow=dict(ref.DEFAULTS))
    assert got.shape == (N, h, w) and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    got = reader.trimap_from_plate(cmp, bg, shadow="chroma")
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    got = reader.trimap_from_plate(dev(cmp[1]), dev(bg[1]), lo=8, hi=30, shadow="chroma", shadow_options={"floor": 200})
    assert got.is_cuda and np.array_equal(got.cpu().numpy(),
                                          ref.trimap(cmp[1], bg[1], lo=8, hi=30, shadow={"floor": 200}))
    assert not np.array_equal(got.cpu().numpy(), ref.trimap(cmp[1], bg[1], lo=8, hi=30, shadow={}))


def test_no_shadow_is_the_call_as_it_was():
    from vmatting import ops
    h, w = 70, 90
    for kind in ("noise", "blob", "ratio"):
        cmp, bg = stack(kind, h, w, seed=4)
        for lo, hi, r_bg, r_fg in SETTINGS:
            want = plain.trimaps(cmp, bg, lo=lo, hi=hi, r_bg=r_bg, r_fg=r_fg)
            assert np.array_equal(ops.trimap_from_plate(dev(cmp), dev(bg), lo, hi, r_bg, r_fg, shadow=None).cpu().numpy(),
                                  want)
            assert np.array_equal(ops.trimap_from_plate(dev(cmp), dev(bg), lo, hi, r_bg, r_fg).cpu().numpy(), want)


def test_captured_call_replays_on_new_inputs():
    from vmatting import ops
    h, w = 70, 90
    d_cmp = torch.zeros((N, h, w, 3), dtype=torch.uint8, device="cuda")
    d_bg = torch.zeros((N, h, w, 3), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((N, h, w), dtype=torch.uint8, device="cuda")
    work = torch.zeros(ops.trimap_from_plate_workspace_bytes(N, h, w), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.trimap_from_plate(d_cmp, d_bg, 8, 30, 1, 1, out=d_out, work=work, shadow={})
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.trimap_from_plate(d_cmp, d_bg, 8, 30, 1, 1, out=d_out, work=work, shadow={})
    for seed, kind in ((1, "ratio"), (2, "noise")):
        cmp, bg = stack(kind, h, w, seed)
        d_cmp.copy_(dev(cmp))
        d_bg.copy_(dev(bg))
        d_out.zero_()
        g.replay()
        assert np.array_equal(d_out.cpu().numpy(), ref.trimaps(cmp, bg, lo=8, hi=30, r_bg=1, r_fg=1, shadow={}))


def test_invalid_arguments():
    from vmatting import _lib, ops
    lib = _lib.lib()
    n, h, w = 2, 8, 12
    cmp = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    bg = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((n, h, w), 7, dtype=torch.uint8, device="cuda")
    work = torch.zeros(ops.trimap_from_plate_workspace_bytes(n, h, w) + 16, dtype=torch.uint8, device="cuda")
    ok = dict(cmp=cmp.data_ptr(), bg=bg.data_ptr(), nb=n, n=n, h=h, w=w, lo=16, hi=48, r_bg=4, r_fg=8, floor=128,
              ceil=256, dark=32, out=out.data_ptr(), work=work.data_ptr())
    order = ("cmp", "bg", "nb", "n", "h", "w", "lo", "hi", "r_bg", "r_fg", "floor", "ceil", "dark", "out", "work")
    bad = [dict(floor=0), dict(floor=257), dict(ceil=255), dict(ceil=513), dict(dark=-1), dict(dark=256), dict(cmp=None),
           dict(work=None), dict(nb=3), dict(lo=48), dict(r_fg=33), dict(out=cmp.data_ptr()),
           dict(work=work.data_ptr() + 8)]
    for change in bad:
        args = dict(ok, **change)
        assert lib.vm_trimap_from_plate_shadow(*[args[k] for k in order], None) == _lib.VM_EINVAL, change
    torch.cuda.synchronize()
    assert (out == 7).all()
    assert lib.vm_trimap_from_plate_shadow(*[ok[k] for k in order], None) == _lib.VM_OK
    torch.cuda.synchronize()
    assert (out == 0).all()                                   # frame == plate: background everywhere
    with pytest.raises(ValueError, match="out must not alias cmp or bg"):
        ops.trimap_from_plate(cmp, bg, out=cmp.view(-1)[:n * h * w].view(n, h, w), shadow={})
    with pytest.raises(ValueError):
        ops.trimap_from_plate(cmp, bg, shadow={"ceil": 600})
