"""The trimap from the background plate on the GPU: ops.trimap_from_plate against the numpy restatement
(tests/trimap_plate_ref.py), byte for byte, and FrameStream(trimap="auto") against FrameStream(trimap=True) fed the
restatement's trimaps, bit for bit."""

import numpy as np
import pytest
import torch

import trimap_plate_ref as ref
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

# 133 x 261: 2 x 9 candidate tiles and 3 x 5 erosion tiles per frame, ragged in both axes, 5 words per row; 40 x 200: a
# row of 4 words whose last is ragged; 70 x 90 and the two one-pixel-wide shapes: a row shorter than any tile
SHAPES = [(70, 90), (133, 261), (40, 200), (1, 17), (19, 1)]
RADII = [(0, 0), (1, 3), (8, 2), (0, 32), (32, 32)]          # (r_bg, r_fg)
LEVELS = [(0, 1), (16, 48), (441, 442)]                      # (lo, hi)
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


def expected(D, lo, hi, r_bg, r_fg):
    """ref.trimap from the box sums D [n,h,w] (computed once per input)."""
    out = np.full(D.shape, 128, np.uint8)
    for i in range(len(D)):
        out[i][ref.erode(D[i] <= 9 * lo * lo, r_bg)] = 0
        out[i][ref.erode(D[i] >= 9 * hi * hi, r_fg)] = 255
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_equals_the_restatement(shape):
    from vmatting import ops
    h, w = shape
    nwork = ops.trimap_from_plate_workspace_bytes(N, h, w)
    assert nwork == N * h * ((w + 63) // 64) * 16
    labels = set()
    for kind in ref.PAIRS:
        cmp, bgs = stack(kind, h, w, seed=11)
        d_cmp = dev(cmp)
        for bg in (bgs, bgs[:1]):                             # nb = 3 and nb = 1
            d_bg = dev(bg)
            D = np.stack([ref.box_sum(cmp[i], bg[i if len(bg) > 1 else 0]) for i in range(N)])
            for lo, hi in LEVELS:
                for r_bg, r_fg in RADII:
                    obuf, out = guarded(N * h * w, 0xA5)
                    wbuf, work = guarded(nwork, 0x5A)
                    got = ops.trimap_from_plate(d_cmp, d_bg, lo, hi, r_bg, r_fg, out=out.view(N, h, w), work=work)
                    assert got.data_ptr() == out.data_ptr()
                    want = expected(D, lo, hi, r_bg, r_fg)
                    case = (kind, len(bg), lo, hi, r_bg, r_fg)
                    assert np.array_equal(got.cpu().numpy(), want), case
                    assert intact(obuf, N * h * w, 0xA5) and intact(wbuf, nwork, 0x5A), case
                    labels |= set(np.unique(want).tolist())
            assert np.array_equal(d_bg.cpu().numpy(), bg)
        assert np.array_equal(d_cmp.cpu().numpy(), cmp)
    assert labels == {0, 128, 255}
    # the restatement itself, through its own entry, once
    cmp, bgs = stack("blob", h, w, seed=11)
    assert np.array_equal(ops.trimap_from_plate(dev(cmp), dev(bgs), 16, 48, 1, 3).cpu().numpy(),
                          ref.trimaps(cmp, bgs, lo=16, hi=48, r_bg=1, r_fg=3))


def test_planes_off_four_bytes_are_read_bytewise():
    """cmp and bg that do not start on 4 bytes take the bytewise loads: the same bytes."""
    from vmatting import ops
    h, w = 70, 90
    cmp, bg = stack("blob", h, w, seed=5)
    want = ref.trimaps(cmp, bg[0], **ref.DEFAULTS)
    for lead_c, lead_b in ((1, 0), (0, 3), (2, 2)):
        _, c = guarded(cmp.size, 0, lead=lead_c)
        _, b = guarded(bg[0].size, 0, lead=lead_b)
        c.copy_(dev(cmp).view(-1))
        b.copy_(dev(bg[0]).view(-1))
        assert c.data_ptr() % 4 == lead_c and b.data_ptr() % 4 == lead_b
        got = ops.trimap_from_plate(c.view(N, h, w, 3), b.view(h, w, 3))
        assert np.array_equal(got.cpu().numpy(), want), (lead_c, lead_b)


def test_unaligned_output_and_allocated_buffers():
    """An output that does not start on 16 bytes is stored bytewise, nothing before or behind it is touched; the call
    allocates what it is not given; reader.trimap_from_plate returns what it was given."""
    from vmatting import ops, reader
    h, w = 133, 261
    cmp, bg = stack("blob", h, w, seed=2)
    want = ref.trimaps(cmp, bg, **ref.DEFAULTS)
    assert set(np.unique(want).tolist()) == {0, 128, 255}
    obuf, out = guarded(N * h * w, 0xA5, lead=3)
    assert out.data_ptr() % 16 == 3
    got = ops.trimap_from_plate(dev(cmp), dev(bg), out=out.view(N, h, w))
    assert np.array_equal(got.cpu().numpy(), want) and intact(obuf, N * h * w, 0xA5, lead=3)
    got = ops.trimap_from_plate(dev(cmp), dev(bg))
    assert got.shape == (N, h, w) and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    # reader.trimap_from_plate: numpy in, numpy out; device tensors stay on the device; one frame or a stack
    got = reader.trimap_from_plate(cmp, bg)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    got = reader.trimap_from_plate(dev(cmp), dev(bg))
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    got = reader.trimap_from_plate(cmp[1], bg[1])
    assert got.shape == (h, w) and np.array_equal(got, want[1])
    got = reader.trimap_from_plate(dev(cmp[1]), dev(bg[1]), lo=8, hi=30, r_bg=1, r_fg=2)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), ref.trimap(cmp[1], bg[1], 8, 30, 1, 2))
    got = reader.trimap_from_plate(cmp, bg[0])                # a stack over one plate
    assert np.array_equal(got, ref.trimaps(cmp, bg[0], **ref.DEFAULTS))


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
        ops.trimap_from_plate(d_cmp, d_bg, out=d_out, work=work)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.trimap_from_plate(d_cmp, d_bg, out=d_out, work=work)
    for seed, kind in ((1, "blob"), (2, "noise")):
        cmp, bg = stack(kind, h, w, seed)
        d_cmp.copy_(dev(cmp))
        d_bg.copy_(dev(bg))
        eager = ops.trimap_from_plate(d_cmp, d_bg).cpu().numpy()
        assert np.array_equal(eager, ref.trimaps(cmp, bg, **ref.DEFAULTS))
        for _ in range(2):
            d_out.zero_()
            g.replay()
            assert np.array_equal(d_out.cpu().numpy(), eager)


def test_invalid_arguments():
    from vmatting import _lib, ops
    lib = _lib.lib()
    n, h, w = 2, 8, 12
    cmp = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    bg = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    work = torch.zeros(ops.trimap_from_plate_workspace_bytes(n, h, w) + 16, dtype=torch.uint8, device="cuda")
    ok = dict(cmp=cmp.data_ptr(), bg=bg.data_ptr(), nb=n, n=n, h=h, w=w, lo=16, hi=48, r_bg=4, r_fg=8,
              out=out.data_ptr(), work=work.data_ptr())
    order = ("cmp", "bg", "nb", "n", "h", "w", "lo", "hi", "r_bg", "r_fg", "out", "work")
    assert lib.vm_trimap_from_plate(*[ok[k] for k in order], None) == _lib.VM_OK
    bad = [dict(cmp=None), dict(bg=None), dict(out=None), dict(work=None), dict(n=0), dict(h=0), dict(w=0),
           dict(nb=0), dict(nb=3), dict(lo=-1), dict(lo=48), dict(hi=443), dict(r_bg=33), dict(r_fg=33), dict(r_bg=-1),
           dict(r_fg=-1), dict(out=cmp.data_ptr()), dict(out=bg.data_ptr() + 16), dict(work=work.data_ptr() + 8)]
    for change in bad:
        args = dict(ok, **change)
        assert lib.vm_trimap_from_plate(*[args[k] for k in order], None) == _lib.VM_EINVAL, change
    assert (out == 0).all()
    for shape in ((0, h, w), (n, 0, w), (n, h, 0), (1 << 15, 1 << 8, 1 << 8)):
        assert lib.vm_trimap_from_plate_workspace_bytes(*shape) == 0
    with pytest.raises(ValueError, match="trimap_from_plate: trimap_from_plate: out must not alias cmp or bg"):
        ops.trimap_from_plate(cmp, bg, out=cmp.view(-1)[:n * h * w].view(n, h, w))
    with pytest.raises(ValueError):
        ops.trimap_from_plate(cmp, bg, out=torch.zeros((n, h, 11), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ops.trimap_from_plate(cmp, bg, work=torch.zeros(8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ops.trimap_from_plate(cmp.permute(0, 2, 1, 3), bg.permute(0, 2, 1, 3))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- FrameStream(trimap="auto")

H, W, F, CHUNK = 70, 90, 7, 3    # items of 3, 3 and 1 frames: two full chunks and a short, eager one
AUTO = {"lo": 12, "hi": 40, "r_bg": 2, "r_fg": 3}


def items(cmp, bg, tris=None, new_bg=None):
    """The clip in chunks: (cmp, bg | None, the per-frame trimaps | None) and new_bg after them when given."""
    for a in range(0, len(cmp), CHUNK):
        b = min(a + CHUNK, len(cmp))
        item = (cmp[a:b], None if bg is None else bg[a:b], None if tris is None else tris[a:b])
        yield item if new_bg is None else item + (new_bg[a:b],)


@pytest.fixture(scope="module")
def clip(vgg0):
    """7 frames of a disc over per-frame plates, the bf16 model, and the restatement's trimaps over the per-frame plates
    and over plate 0 alone."""
    from vmatting import unet
    pairs = [ref.blob_pair(H, W, seed=30 + t) for t in range(F)]
    cmp, bg = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    new_bg = np.random.RandomState(3).randint(0, 256, (F, H, W, 3)).astype(np.uint8)
    np.random.seed(0)
    model = unet.UNetVideo(vgg0, dtype="bf16", device="cuda").prepare()
    tris = {"frames": ref.trimaps(cmp, bg, **AUTO), "static": ref.trimaps(cmp, bg[0], **AUTO)}
    for t in tris.values():
        assert all(set(np.unique(t[i]).tolist()) == {0, 128, 255} for i in range(F))
        assert len({t[i].tobytes() for i in range(F)}) == F
    return model, cmp, bg, new_bg, tris


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("plate", ["frames", "static"])
def test_stream_auto_equals_per_frame_trimaps(clip, plate, graph):
    from vmatting import FrameStream
    model, cmp, bg, _, tris = clip
    static = bg[0] if plate == "static" else None
    feed = None if plate == "static" else bg
    want = np.concatenate(list(FrameStream(model, H, W, chunk=CHUNK, out="u16", static_bg=static)
                               .run(items(cmp, feed, tris[plate]))))
    assert len({want[t].tobytes() for t in range(F)}) == F
    fs = FrameStream(model, H, W, chunk=CHUNK, trimap="auto", auto_options=AUTO, out="u16", static_bg=static, graph=graph)
    for _ in range(2):  # the object runs again with the same result
        got = list(fs.run(items(cmp, feed)))
        assert [g.shape for g in got] == [(3, H, W), (3, H, W), (1, H, W)]
        assert np.array_equal(np.concatenate(got), want)
    assert fs.overflowed_chunks == []
    assert all((s.graph is not None) == graph and s.h_tri is None and s.d_tri is not None for s in fs._slots)
    # what the stream fed the model is what reader.trimap_from_plate shows
    from vmatting import reader
    assert np.array_equal(reader.trimap_from_plate(cmp, bg if static is None else static, **AUTO), tris[plate])


def test_stream_auto_over_a_new_plate(clip):
    from vmatting import FrameStream
    model, cmp, bg, new_bg, tris = clip
    kw = dict(chunk=CHUNK, out="over", new_bg="per_frame")
    want = np.concatenate(list(FrameStream(model, H, W, **kw).run(items(cmp, bg, tris["frames"], new_bg))))
    got = np.concatenate(list(FrameStream(model, H, W, trimap="auto", auto_options=AUTO, **kw)
                              .run(items(cmp, bg, None, new_bg))))
    assert got.shape == (F, H, W, 3) and np.array_equal(got, want)


def test_stream_auto_defaults_differ_from_the_options(clip):
    """auto_options reach the kernel: the defaults give other trimaps on these frames, and other mattes."""
    from vmatting import FrameStream
    model, cmp, bg, _, tris = clip
    tri = ref.trimaps(cmp, bg, **ref.DEFAULTS)
    assert not np.array_equal(tri, tris["frames"])
    want = np.concatenate(list(FrameStream(model, H, W, chunk=CHUNK, out="u16").run(items(cmp, bg, tri))))
    got = np.concatenate(list(FrameStream(model, H, W, chunk=CHUNK, trimap="auto", out="u16").run(items(cmp, bg))))
    assert np.array_equal(got, want)
