"""vm_matte_compose (csrc/ingest.hip) on the GPU, bit for bit against its numpy restatement (tests/compose_ref.py):
every byte, no tolerance; then reader.estimate_foreground / replace_background, and out="over" / "bgra" / "premul" of
FrameStream and ClipStream against the restatement applied to the alphas the same models yield as f32."""

import numpy as np
import pytest
import torch

import compose_ref as cr
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
SENTINEL, PAD = 0xC3, 64  # (64 bytes of padding keep a 16-byte aligned output aligned)

# (1,1,1); hw % 4 == 0; hw = 35: a broadcast plate's group straddles its end, total 105: a tail of 1; n = 1 with
# nb = 1: not a broadcast; hw = 189, total 567: room for every special alpha, a tail of 3
SHAPES = [(1, 1, 1), (2, 4, 6), (3, 5, 7), (1, 3, 5), (3, 9, 21)]
CHANNELS = {"over": 3, "bgra": 4, "premul": 4}


def make_alpha(rs, shape):
    """Random alphas in [0,1] with the special values among them: all of them where they fit, else a random draw."""
    total = int(np.prod(shape))
    alpha = rs.uniform(0.0, 1.0, total).astype(np.float32)
    special = cr.special_alphas()
    if total >= 2 * special.size:
        alpha[rs.permutation(total)[:special.size]] = special
    else:
        where = rs.permutation(total)[:(total + 1) // 2]
        alpha[where] = special[rs.randint(0, special.size, where.size)]
    return alpha.reshape(shape)


def planes(rs, kind, shape):
    """cmp, bg, new_bg [n,h,w,3]: random, or constant planes at which both clamps of fin fire."""
    if kind == "random":
        return tuple(rs.randint(0, 256, shape + (3,)).astype(np.uint8) for _ in range(3))
    lo, hi = np.zeros(shape + (3,), np.uint8), np.full(shape + (3,), 255, np.uint8)
    return (lo, hi, lo) if kind == "low" else (hi, lo, hi)  # c + (1 - a)(nw - b): 0 - 255(1 - a) | 255 + 255(1 - a)


def run_kernel(alpha, cmp, bg, new_bg, mode, offset=()):
    """ops.matte_compose into the middle of a sentinel-filled buffer; ``offset``: the operands taken as 1-element-offset
    slices of larger buffers (unaligned for the 4-pixel form).  Returns the output; the sentinels are checked."""
    from vmatting import ops

    def dev(name, a):
        if a is None:
            return None
        flat = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
        if name in offset:
            buf = torch.empty(flat.numel() + 1, dtype=flat.dtype, device="cuda")
            buf[1:].copy_(flat)
            t = buf[1:].view(a.shape)
            assert t.data_ptr() % (16 if name == "alpha" else 4) != 0 and t.is_contiguous()
            return t
        return flat.cuda().view(a.shape)
    n, h, w = alpha.shape
    size = n * h * w * CHANNELS[mode]
    shift = 1 if "out" in offset else 0
    buf = torch.full((PAD + shift + size + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = buf[PAD + shift:PAD + shift + size].view(n, h, w, CHANNELS[mode])
    assert (out.data_ptr() % 4 != 0) == bool(shift)
    got = ops.matte_compose(dev("alpha", alpha), dev("cmp", cmp), dev("bg", bg), dev("new_bg", new_bg), mode=mode, out=out)
    assert got is out
    host = buf.cpu().numpy()
    assert (host[:PAD + shift] == SENTINEL).all() and (host[PAD + shift + size:] == SENTINEL).all(), "wrote out of bounds"
    return host[PAD + shift:PAD + shift + size].reshape(n, h, w, CHANNELS[mode])


def plate_choices(mode, bg, nw):
    """Every combination of a per-frame or static original plate and, for "over", a per-frame or static new plate
    (static: frame 0's, as [h,w,3] and as [1,h,w,3])."""
    for b in (bg, bg[0], bg[:1]):
        if mode != "over":
            yield b, None
        else:
            for v in (nw, nw[0], nw[:1]):
                yield b, v


@pytest.mark.parametrize("mode", cr.MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_kernel_equals_restatement_bit_for_bit(shape, mode):
    rs = np.random.RandomState(sum(shape) * 7 + len(mode))
    alpha = make_alpha(rs, shape)
    for kind in ("random", "low", "high"):
        cmp, bg, nw = planes(rs, kind, shape)
        for b, v in plate_choices(mode, bg, nw):
            want = cr.compose(alpha, cmp, b, v, mode)
            got = run_kernel(alpha, cmp, b, v, mode)
            assert np.array_equal(got, want), (kind, b.shape, None if v is None else v.shape,
                                               int((got != want).sum()), "bytes differ")


def test_special_alphas_reach_the_kernel():
    """The 3x9x21 case holds every special alpha (so every rounding tie of the 8-bit matte is compared)."""
    alpha = make_alpha(np.random.RandomState(sum(SHAPES[-1]) * 7 + 4), SHAPES[-1])
    special = cr.special_alphas()
    have = set(alpha.reshape(-1).view(np.uint32).tolist())
    assert all(int(s.view(np.uint32)) in have for s in special) and np.isnan(alpha).sum() == 1
    q = run_kernel(alpha, *planes(np.random.RandomState(0), "random", SHAPES[-1])[:2], None, "bgra")[..., 3]
    from vmatting import ops
    assert np.array_equal(q, ops.matte_quantize(T(alpha)).cpu().numpy())  # the layer's alpha is vm_matte_quantize's


@pytest.mark.parametrize("mode", cr.MODES)
@pytest.mark.parametrize("shape", [(2, 4, 6), (3, 5, 7)], ids=lambda s: "%dx%dx%d" % s)
def test_unaligned_operands_take_the_scalar_form(shape, mode):
    rs = np.random.RandomState(5)
    alpha = make_alpha(rs, shape)
    cmp, bg, nw = planes(rs, "random", shape)
    names = ("alpha", "cmp", "bg", "out") + (("new_bg",) if mode == "over" else ())
    for b, v in ((bg, nw), (bg[0], nw[0])):
        v = v if mode == "over" else None
        want = cr.compose(alpha, cmp, b, v, mode)
        for offset in [(name,) for name in names] + [names]:
            got = run_kernel(alpha, cmp, b, v, mode, offset)
            assert np.array_equal(got, want), (offset, b.shape)


# more than one pass of the launcher's grid (256 * 32 blocks of 256 threads, 4 pixels each = 8 388 608 pixels), with an
# odd hw (a static plate's groups straddle its end in every pass) and a tail of 2
BIG = (2, 1449, 2897)


@pytest.mark.parametrize("mode,static_bg,static_nw", [("over", True, False), ("bgra", False, None),
                                                      ("premul", True, None)])
def test_more_than_one_grid_pass(mode, static_bg, static_nw):
    n, h, w = BIG
    assert n * h * w > 256 * 32 * 256 * 4 and (h * w) % 4 and (n * h * w) % 4
    rs = np.random.RandomState(3)
    alpha = rs.uniform(0.0, 1.0, BIG).astype(np.float32)
    special = cr.special_alphas()
    alpha.reshape(-1)[-special.size:] = special  # (in the second pass and the tail)
    cmp = rs.randint(0, 256, BIG + (3,), dtype=np.uint8)
    bg = rs.randint(0, 256, ((1,) if static_bg else (n,)) + (h, w, 3), dtype=np.uint8)
    nw = None if mode != "over" else rs.randint(0, 256, ((1,) if static_nw else (n,)) + (h, w, 3), dtype=np.uint8)
    got = run_kernel(alpha, cmp, bg, nw, mode)
    for i in range(n):  # frame by frame: the float64 temporaries of the restatement stay small
        want = cr.compose(alpha[i:i + 1], cmp[i:i + 1], bg[0 if static_bg else i][None],
                          None if nw is None else nw[0 if static_nw else i][None], mode)
        assert np.array_equal(got[i:i + 1], want), "frame %d" % i


# ---------------------------------------------------------------------------------------------- reader
def test_reader_estimate_foreground_and_replace_background():
    from vmatting import reader
    rs = np.random.RandomState(9)
    h, w = 24, 40
    alpha = make_alpha(rs, (1, h, w))
    cmp, bg, nw = planes(rs, "random", (1, h, w))
    for a in (alpha[0], alpha[0].astype(np.float64)):  # f64 is rounded to f32 first (here: exactly)
        assert np.array_equal(reader.estimate_foreground(cmp[0], bg[0], a), cr.compose(alpha, cmp, bg, mode="bgra")[0])
        assert np.array_equal(reader.estimate_foreground(cmp[0], bg[0], a, premultiplied=True),
                              cr.compose(alpha, cmp, bg, mode="premul")[0])
        assert np.array_equal(reader.replace_background(cmp[0], bg[0], a, nw[0]),
                              cr.compose(alpha, cmp, bg, nw, "over")[0])
    a64 = rs.uniform(0.0, 1.0, (h, w))  # not representable in f32
    assert np.array_equal(reader.replace_background(cmp[0], bg[0], a64, nw[0]),
                          cr.compose(a64.astype(np.float32)[None], cmp, bg, nw, "over")[0])
    with pytest.raises(TypeError):
        reader.estimate_foreground(cmp[0].astype(np.float32), bg[0], alpha[0])
    with pytest.raises(ValueError):
        reader.replace_background(cmp[0], bg[0], alpha[0], nw[0, :3])


# ---------------------------------------------------------------------------------------------- FrameStream
VGG_MEAN = np.array([103.939, 116.779, 123.68], np.float64)
H, W, F, CHUNK = 24, 40, 19, 8  # tests/test_gpu_stream.py's shape: chunks of 8, 8 and 3 (the last one runs eagerly)


def feed(cmp, bg, tri):
    return np.concatenate([(cmp.astype(np.float64) - VGG_MEAN).astype(np.float32),
                           (bg.astype(np.float64) - VGG_MEAN).astype(np.float32),
                           (tri.astype(np.float64) / 255.0 - 0.5).astype(np.float32)[..., None]], -1)


def reusing_source(cmp, bg, tri, nw, chunk):
    """Yields the clip in chunks out of ONE set of arrays that it overwrites after every yield (a decoder's ring);
    bg None: a static plate; nw None: no per-frame new plate (items of three)."""
    n = cmp.shape[0]
    bc, bb, bt, bn = (np.empty_like(a[:chunk]) for a in (cmp, cmp, tri, cmp))
    for a in range(0, n, chunk):
        k = min(chunk, n - a)
        bc[:k], bt[:k] = cmp[a:a + k], tri[a:a + k]
        if bg is not None:
            bb[:k] = bg[a:a + k]
        if nw is not None:
            bn[:k] = nw[a:a + k]
        yield (bc[:k], (None if bg is None else bb[:k]), bt[:k]) + (() if nw is None else (bn[:k],))
        bc[...], bb[...], bt[...], bn[...] = 0xA5, 0x5A, 0x33, 0x99


@pytest.fixture(scope="module")
def frames(vgg0):
    """19 distinct frames, the bf16 model, and model.forward of every numpy-built frame on its own (computed once),
    with the per-frame backgrounds and with frame 3's as a static plate."""
    from vmatting import unet
    rs = np.random.RandomState(42)
    cmp, bg, nw = (rs.randint(0, 256, (F, H, W, 3)).astype(np.uint8) for _ in range(3))
    tri = rs.choice(np.array([0, 128, 255], np.uint8), (F, H, W))
    np.random.seed(0)
    model = unet.UNetVideo(vgg0, dtype="bf16", device="cuda")
    # the synthetic weights' logits saturate the sigmoid (0.3 % of the pixels end up partly transparent, and a layer
    # of 0 / 255 mattes is trivial): the output conv scaled by 2^-8 (exact) leaves most of the matte in between
    model.params = model._make_params()
    w15, b15 = model.params["conv1_5"]
    model.load_params(dict(model.params, conv1_5=(w15 * np.float32(2.0 ** -8), b15 * np.float32(2.0 ** -8)))).prepare()

    def reference(bgs):
        x = feed(cmp, bgs, tri)
        return np.stack([model.forward(torch.from_numpy(x[i:i + 1]).cuda())[0, :, :, 0].cpu().numpy() for i in range(F)])
    alpha = reference(bg)
    assert len({alpha[i].tobytes() for i in range(F)}) == F  # distinct mattes: a swapped or stale frame would show
    q = cr.quantize8(alpha)
    print("partly transparent pixels: %.1f %%, %d distinct 8-bit levels" % (100.0 * ((q > 0) & (q < 255)).mean(),
                                                                       np.unique(q).size))
    assert ((q > 0) & (q < 255)).mean() > 0.5 and np.unique(q).size >= 16  # the layers are not trivial
    return dict(model=model, cmp=cmp, bg=bg, nw=nw, tri=tri, alpha=alpha,
                alpha_plate=reference(np.broadcast_to(bg[3], bg.shape)))


def stream_case(f, out, plate):
    """(FrameStream keywords, the source's new plates, the expected frames) of one new ``out``."""
    kw, nw = dict(out=out), None
    if out == "over":
        kw["new_bg"], nw = ("per_frame", f["nw"]) if plate == "per_frame" else (f["nw"][5], None)
    want = cr.compose(f["alpha"], f["cmp"], f["bg"], None if out != "over" else f["nw"] if nw is not None else f["nw"][5],
                      out)
    return kw, nw, want


CASES = [("over", "static"), ("over", "per_frame"), ("bgra", None), ("premul", None)]


@pytest.mark.parametrize("out,plate", CASES)
def test_frame_stream_composes_frame_by_frame(frames, out, plate):
    from vmatting import FrameStream
    f = frames
    kw, nw, want = stream_case(f, out, plate)
    fs = FrameStream(f["model"], H, W, chunk=CHUNK, depth=2, **kw)
    for _ in range(2):  # twice in a row on one object (the slots' graphs are reused)
        got = list(fs.run(reusing_source(f["cmp"], f["bg"], f["tri"], nw, CHUNK)))
        assert [g.shape for g in got] == [(k, H, W, CHANNELS[out]) for k in (8, 8, 3)]
        assert all(g.dtype == np.uint8 for g in got)
        got = np.concatenate(got)
        for i in range(F):  # in order, frame by frame
            assert np.array_equal(got[i], want[i]), "frame %d" % i
    assert sum(s.graph is not None for s in fs._slots) == 2
    if out != "over":  # the mattes in the BGRA alpha channel are what out="u8" yields
        u8 = np.concatenate(list(FrameStream(f["model"], H, W, chunk=CHUNK, out="u8").run(
            reusing_source(f["cmp"], f["bg"], f["tri"], None, CHUNK))))
        assert np.array_equal(got[..., 3], u8)


@pytest.mark.parametrize("depth,graph", [(1, True), (3, True), (2, False)])
@pytest.mark.parametrize("out,plate", CASES[:3])
def test_frame_stream_depths_and_eager_compose_the_same(frames, out, plate, depth, graph):
    from vmatting import FrameStream
    f = frames
    kw, nw, want = stream_case(f, out, plate)
    fs = FrameStream(f["model"], H, W, chunk=CHUNK, depth=depth, graph=graph, **kw)
    got = np.concatenate(list(fs.run(reusing_source(f["cmp"], f["bg"], f["tri"], nw, CHUNK))))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("out", ["over", "premul"])
def test_frame_stream_composes_with_a_static_original_plate(frames, out):
    from vmatting import FrameStream
    f = frames
    kw = dict(new_bg=f["nw"][5]) if out == "over" else {}
    want = cr.compose(f["alpha_plate"], f["cmp"], f["bg"][3], kw.get("new_bg"), out)
    fs = FrameStream(f["model"], H, W, chunk=CHUNK, static_bg=f["bg"][3], out=out, **kw)
    got = np.concatenate(list(fs.run(reusing_source(f["cmp"], None, f["tri"], None, CHUNK))))
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------- ClipStream
FC = 5  # frames of the clip (tests/test_gpu_clip_stream.py's shape: 24 x 40, 5 frames)


@pytest.fixture(scope="module")
def clip(vgg0):
    """A 5-frame clip, the bf16 video model on the oracle's parameters (output conv scaled by 2^-6: no saturated
    sigmoid), and the f32 alphas of an out="f32" run per original-plate mode (computed on demand, once)."""
    from oracle import flow as oflow
    from oracle import models as om
    from vmatting import ClipStream, unet_simple
    rs = np.random.RandomState(42)
    c = dict(cmp=rs.randint(0, 256, (FC, H, W, 3)).astype(np.uint8), bg=rs.randint(0, 256, (FC, H, W, 3)).astype(np.uint8),
             nw=rs.randint(0, 256, (FC, H, W, 3)).astype(np.uint8),
             bw=np.stack([oflow.smooth_flow(H, W, seed=100 + t, amp=6.0) for t in range(FC)]),
             alpha0=rs.uniform(0.0, 1.0, (H, W)).astype(np.float32))
    p = om.unet_simple_params(np.random.RandomState(1))
    w, b = p["output"]
    p["output"] = (w * np.float32(2.0 ** -6), b * np.float32(2.0 ** -6))
    bn = {"conv4": (rs.uniform(0.5, 1.5, 48).astype(np.float32), rs.normal(size=48).astype(np.float32) * 0.1),
          "upconv2": (rs.uniform(0.5, 1.5, 32).astype(np.float32), rs.normal(size=32).astype(np.float32) * 0.1)}
    np.random.seed(0)
    c["model"] = unet_simple.UNetSimple(unet_simple.Vgg16(vgg0, "bf16"), False, "bf16").load_params(p, bn)

    def source(plate, per_frame_nw):
        """One set of arrays, overwritten after every yield (a decoder's ring)."""
        cm, b_, bw_, n_ = (np.empty_like(a[0]) for a in (c["cmp"], c["bg"], c["bw"], c["nw"]))
        for t in range(FC):
            cm[...], b_[...], bw_[...], n_[...] = c["cmp"][t], c["bg"][t], c["bw"][t], c["nw"][t]
            yield (cm, (None if plate else b_), bw_, None) + ((n_,) if per_frame_nw else ())
            cm[...], b_[...], bw_[...], n_[...] = 0xA5, 0x5A, 1e3, 0x99

    def run(plate, per_frame_nw=False, **kw):
        cs = ClipStream(c["model"], H, W, static_bg=c["bg"][2] if plate else None, **kw)
        return np.stack(list(cs.run(source(plate, per_frame_nw), c["alpha0"])))
    f32 = {}

    def alphas(plate, **kw):
        key = (plate,) + tuple(sorted(kw.items()))
        if key not in f32:
            f32[key] = run(plate, out="f32", **kw)
            a = f32[key]
            assert (a > 0.01).all() and (a < 0.99).all() and len({a[i].tobytes() for i in range(FC)}) == FC
        return f32[key]
    c["run"], c["alphas"] = run, alphas
    return c


@pytest.mark.parametrize("reuse", [True, False], ids=["reuse", "full"])
@pytest.mark.parametrize("out,plate", CASES[:3])
def test_clip_stream_composes_without_disturbing_the_recurrence(clip, out, plate, reuse):
    c = clip
    want_alpha = c["alphas"](True, reuse_bg_tower=reuse)
    assert np.array_equal(want_alpha, c["alphas"](True, reuse_bg_tower=not reuse))  # (the towers' reuse is exact)
    kw = dict(out=out, reuse_bg_tower=reuse)
    new_bg = None
    if out == "over":
        kw["new_bg"], new_bg = ("per_frame", c["nw"]) if plate == "per_frame" else (c["nw"][1], c["nw"][1])
    got = c["run"](True, per_frame_nw=plate == "per_frame", **kw)
    assert got.shape == (FC, H, W, CHANNELS[out]) and got.dtype == np.uint8
    want = cr.compose(want_alpha, c["cmp"], c["bg"][2], new_bg, out)
    for t in range(FC):
        assert np.array_equal(got[t], want[t]), "frame %d" % t
    if out == "bgra":
        assert np.array_equal(got[..., 3], c["run"](True, out="u8", reuse_bg_tower=reuse))


@pytest.mark.parametrize("depth,graph", [(1, True), (3, False)])
def test_clip_stream_composes_with_per_frame_plates(clip, depth, graph):
    """Per-frame original and new plates, eager and graph: the layers and the frames over the new plates come from
    the f32 recurrence of the same clip."""
    c = clip
    want_alpha = c["alphas"](False)
    got = c["run"](False, per_frame_nw=True, out="over", new_bg="per_frame", depth=depth, graph=graph)
    assert np.array_equal(got, cr.compose(want_alpha, c["cmp"], c["bg"], c["nw"], "over"))
    got = c["run"](False, out="premul", depth=depth, graph=graph)
    assert np.array_equal(got, cr.compose(want_alpha, c["cmp"], c["bg"], mode="premul"))
