"""vm_clip_feed (csrc/flow.hip) on the GPU, bit for bit against the entry points it fuses: the uint8 feed restated in
numpy (loader.py:45,75-78: float64 mean subtraction rounded to f32 once, as tests/test_gpu_ingest.py), then
ops.remap_f32(mode="opencv") [-> ops.fb_consistency] for the third tower and ops.convert into the model's buffers."""

import numpy as np
import pytest
import torch

from conftest import golden, gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

VGG_MEAN = np.array([103.939, 116.779, 123.68], np.float64)
DTYPES = {"bf16": (torch.bfloat16, torch.int16, 0x7B7B), "f32": (torch.float32, torch.int32, 0x7B7B7B7B)}
SHAPES = [(1, 1, 1), (2, 5, 7), (1, 16, 24), (3, 9, 20)]
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731


def feed(u8):
    return (u8.astype(np.float64) - VGG_MEAN).astype(np.float32)


def make_flows(n, h, w, seed, occlusion):
    """Backward (and forward) flows whose targets leave the frame on all four sides by more than its size, with
    exact-integer flows and flows of the form k/64 (rintf(x * 32) on a tie) among them.  With ``occlusion`` the targets
    stay above -dim, where correct_alpha wraps numpy-style instead of raising, and about half the pixels move by less
    than 2 px with a forward flow that nearly closes the round trip."""
    rs = np.random.RandomState(seed)
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    lo = -1.0 if occlusion else -2.0
    tx = rs.uniform(lo * w + 0.5, 2.0 * w, (n, h, w))
    ty = rs.uniform(lo * h + 0.5, 2.0 * h, (n, h, w))
    bw = np.stack([tx - jj, ty - ii], -1)
    near = rs.uniform(size=(n, h, w)) < 0.5
    bw[near] = rs.uniform(-2, 2, (int(near.sum()), 2))
    kind = rs.randint(0, 4, (n, h, w))
    bw[kind == 1] = np.round(bw[kind == 1])                 # exact integers
    bw[kind == 2] = (np.floor(bw[kind == 2] * 32) * 2 + 1) / 64   # odd k / 64: a tie of rintf(x * 32)
    bw = bw.astype(np.float32)
    fw = None
    if occlusion:
        fw = rs.uniform(-30, 30, (n, h, w, 2))
        fw[rs.uniform(size=(n, h, w)) < 0.6] = rs.uniform(-1.5, 1.5, 2)
        fw = fw.astype(np.float32)
    return bw, fw


def clip(n, h, w, seed):
    rs = np.random.RandomState(seed)
    cmp = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    bg = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    prev = rs.uniform(0.05, 1.0, (n, h, w)).astype(np.float32)
    return cmp, bg, prev


def reference(cmp, bg, prev, bw, fw, dtype, thresh=15.0, promote="numpy1"):
    """The unfused route: (tin [3n,h,w,8], in9 [n,h,w,32], warped [n,h,w]) device tensors."""
    from vmatting import ops
    n, h, w = prev.shape
    a = ops.remap_f32(T(prev), T(bw), mode="opencv")
    if fw is not None:
        for i in range(n):
            ops.fb_consistency(T(bw[i]), T(fw[i]), a[i], thresh, promote)
    # (a fresh copy: broadcast_to leaves zero strides on size-1 axes, which ascontiguousarray keeps)
    xs = [T(feed(cmp)), T(np.broadcast_to(feed(bg).reshape((-1, h, w, 3)), (n, h, w, 3)).copy()),
          a[..., None].repeat(1, 1, 1, 3)]
    tin = torch.zeros((3 * n, h, w, 8), dtype=dtype, device="cuda")
    in9 = torch.zeros((n, h, w, 32), dtype=dtype, device="cuda")
    for t in range(3):
        ops.convert(xs[t], tin[t * n:(t + 1) * n])
        ops.convert(xs[t], in9[..., 3 * t:3 * t + 3])
    return tin, in9, a


def odd(a):
    """The array on the device, starting one byte past a 4-byte boundary."""
    raw = torch.zeros(a.size + 1, dtype=torch.uint8, device="cuda")
    raw[1:] = T(a.reshape(-1))
    out = raw[1:].view(a.shape)
    assert out.data_ptr() % 4 == 1
    return out


def run_feed(cmp, bg, prev, bw, fw, dt, thresh=15.0, promote="numpy1", unaligned=False, want_warped=True):
    """ops.clip_feed into sentinel-filled buffers -> (towers bits [3n+2,h,w,8], cat bits [n+2,h,w,32], warped, flag)."""
    from vmatting import ops
    dtype, bits, sent = DTYPES[dt]
    n, h, w = prev.shape
    tb = torch.full((3 * n + 2, h, w, 8), sent, dtype=bits, device="cuda")
    cb = torch.full((n + 2, h, w, 32), sent, dtype=bits, device="cuda")
    towers = tb.view(dtype)[1:3 * n + 1, :, :, :3]
    cat = cb.view(dtype)[1:n + 1, :, :, :9]
    up = odd if unaligned else T
    warped = torch.full((n + 2, h, w), -7.0, device="cuda") if want_warped else None
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.clip_feed(up(cmp), up(bg), T(prev), T(bw), None if fw is None else T(fw), thresh, promote, towers=towers,
                  cat=cat, warped=None if warped is None else warped[1:n + 1], err=flag)
    torch.cuda.synchronize()
    if warped is not None:
        assert (warped[0] == -7.0).all() and (warped[n + 1] == -7.0).all()
        warped = warped[1:n + 1]
    return tb, cb, warped, int(flag.item())


def check_against_reference(tb, cb, warped, ref, dt):
    _, bits, sent = DTYPES[dt]
    tin, in9, a = ref
    n = in9.shape[0]
    assert (tb[0] == sent).all() and (tb[3 * n + 1] == sent).all(), "towers: bytes outside the view were written"
    assert (cb[0] == sent).all() and (cb[n + 1] == sent).all(), "cat: bytes outside the view were written"
    assert (cb[1:n + 1, :, :, 16:] == sent).all(), "cat: channels >= 16 were touched"
    assert (tb[1:3 * n + 1, :, :, 3:] == 0).all() and (cb[1:n + 1, :, :, 9:16] == 0).all()
    assert torch.equal(tb[1:3 * n + 1], tin.view(bits)), "towers differ from the unfused route"
    assert torch.equal(cb[1:n + 1, :, :, :16], in9.view(bits)[..., :16]), "cat differs from the unfused route"
    if warped is not None:
        assert torch.equal(warped.view(torch.int32), a.view(torch.int32)), "warped differs from remap_f32"


def test_flows_cover_borders_integers_and_ties():
    """The flows of the cases below do what the docstring of make_flows says (checked on the host)."""
    for n, h, w in SHAPES[1:]:
        for occ in (False, True):
            bw, _ = make_flows(n, h, w, seed=h * w, occlusion=occ)
            jj, ii = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
            mx, my = (jj + bw[..., 0]) * np.float32(32), (ii + bw[..., 1]) * np.float32(32)
            X, Y = np.rint(mx).astype(np.int64) >> 5, np.rint(my).astype(np.int64) >> 5
            assert (X < -1).any() and (X >= w).any() and (Y < -1).any() and (Y >= h).any()
            assert np.abs(bw[..., 0]).max() > w and np.abs(bw[..., 1]).max() > h
            assert ((mx - np.floor(mx)) == 0.5).sum() >= 3 and ((my - np.floor(my)) == 0.5).sum() >= 3
            assert (bw == np.round(bw)).all(-1).sum() >= 3
            inside = (X >= 0) & (X < w - 1) & (Y >= 0) & (Y < h - 1)
            assert inside.mean() > 0.2


@pytest.mark.parametrize("occ", [None, "numpy1", "numpy2"], ids=["warp", "occ-p0", "occ-p1"])
@pytest.mark.parametrize("static", [False, True], ids=["nb=n", "nb=1"])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_clip_feed_bit_exact(shape, dt, static, occ):
    n, h, w = shape
    cmp, bg, prev = clip(n, h, w, seed=n * h + w)
    if static:
        bg = bg[0]
    bw, fw = make_flows(n, h, w, seed=h * w, occlusion=occ is not None)
    thresh, promote = 4.0, occ or "numpy1"
    ref = reference(cmp, bg, prev, bw, fw, DTYPES[dt][0], thresh, promote)
    if occ is not None and n * h * w >= 35:
        # the mask is neither empty nor full (by the oracle), and it zeroes values the warp alone leaves non-zero
        from oracle import flow as oflow
        frac = np.mean([oflow.correct_alpha(bw[i], fw[i], np.ones((h, w), np.float32), occ, thresh) == 0
                        for i in range(n)])
        assert 0.1 < frac < 0.9, frac
        unmasked = reference(cmp, bg, prev, bw, None, DTYPES[dt][0])[2]
        assert int(((ref[2] == 0) & (unmasked != 0)).sum()) >= 3
    tb, cb, warped, flag = run_feed(cmp, bg, prev, bw, fw, dt, thresh, promote)
    assert flag == 0
    check_against_reference(tb, cb, warped, ref, dt)
    # without the optional warped output: the same buffers
    tb2, cb2, _, _ = run_feed(cmp, bg, prev, bw, fw, dt, thresh, promote, want_warped=False)
    assert torch.equal(tb2, tb) and torch.equal(cb2, cb)


@pytest.mark.parametrize("occ", [None, "numpy1"], ids=["warp", "occ"])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_clip_feed_unaligned_planes(dt, occ):
    """uint8 planes that start at an odd byte (no alignment is required of them): the same values."""
    n, h, w = 3, 9, 20
    cmp, bg, prev = clip(n, h, w, seed=5)
    bw, fw = make_flows(n, h, w, seed=6, occlusion=occ is not None)
    ref = reference(cmp, bg, prev, bw, fw, DTYPES[dt][0], 4.0)
    for plate in (False, True):
        b = bg[1] if plate else bg
        r = reference(cmp, b, prev, bw, fw, DTYPES[dt][0], 4.0) if plate else ref
        tb, cb, warped, flag = run_feed(cmp, b, prev, bw, fw, dt, 4.0, unaligned=True)
        assert flag == 0
        check_against_reference(tb, cb, warped, r, dt)


def test_clip_feed_pixels_not_a_multiple_of_four_with_a_plate():
    """h*w % 4 != 0 with one plate for n frames: the plate's end falls inside a wave, at no 16-byte boundary."""
    n, h, w = 3, 5, 7
    cmp, bg, prev = clip(n, h, w, seed=9)
    bw, _ = make_flows(n, h, w, seed=10, occlusion=False)
    for dt in ("bf16", "f32"):
        tb, cb, warped, _ = run_feed(cmp, bg[2], prev, bw, None, dt)
        check_against_reference(tb, cb, warped, reference(cmp, bg[2], prev, bw, None, DTYPES[dt][0]), dt)


def test_clip_feed_smooth_flow_occlusion_is_not_trivial():
    """The stream tests' flows (smooth_flow at 24x40, amp 6, thresh 6), as one batch of 5 frames: the oracle's mask
    zeroes between 10 % and 90 % of every frame (the default threshold 15 zeroes nothing at this size), and the kernel
    reproduces the unfused route under it."""
    from oracle import flow as oflow
    n, h, w = 5, 24, 40
    cmp, bg, prev = clip(n, h, w, seed=3)
    bw = np.stack([oflow.smooth_flow(h, w, seed=100 + t, amp=6.0) for t in range(n)])
    fw = np.stack([oflow.smooth_flow(h, w, seed=200 + t, amp=6.0) for t in range(n)])
    for t in range(n):
        ones = np.ones((h, w), np.float32)
        frac = (oflow.correct_alpha(bw[t], fw[t], ones.copy(), thresh=6.0) == 0).mean()
        assert 0.1 < frac < 0.9, (t, frac)
        assert (oflow.correct_alpha(bw[t], fw[t], ones.copy(), thresh=15.0) != 0).all()
    for dt in ("bf16", "f32"):
        ref = reference(cmp, bg, prev, bw, fw, DTYPES[dt][0], 6.0)
        for t in range(n):  # the device mask is the oracle's
            want = oflow.correct_alpha(bw[t], fw[t], np.ones((h, w), np.float32), thresh=6.0) == 0
            plain = reference(cmp[t:t + 1], bg[t:t + 1], prev[t:t + 1], bw[t:t + 1], None, DTYPES[dt][0])[2][0]
            got = ((ref[2][t] == 0) & (plain != 0)).cpu().numpy()
            assert np.array_equal(got, want & (plain != 0).cpu().numpy())
        tb, cb, warped, flag = run_feed(cmp, bg, prev, bw, fw, dt, 6.0)
        assert flag == 0
        check_against_reference(tb, cb, warped, ref, dt)


def test_clip_feed_warp_matches_reference_golden():
    """The golden anchor of test_warp_img_matches_reference_golden, through the fused kernel (bound 1e-6 from there)."""
    from oracle import flow as oflow
    g = golden("flow_500x1200")
    h, w = 500, 1200
    fb = oflow.smooth_flow(h, w, seed=int(g["flow_seed_b"]))
    alpha = (g["alpha_u8"] / 255.0).astype(np.float32)
    rs = np.random.RandomState(0)
    cmp = rs.randint(0, 256, (1, h, w, 3)).astype(np.uint8)
    _, _, warped, _ = run_feed(cmp, cmp[0], alpha[None], fb[None], None, "bf16")
    assert np.abs(warped[0].cpu().numpy().astype(np.float64) - g["warped"]).max() <= 1e-6


def test_clip_feed_index_error_flag():
    """The reference's IndexError (flow.py:46): a backward target below -dim sets the flag; it stays 0 otherwise, and
    without a forward flow nothing is checked (warp_img raises nothing)."""
    from vmatting import ops
    h, w = 16, 20
    cmp, bg, prev = clip(1, h, w, seed=1)
    bw = np.zeros((1, h, w, 2), np.float32)
    fw = np.zeros((1, h, w, 2), np.float32)
    assert run_feed(cmp, bg, prev, bw, fw, "bf16")[3] == 0
    bw[0, 3, 4, 1] = -40.0  # i0 = 3 - 40 = -37 < -h
    for dt in ("bf16", "f32"):
        for promote in ("numpy1", "numpy2"):
            assert run_feed(cmp, bg, prev, bw, fw, dt, promote=promote)[3] == 1
        assert run_feed(cmp, bg, prev, bw, None, dt)[3] == 0
    # without a flag of the caller's, the wrapper waits for its own and raises
    tin = torch.zeros((3, h, w, 8), dtype=torch.bfloat16, device="cuda")
    in9 = torch.zeros((1, h, w, 32), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(IndexError):
        ops.clip_feed(T(cmp), T(bg), T(prev), T(bw), T(fw), towers=tin[..., :3], cat=in9[..., :9])
    bw[0, 3, 4, 1] = -19.0  # i0 = -16 = -h: the last index that still wraps
    assert run_feed(cmp, bg, prev, bw, fw, "bf16")[3] == 0
