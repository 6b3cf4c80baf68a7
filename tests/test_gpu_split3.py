"""The split-fp16 x3 forward (vmatting/split3.py, UNetVideo(dtype="f16x3")): unet.py's forward (unet.py:86-217) at f32
accuracy in three fp16 MFMA products per conv (VERDICT r05 "next" item 2: north_star's 1e-4 bound faster than x6).

  split kernel   vm_split3h_nhwc bit-exact against torch's RNE fp16 split, incl. the fused 2x2 SAME pool (odd sizes),
                 an explicit slab width, a concat segment and the overflow flag
  one conv       split input x split filter on the fp16 patch kernel (and split-K) against a float64 conv: within
                 the f32 path's error class
  goldens        the reference-generated goldens (tests/golden/unet_*_70x90.npz): alpha within 1e-4
  1080p          the bench's timed frame and weights: alpha within 1e-4 of the CPU oracle's f32 forward — north_star's
                 bound — and logits within 1e-5 relative
  overflow       frames whose activations leave fp16's range set the flag, and build() re-runs them on bf16x6 — also
                 where the input itself is in range and the overflow starts inside the network, and on a caller's flag
                 slot (the kernels' own values and flags: test_gpu_split3_epilogues.py)
"""

import numpy as np
import pytest
import torch

from conftest import golden, gpu_available
from oracle import models as om
from oracle import ops as oo

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

DEV = "cuda"


def H(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _split_ref(x):
    """x f32 (CPU torch) -> the three slabs [l, h, h] as fp16 (torch's RNE conversion)."""
    h = x.half()
    lo = (x - h.float()).half()
    return [lo, h, h]


@pytest.mark.parametrize("n,h,w,c,S,off,width", [(2, 7, 9, 7, 16, 0, 64), (1, 16, 33, 64, 64, 0, 128),
                                                 (1, 5, 6, 128, 256, 128, 512), (2, 3, 5, 24, 40, 16, 120),
                                                 (1, 9, 17, 64, 64, 0, 192)])
@pytest.mark.parametrize("pool", [False, True])
def test_split3h_kernel_bit_exact(n, h, w, c, S, off, width, pool):
    """slabs [l, h] (and the third, [h] again, where the row holds 3 * S channels: the conv1_1 input's 4 x 16 layout,
    the 3 * 64 case) at p * S + off."""
    from vmatting.split3 import split3h
    torch.manual_seed(c + h)
    x = (torch.randn(n, h, w, c + 3) * torch.logspace(-9, 4, c + 3)).float()
    xd = x.to(DEV)[..., 1:1 + c]  # a channel-slice f32 view
    slab = S
    nsl = 3 if 3 * S <= width else 2
    buf = torch.zeros((n, h, w, width), dtype=torch.float16, device=DEV)
    cc = (c + 7) // 8 * 8
    pb = None
    if pool:
        pb = torch.zeros((n, (h + 1) // 2, (w + 1) // 2, width), dtype=torch.float16, device=DEV)
    ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    split3h(xd, buf[..., off:off + cc], None if pb is None else pb[..., off:off + cc], slab=slab, overflow=ovf)
    torch.cuda.synchronize()
    assert int(ovf.item()) == 0
    xs = x[..., 1:1 + c]
    xp = torch.zeros((n, h, w, cc))
    xp[..., :c] = xs
    got = buf.cpu()
    for p, ref in enumerate(_split_ref(xp)[:nsl]):
        assert torch.equal(got[..., p * S + off:p * S + off + cc].view(torch.int16), ref.view(torch.int16)), p
    assert not got[..., nsl * S:].any()  # past the written slabs: untouched
    # h + l carries x to 2^-22 relative (normal range) / 2^-25 absolute (the fp16 subnormal spacing of l)
    parts = [got[..., p * S + off:p * S + off + c].double() for p in range(2)]
    xd64 = xs.double()
    assert ((parts[0] + parts[1] - xd64).abs() <= 2.0 ** -22 * xd64.abs() + 2.0 ** -25).all()
    if pool:
        ph, pw = (h + 1) // 2, (w + 1) // 2
        xx = torch.full((n, 2 * ph, 2 * pw, cc), -float("inf"))
        xx[:, :h, :w] = xp
        mx = xx.view(n, ph, 2, pw, 2, cc).amax(dim=(2, 4))
        gp = pb.cpu()
        for p, ref in enumerate(_split_ref(mx)[:nsl]):
            assert torch.equal(gp[..., p * S + off:p * S + off + cc].view(torch.int16), ref.view(torch.int16)), p


def test_split3h_overflow_flag():
    from vmatting.split3 import split3h
    x = torch.full((1, 4, 4, 8), 1000.0, device=DEV)
    y = torch.zeros((1, 4, 4, 16), dtype=torch.float16, device=DEV)
    ovf = torch.zeros(1, dtype=torch.int32, device=DEV)
    split3h(x, y[..., :8], overflow=ovf)
    assert int(ovf.item()) == 0
    x[0, 2, 3, 5] = 65520.0  # rounds to inf in fp16
    split3h(x, y[..., :8], overflow=ovf)
    assert int(ovf.item()) == 1
    ovf.zero_()
    x[0, 2, 3, 5] = -7e4
    split3h(x, y[..., :8], overflow=ovf)
    assert int(ovf.item()) == 1


@pytest.mark.parametrize("n,h,w,cin,cout,splitk", [(1, 40, 70, 64, 128, False), (2, 17, 33, 256, 64, True),
                                                   (1, 9, 13, 512, 256, True)])
def test_f16x3_conv_matches_float64(n, h, w, cin, cout, splitk):
    """split input x split filter on the fp16 patch kernel: the conv of the f32 operands to f32-class accuracy."""
    from vmatting import ops
    from vmatting.split3 import filter_scale, split3_filter, split3h
    rs = np.random.RandomState(cin + cout)
    x = (rs.randn(n, h, w, cin) * 300).astype(np.float32)
    wt = (rs.randn(3, 3, cin, cout) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    b = rs.randn(cout).astype(np.float32)
    t = filter_scale(wt)
    pc = ops.PackedConv(split3_filter(wt, cin, cout, t), None, "f16", DEV, scale=np.full(cout, 1.0 / t, np.float32),
                        shift=b)
    xs = torch.zeros((n, h, w, 2 * cin), dtype=torch.float16, device=DEV)  # [l, h], read as [l, h, h]
    split3h(torch.from_numpy(x).to(DEV), xs[..., :cin])
    y = torch.empty((n, h, w, cout), dtype=torch.float32, device=DEV)
    from vmatting.split3 import conv_f32
    conv_f32(xs, pc, y, "none", splitk=splitk)
    torch.cuda.synchronize()
    ref = oo.conv3x3_same(x.astype(np.float64), wt.astype(np.float64), b.astype(np.float64))
    got = H(y)
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max() / scale
    print("f16x3 conv %s: max err %.3e of max |y|" % ((n, h, w, cin, cout), err))
    assert err <= 2e-6  # f32 accumulation over 27 * cin products (the exact-f32 MFMA path: ~1e-6 here)


@pytest.mark.parametrize("n,h,w", [(1, 72, 100), (2, 35, 61)])
def test_f16x3_fused_split_equals_unfused(n, h, w, vgg0):
    """vm_conv3x3_split3_nhwc (split + pool split in the conv epilogue — the patch kernel's staged epilogue, the
    row-stationary kernel's register one, the split-K reduction) and the fused resize + split against the f32 output
    + vm_split3h_nhwc round trip: the same forward, bit for bit."""
    from vmatting import unet
    np.random.seed(0)
    m = unet.UNetVideo(vgg0, dtype="f16x3")
    m.prepare()
    x = torch.randn(n, h, w, 7, device=DEV) * 60
    m._x6.fold_up = False  # (the folded upconvs are another arithmetic: test_f16x3_folded_upconvs_match_...)
    m._x6.fuse_split = False
    a0 = m.forward(x).clone()
    l0 = m.conv1_3.clone()
    m._x6.fuse_split = True
    a1 = m.forward(x).clone()
    torch.cuda.synchronize()
    assert torch.equal(a0, a1)
    assert torch.equal(l0, m.conv1_3)


@pytest.mark.parametrize("n,h,w", [(1, 72, 100), (2, 35, 61), (1, 64, 96)])
def test_f16x3_folded_upconvs_match_the_resize_path(n, h, w, vgg0):
    """The exact-2x upconvs on the folded filter (vm_conv3x3_up2x_split3_nhwc: interior phase filters + the split
    border pass) against resize -> split -> conv: the same forward to f32 accumulation order (logits within 1e-6 of
    their max), on odd sizes (the L2..L4 levels of 35 x 61: 18 x 31 ... where only some upconvs are exact 2x)."""
    from vmatting import unet
    np.random.seed(0)
    m = unet.UNetVideo(vgg0, dtype="f16x3")
    m.prepare()
    x = torch.randn(n, h, w, 7, device=DEV) * 60
    m._x6.fold_up = False
    m.forward(x)
    l0 = H(m.conv1_3)
    m._x6.fold_up = True
    m.forward(x)
    l1 = H(m.conv1_3)
    err = np.abs(l1 - l0).max() / np.abs(l0).max()
    print("folded vs resize path: logits rel %.3e" % err)
    assert err <= 1e-6


@pytest.mark.parametrize("case", ["unet_video_70x90", "unet_video_64x96", "unet_image_70x90"])
def test_unet_f16x3_matches_reference_golden(case, vgg0):
    from vmatting import unet
    g = golden(case)
    cls = unet.UNetVideo if int(g["video"]) else unet.UNetImage
    np.random.seed(int(g["weight_seed"]))
    m = cls(vgg0, dtype="f16x3")
    m.build(g["x"])
    torch.cuda.synchronize()
    assert m.split_mode == "f16x3" and not m.overflowed()
    alpha, logits = H(m.output), H(m.conv1_3)
    err = np.abs(alpha - g["output"]).max()
    print("%s f16x3 alpha max-abs %.3g, logits rel %.3g" % (case, err, np.abs(logits - g["logits"]).max()
                                                              / np.abs(g["logits"]).max()))
    assert err <= 1e-4
    assert np.all(np.abs(logits - g["logits"]) <= 1e-4 * np.abs(g["logits"]).max() + 1e-4)


def test_unet_f16x3_graph_equals_eager(vgg0):
    from vmatting import unet
    np.random.seed(0)
    m = unet.UNetVideo(vgg0, dtype="f16x3")
    m.prepare()
    x = torch.randn(2, 72, 100, 7, device=DEV) * 40
    a = m.forward(x).clone()
    lg = m.conv1_3.clone()
    g = m.capture(x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(g.output, a)
    assert torch.equal(m.conv1_3, lg)


def test_unet_f16x3_overflow_falls_back_to_x6(vgg0):
    """Frames whose activations leave fp16's range: the flag is set, and build() re-runs them on bf16x6 (f32 range),
    whose alpha matches the f64 oracle."""
    from vmatting import unet
    np.random.seed(0)
    m = unet.UNetVideo(vgg0, dtype="f16x3")
    x = np.random.RandomState(3).uniform(-1, 1, (1, 24, 40, 7)).astype(np.float32) * 1e5
    m.prepare()
    m.forward(torch.from_numpy(x).to(DEV))
    assert m.overflowed()
    np.random.seed(0)
    m = unet.UNetVideo(vgg0, dtype="f16x3")
    m.build(x)
    assert m.split_mode == "bf16x6"
    r = om.unet_forward(x, m.params, dtype=np.float64)
    lg = H(m.conv1_3)
    assert np.abs(lg - r["conv1_3"]).max() <= 1e-5 * np.abs(r["conv1_3"]).max()


# the layers of oracle.models.unet_forward whose values the f16x3 forward stores split (conv outputs, pools, the
# [upconv, skip] concats); conv5_2, conv4_4, conv3_4 and conv2_3 stay f32 and reach a split only through their resize
SPLIT_LAYERS = ("conv1_1", "conv1_2", "pool1", "conv2_1", "conv2_2", "pool2", "conv3_1", "conv3_2", "conv3_3", "pool3",
                "conv4_1", "conv4_2", "conv4_3", "pool4", "conv5_1", "upconv1", "upconv2", "upconv3", "upconv4")


def test_unet_f16x3_mid_network_overflow(vgg0):
    """Overflow that starts inside the network: a frame whose input is in fp16's range (so the first split3h raises
    nothing) but whose activations are not — uniform(-1, 1) * 3e4: the float64 oracle puts max |x| at 29999 and the
    largest split activation at 2.8e5 (conv3_1; conv1_1 already 1.6e5), both asserted here.  forward() reports it
    through overflowed(), and build() lands on bf16x6 with logits within 1e-5 of the oracle's max."""
    from vmatting import unet
    x = np.random.RandomState(3).uniform(-1, 1, (1, 24, 40, 7)).astype(np.float32) * np.float32(3e4)
    np.random.seed(0)
    m = unet.UNetVideo(vgg0, dtype="f16x3")
    m.prepare()
    r = om.unet_forward(x, m.params, dtype=np.float64)
    assert np.abs(x).max() < 32760
    assert max(np.abs(r[k]).max() for k in SPLIT_LAYERS) >= 2 * 65520
    m.forward(torch.from_numpy(x).to(DEV))
    assert m.overflowed()
    assert m.split_mode == "f16x3"  # forward() reports, only build() switches
    # a forward on a slot of its own reports there and leaves the model's flag alone
    cool = torch.from_numpy(x / np.float32(250)).to(DEV)
    slot = torch.ones(3, dtype=torch.int32, device=DEV)
    m.forward(cool, overflow=slot[1:2])
    assert slot.tolist() == [1, 0, 1] and m.overflowed()
    m.forward(cool)
    assert not m.overflowed()
    m.forward(torch.from_numpy(x).to(DEV), overflow=slot[1:2])
    assert slot.tolist() == [1, 1, 1] and not m.overflowed()
    np.random.seed(0)
    m = unet.UNetVideo(vgg0, dtype="f16x3")
    m.build(x)
    assert m.split_mode == "bf16x6"
    lg = H(m.conv1_3)
    assert np.isfinite(H(m.output)).all()
    assert np.abs(lg - r["conv1_3"]).max() <= 1e-5 * np.abs(r["conv1_3"]).max()


@pytest.mark.slow
def test_unet_f16x3_1080p_timed_frame_vs_oracle():
    """north_star's bound on the bench's own frame and weights: the f16x3 alpha within 1e-4 max-abs of the CPU
    oracle's float32 forward (the reference's op sequence), where the bf16 path is 0.45 off."""
    from vmatting import unet, video
    from vmatting.weights import synthetic_vgg16
    np.random.seed(0)
    m = unet.UNetVideo(synthetic_vgg16(0), dtype="f16x3")
    m.prepare()
    x = video.synthetic_frames(1, 1080, 1920, first=0, device=DEV)
    alpha = H(m.forward(x))
    assert not m.overflowed()
    logits = H(m.conv1_3)
    r = om.unet_forward(x.cpu().numpy(), m.params, dtype=np.float32)
    err = np.abs(alpha - r["output"]).max()
    lrel = np.abs(logits - r["conv1_3"]).max() / np.abs(r["conv1_3"]).max()
    print("1080p f16x3 alpha max-abs vs oracle %.3e, logits rel %.3e" % (err, lrel))
    assert err <= 1e-4
    assert lrel <= 1e-5


def test_f16x3_fused_head_matches_two_chunk_head(vgg0):
    """conv1_5 in one aliased 12-step MFMA-head call (Split3Forward.head_fused) against the two-call form ([l | h] x
    [Wh | Wl], then [h] x [Wh] adding the first's logits): the same products in another f32 summation order — logits
    within 1e-6 of their max (a 1e-3 logit near alpha 0.5 moves it 2.5e-4; measured 4.7e-6), alpha within 2e-5."""
    from vmatting import split3, unet
    x = torch.from_numpy(np.random.RandomState(5).uniform(-120, 120, (1, 72, 100, 7)).astype(np.float32)).to(DEV)
    outs = []
    for fused in (True, False):
        split3.Split3Forward.head_fused = fused
        try:
            np.random.seed(0)
            m = unet.UNetVideo(vgg0, dtype="f16x3")
            m.build(x)
            torch.cuda.synchronize()
            outs.append((H(m.output), H(m.conv1_3)))
        finally:
            split3.Split3Forward.head_fused = True
    (a0, l0), (a1, l1) = outs
    assert np.abs(l0 - l1).max() <= 1e-6 * np.abs(l1).max()
    assert np.abs(a0 - a1).max() <= 2e-5


# the 19 profiled convs of one split forward at 1x35x61 in walk order (the head runs unprofiled): scope, the rows and
# columns of its input (no level of 35x61 is an exact 2x: every pool is ragged), its concat width, cout
PROFILE_WALK = (("conv1_1", 35, 61, None, 64), ("conv1_2", 35, 61, 64, 64), ("conv2_1", 18, 31, 64, 128),
                ("conv2_2", 18, 31, 128, 128), ("conv3_1", 9, 16, 128, 256), ("conv3_2", 9, 16, 256, 256),
                ("conv3_3", 9, 16, 256, 256), ("conv4_1", 5, 8, 256, 512), ("conv4_2", 5, 8, 512, 512),
                ("conv4_3", 5, 8, 512, 512), ("conv5_1", 3, 4, 512, 512), ("conv5_2", 3, 4, 512, 512),
                ("upconv_1", 5, 8, 512, 512), ("conv4_4", 5, 8, 1024, 512), ("upconv_2", 9, 16, 512, 256),
                ("conv3_4", 9, 16, 512, 256), ("upconv_3", 18, 31, 256, 128), ("conv2_3", 18, 31, 256, 128),
                ("upconv_4", 35, 61, 128, 64))


# (slabs the conv reads per input channel, conv1_1's slab width: f16x3's first_slab 32, bf16x6's 16)
@pytest.mark.parametrize("dtype,slabs,first", [("f16x3", 3, 32), ("bf16x6", 6, 16)])
def test_split_forward_profile_lists_the_walk(dtype, slabs, first, vgg0):
    """conv_profile over one split forward: one (flops, kernel, ev0, ev1, (n, h, w, cin, cout)) entry per conv, in
    the walk's order, cin = the slabs read x the concat width."""
    from vmatting import ops, unet
    np.random.seed(0)
    m = unet.UNetVideo(vgg0, dtype=dtype).prepare()
    x = torch.from_numpy((np.random.RandomState(1).normal(size=(1, 35, 61, 7)) * 0.5).astype(np.float32)).to(DEV)
    try:
        prof = ops.conv_profile(True)
        assert ops._CONV_PROFILE is prof
        m.forward(x)
        torch.cuda.synchronize()
    finally:
        ops.conv_profile(False)
    assert ops._CONV_PROFILE is None
    want = [(1, h, w, slabs * (first if cw is None else cw), co) for _, h, w, cw, co in PROFILE_WALK]
    assert [len(p) for p in prof] == [5] * 19
    assert [p[4] for p in prof] == want
    for (flops, kernel, ev0, ev1, _), (n, h, w, ci, co) in zip(prof, want):
        assert flops == 2 * n * h * w * 9 * ci * co
        assert isinstance(kernel, str) and kernel
        assert ev0.elapsed_time(ev1) >= 0.0
    assert m.split_mode == dtype and not m.overflowed()
