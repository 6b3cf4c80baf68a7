"""unet.py's forward at f32 accuracy in three fp16 MFMA products per conv: the split-fp16 x3 path
(``UNetVideo(dtype="f16x3")``).

north_star asks for alpha within 1e-4 of the reference's CPU forward (unet.py:161-205).  The split-bf16 x6 path
(split6.py) gets there with SIX bf16 products per conv, because a bf16 part holds 8 significant bits and two parts
(16 bits; x3 = hh + hl + lh) leave alpha 7.3e-4 off on the timed frame.  An fp16 part holds 11 bits, so two parts
hold 22:

    x = h + l,  h = fp16(x), l = fp16(x - h)          (the difference is exact in f32)
    W * 2^t = Wh + Wl                                  (t per filter: max |W * 2^t| just under 2^12)
    y = (l*Wh + h*Wl + h*Wh) * 2^-t                    (exact fp16 x fp16 products, f32 accumulation)

The dropped l*Wl term and the parts' residuals are ~2^-22 of h*Wh, 64x below bf16 x3's.  A float64 emulation of the
whole 1080p forward on the bench's frame and weights (tools/split_emulate.py) puts alpha 1.9e-5 from the exact
forward (logits 4.0e-7 relative), bf16 x3 7.3e-4.  The filter scale keeps the small parts Wl in fp16's normal range
(He-normal filters are ~0.01-0.1, so their unscaled low parts would be subnormal); it is a power of two, so the
epilogue's ``* 2^-t`` is exact (the conv's per-channel scale; the bias rides in the shift).  Activations stay
unscaled: |x| on this network is ~2e3 against fp16's 65504; every kernel that writes a split activation sets an
overflow flag where it meets |x| >= 65520.  A forward zeroes and sets one flag slot: the model's own by default
(``overflowed()``; ``UNet.build`` then re-runs the frames on the bf16x6 path), or the one-element int32 device view
its caller hands it (``forward(..., overflow=slot)``: video.VideoMatter gives every chunk of a video batch its own
slot, reads them once after the run and re-runs the flagged chunks on a bf16x6 forward).

Cost: 3x the MFMA work of the bf16 forward (x6: 6x) on the same patch kernels (their fp16 MFMA form,
v_mfma_f32_16x16x32_f16); the conv's epilogue writes its output split (vm_conv3x3_split3_nhwc, and the split of the
fused 2x2 pool), so activations never round-trip through f32 except where a resize follows (conv5_2, conv4_4,
conv3_4, conv2_3 feed the TF-1 resizes, which run in f32).  Layout: a split buffer holds slabs [l, h] of its S
channels at p*S + c (S = the concat width, so the [up, skip] concats are channel ranges written by their own
producers, as in split6.py); the convs read it as [l, h, h] (the kernel re-reads slab h for the third K range,
ConvArgs::xalias), so h is stored once.  conv1_1's 7-channel frame is split into two stored slabs [l, h] of 32 channels, read as
[l, h, h] (Split3Forward.first_slab).  conv1_5 (cout 1) is one MFMA-head call over cat1's [l, h] read as [l, h, h] (12 k-steps, the third
range's fragments reused), undoing the filter scale before the sigmoid (Split3Forward.head_fused).
"""

import numpy as np
import torch

from . import ops
from .split6 import SplitForward
from .unet import split_layers

# slab order of the activations and the filter parts they meet: l*Wh, h*Wl, h*Wh
W_PARTS = (0, 1, 0)  # index into (Wh, Wl)
WTOP = 12  # filter scale: max |W * 2^t| in (2^11, 2^12]

# (conv scope, channels of its split input (the concat width), output channels); conv1_1's 8 live channels are packed
# at Split3Forward.first_slab
LAYERS = split_layers(8, 1)


def filter_scale(w):
    """2^t putting max |w * 2^t| in (2^(WTOP-1), 2^WTOP] (1 for an all-zero filter)."""
    m = float(np.abs(np.asarray(w, np.float64)).max())
    if m == 0.0:
        return 1.0
    return 2.0 ** (WTOP - int(np.ceil(np.log2(m))))


def split2h(w):
    """f32 -> (h, l): h = fp16(w), l = fp16(w - h) (RNE), returned as f32 holding fp16 values exactly."""
    w = torch.as_tensor(w, dtype=torch.float32)
    h = w.half().float()
    lo = (w - h).half().float()
    return h, lo


def split3_filter(w_hwio, cin, cout, t):
    """[3,3,ci,co] filter (f32, or f64 for a folded one), scale 2^t -> the [3,3,3*cin,cout] f32 stack of the fp16 parts
    of w * 2^t in slab order (zero rows past ci, zero columns past co).  Split in float64: h = fp16(w * 2^t), l =
    fp16(w * 2^t - h) (for an f32 w the same parts as in f32, whose difference is exact)."""
    w = torch.from_numpy(np.asarray(w_hwio, np.float64) * float(t))  # exact: a power of two
    ci, co = int(w.shape[2]), int(w.shape[3])
    h = w.half().double()
    parts = (h.float(), (w - h).half().float())
    out = torch.zeros((3, 3, 3 * cin, cout), dtype=torch.float32)
    for p, k in enumerate(W_PARTS):
        out[:, :, p * cin:p * cin + ci, :co] = parts[k]
    return out


# TF-1 legacy bilinear 2x (scale 0.5) as a phase filter: resized row 2i + a blends low-res rows by R[a] (rows: the
# low-res tap u = offset u - 1, columns: the 3x3 kernel row kh), the same table as csrc/conv_up2x.hip fold_up2x_weights
_R = np.array([[[.5, 0., 0.], [.5, 1., .5], [0., 0., .5]], [[0., 0., 0.], [1., .5, 0.], [0., .5, 1.]]])


def fold_up2x(w_hwio):
    """conv3x3(resize2x(x), w) = conv3x3(x, W') away from the frame border: W' [3,3,cin,4*cout] (channel p*cout + co =
    phase p = 2a + b of output channel co, pixel (2i + a, 2j + b)), in float64 (vm_conv3x3_fold_up2x_weights rounds it
    to f32; here the fp16 parts are cut from the exact sum)."""
    w = np.asarray(w_hwio, np.float64)
    co = w.shape[3]
    out = np.zeros((3, 3, w.shape[2], 4 * co))
    for p in range(4):
        out[..., p * co:(p + 1) * co] = np.einsum("uk,vl,klio->uvio", _R[p >> 1], _R[p & 1], w)
    return out


# upconvs whose resize is an exact 2x (unet.py:191-200 at 1080p: upconv_2..4; upconv_1's 68 -> 135 is not): with
# Split3Forward.fold_up the resize is folded into the filter (vm_conv3x3_up2x_split3_nhwc), zero phase taps skipped
# (25 of 36), no resized tensor
FOLD = ("upconv_2", "upconv_3", "upconv_4")


def split3h(x, y, pool=None, slab=0, overflow=None):
    """vm_split3h_nhwc: f32 view x -> its [l, h, h] slabs in the fp16 view y (a channel range of a 3*S-wide buffer,
    S = ``slab`` or y's concat width), optionally the split of its 2x2 SAME max-pool into ``pool``; ``overflow`` (a
    device int32) is set to 1 where |x| >= 65520."""
    xv, yv = ops.nhwc(x), ops.nhwc(y)
    pv = ops.nhwc(pool) if pool is not None else None
    ops.check(ops.lib().vm_split3h_nhwc(ops._ref(xv), ops._ref(yv), ops._ref(pv), int(slab), ops._ptr(overflow),
                                        ops.stream_handle()), "split3h")
    return y


def resize_split3h(x, y, slab=0, overflow=None):
    """vm_resize_split3h_nhwc: TF-1 legacy bilinear resize (unet.py:58) of the f32 view x to y's size, written split
    into the fp16 view y (bit-identical to ops.resize_bilinear + split3h)."""
    xv, yv = ops.nhwc(x), ops.nhwc(y)
    ops.check(ops.lib().vm_resize_split3h_nhwc(ops.ctypes.byref(xv), ops.ctypes.byref(yv), int(slab),
                                               ops._ptr(overflow), ops.stream_handle()), "resize_split3h")
    return y


def conv_f32(x, pc, y, act="relu", splitk=True):
    """The fp16 conv of split input x (a two-slab [l, h] view read as [l, h, h], or a plain fp16 view of pc.cin
    channels) into the f32 view y (vm_conv3x3_ex_nhwc; split-K on small grids)."""
    xv, yv = ops.nhwc(x), ops.nhwc(y)
    wsz = ops.lib().vm_conv3x3_workspace_bytes(ops.ctypes.byref(xv), pc.cin, pc.cout) if splitk else 0
    ws = ops._workspace(wsz, x.device) if wsz else None
    prof = ops._ConvProf()
    ops.check(ops.lib().vm_conv3x3_ex_nhwc(ops.ctypes.byref(xv), 1, 0, ops._ptr(pc.packed), pc.cin, pc.cout,
                                           ops._ptr(pc.bias), ops._ptr(pc.scale), ops._ptr(pc.shift), ops._lib.ACT[act],
                                           ops.ctypes.byref(yv), ops._ptr(ws), wsz, ops.stream_handle()), "conv3x3(f16)")
    n, h, w, _ = x.shape
    prof.done(2 * n * h * w * 9 * pc.cin * pc.cout, (n, h, w, pc.cin, pc.cout))
    return y


def conv_split(x, pc, y, act="relu", pool=None, overflow=None, y_slab=0, pool_slab=0, splitk=True):
    """vm_conv3x3_split3_nhwc: the fp16 conv of split input x with its output written split into the fp16 view y
    (and the split of its 2x2 SAME max-pool into ``pool``) from the conv's epilogue — no f32 round trip."""
    xv, yv = ops.nhwc(x), ops.nhwc(y)
    pv = ops.nhwc(pool) if pool is not None else None
    wsz = ops.lib().vm_conv3x3_workspace_bytes(ops.ctypes.byref(xv), pc.cin, pc.cout) if (splitk and pool is None) else 0
    ws = ops._workspace(wsz, x.device) if wsz else None
    prof = ops._ConvProf()
    ops.check(ops.lib().vm_conv3x3_split3_nhwc(
        ops._ref(xv), ops._ptr(pc.packed), pc.cin, pc.cout, ops._ptr(pc.bias), ops._ptr(pc.scale), ops._ptr(pc.shift),
        ops._lib.ACT[act], ops._ref(yv), int(y_slab), ops._ref(pv), int(pool_slab), ops._ptr(overflow), ops._ptr(ws),
        wsz, ops.stream_handle()), "conv3x3_split3")
    n, h, w, _ = x.shape
    prof.done(2 * n * h * w * 9 * pc.cin * pc.cout, (n, h, w, pc.cin, pc.cout))
    return y


def up_split(x, pc_up, pc, y, overflow=None, act="none", y_slab=0):
    """vm_conv3x3_up2x_split3_nhwc: the folded 2x upconv of the low-res split input x ([l, h]) into the full-res split
    view y (pc_up: the folded filter's parts, pc: the plain filter's, for the border pass; same scale)."""
    xv, yv = ops.nhwc(x), ops.nhwc(y)
    prof = ops._ConvProf()
    ops.check(ops.lib().vm_conv3x3_up2x_split3_nhwc(
        ops.ctypes.byref(xv), ops._ptr(pc_up.packed), ops._ptr(pc.packed), pc.cin, pc.cout, ops._ptr(pc.bias),
        ops._ptr(pc.scale), ops._ptr(pc.shift), ops._lib.ACT[act], ops.ctypes.byref(yv), int(y_slab),
        ops._ptr(overflow), ops.stream_handle()), "conv3x3_up2x_split3")
    n, h, w, _ = y.shape  # FLOPs of the unfolded conv it stands for (its output pixels)
    prof.done(2 * n * h * w * 9 * pc.cin * pc.cout, (n, h, w, pc.cin, pc.cout))
    return y


def _descale(cout, t, bias=None):
    """A conv's epilogue (acc * 2^-t) + b: exact descale, then the bias (unet.py:41,73)."""
    return dict(scale=np.full(cout, 1.0 / t, np.float32), shift=np.zeros(cout, np.float32) if bias is None else bias)


class Split3Forward(SplitForward):
    """The split-fp16 x3 forward of a UNet (unet.UNetVideo / UNetImage) with its parameters."""

    SLABS, DTYPE, LAYERS = 2, torch.float16, LAYERS  # (two stored slabs [l, h], read as [l, h, h])
    # + the folded upconvs' low-res split inputs: conv4_4 / conv3_4 / conv2_3 written split
    SPLIT = dict(SplitForward.SPLIT, c44s=(3, 512), c34s=(2, 256), c23s=(1, 128))
    LOWRES = {"conv4_4": "c44s", "conv3_4": "c34s", "conv2_3": "c23s"}
    # conv -> split in the conv's epilogue (vm_conv3x3_split3_nhwc); False: f32 output + vm_split3h_nhwc (A/B)
    fuse_split = True
    # the exact-2x upconvs on the folded filter (fuse_split only) — measured slower here (1080p: upconv_2 / _3 / _4
    # 1.49 / 1.06 / 0.92 ms folded with their split border pass, against 0.75 / 0.82 / 0.85 resized; the 12-step split
    # border pass is latency-bound) and ~2x the f32 accumulation error (the 64x96 golden 1.4e-4): off, kept for A/B
    fold_up = False
    # conv1_1's input slab width: 32 (three granules: the l*Wh and h*Wl sums run before h*Wh joins them) or 8 (three
    # slabs + a zero 4th in ONE granule, 0.03 ms faster at 1080p, but every MFMA mixes the small and the large products:
    # the 64x96 golden's alpha 1.01e-4 against 7.8e-5 with 32, fp32 4.1e-5 — tools/x3_golden_study.py)
    first_slab = 32
    # conv1_5 in one MFMA-head call over cat1's [l, h] read as [l, h, h] (12 k-steps, the third range's fragments
    # reused); False: two calls, [l | h] x [Wh | Wl] then [h] x [Wh] adding the first's logits (A/B)
    head_fused = True

    def __init__(self, model):
        self.scales = {}
        super().__init__(model)  # (.up: the folded upconv filters, FOLD)
        self.overflow = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._ovf = self.overflow  # the flag slot of the forward under way

    def pack(self, name, cin, cout, w, b):
        t = self.scales[name] = filter_scale(w)
        if name == "conv1_5":
            wf = split3_filter(w, cin, 1, t)
            if self.head_fused:  # [l, h, h] x [Wh, Wl, Wh], descaled + bias in the epilogue
                self.head = [ops.PackedConv(wf, None, "f16", self.dev, **_descale(1, t, b))]
            else:  # [l | h] against [Wh | Wl] (256 channels), then [h] against [Wh] adding the first chunk's logits
                self.head = [ops.PackedConv(wf[:, :, :256].contiguous(), None, "f16", self.dev),
                             ops.PackedConv(wf[:, :, 256:].contiguous(), None, "f16", self.dev, **_descale(1, t, b))]
            return self.head[-1]
        cp = self.first_slab if name == "conv1_1" else cin  # slab width (7 or 6 live channels): see first_slab
        if name in FOLD:  # one scale for the folded filter and the plain one (its border pass)
            wu = fold_up2x(w)
            t = self.scales[name] = min(t, filter_scale(wu))  # max |W' * 2^t| and max |W * 2^t| both <= 2^12
            self.up[name] = ops.PackedConv(split3_filter(wu, cin, 4 * cout, t), None, "f16", self.dev,
                                           **_descale(cout, t))
        wf = split3_filter(w, cp, cout, t)
        if name == "conv1_1" and cp == 8:
            wf = torch.cat([wf, torch.zeros((3, 3, 8, cout))], 2)
        return ops.PackedConv(wf, None, "f16", self.dev, **_descale(cout, t, b))

    def x_width(self):
        # (slab 8: [l, h, h] + a zero 4th slab in one granule; wider: the two stored slabs [l, h], read as [l, h, h])
        return 16 if self.first_slab == 8 else self.first_slab

    def overflowed(self):
        """True when the last forward that ran on the model's own flag (no ``overflow=`` slot) met |x| >= 65520
        (synchronises)."""
        return bool(self.overflow.item())

    def forward(self, x, out=None, overflow=None):
        """x: [N,H,W,C] f32 frames (C = 7 video / 6 image) -> alpha [N,H,W,1] f32 (``out`` if given).  ``overflow``: the
        one-element int32 device view this forward zeroes and sets to 1 where an activation left fp16's range
        (default: the model's own flag, read by ``overflowed()``); no other flag is touched."""
        if overflow is not None and not (isinstance(overflow, torch.Tensor) and overflow.dtype == torch.int32 and
                                         overflow.numel() == 1 and overflow.device == x.device):
            raise ValueError("overflow must be a one-element int32 view on the frames' device")
        self._ovf = self.overflow if overflow is None else overflow
        self._ovf.zero_()
        return super().forward(x, out)

    def first(self, x, y):
        split3h(x, y, slab=self.first_slab, overflow=self._ovf)

    def conv(self, src, name, dst_f32, act="relu", splitk=True):
        return conv_f32(src, self.convs[name], dst_f32, act, splitk)

    def conv_split(self, src, name, dst_f32, y, pool, act):
        """conv -> split (-> pool split): fused, or the f32 round trip"""
        if self.fuse_split:
            return conv_split(src, self.convs[name], y, act, pool, self._ovf)
        # (no split-K under a pool, as the fused form: the same sums, bit for bit)
        split3h(self.conv(src, name, dst_f32, act, splitk=pool is None), y, pool, overflow=self._ovf)

    def resize_split(self, f_src, r_split, lv):
        if self.fuse_split:  # the resize written split, no f32 resized tensor
            return resize_split3h(f_src, r_split, overflow=self._ovf)
        rr = torch.empty(r_split.shape[:3] + f_src.shape[3:], dtype=torch.float32, device=f_src.device)
        ops.resize_bilinear(f_src, rr.shape[1:3], out=rr)
        split3h(rr, r_split, overflow=self._ovf)

    def level(self, src, name, r, up, y):
        """As the base's; with fold_up (and fuse_split), where the resize is an exact 2x, conv ``name`` is written split
        and ``up`` runs as the folded 2x upconv on that low-res output (unet.py:192-200)."""
        x = self._b[src]
        if not (self.fold_up and self.fuse_split and up in FOLD and
                tuple(y.shape[1:3]) == (2 * x.shape[1], 2 * x.shape[2])):
            return super().level(src, name, r, up, y)
        s = self._b[self.LOWRES[name]]
        self.conv_split(x, name, self.f32(name), self.whole(s), None, "relu")
        up_split(s, self.up[up], self.convs[up], y, self._ovf)

    def run_head(self, alpha):
        """[l | h] x [Wh | Wl], then [h] x [Wh] + those logits, * 2^-t + bias (head_fused: one call)."""
        b = self._b
        lg0, logits = b["lg0"], b["f0"][..., :1]
        chunks = (((b["cat1"], logits, None),) if self.head_fused else
                  ((b["cat1"], lg0, None), (b["cat1"][..., 128:], logits, lg0)))
        for k, (xs, yv, acc) in enumerate(chunks):
            pc = self.head[k]
            xv, yvv = ops.nhwc(xs), ops.nhwc(yv)
            ops.check(ops.lib().vm_conv3x3_head_acc_ex_nhwc(
                ops.ctypes.byref(xv), ops._ptr(pc.packed), pc.cin, None, ops._ptr(pc.scale),
                ops._ptr(pc.shift), ops._ptr(acc), ops.ctypes.byref(yvv),
                ops._ptr(alpha if k == len(chunks) - 1 else None), ops.stream_handle()), "conv3x3_head_acc_ex")
        return logits
