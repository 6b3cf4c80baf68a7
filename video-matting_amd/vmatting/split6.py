"""unet.py's forward at f32 accuracy on the bf16 MFMA kernels: the split-bf16 x6 conv (``UNetVideo(dtype="bf16x6")``).

north_star asks for alpha within 1e-4 of the reference's CPU forward (unet.py:161-205).  The bf16 path misses it
(20 bf16-rounded layers; alpha 0.45 max-abs on the timed frame's steep-sigmoid pixels) and the exact-f32 MFMA
(v_mfma_f32_16x16x4_f32) runs at 1/16 of the bf16 rate.  Here every conv input and filter is carried as three bf16
parts (x = h + m + l, csrc/elementwise.hip vm_split6_nhwc; 24 significant bits) and each conv is ONE bf16 MFMA conv
over 6 stacked channel slabs,

    y = l*Wh + m*Wm + h*Wl + m*Wh + h*Wm + h*Wh       (all cross products down to 2^-16 of h*Wh)

with exact bf16 x bf16 products and f32 accumulation, smallest terms first along K.  A float64 emulation of the
whole 1080p forward puts the representation error at 3.6e-8 of max |logit| (alpha 4e-7): what remains is the f32
accumulation order, as in the f32 path.  Cost: 6x the MFMA work of the bf16 forward plus one split pass per
activation; no kernel changes — the convs run on the same patch / row kernels with f32 epilogues.

Per layer: conv (bias + relu in the f32 epilogue) -> f32 scratch -> vm_split6_nhwc into the next conv's split input
(and, fused, the split of its 2x2 SAME max-pool); the [up, skip] concats are channel ranges of one split buffer
(slab p of channel c at p*S + c, S = the concat's width), so each producer writes its own range; the upconvs resize
the f32 conv output (TF-1 legacy bilinear) before splitting.  conv1_5 (cout 1) runs with its output channels padded
to 8 and the sigmoid from the logits in a second pass.
"""

import numpy as np
import torch

from . import ops
from .unet import COUT, LEVEL, _levels, split_layers

# slab order of the activations and of the filter parts they meet (vm_split6_nhwc): l*h, m*m, h*l, m*h, h*m, h*h
W_PARTS = (0, 1, 2, 0, 1, 0)  # index into (wh, wm, wl)

# (conv scope, input channels of its split input (the concat width), output channels): conv1_1 reads 6 slabs of 16
# (8 live): 96 channels, whole 32-channel granules for the patch kernel; conv1_5's output is padded to 8
LAYERS = split_layers(16, 8)


def split3(w):
    """f32 -> (h, m, l): h = bf16(w), m = bf16(w - h), l = bf16(w - h - m) (RNE), each returned as f32 holding a
    bf16 value exactly (the pack's bf16 rounding then keeps it)."""
    w = torch.as_tensor(w, dtype=torch.float32)
    h = w.bfloat16().float()
    r = w - h
    m = r.bfloat16().float()
    lo = (r - m).bfloat16().float()
    return h, m, lo


def split6_filter(w_hwio, cin, cout):
    """[3,3,ci,co] f32 filter -> the [3,3,6*cin,cout] stack of its parts in slab order (zero rows past ci, zero
    columns past co)."""
    w = torch.as_tensor(np.asarray(w_hwio, np.float32) if not isinstance(w_hwio, torch.Tensor) else w_hwio,
                        dtype=torch.float32).cpu()
    ci, co = int(w.shape[2]), int(w.shape[3])
    parts = split3(w)
    out = torch.zeros((3, 3, 6 * cin, cout), dtype=torch.float32)
    for p, k in enumerate(W_PARTS):
        out[:, :, p * cin:p * cin + ci, :co] = parts[k]
    return out


def split6(x, y, pool=None):
    """vm_split6_nhwc: f32 view x -> its split slabs in the bf16 view y (a channel range of a 6*S-wide buffer, S =
    y's concat width), and optionally the split of its 2x2 SAME max-pool into ``pool``."""
    xv, yv = ops.nhwc(x), ops.nhwc(y)
    pv = ops.nhwc(pool) if pool is not None else None
    ops.check(ops.lib().vm_split6_nhwc(ops._ref(xv), ops._ref(yv), ops._ref(pv), ops.stream_handle()), "split6")
    return y


class SplitForward:
    """unet.py:161-205 over split activations: the walk, the buffer plan and the caches that the bf16x6 and the f16x3
    (split3.Split3Forward) forwards share.  A subclass gives the split format (SLABS stored slabs of DTYPE per
    buffer, its LAYERS view of the conv table, ``pack``) and what one step does (``first``, ``conv``, ``conv_split``,
    ``resize_split``, ``run_head``; optionally another ``level``)."""

    # the activation buffers, name -> (pyramid level, channels): split ones (SLABS * channels wide; the concats cat1..4
    # are [up, skip] channel ranges, r1..r4 the resized upconv inputs, "x" is added by plan) and f32 ones (f0..f4: the
    # convs' f32 scratch per level)
    SPLIT = dict(s11=(0, 64), cat1=(0, 128), r4=(0, 128), p1=(1, 64), s21=(1, 128), cat2=(1, 256), r3=(1, 256),
                 p2=(2, 128), s31=(2, 256), s32=(2, 256), cat3=(2, 512), r2=(2, 512), p3=(3, 256), s41=(3, 512),
                 s42=(3, 512), cat4=(3, 1024), r1=(3, 512), p4=(4, 512), s51=(4, 512))
    F32 = dict(f0=(0, 128), f1=(1, 256), f2=(2, 512), f3=(3, 512), f4=(4, 512), lg0=(0, 1), out=(0, 1))
    ZEROED = ("x",)  # allocated zeroed: the first layer's slabs are only partly written

    def __init__(self, model):
        self.m = model
        self.dev = model.device
        self.convs, self.head, self.up = {}, None, {}
        for name, cin, cout in self.LAYERS:
            self.convs[name] = self.pack(name, cin, cout, *model.params[name])
        self._b, self._key = None, None
        self.logits = None

    def weights_flat(self):
        out = []
        for pc in ([self.convs[k] for k in sorted(self.convs) if k != "conv1_5"] + self.head +
                   [self.up[k] for k in sorted(self.up)]):
            out.append(pc.packed)
            out += [t for t in (pc.bias, pc.scale, pc.shift) if t is not None]
        return out

    def plan(self, n, h, w):
        """The buffer set of an [n,h,w] batch, {name: (shape, dtype, zeroed)}: a pure function of the shape and the
        class's constants (``_buffers`` allocates it)."""
        L = _levels(h, w)
        rows = [(k, lv, self.SLABS * c, self.DTYPE) for k, (lv, c) in dict(self.SPLIT, x=(0, self.x_width())).items()]
        rows += [(k, lv, c, torch.float32) for k, (lv, c) in self.F32.items()]
        return {k: ((n,) + L[lv] + (c,), dt, k in self.ZEROED) for k, lv, c, dt in rows}

    def _buffers(self, n, h, w):
        if self._key != (n, h, w):
            self._b = {k: (torch.zeros if zeroed else torch.empty)(shape, dtype=dt, device=self.dev)
                       for k, (shape, dt, zeroed) in self.plan(n, h, w).items()}
            self._key = (n, h, w)
        return self._b

    def whole(self, buf):
        """The split-layout view of all channels of a SLABS*S-wide split buffer."""
        return buf[..., :buf.shape[-1] // self.SLABS]

    @staticmethod
    def seg(buf, off, c):
        """The split-layout view of channels [off, off + c) of a SLABS*S-wide split buffer: a [n,h,w,c] view starting
        at channel off whose rows are SLABS*S wide (the writers put the slabs at p*S + off)."""
        return buf[..., off:off + c]

    def f32(self, name):
        """Conv ``name``'s f32 scratch: its cout channels of its level's buffer."""
        return self._b["f%d" % LEVEL[name]][..., :COUT[name]]

    def level(self, src, name, r, up, y):
        """conv ``name`` (relu) over the buffer ``src`` -> f32 -> resize -> split into ``r`` -> conv ``up`` (no bias, no
        relu) into the view y, the next concat's up range (unet.py:191-200)."""
        b = self._b
        f = self.conv(b[src], name, self.f32(name))
        self.resize_split(f, self.whole(b[r]), LEVEL[up])
        self.conv_split(b[r], up, self.f32(up), y, None, "none")

    def forward(self, x, out=None):
        """x: [N,H,W,C] f32 frames (C = 7 video / 6 image) -> alpha [N,H,W,1] f32 (``out`` if given)."""
        n, h, w, _ = x.shape
        b = self._buffers(n, h, w)
        self.first(x, b["x"][..., :8])  # channels 0..7 of each slab (the frame's 7 or 6 and zeros); the rest stay zero

        def step(src, name, dst, pool=None):
            """conv (relu) -> split into all of ``dst``, or with a pool (-> its split into ``pool``) into the skip
            range of the concat ``dst``"""
            y = self.whole(b[dst]) if pool is None else self.seg(b[dst], COUT[name], COUT[name])
            self.conv_split(b[src], name, self.f32(name), y, pool and self.whole(b[pool]), "relu")

        def level(src, name, r, up, cat):
            self.level(src, name, r, up, self.seg(b[cat], 0, COUT[up]))

        # encoder (unet.py:170-189)
        step("x", "conv1_1", "s11")
        step("s11", "conv1_2", "cat1", "p1")
        step("p1", "conv2_1", "s21")
        step("s21", "conv2_2", "cat2", "p2")
        step("p2", "conv3_1", "s31")
        step("s31", "conv3_2", "s32")
        step("s32", "conv3_3", "cat3", "p3")
        step("p3", "conv4_1", "s41")
        step("s41", "conv4_2", "s42")
        step("s42", "conv4_3", "cat4", "p4")
        step("p4", "conv5_1", "s51")
        # decoder: resize (f32) -> split -> conv (no bias, no relu) into the concat's up range (unet.py:191-200)
        level("s51", "conv5_2", "r1", "upconv_1", "cat4")
        level("cat4", "conv4_4", "r2", "upconv_2", "cat3")
        level("cat3", "conv3_4", "r3", "upconv_3", "cat2")
        level("cat2", "conv2_3", "r4", "upconv_4", "cat1")
        # conv1_5 + sigmoid (unet.py:203-205)
        alpha = b["out"] if out is None else out
        self.logits = self.run_head(alpha)
        return alpha


class Split6Forward(SplitForward):
    """The split-bf16 x6 forward of a UNet (unet.UNetVideo / UNetImage) with its parameters."""

    SLABS, DTYPE, LAYERS = 6, torch.bfloat16, LAYERS
    # + the resize targets per level, the head's chunk logits and the zero logits its first chunk adds
    F32 = dict(SplitForward.F32, rr0=(0, 128), rr1=(1, 256), rr2=(2, 512), rr3=(3, 512), lg1=(0, 1), lg2=(0, 1),
               zero=(0, 1))
    ZEROED = ("x", "zero")

    def x_width(self):
        return 16

    def pack(self, name, cin, cout, w, b):
        if name == "conv1_5":
            # the cout-1 head over 6 x 128 channels as three 256-channel MFMA-head chunks [l m | h m | h h],
            # the smallest first, each adding the previous chunk's logits (vm_conv3x3_head_acc_nhwc)
            wf = split6_filter(w, cin, 1)
            self.head = [ops.PackedConv(wf[:, :, 256 * k:256 * (k + 1)].contiguous(), b if k == 0 else None,
                                        "bf16", self.dev) for k in range(3)]
            return self.head[0]
        return ops.PackedConv(split6_filter(w, cin, cout), b, "bf16", self.dev)

    def first(self, x, y):
        split6(x, y)

    def conv(self, src, name, dst_f32, act="relu"):
        return ops.conv3x3(src, self.convs[name], act, out=dst_f32, affine=False, splitk=True)

    def conv_split(self, src, name, dst_f32, y, pool, act):
        split6(self.conv(src, name, dst_f32, act), y, pool)

    def resize_split(self, f_src, r_split, lv):
        rr = self._b["rr%d" % lv]
        ops.resize_bilinear(f_src, rr.shape[1:3], out=rr)
        split6(rr, r_split)

    def run_head(self, alpha):
        """Three 256-channel chunks of the split cat1, logits accumulated, the sigmoid from the last."""
        b = self._b
        lg = [b["zero"], b["lg0"], b["lg1"], b["lg2"]]
        for k, pc in enumerate(self.head):
            xv, yv = ops.nhwc(b["cat1"][..., 256 * k:256 * (k + 1)]), ops.nhwc(lg[k + 1])
            ops.check(ops.lib().vm_conv3x3_head_acc_nhwc(
                ops.ctypes.byref(xv), ops._ptr(pc.packed), 256, ops._ptr(pc.bias), ops._ptr(lg[k]),
                ops.ctypes.byref(yv), ops._ptr(alpha if k == 2 else None), ops.stream_handle()), "conv3x3_head_acc")
        return lg[3]


def rerun_x6(owner, frames, out):
    """A span of ``owner.model``'s frames again on bf16x6 (f32 range) into ``out``: what a streamed path does with a
    chunk whose f16x3 forward left fp16's range.  ``owner._x6``, the bf16x6 forward of the same parameters, is built
    on first use (it reads the model's parameters only)."""
    if owner._x6 is None:
        owner._x6 = Split6Forward(owner.model)
    return owner._x6.forward(frames, out=out)
