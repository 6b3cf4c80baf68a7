"""Tensor-level wrappers over the C ABI (torch tensors on a ROCm device in, out).

Each function is one TF/OpenCV op of the reference (cited in include/vmatting.h).
NHWC views: any torch tensor whose last dim is contiguous and whose pixel rows
are evenly strided (stride(1) == W*stride(2), stride(0) == H*stride(1)) — in
particular a channel slice ``buf[..., a:b]`` of a wider buffer, which is how
tf.concat is expressed without copies.
"""

import ctypes
import functools

import numpy as np
import torch

from . import _lib
from ._lib import VmTensor, check, lib, stream_handle

_DT = {torch.float32: _lib.VM_F32, torch.bfloat16: _lib.VM_BF16, torch.uint8: _lib.VM_U8,
       torch.float16: _lib.VM_F16}  # (fp16: the split-fp16 x3 conv operands only, vmatting/split3.py)
TORCH_DTYPE = {"fp32": torch.float32, "f32": torch.float32, "float32": torch.float32,
               "bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "f16": torch.float16}


def _require_gpu(t):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise TypeError("vmatting ops take ROCm device tensors (got %r)" % (type(t) if not isinstance(t, torch.Tensor)
                                                                          else t.device))


def nhwc(t):
    """Describe a 4-D NHWC torch view as a vm_tensor (by value)."""
    _require_gpu(t)
    if t.dim() != 4:
        raise ValueError("expected NHWC 4-D tensor, got shape %s" % (tuple(t.shape),))
    n, h, w, c = t.shape
    s0, s1, s2, s3 = t.stride()
    if s3 != 1 or (h > 1 and s1 != w * s2) or (n > 1 and s0 != h * s1):
        raise ValueError("tensor is not an NHWC channel-slice view (strides %s)" % (t.stride(),))
    if t.dtype not in _DT:
        raise TypeError("unsupported dtype %s" % t.dtype)
    return VmTensor(t.data_ptr(), n, h, w, c, s2, 0, _DT[t.dtype])


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _ref(v):
    """byref of a vm_tensor, or NULL for an absent one."""
    return None if v is None else ctypes.byref(v)


def _f32(t):
    if t is None:
        return None
    _require_gpu(t)
    assert t.dtype == torch.float32 and t.is_contiguous()
    return t


# ---------------------------------------------------------------------------------------------- conv

class PackedConv:
    """One 3x3 conv's weights in kernel layout, plus its f32 bias / per-channel affine (folded BN).

    ``w_hwio``: TF-layout filter [3,3,cin,cout] (numpy or tensor).  The reference creates
    these in unet.py:11-17 (init_conv) / 65-74 (VGG filters).
    """

    def __init__(self, w_hwio, bias=None, dtype="bf16", device="cuda", scale=None, shift=None):
        w = torch.as_tensor(np.asarray(w_hwio, np.float32) if not isinstance(w_hwio, torch.Tensor) else w_hwio,
                            dtype=torch.float32).to(device).contiguous()
        if w.dim() != 4 or w.shape[0] != 3 or w.shape[1] != 3:
            raise ValueError("expected a [3,3,cin,cout] filter, got %s" % (tuple(w.shape),))
        self.cin, self.cout = int(w.shape[2]), int(w.shape[3])
        self.dtype = TORCH_DTYPE[dtype] if isinstance(dtype, str) else dtype
        self.w_hwio = w
        vdt = _DT[self.dtype]
        nbytes = lib().vm_conv3x3_packed_bytes(self.cin, self.cout, vdt)
        self.packed = torch.empty(nbytes, dtype=torch.uint8, device=device)
        check(lib().vm_conv3x3_pack_weights(_ptr(w), self.cin, self.cout, vdt, _ptr(self.packed),
                                            stream_handle()), "pack_weights")
        as_f = lambda v: None if v is None else torch.as_tensor(np.asarray(v, np.float32) if not isinstance(  # noqa
            v, torch.Tensor) else v, dtype=torch.float32).to(device).contiguous()
        self.bias = as_f(bias)
        self.scale = as_f(scale)
        self.shift = as_f(shift)

    @classmethod
    def from_source(cls, src, cin, cout, dtype="bf16", flip=False, bias=None):
        """A (cin, cout) conv packed from the f32 HWIO filter ``src`` with zeros outside it: a cout-padded copy of a
        narrow conv (flip=False), or the data-gradient conv of ``src`` (flip=True: spatially flipped, in/out
        transposed, so cin >= src's cout and cout = src's cin).  ``src`` is read again by every pack_batch."""
        self = cls.__new__(cls)
        self.cin, self.cout = int(cin), int(cout)
        self.dtype = TORCH_DTYPE[dtype] if isinstance(dtype, str) else dtype
        self.w_hwio, self._src, self._flip = None, src, bool(flip)  # src: a tensor, or a PackedConv (its filter)
        nbytes = lib().vm_conv3x3_packed_bytes(self.cin, self.cout, _DT[self.dtype])
        self.packed = torch.empty(nbytes, dtype=torch.uint8, device=self._source().device)
        self.bias, self.scale, self.shift = bias, None, None
        pack_batch([self])
        return self

    def _source(self):
        src = self.w_hwio if self.w_hwio is not None else self._src
        return src.w_hwio if isinstance(src, PackedConv) else src

    def pack_job(self):
        src = self._source()
        flip = getattr(self, "_flip", False)
        return _lib.VmPackJob(_ptr(src), _ptr(self.packed), self.cin, self.cout, _DT[self.dtype], int(flip),
                              int(src.shape[2]), int(src.shape[3]))

    def up2x(self):
        """The folded-resize weights of this filter (vm_conv3x3_fold_up2x_weights + pack, cout' = 4*cout),
        built once on first use; None when the compute dtype has no folded path (f32)."""
        if self.dtype != torch.bfloat16 or self.cout % 64:
            return None
        if getattr(self, "_up", None) is None:
            dev = self.packed.device
            wu = torch.empty((3, 3, self.cin, 4 * self.cout), dtype=torch.float32, device=dev)
            check(lib().vm_conv3x3_fold_up2x_weights(_ptr(self.w_hwio), self.cin, self.cout, _ptr(wu),
                                                     stream_handle()), "fold_up2x_weights")
            nbytes = lib().vm_conv3x3_packed_bytes(self.cin, 4 * self.cout, _DT[self.dtype])
            self._up = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            check(lib().vm_conv3x3_pack_weights(_ptr(wu), self.cin, 4 * self.cout, _DT[self.dtype], _ptr(self._up),
                                                stream_handle()), "pack_weights(up2x)")
        return self._up

    def repack(self):
        """Re-pack after the f32 HWIO filter changed in place (the optimizer step of train.VideoTrainer)."""
        pack_batch([self])
        return self

    def set_affine(self, scale, shift):
        self.scale = None if scale is None else torch.as_tensor(scale, dtype=torch.float32).to(self.packed.device)
        self.shift = None if shift is None else torch.as_tensor(shift, dtype=torch.float32).to(self.packed.device)

    def __call__(self, x, act="none", out=None, out_dtype=None, affine=None):
        return conv3x3(x, self, act, out, out_dtype, affine)


class PackBatch:
    """Re-pack many PackedConvs in one launch (vm_conv3x3_pack_weights_batch); the job array is built once, so the
    sources and packed buffers must stay where they are (the trainer's flat parameter buffer does)."""

    def __init__(self, convs):
        self.convs = list(convs)
        self.jobs = (_lib.VmPackJob * max(1, len(self.convs)))(*[pc.pack_job() for pc in self.convs])

    def __call__(self):
        check(lib().vm_conv3x3_pack_weights_batch(len(self.convs), self.jobs, stream_handle()), "pack_weights_batch")
        for pc in self.convs:
            pc._up = None


def pack_batch(convs):
    PackBatch(convs)()


class SourceConcat:
    """The channel concat of ``nsrc`` equally shaped feature maps stored one after another in ``base``
    ([nsrc*N, H, W, C], contiguous) — unet_simple.py:153-168's per-level concat of the three VGG towers, which
    run as ONE batch-3N pass here.  Never materialised: conv3x3 / conv_wgrad read it as split sources."""

    def __init__(self, base, nsrc):
        if base.dim() != 4 or base.shape[0] % nsrc or not base.is_contiguous():
            raise ValueError("SourceConcat: base must be a contiguous [nsrc*N,H,W,C] tensor")
        self.base, self.nsrc = base, int(nsrc)
        n = base.shape[0] // nsrc
        self.src0 = base[:n]
        self.stride = n * base.shape[1] * base.shape[2] * base.shape[3]
        self.shape = (n, base.shape[1], base.shape[2], nsrc * base.shape[3])
        self.dtype, self.device, self.is_cuda = base.dtype, base.device, base.is_cuda

    def source(self, i):
        n = self.shape[0]
        return self.base[i * n:(i + 1) * n]

    def materialize(self):
        return torch.cat([self.source(i) for i in range(self.nsrc)], -1)


def conv3x3(x, pc, act="none", out=None, out_dtype=None, affine=None, pool_out=None, splitk=False):
    """tf.nn.conv2d 3x3 SAME + bias_add (+ folded BN affine) + activation, on MFMA.

    ``affine``: None -> the PackedConv's own scale/shift; False -> none; (scale, shift) -> those.
    ``pool_out``: also write tf.nn.max_pool 2x2/2 SAME of the result there (fused into the conv epilogue when
    the kernel supports it, else a separate max-pool launch).
    ``splitk``: allow split-K on small grids (a workspace is passed; the per-pixel summation order then depends
    on the batch size, so the inference nets, whose frames must not depend on their batch, leave it off).
    """
    if x.dtype != pc.dtype:
        raise TypeError("conv input dtype %s != packed weights dtype %s" % (x.dtype, pc.dtype))
    if x.shape[-1] != pc.cin:
        raise ValueError("conv input has %d channels, filter expects %d" % (x.shape[-1], pc.cin))
    n, h, w, _ = x.shape
    if out is None:
        out = torch.empty((n, h, w, pc.cout), dtype=out_dtype or x.dtype, device=x.device)
    if affine is None:
        scale, shift = pc.scale, pc.shift
    elif affine is False:
        scale = shift = None
    else:
        scale, shift = affine
    if isinstance(x, SourceConcat) or pool_out is None:
        # the general entry: split sources and/or a workspace for split-K on small grids
        if isinstance(x, SourceConcat):
            xv, nsrc, stride = nhwc(x.src0), x.nsrc, x.stride
            if pool_out is not None:
                raise ValueError("conv3x3: no fused pooling over split sources")
        else:
            xv, nsrc, stride = nhwc(x), 1, 0
        yv = nhwc(out)
        wsz = lib().vm_conv3x3_workspace_bytes(ctypes.byref(xv), pc.cin, pc.cout) if splitk else 0
        ws = _workspace(wsz, x.device) if wsz else None
        prof = _ConvProf()
        rc = lib().vm_conv3x3_ex_nhwc(ctypes.byref(xv), nsrc, stride, _ptr(pc.packed), pc.cin, pc.cout,
                                      _ptr(pc.bias), _ptr(scale), _ptr(shift), _lib.ACT[act], ctypes.byref(yv),
                                      _ptr(ws), wsz, stream_handle())
        if rc == _lib.VM_EUNSUPPORTED and nsrc > 1:
            # sources spread wider than the kernels' 32-bit offsets reach (large batches): one materialised concat
            xm = x.materialize()
            xv = nhwc(xm)
            rc = lib().vm_conv3x3_ex_nhwc(ctypes.byref(xv), 1, 0, _ptr(pc.packed), pc.cin, pc.cout, _ptr(pc.bias),
                                          _ptr(scale), _ptr(shift), _lib.ACT[act], ctypes.byref(yv), _ptr(ws), wsz,
                                          stream_handle())
        check(rc, "conv3x3")
        prof.done(2 * n * h * w * 9 * pc.cin * pc.cout, (n, h, w, pc.cin, pc.cout))
        return out
    xv, yv = nhwc(x), nhwc(out)
    prof = _ConvProf()
    fused = False
    if pool_out is not None:
        pv = nhwc(pool_out)
        rc = lib().vm_conv3x3_pool_nhwc(ctypes.byref(xv), _ptr(pc.packed), pc.cin, pc.cout, _ptr(pc.bias),
                                        _ptr(scale), _ptr(shift), _lib.ACT[act], ctypes.byref(yv), ctypes.byref(pv),
                                        stream_handle())
        if rc != _lib.VM_EUNSUPPORTED:
            check(rc, "conv3x3_pool")
            fused = True
    if not fused:
        check(lib().vm_conv3x3_nhwc(ctypes.byref(xv), _ptr(pc.packed), pc.cin, pc.cout, _ptr(pc.bias), _ptr(scale),
                                    _ptr(shift), _lib.ACT[act], ctypes.byref(yv), stream_handle()), "conv3x3")
    prof.done(2 * n * h * w * 9 * pc.cin * pc.cout, (n, h, w, pc.cin, pc.cout))
    if pool_out is not None and not fused:
        maxpool2x2(out, out=pool_out)
    return out


def conv_head(x, pc, act="none", out=None, alpha=None, partial=None):
    """cout == 1 conv (unet.py:203-204 conv1_5) into ``out``; with ``alpha`` (contiguous f32, one value per pixel)
    also tf.nn.sigmoid of the pre-activation from the same pass (unet.py:205), saving a separate elementwise launch."""
    if pc.cout != 1:
        raise ValueError("conv_head needs a cout == 1 filter")
    if x.dtype != pc.dtype:
        raise TypeError("conv input dtype %s != packed weights dtype %s" % (x.dtype, pc.dtype))
    n, h, w, _ = x.shape
    if out is None:
        out = torch.empty((n, h, w, 1), dtype=torch.float32, device=x.device)
    if alpha is not None:
        _require_gpu(alpha)
        if alpha.dtype != torch.float32 or not alpha.is_contiguous() or alpha.numel() != n * h * w:
            raise ValueError("alpha must be a contiguous f32 tensor of n*h*w elements")
    xv, yv = nhwc(x), nhwc(out)
    prof = _ConvProf()
    if partial is not None:  # + the per-tap shares of the channels x does not carry (conv_pair_first_head)
        if partial.dtype != torch.float32 or not partial.is_contiguous() or tuple(partial.shape) != (n, h, w, 12):
            raise ValueError("partial must be a contiguous f32 [n,h,w,12] tensor")
        check(lib().vm_conv3x3_head_partial_nhwc(ctypes.byref(xv), _ptr(pc.packed), pc.cin, _ptr(pc.bias),
                                                 _ptr(pc.scale), _ptr(pc.shift), _lib.ACT[act], ctypes.byref(yv),
                                                 _ptr(alpha), _ptr(partial), stream_handle()), "conv3x3_head_partial")
    else:
        check(lib().vm_conv3x3_head_nhwc(ctypes.byref(xv), _ptr(pc.packed), pc.cin, _ptr(pc.bias), _ptr(pc.scale),
                                         _ptr(pc.shift), _lib.ACT[act], ctypes.byref(yv), _ptr(alpha),
                                         stream_handle()), "conv3x3_head")
    prof.done(2 * n * h * w * 9 * pc.cin)
    return out


def conv_pair_first_head(x, pc1, pc2, head_w, head_coff, partial, act2="relu", out=None, pool_out=None,
                         store_y=False, fallback=False):
    """conv_pair_first with the head split (vm_conv3x3_pair_first_head_nhwc): besides pool_out (and ``out`` when
    store_y) the pair kernel writes ``partial`` [n,h,w,12] f32 = per-tap shares of the cout == 1 head filter
    ``head_w`` (device f32 HWIO [3,3,cin_head,1]) over its output channels, which sit at head_coff of the head's
    input (unet.py:203: conv1_5 over cat1 = [upconv_4, conv1_2]).  conv_head(..., partial=partial) finishes it.
    ``fallback``: return None instead of raising when the kernel cannot take the case (the caller runs the
    unsplit path)."""
    n, h, w, _ = x.shape
    if pc1.dtype != torch.bfloat16 or pc2.dtype != torch.bfloat16 or pc1.cout != 64 or pc2.cin != 64:
        raise NotImplementedError("conv_pair_first_head: bf16 64-channel pair only")
    if head_w.dtype != torch.float32 or not head_w.is_contiguous() or head_w.dim() != 4 or head_w.shape[3] != 1:
        raise ValueError("head_w must be a contiguous f32 [3,3,cin,1] filter")
    if partial.dtype != torch.float32 or not partial.is_contiguous() or tuple(partial.shape) != (n, h, w, 12):
        raise ValueError("partial must be a contiguous f32 [n,h,w,12] tensor")
    _require_gpu(head_w)
    _require_gpu(partial)
    if out is None:
        out = torch.empty((n, h, w, pc2.cout), dtype=torch.bfloat16, device=x.device)
    xv, yv = nhwc(x), nhwc(out)
    pv = nhwc(pool_out) if pool_out is not None else None
    prof = _ConvProf()
    rc = lib().vm_conv3x3_pair_first_head_nhwc(
        ctypes.byref(xv), _ptr(pc1.packed), pc1.cin, _ptr(pc1.bias), _ptr(pc2.packed), pc2.cout, _ptr(pc2.bias),
        _ptr(pc2.scale), _ptr(pc2.shift), _lib.ACT[act2], ctypes.byref(yv),
        _ref(pv), _ptr(head_w), int(head_w.shape[2]), head_coff, _ptr(partial), int(bool(store_y)), stream_handle())
    if rc == _lib.VM_EUNSUPPORTED and fallback:
        return None  # e.g. a kernel-selection override (vm_set_option "conv_kernel"/"pair_kernel") rules it out
    check(rc, "conv3x3_pair_first_head")
    prof.done(2 * n * h * w * 9 * (pc1.cin * pc1.cout + pc2.cin * pc2.cout))
    return out


def conv_pair_first(x, pc1, pc2, act2="relu", out=None, pool_out=None, mid=None, keep_mid=False):
    """conv3x3(relu(conv3x3(x, pc1)), pc2) (+ 2x2 SAME max-pool into pool_out): unet.py:170-172, conv1_1 -> conv1_2
    (-> pool1).  bf16 runs ONE kernel whose 64-channel intermediate stays in LDS (vm_conv3x3_pair_first_nhwc); any
    other case runs the two convs through ``mid`` (the intermediate, allocated when None).  ``keep_mid``: ``mid``
    receives conv1_1's output in every case (the fused kernel writes it too, vm_conv3x3_pair_first_mid_nhwc)."""
    n, h, w, _ = x.shape
    if out is None:
        out = torch.empty((n, h, w, pc2.cout), dtype=x.dtype, device=x.device)
    if x.dtype in (torch.bfloat16, torch.float32) and pc1.dtype == pc2.dtype == torch.bfloat16 and pc1.cout == 64 \
            and pc2.cin == 64:
        xv, yv = nhwc(x), nhwc(out)
        pv = nhwc(pool_out) if pool_out is not None else None
        prof = _ConvProf()
        if keep_mid:
            if mid is None or mid.dtype != torch.bfloat16:
                raise ValueError("keep_mid needs a bf16 mid buffer")
            mv = nhwc(mid)
            rc = lib().vm_conv3x3_pair_first_mid_nhwc(ctypes.byref(xv), _ptr(pc1.packed), pc1.cin, _ptr(pc1.bias),
                                                      _ptr(pc2.packed), pc2.cout, _ptr(pc2.bias), _ptr(pc2.scale),
                                                      _ptr(pc2.shift), _lib.ACT[act2], ctypes.byref(yv),
                                                      _ref(pv), ctypes.byref(mv), stream_handle())
        else:
            rc = lib().vm_conv3x3_pair_first_nhwc(ctypes.byref(xv), _ptr(pc1.packed), pc1.cin, _ptr(pc1.bias),
                                                  _ptr(pc2.packed), pc2.cout, _ptr(pc2.bias), _ptr(pc2.scale),
                                                  _ptr(pc2.shift), _lib.ACT[act2], ctypes.byref(yv),
                                                  _ref(pv), stream_handle())
        if rc != _lib.VM_EUNSUPPORTED:
            check(rc, "conv3x3_pair_first")
            prof.done(2 * n * h * w * 9 * (pc1.cin * pc1.cout + pc2.cin * pc2.cout))
            return out
    if x.dtype != pc1.dtype:  # the unfused path takes the frame in the compute dtype, channels padded to 8
        c = x.shape[-1]
        xb = torch.empty((n, h, w, (c + 7) // 8 * 8), dtype=pc1.dtype, device=x.device)
        x = convert(x, xb)[..., :c]
    m = conv3x3(x, pc1, "relu", out=mid)
    return conv3x3(m, pc2, act2, out=out, pool_out=pool_out)


def upconv3x3(x, pc, act="none", out=None, size=None, rbuf=None, fold=True):
    """tf.image.resize_images(x, size) -> conv3x3 (unet.py:44-63, the upconv half of upconv_concat).

    Exact 2x upsampling in bf16 runs as ONE folded conv on the low-res frame (vm_conv3x3_up2x_nhwc, no resized
    tensor in HBM) when ``fold``; any other case is the resize kernel (into ``rbuf`` if given) followed by the
    conv kernel."""
    n, h, w, _ = x.shape
    oh, ow = (2 * h, 2 * w) if size is None else (int(size[0]), int(size[1]))
    if out is None:
        out = torch.empty((n, oh, ow, pc.cout), dtype=x.dtype, device=x.device)
    up = pc.up2x() if fold and (oh, ow) == (2 * h, 2 * w) and x.dtype == pc.dtype else None
    if up is not None:
        xv, yv = nhwc(x), nhwc(out)
        prof = _ConvProf()
        rc = lib().vm_conv3x3_up2x_nhwc(ctypes.byref(xv), _ptr(up), _ptr(pc.packed), pc.cin, pc.cout, _ptr(pc.bias),
                                        _ptr(pc.scale), _ptr(pc.shift), _lib.ACT[act], ctypes.byref(yv),
                                        stream_handle())
        if rc != _lib.VM_EUNSUPPORTED:
            check(rc, "conv3x3_up2x")
            prof.done(2 * n * oh * ow * 9 * pc.cin * pc.cout)
            return out
    r = resize_bilinear(x, (oh, ow), out=rbuf)
    return conv3x3(r, pc, act, out=out)


def upconv3x3_head(x, pc, head_w, head_coff, partial, act="none", out=None, store_y=False):
    """upconv3x3 (exact 2x, folded) with the head split (vm_conv3x3_up2x_head_nhwc): besides ``out`` (written only
    when store_y) the conv writes ``partial`` [n,2h,2w,12] f32 = per-tap shares of the cout == 1 head filter
    ``head_w`` (device f32 HWIO [3,3,cin_head,1]) over its 64 output channels, which sit at head_coff of the head's
    input (unet.py:200-205: conv1_5 over cat1 = [upconv_4, conv1_2]).  Returns None when the kernel cannot take the
    case (the caller runs the unsplit path)."""
    n, h, w, _ = x.shape
    up = pc.up2x() if x.dtype == pc.dtype == torch.bfloat16 and pc.cout == 64 else None
    if up is None:
        return None
    if head_w.dtype != torch.float32 or not head_w.is_contiguous() or head_w.dim() != 4 or head_w.shape[3] != 1:
        raise ValueError("head_w must be a contiguous f32 [3,3,cin,1] filter")
    if partial.dtype != torch.float32 or not partial.is_contiguous() or tuple(partial.shape) != (n, 2 * h, 2 * w, 12):
        raise ValueError("partial must be a contiguous f32 [n,2h,2w,12] tensor")
    _require_gpu(head_w)
    _require_gpu(partial)
    if out is None:
        out = torch.empty((n, 2 * h, 2 * w, pc.cout), dtype=x.dtype, device=x.device)
    xv, yv = nhwc(x), nhwc(out)
    prof = _ConvProf()
    rc = lib().vm_conv3x3_up2x_head_nhwc(
        ctypes.byref(xv), _ptr(up), _ptr(pc.packed), pc.cin, pc.cout, _ptr(pc.bias), _ptr(pc.scale), _ptr(pc.shift),
        _lib.ACT[act], ctypes.byref(yv), _ptr(head_w), int(head_w.shape[2]), head_coff, _ptr(partial),
        int(bool(store_y)), stream_handle())
    if rc == _lib.VM_EUNSUPPORTED:
        return None
    check(rc, "conv3x3_up2x_head")
    prof.done(2 * n * 4 * h * w * 9 * pc.cin * pc.cout)
    return out


def head_from_partials(pa, pb, bias=None, logits=None, alpha=None):
    """conv1_5 + sigmoid from the two halves' per-tap partials (vm_conv3x3_head_from_partials): logits =
    bias + sum_tap (pa + pb)[p + off(tap)][tap], alpha = sigmoid(logits).  pa, pb: contiguous f32 [n,h,w,12]."""
    n, h, w, k = pa.shape
    if k != 12 or tuple(pb.shape) != (n, h, w, 12) or pa.dtype != torch.float32 or pb.dtype != torch.float32 \
            or not pa.is_contiguous() or not pb.is_contiguous():
        raise ValueError("pa, pb must be contiguous f32 [n,h,w,12] partials")
    _require_gpu(pa)
    _require_gpu(pb)
    if logits is None:
        logits = torch.empty((n, h, w, 1), dtype=torch.float32, device=pa.device)
    lv = nhwc(logits)
    if alpha is not None and (alpha.dtype != torch.float32 or not alpha.is_contiguous() or alpha.numel() != n * h * w):
        raise ValueError("alpha must be a contiguous f32 tensor of n*h*w values")
    prof = _ConvProf()
    check(lib().vm_conv3x3_head_from_partials(_ptr(pa), _ptr(pb), n, h, w, _ptr(bias), ctypes.byref(lv),
                                              _ptr(alpha), stream_handle()), "head_from_partials")
    prof.done(2 * n * h * w * 9 * 128)  # (its conv FLOPs were made in the two epilogues; listed for its time)
    return logits


# When a list, every conv launch appends (algorithmic FLOPs, kernel name, start_event, end_event[, (n, h, w, cin,
# cout)]) — HIP events on the launch stream, used by bench.py for the roofline's achieved TFLOP/s.
_CONV_PROFILE = None


class _ConvProf:
    """One conv launch's profile entry: create it right before the launch (records the start event when profiling is
    on), call ``done`` after a launch that ran (a fall-back after VM_EUNSUPPORTED appends nothing)."""

    def __init__(self):
        self.prof = _CONV_PROFILE
        if self.prof is not None:
            self.ev0 = torch.cuda.Event(enable_timing=True)
            self.ev1 = torch.cuda.Event(enable_timing=True)
            self.ev0.record()

    def done(self, flops, shape=None):
        if self.prof is not None:
            self.ev1.record()
            entry = (flops, _lib.last_conv_kernel(), self.ev0, self.ev1)
            self.prof.append(entry if shape is None else entry + (shape,))


def conv_profile(enable):
    global _CONV_PROFILE
    _CONV_PROFILE = [] if enable else None
    return _CONV_PROFILE


# ---------------------------------------------------------------------------------------------- memory-bound ops

def maxpool2x2(x, out=None):
    """tf.nn.max_pool 2x2/2 SAME."""
    n, h, w, c = x.shape
    if out is None:
        out = torch.empty((n, (h + 1) // 2, (w + 1) // 2, c), dtype=x.dtype, device=x.device)
    xv, yv = nhwc(x), nhwc(out)
    check(lib().vm_maxpool2x2_same_nhwc(ctypes.byref(xv), ctypes.byref(yv), stream_handle()), "maxpool2x2")
    return out


def widen(x, c):
    """The channel view ``x`` widened to ``c`` channels over the same storage: the zero pad channels of a padded
    buffer, read by a conv whose pack is channel-padded (UNetSimple.padded).  x's channel stride must cover c."""
    if x.shape[-1] == c:
        return x
    cs = x.stride(-2)
    if x.dim() != 4 or x.stride(-1) != 1 or (x.storage_offset() % cs) + c > cs:
        raise ValueError("widen: a [N,H,W,%d] view needs %d channels of stride, has %d" % (x.shape[-1], c, cs))
    return x.as_strided(tuple(x.shape[:-1]) + (c,), x.stride(), x.storage_offset())


def resize_bilinear(x, size, out=None):
    """tf.image.resize_images(x, size) with TF-1.x defaults (bilinear, legacy coordinates)."""
    n, h, w, c = x.shape
    oh, ow = int(size[0]), int(size[1])
    if out is None:
        out = torch.empty((n, oh, ow, c), dtype=x.dtype, device=x.device)
    xv, yv = nhwc(x), nhwc(out)
    check(lib().vm_resize_bilinear_tf1_nhwc(ctypes.byref(xv), ctypes.byref(yv), stream_handle()), "resize")
    return out


def convert(x, out, scale=None, shift=None, act="none"):
    """Copy x into out (dtype change, zero-filled extra channels, optional affine + activation)."""
    xv, yv = nhwc(x), nhwc(out)
    check(lib().vm_convert_nhwc(ctypes.byref(xv), ctypes.byref(yv), _ptr(_f32(scale)), _ptr(_f32(shift)),
                                _lib.ACT[act], stream_handle()), "convert")
    return out


_ws_cache = {}
_masked_streams = {}


_beside = {}


def _runs_beside(main, side, spin_us=1500):
    """True when a short kernel queued on ``side`` finishes while one queued before it on ``main`` still spins."""
    torch.cuda.synchronize(main.device)
    check(lib().vm_spin(spin_us, ctypes.c_void_p(main.cuda_stream)), "spin")
    e_main = torch.cuda.Event()
    e_main.record(main)
    check(lib().vm_spin(1, ctypes.c_void_p(side.cuda_stream)), "spin")
    e_side = torch.cuda.Event()
    e_side.record(side)
    beside = False
    while not e_main.query():
        if e_side.query():
            beside = True
            break
    torch.cuda.synchronize(main.device)
    return beside


def concurrent_streams(device, n, tries=16):
    """``n`` distinct pooled streams that each run beside the caller's current stream (as concurrent_stream; the
    candidates that share the caller's hardware queue are skipped), cached per (device, caller stream, n)."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    main = torch.cuda.current_stream(idx)
    key = (idx, main.cuda_stream, "n", n)
    got = _beside.get(key)
    if got is None:
        got, last = [], None
        for _ in range(tries):
            last = torch.cuda.Stream(device=torch.device("cuda", idx))
            if _runs_beside(main, last):
                got.append(last)
                if len(got) == n:
                    break
        while len(got) < n:  # (the probe kept failing: plain pool streams, slower at worst, never wrong)
            got.append(torch.cuda.Stream(device=torch.device("cuda", idx)))
        _beside[key] = got
    return list(got)


def concurrent_stream(device, tries=8):
    """A pooled torch stream that runs beside the caller's current stream of ``device``: a plain stream takes one of
    the process's hardware queues (GPU_MAX_HW_QUEUES) with no say in which, and on the caller's own queue a side
    stream's work is serialised behind the caller's (kernel traces).  Probed once per (device, current
    stream) with vm_spin; the chosen stream is cached and shared."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    main = torch.cuda.current_stream(idx)
    key = (idx, main.cuda_stream)
    s = _beside.get(key)
    if s is None:
        for _ in range(tries):
            s = torch.cuda.Stream(device=torch.device("cuda", idx))
            if _runs_beside(main, s):
                break
        _beside[key] = s  # (after `tries` misses: the last one; the step is then only slower, never wrong)
    return s


def side_stream(device, slot=0):
    """A CU-masked side stream of ``device`` (vm_stream_create_masked), one per ``slot``, created once per process and
    shared by the trainers that ask for that slot.  A plain torch stream takes one of the process's hardware queues
    without a say in which: a kernel trace caught a UNetImage trainer whose side stream sat on the caller's queue,
    serialising its filter gradients behind the data-gradient chain."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    s = _masked_streams.get((idx, slot))
    if s is None:
        ptr = ctypes.c_void_p()
        with torch.cuda.device(idx):
            check(lib().vm_stream_create_masked(ctypes.byref(ptr)), "stream_create_masked")
        s = torch.cuda.ExternalStream(ptr.value, device=torch.device("cuda", idx))
        _masked_streams[(idx, slot)] = s
    return s


def _workspace(nbytes, device):
    key = (str(device), _lib.current_raw_stream(device.index if isinstance(device, torch.device) else None))
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def bn_stats(x, mean=None, var=None):
    """Batch mean / biased variance over N,H,W (tf.contrib batch_norm, is_training=True)."""
    c = x.shape[-1]
    mean = torch.empty(c, dtype=torch.float32, device=x.device) if mean is None else mean
    var = torch.empty(c, dtype=torch.float32, device=x.device) if var is None else var
    xv = nhwc(x)
    ws = _workspace(lib().vm_bn_workspace_bytes(ctypes.byref(xv)), x.device)
    check(lib().vm_bn_stats_nhwc(ctypes.byref(xv), _ptr(mean), _ptr(var), _ptr(ws), stream_handle()), "bn_stats")
    return mean, var


def bn_apply(x, mean, var, gamma, beta, eps=1e-3, act="none", out=None):
    out = x if out is None else out
    xv, yv = nhwc(x), nhwc(out)
    check(lib().vm_bn_apply_nhwc(ctypes.byref(xv), ctypes.byref(yv), _ptr(mean), _ptr(var), _ptr(gamma),
                                 _ptr(beta), float(eps), _lib.ACT[act], stream_handle()), "bn_apply")
    return out


def softmax_lastdim(x, out=None):
    out = torch.empty_like(x) if out is None else out
    xv, yv = nhwc(x), nhwc(out)
    check(lib().vm_softmax_lastdim_nhwc(ctypes.byref(xv), ctypes.byref(yv), stream_handle()), "softmax")
    return out



def composite_image(fg, bg, alpha, out_dtype=torch.float64, out=None):
    """vm_composite_image: reader.create_composite_image (reader.py:72-79) on the device.

    fg, bg: [..., cn] uint8 / float32 / float64 (same dtype); alpha: [...] float32 / float64.  Computed in
    float64 like numpy; out_dtype float64 (bit-identical to the reference) or float32.
    """
    _require_gpu(fg)
    if bg.shape != fg.shape or bg.dtype != fg.dtype or bg.device != fg.device:
        raise ValueError("composite_image: fg and bg must have the same shape, dtype and device")
    if fg.dim() < 1 or tuple(alpha.shape) != tuple(fg.shape[:-1]):
        raise ValueError("composite_image: alpha must be fg.shape[:-1], got %s vs %s" % (tuple(alpha.shape), tuple(fg.shape)))
    if fg.dtype not in (torch.uint8, torch.float32, torch.float64) or alpha.dtype not in (torch.float32, torch.float64):
        raise TypeError("composite_image: u8/f32/f64 images and f32/f64 alpha expected")
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError("composite_image: out_dtype must be float32 or float64")
    fg, bg, alpha = fg.contiguous(), bg.contiguous(), alpha.contiguous()
    if out is None:
        out = torch.empty(fg.shape, dtype=out_dtype, device=fg.device)
    elif out.shape != fg.shape or out.dtype != out_dtype or not out.is_contiguous():
        raise ValueError("composite_image: out must be a contiguous %s tensor of fg's shape" % out_dtype)
    cn = fg.shape[-1]
    check(lib().vm_composite_image(_ptr(fg), _ptr(bg), _AUG_DT[fg.dtype], _ptr(alpha), _AUG_DT[alpha.dtype],
                                   fg.numel() // max(cn, 1), cn, _ptr(out), _AUG_DT[out_dtype], stream_handle()),
          "composite_image")
    return out


# ---------------------------------------------------------------------------------------------- flow

def remap_f32(img, flow, mode="opencv", out=None):
    """Backward warp of single-channel f32 frames: img [n?,ih,iw], flow [n?,h,w,2] -> [n?,h,w]."""
    _require_gpu(img)
    _require_gpu(flow)
    batched = flow.dim() == 4
    f = flow if batched else flow[None]
    im = img if img.dim() == 3 else img[None]
    n, h, w, two = f.shape
    if two != 2 or im.shape[0] != n:
        raise ValueError("flow must be [h,w,2] (or [n,h,w,2]) matching img frames")
    im = im.contiguous().float()
    f = f.contiguous().float()
    if out is None:
        out = torch.empty((n, h, w), dtype=torch.float32, device=img.device)
    check(lib().vm_remap_bilinear_f32(_ptr(im), im.shape[1], im.shape[2], _ptr(f), h, w, n, _ptr(out),
                                      0 if mode == "opencv" else 1, stream_handle()), "remap_f32")
    return out if batched else out[0]


def remap_u8(img, flow):
    _require_gpu(img)
    _require_gpu(flow)
    img = img.contiguous()
    ih, iw = img.shape[:2]
    cn = 1 if img.dim() == 2 else img.shape[2]
    h, w = flow.shape[:2]
    out = torch.empty((h, w) + (() if img.dim() == 2 else (cn,)), dtype=torch.uint8, device=img.device)
    f = flow.contiguous().float()
    check(lib().vm_remap_bilinear_u8(_ptr(img), ih, iw, cn, _ptr(f), h, w, _ptr(out), stream_handle()), "remap_u8")
    return out


def fb_consistency(backward, forward, alpha, thresh=15.0, promote="numpy1"):
    """flow.correct_alpha on device; alpha (f32 [h,w], contiguous) is modified in place."""
    for t in (backward, forward, alpha):
        _require_gpu(t)
    h, w = backward.shape[:2]
    if alpha.dtype != torch.float32 or not alpha.is_contiguous() or tuple(alpha.shape) != (h, w):
        raise ValueError("alpha must be a contiguous f32 [h,w] device tensor")
    bw = backward.contiguous().float()
    fw = forward.contiguous().float()
    err = torch.zeros(1, dtype=torch.int32, device=alpha.device)
    check(lib().vm_fb_consistency(_ptr(bw), _ptr(fw), h, w, _ptr(alpha), float(thresh),
                                  0 if promote == "numpy1" else 1, _ptr(err), stream_handle()), "fb_consistency")
    if int(err.item()) != 0:
        raise IndexError("correct_alpha: a backward-flow target lies more than one frame outside the image "
                         "(the reference's numpy IndexError, flow.py:46)")
    return alpha


def matting_loss(pred, gt, raw_fg, in_bg, in_cmp):
    """train.py:42-47 loss on device -> tensor [loss, alpha_loss, compositional_loss]."""
    ts = [t.contiguous().float() for t in (pred, gt, raw_fg, in_bg, in_cmp)]
    for t in ts:
        _require_gpu(t)
    pixels = ts[0].numel()
    out = torch.empty(3, dtype=torch.float32, device=pred.device)
    ws = _workspace(lib().vm_loss_workspace_bytes(pixels), pred.device)
    check(lib().vm_matting_loss(*[_ptr(t) for t in ts], pixels, _ptr(out), _ptr(ws), stream_handle()),
          "matting_loss")
    return out


# ---------------------------------------------------------------- augmentation row (tps.py / augmentation.py)

_AUG_DT = {torch.uint8: _lib.VM_U8, torch.float32: _lib.VM_F32, torch.float64: _lib.VM_F64}


def _dtype_code(t, what):
    if t.dtype not in _AUG_DT:
        raise TypeError("%s: unsupported dtype %s (uint8, float32, float64)" % (what, t.dtype))
    return _AUG_DT[t.dtype]


def tps_grid(points, coeffs, nx, ny, x_lo, x_step, y_lo, y_step, out=None):
    """vm_tps_grid: the TPS map evaluated on an nx x ny np.mgrid lattice -> f64 [2, nx, ny] on the device."""
    _require_gpu(points)
    _require_gpu(coeffs)
    p = points.contiguous().double()
    c = coeffs.contiguous().double()
    if p.dim() != 2 or p.shape[1] != 2 or c.shape != (p.shape[0] + 3, 2):
        raise ValueError("tps_grid: points [n,2] and coeffs [n+3,2], got %s %s" % (tuple(p.shape), tuple(c.shape)))
    if out is None:
        out = torch.empty((2, nx, ny), dtype=torch.float64, device=p.device)
    check(lib().vm_tps_grid(_ptr(p), _ptr(c), p.shape[0], nx, ny, float(x_lo), float(x_step), float(y_lo),
                            float(y_step), _ptr(out), stream_handle()), "tps_grid")
    return out


def tps_sample(grid, img, order=1, upsample=None, out=None):
    """vm_tps_sample: map_coordinates of img [ih, iw, cn] (u8/f32/f64) through the grid (or its upsampling:
    upsample = (x_steps, x_span, y_steps, y_span)) -> [oh, ow, cn] of img's dtype."""
    _require_gpu(grid)
    _require_gpu(img)
    img = img.contiguous()
    if img.dim() == 2:
        img = img[:, :, None]
    ih, iw, cn = img.shape
    nx, ny = grid.shape[1:]
    m = _lib.VmTpsMap()
    m.grid = _ptr(grid)
    m.nx, m.ny = nx, ny
    if upsample is None:
        m.upsample = 0
        oh, ow = nx, ny
    else:
        xs, xspan, ys, yspan = upsample
        m.upsample, m.x_steps, m.x_span, m.y_steps, m.y_span = 1, float(xs), int(xspan), float(ys), int(yspan)
        oh, ow = int(xspan) + 1, int(yspan) + 1
    if out is None:
        out = torch.empty((oh, ow, cn), dtype=img.dtype, device=img.device)
    check(lib().vm_tps_sample(ctypes.byref(m), _ptr(img), ih, iw, cn, _dtype_code(img, "tps_sample"), int(order),
                              _ptr(out), stream_handle()), "tps_sample")
    return out


def warp_affine(src, M, dsize, out=None):
    """vm_warp_affine: cv2.warpAffine(src, M, dsize=(w, h)), INTER_LINEAR, BORDER_CONSTANT 0."""
    _require_gpu(src)
    src = src.contiguous()
    two_d = src.dim() == 2
    ih, iw = src.shape[:2]
    cn = 1 if two_d else src.shape[2]
    w, h = int(dsize[0]), int(dsize[1])
    m = (ctypes.c_double * 6)(*[float(v) for v in np.asarray(M, np.float64).reshape(6)])
    if out is None:
        out = torch.empty((h, w) if two_d else (h, w, cn), dtype=src.dtype, device=src.device)
    check(lib().vm_warp_affine(_ptr(src), ih, iw, cn, _dtype_code(src, "warp_affine"), m, _ptr(out), h, w,
                               stream_handle()), "warp_affine")
    return out


def warp_image(src, tu, tv, M, dsize, lut=None, out=None):
    """vm_warp_image: augmentation.warp_image's translate + warpAffine pair (augmentation.py:59-63) in one pass,
    optionally followed by change_illumination with the S/V map ``lut`` (u8 BGR)."""
    _require_gpu(src)
    src = src.contiguous()
    two_d = src.dim() == 2
    ih, iw = src.shape[:2]
    cn = 1 if two_d else src.shape[2]
    w, h = int(dsize[0]), int(dsize[1])
    m = (ctypes.c_double * 6)(*[float(v) for v in np.asarray(M, np.float64).reshape(6)])
    lp = None
    if lut is not None:
        lut = np.ascontiguousarray(lut, np.uint8)
        if lut.shape != (256,):
            raise ValueError("warp_image: lut must have 256 entries")
        lp = lut.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    if out is None:
        out = torch.empty((h, w) if two_d else (h, w, cn), dtype=src.dtype, device=src.device)
    check(lib().vm_warp_image(_ptr(src), ih, iw, cn, _dtype_code(src, "warp_image"), int(tu), int(tv), m, lp,
                              _ptr(out), h, w, stream_handle()), "warp_image")
    return out


def change_illumination(bgr, lut, out=None):
    """vm_change_illumination_u8: BGR u8 -> HSV -> (h, lut[s], lut[v]) -> BGR u8."""
    _require_gpu(bgr)
    if bgr.dtype != torch.uint8 or bgr.shape[-1] != 3:
        raise TypeError("change_illumination: uint8 [..., 3] expected")
    bgr = bgr.contiguous()
    lut = np.ascontiguousarray(lut, np.uint8)
    if lut.shape != (256,):
        raise ValueError("change_illumination: lut must have 256 entries")
    if out is None:
        out = torch.empty_like(bgr)
    check(lib().vm_change_illumination_u8(_ptr(bgr), bgr.numel() // 3,
                                          lut.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), _ptr(out),
                                          stream_handle()), "change_illumination")
    return out


def bgra(fg, alpha, out=None):
    """vm_bgra_u8: concat(fg u8 [h, w, 3], uint8(255. * alpha [h, w] f64 / f32)) -> u8 [h, w, 4]."""
    _require_gpu(fg)
    _require_gpu(alpha)
    fg, alpha = fg.contiguous(), alpha.contiguous()
    h, w = fg.shape[:2]
    if fg.dtype != torch.uint8 or tuple(fg.shape) != (h, w, 3) or alpha.numel() != h * w:
        raise ValueError("bgra: fg u8 [h, w, 3] and alpha [h, w]")
    if out is None:
        out = torch.empty((h, w, 4), dtype=torch.uint8, device=fg.device)
    check(lib().vm_bgra_u8(_ptr(fg), _ptr(alpha), _dtype_code(alpha, "bgra"), h * w, _ptr(out), stream_handle()),
          "bgra")
    return out


def nonzero_stats(alpha, out=None):
    """vm_nonzero_stats: (count, row-index sum, column-index sum) of alpha != 0, int64[3] on the device."""
    _require_gpu(alpha)
    alpha = alpha.contiguous()
    if alpha.dim() != 2:
        raise ValueError("nonzero_stats: alpha must be [h, w]")
    if out is None:
        out = torch.empty(3, dtype=torch.int64, device=alpha.device)
    check(lib().vm_nonzero_stats(_ptr(alpha), alpha.shape[0], alpha.shape[1], _dtype_code(alpha, "nonzero_stats"),
                                 _ptr(out), stream_handle()), "nonzero_stats")
    return out


def trimap_from_matte(matte, dilate=1, crop=3, out=None):
    """vm_trimap_from_matte: data.trimap_from_matte on a float64 [h, w] device matte -> uint8 [h, w]."""
    _require_gpu(matte)
    if matte.dtype != torch.float64 or matte.dim() != 2:
        raise AssertionError("trimap_from_matte: float64 [h, w] matte expected (data.py:42)")
    matte = matte.contiguous()
    if out is None:
        out = torch.empty(matte.shape, dtype=torch.uint8, device=matte.device)
    check(lib().vm_trimap_from_matte(_ptr(matte), matte.shape[0], matte.shape[1], int(dilate), int(crop), _ptr(out),
                                     stream_handle()), "trimap_from_matte")
    return out


# ---------------------------------------------------------------- argument checks of the frame ops (host only)

def check_int(who, name, v, lo=None, hi=None):
    """``v``, a Python or numpy integer (no bool) within lo..hi, both ends included (None: open) -> int."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise TypeError("%s: %s must be an integer, got %r" % (who, name, v))
    if (lo is not None and v < lo) or (hi is not None and v > hi):
        want = "at least %d" % lo if hi is None else "at most %d" % hi if lo is None else "in %d..%d" % (lo, hi)
        raise ValueError("%s: %s must be %s, got %d" % (who, name, want, v))
    return int(v)


@functools.lru_cache(maxsize=None)
def _parse_shapes(shapes):
    """"n,h,w | n,h,w,1" -> (("n", "h", "w"), ("n", "h", "w", 1))."""
    return tuple(tuple(int(d) if d.isdigit() else d for d in s.strip().split(",")) for s in shapes.split("|"))


def _match_shape(who, name, shape, shapes, dims):
    """``shape`` is one of ``shapes`` -> that shape, as ints; a ValueError otherwise.  ``shapes``: alternatives like
    "n,h,w | n,h,w,1"; a number stands for itself, a letter for the size ``dims`` gives it or, where it gives none, for
    any size >= 1."""
    shape = tuple(int(v) for v in shape)
    for spec in _parse_shapes(shapes):
        if len(spec) == len(shape) and all(v == dims[d] if d in dims else v >= 1 if isinstance(d, str) else v == d
                                           for v, d in zip(shape, spec)):
            return shape
    sizes = ", ".join("%s=%d" % kv for kv in dims.items())
    raise ValueError("%s: %s must be %s%s, got %s" % (who, name, " or ".join("[%s]" % s.strip() for s in
                                                                             shapes.split("|")),
                                                      " with " + sizes if sizes else "", shape))


def _check_tensor(who, name, t, dtypes, shapes, wrong=TypeError, **dims):
    """``t`` is a contiguous torch tensor of one of ``dtypes`` whose shape is one of ``shapes`` (_match_shape's grammar)
    -> that shape, as ints.  ``wrong``: what a non-tensor or another dtype raises; a shape or strides raise ValueError.
    The device is never looked at: _require_gpu is every op's last check."""
    if not isinstance(t, torch.Tensor):
        raise wrong("%s: %s must be a torch tensor, got %s" % (who, name, type(t).__name__))
    if t.dtype not in dtypes:
        raise wrong("%s: %s must be %s, got %s" % (who, name, " or ".join(str(d) for d in dtypes), t.dtype))
    shape = _match_shape(who, name, t.shape, shapes, dims)
    if not t.is_contiguous():
        raise ValueError("%s: %s must be contiguous" % (who, name))
    return shape


# what the layer above the ops takes from its callers: host arrays, device tensors, or either
NUMPY, DEVICE, EITHER = "a numpy array", "a ROCm device tensor", "a numpy array or a ROCm device tensor"
NUMPY_DTYPES = {np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32,
                np.dtype(np.float64): torch.float64}  # the one numpy -> torch dtype table


def torch_dtype(a):
    """The torch dtype of a tensor or a numpy array (a numpy dtype without a torch twin here stays what it is)."""
    return a.dtype if isinstance(a, torch.Tensor) else NUMPY_DTYPES.get(a.dtype, a.dtype)


def check_array(who, name, a, dtypes, shapes, accept=NUMPY, wrong=TypeError, strided=False, **dims):
    """_check_tensor's sibling for the streams and conveniences: ``a`` is what ``accept`` names (NUMPY, DEVICE or
    EITHER), of one of the torch ``dtypes`` (torch_dtype) and one of ``shapes`` (_match_shape's grammar) -> that shape,
    as ints.  ``wrong``: what another type, another dtype and a tensor on the host raise; a shape or a tensor's strides
    raise ValueError.  ``strided``: the consumer copies the tensor, so any strides are taken (a numpy array's always
    are: it is staged or uploaded).  A tensor's device is looked at last, so every other fault shows without one."""
    tensor = isinstance(a, torch.Tensor)
    if not (tensor and accept != NUMPY or isinstance(a, np.ndarray) and accept != DEVICE):
        raise wrong("%s: %s must be %s, got %s" % (who, name, accept, type(a).__name__))
    if torch_dtype(a) not in dtypes:
        raise wrong("%s: %s must be %s, got %s" % (who, name, " or ".join(str(d) for d in dtypes), a.dtype))
    shape = _match_shape(who, name, a.shape, shapes, dims)
    if tensor and not strided and not a.is_contiguous():
        raise ValueError("%s: %s must be contiguous" % (who, name))
    if tensor and not a.is_cuda:
        raise wrong("%s: %s is a host tensor; pass %s" % (who, name, accept))
    return shape


def _out_or_new(who, name, t, dtype, shapes, device, wrong=TypeError, **dims):
    """A caller's result tensor, checked as _check_tensor does, or a new one of the first of ``shapes`` (whose letters
    ``dims`` all gives) on ``device``."""
    if t is None:
        return torch.empty(tuple(dims.get(d, d) for d in _parse_shapes(shapes)[0]), dtype=dtype, device=device)
    _check_tensor(who, name, t, (dtype,), shapes, wrong, **dims)
    return t


def _buffer_or_new(who, name, t, dtype, numel, device):
    """A caller's contiguous device buffer of at least ``numel`` elements (a workspace, a pyramid), or a new one.  Its
    size is the library's to tell, so this comes after the inputs' _require_gpu."""
    if t is None:
        return torch.empty(numel, dtype=dtype, device=device)
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.numel() < numel or not t.is_contiguous():
        raise ValueError("%s: %s must be a contiguous %s tensor of at least %d elements" % (who, name, dtype, numel))
    _require_gpu(t)
    return t


def _check_frames_and_bg(who, cmp, bg):
    """Decoded frames as contiguous torch tensors: cmp u8 [n,h,w,3], bg u8 [n,h,w,3] or one plate -> (n, h, w, nb)."""
    n, h, w, _ = _check_tensor(who, "cmp", cmp, (torch.uint8,), "n,h,w,3")
    shape = _check_tensor(who, "bg", bg, (torch.uint8,), "n,h,w,3 | 1,h,w,3 | h,w,3", n=n, h=h, w=w)
    return n, h, w, (n if shape == (n, h, w, 3) else 1)


def _options(who, defaults, options, check, *args):
    """A family's options: ``options`` (a dict, or None) over ``defaults``, through the family's
    ``check(who, *args, **options)`` (-> the checked values in the defaults' key order) -> a dict in that order.  An
    unknown key is a ValueError."""
    opts = dict(defaults)
    for k, v in dict(options or {}).items():
        if k not in opts:
            raise ValueError("%s takes %s, got %r" % (who, sorted(opts), k))
        opts[k] = v
    return dict(zip(defaults, check(who, *args, **opts)))


# ---------------------------------------------------------------- inference on a decoded clip

def frame_buffer(model, n, h, w, native=None):
    """An [n,h,w,IN_CH] input-frame buffer for ``model``: ``native`` (default: a plain bf16 model) gives bf16 pixels 8
    channels wide, the pad zeroed once, which the forward reads in place; otherwise f32."""
    if native is None:
        native = not model.x6mode and model.dtype == torch.bfloat16
    if native:
        return torch.zeros((n, h, w, 8), dtype=torch.bfloat16, device=model.device)[..., :model.IN_CH]
    return torch.empty((n, h, w, model.IN_CH), dtype=torch.float32, device=model.device)


def frames_from_u8(cmp, bg, trimap=None, out=None, dtype=torch.float32):
    """vm_frames_from_u8: decoded uint8 frames -> the network input in one pass.  cmp u8 [n,h,w,3] BGR, bg u8
    [n,h,w,3] or one static plate [h,w,3] / [1,h,w,3], trimap u8 [n,h,w] or None -> ``out`` [n,h,w,C] (C = 7 with a
    trimap, 6 without): channels = f32((double)u - VGG_MEAN) and f32((double)u / 255 - .5) as the reference feeds them.
    ``out``: an f32 NHWC view (dense or a channel slice), or the [..., :C] view of a bf16 [n,h,w,8] buffer (whose
    channels C..7 are zeroed); allocated in ``dtype`` when None."""
    who = "frames_from_u8"
    n, h, w, nb = _check_frames_and_bg(who, cmp, bg)
    if trimap is not None:
        _check_tensor(who, "trimap", trimap, (torch.uint8,), "n,h,w", n=n, h=h, w=w)
    c = 6 if trimap is None else 7
    if out is None and dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("frames_from_u8: f32 or bf16 output, got %s" % dtype)
    if out is not None and tuple(out.shape) != (n, h, w, c):
        raise ValueError("frames_from_u8: out must be [n,h,w,%d] = %s, got %s" % (c, (n, h, w, c), tuple(out.shape)))
    for t in (cmp, bg, trimap):
        if t is not None:
            _require_gpu(t)
    if out is None:
        out = torch.empty((n, h, w, 8 if dtype == torch.bfloat16 else c), dtype=dtype, device=cmp.device)[..., :c]
    ov = nhwc(out)
    check(lib().vm_frames_from_u8(_ptr(cmp), _ptr(bg), _ptr(trimap), nb, ctypes.byref(ov), stream_handle()),
          "frames_from_u8")
    return out


def matte_quantize(alpha, out=None, bits=8):
    """vm_matte_quantize: f32 alpha (any shape, contiguous) -> uint8 (bits 8) or uint16 (bits 16) of the same shape:
    min(max(rint(alpha * M), 0), M), M = 255 / 65535, ties to even, NaN -> 0."""
    if bits not in (8, 16):
        raise ValueError("matte_quantize: bits 8 or 16, got %r" % (bits,))
    qt = torch.uint8 if bits == 8 else torch.uint16
    if isinstance(alpha, torch.Tensor) and (alpha.dtype != torch.float32 or not alpha.is_contiguous()):
        raise ValueError("matte_quantize: contiguous f32 alpha expected")
    _require_gpu(alpha)
    if out is None:
        out = torch.empty(alpha.shape, dtype=qt, device=alpha.device)
    _require_gpu(out)
    if out.dtype != qt or out.numel() != alpha.numel() or not out.is_contiguous():
        raise ValueError("matte_quantize: out must be a contiguous %s tensor of %d elements" % (qt, alpha.numel()))
    if alpha.numel():
        check(lib().vm_matte_quantize(_ptr(alpha), alpha.numel(), bits, _ptr(out), stream_handle()), "matte_quantize")
    return out


COMPOSE_MODES = {"over": _lib.VM_COMPOSE_OVER, "bgra": _lib.VM_COMPOSE_STRAIGHT, "premul": _lib.VM_COMPOSE_PREMUL}


def matte_compose(alpha, cmp, bg, new_bg=None, mode="over", out=None):
    """vm_matte_compose: the matte applied, with the known background.  alpha f32 [n,h,w] or [n,h,w,1], cmp u8
    [n,h,w,3] BGR, bg u8 [n,h,w,3] or one plate [h,w,3] / [1,h,w,3]; all contiguous.  mode "over": the frame over
    ``new_bg`` (u8, shaped like bg), cmp + (1 - alpha)(new_bg - bg) -> u8 [n,h,w,3]; "bgra" / "premul": the straight /
    premultiplied foreground layer with the 8-bit matte of matte_quantize as its alpha -> u8 [n,h,w,4] BGRA (no
    ``new_bg``).  float64 arithmetic, one rounding (include/vmatting.h)."""
    if mode not in COMPOSE_MODES:
        raise ValueError("matte_compose: mode must be one of %s, got %r" % (sorted(COMPOSE_MODES), mode))
    over = mode == "over"
    if over and new_bg is None:
        raise ValueError("matte_compose: mode 'over' needs new_bg")
    if not over and new_bg is not None:
        raise ValueError("matte_compose: mode %r takes no new_bg" % mode)
    who = "matte_compose"
    n, h, w, nb = _check_frames_and_bg(who, cmp, bg)
    _check_tensor(who, "alpha", alpha, (torch.float32,), "n,h,w | n,h,w,1", n=n, h=h, w=w)
    nn = 0
    if over:
        shape = _check_tensor(who, "new_bg", new_bg, (torch.uint8,), "n,h,w,3 | 1,h,w,3 | h,w,3", n=n, h=h, w=w)
        nn = n if shape == (n, h, w, 3) else 1
    out = _out_or_new(who, "out", out, torch.uint8, "n,h,w,c", cmp.device, ValueError, n=n, h=h, w=w, c=3 if over else 4)
    for t in (alpha, cmp, bg, new_bg, out):
        if t is not None:
            _require_gpu(t)
    check(lib().vm_matte_compose(_ptr(alpha), _ptr(cmp), _ptr(bg), nb, _ptr(new_bg), nn, n, h, w, COMPOSE_MODES[mode],
                                 _ptr(out), stream_handle()), "matte_compose")
    return out


def clip_feed(cmp, bg, prev_alpha, backward, forward=None, thresh=15.0, promote="numpy1", towers=None, cat=None,
              warped=None, err=None):
    """vm_clip_feed: the video model's feed in one pass.  cmp u8 [n,h,w,3] BGR, bg u8 [n,h,w,3] or one plate [h,w,3] /
    [1,h,w,3], prev_alpha f32 [n,h,w] (or [n,h,w,1]), backward / forward f32 [n,h,w,2] (forward None: warp only) ->
    ``towers`` (the [3n,h,w,3] view of a [3n,h,w,8] buffer: cmp, bg and [a,a,a] frames, a = warp_img(prev_alpha,
    backward) [corrected by correct_alpha]) and ``cat`` (the [n,h,w,9] view of a buffer >= 16 channels wide), both in
    the model's dtype — UNetSimple.feed_views returns the pair; ``warped`` f32 [n,h,w] optionally receives a.
    With a forward flow, ``err`` (int32 [1], zeroed by the caller) is set where the reference raises IndexError; when
    ``err`` is None the call keeps a flag of its own, waits for it and raises IndexError itself.  Returns warped."""
    who = "clip_feed"
    n, h, w, nb = _check_frames_and_bg(who, cmp, bg)
    if promote not in ("numpy1", "numpy2"):
        raise ValueError("clip_feed: promote must be 'numpy1' or 'numpy2', got %r" % (promote,))
    for name, t, shapes in (("prev_alpha", prev_alpha, "n,h,w | n,h,w,1"), ("backward", backward, "n,h,w,2"),
                            ("forward", forward, "n,h,w,2"), ("warped", warped, "n,h,w | n,h,w,1")):
        if t is not None or name in ("prev_alpha", "backward"):
            _check_tensor(who, name, t, (torch.float32,), shapes, n=n, h=h, w=w)
    if towers is None or cat is None:
        raise ValueError("clip_feed: towers and cat views are required (UNetSimple.feed_views)")
    if tuple(towers.shape) != (3 * n, h, w, 3) or tuple(cat.shape) != (n, h, w, 9):
        raise ValueError("clip_feed: towers must be %s and cat %s, got %s and %s" %
                         ((3 * n, h, w, 3), (n, h, w, 9), tuple(towers.shape), tuple(cat.shape)))
    if towers.dtype != cat.dtype or cat.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("clip_feed: towers and cat are both f32 or both bf16, got %s and %s" % (towers.dtype, cat.dtype))
    if err is not None and (not isinstance(err, torch.Tensor) or err.dtype != torch.int32 or err.numel() != 1):
        raise TypeError("clip_feed: err must be an int32 tensor of one element")
    for t in (cmp, bg, prev_alpha, backward, forward, towers, cat, warped, err):
        if t is not None:
            _require_gpu(t)
    own = forward is not None and err is None
    if own:
        err = torch.zeros(1, dtype=torch.int32, device=cmp.device)
    tv, cv = nhwc(towers), nhwc(cat)
    check(lib().vm_clip_feed(_ptr(cmp), _ptr(bg), nb, _ptr(prev_alpha), _ptr(backward), _ptr(forward), float(thresh),
                             0 if promote == "numpy1" else 1, ctypes.byref(tv), ctypes.byref(cv), _ptr(warped),
                             _ptr(err), stream_handle()), "clip_feed")
    if own and int(err.item()) != 0:
        raise IndexError("clip_feed: a backward-flow target lies more than one frame outside the image "
                         "(the reference's numpy IndexError, flow.py:46)")
    return warped


# ---------------------------------------------------------------- optical flow between two decoded frames

FLOW_DEFAULTS = {"levels": 6, "warps": 3, "iters": 20, "alpha": 15.0}
FLOW_MODES = ("given", "estimate")  # where a stream's flows come from: its source's items, or its frames


def check_flow_options(who, h, w, levels=6, warps=3, iters=20, alpha=15.0):
    """The estimator's shape and options as vm_flow_estimate checks them, on the host -> (levels, warps, iters,
    alpha)."""
    levels, warps, iters = (check_int(who, name, v, 1) for name, v in (("levels", levels), ("warps", warps),
                                                                       ("iters", iters)))
    alpha = float(alpha)
    if not alpha > 0.0:
        raise ValueError("%s: alpha must be a positive number, got %r" % (who, alpha))
    if h < 16 or w < 16:
        raise ValueError("%s: frames of at least 16 x 16, got %d x %d" % (who, h, w))
    return levels, warps, iters, alpha


def flow_options(who, h, w, options):
    """A dict over FLOW_DEFAULTS (None: the defaults), checked for [h,w] frames -> {"levels": ..., "warps": ...,
    "iters": ..., "alpha": ...}."""
    return _options(who, FLOW_DEFAULTS, options, check_flow_options, h, w)


def check_flow_mode(who, flow, options, h, w, modes=FLOW_MODES, default=None):
    """The ``flow`` argument of FrameStream, ClipStream and MatteScorer: one of the ``modes`` this caller allows (None,
    where allowed, stands for ``default``), and their ``flow_options`` (a dict over FLOW_DEFAULTS) only with "estimate"
    -> the options checked for [h,w] frames, or None in every other mode."""
    if flow not in modes:
        raise ValueError("%s: flow must be one of %s, got %r" % (who, list(modes), flow))
    if (default if flow is None else flow) != "estimate":
        if options is not None:
            raise ValueError("%s: flow_options go with flow='estimate'" % who)
        return None
    return flow_options("%s: flow_options" % who, h, w, options)


def flow_workspace_bytes(h, w, levels=6):
    return lib().vm_flow_estimate_workspace_bytes(h, w, levels)


def flow_pyramid_floats(h, w, levels=6):
    return lib().vm_flow_pyramid_bytes(h, w, levels) // 4


def flow_pyramid(frame, levels=6, out=None, work=None):
    """vm_flow_pyramid: the smoothed grey pyramid of one uint8 [h,w,3] BGR frame -> f32 [flow_pyramid_floats(h, w,
    levels)], the levels finest first, each level's start padded to 4 floats."""
    who = "flow_pyramid"
    h, w, _ = _check_tensor(who, "frame", frame, (torch.uint8,), "h,w,3")
    levels = check_flow_options(who, h, w, levels)[0]
    _require_gpu(frame)
    out = _buffer_or_new(who, "out", out, torch.float32, flow_pyramid_floats(h, w, levels), frame.device)
    work = _buffer_or_new(who, "work", work, torch.uint8, flow_workspace_bytes(h, w, levels), frame.device)
    check(lib().vm_flow_pyramid(_ptr(frame), h, w, levels, _ptr(out), _ptr(work), stream_handle()), who)
    return out


def flow_from_pyramids(cur, prev, h, w, levels=6, warps=3, iters=20, alpha=15.0, out=None, work=None):
    """vm_flow_from_pyramids: the flow of estimate_flow from two flow_pyramid results of [h,w] frames."""
    who = "flow_from_pyramids"
    levels, warps, iters, alpha = check_flow_options(who, h, w, levels, warps, iters, alpha)
    for t in (cur, prev):  # (buffers whose size is the library's to tell: the device first)
        _require_gpu(t)
    n = flow_pyramid_floats(h, w, levels)
    cur = _buffer_or_new(who, "cur", cur, torch.float32, n, cur.device)
    prev = _buffer_or_new(who, "prev", prev, torch.float32, n, cur.device)
    out = _out_or_new(who, "out", out, torch.float32, "h,w,2", cur.device, ValueError, h=h, w=w)
    _require_gpu(out)
    work = _buffer_or_new(who, "work", work, torch.uint8, flow_workspace_bytes(h, w, levels), cur.device)
    check(lib().vm_flow_from_pyramids(_ptr(cur), _ptr(prev), h, w, levels, warps, iters, alpha, _ptr(out), _ptr(work),
                                      stream_handle()), who)
    return out


def estimate_flow(cur_u8, prev_u8, levels=6, warps=3, iters=20, alpha=15.0, out=None, work=None):
    """vm_flow_estimate: the dense flow f between two uint8 [h,w,3] BGR frames with cur(x, y) ~ prev(x + f[...,0],
    y + f[...,1]) -> f32 [h,w,2] in reader.read_flow layout: the backward flow warp_img / clip_feed consume (the
    forward flow is estimate_flow(prev, cur)).  Coarse-to-fine Horn-Schunck with warping, f32 (include/vmatting.h).
    ``out``: a contiguous f32 [h,w,2] device tensor; ``work``: a uint8 device buffer of flow_workspace_bytes(h, w,
    levels); both are allocated when None."""
    who = "estimate_flow"
    h, w, _ = _check_tensor(who, "cur", cur_u8, (torch.uint8,), "h,w,3")
    _check_tensor(who, "prev", prev_u8, (torch.uint8,), "h,w,3", h=h, w=w)
    levels, warps, iters, alpha = check_flow_options(who, h, w, levels, warps, iters, alpha)
    out = _out_or_new(who, "out", out, torch.float32, "h,w,2", cur_u8.device, ValueError, h=h, w=w)
    for t in (cur_u8, prev_u8, out):
        _require_gpu(t)
    work = _buffer_or_new(who, "work", work, torch.uint8, flow_workspace_bytes(h, w, levels), cur_u8.device)
    check(lib().vm_flow_estimate(_ptr(cur_u8), _ptr(prev_u8), h, w, levels, warps, iters, alpha, _ptr(out), _ptr(work),
                                 stream_handle()), who)
    return out


# ---------------------------------------------------------------- trimap propagation by optical flow

GROW_MAX = 8


def check_grow(who, grow):
    """``grow`` as vm_trimap_propagate checks it, on the host: an integer in 0..8."""
    return check_int(who, "grow", grow, 0, GROW_MAX)


def trimap_propagate_workspace_bytes(h, w, grow):
    return lib().vm_trimap_propagate_workspace_bytes(h, w, grow)


def trimap_propagate(prev, flow, grow=1, out=None, work=None):
    """vm_trimap_propagate: the trimap of the next frame from ``prev`` (uint8 [h,w]: 255 foreground, 0 background,
    anything else unknown) and that frame's backward flow (f32 [h,w,2], reader.read_flow layout, as estimate_flow
    returns it) -> uint8 [h,w] of 0 / 128 / 255.  A label survives where every pixel of prev the bilinear warp would
    touch, and every pixel within ``grow`` (0..8) of those, carries it (include/vmatting.h).  ``out``: a contiguous
    uint8 [h,w] device tensor that is not ``prev``; ``work``: a uint8 device buffer of
    trimap_propagate_workspace_bytes(h, w, grow); both are allocated when None."""
    who = "trimap_propagate"
    h, w = _check_tensor(who, "prev", prev, (torch.uint8,), "h,w")
    _check_tensor(who, "flow", flow, (torch.float32,), "h,w,2", h=h, w=w)
    grow = check_int(who, "grow", grow)  # (its range is the library's check: the size query gives 0 outside it)
    out = _out_or_new(who, "out", out, torch.uint8, "h,w", prev.device, ValueError, h=h, w=w)
    for t in (prev, flow, out):
        _require_gpu(t)
    work = _buffer_or_new(who, "work", work, torch.uint8, trimap_propagate_workspace_bytes(h, w, grow), prev.device)
    check(lib().vm_trimap_propagate(_ptr(prev), _ptr(flow), h, w, grow, _ptr(out), _ptr(work), stream_handle()), who)
    return out


# ---------------------------------------------------------------- trimaps from the background plate

# colour distances in levels and erosion radii in pixels; untuned on real footage
PLATE_DEFAULTS = {"lo": 16, "hi": 48, "r_bg": 4, "r_fg": 8}
PLATE_LEVEL_MAX, PLATE_RADIUS_MAX = 442, 32


def check_plate_options(who, lo, hi, r_bg, r_fg):
    """The options of vm_trimap_from_plate as it checks them, on the host: integers with 0 <= lo < hi <= 442 and radii
    in 0..32 -> (lo, hi, r_bg, r_fg)."""
    lo, hi, r_bg, r_fg = (check_int(who, name, v) for name, v in (("lo", lo), ("hi", hi), ("r_bg", r_bg), ("r_fg", r_fg)))
    if not 0 <= lo < hi <= PLATE_LEVEL_MAX:
        raise ValueError("%s: 0 <= lo < hi <= %d expected, got lo %d, hi %d" % (who, PLATE_LEVEL_MAX, lo, hi))
    for name, v in (("r_bg", r_bg), ("r_fg", r_fg)):
        check_int(who, name, v, 0, PLATE_RADIUS_MAX)
    return lo, hi, r_bg, r_fg


def plate_options(who, options):
    """A dict over PLATE_DEFAULTS (None: the defaults), checked -> {"lo": lo, "hi": hi, "r_bg": r_bg, "r_fg": r_fg}."""
    return _options(who, PLATE_DEFAULTS, options, check_plate_options)


def trimap_from_plate_workspace_bytes(n, h, w):
    return lib().vm_trimap_from_plate_workspace_bytes(n, h, w)


# the shadow-tolerant distance (vm_trimap_from_plate_shadow): light ratios in 1/256 and a level; a numpy prototype's
# values, untuned on real footage
SHADOW_DEFAULTS = {"floor": 128, "ceil": 256, "dark": 32}
SHADOW_ONE = 256


def check_shadow_options(who, floor=SHADOW_DEFAULTS["floor"], ceil=SHADOW_DEFAULTS["ceil"],
                         dark=SHADOW_DEFAULTS["dark"]):
    """The options of vm_trimap_from_plate_shadow as it checks them, on the host: integers, floor in 1..256, ceil in
    256..512 (so floor <= ceil) and dark in 0..255 -> (floor, ceil, dark)."""
    floor, ceil = check_int(who, "floor", floor), check_int(who, "ceil", ceil)
    dark = check_int(who, "dark", dark, 0, 255)
    if floor > ceil:
        raise ValueError("%s: floor <= ceil expected, got floor %d, ceil %d" % (who, floor, ceil))
    return check_int(who, "floor", floor, 1, SHADOW_ONE), check_int(who, "ceil", ceil, SHADOW_ONE, 2 * SHADOW_ONE), dark


def shadow_options(who, options):
    """A dict over SHADOW_DEFAULTS (None: the defaults), checked -> {"floor": floor, "ceil": ceil, "dark": dark}."""
    return _options(who, SHADOW_DEFAULTS, options, check_shadow_options)


SHADOW_CHROMA = "chroma"


def check_shadow_mode(who, shadow, options):
    """The ``shadow`` argument of FrameStream and reader.trimap_from_plate: None or "chroma", and their
    ``shadow_options`` (a dict over SHADOW_DEFAULTS) only with "chroma" -> the checked options, or None without it."""
    if shadow is not None and not (isinstance(shadow, str) and shadow == SHADOW_CHROMA):
        raise ValueError("%s: shadow must be None or %r, got %r" % (who, SHADOW_CHROMA, shadow))
    if shadow is None:
        if options is not None:
            raise ValueError("%s: shadow_options go with shadow=%r" % (who, SHADOW_CHROMA))
        return None
    return shadow_options("%s: shadow_options" % who, options)


def trimap_from_plate(cmp, bg, lo=PLATE_DEFAULTS["lo"], hi=PLATE_DEFAULTS["hi"], r_bg=PLATE_DEFAULTS["r_bg"],
                      r_fg=PLATE_DEFAULTS["r_fg"], out=None, work=None, shadow=None):
    """vm_trimap_from_plate: trimaps from the frames' difference to the background.  cmp u8 [n,h,w,3] BGR, bg u8
    [n,h,w,3] or one static plate [h,w,3] / [1,h,w,3] -> uint8 [n,h,w]: 0 where the 3x3 box sum of the squared colour
    distance stays within 9 lo^2 over a (2 r_bg + 1)^2 window, 255 where it reaches 9 hi^2 over a (2 r_fg + 1)^2 window,
    128 elsewhere (include/vmatting.h).  ``out``: a contiguous uint8 [n,h,w] device tensor; ``work``: a uint8 device
    buffer of trimap_from_plate_workspace_bytes(n, h, w); both are allocated when None.  ``shadow``: None, or a dict
    over SHADOW_DEFAULTS for vm_trimap_from_plate_shadow: where the frame's pixel is the plate's colour under a light
    ratio within floor / 256 .. ceil / 256, and the plate is no darker than ``dark``, the squared distance to the line
    through the plate's colour stands for the squared distance to the plate (a per-pixel colour test: a subject that
    is a darker version of the plate's own hue passes as shadow)."""
    who = "trimap_from_plate"
    n, h, w, nb = _check_frames_and_bg(who, cmp, bg)
    lo, hi, r_bg, r_fg = check_plate_options(who, lo, hi, r_bg, r_fg)
    if shadow is not None:
        shadow = shadow_options("%s: shadow" % who, shadow)
    out = _out_or_new(who, "out", out, torch.uint8, "n,h,w", cmp.device, ValueError, n=n, h=h, w=w)
    for t in (cmp, bg, out):
        _require_gpu(t)
    work = _buffer_or_new(who, "work", work, torch.uint8, trimap_from_plate_workspace_bytes(n, h, w), cmp.device)
    if shadow is None:
        check(lib().vm_trimap_from_plate(_ptr(cmp), _ptr(bg), nb, n, h, w, lo, hi, r_bg, r_fg, _ptr(out), _ptr(work),
                                         stream_handle()), who)
    else:
        check(lib().vm_trimap_from_plate_shadow(_ptr(cmp), _ptr(bg), nb, n, h, w, lo, hi, r_bg, r_fg, shadow["floor"],
                                                shadow["ceil"], shadow["dark"], _ptr(out), _ptr(work),
                                                stream_handle()), who)
    return out


# ---------------------------------------------------------------- connected components, and enclosed background

def label_components(mask, value=0, connectivity=4, out=None):
    """vm_components_label: the connected components of the pixels of ``mask`` (uint8 [n,h,w]) whose byte equals
    ``value`` -> int32 [n,h,w]: for such a pixel the smallest row-major index y * w + x, within its own frame, of its 4-
    or 8-connected component; -1 for every other pixel (include/vmatting.h).  ``out``: a contiguous int32 [n,h,w] device
    tensor, allocated when None."""
    who = "label_components"
    n, h, w = _check_tensor(who, "mask", mask, (torch.uint8,), "n,h,w")
    value, connectivity = check_int(who, "value", value, 0, 255), check_int(who, "connectivity", connectivity)
    if connectivity not in (4, 8):
        raise ValueError("%s: connectivity must be 4 or 8, got %d" % (who, connectivity))
    out = _out_or_new(who, "out", out, torch.int32, "n,h,w", mask.device, ValueError, n=n, h=h, w=w)
    for t in (mask, out):
        _require_gpu(t)
    check(lib().vm_components_label(_ptr(mask), n, h, w, value, connectivity, _ptr(out), stream_handle()), who)
    return out


def check_fill(who, fill):
    """The hole-filling option of the automatic trimap -> None (off: None or False) or the area cap handed to
    vm_trimap_fill_enclosed: 0 (True: any area) or an integer >= 1."""
    if fill is None or fill is False:
        return None
    if fill is True:
        return 0
    try:
        return check_int(who, "fill", fill, 1)
    except (TypeError, ValueError):
        raise ValueError("%s: fill is None / False (off), True (any area) or an integer area cap >= 1, got %r" %
                         (who, fill)) from None


def trimap_fill_enclosed_workspace_bytes(n, h, w):
    return lib().vm_trimap_fill_enclosed_workspace_bytes(n, h, w)


def trimap_fill_enclosed(trimap, max_area=0, out=None, work=None):
    """vm_trimap_fill_enclosed: trimap uint8 [n,h,w] -> uint8 [n,h,w] with 128 on every 4-connected component of zero
    bytes that does not touch the frame's border and has at most ``max_area`` pixels (0: any area); every other byte is
    copied (include/vmatting.h).  ``out``: a contiguous uint8 [n,h,w] device tensor, allocated when None; ``trimap``
    itself fills in place.  ``work``: a uint8 device buffer of trimap_fill_enclosed_workspace_bytes(n, h, w), allocated
    when None."""
    who = "trimap_fill_enclosed"
    n, h, w = _check_tensor(who, "trimap", trimap, (torch.uint8,), "n,h,w")
    max_area = check_int(who, "max_area", max_area, 0)
    out = _out_or_new(who, "out", out, torch.uint8, "n,h,w", trimap.device, ValueError, n=n, h=h, w=w)
    for t in (trimap, out):
        _require_gpu(t)
    work = _buffer_or_new(who, "work", work, torch.uint8, trimap_fill_enclosed_workspace_bytes(n, h, w), trimap.device)
    check(lib().vm_trimap_fill_enclosed(_ptr(trimap), n, h, w, max_area, _ptr(out), _ptr(work), stream_handle()), who)
    return out


# ---------------------------------------------------------------- the background plate from the clip itself

PLATE_MAX_SAMPLES = 64


def plate_from_samples(samples, plate=None, spread=None, want_spread=True):
    """vm_plate_from_samples: the background plate of a locked-off shot from n of its frames.  samples u8 [n,h,w,3],
    contiguous, 1 <= n <= 64 -> (plate u8 [h,w,3], spread u8 [h,w]): per byte the lower median over the samples
    (np.sort(samples, 0)[(n - 1) // 2]), and per pixel the largest interquantile range of its three bytes, which is
    large where the plate is not to be trusted (include/vmatting.h).  ``plate`` / ``spread``: contiguous uint8 device
    tensors of those shapes, allocated when None; with ``want_spread`` False no spread is computed and (plate, None)
    returned."""
    who = "plate_from_samples"
    n, h, w, _ = _check_tensor(who, "samples", samples, (torch.uint8,), "n,h,w,3")
    if n > PLATE_MAX_SAMPLES:
        raise ValueError("%s: at most %d samples, got %d" % (who, PLATE_MAX_SAMPLES, n))
    if spread is not None and not want_spread:
        raise ValueError("%s: a spread buffer although want_spread is False" % who)
    plate = _out_or_new(who, "plate", plate, torch.uint8, "h,w,3", samples.device, h=h, w=w)
    if want_spread:
        spread = _out_or_new(who, "spread", spread, torch.uint8, "h,w", samples.device, h=h, w=w)
    for t in (samples, plate, spread):
        if t is not None:
            _require_gpu(t)
    check(lib().vm_plate_from_samples(_ptr(samples), n, h, w, _ptr(plate), _ptr(spread), stream_handle()), who)
    return plate, spread


# ---------------------------------------------------------------- matting metrics against ground truth

_SCORE_DT = {torch.float32: _lib.VM_F32, torch.uint8: _lib.VM_U8}


def matte_score_workspace_bytes(n, h, w):
    return lib().vm_matte_score_workspace_bytes(n, h, w)


def matte_score(pred, gt, trimap=None, prev=None, backward=None, out=None, grad_map=None, work=None):
    """vm_matte_score: the sums behind SAD, MSE, gradient error, dtSSD and MESSDdt of ``pred`` against ``gt`` (each
    [n,h,w], f32 or uint8 independently; an f32 value is clamped to [0,1], a uint8 is q / 255) -> f64 [n,8], row j =
    [pixels of the region, sum |d|, sum d^2, sum gradient error, sum dt, sum me, pixels behind sum me, 0]
    (include/vmatting.h; score_summary turns the rows into the figures).  ``trimap`` uint8 [n,h,w]: the region is where
    it is neither 0 nor 255; None: every pixel.  ``prev`` = (prev_pred, prev_gt), [h,w] with the dtypes of pred and gt:
    the frame before frame 0, for its temporal entries (None: they are 0).  ``backward`` f32 [n,h,w,2]: frame j's flow
    into frame j - 1 (reader.read_flow layout, as estimate_flow returns it), for MESSDdt.  ``out`` f64 [n,8],
    ``grad_map`` f32 [n,h,w] (receives the gradient error of every pixel), ``work`` a uint8 buffer of
    matte_score_workspace_bytes(n, h, w): contiguous device tensors; out and work are allocated when None."""
    who = "matte_score"
    n, h, w = _check_tensor(who, "pred", pred, tuple(_SCORE_DT), "n,h,w")
    dims = {"n": n, "h": h, "w": w}
    _check_tensor(who, "gt", gt, tuple(_SCORE_DT), "n,h,w", **dims)
    pp = pg = None
    if prev is not None:
        if not isinstance(prev, (tuple, list)) or len(prev) != 2:
            raise TypeError("%s: prev must be the pair (prev_pred, prev_gt)" % who)
        pp, pg = prev
        _check_tensor(who, "prev_pred", pp, (pred.dtype,), "h,w", **dims)
        _check_tensor(who, "prev_gt", pg, (gt.dtype,), "h,w", **dims)
    for name, t, dtype, shape in (("trimap", trimap, torch.uint8, "n,h,w"), ("backward", backward, torch.float32, "n,h,w,2"),
                                  ("grad_map", grad_map, torch.float32, "n,h,w")):
        if t is not None:
            _check_tensor(who, name, t, (dtype,), shape, **dims)
    out = _out_or_new(who, "out", out, torch.float64, "n,8", pred.device, n=n)
    for t in (pred, gt, trimap, pp, pg, backward, out, grad_map):
        if t is not None:
            _require_gpu(t)
    work = _buffer_or_new(who, "work", work, torch.uint8, matte_score_workspace_bytes(n, h, w), pred.device)
    check(lib().vm_matte_score(_ptr(pred), _SCORE_DT[pred.dtype], _ptr(gt), _SCORE_DT[gt.dtype], _ptr(trimap), _ptr(pp),
                               _ptr(pg), _ptr(backward), n, h, w, _ptr(out), _ptr(grad_map), _ptr(work),
                               stream_handle()), who)
    return out


SCORE_FIGURES = ("sad", "mse", "grad", "dtssd", "messddt")


def score_summary(stats, first_has_prev=False, has_flow=False):
    """The figures behind matte_score's rows, on the host (no GPU): ``stats`` f64 [n,8] (a numpy array or a tensor) ->
    a dict of per-frame float64 arrays, "count" (pixels of the region), "sad" = sum |d|, "mse" = sum d^2 / count,
    "grad" = the summed gradient error, "dtssd" = sqrt(sum dt / count), "messddt" = sum me / "taking_part", and under
    "clip" the mean of each figure over the frames where it exists.  A figure that does not exist is NaN and left out
    of its mean: every figure of a frame whose region is empty, dtssd and messddt of frame 0 unless ``first_has_prev``
    (the call was given ``prev``), messddt without ``has_flow`` or where no pixel took part.  Published tables usually
    quote SAD / 1000, MSE * 1000 and Grad / 1000."""
    if isinstance(stats, torch.Tensor):
        stats = stats.detach().cpu().numpy()
    s = np.asarray(stats)
    if s.dtype != np.float64:
        raise TypeError("score_summary: stats must be float64, got %s" % s.dtype)
    if s.ndim != 2 or s.shape[1] != 8:
        raise ValueError("score_summary: stats must be [n,8], got %s" % (s.shape,))
    n = s.shape[0]
    count, part = s[:, 0].copy(), s[:, 6].copy()
    exists = count > 0
    temporal = exists.copy()
    if n and not first_has_prev:
        temporal[0] = False
    flow = temporal & bool(has_flow) & (part > 0)
    safe, safe_part = np.where(exists, count, 1.0), np.where(flow, part, 1.0)
    nan = np.full(n, np.nan)
    res = {"count": count, "taking_part": part,
           "sad": np.where(exists, s[:, 1], nan), "mse": np.where(exists, s[:, 2] / safe, nan),
           "grad": np.where(exists, s[:, 3], nan), "dtssd": np.where(temporal, np.sqrt(s[:, 4] / safe), nan),
           "messddt": np.where(flow, s[:, 5] / safe_part, nan)}
    res["clip"] = {k: float(res[k][~np.isnan(res[k])].mean()) if (~np.isnan(res[k])).any() else float("nan")
                   for k in SCORE_FIGURES}
    return res


# ---------------------------------------------------------------- guided matte upsampling

SCALES = (2, 3, 4)
REDUCE_KINDS = {"mean": (_lib.VM_REDUCE_MEAN, 3), "trimap": (_lib.VM_REDUCE_TRIMAP, 1)}  # kind -> (code, channels)
# window radius on the reduced frame and the regulariser, the values of the CPU prototype; untuned on real footage
# 
GUIDED_DEFAULTS = {"r": 2, "eps": 1e-3}
GUIDED_R_MAX, GUIDED_EPS_MIN, GUIDED_EPS_MAX = 8, 1e-5, 1.0


def check_scale(who, scale, smallest=2):
    """The reduction factor: an integer in ``smallest``..4 (an op takes 2..4; FrameStream also 1: no reduction)."""
    return check_int(who, "scale", scale, smallest, SCALES[-1])


def reduced_size(h, w, scale):
    """(ceil(h / scale), ceil(w / scale)): the size the model runs at."""
    return -(-int(h) // scale), -(-int(w) // scale)


def check_guided_options(who, r=GUIDED_DEFAULTS["r"], eps=GUIDED_DEFAULTS["eps"]):
    """The options of vm_guided_coeffs as it checks them, on the host: an integer r in 1..8 and a real eps in
    [1e-5, 1] -> (r, eps)."""
    r = check_int(who, "r", r, 1, GUIDED_R_MAX)
    if not isinstance(eps, (int, float, np.integer, np.floating)) or isinstance(eps, (bool, np.bool_)):
        raise TypeError("%s: eps must be a real number, got %r" % (who, eps))
    if not GUIDED_EPS_MIN <= eps <= GUIDED_EPS_MAX:  # (false for NaN)
        raise ValueError("%s: eps must be in [%g, %g], got %r" % (who, GUIDED_EPS_MIN, GUIDED_EPS_MAX, eps))
    return r, float(eps)


def guided_options(who, options):
    """A dict over GUIDED_DEFAULTS (None: the defaults), checked -> {"r": r, "eps": eps}."""
    return _options(who, GUIDED_DEFAULTS, options, check_guided_options)


def frames_reduce_u8(frames, scale, kind="mean", out=None):
    """vm_frames_reduce_u8: uint8 frames to the model's resolution.  kind "mean": ``frames`` [n,h,w,3] -> [n,hm,wm,3],
    per byte the mean of the scale x scale block, halves rounded up; kind "trimap": ``frames`` [n,h,w] -> [n,hm,wm],
    the block's byte if all its pixels agree, else 128.  hm = ceil(h / scale), wm = ceil(w / scale); the last blocks of a
    ragged frame are smaller (include/vmatting.h).  ``out``: a contiguous uint8 device tensor of the result's shape,
    allocated when None."""
    who = "frames_reduce_u8"
    if kind not in REDUCE_KINDS:
        raise ValueError("%s: kind must be one of %s, got %r" % (who, sorted(REDUCE_KINDS), kind))
    code, c = REDUCE_KINDS[kind]
    scale = check_scale(who, scale)
    n, h, w = _check_tensor(who, "frames", frames, (torch.uint8,), "n,h,w,3" if c == 3 else "n,h,w")[:3]
    hm, wm = reduced_size(h, w, scale)
    out = _out_or_new(who, "out", out, torch.uint8, "n,hm,wm,3" if c == 3 else "n,hm,wm", frames.device, n=n, hm=hm, wm=wm)
    for t in (frames, out):
        _require_gpu(t)
    check(lib().vm_frames_reduce_u8(_ptr(frames), n, h, w, c, scale, code, _ptr(out), stream_handle()), who)
    return out


def guided_workspace_bytes(n, hm, wm):
    return lib().vm_guided_workspace_bytes(n, hm, wm)


def guided_coeffs(guide_lo, alpha_lo, r=GUIDED_DEFAULTS["r"], eps=GUIDED_DEFAULTS["eps"], out=None, work=None):
    """vm_guided_coeffs: the guided filter's linear model on the reduced frame.  ``guide_lo`` u8 [n,hm,wm,3], ``alpha_lo``
    f32 [n,hm,wm] or [n,hm,wm,1] -> f32 [n,hm,wm,4] = (a_0, a_1, a_2, b): alpha_lo ~ a . guide_lo / 255 + b over the
    clipped (2 r + 1)^2 window of every pixel, regularised by eps, then averaged over the same window
    (include/vmatting.h).  ``out``: a contiguous f32 [n,hm,wm,4] device tensor; ``work``: a uint8 device buffer of
    guided_workspace_bytes(n, hm, wm); both are allocated when None."""
    who = "guided_coeffs"
    n, hm, wm, _ = _check_tensor(who, "guide_lo", guide_lo, (torch.uint8,), "n,hm,wm,3")
    _check_tensor(who, "alpha_lo", alpha_lo, (torch.float32,), "n,hm,wm | n,hm,wm,1", n=n, hm=hm, wm=wm)
    r, eps = check_guided_options(who, r, eps)
    out = _out_or_new(who, "out", out, torch.float32, "n,hm,wm,4", guide_lo.device, n=n, hm=hm, wm=wm)
    for t in (guide_lo, alpha_lo, out):
        _require_gpu(t)
    work = _buffer_or_new(who, "work", work, torch.uint8, guided_workspace_bytes(n, hm, wm), guide_lo.device)
    check(lib().vm_guided_coeffs(_ptr(guide_lo), _ptr(alpha_lo), n, hm, wm, r, eps, _ptr(out), _ptr(work),
                                 stream_handle()), who)
    return out


def guided_apply(ab, guide_hi, scale, out=None):
    """vm_guided_apply: the matte at full resolution.  ``ab`` f32 [n,hm,wm,4] (guided_coeffs), ``guide_hi`` u8
    [n,h,w,3] with hm = ceil(h / scale), wm = ceil(w / scale) -> f32 [n,h,w,1]: (a, b) interpolated bilinearly at the
    pixel (half-pixel centres, clamped), alpha = min(max(a . guide_hi / 255 + b, 0), 1), in f32 operation by operation
    (include/vmatting.h).  ``out``: a contiguous f32 [n,h,w,1] or [n,h,w] device tensor, allocated when None."""
    who = "guided_apply"
    scale = check_scale(who, scale)
    n, h, w, _ = _check_tensor(who, "guide_hi", guide_hi, (torch.uint8,), "n,h,w,3")
    hm, wm = reduced_size(h, w, scale)
    _check_tensor(who, "ab", ab, (torch.float32,), "n,hm,wm,4", n=n, hm=hm, wm=wm)
    out = _out_or_new(who, "out", out, torch.float32, "n,h,w,1 | n,h,w", guide_hi.device, n=n, h=h, w=w)
    for t in (ab, guide_hi, out):
        _require_gpu(t)
    check(lib().vm_guided_apply(_ptr(ab), _ptr(guide_hi), n, h, w, scale, _ptr(out), stream_handle()), who)
    return out


def guided_upsample(alpha_lo, guide_hi, scale, r=GUIDED_DEFAULTS["r"], eps=GUIDED_DEFAULTS["eps"], guide_lo=None):
    """The three in a row: ``alpha_lo`` f32 [n,hm,wm] or [n,hm,wm,1], the matte of the model on the frames reduced by
    ``scale``, and the full-resolution frames ``guide_hi`` u8 [n,h,w,3] -> f32 [n,h,w,1].  ``guide_lo``: the reduced
    frames the model saw (frames_reduce_u8(guide_hi, scale)); made here when None."""
    who = "guided_upsample"
    scale = check_scale(who, scale)
    r, eps = check_guided_options(who, r, eps)
    if guide_lo is None:
        guide_lo = frames_reduce_u8(guide_hi, scale)
    return guided_apply(guided_coeffs(guide_lo, alpha_lo, r, eps), guide_hi, scale)


# ---------------------------------------------------------------- the plate's exposure matched to the frame

# the inlier band around the mode in 1/64 of the ratio, and the share of the frame (1 / min_share) the inliers must
# reach; band 8 from the CPU prototype (4 was worse by half), untuned on real footage
GAIN_DEFAULTS = {"band": 8, "min_share": 16}
GAIN_BAND_MAX, GAIN_SHARE_MAX = 16, 4096
GAIN_ONE = 4096  # the gains are Q12 integers


def check_gain_options(who, band=GAIN_DEFAULTS["band"], min_share=GAIN_DEFAULTS["min_share"]):
    """The options of vm_plate_gain_fit as it checks them, on the host: integers, band in 1..16 and min_share in
    1..4096 -> (band, min_share)."""
    return check_int(who, "band", band, 1, GAIN_BAND_MAX), check_int(who, "min_share", min_share, 1, GAIN_SHARE_MAX)


def gain_options(who, options):
    """A dict over GAIN_DEFAULTS (None: the defaults), checked -> {"band": band, "min_share": min_share}."""
    return _options(who, GAIN_DEFAULTS, options, check_gain_options)


GAIN_FIT = "fit"


def check_gain_mode(who, gain, options):
    """The ``gain`` argument of FrameStream and reader.trimap_from_plate: None or "fit", and their ``gain_options`` (a
    dict over GAIN_DEFAULTS) only with "fit" -> the checked options, or None without a gain."""
    if gain is not None and not (isinstance(gain, str) and gain == GAIN_FIT):
        raise ValueError("%s: gain must be None or %r, got %r" % (who, GAIN_FIT, gain))
    if gain is None:
        if options is not None:
            raise ValueError("%s: gain_options go with gain=%r" % (who, GAIN_FIT))
        return None
    return gain_options("%s: gain_options" % who, options)


def plate_gain_workspace_bytes(n):
    return lib().vm_plate_gain_workspace_bytes(n)


def plate_gain_fit(cmp, bg, band=GAIN_DEFAULTS["band"], min_share=GAIN_DEFAULTS["min_share"], out=None, support=None,
                   work=None):
    """vm_plate_gain_fit: one gain per frame and colour channel between the frames and their background.  cmp u8
    [n,h,w,3] BGR, bg u8 [n,h,w,3] or one static plate [h,w,3] / [1,h,w,3] -> (gain, support), both int32 [n,3]: the
    gain in Q12 (4096 is 1.0) is the least-squares ratio over the pixels within ``band`` / 64 of the histogram mode of
    cmp / bg, or 4096 where fewer than h w / ``min_share`` pixels are; support is their count (include/vmatting.h).
    ``out`` / ``support``: contiguous int32 [n,3] device tensors; ``work``: a uint8 device buffer of
    plate_gain_workspace_bytes(n); all allocated when None."""
    who = "plate_gain_fit"
    n, h, w, nb = _check_frames_and_bg(who, cmp, bg)
    band, min_share = check_gain_options(who, band, min_share)
    out = _out_or_new(who, "out", out, torch.int32, "n,3", cmp.device, ValueError, n=n)
    support = _out_or_new(who, "support", support, torch.int32, "n,3", cmp.device, ValueError, n=n)
    for t in (cmp, bg, out, support):
        _require_gpu(t)
    work = _buffer_or_new(who, "work", work, torch.uint8, plate_gain_workspace_bytes(n), cmp.device)
    check(lib().vm_plate_gain_fit(_ptr(cmp), _ptr(bg), nb, n, h, w, band, min_share, _ptr(out), _ptr(support),
                                  _ptr(work), stream_handle()), who)
    return out, support


def plate_gain_apply(bg, gain, out=None):
    """vm_plate_gain_apply: the plate under the gains.  bg u8 [n,h,w,3], or one static plate [h,w,3] / [1,h,w,3] for
    all n rows of ``gain`` (int32 [n,3], Q12, as plate_gain_fit returns it) -> u8 [n,h,w,3] = min(255, (gain * bg +
    2048) >> 12) (include/vmatting.h).  ``out``: a contiguous uint8 [n,h,w,3] device tensor, allocated when None."""
    who = "plate_gain_apply"
    n, _ = _check_tensor(who, "gain", gain, (torch.int32,), "n,3")
    shape = _check_tensor(who, "bg", bg, (torch.uint8,), "n,h,w,3 | 1,h,w,3 | h,w,3", n=n)
    h, w = shape[-3], shape[-2]
    nb = n if shape == (n, h, w, 3) else 1
    out = _out_or_new(who, "out", out, torch.uint8, "n,h,w,3", bg.device, ValueError, n=n, h=h, w=w)
    for t in (bg, gain, out):
        _require_gpu(t)
    check(lib().vm_plate_gain_apply(_ptr(bg), nb, _ptr(gain), n, h, w, _ptr(out), stream_handle()), who)
    return out


# ---------------------------------------------------------------- the plate's position matched to the frame

# Gauss-Newton steps per level, the residual gate in grey levels, the share of the frame (1 / min_share) the pixels the
# fit explains must reach, the corner displacement limit min(h, w) / reach, and the pyramids' levels: the values of a
# CPU prototype on synthetic scenes, untuned on real footage
ALIGN_DEFAULTS = {"iters": 4, "tol": 16.0, "min_share": 4, "reach": 6, "levels": 6}
ALIGN_ITERS_MAX, ALIGN_SHARE_MAX, ALIGN_REACH_MAX = 64, 4096, 1024
ALIGN_PARAMS = 7  # of the 8 floats per frame: six affine deviations and the gain


def check_align_options(who, iters=ALIGN_DEFAULTS["iters"], tol=ALIGN_DEFAULTS["tol"],
                        min_share=ALIGN_DEFAULTS["min_share"], reach=ALIGN_DEFAULTS["reach"],
                        levels=ALIGN_DEFAULTS["levels"]):
    """The options of vm_plate_align_fit as it checks them, on the host: iters in 1..64, tol a positive finite number,
    min_share in 1..4096, reach in 1..1024, levels at least 1 -> (iters, tol, min_share, reach, levels)."""
    iters = check_int(who, "iters", iters, 1, ALIGN_ITERS_MAX)
    if isinstance(tol, (bool, np.bool_)) or not isinstance(tol, (int, float, np.integer, np.floating)):
        raise TypeError("%s: tol must be a number, got %r" % (who, tol))
    tol = float(tol)
    if not (tol > 0.0 and np.isfinite(tol)):
        raise ValueError("%s: tol must be a positive finite number, got %r" % (who, tol))
    return (iters, tol, check_int(who, "min_share", min_share, 1, ALIGN_SHARE_MAX),
            check_int(who, "reach", reach, 1, ALIGN_REACH_MAX), check_int(who, "levels", levels, 1))


def align_options(who, options):
    """A dict over ALIGN_DEFAULTS (None: the defaults), checked -> {"iters": ..., "tol": ..., "min_share": ...,
    "reach": ..., "levels": ...}."""
    return _options(who, ALIGN_DEFAULTS, options, check_align_options)


ALIGN_FIT = "fit"


def check_align_mode(who, align, options):
    """The ``align`` argument of FrameStream and reader.trimap_from_plate: None or "fit", and their ``align_options``
    (a dict over ALIGN_DEFAULTS) only with "fit" -> the checked options, or None without an alignment."""
    if align is not None and not (isinstance(align, str) and align == ALIGN_FIT):
        raise ValueError("%s: align must be None or %r, got %r" % (who, ALIGN_FIT, align))
    if align is None:
        if options is not None:
            raise ValueError("%s: align_options go with align=%r" % (who, ALIGN_FIT))
        return None
    return align_options("%s: align_options" % who, options)


def plate_align_workspace_bytes(n, h, w, levels=ALIGN_DEFAULTS["levels"]):
    return lib().vm_plate_align_workspace_bytes(n, h, w, levels)


def plate_align_fit(cmp_pyr, bg_pyr, h, w, iters=ALIGN_DEFAULTS["iters"], tol=ALIGN_DEFAULTS["tol"],
                    min_share=ALIGN_DEFAULTS["min_share"], reach=ALIGN_DEFAULTS["reach"],
                    levels=ALIGN_DEFAULTS["levels"], out=None, support=None, work=None):
    """vm_plate_align_fit: one affine map and one photometric gain per frame between the frames' and the plate's grey
    pyramids.  cmp_pyr f32 [n,floats]: row i is flow_pyramid(frame i, levels) of an [h,w] frame (floats at least
    flow_pyramid_floats(h, w, levels)); bg_pyr f32 [n,floats], or [1,floats] / [floats] for one static plate ->
    (params f32 [n,8] = (p0..p5, g, 0), support int32 [n]): frame pixel (x, y) sees the plate at (x + p0 xc + p1 yc +
    p2, y + p3 xc + p4 yc + p5) in centred coordinates, and is g times as bright; the identity (0 .. 0, 1, 0) where
    fewer than h w / ``min_share`` pixels end within ``tol`` / 4 grey levels of the fit (``support`` is their count), or
    a corner moves by more than min(h, w) / ``reach`` pixels (include/vmatting.h).  ``out`` / ``support``: contiguous
    f32 [n,8] / int32 [n] device tensors; ``work``: a uint8 device buffer of plate_align_workspace_bytes(n, h, w,
    levels); all allocated when None."""
    who = "plate_align_fit"
    h, w = check_int(who, "h", h, 1), check_int(who, "w", w, 1)
    iters, tol, min_share, reach, levels = check_align_options(who, iters, tol, min_share, reach, levels)
    check_flow_options(who, h, w, levels)
    n, stride = _check_tensor(who, "cmp_pyr", cmp_pyr, (torch.float32,), "n,f")
    shape = _check_tensor(who, "bg_pyr", bg_pyr, (torch.float32,), "n,f | 1,f | f", n=n)
    nb = n if shape == (n, shape[-1]) else 1
    out = _out_or_new(who, "out", out, torch.float32, "n,8", cmp_pyr.device, ValueError, n=n)
    support = _out_or_new(who, "support", support, torch.int32, "n", cmp_pyr.device, ValueError, n=n)
    for t in (cmp_pyr, bg_pyr, out, support):
        _require_gpu(t)
    floats = flow_pyramid_floats(h, w, levels)
    if stride < floats or shape[-1] < floats:
        raise ValueError("%s: a pyramid of [%d,%d] frames at %d levels is %d floats, got rows of %d and %d" %
                         (who, h, w, levels, floats, stride, shape[-1]))
    work = _buffer_or_new(who, "work", work, torch.uint8, plate_align_workspace_bytes(n, h, w, levels), cmp_pyr.device)
    check(lib().vm_plate_align_fit(_ptr(cmp_pyr), stride, _ptr(bg_pyr), shape[-1], nb, n, h, w, levels, iters, tol,
                                   min_share, reach, _ptr(out), _ptr(support), _ptr(work), stream_handle()), who)
    return out, support


def plate_align_apply(bg, params, out=None):
    """vm_plate_align_apply: the plate seen through the maps.  bg u8 [n,h,w,3], or one static plate [h,w,3] / [1,h,w,3]
    for all n rows of ``params`` (f32 [n,8], as plate_align_fit returns it) -> u8 [n,h,w,3]: per pixel the plate's
    bilinear sample at the mapped position, coordinates clamped to the plate, rounded once; identity parameters return
    the plate (include/vmatting.h).  ``out``: a contiguous uint8 [n,h,w,3] device tensor, allocated when None."""
    who = "plate_align_apply"
    n, _ = _check_tensor(who, "params", params, (torch.float32,), "n,8")
    shape = _check_tensor(who, "bg", bg, (torch.uint8,), "n,h,w,3 | 1,h,w,3 | h,w,3", n=n)
    h, w = shape[-3], shape[-2]
    nb = n if shape == (n, h, w, 3) else 1
    out = _out_or_new(who, "out", out, torch.uint8, "n,h,w,3", bg.device, ValueError, n=n, h=h, w=w)
    for t in (bg, params, out):
        _require_gpu(t)
    check(lib().vm_plate_align_apply(_ptr(bg), nb, _ptr(params), n, h, w, _ptr(out), stream_handle()), who)
    return out


def frame_pyramids(frames, levels, out, work):
    """flow_pyramid of every frame of a uint8 [n,h,w,3] stack into the rows of ``out`` (f32 [n,floats], rows 16-byte
    aligned) -> out."""
    for j in range(len(frames)):
        flow_pyramid(frames[j], levels, out=out[j], work=work)
    return out


# ---------------------------------------------------------------- flow-compensated temporal matte filter

# the share of the previous matte, the colour difference (grey levels) and the matte difference at which the gates shut:
# the values of the CPU prototype on a synthetic clip, untuned on real footage
SMOOTH_DEFAULTS = {"strength": 0.5, "tol": 24.0, "jump": 0.3}
SMOOTH_FLOW = "flow"
_F32_MAX = float(np.finfo(np.float32).max)


def check_smooth_options(who, strength=SMOOTH_DEFAULTS["strength"], tol=SMOOTH_DEFAULTS["tol"],
                         jump=SMOOTH_DEFAULTS["jump"]):
    """The options of vm_matte_smooth as it checks them, on the host: numbers (no bool), 0 <= strength < 1, tol and jump
    positive and finite as f32 -> (strength, tol, jump) as floats."""
    vals = []
    for name, v in (("strength", strength), ("tol", tol), ("jump", jump)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise TypeError("%s: %s must be a number, got %r" % (who, name, v))
        vals.append(float(v))
    strength, tol, jump = vals  # (the library sees them rounded to f32, and checks again)
    if not 0.0 <= strength < 1.0:
        raise ValueError("%s: strength must be in [0, 1), got %r" % (who, strength))
    for name, v in (("tol", tol), ("jump", jump)):
        if not 0.0 < v <= _F32_MAX:
            raise ValueError("%s: %s must be a positive finite number, got %r" % (who, name, v))
    return strength, tol, jump


def smooth_options(who, options):
    """A dict over SMOOTH_DEFAULTS (None: the defaults), checked -> {"strength": ..., "tol": ..., "jump": ...}."""
    return _options(who, SMOOTH_DEFAULTS, options, check_smooth_options)


def check_smooth_mode(who, smooth, options):
    """The ``smooth`` argument of FrameStream: None or "flow", and its ``smooth_options`` (a dict over SMOOTH_DEFAULTS)
    only with "flow" -> the checked options, or None without the filter."""
    if smooth is not None and not (isinstance(smooth, str) and smooth == SMOOTH_FLOW):
        raise ValueError("%s: smooth must be None or %r, got %r" % (who, SMOOTH_FLOW, smooth))
    if smooth is None:
        if options is not None:
            raise ValueError("%s: smooth_options go with smooth=%r" % (who, SMOOTH_FLOW))
        return None
    return smooth_options("%s: smooth_options" % who, options)


def matte_smooth(alpha, cmp, backward, prev=None, strength=SMOOTH_DEFAULTS["strength"], tol=SMOOTH_DEFAULTS["tol"],
                 jump=SMOOTH_DEFAULTS["jump"], out=None, weight=None):
    """vm_matte_smooth: the mattes of consecutive frames filtered along the flow.  alpha f32 [n,h,w] or [n,h,w,1] (the
    model's mattes), cmp u8 [n,h,w,3] BGR, backward f32 [n,h,w,2] (frame j's flow into frame j - 1, reader.read_flow
    layout, as estimate_flow returns it) -> f32 of alpha's shape: frame j's matte pulled towards the previous filtered
    matte at the flow's target by ``strength`` times a weight that is 1 where the frame equals the warped previous
    frame and the matte the warped previous matte, and falls to 0 at a colour difference of ``tol`` grey levels or a
    matte difference of ``jump`` (include/vmatting.h).  ``prev`` = (prev_alpha f32 [h,w] or [h,w,1], prev_cmp u8
    [h,w,3]): the filtered matte and the frame before frame 0; None: frame 0 starts a run, its result is its clamped
    matte and backward[0] is not read.  ``out``: a contiguous f32 device tensor of alpha's shape, which may be
    ``alpha`` itself (in place); ``weight``: one more, which receives the weights (0 where the filter held back
    entirely).  out is allocated when None."""
    who = "matte_smooth"
    shape = _check_tensor(who, "alpha", alpha, (torch.float32,), "n,h,w | n,h,w,1")
    n, h, w = shape[:3]
    dims = {"n": n, "h": h, "w": w}
    _check_tensor(who, "cmp", cmp, (torch.uint8,), "n,h,w,3", **dims)
    _check_tensor(who, "backward", backward, (torch.float32,), "n,h,w,2", **dims)
    pa = pc = None
    if prev is not None:
        if not isinstance(prev, (tuple, list)) or len(prev) != 2:
            raise TypeError("%s: prev must be the pair (prev_alpha, prev_cmp)" % who)
        pa, pc = prev
        _check_tensor(who, "prev_alpha", pa, (torch.float32,), "h,w | h,w,1", **dims)
        _check_tensor(who, "prev_cmp", pc, (torch.uint8,), "h,w,3", **dims)
    strength, tol, jump = check_smooth_options(who, strength, tol, jump)
    out = _out_or_new(who, "out", out, torch.float32, "n,h,w,1 | n,h,w" if len(shape) == 4 else "n,h,w | n,h,w,1",
                      alpha.device, ValueError, **dims)
    if weight is not None:
        _check_tensor(who, "weight", weight, (torch.float32,), "n,h,w | n,h,w,1", ValueError, **dims)
    for t in (alpha, cmp, backward, pa, pc, out, weight):
        if t is not None:
            _require_gpu(t)
    check(lib().vm_matte_smooth(_ptr(alpha), _ptr(cmp), _ptr(backward), _ptr(pa), _ptr(pc), n, h, w, strength, tol, jump,
                                _ptr(out), _ptr(weight), stream_handle()), who)
    return out


# ---------------------------------------------------------------- training step (train.py:288-343, config 5)

def matting_loss_backward(pred, gt, raw_fg, in_bg, in_cmp, out=None):
    """dL/dlogits of train.py:294-298's loss for pred = sigmoid(logits) (all contiguous f32 device tensors)."""
    ts = [_f32(t) for t in (pred, gt, raw_fg, in_bg, in_cmp)]
    pixels = ts[0].numel()
    if ts[1].numel() != pixels or any(t.numel() != 3 * pixels for t in ts[2:]):
        raise ValueError("matting_loss_backward: pred/gt [P], raw_fg/bg/cmp [P,3]")
    out = torch.empty_like(ts[0]) if out is None else _f32(out)
    check(lib().vm_matting_loss_backward(*[_ptr(t) for t in ts], pixels, _ptr(out), stream_handle()),
          "matting_loss_backward")
    return out


def bn_backward(x, dy, y, mean, var, gamma, eps=1e-3, dx=None, dgamma=None, dbeta=None, dx2=None, dbias=None):
    """Gradient of tf.contrib batch_norm(is_training=True) (+ the relu after it when ``y`` is given).
    x None: only dbeta = channel sum of dy (a bias gradient).  dx2: optional second copy of dx (e.g. bf16).
    dbias: the gradient of a conv bias added before the BN (= channel sum of dx) from the same reduction."""
    c = dy.shape[-1]
    views = [None if t is None else nhwc(t) for t in (x, dy, y, dx, dx2)]
    ws = _workspace(lib().vm_bn_backward_workspace_bytes(c), dy.device)
    check(lib().vm_bn_backward_ex_nhwc(_ref(views[0]), _ref(views[1]), _ref(views[2]), _ptr(mean), _ptr(var),
                                       _ptr(gamma), float(eps), _ref(views[3]), _ref(views[4]), _ptr(dgamma),
                                       _ptr(dbeta), _ptr(dbias), _ptr(ws), stream_handle()), "bn_backward")
    return dx


def bn_backward_apply(x, dy, y, mean, var, gamma, sum_g, sum_gx, count, dx, eps=1e-3, dx2=None):
    """The input-gradient pass of bn_backward with given channel sums over ``count`` pixels (SyncBN: the sums
    all-reduced over the replicas, count = their pixels)."""
    views = [None if t is None else nhwc(t) for t in (x, dy, y, dx, dx2)]
    check(lib().vm_bn_backward_apply_nhwc(_ref(views[0]), _ref(views[1]), _ref(views[2]), _ptr(mean), _ptr(var),
                                          _ptr(gamma), float(eps), _ptr(_f32(sum_g)), _ptr(_f32(sum_gx)), int(count),
                                          _ref(views[3]), _ref(views[4]), stream_handle()), "bn_backward_apply")
    return dx


def relu_backward(dy, y, dx, dx2=None, dx_lo=None):
    """dx = dy * (y > 0) (+ a second copy dx2, e.g. bf16).  ``dx_lo``: its channels k = dx_lo.shape[-1] take the
    first k channels of the gradient and dx / dx2 the rest (one pass over a decoder level's concat)."""
    dv, yv, xv = nhwc(dy), nhwc(y), nhwc(dx)
    x2 = ctypes.byref(nhwc(dx2)) if dx2 is not None else None
    if dx_lo is None:
        check(lib().vm_relu_backward_ex_nhwc(ctypes.byref(dv), ctypes.byref(yv), ctypes.byref(xv), x2,
                                             stream_handle()), "relu_backward")
        return dx
    lv = nhwc(dx_lo)
    check(lib().vm_relu_backward_split_nhwc(ctypes.byref(dv), ctypes.byref(yv), dx_lo.shape[-1], ctypes.byref(lv),
                                            ctypes.byref(xv), x2, stream_handle()), "relu_backward")
    return dx


def maxpool_backward(x, dy, dx, add=None):
    """Adjoint of maxpool2x2 (tf.nn.max_pool 2x2/2 SAME): dx = add + dy routed to each window's first maximum of x
    (TF MaxPoolGrad's tie rule).  ``add`` may be dx itself."""
    xv, dv, ov = nhwc(x), nhwc(dy), nhwc(dx)
    av = ctypes.byref(nhwc(add)) if add is not None else None
    check(lib().vm_maxpool2x2_backward_nhwc(ctypes.byref(xv), ctypes.byref(dv), av, ctypes.byref(ov),
                                            stream_handle()), "maxpool_backward")
    return dx


def relu_backward_bias(dy, y, dz, dbias, add=None):
    """vm_relu_backward_bias_nhwc: dz = (y > 0) * g and dbias = channel sums of dz in one pass; g = dy (+ add), or —
    when dy has the 2x2 SAME pool's shape — add + the max-pool adjoint of dy (TF MaxPoolGrad's first maximum)."""
    _f32(dbias)
    views = [nhwc(dy), nhwc(y), None if add is None else nhwc(add), nhwc(dz)]
    ws = _workspace(lib().vm_relu_backward_bias_workspace_bytes(y.shape[-1]), y.device)
    check(lib().vm_relu_backward_bias_nhwc(_ref(views[0]), _ref(views[1]), _ref(views[2]), _ref(views[3]),
                                           _ptr(dbias), _ptr(ws), stream_handle()), "relu_backward_bias")
    return dz


def resize_backward(dy, dx):
    """Adjoint of resize_bilinear: dy [n,oh,ow,c] -> dx contiguous f32 (or bf16, c % 4 == 0) [n,ih,iw,c]
    (overwritten)."""
    if dx.shape[0] != dy.shape[0] or dx.shape[3] != dy.shape[3]:
        raise ValueError("resize_backward: batch/channel mismatch")
    dv = nhwc(dy)
    if dx.dtype == torch.bfloat16:
        xv = nhwc(dx)
        check(lib().vm_resize_bilinear_tf1_backward_nhwc(ctypes.byref(dv), ctypes.byref(xv), stream_handle()),
              "resize_backward")
        return dx
    _f32(dx)
    check(lib().vm_resize_bilinear_tf1_backward(ctypes.byref(dv), _ptr(dx), dx.shape[1], dx.shape[2],
                                                stream_handle()), "resize_backward")
    return dx


def conv_wgrad(x, dy, dw, mfma=False, sources=None):
    """dw[3,3,cin,cout] += 3x3 SAME conv weight gradient of input view x and output-gradient view dy (f32; bf16 too
    for the wide MFMA kernel, cout > 48).

    ``mfma``: bf16 x only — the MFMA kernel with dy rounded to bf16 (the bf16 training path); else the exact-f32
    FMA kernel.  ``sources`` = (number of sources, element stride between sources): x is the [n,h,w,c] view of
    source 0 and the conv input is the channel concat of the sources (tower-major features, MFMA kernel only)."""
    _f32(dw)
    if isinstance(x, SourceConcat):
        x, sources = x.src0, (x.nsrc, x.stride)
    n, h, w, cin = x.shape
    cout = dy.shape[-1]
    src_c = cin
    if sources is not None:
        cin = src_c * int(sources[0])
    if tuple(dy.shape[:3]) != (n, h, w) or dw.numel() != 9 * cin * cout:
        raise ValueError("conv_wgrad: x %s, dy %s, dw %s" % (tuple(x.shape), tuple(dy.shape), tuple(dw.shape)))
    dv = nhwc(dy)
    if mfma or sources is not None or cout > 48:  # (cout > 48: the wide kernels, UNetImage training)
        xv = nhwc(x)
        xv.c = cin
        src_c, stride = (src_c, int(sources[1])) if sources is not None else (0, 0)
        mode = 1 if mfma else 0
        ws = _workspace(lib().vm_conv3x3_wgrad_ex_workspace_bytes(n, h, w, cin, cout, mode), x.device)
        check(lib().vm_conv3x3_wgrad_ex_nhwc(ctypes.byref(xv), src_c, stride, ctypes.byref(dv), _ptr(dw), _ptr(ws),
                                             mode, stream_handle()), "conv_wgrad_ex")
        return dw
    xv = nhwc(x)
    ws = _workspace(lib().vm_conv3x3_wgrad_workspace_bytes(n, h, w, cin, cout), x.device)
    check(lib().vm_conv3x3_wgrad_nhwc(ctypes.byref(xv), ctypes.byref(dv), _ptr(dw), _ptr(ws), stream_handle()),
          "conv_wgrad")
    return dw


def flip_weights(w_hwio, out):
    cin, cout = int(w_hwio.shape[2]), int(w_hwio.shape[3])
    check(lib().vm_conv3x3_flip_weights(_ptr(_f32(w_hwio)), cin, cout, _ptr(_f32(out)), stream_handle()),
          "flip_weights")
    return out


def adam_tf(var, m, v, grad, lr_t, beta1, beta2, eps, grad_scale=1.0):
    for t in (var, m, v, grad):
        _f32(t)
    check(lib().vm_adam_tf(_ptr(var), _ptr(m), _ptr(v), _ptr(grad), var.numel(), float(lr_t), float(beta1),
                           float(beta2), float(eps), float(grad_scale), stream_handle()), "adam")
    return var
