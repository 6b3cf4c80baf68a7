"""Two-frame temporal helpers (reference flow.py) on gfx950 kernels.

Same names and call shapes as flow.py:9-65.  numpy arguments are accepted like the
reference (uploaded, computed on the GPU, returned as numpy; ``correct_alpha`` still
mutates the caller's array in place); torch device tensors stay on the device.
"""

import numpy as np
import torch

from . import ops


def _dev(a, dtype=torch.float32):
    if isinstance(a, torch.Tensor):
        return a.to("cuda" if not a.is_cuda else a.device, dtype)
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def warp_img(img, flow, mode="opencv"):
    """flow.warp_img (flow.py:9-18): backward-warp a single-channel image by a dense flow.

    mode 'opencv' = cv2.remap's 1/32-pixel fixed-point coordinates (reference behaviour),
    'exact' = plain bilinear.  img [H,W] (or [N,H,W] with flow [N,H,W,2]).
    """
    if isinstance(img, torch.Tensor):
        if img.dim() not in (2, 3):
            raise AssertionError("warp_img: image must be 1 channel")
        return ops.remap_f32(_dev(img), _dev(flow), mode)
    assert len(img.shape) == 2  # flow.py:11
    out = ops.remap_f32(_dev(img), _dev(flow), mode)
    return out.cpu().numpy().astype(img.dtype if img.dtype.kind == "f" else np.float32)


def warp_bgr(img, flow):
    """flow.warp_bgr (flow.py:21-33): uint8 [H,W,3], OpenCV fixed-point bilinear per plane."""
    if isinstance(img, torch.Tensor):
        return ops.remap_u8(img.to(torch.uint8), _dev(flow))
    out = ops.remap_u8(torch.from_numpy(np.ascontiguousarray(img, np.uint8)).cuda(), _dev(flow))
    return out.cpu().numpy()


def estimate_flow(cur, prev, levels=6, warps=3, iters=20, alpha=15.0):
    """The dense flow f between two uint8 [H,W,3] BGR frames with cur(x, y) ~ prev(x + f[...,0], y + f[...,1]), f32
    [H,W,2] in reader.read_flow layout: what ``warp_img(img_of_prev, f)`` and ``correct_alpha`` take as the backward
    flow of ``cur``; the forward flow is ``estimate_flow(prev, cur)``.  The reference reads such flows from .flo
    files and computes none; this is coarse-to-fine Horn-Schunck with warping (ops.estimate_flow).  numpy frames
    return numpy, device tensors stay on the device."""
    if isinstance(cur, torch.Tensor) != isinstance(prev, torch.Tensor):
        raise TypeError("estimate_flow: cur and prev are both numpy arrays or both torch tensors")
    if isinstance(cur, torch.Tensor):
        return ops.estimate_flow(cur.contiguous(), prev.contiguous(), levels, warps, iters, alpha)
    c, p = (np.ascontiguousarray(a) for a in (cur, prev))
    if c.dtype != np.uint8 or p.dtype != np.uint8:
        raise TypeError("estimate_flow: uint8 frames expected, got %s and %s" % (c.dtype, p.dtype))
    if c.ndim != 3 or c.shape[2] != 3 or p.shape != c.shape:
        raise ValueError("estimate_flow: two [H,W,3] BGR frames of one size expected, got %s and %s" % (c.shape, p.shape))
    ops.check_flow_options("estimate_flow", c.shape[0], c.shape[1], levels, warps, iters, alpha)
    out = ops.estimate_flow(torch.from_numpy(c).cuda(), torch.from_numpy(p).cuda(), levels, warps, iters, alpha)
    return out.cpu().numpy()


def propagate_trimap(trimap, backward, grow=1):
    """The trimap of the next frame from the previous frame's uint8 [H,W] ``trimap`` (255 foreground, 0 background,
    anything else unknown) and the next frame's ``backward`` flow, f32 [H,W,2] as estimate_flow(next, previous)
    returns it: a label survives where every pixel the bilinear warp would touch, and every pixel within ``grow``
    (0..8) of those, carries it; the rest is 128 (ops.trimap_propagate).  The reference takes a trimap per frame and
    propagates none.  numpy arrays return numpy, device tensors stay on the device."""
    if isinstance(trimap, torch.Tensor) != isinstance(backward, torch.Tensor):
        raise TypeError("propagate_trimap: trimap and backward are both numpy arrays or both torch tensors")
    if isinstance(trimap, torch.Tensor):
        return ops.trimap_propagate(trimap.contiguous(), backward.contiguous(), grow)
    t, b = np.ascontiguousarray(trimap), np.ascontiguousarray(backward)
    if t.dtype != np.uint8 or b.dtype != np.float32:
        raise TypeError("propagate_trimap: a uint8 trimap and a float32 flow expected, got %s and %s" % (t.dtype, b.dtype))
    if t.ndim != 2 or b.shape != t.shape + (2,):
        raise ValueError("propagate_trimap: an [H,W] trimap and an [H,W,2] flow expected, got %s and %s" %
                         (t.shape, b.shape))
    ops.check_grow("propagate_trimap", grow)
    return ops.trimap_propagate(torch.from_numpy(t).cuda(), torch.from_numpy(b).cuda(), grow).cpu().numpy()


def correct_alpha(backward, forward, alpha, promote="numpy1", thresh=15.0):
    """flow.correct_alpha (flow.py:36-65): zero alpha where the forward/backward round trip misses by > 15 px.

    Mutates ``alpha`` in place and returns it.  ``promote``: 'numpy1' (the reference's numpy-1.x
    float64 index arithmetic) or 'numpy2' (float32, what the same code does under numpy 2).
    Raises IndexError, leaving alpha untouched, where the reference would (flow.py:46).
    The reference's GUI side effects (cv2.imshow of the error map, flow.py:51-52) are not reproduced.
    """
    if isinstance(alpha, torch.Tensor) and alpha.is_cuda and alpha.dtype == torch.float32 and alpha.is_contiguous():
        return ops.fb_consistency(_dev(backward), _dev(forward), alpha, thresh, promote)
    a = _dev(alpha).contiguous()
    ops.fb_consistency(_dev(backward), _dev(forward), a, thresh, promote)
    res = a.cpu()
    if isinstance(alpha, torch.Tensor):
        alpha.copy_(res.to(alpha.dtype))
    else:
        alpha[...] = res.numpy()
    return alpha
