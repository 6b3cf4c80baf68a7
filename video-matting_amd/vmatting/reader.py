"""Formats on the path (reference reader.py): Middlebury .flo I/O and compositing.

``read_flow`` keeps reader.py:21-30's semantics exactly (float32 magic 202021.25, int32 w,
int32 h, h*w*2 float32, little-endian; a bad magic prints and continues).  The rest of
reader.py (PNG decoding via cv2, GUI playback, HSV flow visualisation) is outside the hot
path — ``read_fg_img`` is provided through PIL for convenience only.
"""

import numpy as np
import torch

FLO_MAGIC = 202021.25


def read_flow(flow_path, device=None):
    """reader.read_flow; ``device='cuda'`` returns a device tensor (pinned host staging)."""
    with open(flow_path, "rb") as f:
        key = np.fromfile(f, dtype=np.float32, count=1)
        if FLO_MAGIC != key:
            print("ERROR: invalid key ({})".format(key))
        w = np.fromfile(f, dtype=np.int32, count=1)[0]
        h = np.fromfile(f, dtype=np.int32, count=1)[0]
        data = np.fromfile(f, dtype=np.float32, count=2 * h * w).reshape((h, w, 2))
    if device is None:
        return data
    host = torch.from_numpy(data).pin_memory()
    return host.to(device, non_blocking=True)


def write_flow(flow_path, flow):
    """The .flo writer matching read_flow (the reference ships none)."""
    if isinstance(flow, torch.Tensor):
        flow = flow.detach().cpu().numpy()
    flow = np.asarray(flow, np.float32)
    h, w = flow.shape[:2]
    with open(flow_path, "wb") as f:
        np.array([FLO_MAGIC], np.float32).tofile(f)
        np.array([w, h], np.int32).tofile(f)
        flow.tofile(f)


def create_composite_image(fg, bg, alpha, out_dtype=torch.float64):
    """reader.create_composite_image (reader.py:72-79): alpha*fg + (1-alpha)*bg per channel.

    numpy in -> float64 numpy out (like the reference); device tensors -> float64 device tensor from the
    vm_composite_image kernel (bit-identical to the numpy expression; pass out_dtype=torch.float32 to halve
    the write).
    """
    if isinstance(fg, torch.Tensor):
        from vmatting import ops
        return ops.composite_image(fg, bg, alpha, out_dtype=out_dtype)
    a = np.asarray(alpha, np.float64)[..., None]
    return a * np.asarray(fg) + (1.0 - a) * np.asarray(bg)


def _compose_frame(cmp, bg, alpha, new_bg, mode):
    """One host frame through ops.matte_compose: uint8 [h,w,3] cmp / bg (/ new_bg), alpha f32 or f64 [h,w]."""
    from vmatting import ops
    alpha = np.asarray(alpha)
    if alpha.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("alpha must be float32 or float64, got %s" % alpha.dtype)
    planes = [np.asarray(a) for a in (cmp, bg) + (() if new_bg is None else (new_bg,))]
    for name, a in zip(("cmp", "bg", "new_bg"), planes):
        if a.dtype != np.uint8:
            raise TypeError("%s must be uint8, got %s" % (name, a.dtype))
        if a.ndim != 3 or a.shape[2] != 3 or a.shape != planes[0].shape:
            raise ValueError("%s must be [h,w,3] like cmp %s, got %s" % (name, planes[0].shape, a.shape))
    if alpha.shape != planes[0].shape[:2]:
        raise ValueError("alpha must be [h,w] = %s, got %s" % (planes[0].shape[:2], alpha.shape))
    dev = [torch.from_numpy(np.ascontiguousarray(a)[None]).cuda() for a in planes]
    a32 = torch.from_numpy(np.ascontiguousarray(alpha.astype(np.float32))[None]).cuda()
    return ops.matte_compose(a32, dev[0], dev[1], dev[2] if len(dev) == 3 else None, mode=mode)[0].cpu().numpy()


def estimate_foreground(cmp, bg, alpha, premultiplied=False):
    """The inverse of create_composite_image for a known background: the foreground layer of one frame as uint8
    [h,w,4] BGRA, its alpha channel the 8-bit matte q = rint(alpha * 255).  Straight (the default) is
    bg + (cmp - bg) * 255 / q, zero where q = 0: the layout of the reference's foreground files (data.create_bgra), so
    cv2.imwrite of it is a file read_fg_img reads back.  ``premultiplied``: cmp - (255 - q) * bg / 255, the form
    compositors take.  cmp, bg uint8 [h,w,3] BGR; alpha f32 or f64 [h,w] (f64 is rounded to f32 first).  numpy in ->
    numpy out, through the vm_matte_compose kernel (float64 arithmetic, one rounding)."""
    return _compose_frame(cmp, bg, alpha, None, "premul" if premultiplied else "bgra")


def replace_background(cmp, bg, alpha, new_bg):
    """One frame moved onto another plate: cmp + (1 - alpha) * (new_bg - bg) as uint8 [h,w,3] BGR, exact where the
    frame is a composite over bg (no foreground estimate, no division; the old plate does not bleed through at partly
    transparent pixels as it does in alpha * cmp + (1 - alpha) * new_bg).  cmp, bg, new_bg uint8 [h,w,3]; alpha f32 or
    f64 [h,w] (f64 is rounded to f32 first), clamped to [0,1].  numpy in -> numpy out, through the vm_matte_compose
    kernel (float64 arithmetic, one rounding)."""
    return _compose_frame(cmp, bg, alpha, new_bg, "over")


def score_matte(pred, gt, trimap=None):
    """The per-frame matting metrics of one matte against its ground truth: {"count": pixels of the region, "sad": sum
    |pred - gt|, "mse": mean squared error, "grad": summed Gaussian-gradient error} over the trimap's unknown region
    (bytes that are neither 0 nor 255; every pixel without a trimap).  pred, gt [h,w], each f32 or f64 in [0,1] (f64
    is rounded to f32 first, values are clamped) or uint8 (q / 255); trimap uint8 [h,w] or None.  numpy in -> floats
    out, through the vm_matte_score kernel (include/vmatting.h; published tables quote SAD / 1000, MSE * 1000 and
    Grad / 1000).  A clip, and its temporal metrics, go through vmatting.MatteScorer."""
    from vmatting import ops
    planes = []
    for name, a in (("pred", pred), ("gt", gt)):
        a = np.asarray(a)
        if a.dtype == np.float64:
            a = a.astype(np.float32)
        if a.dtype not in (np.dtype(np.float32), np.dtype(np.uint8)):
            raise TypeError("%s must be float32, float64 or uint8, got %s" % (name, a.dtype))
        if a.ndim != 2 or a.size == 0 or a.shape != np.shape(pred):
            raise ValueError("%s must be [h,w] like pred %s, got %s" % (name, np.shape(pred), a.shape))
        planes.append(a)
    if trimap is not None:
        trimap = np.asarray(trimap)
        if trimap.dtype != np.uint8:
            raise TypeError("trimap must be uint8, got %s" % trimap.dtype)
        if trimap.shape != planes[0].shape:
            raise ValueError("trimap must be [h,w] = %s, got %s" % (planes[0].shape, trimap.shape))
        planes.append(trimap)
    dev = [torch.from_numpy(np.ascontiguousarray(a)[None]).cuda() for a in planes]
    res = ops.score_summary(ops.matte_score(dev[0], dev[1], dev[2] if len(dev) == 3 else None))
    return {k: float(res[k][0]) for k in ("count", "sad", "mse", "grad")}


def upsample_matte(alpha_lo, cmp_u8, scale, **options):
    """The matte of a reduced frame carried back to the frame's size by a guided filter: what FrameStream(scale=...)
    does with the model's output.  alpha_lo [hm,wm] f32 (or f64, rounded to f32 first), the matte of the model on
    frames_reduce(cmp_u8, scale); cmp_u8 uint8 [h,w,3] BGR with hm = ceil(h / scale), wm = ceil(w / scale); ``scale``
    2..4; ``options`` over ops.GUIDED_DEFAULTS (r, eps) -> f32 [h,w] in [0,1] (ops.guided_upsample, include/vmatting.h).
    numpy in, numpy out, through the kernels."""
    from vmatting import ops
    who = "upsample_matte"
    scale = ops.check_scale(who, scale)
    opts = ops.guided_options(who, options)
    alpha_lo, cmp_u8 = np.asarray(alpha_lo), np.asarray(cmp_u8)
    if alpha_lo.dtype == np.float64:
        alpha_lo = alpha_lo.astype(np.float32)
    if alpha_lo.dtype != np.float32:
        raise TypeError("%s: alpha_lo must be float32 or float64, got %s" % (who, alpha_lo.dtype))
    if cmp_u8.dtype != np.uint8:
        raise TypeError("%s: cmp must be uint8, got %s" % (who, cmp_u8.dtype))
    if cmp_u8.ndim != 3 or cmp_u8.shape[2] != 3 or cmp_u8.size == 0:
        raise ValueError("%s: cmp must be [h,w,3] BGR, got %s" % (who, cmp_u8.shape))
    lo = ops.reduced_size(cmp_u8.shape[0], cmp_u8.shape[1], scale)
    if alpha_lo.shape != lo:
        raise ValueError("%s: alpha_lo must be [hm,wm] = %s for cmp %s at scale %d, got %s" %
                         (who, lo, cmp_u8.shape, scale, alpha_lo.shape))
    dev = [torch.from_numpy(np.ascontiguousarray(a)[None]).cuda() for a in (alpha_lo, cmp_u8)]
    return ops.guided_upsample(dev[0], dev[1], scale, **opts)[0, :, :, 0].cpu().numpy()


def fill_enclosed(trimap_u8, max_area=0):
    """A trimap with its enclosed background turned unknown: 128 on every 4-connected region of zero bytes that does not
    touch the frame's border and has at most ``max_area`` pixels (0: any area), every other byte as it was
    (ops.trimap_fill_enclosed, include/vmatting.h).  A region of sure background that the subject surrounds is far more
    often foreground that matches the plate than background; a hole that reaches the border is not filled.  trimap_u8
    uint8, one frame [H,W] or a stack [N,H,W]; numpy arrays return numpy, device tensors stay on the device."""
    from vmatting import ops
    who = "fill_enclosed"
    device = isinstance(trimap_u8, torch.Tensor)
    if not device:
        trimap_u8 = np.ascontiguousarray(trimap_u8)
    if trimap_u8.dtype not in (torch.uint8, np.dtype(np.uint8)):
        raise TypeError("%s: the trimap must be uint8, got %s" % (who, trimap_u8.dtype))
    if len(trimap_u8.shape) not in (2, 3) or min(trimap_u8.shape) < 1:
        raise ValueError("%s: the trimap must be [H,W] or [N,H,W], got %s" % (who, tuple(trimap_u8.shape)))
    max_area = ops.check_int(who, "max_area", max_area, 0)
    single = len(trimap_u8.shape) == 2
    tri = trimap_u8[None] if single else trimap_u8
    if device:
        out = ops.trimap_fill_enclosed(tri.contiguous(), max_area)
    else:
        out = ops.trimap_fill_enclosed(torch.from_numpy(tri).cuda(), max_area).cpu().numpy()
    return out[0] if single else out


def match_plate(cmp_u8, bg_u8, **options):
    """The background plate brought to one frame's exposure: what FrameStream(gain="fit") puts in the plate's place.
    cmp_u8, bg_u8 uint8 [h,w,3] BGR; ``options`` over ops.GAIN_DEFAULTS (band, min_share) -> (plate uint8 [h,w,3], gains
    f32 [3], support int [3]): per channel one gain, the least-squares ratio frame / plate over the pixels near the mode
    of that ratio's histogram, and the plate times it, clamped at 255 (ops.plate_gain_fit, ops.plate_gain_apply,
    include/vmatting.h).  ``support`` counts the pixels the fit rests on; below h w / min_share the gain is 1.  No offset,
    no shadows, nothing local.  numpy in, numpy out, through the kernels."""
    from vmatting import ops
    who = "match_plate"
    opts = ops.gain_options(who, options)
    cmp_u8, bg_u8 = np.asarray(cmp_u8), np.asarray(bg_u8)
    for name, a in (("cmp", cmp_u8), ("bg", bg_u8)):
        if a.dtype != np.uint8:
            raise TypeError("%s: %s must be uint8, got %s" % (who, name, a.dtype))
    if cmp_u8.ndim != 3 or cmp_u8.shape[2] != 3 or cmp_u8.size == 0:
        raise ValueError("%s: cmp must be [h,w,3] BGR, got %s" % (who, cmp_u8.shape))
    if bg_u8.shape != cmp_u8.shape:
        raise ValueError("%s: bg must be [h,w,3] like cmp %s, got %s" % (who, cmp_u8.shape, bg_u8.shape))
    cmp, bg = (torch.from_numpy(np.ascontiguousarray(a)[None]).cuda() for a in (cmp_u8, bg_u8))
    gain, support = ops.plate_gain_fit(cmp, bg, **opts)
    plate = ops.plate_gain_apply(bg, gain)
    return (plate[0].cpu().numpy(), gain[0].cpu().numpy().astype(np.float32) / np.float32(ops.GAIN_ONE),
            support[0].cpu().numpy().astype(np.int64))


def trimap_from_plate(cmp_u8, bg_u8, lo=None, hi=None, r_bg=None, r_fg=None, *, fill=None, gain=None,
                      gain_options=None):
    """The trimap of a frame from its difference to the background plate: what FrameStream(trimap="auto") feeds the
    model, and the trimap of a clip's first frame for ClipStream's alpha0.  cmp_u8 uint8 BGR, one frame [H,W,3] or a
    stack [N,H,W,3]; bg_u8 uint8 [H,W,3] (one plate) or, with a stack, [N,H,W,3] -> uint8 [H,W] or [N,H,W]: 0 where the
    frame equals the plate within ``lo`` levels over a (2 r_bg + 1)^2 window, 255 where it differs by ``hi`` or more
    over a (2 r_fg + 1)^2 window, 128 elsewhere (ops.trimap_from_plate, include/vmatting.h; None: ops.PLATE_DEFAULTS,
    which are untuned).  No shadow model, and no exposure model unless ``gain`` is "fit" (FrameStream's ``gain``): every
    frame is then compared with the plate under that frame's fitted gains (match_plate; ``gain_options`` over
    ops.GAIN_DEFAULTS).  ``fill`` (FrameStream's ``auto_fill``): True, or an integer area cap, turns the enclosed
    background of the result unknown (fill_enclosed); None or False leaves it.  numpy arrays return numpy, device tensors
    stay on the device."""
    from vmatting import ops
    who = "trimap_from_plate"
    cap = ops.check_fill(who, fill)
    gopts = ops.check_gain_mode(who, gain, gain_options)
    if isinstance(cmp_u8, torch.Tensor) != isinstance(bg_u8, torch.Tensor):
        raise TypeError("%s: cmp and bg are both numpy arrays or both torch tensors" % who)
    given = {"lo": lo, "hi": hi, "r_bg": r_bg, "r_fg": r_fg}
    opts = ops.plate_options(who, {k: v for k, v in given.items() if v is not None})
    device = isinstance(cmp_u8, torch.Tensor)
    if not device:
        cmp_u8, bg_u8 = np.ascontiguousarray(cmp_u8), np.ascontiguousarray(bg_u8)
    single = len(cmp_u8.shape) == 3
    cmp = cmp_u8[None] if single else cmp_u8
    if single and len(bg_u8.shape) != 3:
        raise ValueError("%s: one [H,W,3] frame takes one [H,W,3] plate, got %s" % (who, tuple(bg_u8.shape)))
    ops._check_u8_frames(cmp, bg_u8, None)
    if device:
        cmp, bg = cmp.contiguous(), bg_u8.contiguous()
    else:
        cmp, bg = torch.from_numpy(cmp).cuda(), torch.from_numpy(bg_u8).cuda()
    if gopts is not None:
        bg = ops.plate_gain_apply(bg, ops.plate_gain_fit(cmp, bg, **gopts)[0])
    out = ops.trimap_from_plate(cmp, bg, **opts)
    if cap is not None:
        ops.trimap_fill_enclosed(out, cap, out=out)
    if not device:
        out = out.cpu().numpy()
    return out[0] if single else out


def plate_from_clip(frames_u8, capacity=64, every=1):
    """The background plate of a locked-off clip estimated from its own frames, for a shot without a clean plate:
    frames_u8 uint8 BGR [N,H,W,3] -> (plate uint8 [H,W,3], spread uint8 [H,W]).  Up to ``capacity`` (even, 2..64) of
    every ``every``-th frame, spread evenly over the clip (plate.SampleSchedule), and per byte their lower median;
    ``spread`` is the per-pixel interquantile range, large where the subject stood for a good share of the clip and the
    plate is not to be trusted (ops.plate_from_samples, include/vmatting.h).  No exposure or flicker compensation.
    numpy arrays return numpy, device tensors stay on the device."""
    from vmatting.plate import PlateEstimator
    who = "plate_from_clip"
    if not isinstance(frames_u8, (np.ndarray, torch.Tensor)):
        raise TypeError("%s: frames must be a numpy array or a device tensor, got %s" % (who, type(frames_u8).__name__))
    if str(frames_u8.dtype).split(".")[-1] != "uint8":
        raise TypeError("%s: frames must be uint8, got %s" % (who, frames_u8.dtype))
    shape = tuple(frames_u8.shape)
    if len(shape) != 4 or shape[3] != 3 or min(shape) < 1:
        raise ValueError("%s: frames must be [N,H,W,3] BGR, got %s" % (who, shape))
    est = PlateEstimator(shape[1], shape[2], capacity, every)
    plate, spread = est.add(frames_u8).result()
    if isinstance(frames_u8, torch.Tensor):
        return plate, spread
    return plate.cpu().numpy(), spread.cpu().numpy()


def read_fg_img(img_path):
    """reader.read_fg_img (reader.py:10-18) via PIL: returns (alpha in [0,1] float64, BGR uint8)."""
    from PIL import Image
    im = np.asarray(Image.open(img_path))
    if im.dtype == np.uint16:
        im = (((im + 1) / 256.0) - 1).astype(np.uint8)  # reader.py:13-14
    bgr = im[:, :, [2, 1, 0]]
    alpha = im[:, :, 3] / 255.0
    return alpha, bgr
