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


U8 = (torch.uint8,)


def _stack(a, single=True):
    """``a``, one frame (``single``) or a stack of them, checked already, as a contiguous device tensor with a leading
    frame axis: a host array is uploaded, a device tensor stays on its device (made contiguous where it is not)."""
    if isinstance(a, torch.Tensor):
        a = a.contiguous()
    else:
        a = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return a[None] if single else a


def _like(out, given, single):
    """A device result with a leading frame axis as what the caller gave: its one frame for one frame (``single``), a
    numpy array for a numpy array."""
    out = out[0] if single else out
    return out if isinstance(given, torch.Tensor) else out.cpu().numpy()


def _compose_frame(cmp, bg, alpha, new_bg, mode):
    """One host frame through ops.matte_compose: uint8 [h,w,3] cmp / bg (/ new_bg), alpha f32 or f64 [h,w]."""
    from vmatting import ops
    who = "replace_background" if mode == "over" else "estimate_foreground"
    alpha, cmp, bg = np.asarray(alpha), np.asarray(cmp), np.asarray(bg)
    h, w, _ = ops.check_array(who, "cmp", cmp, U8, "h,w,3")
    ops.check_array(who, "bg", bg, U8, "h,w,3", h=h, w=w)
    if new_bg is not None:
        new_bg = np.asarray(new_bg)
        ops.check_array(who, "new_bg", new_bg, U8, "h,w,3", h=h, w=w)
    ops.check_array(who, "alpha", alpha, (torch.float32, torch.float64), "h,w", h=h, w=w)
    a32 = _stack(np.asarray(alpha, np.float32))  # (f64 rounded to f32; f32 as it is)
    out = ops.matte_compose(a32, _stack(cmp), _stack(bg), None if new_bg is None else _stack(new_bg), mode=mode)
    return _like(out, alpha, True)


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
    who, matte = "score_matte", (torch.float32, torch.float64, torch.uint8)
    pred, gt = np.asarray(pred), np.asarray(gt)
    h, w = ops.check_array(who, "pred", pred, matte, "h,w")
    ops.check_array(who, "gt", gt, matte, "h,w", h=h, w=w)
    if trimap is not None:
        trimap = np.asarray(trimap)
        ops.check_array(who, "trimap", trimap, U8, "h,w", h=h, w=w)
    pred, gt = (a.astype(np.float32) if a.dtype == np.float64 else a for a in (pred, gt))
    res = ops.score_summary(ops.matte_score(_stack(pred), _stack(gt), None if trimap is None else _stack(trimap)))
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
    h, w, _ = ops.check_array(who, "cmp", cmp_u8, U8, "h,w,3")
    hm, wm = ops.reduced_size(h, w, scale)  # (ceil(h / scale), ceil(w / scale))
    ops.check_array(who, "alpha_lo", alpha_lo, (torch.float32, torch.float64), "hm,wm", hm=hm, wm=wm)
    out = ops.guided_upsample(_stack(np.asarray(alpha_lo, np.float32)), _stack(cmp_u8), scale, **opts)
    return _like(out[..., 0], alpha_lo, True)


def fill_enclosed(trimap_u8, max_area=0):
    """A trimap with its enclosed background turned unknown: 128 on every 4-connected region of zero bytes that does not
    touch the frame's border and has at most ``max_area`` pixels (0: any area), every other byte as it was
    (ops.trimap_fill_enclosed, include/vmatting.h).  A region of sure background that the subject surrounds is far more
    often foreground that matches the plate than background; a hole that reaches the border is not filled.  trimap_u8
    uint8, one frame [H,W] or a stack [N,H,W]; numpy arrays return numpy, device tensors stay on the device."""
    from vmatting import ops
    who = "fill_enclosed"
    if not isinstance(trimap_u8, torch.Tensor):
        trimap_u8 = np.asarray(trimap_u8)
    shape = ops.check_array(who, "the trimap", trimap_u8, U8, "H,W | N,H,W", ops.EITHER, strided=True)
    single = len(shape) == 2
    max_area = ops.check_int(who, "max_area", max_area, 0)
    return _like(ops.trimap_fill_enclosed(_stack(trimap_u8, single), max_area), trimap_u8, single)


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
    h, w, _ = ops.check_array(who, "cmp", cmp_u8, U8, "h,w,3")
    ops.check_array(who, "bg", bg_u8, U8, "h,w,3", h=h, w=w)
    cmp, bg = _stack(cmp_u8), _stack(bg_u8)
    gain, support = ops.plate_gain_fit(cmp, bg, **opts)
    plate, gain, support = (_like(t, cmp_u8, True) for t in (ops.plate_gain_apply(bg, gain), gain, support))
    return plate, gain.astype(np.float32) / np.float32(ops.GAIN_ONE), support.astype(np.int64)


def _aligned_plates(cmp, bg, opts):
    """The device side of align_plate for stacks: cmp u8 [n,h,w,3], bg u8 [n,h,w,3], [1,h,w,3] or [h,w,3] -> (the aligned plates
    u8 [n,h,w,3], params f32 [n,8], support int32 [n])."""
    from vmatting import ops
    n, h, w, _ = cmp.shape
    bg = bg[None] if bg.dim() == 3 else bg
    levels = opts["levels"]
    floats = (ops.flow_pyramid_floats(h, w, levels) + 3) // 4 * 4
    work = torch.empty(ops.flow_workspace_bytes(h, w, levels), dtype=torch.uint8, device=cmp.device)
    rows = [ops.frame_pyramids(t, levels, torch.zeros((len(t), floats), dtype=torch.float32, device=cmp.device), work)
            for t in (cmp, bg)]
    params, support = ops.plate_align_fit(rows[0], rows[1], h, w, **opts)
    return ops.plate_align_apply(bg, params), params, support


def align_plate(cmp_u8, bg_u8, **options):
    """The background plate brought to one frame's position: what FrameStream(align="fit") puts in the plate's place.
    cmp_u8, bg_u8 uint8 [h,w,3] BGR, h and w at least 16; ``options`` over ops.ALIGN_DEFAULTS (iters, tol, min_share,
    reach, levels) -> (plate uint8 [h,w,3], params f32 [7] = (p0..p5, g), support int): one affine map, fitted coarse to
    fine between the grey pyramids of frame and plate over the pixels that agree within ``tol`` grey levels, and the
    plate resampled through it (ops.plate_align_fit, ops.plate_align_apply, include/vmatting.h).  The frame's pixel
    (x, y) sees the plate at (x + p0 xc + p1 yc + p2, y + p3 xc + p4 yc + p5), xc = x - (w - 1) / 2, yc = y - (h - 1) /
    2; g is the fitted photometric gain, reported and not applied.  ``support`` counts the pixels within tol / 4 of the
    fit; below h w / min_share, or with a corner moved by more than min(h, w) / reach, the map is the identity.  One
    global map: no parallax, no lens distortion.  numpy in, numpy out, through the kernels."""
    from vmatting import ops
    who = "align_plate"
    opts = ops.align_options(who, options)
    cmp_u8, bg_u8 = np.asarray(cmp_u8), np.asarray(bg_u8)
    h, w, _ = ops.check_array(who, "cmp", cmp_u8, U8, "h,w,3")
    ops.check_array(who, "bg", bg_u8, U8, "h,w,3", h=h, w=w)
    ops.check_flow_options(who, h, w, opts["levels"])
    plate, params, support = (_like(t, cmp_u8, True) for t in _aligned_plates(_stack(cmp_u8), _stack(bg_u8), opts))
    return plate, params[:ops.ALIGN_PARAMS], int(support)


def smooth_mattes(mattes, frames_u8, flows=None, **options):
    """The mattes of a clip filtered along time: what FrameStream(smooth="flow") does to the model's output, on a clip
    in host memory.  mattes f32 (clamped to [0,1]) or uint8 (q / 255) [n,h,w], the clip's frames uint8 [n,h,w,3] BGR,
    ``flows`` f32 [n,h,w,2]: frame j's backward flow into frame j - 1 in read_flow layout (entry 0 is not read), or None
    to estimate them from consecutive frames (ops.estimate_flow at its defaults; h and w at least 16); ``options`` over
    ops.SMOOTH_DEFAULTS (strength, tol, jump) -> f32 [n,h,w]: frame 0 as it is, every later matte pulled towards the
    filtered matte before it along the flow, gated by the frames' colours and the matte's jump (ops.matte_smooth,
    include/vmatting.h).  One frame of history, no look-ahead, no cut detection.  numpy in, numpy out, through the
    kernels."""
    from vmatting import ops
    who = "smooth_mattes"
    opts = ops.smooth_options(who, options)
    mattes, frames_u8 = np.asarray(mattes), np.asarray(frames_u8)
    n, h, w = ops.check_array(who, "mattes", mattes, (torch.float32, torch.uint8), "n,h,w")
    ops.check_array(who, "frames", frames_u8, U8, "n,h,w,3", n=n, h=h, w=w)
    if flows is None:
        ops.check_flow_options(who, h, w)
    else:
        flows = np.asarray(flows)
        ops.check_array(who, "flows", flows, (torch.float32,), "n,h,w,2", n=n, h=h, w=w)
    if mattes.dtype == np.uint8:
        mattes = mattes.astype(np.float32) / np.float32(255.0)
    alpha, cmp = _stack(mattes, False), _stack(frames_u8, False)
    if flows is None:
        backward = torch.zeros((n, h, w, 2), dtype=torch.float32, device=cmp.device)
        work = torch.empty(ops.flow_workspace_bytes(h, w), dtype=torch.uint8, device=cmp.device)
        for j in range(1, n):
            ops.estimate_flow(cmp[j], cmp[j - 1], out=backward[j], work=work)
    else:
        backward = _stack(flows, False)
    return ops.matte_smooth(alpha, cmp, backward, out=alpha, **opts).cpu().numpy()


def trimap_from_plate(cmp_u8, bg_u8, lo=None, hi=None, r_bg=None, r_fg=None, *, fill=None, gain=None,
                      gain_options=None, align=None, align_options=None, shadow=None, shadow_options=None):
    """The trimap of a frame from its difference to the background plate: what FrameStream(trimap="auto") feeds the
    model, and the trimap of a clip's first frame for ClipStream's alpha0.  cmp_u8 uint8 BGR, one frame [H,W,3] or a
    stack [N,H,W,3]; bg_u8 uint8 [H,W,3] (one plate) or, with a stack, [N,H,W,3] -> uint8 [H,W] or [N,H,W]: 0 where the
    frame equals the plate within ``lo`` levels over a (2 r_bg + 1)^2 window, 255 where it differs by ``hi`` or more
    over a (2 r_fg + 1)^2 window, 128 elsewhere (ops.trimap_from_plate, include/vmatting.h; None: ops.PLATE_DEFAULTS,
    which are untuned).  No shadow model unless ``shadow`` is "chroma" (FrameStream's ``shadow``): after ``align`` and
    ``gain``, on the plate they produce, a pixel that is the plate's colour under a light ratio a shadow may have is
    measured by its distance to the line through that colour (``shadow_options`` over ops.SHADOW_DEFAULTS, untuned; a
    per-pixel colour test: a subject that is a darker version of the plate's own hue passes as shadow and is labelled
    background).  No exposure model unless ``gain`` is "fit" (FrameStream's ``gain``): every
    frame is then compared with the plate under that frame's fitted gains (match_plate; ``gain_options`` over
    ops.GAIN_DEFAULTS).  No motion model unless ``align`` is "fit" (FrameStream's ``align``): the plate is first, ahead
    of the gain, resampled through each frame's fitted affine map (align_plate; ``align_options`` over
    ops.ALIGN_DEFAULTS; H and W at least 16).  ``fill`` (FrameStream's ``auto_fill``): True, or an integer area cap, turns the enclosed
    background of the result unknown (fill_enclosed); None or False leaves it.  numpy arrays return numpy, device tensors
    stay on the device."""
    from vmatting import ops
    who = "trimap_from_plate"
    cap = ops.check_fill(who, fill)
    gopts = ops.check_gain_mode(who, gain, gain_options)
    aopts = ops.check_align_mode(who, align, align_options)
    sopts = ops.check_shadow_mode(who, shadow, shadow_options)
    if isinstance(cmp_u8, torch.Tensor) != isinstance(bg_u8, torch.Tensor):
        raise TypeError("%s: cmp and bg are both numpy arrays or both torch tensors" % who)
    given = {"lo": lo, "hi": hi, "r_bg": r_bg, "r_fg": r_fg}
    opts = ops.plate_options(who, {k: v for k, v in given.items() if v is not None})
    if not isinstance(cmp_u8, torch.Tensor):
        cmp_u8, bg_u8 = np.asarray(cmp_u8), np.asarray(bg_u8)
    shape = ops.check_array(who, "cmp", cmp_u8, U8, "H,W,3 | N,H,W,3", ops.EITHER, strided=True)
    single = len(shape) == 3
    if single:  # one [H,W,3] frame takes one [H,W,3] plate
        ops.check_array(who, "bg", bg_u8, U8, "H,W,3", ops.EITHER, strided=True, H=shape[0], W=shape[1])
    else:
        ops.check_array(who, "bg", bg_u8, U8, "N,H,W,3 | 1,H,W,3 | H,W,3", ops.EITHER, strided=True, N=shape[0],
                        H=shape[1], W=shape[2])
    if aopts is not None:
        ops.check_flow_options(who, shape[-3], shape[-2], aopts["levels"])
    cmp, bg = _stack(cmp_u8, single), _stack(bg_u8, False)
    if aopts is not None:
        bg = _aligned_plates(cmp, bg, aopts)[0]
    if gopts is not None:
        bg = ops.plate_gain_apply(bg, ops.plate_gain_fit(cmp, bg, **gopts)[0])
    out = ops.trimap_from_plate(cmp, bg, shadow=sopts, **opts)
    if cap is not None:
        ops.trimap_fill_enclosed(out, cap, out=out)
    return _like(out, cmp_u8, single)


def plate_from_clip(frames_u8, capacity=64, every=1):
    """The background plate of a locked-off clip estimated from its own frames, for a shot without a clean plate:
    frames_u8 uint8 BGR [N,H,W,3] -> (plate uint8 [H,W,3], spread uint8 [H,W]).  Up to ``capacity`` (even, 2..64) of
    every ``every``-th frame, spread evenly over the clip (plate.SampleSchedule), and per byte their lower median;
    ``spread`` is the per-pixel interquantile range, large where the subject stood for a good share of the clip and the
    plate is not to be trusted (ops.plate_from_samples, include/vmatting.h).  No exposure or flicker compensation.
    numpy arrays return numpy, device tensors stay on the device."""
    from vmatting.plate import PlateEstimator
    from vmatting import ops
    # (the clip's size for the estimator, whose add() copies the frames it keeps: any strides)
    _, h, w, _ = ops.check_array("plate_from_clip", "frames", frames_u8, U8, "N,H,W,3", ops.EITHER, strided=True)
    plate, spread = PlateEstimator(h, w, capacity, every).add(frames_u8).result()
    return _like(plate, frames_u8, False), _like(spread, frames_u8, False)


def read_fg_img(img_path):
    """reader.read_fg_img (reader.py:10-18) via PIL: returns (alpha in [0,1] float64, BGR uint8)."""
    from PIL import Image
    im = np.asarray(Image.open(img_path))
    if im.dtype == np.uint16:
        im = (((im + 1) / 256.0) - 1).astype(np.uint8)  # reader.py:13-14
    bgr = im[:, :, [2, 1, 0]]
    alpha = im[:, :, 3] / 255.0
    return alpha, bgr
