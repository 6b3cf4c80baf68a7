"""Streamed matting of a decoded clip: uint8 frames in from the host, quantised mattes back out.

video.VideoMatter serves frames that are already network input on the device.  A decoded clip is uint8 BGR composites,
a uint8 BGR background (often one static plate) and uint8 trimaps in host memory, and its user wants 8- or 16-bit
mattes back.  FrameStream moves chunks of such frames through ``depth`` slots:

    host arrays -> pinned buffers -> (upload stream) device uint8 -> (compute stream) ops.frames_from_u8 ->
    UNet.forward -> ops.matte_quantize | ops.matte_compose -> pinned output -> numpy

The upload of chunk i + 1 runs beside the compute of chunk i; the download is the tail of each chunk's compute chain.
A full chunk's chain (ingest, forward, quantise, download) is one HIP graph per slot, captured once over the slot's
static buffers on one stream; a short chunk runs the same calls eagerly on leading slices of them.  A frame's matte
is the matte of ``model.forward`` on the reference's feed of that frame (loader.py:45,75-78: the float64 mean
subtraction rounded to f32 once), bit for bit, then quantised.

``trimap="propagate"``: the user has one trimap per shot, not one per frame.  Source items then carry a key trimap
(or None: continue) and the frames' backward flows (or None with ``flow="estimate"``: estimated from the frames), and
the chunk's chain starts with the recurrence tri[j] = ops.trimap_propagate(tri[j-1], backward[j], grow).  It depends on
the frames only, never on the model's output, so the forward stays chunked.

``trimap="auto"``: the user has no trimap at all.  The chunk's chain starts with ops.trimap_from_plate on the uploaded
frames and the plate, followed with ``auto_fill`` by ops.trimap_fill_enclosed in place; nothing is kept between chunks.
With ``shadow="chroma"`` that call measures a pixel that may be the plate in shadow by its chromaticity alone.

``gain="fit"``: the plate and the frames were not shot at one exposure.  The chunk's chain starts with
ops.plate_gain_fit and ops.plate_gain_apply: one gain per frame and colour channel, and a gained copy of the plate per
frame, which everything after it in the chain takes for the background.

``align="fit"``: the plate and the frames are not registered pixel for pixel (a bumped tripod, a handheld plate, a slow
pan).  The chunk's chain starts, ahead of the gain, with the frames' grey pyramids, ops.plate_align_fit and
ops.plate_align_apply: one affine map per frame, and a copy of the plate seen through it per frame, which everything
after it in the chain takes for the background.

``scale=2..4``: the frames are larger than the model should see (2160 x 3840).  The chunk's chain reduces the uploaded
frames (and per-frame backgrounds and trimaps) by ``scale`` (ops.frames_reduce_u8), runs the model on the reduced
frames, and carries its matte back to the frames' size with a guided filter steered by the full-resolution frame
(ops.guided_coeffs, ops.guided_apply); the download then works on full-resolution data as ever.

``smooth="flow"``: mattes made frame by frame shimmer along soft edges.  The chunk's chain then ends, before the
download, with ops.matte_smooth in place on the full-resolution alpha: every matte is pulled towards the previous
filtered matte along the frames' backward flow, gated by the frames' colours and the matte's jump.  It is a filter on
the model's output, so the forward stays chunked; the last filtered matte and the last frame stay on the device for the
next chunk.

This is one process's share of a clip; sharding a clip across ranks stays video.shard's job.
"""

import numpy as np
import torch

from . import ops
from .flow_track import FlowTracker
from .pipeline import OUT_DTYPES  # noqa: F401  (public)
from .pipeline import PER_FRAME, Slot, SlotPipeline, check_new_bg, check_out, check_static_bg
from .split6 import rerun_x6

PROPAGATE = "propagate"
AUTO = "auto"
U8 = (torch.uint8,)


class _Slot(Slot):
    """One chunk in flight: pinned host inputs, their device copies, the frame buffer in the model's input format,
    the f32 alpha, the quantised matte, the pinned output and the two events."""

    def __init__(self, fs):
        n, h, w = fs.chunk, fs.h, fs.w
        u8 = torch.uint8
        given = fs.propagate and not fs.estimate
        super().__init__(fs.device, (("cmp", (n, h, w, 3), u8),
                                     ("bg", (n, h, w, 3) if fs.static_bg is None else None, u8),
                                     ("tri", (n, h, w) if fs.trimap and not (fs.propagate or fs.auto) else None, u8),
                                     ("key", (1, h, w) if fs.propagate else None, u8),
                                     ("bw", (n, h, w, 2) if given else None, torch.float32),
                                     ("nw", (n, h, w, 3) if fs.new_bg is PER_FRAME else None, u8)),
                         n, h, w, fs.out, flag=fs.model.split_mode == "f16x3")  # f16x3: this slot's range flag
        if fs.propagate or fs.auto:  # the chunk's trimaps are made on the device: no pinned twin, nothing uploaded
            self.d_tri = torch.zeros((n, h, w), dtype=u8, device=fs.device)
        if fs.estimate:  # ... and so are its flows (trimap="propagate" and smooth="flow" share them)
            self.d_bw = torch.zeros((n, h, w, 2), dtype=torch.float32, device=fs.device)
        if fs.align is not None:  # the chunk's background seen through its frames' maps, the maps and their support
            self.a_bg = torch.zeros((n, h, w, 3), dtype=u8, device=fs.device)
            self.align = torch.zeros((n, 8), dtype=torch.float32, device=fs.device)
            self.align_support = torch.zeros((n,), dtype=torch.int32, device=fs.device)
        if fs.gain is not None:  # the chunk's background under its frames' gains, the gains and their support
            self.g_bg = torch.zeros((n, h, w, 3), dtype=u8, device=fs.device)
            self.gain = torch.zeros((n, 3), dtype=torch.int32, device=fs.device)
            self.support = torch.zeros((n, 3), dtype=torch.int32, device=fs.device)
        self.graphs = {}  # trimap="propagate" / smooth="flow": the full-chunk graph of an item that restarts the
        #                   chain's state (True: a keyed item, the first item of a run) and of one that continues
        if fs.scale > 1:
            # the model's side of the chunk: the reduced uint8 frames it is fed from, its matte, and the guided
            # filter's coefficients; the frame buffer below is then the model's size too
            h, w = fs.hm, fs.wm
            self.r_cmp = torch.zeros((n, h, w, 3), dtype=u8, device=fs.device)
            per_frame = fs.static_bg is None or fs.gain is not None or fs.align is not None
            self.r_bg = torch.zeros((n, h, w, 3), dtype=u8, device=fs.device) if per_frame else None
            self.r_tri = torch.zeros((n, h, w), dtype=u8, device=fs.device) if fs.trimap else None
            self.alpha_lo = torch.empty((n, h, w, 1), dtype=torch.float32, device=fs.device)
            self.ab = torch.empty((n, h, w, 4), dtype=torch.float32, device=fs.device)
        self.frames = ops.frame_buffer(fs.model, n, h, w)
        self.alpha = torch.empty((n, fs.h, fs.w, 1), dtype=torch.float32, device=fs.device)
        self.graph = None
        self.k = 0       # frames of the chunk in flight


class FrameStream(SlotPipeline):
    """``FrameStream(model, h, w, ...).run(source)`` yields one [k,h,w] numpy matte per item of ``source``, in order.

    ``source`` yields ``(cmp, bg, trimap)``: uint8 numpy arrays [k,h,w,3], [k,h,w,3] | None, [k,h,w] | None with
    1 <= k <= chunk.  ``bg`` is None exactly when ``static_bg`` (uint8 [h,w,3], uploaded once) was given; ``trimap`` is
    None exactly when ``trimap=False`` (a 6-channel UNetImage).  An item's arrays are copied before the next item is
    asked for, so the source may reuse them.  ``out``: "u8" / "u16" mattes (ops.matte_quantize) or the "f32" alpha.

    ``out`` "over" / "bgra" / "premul" applies the matte with the known background (ops.matte_compose) and yields uint8
    [k,h,w,3] frames over a new plate, or [k,h,w,4] BGRA foreground layers (straight / premultiplied; their alpha
    channel is the "u8" matte).  "over" takes ``new_bg``: a uint8 [h,w,3] plate (uploaded once), or "per_frame", and
    then every source item is ``(cmp, bg, trimap, new_bg)`` with new_bg uint8 [k,h,w,3].
    Results lag the source by ``depth - 1`` chunks.  On an f16x3 model a chunk whose activations leave fp16's range is
    run again on bf16x6 before it is yielded and its index is appended to ``overflowed_chunks``.

    ``trimap="propagate"`` (a 7-channel model): the trimaps are propagated on the device from key trimaps by the
    frames' backward flows.  Source items are ``(cmp, bg, key, backward)`` (and new_bg last with "per_frame").
    ``key``: the uint8 [h,w] trimap of the item's first frame, or None to continue from the previous item's last
    frame; the first item of a run carries one, and a later one restarts the chain there.  ``backward``: f32
    [k,h,w,2], frame j's flow into frame j - 1 in reader.read_flow layout (entry 0 is unused when the item has a key);
    None exactly when ``flow="estimate"`` (the default with "propagate"; ``flow="given"`` is the other mode), which
    estimates it from consecutive frames (ops.estimate_flow's arithmetic, ``flow_options`` its levels / warps / iters /
    alpha; h and w at least 16).  Frame j's trimap is
    ops.trimap_propagate(trimap of frame j - 1, backward[j], grow): a label survives where the warp is unambiguous, and
    ``grow`` (0..8) widens the unknown band by that many pixels per frame to absorb flow error.  The mattes are those
    of ``trimap=True`` fed with these trimaps, bit for bit.  ``last_trimap()`` returns the last frame's trimap after a
    run: inspect its drift to place the next key.

    ``trimap="auto"`` (a 7-channel model): no trimap is supplied at all.  Source items are the ordinary
    ``(cmp, bg, None)`` (and new_bg last with "per_frame"), and every frame's trimap is
    ops.trimap_from_plate(cmp, bg, **auto_options) on the device: background where the frame equals the plate, foreground
    where it clearly differs, unknown in between (include/vmatting.h; no exposure model, and no shadow model without
    ``shadow``).  ``auto_options``: a
    dict over ops.PLATE_DEFAULTS (lo, hi, r_bg, r_fg).  The mattes are those of ``trimap=True`` fed with these trimaps,
    bit for bit; reader.trimap_from_plate shows them.  ``auto_fill``: True, or an integer area cap, turns every region
    of sure background that does not reach the frame's border (with a cap: and has at most that many pixels) unknown
    (ops.trimap_fill_enclosed): foreground that matches the plate over a wide area is otherwise a hole in the subject
    that no model output repairs.  A hole that reaches the border is not filled, and a real gap the subject encloses
    becomes unknown too.  None (the default) or False: no fill.

    ``scale`` (1..4, default 1: off): run the model on frames reduced by ``scale`` and upsample its matte with a guided
    filter.  ``h, w`` stay the frames' size, and so do all source items and results; the model runs at
    ceil(h / scale) x ceil(w / scale).  cmp and per-frame backgrounds (the static plate once) are reduced to block means,
    trimaps - given, propagated or automatic, all made at full resolution first - to the block's label where all its
    pixels agree and unknown elsewhere (ops.frames_reduce_u8).  The full-resolution matte is
    ops.guided_upsample(model matte, cmp, scale, **guided_options): per reduced pixel a linear model of the matte in the
    frame's colours over a (2 r + 1)^2 window, regularised by eps, interpolated to every full-resolution pixel and applied
    to its colour (He & Sun, "Fast Guided Filter"; include/vmatting.h).  ``guided_options``: a dict over
    ops.GUIDED_DEFAULTS (r, eps; untuned on real footage), only with scale > 1.  Every ``out`` mode works on the
    full-resolution matte.  scale=1 is the stream without any of this, call for call.

    ``gain`` (None, the default, or "fit"): match the background's exposure to every frame before anything uses it.
    Per frame and colour channel one multiplicative gain is fitted between the frame and the background (the static
    plate, or the item's per-frame ``bg``) on the device (ops.plate_gain_fit, ``gain_options`` a dict over
    ops.GAIN_DEFAULTS: band, min_share; untuned on real footage), and a copy of the background under those gains
    (ops.plate_gain_apply) stands in for it in the rest of the chain: the automatic trimap, the model's feed (with
    ``scale`` its reduction) and the compose modes.  The mattes are those of a stream fed these gained backgrounds as
    per-frame ``bg``, bit for bit; reader.match_plate shows one.  ``last_gains()`` returns the last chunk's gains and
    their support after a run.  What it is not: one gain per channel and frame, so no offset, no shadows, no
    vignetting or local change; a clipped region gets no match; the fit fails where the subject and not the background
    is the largest population of one ratio, or where too little of the plate lies within 16..250 - ``support`` shows
    it, and below h w / min_share the gain is 1; the new plate of out="over" is not gained.  gain=None is the stream
    without any of this, call for call.  ClipStream, VideoMatter and PlateEstimator do not take it.

    ``align`` (None, the default, or "fit"): match the background's position to every frame before anything uses it,
    the gain fit included.  Per frame one affine map (and, as a nuisance parameter, one photometric gain) is fitted
    between the grey pyramids of the frame and of the background (the static plate, or the item's per-frame ``bg``) on
    the device, coarse to fine over the pixels that agree within ``tol`` grey levels (ops.plate_align_fit,
    ``align_options`` a dict over ops.ALIGN_DEFAULTS: iters, tol, min_share, reach, levels; untuned on real footage; h
    and w at least 16), and a copy of the background resampled through the map (ops.plate_align_apply) stands in for it
    in the rest of the chain: the gain fit, the automatic trimap, the model's feed (with ``scale`` its reduction) and
    the compose modes.  The mattes are those of a stream fed these aligned backgrounds as per-frame ``bg``, bit for
    bit; reader.align_plate shows one.  Where the stream estimates flows (smooth="flow", trimap="propagate") at the
    same ``levels``, the frames' pyramids are the flow estimate's own and are not built twice.  ``last_alignment()``
    returns the last chunk's maps and their support after a run.  What it is not: one global affine map per frame, so
    no parallax, no rolling shutter, no lens distortion; a textureless plate has nothing to fit and keeps its place
    (``support`` is 0); so does a frame in which fewer than h w / min_share pixels end within tol / 4 of the fit, and
    one whose fitted corners move by more than min(h, w) / reach; the strip that leaves the plate is replicated border
    and will not be labelled background; the new plate of out="over" is not moved.  align=None is the stream without
    any of this, call for call.  ClipStream, VideoMatter and PlateEstimator do not take it.

    ``shadow`` (None, the default, or "chroma"; only with trimap="auto"): let the automatic trimap tolerate cast
    shadows.  A shadowed background pixel is the plate's colour scaled by a factor below 1 (Horprasert et al., 1999), so
    where the frame's pixel has a light ratio to the background's within floor / 256 .. ceil / 256, and the
    background's mean level is at least ``dark``, the squared distance to the line through the background's colour
    stands for the squared distance to the background itself; everything after that in ops.trimap_from_plate is
    unchanged (include/vmatting.h, all integer).  ``shadow_options``: a dict over ops.SHADOW_DEFAULTS (floor, ceil, dark
    - the values of a numpy prototype, untuned on real footage).  It sees the background the rest of the chain sees:
    aligned and gained where ``align`` and ``gain`` are on.  The mattes are those of ``trimap=True`` fed with
    reader.trimap_from_plate(..., shadow="chroma")'s trimaps, bit for bit.  It keeps no state and works with
    ``auto_fill``, ``scale``, ``gain``, ``align``, ``smooth`` and every ``out``.  On a synthetic scene a
    soft shadow keeping 0.8 or 0.6 of the light has none of its core labelled background without it - at 0.6 some of
    it sure foreground - and 0.72-0.84 with it.  What it is not: a per-pixel colour test, so a subject that is a darker
    version of the plate's own hue passes as shadow and is labelled background (a dark-grey shirt on a light-grey wall,
    any grey on any grey; ``auto_fill`` repairs only an enclosed one); no smoothness or texture test of the light
    ratio and no temporal test; a shadow deeper than ``floor``, or within noise of it, falls back to the plain
    distance, and one such pixel costs its whole (2 r_bg + 3)^2 neighbourhood (with floor 128 a 0.6 shadow holds, a
    0.45 shadow with floor 100 mostly does not); background pixels darker than ``dark`` get no tolerance; only the
    trimap changes - the model still sees the shadowed frame against the unshadowed plate - and out="over" carries the
    shadow onto the new plate additively (cmp - bg), not as a multiplicative shadow pass.  shadow=None is the stream
    without any of this, call for call.  ClipStream, VideoMatter and PlateEstimator do not take it.

    ``smooth`` (None, the default, or "flow"): filter the mattes along time before they are quantised or composed.
    After the forward (and, with ``scale``, the upsampling) frame j's matte is pulled towards the filtered matte of
    frame j - 1, sampled where frame j's backward flow says each pixel came from, by ``strength`` times a weight that
    is 1 where frame j equals the warped frame j - 1 and the matte the warped previous matte, and falls to 0 at a
    colour difference of ``tol`` grey levels or a matte difference of ``jump`` (ops.matte_smooth, include/vmatting.h;
    ``smooth_options`` a dict over ops.SMOOTH_DEFAULTS: strength, tol, jump - the values of a CPU prototype, untuned on
    real footage).  The recurrence runs across chunks: the last filtered matte and the last frame stay on the device.
    It restarts (the frame has no predecessor and keeps its matte) at the first item of a run and, with
    trimap="propagate", at every keyed item.  The flows are those of trimap="propagate" where that is on, estimated or
    given; otherwise they are estimated from consecutive frames (``flow`` None or "estimate", ``flow_options``; h and
    w at least 16), which costs one flow estimate per frame.  It works on the full-resolution matte with every ``out``,
    trimap mode, ``scale`` and ``gain``; the result is ops.matte_smooth run over the whole clip on the unsmoothed
    stream's "f32" mattes, bit for bit; reader.smooth_mattes does that to a clip in host memory.  ``last_weight()``
    returns the weights of the last frame after a run: 0 is where the filter held back.  What it is not: one-sided and
    recursive - one frame of history, no look-ahead; it detects no cuts (a cut is caught only by the colour gate,
    pixel by pixel); the gate is colour-based, so a flicker where subject and plate share a colour passes through;
    its effect is measured on a synthetic clip only, not on a trained model's mattes of real footage.  A
    model whose split_mode is "f16x3" is refused: an overflowed chunk is run again when it is retired, after the next
    chunk has consumed its last matte, so the recurrence could not be repaired.  smooth=None is the stream without any
    of this, call for call.  ClipStream and VideoMatter do not take it.

    If the source raises, or yields a wrong shape, dtype or k, the chunks already taken are finished and yielded, the
    streams are synchronised, and the exception then propagates; the object can run again."""

    def __init__(self, model, h, w, chunk=8, depth=2, trimap=True, static_bg=None, out="u8", graph=True, new_bg=None,
                 flow=None, flow_options=None, grow=1, auto_options=None, auto_fill=None, scale=1, guided_options=None,
                 gain=None, gain_options=None, smooth=None, smooth_options=None, align=None, align_options=None,
                 shadow=None, shadow_options=None):
        h, w, chunk, depth = int(h), int(w), int(chunk), int(depth)
        if h < 1 or w < 1 or chunk < 1 or depth < 1:
            raise ValueError("FrameStream: h, w, chunk and depth must be positive (got %d, %d, %d, %d)" %
                             (h, w, chunk, depth))
        check_out("FrameStream", out)
        # scale: the model's size and the guided filter's options
        self.scale = ops.check_scale("FrameStream", scale, smallest=1)
        if guided_options is not None and self.scale == 1:
            raise ValueError("FrameStream: guided_options go with scale > 1")
        if self.scale > 1:
            self.guided = ops.guided_options("FrameStream: guided_options", guided_options)
            self.hm, self.wm = ops.reduced_size(h, w, self.scale)
        # trimap: one per frame, propagated from keys, made from the plate, or none
        if isinstance(trimap, str) and trimap not in (PROPAGATE, AUTO):
            raise ValueError("FrameStream: trimap must be True, False, %r or %r, got %r" % (PROPAGATE, AUTO, trimap))
        self.propagate = isinstance(trimap, str) and trimap == PROPAGATE
        self.auto = isinstance(trimap, str) and trimap == AUTO
        if (7 if trimap else 6) != model.IN_CH:
            raise ValueError("FrameStream: %s takes %d channels, so trimap must be %s" %
                             (type(model).__name__, model.IN_CH,
                              "True, %r or %r" % (PROPAGATE, AUTO) if model.IN_CH == 7 else False))
        # trimap="auto": the plate trimap's options and the hole filling
        if auto_options is not None and not self.auto:
            raise ValueError("FrameStream: auto_options go with trimap=%r" % AUTO)
        if self.auto:
            self.auto_options = ops.plate_options("FrameStream: auto_options", auto_options)
        if auto_fill is not None and not self.auto:
            raise ValueError("FrameStream: auto_fill goes with trimap=%r" % AUTO)
        self.auto_fill = ops.check_fill("FrameStream: auto_fill", auto_fill)
        # shadow="chroma": the shadow-tolerant distance's options (None: the plain distance)
        if (shadow is not None or shadow_options is not None) and not self.auto:
            raise ValueError("FrameStream: shadow and shadow_options go with trimap=%r" % AUTO)
        self.shadow = ops.check_shadow_mode("FrameStream", shadow, shadow_options)
        # smooth="flow": the filter's options (None: no filter)
        self.smooth = ops.check_smooth_mode("FrameStream", smooth, smooth_options)
        if self.smooth is not None and model.split_mode == "f16x3":
            raise ValueError("FrameStream: smooth=%r does not go with an f16x3 model: an overflowed chunk is run again "
                             "after the next chunk has consumed its last matte" % ops.SMOOTH_FLOW)
        # trimap="propagate": the unknown band's growth; with it or smooth="flow": where the flows come from
        flows = self.propagate or self.smooth is not None
        if not flows and (flow is not None or flow_options is not None):
            raise ValueError("FrameStream: flow and flow_options go with trimap=%r or smooth=%r" %
                             (PROPAGATE, ops.SMOOTH_FLOW))
        self.grow = ops.check_grow("FrameStream", grow)
        if flows:  # (flow=None stands for "estimate"; only the propagation's items carry given flows)
            flow_options = ops.check_flow_mode("FrameStream", flow, flow_options, h, w,
                                               (None,) + ops.FLOW_MODES if self.propagate else (None, "estimate"),
                                               "estimate")
        self.estimate = flows and flow_options is not None
        if self.estimate:
            self.flow_options = flow_options
        # gain="fit": the fit's options (None: no gain)
        self.gain = ops.check_gain_mode("FrameStream", gain, gain_options)
        # align="fit": the fit's options (None: no alignment)
        self.align = ops.check_align_mode("FrameStream", align, align_options)
        if self.align is not None:
            ops.check_flow_options("FrameStream: align", h, w, self.align["levels"])
        # the plates
        static_bg = check_static_bg("FrameStream", static_bg, h, w)
        self.new_bg = check_new_bg("FrameStream", out, new_bg, h, w)
        self.model, self.h, self.w, self.chunk, self.depth = model, h, w, chunk, depth
        self.trimap, self.static_bg, self.out, self.graph = bool(trimap), static_bg, out, bool(graph)
        self.device = model.device
        self.overflowed_chunks = []
        self._plate_lo = self._guided_work = None  # scale > 1: the reduced plate, the guided filter's workspace
        self._gain_work = self._gain_last = None   # gain="fit": the fit's workspace; the last chunk's (slot, frames)
        # align="fit": the fit's workspace, the pyramids of the chunk's frames (None: the flow tracker's) and of its
        # backgrounds (one row for a static plate), the pyramids' workspace, and the last chunk's (slot, frames)
        self._align_work = self._align_rows = self._align_bg_rows = self._align_pyr_work = self._align_last = None
        self._x6 = None
        self._keyed = False      # trimap="propagate": whether this run has had its first key
        self._tri_last = None    # ... and the last frame's trimap, at a fixed device address
        self._started = False    # whether this run has had its first item (smooth="flow" restarts there)
        self._smooth_last = self._smooth_cmp = self._smooth_weight = None  # smooth="flow": what _setup_smooth keeps
        self._smooth_k = 0       # ... and the frames of the last chunk submitted

    # ------------------------------------------------------------------ checks (host only)
    def check_item(self, item):
        """Validate one source item; returns (cmp, bg, trimap, k), and new_bg after them with new_bg="per_frame".
        With trimap="propagate": (cmp, bg, key, k, new_bg | None, backward)."""
        if self.propagate:
            return self._check_propagate_item(item)
        per_frame = self.new_bg is PER_FRAME
        if not isinstance(item, (tuple, list)) or len(item) != 3 + per_frame:
            raise ValueError("FrameStream: the source yields (cmp, bg, trimap%s)" %
                             (", new_bg) with new_bg='per_frame'" if per_frame else ") triples"))
        cmp, bg, tri = item[:3]
        if self.auto and tri is not None:
            raise ValueError("FrameStream: with trimap=%r the trimaps are made from the plate: the item's trimap is "
                             "None" % AUTO)
        k, nw = self._check_frames(cmp, bg, tri, item[3] if per_frame else None)
        return (cmp, bg, tri, k, nw) if per_frame else (cmp, bg, tri, k)

    def _check_frames(self, cmp, bg, tri, nw):
        """The frames of one item: cmp, bg | None, the per-frame trimaps | None, and new_bg with new_bg="per_frame"
        -> (k, new_bg)."""
        k = ops.check_array("FrameStream", "cmp", cmp, U8, "k,h,w,3", h=self.h, w=self.w)[0]
        if (bg is None) != (self.static_bg is not None):
            raise ValueError("FrameStream: bg is None exactly when a static_bg was given")
        if not (self.propagate or self.auto) and (tri is None) == self.trimap:
            raise ValueError("FrameStream: trimap is None exactly when trimap=False")
        for name, a, shapes in (("bg", bg, "k,h,w,3"), ("trimap", tri, "k,h,w")):
            if a is not None:
                ops.check_array("FrameStream", name, a, U8, shapes, k=k, h=self.h, w=self.w)
        if k > self.chunk:
            raise ValueError("FrameStream: an item of %d frames exceeds chunk=%d" % (k, self.chunk))
        if self.new_bg is PER_FRAME:
            ops.check_array("FrameStream", "new_bg", nw, U8, "k,h,w,3", k=k, h=self.h, w=self.w)
        return k, nw

    def _check_propagate_item(self, item):
        per_frame = self.new_bg is PER_FRAME
        if not isinstance(item, (tuple, list)) or len(item) != 4 + per_frame:
            raise ValueError("FrameStream: with trimap='propagate' the source yields (cmp, bg, key, backward%s)" %
                             (", new_bg) with new_bg='per_frame'" if per_frame else ")"))
        cmp, bg, key, bw = item[:4]
        if key is None and not self._keyed:
            raise ValueError("FrameStream: the first item of a run carries a key trimap")
        if (bw is None) != self.estimate:
            raise ValueError("FrameStream: backward is None exactly when flow='estimate'")
        if key is not None:
            ops.check_array("FrameStream", "key", key, U8, "h,w", h=self.h, w=self.w)
        k, nw = self._check_frames(cmp, bg, None, item[4] if per_frame else None)
        if bw is not None:
            ops.check_array("FrameStream", "backward", bw, (torch.float32,), "k,h,w,2", k=k, h=self.h, w=self.w)
        self._keyed = True
        return cmp, bg, key, k, nw, bw

    # ------------------------------------------------------------------ device side
    def _setup(self):
        self.model.prepare()
        self._make_streams()
        self._upload_plates()
        if self.scale > 1:  # the plate at the model's size, once; one workspace for every slot, like _auto_work
            if self._plate is not None and self.gain is None and self.align is None:  # (a gained or aligned plate is
                #                                                                       reduced per chunk)
                self._plate_lo = ops.frames_reduce_u8(self._plate[None], self.scale)
            self._guided_work = torch.zeros(ops.guided_workspace_bytes(self.chunk, self.hm, self.wm), dtype=torch.uint8,
                                            device=self.device)
        if self.gain is not None:  # one workspace for every slot, like _auto_work
            self._gain_work = torch.zeros(ops.plate_gain_workspace_bytes(self.chunk), dtype=torch.uint8,
                                          device=self.device)
        if self.estimate:  # the pyramids of the previous chunk's last frame and of this chunk's, once for every slot
            self._flow = FlowTracker(self.h, self.w, self.flow_options, self.device, frames=self.chunk)
        if self.align is not None:
            self._setup_align()
        if self.propagate:
            self._setup_propagate()
        if self.smooth is not None:
            self._setup_smooth()
        if self.auto:  # one workspace for every slot: the chains run one after another on the compute stream
            self._auto_work = torch.zeros(ops.trimap_from_plate_workspace_bytes(self.chunk, self.h, self.w),
                                          dtype=torch.uint8, device=self.device)
            if self.auto_fill is not None:
                self._fill_work = torch.zeros(ops.trimap_fill_enclosed_workspace_bytes(self.chunk, self.h, self.w),
                                              dtype=torch.uint8, device=self.device)
        self._slots = [_Slot(self) for _ in range(self.depth)]
        torch.cuda.synchronize(self.device)  # the plates and the zeroed pad channels, before another stream reads them
        if self._stateful and self.graph:
            # captured here, not with the first full chunk: a capture runs its chain once to warm up, and that run
            # would move the chain's state (the last trimap, the last pyramid, the last filtered matte) one chunk ahead
            # of the clip
            with torch.cuda.stream(self._compute):
                for s in self._slots:
                    for keyed in (True, False):
                        self._capture(s, keyed)
            torch.cuda.synchronize(self.device)

    def _setup_propagate(self):
        """What the trimap chain keeps between chunks, once for every slot (the chains run one after another on the
        compute stream) and at fixed addresses (every slot's graphs read and leave it there): the last frame's
        trimap."""
        dev, h, w = self.device, self.h, self.w
        self._tri_last = torch.zeros((h, w), dtype=torch.uint8, device=dev)
        self._tri_work = torch.zeros(max(ops.trimap_propagate_workspace_bytes(h, w, self.grow), 1), dtype=torch.uint8,
                                     device=dev)

    def _setup_align(self):
        """What the alignment needs besides the slots' buffers, once for every slot: the fit's workspace, the rows of
        the frames' pyramids unless the flow tracker makes them anyway (the same levels), the rows of the backgrounds'
        pyramids - one, filled here, for a static plate - and the pyramids' workspace."""
        dev, h, w, n, levels = self.device, self.h, self.w, self.chunk, self.align["levels"]
        floats = (ops.flow_pyramid_floats(h, w, levels) + 3) // 4 * 4  # every row 16-byte aligned
        rows = lambda k: torch.zeros((k, floats), dtype=torch.float32, device=dev)  # noqa: E731
        self._align_work = torch.zeros(ops.plate_align_workspace_bytes(n, h, w, levels), dtype=torch.uint8, device=dev)
        self._align_pyr_work = torch.zeros(ops.flow_workspace_bytes(h, w, levels), dtype=torch.uint8, device=dev)
        if not (self.estimate and self.flow_options["levels"] == levels):
            self._align_rows = rows(n)
        self._align_bg_rows = rows(1 if self._plate is not None else n)
        if self._plate is not None:
            ops.frame_pyramids(self._plate[None], levels, self._align_bg_rows, self._align_pyr_work)

    def _setup_smooth(self):
        """What the temporal filter keeps between chunks, once for every slot and at fixed addresses like the trimap
        chain's state: the last filtered matte and the last frame; and the weights of the chunk in flight (one buffer:
        the filter writes them in the launches it makes anyway)."""
        dev, h, w = self.device, self.h, self.w
        self._smooth_last = torch.zeros((h, w, 1), dtype=torch.float32, device=dev)
        self._smooth_cmp = torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)
        self._smooth_weight = torch.zeros((self.chunk, h, w, 1), dtype=torch.float32, device=dev)

    @property
    def _stateful(self):
        """Whether the chain keeps state between chunks: a slot then has two graphs, graphs[restart]."""
        return self.propagate or self.smooth is not None

    def _flows(self, s, k, keyed):
        """flow="estimate": the backward flows of the slot's first k frames into s.d_bw, on the current stream: each
        frame's pyramid, then its flow against the previous frame's (none for frame 0 of an item that restarts).  Once
        per chunk, for the trimap chain and the temporal filter alike; the last pyramid stays behind."""
        if self.estimate:
            self._flow.advance(s.d_cmp[:k], s.d_bw[:k], has_previous=not keyed)

    def _trimaps(self, s, k, keyed):
        """The trimaps of the slot's first k frames into s.d_tri, on the current stream: the key or the propagated last
        trimap for frame 0, then frame by frame along s.d_bw.  The last trimap stays behind for the next chunk."""
        for j in range(k):
            if j == 0 and keyed:
                s.d_tri[0].copy_(s.d_key[0])
            else:
                ops.trimap_propagate(s.d_tri[j - 1] if j else self._tri_last, s.d_bw[j], self.grow, out=s.d_tri[j],
                                     work=self._tri_work)
        self._tri_last.copy_(s.d_tri[k - 1])

    def last_trimap(self):
        """trimap="propagate": the uint8 [h,w] trimap of the last frame submitted, once the run has drained."""
        if not self.propagate:
            raise ValueError("FrameStream: last_trimap() goes with trimap='propagate'")
        if self._tri_last is None:
            raise RuntimeError("FrameStream: last_trimap() before any frame was submitted")
        return self._tri_last.cpu().numpy()

    def _smooth(self, s, k, keyed):
        """smooth="flow": the slot's first k full-resolution mattes filtered in place along s.d_bw, frame 0 against
        the last filtered matte and frame unless the item restarts; the last of both stay behind for the next chunk."""
        if self.smooth is not None:
            prev = None if keyed else (self._smooth_last, self._smooth_cmp)
            ops.matte_smooth(s.alpha[:k], s.d_cmp[:k], s.d_bw[:k], prev, out=s.alpha[:k],
                             weight=self._smooth_weight[:k], **self.smooth)
            self._smooth_last.copy_(s.alpha[k - 1])
            self._smooth_cmp.copy_(s.d_cmp[k - 1])

    def last_weight(self):
        """smooth="flow": the f32 [h,w] weights of the last frame submitted, once the run has drained: 1 where the
        filter took ``strength`` of the previous matte, 0 where it held back (or the frame had no predecessor)."""
        if self.smooth is None:
            raise ValueError("FrameStream: last_weight() goes with smooth='flow'")
        if not self._smooth_k:
            raise RuntimeError("FrameStream: last_weight() before any frame was submitted")
        return self._smooth_weight[self._smooth_k - 1, :, :, 0].cpu().numpy()

    def last_gains(self):
        """gain="fit": (gains f32 [k,3] = Q12 gain / 4096, support int [k,3]) of the last chunk submitted, once the run
        has drained."""
        if self.gain is None:
            raise ValueError("FrameStream: last_gains() goes with gain='fit'")
        if self._gain_last is None:
            raise RuntimeError("FrameStream: last_gains() before any frame was submitted")
        s, k = self._gain_last
        return (s.gain[:k].cpu().numpy().astype(np.float32) / np.float32(ops.GAIN_ONE),
                s.support[:k].cpu().numpy().astype(np.int64))

    def last_alignment(self):
        """align="fit": (params f32 [k,7] = (p0..p5, g), support int [k]) of the last chunk submitted, once the run
        has drained: frame pixel (x, y) sees the plate at (x + p0 xc + p1 yc + p2, y + p3 xc + p4 yc + p5), xc = x -
        (w - 1) / 2, yc = y - (h - 1) / 2; (0 .. 0, 1) is the identity."""
        if self.align is None:
            raise ValueError("FrameStream: last_alignment() goes with align='fit'")
        if self._align_last is None:
            raise RuntimeError("FrameStream: last_alignment() before any frame was submitted")
        s, k = self._align_last
        return (s.align[:k, :ops.ALIGN_PARAMS].cpu().numpy(), s.align_support[:k].cpu().numpy().astype(np.int64))

    def _aligned(self, s, k):
        """The background before the gain: the plate, the uploaded per-frame backgrounds, or with align="fit" the slot's
        aligned copy (made by _align)."""
        return s.a_bg[:k] if self.align is not None else self._plates(s, k)[0]

    def _background(self, s, k):
        """What the chain of the slot's first k frames takes for the background: _aligned, or with gain="fit" the
        slot's gained copy of it (made by _before)."""
        return s.g_bg[:k] if self.gain is not None else self._aligned(s, k)

    def _align(self, s, k):
        """align="fit": the maps of the slot's first k frames and the background seen through them into s.a_bg, on the
        current stream: the frames' pyramids (the flow tracker's where _flows has just made them), with per-frame
        backgrounds theirs, the fit, the resampling."""
        if self.align is None:
            return
        o, bg = self.align, self._plates(s, k)[0]
        if self._align_rows is None:
            cmp_rows = self._flow.rows[1:k + 1]
        else:
            cmp_rows = ops.frame_pyramids(s.d_cmp[:k], o["levels"], self._align_rows[:k], self._align_pyr_work)
        if self._plate is None:
            bg_rows = ops.frame_pyramids(bg, o["levels"], self._align_bg_rows[:k], self._align_pyr_work)
        else:
            bg_rows = self._align_bg_rows
        ops.plate_align_fit(cmp_rows, bg_rows, self.h, self.w, out=s.align[:k], support=s.align_support[:k],
                            work=self._align_work, **o)
        ops.plate_align_apply(bg, s.align[:k], out=s.a_bg[:k])

    def _feed(self, s, k, bg):
        """The network input of the slot's first k frames from its uint8 frames; with scale > 1 from their reductions."""
        tri = None if s.d_tri is None else s.d_tri[:k]
        if self.scale == 1:
            ops.frames_from_u8(s.d_cmp[:k], bg, tri, out=s.frames[:k])
            return
        ops.frames_reduce_u8(s.d_cmp[:k], self.scale, out=s.r_cmp[:k])
        if self._plate_lo is None:
            bg = ops.frames_reduce_u8(bg, self.scale, out=s.r_bg[:k])
        else:
            bg = self._plate_lo
        if tri is not None:
            tri = ops.frames_reduce_u8(tri, self.scale, "trimap", out=s.r_tri[:k])
        ops.frames_from_u8(s.r_cmp[:k], bg, tri, out=s.frames[:k])

    def _matte(self, s, k):
        """Where the model's matte of the slot's first k frames goes: the slot's alpha, or with scale > 1 its reduced
        twin."""
        return s.alpha[:k] if self.scale == 1 else s.alpha_lo[:k]

    def _upsample(self, s, k):
        """scale > 1: the model's reduced matte to the slot's full-resolution alpha, steered by the uploaded frames."""
        if self.scale > 1:
            ops.guided_coeffs(s.r_cmp[:k], s.alpha_lo[:k], out=s.ab[:k], work=self._guided_work, **self.guided)
            ops.guided_apply(s.ab[:k], s.d_cmp[:k], self.scale, out=s.alpha[:k])

    def _download(self, s, k):
        """The result of the slot's first k frames from its alpha (and, composed, its uint8 inputs)."""
        s.download(s.alpha[:k], s.d_cmp[:k], self._background(s, k), self._plates(s, k)[1])

    def _before(self, s, k, keyed):
        """What the chain of the slot's first k frames runs before the forward, on the current stream: with
        flow="estimate" the frames' flows, with align="fit" the maps and the aligned background, with gain="fit" the
        gains and the gained background, with trimap="propagate" or "auto" their trimaps, then the ingest.  ``keyed``:
        the item restarts the chain's state."""
        self._flows(s, k, keyed)  # (first: the alignment reads the frames' pyramids it leaves behind)
        self._align(s, k)
        if self.gain is not None:
            bg = self._aligned(s, k)
            ops.plate_gain_fit(s.d_cmp[:k], bg, out=s.gain[:k], support=s.support[:k], work=self._gain_work, **self.gain)
            ops.plate_gain_apply(bg, s.gain[:k], out=s.g_bg[:k])
        bg = self._background(s, k)
        if self.propagate:
            self._trimaps(s, k, keyed)
        if self.auto:
            ops.trimap_from_plate(s.d_cmp[:k], bg, out=s.d_tri[:k], work=self._auto_work, shadow=self.shadow,
                                  **self.auto_options)
            if self.auto_fill is not None:
                ops.trimap_fill_enclosed(s.d_tri[:k], self.auto_fill, out=s.d_tri[:k], work=self._fill_work)
        self._feed(s, k, bg)

    def _after(self, s, k, keyed=False):
        """... and after it: the matte to full resolution (scale > 1), the temporal filter (smooth="flow"), then
        quantise | compose -> download."""
        self._upsample(s, k)
        self._smooth(s, k, keyed)
        self._download(s, k)

    def _chain(self, s, k, keyed=False):
        """Ingest -> forward -> quantise | compose -> download of the slot's first k frames, on the current stream."""
        self._before(s, k, keyed)
        self.model.forward(s.frames[:k], out=self._matte(s, k), overflow=s.flag)
        self._after(s, k, keyed)

    def _capture(self, s, keyed=False):
        """The full-chunk chain of one slot as one HIP graph: UNet.capture records the forward over the slot's static
        buffers with _before ahead of it and _after behind it, all on the capturing stream; a leading slice of full
        length is the buffer itself, so these are _chain's calls.  ``keyed`` (a chain with state): the graph of an item
        that restarts it, or of one that continues."""
        n = self.chunk
        graph = self.model.capture(s.frames, static=True, out=self._matte(s, n), overflow=s.flag,
                                   pre=lambda: self._before(s, n, keyed), post=lambda: self._after(s, n, keyed))
        if self._stateful:
            s.graphs[keyed] = graph
        else:
            s.graph = graph

    def _submit(self, s, index, cmp, bg, tri, k, nw=None, bw=None):
        s.k, s.index = k, index
        if self.gain is not None:
            self._gain_last = (s, k)
        if self.align is not None:
            self._align_last = (s, k)
        # the item restarts the chain's state: it carries a key, or without trimap="propagate" it is a run's first
        keyed = tri is not None if self.propagate else self.smooth is not None and not self._started
        self._started, self._smooth_k = True, k
        for name, a in (("cmp", cmp), ("bg", bg), ("key" if self.propagate else "tri", tri), ("bw", bw), ("nw", nw)):
            s.stage(name, a, 1 if name == "key" else k)
        with torch.cuda.stream(self._upload):
            s.upload(k)
            s.uploaded.record(self._upload)
        with torch.cuda.stream(self._compute):
            self._compute.wait_event(s.uploaded)
            if self.graph and k == self.chunk:
                if self._stateful:
                    s.graphs[keyed].replay()
                else:
                    if s.graph is None:
                        self._capture(s)
                    s.graph.replay()
            else:
                self._chain(s, k, keyed)
            s.done.record(self._compute)

    def _retire(self, s):
        s.done.synchronize()
        k = s.k
        if s.h_flag is not None and int(s.h_flag[0]):
            # the chunk left fp16's range: the same frames on bf16x6 (f32 range), re-quantised and re-downloaded
            self.overflowed_chunks.append(s.index)
            with torch.cuda.stream(self._compute):
                rerun_x6(self, s.frames[:k], self._matte(s, k))
                s.flag.zero_()
                self._after(s, k)
            self._compute.synchronize()
        return s.h_out[:k].numpy().copy()

    def run(self, source):
        """Generator: one [k,h,w] matte (numpy, the ``out`` dtype), or one composed [k,h,w,3 | 4] uint8 array, per source
        item, in source order."""
        self.overflowed_chunks = []
        self._keyed = self._started = False
        yield from super().run(source)
