"""Streamed inference of the video model on a decoded clip: the recurrence the reference trains (train.py:346-366,
loader.py:285-330),

    alpha[t] = UNetSimple(cmp[t], bg[t], warp_img(alpha[t-1], backward[t]))        with phase False,

optionally with flow.correct_alpha's occlusion mask on the warped matte.  A decoded clip is uint8 BGR composites, uint8
backgrounds (often one static plate) and the .flo flows between neighbouring frames, all in host memory.  ClipStream
moves one frame per step through ``depth`` slots:

    host arrays -> pinned buffers -> (upload stream) device uint8 + flows -> (compute stream) ops.clip_feed ->
    UNetSimple.forward_fed -> ops.matte_quantize | ops.matte_compose -> pinned output -> numpy

The upload of frame t + 1 runs beside the compute of frame t.  The matte never leaves the device between frames: the
feed kernel of frame t reads the model's f32 output buffer, which still holds alpha[t-1], and the forward that follows
it in stream order overwrites that buffer with alpha[t].  A frame's compute chain (zero the flag, feed, forward,
quantise, download) is one HIP graph per slot, captured once over static buffers on one stream.

The flows come from the caller, as in the reference's .flo files, or (``flow="estimate"``) from the frames themselves:
the frame's pyramid and its flows against the previous frame's pyramid (flow_track.FlowTracker) head the frame's chain,
and nothing is staged or uploaded for the flows.  The matte before the first frame comes from the caller (for example
a key frame's matte by UNetVideo).
"""

import numpy as np
import torch

from . import ops
from .flow_track import FlowTracker
from .pipeline import PER_FRAME, Slot, SlotPipeline, check_new_bg, check_out, check_static_bg
from .unet_simple import UNetSimple

PROMOTE = ("numpy1", "numpy2")


class _Slot(Slot):
    """One frame in flight: pinned host inputs, their device copies, the quantised matte, the pinned output, the
    IndexError flag with its pinned copy, the two events and the slot's graphs (by the towers they run)."""

    def __init__(self, cs):
        h, w = cs.h, cs.w
        super().__init__(cs.device, (("cmp", (1, h, w, 3), torch.uint8),
                                     ("bw", None if cs.estimate else (1, h, w, 2), torch.float32),
                                     ("bg", (1, h, w, 3) if cs.static_bg is None else None, torch.uint8),
                                     ("fw", (1, h, w, 2) if cs.occlusion and not cs.estimate else None, torch.float32),
                                     ("nw", (1, h, w, 3) if cs.new_bg is PER_FRAME else None, torch.uint8)),
                         1, h, w, cs.out, flag=cs.occlusion)
        self.graphs = {}


class ClipStream(SlotPipeline):
    """``ClipStream(model, h, w, ...).run(source, alpha0)`` yields one [h,w] numpy matte per item of ``source``, in
    order.

    ``model``: a UNetSimple in bf16 or fp32 (its trained parameters through ``load_params``).  ``source`` yields
    ``(cmp, bg, backward, forward)`` per frame: cmp uint8 [h,w,3] BGR; bg uint8 [h,w,3], None exactly when
    ``static_bg`` (uint8 [h,w,3], uploaded once) was given; backward f32 [h,w,2] in reader.read_flow layout, mapping
    this frame into the previous one; forward f32 [h,w,2], None exactly when ``occlusion=False``.  An item's arrays are
    copied before the next item is asked for, so the source may reuse them.  ``alpha0``: the matte of the frame before
    the first item, f32 [h,w], or uint8 converted as f32(u / 255.0) (reader.py:16).

    ``occlusion``: flow.correct_alpha(backward, forward, warped, promote, thresh) on the warped matte.  Off by default:
    the model is trained on the warp alone (loader.video_load_crop).  Where the reference raises IndexError on a
    frame's flows, run() finishes nothing further, synchronises and raises IndexError naming the frame; the mattes
    already yielded stand.  ``out``: "u8" / "u16" mattes (ops.matte_quantize) or the "f32" alpha.  Results lag the
    source by ``depth - 1`` frames.

    ``out`` "over" / "bgra" / "premul" applies each frame's matte with the known background (ops.matte_compose) and
    yields the uint8 [h,w,3] frame over a new plate, or the [h,w,4] BGRA foreground layer (straight / premultiplied;
    its alpha channel is the "u8" matte).  "over" takes ``new_bg``: a uint8 [h,w,3] plate (uploaded once), or
    "per_frame", and then every source item is ``(cmp, bg, backward, forward, new_bg)`` with new_bg uint8 [h,w,3].
    The compose step only reads the model's output buffer: the recurrence is the one of out="f32".

    ``reuse_bg_tower`` with a static plate: the plate's tower (13 VGG feature maps, the same every frame) runs with the
    first frame only; later frames run the cmp and warped-matte towers.  ``stats["bg_tower_evals"]`` counts the frames
    of the last run that ran the background tower.

    ``flow="estimate"``: the flows are estimated on the device from consecutive frames (ops.estimate_flow's
    arithmetic; ``flow_options``: its levels / warps / iters / alpha) instead of given.  Source items keep their shape
    with both flows None, ``(cmp, bg, None, None[, new_bg])``; h and w are at least 16.  ``run(source, alpha0, cmp0)``
    takes the uint8 [h,w,3] frame ``alpha0`` belongs to; with ``cmp0=None``, alpha0 belongs to the first frame itself
    and that frame's flows are zero.  The mattes are those of ``flow="given"`` fed with ops.estimate_flow(cmp[t],
    cmp[t-1]) (and, with ``occlusion``, ops.estimate_flow(cmp[t-1], cmp[t])), bit for bit.

    If the source raises, or yields a bad item, the frames already taken are finished and yielded, the streams are
    synchronised, and the exception then propagates; the object can run again."""

    def __init__(self, model, h, w, depth=2, static_bg=None, occlusion=False, thresh=15.0, promote="numpy1", out="u8",
                 graph=True, reuse_bg_tower=True, new_bg=None, flow="given", flow_options=None):
        if not isinstance(model, UNetSimple):
            raise TypeError("ClipStream: the video model is a UNetSimple, got %s" % type(model).__name__)
        if model.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError("ClipStream: a bf16 or fp32 UNetSimple, got %s" % (model.dtype,))
        h, w, depth = int(h), int(w), int(depth)
        if h < 1 or w < 1 or depth < 1:
            raise ValueError("ClipStream: h, w and depth must be positive (got %d, %d, %d)" % (h, w, depth))
        check_out("ClipStream", out)
        if promote not in PROMOTE:
            raise ValueError("ClipStream: promote must be one of %s, got %r" % (PROMOTE, promote))
        thresh = float(thresh)
        if not thresh >= 0.0:
            raise ValueError("ClipStream: thresh must be a non-negative number, got %r" % (thresh,))
        flow_options = ops.check_flow_mode("ClipStream", flow, flow_options, h, w)
        self.estimate = flow_options is not None
        if self.estimate:
            self.flow_options = flow_options
        static_bg = check_static_bg("ClipStream", static_bg, h, w)
        self.new_bg = check_new_bg("ClipStream", out, new_bg, h, w)
        self.model, self.h, self.w, self.depth = model, h, w, depth
        self.static_bg, self.occlusion, self.thresh, self.promote = static_bg, bool(occlusion), thresh, promote
        self.out, self.graph = out, bool(graph)
        self.reuse_bg_tower = bool(reuse_bg_tower) and static_bg is not None
        self.device = model.device
        self.stats = {"bg_tower_evals": 0, "frames": 0}
        self._buf = None
        self._cmp0 = self._bw = self._fw = None

    # ------------------------------------------------------------------ checks (host only)
    def check_item(self, item):
        """Validate one source item; returns (cmp, bg, backward, forward), and new_bg after them with
        new_bg="per_frame"."""
        per_frame = self.new_bg is PER_FRAME
        if not isinstance(item, (tuple, list)) or len(item) != 4 + per_frame:
            raise ValueError("ClipStream: the source yields (cmp, bg, backward, forward%s) per frame" %
                             (", new_bg" if per_frame else ""))
        cmp, bg, bw, fw = item[:4]
        if self.estimate and (bw is not None or fw is not None):
            raise ValueError("ClipStream: flow='estimate' takes (cmp, bg, None, None%s): both flows are estimated" %
                             (", new_bg" if per_frame else ""))
        if (bg is None) != (self.static_bg is not None):
            raise ValueError("ClipStream: bg is None exactly when a static_bg was given")
        if (fw is None) == self.occlusion and not self.estimate:
            raise ValueError("ClipStream: forward is None exactly when occlusion=False")
        arrays = [("cmp", cmp, torch.uint8, "h,w,3"), ("bg", bg, torch.uint8, "h,w,3"),
                  ("backward", bw, torch.float32, "h,w,2"), ("forward", fw, torch.float32, "h,w,2")]
        if per_frame:
            arrays.append(("new_bg", item[4], torch.uint8, "h,w,3"))
        for name, a, dt, shape in arrays:
            if a is None and (name in ("bg", "forward") or self.estimate and name == "backward"):
                continue
            ops.check_array("ClipStream", name, a, (dt,), shape, h=self.h, w=self.w)
        return (cmp, bg, bw, fw, item[4]) if per_frame else (cmp, bg, bw, fw)

    def check_alpha0(self, alpha0):
        """The matte before the first frame as f32 [h,w]: f32 as it is, uint8 as f32(u / 255.0) (reader.py:16)."""
        ops.check_array("ClipStream", "alpha0", alpha0, (torch.float32, torch.uint8), "h,w", h=self.h, w=self.w)
        if alpha0.dtype == np.uint8:
            return (alpha0.astype(np.float64) / 255.0).astype(np.float32)
        return np.ascontiguousarray(alpha0)

    # ------------------------------------------------------------------ device side
    def _towers_of(self, index):
        return (0, 2) if self.reuse_bg_tower and index > 0 else (0, 1, 2)

    def _setup(self):
        """Streams, slots and (graph=True) every slot's graphs.  The graphs are captured here, before alpha0 is in
        place: a capture runs its chain once to warm up, which overwrites the model's output buffer."""
        dev = self.device
        self._make_streams()
        self._buf = self.model._buffers(1, self.h, self.w)
        self._views = self.model.feed_views(1, self.h, self.w)
        self._alpha = self._buf["out"]
        self._upload_plates()
        if self.estimate:
            # one set of flow buffers for every slot (the chains run one after another on the compute stream), and
            # the tracker's pyramids at fixed addresses: every slot's graph reads the previous frame's and leaves its own
            f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
            self._bw, self._fw = f32(1, self.h, self.w, 2), f32(1, self.h, self.w, 2) if self.occlusion else None
            self._flow = FlowTracker(self.h, self.w, self.flow_options, dev)
            self._d_cmp0 = torch.zeros((self.h, self.w, 3), dtype=torch.uint8, device=dev)
        self._slots = [_Slot(self) for _ in range(self.depth)]
        torch.cuda.synchronize(dev)  # the plate and the zeroed buffers, before another stream touches them
        if self.graph:
            with torch.cuda.stream(self._compute):
                for i, s in enumerate(self._slots):
                    for towers in sorted({self._towers_of(j) for j in range(i, i + 2 * self.depth, self.depth)}):
                        s.graphs[towers] = self.model.capture_fed(
                            1, self.h, self.w, towers, pre=lambda s=s: self._feed(s),
                            post=lambda s=s: self._download(s))
            torch.cuda.synchronize(dev)

    def _needs_setup(self):  # (again when the model ran another shape since: its buffers were replaced)
        return self._slots is None or self.model._buffers(1, self.h, self.w) is not self._buf

    def _begin(self):  # what the caller queued comes first; then the matte before the first frame
        super()._begin()
        with torch.cuda.stream(self._compute):
            self._alpha.copy_(torch.from_numpy(self._alpha0).view(1, self.h, self.w, 1))
            if self._cmp0 is not None:  # the previous frame of the first one
                self._d_cmp0.copy_(torch.from_numpy(self._cmp0))
                self._flow.seed(self._d_cmp0)

    def _download(self, s):
        """The slot's result from the model's output buffer (and, composed, the slot's uint8 inputs), which it only
        reads."""
        s.download(self._alpha, s.d_cmp, *self._plates(s, 1))

    def _feed(self, s):
        if s.flag is not None:
            s.flag.zero_()
        towers, cat = self._views
        if self.estimate:  # this frame's flows against the previous frame, and its pyramid left for the next chain
            self._flow.advance(s.d_cmp, self._bw, self._fw)
        bw, fw = (self._bw, self._fw) if self.estimate else (s.d_bw, s.d_fw)
        ops.clip_feed(s.d_cmp, self._plates(s, 1)[0], self._alpha, bw, fw, self.thresh, self.promote, towers=towers,
                      cat=cat, err=s.flag)

    def _submit(self, s, index, cmp, bg, bw, fw, nw=None):
        s.index = index
        for name, a in (("cmp", cmp), ("bw", bw), ("bg", bg), ("fw", fw), ("nw", nw)):
            s.stage(name, a, 1)
        with torch.cuda.stream(self._upload):
            s.upload(1)
            s.uploaded.record(self._upload)
        towers = self._towers_of(index)
        self.stats["frames"] += 1
        self.stats["bg_tower_evals"] += 1 in towers
        with torch.cuda.stream(self._compute):
            self._compute.wait_event(s.uploaded)
            if self.estimate and index == 0 and self._cmp0 is None:  # alpha0 belongs to this frame: zero flows
                self._flow.seed(s.d_cmp[0])
            if self.graph:
                s.graphs[towers].replay()
            else:
                self._feed(s)
                self.model.forward_fed(1, self.h, self.w, towers)
                self._download(s)
            s.done.record(self._compute)

    def _retire(self, s):
        s.done.synchronize()
        if s.h_flag is not None and int(s.h_flag[0]):
            raise IndexError("ClipStream: frame %d: a backward-flow target lies more than one frame outside the image "
                             "(the reference's numpy IndexError, flow.py:46)" % s.index)
        return s.h_out[0].numpy().copy()

    def run(self, source, alpha0, cmp0=None):
        """Generator: one [h,w] matte (numpy, the ``out`` dtype), or one composed [h,w,3 | 4] uint8 array, per source
        item, in source order.  ``cmp0`` (flow="estimate" only): the uint8 [h,w,3] frame ``alpha0`` belongs to."""
        if cmp0 is not None and not self.estimate:
            raise ValueError("ClipStream: cmp0 goes with flow='estimate'")
        self._alpha0 = self.check_alpha0(alpha0)
        cmp0 = check_static_bg("ClipStream", cmp0, self.h, self.w, name="cmp0")
        self._cmp0 = None if cmp0 is None else cmp0.copy()
        self.stats = {"bg_tower_evals": 0, "frames": 0}
        yield from super().run(source)
