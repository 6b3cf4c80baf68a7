"""Streamed inference of the video model on a decoded clip: the recurrence the reference trains (train.py:346-366,
loader.py:285-330),

    alpha[t] = UNetSimple(cmp[t], bg[t], warp_img(alpha[t-1], backward[t]))        with phase False,

optionally with flow.correct_alpha's occlusion mask on the warped matte.  A decoded clip is uint8 BGR composites, uint8
backgrounds (often one static plate) and the .flo flows between neighbouring frames, all in host memory.  ClipStream
moves one frame per step through ``depth`` slots:

    host arrays -> pinned buffers -> (upload stream) device uint8 + flows -> (compute stream) ops.clip_feed ->
    UNetSimple.forward_fed -> ops.matte_quantize -> pinned output -> numpy

The upload of frame t + 1 runs beside the compute of frame t.  The matte never leaves the device between frames: the
feed kernel of frame t reads the model's f32 output buffer, which still holds alpha[t-1], and the forward that follows
it in stream order overwrites that buffer with alpha[t].  A frame's compute chain (zero the flag, feed, forward,
quantise, download) is one HIP graph per slot, captured once over static buffers on one stream.

The flows come from the caller, as in the reference's .flo files; so does the matte before the first frame (for
example a key frame's matte by UNetVideo).
"""

import numpy as np
import torch

from . import ops
from .stream import OUT_DTYPES
from .unet_simple import UNetSimple

PROMOTE = ("numpy1", "numpy2")


class _Slot:
    """One frame in flight: pinned host inputs, their device copies, the quantised matte, the pinned output, the
    IndexError flag with its pinned copy, the two events and the slot's graphs (by the towers they run)."""

    def __init__(self, cs):
        dev, h, w = cs.device, cs.h, cs.w
        pin = lambda shape, dt: torch.zeros(shape, dtype=dt).pin_memory()  # noqa: E731
        gpu = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self.h_cmp, self.d_cmp = pin((1, h, w, 3), torch.uint8), gpu((1, h, w, 3), torch.uint8)
        self.h_bg = self.d_bg = self.h_fw = self.d_fw = None
        if cs.static_bg is None:
            self.h_bg, self.d_bg = pin((1, h, w, 3), torch.uint8), gpu((1, h, w, 3), torch.uint8)
        self.h_bw, self.d_bw = pin((1, h, w, 2), torch.float32), gpu((1, h, w, 2), torch.float32)
        if cs.occlusion:
            self.h_fw, self.d_fw = pin((1, h, w, 2), torch.float32), gpu((1, h, w, 2), torch.float32)
        _, t_dt, _ = OUT_DTYPES[cs.out]
        self.q = None if t_dt is None else gpu((1, h, w), t_dt)
        self.h_out = pin((1, h, w), t_dt or torch.float32)
        self.flag = gpu((1,), torch.int32)
        self.h_flag = pin((1,), torch.int32)
        self.uploaded, self.done = torch.cuda.Event(), torch.cuda.Event()
        self.graphs = {}
        self.index = 0  # the frame in flight


class ClipStream:
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

    ``reuse_bg_tower`` with a static plate: the plate's tower (13 VGG feature maps, the same every frame) runs with the
    first frame only; later frames run the cmp and warped-matte towers.  ``stats["bg_tower_evals"]`` counts the frames
    of the last run that ran the background tower.

    If the source raises, or yields a bad item, the frames already taken are finished and yielded, the streams are
    synchronised, and the exception then propagates; the object can run again."""

    def __init__(self, model, h, w, depth=2, static_bg=None, occlusion=False, thresh=15.0, promote="numpy1", out="u8",
                 graph=True, reuse_bg_tower=True):
        if not isinstance(model, UNetSimple):
            raise TypeError("ClipStream: the video model is a UNetSimple, got %s" % type(model).__name__)
        if model.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError("ClipStream: a bf16 or fp32 UNetSimple, got %s" % (model.dtype,))
        h, w, depth = int(h), int(w), int(depth)
        if h < 1 or w < 1 or depth < 1:
            raise ValueError("ClipStream: h, w and depth must be positive (got %d, %d, %d)" % (h, w, depth))
        if out not in OUT_DTYPES:
            raise ValueError("ClipStream: out must be one of %s, got %r" % (sorted(OUT_DTYPES), out))
        if promote not in PROMOTE:
            raise ValueError("ClipStream: promote must be one of %s, got %r" % (PROMOTE, promote))
        thresh = float(thresh)
        if not thresh >= 0.0:
            raise ValueError("ClipStream: thresh must be a non-negative number, got %r" % (thresh,))
        if static_bg is not None:
            static_bg = np.asarray(static_bg)
            if static_bg.dtype != np.uint8:
                raise TypeError("ClipStream: static_bg must be uint8, got %s" % static_bg.dtype)
            if static_bg.shape != (h, w, 3):
                raise ValueError("ClipStream: static_bg must be [h,w,3] = %s, got %s" % ((h, w, 3), static_bg.shape))
            static_bg = np.ascontiguousarray(static_bg)
        self.model, self.h, self.w, self.depth = model, h, w, depth
        self.static_bg, self.occlusion, self.thresh, self.promote = static_bg, bool(occlusion), thresh, promote
        self.out, self.graph = out, bool(graph)
        self.reuse_bg_tower = bool(reuse_bg_tower) and static_bg is not None
        self.device = model.device
        self.stats = {"bg_tower_evals": 0, "frames": 0}
        self._slots = None   # built with the first valid item: nothing touches the device before that
        self._plate = self._buf = None
        self._upload = self._compute = None

    # ------------------------------------------------------------------ checks (host only)
    def check_item(self, item):
        """Validate one source item; returns (cmp, bg, backward, forward)."""
        if not isinstance(item, (tuple, list)) or len(item) != 4:
            raise ValueError("ClipStream: the source yields (cmp, bg, backward, forward) per frame")
        cmp, bg, bw, fw = item
        if (bg is None) != (self.static_bg is not None):
            raise ValueError("ClipStream: bg is None exactly when a static_bg was given")
        if (fw is None) == self.occlusion:
            raise ValueError("ClipStream: forward is None exactly when occlusion=False")
        for name, a, dt, c in (("cmp", cmp, np.uint8, 3), ("bg", bg, np.uint8, 3), ("backward", bw, np.float32, 2),
                               ("forward", fw, np.float32, 2)):
            if a is None and name in ("bg", "forward"):
                continue
            if not isinstance(a, np.ndarray):
                raise TypeError("ClipStream: %s must be a numpy array, got %s" % (name, type(a).__name__))
            if a.dtype != dt:
                raise TypeError("ClipStream: %s must be %s, got %s" % (name, np.dtype(dt).name, a.dtype))
            if a.shape != (self.h, self.w, c):
                raise ValueError("ClipStream: %s must be [h,w,%d] = %s, got %s" % (name, c, (self.h, self.w, c), a.shape))
        return cmp, bg, bw, fw

    def check_alpha0(self, alpha0):
        """The matte before the first frame as f32 [h,w]: f32 as it is, uint8 as f32(u / 255.0) (reader.py:16)."""
        if not isinstance(alpha0, np.ndarray):
            raise TypeError("ClipStream: alpha0 must be a numpy array, got %s" % type(alpha0).__name__)
        if alpha0.dtype not in (np.dtype(np.float32), np.dtype(np.uint8)):
            raise TypeError("ClipStream: alpha0 must be float32 or uint8, got %s" % alpha0.dtype)
        if alpha0.shape != (self.h, self.w):
            raise ValueError("ClipStream: alpha0 must be [h,w] = %s, got %s" % ((self.h, self.w), alpha0.shape))
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
        self._upload, self._compute = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        self._buf = self.model._buffers(1, self.h, self.w)
        self._views = self.model.feed_views(1, self.h, self.w)
        self._alpha = self._buf["out"]
        if self.static_bg is not None:
            self._plate = torch.from_numpy(self.static_bg).to(dev)
        self._slots = [_Slot(self) for _ in range(self.depth)]
        torch.cuda.synchronize(dev)  # the plate and the zeroed buffers, before another stream touches them
        if self.graph:
            with torch.cuda.stream(self._compute):
                for i, s in enumerate(self._slots):
                    for towers in sorted({self._towers_of(j) for j in range(i, i + 2 * self.depth, self.depth)}):
                        s.graphs[towers] = self.model.capture_fed(
                            1, self.h, self.w, towers, pre=lambda s=s: self._feed(s), post=lambda s=s: self._finish(s))
            torch.cuda.synchronize(dev)

    def _feed(self, s):
        if self.occlusion:
            s.flag.zero_()
        towers, cat = self._views
        ops.clip_feed(s.d_cmp, self._plate if self._plate is not None else s.d_bg, self._alpha, s.d_bw, s.d_fw,
                      self.thresh, self.promote, towers=towers, cat=cat, err=s.flag)

    def _finish(self, s):
        if s.q is None:
            s.h_out.copy_(self._alpha[:, :, :, 0], non_blocking=True)
        else:
            ops.matte_quantize(self._alpha, out=s.q, bits=OUT_DTYPES[self.out][2])
            s.h_out.copy_(s.q, non_blocking=True)
        if self.occlusion:
            s.h_flag.copy_(s.flag, non_blocking=True)

    def _submit(self, s, index, cmp, bg, bw, fw):
        s.index = index
        s.h_cmp[0].numpy()[...] = cmp
        s.h_bw[0].numpy()[...] = bw
        if bg is not None:
            s.h_bg[0].numpy()[...] = bg
        if fw is not None:
            s.h_fw[0].numpy()[...] = fw
        with torch.cuda.stream(self._upload):
            s.d_cmp.copy_(s.h_cmp, non_blocking=True)
            s.d_bw.copy_(s.h_bw, non_blocking=True)
            if bg is not None:
                s.d_bg.copy_(s.h_bg, non_blocking=True)
            if fw is not None:
                s.d_fw.copy_(s.h_fw, non_blocking=True)
            s.uploaded.record(self._upload)
        towers = self._towers_of(index)
        self.stats["frames"] += 1
        self.stats["bg_tower_evals"] += 1 in towers
        with torch.cuda.stream(self._compute):
            self._compute.wait_event(s.uploaded)
            if self.graph:
                s.graphs[towers].replay()
            else:
                self._feed(s)
                self.model.forward_fed(1, self.h, self.w, towers)
                self._finish(s)
            s.done.record(self._compute)

    def _retire(self, s):
        s.done.synchronize()
        if self.occlusion and int(s.h_flag[0]):
            raise IndexError("ClipStream: frame %d: a backward-flow target lies more than one frame outside the image "
                             "(the reference's numpy IndexError, flow.py:46)" % s.index)
        return s.h_out[0].numpy().copy()

    def run(self, source, alpha0):
        """Generator: one [h,w] matte (numpy, the ``out`` dtype) per source item, in source order."""
        alpha0 = self.check_alpha0(alpha0)
        self.stats = {"bg_tower_evals": 0, "frames": 0}
        inflight, error, index = [], None, 0
        it = iter(source)
        try:
            while True:
                try:
                    item = next(it)
                    cmp, bg, bw, fw = self.check_item(item)
                except StopIteration:
                    break
                except Exception as e:  # the source failed or yielded a bad item: finish what was taken, then raise
                    error = e
                    break
                if self._slots is None or self.model._buffers(1, self.h, self.w) is not self._buf:
                    self._setup()  # (again when the model ran another shape since: its buffers were replaced)
                if index == 0:  # what the caller queued comes first; then the matte before the first frame
                    self._compute.wait_stream(torch.cuda.current_stream(self.device))
                    with torch.cuda.stream(self._compute):
                        self._alpha.copy_(torch.from_numpy(alpha0).view(1, self.h, self.w, 1))
                s = self._slots[index % self.depth]
                self._submit(s, index, cmp, bg, bw, fw)
                index += 1
                inflight.append(s)
                if len(inflight) >= self.depth:
                    yield self._retire(inflight.pop(0))
            while inflight:
                yield self._retire(inflight.pop(0))
        finally:
            # also when the consumer abandons the generator or a frame raised IndexError: nothing stays queued
            if self._slots is not None:
                self._upload.synchronize()
                self._compute.synchronize()
        if error is not None:
            raise error
