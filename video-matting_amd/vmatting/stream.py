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

This is one process's share of a clip; sharding a clip across ranks stays video.shard's job.
"""

import numpy as np
import torch

from . import ops
from .pipeline import OUT_DTYPES  # noqa: F401  (public)
from .pipeline import PER_FRAME, Slot, SlotPipeline, check_new_bg, check_out, check_static_bg
from .split6 import rerun_x6


class _Slot(Slot):
    """One chunk in flight: pinned host inputs, their device copies, the frame buffer in the model's input format,
    the f32 alpha, the quantised matte, the pinned output and the two events."""

    def __init__(self, fs):
        n, h, w = fs.chunk, fs.h, fs.w
        u8 = torch.uint8
        super().__init__(fs.device, (("cmp", (n, h, w, 3), u8),
                                     ("bg", (n, h, w, 3) if fs.static_bg is None else None, u8),
                                     ("tri", (n, h, w) if fs.trimap else None, u8),
                                     ("nw", (n, h, w, 3) if fs.new_bg is PER_FRAME else None, u8)),
                         n, h, w, fs.out, flag=fs.model.split_mode == "f16x3")  # f16x3: this slot's range flag
        self.frames = ops.frame_buffer(fs.model, n, h, w)
        self.alpha = torch.empty((n, h, w, 1), dtype=torch.float32, device=fs.device)
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

    If the source raises, or yields a wrong shape, dtype or k, the chunks already taken are finished and yielded, the
    streams are synchronised, and the exception then propagates; the object can run again."""

    def __init__(self, model, h, w, chunk=8, depth=2, trimap=True, static_bg=None, out="u8", graph=True, new_bg=None):
        h, w, chunk, depth = int(h), int(w), int(chunk), int(depth)
        if h < 1 or w < 1 or chunk < 1 or depth < 1:
            raise ValueError("FrameStream: h, w, chunk and depth must be positive (got %d, %d, %d, %d)" %
                             (h, w, chunk, depth))
        check_out("FrameStream", out)
        if (7 if trimap else 6) != model.IN_CH:
            raise ValueError("FrameStream: %s takes %d channels, so trimap must be %s" %
                             (type(model).__name__, model.IN_CH, model.IN_CH == 7))
        static_bg = check_static_bg("FrameStream", static_bg, h, w)
        self.new_bg = check_new_bg("FrameStream", out, new_bg, h, w)
        self.model, self.h, self.w, self.chunk, self.depth = model, h, w, chunk, depth
        self.trimap, self.static_bg, self.out, self.graph = bool(trimap), static_bg, out, bool(graph)
        self.device = model.device
        self.overflowed_chunks = []
        self._plate = self._new_plate = None
        self._x6 = None

    # ------------------------------------------------------------------ checks (host only)
    def check_item(self, item):
        """Validate one source item; returns (cmp, bg, trimap, k), and new_bg after them with new_bg="per_frame"."""
        per_frame = self.new_bg is PER_FRAME
        if not isinstance(item, (tuple, list)) or len(item) != 3 + per_frame:
            raise ValueError("FrameStream: the source yields (cmp, bg, trimap%s)" %
                             (", new_bg) with new_bg='per_frame'" if per_frame else ") triples"))
        cmp, bg, tri = item[:3]
        if not isinstance(cmp, np.ndarray):
            raise TypeError("FrameStream: cmp must be a numpy array, got %s" % type(cmp).__name__)
        if (bg is None) != (self.static_bg is not None):
            raise ValueError("FrameStream: bg is None exactly when a static_bg was given")
        if (tri is None) == self.trimap:
            raise ValueError("FrameStream: trimap is None exactly when trimap=False")
        for name, a in (("bg", bg), ("trimap", tri)):
            if a is not None and not isinstance(a, np.ndarray):
                raise TypeError("FrameStream: %s must be a numpy array, got %s" % (name, type(a).__name__))
        k, _, _, nb = ops._check_u8_frames(cmp, self.static_bg if bg is None else bg, tri)
        if tuple(cmp.shape[1:3]) != (self.h, self.w):
            raise ValueError("FrameStream: frames must be %d x %d, got %s" % (self.h, self.w, tuple(cmp.shape)))
        if bg is not None and nb != k:
            raise ValueError("FrameStream: bg must be [k,h,w,3] like cmp, got %s" % (tuple(bg.shape),))
        if k > self.chunk:
            raise ValueError("FrameStream: an item of %d frames exceeds chunk=%d" % (k, self.chunk))
        if per_frame:
            nw = item[3]
            if not isinstance(nw, np.ndarray):
                raise TypeError("FrameStream: new_bg must be a numpy array, got %s" % type(nw).__name__)
            if nw.dtype != np.uint8:
                raise TypeError("FrameStream: new_bg must be uint8, got %s" % nw.dtype)
            if nw.shape != cmp.shape:
                raise ValueError("FrameStream: new_bg must be [k,h,w,3] like cmp, got %s" % (tuple(nw.shape),))
            return cmp, bg, tri, k, nw
        return cmp, bg, tri, k

    # ------------------------------------------------------------------ device side
    def _setup(self):
        self.model.prepare()
        self._make_streams()
        if self.static_bg is not None:
            self._plate = torch.from_numpy(self.static_bg).to(self.device)
        if isinstance(self.new_bg, np.ndarray):
            self._new_plate = torch.from_numpy(self.new_bg).to(self.device)
        self._slots = [_Slot(self) for _ in range(self.depth)]
        torch.cuda.synchronize(self.device)  # the plates and the zeroed pad channels, before another stream reads them

    def _download(self, s, k):
        """The result of the slot's first k frames from its alpha (and, composed, its uint8 inputs)."""
        bg = self._plate if self._plate is not None else s.d_bg[:k]
        nw = self._new_plate if self._new_plate is not None else None if s.d_nw is None else s.d_nw[:k]
        s.download(s.alpha[:k], s.d_cmp[:k], bg, nw)

    def _chain(self, s, k):
        """Ingest -> forward -> quantise | compose -> download of the slot's first k frames, on the current stream."""
        bg = self._plate if self._plate is not None else s.d_bg[:k]
        ops.frames_from_u8(s.d_cmp[:k], bg, None if s.d_tri is None else s.d_tri[:k], out=s.frames[:k])
        self.model.forward(s.frames[:k], out=s.alpha[:k], overflow=s.flag)
        self._download(s, k)

    def _capture(self, s):
        """The full-chunk chain of one slot as one HIP graph: UNet.capture records the forward over the slot's static
        buffers with the ingest before it and the quantisation and download after it, all on the capturing stream."""
        bg = self._plate if self._plate is not None else s.d_bg
        s.graph = self.model.capture(
            s.frames, static=True, out=s.alpha, overflow=s.flag,
            pre=lambda: ops.frames_from_u8(s.d_cmp, bg, s.d_tri, out=s.frames),
            post=lambda: self._download(s, self.chunk))

    def _submit(self, s, index, cmp, bg, tri, k, nw=None):
        s.k, s.index = k, index
        for name, a in (("cmp", cmp), ("bg", bg), ("tri", tri), ("nw", nw)):
            s.stage(name, a, k)
        with torch.cuda.stream(self._upload):
            s.upload(k)
            s.uploaded.record(self._upload)
        with torch.cuda.stream(self._compute):
            self._compute.wait_event(s.uploaded)
            if self.graph and k == self.chunk:
                if s.graph is None:
                    self._capture(s)
                s.graph.replay()
            else:
                self._chain(s, k)
            s.done.record(self._compute)

    def _retire(self, s):
        s.done.synchronize()
        k = s.k
        if s.h_flag is not None and int(s.h_flag[0]):
            # the chunk left fp16's range: the same frames on bf16x6 (f32 range), re-quantised and re-downloaded
            self.overflowed_chunks.append(s.index)
            with torch.cuda.stream(self._compute):
                rerun_x6(self, s.frames[:k], s.alpha[:k])
                s.flag.zero_()
                self._download(s, k)
            self._compute.synchronize()
        return s.h_out[:k].numpy().copy()

    def run(self, source):
        """Generator: one [k,h,w] matte (numpy, the ``out`` dtype), or one composed [k,h,w,3 | 4] uint8 array, per source
        item, in source order."""
        self.overflowed_chunks = []
        yield from super().run(source)
