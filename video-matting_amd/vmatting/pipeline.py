"""The slot pipeline the streamed paths share (stream.FrameStream, clip.ClipStream): items of a host source move
through ``depth`` slots, the upload of item i + 1 on one stream beside the compute of item i on another, and results
come back in order, ``depth - 1`` items behind the source.

SlotPipeline owns the generator; a streamed path supplies the hooks.  Slot holds what one item in flight needs: pinned
host / device buffer pairs, the quantised output and its pinned copy, an optional int32 flag pair and two events.
"""

import numpy as np
import torch

from . import ops

OUT_DTYPES = {"u8": (np.uint8, torch.uint8, 8), "u16": (np.uint16, torch.uint16, 16), "f32": (np.float32, None, 0),
              # the matte applied (ops.matte_compose): the frame over a new plate, the straight / premultiplied layer
              "over": (np.uint8, torch.uint8, 8), "bgra": (np.uint8, torch.uint8, 8), "premul": (np.uint8, torch.uint8, 8)}
COMPOSE_CHANNELS = {"over": 3, "bgra": 4, "premul": 4}  # out -> channels of the composed result
PER_FRAME = "per_frame"


def check_out(who, out):
    if out not in OUT_DTYPES:
        raise ValueError("%s: out must be one of %s, got %r" % (who, sorted(OUT_DTYPES), out))
    return out


def check_static_bg(who, static_bg, h, w, name="static_bg"):
    """``static_bg`` as a contiguous uint8 [h,w,3] array (None stays None)."""
    if static_bg is None:
        return None
    static_bg = np.asarray(static_bg)
    ops.check_array(who, name, static_bg, (torch.uint8,), "h,w,3", h=h, w=w)
    return np.ascontiguousarray(static_bg)


def check_new_bg(who, out, new_bg, h, w):
    """The new plate of out="over": the string "per_frame" (every source item carries its plates) or a contiguous
    uint8 [h,w,3] array; None for every other ``out``, which takes none."""
    if out != "over":
        if new_bg is not None:
            raise ValueError("%s: new_bg goes with out='over', not out=%r" % (who, out))
        return None
    if new_bg is None:
        raise ValueError("%s: out='over' needs new_bg: a uint8 [h,w,3] plate or %r" % (who, PER_FRAME))
    if isinstance(new_bg, str):
        if new_bg != PER_FRAME:
            raise ValueError("%s: new_bg must be a uint8 [h,w,3] plate or %r, got %r" % (who, PER_FRAME, new_bg))
        return PER_FRAME
    return check_static_bg(who, new_bg, h, w, name="new_bg")


class Slot:
    """One item in flight.  ``pairs``: (name, shape | None, dtype) per input; each gives a pinned ``h_<name>`` and its
    device copy ``d_<name>`` (both None for a None shape: an input this configuration does not take).  ``q`` [n,h,w]
    is the quantised matte (None for out="f32"), or [n,h,w,C] the composed result (out "over": C = 3, "bgra" /
    "premul": C = 4), and ``h_out`` its pinned copy; ``flag`` / ``h_flag`` an int32 [1] pair (None without ``flag``);
    ``uploaded`` / ``done`` the events of the item's upload and of its compute chain."""

    def __init__(self, device, pairs, n, h, w, out, flag):
        pin = lambda shape, dt: torch.zeros(shape, dtype=dt).pin_memory()  # noqa: E731
        gpu = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)  # noqa: E731
        self._names = [name for name, shape, _ in pairs if shape is not None]
        for name, shape, dt in pairs:
            setattr(self, "h_" + name, None if shape is None else pin(shape, dt))
            setattr(self, "d_" + name, None if shape is None else gpu(shape, dt))
        _, t_dt, self._bits = OUT_DTYPES[out]
        self._mode = out if out in COMPOSE_CHANNELS else None
        shape = (n, h, w) + ((COMPOSE_CHANNELS[out],) if self._mode else ())
        self.q = None if t_dt is None else gpu(shape, t_dt)
        self.h_out = pin(shape, t_dt or torch.float32)
        self.flag = gpu((1,), torch.int32) if flag else None
        self.h_flag = pin((1,), torch.int32) if flag else None
        self.uploaded, self.done = torch.cuda.Event(), torch.cuda.Event()
        self.index = 0  # the item in flight: its position in the source

    def stage(self, name, array, k):
        """Copy a host array into the first k frames of the pinned buffer (None: an input not taken)."""
        if array is not None:
            getattr(self, "h_" + name)[:k].numpy()[...] = array

    def upload(self, k):
        """Queue the first k frames of every pinned input to its device copy, on the current stream."""
        for name in self._names:
            getattr(self, "d_" + name)[:k].copy_(getattr(self, "h_" + name)[:k], non_blocking=True)

    def download(self, alpha, cmp=None, bg=None, new_bg=None):
        """Quantise ``alpha`` ([k,h,w,1] f32), or compose it with ``cmp``, ``bg`` (and ``new_bg``) in the out modes of
        ops.matte_compose, and queue the result, and the flag, to the pinned outputs, on the current stream."""
        k = alpha.shape[0]
        if self.q is None:
            self.h_out[:k].copy_(alpha[:, :, :, 0], non_blocking=True)
        elif self._mode:
            ops.matte_compose(alpha, cmp, bg, new_bg, mode=self._mode, out=self.q[:k])
            self.h_out[:k].copy_(self.q[:k], non_blocking=True)
        else:
            ops.matte_quantize(alpha, out=self.q[:k], bits=self._bits)
            self.h_out[:k].copy_(self.q[:k], non_blocking=True)
        if self.flag is not None:
            self.h_flag.copy_(self.flag, non_blocking=True)


class SlotPipeline:
    """``run(source)`` over the hooks of a streamed path:

    check_item(item) -> args   host-only validation of one source item, before any device work for it
    _needs_setup()             True until _setup() has built ``_slots`` (a list of ``depth`` slots)
    _setup()                   streams (_make_streams), plates (_upload_plates), slots and whatever else the first
                               valid item needs
    _begin()                   before the first item of a run is submitted; here: the compute stream waits on what
                               the caller queued
    _submit(slot, index, *args) stage, upload and queue the compute chain of one item
    _retire(slot) -> result    wait for the slot's chain; the host result
    _drain()                   nothing stays queued on the slots: both streams synchronised
    """

    device = None
    depth = 1
    _slots = None   # built with the first valid item: nothing touches the device before that
    _upload = _compute = None
    static_bg = new_bg = None      # check_static_bg's and check_new_bg's results
    _plate = _new_plate = None     # ... and the plates among them on the device, once _setup() has run

    def check_item(self, item):
        raise NotImplementedError

    def _needs_setup(self):
        return self._slots is None

    def _make_streams(self):
        self._upload, self._compute = torch.cuda.Stream(device=self.device), torch.cuda.Stream(device=self.device)

    def _upload_plates(self):
        """The static background and a new plate, where the stream was given them, to the device."""
        if self.static_bg is not None:
            self._plate = torch.from_numpy(self.static_bg).to(self.device)
        if isinstance(self.new_bg, np.ndarray):
            self._new_plate = torch.from_numpy(self.new_bg).to(self.device)

    def _plates(self, s, k):
        """(background, new background | None) of the slot's first k frames: the plate, or the slot's per-frame
        copies."""
        return (self._plate if self._plate is not None else s.d_bg[:k],
                self._new_plate if self._new_plate is not None else None if s.d_nw is None else s.d_nw[:k])

    def _begin(self):
        self._compute.wait_stream(torch.cuda.current_stream(self.device))

    def _drain(self):
        self._upload.synchronize()
        self._compute.synchronize()

    def run(self, source):
        """Generator: one result per source item, in source order, ``depth - 1`` items behind the source.  If the
        source raises or yields a bad item, what was taken is finished and yielded, then the exception propagates."""
        inflight, error, index = [], None, 0
        it = iter(source)
        try:
            while True:
                try:
                    args = self.check_item(next(it))
                except StopIteration:
                    break
                except Exception as e:  # the source failed or yielded a bad item: finish what was taken, then raise
                    error = e
                    break
                if self._needs_setup():
                    self._setup()
                if index == 0:
                    self._begin()
                s = self._slots[index % self.depth]
                self._submit(s, index, *args)
                index += 1
                inflight.append(s)
                if len(inflight) >= self.depth:
                    yield self._retire(inflight.pop(0))
            while inflight:
                yield self._retire(inflight.pop(0))
        finally:
            # also when the consumer abandons the generator or _retire raises: nothing stays queued on the slots
            if self._slots is not None:
                self._drain()
        if error is not None:
            raise error
