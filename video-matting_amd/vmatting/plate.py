"""The background plate from the clip itself: which frames to sample (SampleSchedule, pure host code) and the
estimator that keeps them on the device and takes their per-pixel temporal median (PlateEstimator over
ops.plate_from_samples; the definition: include/vmatting.h).

The plate has to exist before the first forward, so a clip without a clean plate takes two passes:

    est = PlateEstimator(1080, 1920)
    for chunk in chunks(): est.add(chunk)                       # pass 1
    plate, spread = est.result()
    stream = FrameStream(model, 1080, 1920, chunk=8, static_bg=plate.cpu().numpy(), trimap="auto")

It needs a locked-off camera.  A pixel that the subject covers in more than half the samples gets the subject's colour;
``spread`` is large there.  Nothing compensates exposure changes or flicker."""

import numpy as np

from .ops import check_int

CAPACITY_MAX = 64  # ops.PLATE_MAX_SAMPLES, VM_PLATE_MAX_SAMPLES


class SampleSchedule:
    """Which frames of a clip of unknown length to keep in ``capacity`` slots so that they cover it evenly.

    Frame t is taken when t % stride == 0, stride starting at ``every``.  When a taken frame finds every slot full, the
    schedule first compacts: slot 2 j moves to slot j for j = 1 .. capacity / 2 - 1, in that order (each source lies
    above every earlier destination, so the moves are safe as sequential copies), the stride doubles and capacity / 2
    slots stay in use; the frame, whose index is a multiple of the new stride, then goes to the next slot.  The slots
    thus always hold the multiples of the current stride seen so far, in order: a deterministic function of
    (capacity, every, frames seen), between capacity / 2 and capacity of them once the clip is that long."""

    def __init__(self, capacity=64, every=1):
        self.capacity = check_int("SampleSchedule", "capacity", capacity, 2, CAPACITY_MAX)
        if self.capacity % 2:
            raise ValueError("SampleSchedule: capacity must be even, got %d" % capacity)
        self.every = check_int("SampleSchedule", "every", every, 1)
        self.reset()

    def reset(self):
        self.stride, self.n, self.frames_seen = self.every, 0, 0
        self._kept = []

    def offer(self, t):
        """Frame ``t`` (the running index: 0, 1, 2, ...) arrives -> (slot, moves): the slot to store it in, or None if
        it is not taken, and the (source, destination) slot copies to perform, in order, before storing it."""
        if t != self.frames_seen:
            raise ValueError("SampleSchedule: frame %r offered, %d expected" % (t, self.frames_seen))
        self.frames_seen += 1
        if t % self.stride:
            return None, []
        moves = []
        if self.n == self.capacity:
            moves = [(2 * j, j) for j in range(1, self.capacity // 2)]
            self._kept = self._kept[::2]
            self.stride *= 2
            self.n = self.capacity // 2
        slot = self.n
        self._kept.append(t)
        self.n += 1
        return slot, moves

    def kept(self):
        """The frame indices held, in slot order."""
        return list(self._kept)


class PlateEstimator:
    """Estimates the background plate of an [h,w] clip from its own frames: ``add`` keeps SampleSchedule's frames in
    one uint8 [capacity,h,w,3] device buffer, ``result`` is ops.plate_from_samples of those kept."""

    def __init__(self, h, w, capacity=64, every=1, device=None):
        self.h, self.w = check_int("PlateEstimator", "h", h, 1), check_int("PlateEstimator", "w", w, 1)
        self.schedule = SampleSchedule(capacity, every)
        self.device = device
        self._buf = None  # allocated by the first add

    @property
    def frames_seen(self):
        return self.schedule.frames_seen

    def kept(self):
        return self.schedule.kept()

    def reset(self):
        self.schedule.reset()

    def _check(self, frames):
        import torch
        from . import ops
        # (any strides: add() copies the frames the schedule keeps, one by one)
        shape = ops.check_array("PlateEstimator.add", "frames", frames, (torch.uint8,), "k,h,w,3 | h,w,3", ops.EITHER,
                                strided=True, h=self.h, w=self.w)
        return frames[None] if len(shape) == 3 else frames

    def add(self, frames_u8):
        """The next frame [h,w,3] or frames [k,h,w,3] of the clip, uint8 BGR, numpy or device tensor.  Uploads and slot
        moves run on the current stream."""
        import torch
        frames = self._check(frames_u8)
        if self._buf is None:
            device = self.device if self.device is not None else (frames.device if isinstance(frames, torch.Tensor)
                                                                  else "cuda")
            self._buf = torch.empty((self.schedule.capacity, self.h, self.w, 3), dtype=torch.uint8, device=device)
        for i in range(frames.shape[0]):
            slot, moves = self.schedule.offer(self.schedule.frames_seen)
            for src, dst in moves:
                self._buf[dst].copy_(self._buf[src])
            if slot is not None:
                frame = frames[i]
                self._buf[slot].copy_(frame if isinstance(frame, torch.Tensor)
                                      else torch.from_numpy(np.ascontiguousarray(frame)))
        return self

    def result(self, want_spread=True):
        """(plate uint8 [h,w,3], spread uint8 [h,w] or None) of the frames kept so far, as device tensors."""
        from . import ops
        if self.schedule.n == 0:
            raise ValueError("PlateEstimator.result: no frame was added")
        return ops.plate_from_samples(self._buf[:self.schedule.n], want_spread=want_spread)
