"""Frame-parallel matting of a video batch (BASELINE config 4) — the product path that bench.py times.

The reference evaluates its per-frame forward inside sess.run over batches drawn from a frame list
(train.py:318-332); frames never interact at inference (UNetVideo has no BN), so a video batch of F frames is
cut into contiguous per-rank blocks (parallel.shard_range), each rank runs its block through UNetVideo in
chunks of ``chunk`` frames, and one all-gather (RCCL ring over xGMI) hands every rank the whole matte batch.

Chunks are recorded as HIP graphs whose input IS the caller's frame slice and whose alpha output IS the
result slice (UNet.capture(static=True, out=...)): no per-frame staging copies, one host call per chunk, and a
chunk of 8 frames gives the small L4/L5 convs 8x the tiles of a single frame.  All chunks share the model's
activation buffers (they run in order on one stream).
"""

import torch

from . import ops, parallel
from .split6 import rerun_x6

VGG_MEAN = (103.939, 116.779, 123.68)  # params.py:10


def synthetic_frames(n, h, w, first=0, device="cuda"):
    """SURVEY.md §8d synthetic 7-channel frames, generated on the device: frame f (seed 1234+f): composite and
    background BGR U{0..255} - VGG_MEAN; trimap {0, .5, 1} - .5 from a random ellipse with an 8-px unknown band
    (loader.py:76-78 layout).  -> [n, h, w, 7] f32."""
    out = torch.empty((n, h, w, 7), dtype=torch.float32, device=device)
    mean = torch.tensor(VGG_MEAN, device=device)
    yy = torch.arange(h, device=device, dtype=torch.float32)[:, None]
    xx = torch.arange(w, device=device, dtype=torch.float32)[None, :]
    for i in range(n):
        g = torch.Generator(device=device)
        g.manual_seed(1234 + first + i)
        out[i, :, :, 0:3] = torch.randint(0, 256, (h, w, 3), generator=g, device=device).float() - mean
        out[i, :, :, 3:6] = torch.randint(0, 256, (h, w, 3), generator=g, device=device).float() - mean
        c = torch.rand(4, generator=g, device=device)
        cy, cx = (0.3 + 0.4 * c[0]) * h, (0.3 + 0.4 * c[1]) * w
        ry, rx = (0.15 + 0.15 * c[2]) * h, (0.15 + 0.15 * c[3]) * w
        d = torch.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)
        band = 8.0 / float(min(ry, rx))
        tri = torch.where(d < 1 - band, 1.0, torch.where(d < 1 + band, 0.5, 0.0))
        out[i, :, :, 6] = tri - 0.5
    return out


class VideoMatter:
    """Mattes for frames[a:b] of a video batch resident on the device: ``run()`` replays the chunk graphs into
    ``alpha`` ([b-a, H, W, 1] f32).  ``frames`` is this rank's [b-a, H, W, 7] f32 block (kept alive by the
    object: the graphs read it in place).  On an f16x3 model, chunks whose activations leave fp16's range are
    re-run on bf16x6 and listed in ``overflowed_chunks`` (see run())."""

    def __init__(self, model, frames, chunk=8, graph=True, alpha=None, _u8=None):
        # _u8 (from_uint8 only): the (cmp, bg, trimap) uint8 tensors each chunk's frames are made from, in its graph
        if _u8 is None and (frames.dim() != 4 or not frames.is_cuda or frames.dtype != torch.float32 or
                            not frames.is_contiguous()):
            raise ValueError("frames must be a contiguous [F,H,W,C] f32 device tensor")
        model.prepare()
        self.model, self.frames, self.chunk = model, frames, max(1, int(chunk))
        self._u8 = _u8
        f, h, w, _ = frames.shape
        self.alpha = alpha if alpha is not None else torch.empty((f, h, w, 1), dtype=torch.float32,
                                                                 device=frames.device)
        if tuple(self.alpha.shape) != (f, h, w, 1) or not self.alpha.is_contiguous():
            raise ValueError("alpha must be a contiguous [F,H,W,1] f32 tensor")
        self.spans = [(i, min(f, i + self.chunk)) for i in range(0, f, self.chunk)]
        # f16x3: one range-flag slot per chunk (chunk k's forward, captured or eager, zeroes and sets slot k only), so
        # a later chunk cannot clear an earlier one's report; the other paths have no flag and get no slot
        self._slots = None
        if model.split_mode == "f16x3" and self.spans:
            self._slots = torch.zeros(len(self.spans), dtype=torch.int32, device=frames.device)
        self._x6 = None  # the bf16x6 forward of the same parameters, built when a chunk first overflows
        self.overflowed_chunks = []  # after run(): the chunks (indices into spans) that left fp16's range
        self.graphs = None
        if graph and f > 0:
            self.graphs = [model.capture(frames[a:b], static=True, out=self.alpha[a:b], overflow=self._slot(k),
                                         pre=None if _u8 is None else (lambda k=k: self._ingest(k)))
                           for k, (a, b) in enumerate(self.spans)]

    @classmethod
    def from_uint8(cls, model, cmp, bg, trimap=None, chunk=8, graph=True, alpha=None):
        """A VideoMatter over decoded frames resident on the device: cmp uint8 [F,H,W,3] BGR, bg uint8 [F,H,W,3] or
        one static plate [H,W,3], trimap uint8 [F,H,W] (UNetVideo) or None (UNetImage).  The frame buffer is
        allocated in the model's input format (bf16 8-channel pixels for a plain bf16 model, f32 otherwise) and
        every chunk's frames are made by ops.frames_from_u8 inside that chunk's graph (or eagerly), so ``run()``
        reads the uint8 tensors as they are then: the float64 mean subtraction of the reference's feed
        (loader.py:45,75-78), bit for bit.  Otherwise it is the VideoMatter of those frames."""
        f, h, w, _ = ops._check_frames_and_bg("from_uint8", cmp, bg)
        if trimap is not None:
            ops._check_tensor("from_uint8", "trimap", trimap, (torch.uint8,), "n,h,w", n=f, h=h, w=w)
        c = 6 if trimap is None else 7
        if c != model.IN_CH:
            raise ValueError("%s takes %d input channels: trimap %s" % (type(model).__name__, model.IN_CH,
                                                                       "required" if model.IN_CH == 7 else "not taken"))
        for t in (cmp, bg) + (() if trimap is None else (trimap,)):
            ops._require_gpu(t)
        return cls(model, ops.frame_buffer(model, f, h, w), chunk, graph, alpha, _u8=(cmp, bg, trimap))

    def _ingest(self, k):
        a, b = self.spans[k]
        cmp, bg, tri = self._u8
        ops.frames_from_u8(cmp[a:b], bg if bg.dim() == 3 or bg.shape[0] == 1 and cmp.shape[0] > 1 else bg[a:b],
                           None if tri is None else tri[a:b], out=self.frames[a:b])

    def _slot(self, k):
        return None if self._slots is None else self._slots[k:k + 1]

    def run(self):
        """Matte every chunk into ``alpha``.  On an f16x3 model the chunks' range flags are then read once (one host
        synchronisation per run) and every flagged chunk is run again, eagerly, on a bf16x6 forward of the same
        parameters (f32 range; ~2x slower) into the same alpha slice; ``overflowed_chunks`` lists them.  The model
        stays f16x3 and the captured graphs stay valid (its .output / .conv1_3 attributes still describe the last
        f16x3 forward)."""
        if self.graphs is not None:
            for g in self.graphs:
                g.replay()
        else:
            for k, (a, b) in enumerate(self.spans):
                if self._u8 is not None:
                    self._ingest(k)
                self.model.forward(self.frames[a:b], out=self.alpha[a:b], overflow=self._slot(k))
        if self._slots is not None:
            self.overflowed_chunks = [k for k, v in enumerate(self._slots.tolist()) if v]
            for k in self.overflowed_chunks:
                a, b = self.spans[k]
                rerun_x6(self, self.frames[a:b], self.alpha[a:b])
        return self.alpha


def shard(n_frames, rank=None, world=None):
    """This rank's contiguous [start, stop) block of an n_frames video batch."""
    if world is None:
        world = parallel.world_size()
    if rank is None:
        rank = torch.distributed.get_rank() if world > 1 else 0
    return parallel.shard_range(n_frames, rank, world)


def matte_video(model, frames, n_frames, chunk=8, graph=True, recv=None):
    """Config 4 in one call: ``frames`` is this rank's block (shard(n_frames)) as [b-a, H, W, 7] f32 on the
    device; returns (the all-gathered [n_frames, H, W, 1] matte batch, the VideoMatter, so a caller can replay
    it).  ``recv`` optionally preallocates the [world * max_block, H, W, 1] all-gather buffer."""
    vm = VideoMatter(model, frames, chunk, graph)
    vm.run()
    return parallel.gather_frames(vm.alpha, n_frames, out=recv), vm
