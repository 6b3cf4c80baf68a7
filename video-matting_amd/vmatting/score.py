"""MatteScorer: the matting metrics of a clip against ground truth, followed chunk by chunk on the device.

    scorer = MatteScorer(h, w)
    for mattes, gt, trimaps in chunks:        # [k,h,w] each, numpy arrays or device tensors
        scorer.add(mattes, gt, trimaps)
    figures = scorer.result()                 # ops.score_summary of every frame added

Each add() is one ops.matte_score call (include/vmatting.h has the definitions).  The last frame of a chunk stays behind
as the next chunk's ``prev``, so the temporal figures do not depend on how the clip is cut; nothing synchronises before
result().
"""

import numpy as np
import torch

from . import ops

FLOW_MODES = (None,) + ops.FLOW_MODES


class MatteScorer:
    """SAD, MSE, gradient error, dtSSD and MESSDdt of predicted mattes against ground truth over a clip of [h,w] frames.

    ``flow``: None scores without MESSDdt; "given": add() takes each frame's backward flow (frame j into frame j - 1,
    reader.read_flow layout, what ClipStream and FrameStream(trimap="propagate") consume); "estimate": add() takes the
    frames' uint8 BGR composites and estimates the flows itself with ops.estimate_flow's arithmetic (``flow_options``:
    its levels / warps / iters / alpha), one pyramid per frame shared by the two pairs it belongs to."""

    def __init__(self, h, w, device="cuda", flow=None, flow_options=None):
        self.h, self.w = ops.check_int("MatteScorer", "h", h, 1), ops.check_int("MatteScorer", "w", w, 1)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("MatteScorer: a ROCm device is required, got %r" % (device,))
        self.flow_options = ops.check_flow_mode("MatteScorer", flow, flow_options, self.h, self.w, FLOW_MODES)
        self.flow = flow
        self._work = self._pyr = self._flow_work = None
        self.reset()

    def reset(self):
        """Start a new clip: the frames added so far, the carried previous frame and the matte dtypes are forgotten."""
        self._rows = []
        self._prev = None       # (pred, gt) of the last frame added, device [h,w]
        self._dtypes = None     # (pred dtype, gt dtype) of the clip
        self._have_pyr = False  # flow="estimate": self._pyr[self._last_pyr] holds the last frame's pyramid
        self._last_pyr = 0
        self.frames = 0

    # ------------------------------------------------------------------------------------------ host-side checks
    def check_chunk(self, pred, gt, trimap=None, backward=None, cmp=None):
        """Types, dtypes and shapes of one add(), on the host -> k."""
        who, matte, dims = "MatteScorer.add", (torch.float32, torch.uint8), {"h": self.h, "w": self.w}
        dims["k"] = k = ops.check_array(who, "pred", pred, matte, "k,h,w", ops.EITHER, **dims)[0]
        for name, given, mode in (("backward", backward, "given"), ("cmp", cmp, "estimate")):
            if (given is not None) != (self.flow == mode):
                raise ValueError("%s: %s goes with flow=%r, and then every chunk needs it (this scorer has flow=%r)" %
                                 (who, name, mode, self.flow))
        for name, a, dtypes, shapes in (("gt", gt, matte, "k,h,w"), ("trimap", trimap, (torch.uint8,), "k,h,w"),
                                        ("backward", backward, (torch.float32,), "k,h,w,2"),
                                        ("cmp", cmp, (torch.uint8,), "k,h,w,3")):
            if a is not None or name == "gt":
                ops.check_array(who, name, a, dtypes, shapes, ops.EITHER, **dims)
        dts = (ops.torch_dtype(pred), ops.torch_dtype(gt))
        if self._dtypes is not None and dts != self._dtypes:
            raise TypeError("%s: pred / gt were %s / %s so far and are %s / %s now; reset() starts a new clip" %
                            ((who,) + self._dtypes + dts))
        return k

    # ------------------------------------------------------------------------------------------ the device side
    def _dev(self, a):
        if a is None or isinstance(a, torch.Tensor):
            return a
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def _flows(self, cmp, k):
        """The backward flow of each of the chunk's k frames from the composites: frame j's pyramid, then its flow
        against the pyramid before it (the previous chunk's last one for frame 0).  Frame 0 of a clip has no flow; its
        zeros are not read."""
        o = self.flow_options
        if self._pyr is None:
            floats = (ops.flow_pyramid_floats(self.h, self.w, o["levels"]) + 3) // 4 * 4  # row 1 16-byte aligned too
            self._pyr = torch.zeros((2, floats), dtype=torch.float32, device=self.device)
            self._flow_work = torch.zeros(ops.flow_workspace_bytes(self.h, self.w, o["levels"]), dtype=torch.uint8,
                                          device=self.device)
        bw = torch.zeros((k, self.h, self.w, 2), dtype=torch.float32, device=self.device)
        for j in range(k):
            cur = 1 - self._last_pyr
            ops.flow_pyramid(cmp[j], o["levels"], out=self._pyr[cur], work=self._flow_work)
            if self._have_pyr:
                ops.flow_from_pyramids(self._pyr[cur], self._pyr[self._last_pyr], self.h, self.w, o["levels"], o["warps"],
                                       o["iters"], o["alpha"], out=bw[j], work=self._flow_work)
            self._last_pyr, self._have_pyr = cur, True
        return bw

    def add(self, pred, gt, trimap=None, backward=None, cmp=None):
        """Score the next k >= 1 frames of the clip: ``pred`` and ``gt`` [k,h,w] (f32 or uint8, independently, the same
        for the whole clip), ``trimap`` uint8 [k,h,w] or None; with flow="given" ``backward`` f32 [k,h,w,2], with
        flow="estimate" ``cmp`` uint8 [k,h,w,3].  numpy arrays are uploaded on the current stream; contiguous device
        tensors are read in place.  Nothing is waited for."""
        k = self.check_chunk(pred, gt, trimap, backward, cmp)
        pred, gt, trimap, backward, cmp = (self._dev(a) for a in (pred, gt, trimap, backward, cmp))
        if self.flow == "estimate":
            backward = self._flows(cmp, k)
        nwork = ops.matte_score_workspace_bytes(k, self.h, self.w)
        if self._work is None or self._work.numel() < nwork:
            self._work = torch.empty(nwork, dtype=torch.uint8, device=self.device)
        self._rows.append(ops.matte_score(pred, gt, trimap, self._prev, backward, work=self._work))
        if self._prev is None:
            self._prev = (torch.empty_like(pred[0]), torch.empty_like(gt[0]))
            self._dtypes = (pred.dtype, gt.dtype)
        self._prev[0].copy_(pred[k - 1])
        self._prev[1].copy_(gt[k - 1])
        self.frames += k
        return self

    def stats(self):
        """The f64 [frames,8] table of ops.matte_score rows added so far, on the host (waits for the device)."""
        if not self._rows:
            return np.zeros((0, 8), np.float64)
        return torch.cat(self._rows).cpu().numpy()

    def result(self):
        """ops.score_summary of every frame added since the last reset(): per-frame arrays and the clip's means.  The
        one place that waits for the device."""
        return ops.score_summary(self.stats(), first_has_prev=False, has_flow=self.flow is not None)
