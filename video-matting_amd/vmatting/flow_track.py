"""The running flow estimate of consecutive frames: one pyramid per frame, its flow against the previous frame's
pyramid, and the last pyramid kept for the next call.  FrameStream(trimap="propagate") and ClipStream, each with
flow="estimate", follow a clip through one FlowTracker inside their captured chains.  MatteScorer keeps its own two
alternating pyramids: through a tracker its eager add() paid one pyramid copy per frame, measurably."""

import torch

from . import ops


class FlowTracker:
    """The pyramids of up to ``frames`` consecutive uint8 [h,w,3] frames per call, at fixed device addresses (a captured
    graph reads the previous frame's pyramid and leaves its last one there): ``rows`` f32 [frames + 1, floats], row 0
    the frame before the call, and ``work``, the one workspace of both flow ops.  ``flow_options``: a checked
    ops.flow_options dict.  Nothing here lives on the host between calls, and nothing is allocated or waited for after
    construction, so seed() and advance() can be captured."""

    def __init__(self, h, w, flow_options, device, frames=1):
        self.h, self.w, self.options = h, w, dict(flow_options)
        levels = self.options["levels"]
        floats = (ops.flow_pyramid_floats(h, w, levels) + 3) // 4 * 4  # every row 16-byte aligned: the C entries ask it
        self.rows = torch.zeros((frames + 1, floats), dtype=torch.float32, device=device)
        self.work = torch.zeros(ops.flow_workspace_bytes(h, w, levels), dtype=torch.uint8, device=device)

    def seed(self, frame):
        """``frame`` (uint8 [h,w,3]) is the frame before the next advance()."""
        ops.flow_pyramid(frame, self.options["levels"], out=self.rows[0], work=self.work)

    def advance(self, frames, backward, forward=None, has_previous=True):
        """The next k <= ``frames`` frames of the clip (uint8 [k,h,w,3]), on the current stream: frame j's pyramid, then
        its flow into the frame before it -> ``backward[j]`` and, with ``forward`` (f32 [k,h,w,2] each), that frame's
        flow into frame j -> ``forward[j]``.  ``has_previous`` False: nothing came before frame 0, whose two flows
        are then not written.  The last frame's pyramid stays behind in row 0."""
        o, rows, k = self.options, self.rows, len(frames)
        for j in range(k):
            ops.flow_pyramid(frames[j], o["levels"], out=rows[j + 1], work=self.work)
            for out, cur, prev in ((backward, rows[j + 1], rows[j]), (forward, rows[j], rows[j + 1])):
                if out is not None and (j or has_previous):
                    ops.flow_from_pyramids(cur, prev, self.h, self.w, o["levels"], o["warps"], o["iters"], o["alpha"],
                                           out=out[j], work=self.work)
        rows[0].copy_(rows[k])
