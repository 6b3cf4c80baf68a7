"""vmatting.graphs.capture_passes on the GPU, and the one caller that did not tell the caching allocator about its
warm-up's buffers before it went through it (UNetSimple.capture_fed)."""

import gc

import numpy as np
import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]


def test_capture_passes_two_passes_replay_equals_eager():
    from vmatting.graphs import capture_passes
    x = torch.arange(12, dtype=torch.float32, device="cuda").reshape(3, 4) / 7
    buf, events = {}, []

    def first():  # y = 2x into a buffer made on the first call (the warm-up)
        if "y" not in buf:
            buf["y"] = torch.empty_like(x)
            events.append("alloc")
        return torch.mul(x, 2, out=buf["y"])

    def second():
        if "z" not in buf:
            buf["z"] = torch.empty_like(x)
        return torch.add(buf["y"], 1, out=buf["z"])

    def keep():
        events.append("keep")
        kept.extend(buf.values())
        return [(buf["y"], buf["z"]), None, "not a tensor"]  # tuples are flattened, non-tensors skipped

    def hook():
        events.append("hook")
        capturing.append(torch.cuda.is_current_stream_capturing())
    kept, capturing = [], []
    graphs, results = capture_passes(torch.device("cuda"), [first, second], keep, hook)
    assert len(graphs) == 2 and all(isinstance(g, torch.cuda.CUDAGraph) for g in graphs)
    assert results[0] is buf["y"] and results[1] is buf["z"]
    assert events == ["alloc", "keep", "hook", "hook"] and capturing == [True, True]
    assert len(kept) == 2 and kept[0] is buf["y"]  # keep() ran after the warm-up: it saw the lazily made buffers
    assert not torch.cuda.is_current_stream_capturing()
    x.mul_(-3).add_(0.125)
    buf["y"].zero_()
    buf["z"].zero_()
    for g in graphs:
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(buf["y"], x * 2) and torch.equal(buf["z"], x * 2 + 1)


# the frame of tests/test_gpu_clip_stream.py's fixture, and a second shape that differs in both dimensions: the
# smallest whose five levels (18x26 -> 9x13 -> 5x7 -> 3x4 -> 2x2) still include odd sizes and end above one pixel
HA, WA = 24, 40
HB, WB = 18, 26


def _fed_model(vgg0):
    from oracle import models as om
    from vmatting import unet_simple
    np.random.seed(0)
    m = unet_simple.UNetSimple(unet_simple.Vgg16(vgg0, "bf16"), False, "bf16")
    p = om.unet_simple_params(np.random.RandomState(1))
    w, b = p["output"]  # scaled by 2^-6 (exact) so that the sigmoid does not saturate, as in test_gpu_clip_stream.py
    p["output"] = (w * np.float32(2.0 ** -6), b * np.float32(2.0 ** -6))
    return m.load_params(p)


def _feed(m, h, w, seed):
    """Fill the model's feed_views for one [h,w] frame (ops.clip_feed on seeded uint8 frames, zero flow)."""
    from vmatting import ops
    rs = np.random.RandomState(seed)
    T = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    cmp, bg = (T(rs.randint(0, 256, (1, h, w, 3)).astype(np.uint8)) for _ in range(2))
    prev = T(rs.uniform(0, 1, (1, h, w)).astype(np.float32))
    towers, cat = m.feed_views(1, h, w)
    ops.clip_feed(cmp, bg, prev, torch.zeros((1, h, w, 2), device="cuda"), towers=towers, cat=cat)


def test_fed_shape_switch_after_dropped_graph(vgg0):
    """The analogue of test_shape_switch_after_dropped_graph for UNetSimple.capture_fed: capture at one shape, replay,
    drop the graph, run forward_fed at another shape (the old buffer set is freed and its memory handed out again) and
    back: every output equals a fresh model's eager forward_fed, bit for bit."""
    m, ref = _fed_model(vgg0), _fed_model(vgg0)
    _feed(m, HA, WA, 1)
    g = m.capture_fed(1, HA, WA)
    for _ in range(3):
        g.replay()
    got_a = g.output.clone()
    del g
    gc.collect()
    _feed(m, HB, WB, 2)
    out_b = m.forward_fed(1, HB, WB).clone()
    _feed(m, HA, WA, 1)
    out_a = m.forward_fed(1, HA, WA).clone()
    torch.cuda.synchronize()
    _feed(ref, HA, WA, 1)
    want_a = ref.forward_fed(1, HA, WA).clone()
    _feed(ref, HB, WB, 2)
    want_b = ref.forward_fed(1, HB, WB).clone()
    assert want_a.std() > 0 and want_b.std() > 0
    assert torch.equal(got_a, want_a)
    assert torch.equal(out_b, want_b)
    assert torch.equal(out_a, got_a)
