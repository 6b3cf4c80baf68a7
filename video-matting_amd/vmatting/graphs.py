"""HIP-graph capture, in one place: every captured path of the package (UNet.capture, UNetSimple.capture_fed and the
three trainers' capture()) records its passes through capture_passes.

A capture must not be the first run of its launches: kernels' attributes, folded filters, buffer sets and per-stream
workspaces are built lazily, and an allocation inside a capture would land in the graph's private pool.  So the passes
run once before they are recorded, on a side stream (torch's recipe for warming up ahead of a capture).  What that
warm-up allocated
belongs to the side stream as far as the caching allocator knows, while the graphs replay on the caller's stream:
``record_stream`` tells it, so that a buffer set freed later (the model moved to another shape and the graph was
dropped) is not handed out again while replays queued on the caller's stream may still use it.

No garbage collection may run while a capture is under way: on ROCm a torch.cuda.CUDAGraph synchronises the device when
it is destroyed, a capture under way refuses that call, and the error, raised in a destructor, ends the process.  A dead
reference cycle that holds an earlier graph (a stream whose source raised keeps one alive through the exception's
traceback) is collected whenever the collector next runs, and torch no longer collects on entering a capture.  So
capture_passes collects before it records and keeps the collector off until the last pass is recorded.
"""

import gc

import torch

from . import ops


def _tensors(items):
    for t in items:
        if isinstance(t, (tuple, list)):
            yield from _tensors(t)
        elif isinstance(t, torch.Tensor):
            yield t


def chained(pre, fn, post):
    """One pass: ``pre()`` (if not None), ``fn()``, ``post()`` (if not None); returns fn's result."""
    def run():
        if pre is not None:
            pre()
        out = fn()
        if post is not None:
            post()
        return out
    return run


def capture_passes(device, passes, keep=None, hook=None):
    """Record each of ``passes`` (zero-argument callables that only launch work on the current stream and its forks)
    as one torch.cuda.CUDAGraph, in order, on the current stream -> (graphs, the passes' captured return values).

    All passes first run once, in order, on a fresh side stream that waits on the caller's stream; the caller's stream
    then waits on it and the device is synchronised.  ``keep()`` is called after that warm-up (buffer sets are built
    during it) and returns the tensors the graphs read and write: every tensor in it (tuples and lists flattened,
    anything else skipped) and every per-stream workspace of ops is recorded as used on the caller's stream.
    ``hook()``, if given, runs first inside each pass's capture context."""
    dev = torch.device(device)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for p in passes:
            p()
    main = torch.cuda.current_stream(dev)
    main.wait_stream(side)
    torch.cuda.synchronize(dev)
    for t in _tensors([list(keep()) if keep is not None else (), list(ops._ws_cache.values())]):
        t.record_stream(main)
    graphs, results = [], []
    gc.collect()
    collecting = gc.isenabled()
    gc.disable()
    try:
        for p in passes:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                if hook is not None:
                    hook()
                results.append(p())
            graphs.append(g)
    finally:
        if collecting:
            gc.enable()
    return graphs, results
