"""graphs.capture_passes keeps the garbage collector out of a capture: it collects before it records and leaves the
collector off while it records (vmatting/graphs.py says why), and puts it back as it found it."""

import gc
import weakref

import pytest
import torch

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]


class Node:
    pass


@pytest.mark.parametrize("enabled", [True, False])
def test_no_collection_inside_a_capture(enabled):
    from vmatting import graphs
    a, b = Node(), Node()
    a.other, b.other = b, a  # a dead cycle of plain objects once the names go
    alive = weakref.ref(a)
    del a, b
    x = torch.zeros(64, device="cuda")
    seen = []

    def one_pass():
        if torch.cuda.is_current_stream_capturing():
            seen.append((gc.isenabled(), alive() is None))
        x.add_(1.0)

    was = gc.isenabled()
    (gc.enable if enabled else gc.disable)()
    try:
        (g,), _ = graphs.capture_passes(x.device, [one_pass])
        assert gc.isenabled() == enabled
    finally:
        (gc.enable if was else gc.disable)()
    assert seen == [(False, True)]
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 2.0  # the warm-up and one replay
