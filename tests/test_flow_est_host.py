"""CPU checks of the flow estimator (csrc/flow_est.hip, ops.estimate_flow, ClipStream(flow="estimate")): the numpy
restatement the kernels are held to (tests/flow_est_ref.py) finds known flows, and every argument check happens on the
host, before any GPU call."""

import numpy as np
import pytest
import torch

import flow_est_ref as ref

P = 64  # a non-null, 16-byte aligned address: validation never dereferences it
BOUND = 0.1  # mean endpoint error in pixels, 20 px inside the border


@pytest.fixture(scope="module")
def errors():
    """name -> mean endpoint error of the f32 restatement at 96 x 128, defaults."""
    out = {}
    for name in ref.FLOWS:
        cur, prev, flow = ref.pair(96, 128, name)
        got = ref.estimate(cur, prev)
        assert got.dtype == np.float32 and got.shape == (96, 128, 2)
        out[name] = ref.endpoint_error(got, flow)
    return out


@pytest.mark.parametrize("name", sorted(ref.FLOWS))
def test_restatement_finds_known_flows(errors, name):
    print("%s: mean endpoint error %.4f px" % (name, errors[name]))
    assert errors[name] <= BOUND


def test_one_level_misses_the_large_shift():
    """Without the pyramid the 12.5 px shift is out of reach: the bound above exercises the coarse-to-fine part."""
    cur, prev, flow = ref.pair(96, 128, "large")
    err = ref.endpoint_error(ref.estimate(cur, prev, levels=1), flow)
    print("levels=1: mean endpoint error %.3f px" % err)
    assert err > BOUND


def test_restatement_pieces():
    assert ref.level_shapes(70, 90, 6) == [(70, 90), (35, 45), (18, 23), (9, 12)]
    assert ref.level_shapes(96, 128, 2) == [(96, 128), (48, 64)]
    assert ref.level_shapes(24, 40, 6) == [(24, 40), (12, 20)]
    cur, prev, _ = ref.pair(32, 48, "small")
    for a in ref.pyramid(cur, 6):
        assert a.dtype == np.float32
    z = ref.estimate(cur, cur)  # a frame against itself: exactly zero, which ClipStream's first frame relies on
    assert not z.any() and not np.signbit(z).any()
    assert ref.estimate(cur, prev, dt=np.float64).dtype == np.float64


def test_level_plan_matches_the_library():
    from vmatting import _lib
    lib = _lib.lib()
    for h, w, levels in ((70, 90, 6), (96, 128, 6), (96, 128, 2), (24, 40, 6), (133, 261, 6), (16, 16, 1)):
        floats = sum((a * b + 3) // 4 * 4 for a, b in ref.level_shapes(h, w, levels))
        assert lib.vm_flow_pyramid_bytes(h, w, levels) == 4 * floats
        assert lib.vm_flow_estimate_workspace_bytes(h, w, levels) >= 3 * 4 * floats + h * w * (3 * 8 + 16)
    assert lib.vm_flow_pyramid_bytes(15, 90, 6) == 0 and lib.vm_flow_estimate_workspace_bytes(70, 90, 0) == 0


def test_c_entries_reject_bad_arguments():
    from vmatting import _lib
    lib = _lib.lib()
    ok = dict(cur=P, prev=P, h=70, w=90, levels=6, warps=3, iters=20, alpha=15.0, flow=P, work=P)

    def estimate(**kw):
        a = dict(ok, **kw)
        return lib.vm_flow_estimate(a["cur"], a["prev"], a["h"], a["w"], a["levels"], a["warps"], a["iters"], a["alpha"],
                                    a["flow"], a["work"], None)

    def from_pyramids(**kw):
        a = dict(ok, **kw)
        return lib.vm_flow_from_pyramids(a["cur"], a["prev"], a["h"], a["w"], a["levels"], a["warps"], a["iters"],
                                         a["alpha"], a["flow"], a["work"], None)

    bad = [dict(cur=None), dict(prev=None), dict(flow=None), dict(work=None), dict(h=15), dict(w=15), dict(h=0),
           dict(w=-3), dict(levels=0), dict(warps=0), dict(iters=0), dict(iters=-1), dict(alpha=0.0), dict(alpha=-1.0),
           dict(alpha=float("nan"))]
    for call, name in ((estimate, b"flow_estimate"), (from_pyramids, b"flow_from_pyramids")):
        for kw in bad:
            rc = call(**kw)
            assert rc == _lib.VM_EINVAL, (name, kw, rc)
            assert name in lib.vm_last_error()
            with pytest.raises(ValueError):
                _lib.check(rc, "flow")
        for kw in (dict(flow=P + 4), dict(work=P + 8), dict(h=40000)):
            assert call(**kw) == _lib.VM_EUNSUPPORTED, (name, kw)
    assert from_pyramids(cur=P + 4) == _lib.VM_EUNSUPPORTED
    for kw in (dict(frame=None), dict(pyr=None), dict(work=None), dict(h=8), dict(levels=0)):
        a = dict(frame=P, h=70, w=90, levels=6, pyr=P, work=P)
        a.update(kw)
        rc = lib.vm_flow_pyramid(a["frame"], a["h"], a["w"], a["levels"], a["pyr"], a["work"], None)
        assert rc == _lib.VM_EINVAL and b"flow_pyramid" in lib.vm_last_error(), kw
    # the per-sweep path is an option of its own
    assert lib.vm_set_option(b"flow_blocked", 0) == _lib.VM_OK and lib.vm_set_option(b"flow_blocked", 1) == _lib.VM_OK
    assert lib.vm_set_option(b"flow_blocked", 2) == _lib.VM_EINVAL


def test_ops_estimate_flow_checks_on_the_host():
    from vmatting import flow, ops
    import flow as shim
    assert shim.estimate_flow is flow.estimate_flow
    a, b = torch.zeros((32, 48, 3), dtype=torch.uint8), torch.zeros((32, 48, 3), dtype=torch.uint8)
    with pytest.raises(TypeError):  # everything is right but the device
        ops.estimate_flow(a, b)
    with pytest.raises(TypeError):
        ops.flow_pyramid(a)
    for kw in (dict(cur=a.float()), dict(prev=b.to(torch.int8)), dict(cur=a.numpy()), dict(levels=2.0), dict(iters=True)):
        k = dict(cur=a, prev=b, levels=6, warps=3, iters=20, alpha=15.0)
        k.update(kw)
        with pytest.raises(TypeError):
            ops.estimate_flow(k.pop("cur"), k.pop("prev"), **k)
    for kw in (dict(cur=a[:, :, :2]), dict(prev=b[:31]), dict(cur=a[None]), dict(cur=a[:, ::2], prev=b[:, ::2]),
               dict(cur=a[:15], prev=b[:15]), dict(levels=0), dict(warps=0), dict(iters=0), dict(alpha=0.0),
               dict(alpha=float("nan")), dict(out=torch.zeros(32, 48)), dict(out=torch.zeros(48, 32, 2))):
        k = dict(cur=a, prev=b, levels=6, warps=3, iters=20, alpha=15.0, out=None)
        k.update(kw)
        with pytest.raises(ValueError):
            ops.estimate_flow(k.pop("cur"), k.pop("prev"), **k)
    # the public wrapper checks numpy frames before it uploads them
    n = np.zeros((32, 48, 3), np.uint8)
    with pytest.raises(TypeError):
        flow.estimate_flow(n.astype(np.float32), n)
    with pytest.raises(TypeError):
        flow.estimate_flow(n, b)
    for args, kw in (((n, n[:31]), {}), ((n[..., 0], n[..., 0]), {}), ((n, n), dict(iters=0)), ((n[:8], n[:8]), {})):
        with pytest.raises(ValueError):
            flow.estimate_flow(*args, **kw)


def _stub_model(dtype=torch.float32):
    """A UNetSimple without its constructor (which packs weights on the device): ClipStream's host-side checks read
    only its type, dtype and device."""
    from vmatting.unet_simple import UNetSimple
    m = UNetSimple.__new__(UNetSimple)
    m.dtype, m.device = dtype, torch.device("cuda")
    return m


def test_clip_stream_estimate_mode_checks_on_the_host():
    from vmatting import ClipStream
    m = _stub_model()
    h, w = 24, 40
    cmp, bg = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.uint8)
    bw = np.zeros((h, w, 2), np.float32)
    a0 = np.zeros((h, w), np.float32)
    for kw in (dict(flow="farneback"), dict(flow=None), dict(flow="estimate", flow_options={"sweeps": 3}),
               dict(flow="estimate", flow_options={"iters": 0}), dict(flow="estimate", flow_options={"alpha": -1.0}),
               dict(flow="given", flow_options={"iters": 5})):
        with pytest.raises(ValueError):
            ClipStream(m, h, w, **kw)
    with pytest.raises(ValueError):
        ClipStream(m, 12, 40, flow="estimate")  # below the estimator's 16 x 16
    assert not ClipStream(m, h, w).estimate  # the default: given flows
    cs = ClipStream(m, h, w, flow="estimate", flow_options={"iters": 7})
    assert cs.estimate and cs.flow_options == {"levels": 6, "warps": 3, "iters": 7, "alpha": 15.0}
    assert cs.check_item((cmp, bg, None, None)) == (cmp, bg, None, None)

    def first(cs, item, **kw):
        return next(cs.run(iter([item]), a0, **kw))

    for item in [(cmp, bg, bw, None), (cmp, bg, None, bw), (cmp, bg, bw, bw), (cmp, bg, None), (cmp, None, None, None),
                 (cmp[:, :39], bg, None, None), (cmp.astype(np.float32), bg, None, None), (cmp, bg, None, None, bg)]:
        with pytest.raises((ValueError, TypeError)):
            first(cs, item)
        assert cs._slots is None  # rejected before anything was allocated on the device
    occ = ClipStream(m, h, w, flow="estimate", occlusion=True, static_bg=bg, out="over", new_bg="per_frame")
    assert occ.check_item((cmp, None, None, None, bg))[4] is bg
    for item in [(cmp, None, None, bw, bg), (cmp, None, bw, bw, bg), (cmp, None, None, None), (cmp, bg, None, None, bg)]:
        with pytest.raises((ValueError, TypeError)):
            first(occ, item)
        assert occ._slots is None
    # cmp0: the uint8 [h,w,3] frame of alpha0, in estimate mode only
    for cmp0 in (cmp[:23], cmp.astype(np.float32), cmp[..., :2]):
        with pytest.raises((ValueError, TypeError)):
            first(cs, (cmp, bg, None, None), cmp0=cmp0)
        assert cs._slots is None
    given = ClipStream(m, h, w)
    with pytest.raises(ValueError, match="cmp0"):
        first(given, (cmp, bg, bw, None), cmp0=cmp)
    assert given._slots is None


def test_flow_tracker_rows_are_16_byte_aligned(monkeypatch):
    """FlowTracker's buffers, allocated on the host here (nothing runs): frames + 1 rows of a multiple of 4 floats.
    The library's count is one already at every size tried, so the round-up is shown on a count that needs it."""
    from vmatting import ops
    from vmatting.flow_track import FlowTracker
    count = ops.flow_pyramid_floats
    for h, w, levels, frames in ((24, 40, 6, 1), (70, 90, 6, 3), (133, 261, 2, 8)):
        opts = ops.flow_options("t", h, w, {"levels": levels})
        assert count(h, w, levels) % 4 == 0
        for extra in (0, 1, 2, 3):
            monkeypatch.setattr(ops, "flow_pyramid_floats", lambda *a, extra=extra: count(*a) + extra)
            tr = FlowTracker(h, w, opts, "cpu", frames=frames)
            monkeypatch.undo()
            floats = count(h, w, levels) + (4 if extra else 0)
            assert tr.rows.shape == (frames + 1, floats) and tr.rows.dtype == torch.float32 and not tr.rows.any()
            assert all(tr.rows[j].data_ptr() % 16 == 0 for j in range(frames + 1))
            assert tr.work.dtype == torch.uint8 and tr.work.numel() == ops.flow_workspace_bytes(h, w, levels)
            assert tr.options == opts and tr.options is not opts
