"""vm_plate_align_fit / vm_plate_align_apply on the GPU against the numpy restatement (tests/plate_align_ref.py): the
resampled plate bit for bit, the fit's support exactly and its map within a measured bound (the two differ in the order
of their f64 sums only); a batch equals single calls and two runs each other, bit for bit."""

import numpy as np
import pytest
import torch

import flow_est_ref as fe
import plate_align_ref as ref
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

FILL = 0xA5
# The largest difference between the device's and the restatement's corner displacements over every case of
# test_fit_equals_the_restatement, measured on an MI355X: 0 - every parameter came out bit for bit (the f64 sums differ
# in their order only, and that does not survive the rounding of a step to f32).  Eight times that is no bound, so the
# bound is what the number format leaves open instead: a parameter that rounds the other way moves a corner by an f32
# ulp of its displacement, 2^-20 px below 16 px, and 2^-18 px allows four of those.  The issue's ceiling is 1 / 1024 px: a
# position error d moves a bilinear byte by at most 2 * 255 * d, under half a level there.
WORST_SEEN = 0.0
BOUND = max(8 * WORST_SEEN, 2.0 ** -18)
assert BOUND <= 1.0 / 1024


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def at_offset(a, off):
    """``a`` (uint8 numpy) on the device at byte 32 + ``off`` of a buffer with FILL bytes around it -> (buffer, view)."""
    buf = torch.full((32 + 4 + a.size + 32,), FILL, dtype=torch.uint8, device="cuda")
    view = buf[32 + off:32 + off + a.size].view(a.shape)
    view.copy_(dev(a))
    return buf, view


def pyramids(frames, levels=6):
    """uint8 [n,h,w,3] numpy -> the frames' pyramids on the device, f32 [n,floats]."""
    from vmatting import ops
    n, h, w, _ = frames.shape
    floats = (ops.flow_pyramid_floats(h, w, levels) + 3) // 4 * 4
    rows = torch.zeros((n, floats), dtype=torch.float32, device="cuda")
    work = torch.empty(ops.flow_workspace_bytes(h, w, levels), dtype=torch.uint8, device="cuda")
    return ops.frame_pyramids(dev(frames), levels, rows, work)


def device_fit(cmp, bg, **opts):
    """cmp uint8 [n,h,w,3], bg [nb,h,w,3] -> (params f32 [n,8], support int64 [n]) as numpy, with the workspace
    pre-filled with 0xFF and sentinels around the results."""
    from vmatting import ops
    n, h, w, _ = cmp.shape
    pbuf = torch.full((n * 8 + 16,), -7777.0, dtype=torch.float32, device="cuda")
    sbuf = torch.full((n + 8,), -7777, dtype=torch.int32, device="cuda")
    work = torch.full((ops.plate_align_workspace_bytes(n, h, w, opts.get("levels", 6)),), 0xFF, dtype=torch.uint8,
                      device="cuda")
    prm, sup = ops.plate_align_fit(pyramids(cmp, opts.get("levels", 6)), pyramids(bg, opts.get("levels", 6)), h, w,
                                   out=pbuf[8:8 + 8 * n].view(n, 8), support=sbuf[4:4 + n], work=work, **opts)
    for buf, lo, hi in ((pbuf.cpu().numpy(), 8, 8 + 8 * n), (sbuf.cpu().numpy(), 4, 4 + n)):
        assert (buf[:lo] == -7777).all() and (buf[hi:] == -7777).all()
    return prm.cpu().numpy(), sup.cpu().numpy().astype(np.int64)


# ---------------------------------------------------------------- apply
MAPS = np.array([[0, 0, 0, 0, 0, 0, 1, 0],                       # the identity
                 [0, 0, .5, 0, 0, .5, 1, 0],                     # half a pixel
                 [0, 0, 3.5, 0, 0, -2.25, .8, 0],                # (the gain is not applied)
                 [-5e-5, -.01, 1.2, .01, -5e-5, -.8, 1, 0],      # a rotation
                 [.5, .05, 1.3, -.05, .5, -.7, 1, 0],            # leaves the plate on every side
                 [0, 0, 1e6, 0, 0, -1e6, 1, 0]], np.float32)     # far outside: one corner's colour


@pytest.mark.parametrize("h,w,offs", [(16, 16, (0, 0)), (17, 23, (1, 3)), (17, 23, (2, 1)), (96, 160, (3, 2))])
def test_apply_equals_the_restatement(h, w, offs):
    from vmatting import ops
    rs = np.random.RandomState(h)
    n = len(MAPS)
    bg = rs.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    for nb in (1, n):
        _, d_bg = at_offset(bg[:nb], offs[0])
        obuf, out = at_offset(np.zeros((n, h, w, 3), np.uint8), offs[1])
        out.fill_(FILL)
        ops.plate_align_apply(d_bg, dev(MAPS), out=out)
        got = out.cpu().numpy()
        assert np.array_equal(got, ref.applies(bg[:nb], MAPS))
        assert np.array_equal(got[0], bg[0])                      # the identity reproduces the plate
        assert (got[5] == bg[0 if nb == 1 else 5][0, -1]).all()
        edge = obuf.cpu().numpy()
        assert (edge[:32 + offs[1]] == FILL).all() and (edge[32 + offs[1] + bg.size:] == FILL).all()
    one = ops.plate_align_apply(dev(bg[0]), dev(MAPS[1:2])).cpu().numpy()  # one [h,w,3] plate, out allocated
    assert np.array_equal(one, ref.applies(bg[0], MAPS[1:2]))


# ---------------------------------------------------------------- fit
CASES = [(16, 16, "id", 1.0), (16, 16, "sub", 1.25), (17, 23, "sub", 1.0), (17, 23, "one", 0.8),
         (64, 96, "id", 0.8), (64, 96, "sub", 1.0), (64, 96, "rot", 1.25), (64, 96, "zoom", 1.0), (64, 96, "big", 1.0),
         (64, 96, "shift", 1.25), (96, 160, "id", 1.0), (96, 160, "sub", 0.8), (96, 160, "one", 1.25),
         (96, 160, "shift", 1.0), (96, 160, "big", 0.8), (96, 160, "rot", 1.0), (96, 160, "zoom", 1.25)]


def clear_scene(h, w, motion, gain):
    """The scene of the first seed whose last step in the restatement has no residual within 1e-3 of a gate (``tol`` for
    the inliers, ``tol`` / 4 for the support): a gate decision on such a residual is the one thing that could move the
    device's result off the restatement's -> (frame, plate, true, params, support, seed)."""
    for seed in range(8):
        frame, plate, _, true = ref.scene(h, w, motion, gain, seed)
        trace = []
        prm, sup = ref.fit(fe.pyramid(frame, 6), fe.pyramid(plate, 6), h, w, trace=trace)
        r = np.abs(trace[-1][1])
        if min(np.abs(r - np.float32(16)).min(), np.abs(r - np.float32(4)).min()) > 1e-3:
            return frame, plate, true, prm, sup, seed
    raise AssertionError("no clear seed")


@pytest.fixture(scope="module")
def scenes():
    return {c: clear_scene(*c) for c in CASES}


def test_fit_equals_the_restatement(scenes):
    worst, errors = 0.0, {}
    for (h, w, motion, gain), (frame, plate, true, prm, sup, seed) in scenes.items():
        got, gsup = device_fit(frame[None], plate[None])
        d = ref.displacement(got[0], h, w).astype(np.float64) - ref.displacement(prm, h, w).astype(np.float64)
        diff = float(np.sqrt((d ** 2).sum(-1)).max())
        err = ref.corner_error(got[0], true, h, w)
        print("%3d x %3d %-5s gain %.2f seed %d: support %5d / %5d, device - restatement %.3e px, g %.3e, corner error "
              "%.4f px%s" % (h, w, motion, gain, seed, gsup[0], sup, diff, abs(float(got[0, 6]) - float(prm[6])), err,
                             " (identity)" if np.array_equal(got[0], ref.identity()) else ""))
        worst = max(worst, diff)
        errors[h, w, motion, gain] = (gsup[0] == sup, diff, abs(float(got[0, 6]) - float(prm[6])), got[0, 7])
    print("worst device - restatement corner difference: %.3e px (bound %.3e)" % (worst, BOUND))
    for case, (same, diff, dg, pad) in errors.items():
        assert same and diff <= BOUND and dg <= 1e-5 and pad == 0, (case, same, diff, dg)
    fitted = [c for c, s in scenes.items() if not np.array_equal(s[3], ref.identity())]
    assert len(fitted) >= len(CASES) - 4  # (the identity would pass a lazy kernel)


def test_options_reach_the_kernels(scenes):
    h, w = 96, 160
    frame, plate, true, prm, sup, _ = scenes[h, w, "big", 0.8]
    got, _ = device_fit(frame[None], plate[None], reach=8)   # 12 px: the 15.4 px of `big` are beyond it
    assert np.array_equal(got[0], ref.identity())
    frame, plate = scenes[h, w, "one", 1.25][:2]
    default = scenes[h, w, "one", 1.25][3]
    for opts in ({"levels": 3, "iters": 3}, {"tol": 8.0, "min_share": 2}):
        want, wsup = ref.fit_frames(frame, plate, **opts)
        assert not np.array_equal(want, default) and not np.array_equal(want, ref.identity())
        got, gsup = device_fit(frame[None], plate[None], **opts)
        d = ref.displacement(got[0], h, w).astype(np.float64) - ref.displacement(want, h, w).astype(np.float64)
        print(opts, gsup[0], wsup, float(np.abs(d).max()))
        # (this seed is not picked clear of these options' gates: a pixel or two may fall on the other side of one,
        # each a share of about 1 / support of the sums)
        assert abs(gsup[0] - wsup) <= 2 and np.abs(d).max() <= 1.0 / 1024


def test_batches_and_reruns_are_bit_equal(scenes):
    """n = 3 in one call equals three single calls and a second run, bit for bit, for nb = 1 and nb = n."""
    h, w = 96, 160
    keys = [(h, w, "shift", 1.0), (h, w, "rot", 1.0), (h, w, "zoom", 1.25)]
    cmp = np.stack([scenes[k][0] for k in keys])
    plates = np.stack([scenes[k][1] for k in keys])
    for bg in (plates, plates[:1]):
        prm, sup = device_fit(cmp, bg)
        again, sup2 = device_fit(cmp, bg)
        assert prm.tobytes() == again.tobytes() and np.array_equal(sup, sup2)
        for i in range(3):
            one, s1 = device_fit(cmp[i:i + 1], bg[i:i + 1] if len(bg) > 1 else bg)
            assert one.tobytes() == prm[i:i + 1].tobytes() and s1[0] == sup[i]
        assert not any(np.array_equal(p, ref.identity()) for p in prm[:1])
    # several blocks per frame (more than 2048 pixels a level) and one: both sides of the partials' sum
    assert h * w > 2048 * 4 and (h // 8) * (w // 8) < 2048


@pytest.mark.parametrize("h,w", [(96, 160), (17, 23)])
def test_nothing_to_fit_is_the_identity(h, w):
    pairs = [fn(h, w, 1) for fn in ref.DEGENERATE.values()]
    cmp, bg = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    want, wsup = ref.fits(cmp, bg)
    prm, sup = device_fit(cmp, bg)
    assert np.array_equal(prm, np.stack([ref.identity()] * 3)) and np.array_equal(want, prm)
    assert np.array_equal(sup, wsup) and sup[0] == 0 and (sup * 4 < h * w).all()


def test_captured_graph_follows_its_inputs(scenes):
    import gc
    from vmatting import ops
    h, w = 64, 96
    a, b = scenes[h, w, "rot", 1.25], scenes[h, w, "zoom", 1.0]
    d_cmp, d_bg = dev(a[0][None]), dev(a[1][None])
    floats = (ops.flow_pyramid_floats(h, w, 6) + 3) // 4 * 4
    rows = torch.zeros((2, floats), dtype=torch.float32, device="cuda")
    pwork = torch.empty(ops.flow_workspace_bytes(h, w, 6), dtype=torch.uint8, device="cuda")
    prm, sup = torch.zeros((1, 8), device="cuda"), torch.zeros((1,), dtype=torch.int32, device="cuda")
    out = torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
    work = torch.full((ops.plate_align_workspace_bytes(1, h, w, 6),), 0xFF, dtype=torch.uint8, device="cuda")

    def chain():
        ops.frame_pyramids(d_cmp, 6, rows[:1], pwork)
        ops.frame_pyramids(d_bg, 6, rows[1:], pwork)
        ops.plate_align_fit(rows[:1], rows[1:], h, w, out=prm, support=sup, work=work)
        ops.plate_align_apply(d_bg, prm, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gc.collect()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    for frame, plate in ((b[0], b[1]), (a[0], a[1])):
        d_cmp.copy_(dev(frame[None]))
        d_bg.copy_(dev(plate[None]))
        for t in (prm, sup, out):
            t.zero_()
        g.replay()
        eager, esup = device_fit(frame[None], plate[None])
        assert prm.cpu().numpy().tobytes() == eager.tobytes() and int(sup[0]) == esup[0]
        assert np.array_equal(out.cpu().numpy(), ref.applies(plate, eager))


def test_c_calls_reject_bad_arguments():
    """Every refused call returns before it touches the device: the pointers are not device memory."""
    from vmatting import _lib
    lib = _lib.lib()
    torch.cuda.synchronize()
    for args in ref.bad_fit_arguments():
        assert lib.vm_plate_align_fit(*args, None) == _lib.VM_EINVAL, args
    for args in ref.bad_apply_arguments():
        assert lib.vm_plate_align_apply(*args, None) == _lib.VM_EINVAL, args
    torch.cuda.synchronize()
