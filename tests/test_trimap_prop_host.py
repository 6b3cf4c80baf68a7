"""CPU checks of trimap propagation: the numpy restatement (tests/trimap_prop_ref.py) against the definition read
pixel by pixel, its invariants, and the host-side argument checks of FrameStream(trimap="propagate"), which all
happen before any GPU call."""

import numpy as np
import pytest
import torch

import trimap_prop_ref as ref


def brute(prev, flow, grow):
    """include/vmatting.h's definition, one output pixel at a time."""
    h, w = prev.shape
    out = np.empty((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            xs, ys = np.float32(x) + flow[y, x, 0], np.float32(y) + flow[y, x, 1]
            if not (0 <= xs <= w - 1 and 0 <= ys <= h - 1):
                out[y, x] = 128
                continue
            x0, y0 = int(np.floor(xs)), int(np.floor(ys))
            x1, y1 = x0 + (xs > x0), y0 + (ys > y0)
            win = prev[max(y0 - grow, 0):min(y1 + grow, h - 1) + 1, max(x0 - grow, 0):min(x1 + grow, w - 1) + 1]
            out[y, x] = 255 if (win == 255).all() else 0 if (win == 0).all() else 128
    return out


@pytest.mark.parametrize("shape", [(9, 11), (16, 13)])
@pytest.mark.parametrize("grow", [0, 1, 3])
def test_restatement_equals_the_definition(shape, grow):
    h, w = shape
    with np.errstate(invalid="ignore"):
        for tname, make in ref.TRIMAPS.items():
            tri = make(h, w, seed=3)
            for fname, flow in ref.flow_fields(h, w, seed=5).items():
                flow = flow if fname != "random" else flow / np.float32(4)  # (+-3 px: most targets stay inside)
                assert np.array_equal(ref.propagate(tri, flow, grow), brute(tri, flow, grow)), (tname, fname)


def test_inputs_cover_what_they_claim():
    tri = ref.noise_trimap(70, 90)
    assert {0, 128, 255, 1, 127, 254} <= set(np.unique(tri).tolist())
    assert set(np.unique(ref.blob_trimap(70, 90)).tolist()) == {0, 128, 255}
    f = ref.edge_flow(70, 90)
    assert np.isnan(f).any() and np.isposinf(f).any() and np.isneginf(f).any()
    x, y = ref.fer.grid(70, 90, np.float32)
    with np.errstate(invalid="ignore"):
        xs, ys = x + f[..., 0], y + f[..., 1]
        for t, last in ((xs, 89), (ys, 69)):
            assert (t == last).any() and (t == 0).any()
            assert ((t > last) & (t < last + 0.5)).any() and ((t < 0) & (t > -0.5)).any()


def test_zero_flow_without_grow_canonicalises():
    for make in ref.TRIMAPS.values():
        tri = make(37, 53, seed=1)
        assert np.array_equal(ref.propagate(tri, np.zeros((37, 53, 2), np.float32), 0), ref.canonical(tri))


def test_integer_shift_translates_the_interior():
    tri = ref.blob_trimap(40, 60, seed=2)
    dx, dy = 3, -2
    out = ref.propagate(tri, ref.fer.shift_flow(40, 60, dx, dy).astype(np.float32), 0)
    # out(x, y) = tri(x + dx, y + dy) wherever that lies in the image, 128 elsewhere
    assert np.array_equal(out[2:, :57], tri[:38, 3:])
    assert (out[:2] == 128).all() and (out[:, 57:] == 128).all()


def test_unknown_set_grows_with_grow():
    for tname, make in ref.TRIMAPS.items():
        tri = make(45, 67, seed=4)
        for fname, flow in ref.flow_fields(45, 67, seed=6).items():
            unknown = [ref.propagate(tri, flow, g) == 128 for g in (0, 1, 2, 3, 4)]
            for a, b in zip(unknown, unknown[1:]):
                assert (b | ~a).all(), (tname, fname)  # a subset of b
            assert unknown[4].sum() > unknown[0].sum() or fname == "random"


def test_outside_and_non_finite_targets_are_unknown():
    h, w = 12, 20
    tri = np.full((h, w), 255, np.uint8)
    flow = np.zeros((h, w, 2), np.float32)
    flow[0, 0] = (np.nan, 0)
    flow[0, 1] = (0, np.inf)
    flow[0, 2] = (-np.inf, 0)
    flow[1, 3] = (-3.001, 0)          # xs just below 0
    flow[2, 19] = (0.001, 0)          # xs just beyond w - 1
    flow[11, 4] = (0, 0.001)          # ys just beyond h - 1
    flow[5, 5] = (w - 1 - 5, h - 1 - 5)   # exactly the last pixel: inside
    flow[6, 6] = (-6, -6)                 # exactly pixel (0, 0): inside
    for grow in (0, 2):
        out = ref.propagate(tri, flow, grow)
        want = np.full((h, w), 255, np.uint8)
        for y, x in ((0, 0), (0, 1), (0, 2), (1, 3), (2, 19), (11, 4)):
            want[y, x] = 128
        assert np.array_equal(out, want)


def test_chain_keeps_the_key_and_steps_by_each_flow():
    key = ref.noise_trimap(20, 30, seed=7)
    flows = np.stack([f for f in list(ref.flow_fields(20, 30).values())[:4]])
    tris = ref.chain(key, flows, 1)
    assert tris.shape == (4, 20, 30) and np.array_equal(tris[0], key)
    for j in (1, 2, 3):
        assert np.array_equal(tris[j], ref.propagate(tris[j - 1], flows[j], 1))


# ---------------------------------------------------------------- the C entry point and the wrappers, on the host

def test_c_entry_rejects_bad_arguments():
    from vmatting import _lib
    lib = _lib.lib()
    P, Q = 64, 128  # non-null addresses: validation never dereferences them
    bad = [(P, P, 0, 5, 1, Q, P), (P, P, 5, 0, 1, Q, P), (P, P, -1, 5, 1, Q, P),          # h, w < 1
           (P, P, 5, 5, -1, Q, P), (P, P, 5, 5, 9, Q, P),                                 # grow outside 0..8
           (None, P, 5, 5, 1, Q, P), (P, None, 5, 5, 1, Q, P), (P, P, 5, 5, 1, None, P),  # NULLs
           (P, P, 5, 5, 1, Q, None),                                                      # grow > 0 needs a workspace
           (P, P, 5, 5, 1, P, Q), (P, P, 5, 5, 0, P, None),                               # out is prev
           (P, 68, 5, 5, 1, Q, P), (P, P, 5, 5, 1, Q, 72)]                                # misaligned flow / workspace
    for prev, flow, h, w, grow, out, work in bad:
        rc = lib.vm_trimap_propagate(prev, flow, h, w, grow, out, work, None)
        assert rc == _lib.VM_EINVAL, (prev, flow, h, w, grow, out, work)
        assert b"trimap_propagate" in lib.vm_last_error()
    assert lib.vm_trimap_propagate_workspace_bytes(1080, 1920, 0) == 0
    assert lib.vm_trimap_propagate_workspace_bytes(1080, 1920, 9) == 0
    assert lib.vm_trimap_propagate_workspace_bytes(0, 1920, 1) == 0
    # bit rows: one {foreground, background} pair of 64-bit words per 64 pixels of a row
    assert lib.vm_trimap_propagate_workspace_bytes(1080, 1920, 1) == 1080 * 30 * 16
    assert lib.vm_trimap_propagate_workspace_bytes(3, 65, 8) == 3 * 2 * 16
    assert lib.vm_abi_version() == 1


def test_wrappers_check_on_the_host():
    from vmatting import flow, ops
    prev, fl = torch.zeros((4, 6), dtype=torch.uint8), torch.zeros((4, 6, 2))
    with pytest.raises(TypeError):
        ops.trimap_propagate(prev, fl)                       # right tensors, but on the host
    with pytest.raises(TypeError):
        ops.trimap_propagate(prev.float(), fl)
    with pytest.raises(TypeError):
        ops.trimap_propagate(prev, fl.double())
    with pytest.raises(TypeError):
        ops.trimap_propagate(prev.numpy(), fl)
    with pytest.raises(ValueError):
        ops.trimap_propagate(prev, fl[:, :5])
    with pytest.raises(ValueError):
        ops.trimap_propagate(prev[None], fl)
    with pytest.raises(TypeError):
        flow.propagate_trimap(prev.numpy(), fl)              # numpy and torch mixed
    with pytest.raises(TypeError):
        flow.propagate_trimap(prev.numpy().astype(np.int8), fl.numpy())
    with pytest.raises(ValueError):
        flow.propagate_trimap(prev.numpy(), fl.numpy()[:3])
    with pytest.raises(ValueError):
        flow.propagate_trimap(prev.numpy(), fl.numpy(), grow=9)
    with pytest.raises(TypeError):
        flow.propagate_trimap(prev.numpy(), fl.numpy(), grow=1.0)


# ---------------------------------------------------------------- FrameStream(trimap="propagate"), host side

@pytest.fixture(scope="module")
def models(vgg0):
    from vmatting import unet
    np.random.seed(0)  # (the constructors do not touch the device)
    return unet.UNetVideo(vgg0, dtype="bf16", device="cuda"), unet.UNetImage(vgg0, dtype="bf16", device="cuda")


def test_frame_stream_propagate_constructor_errors(models):
    from vmatting import FrameStream
    mv, mi = models
    with pytest.raises(ValueError):
        FrameStream(mi, 32, 48, trimap="propagate")                      # a 6-channel model takes no trimap
    with pytest.raises(ValueError):
        FrameStream(mv, 32, 48, trimap="propagated")
    for kw in (dict(flow="estimate"), dict(flow="given"), dict(flow_options={"iters": 5})):
        with pytest.raises(ValueError):
            FrameStream(mv, 32, 48, **kw)                                # flow / flow_options without propagate
        with pytest.raises(ValueError):
            FrameStream(mi, 32, 48, trimap=False, **kw)
    with pytest.raises(ValueError):
        FrameStream(mv, 32, 48, trimap="propagate", flow="files")
    with pytest.raises(ValueError):
        FrameStream(mv, 32, 48, trimap="propagate", flow="given", flow_options={"iters": 5})
    with pytest.raises(ValueError):
        FrameStream(mv, 32, 48, trimap="propagate", flow_options={"sweeps": 5})
    with pytest.raises(ValueError):
        FrameStream(mv, 32, 48, trimap="propagate", flow_options={"iters": 0})
    with pytest.raises(ValueError):
        FrameStream(mv, 15, 48, trimap="propagate")                      # the estimator needs 16 x 16
    FrameStream(mv, 15, 48, trimap="propagate", flow="given")            # given flows do not
    for grow, exc in ((9, ValueError), (-1, ValueError), (1.0, TypeError), ("1", TypeError), (True, TypeError)):
        with pytest.raises(exc):
            FrameStream(mv, 32, 48, trimap="propagate", grow=grow)
    fs = FrameStream(mv, 32, 48, trimap="propagate", grow=0, flow_options={"iters": 5})
    assert fs.estimate and fs.grow == 0 and fs.flow_options == {"levels": 6, "warps": 3, "iters": 5, "alpha": 15.0}
    assert not FrameStream(mv, 32, 48, trimap="propagate", flow="given").estimate
    assert fs._slots is None
    with pytest.raises(ValueError):
        FrameStream(mv, 32, 48).last_trimap()
    with pytest.raises(RuntimeError):
        fs.last_trimap()


def test_frame_stream_propagate_check_item(models):
    from vmatting import FrameStream
    mv, _ = models
    h, w, k = 16, 24, 2
    cmp, bg = np.zeros((k, h, w, 3), np.uint8), np.zeros((k, h, w, 3), np.uint8)
    key, bw = np.zeros((h, w), np.uint8), np.zeros((k, h, w, 2), np.float32)

    given = FrameStream(mv, h, w, chunk=2, trimap="propagate", flow="given")
    with pytest.raises(ValueError, match="first item"):
        given.check_item((cmp, bg, None, bw))                            # the first item has no key
    bad = [(cmp, bg, key.astype(np.float32), bw), (cmp, bg, key[None], bw), (cmp, bg, key[:, :5], bw),  # the key
           (cmp, bg, torch.zeros(h, w, dtype=torch.uint8), bw),
           (cmp, bg, key, None),                                         # flow="given" without flows
           (cmp, bg, key, bw.astype(np.float64)), (cmp, bg, key, bw[:1]), (cmp, bg, key, bw[..., :1]),
           (cmp, bg, key, bw[0]), (cmp, bg, key, torch.zeros(k, h, w, 2)),
           (cmp, bg, key), (cmp, bg, key, bw, bw),                       # not four entries
           (cmp.astype(np.float32), bg, key, bw), (cmp, None, key, bw), (cmp, bg[:1], key, bw),  # the frames, as ever
           (np.zeros((3, h, w, 3), np.uint8), np.zeros((3, h, w, 3), np.uint8), key, np.zeros((3, h, w, 2), np.float32))]
    for item in bad:
        with pytest.raises((ValueError, TypeError)):
            given.check_item(item)
        with pytest.raises((ValueError, TypeError)):
            next(given.run(iter([item])))
        assert given._slots is None                                      # rejected before anything was allocated
    assert given.check_item((cmp, bg, key, bw))[3] == k
    assert given.check_item((cmp, bg, None, bw))[2] is None              # after a key, an item may continue
    given._keyed = False

    est = FrameStream(mv, h, w, chunk=2, trimap="propagate")
    with pytest.raises(ValueError, match="estimate"):
        est.check_item((cmp, bg, key, bw))                               # flows given although they are estimated
    with pytest.raises(ValueError, match="first item"):
        est.check_item((cmp, bg, None, None))
    assert est.check_item((cmp, bg, key, None))[5] is None

    plates = FrameStream(mv, h, w, chunk=2, trimap="propagate", flow="given", out="over", new_bg="per_frame")
    with pytest.raises(ValueError):
        plates.check_item((cmp, bg, key, bw))                            # new_bg comes last
    with pytest.raises((ValueError, TypeError)):
        plates.check_item((cmp, bg, key, bw, cmp[:1]))
    assert plates.check_item((cmp, bg, key, bw, cmp))[4] is cmp


def test_a_run_starts_without_a_key_again(models):
    """Every run needs its own first key: what the previous run left behind is not continued silently."""
    from vmatting import FrameStream
    mv, _ = models
    fs = FrameStream(mv, 16, 24, chunk=2, trimap="propagate", flow="given")
    fs._keyed = True  # (as after a run)
    item = (np.zeros((2, 16, 24, 3), np.uint8), np.zeros((2, 16, 24, 3), np.uint8), None,
            np.zeros((2, 16, 24, 2), np.float32))
    with pytest.raises(ValueError, match="first item"):
        next(fs.run(iter([item])))
    assert fs._slots is None
