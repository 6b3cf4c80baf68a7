"""Trimap propagation on the GPU: ops.trimap_propagate against the numpy restatement (tests/trimap_prop_ref.py), byte
for byte, and FrameStream(trimap="propagate") against FrameStream(trimap=True) fed the restatement's trimaps, bit for
bit."""

import numpy as np
import pytest
import torch

import flow_est_ref as fer
import trimap_prop_ref as ref
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

SHAPES = [(70, 90), (133, 261), (1, 17), (19, 1)]  # 133 x 261: 5 x 3 class-map tiles, 9 gather blocks, a ragged last one
GROWS = [0, 1, 3, 8]
SENTINEL = 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(nbytes, fill, lead=0):
    """A uint8 device buffer of ``nbytes`` with SENTINEL bytes of ``fill`` behind it (and ``lead`` in front)."""
    buf = torch.full((lead + nbytes + SENTINEL,), fill, dtype=torch.uint8, device="cuda")
    return buf, buf[lead:lead + nbytes]


def intact(buf, nbytes, fill, lead=0):
    b = buf.cpu().numpy()
    return (b[:lead] == fill).all() and (b[lead + nbytes:] == fill).all()


@pytest.mark.parametrize("grow", GROWS)
@pytest.mark.parametrize("shape", SHAPES)
def test_propagate_equals_the_restatement(shape, grow):
    from vmatting import ops
    h, w = shape
    nwork = ops.trimap_propagate_workspace_bytes(h, w, grow)
    assert (nwork > 0) == (grow > 0)
    for tname, make in ref.TRIMAPS.items():
        tri = make(h, w, seed=11)
        d_tri = dev(tri)
        for fname, flow in ref.flow_fields(h, w, seed=13).items():
            obuf, out = guarded(h * w, 0xA5)
            wbuf, work = guarded(nwork, 0x5A)
            got = ops.trimap_propagate(d_tri, dev(flow), grow, out=out.view(h, w), work=work)
            assert got.data_ptr() == out.data_ptr()
            want = ref.propagate(tri, flow, grow)
            assert np.array_equal(got.cpu().numpy(), want), (tname, fname)
            assert intact(obuf, h * w, 0xA5) and intact(wbuf, nwork, 0x5A), (tname, fname)
            assert np.array_equal(d_tri.cpu().numpy(), tri)


@pytest.mark.parametrize("grow", [0, 3])
def test_unaligned_output_and_allocated_buffers(grow):
    """An output that does not start on 16 bytes is stored bytewise, nothing before or behind it is touched; and the
    call allocates what it is not given."""
    from vmatting import flow as vflow
    from vmatting import ops
    h, w = 133, 261
    tri, fl = ref.blob_trimap(h, w, seed=2), ref.flow_fields(h, w, seed=3)["random"]
    want = ref.propagate(tri, fl, grow)
    obuf, out = guarded(h * w, 0xA5, lead=3)
    assert out.data_ptr() % 16 == 3
    got = ops.trimap_propagate(dev(tri), dev(fl), grow, out=out.view(h, w))
    assert np.array_equal(got.cpu().numpy(), want) and intact(obuf, h * w, 0xA5, lead=3)
    assert np.array_equal(ops.trimap_propagate(dev(tri), dev(fl), grow).cpu().numpy(), want)
    # flow.propagate_trimap: numpy in, numpy out; device tensors stay on the device
    got = vflow.propagate_trimap(tri, fl, grow)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want)
    got = vflow.propagate_trimap(dev(tri), dev(fl), grow)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)


def test_five_step_chain():
    from vmatting import ops
    h, w = 133, 261
    key = ref.blob_trimap(h, w, seed=5)
    fields = ref.flow_fields(h, w, seed=7)
    flows = np.stack([fields[n] for n in ("zero", "shift", "zoom", "shift_int", "edge", "shift")])
    want = ref.chain(key, flows, 1)
    assert len({want[j].tobytes() for j in range(6)}) == 6
    tri = dev(key)
    for j in range(1, 6):
        tri = ops.trimap_propagate(tri, dev(flows[j]), 1)
        assert np.array_equal(tri.cpu().numpy(), want[j]), "step %d" % j


@pytest.mark.parametrize("grow", [0, 2])
def test_captured_call_replays_on_new_inputs(grow):
    from vmatting import ops
    h, w = 70, 90
    d_tri = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    d_flow = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
    d_out = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    work = torch.zeros(max(ops.trimap_propagate_workspace_bytes(h, w, grow), 1), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.trimap_propagate(d_tri, d_flow, grow, out=d_out, work=work)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.trimap_propagate(d_tri, d_flow, grow, out=d_out, work=work)
    for seed, tname, fname in ((1, "blob", "zoom"), (2, "noise", "random"), (3, "blob", "edge")):
        tri, fl = ref.TRIMAPS[tname](h, w, seed), ref.flow_fields(h, w, seed)[fname]
        d_tri.copy_(dev(tri))
        d_flow.copy_(dev(fl))
        g.replay()
        replayed = d_out.cpu().numpy()
        eager = ops.trimap_propagate(d_tri, d_flow, grow).cpu().numpy()
        assert np.array_equal(replayed, eager) and np.array_equal(eager, ref.propagate(tri, fl, grow))


def test_invalid_arguments_raise_with_the_librarys_text():
    from vmatting import ops
    tri = torch.zeros((8, 12), dtype=torch.uint8, device="cuda")
    fl = torch.zeros((8, 12, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match=r"trimap_propagate: trimap_propagate: grow 9 \(0\.\.8\)"):
        ops.trimap_propagate(tri, fl, grow=9)
    with pytest.raises(ValueError, match="trimap_propagate: trimap_propagate: out must not alias prev"):
        ops.trimap_propagate(tri, fl, out=tri)
    with pytest.raises(ValueError, match=r"flow must be \[h,w,2\]"):
        ops.trimap_propagate(tri, fl[:, :11].contiguous())
    with pytest.raises(ValueError):
        ops.trimap_propagate(tri, fl.permute(1, 0, 2))
    with pytest.raises(ValueError):
        ops.trimap_propagate(tri, fl, out=torch.zeros((8, 11), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ops.trimap_propagate(tri, fl, grow=2, work=torch.zeros(8, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- FrameStream(trimap="propagate")

H, W, F, CHUNK = 64, 96, 11, 4   # items of 4, 4 and 3 frames: two full chunks and a short, eager one
GROW = 1                         # (of the estimate test; the given-flow cases carry their own)


def items(cmp, bg, third, flows, chunk=CHUNK):
    """The clip in chunks; ``third``: item start -> key (propagate), or the per-frame trimaps [F,h,w] (trimap=True)."""
    for a in range(0, len(cmp), chunk):
        b = min(a + chunk, len(cmp))
        if isinstance(third, dict):
            yield cmp[a:b], bg[a:b], third.get(a), None if flows is None else flows[a:b]
        else:
            yield cmp[a:b], bg[a:b], third[a:b]


def chain_with_keys(keys, flows, grow):
    """ref.chain restarted at every key: keys maps a frame index to the trimap given for it."""
    starts = sorted(keys) + [len(flows)]
    return np.concatenate([ref.chain(keys[a], flows[a:b], grow) for a, b in zip(starts, starts[1:])])


@pytest.fixture(scope="module")
def clip(vgg0):
    """11 frames, their backward flows, two keys, the bf16 model and, per key placement, the restatement's trimaps with
    the mattes FrameStream(trimap=True) gives for them (computed once)."""
    from vmatting import FrameStream, unet
    rs = np.random.RandomState(21)
    cmp = rs.randint(0, 256, (F, H, W, 3)).astype(np.uint8)
    bg = rs.randint(0, 256, (F, H, W, 3)).astype(np.uint8)
    flows = np.stack([fer.shift_flow(H, W, 1.25 * (t % 3) - 1.5, 0.75 * (t % 4) - 1.0).astype(np.float32) +
                      rs.uniform(-0.5, 0.5, (H, W, 2)).astype(np.float32) for t in range(F)])
    flows[5] = fer.zoom_flow(H, W).astype(np.float32)
    flows[0] = np.nan  # entry 0 of a keyed item is unused
    key0, key8 = ref.blob_trimap(H, W, seed=1), ref.noise_trimap(H, W, seed=2)
    np.random.seed(0)
    model = unet.UNetVideo(vgg0, dtype="bf16", device="cuda").prepare()
    cases = {}
    # grow 0 (no class map): labels last through all 11 frames; grow 1: the band has eaten them after 8, where the
    # second key sits
    for name, keys, grow in (("one", {0: key0}, 0), ("two", {0: key0, 8: key8}, 1)):
        tris = chain_with_keys(keys, flows, grow)
        mattes = np.concatenate(list(FrameStream(model, H, W, chunk=CHUNK, out="u16").run(items(cmp, bg, tris, None))))
        assert len({mattes[t].tobytes() for t in range(F)}) == F
        cases[name] = (keys, tris, mattes, grow)
    tris = cases["one"][1]
    assert len({tris[t].tobytes() for t in range(F)}) == F and (tris[-1] == 255).any() and (tris[-1] == 0).any()
    tris = cases["two"][1]
    assert all((tris[t] == 255).any() and (tris[t] == 0).any() for t in (6, 10))  # (6: well into the continued chunk)
    return model, cmp, bg, flows, cases


@pytest.mark.parametrize("depth,graph", [(2, True), (1, True), (2, False), (1, False)])
@pytest.mark.parametrize("case", ["one", "two"])
def test_stream_given_flows_equals_per_frame_trimaps(clip, case, depth, graph):
    from vmatting import FrameStream
    model, cmp, bg, flows, cases = clip
    keys, tris, mattes, grow = cases[case]
    fs = FrameStream(model, H, W, chunk=CHUNK, depth=depth, trimap="propagate", flow="given", grow=grow, out="u16",
                     graph=graph)
    for _ in range(2):  # the object runs again with the same result: the chain restarts at the key
        got = list(fs.run(items(cmp, bg, keys, flows)))
        assert [g.shape for g in got] == [(4, H, W), (4, H, W), (3, H, W)]
        got = np.concatenate(got)
        for t in range(F):
            assert np.array_equal(got[t], mattes[t]), "frame %d" % t
        assert np.array_equal(fs.last_trimap(), tris[-1])
    assert fs.overflowed_chunks == []
    # one graph per slot for keyed and one for continued items; none without graph
    assert all(sorted(s.graphs) == ([False, True] if graph else []) for s in fs._slots) and len(fs._slots) == depth


def test_stream_estimated_flows_equal_given_estimates(clip):
    """flow="estimate" is flow="given" fed with ops.estimate_flow(cmp[t], cmp[t-1]): 6 frames of one texture under
    successive shifts (flow_est_ref.pair's frames, then further), in items of 4 and 2."""
    from vmatting import FrameStream, ops
    model = clip[0]
    n = 6
    tex = fer.texture(H, W, 7)
    cmp = np.stack([fer.render(tex, H, W, None if t == 0 else fer.shift_flow(H, W, 3.5 * t, -2.25 * t)) for t in range(n)])
    cur, prev, _ = fer.pair(H, W, "small")
    assert np.array_equal(cmp[1], cur) and np.array_equal(cmp[0], prev)
    bg = np.random.RandomState(5).randint(0, 256, (n, H, W, 3)).astype(np.uint8)
    key = {0: ref.blob_trimap(H, W, seed=4)}
    flows = np.zeros((n, H, W, 2), np.float32)
    for t in range(1, n):
        flows[t] = ops.estimate_flow(dev(cmp[t]), dev(cmp[t - 1])).cpu().numpy()
    given = FrameStream(model, H, W, chunk=CHUNK, trimap="propagate", flow="given", grow=GROW, out="u16")
    want = np.concatenate(list(given.run(items(cmp, bg, key, flows))))
    assert np.array_equal(given.last_trimap(), ref.chain(key[0], flows, GROW)[-1])
    assert (given.last_trimap() != 128).any()
    # chunk 4: a keyed graph and a short eager chunk; chunk 2: a keyed graph, then the continued graph of either slot
    for chunk, graph in ((4, True), (2, True), (4, False)):
        est = FrameStream(model, H, W, chunk=chunk, trimap="propagate", grow=GROW, out="u16", graph=graph)
        assert est.estimate
        got = np.concatenate(list(est.run(items(cmp, bg, key, None, chunk))))
        assert np.array_equal(got, want), (chunk, graph)
        assert np.array_equal(est.last_trimap(), given.last_trimap())


def test_a_failing_source_finishes_what_was_taken_and_the_object_runs_again(clip):
    from vmatting import FrameStream
    model, cmp, bg, flows, cases = clip
    keys, tris, mattes, grow = cases["one"]

    def failing():
        for i, item in enumerate(items(cmp, bg, keys, flows)):
            if i == 2:
                raise KeyError("decoder")
            yield item

    fs = FrameStream(model, H, W, chunk=CHUNK, depth=2, trimap="propagate", flow="given", grow=grow, out="u16")
    got = []
    with pytest.raises(KeyError, match="decoder"):
        for m in fs.run(failing()):
            got.append(m)
    assert len(got) == 2 and np.array_equal(np.concatenate(got), mattes[:8])
    assert np.array_equal(fs.last_trimap(), tris[7])
    # again, from a new key: the second key's chain from frame 8 on
    key8 = cases["two"][0][8]
    rest = np.concatenate(list(fs.run(items(cmp[8:], bg[8:], {0: key8}, flows[8:]))))
    tris8 = ref.chain(key8, flows[8:], grow)
    want = np.concatenate(list(FrameStream(model, H, W, chunk=CHUNK, out="u16").run(items(cmp[8:], bg[8:], tris8, None))))
    assert np.array_equal(rest, want) and np.array_equal(fs.last_trimap(), tris8[-1])
    # and an item without a key cannot start a run
    with pytest.raises(ValueError, match="first item"):
        list(fs.run(items(cmp[8:], bg[8:], {}, flows[8:])))
