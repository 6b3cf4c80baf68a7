"""The plate estimate on the GPU: ops.plate_from_samples against the numpy restatement (tests/plate_ref.py), byte for
byte and with no tolerance anywhere; PlateEstimator against the restatement of exactly the frames its schedule keeps;
and FrameStream fed the estimated plate against the same stream fed the true one, bit for bit."""

import numpy as np
import pytest
import torch

import plate_ref as ref
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

# 70 x 90: 7 blocks of 1024 pixels, the last ragged; 7 x 11: 231 bytes a frame, so every frame after the first starts off
# a dword and the last dword is partial; 1 x 1: a frame smaller than a dword; 33 x 65: 3 blocks and 6435 = 4 k + 3 bytes
SHAPES = [(70, 90), (7, 11), (1, 1), (1, 17), (19, 1), (33, 65)]
COUNTS = [1, 2, 3, 4, 5, 8, 31, 32, 33, 63, 64]
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


@pytest.mark.parametrize("shape", SHAPES)
def test_equals_the_restatement(shape):
    from vmatting import ops
    h, w = shape
    for kind, make in ref.STACKS.items():
        full = make(64, h, w, seed=7)
        if kind in ("ascending", "descending", "lanes"):
            stacks = {n: make(n, h, w, seed=7) for n in COUNTS}   # ordered along their own n
        else:
            stacks = {n: full[:n] for n in COUNTS}
        for n in COUNTS:
            samples = stacks[n]
            d_samples = dev(samples)
            pbuf, plate = guarded(h * w * 3, 0xA5, lead=SENTINEL)
            sbuf, spread = guarded(h * w, 0x5A, lead=SENTINEL)
            got = ops.plate_from_samples(d_samples, plate=plate.view(h, w, 3), spread=spread.view(h, w))
            assert got[0].data_ptr() == plate.data_ptr() and got[1].data_ptr() == spread.data_ptr()
            want = ref.plate(samples)
            assert np.array_equal(got[0].cpu().numpy(), want[0]), (kind, n, "plate")
            assert np.array_equal(got[1].cpu().numpy(), want[1]), (kind, n, "spread")
            assert intact(pbuf, h * w * 3, 0xA5, SENTINEL) and intact(sbuf, h * w, 0x5A, SENTINEL), (kind, n)
            assert np.array_equal(d_samples.cpu().numpy(), samples), (kind, n)
            if n == 1:
                assert np.array_equal(want[0], samples[0]) and not want[1].any()


@pytest.mark.parametrize("shape,n", [((7, 11), 5), ((33, 65), 8), ((1, 1), 3)])
def test_buffers_at_any_byte_offset(shape, n):
    """samples, plate and spread each 0, 1 and 3 bytes into a larger buffer: the same bytes, nothing around the outputs
    touched, the samples as they were; without a spread the plate is the same."""
    from vmatting import ops
    h, w = shape
    samples = ref.noise(n, h, w, seed=3)
    want = ref.plate(samples)
    for lead_s in (0, 1, 3):
        _, s = guarded(samples.size, 0x11, lead=lead_s)
        s.copy_(dev(samples).view(-1))
        for lead_p in (0, 1, 3):
            for lead_r in (0, 1, 3):
                pbuf, plate = guarded(h * w * 3, 0xA5, lead=lead_p)
                sbuf, spread = guarded(h * w, 0x5A, lead=lead_r)
                assert (s.data_ptr() % 4, plate.data_ptr() % 4, spread.data_ptr() % 4) == (lead_s, lead_p, lead_r)
                got = ops.plate_from_samples(s.view(n, h, w, 3), plate=plate.view(h, w, 3), spread=spread.view(h, w))
                case = (lead_s, lead_p, lead_r)
                assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1]), case
                assert intact(pbuf, h * w * 3, 0xA5, lead_p) and intact(sbuf, h * w, 0x5A, lead_r), case
            pbuf, plate = guarded(h * w * 3, 0xA5, lead=lead_p)
            got = ops.plate_from_samples(s.view(n, h, w, 3), plate=plate.view(h, w, 3), want_spread=False)
            assert got[1] is None and np.array_equal(got[0].cpu().numpy(), want[0])
            assert intact(pbuf, h * w * 3, 0xA5, lead_p)
        assert np.array_equal(s.cpu().numpy(), samples.reshape(-1))
    got = ops.plate_from_samples(dev(samples))                # everything allocated
    assert got[0].shape == (h, w, 3) and got[1].shape == (h, w) and got[0].dtype == got[1].dtype == torch.uint8
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])


@pytest.mark.parametrize("n", [9, 64])
def test_recovers_a_plate_that_no_frame_shows(n):
    from vmatting import ops
    frames, bg, cover, parked = ref.recovery_clip(n)
    # (asserted on the input alone, before the GPU is touched)
    assert 1 <= cover.max() <= (n - 1) // 4 and (frames != bg).any(-1).any((1, 2)).all()
    plate, spread = ops.plate_from_samples(dev(frames))
    assert np.array_equal(plate.cpu().numpy(), bg) and not spread.cpu().numpy().any()
    # a disc parked for more than half the clip stays in the plate, and the spread shows where
    frames, bg, cover, parked = ref.recovery_clip(n, park=True)
    want = ref.plate(frames)
    y, x = np.nonzero(parked)
    rim = parked & ~(np.hypot(np.mgrid[:40, :56][1] - x.mean(), np.mgrid[:40, :56][0] - y.mean()) <= ref.RADIUS - 1.5)
    assert rim.sum() >= 16 and (want[0][parked] == np.array(ref.DARK, np.uint8)).all() and (want[1][rim] > 0).all()
    plate, spread = ops.plate_from_samples(dev(frames))
    assert np.array_equal(plate.cpu().numpy(), want[0]) and np.array_equal(spread.cpu().numpy(), want[1])
    assert (plate.cpu().numpy()[parked] == np.array(ref.DARK, np.uint8)).all()


def test_captured_call_replays_on_new_samples():
    from vmatting import ops
    n, h, w = 9, 33, 65
    d_samples = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    d_plate = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    d_spread = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.plate_from_samples(d_samples, plate=d_plate, spread=d_spread)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.plate_from_samples(d_samples, plate=d_plate, spread=d_spread)
    for seed, kind in ((1, "noise"), (2, "lanes")):
        samples = ref.STACKS[kind](n, h, w, seed)
        want = ref.plate(samples)
        d_samples.copy_(dev(samples))
        for _ in range(2):
            d_plate.zero_()
            d_spread.fill_(7)
            g.replay()
            assert np.array_equal(d_plate.cpu().numpy(), want[0]) and np.array_equal(d_spread.cpu().numpy(), want[1])


def test_invalid_arguments():
    from vmatting import _lib, ops
    lib = _lib.lib()
    n, h, w = 4, 5, 6
    s = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    plate = torch.full((h * w * 3 + h * w,), 9, dtype=torch.uint8, device="cuda")
    ok = dict(samples=s.data_ptr(), n=n, h=h, w=w, plate=plate.data_ptr(), spread=plate.data_ptr() + h * w * 3)
    order = ("samples", "n", "h", "w", "plate", "spread")
    assert lib.vm_plate_from_samples(*[ok[k] for k in order], None) == _lib.VM_OK      # spread right behind plate
    torch.cuda.synchronize()
    assert (plate == 0).all()
    plate.fill_(9)
    bad = [dict(samples=None), dict(plate=None), dict(n=0), dict(n=65), dict(h=0), dict(w=0),
           dict(plate=s.data_ptr() + 8), dict(spread=s.data_ptr()), dict(spread=plate.data_ptr() + h * w * 3 - 1)]
    for change in bad:
        args = dict(ok, **change)
        assert lib.vm_plate_from_samples(*[args[k] for k in order], None) == _lib.VM_EINVAL, change
    with pytest.raises(ValueError, match="plate_from_samples: plate_from_samples: plate and spread must not alias"):
        ops.plate_from_samples(s, plate=s.view(-1)[:h * w * 3].view(h, w, 3))
    torch.cuda.synchronize()
    assert (plate == 9).all()


# ---------------------------------------------------------------- PlateEstimator and reader.plate_from_clip

def test_estimator_uses_the_schedules_frames():
    """Frame t is the constant t, so the plate names the median frame kept and the spread the quantile frames."""
    from vmatting import PlateEstimator, reader
    from vmatting.plate import SampleSchedule
    frames, h, w = 200, 20, 30
    clip = np.repeat(np.arange(frames, dtype=np.uint8), h * w * 3).reshape(frames, h, w, 3)
    sched = SampleSchedule(8)
    for t in range(frames):
        sched.offer(t)
    kept = sched.kept()
    assert kept == list(range(0, 200, 32)) and len(kept) == 7
    want = ref.plate(clip[kept])
    assert (want[0] == kept[3]).all() and (want[1] == kept[5] - kept[1]).all()
    for to_input in (lambda a: a, dev):
        est = PlateEstimator(h, w, capacity=8)
        for a in range(0, frames, 7):                         # ragged: 28 chunks of 7 and one of 4
            assert est.add(to_input(clip[a:a + 7])) is est
        assert est.frames_seen == frames and est.kept() == kept
        plate, spread = est.result()
        assert plate.is_cuda and spread.is_cuda
        assert np.array_equal(plate.cpu().numpy(), want[0]) and np.array_equal(spread.cpu().numpy(), want[1])
        assert est.result(want_spread=False)[1] is None
        # a single frame per call, and a second clip after reset
        est.reset()
        assert est.frames_seen == 0 and est.kept() == []
        for t in range(5):
            est.add(to_input(clip[10 + t]))
        assert est.kept() == [0, 1, 2, 3, 4] and (est.result()[0].cpu().numpy() == 12).all()
    got = reader.plate_from_clip(clip, capacity=8)
    assert isinstance(got[0], np.ndarray) and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    got = reader.plate_from_clip(dev(clip), capacity=8)
    assert got[0].is_cuda and np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    # every = 3, capacity 64: frames 0, 3, .. 189 until the 65th, then every 6th
    got = reader.plate_from_clip(clip, every=3)
    sched = SampleSchedule(64, 3)
    for t in range(frames):
        sched.offer(t)
    assert sched.kept() == list(range(0, 200, 6))
    assert np.array_equal(got[0], ref.plate(clip[sched.kept()])[0])


def test_a_strided_device_clip_is_taken_as_it_is():
    """reader.plate_from_clip and PlateEstimator.add copy the frames they keep one by one, so a device clip of any
    strides is taken: every second frame, a window of every frame, and a clip stored [N,W,H,3] seen as [N,H,W,3] give
    the plates of their contiguous copies."""
    from vmatting import PlateEstimator, reader
    clip = dev(ref.noise(21, 12, 10))
    views = [clip[::2], clip[:, 1:11:2, 3:], clip.permute(0, 2, 1, 3)]
    for view in views:
        assert not view.is_contiguous()
        host = view.cpu().numpy()
        want = ref.plate(host[kept_frames(host.shape[0])])
        plate, spread = reader.plate_from_clip(view, capacity=8)
        assert plate.is_cuda and np.array_equal(plate.cpu().numpy(), want[0])
        assert np.array_equal(spread.cpu().numpy(), want[1])
        est = PlateEstimator(host.shape[1], host.shape[2], capacity=8)
        for a in range(0, host.shape[0], 4):
            est.add(view[a:a + 4])
        est.add(view[0])                                      # and one frame on its own, strided too in two of the views
        assert est.frames_seen == host.shape[0] + 1
        assert np.array_equal(est.result()[0].cpu().numpy(),
                              ref.plate(np.concatenate([host, host[:1]])[kept_frames(host.shape[0] + 1)])[0])


def kept_frames(frames, capacity=8):
    """The frames a capacity-8 schedule holds after ``frames`` frames."""
    from vmatting.plate import SampleSchedule
    sched = SampleSchedule(capacity)
    for t in range(frames):
        sched.offer(t)
    return sched.kept()


# ---------------------------------------------------------------- end to end: a clip with nothing but its own frames

def test_stream_over_the_estimated_plate(vgg0):
    from vmatting import FrameStream, PlateEstimator, unet
    H, W, F, CHUNK = 70, 90, 7, 3
    cmp, bg, cover, _ = ref.recovery_clip(F, H, W)
    assert 1 <= cover.max() <= (F - 1) // 2
    np.random.seed(0)
    model = unet.UNetVideo(vgg0, dtype="bf16", device="cuda").prepare()
    est = PlateEstimator(H, W)
    for a in range(0, F, CHUNK):
        est.add(cmp[a:a + CHUNK])                             # pass 1
    plate, spread = est.result()
    plate = plate.cpu().numpy()
    assert np.array_equal(plate, bg)

    def mattes(static):
        fs = FrameStream(model, H, W, chunk=CHUNK, static_bg=static, trimap="auto", out="u16")
        return np.concatenate(list(fs.run((cmp[a:a + CHUNK], None, None) for a in range(0, F, CHUNK))))

    got, want = mattes(plate), mattes(bg)
    assert got.shape == (F, H, W) and got.dtype == np.uint16 and np.array_equal(got, want)
    assert len({want[t].tobytes() for t in range(F)}) == F
