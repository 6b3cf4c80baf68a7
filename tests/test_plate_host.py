"""CPU checks of the plate estimate: the numpy restatement (tests/plate_ref.py) against the definition read byte by
byte, the two coverage facts the GPU tests lean on, the sampling schedule, and the host-side argument checks of the C
entry and the wrappers, which all happen before any GPU call."""

import numpy as np
import pytest
import torch

import plate_ref as ref


def brute(samples):
    """include/vmatting.h's definition, one byte position at a time."""
    n, h, w, _ = samples.shape
    lo, m, hi = (n - 1) // 4, (n - 1) // 2, n - 1 - (n - 1) // 4
    plate, spread = np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            for c in range(3):
                s = sorted(int(v) for v in samples[:, y, x, c])
                plate[y, x, c] = s[m]
                spread[y, x] = max(spread[y, x], s[hi] - s[lo])
    return plate, spread


@pytest.mark.parametrize("n", list(range(1, 10)) + [64])
def test_restatement_equals_the_definition(n):
    assert ref.ranks(n) == ((n - 1) // 4, (n - 1) // 2, n - 1 - (n - 1) // 4)
    for name, make in ref.STACKS.items():
        samples = make(n, 5, 7, seed=n)
        plate, spread = ref.plate(samples)
        want = brute(samples)
        assert plate.dtype == np.uint8 and spread.dtype == np.uint8 and spread.shape == (5, 7)
        assert np.array_equal(plate, want[0]) and np.array_equal(spread, want[1]), name
        assert np.array_equal(plate, torch.from_numpy(samples).median(dim=0).values.numpy()), name
    one = ref.noise(1, 5, 7)
    assert np.array_equal(ref.plate(one)[0], one[0]) and not ref.plate(one)[1].any()


def test_inputs_are_what_they_claim():
    a = ref.ascending(9, 5, 7)
    assert (np.diff(a.astype(int), axis=0) >= 0).all() and (np.diff(ref.descending(9, 5, 7).astype(int), axis=0) <= 0).all()
    assert set(np.unique(ref.binary(9, 5, 7)).tolist()) == {0, 255}
    assert (ref.constant(9, 5, 7) == ref.constant(9, 5, 7)[0]).all()
    flat, base = ref.lanes(9, 5, 7).reshape(9, -1), a.reshape(9, -1)
    for k in range(4):
        assert np.array_equal(flat[:, k::4], np.roll(base[:, k::4], k, 0))
    assert np.array_equal(np.sort(flat, 0), base)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9, 33, 64])
def test_coverage_facts(n):
    """Covered in at most (n - 1) // 2 samples by anything at all, a pixel that shows one value in the others keeps it;
    covered in at most (n - 1) // 4, its spread is 0 too.  One more covering sample of an extreme value breaks each."""
    rs = np.random.RandomState(n)
    h, w = 6, 8
    bg = ref.true_plate(h, w)
    half, quarter = (n - 1) // 2, (n - 1) // 4
    for cover, flat in ((half, False), (quarter, True)):
        samples = np.repeat(bg[None], n, 0)
        for y in range(h):
            for x in range(w):
                which = rs.permutation(n)[:rs.randint(0, cover + 1)]
                samples[which, y, x] = rs.randint(0, 256, (len(which), 3))
        plate, spread = ref.plate(samples)
        assert np.array_equal(plate, bg)
        assert not flat or not spread.any()
    samples = np.repeat(bg[None], n, 0)
    samples[:half + 1, 2, 3] = 0                             # (the plate has no 0)
    samples[:quarter + 1, 4, 5] = 0
    plate, spread = ref.plate(samples)
    assert (plate[2, 3] == 0).all() and (spread[4, 5] > 0) == (n > 1)


@pytest.mark.parametrize("n,h,w", [(9, 40, 56), (64, 40, 56), (7, 70, 90)])
def test_recovery_clip_is_what_it_claims(n, h, w):
    frames, bg, cover, parked = ref.recovery_clip(n, h, w)
    assert frames.shape == (n, h, w, 3) and 1 <= cover.max() <= (n - 1) // 4 and not parked.any()
    assert (frames == np.array(ref.BRIGHT, np.uint8)).all(-1).any() and (frames == np.array(ref.DARK, np.uint8)).all(-1).any()
    plate, spread = ref.plate(frames)
    assert np.array_equal(plate, bg) and not spread.any()
    if n < 9:
        return                                               # (parking takes (n - 1) // 2 + 2 frames)
    frames, bg, cover, parked = ref.recovery_clip(n, h, w, park=True)
    plate, spread = ref.plate(frames)
    assert parked.sum() > 40 and (cover[parked] > n // 2).all()
    assert (plate[parked] == np.array(ref.DARK, np.uint8)).all() and np.array_equal(plate[~parked], bg[~parked])
    assert (spread[parked] > 0).all()


# ---------------------------------------------------------------- the sampling schedule

@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("capacity", [2, 4, 8, 64])
def test_sample_schedule(capacity, every):
    from vmatting.plate import SampleSchedule
    sched = SampleSchedule(capacity, every)
    assert sched.kept() == [] and sched.n == 0 and sched.stride == every
    slots = np.full(capacity, -1)
    strides = set()
    for t in range(5 * capacity * every):
        slot, moves = sched.offer(t)
        written = []
        for j, (src, dst) in enumerate(moves):
            assert (src, dst) == (2 * (j + 1), j + 1) and all(src > d for d in written + [dst])
            slots[dst] = slots[src]
            written.append(dst)
        assert not moves or (len(moves) == capacity // 2 - 1 and slot == capacity // 2)
        if slot is not None:
            assert t % sched.stride == 0 and slot == sched.n - 1
            slots[slot] = t
        else:
            assert t % sched.stride != 0 and moves == []
        # the clip so far has t + 1 frames
        assert 1 <= sched.n <= capacity and sched.frames_seen == t + 1
        assert sched.kept() == list(range(0, t + 1, sched.stride)) == slots[:sched.n].tolist()
        assert sched.n >= min(capacity // 2, t // every + 1)
        strides.add(sched.stride)
    assert strides == {every, 2 * every, 4 * every, 8 * every}
    # a deterministic function of (capacity, every, frames seen); reset starts over
    again = SampleSchedule(capacity, every)
    for t in range(5 * capacity * every):
        again.offer(t)
    assert again.kept() == sched.kept()
    sched.reset()
    assert sched.kept() == [] and sched.offer(0) == (0, [])


def test_sample_schedule_arguments():
    from vmatting.plate import SampleSchedule
    for capacity in (0, 1, 3, 63, 65, 66, -2):
        with pytest.raises(ValueError):
            SampleSchedule(capacity)
    for capacity in (2.0, "8", None, True):
        with pytest.raises(TypeError):
            SampleSchedule(capacity)
    for every in (0, -1):
        with pytest.raises(ValueError):
            SampleSchedule(8, every)
    with pytest.raises(TypeError):
        SampleSchedule(8, 1.5)
    sched = SampleSchedule(8)
    sched.offer(0)
    with pytest.raises(ValueError):
        sched.offer(2)                                       # the running index, no gaps
    assert SampleSchedule().capacity == 64 and SampleSchedule(np.int64(4), np.int32(2)).every == 2


# ---------------------------------------------------------------- the C entry point and the wrappers, on the host

def test_c_entry_rejects_bad_arguments():
    from vmatting import _lib
    lib = _lib.lib()
    P, Q, S = 4096, 16384, 32768  # non-null addresses: validation never dereferences them
    ok = dict(samples=P, n=4, h=5, w=5, plate=Q, spread=S)   # 300 sample bytes, 75 plate bytes, 25 spread bytes
    bad = [dict(samples=None), dict(plate=None),
           dict(n=0), dict(n=-1), dict(n=65), dict(h=0), dict(w=0), dict(h=-1), dict(w=-3),
           dict(n=64, h=1 << 12, w=1 << 12), dict(n=1, h=1, w=715827883), dict(n=2, h=1 << 15, w=10923),   # > 2^31 - 1 bytes
           dict(plate=P), dict(plate=P + 299), dict(plate=P - 74), dict(plate=P + 100, spread=None),
           dict(spread=P), dict(spread=P + 299), dict(spread=P - 24),
           dict(spread=Q), dict(spread=Q + 74), dict(spread=Q - 24)]
    order = ("samples", "n", "h", "w", "plate", "spread")
    for change in bad:
        args = dict(ok, **change)
        rc = lib.vm_plate_from_samples(*[args[k] for k in order], None)
        assert rc == _lib.VM_EINVAL, change
        assert b"plate_from_samples" in lib.vm_last_error()
    assert lib.vm_abi_version() == 1


def test_wrappers_check_on_the_host():
    from vmatting import PlateEstimator, ops, reader
    s = torch.zeros((4, 5, 6, 3), dtype=torch.uint8)
    assert ops.PLATE_MAX_SAMPLES == ref.MAX_SAMPLES == 64
    with pytest.raises(TypeError):
        ops.plate_from_samples(s)                            # the right tensor, but on the host
    with pytest.raises(TypeError):
        ops.plate_from_samples(s.float())
    with pytest.raises(TypeError):
        ops.plate_from_samples(s.numpy())
    with pytest.raises(TypeError):
        ops.plate_from_samples(s, plate=np.zeros((5, 6, 3), np.uint8))
    with pytest.raises(TypeError):
        ops.plate_from_samples(s, spread=torch.zeros((5, 6)))
    for bad in (s[0], s[..., :2], s[:0], torch.zeros((65, 2, 2, 3), dtype=torch.uint8), s.permute(0, 2, 1, 3)):
        with pytest.raises(ValueError):
            ops.plate_from_samples(bad)
    with pytest.raises(ValueError):
        ops.plate_from_samples(s, plate=torch.zeros((5, 6), dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.plate_from_samples(s, spread=torch.zeros((5, 6, 3), dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.plate_from_samples(s, spread=torch.zeros((5, 6), dtype=torch.uint8), want_spread=False)

    clip = s.numpy()
    for bad in (clip.astype(np.int8), clip.astype(np.float32), clip.tolist()):
        with pytest.raises(TypeError):
            reader.plate_from_clip(bad)
    for bad in (clip[0], clip[..., :2], clip[:0]):
        with pytest.raises(ValueError):
            reader.plate_from_clip(bad)
    for kw in (dict(capacity=3), dict(capacity=66), dict(capacity=0), dict(every=0)):
        with pytest.raises(ValueError):
            reader.plate_from_clip(clip, **kw)
    with pytest.raises(TypeError):
        reader.plate_from_clip(clip, capacity=8.0)

    for args in ((0, 6), (5, 0), (5, 6, 7), (5, 6, 128), (5, 6, 8, 0)):
        with pytest.raises(ValueError):
            PlateEstimator(*args)
    for args in ((5.0, 6), (5, "6"), (5, 6, 8.0), (5, 6, 8, None)):
        with pytest.raises(TypeError):
            PlateEstimator(*args)
    est = PlateEstimator(5, 6, capacity=8, every=2)
    assert est.frames_seen == 0 and est.kept() == []
    with pytest.raises(ValueError, match="no frame"):
        est.result()
    for bad in (clip.astype(np.float32), s, s[0], clip.tolist(), None):   # (s: a torch tensor on the host)
        with pytest.raises(TypeError):
            est.add(bad)
    wide = torch.zeros((4, 5, 12, 3), dtype=torch.uint8)[:, :, ::2]       # strided, and on the host: the device is the fault
    assert not wide.is_contiguous() and wide.shape == s.shape
    with pytest.raises(TypeError):
        est.add(wide)
    with pytest.raises(TypeError):
        reader.plate_from_clip(wide)
    for bad in (clip[:, :4], clip[..., :2], clip[0, 0], clip[None]):
        with pytest.raises(ValueError):
            est.add(bad)
    assert est.frames_seen == 0 and est._buf is None         # rejected before anything was allocated
