"""Measures the plate estimate on the device and writes profiles/plate_estimate.json.

For n = 8, 16, 32, 64 samples of a 1080 x 1920 frame: vm_plate_from_samples by the method of stream_bench.py's auto
section (hipEvent medians over replays of a graph whose calls cycle through buffer sets that together exceed the
256 MB memory-side cache) against its bytes model, (3 n + 4) B per pixel, beside a large torch copy timed in the same
process; and the same definition in torch ops (torch.sort along the samples and indexing), asserted byte-equal before
it is timed.  Then PlateEstimator.add + result over a 256-frame host clip.

    python tools/plate_bench.py [--height 1080 --width 1920 --counts 8,16,32,64 --reps 9 --clip-frames 256]

The select that was not chosen, a bit-serial radix select, is in the study build only (`make study`):
    VM_LIB_PATH=video-matting_amd/study/libvmatting_study.so VM_PLATE_RADIX=1 python tools/plate_bench.py \
        --clip-frames 0 --out profiles/plate_radix.json

Each step runs under its own wall-clock limit (--step-limit seconds)."""

import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from stream_bench import HBM_PEAK, REPO, event_ms, graph_ms, rate, step  # noqa: E402  (it sets up the import path)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def torch_plate(samples):
    """include/vmatting.h's definition in torch ops."""
    n = samples.shape[0]
    lo, m = (n - 1) // 4, (n - 1) // 2
    s = torch.sort(samples, dim=0).values
    return s[m], (s[n - 1 - lo] - s[lo]).amax(-1)            # (s[hi] >= s[lo]: no wrap in uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--counts", default="8,16,32,64")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--clip-frames", type=int, default=256)
    ap.add_argument("--step-limit", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "plate_estimate.json"))
    a = ap.parse_args()
    from vmatting import PlateEstimator, ops
    h, w = a.height, a.width
    hw = h * w
    res = {"height": h, "width": w, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "hbm_peak_GBps": HBM_PEAK / 1e9, "kernels": {},
           # the study build holds the variant that lost (csrc/plate.hip radix_select), behind VM_PLATE_RADIX
           "library": "study" if os.environ.get("VM_LIB_PATH") else "shipped",
           "select": "radix" if os.environ.get("VM_LIB_PATH") and os.environ.get("VM_PLATE_RADIX") else "network"}
    g = torch.Generator(device="cuda")
    g.manual_seed(0)

    def kernel(n):
        bpp = 3 * n + 4
        # enough buffer sets that one round of calls streams more than the 256 MB memory-side cache
        nsets = max(2, int(300e6 / (bpp * hw)) + 1)
        samples = torch.randint(0, 256, (nsets, n, h, w, 3), generator=g, device="cuda", dtype=torch.uint8)
        plates = torch.empty((nsets, h, w, 3), dtype=torch.uint8, device="cuda")
        spreads = torch.empty((nsets, h, w), dtype=torch.uint8, device="cuda")
        call = lambda i: ops.plate_from_samples(samples[i], plate=plates[i], spread=spreads[i])  # noqa: E731
        want = torch_plate(samples[0])
        got = call(0)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), n   # the same bytes: the same work
        del want
        ms = graph_ms([lambda i=i: call(i) for i in range(nsets)], a.reps, calls=max(nsets, 40))
        per = dict(rate(bpp * hw, ms), us=round(ms * 1e3, 2), bytes_per_pixel=bpp, buffer_sets=nsets)
        ms_t = event_ms([lambda i=i: torch_plate(samples[i]) for i in range(nsets)], max(3, a.reps // 3), warmup=1)
        per["torch_route_ms"] = round(ms_t, 3)
        per["speedup_over_torch"] = round(ms_t / ms, 1)
        return per

    for n in (int(v) for v in a.counts.split(",")):
        res["kernels"]["n%d" % n] = step("kernel n=%d" % n, a.step_limit, lambda n=n: kernel(n))
        torch.cuda.empty_cache()

    def copy():
        # the HBM yardstick on this box: a torch copy of 265 MB (tools/membw.py's "copy")
        m = 1080 * 1920 * 64
        x, y = torch.empty(m, dtype=torch.bfloat16, device="cuda"), torch.empty(m, dtype=torch.bfloat16, device="cuda")
        return rate(4 * m, event_ms([lambda: y.copy_(x)], a.reps))
    res["torch_copy_265MB"] = step("copy", a.step_limit, copy)
    torch.cuda.empty_cache()

    def estimator():
        F = a.clip_frames
        k = 16  # distinct host frames, cycled in chunks of 8 (the estimator copies what it keeps)
        clip = np.random.RandomState(0).randint(0, 256, (k, h, w, 3)).astype(np.uint8)
        est = PlateEstimator(h, w)
        times = []
        for i in range(1 + max(3, a.reps // 3)):              # round 0 warms up
            est.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for t in range(0, F, 8):
                est.add(clip[t % k:t % k + min(8, F - t)])
            plate, spread = est.result()
            torch.cuda.synchronize()
            if i:
                times.append((time.perf_counter() - t0) * 1e3)
        ms = statistics.median(times)
        return {"frames": F, "kept": len(est.kept()), "stride": est.schedule.stride, "ms": round(ms, 2),
                "ms_per_frame": round(ms / F, 4), "min_ms": round(min(times), 2), "max_ms": round(max(times), 2)}
    if a.clip_frames > 0:
        res["estimator_host_clip"] = step("estimator", a.step_limit, estimator)

    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
