#!/usr/bin/env python
"""Times the plate's exposure match at 1080 x 1920 and writes profiles/plate_gain.json.

Kernels, at ``--chunk`` frames per call: ops.plate_gain_fit (per-frame backgrounds, so that every byte it needs comes
from memory) on three inputs - uniform noise (the bins spread), a frame at 3/4 of a noise plate (two or three bins, what
a real frame looks like to the histogram) and a constant frame over a constant plate (every pixel in one bin, the worst
case for the same-address LDS atomics) - and ops.plate_gain_apply with per-frame backgrounds and with one static plate.
Each against the bytes its arithmetic requires (every input byte read once, every output byte written once), and beside
it a device-to-device ``copy_`` that moves the same number of bytes (half read, half written), window by window in the
one process.  Every timed window runs the call on each of ``--sets`` buffer sets in turn, so consecutive calls stream
more than the 256 MiB Infinity Cache holds.  Times are hipEvent medians after a warm-up.

Streams: bf16 UNetVideo (synthetic weights), chunk 8, depth 2, out="u8", interleaved run by run: the static plate
without a gain, per-frame uploaded backgrounds, and the static plate with gain="fit".  The gained stream does the
per-frame-background stream's device work plus the two new calls and uploads one frame's worth of background less per
frame, so its time per frame is to be read against that stream's plus the kernel times above.

Each step runs under its own wall-clock limit (--step-limit seconds)."""

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "video-matting_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from upscale_bench import HBM_PEAK, pair_ms, step  # noqa: E402  (the windows and the step limit of the §3.4k table)


def kernels(a):
    from vmatting import ops
    n, h, w = a.chunk, a.height, a.width
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    rnd = lambda lo, hi: torch.randint(lo, hi, (n, h, w, 3), generator=g, device="cuda", dtype=torch.uint8)  # noqa: E731
    pixels = n * h * w
    inputs = {}
    inputs["noise"] = [(rnd(0, 256), rnd(0, 256)) for _ in range(a.sets)]
    plates = [rnd(16, 251) for _ in range(a.sets)]
    inputs["ratio_3_4"] = [((p.to(torch.int32) * 3 >> 2).to(torch.uint8), p) for p in plates]
    inputs["one_bin"] = [(torch.full((n, h, w, 3), 150, dtype=torch.uint8, device="cuda"),
                          torch.full((n, h, w, 3), 200, dtype=torch.uint8, device="cuda")) for _ in range(a.sets)]
    gain = [torch.zeros((n, 3), dtype=torch.int32, device="cuda") for _ in range(a.sets)]
    sup = [torch.zeros((n, 3), dtype=torch.int32, device="cuda") for _ in range(a.sets)]
    work = torch.zeros(ops.plate_gain_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    out = [torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(a.sets)]
    half = 3 * pixels  # fit: 6 B per pixel read; apply: 3 read, 3 written
    src = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(a.sets)]
    dst = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(a.sets)]
    copies = [lambda i=i: dst[i].copy_(src[i]) for i in range(a.sets)]
    calls = {"fit_" + name: [lambda i=i, s=sets: ops.plate_gain_fit(s[i][0], s[i][1], out=gain[i], support=sup[i],
                                                                    work=work) for i in range(a.sets)]
             for name, sets in inputs.items()}
    fitted = torch.tensor([[3277, 4096, 5120]] * n, dtype=torch.int32, device="cuda")
    calls["apply_per_frame"] = [lambda i=i: ops.plate_gain_apply(plates[i], fitted, out=out[i]) for i in range(a.sets)]
    calls["apply_static"] = [lambda i=i: ops.plate_gain_apply(plates[i][0], fitted, out=out[i]) for i in range(a.sets)]
    res = {}
    for name, fns in calls.items():
        nbytes = 6 * pixels if name != "apply_static" else 3 * pixels + 3 * h * w
        ms, ms_copy, lo_ms, hi_ms = pair_ms(fns, copies, a.reps)
        res[name] = {"bytes": nbytes, "ms": round(ms, 4), "min_ms": round(lo_ms, 4), "max_ms": round(hi_ms, 4),
                     "GBps": round(nbytes / ms / 1e6, 1), "hbm_frac": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3),
                     "copy_6B_per_pixel_ms": round(ms_copy, 4), "copy_GBps": round(2 * half / ms_copy / 1e6, 1),
                     "over_copy": round(ms / ms_copy, 2)}
        print("# %-16s %.4f ms, %.0f GB/s; copy of 6 B per pixel %.4f ms; x%.2f" %
              (name, ms, res[name]["GBps"], ms_copy, ms / ms_copy), file=sys.stderr)
    res["fit_one_bin_over_noise"] = round(res["fit_one_bin"]["ms"] / res["fit_noise"]["ms"], 2)
    res["fit_ratio_3_4_over_noise"] = round(res["fit_ratio_3_4"]["ms"] / res["fit_noise"]["ms"], 2)
    # what the fits make of the inputs, as a check that the timed calls ran on what they were meant to
    res["fits_seen"] = {}
    for name, sets in inputs.items():
        ops.plate_gain_fit(*sets[0], out=gain[0], support=sup[0], work=work)
        res["fits_seen"][name] = {"gain": gain[0][0].tolist(),
                                  "support_share": [round(v / (h * w), 3) for v in sup[0][0].tolist()]}
    return res


def streams(a):
    from vmatting import FrameStream, unet
    from vmatting.weights import synthetic_vgg16
    n, F, h, w = a.chunk, a.frames, a.height, a.width
    np.random.seed(0)
    model = unet.UNetVideo(synthetic_vgg16(0), dtype="bf16", device="cuda").prepare()
    rs = np.random.RandomState(1)
    k = min(F, 2 * n)  # two distinct chunks of host frames, cycled
    yy, xx = np.mgrid[0:h, 0:w]
    plate = np.stack([120 + 60 * np.sin(xx / 90.0 + c) + 40 * np.cos(yy / 70.0 + 2 * c) for c in range(3)], -1)
    plate = np.clip(np.rint(plate), 0, 255).astype(np.uint8)
    cmp = np.repeat(plate[None], k, 0)
    y0, y1, x0, x1 = h // 4, 3 * h // 4, w // 3, 2 * w // 3
    cmp[:, y0:y1, x0:x1] = rs.randint(0, 256, (k, y1 - y0, x1 - x0, 3))  # the subject: a sixth of the frame
    cmp = np.clip(np.rint(cmp * rs.uniform(0.75, 1.25, (k, 1, 1, 3))), 0, 255).astype(np.uint8)
    bg = np.repeat(plate[None], k, 0)
    tri = np.full((k, h, w), 128, np.uint8)
    tri[:, :h // 8] = 0
    tri[:, 3 * h // 8:5 * h // 8, 5 * w // 12:7 * w // 12] = 255
    plan = {"static_plate": dict(static_bg=plate), "per_frame_bg": dict(),
            "static_plate_gain_fit": dict(static_bg=plate, gain="fit")}
    made = {name: FrameStream(model, h, w, chunk=n, depth=2, out="u8", **kw) for name, kw in plan.items()}

    def run(name):
        static = "static_bg" in plan[name]
        src = ((cmp[i % k:i % k + min(n, F - i)], None if static else bg[i % k:i % k + min(n, F - i)],
                tri[i % k:i % k + min(n, F - i)]) for i in range(0, F, n))
        t0 = time.perf_counter()
        tot = sum(m.shape[0] for m in made[name].run(src))
        torch.cuda.synchronize()
        assert tot == F
        return (time.perf_counter() - t0) * 1e3

    times = {name: [] for name in made}
    for i in range(1 + a.rounds):  # interleaved; round 0 warms up (and captures the graphs)
        for name in times:
            ms = run(name)
            if i:
                times[name].append(ms)
    out = {}
    for name, t in times.items():
        ms = statistics.median(t)
        out[name] = {"ms_per_frame": round(ms / F, 3), "frames_per_s": round(F / ms * 1e3, 1),
                     "min_ms_per_frame": round(min(t) / F, 3), "max_ms_per_frame": round(max(t) / F, 3)}
    gains, support = made["static_plate_gain_fit"].last_gains()
    out["last_gains"] = {"gains": np.round(gains.astype(np.float64), 4).tolist(),
                         "support_share": np.round(support / (h * w), 3).tolist()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--frames", type=int, default=32, help="frames per stream run")
    ap.add_argument("--sets", type=int, default=4, help="buffer sets taken in turn (4 x 100 MB of frames at 1080p)")
    ap.add_argument("--reps", type=int, default=10, help="timed windows per kernel")
    ap.add_argument("--rounds", type=int, default=3, help="timed runs per stream")
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--skip-streams", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "plate_gain.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gain_bench: needs a ROCm GPU (no figure is produced without one)")
    from vmatting import ops
    doc = {"device": torch.cuda.get_device_name(0),
           "measured_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "shape": [a.chunk, a.height, a.width],
           "sets": a.sets, "reps": a.reps, "hbm_peak_GBps": HBM_PEAK / 1e9, "timing": "hipEvent median per call",
           "defaults": dict(ops.GAIN_DEFAULTS), "model": "UNetVideo bf16, synthetic weights"}
    doc["kernels"] = step("kernels", a.step_limit, lambda: kernels(a))
    torch.cuda.empty_cache()
    if not a.skip_streams:
        doc["streams"] = step("streams", a.step_limit, lambda: streams(a))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"plate_gain": {"kernels": {k: (v["over_copy"] if isinstance(v, dict) and "over_copy" in v else v)
                                                 for k, v in doc["kernels"].items()},
                                     "streams": {k: v.get("ms_per_frame", v) for k, v in doc.get("streams", {}).items()}}}))


if __name__ == "__main__":
    main()
