#!/usr/bin/env python
"""Times the guided matte upsampling at 2160 x 3840 and writes profiles/guided_upsample.json.

Kernels, per scale 2 and 4 at ``--chunk`` frames per call: ops.frames_reduce_u8 (both kinds), ops.guided_coeffs (the
defaults) and ops.guided_apply, each against the bytes its arithmetic requires (every input byte read once, every
output byte written once; the coefficients' unaveraged (a, b) written and read once), and beside it a device-to-device
``copy_`` that moves the same number of bytes (half read, half written), window by window in the one process.  Every
timed window runs the call on each of ``--sets`` buffer sets in turn, so consecutive calls stream more than the 256 MiB
Infinity Cache holds.  Times are hipEvent medians after a warm-up.

Streams: FrameStream(scale=2) at 2160 x 3840 beside the native scale=1 stream at 2160 x 3840 and the scale=1 stream at
1080 x 1920, same model (bf16 UNetVideo, synthetic weights), static plate, per-frame trimaps, out="u8", interleaved run
by run; a stream that does not fit or does not run is recorded as such.  The pinned upload of one UHD chunk, and the
host's own copies into and out of the pinned buffers, are timed on their own: their shares of the scale=2 stream's time
per frame say whether the link or the host bounds the stream.

Each step runs under its own wall-clock limit (--step-limit seconds)."""

import argparse
import json
import os
import signal
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "video-matting_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s


class StepTimeout(Exception):
    pass


def step(name, limit, fn):
    """Run one measurement under its own wall-clock limit."""
    def on_alarm(signum, frame):
        raise StepTimeout("step %r exceeded %d s" % (name, limit))
    signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(limit)
    t0 = time.time()
    try:
        return fn()
    finally:
        signal.alarm(0)
        print("# %-22s %.1f s" % (name, time.time() - t0), file=sys.stderr)


def window_ms(fns):
    """hipEvent time of one window: each of ``fns`` once, back to back, per call."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for fn in fns:
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / len(fns)


def pair_ms(calls, copies, reps, warmup=3):
    """Medians of the call and of the copy, their windows alternating."""
    for _ in range(warmup):
        window_ms(calls)
        window_ms(copies)
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(reps):
        a.append(window_ms(calls))
        b.append(window_ms(copies))
    return statistics.median(a), statistics.median(b), min(a), max(a)


def kernel_bytes(n, h, w, s):
    """The bytes each call's arithmetic requires, from the shapes."""
    hm, wm = -(-h // s), -(-w // s)
    hi, lo = n * h * w, n * hm * wm
    return {"reduce_mean": 3 * hi + 3 * lo, "reduce_trimap": hi + lo,
            "coeffs": lo * (3 + 4) + lo * 16 * 3,   # guide + matte in; (a, b) out, in again, ab out
            "apply": hi * (3 + 4) + lo * 16}


def kernels(a):
    from vmatting import ops
    n, h, w = a.chunk, a.height, a.width
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    rnd = lambda *shape: torch.randint(0, 256, shape, generator=g, device="cuda", dtype=torch.uint8)  # noqa: E731
    cmp = [rnd(n, h, w, 3) for _ in range(a.sets)]
    tri = [torch.where(rnd(n, h // 16 + 1, w // 16 + 1) < 128, 0, 255).to(torch.uint8).repeat_interleave(16, 1)
           .repeat_interleave(16, 2)[:, :h, :w].contiguous() for _ in range(a.sets)]
    alpha = [torch.empty((n, h, w, 1), dtype=torch.float32, device="cuda") for _ in range(a.sets)]
    res = {}
    for s in a.scales:
        hm, wm = ops.reduced_size(h, w, s)
        nb = kernel_bytes(n, h, w, s)
        lo = [ops.frames_reduce_u8(c, s) for c in cmp]
        tlo = [torch.empty((n, hm, wm), dtype=torch.uint8, device="cuda") for _ in range(a.sets)]
        p = [torch.rand((n, hm, wm, 1), generator=g, device="cuda") for _ in range(a.sets)]
        ab = [ops.guided_coeffs(lo[i], p[i]) for i in range(a.sets)]
        work = torch.empty(ops.guided_workspace_bytes(n, hm, wm), dtype=torch.uint8, device="cuda")
        calls = {
            "reduce_mean": [lambda i=i: ops.frames_reduce_u8(cmp[i], s, out=lo[i]) for i in range(a.sets)],
            "reduce_trimap": [lambda i=i: ops.frames_reduce_u8(tri[i], s, "trimap", out=tlo[i]) for i in range(a.sets)],
            "coeffs": [lambda i=i: ops.guided_coeffs(lo[i], p[i], out=ab[i], work=work) for i in range(a.sets)],
            "apply": [lambda i=i: ops.guided_apply(ab[i], cmp[i], s, out=alpha[i]) for i in range(a.sets)],
        }
        per = {"reduced": [hm, wm]}
        for name, fns in calls.items():
            half = nb[name] // 2
            src = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(a.sets)]
            dst = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(a.sets)]
            copies = [lambda i=i: dst[i].copy_(src[i]) for i in range(a.sets)]
            ms, ms_copy, lo_ms, hi_ms = pair_ms(fns, copies, a.reps)
            per[name] = {"bytes": nb[name], "ms": round(ms, 4), "min_ms": round(lo_ms, 4), "max_ms": round(hi_ms, 4),
                         "GBps": round(nb[name] / ms / 1e6, 1), "hbm_frac": round(nb[name] / (ms * 1e-3) / HBM_PEAK, 3),
                         "copy_same_bytes_ms": round(ms_copy, 4), "copy_GBps": round(2 * half / ms_copy / 1e6, 1),
                         "over_copy": round(ms / ms_copy, 2)}
            print("# s=%d %-14s %.4f ms, %.0f GB/s; copy of the same bytes %.4f ms; x%.2f" %
                  (s, name, ms, per[name]["GBps"], ms_copy, ms / ms_copy), file=sys.stderr)
            del src, dst, copies
        res["scale%d" % s] = per
        del lo, tlo, p, ab, work, calls
        torch.cuda.empty_cache()
    return res


def streams(a):
    from vmatting import FrameStream, unet
    from vmatting.weights import synthetic_vgg16
    n, F = a.chunk, a.frames
    np.random.seed(0)
    model = unet.UNetVideo(synthetic_vgg16(0), dtype="bf16", device="cuda").prepare()
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    k = min(F, 2 * n)  # two distinct chunks of host frames, cycled

    def clip(h, w):
        cmp = torch.randint(0, 256, (k, h, w, 3), generator=g, device="cuda", dtype=torch.uint8).cpu().numpy()
        tri = np.full((k, h, w), 128, np.uint8)
        tri[:, :h // 4] = 0
        tri[:, h // 2:3 * h // 4, w // 4:w // 2] = 255
        return cmp, tri, cmp[0].copy()

    sizes = {"uhd": (a.height, a.width), "hd": (a.height // 2, a.width // 2)}
    clips = {name: clip(*hw) for name, hw in sizes.items()}
    torch.cuda.empty_cache()
    plan = {"uhd_scale2": ("uhd", 2), "uhd_native": ("uhd", 1), "hd_native": ("hd", 1)}
    out, made = {}, {}
    for name, (size, s) in plan.items():
        h, w = sizes[size]
        try:
            made[name] = FrameStream(model, h, w, chunk=n, depth=2, out="u8", static_bg=clips[size][2], scale=s)
        except Exception as e:  # recorded, not a failure of the measurement
            out[name] = {"error": "%s: %s" % (type(e).__name__, e)}

    def run(name):
        cmp, tri, _ = clips[plan[name][0]]
        src = ((cmp[i % k:i % k + min(n, F - i)], None, tri[i % k:i % k + min(n, F - i)]) for i in range(0, F, n))
        t0 = time.perf_counter()
        tot = sum(m.shape[0] for m in made[name].run(src))
        torch.cuda.synchronize()
        assert tot == F
        return (time.perf_counter() - t0) * 1e3

    times = {name: [] for name in made}
    for i in range(1 + a.rounds):  # interleaved; round 0 warms up (and captures the graphs)
        for name in list(times):
            try:
                ms = run(name)
            except (RuntimeError, MemoryError) as e:  # does not fit, or does not run: recorded
                out[name] = {"error": "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200])}
                del times[name], made[name]
                torch.cuda.empty_cache()
                continue
            if i:
                times[name].append(ms)
    for name, t in times.items():
        ms = statistics.median(t)
        out[name] = {"size": list(sizes[plan[name][0]]), "scale": plan[name][1], "ms_per_frame": round(ms / F, 3),
                     "frames_per_s": round(F / ms * 1e3, 1), "min_ms_per_frame": round(min(t) / F, 3),
                     "max_ms_per_frame": round(max(t) / F, 3)}
    # the upload of one UHD chunk (frames and trimaps), pinned -> device, on its own
    h, w = sizes["uhd"]
    pin = [torch.zeros((n, h, w, 3), dtype=torch.uint8).pin_memory(), torch.zeros((n, h, w), dtype=torch.uint8).pin_memory()]
    dst = [torch.empty_like(t, device="cuda") for t in pin]
    ups = [lambda: [d.copy_(s, non_blocking=True) for d, s in zip(dst, pin)]]
    for _ in range(2):
        window_ms(ups)
    up = statistics.median(window_ms(ups) for _ in range(a.reps))
    nbytes = sum(t.numel() for t in pin)
    out["uhd_upload"] = {"bytes_per_frame": nbytes // n, "ms_per_frame": round(up / n, 3),
                         "GBps": round(nbytes / up / 1e6, 1)}
    # the host's own copies per UHD chunk, as the stream makes them on its one thread: the source's arrays into the
    # pinned buffers, and the pinned result into the array it yields
    cmp, tri, _ = clips["uhd"]
    res = torch.zeros((n, h, w), dtype=torch.uint8).pin_memory()
    host = []
    for _ in range(1 + a.rounds):
        t0 = time.perf_counter()
        pin[0].numpy()[...] = cmp[:n]
        pin[1].numpy()[...] = tri[:n]
        res.numpy().copy()
        host.append((time.perf_counter() - t0) * 1e3)
    hc = statistics.median(host[1:])
    out["uhd_host_copies"] = {"bytes_per_frame": nbytes // n + h * w, "ms_per_frame": round(hc / n, 3),
                              "GBps": round((nbytes + n * h * w) / hc / 1e6, 1)}
    if "ms_per_frame" in out.get("uhd_scale2", {}):
        out["uhd_upload"]["share_of_uhd_scale2"] = round(up / n / out["uhd_scale2"]["ms_per_frame"], 3)
        out["uhd_host_copies"]["share_of_uhd_scale2"] = round(hc / n / out["uhd_scale2"]["ms_per_frame"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--frames", type=int, default=32, help="frames per stream run")
    ap.add_argument("--scales", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--sets", type=int, default=2, help="buffer sets taken in turn (2 x 199 MB of frames at UHD)")
    ap.add_argument("--reps", type=int, default=10, help="timed windows per kernel")
    ap.add_argument("--rounds", type=int, default=3, help="timed runs per stream")
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--skip-streams", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "guided_upsample.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("upscale_bench: needs a ROCm GPU (no figure is produced without one)")
    from vmatting import ops
    doc = {"device": torch.cuda.get_device_name(0),
           "measured_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "shape": [a.chunk, a.height, a.width],
           "sets": a.sets, "reps": a.reps, "hbm_peak_GBps": HBM_PEAK / 1e9, "timing": "hipEvent median per call",
           "defaults": dict(ops.GUIDED_DEFAULTS), "model": "UNetVideo bf16, synthetic weights"}
    doc["kernels"] = step("kernels", a.step_limit, lambda: kernels(a))
    torch.cuda.empty_cache()
    if not a.skip_streams:
        doc["streams"] = step("streams", a.step_limit, lambda: streams(a))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"guided_upsample": {"kernels": {s: {k: v["over_copy"] for k, v in per.items() if k != "reduced"}
                                                      for s, per in doc["kernels"].items()},
                                          "streams": {k: v.get("frames_per_s", v.get("error", v.get("ms_per_frame")))
                                                      for k, v in doc.get("streams", {}).items()}}}))


if __name__ == "__main__":
    main()
