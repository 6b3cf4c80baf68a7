#!/usr/bin/env python
"""Measure the flow-compensated temporal matte filter and write profiles/matte_smooth.json (one JSON line, printed too).

    python tools/smooth_bench.py [--frames 64] [--chunk 8] [--reps 9] [--sizes 1080x1920,2160x3840]

(a) ``kernel``: vm_matte_smooth alone at every size of ``--sizes``, one frame with a predecessor per call, with and
    without the ``weight`` output: microseconds per frame and GB/s against its bytes model (flow 8 + alpha 4 + out 4 +
    frame 3 bytes per pixel, + 4 with weight; the four-tap gathers of the previous matte and frame are not counted),
    beside a device-to-device copy of the same number of bytes, their windows alternating.  The calls are captured in a
    HIP graph (the host could not launch them back to back) that cycles through enough buffer sets to stream more than
    the 256 MiB memory-side cache.  The flows are smooth (a zoom plus a shift) with a little noise, as an estimate is.
(b) ``streams``: the 1080 x 1920 bf16 chunk-8 FrameStream plain, with smooth="flow", with trimap="propagate" and with
    both (estimated flows), interleaved run by run; milliseconds per frame, with the spread.
(c) ``quality``: tests/matte_smooth_ref.py's synthetic noisy clip through vmatting.MatteScorer before and after
    reader.smooth_mattes on the device's own flow estimates: dtSSD and SAD, filtered over raw.

Each step runs under its own wall-clock limit (``--step-limit`` seconds)."""

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "video-matting_amd"), REPO, os.path.join(REPO, "tests"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from stream_bench import HBM_PEAK, rate, step  # noqa: E402

BYTES_PER_PIXEL = 8 + 4 + 4 + 3  # flow and alpha read, out written, the frame read


def replay_pair_ms(calls, copies, reps, rounds):
    """Medians per call of two HIP graphs whose replays alternate: ``rounds`` rounds of ``calls`` in one, of ``copies``
    in the other -> (call ms, copy ms, call min, call max)."""
    def capture(fns):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for fn in fns:
                fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(rounds):
                for fn in fns:
                    fn()
        return g

    def window(g, count):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / count
    ga, gb = capture(calls), capture(copies)
    na, nb = rounds * len(calls), rounds * len(copies)
    for _ in range(2):
        window(ga, na)
        window(gb, nb)
    a, b = [], []
    for _ in range(reps):
        a.append(window(ga, na))
        b.append(window(gb, nb))
    return statistics.median(a), statistics.median(b), min(a), max(a)


def kernel_size(a, h, w):
    from vmatting import ops
    hw = h * w
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    nsets = max(3, int(300e6 / (BYTES_PER_PIXEL * hw)) + 1)
    yy, xx = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32),
                            torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    flow = torch.stack([(xx - w / 2) * 0.004 + 1.5, (yy - h / 2) * 0.004 - 0.75], -1)
    flow = (flow[None] + 0.1 * torch.randn((nsets, h, w, 2), generator=g, device="cuda")).contiguous()
    alpha = torch.rand((nsets, h, w), generator=g, device="cuda")
    prev = torch.rand((nsets, h, w), generator=g, device="cuda")
    # frames of coarse blocks with a little noise: the colour gate is open over most of the frame, as on footage
    coarse = torch.randint(0, 256, (nsets, (h + 31) // 32, (w + 31) // 32, 3), generator=g, device="cuda", dtype=torch.uint8)
    cmp = coarse.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :h, :w].contiguous()
    prev_cmp = cmp ^ torch.randint(0, 4, cmp.shape, generator=g, device="cuda", dtype=torch.uint8)
    out, weight = torch.empty_like(alpha), torch.empty_like(alpha)
    res = {"buffer_sets": nsets, "bytes_per_pixel": BYTES_PER_PIXEL}
    rounds = max(1, 200 // nsets)
    for name, wt, bpp in (("no_weight", None, BYTES_PER_PIXEL), ("with_weight", weight, BYTES_PER_PIXEL + 4)):
        calls = [lambda i=i: ops.matte_smooth(alpha[i:i + 1], cmp[i:i + 1], flow[i:i + 1], (prev[i], prev_cmp[i]),
                                              out=out[i:i + 1], weight=None if wt is None else wt[i:i + 1])
                 for i in range(nsets)]
        half = hw * bpp // 2 // 4 * 4
        src = torch.empty((nsets, half), dtype=torch.uint8, device="cuda")
        dst = torch.empty((nsets, half), dtype=torch.uint8, device="cuda")
        copies = [lambda i=i: dst[i].copy_(src[i]) for i in range(nsets)]
        ms, ms_copy, lo, hi = replay_pair_ms(calls, copies, a.reps, rounds)
        res[name] = dict(rate(hw * bpp, ms), us=round(ms * 1e3, 2), min_us=round(lo * 1e3, 2), max_us=round(hi * 1e3, 2),
                         copy_same_bytes=dict(rate(2 * half, ms_copy), us=round(ms_copy * 1e3, 2)))
        res[name]["of_copy"] = round(ms_copy / ms, 3)
        del src, dst
    k = torch.empty_like(alpha[:1])
    ops.matte_smooth(alpha[:1], cmp[:1], flow[:1], (prev[0], prev_cmp[0]), out=out[:1], weight=k)
    res["mean_weight"] = round(float(k.mean()), 3)
    return res


def streams(a):
    from vmatting import FrameStream, unet
    from vmatting.weights import synthetic_vgg16
    h, w, n, F = 1080, 1920, a.chunk, a.frames
    np.random.seed(0)
    model = unet.UNetVideo(synthetic_vgg16(0), dtype="bf16", device="cuda").prepare()
    rs = np.random.RandomState(1)
    k = min(F, 2 * n)  # two distinct chunks of host frames, cycled (the source hands out views of them)
    cmp, bg = (rs.randint(0, 256, (k, h, w, 3), dtype=np.uint8) for _ in range(2))
    tri = rs.choice(np.array([0, 128, 255], np.uint8), (k, h, w))

    def source(propagate):
        for i in range(0, F, n):
            m, o = min(n, F - i), i % k
            if propagate:
                yield cmp[o:o + m], bg[o:o + m], (tri[0] if i == 0 else None), None
            else:
                yield cmp[o:o + m], bg[o:o + m], tri[o:o + m]
    kw = dict(chunk=n, depth=2, out="u8")
    made = {"plain": FrameStream(model, h, w, **kw),
            "smooth": FrameStream(model, h, w, smooth="flow", **kw),
            "propagate": FrameStream(model, h, w, trimap="propagate", **kw),
            "propagate_smooth": FrameStream(model, h, w, trimap="propagate", smooth="flow", **kw)}

    def run(name):
        t0 = time.perf_counter()
        tot = sum(m.shape[0] for m in made[name].run(source(name.startswith("propagate"))))
        torch.cuda.synchronize()
        assert tot == F
        return (time.perf_counter() - t0) * 1e3
    times = {name: [] for name in made}
    for i in range(1 + max(3, a.reps // 2)):  # interleaved; round 0 warms up (and captures the graphs)
        for name in made:
            ms = run(name)
            if i:
                times[name].append(ms)
    out = {"height": h, "width": w, "chunk": n, "frames": F, "rounds": len(times["plain"])}
    for name, t in times.items():
        ms = statistics.median(t)
        out["frame_stream_bf16_" + name] = {"ms_per_frame": round(ms / F, 3), "frames_per_s": round(F / ms * 1e3, 1),
                                            "min_ms_per_frame": round(min(t) / F, 3),
                                            "max_ms_per_frame": round(max(t) / F, 3)}
    per = lambda name: out["frame_stream_bf16_" + name]["ms_per_frame"]  # noqa: E731
    out["smooth_adds_ms_per_frame"] = round(per("smooth") - per("plain"), 3)
    out["propagate_adds_ms_per_frame"] = round(per("propagate") - per("plain"), 3)
    out["smooth_on_propagate_adds_ms_per_frame"] = round(per("propagate_smooth") - per("propagate"), 3)
    return out


def quality(a):
    import matte_smooth_ref as ref
    from vmatting import MatteScorer, reader
    out = {}
    for h, w in ((48, 64), (96, 128)):
        for seed in range(3):
            c = ref.noisy_clip(8, h, w, seed)
            filtered = reader.smooth_mattes(c["alpha"], c["cmp"])
            fig = {}
            for name, pred in (("raw", c["alpha"]), ("filtered", filtered)):
                r = MatteScorer(h, w).add(pred, c["gt"]).result()
                fig[name] = {"dtssd": r["clip"]["dtssd"], "sad": float(np.nansum(r["sad"]))}
            out["%dx%d_seed%d" % (h, w, seed)] = {
                "dtssd_ratio": round(fig["filtered"]["dtssd"] / fig["raw"]["dtssd"], 4),
                "sad_ratio": round(fig["filtered"]["sad"] / fig["raw"]["sad"], 4)}
    out["dtssd_ratio_range"] = [min(v["dtssd_ratio"] for v in out.values()), max(v["dtssd_ratio"] for v in out.values())]
    out["sad_ratio_range"] = [min(v["sad_ratio"] for v in out.values() if isinstance(v, dict)),
                              max(v["sad_ratio"] for v in out.values() if isinstance(v, dict))]
    out["flows"] = "ops.estimate_flow at its defaults on the clip's own frames"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", default="1080x1920,2160x3840")
    ap.add_argument("--step-limit", type=int, default=150)
    ap.add_argument("--sections", default="kernel,streams,quality")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "matte_smooth.json"))
    a = ap.parse_args()
    sections = set(a.sections.split(","))
    if not sections or sections - {"kernel", "streams", "quality"}:
        raise SystemExit("smooth_bench: --sections takes kernel, streams and / or quality, got %r" % a.sections)
    if not torch.cuda.is_available():
        raise SystemExit("smooth_bench needs a ROCm GPU")
    from vmatting import ops
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_GBps": HBM_PEAK / 1e9, "reps": a.reps,
           "options": dict(ops.SMOOTH_DEFAULTS)}
    if "kernel" in sections:
        res["kernel"] = {}
        for size in a.sizes.split(","):
            h, w = (int(v) for v in size.split("x"))
            res["kernel"][size] = step("kernel %s" % size, a.step_limit, lambda: kernel_size(a, h, w))
            torch.cuda.empty_cache()
    if "quality" in sections:
        res["quality"] = step("quality", a.step_limit, lambda: quality(a))
    if "streams" in sections:
        res["streams"] = step("streams", a.step_limit, lambda: streams(a))
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
