"""What the enclosed-background fill costs (profiles/trimap_fill.json), by tools/stream_bench.py's method: hipEvent
medians of ``--reps`` replays of a HIP graph that cycles through enough buffer sets to stream more than the 256 MB
memory-side cache per round, one process.

(a) vm_trimap_fill_enclosed at [1 | chunk, height, width] with max_area 0 and 4096 on three inputs (the automatic
    trimaps of a disc with a plate-coloured hole, a random trimap at the site-percolation threshold, a serpentine
    corridor), beside its bytes model, a 265 MB torch copy, and the only other device route: a torch flood from the
    border to a fixpoint, byte-equal, with its iteration count.
(b) FrameStream(trimap="auto") with and without auto_fill=True on the same frames, runs alternating.

    python tools/fill_bench.py [--frames 64] [--chunk 8] [--height 1080] [--width 1920] [--reps 9]
"""

import argparse
import json
import os
import statistics
import sys
import time

TOOLS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TOOLS)
for p in (os.path.join(REPO, "video-matting_amd"), REPO, TOOLS):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from stream_bench import HBM_PEAK, event_ms, graph_ms, rate, step  # noqa: E402

FLOOD_MAX_ITERS = 100000
PARENT_AUTO_FRAMES_PER_S = 334.1  # profiles/trimap_auto.json, streams.frame_stream_bf16_trimap_auto, the commit before


def holed_blob(h, w, seed):
    """A smooth plate with a little noise, a soft-edged disc of another colour on it, and a square of plate colour in the
    disc: foreground that matches the plate (tests/trimap_fill_ref.py's holed_blob_pair, at any size)."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[:h, :w].astype(np.float32)
    plate = np.stack([60 + 40 * np.sin(x / 9), 90 + 30 * np.cos(y / 7), 120 + 0 * x], -1)
    fg = np.stack([200 + 20 * np.sin(y / 5), 40 + 20 * np.cos(x / 6), 30 + 0 * x], -1)
    cx, cy = rs.uniform(0.3, 0.7) * w, rs.uniform(0.3, 0.7) * h
    rad = 0.3 * min(h, w)
    a = np.clip((rad - np.hypot(x - cx, y - cy)) / 4 + 0.5, 0, 1)[..., None]
    frame = a * fg + (1 - a) * plate
    half = int(rad / 3)
    ys, xs = slice(int(cy) - half, int(cy) + half + 1), slice(int(cx) - half, int(cx) + half + 1)
    frame[ys, xs] = plate[ys, xs]
    u8 = lambda v: np.clip(np.rint(v + rs.normal(0, 2, v.shape).astype(np.float32)), 0, 255).astype(np.uint8)  # noqa: E731
    return u8(frame), u8(plate)


def serpentine(h, w):
    """tests/trimap_fill_ref.py's serpentine: one enclosed corridor over the whole frame."""
    t = np.full((h, w), 128, np.uint8)
    rows = list(range(1, h - 1, 2))
    for k, y in enumerate(rows):
        t[y, 1:w - 1] = 0
        if k + 1 < len(rows):
            t[y + 1, w - 2 if k % 2 == 0 else 1] = 0
    return t


def torch_flood(tri, max_area=0):
    """The fill by a flood from the border: the zero pixels reachable from the frame's border by repeated 4-neighbour
    dilation masked to the zero pixels, to a fixpoint; every other zero pixel becomes 128 -> (out, iterations).  No
    area cap (max_area is 0): areas need the components themselves."""
    assert max_area == 0
    z = tri == 0
    reach = z.clone()
    reach[:, 1:-1, 1:-1] = False
    its = 0
    while its < FLOOD_MAX_ITERS:
        its += 1
        grown = reach.clone()
        grown[:, 1:] |= reach[:, :-1]
        grown[:, :-1] |= reach[:, 1:]
        grown[:, :, 1:] |= reach[:, :, :-1]
        grown[:, :, :-1] |= reach[:, :, 1:]
        grown &= z
        if torch.equal(grown, reach):
            break
        reach = grown
    out = tri.clone()
    out[z & ~reach] = 128
    return out, its


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--step-limit", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trimap_fill.json"))
    a = ap.parse_args()
    from vmatting import FrameStream, ops, unet
    from vmatting.weights import synthetic_vgg16
    h, w, F = a.height, a.width, a.frames
    hw = h * w
    res = {"height": h, "width": w, "chunk": a.chunk, "frames": F, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "hbm_peak_GBps": HBM_PEAK / 1e9,
           "bytes_model": "per pixel 1 B read + 1 B written + 4 B of labels written and 4 B read back = 10 B; beyond it the "
                          "seams' labels (4 B on 1/32 + 1/64 of the pixels, a few times), the second read of the trimap by "
                          "emit and of the labels of zero pixels, and the roots' flag words"}
    pairs = [holed_blob(h, w, 40 + i) for i in range(2 * a.chunk)]
    host_cmp, host_bg = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])

    def inputs(n):
        g = torch.Generator(device="cuda")
        g.manual_seed(0)
        blob = ops.trimap_from_plate(torch.from_numpy(host_cmp[:n]).cuda(), torch.from_numpy(host_bg[:n]).cuda())
        u = torch.rand((n, h, w), generator=g, device="cuda")
        rnd = torch.where(u < 0.6, 0, torch.where(u < 0.8, 128, 255)).to(torch.uint8)
        serp = torch.from_numpy(serpentine(h, w)).cuda()[None].repeat(n, 1, 1)
        return {"auto_blob_with_hole": blob, "random_p0.6": rnd, "serpentine": serp}

    def kernels():
        out = {}
        for n in (1, a.chunk):
            nsets = max(3, int(300e6 / (10 * n * hw)) + 1)
            work = torch.empty(ops.trimap_fill_enclosed_workspace_bytes(n, h, w), dtype=torch.uint8, device="cuda")
            per = {"buffer_sets": nsets}
            for name, tri in inputs(n).items():
                tris = tri[None].repeat(nsets, 1, 1, 1)
                outs = torch.empty_like(tris)
                e = {"zero_share": round(float((tri == 0).float().mean()), 3)}
                want, its = torch_flood(tri)
                e["filled_share"] = round(float((want != tri).float().mean()), 4)
                for cap in (0, 4096):
                    call = lambda i, cap=cap: ops.trimap_fill_enclosed(tris[i], cap, out=outs[i], work=work)  # noqa: E731
                    if cap == 0:
                        assert torch.equal(call(0), want), (n, name)   # the same bytes, so the same work is compared
                    ms = graph_ms([lambda i=i: call(i) for i in range(nsets)], a.reps, calls=max(nsets, 24 // n))
                    e["max_area_%d" % cap] = dict(rate(n * hw * 10, ms), us=round(ms * 1e3, 2),
                                                  ns_per_pixel=round(ms * 1e6 / (n * hw), 4))
                # in place, as the stream calls it (the input is restored by a copy inside the timed graph, timed alone too)
                buf = tris.clone()
                ms_c = graph_ms([lambda i=i: buf[i].copy_(tris[i]) for i in range(nsets)], a.reps, calls=max(nsets, 24 // n))
                ms_i = graph_ms([lambda i=i: (buf[i].copy_(tris[i]), ops.trimap_fill_enclosed(buf[i], 0, out=buf[i], work=work))
                                 for i in range(nsets)], a.reps, calls=max(nsets, 24 // n))
                e["in_place_max_area_0_us"] = round((ms_i - ms_c) * 1e3, 2)
                ms_t = event_ms([lambda: torch_flood(tri)], 1, warmup=0)   # (long, and warmed by the check above)
                e["torch_flood"] = {"ms": round(ms_t, 3), "iterations": its,
                                    "over_kernel": round(ms_t / e["max_area_0"]["ms"], 1)}
                per[name] = e
                del tris, outs, buf
            out["n%d" % n] = per
            del work
            torch.cuda.empty_cache()
        m = 1080 * 1920 * 64
        x, y = torch.empty(m, dtype=torch.bfloat16, device="cuda"), torch.empty(m, dtype=torch.bfloat16, device="cuda")
        out["torch_copy_265MB"] = rate(4 * m, event_ms([lambda: y.copy_(x)], a.reps))
        return out
    res["kernels"] = step("fill kernels", a.step_limit, kernels)
    torch.cuda.empty_cache()

    np.random.seed(0)
    model = unet.UNetVideo(synthetic_vgg16(0), dtype="bf16", device="cuda").prepare()

    def streamed():
        n = a.chunk
        k = min(F, 2 * n)  # two distinct chunks of host frames, cycled (the source hands out views of them)

        def source():
            for i in range(0, F, n):
                m, s = min(n, F - i), i % k
                yield host_cmp[s:s + m], host_bg[s:s + m], None
        kw = dict(chunk=n, depth=2, out="u8", trimap="auto")
        streams = {"auto": FrameStream(model, h, w, **kw), "auto_fill": FrameStream(model, h, w, auto_fill=True, **kw)}

        def run(mode):
            t0 = time.perf_counter()
            tot = sum(m.shape[0] for m in streams[mode].run(source()))
            torch.cuda.synchronize()
            assert tot == F
            return (time.perf_counter() - t0) * 1e3
        times = {mode: [] for mode in streams}
        for i in range(1 + max(3, a.reps // 2)):  # alternating; round 0 warms up (and captures the graphs)
            for mode in streams:
                ms = run(mode)
                if i:
                    times[mode].append(ms)
        out = {}
        for mode, t in times.items():
            ms = statistics.median(t)
            out["frame_stream_bf16_trimap_" + mode] = {
                "ms_per_frame": round(ms / F, 3), "frames_per_s": round(F / ms * 1e3, 1),
                "min_frames_per_s": round(F / max(t) * 1e3, 1), "max_frames_per_s": round(F / min(t) * 1e3, 1)}
        out["fill_costs_frames_per_s"] = round(out["frame_stream_bf16_trimap_auto"]["frames_per_s"] -
                                               out["frame_stream_bf16_trimap_auto_fill"]["frames_per_s"], 1)
        out["parent_commit_auto_frames_per_s"] = PARENT_AUTO_FRAMES_PER_S
        return out
    res["streams"] = step("fill streams", a.step_limit, streamed)
    res["not_measured"] = ["real footage", "sizes other than %d x %d" % (h, w), "graph=False throughput"]
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
