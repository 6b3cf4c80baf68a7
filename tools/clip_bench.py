"""Measure the video model's clip path: the fused feed kernel beside the unfused route it replaces, the per-frame graph
and its parts, the host link, and ClipStream from host arrays.  Prints one JSON line and writes it to
profiles/clip_stream.json.  The compose section (``--sections compose``) runs ClipStream with out="over" (a static
new plate) beside out="u8" on the same clip, their runs interleaved in one process; it prints a second JSON line and
writes it under "clip_bench" in profiles/compose_stream.json.  The flow section (``--sections flow``) times the flow
estimator (ops.estimate_flow: the blocked sweep kernel beside the one-sweep-per-launch path, and the time of one
full-resolution sweep of each) and ClipStream(flow="estimate") beside ClipStream(flow="given") on the same frames; it
writes profiles/flow_estimate.json.

    python tools/clip_bench.py [--sizes 500x1200,1080x1920] [--frames 48] [--reps 9] [--dtype bf16]
                               [--sections clip,compose,flow]

Kernel times are hipEvent medians over ``--reps`` runs after a warm-up; every run of a kernel works on another of
several buffer sets, so its inputs and outputs do not sit in the 256 MB memory-side cache between runs.  The fused and
the unfused feed are timed in the same process, their windows interleaved.  GB/s are algorithmic bytes over that time
(per pixel: 6 B of uint8 + 8 B of backward flow [+ 8 B of forward flow] read, 80 B written in bf16 / 160 B in f32; the
4 bilinear taps of the previous matte come from L2 and are not counted); ``hbm_frac`` is that over the 8 TB/s peak.
Each step runs under its own wall-clock limit (``--step-limit`` seconds): a step that overruns ends the tool with an
error instead of starting the next one.
"""

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
        print("# %-28s %.1f s" % (name, time.time() - t0), file=sys.stderr)


def window_ms(fns):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for fn in fns:
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / len(fns)


def event_ms(fns, reps, warmup=3):
    """Median hipEvent time of one call: every timed window runs each of ``fns`` once (the same work on different
    buffers, back to back) and is divided by their number."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    return statistics.median(window_ms(fns) for _ in range(reps))


def interleaved_ms(fa, fb, reps, warmup=3):
    """Medians of two routes whose windows alternate (a, b, a, b, ...): clocks and cache state drift alike for both."""
    for _ in range(warmup):
        for fn in fa + fb:
            fn()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(window_ms(fa))
        tb.append(window_ms(fb))
    return statistics.median(ta), statistics.median(tb)


def rate(nbytes, ms):
    return {"ms": round(ms, 4), "GBps": round(nbytes / ms / 1e6, 1), "hbm_frac": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)}


def measure(h, w, a, vgg, params):
    from oracle.flow import smooth_flow
    from vmatting import ClipStream, _lib, ops, unet_simple
    dtype = a.dtype
    tdt = ops.TORCH_DTYPE[dtype]
    px = h * w
    res = {}
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    bwn = smooth_flow(h, w, seed=7, amp=6.0)
    fwn = smooth_flow(h, w, seed=8, amp=6.0)

    def buffers(dt):
        return (torch.zeros((3, h, w, 8), dtype=dt, device="cuda"), torch.zeros((1, h, w, 32), dtype=dt, device="cuda"))
    sets = []
    for _ in range(a.sets):
        sets.append(dict(cmp=torch.randint(0, 256, (1, h, w, 3), generator=g, device="cuda", dtype=torch.uint8),
                         bg=torch.randint(0, 256, (1, h, w, 3), generator=g, device="cuda", dtype=torch.uint8),
                         prev=torch.rand((1, h, w), generator=g, device="cuda"),
                         bw=torch.from_numpy(bwn).cuda()[None].clone(), fw=torch.from_numpy(fwn).cuda()[None].clone(),
                         flag=torch.zeros(1, dtype=torch.int32, device="cuda"), out=buffers(tdt)))

    def fused(s, occ, out=None, bg=None):
        tin, in9 = out or s["out"]
        ops.clip_feed(s["cmp"], s["bg"] if bg is None else bg, s["prev"], s["bw"], s["fw"] if occ else None, a.thresh,
                      towers=tin[..., :3], cat=in9[..., :9], err=s["flag"])

    # the unfused route to the same buffers, from calls of the parent commit only: the uint8 feed into one f32 frame,
    # the warp, the mask (the C call: ops.fb_consistency waits for its flag), a repeat and six converts
    def unfused(s, occ, scratch):
        tin, in9 = scratch["out"]
        ops.frames_from_u8(s["cmp"], s["bg"], out=scratch["x6"])
        ops.remap_f32(s["prev"], s["bw"], out=scratch["a"])
        if occ:
            _lib.check(_lib.lib().vm_fb_consistency(ops._ptr(s["bw"]), ops._ptr(s["fw"]), h, w, ops._ptr(scratch["a"]),
                                                    a.thresh, 0, ops._ptr(s["flag"]), _lib.stream_handle()), "fb")
        a3 = scratch["a"][..., None].repeat(1, 1, 1, 3)
        for t, x in enumerate((scratch["x6"][..., :3], scratch["x6"][..., 3:6], a3)):
            ops.convert(x, tin[t:t + 1])
            ops.convert(x, in9[..., 3 * t:3 * t + 3])
    scr = [dict(out=buffers(tdt), x6=torch.empty((1, h, w, 6), device="cuda"), a=torch.empty((1, h, w), device="cuda"))
           for _ in sets]

    def feed_kernel():
        out = {}
        for occ in (False, True):
            # the same buffers from both routes, so the same work is compared
            fused(sets[0], occ)
            unfused(sets[0], occ, scr[0])
            assert all(torch.equal(x.view(torch.int16 if tdt == torch.bfloat16 else torch.int32),
                                   y.view(torch.int16 if tdt == torch.bfloat16 else torch.int32))
                       for x, y in zip(sets[0]["out"], scr[0]["out"])), "fused and unfused feeds differ"
            ms_f, ms_u = interleaved_ms([lambda s=s, occ=occ: fused(s, occ) for s in sets],
                                        [lambda s=s, c=c, occ=occ: unfused(s, occ, c) for s, c in zip(sets, scr)], a.reps)
            eb = 80 if tdt == torch.bfloat16 else 160
            key = "occ" if occ else "warp"
            out["clip_feed_%s_%s" % (dtype, key)] = rate(px * (6 + 8 + (8 if occ else 0) + eb), ms_f)
            out["unfused_feed_%s_%s" % (dtype, key)] = {"ms": round(ms_u, 4)}
            out["fused_speedup_%s" % key] = round(ms_u / ms_f, 2)
        plate = sets[0]["bg"][0].clone()
        ms = event_ms([lambda s=s: fused(s, False, bg=plate) for s in sets], a.reps)
        out["clip_feed_%s_warp_static_bg" % dtype] = rate(px * (3 + 8 + (80 if tdt == torch.bfloat16 else 160)) + px * 3, ms)
        if tdt == torch.bfloat16:
            o32 = [buffers(torch.float32) for _ in sets]
            for occ in (False, True):
                ms = event_ms([lambda s=s, o=o, occ=occ: fused(s, occ, out=o) for s, o in zip(sets, o32)], a.reps)
                out["clip_feed_f32_%s" % ("occ" if occ else "warp")] = rate(px * (6 + 8 + (8 if occ else 0) + 160), ms)
        return out
    res.update(step("feed kernel %dx%d" % (h, w), a.step_limit, feed_kernel))
    del scr
    torch.cuda.empty_cache()

    # ---- the host link per frame: cmp + bg + backward (+ forward) up from pinned memory, one u8 matte down
    def link():
        hs = [torch.empty(s, dtype=d).pin_memory() for s, d in (((1, h, w, 3), torch.uint8), ((1, h, w, 3), torch.uint8),
                                                                ((1, h, w, 2), torch.float32), ((1, h, w, 2), torch.float32))]
        ds = [sets[0]["cmp"], sets[0]["bg"], sets[0]["bw"], sets[0]["fw"]]
        up = lambda k: [d.copy_(s, non_blocking=True) for d, s in list(zip(ds, hs))[:k]]  # noqa: E731
        ms3, ms4 = event_ms([lambda: up(3)], a.reps), event_ms([lambda: up(4)], a.reps)
        ms_plate = event_ms([lambda: [ds[0].copy_(hs[0], non_blocking=True), ds[2].copy_(hs[2], non_blocking=True)]], a.reps)
        hq = torch.empty((1, h, w), dtype=torch.uint8).pin_memory()
        dq = torch.empty((1, h, w), dtype=torch.uint8, device="cuda")
        ms_dn = event_ms([lambda: hq.copy_(dq, non_blocking=True)], a.reps)
        src = [np.frombuffer(np.random.RandomState(2).bytes(t.numel() * t.element_size()), np.uint8) for t in hs[:3]]
        t0 = time.perf_counter()
        for _ in range(3):
            for s, t in zip(src, hs):
                t.numpy().reshape(-1).view(np.uint8)[...] = s
        ms_host = (time.perf_counter() - t0) / 3 * 1e3
        return {"h2d_frame_warp": {"ms": round(ms3, 3), "GBps": round(px * 14 / ms3 / 1e6, 1)},
                "h2d_frame_occ": {"ms": round(ms4, 3), "GBps": round(px * 22 / ms4 / 1e6, 1)},
                "h2d_frame_warp_static_bg": {"ms": round(ms_plate, 3), "GBps": round(px * 11 / ms_plate / 1e6, 1)},
                "d2h_u8_matte": {"ms": round(ms_dn, 3), "GBps": round(px / ms_dn / 1e6, 1)},
                "host_copy_into_pinned_warp": {"ms": round(ms_host, 3), "GBps": round(px * 14 / ms_host / 1e6, 1)}}
    res.update(step("link %dx%d" % (h, w), a.step_limit, link))
    s0 = sets[0]
    del sets
    torch.cuda.empty_cache()

    # ---- the model: forward_fed and the whole per-frame chain as graph replays, all towers and without the bg tower
    np.random.seed(0)
    model = unet_simple.UNetSimple(unet_simple.Vgg16(vgg, dtype), False, dtype).load_params(params)

    def graphs():
        out = {}
        tin, in9 = model.feed_views(1, h, w)
        alpha = model._buffers(1, h, w)["out"]
        q = torch.empty((1, h, w), dtype=torch.uint8, device="cuda")
        ms_q = event_ms([lambda: ops.matte_quantize(alpha, out=q)], a.reps)
        out["matte_quantize_u8"] = {"ms": round(ms_q, 4)}
        for towers, key in (((0, 1, 2), "all_towers"), ((0, 2), "no_bg_tower")):
            gf = model.capture_fed(1, h, w, towers)
            out["forward_fed_graph_%s" % key] = {"ms": round(event_ms([gf.replay], a.reps), 3)}
            gc = model.capture_fed(1, h, w, towers,
                                   pre=lambda: ops.clip_feed(s0["cmp"], s0["bg"], alpha, s0["bw"], None, towers=tin,
                                                             cat=in9, err=s0["flag"]),
                                   post=lambda: ops.matte_quantize(alpha, out=q))
            out["frame_graph_%s" % key] = {"ms": round(event_ms([gc.replay], a.reps), 3)}
            del gf, gc
        return out
    res.update(step("graphs %dx%d" % (h, w), a.step_limit, graphs))

    # ---- ClipStream from host arrays: two distinct host frames, cycled
    def streamed():
        rs = np.random.RandomState(1)
        F = a.frames
        cmp, bg = (rs.randint(0, 256, (2, h, w, 3), dtype=np.uint8) for _ in range(2))
        alpha0 = rs.uniform(size=(h, w)).astype(np.float32)
        out = {}

        def source(plate, occ, n):
            for i in range(n):
                yield cmp[i % 2], (None if plate else bg[i % 2]), bwn, (fwn if occ else None)

        def fps(cs, plate, occ):
            def run():
                t0 = time.perf_counter()
                tot = sum(1 for _ in cs.run(source(plate, occ, F), alpha0))
                torch.cuda.synchronize()
                assert tot == F
                return (time.perf_counter() - t0) * 1e3
            run()
            ms = statistics.median(run() for _ in range(max(3, a.reps // 3)))
            return {"ms_per_frame": round(ms / F, 3), "frames_per_s": round(F / ms * 1e3, 1),
                    "bg_tower_evals": cs.stats["bg_tower_evals"]}
        kw = dict(depth=2, out="u8", thresh=a.thresh)
        out["clip_stream_per_frame_bg"] = fps(ClipStream(model, h, w, **kw), False, False)
        out["clip_stream_per_frame_bg_occ"] = fps(ClipStream(model, h, w, occlusion=True, **kw), False, True)
        out["clip_stream_plate_full"] = fps(ClipStream(model, h, w, static_bg=bg[0], reuse_bg_tower=False, **kw), True, False)
        out["clip_stream_plate_reuse"] = fps(ClipStream(model, h, w, static_bg=bg[0], reuse_bg_tower=True, **kw), True, False)
        # do the mattes of the plate-reuse route equal the full-tower mattes, bit for bit, at this size?
        k = min(F, 6)
        mattes = [np.stack(list(ClipStream(model, h, w, static_bg=bg[0], reuse_bg_tower=r, out="f32", thresh=a.thresh)
                                .run(source(True, False, k), alpha0))) for r in (False, True)]
        out["plate_reuse_bit_equal"] = bool(np.array_equal(mattes[0], mattes[1]))
        out["plate_reuse_max_abs_diff"] = float(np.abs(mattes[0] - mattes[1]).max())
        return out
    res.update(step("streamed %dx%d" % (h, w), a.step_limit, streamed))

    # ---- which leg bounds the stream (the device legs overlap across slots; the host's copies are serial with them)
    legs = {"upload": res["h2d_frame_warp"]["ms"], "compute": res["frame_graph_all_towers"]["ms"],
            "download": res["d2h_u8_matte"]["ms"], "host_copy": res["host_copy_into_pinned_warp"]["ms"]}
    res["legs_ms_per_frame"] = legs
    res["bounding_leg"] = max(legs, key=legs.get)
    res["frame_parts_ms"] = {"feed": res["clip_feed_%s_warp" % dtype]["ms"],
                             "forward": res["forward_fed_graph_all_towers"]["ms"],
                             "forward_no_bg_tower": res["forward_fed_graph_no_bg_tower"]["ms"],
                             "quantise": res["matte_quantize_u8"]["ms"], "upload": legs["upload"],
                             "download": legs["download"]}
    del model
    torch.cuda.empty_cache()
    return res


def measure_compose(h, w, a, vgg, params):
    """ClipStream frames/s with out="u8" and out="over" (static original and new plates, the plate's tower reused),
    interleaved: every round runs each output once."""
    from oracle.flow import smooth_flow
    from vmatting import ClipStream, unet_simple
    np.random.seed(0)
    model = unet_simple.UNetSimple(unet_simple.Vgg16(vgg, a.dtype), False, a.dtype).load_params(params)
    rs = np.random.RandomState(1)
    F = a.frames
    cmp, bg = (rs.randint(0, 256, (2, h, w, 3), dtype=np.uint8) for _ in range(2))
    plate = rs.randint(0, 256, (h, w, 3), dtype=np.uint8)
    alpha0 = rs.uniform(size=(h, w)).astype(np.float32)
    bwn = smooth_flow(h, w, seed=7, amp=6.0)

    def source():
        for i in range(F):
            yield cmp[i % 2], None, bwn, None
    kw = dict(depth=2, static_bg=bg[0], reuse_bg_tower=True, thresh=a.thresh)
    streams = {"u8": ClipStream(model, h, w, out="u8", **kw), "over": ClipStream(model, h, w, out="over", new_bg=plate, **kw)}

    def run(cs):
        t0 = time.perf_counter()
        tot = sum(1 for _ in cs.run(source(), alpha0))
        torch.cuda.synchronize()
        assert tot == F
        return (time.perf_counter() - t0) * 1e3

    def streamed():
        times = {name: [] for name in streams}
        for i in range(1 + max(3, a.reps // 3)):  # round 0 warms up (and captures the graphs)
            for name, cs in streams.items():
                ms = run(cs)
                if i:
                    times[name].append(ms)
        out = {}
        for name, t in times.items():
            ms = statistics.median(t)
            out["clip_stream_plate_reuse_" + name] = {"ms_per_frame": round(ms / F, 3), "frames_per_s": round(F / ms * 1e3, 1),
                                                      "min_ms_per_frame": round(min(t) / F, 3),
                                                      "max_ms_per_frame": round(max(t) / F, 3)}
        out["over_keeps_of_u8"] = round(out["clip_stream_plate_reuse_over"]["frames_per_s"] /
                                        out["clip_stream_plate_reuse_u8"]["frames_per_s"], 3)
        return out
    res = step("compose streamed %dx%d" % (h, w), a.step_limit, streamed)
    del streams, model
    torch.cuda.empty_cache()
    return res


def measure_flow(h, w, a, vgg, params):
    """The flow estimator: one direction with the defaults, blocked against per-sweep (interleaved windows, two buffer
    sets); one full-resolution sweep of either path, from the difference of two sweep counts at levels=1; and ClipStream
    with flow="estimate" (with and without occlusion) beside flow="given" fed with the same flows, round-robin."""
    from vmatting import ClipStream, _lib, ops, unet_simple
    px = h * w
    rs = np.random.RandomState(3)
    # four frames cut from one smooth texture, each 3 px right and 2 px down of the one before
    tex = rs.uniform(0, 255, (h + 16, w + 16, 3)).astype(np.float32)
    for _ in range(3):
        tex = sum(np.roll(tex, (i, j), (0, 1)) for i in (-1, 0, 1) for j in (-1, 0, 1)) / 9.0
    tex = np.clip((tex - tex.mean()) / tex.std() * 48.0 + 128.0, 0, 255).astype(np.uint8)
    frames = np.stack([tex[2 * i:2 * i + h, 3 * i:3 * i + w] for i in range(4)])
    dev = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames]
    sets = [dict(cur=dev[i + 1], prev=dev[i], out=torch.empty((h, w, 2), device="cuda"),
                 work=torch.empty(ops.flow_workspace_bytes(h, w), dtype=torch.uint8, device="cuda")) for i in range(2)]

    def est(s, blocked, **kw):
        _lib.set_option("flow_blocked", blocked)
        ops.estimate_flow(s["cur"], s["prev"], out=s["out"], work=s["work"], **kw)

    def kernels():
        out = {}
        flows = []
        for blocked in (1, 0):
            est(sets[0], blocked)
            flows.append(sets[0]["out"].clone())
        assert torch.equal(flows[0].view(torch.int32), flows[1].view(torch.int32)), "blocked and per-sweep flows differ"
        out["mean_abs_flow_px"] = round(float(flows[0].abs().mean()), 3)
        ms_b, ms_p = interleaved_ms([lambda s=s: est(s, 1) for s in sets], [lambda s=s: est(s, 0) for s in sets], a.reps)
        out["estimate_blocked"] = {"ms": round(ms_b, 3)}
        out["estimate_per_sweep"] = {"ms": round(ms_p, 3)}
        out["blocked_speedup"] = round(ms_p / ms_b, 2)
        # one full-resolution sweep: levels=1, warps=3, (iters 40 - iters 20) / 60
        per = {}
        for blocked, key in ((1, "blocked"), (0, "per_sweep")):
            lo, hi = interleaved_ms([lambda s=s: est(s, blocked, levels=1, iters=20) for s in sets],
                                    [lambda s=s: est(s, blocked, levels=1, iters=40) for s in sets], a.reps)
            per[key] = (hi - lo) / 60.0
        # bytes per pixel and sweep: per-sweep 8 (u, v) + 16 (Ix, Iy, It, den) + 8 (u0, v0) read, 8 written; blocked
        # the same reads for the 64 x 40 staged pixels of a 56 x 32 tile and one write per 4 sweeps
        model = {"per_sweep": 40.0, "blocked": (32.0 * (64 * 40) / (56 * 32) + 8.0) / 4}
        for key, ms in per.items():
            out["sweep_" + key] = dict(rate(px * model[key], ms), us=round(ms * 1e3, 2), model_bytes_per_px=round(model[key], 2))
        _lib.set_option("flow_blocked", 1)
        return out
    res = step("flow kernels %dx%d" % (h, w), a.step_limit, kernels)

    def streamed():
        np.random.seed(0)
        model = unet_simple.UNetSimple(unet_simple.Vgg16(vgg, a.dtype), False, a.dtype).load_params(params)
        F = a.frames
        bg = rs.randint(0, 256, (h, w, 3), dtype=np.uint8)
        alpha0 = rs.uniform(size=(h, w)).astype(np.float32)
        # the flows a caller of flow="given" would bring: frame i against frame i - 1 of the 4-cycle, both directions
        bw = [ops.estimate_flow(dev[i], dev[i - 1]).cpu().numpy() for i in range(4)]
        fw = [ops.estimate_flow(dev[i - 1], dev[i]).cpu().numpy() for i in range(4)]

        def source(given, occ):
            for i in range(F):
                k = i % 4
                yield frames[k], bg, (bw[k] if given else None), (fw[k] if given and occ else None)
        kw = dict(depth=2, out="u8", thresh=a.thresh)
        streams = {(mode, occ): ClipStream(model, h, w, occlusion=occ, flow=mode, **kw)
                   for occ in (False, True) for mode in ("given", "estimate")}

        def run(mode, occ):
            t0 = time.perf_counter()
            extra = dict(cmp0=frames[3]) if mode == "estimate" else {}
            tot = sum(1 for _ in streams[mode, occ].run(source(mode == "given", occ), alpha0, **extra))
            torch.cuda.synchronize()
            assert tot == F
            return (time.perf_counter() - t0) * 1e3
        times = {k: [] for k in streams}
        for i in range(1 + max(3, a.reps // 3)):  # round 0 warms up (and captures the graphs)
            for k in streams:
                ms = run(*k)
                if i:
                    times[k].append(ms)
        out = {}
        for (mode, occ), t in times.items():
            ms = statistics.median(t)
            out["clip_stream_%s%s" % (mode, "_occ" if occ else "")] = {
                "ms_per_frame": round(ms / F, 3), "frames_per_s": round(F / ms * 1e3, 1),
                "min_ms_per_frame": round(min(t) / F, 3), "max_ms_per_frame": round(max(t) / F, 3)}
        for occ in ("", "_occ"):
            out["estimator_cost_ms_per_frame" + occ] = round(out["clip_stream_estimate" + occ]["ms_per_frame"] -
                                                             out["clip_stream_given" + occ]["ms_per_frame"], 3)
        return out
    res.update(step("flow streamed %dx%d" % (h, w), a.step_limit, streamed))
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500x1200,1080x1920")
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--thresh", type=float, default=6.0)
    ap.add_argument("--sets", type=int, default=5, help="buffer sets the kernel timings cycle through")
    ap.add_argument("--step-limit", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "clip_stream.json"))
    ap.add_argument("--compose-out", default=os.path.join(REPO, "profiles", "compose_stream.json"))
    ap.add_argument("--flow-out", default=os.path.join(REPO, "profiles", "flow_estimate.json"))
    ap.add_argument("--sections", default="clip,compose", help="comma-separated: clip, compose, flow")
    a = ap.parse_args()
    sections = set(a.sections.split(","))
    if not sections or sections - {"clip", "compose", "flow"}:
        raise SystemExit("clip_bench: --sections takes clip, compose and / or flow, got %r" % a.sections)
    if not torch.cuda.is_available():
        raise SystemExit("clip_bench needs a ROCm GPU")
    from oracle import models as om
    from vmatting.weights import synthetic_vgg16
    vgg = synthetic_vgg16(0)
    params = om.unet_simple_params(np.random.RandomState(1))
    head = {"device": torch.cuda.get_device_name(0), "dtype": a.dtype, "frames": a.frames, "reps": a.reps}
    sizes = [tuple(int(v) for v in size.split("x")) for size in a.sizes.split(",")]
    if "clip" in sections:
        res = dict(head, hbm_peak_GBps=HBM_PEAK / 1e9, sizes={})
        for h, w in sizes:
            res["sizes"]["%dx%d" % (h, w)] = measure(h, w, a, vgg, params)
        line = json.dumps(res)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
        print(line)
    if "compose" in sections:
        res = dict(head, sizes={"%dx%d" % (h, w): measure_compose(h, w, a, vgg, params) for h, w in sizes})
        doc = {}
        if os.path.exists(a.compose_out):
            with open(a.compose_out) as f:
                doc = json.load(f)
        doc["clip_bench"] = res
        os.makedirs(os.path.dirname(a.compose_out), exist_ok=True)
        with open(a.compose_out, "w") as f:
            f.write(json.dumps(doc) + "\n")
        print(json.dumps(res))
    if "flow" in sections:
        res = dict(head, hbm_peak_GBps=HBM_PEAK / 1e9,
                   sizes={"%dx%d" % (h, w): measure_flow(h, w, a, vgg, params) for h, w in sizes})
        line = json.dumps(res)
        os.makedirs(os.path.dirname(a.flow_out), exist_ok=True)
        with open(a.flow_out, "w") as f:
            f.write(line + "\n")
        print(line)


if __name__ == "__main__":
    main()
