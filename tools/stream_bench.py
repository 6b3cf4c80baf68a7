"""Measure the clip ends: the ingest and quantise kernels, the torch route they replace, the host link, and the
streamed pipeline beside the resident-frames VideoMatter.  Prints one JSON line and writes it to
profiles/ingest_stream.json.  The compose section (``--sections compose``) measures vm_matte_compose the same way: the
three modes with per-frame and static plates, the torch route to the same bytes (float64 elementwise ops, bit-equal
output asserted), and FrameStream with out="u8" / "over" / "bgra" interleaved in one process; it prints a second JSON
line and writes it under "stream_bench" in profiles/compose_stream.json.  The propagate section (``--sections
propagate``, at every size of ``--propagate-sizes``) measures vm_trimap_propagate alone for grow 0, 1 and 4 against its
bytes-per-pixel model, the flow estimator's calls per frame, and FrameStream with per-frame trimaps, with
trimap="propagate" on given flows and on estimated ones, interleaved in one process; it prints a third JSON line and
writes profiles/trimap_propagate.json.  The auto section (``--sections auto``) measures vm_trimap_from_plate for one
frame and for a chunk at radii (0, 0), the defaults and (32, 32) against its bytes model and against the same
definition in torch ops (equal bytes asserted), and FrameStream(trimap="auto") beside per-frame trimaps, interleaved; it
prints a JSON line and writes profiles/trimap_auto.json.  Its last leg (alone with ``--sections shadow``) measures the
same call with the shadow-tolerant distance beside the plain one, in turn in one run, and FrameStream(trimap="auto") with
and without shadow="chroma", interleaved; it prints a JSON line and writes profiles/plate_shadow.json.

    python tools/stream_bench.py [--frames 64] [--chunk 8] [--height 1080] [--width 1920] [--reps 9]
                                 [--sections ingest,compose,propagate,auto,shadow] [--propagate-sizes 500x1200,1080x1920]

Kernel times are hipEvent medians over ``--reps`` runs after a warm-up; every run of a kernel works on another of
several buffer sets, so the 83 MB alpha of the quantise kernel does not sit in the 256 MB memory-side cache between
runs.  GB/s are algorithmic bytes (read once + written once) over that time; ``hbm_frac`` is that over the 8 TB/s peak.
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
VGG_MEAN = (103.939, 116.779, 123.68)


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


def event_ms(fns, reps, warmup=3):
    """Median hipEvent time of one call: every timed window runs each of ``fns`` once (the same work on different
    buffers, back to back) and is divided by their number."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for fn in fns:
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / len(fns))
    return statistics.median(times)


def graph_ms(fns, reps, calls=1000):
    """Median hipEvent time of one call inside a HIP graph, for calls so short that the host could not launch them
    back to back: ``fns`` in turn, about ``calls`` calls in all, are captured once and every timed window is one
    replay."""
    inner = max(1, calls // len(fns))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for fn in fns:
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            for fn in fns:
                fn()
    return event_ms([g.replay], reps) / (inner * len(fns))


def rate(nbytes, ms):
    return {"ms": round(ms, 4), "GBps": round(nbytes / ms / 1e6, 1), "hbm_frac": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)}


def merge_json(path, key, value):
    """Write ``value`` under ``key`` of the JSON object in ``path``, keeping what other tools wrote there."""
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc[key] = value
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(doc) + "\n")


def compose_bytes(px, hw, mode, static_bg, static_nw):
    """Algorithmic bytes of one vm_matte_compose call: alpha + cmp + bg (+ new plate) read once, the result written
    once; a static plate counts once, not per frame."""
    plate = lambda static: hw * 3 if static else px * 3  # noqa: E731
    return px * (4 + 3) + plate(static_bg) + (plate(static_nw) if mode == "over" else 0) + px * (3 if mode == "over" else 4)


def torch_compose(alpha, cmp, bg, new_bg, mode):
    """The same bytes by torch ops on the device: float64 elementwise, one rounding (half to even)."""
    c, b = cmp.double(), bg.double()
    fin = lambda v: v.clamp(0.0, 255.0).round().to(torch.uint8)  # noqa: E731
    if mode == "over":
        a = alpha.double().clamp(0.0, 1.0)
        return fin(c + (1.0 - a) * (new_bg.double() - b))
    q = (alpha * 255.0).round().clamp(0.0, 255.0)
    qd = q.double()
    if mode == "premul":
        bgr = fin(c - ((255.0 - qd) * b) / 255.0)
    else:
        bgr = torch.where(qd == 0.0, torch.zeros((), dtype=torch.uint8, device=cmp.device),
                          fin(b + ((c - b) * 255.0) / qd.clamp(min=1.0)))
    return torch.cat([bgr, q.to(torch.uint8)], -1)


def compose_section(a):
    """vm_matte_compose at [chunk, height, width]: kernel times, the torch route, FrameStream with the new outputs."""
    from vmatting import FrameStream, ops, unet
    from vmatting.weights import synthetic_vgg16
    n, h, w, F = a.chunk, a.height, a.width, a.frames
    px, hw = n * h * w, h * w
    res = {"shape": [n, h, w], "frames": F, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "hbm_peak_GBps": HBM_PEAK / 1e9}
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    u8 = lambda: torch.randint(0, 256, (n, h, w, 3), generator=g, device="cuda", dtype=torch.uint8)  # noqa: E731
    # one set is 4 + 3 + 3 + 3 + 4 B per pixel = 282 MB at 8 x 1080 x 1920: past the 256 MB memory-side cache
    sets = [dict(alpha=torch.rand((n, h, w, 1), generator=g, device="cuda"), cmp=u8(), bg=u8(), nw=u8())
            for _ in range(a.sets)]

    def kernels():
        out = {}
        for mode in ("over", "bgra", "premul"):
            o = [torch.empty((n, h, w, 3 if mode == "over" else 4), dtype=torch.uint8, device="cuda") for _ in sets]
            plates = [(False, False), (True, False)] + ([(False, True), (True, True)] if mode == "over" else [])
            for static_bg, static_nw in plates:
                def call(s, dst):
                    bg = s["bg"][0] if static_bg else s["bg"]
                    nw = None if mode != "over" else s["nw"][0] if static_nw else s["nw"]
                    return ops.matte_compose(s["alpha"], s["cmp"], bg, nw, mode=mode, out=dst)
                ms = event_ms([lambda s=s, d=d: call(s, d) for s, d in zip(sets, o)], a.reps)
                name = mode + ("_static_bg" if static_bg else "") + ("_static_new" if static_nw else "")
                out[name] = rate(compose_bytes(px, hw, mode, static_bg, static_nw), ms)
            s = sets[0]
            nw = s["nw"] if mode == "over" else None
            assert torch.equal(torch_compose(s["alpha"], s["cmp"], s["bg"], nw, mode),
                               ops.matte_compose(s["alpha"], s["cmp"], s["bg"], nw, mode=mode)), mode
            ms_t = event_ms([lambda s=s: torch_compose(s["alpha"], s["cmp"], s["bg"], s["nw"] if mode == "over" else None,
                                                       mode) for s in sets], a.reps)
            out["torch_route_" + mode] = {"ms": round(ms_t, 4)}
            out["speedup_over_torch_" + mode] = round(ms_t / out[mode]["ms"], 1)
            del o
        return out
    res["kernels"] = step("compose kernels", a.step_limit, kernels)
    del sets
    torch.cuda.empty_cache()

    np.random.seed(0)
    model = unet.UNetVideo(synthetic_vgg16(0), dtype="bf16", device="cuda").prepare()

    def streamed():
        rs = np.random.RandomState(1)
        k = min(F, 2 * n)  # two distinct chunks of host frames, cycled (the source hands out views of them)
        cmp, bg = (rs.randint(0, 256, (k, h, w, 3), dtype=np.uint8) for _ in range(2))
        tri = rs.choice(np.array([0, 128, 255], np.uint8), (k, h, w))
        plate = rs.randint(0, 256, (h, w, 3), dtype=np.uint8)

        def source():
            for i in range(0, F, n):
                m = min(n, F - i)
                o = i % k
                yield cmp[o:o + m], bg[o:o + m], tri[o:o + m]
        streams = {"u8": FrameStream(model, h, w, chunk=n, depth=2, out="u8"),
                   "over": FrameStream(model, h, w, chunk=n, depth=2, out="over", new_bg=plate),
                   "bgra": FrameStream(model, h, w, chunk=n, depth=2, out="bgra")}

        def run(fs):
            t0 = time.perf_counter()
            tot = sum(m.shape[0] for m in fs.run(source()))
            torch.cuda.synchronize()
            assert tot == F
            return (time.perf_counter() - t0) * 1e3
        times = {name: [] for name in streams}
        for i in range(1 + max(3, a.reps // 2)):  # interleaved: every round runs each output once; round 0 warms up
            for name, fs in streams.items():
                ms = run(fs)
                if i:
                    times[name].append(ms)
        out = {}
        for name, t in times.items():
            ms = statistics.median(t)
            out["frame_stream_bf16_%s_depth2" % name] = {"ms": round(ms, 2), "frames_per_s": round(F / ms * 1e3, 1),
                                                         "min_ms": round(min(t), 2), "max_ms": round(max(t), 2)}
        for name in ("over", "bgra"):
            out["%s_keeps_of_u8" % name] = round(out["frame_stream_bf16_%s_depth2" % name]["frames_per_s"] /
                                                 out["frame_stream_bf16_u8_depth2"]["frames_per_s"], 3)
        return out
    res["streams"] = step("compose streams", a.step_limit, streamed)

    # the download leg grows from 1 to 3 - 4 B per pixel
    def link():
        out = {}
        for c in (1, 3, 4):
            hq = torch.empty((n, h, w, c), dtype=torch.uint8).pin_memory()
            dq = torch.empty((n, h, w, c), dtype=torch.uint8, device="cuda")
            ms = event_ms([lambda: hq.copy_(dq, non_blocking=True)], a.reps)
            out["d2h_pinned_u8_x%d" % c] = {"ms": round(ms, 3), "GBps": round(px * c / ms / 1e6, 1)}
        return out
    res["link"] = step("compose link", a.step_limit, link)
    merge_json(a.compose_out, "stream_bench", res)
    print(json.dumps(res))


def propagate_bytes_per_pixel(grow):
    """The bytes model of one vm_trimap_propagate call, per pixel: 8 B of flow read and 1 B written by the gather;
    1 B of prev read (by the gather itself for grow 0, else by the class-map pass); and for grow > 0 the class map,
    two bits per pixel, written once (0.25 B) and gathered (0.25 B counted once: neighbouring pixels share words)."""
    return 8 + 1 + 1 + (0.5 if grow else 0.0)


def propagate_size(a, h, w):
    from vmatting import FrameStream, ops, unet
    from vmatting.weights import synthetic_vgg16
    n, F, hw = a.chunk, a.frames, h * w
    res = {}
    g = torch.Generator(device="cuda")
    g.manual_seed(0)

    def kernels():
        # enough buffer sets that one round of calls streams more than the 256 MB memory-side cache
        nsets = max(a.sets, int(300e6 / (10 * hw)) + 1)
        coarse = torch.randint(0, 3, (nsets, (h + 7) // 8, (w + 7) // 8), generator=g, device="cuda")
        tri = (coarse * 128).clamp(max=255).to(torch.uint8).repeat_interleave(8, 1).repeat_interleave(8, 2)
        tri = tri[:, :h, :w].contiguous()  # blocks of 0 / 128 / 255, 8 pixels wide
        flow = (torch.rand((nsets, h, w, 2), generator=g, device="cuda") - 0.5) * 6.0  # +-3 px
        outs = torch.empty((nsets, h, w), dtype=torch.uint8, device="cuda")
        out = {"buffer_sets": nsets}
        for grow in (0, 1, 4):
            work = torch.empty(max(ops.trimap_propagate_workspace_bytes(h, w, grow), 1), dtype=torch.uint8, device="cuda")
            ms = graph_ms([lambda i=i: ops.trimap_propagate(tri[i], flow[i], grow, out=outs[i], work=work)
                           for i in range(nsets)], a.reps)
            bpp = propagate_bytes_per_pixel(grow)
            out["trimap_propagate_grow%d" % grow] = dict(rate(hw * bpp, ms), us=round(ms * 1e3, 2), bytes_per_pixel=bpp)
        # the HBM yardstick on this box: a torch copy of 265 MB (tools/membw.py's "copy")
        m = 1080 * 1920 * 64
        x, y = torch.empty(m, dtype=torch.bfloat16, device="cuda"), torch.empty(m, dtype=torch.bfloat16, device="cuda")
        ms = event_ms([lambda: y.copy_(x)], a.reps)
        out["torch_copy_265MB"] = rate(4 * m, ms)
        return out
    res["kernels"] = step("propagate kernels %dx%d" % (h, w), a.step_limit, kernels)
    torch.cuda.empty_cache()

    def estimator():
        # what flow="estimate" adds per frame: one pyramid and one flow between two pyramids
        o = ops.FLOW_DEFAULTS
        frames = torch.randint(0, 256, (2, h, w, 3), generator=g, device="cuda", dtype=torch.uint8)
        floats = ops.flow_pyramid_floats(h, w, o["levels"])
        pyr = torch.zeros((2, (floats + 3) // 4 * 4), dtype=torch.float32, device="cuda")
        work = torch.zeros(ops.flow_workspace_bytes(h, w, o["levels"]), dtype=torch.uint8, device="cuda")
        bw = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
        ops.flow_pyramid(frames[0], o["levels"], out=pyr[0], work=work)

        def call():
            ops.flow_pyramid(frames[1], o["levels"], out=pyr[1], work=work)
            ops.flow_from_pyramids(pyr[1], pyr[0], h, w, o["levels"], o["warps"], o["iters"], o["alpha"], out=bw,
                                   work=work)
        return {"estimator_cost_ms_per_frame": round(graph_ms([call], a.reps, calls=20), 3)}
    res.update(step("propagate estimator %dx%d" % (h, w), a.step_limit, estimator))

    np.random.seed(0)
    model = unet.UNetVideo(synthetic_vgg16(0), dtype="bf16", device="cuda").prepare()

    def streamed():
        rs = np.random.RandomState(1)
        k = min(F, 2 * n)  # two distinct chunks of host frames, cycled (the source hands out views of them)
        cmp, bg = (rs.randint(0, 256, (k, h, w, 3), dtype=np.uint8) for _ in range(2))
        tri = rs.choice(np.array([0, 128, 255], np.uint8), (k, h, w))
        bw = rs.uniform(-3, 3, (k, h, w, 2)).astype(np.float32)

        def source(mode):
            for i in range(0, F, n):
                m = min(n, F - i)
                o = i % k
                if mode == "per_frame":
                    yield cmp[o:o + m], bg[o:o + m], tri[o:o + m]
                else:
                    yield cmp[o:o + m], bg[o:o + m], (tri[0] if i == 0 else None), (bw[o:o + m] if mode == "given" else None)
        kw = dict(chunk=n, depth=2, out="u8")
        streams = {"per_frame": FrameStream(model, h, w, **kw),
                   "given": FrameStream(model, h, w, trimap="propagate", flow="given", **kw),
                   "estimate": FrameStream(model, h, w, trimap="propagate", flow="estimate", **kw)}

        def run(mode):
            t0 = time.perf_counter()
            tot = sum(m.shape[0] for m in streams[mode].run(source(mode)))
            torch.cuda.synchronize()
            assert tot == F
            return (time.perf_counter() - t0) * 1e3
        times = {mode: [] for mode in streams}
        for i in range(1 + max(3, a.reps // 2)):  # interleaved; round 0 warms up (and captures the graphs)
            for mode in streams:
                ms = run(mode)
                if i:
                    times[mode].append(ms)
        out = {}
        for mode, t in times.items():
            ms = statistics.median(t)
            name = "frame_stream_bf16_" + ("trimap_per_frame" if mode == "per_frame" else "propagate_" + mode)
            out[name] = {"ms_per_frame": round(ms / F, 3), "frames_per_s": round(F / ms * 1e3, 1),
                         "min_ms_per_frame": round(min(t) / F, 3), "max_ms_per_frame": round(max(t) / F, 3)}
        base = out["frame_stream_bf16_trimap_per_frame"]["ms_per_frame"]
        for mode in ("given", "estimate"):
            out["propagate_%s_adds_ms_per_frame" % mode] = round(
                out["frame_stream_bf16_propagate_" + mode]["ms_per_frame"] - base, 3)
        return out
    res.update(step("propagate streams %dx%d" % (h, w), a.step_limit, streamed))

    def link():
        """What each mode stages and uploads per frame (7 B per pixel with per-frame trimaps, 14 B with given flows, 6 B
        with estimated ones): the host's copy into pinned memory, which is serial host work, and the upload."""
        out = {}
        for name, nbytes in (("per_frame_7B", 7), ("given_14B", 14), ("estimate_6B", 6)):
            hb = torch.empty(n * hw * nbytes, dtype=torch.uint8).pin_memory()
            db = torch.empty(n * hw * nbytes, dtype=torch.uint8, device="cuda")
            ms = event_ms([lambda: db.copy_(hb, non_blocking=True)], a.reps)
            out["h2d_pinned_" + name] = {"ms_per_frame": round(ms / n, 3), "GBps": round(n * hw * nbytes / ms / 1e6, 1)}
            src = np.frombuffer(np.random.RandomState(2).bytes(hb.numel()), np.uint8)
            t0 = time.perf_counter()
            for _ in range(3):
                hb.numpy()[...] = src
            ms = (time.perf_counter() - t0) / 3 * 1e3
            out["host_copy_" + name] = {"ms_per_frame": round(ms / n, 3), "GBps": round(n * hw * nbytes / ms / 1e6, 1)}
        return out
    res["link"] = step("propagate link %dx%d" % (h, w), a.step_limit, link)
    del model
    torch.cuda.empty_cache()
    return res


def propagate_section(a):
    res = {"chunk": a.chunk, "frames": a.frames, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "hbm_peak_GBps": HBM_PEAK / 1e9, "grow_of_streams": 1, "sizes": {}}
    for size in a.propagate_sizes.split(","):
        h, w = (int(v) for v in size.split("x"))
        res["sizes"][size] = propagate_size(a, h, w)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.propagate_out), exist_ok=True)
    with open(a.propagate_out, "w") as f:
        f.write(line + "\n")
    print(line)


AUTO_BYTES_PER_PIXEL = 6 + 1 + 0.5  # cmp and bg read, the trimap written, the bit rows written and read back


def torch_plate(cmp, bg, lo, hi, r_bg, r_fg):
    """vm_trimap_from_plate's definition in torch ops on the device.  d <= 3 * 255^2 and its box sum < 2^24, so f32
    holds them exactly; max_pool2d pads with -inf, which is a window clipped to the image."""
    F = torch.nn.functional
    q = cmp.float() - bg.float()
    d = (q * q).sum(-1)[:, None]
    D = F.avg_pool2d(F.pad(d, (1, 1, 1, 1), mode="replicate"), 3, stride=1, divisor_override=1)
    def erode(m, r):  # (the square window as a row pass and a column pass: 2 (2 r + 1) taps, not (2 r + 1)^2)
        if r == 0:
            return m
        rows = F.max_pool2d(-m, (1, 2 * r + 1), stride=1, padding=(0, r))
        return -F.max_pool2d(rows, (2 * r + 1, 1), stride=1, padding=(r, 0))
    back = erode((D <= 9 * lo * lo).float(), r_bg) > 0
    fore = erode((D >= 9 * hi * hi).float(), r_fg) > 0
    out = torch.full(D.shape, 128, dtype=torch.uint8, device=cmp.device)
    out[back] = 0
    out[fore] = 255
    return out[:, 0]


def auto_section(a):
    """vm_trimap_from_plate at [1 | chunk, height, width] for three radius pairs against its bytes model, the torch route
    to the same bytes, and FrameStream(trimap="auto") beside trimap=True on the same frames, interleaved."""
    from vmatting import FrameStream, ops, unet
    from vmatting.weights import synthetic_vgg16
    h, w, F = a.height, a.width, a.frames
    hw = h * w
    res = {"height": h, "width": w, "chunk": a.chunk, "frames": F, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "hbm_peak_GBps": HBM_PEAK / 1e9,
           "bytes_per_pixel": AUTO_BYTES_PER_PIXEL, "defaults": dict(ops.PLATE_DEFAULTS)}
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    o = ops.PLATE_DEFAULTS
    radii = {"r0_0": (0, 0), "defaults": (o["r_bg"], o["r_fg"]), "r32_32": (32, 32)}

    def frames(n, nsets):
        """Plates of coarse blocks, and frames that equal them but for a little noise and a band of another colour: every
        label occurs, in regions wider than the erosion windows."""
        bg = torch.randint(0, 256, (nsets, n, (h + 63) // 64, (w + 63) // 64, 3), generator=g, device="cuda",
                           dtype=torch.uint8).repeat_interleave(64, 2).repeat_interleave(64, 3)[:, :, :h, :w].contiguous()
        cmp = bg ^ torch.randint(0, 4, bg.shape, generator=g, device="cuda", dtype=torch.uint8)
        cmp[:, :, h // 4:3 * h // 4, w // 3:2 * w // 3] ^= 0x80
        return cmp, bg

    def kernels():
        out = {}
        for n in (1, a.chunk):
            # enough buffer sets that one round of calls streams more than the 256 MB memory-side cache
            nsets = max(a.sets, int(300e6 / (AUTO_BYTES_PER_PIXEL * n * hw)) + 1)
            cmp, bg = frames(n, nsets)
            outs = torch.empty((nsets, n, h, w), dtype=torch.uint8, device="cuda")
            work = torch.empty(ops.trimap_from_plate_workspace_bytes(n, h, w), dtype=torch.uint8, device="cuda")
            per = {"buffer_sets": nsets}
            for name, (r_bg, r_fg) in radii.items():
                call = lambda i, r_bg=r_bg, r_fg=r_fg: ops.trimap_from_plate(  # noqa: E731
                    cmp[i], bg[i], o["lo"], o["hi"], r_bg, r_fg, out=outs[i], work=work)
                ms = graph_ms([lambda i=i: call(i) for i in range(nsets)], a.reps, calls=200)
                per[name] = dict(rate(n * hw * AUTO_BYTES_PER_PIXEL, ms), us=round(ms * 1e3, 2))
                want = torch_plate(cmp[0], bg[0], o["lo"], o["hi"], r_bg, r_fg)
                assert torch.equal(call(0), want), (n, name)  # the same bytes, so the same work is compared
                per[name]["label_shares"] = [round(float((want == v).float().mean()), 3) for v in (0, 128, 255)]
                ms_t = event_ms([lambda i=i: torch_plate(cmp[i], bg[i], o["lo"], o["hi"], r_bg, r_fg)
                                 for i in range(min(nsets, 3))], a.reps)
                per[name]["torch_route_ms"] = round(ms_t, 4)
                per[name]["speedup_over_torch"] = round(ms_t / ms, 1)
            # one static plate for all n frames
            ms = graph_ms([lambda i=i: ops.trimap_from_plate(cmp[i], bg[i, 0], out=outs[i], work=work)
                           for i in range(nsets)], a.reps, calls=200)
            per["defaults_static_bg"] = dict(rate(n * hw * (AUTO_BYTES_PER_PIXEL - 3) + hw * 3, ms), us=round(ms * 1e3, 2))
            out["n%d" % n] = per
            del cmp, bg, outs, work
            torch.cuda.empty_cache()
        # the HBM yardstick on this box: a torch copy of 265 MB (tools/membw.py's "copy")
        m = 1080 * 1920 * 64
        x, y = torch.empty(m, dtype=torch.bfloat16, device="cuda"), torch.empty(m, dtype=torch.bfloat16, device="cuda")
        out["torch_copy_265MB"] = rate(4 * m, event_ms([lambda: y.copy_(x)], a.reps))
        return out
    res["kernels"] = step("auto kernels", a.step_limit, kernels)
    torch.cuda.empty_cache()

    np.random.seed(0)
    model = unet.UNetVideo(synthetic_vgg16(0), dtype="bf16", device="cuda").prepare()

    def streamed():
        n = a.chunk
        k = min(F, 2 * n)  # two distinct chunks of host frames, cycled (the source hands out views of them)
        cmp, bg = (t[0].cpu().numpy() for t in frames(k, 1))
        tri = ops.trimap_from_plate(torch.from_numpy(cmp).cuda(), torch.from_numpy(bg).cuda()).cpu().numpy()
        torch.cuda.empty_cache()

        def source(mode):
            for i in range(0, F, n):
                m, s = min(n, F - i), i % k
                yield cmp[s:s + m], bg[s:s + m], (tri[s:s + m] if mode == "per_frame" else None)
        kw = dict(chunk=n, depth=2, out="u8")
        streams = {"per_frame": FrameStream(model, h, w, **kw), "auto": FrameStream(model, h, w, trimap="auto", **kw)}

        def run(mode):
            t0 = time.perf_counter()
            tot = sum(m.shape[0] for m in streams[mode].run(source(mode)))
            torch.cuda.synchronize()
            assert tot == F
            return (time.perf_counter() - t0) * 1e3
        times = {mode: [] for mode in streams}
        for i in range(1 + max(3, a.reps // 2)):  # interleaved; round 0 warms up (and captures the graphs)
            for mode in streams:
                ms = run(mode)
                if i:
                    times[mode].append(ms)
        out = {}
        for mode, t in times.items():
            ms = statistics.median(t)
            out["frame_stream_bf16_trimap_" + mode] = {
                "ms_per_frame": round(ms / F, 3), "frames_per_s": round(F / ms * 1e3, 1),
                "min_ms_per_frame": round(min(t) / F, 3), "max_ms_per_frame": round(max(t) / F, 3)}
        out["auto_adds_ms_per_frame"] = round(out["frame_stream_bf16_trimap_auto"]["ms_per_frame"] -
                                              out["frame_stream_bf16_trimap_per_frame"]["ms_per_frame"], 3)
        return out
    res["streams"] = step("auto streams", a.step_limit, streamed)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.auto_out), exist_ok=True)
    with open(a.auto_out, "w") as f:
        f.write(line + "\n")
    print(line)
    del model
    torch.cuda.empty_cache()
    shadow_leg(a)


def spread(times, per=1):
    """Median, min and max of a list of times, each divided by ``per``."""
    return {"median": round(statistics.median(times) / per, 4), "min": round(min(times) / per, 4),
            "max": round(max(times) / per, 4), "runs": len(times)}


def shadow_leg(a):
    """The shadow-tolerant distance beside the plain one (``--sections shadow`` runs this leg alone):
    ops.trimap_from_plate at [1 | chunk, height, width] with the defaults, plain and with shadow=SHADOW_DEFAULTS in turn,
    round by round in one run, and FrameStream(trimap="auto") with and without shadow="chroma", interleaved."""
    from vmatting import FrameStream, ops, unet
    from vmatting.weights import synthetic_vgg16
    h, w, F = a.height, a.width, a.frames
    hw = h * w
    res = {"height": h, "width": w, "chunk": a.chunk, "frames": F, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "bytes_per_pixel": AUTO_BYTES_PER_PIXEL,
           "defaults": dict(ops.PLATE_DEFAULTS), "shadow_defaults": dict(ops.SHADOW_DEFAULTS)}
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    modes = {"plain": None, "shadow": dict(ops.SHADOW_DEFAULTS)}

    def frames(n, nsets):
        """auto_section's frames with the lower left third of every frame at 0.7 of its light: a shadow that the plain
        distance calls a difference and the shadow distance does not."""
        bg = torch.randint(32, 256, (nsets, n, (h + 63) // 64, (w + 63) // 64, 3), generator=g, device="cuda",
                           dtype=torch.uint8).repeat_interleave(64, 2).repeat_interleave(64, 3)[:, :, :h, :w].contiguous()
        cmp = bg ^ torch.randint(0, 4, bg.shape, generator=g, device="cuda", dtype=torch.uint8)
        cmp[:, :, h // 4:3 * h // 4, w // 3:2 * w // 3] ^= 0x80
        cmp[:, :, h // 2:, :w // 3] = (cmp[:, :, h // 2:, :w // 3].float() * 0.7).round().to(torch.uint8)
        return cmp, bg

    def kernels():
        out = {}
        for n in (1, a.chunk):
            nsets = max(a.sets, int(300e6 / (AUTO_BYTES_PER_PIXEL * n * hw)) + 1)
            cmp, bg = frames(n, nsets)
            outs = torch.empty((nsets, n, h, w), dtype=torch.uint8, device="cuda")
            work = torch.empty(ops.trimap_from_plate_workspace_bytes(n, h, w), dtype=torch.uint8, device="cuda")
            times = {mode: [] for mode in modes}
            for _ in range(5):  # the two calls in turn, five rounds
                for mode, shadow in modes.items():
                    times[mode].append(graph_ms([lambda i=i: ops.trimap_from_plate(cmp[i], bg[i], out=outs[i], work=work,
                                                                                   shadow=shadow)
                                                 for i in range(nsets)], a.reps, calls=200))
            per = {"buffer_sets": nsets}
            for mode, shadow in modes.items():
                tri = ops.trimap_from_plate(cmp[0], bg[0], shadow=shadow)
                per[mode] = dict(rate(n * hw * AUTO_BYTES_PER_PIXEL, statistics.median(times[mode])), ms_spread=spread(times[mode]),
                                 label_shares=[round(float((tri == v).float().mean()), 3) for v in (0, 128, 255)])
            per["shadow_over_plain"] = round(per["shadow"]["ms"] / per["plain"]["ms"], 3)
            out["n%d" % n] = per
            del cmp, bg, outs, work
            torch.cuda.empty_cache()
        return out
    res["kernels"] = step("shadow kernels", a.step_limit, kernels)
    torch.cuda.empty_cache()

    np.random.seed(0)
    model = unet.UNetVideo(synthetic_vgg16(0), dtype="bf16", device="cuda").prepare()

    def streamed():
        n = a.chunk
        k = min(F, 2 * n)
        cmp, bg = (t[0].cpu().numpy() for t in frames(k, 1))
        torch.cuda.empty_cache()

        def source():
            for i in range(0, F, n):
                m, s = min(n, F - i), i % k
                yield cmp[s:s + m], bg[s:s + m], None
        kw = dict(chunk=n, depth=2, out="u8", trimap="auto")
        streams = {"auto": FrameStream(model, h, w, **kw), "auto_shadow": FrameStream(model, h, w, shadow="chroma", **kw)}

        def run(mode):
            t0 = time.perf_counter()
            tot = sum(m.shape[0] for m in streams[mode].run(source()))
            torch.cuda.synchronize()
            assert tot == F
            return (time.perf_counter() - t0) * 1e3
        times = {mode: [] for mode in streams}
        for i in range(1 + max(3, a.reps // 2)):  # interleaved; round 0 warms up (and captures the graphs)
            for mode in streams:
                ms = run(mode)
                if i:
                    times[mode].append(ms)
        out = {"frame_stream_bf16_trimap_" + mode: {"ms_per_frame": spread(t, F)} for mode, t in times.items()}
        out["shadow_adds_ms_per_frame"] = round(out["frame_stream_bf16_trimap_auto_shadow"]["ms_per_frame"]["median"] -
                                                out["frame_stream_bf16_trimap_auto"]["ms_per_frame"]["median"], 4)
        return out
    res["streams"] = step("shadow streams", a.step_limit, streamed)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.shadow_out), exist_ok=True)
    with open(a.shadow_out, "w") as f:
        f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sets", type=int, default=3, help="buffer sets the kernel timings cycle through")
    ap.add_argument("--step-limit", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ingest_stream.json"))
    ap.add_argument("--compose-out", default=os.path.join(REPO, "profiles", "compose_stream.json"))
    ap.add_argument("--propagate-out", default=os.path.join(REPO, "profiles", "trimap_propagate.json"))
    ap.add_argument("--propagate-sizes", default="500x1200,1080x1920", help="comma-separated HxW of the propagate section")
    ap.add_argument("--auto-out", default=os.path.join(REPO, "profiles", "trimap_auto.json"))
    ap.add_argument("--shadow-out", default=os.path.join(REPO, "profiles", "plate_shadow.json"))
    ap.add_argument("--sections", default="ingest,compose",
                    help="comma-separated: ingest, compose, propagate, auto, shadow (the auto section's last leg alone)")
    a = ap.parse_args()
    sections = set(a.sections.split(","))
    if not sections or sections - {"ingest", "compose", "propagate", "auto", "shadow"}:
        raise SystemExit("stream_bench: --sections takes ingest, compose, propagate, auto and / or shadow, got %r" %
                         a.sections)
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench needs a ROCm GPU")
    if "ingest" in sections:
        ingest_section(a)
        torch.cuda.empty_cache()
    if "compose" in sections:
        compose_section(a)
        torch.cuda.empty_cache()
    if "propagate" in sections:
        propagate_section(a)
        torch.cuda.empty_cache()
    if "auto" in sections:
        auto_section(a)
    elif "shadow" in sections:
        shadow_leg(a)


def ingest_section(a):
    from vmatting import FrameStream, ops, unet, video
    from vmatting.weights import synthetic_vgg16
    n, h, w, F = a.chunk, a.height, a.width, a.frames
    px = n * h * w
    res = {"shape": [n, h, w], "frames": F, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "hbm_peak_GBps": HBM_PEAK / 1e9}
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    sets = []
    for _ in range(a.sets):
        sets.append(dict(cmp=torch.randint(0, 256, (n, h, w, 3), generator=g, device="cuda", dtype=torch.uint8),
                         bg=torch.randint(0, 256, (n, h, w, 3), generator=g, device="cuda", dtype=torch.uint8),
                         tri=torch.randint(0, 256, (n, h, w), generator=g, device="cuda", dtype=torch.uint8),
                         alpha=torch.rand((n, h, w, 1), generator=g, device="cuda")))

    # ---- the kernels
    def kernels():
        out = {}
        f32 = [torch.empty((n, h, w, 7), dtype=torch.float32, device="cuda") for _ in sets]
        ms = event_ms([lambda s=s, o=o: ops.frames_from_u8(s["cmp"], s["bg"], s["tri"], out=o)
                       for s, o in zip(sets, f32)], a.reps)
        out["frames_from_u8_f32_c7"] = rate(px * (7 + 28), ms)
        ms = event_ms([lambda s=s, o=o: ops.frames_from_u8(s["cmp"], s["bg"][0], s["tri"], out=o)
                       for s, o in zip(sets, f32)], a.reps)
        out["frames_from_u8_f32_c7_static_bg"] = rate(px * (4 + 28) + h * w * 3, ms)
        # the parent commit's only route to the same f32 frames: torch ops on the device
        mean = torch.tensor(VGG_MEAN, dtype=torch.float64, device="cuda")

        def torch_route(s):
            return torch.cat([(s["cmp"].double() - mean).float(), (s["bg"].double() - mean).float(),
                              (s["tri"].double() / 255.0 - 0.5).float()[..., None]], -1)
        # the same values, so the same work is compared
        assert torch.equal(torch_route(sets[0]), ops.frames_from_u8(sets[0]["cmp"], sets[0]["bg"], sets[0]["tri"]))
        ms_t = event_ms([lambda s=s: torch_route(s) for s in sets], a.reps)
        out["torch_route_f32_c7"] = {"ms": round(ms_t, 4)}
        out["ingest_speedup_over_torch"] = round(ms_t / out["frames_from_u8_f32_c7"]["ms"], 2)
        del f32
        b16 = [torch.empty((n, h, w, 8), dtype=torch.bfloat16, device="cuda")[..., :7] for _ in sets]
        ms = event_ms([lambda s=s, o=o: ops.frames_from_u8(s["cmp"], s["bg"], s["tri"], out=o)
                       for s, o in zip(sets, b16)], a.reps)
        out["frames_from_u8_bf16x8"] = rate(px * (7 + 16), ms)
        del b16
        for bits in (8, 16):
            q = [torch.empty((n, h, w), dtype=torch.uint8 if bits == 8 else torch.uint16, device="cuda") for _ in sets]
            ms = event_ms([lambda s=s, o=o: ops.matte_quantize(s["alpha"], out=o, bits=bits)
                           for s, o in zip(sets, q)], a.reps)
            out["matte_quantize_u%d" % bits] = rate(px * (4 + bits // 8), ms)
        return out
    res.update(step("kernels", a.step_limit, kernels))

    # ---- the host link: one uint8 chunk (cmp + bg + trimap = 7 B per pixel) from pinned memory, one matte back
    def link():
        hc = [torch.empty(s, dtype=torch.uint8).pin_memory() for s in ((n, h, w, 3), (n, h, w, 3), (n, h, w))]
        dc = [sets[0]["cmp"], sets[0]["bg"], sets[0]["tri"]]
        ms_up = event_ms([lambda: [d.copy_(s, non_blocking=True) for d, s in zip(dc, hc)]], a.reps)
        hq, dq = torch.empty((n, h, w), dtype=torch.uint8).pin_memory(), torch.empty((n, h, w), dtype=torch.uint8,
                                                                                     device="cuda")
        ms_dn = event_ms([lambda: hq.copy_(dq, non_blocking=True)], a.reps)
        src = [np.frombuffer(np.random.RandomState(2).bytes(t.numel()), np.uint8).reshape(tuple(t.shape)) for t in hc]
        t0 = time.perf_counter()
        for _ in range(3):
            for s, t in zip(src, hc):
                t.numpy()[...] = s
        ms_host = (time.perf_counter() - t0) / 3 * 1e3
        return {"h2d_pinned_u8_chunk": {"ms": round(ms_up, 3), "GBps": round(px * 7 / ms_up / 1e6, 1)},
                "d2h_pinned_u8_matte": {"ms": round(ms_dn, 3), "GBps": round(px / ms_dn / 1e6, 1)},
                "host_copy_into_pinned": {"ms": round(ms_host, 3), "GBps": round(px * 7 / ms_host / 1e6, 1)}}
    res.update(step("link", a.step_limit, link))
    del sets
    torch.cuda.empty_cache()

    # ---- the pipeline: FrameStream (bf16, u8 mattes, depth 2) beside VideoMatter.run() on resident f32 frames
    np.random.seed(0)
    model = unet.UNetVideo(synthetic_vgg16(0), dtype="bf16", device="cuda").prepare()

    def resident():
        frames = video.synthetic_frames(F, h, w)
        vm = video.VideoMatter(model, frames, chunk=n)
        ms = event_ms([vm.run], max(3, a.reps // 2), warmup=2)
        return {"video_matter_resident_f32": {"ms": round(ms, 2), "frames_per_s": round(F / ms * 1e3, 1)}}
    res.update(step("resident", a.step_limit, resident))
    torch.cuda.empty_cache()

    def streamed():
        rs = np.random.RandomState(1)
        k = min(F, 2 * n)  # two distinct chunks of host frames, cycled (the source hands out views of them)
        cmp, bg = (rs.randint(0, 256, (k, h, w, 3), dtype=np.uint8) for _ in range(2))
        tri = rs.choice(np.array([0, 128, 255], np.uint8), (k, h, w))

        def source():
            for i in range(0, F, n):
                m = min(n, F - i)
                o = i % k
                yield cmp[o:o + m], bg[o:o + m], tri[o:o + m]
        fs = FrameStream(model, h, w, chunk=n, depth=2, out="u8")

        def run():
            t0 = time.perf_counter()
            tot = sum(m.shape[0] for m in fs.run(source()))
            torch.cuda.synchronize()
            assert tot == F
            return (time.perf_counter() - t0) * 1e3
        run()
        ms = statistics.median(run() for _ in range(max(3, a.reps // 2)))
        return {"frame_stream_bf16_u8_depth2": {"ms": round(ms, 2), "frames_per_s": round(F / ms * 1e3, 1)}}
    res.update(step("streamed", a.step_limit, streamed))

    # ---- which leg bounds the stream: per chunk, upload vs compute vs download (device legs overlap across slots),
    # and the host's own serial work per chunk (the copy into pinned memory + the copy of the matte out of it)
    per_chunk = res["video_matter_resident_f32"]["ms"] * n / F
    legs = {"upload": res["h2d_pinned_u8_chunk"]["ms"],
            "compute": round(per_chunk + res["frames_from_u8_bf16x8"]["ms"] + res["matte_quantize_u8"]["ms"], 3),
            "download": res["d2h_pinned_u8_matte"]["ms"],
            "host_copy": res["host_copy_into_pinned"]["ms"]}
    res["legs_ms_per_chunk"] = legs
    res["bounding_leg"] = max(legs, key=legs.get)
    res["stream_keeps_of_resident"] = round(res["frame_stream_bf16_u8_depth2"]["frames_per_s"] /
                                            res["video_matter_resident_f32"]["frames_per_s"], 3)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
