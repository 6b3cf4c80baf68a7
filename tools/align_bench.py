#!/usr/bin/env python
"""Times the plate's position match at 1080 x 1920 and writes profiles/plate_align.json.

Kernels, at ``--chunk`` frames per call against one static plate, as FrameStream(align="fit") runs them: the frames'
grey pyramids (ops.flow_pyramid per frame: what the alignment pays unless a flow estimate makes them anyway),
ops.plate_align_fit at the defaults, and ops.plate_align_apply.  The frames are a smooth texture seen through a known
shift of (1.5, j) pixels behind a block of noise, so the fit has something to find and the timed calls' results are
checked against it.  Every timed window runs the call on each of ``--sets`` buffer sets in turn; times are hipEvent
medians after a warm-up, per call and per frame.

Accuracy: the device fit on the scenes of tests/plate_align_ref.py at 96 x 160 (every motion x gain x three seeds): the
largest corner error against the true map, and the largest difference to the numpy restatement's map.

Streams: bf16 UNetVideo (synthetic weights), chunk 8, depth 2, out="u8", interleaved run by run: the static plate
as it is (call for call the stream without the feature), with align="fit", with align and gain="fit", with
smooth="flow" alone, and with align and smooth="flow" (the alignment then reads the flow estimate's pyramids).

Each step runs under its own wall-clock limit (--step-limit seconds)."""

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "video-matting_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from upscale_bench import step, window_ms  # noqa: E402  (the windows and the step limit of the §3.4k table)


def texture(h, w, gen):
    """A smooth uint8 [h,w,3] texture on the device: blurred noise plus a low-frequency term, 30..225."""
    import torch.nn.functional as fn
    fine = torch.rand((1, 3, h, w), generator=gen, device="cuda")
    for _ in range(3):
        fine = fn.avg_pool2d(fn.pad(fine, (1, 1, 1, 1), mode="replicate"), 3, 1)
    low = fn.interpolate(torch.rand((1, 3, h // 32 + 2, w // 32 + 2), generator=gen, device="cuda"), size=(h, w),
                         mode="bilinear", align_corners=False)
    t = (fine - fine.mean()) / fine.std() + 1.5 * (low - low.mean()) / low.std()
    t = 30 + 195 * (t - t.min()) / (t.max() - t.min())
    return t[0].permute(1, 2, 0).round().to(torch.uint8).contiguous()


def moved(plate, j, gen):
    """The plate seen through a shift of (1.5, j) pixels, with a block of noise over a sixth of it."""
    p = plate.to(torch.float32)
    f = 0.5 * (torch.roll(p, (-j, -1), (0, 1)) + torch.roll(p, (-j, -2), (0, 1)))
    h, w, _ = plate.shape
    y0, y1, x0, x1 = h // 4, 3 * h // 4, w // 3, 2 * w // 3
    f[y0:y1, x0:x1] = torch.rand((y1 - y0, x1 - x0, 3), generator=gen, device="cuda") * 255
    return f.round().to(torch.uint8)


def median_ms(fns, reps, warmup=3):
    for _ in range(warmup):
        window_ms(fns)
    torch.cuda.synchronize()
    t = [window_ms(fns) for _ in range(reps)]
    return statistics.median(t), min(t), max(t)


def kernels(a):
    from vmatting import ops
    n, h, w, levels = a.chunk, a.height, a.width, ops.ALIGN_DEFAULTS["levels"]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    plates = [texture(h, w, gen) for _ in range(a.sets)]
    frames = [torch.stack([moved(p, j % 4, gen) for j in range(n)]) for p in plates]
    floats = (ops.flow_pyramid_floats(h, w, levels) + 3) // 4 * 4
    rows = [torch.zeros((n, floats), dtype=torch.float32, device="cuda") for _ in range(a.sets)]
    bg_rows = [torch.zeros((1, floats), dtype=torch.float32, device="cuda") for _ in range(a.sets)]
    pwork = torch.zeros(ops.flow_workspace_bytes(h, w, levels), dtype=torch.uint8, device="cuda")
    work = torch.zeros(ops.plate_align_workspace_bytes(n, h, w, levels), dtype=torch.uint8, device="cuda")
    prm = [torch.zeros((n, 8), dtype=torch.float32, device="cuda") for _ in range(a.sets)]
    sup = [torch.zeros((n,), dtype=torch.int32, device="cuda") for _ in range(a.sets)]
    out = [torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(a.sets)]
    for i in range(a.sets):
        ops.frame_pyramids(plates[i][None], levels, bg_rows[i], pwork)
    calls = {
        "pyramids": [lambda i=i: ops.frame_pyramids(frames[i], levels, rows[i], pwork) for i in range(a.sets)],
        "fit": [lambda i=i: ops.plate_align_fit(rows[i], bg_rows[i], h, w, out=prm[i], support=sup[i], work=work)
                for i in range(a.sets)],
        "apply": [lambda i=i: ops.plate_align_apply(plates[i], prm[i], out=out[i]) for i in range(a.sets)],
    }
    res = {}
    for name, fns in calls.items():
        ms, lo, hi = median_ms(fns, a.reps)
        res[name] = {"ms_per_call": round(ms, 4), "ms_per_frame": round(ms / n, 4), "min_ms": round(lo, 4),
                     "max_ms": round(hi, 4)}
        print("# %-10s %.4f ms per call of %d frames, %.4f per frame" % (name, ms, n, ms / n), file=sys.stderr)
    res["fit_plus_apply_ms_per_frame"] = round(res["fit"]["ms_per_frame"] + res["apply"]["ms_per_frame"], 4)
    res["with_pyramids_ms_per_frame"] = round(res["fit_plus_apply_ms_per_frame"] + res["pyramids"]["ms_per_frame"], 4)
    res["fit_launches"] = 1 + 2 * ops.ALIGN_DEFAULTS["iters"] * levels
    p = prm[0].cpu().numpy()
    res["fits_seen"] = {"shift_x_true": 1.5, "shift_y_true": [j % 4 for j in range(n)],
                        "shift_x": np.round(p[:, 2].astype(np.float64), 3).tolist(),
                        "shift_y": np.round(p[:, 5].astype(np.float64), 3).tolist(),
                        "support_share": np.round(sup[0].cpu().numpy() / (h * w), 3).tolist()}
    return res


def accuracy(a):
    import plate_align_ref as ref
    from vmatting import reader
    h, w = 96, 160
    worst_err = worst_diff = 0.0
    cases = 0
    for m in ref.MOTIONS:
        for g in ref.GAINS:
            for seed in range(3):
                frame, plate, _, true = ref.scene(h, w, m, g, seed)
                want, _ = ref.fit_frames(frame, plate)
                _, got, _ = reader.align_plate(frame, plate)
                got = np.concatenate([got, [0]]).astype(np.float32)
                worst_err = max(worst_err, ref.corner_error(got, true, h, w))
                worst_diff = max(worst_diff, ref.corner_error(got, want, h, w))
                cases += 1
    return {"shape": [h, w], "cases": cases, "worst_corner_error_px": round(worst_err, 4),
            "worst_device_minus_restatement_px": worst_diff}


def streams(a):
    from vmatting import FrameStream, unet
    from vmatting.weights import synthetic_vgg16
    n, F, h, w = a.chunk, a.frames, a.height, a.width
    np.random.seed(0)
    model = unet.UNetVideo(synthetic_vgg16(0), dtype="bf16", device="cuda").prepare()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    k = min(F, 2 * n)  # two distinct chunks of host frames, cycled
    d_plate = texture(h, w, gen)
    plate = d_plate.cpu().numpy()
    cmp = torch.stack([moved(d_plate, j % 4, gen) for j in range(k)]).cpu().numpy()
    tri = np.full((k, h, w), 128, np.uint8)
    tri[:, :h // 8] = 0
    tri[:, 3 * h // 8:5 * h // 8, 5 * w // 12:7 * w // 12] = 255
    plan = {"plain": dict(), "align": dict(align="fit"), "align_gain": dict(align="fit", gain="fit"),
            "smooth": dict(smooth="flow"), "align_smooth": dict(align="fit", smooth="flow")}
    made = {name: FrameStream(model, h, w, chunk=n, depth=2, out="u8", static_bg=plate, **kw) for name, kw in plan.items()}

    def run(name):
        src = ((cmp[i % k:i % k + min(n, F - i)], None, tri[i % k:i % k + min(n, F - i)]) for i in range(0, F, n))
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
    for name, base in (("align", "plain"), ("align_gain", "plain"), ("align_smooth", "smooth")):
        out[name]["over_" + base + "_ms_per_frame"] = round(out[name]["ms_per_frame"] - out[base]["ms_per_frame"], 3)
    params, support = made["align"].last_alignment()
    out["last_alignment"] = {"shift_x": np.round(params[:, 2].astype(np.float64), 3).tolist(),
                             "shift_y": np.round(params[:, 5].astype(np.float64), 3).tolist(),
                             "support_share": np.round(support / (h * w), 3).tolist()}
    out["shared_pyramids"] = made["align_smooth"]._align_rows is None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--frames", type=int, default=32, help="frames per stream run")
    ap.add_argument("--sets", type=int, default=4, help="buffer sets taken in turn")
    ap.add_argument("--reps", type=int, default=10, help="timed windows per kernel")
    ap.add_argument("--rounds", type=int, default=3, help="timed runs per stream")
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--skip-streams", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "plate_align.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("align_bench: needs a ROCm GPU (no figure is produced without one)")
    from vmatting import ops
    doc = {"device": torch.cuda.get_device_name(0),
           "measured_utc": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "shape": [a.chunk, a.height, a.width],
           "sets": a.sets, "reps": a.reps, "timing": "hipEvent median per call",
           "defaults": dict(ops.ALIGN_DEFAULTS), "model": "UNetVideo bf16, synthetic weights"}
    doc["kernels"] = step("kernels", a.step_limit, lambda: kernels(a))
    doc["accuracy"] = step("accuracy", a.step_limit, lambda: accuracy(a))
    torch.cuda.empty_cache()
    if not a.skip_streams:
        doc["streams"] = step("streams", a.step_limit, lambda: streams(a))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"plate_align": {"kernels_ms_per_frame": {k: v["ms_per_frame"] for k, v in doc["kernels"].items()
                                                               if isinstance(v, dict) and "ms_per_frame" in v},
                                      "accuracy": doc["accuracy"],
                                      "streams": {k: v.get("ms_per_frame", v) if isinstance(v, dict) else v
                                                  for k, v in doc.get("streams", {}).items()}}}))


if __name__ == "__main__":
    main()
