#!/usr/bin/env python
"""Times ops.matte_score at 1080p, 8 frames per call, against the same statistics written with torch ops, and writes
profiles/matte_score.json.

Six combinations: with / without a trimap, times
  frames         8 independent frames: no temporal term (8 calls of one frame each, no ``prev``)
  temporal       one call of 8 frames with ``prev``: + the dtSSD sums
  temporal+flow  ... and ``backward``: + the MESSDdt sums
pred is f32 (a model's alpha), gt uint8 (a ground-truth file).  Every timed window is one call on one of ``--sets``
input sets, taken in turn, so that consecutive windows stream more than 256 MiB of different inputs and the Infinity
Cache holds none of them; the fused call and the torch formulation alternate window by window in the one process.
Times are hipEvent medians after a warm-up.  Per combination: the algorithmic bytes and operations (each input byte
read once; every f32 arithmetic step of the definition once per pixel, plus the horizontal passes over a tile's halo
rows) computed from shapes below, bytes/s achieved, and the share of the hardware's least time, which is the larger of
bytes over the 8 TB/s HBM peak and operations over the 157.3 TFLOP/s vector-f32 peak, named.
"""

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "video-matting_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402

HBM_PEAK = 8.0e12       # MI355X HBM3E, bytes/s
F32_PEAK = 157.3e12     # vector f32, FLOP/s (a fused multiply-add counted as 2; the scorer's are not fused)
TILE_H, TILE_W, RADIUS = 16, 64, 4  # csrc/score.hip
G = [0.010715649, 0.0639064, 0.22881863, 0.4918805, 0.63481766, 0.4918805, 0.22881863, 0.0639064, 0.010715649]
D = [0.04329901, 0.19367121, 0.46229678, 0.49688867, 0.0, -0.49688867, -0.46229678, -0.19367121, -0.04329901]
MODES = ("frames", "temporal", "temporal+flow")


def algorithmic(n, h, w, trimap, mode):
    """(bytes, f32 operations) of one scoring of n frames, from the shapes."""
    px = n * h * w
    nbytes = px * (4 + 1) + (px if trimap else 0) + n * 8 * 8
    tiles = -(-h // TILE_H) * -(-w // TILE_W) * n
    # both planes: two 9-tap filters along x for every staged row of a tile, two along y per pixel (a multiply and an
    # add per tap), then 2 x (2 mul + add + sqrt) for the magnitudes, 3 for the gradient term, 3 for d, |d|, d^2
    ops = 2 * 36 * tiles * (TILE_H + 2 * RADIUS) * TILE_W + px * (2 * 36 + 8 + 3 + 3)
    if mode != "frames":
        nbytes += h * w * (4 + 1)  # the frame before the first; the others are frames of the call
        ops += px * 4
    if mode == "temporal+flow":
        nbytes += px * 8
        ops += px * (2 + 2 + 4 * 2 + 6 + 2)  # xs, ys; fx, fy; four squared errors; the bilinear; |sse - e|
    return nbytes, ops


def torch_score(pred, gt, trimap, prev, backward, taps):
    """The statistics of ops.matte_score with torch ops on the device (what a user would write without the kernel):
    conv2d for the filters, index gathers for the warp, float64 reductions -> f64 [n,8]."""
    n, h, w = pred.shape
    unit = lambda p: p.float() / 255.0 if p.dtype == torch.uint8 else torch.nan_to_num(p, nan=0.0).clamp(0.0, 1.0)
    a, g = unit(pred), unit(gt)
    gd_x, gg_x, gd_y, gg_y = taps

    def magnitude(x):
        xp = TF.pad(x[:, None], (RADIUS, RADIUS, RADIUS, RADIUS), mode="replicate")
        gx = TF.conv2d(TF.conv2d(xp, gd_x), gg_y)
        gy = TF.conv2d(TF.conv2d(xp, gg_x), gd_y)
        return torch.sqrt(gx * gx + gy * gy)[:, 0]

    region = torch.ones_like(a, dtype=torch.bool) if trimap is None else (trimap != 0) & (trimap != 255)
    total = lambda t, m: (t * m).double().sum((1, 2))
    d = a - g
    sse = d * d
    dm = magnitude(a) - magnitude(g)
    stats = torch.zeros((n, 8), dtype=torch.float64, device=pred.device)
    stats[:, 0] = region.sum((1, 2))
    stats[:, 1], stats[:, 2], stats[:, 3] = total(d.abs(), region), total(sse, region), total(dm * dm, region)
    if prev is not None:
        a1, g1 = torch.cat([unit(prev[0])[None], a[:-1]]), torch.cat([unit(prev[1])[None], g[:-1]])
        dd = (a - a1) - (g - g1)
        stats[:, 4] = total(dd * dd, region)
        if backward is not None:
            xs = torch.arange(w, device=pred.device, dtype=torch.float32)[None, None, :] + backward[..., 0]
            ys = torch.arange(h, device=pred.device, dtype=torch.float32)[None, :, None] + backward[..., 1]
            take = region & (xs >= 0) & (xs <= w - 1) & (ys >= 0) & (ys <= h - 1)
            xc, yc = torch.where(take, xs, 0.0), torch.where(take, ys, 0.0)
            xf, yf = xc.floor(), yc.floor()
            fx, fy = xc - xf, yc - yf
            x0, y0 = xf.long(), yf.long()
            x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
            e1 = ((a1 - g1) ** 2).flatten(1)
            at = lambda yy, xx: e1.gather(1, (yy * w + xx).flatten(1)).view(n, h, w)
            top = at(y0, x0) + fx * (at(y0, x1) - at(y0, x0))
            bot = at(y1, x0) + fx * (at(y1, x1) - at(y1, x0))
            e = top + fy * (bot - top)
            stats[:, 5], stats[:, 6] = total((sse - e).abs(), take), take.sum((1, 2))
    return stats


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--sets", type=int, default=4, help="input sets taken in turn (4 x 83 MB of mattes at 1080p)")
    ap.add_argument("--reps", type=int, default=12, help="timed windows per combination and formulation")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "matte_score.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("score_bench: needs a ROCm GPU (no figure is produced without one)")
    from vmatting import ops

    n, h, w = a.frames, a.height, a.width
    dev = torch.device("cuda")
    rs = np.random.RandomState(0)
    sets = []
    for _ in range(a.sets):
        up = lambda x: torch.from_numpy(x).to(dev)
        pred = up(rs.uniform(-0.1, 1.1, (n + 1, h, w)).astype(np.float32))
        gt = up(rs.randint(0, 256, (n + 1, h, w)).astype(np.uint8))
        tri = up(rs.choice(np.array([0, 128, 255], np.uint8), size=(n, h, w), p=[0.45, 0.1, 0.45]))
        bw = up(rs.uniform(-3.0, 3.0, (n, h, w, 2)).astype(np.float32))
        sets.append({"pred": pred[1:], "gt": gt[1:], "prev": (pred[0], gt[0]), "trimap": tri, "backward": bw})
    rotated = sum(s["pred"].numel() * 4 + s["gt"].numel() for s in sets)
    assert a.sets < 2 or rotated > 256 << 20 or h * w < 1080 * 1920, "the rotated mattes must exceed 256 MiB"
    taps = tuple(torch.tensor(t, dtype=torch.float32, device=dev).view(shape)
                 for t, shape in ((D, (1, 1, 1, 9)), (G, (1, 1, 1, 9)), (D, (1, 1, 9, 1)), (G, (1, 1, 9, 1))))
    out = torch.zeros((n, 8), dtype=torch.float64, device=dev)
    work = torch.zeros(ops.matte_score_workspace_bytes(n, h, w), dtype=torch.uint8, device=dev)

    def fused(s, trimap, mode):
        tri = s["trimap"] if trimap else None
        if mode == "frames":
            for j in range(n):
                ops.matte_score(s["pred"][j:j + 1], s["gt"][j:j + 1], None if tri is None else tri[j:j + 1],
                                out=out[j:j + 1], work=work)
            return out
        return ops.matte_score(s["pred"], s["gt"], tri, s["prev"], s["backward"] if mode == "temporal+flow" else None,
                               out=out, work=work)

    def plain(s, trimap, mode):
        return torch_score(s["pred"], s["gt"], s["trimap"] if trimap else None, None if mode == "frames" else s["prev"],
                           s["backward"] if mode == "temporal+flow" else None, taps)

    def window(fn, s, trimap, mode):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(s, trimap, mode)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    doc = {"device": torch.cuda.get_device_name(0), "shape": [n, h, w], "pred": "f32", "gt": "u8", "sets": a.sets,
           "rotated_matte_MiB": round(rotated / 2.0 ** 20, 1), "reps": a.reps, "warmup": a.warmup,
           "hbm_peak_GBps": HBM_PEAK / 1e9, "f32_peak_TFLOPs": F32_PEAK / 1e12, "timing": "hipEvent median per call",
           "combinations": {}}
    for trimap in (False, True):
        for mode in MODES:
            name = "%s, %s" % ("trimap" if trimap else "no trimap", mode)
            s0 = sets[0]
            # the two formulations agree on this input before either is timed
            f, p = fused(s0, trimap, mode).clone(), plain(s0, trimap, mode)
            torch.cuda.synchronize()
            scale = p.abs().clamp(min=1.0)
            differ = float(((f - p).abs() / scale).max())
            for k in range(a.warmup):
                fused(sets[k % a.sets], trimap, mode)
                plain(sets[k % a.sets], trimap, mode)
            torch.cuda.synchronize()
            tf, tp = [], []
            for k in range(a.reps):  # alternating, each on the next input set
                tf.append(window(fused, sets[(2 * k) % a.sets], trimap, mode))
                tp.append(window(plain, sets[(2 * k + 1) % a.sets], trimap, mode))
            ms_f, ms_p = statistics.median(tf), statistics.median(tp)
            nbytes, nops = algorithmic(n, h, w, trimap, mode)
            t_bytes, t_ops = nbytes / HBM_PEAK, nops / F32_PEAK
            row = {"bytes": nbytes, "f32_ops": nops,
                   "fused": {"ms": round(ms_f, 4), "min_ms": round(min(tf), 4), "max_ms": round(max(tf), 4),
                             "GBps": round(nbytes / ms_f / 1e6, 1), "hbm_frac": round(nbytes / (ms_f * 1e-3) / HBM_PEAK, 3),
                             "launches": 2 * (n if mode == "frames" else 1)},
                   "least_time_us": round(max(t_bytes, t_ops) * 1e6, 2),
                   "bound": "HBM bytes" if t_bytes >= t_ops else "f32 operations",
                   "share_of_least_time": round(max(t_bytes, t_ops) / (ms_f * 1e-3), 3),
                   "torch": {"ms": round(ms_p, 4), "min_ms": round(min(tp), 4), "max_ms": round(max(tp), 4)},
                   "torch_over_fused": round(ms_p / ms_f, 2), "fused_not_slower": bool(ms_f <= ms_p),
                   "max_rel_difference_of_the_sums": differ}
            doc["combinations"][name] = row
            print("# %-28s fused %.4f ms (%.0f GB/s, %.3f of HBM peak), torch %.4f ms, x%.1f; sums differ by %.2g" %
                  (name, ms_f, row["fused"]["GBps"], row["fused"]["hbm_frac"], ms_p, ms_p / ms_f, differ), file=sys.stderr)
    doc["expectation_fused_not_slower_holds"] = all(r["fused_not_slower"] for r in doc["combinations"].values())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"matte_score": {k: {"fused_ms": v["fused"]["ms"], "torch_ms": v["torch"]["ms"]}
                                      for k, v in doc["combinations"].items()},
                      "fused_not_slower": doc["expectation_fused_not_slower_holds"]}))


if __name__ == "__main__":
    main()
