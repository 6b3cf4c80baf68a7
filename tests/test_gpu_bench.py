"""bench.py's plain run on the GPU: the headline line alone, and --dump-outputs.

One child process runs `bench.py --gpus 1 --steps 2 --warmup 1 --dump-outputs DIR` on a 70x90 frame (odd sizes, every
pooling level ragged).  The line must carry the headline keys and none of the --full records, and DIR/alpha.npy must
be the float32 alpha of the timed forward: bit for bit the graph replay of the same model on the same seeded frame
built in this process (the forward has no atomics and a fixed launch order, so equal inputs give equal bits)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a ROCm GPU")]

H, W = 70, 90
FULL_ONLY = ("fp32", "f16x3", "bf16x6", "parity", "video_batch", "temporal", "train", "train_small", "train_image",
             "loader", "augment", "hbm")


def test_plain_run_prints_the_headline_and_dumps_the_timed_alpha(tmp_path):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--height", str(H), "--width", str(W), "--dump-outputs", str(out)],
                       env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["unit"] == "frames/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16"
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["ms_per_step"] > 0 and rec["value"] == pytest.approx(1000.0 / rec["ms_per_step"], rel=1e-3)
    assert rec["roofline"] is None and rec["cpu_baseline"] is None
    assert not [k for k in FULL_ONLY if k in rec]
    assert sorted(os.listdir(out)) == ["alpha.npy"]
    got = np.load(out / "alpha.npy")
    assert got.dtype == np.float32 and got.shape == (1, H, W, 1)

    from vmatting import unet, video
    from vmatting.weights import synthetic_vgg16
    np.random.seed(0)
    m = unet.UNetVideo(synthetic_vgg16(0), dtype="bf16", device="cuda:0").prepare()
    g = m.capture(video.synthetic_frames(1, H, W, first=0, device="cuda:0"))
    g.replay()
    torch.cuda.synchronize()
    want = g.output.float().cpu().numpy()
    assert np.array_equal(got, want), np.abs(got - want).max()
