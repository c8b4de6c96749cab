"""bench.py's plain single-GPU run (no --full): the headline line only, and --dump-outputs writing what the timed path
computed in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_bench_plain_run_dumps_the_last_step(hip_lib, tmp_path):
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(out)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["full"] is False and d["n_gpus"] == 1 and d["steps"] == 7 and d["warmup"] == 2
    assert d["value"] > 0 and d["unit"] == "pairs/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]
    assert "roofline" not in d and "cpu_baseline" not in d and "pipelined" not in d      # (--full only)
    # the dumped maps are the four stage maps a caller receives for the seeded pair, bit for bit
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.synth import make_batch
    from lwsnet_amd.weights import default_args, make_state_dict
    dev = torch.device("cuda:0")
    margs = default_args(maxdisplist=(24, 5, 5))
    model = LWSNet(margs, device=dev).set_state_dict(make_state_dict(7, margs)).eval()
    left, right = make_batch(1, 256, 512, first_index=0)
    pred = model(torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev))
    for s in range(4):
        got = np.load(out / f"stage{s + 1}.npy")
        assert got.dtype == np.float32 and got.shape == (1, 1, 256, 512)
        assert np.array_equal(got, pred[s].cpu().numpy()), f"stage {s + 1}"
