"""GPU: `bench.py --dump-outputs` writes what the timed path computed in its last step, and the same in every run whatever the
untimed clock conditioning did before (the engine state is reset in front of the warm-up steps)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

B, W, K = 8, 3, 5


def _bench(out_dir, condition_ms):
    args = ["--gpus", "1", "--batch", str(B), "--warmup", str(W), "--steps", str(K), "--condition-ms", str(condition_ms),
            "--dump-outputs", str(out_dir)]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), np.load(os.path.join(out_dir, "enhanced_mag.npy"))


@pytest.mark.timeout(600)
def test_bench_dump_is_the_last_timed_step_and_repeats_bitwise(tmp_path):
    import torch
    import nunet_amd
    sys.path.insert(0, ROOT)
    import bench
    j0, d0 = _bench(tmp_path / "a", 0)
    j1, d1 = _bench(tmp_path / "b", 100)           # ~hundreds of untimed steps in front: reset away
    assert j0["steps"] == j1["steps"] == K and j1["conditioning_steps"] > 0 and j0["conditioning_steps"] == 0
    for j in (j0, j1):       # a plain line carries none of what --full adds
        assert not {"roofline", "encoder_conv_stack", "cpu_baseline", "parity_rms_vs_oracle", "other_configs"} & set(j)
        assert j["value_unconditioned"] is None and j["ms_per_step"] > 0
    assert d0.dtype == np.float32 and d0.shape == (B, 256) and np.isfinite(d0).all()
    np.testing.assert_array_equal(d0, d1)
    # the same W + K steps from the zero state, in this process: the dump is the output of the last of them
    pool = torch.from_numpy(bench.synthetic_pool(B, 8, 1234)).cuda()
    eng = nunet_amd.NutlsEngine(batch=B, device=0, mode="fused")
    out = torch.empty(B, 256, device="cuda")
    for s in range(W):
        eng.step(pool[s % 8], out)
    for s in range(K):
        eng.step(pool[s % 8], out)
    want = out.cpu().numpy()
    eng.close()
    np.testing.assert_array_equal(d0, want)
