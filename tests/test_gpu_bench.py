"""GPU test of bench.py's plain run: the one JSON line it prints, and the files --dump-outputs writes -- the state the last timed step
left, which is what two builds are compared by."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(gpu, tmp_path):
    import torch
    import bench
    from iwae_amd import utils
    from iwae_amd.native import NativeModel
    out_dir = tmp_path / "outputs"
    steps, warmup = 3, 2
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--settle", "0", "--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup and d["config"]["settle_steps"] == warmup
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 1024 * 1e3 / d["ms_per_step"]) < 1e-2 * d["value"]
    assert d["config"]["full"] is False and "roofline" not in d and "cpu_baseline" not in d      # (--full only)

    # the same warmup + timed steps in this process, through the same calls: the dump is bitwise their state
    cfg = bench.CONFIGS["c1"]
    x_np, p = bench.synthetic_batch(cfg["B"], 123)
    x_dev = torch.tensor(x_np, device="cuda")
    m = NativeModel(cfg["layers"], cfg["nh"], cfg["nl"], seed=123)
    m.set_output_bias(utils.bias_from_mean(p))
    for i in range(warmup + steps):
        m.set_step(i, 0)
        m.train_step_devptr(x_dev.data_ptr(), cfg["B"], cfg["k"], 1.0, 1e-3, bench.OBJ_ID[cfg["obj"]])
    mom, vel, t = m.get_adam_state()
    assert t == warmup + steps
    want = {"params": m.get_params(), "grads": m.get_grads(), "adam_m": mom, "adam_v": vel}
    m.close()
    assert sorted(os.listdir(out_dir)) == sorted(n + ".npy" for n in want)
    for name, a in want.items():
        got = np.load(out_dir / (name + ".npy"))
        assert got.dtype == np.float32 and got.shape == a.shape and np.all(np.isfinite(got)), name
        np.testing.assert_array_equal(got, a, err_msg=name)
