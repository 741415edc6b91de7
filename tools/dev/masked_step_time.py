"""Developer script (GPU box): the masked float32 train step (iwae_train_step_masked) at its timing workload -- B = 1 024 binarised images,
k = 50, the 1-layer model at the reference's dims (784 / 200 / 100), a 50 % completely-at-random mask, x and the mask resident on the device,
device noise -- on both routes of the output layer (options no_masked_out_fused / masked_out_min_rows = 1), interleaved in one process with
the unmasked float32 step (iwae_train_step on the same handle type; its plan and kernels are what they were before the masked step
existed).  Three handles take turns, ROUNDS rounds of STEPS steps each, synchronised around each block; printed are the median and the
spread of the per-step times over the rounds and, for the fast route, masked_out_f32_kernel's mean launch time (HIP events,
iwae_enable_timing, in a block of its own).  One GPU process; run it under a time limit.

    python tools/dev/masked_step_time.py [rounds] [steps] [B]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np
import torch

from oracle import iwae_np as O
from iwae_amd import utils
from iwae_amd.native import NativeModel, OBJECTIVES

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 40
B = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
K, H, D, X = 50, 200, 100, 784
x = torch.tensor(O.synthetic_binarized(B, 1), device="cuda")
mask = torch.tensor(utils.mcar_mask((B, X), 0.5, seed=2), device="cuda")
obj = OBJECTIVES["iwae_elbo"]
handles = {"unmasked": {}, "masked_general": {"no_masked_out_fused": 1}, "masked_fast": {"masked_out_min_rows": 1}}
models = {}
for name, opts in handles.items():
    m = NativeModel(1, H, D, seed=5, precision="fp32", options=opts)
    m.set_output_bias(O.output_bias_from_mean(O.synthetic_pixel_means()))
    models[name] = m


def block(name, steps):
    m = models[name]
    m.sync()
    t = time.perf_counter()
    for _ in range(steps):
        if name == "unmasked":
            m.train_step_devptr(x.data_ptr(), B, K, 1.0, 1e-3, obj)
        else:
            m.train_step_masked_devptr(x.data_ptr(), mask.data_ptr(), B, K, 1.0, 1e-3, obj)
    m.sync()
    return (time.perf_counter() - t) / steps


for name in models:
    block(name, 10)          # (warm-up: module load, the buffers grow)
times = {name: [] for name in models}
for _ in range(ROUNDS):
    for name in models:
        times[name].append(block(name, STEPS))
print("# B = %d, k = %d, %d / %d / %d, float32, iwae_elbo; %d rounds of %d steps, interleaved" % (B, K, X, H, D, ROUNDS, STEPS))
for name, ts in times.items():
    print("%-15s median %.4f ms per step  (min %.4f, max %.4f)" % (name, statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3))
base = statistics.median(times["unmasked"])
for name in ("masked_general", "masked_fast"):
    print("%-15s / unmasked = %.3f" % (name, statistics.median(times[name]) / base))
m = models["masked_fast"]
m.enable_timing(1)
block("masked_fast", STEPS)
us, launches = m.kernel_time("masked_out")
m.enable_timing(0)
print("masked_out      %.1f us per launch of masked_out_f32_kernel (%d launches)" % (us, launches))
for m in models.values():
    m.close()
