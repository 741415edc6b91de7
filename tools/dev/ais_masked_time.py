"""Developer script (GPU box): iwae_ais_masked and iwae_local_posterior_masked against the unmasked calls at the timing workloads of
tools/dev/ais_time.py (N = 1 000, C = 16, T = 500, L = 10) and tools/dev/local_q_time.py (N = 1 000, S = 16, T = 500, E = 8): 1-layer model
at the reference's dims (784 / 200 / 100), float32.  In ONE process, interleaved, `repeats` times each: the unmasked call, the masked call
with a mask of ones, the masked call at 50 % MCAR (utils.device_mcar_mask).  Every launch of ais_chain_kernel / local_q_kernel is bracketed
by HIP events (iwae_enable_timing); per variant the median, minimum and maximum of the time per transition / per pass are printed, and the
masked medians over the unmasked one.  The yardstick is the unmasked call of the same run: the masked kernels do the same MFMA work plus
one compare-and-select per pixel in the output layer's epilogue.  One GPU process; run it under a time limit.

    python tools/dev/ais_masked_time.py [repeats] [T] [images]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from oracle import iwae_np as O
from iwae_amd import utils
from iwae_amd.native import NativeModel

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
T = int(sys.argv[2]) if len(sys.argv) > 2 else 500
N = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
Cn, L, S, E, H, D, X = 16, 10, 16, 8, 200, 100, 784
x = O.synthetic_binarized(N, 1)
masks = {"unmasked": None, "ones": np.ones((N, X), np.uint8), "mcar50": utils.device_mcar_mask(N, X, 0.5, seed=1)}
m = NativeModel(1, H, D, seed=5)
m.set_output_bias(O.output_bias_from_mean(O.synthetic_pixel_means()))
m.set_eval_precision("fp32")


def run_ais(mask, temps):
    return m.ais(x, mask=mask, n_chains=Cn, n_temps=temps, leapfrog=L, step_size=0.05, adapt=True)


def run_local(mask, iters):
    return m.local_posterior(x, mask=mask, n_samples=S, n_iters=iters, n_eval=E, objective="elbo", lr=0.05)


def measure(name, kernel, run, units):
    """repeats x (unmasked, ones, mcar50), interleaved; per variant the kernel's ms per unit (transition / pass) of every repeat"""
    for mask in masks.values():
        run(mask, 1)                    # (warm-up: module load, and the buffers grow here, not in a timed call)
    m.sync()
    per, wall, value = {k: [] for k in masks}, {k: [] for k in masks}, {}
    for _ in range(repeats):
        for key, mask in masks.items():
            m.set_step(1, 0)            # every repeat draws the same noise: the same work
            m.enable_timing(1)
            t = time.perf_counter()
            r = run(mask, T)
            wall[key].append(time.perf_counter() - t)
            us, launches = m.kernel_time(kernel)
            m.enable_timing(0)
            per[key].append(us * 1e-3 * launches / units)
            value[key] = float(np.mean(r["log_px"] if "log_px" in r else r["elbo"]))
    med = {k: float(np.median(v)) for k, v in per.items()}
    for key in masks:
        v = per[key]
        print("%s %-8s: median %.4f ms per %s (min %.4f, max %.4f, spread %.2f %%; %d repeats), wall median %.3f s, %.3f of unmasked; mean value %.3f"
              % (name, key, med[key], "transition" if kernel == "ais_chain" else "pass", min(v), max(v), 100.0 * (max(v) - min(v)) / med[key], repeats,
                 float(np.median(wall[key])), med[key] / med["unmasked"], value[key]))


print("N=%d C=%d T=%d L=%d | S=%d T=%d E=%d, 784 / 200 / 100 float32, %d interleaved repeats" % (N, Cn, T, L, S, T, E, repeats))
measure("ais", "ais_chain", run_ais, T)
measure("local_q", "local_q", run_local, T + E)
m.close()
