"""Developer script (GPU box): wall time of iwae_latent_activity at N = 10 000 binarised images -- the 2-layer model at the reference's dims
([200, 100] hidden, [100, 50] latent) with k = 5000 z1 draws per image, and the 1-layer model (200 hidden, 100 latent) -- in both eval
precisions, against the k = 5000 evaluator (iwae_eval_llh) on the same model and images in the same process.  The acceptance bar of the
2-layer call is 0.25x the evaluator's time (the q(z2|z1) block is ~11 % of the evaluator's per-row FLOPs).  Run it once more under
rocprofv3 --kernel-trace --stats (no counters) to see which kernels each path launches.

    python tools/dev/activity_time.py [images]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from oracle import iwae_np as O
from iwae_amd.native import NativeModel

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
K = 5000
x = O.synthetic_binarized(N, 1)


def best_of(fn, n=3):
    times = []
    out = None
    for _ in range(n):
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
    return min(times), times, out


for layers, nh, nl in ((2, [200, 100], [100, 50]), (1, 200, 100)):
    m = NativeModel(layers, nh, nl, seed=5)
    m.set_output_bias(O.output_bias_from_mean(O.synthetic_pixel_means()))
    for prec in ("fp32", "bf16"):
        m.set_eval_precision(prec)
        m.latent_activity(x[:64], k=K)           # (warm-up: buffers grow here)
        m.eval_llh(x[:64], K)
        dt, times, r = best_of(lambda: m.latent_activity(x, k=K))
        de, etimes, llh = best_of(lambda: m.eval_llh(x, K), 2)
        counts = [int(np.sum(a > 1e-2)) for a in r["activity"]]
        print("%d-layer %s N=%d k=%d: latent_activity %.2f ms (min of 3: %s), eval_llh %.2f ms (min of 2: %s), ratio %.3f; active %s, llh %.4f"
              % (layers, prec, N, K, dt * 1e3, ", ".join("%.2f" % (v * 1e3) for v in times), de * 1e3,
                 ", ".join("%.2f" % (v * 1e3) for v in etimes), dt / de, counts, llh))
    m.close()
