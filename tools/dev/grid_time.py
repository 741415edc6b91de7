"""Developer script (GPU box): wall time of iwae_grid_posterior at N = 10 000 images against G = 200^2 and 1000^2 grid points, in both eval
precisions, plus the k = 5000 evaluator on the same images for scale.  The score kernel's work is counted as 2 * 2 * N * G * 800 FLOP
(the hi and the lo product, K = 800); the rate printed divides it by the whole call's time (decoder, prep, merge and copies included),
so it is a lower bound on the kernel's own -- run under rocprofv3 --kernel-trace --stats for grid_score_kernel alone.

    python tools/dev/grid_time.py [images]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from oracle import iwae_np as O
from iwae_amd import utils
from iwae_amd.native import NativeModel

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
x = O.synthetic_binarized(N, 1)
m = NativeModel(1, 200, 2, seed=5)
m.set_output_bias(O.output_bias_from_mean(O.synthetic_pixel_means()))
for prec in ("fp32", "bf16"):
    m.set_eval_precision(prec)
    for n in (200, 1000):
        z, lw = utils.latent_grid([(-5.0, 5.0)] * 2, n)
        G = z.shape[0]
        m.grid_posterior(x[:64], z, lw)        # (warm-up: buffers grow here)
        times = []
        for _ in range(3):
            t = time.perf_counter()
            r = m.grid_posterior(x, z, lw)
            times.append(time.perf_counter() - t)
        dt = min(times)
        flop = 2.0 * 2.0 * N * G * 800
        print("%s N=%d G=%d^2: %.2f ms per call (min of 3: %s), %.1f TFLOP/s of score-kernel work over the whole call, mean log p(x) %.4f"
              % (prec, N, n, dt * 1e3, ", ".join("%.2f" % (v * 1e3) for v in times), flop / dt / 1e12, float(np.mean(r["log_px"]))))
    m.eval_llh(x[:500], 5000)
    t = time.perf_counter()
    llh = m.eval_llh(x, 5000)
    print("%s k=5000 evaluator on the same %d images: %.3f s, llh %.4f" % (prec, N, time.perf_counter() - t, llh))
m.close()
