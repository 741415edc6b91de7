"""Developer script (GPU box): wall time of iwae_aggregate_posterior at N = 10 000 binarised images on the 1-layer model at the reference's
dims (784 / 200 / 100), S = 1 and S = 10 draws per image, in both eval precisions, against the k = 5000 evaluator (iwae_eval_llh) on the
same model and images in the same process.  Run it once more under rocprofv3 --kernel-trace --stats (no counters) for the per-kernel split.

    python tools/dev/aggregate_time.py [images]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

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


m = NativeModel(1, 200, 100, seed=5)
m.set_output_bias(O.output_bias_from_mean(O.synthetic_pixel_means()))
for prec in ("fp32", "bf16"):
    m.set_eval_precision(prec)
    m.eval_llh(x[:64], K)
    de, etimes, llh = best_of(lambda: m.eval_llh(x, K), 2)
    for S in (1, 10):
        m.aggregate_posterior(x, n_samples=S)            # (warm-up: buffers grow here)
        dt, times, r = best_of(lambda: m.aggregate_posterior(x, n_samples=S))
        terms = float(N) * N * S * 100
        print("1-layer %s N=%d S=%d: aggregate_posterior %.2f ms (min of 3: %s) = %.1f G terms/s; eval_llh(k=%d) %.2f ms (min of 2: %s), ratio %.4f; "
              "kl %.4f mi %.4f tc %.4f dim_kl %.4f log N %.4f"
              % (prec, N, S, dt * 1e3, ", ".join("%.2f" % (v * 1e3) for v in times), terms / dt * 1e-9, K, de * 1e3,
                 ", ".join("%.2f" % (v * 1e3) for v in etimes), dt / de, r["kl"], r["mi"], r["tc"], r["dim_kl"], r["log_n"]))
m.close()
