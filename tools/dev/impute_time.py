"""Developer script (GPU box): iwae_impute at its timing workload -- N = 1 000 and 10 000 binarised images, k = 50 and 5 000 draws, a 50 %
completely-at-random mask, the 1-layer model at the reference's dims (784 / 200 / 100), float32 heads -- against iwae_eval_llh in float32
at the same N and k in the same process (the evaluator does one float32 decoder forward per row; iwae_impute does two, the second with the
weights final).  Per workload: seconds per call, microseconds per 1 000 rows, the same for the bound alone (no xhat: one forward) and for the
evaluator, the ratios, and the launches of impute_rows_kernel with their mean time (HIP events, iwae_enable_timing).  One GPU process; run
it under a time limit.

    python tools/dev/impute_time.py [impute_rows] [N ...]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from oracle import iwae_np as O
from iwae_amd import utils
from iwae_amd.native import NativeModel

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 0
Ns = [int(v) for v in sys.argv[2:]] or [1000, 10000]
H, D, X = 200, 100, 784
xall = O.synthetic_binarized(max(Ns), 1)
mall = utils.mcar_mask(xall.shape, 0.5, seed=2)
m = NativeModel(1, H, D, seed=5)
m.set_output_bias(O.output_bias_from_mean(O.synthetic_pixel_means()))
m.set_eval_precision("fp32")
m.set_option("impute_rows", rows)
m.impute(xall[:64], mask=mall[:64], n_samples=70)                  # (warm-up: module load)
m.eval_llh(xall[:64], k=70)


def timed(fn):
    fn()                                                          # (the buffers grow here, not in the timed call)
    m.sync()
    t = time.perf_counter()
    fn()
    m.sync()
    return time.perf_counter() - t


print("# impute_rows = %s" % (rows or "default"))
for N in Ns:
    x, mask = xall[:N], mall[:N]
    for k in (50, 5000):
        krows = N * k / 1000.0
        t_ev = timed(lambda: m.eval_llh(x, k=k))
        t_b = timed(lambda: m.impute(x, mask=mask, n_samples=k, outputs=("log_px",)))
        m.enable_timing(1)
        t_i = timed(lambda: m.impute(x, mask=mask, n_samples=k, outputs=("log_px", "xhat", "ess")))
        us, launches = m.kernel_time("impute")
        m.enable_timing(0)
        print("impute N=%d k=%d: %.4f s per call, %.2f us per 1000 rows (%d launches of impute_rows_kernel in the two calls, %.2f ms each); bound alone %.4f s, "
              "%.2f us per 1000 rows; eval_llh float32 %.4f s, %.2f us per 1000 rows; ratio impute / eval_llh %.2f, bound alone / eval_llh %.2f"
              % (N, k, t_i, t_i * 1e6 / krows, launches, us * 1e-3, t_b, t_b * 1e6 / krows, t_ev, t_ev * 1e6 / krows, t_i / t_ev, t_b / t_ev))
m.close()
