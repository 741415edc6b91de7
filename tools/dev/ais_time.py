"""Developer script (GPU box): iwae_ais at the timing workload -- N = 1 000 binarised images, C = 16 chains, T = 500 temperatures, L = 10
leapfrog steps on the 1-layer model at the reference's dims (784 / 200 / 100) -- with every launch of ais_chain_kernel bracketed by HIP
events (iwae_enable_timing).  Prints wall seconds, launches, time per launch and the achieved float32 rate, counting 2 x (forward + dX)
multiply-adds per gradient evaluation and L + 1 evaluations per transition (the one at the transition's start, which also yields the
weight increment, and one per leapfrog step).  One GPU process; run it under a time limit.

    python tools/dev/ais_time.py [T] [ais_t_chunk] [images] [chains]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from oracle import iwae_np as O
from iwae_amd.native import NativeModel

T = int(sys.argv[1]) if len(sys.argv) > 1 else 500
chunk = int(sys.argv[2]) if len(sys.argv) > 2 else 0
N = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
Cn = int(sys.argv[4]) if len(sys.argv) > 4 else 16
L, H, D, X = 10, 200, 100, 784
x = O.synthetic_binarized(N, 1)
m = NativeModel(1, H, D, seed=5)
m.set_output_bias(O.output_bias_from_mean(O.synthetic_pixel_means()))
m.set_option("ais_t_chunk", chunk)
m.ais(x[:64], n_chains=Cn, n_temps=2, leapfrog=1)            # (warm-up: module load)
m.ais(x, n_chains=Cn, n_temps=1, leapfrog=1)                 # (the buffers grow here, not in the timed call)
m.sync()
m.enable_timing(1)
t = time.perf_counter()
r = m.ais(x, n_chains=Cn, n_temps=T, leapfrog=L, step_size=0.05, adapt=True)
dt = time.perf_counter() - t
us, launches = m.kernel_time("ais_chain")
m.enable_timing(0)
evals = T * (L + 1)
flop = 2.0 * 2.0 * (D * H + H * H + H * X) * N * Cn * evals
kern = us * 1e-6 * launches
print("ais N=%d C=%d T=%d L=%d ais_t_chunk=%s: %.3f s wall, %d launches of ais_chain_kernel, %.2f ms per launch (%.3f s in the kernel, "
      "%.2f ms per transition), %.1f TFLOP/s float32 in the kernel; mean log_px %.3f, accept rate %.3f, mean step %.4f, mean ESS %.2f of %d"
      % (N, Cn, T, L, chunk or "default", dt, launches, us * 1e-3, kern, kern * 1e3 / T, flop / kern * 1e-12, r["log_px"].mean(),
         r["accept_rate"].mean(), r["step_size"].mean(), r["ess"].mean(), Cn))
m.close()
