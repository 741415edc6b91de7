"""Developer script (GPU box): iwae_local_posterior at the timing workload -- N = 1 000 binarised images, S = 16 draws, T = 500 Adam
iterations (ELBO) and E = 8 evaluation passes on the 1-layer model at the reference's dims (784 / 200 / 100), float32 -- with every launch
of local_q_kernel bracketed by HIP events (iwae_enable_timing).  Prints wall seconds, launches, time per launch and per pass, and the
achieved float32 rate counted as tools/dev/ais_time.py counts it: 2 x (forward + dX) multiply-adds per row evaluation, one evaluation per
row and pass (evaluation passes run the dX chain too).  One GPU process; run it under a time limit.

    python tools/dev/local_q_time.py [T] [local_t_chunk] [images] [draws]
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
S = int(sys.argv[4]) if len(sys.argv) > 4 else 16
E, H, D, X = 8, 200, 100, 784
x = O.synthetic_binarized(N, 1)
m = NativeModel(1, H, D, seed=5)
m.set_output_bias(O.output_bias_from_mean(O.synthetic_pixel_means()))
m.set_eval_precision("fp32")
m.set_option("local_t_chunk", chunk)
m.local_posterior(x[:64], n_samples=S, n_iters=2, n_eval=1)      # (warm-up: module load)
m.local_posterior(x, n_samples=S, n_iters=1, n_eval=E)           # (the buffers grow here, not in the timed call)
m.sync()
amort = m.local_posterior(x, n_samples=S, n_iters=0, n_eval=E)
m.enable_timing(1)
t = time.perf_counter()
r = m.local_posterior(x, n_samples=S, n_iters=T, n_eval=E, objective="elbo", lr=0.05)
dt = time.perf_counter() - t
us, launches = m.kernel_time("local_q")
m.enable_timing(0)
passes = T + E
flop = 2.0 * 2.0 * (D * H + H * H + H * X) * N * S * passes
kern = us * 1e-6 * launches
print("local_q N=%d S=%d T=%d E=%d local_t_chunk=%s: %.3f s wall, %d launches of local_q_kernel, %.2f ms per launch (%.3f s in the kernel, "
      "%.3f ms per pass), %.1f TFLOP/s float32 in the kernel; mean elbo %.3f from %.3f at the encoder's heads"
      % (N, S, T, E, chunk or "default", dt, launches, us * 1e-3, kern, kern * 1e3 / passes, flop / kern * 1e-12, r["elbo"].mean(),
         amort["elbo"].mean()))
m.close()
