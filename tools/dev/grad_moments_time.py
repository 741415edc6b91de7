"""Developer script (GPU box): wall time of iwae_grad_moments (M = 1000 gradient draws folded on the device) on the 1-layer model at the
reference's dims (200 hidden, 100 latent), B = 20, k in {1, 50, 5000}, in both precisions, against two baselines in the same process:
  (a) M back-to-back train_step(..., scalars=False) at the same shape, synced once (the cost of M training steps);
  (b) the Python loop: forward_backward + get_grads + a numpy float64 Welford fold per draw.
The bar: for bf16 at k in {1, 50}, grad_moments within 1.15x of (a).

    python tools/dev/grad_moments_time.py [draws] > profiles/grad_moments_time.txt
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from oracle import iwae_np as O
from iwae_amd.native import NativeModel

M = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
B = 20
x = O.synthetic_binarized(B, 1)


def timed(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def moments(m, k, draws):
    m.grad_moments(x, k, draws, 1.0, "iwae_elbo")


def train_steps(m, k, draws):
    for _ in range(draws):
        m.train_step(x, k, 1.0, 1e-4, "iwae_elbo", scalars=False)
    m.sync()


def python_loop(m, k, draws):
    P = m.n_params
    g, d, e = np.empty(P), np.empty(P), np.empty(P)      # (the fold in place: no 3.6 MB temporaries per draw)
    mean, m2 = np.empty(P), np.zeros(P)
    for j in range(draws):
        m.forward_backward(x, k, 1.0, "iwae_elbo")
        g[:] = m.get_grads()
        if j == 0:
            mean[:] = g
        else:
            np.subtract(g, mean, out=d)
            np.divide(d, j + 1, out=e)
            mean += e
            np.subtract(g, mean, out=e)
            e *= d
            m2 += e
    return mean, m2 / (draws - 1)


print("iwae_grad_moments vs (a) %d train steps (scalars=False, one sync) and (b) the Python loop (forward_backward + get_grads + numpy "
      "Welford); 1-layer 200/100, B = %d, objective iwae_elbo; times in ms, min of 2 alternated runs for grad_moments and (a)" % (M, B))
for prec in ("bf16", "fp32"):
    for k in (1, 50, 5000):
        m = NativeModel(1, 200, 100, seed=5, precision=prec)
        m.set_output_bias(O.output_bias_from_mean(O.synthetic_pixel_means()))
        for fn in (moments, train_steps, python_loop):       # warm-up: buffers grow, code objects load
            fn(m, k, 20)
        tm, ta = [], []
        for _ in range(2):
            tm.append(timed(lambda: moments(m, k, M)))
            ta.append(timed(lambda: train_steps(m, k, M)))
        tb = timed(lambda: python_loop(m, k, M))
        print("%s k=%5d M=%d: grad_moments %9.2f ms (%s) | (a) train steps %9.2f ms (%s) | (b) python loop %9.2f ms | "
              "moments/(a) %.3f, moments/(b) %.3f, per draw %.1f us"
              % (prec, k, M, min(tm) * 1e3, ", ".join("%.2f" % (v * 1e3) for v in tm), min(ta) * 1e3,
                 ", ".join("%.2f" % (v * 1e3) for v in ta), tb * 1e3, min(tm) / min(ta), min(tm) / tb, min(tm) / M * 1e6))
        sys.stdout.flush()
        m.close()
