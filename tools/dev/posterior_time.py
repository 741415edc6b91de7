"""Developer script (GPU box): iwae_posterior at its timing workload -- N = 1 000 and 10 000 binarised images, k = 50 and 5 000 draws,
R = 200 resampled latent vectors per image, a 50 % completely-at-random mask, the 1-layer model at the reference's dims (784 / 200 / 100),
float32 heads, the device's own noise.  Per workload: seconds per call with every output, with the shared outputs alone (pass (a) and (b):
what iwae_impute's bound costs) and with the moments alone; the time inside the "impute" launches (pass (a)) and inside the "posterior"
launches (moments + merge) of the full call (HIP events, iwae_enable_timing); the resampling down to idx by wall time (a call with idx less
the shared outputs alone: z adds one small kernel and its copy to the host); and the ratios of the moments, of the resampling and of
both to pass (a) of the same call.  One GPU process; run it under a time limit.  Writes
profiles/posterior_time.txt.

    python tools/dev/posterior_time.py [N ...]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import iwae_np as O
from iwae_amd import utils
from iwae_amd.native import NativeModel

Ns = [int(v) for v in sys.argv[1:]] or [1000, 10000]
H, D, X, R = 200, 100, 784, 200
SHARED = ("log_px", "ess", "q_mu", "q_sigma")
xall = O.synthetic_binarized(max(Ns), 1)
mall = utils.mcar_mask(xall.shape, 0.5, seed=2)
m = NativeModel(1, H, D, seed=5)
m.set_output_bias(O.output_bias_from_mean(O.synthetic_pixel_means()))
m.set_eval_precision("fp32")
m.posterior(xall[:64], mask=mall[:64], n_samples=70, n_draws=3)   # (warm-up: module load)


def timed(fn):
    fn()                                                          # (the buffers grow here, not in the timed call)
    m.sync()
    t = time.perf_counter()
    fn()
    m.sync()
    return time.perf_counter() - t


lines = ["# iwae_posterior, %d / %d / %d, R = %d, 50 %% mask, float32 heads, device noise" % (X, H, D, R)]
for N in Ns:
    x, mask = xall[:N], mall[:N]
    for k in (50, 5000):
        t_shared = timed(lambda: m.posterior(x, mask=mask, n_samples=k, outputs=SHARED))
        t_mom = timed(lambda: m.posterior(x, mask=mask, n_samples=k, outputs=SHARED + ("mean", "cov")))
        t_idx = timed(lambda: m.posterior(x, mask=mask, n_samples=k, n_draws=R, outputs=SHARED + ("idx",)))
        t_all = timed(lambda: m.posterior(x, mask=mask, n_samples=k, n_draws=R, outputs=SHARED + ("mean", "cov", "idx", "z", "u")))
        m.enable_timing(1)
        m.posterior(x, mask=mask, n_samples=k, n_draws=R, outputs=SHARED + ("mean", "cov", "idx", "z", "u"))
        us_a, n_a = m.kernel_time("impute")
        us_p, n_p = m.kernel_time("posterior")
        m.enable_timing(0)
        k_a, k_p, t_sir = us_a * n_a * 1e-6, us_p * n_p * 1e-6, t_idx - t_shared
        lines.append("posterior N=%d k=%d R=%d: %.4f s per call with every output on the host (cov %.0f MB, z %.0f MB); shared outputs alone %.4f s; "
                     "with mean and cov %.4f s; with idx %.4f s; in the kernels: \"impute\" (pass (a)) %.4f s in %d launches, \"posterior\" "
                     "(moments + merge) %.4f s in %d launches; resampling to idx (wall, less the shared outputs) %.4f s; moments / pass (a) %.4f; "
                     "resampling / pass (a) %.4f; both / pass (a) %.4f"
                     % (N, k, R, t_all, 4e-6 * N * D * D, 4e-6 * R * N * D, t_shared, t_mom, t_idx, k_a, n_a, k_p, n_p, t_sir, k_p / k_a, t_sir / k_a,
                        (k_p + t_sir) / k_a))
        print(lines[-1], flush=True)
m.close()
with open(os.path.join(ROOT, "profiles", "posterior_time.txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
