"""numpy restatement of iwae_aggregate_posterior's formulas (include/iwae_amd.h), in the dtype given: shared by tests/test_aggregate_host.py
and tests/test_gpu_aggregate_posterior.py.  Not a test module."""
import numpy as np


def _lse(a, axis):
    mx = a.max(axis=axis, keepdims=True)
    return np.squeeze(mx, axis=axis) + np.log(np.exp(a - mx).sum(axis=axis))


def restate(mu, sigma, eps, dtype=np.float64):
    """mu, sigma [N, D], eps [S, N, D] -> per-sample log_qz [S, N], log_qzd, lq_own, lp [S, N, D] and the summary / per-unit means."""
    dt = np.dtype(dtype).type
    mu, sg, eps = np.asarray(mu, dtype=dt), np.asarray(sigma, dtype=dt), np.asarray(eps, dtype=dt)
    S, N, D = eps.shape
    c, half, logn = dt(0.5 * np.log(2.0 * np.pi)), dt(0.5), dt(np.log(N))
    ls = np.log(sg)
    z = mu[None] + sg[None] * eps
    log_qz = np.empty((S, N), dtype=dt)
    log_qzd = np.empty((S, N, D), dtype=dt)
    for s in range(S):
        t = (z[s][:, None, :] - mu[None, :, :]) / sg[None, :, :]          # [n, m, d]
        l = -half * t * t - ls[None, :, :] - c
        log_qzd[s] = _lse(l, 1) - logn
        log_qz[s] = _lse(l.sum(axis=2), 1) - logn
    lq_own = -half * eps * eps - ls[None] - c
    lp = -half * z * z - c
    out = {"log_qz": log_qz, "log_qzd": log_qzd, "lq_own": lq_own, "lp": lp}
    out.update(sums(log_qz, log_qzd, lq_own, lp))
    return out


def sums(log_qz, log_qzd, lq_own, lp):
    """The double means of the per-sample terms: unit_mi, unit_kl [D] and mi, tc, dim_kl, kl."""
    q, qd, lq, lp = (np.asarray(a, dtype=np.float64) for a in (log_qz, log_qzd, lq_own, lp))
    unit_mi = (lq - qd).mean(axis=(0, 1))
    unit_kl = (qd - lp).mean(axis=(0, 1))
    return {"unit_mi": unit_mi, "unit_kl": unit_kl, "mi": (lq.sum(axis=2) - q).mean(), "tc": (q - qd.sum(axis=2)).mean(),
            "dim_kl": unit_kl.sum(), "kl": (lq.sum(axis=2) - lp.sum(axis=2)).mean()}
