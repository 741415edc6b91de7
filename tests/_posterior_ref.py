"""numpy restatement of iwae_posterior's formulas (include/iwae_amd.h), in the dtype given: shared by tests/test_posterior_host.py and
tests/test_gpu_posterior.py.  Not a test module.

Built on tests/_impute_ref.py's restate (the proposal, the mask semantics and log_w are iwae_impute's)."""
import numpy as np

import _ais_ref as R
import _impute_ref as IM

CHUNK = 64


def weights(log_w, dtype=np.float64):
    """al [k, N] of log_w [k, N].  float64: the softmax.  float32: the device's form, exp(log_w - max) in float32 times the float32 rounding
    of 1 / sum, the sum taken in float64 over the double exponentials (pass (b) of iwae_impute)."""
    lw = np.asarray(log_w)
    if np.dtype(dtype) == np.float64:
        lw = lw.astype(np.float64)
        w = np.exp(lw - lw.max(axis=0)[None])
        return w / w.sum(axis=0)[None]
    lw = lw.astype(np.float32)
    d = lw - lw.max(axis=0)[None]
    inv = (1.0 / np.sum(np.exp(d.astype(np.float64)), axis=0)).astype(np.float32)
    return np.exp(d) * inv[None]


def moments(al, mu, sigma, eps, dtype=np.float64):
    """The moments as the header specifies them.  Per 64-draw chunk, in sample order, in `dtype`: m1_c[d] = sum_s al_s e_sd and
    m2_c[d,d'] = sum_s (al_s e_sd) e_sd'; the chunks in chunk order in float64: ebar, M2, Ce = M2 - ebar ebar^T; mean = mu + sigma ebar,
    cov = sigma sigma^T Ce with the diagonal clamped at 0.  al [k, N], mu, sigma [N, D], eps [k, N, D].  Returns mean [N, D], cov
    [N, D, D] (float64 values; the device rounds each to float32 once) and ebar, Ce."""
    al, e = np.asarray(al, dtype=dtype), np.asarray(eps, dtype=dtype)
    k, N, D = e.shape
    ebar, M2 = np.zeros((N, D)), np.zeros((N, D, D))
    for c0 in range(0, k, CHUNK):
        m1, m2 = np.zeros((N, D), dtype=dtype), np.zeros((N, D, D), dtype=dtype)
        for s in range(c0, min(k, c0 + CHUNK)):
            ae = al[s][:, None] * e[s]
            m1 = m1 + ae
            m2 = m2 + ae[:, :, None] * e[s][:, None, :]
        ebar += m1.astype(np.float64)
        M2 += m2.astype(np.float64)
    M2 = np.triu(M2) + np.swapaxes(np.triu(M2, 1), 1, 2)           # (the device computes d <= d' and mirrors it)
    Ce = M2 - ebar[:, :, None] * ebar[:, None, :]
    i = np.arange(D)
    Ce[:, i, i] = np.maximum(Ce[:, i, i], 0.0)
    mu, sigma = np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    return {"mean": mu + sigma * ebar, "cov": sigma[:, :, None] * sigma[:, None, :] * Ce, "ebar": ebar, "Ce": Ce}


def direct_moments(al, z):
    """sum_s al_s z_s and sum_s al_s (z_s - m)(z_s - m)^T in float64, without the standardised variable or the chunks."""
    al, z = np.asarray(al, dtype=np.float64), np.asarray(z, dtype=np.float64)
    m = np.einsum("sn,snd->nd", al, z)
    d = z - m[None]
    return m, np.einsum("sn,snd,sne->nde", al, d, d)


def standard_errors(al, z, mean, cov):
    """Delta-method standard errors of the self-normalised estimates: se(mean_d)^2 = sum_s al_s^2 (z_sd - m_d)^2 and
    se(cov_dd')^2 = sum_s al_s^2 ((z_sd - m_d)(z_sd' - m_d') - cov_dd')^2.  Returns [N, D], [N, D, D]."""
    al, z = np.asarray(al, dtype=np.float64), np.asarray(z, dtype=np.float64)
    d = z - np.asarray(mean, dtype=np.float64)[None]
    a2 = al * al
    se_m = np.sqrt(np.einsum("sn,snd->nd", a2, d * d))
    dev = d[:, :, :, None] * d[:, :, None, :] - np.asarray(cov, dtype=np.float64)[None]
    return se_m, np.sqrt(np.einsum("sn,snde->nde", a2, dev * dev))


def indices(log_w, u):
    """The inverse-CDF rule in float64: w_s = exp((double)(log_w_s - max)) with the difference taken in float32, c = cumsum(w) in sample
    order, idx[r, n] = the smallest s with c_s > (double)u c_{k-1} (np.searchsorted, side="right"); u = 1 (no such s): the first s whose
    c_s reaches c_{k-1}.  log_w [k, N] float32, u [R, N] float32.  Returns int32 [R, N]."""
    lw, u = np.asarray(log_w, dtype=np.float32), np.asarray(u, dtype=np.float32)
    k, N = lw.shape
    w = np.exp((lw - lw.max(axis=0)[None]).astype(np.float64))
    c = np.cumsum(w, axis=0)
    out = np.empty(u.shape, dtype=np.int32)
    for n in range(N):
        i = np.searchsorted(c[:, n], u[:, n].astype(np.float64) * c[-1, n], side="right")
        out[:, n] = np.where(i >= k, np.searchsorted(c[:, n], c[-1, n], side="left"), i)
    return out


def restate(P, x, mask, mu, sigma, eps, dtype=np.float64, log_w=None):
    """IM.restate's dict plus mean, cov (moments() at weights(log_w, dtype)), z [k, N, D] and al.  log_w: the log-weights to take the
    weights from (None: the restatement's own)."""
    r = IM.restate(P, x, mask, mu, sigma, eps, dtype)
    al = weights(r["log_w"] if log_w is None else log_w, dtype)
    r.update(moments(al, mu, sigma, eps, dtype))
    r["al"] = al
    r["z"] = np.asarray(mu, dtype=np.float64)[None] + np.asarray(sigma, dtype=np.float64)[None] * np.asarray(eps, dtype=np.float64)
    return r


def quadrature_posterior(P, x, mask, n=801, extent=8.0):
    """Mean [N, 2] and covariance [N, 2, 2] of p(z | x_obs) of a model with TWO latent dimensions by the rectangle rule on an n x n grid
    over [-extent, extent]^2 (float64): IM.quadrature_log_px_obs's integrand, normalised."""
    dec = R.decoder_of(P, np.float64)
    g = np.linspace(-extent, extent, n)
    obs = np.ones(np.shape(x), dtype=bool) if mask is None else np.asarray(mask) != 0
    xs = np.where(obs, np.asarray(x, dtype=np.float64), 0.0)
    lj, zz = [], []
    for i in range(0, n, 50):
        z = np.stack(np.meshgrid(g[i:i + 50], g, indexing="ij"), axis=-1).reshape(-1, 2)
        l = R.logits_of(dec, z)[2]
        sp = np.maximum(l, 0.0) + np.log1p(np.exp(-np.abs(l)))
        lj.append(xs @ l.T - obs.astype(np.float64) @ sp.T - 0.5 * np.sum(z * z, axis=1)[None])
        zz.append(z)
    lj, zz = np.concatenate(lj, axis=1), np.concatenate(zz, axis=0)
    w = np.exp(lj - lj.max(axis=1)[:, None])
    w /= w.sum(axis=1)[:, None]
    m = w @ zz
    d = zz[None] - m[:, None]
    return m, np.einsum("ng,ngd,nge->nde", w, d, d)
