"""numpy restatement of iwae_local_posterior's formulas (include/iwae_amd.h), in the dtype given, on tests/_ais_ref.py's joint_and_grad and
base_density: shared by tests/test_local_q_host.py and tests/test_gpu_local_q.py.  Not a test module.

Rows are r = s N + n (the [S, N] order of the ABI's eps).  Every product and sum runs in `dtype`; an image's sum over s runs in sample
order; the evaluation's mean and LSE are taken in float64 from log-weights formed in `dtype`, as the device does."""
import numpy as np

import _ais_ref as R

OBJECTIVES = ("elbo", "iwae")


def encoder_heads(P, x):
    """mu, sigma [N, D] of the encoder (src/iwae1.py:39-42) out of the oracle's parameter list, float64."""
    from oracle import iwae_np as O
    return O._Block(P[0:4], O._id).fwd(np.asarray(x, dtype=np.float64))


def log_weights(dec, x, mu, rho, e):
    """One pass: e [S, N, D] -> log_w [S, N], g = grad_z log p(x|z) - z [S, N, D], sigma [N, D], all in e's dtype."""
    S, N, D = e.shape
    sg = np.exp(rho)
    er = e.reshape(S * N, D)
    xr, mur, sgr = np.tile(x, (S, 1)), np.tile(mu, (S, 1)), np.tile(sg, (S, 1))
    lj, g = R.joint_and_grad(dec, xr, mur + sgr * er)
    lq = R.base_density(er, sgr)
    return (lj - lq).reshape(S, N), g.reshape(S, N, D), sg


def bound_and_grad(dec, x, mu, rho, e, objective):
    """bound [N] and the ascent direction (d/dmu, d/drho) [N, D] each of one pass."""
    dt = e.dtype.type
    S = e.shape[0]
    lw, g, sg = log_weights(dec, x, mu, rho, e)
    if objective == "iwae":
        mx = lw.max(axis=0)
        ex = np.exp(lw - mx[None])
        tot = np.zeros_like(mx)
        for s in range(S):
            tot = tot + ex[s]
        w = ex / tot[None]
        bound = mx + np.log(tot) - np.log(dt(S))
    else:
        w = np.full(lw.shape, dt(1) / dt(S), dtype=e.dtype)
        tot = np.zeros(lw.shape[1], dtype=e.dtype)
        for s in range(S):
            tot = tot + lw[s]
        bound = tot * (dt(1) / dt(S))
    dmu, drho = np.zeros_like(mu), np.zeros_like(mu)
    for s in range(S):
        dmu = dmu + w[s][:, None] * g[s]
        drho = drho + w[s][:, None] * (g[s] * (sg * e[s]))
    return bound, dmu, drho + dt(1), lw


def adam_ascent(theta, grad, m, v, t, lr, beta_1=0.9, beta_2=0.999, epsilon=1e-4):
    """Keras Adam (epsilon outside the bias correction), ascending; t the 1-based step count.  The step size is formed in float64 and
    rounded once to theta's dtype, as the library's host code does."""
    dt = theta.dtype.type
    m = dt(beta_1) * m + (dt(1) - dt(beta_1)) * grad
    v = dt(beta_2) * v + (dt(1) - dt(beta_2)) * grad * grad
    alpha = dt(float(lr) * np.sqrt(1.0 - float(beta_2) ** t) / (1.0 - float(beta_1) ** t))
    return theta + alpha * m / (np.sqrt(v) + dt(epsilon)), m, v


def restate(P, x, mu0, sigma0, eps, T, objective="elbo", lr=0.05, beta_1=0.9, beta_2=0.999, epsilon=1e-4, dtype=np.float64):
    """The whole call.  x [N, X]; mu0, sigma0 [N, D]; eps [T + E, S, N, D] (E may be 0: no evaluation).  Returns mu, sigma [N, D],
    bound [T, N], grad [N, 2 D] (the last iteration's), log_w [E S, N] (dtype), elbo, iwae [N] (float64)."""
    dec = R.decoder_of(P, dtype)
    x = np.asarray(x, dtype=dtype)
    mu = np.asarray(mu0, dtype=dtype).copy()
    rho = np.log(np.asarray(sigma0, dtype=dtype))
    eps = np.asarray(eps, dtype=dtype)
    E = eps.shape[0] - T
    S, N, D = eps.shape[1:]
    mm, vm, mr, vr = (np.zeros_like(mu) for _ in range(4))
    bound = np.zeros((T, N), dtype=dtype)
    grad = np.zeros((N, 2 * D), dtype=dtype)
    for t in range(T):
        bound[t], dmu, drho, _ = bound_and_grad(dec, x, mu, rho, eps[t], objective)
        grad = np.concatenate([dmu, drho], axis=1)
        mu, mm, vm = adam_ascent(mu, dmu, mm, vm, t + 1, lr, beta_1, beta_2, epsilon)
        rho, mr, vr = adam_ascent(rho, drho, mr, vr, t + 1, lr, beta_1, beta_2, epsilon)
    out = {"mu": mu, "sigma": np.exp(rho), "rho": rho, "bound": bound, "grad": grad}
    if E > 0:
        lw = np.concatenate([log_weights(dec, x, mu, rho, eps[T + j])[0] for j in range(E)], axis=0)
        l64 = lw.astype(np.float64)
        mx = l64.max(axis=0)
        out.update(log_w=lw, elbo=l64.mean(axis=0), iwae=mx + np.log(np.mean(np.exp(l64 - mx[None]), axis=0)))
    return out


def mean_se(log_w):
    """Standard error of the mean over axis 0 per image (float64)."""
    lw = np.asarray(log_w, dtype=np.float64)
    return lw.std(axis=0, ddof=1) / np.sqrt(lw.shape[0])


def exact_elbo(P, x, mu, sigma, n=801, extent=8.0):
    """ELBO[q] = E_q[log p(x, z) - log q(z)] of the Gaussian q = N(mu, diag sigma^2) per image on a model with TWO latent dimensions, by
    the rectangle rule on R.quadrature_log_px's n x n grid over [-extent, extent]^2 in float64 (q's mass on the grid divides the sum: it
    is 1 to rounding while the grid resolves sigma, spacing 0.02 at n = 801)."""
    dec = R.decoder_of(P, np.float64)
    g = np.linspace(-extent, extent, n)
    x, mu, sigma = (np.asarray(v, dtype=np.float64) for v in (x, mu, sigma))
    num, den = np.zeros(x.shape[0]), np.zeros(x.shape[0])
    for i in range(0, n, 50):
        zz = np.stack(np.meshgrid(g[i:i + 50], g, indexing="ij"), axis=-1).reshape(-1, 2)
        l = R.logits_of(dec, zz)[2]
        sp = np.sum(np.maximum(l, 0.0) + np.log1p(np.exp(-np.abs(l))), axis=1)
        lj = x @ l.T - sp[None] + (-0.5 * np.sum(zz * zz, axis=1) - 2 * R.HALF_LOG_2PI)[None]
        u = (zz[None] - mu[:, None]) / sigma[:, None]
        lq = np.sum(-0.5 * u * u - np.log(sigma)[:, None] - R.HALF_LOG_2PI, axis=-1)
        q = np.exp(lq)
        num += np.sum(q * (lj - lq), axis=1)
        den += np.sum(q, axis=1)
    return num / den
