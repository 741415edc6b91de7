"""numpy restatement of iwae_ais's formulas (include/iwae_amd.h), in the dtype given: shared by tests/test_ais_host.py and
tests/test_gpu_ais.py.  Not a test module.

Chain rows are r = c N + n (the [C, N] order of the ABI).  Every product and sum runs in `dtype`; log_w is accumulated in float64 from
increments formed in `dtype`, as the device does."""
import numpy as np

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def decoder_of(P, dtype):
    """The three Dense layers of the decoder (src/iwae1.py:72-75) out of the oracle's parameter list."""
    return [(np.asarray(W, dtype=dtype), np.asarray(b, dtype=dtype)) for W, b in P[-3:]]


def logits_of(dec, z):
    (W1, b1), (W2, b2), (W3, b3) = dec
    g1 = np.tanh(z @ W1 + b1)
    g2 = np.tanh(g1 @ W2 + b2)
    return g1, g2, g2 @ W3 + b3


def joint_and_grad(dec, xr, z):
    """lj = log p(x|z) + log p(z) per row and g = grad_z log p(x|z) - z."""
    dt = z.dtype.type
    (W1, b1), (W2, b2), (W3, b3) = dec
    g1, g2, l = logits_of(dec, z)
    ex = np.exp(-np.abs(l))
    lpx = np.sum(xr * l - (np.maximum(l, dt(0)) + np.log1p(ex)), axis=1)
    sig = np.where(l >= 0, dt(1) / (dt(1) + ex), ex / (dt(1) + ex))
    d2 = ((xr - sig) @ W3.T) * (dt(1) - g2 * g2)
    d1 = (d2 @ W2.T) * (dt(1) - g1 * g1)
    dz = d1 @ W1.T
    D = z.shape[1]
    lj = lpx + (dt(-0.5) * np.sum(z * z, axis=1) - dt(D * HALF_LOG_2PI))
    return lj, dz - z


def base_density(e, sg):
    dt = e.dtype.type
    D = e.shape[1]
    return dt(-0.5) * np.sum(e * e, axis=1) - np.sum(np.log(sg), axis=1) - dt(D * HALF_LOG_2PI)


def restate(P, x, mu, sigma, betas, L, h, eps0, mom, unif, dtype=np.float64, adapt=False, z0=None):
    """The whole run.  x [N, X]; mu, sigma [N, D] (prior init: zeros, ones); eps0 [C, N, D]; mom [T, C, N, D]; unif [T, C, N].
    Returns log_w [C, N] (float64), z [C, N, D], dH, margin = log u + dH, accepted [T, C, N], step [C, N], e0 [C, N, D]."""
    dt = np.dtype(dtype).type
    dec = decoder_of(P, dtype)
    C, N, D = eps0.shape
    T = len(betas) - 1
    R = C * N
    xr = np.tile(np.asarray(x, dtype=dtype), (C, 1))
    mur = np.tile(np.asarray(mu, dtype=dtype), (C, 1))
    sgr = np.tile(np.asarray(sigma, dtype=dtype), (C, 1))
    b = np.asarray(betas, dtype=np.float32).astype(dtype)
    if z0 is None:
        e = np.asarray(eps0, dtype=dtype).reshape(R, D).copy()
    else:
        e = (np.asarray(z0, dtype=dtype).reshape(R, D) - mur) / sgr
    e0 = e.copy()
    momr = np.asarray(mom, dtype=dtype).reshape(T, R, D)
    ur = np.asarray(unif, dtype=dtype).reshape(T, R)
    hs = np.full(R, h, dtype=dtype)
    nacc = np.zeros(R, dtype=np.int64)
    log_w = np.zeros(R, dtype=np.float64)
    dH = np.zeros((T, R), dtype=dtype)
    margin = np.zeros((T, R), dtype=dtype)
    acc = np.zeros((T, R), dtype=np.uint8)

    def terms(ee):
        lj, g = joint_and_grad(dec, xr, mur + sgr * ee)
        return lj, base_density(ee, sgr), g

    for t in range(1, T + 1):
        bt, bp = b[t], b[t - 1]

        def grad_u(ee, g):
            return (dt(1) - bt) * ee - bt * (sgr * g)

        lj, l0, g = terms(e)
        log_w += np.float64(bt - bp) * (lj - l0).astype(np.float64)
        u0 = -((dt(1) - bt) * l0 + bt * lj)
        p = momr[t - 1].copy()
        k0 = dt(0.5) * np.sum(p * p, axis=1)
        en = e.copy()
        p = p - (dt(0.5) * hs)[:, None] * grad_u(en, g)
        for l in range(L):
            en = en + hs[:, None] * p
            lj1, l01, g1 = terms(en)
            step = dt(0.5) * hs if l == L - 1 else hs
            p = p - step[:, None] * grad_u(en, g1)
        k1 = dt(0.5) * np.sum(p * p, axis=1)
        u1 = -((dt(1) - bt) * l01 + bt * lj1)
        d = ((u1 + k1) - u0) - k0
        with np.errstate(invalid="ignore"):
            take = np.log(ur[t - 1]) < -d
        dH[t - 1], margin[t - 1], acc[t - 1] = d, np.log(ur[t - 1]) + d, take
        e = np.where(take[:, None], en, e)
        nacc += take
        if adapt:
            mean = (nacc / t).astype(dtype)
            hs = np.clip(hs * np.where(mean > dt(0.65), dt(1.02), dt(0.98)), dt(1e-4), dt(0.5)).astype(dtype)
    return {"log_w": log_w.reshape(C, N), "z": (mur + sgr * e).reshape(C, N, D), "dH": dH.reshape(T, C, N), "margin": margin.reshape(T, C, N),
            "accepted": acc.reshape(T, C, N), "step": hs.reshape(C, N), "e0": e0.reshape(C, N, D)}


def log_mean_exp(log_w):
    """Over the chain axis 0 -> [N] (float64)."""
    m = log_w.max(axis=0)
    return m + np.log(np.mean(np.exp(log_w - m[None]), axis=0))


def log_mean_se(log_w):
    """Delta-method standard error of log mean_c exp(log_w) per image: std(w) / (mean(w) sqrt(C))."""
    w = np.exp(log_w - log_w.max(axis=0)[None])
    return w.std(axis=0, ddof=1) / (w.mean(axis=0) * np.sqrt(w.shape[0]))


def quadrature_log_px(P, x, n=801, extent=8.0):
    """log p(x) of a model with TWO latent dimensions on an n x n uniform grid over [-extent, extent]^2 (float64): the integrand is smooth
    and decays like the N(0, I) prior, so the rectangle rule converges geometrically; at n = 801 (spacing 0.02) it is exact to ~1e-12."""
    dec = decoder_of(P, np.float64)
    g = np.linspace(-extent, extent, n)
    lw = 2.0 * np.log(g[1] - g[0])
    x = np.asarray(x, dtype=np.float64)
    run = np.full(x.shape[0], -np.inf)
    for i in range(0, n, 50):
        zz = np.stack(np.meshgrid(g[i:i + 50], g, indexing="ij"), axis=-1).reshape(-1, 2)
        l = logits_of(dec, zz)[2]
        sp = np.sum(np.maximum(l, 0.0) + np.log1p(np.exp(-np.abs(l))), axis=1)
        lj = x @ l.T - sp[None] + (-0.5 * np.sum(zz * zz, axis=1) - 2 * HALF_LOG_2PI)[None] + lw
        m = np.maximum(run, lj.max(axis=1))
        run = m + np.log(np.exp(run - m) + np.sum(np.exp(lj - m[:, None]), axis=1))
    return run


def noise(seed, T, C, N, D):
    rng = np.random.default_rng(seed)
    eps0 = rng.standard_normal((C, N, D)).astype(np.float32)
    mom = rng.standard_normal((T, C, N, D)).astype(np.float32)
    unif = ((rng.integers(0, 1 << 24, (T, C, N)).astype(np.float64) + 0.5) * 2.0 ** -24).astype(np.float32)      # the device generator's grid
    return eps0, mom, unif
