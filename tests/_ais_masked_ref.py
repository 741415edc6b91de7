"""numpy restatement of iwae_ais_masked's and iwae_local_posterior_masked's formulas (include/iwae_amd.h), in the dtype given, and the case
tables of their tests: shared by tests/test_ais_masked_host.py, tests/test_gpu_ais_masked.py and tests/test_gpu_local_masked.py.  Not a
test module.

restate_ais and restate_local are tests/_ais_ref.py's and tests/_local_q_ref.py's restate with one change: log p(x|z) runs over the observed
pixels only and its gradient starts from s = m ? x - sigmoid(l) : 0.  Unobserved pixels are removed with np.where, never multiplied by the
mask, so a NaN in x at such a pixel reaches nothing.  With a mask of ones both equal the unmasked restatements exactly
(test_ais_masked_host.py)."""
import numpy as np

import _ais_ref as R
import _local_q_ref as LQ
import _masked_cases as MC

HALF_LOG_2PI = R.HALF_LOG_2PI


# ---------------------------------------------------------------- the row evaluation
def joint_and_grad(dec, xr, obs, z):
    """lj = log p(x_obs|z) + log p(z) per row and g = grad_z log p(x_obs|z) - z (R.joint_and_grad with the unobserved pixels selected out)."""
    dt = z.dtype.type
    (W1, b1), (W2, b2), (W3, b3) = dec
    g1, g2, l = R.logits_of(dec, z)
    ex = np.exp(-np.abs(l))
    xs = np.where(obs, xr, dt(0))
    lpx = np.sum(np.where(obs, xs * l - (np.maximum(l, dt(0)) + np.log1p(ex)), dt(0)), axis=1)
    sig = np.where(l >= 0, dt(1) / (dt(1) + ex), ex / (dt(1) + ex))
    d2 = (np.where(obs, xs - sig, dt(0)) @ W3.T) * (dt(1) - g2 * g2)
    d1 = (d2 @ W2.T) * (dt(1) - g1 * g1)
    dz = d1 @ W1.T
    D = z.shape[1]
    lj = lpx + (dt(-0.5) * np.sum(z * z, axis=1) - dt(D * HALF_LOG_2PI))
    return lj, dz - z


def restate_ais(P, x, mask, mu, sigma, betas, L, h, eps0, mom, unif, dtype=np.float64, adapt=False, z0=None):
    """R.restate with a mask [N, X] (non-zero = observed): the same arguments, the same outputs."""
    dt = np.dtype(dtype).type
    dec = R.decoder_of(P, dtype)
    C, N, D = eps0.shape
    T = len(betas) - 1
    Rn = C * N
    xr = np.tile(np.asarray(x, dtype=dtype), (C, 1))
    obs = np.tile(np.asarray(mask) != 0, (C, 1))
    mur = np.tile(np.asarray(mu, dtype=dtype), (C, 1))
    sgr = np.tile(np.asarray(sigma, dtype=dtype), (C, 1))
    b = np.asarray(betas, dtype=np.float32).astype(dtype)
    if z0 is None:
        e = np.asarray(eps0, dtype=dtype).reshape(Rn, D).copy()
    else:
        e = (np.asarray(z0, dtype=dtype).reshape(Rn, D) - mur) / sgr
    e0 = e.copy()
    momr = np.asarray(mom, dtype=dtype).reshape(T, Rn, D)
    ur = np.asarray(unif, dtype=dtype).reshape(T, Rn)
    hs = np.full(Rn, h, dtype=dtype)
    nacc = np.zeros(Rn, dtype=np.int64)
    log_w = np.zeros(Rn, dtype=np.float64)
    dH = np.zeros((T, Rn), dtype=dtype)
    margin = np.zeros((T, Rn), dtype=dtype)
    acc = np.zeros((T, Rn), dtype=np.uint8)

    def terms(ee):
        lj, g = joint_and_grad(dec, xr, obs, mur + sgr * ee)
        return lj, R.base_density(ee, sgr), g

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


def log_weights(dec, x, obs, mu, rho, e):
    """LQ.log_weights with the observed pixels obs [N, X]."""
    S, N, D = e.shape
    sg = np.exp(rho)
    er = e.reshape(S * N, D)
    xr, mur, sgr = np.tile(x, (S, 1)), np.tile(mu, (S, 1)), np.tile(sg, (S, 1))
    lj, g = joint_and_grad(dec, xr, np.tile(obs, (S, 1)), mur + sgr * er)
    lq = R.base_density(er, sgr)
    return (lj - lq).reshape(S, N), g.reshape(S, N, D), sg


def bound_and_grad(dec, x, obs, mu, rho, e, objective):
    """LQ.bound_and_grad with the observed pixels obs [N, X]."""
    dt = e.dtype.type
    S = e.shape[0]
    lw, g, sg = log_weights(dec, x, obs, mu, rho, e)
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


def restate_local(P, x, mask, mu0, sigma0, eps, T, objective="elbo", lr=0.05, beta_1=0.9, beta_2=0.999, epsilon=1e-4, dtype=np.float64):
    """LQ.restate with a mask [N, X] (non-zero = observed): the same arguments, the same outputs."""
    dec = R.decoder_of(P, dtype)
    x = np.asarray(x, dtype=dtype)
    obs = np.asarray(mask) != 0
    mu = np.asarray(mu0, dtype=dtype).copy()
    rho = np.log(np.asarray(sigma0, dtype=dtype))
    eps = np.asarray(eps, dtype=dtype)
    E = eps.shape[0] - T
    S, N, D = eps.shape[1:]
    mm, vm, mr, vr = (np.zeros_like(mu) for _ in range(4))
    bound = np.zeros((T, N), dtype=dtype)
    grad = np.zeros((N, 2 * D), dtype=dtype)
    for t in range(T):
        bound[t], dmu, drho, _ = bound_and_grad(dec, x, obs, mu, rho, eps[t], objective)
        grad = np.concatenate([dmu, drho], axis=1)
        mu, mm, vm = LQ.adam_ascent(mu, dmu, mm, vm, t + 1, lr, beta_1, beta_2, epsilon)
        rho, mr, vr = LQ.adam_ascent(rho, drho, mr, vr, t + 1, lr, beta_1, beta_2, epsilon)
    out = {"mu": mu, "sigma": np.exp(rho), "rho": rho, "bound": bound, "grad": grad}
    if E > 0:
        lw = np.concatenate([log_weights(dec, x, obs, mu, rho, eps[T + j])[0] for j in range(E)], axis=0)
        l64 = lw.astype(np.float64)
        mx = l64.max(axis=0)
        out.update(log_w=lw, elbo=l64.mean(axis=0), iwae=mx + np.log(np.mean(np.exp(l64 - mx[None]), axis=0)))
    return out


def quadrature_log_px(P, x, mask, n=801, extent=8.0):
    """log p(x_obs) of a model with TWO latent dimensions on R.quadrature_log_px's grid (float64), the unobserved pixels selected out."""
    dec = R.decoder_of(P, np.float64)
    g = np.linspace(-extent, extent, n)
    lw = 2.0 * np.log(g[1] - g[0])
    obs = np.asarray(mask) != 0
    xs = np.where(obs, np.asarray(x, dtype=np.float64), 0.0)
    run = np.full(xs.shape[0], -np.inf)
    for i in range(0, n, 50):
        zz = np.stack(np.meshgrid(g[i:i + 50], g, indexing="ij"), axis=-1).reshape(-1, 2)
        l = R.logits_of(dec, zz)[2]
        sp = np.maximum(l, 0.0) + np.log1p(np.exp(-np.abs(l)))
        lj = np.stack([l[:, o] @ xi[o] - np.sum(sp[:, o], axis=1) for xi, o in zip(xs, obs)])      # (the observed columns picked, not weighted)
        lj = lj + (-0.5 * np.sum(zz * zz, axis=1) - 2 * HALF_LOG_2PI)[None] + lw
        m = np.maximum(run, lj.max(axis=1))
        run = m + np.log(np.exp(run - m) + np.sum(np.exp(lj - m[:, None]), axis=1))
    return run


# ---------------------------------------------------------------- masks: the smallest at which the output layer's epilogue can go wrong
SHAPES = [(64, 8, 48), (37, 5, 53), (200, 100, 784)]
NMAX = 5


def mask_pass0(N, X, seed):
    """The first 64-pixel pass of the output layer unobserved in every image (its prod stays 1); where X <= 64 that is everything but the
    last pixel, so the cut last pass keeps one live term."""
    m = np.ones((N, X), np.uint8)
    m[:, :min(64, X - 1)] = 0
    return m


def mask_tile1(N, X, seed):
    """One whole 16-pixel tile (the second) unobserved."""
    m = np.ones((N, X), np.uint8)
    m[:, 16:32] = 0
    return m


def mask_last_only(N, X, seed):
    """Of the cut last tile only its last pixel observed (x_dim 53: of columns 48..52 only 52); the tiles before it whole."""
    m = np.ones((N, X), np.uint8)
    m[:, 16 * ((X - 1) // 16):X - 1] = 0
    return m


def mask_last_hole(N, X, seed):
    """Only the last pixel unobserved."""
    m = np.ones((N, X), np.uint8)
    m[:, X - 1] = 0
    return m


def mask_empty_next_to_full(N, X, seed):
    """Image 0 has nothing observed, image 1 everything, the rest 50 % MCAR: at N = 3, C = 7 all three share one wave's 16 rows."""
    m = MC.MR.case_mask(N, X, seed).copy() if N > 2 else np.ones((N, X), np.uint8)
    m = np.asarray(m, np.uint8).copy()
    m[0] = 0
    if N > 1:
        m[1] = 1
    return m


MASKS = {"pass0": mask_pass0, "tile1": mask_tile1, "last_only": mask_last_only, "last_hole": mask_last_hole, "empty_full": mask_empty_next_to_full,
         "tile": MC.mask_tile, "tophalf": MC.mask_tophalf, "none": MC.mask_none, "stripes64": MC.mask_stripes64, "dense95": MC.mask_dense95,
         "sparse05": MC.mask_sparse05}
# which structures run at which shape: every shape sees a dead pass or tile, the two MCAR rates and an empty image beside a full one;
# x_dim 53 the cut last tile both ways; x_dim 784 the 64-pixel stripes (whole passes dead in alternation) and one observed tile (11 of 13 passes dead)
SHAPE_MASKS = {(64, 8, 48): ("tile1", "empty_full", "dense95", "sparse05"),
               (37, 5, 53): ("last_only", "last_hole", "tile1", "empty_full"),
               (200, 100, 784): ("pass0", "stripes64", "tile", "empty_full", "dense95", "sparse05")}


def mask_of(name, N, X):
    return np.ascontiguousarray(MASKS[name](N, X, 17 + N + X), dtype=np.uint8)


# ---------------------------------------------------------------- single-transition cases (test_gpu_ais_masked.py::test_single_transition_parity)
SINGLE_CASES = [(1, 1), (1, 17), (3, 7), (5, 13)]                 # (N, C): row / tile / mixed / workgroup
SINGLE_IDS = ["row", "tile", "mixed", "workgroup"]
SINGLE_BETAS, SINGLE_H = [0.3, 0.7], 0.3                          # tests/_row_eval_bodies.py ais_single_transition's
# The noise seed of a case is that body's, 100 + 10 N + C + L, except where the run-time tolerance it yields on the CPU (8 x the float32
# restatement's dH deviation, floor 1e-5) is below ONE float32 ulp of the energy U_t the dH is a difference of: dH = ((U' + K') - U) - K is
# formed from float32 U's that each carry half an ulp of rounding whatever the summation order, so such a tolerance only says that the one
# chain of a (1, 1) case happened to round luckily in numpy.  test_ais_masked_host.py::test_single_transition_tolerances_resolve_the_energy
# holds every case to that; the three (1, 1) cases below missed it at the body's seed and take the next one in steps of 1000 that does not.
SINGLE_SEEDS = {((200, 100, 784), "pass0", 1, 1, 3, "encoder"): 1114, ((200, 100, 784), "dense95", 1, 1, 3, "prior"): 1114,
                ((200, 100, 784), "sparse05", 1, 1, 3, "prior"): 1114}


def single_seed(shape, mname, N, Cn, L, init):
    return SINGLE_SEEDS.get((tuple(shape), mname, N, Cn, L, init), 100 + 10 * N + Cn + L)


# ---------------------------------------------------------------- trajectory cases (test_gpu_ais_masked.py::test_trajectories)
# (nh, nl, xd, N, C, T, L, h, adapt, mask, seed): the noise seeds are picked on the CPU (test_ais_masked_host.py::test_trajectory_cases_are_admissible)
# so that the float32 and float64 restatements ALONE, under test_gpu_ais.py::test_trajectories' cut rule, cut at most 5 % of the chains
# short -- half the GPU test's 10 % cap -- and leave at least one whole chain.
TRAJECTORIES = {
    "h0.4": (64, 8, 48, 3, 24, 12, 4, 0.4, False, "dense95", 216),
    "h0.9": (64, 8, 48, 3, 24, 12, 4, 0.9, False, "empty_full", 321),
    "adapt": (64, 8, 48, 3, 24, 12, 4, 0.4, True, "sparse05", 301),
    "full": (200, 100, 784, 2, 20, 6, 3, 0.3, False, "stripes64", 209),
}


def first(mask):
    """Per chain: index of the first True along axis 0, or T."""
    T = mask.shape[0]
    return np.where(mask.any(axis=0), mask.argmax(axis=0), T)


def trajectory_cut(e32, e64):
    """test_gpu_ais.py::test_trajectories' cut rule on the two restatements: (dev_dH, delta, cut [C, N], scale, whole [C, N])."""
    T = e64["dH"].shape[0]
    tt = np.arange(T)[:, None, None]
    same = tt <= first(e32["accepted"] != e64["accepted"])[None]
    scale = np.maximum(1.0, np.abs(e64["dH"]))
    dev_dH = float(np.max((np.abs(e32["dH"].astype(np.float64) - e64["dH"]) / scale)[same]))
    delta = max(64.0 * dev_dH, 1e-4)
    cut = first(np.abs(e64["margin"]) < delta * scale)
    whole = (cut == T) & (first(e32["accepted"] != e64["accepted"]) == T)
    return dev_dH, delta, cut, scale, whole


# ---------------------------------------------------------------- local-posterior cases (test_gpu_local_masked.py)
# (nh, nl, xd, N, S, T, objective, mask)
LOCAL_CASES = [(64, 8, 48, 1, 1, 3, "elbo", "tile1"), (64, 8, 48, 3, 13, 6, "iwae", "empty_full"), (64, 8, 48, 2, 64, 4, "elbo", "sparse05"),
               (37, 5, 53, 5, 13, 6, "iwae", "last_only"), (37, 5, 53, 1, 13, 4, "elbo", "last_hole"),
               (200, 100, 784, 2, 64, 3, "elbo", "stripes64"), (200, 100, 784, 3, 13, 4, "iwae", "pass0"), (200, 100, 784, 5, 1, 4, "elbo", "dense95")]
