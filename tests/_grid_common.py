"""Helpers of the iwae_grid_posterior GPU tests (tests/test_gpu_grid_posterior.py, tests/test_gpu_aspect.py): the float64 restatement
built on the oracle's densities, the seeded grid and the float32 parity body with its bounds.  Not a test module.

The restatement: lj(i, g) = sum_j bernoulli_log_prob(x_ij, l_gj) + sum_d normal_log_prob(z_gd, 0, 1) (src/iwae1.py:105-111),
log_px = logsumexp_g(lj + w_g); moments, q_mass and KL(q || p(z|x)) as the header defines them.
"""
import numpy as np

from oracle import iwae_np as O
import make_golden as MG


def _model(nh, nl, x_dim=784, **kw):
    from iwae_amd.native import NativeModel
    return NativeModel(1, nh, nl, x_dim=x_dim, seed=123, **kw)


def _lse(a, axis):
    m = np.max(a, axis=axis, keepdims=True)
    return np.squeeze(m, axis) + np.log(np.sum(np.exp(a - m), axis=axis))


def reference(P, x, z, lw, rnd=None):
    """float64 restatement (rnd = O.bf16_round: the bf16 eval precision's rounding points)."""
    rnd = rnd or (lambda a: np.asarray(a, dtype=np.float64))
    (W1, b1), (W2, b2), (Wm, bm), (Ws, bs), (V1, c1), (V2, c2), (V3, c3) = P
    x = np.asarray(x, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    h = rnd(np.tanh(rnd(x) @ rnd(W1) + b1))
    h = rnd(np.tanh(h @ rnd(W2) + b2))
    mu, sigma = h @ rnd(Wm) + bm, np.exp(h @ rnd(Ws) + bs) + 1e-6                      # src/iwae1.py:39-42
    g = rnd(np.tanh(rnd(z) @ rnd(V1) + c1))
    g = rnd(np.tanh(g @ rnd(V2) + c2))
    logits = g @ rnd(V3) + c3                                                           # src/iwae1.py:72-75
    lpxz = x @ logits.T - np.sum(O.softplus(logits), axis=1)[None, :]                  # = sum_j bernoulli_log_prob
    lj = lpxz + np.sum(O.normal_log_prob(z, 0.0, 1.0), axis=1)[None, :]
    lw = np.zeros(z.shape[0]) if lw is None else np.asarray(lw, dtype=np.float64)
    lpx = _lse(lj + lw[None, :], 1)
    pi = np.exp(lj + lw[None, :] - lpx[:, None])
    mean = pi @ z
    dz = z[None, :, :] - mean[:, None, :]
    cov = np.einsum("ng,ngd,nge->nde", pi, dz, dz)
    lq = np.sum(O.normal_log_prob(z[None, :, :], mu[:, None, :], sigma[:, None, :]), axis=-1)
    qw = np.exp(lq + lw[None, :])
    return {"log_px": lpx, "post_mean": mean, "post_cov": cov, "q_mu": mu, "q_sigma": sigma, "q_mass": qw.sum(1),
            "kl_q_post": np.sum(qw * (lq - lj + lpx[:, None]), axis=1), "log_joint": lj}


def _grid_case(N, G, D, seed):
    rng = np.random.default_rng(seed)
    z = rng.uniform(-3.0, 3.0, (G, D)).astype(np.float32)
    lw = np.log(rng.uniform(0.5, 1.5, G) * 6.0 ** D / G).astype(np.float32)        # non-uniform weights
    return z, lw


def float32_matches_float64(nh, nl, xd, N=37, G=1531):
    x, P, _ = MG.inputs(1, nh, nl, xd, N, 1, 700 + nl + xd)
    z, lw = _grid_case(N, G, nl, 11 + nl)
    m = _model(nh, nl, xd)
    m.set_params(O.flatten_params(P))
    r = m.grid_posterior(x, z, lw, log_joint=True)
    e = reference(P, x, z, lw)
    d = {key: float(np.max(np.abs(r[key] - e[key]))) for key in ("log_px", "kl_q_post", "log_joint", "post_mean", "post_cov", "q_mass")}
    print("grid posterior (%d, %d, %d): log_px %.3g, kl_q_post %.3g, log_joint %.3g (<= 2e-3), post_mean %.3g, post_cov %.3g (<= 1e-3), q_mass %.3g (<= 1e-4)"
          % (nh, nl, xd, d["log_px"], d["kl_q_post"], d["log_joint"], d["post_mean"], d["post_cov"], d["q_mass"]))
    assert r["log_px"].dtype == np.float64
    assert np.max(np.abs(r["log_px"] - e["log_px"])) <= 2e-3
    assert np.max(np.abs(r["kl_q_post"] - e["kl_q_post"])) <= 2e-3
    assert np.max(np.abs(r["log_joint"] - e["log_joint"])) <= 2e-3
    assert np.max(np.abs(r["post_mean"] - e["post_mean"])) <= 1e-3
    assert np.max(np.abs(r["post_cov"] - e["post_cov"])) <= 1e-3
    assert np.max(np.abs(r["q_mass"] - e["q_mass"])) <= 1e-4
    np.testing.assert_allclose(r["q_mu"], e["q_mu"], atol=1e-4)
    np.testing.assert_allclose(r["q_sigma"], e["q_sigma"], rtol=1e-4, atol=1e-6)
    m.close()
