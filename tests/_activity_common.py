"""Helpers of the iwae_latent_activity GPU tests (tests/test_gpu_latent_activity.py, tests/test_gpu_ragged_widths.py): the float64
restatement of the statistic, the seeded set-up and the comparison with its tolerances.  Not a test module."""
import numpy as np

from oracle import iwae_np as O
import make_golden as MG


def _model(layers, nh, nl, xd, **kw):
    from iwae_amd.native import NativeModel
    return NativeModel(layers, nh, nl, x_dim=xd, seed=123, **kw)


def _block(p4, v, rnd):
    (W1, b1), (W2, b2), (Wm, bm), (Ws, bs) = p4
    h = rnd(np.tanh(rnd(v) @ rnd(W1) + b1))
    h = rnd(np.tanh(h @ rnd(W2) + b2))
    return h @ rnd(Wm) + bm, np.exp(h @ rnd(Ws) + bs) + 1e-6


def reference(P, x, eps=None, rnd=None):
    """float64 restatement: per-image means per layer, then activity and data mean (divide by N)."""
    rnd = rnd or (lambda a: np.asarray(a, dtype=np.float64))
    mu1, sig1 = _block(P[0:4], np.asarray(x, dtype=np.float64), rnd)
    means = [mu1]
    if eps is not None:
        z1 = mu1[None] + sig1[None] * np.asarray(eps, dtype=np.float64)          # [k, N, D1]
        mu2, _ = _block(P[4:8], z1.reshape(-1, z1.shape[-1]), rnd)
        means.append(mu2.reshape(z1.shape[0], z1.shape[1], -1).mean(axis=0))
    return {"post_mean": means, "activity": [m.var(axis=0) for m in means], "data_mean": [m.mean(axis=0) for m in means]}


def _setup(layers, nh, nl, xd, N, k, seed, prec):
    x, P, _ = MG.inputs(layers, nh, nl, xd, N, 1, seed)
    m = _model(layers, nh, nl, xd)
    m.set_params(O.flatten_params(P))
    m.set_eval_precision(prec)
    eps = None
    if layers == 2:
        eps = np.random.default_rng(seed + 9).standard_normal((k, N, nl[0])).astype(np.float32)
    return x, P, m, eps


def _check(r, e, prec):
    for l in range(len(e["activity"])):
        pm, em = r["post_mean"][l].astype(np.float64), e["post_mean"][l]
        a, ea = r["activity"][l], e["activity"][l]
        assert r["activity"][l].dtype == np.float64 and r["post_mean"][l].dtype == np.float32
        if prec == "fp32":
            assert np.max(np.abs(pm - em)) <= 1e-4, (l, np.max(np.abs(pm - em)))
            tol = 1e-4 * ea + 4e-6 * np.sqrt(ea) + 1e-9
            assert np.max(np.abs(r["data_mean"][l] - e["data_mean"][l])) <= 1e-4
        else:       # a bf16-ulp flip in a hidden activation moves a head by ~1e-3 (tests/test_gpu_parity.py)
            assert np.max(np.abs(pm - em)) <= 1e-2, (l, np.max(np.abs(pm - em)))
            tol = 2e-2 * ea + 1e-2 * np.sqrt(ea) + 1e-6
            assert np.max(np.abs(r["data_mean"][l] - e["data_mean"][l])) <= 1e-2
        assert np.all(np.abs(a - ea) <= tol), (l, np.max(np.abs(a - ea) - tol))
        np.testing.assert_allclose(a, pm.var(axis=0) if pm.shape[0] > 1 else 0.0, rtol=1e-5, atol=1e-9)
