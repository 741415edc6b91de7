"""The bodies of the row-evaluation analyses' GPU parity tests (iwae_ais, iwae_local_posterior, iwae_impute, iwae_posterior), shared by
their own modules (tests/test_gpu_ais.py, test_gpu_local_q.py, test_gpu_impute.py, test_gpu_posterior.py: the shapes (64, 8, 48),
(200, 100, 784), (37, 5, 53)) and tests/test_gpu_aspect.py (inverted and exact-tile widths).  A module supplies the handle, the images and
the parameters.  Not a test module.

The expected values are float64 restatements on the DEVICE'S OWN q_mu, q_sigma and the noise passed in.  Tolerances are set at run time:
8 x the largest deviation of a float32 numpy run of the same restatement from its float64 run on the same inputs, floor 1e-5.
"""
import ctypes as C

import numpy as np

import _ais_ref as R
import _local_q_ref as LQ
import _impute_ref as IM
import _posterior_ref as PR


def _tol(a32, a64, floor=1e-5):
    return max(8.0 * float(np.max(np.abs(np.asarray(a32, dtype=np.float64) - np.asarray(a64, dtype=np.float64)))), floor)


# ---------------------------------------------------------------- iwae_ais
AIS_KEYS = ("log_w", "z", "step_size", "dH", "accepted", "log_px", "ess", "accept_rate")


def ais_single_transition(m, x, P, nl, N, Cn, L, init):
    """One transition at betas [0.3, 0.7]: dH, log_w and (where the accept decision is resolved) z and the decision itself."""
    x = x[:N]
    betas, h = [0.3, 0.7], 0.3
    eps0, mom, unif = R.noise(100 + 10 * N + Cn + L, 1, Cn, N, nl)
    r = m.ais(x, n_chains=Cn, leapfrog=L, step_size=h, adapt=False, init=init, betas=betas, noise=(eps0, mom, unif), trace=True)
    if init == "prior":
        assert np.array_equal(r["q_mu"], np.zeros((N, nl), np.float32)) and np.array_equal(r["q_sigma"], np.ones((N, nl), np.float32))
    mu, sg = r["q_mu"], r["q_sigma"]
    e64 = R.restate(P, x, mu, sg, betas, L, h, eps0, mom, unif, np.float64)
    e32 = R.restate(P, x, mu, sg, betas, L, h, eps0, mom, unif, np.float32)
    assert r["dH"].shape == (1, Cn, N) and r["z"].shape == (Cn, N, nl) and r["log_w"].shape == (Cn, N) and r["log_w"].dtype == np.float64
    resolved = np.abs(e64["margin"][0]) > 1e-4                    # [C, N]: the decision does not hinge on float32 rounding
    for key in ("dH", "log_w", "z"):
        dev, w64, w32 = (np.asarray(a[key], dtype=np.float64) for a in (r, e64, e32))
        if key == "z":
            dev, w64, w32 = dev[resolved], w64[resolved], w32[resolved]
        tol = _tol(w32, w64)
        err = float(np.max(np.abs(dev - w64))) if dev.size else 0.0
        print("%s: device error %.3g, float32 restatement %.3g, tolerance %.3g" % (key, err, tol / 8.0, tol))
        assert err <= tol, (key, err, tol)
    assert np.array_equal(r["accepted"][0][resolved], e64["accepted"][0][resolved])
    assert np.array_equal(r["step_size"], np.full((Cn, N), h, np.float32))
    np.testing.assert_allclose(r["log_px"], R.log_mean_exp(r["log_w"]), rtol=1e-12, atol=1e-12)


def ais_chunking_position_and_repeat_are_bitwise(m, x):
    N, Cn, T = 5, 13, 5
    kw = dict(n_chains=Cn, leapfrog=2, step_size=0.35, adapt=True, betas=np.linspace(0, 1, T + 1), trace=True)
    runs = []
    for chunk in (0, 1, 2, 0):                                    # default, 1, 2, and the default again (a repeat of the same call)
        m.set_option("ais_t_chunk", chunk)
        m.set_step(3, 20)
        runs.append(m.ais(x, **kw))
    m.set_option("ais_t_chunk", 0)
    for other in runs[1:]:
        for key in AIS_KEYS:
            assert np.array_equal(runs[0][key], other[key]), key
    assert 0 < runs[0]["accepted"].mean() and len(np.unique(runs[0]["step_size"])) > 1
    # image 2 alone, told its global index, against the same image inside N = 5
    m.set_step(3, 22)
    one = m.ais(x[2:3], **kw)
    for key in ("log_w", "step_size", "log_px", "ess"):
        assert np.array_equal(one[key].reshape(one[key].shape[:-1]), runs[0][key][..., 2]), key
    for key in ("dH", "accepted"):
        assert np.array_equal(one[key][..., 0], runs[0][key][..., 2]), key
    assert np.array_equal(one["z"][:, 0], runs[0]["z"][:, 2])


# ---------------------------------------------------------------- iwae_local_posterior
LOCAL_KEYS = ("grad", "bound", "mu", "sigma", "elbo", "iwae", "log_w")


def local_compare(r, e64, e32, keys=LOCAL_KEYS):
    for key in keys:
        dev, w64, w32 = (np.asarray(a[key], dtype=np.float64) for a in (r, e64, e32))
        assert dev.shape == w64.shape, (key, dev.shape, w64.shape)
        tol = _tol(w32, w64)
        err = float(np.max(np.abs(dev - w64)))
        print("%s: device error %.3g, float32 restatement %.3g, tolerance %.3g" % (key, err, tol / 8.0, tol))
        assert err <= tol, (key, err, tol)


def local_noise(N, S, T, nl, E=2, seed=None):
    return np.random.default_rng(100 + 10 * N + S + T if seed is None else seed).standard_normal((T + E, S, N, nl)).astype(np.float32)


def local_iteration_parity(m, x, P, nl, N, S, T, objective, seed=None):
    x = x[:N]
    E = 2
    noise = local_noise(N, S, T, nl, E, seed)
    r = m.local_posterior(x, n_samples=S, n_iters=T, n_eval=E, objective=objective, lr=0.05, noise=noise, trace=True)
    assert r["bound"].shape == (T, N) and r["grad"].shape == (N, 2 * nl) and r["log_w"].shape == (E * S, N) and r["elbo"].dtype == np.float64
    e64 = LQ.restate(P, x, r["q_mu"], r["q_sigma"], noise, T, objective, lr=0.05, dtype=np.float64)
    e32 = LQ.restate(P, x, r["q_mu"], r["q_sigma"], noise, T, objective, lr=0.05, dtype=np.float32)
    local_compare(r, e64, e32)
    # the two outputs of the evaluation are what log_w says they are
    lw = r["log_w"].astype(np.float64)
    np.testing.assert_allclose(r["elbo"], lw.mean(axis=0), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r["iwae"], R.log_mean_exp(lw), rtol=1e-12, atol=1e-12)


def local_chunking_position_and_repeat_are_bitwise(m, x):
    N, S, T = 5, 13, 10
    kw = dict(n_samples=S, n_iters=T, n_eval=2, objective="iwae", lr=0.05, trace=True)
    runs = []
    for chunk in (0, 1, 3, 0):                                    # default, 1, 3, and the default again (a repeat of the same call)
        m.set_option("local_t_chunk", chunk)
        m.set_step(3, 20)
        runs.append(m.local_posterior(x, **kw))
    m.set_option("local_t_chunk", 0)
    for other in runs[1:]:
        for key in LOCAL_KEYS + ("q_mu", "q_sigma"):
            assert np.array_equal(runs[0][key], other[key]), key
    assert not np.array_equal(runs[0]["mu"], runs[0]["q_mu"])
    # image 2 alone, told its global index, against the same image inside N = 5
    m.set_step(3, 22)
    one = m.local_posterior(x[2:3], **kw)
    for key in ("mu", "sigma", "q_mu", "q_sigma", "grad", "elbo", "iwae"):
        assert np.array_equal(one[key][0], runs[0][key][2]), key
    for key in ("bound", "log_w"):
        assert np.array_equal(one[key][:, 0], runs[0][key][:, 2]), key


# ---------------------------------------------------------------- iwae_impute
IMPUTE_KEYS = ("log_px", "xhat", "ess", "log_w", "q_mu", "q_sigma")


def _close(name, dev, w64, w32):
    dev, w64 = np.asarray(dev, dtype=np.float64), np.asarray(w64, dtype=np.float64)
    assert dev.shape == w64.shape, (name, dev.shape, w64.shape)
    tol = _tol(w32, w64)
    err = float(np.max(np.abs(dev - w64)))
    print("%s: device error %.3g, float32 restatement %.3g, tolerance %.3g" % (name, err, tol / 8.0, tol))
    assert err <= tol, (name, err, tol)


def same(a, b, keys):
    for key in keys:
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), key


def impute_run(m, x, P, mask, nl, N, k):
    """The device's outputs and the two restatements at the device's heads."""
    x, mask = x[:N], mask[:N]
    eps = IM.draws(N, k, nl)
    r = m.impute(x, mask=mask, n_samples=k, noise=eps)
    e64 = IM.restate(P, x, mask, r["q_mu"], r["q_sigma"], eps, np.float64)
    e32 = IM.restate(P, x, mask, r["q_mu"], r["q_sigma"], eps, np.float32)
    return r, e64, e32


def impute_weight_parity(run, N, k, xd):
    r, e64, e32 = run
    assert r["log_w"].shape == (k, N) and r["log_px"].dtype == np.float64 and r["xhat"].shape == (N, xd) and r["ess"].shape == (N,)
    for key in ("log_w", "log_px", "ess"):
        _close(key, r[key], e64[key], e32[key])
    # log_px and ess are what the device's own log_w says they are
    lw = r["log_w"].astype(np.float64)
    al = np.exp(lw - lw.max(axis=0)[None])
    al /= al.sum(axis=0)[None]
    np.testing.assert_allclose(r["log_px"], lw.max(axis=0) + np.log(np.mean(np.exp(lw - lw.max(axis=0)[None]), axis=0)), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r["ess"], 1.0 / np.sum(al * al, axis=0), rtol=1e-6)


def impute_imputation_parity(run):
    """xhat against sum_s softmax(DEVICE log_w)_s p64_s: the error of log_w (bounded above) is not charged to xhat."""
    r, e64, e32 = run
    lw = r["log_w"].astype(np.float64)
    al = np.exp(lw - lw.max(axis=0)[None])
    al /= al.sum(axis=0)[None]
    want = np.sum(al[:, :, None] * e64["p"], axis=0)
    tol = _tol(e32["xhat"], e64["xhat"])
    err = float(np.max(np.abs(r["xhat"].astype(np.float64) - want)))
    print("xhat: device error %.3g, float32 restatement %.3g, tolerance %.3g; off the unweighted mean %.3g"
          % (err, tol / 8.0, tol, float(np.max(np.abs(want - e64["p"].mean(axis=0))))))
    assert err <= tol, (err, tol)
    assert np.all(r["xhat"] >= 0.0) and np.all(r["xhat"] <= 1.0)


def impute_nothing_past_the_last_pixel(m, x, mask, nl, xd, base_of, cases=((5, 13), (2, 65))):
    """xhat into a device array with a guard row of sentinels behind it -- through the raw binding, both chunkings of the sum.  base_of(N, k):
    the outputs of the same call through the Python level."""
    import torch
    from iwae_amd import _capi
    for N, k in cases:
        xs, mk = np.ascontiguousarray(x[:N]), np.ascontiguousarray(mask[:N], dtype=np.uint8)
        eps = IM.draws(N, k, nl)
        guard = torch.full((N + 1, xd), -7.0, dtype=torch.float32, device="cuda")
        lpx = np.zeros(N, dtype=np.float64)
        o = _capi.ImputeOptions()
        o.k, o.mask, o.eps = k, mk.ctypes.data, eps.ctypes.data
        outs = _capi.ImputeOutputs()
        outs.log_px, outs.xhat = lpx.ctypes.data, guard.data_ptr()
        assert m.lib.iwae_impute(m.h, xs.ctypes.data, N, C.byref(o), C.byref(outs)) == 0
        torch.cuda.synchronize()
        g = guard.cpu().numpy()
        assert np.all(g[N] == -7.0)
        assert np.array_equal(g[:N], base_of(N, k)["xhat"])


def impute_position_chunking_and_repeat_are_bitwise(m, x, mask, nl, k, base=None):
    N = 5
    eps = IM.draws(N, k, nl)
    if base is None:
        base = m.impute(x, mask=mask, n_samples=k, noise=eps)
    same(base, m.impute(x, mask=mask, n_samples=k, noise=eps), IMPUTE_KEYS)           # a repeat
    m.set_option("impute_rows", k)                                                    # one image per launch
    one_per_launch = m.impute(x, mask=mask, n_samples=k, noise=eps)
    m.set_option("impute_rows", 0)
    same(base, one_per_launch, IMPUTE_KEYS)
    for n in range(N):                                                                # every image alone, with its own draws
        one = m.impute(x[n:n + 1], mask=mask[n:n + 1], n_samples=k, noise=np.ascontiguousarray(eps[:, n:n + 1]))
        for key in ("xhat", "ess", "log_px", "q_mu", "q_sigma"):
            assert np.array_equal(one[key][0], base[key][n]), (key, n)
        assert np.array_equal(one["log_w"][:, 0], base["log_w"][:, n]), n
    no_xhat = m.impute(x, mask=mask, n_samples=k, noise=eps, outputs=("log_px", "ess", "log_w", "q_mu", "q_sigma"))
    assert "xhat" not in no_xhat
    same(base, no_xhat, ("log_px", "ess", "log_w", "q_mu", "q_sigma"))


# ---------------------------------------------------------------- iwae_posterior
POSTERIOR_KEYS = ("log_px", "ess", "mean", "cov", "idx", "z", "u", "log_w", "q_mu", "q_sigma")
R0 = 7


def unif(R, N, k=0):
    return np.random.default_rng(500 + 10 * N + R + k).random((R, N)).astype(np.float32)


def posterior_run(m, x, P, mask, nl, N, k):
    """The device's outputs (masked, the caller's draws and uniforms, R0 resampled draws) and the two restatements at the device's heads."""
    x, mask = x[:N], mask[:N]
    eps = IM.draws(N, k, nl)
    r = m.posterior(x, mask=mask, n_samples=k, n_draws=R0, noise=eps, uniforms=unif(R0, N))
    e64 = PR.restate(P, x, mask, r["q_mu"], r["q_sigma"], eps, np.float64)
    e32 = PR.restate(P, x, mask, r["q_mu"], r["q_sigma"], eps, np.float32)
    return r, e64, e32


def posterior_moment_parity(m, x, mask, nl, N, k, run):
    r, e64, e32 = run
    assert r["mean"].shape == (N, nl) and r["cov"].shape == (N, nl, nl) and r["mean"].dtype == np.float32 and r["cov"].dtype == np.float32
    want = PR.moments(PR.weights(r["log_w"], np.float64), r["q_mu"], r["q_sigma"], IM.draws(N, k, nl), np.float64)
    for key in ("mean", "cov"):
        tol = _tol(e32[key], e64[key])
        err = float(np.max(np.abs(r[key].astype(np.float64) - want[key])))
        print("%s: device error %.3g, float32 restatement %.3g, tolerance %.3g" % (key, err, tol / 8.0, tol))
        assert err <= tol, (key, err, tol)
    assert np.array_equal(r["cov"], np.swapaxes(r["cov"], 1, 2))
    assert np.all(np.diagonal(r["cov"], axis1=1, axis2=2) >= 0.0)
    no_cov = m.posterior(x[:N], mask=mask[:N], n_samples=k, noise=IM.draws(N, k, nl), outputs=("mean",))
    assert "cov" not in no_cov and np.array_equal(no_cov["mean"], r["mean"])


def posterior_nothing_past_the_last_feature(m, x, mask, nl, base_of, cases=((5, 13), (2, 65))):
    """cov [N, D, D], mean [N, D], z [R, N, D] and idx [R, N] into device arrays with a guard row of sentinels behind them, through the raw
    binding, one chunk per image and two.  base_of(N, k): the outputs of the same call through the Python level."""
    import torch
    from iwae_amd import _capi
    for N, k in cases:
        xs, mk = np.ascontiguousarray(x[:N]), np.ascontiguousarray(mask[:N], dtype=np.uint8)
        eps, u = IM.draws(N, k, nl), unif(R0, N)
        cov = torch.full((N + 1, nl, nl), -7.0, dtype=torch.float32, device="cuda")
        mean = torch.full((N + 1, nl), -7.0, dtype=torch.float32, device="cuda")
        z = torch.full((R0 * N + 1, nl), -7.0, dtype=torch.float32, device="cuda")
        idx = torch.full((R0 * N + 1,), -7, dtype=torch.int32, device="cuda")
        lpx = np.zeros(N, dtype=np.float64)
        o = _capi.PosteriorOptions()
        o.k, o.R, o.mask, o.eps, o.unif = k, R0, mk.ctypes.data, eps.ctypes.data, u.ctypes.data
        outs = _capi.PosteriorOutputs()
        outs.log_px, outs.cov, outs.mean, outs.z, outs.idx = lpx.ctypes.data, cov.data_ptr(), mean.data_ptr(), z.data_ptr(), idx.data_ptr()
        assert m.lib.iwae_posterior(m.h, xs.ctypes.data, N, C.byref(o), C.byref(outs)) == 0
        torch.cuda.synchronize()
        base = base_of(N, k)
        for name, got, rows in (("cov", cov, N), ("mean", mean, N), ("z", z, R0 * N), ("idx", idx, R0 * N)):
            g = got.cpu().numpy()
            assert np.all(g[rows] == -7), name
            assert np.array_equal(g[:rows].reshape(base[name].shape), base[name]), name


def posterior_indices_and_draws(m, x, mask, nl, N, k, R, eps, w):
    """idx, z and u of R resampled draws on the weights of a call without resampling (w: its log_w and heads)."""
    u = unif(R, N, k)
    r = m.posterior(x[:N], mask=mask[:N], n_samples=k, n_draws=R, noise=eps, uniforms=u)
    assert np.array_equal(r["log_w"], w["log_w"])
    assert r["idx"].dtype == np.int32 and r["idx"].shape == (R, N) and r["z"].shape == (R, N, nl)
    assert np.array_equal(r["idx"], PR.indices(r["log_w"], u))
    assert np.array_equal(r["u"], u)
    want = r["q_mu"].astype(np.float64)[None] + r["q_sigma"].astype(np.float64)[None] * eps.astype(np.float64)[r["idx"], np.arange(N)[None]]
    np.testing.assert_allclose(r["z"], want, rtol=1e-6, atol=1e-6)
    flat_idx, flat_z = r["idx"].T.reshape(N, R), np.swapaxes(r["z"], 0, 1)
    for n in range(N):                                             # rows with equal idx are bitwise equal
        first = {}
        for j, s in enumerate(flat_idx[n]):
            assert np.array_equal(flat_z[n, j], flat_z[n, first.setdefault(int(s), j)]), (n, j)


def posterior_position_chunking_and_repeat_are_bitwise(m, x, mask, nl, k, base):
    N = 5
    eps, u = IM.draws(N, k, nl), unif(R0, N)
    call = lambda xs: m.posterior(xs, mask=mask, n_samples=k, n_draws=R0, noise=eps, uniforms=u)      # noqa: E731
    same(base, call(x), POSTERIOR_KEYS)                                               # a repeat
    m.set_option("impute_rows", k)                                                    # one image per launch
    one_per_launch = call(x)
    m.set_option("impute_rows", 0)
    same(base, one_per_launch, POSTERIOR_KEYS)
    for n in range(N):                                                                # every image alone, with its own draws and uniforms
        one = m.posterior(x[n:n + 1], mask=mask[n:n + 1], n_samples=k, n_draws=R0, noise=np.ascontiguousarray(eps[:, n:n + 1]),
                          uniforms=np.ascontiguousarray(u[:, n:n + 1]))
        for key in ("log_px", "ess", "mean", "cov", "q_mu", "q_sigma"):
            assert np.array_equal(one[key][0], base[key][n]), (key, n)
        for key in ("log_w", "idx", "z", "u"):
            assert np.array_equal(one[key][:, 0], base[key][:, n]), (key, n)
    xn = np.where(mask, x, np.float32(np.nan)).astype(np.float32)                     # what x holds at an unobserved pixel reaches nothing
    assert np.isnan(xn).any()
    same(base, call(xn), POSTERIOR_KEYS)
