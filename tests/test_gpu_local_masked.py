"""iwae_local_posterior_masked (include/iwae_amd.h): the best factorised Gaussian for p(z | x_obs) of incomplete images.

The expected values are the float64 restatement of tests/_ais_masked_ref.py on the DEVICE'S OWN q_mu, q_sigma and the noise passed in;
tolerances are tests/test_gpu_local_q.py's, set at run time (8 x the float32 restatement's deviation from the float64 one, floor 1e-5).  The
cases are tests/_ais_masked_ref.py LOCAL_CASES, which tests/test_ais_masked_host.py holds well conditioned on the CPU."""
import ctypes as C

import numpy as np
import pytest

from oracle import iwae_np as O
import make_golden as MG
import _ais_ref as R
import _local_q_ref as LQ
import _row_eval_bodies as RB
import _ais_masked_ref as AM

pytestmark = pytest.mark.gpu

NMAX = AM.NMAX
_cache = {}
_tol = RB._tol
KEYS = RB.LOCAL_KEYS + ("q_mu", "q_sigma")


def _net(nh, nl, xd):
    key = (nh, nl, xd)
    if key not in _cache:
        from iwae_amd.native import NativeModel
        x, P, _ = MG.inputs(1, nh, nl, xd, NMAX, 1, 7 + nh)
        m = NativeModel(1, nh, nl, x_dim=xd, seed=123)
        m.set_params(O.flatten_params(P))
        m.set_eval_precision("fp32")
        _cache[key] = (m, x, P)
    return _cache[key]


def _same(a, b, keys=KEYS):
    for key in keys:
        assert np.array_equal(a[key], b[key]), key


# ---------------------------------------------------------------- 1. iterations and evaluation against float64
@pytest.mark.parametrize("case", AM.LOCAL_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_iteration_parity(gpu, case):
    nh, nl, xd, N, S, T, objective, mname = case
    m, x, P = _net(nh, nl, xd)
    x = x[:N]
    mask = AM.mask_of(mname, N, xd)
    E = 2
    noise = RB.local_noise(N, S, T, nl, E)
    r = m.local_posterior(x, mask=mask, n_samples=S, n_iters=T, n_eval=E, objective=objective, lr=0.05, noise=noise, trace=True)
    assert r["bound"].shape == (T, N) and r["grad"].shape == (N, 2 * nl) and r["log_w"].shape == (E * S, N) and r["elbo"].dtype == np.float64
    e64 = AM.restate_local(P, x, mask, r["q_mu"], r["q_sigma"], noise, T, objective, lr=0.05, dtype=np.float64)
    e32 = AM.restate_local(P, x, mask, r["q_mu"], r["q_sigma"], noise, T, objective, lr=0.05, dtype=np.float32)
    RB.local_compare(r, e64, e32)
    lw = r["log_w"].astype(np.float64)
    np.testing.assert_allclose(r["elbo"], lw.mean(axis=0), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r["iwae"], R.log_mean_exp(lw), rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------- 3., 4. a mask of ones; NaN at the unobserved pixels
@pytest.mark.parametrize("nh,nl,xd", [(64, 8, 48), (200, 100, 784)])
def test_a_mask_of_ones_is_the_unmasked_call(gpu, nh, nl, xd):
    m, x, P = _net(nh, nl, xd)
    N, S, T = 5, 13, 6
    kw = dict(n_samples=S, n_iters=T, n_eval=2, objective="iwae", lr=0.05, trace=True)
    ones = np.ones((N, xd), np.uint8)
    rng = np.random.default_rng(3)
    start = (0.1 * rng.standard_normal((N, nl)).astype(np.float32), np.exp(0.1 * rng.standard_normal((N, nl))).astype(np.float32))
    for extra in (dict(), dict(noise=RB.local_noise(N, S, T, nl)), dict(start=start, objective="elbo")):
        kk = dict(kw, **extra)
        m.set_step(3, 20)
        a = m.local_posterior(x, **kk)
        m.set_step(3, 20)
        _same(a, m.local_posterior(x, mask=ones, **kk))
        m.set_step(3, 20)
        _same(a, m.local_posterior(x, mask=None, **kk))           # mask == NULL hands on to the unmasked call
    assert not np.array_equal(a["mu"], a["q_mu"])


@pytest.mark.parametrize("nh,nl,xd,mname", [(64, 8, 48, "sparse05"), (37, 5, 53, "last_only"), (200, 100, 784, "stripes64"), (200, 100, 784, "empty_full")])
def test_nan_at_unobserved_pixels_reaches_no_output(gpu, nh, nl, xd, mname):
    m, x, P = _net(nh, nl, xd)
    N, S, T = 5, 13, 5
    mask = AM.mask_of(mname, N, xd)
    xn = np.where(mask != 0, x, np.float32(np.nan)).astype(np.float32)
    xg = np.where(mask != 0, x, np.float32(-3e38)).astype(np.float32)
    kw = dict(mask=mask, n_samples=S, n_iters=T, n_eval=2, objective="iwae", lr=0.05, trace=True)
    runs = []
    for xx in (x, xn, xg):
        m.set_step(3, 20)
        runs.append(m.local_posterior(xx, **kw))
    for other in runs[1:]:
        _same(runs[0], other)
    assert all(np.all(np.isfinite(runs[0][key])) for key in KEYS)


# ---------------------------------------------------------------- 5. anchor
def test_no_iterations_is_imputes_bound(gpu):
    m, x, P = _net(64, 8, 48)
    N, S = 3, 7
    x = x[:N]
    for mname in ("dense95", "sparse05", "empty_full"):
        mask = AM.mask_of(mname, N, 48)
        m.set_step(5, 11)
        r = m.local_posterior(x, mask=mask, n_samples=S, n_iters=0, n_eval=1, trace=True)
        assert r["bound"].shape == (0, N) and "grad" not in r
        m.set_step(5, 11)
        imp = m.impute(x, mask=mask, n_samples=S, outputs=("log_px", "q_mu", "q_sigma"))
        print(mname, "iwae", r["iwae"], "impute", imp["log_px"])
        assert np.max(np.abs(r["iwae"] - imp["log_px"])) <= 1e-4
        assert np.array_equal(r["q_mu"], imp["q_mu"]) and np.array_equal(r["q_sigma"], imp["q_sigma"])
        assert np.array_equal(r["mu"], r["q_mu"])


# ---------------------------------------------------------------- 6. nothing observed
@pytest.mark.parametrize("nh,nl,xd", AM.SHAPES)
def test_nothing_observed(gpu, nh, nl, xd):
    """The start is the heads of the zero image; the objective is -KL(q || N(0, I)) plus noise, so mu moves towards 0 and sigma towards 1."""
    m, x, P = _net(nh, nl, xd)
    N, S, T, E = 3, 64, 6, 2
    x = x[:N]
    mask = np.zeros((N, xd), np.uint8)
    noise = RB.local_noise(N, S, T, nl, E)
    zero = m.local_posterior(np.zeros((N, xd), np.float32), n_samples=1, n_iters=0, n_eval=1)
    rng = np.random.default_rng(5)
    start = ((1.0 + 0.2 * rng.random((N, nl))).astype(np.float32) * np.where(rng.random((N, nl)) < 0.5, -1, 1).astype(np.float32),
             np.where(rng.random((N, nl)) < 0.5, 0.5, 2.0).astype(np.float32))
    for st in (None, start):
        r = m.local_posterior(x, mask=mask, n_samples=S, n_iters=T, n_eval=E, objective="elbo", lr=0.05, noise=noise, start=st, trace=True)
        if st is None:
            assert np.array_equal(r["q_mu"], zero["q_mu"]) and np.array_equal(r["q_sigma"], zero["q_sigma"])
        e64 = AM.restate_local(P, x, mask, r["q_mu"], r["q_sigma"], noise, T, "elbo", lr=0.05, dtype=np.float64)
        e32 = AM.restate_local(P, x, mask, r["q_mu"], r["q_sigma"], noise, T, "elbo", lr=0.05, dtype=np.float32)
        RB.local_compare(r, e64, e32)
    # from a start well off N(0, I) (|mu| >= 1, sigma 0.5 or 2; S = 64 keeps the draws' noise a quarter of either gradient) every coordinate moves the right way: Adam's first steps are lr sign(grad)
    assert np.all(np.abs(r["mu"]) < np.abs(r["q_mu"])) and np.all(np.abs(np.log(r["sigma"])) < np.abs(np.log(r["q_sigma"])))


# ---------------------------------------------------------------- 7. determinism, bitwise
@pytest.mark.parametrize("nh,nl,xd", [(64, 8, 48), (200, 100, 784)])
def test_chunking_position_masks_and_repeat_are_bitwise(gpu, nh, nl, xd):
    m, x, P = _net(nh, nl, xd)
    N, S, T = 5, 13, 6
    mask = AM.mask_of("dense95" if xd == 48 else "stripes64", N, xd)
    mask[3] = AM.mask_of("sparse05", N, xd)[3]
    kw = dict(n_samples=S, n_iters=T, n_eval=2, objective="iwae", lr=0.05, trace=True)
    runs = []
    for chunk in (0, 1, 3, 0):
        m.set_option("local_t_chunk", chunk)
        m.set_step(3, 20)
        runs.append(m.local_posterior(x, mask=mask, **kw))
    m.set_option("local_t_chunk", 0)
    for other in runs[1:]:
        _same(runs[0], other)
    assert not np.array_equal(runs[0]["mu"], runs[0]["q_mu"])

    def image(r, n):
        return [r[k][n] for k in ("mu", "sigma", "q_mu", "q_sigma", "grad", "elbo", "iwae")] + [r[k][:, n] for k in ("bound", "log_w")]

    m.set_step(3, 22)
    one = m.local_posterior(x[2:3], mask=mask[2:3], **kw)
    for a, b in zip(image(one, 0), image(runs[0], 2)):
        assert np.array_equal(a, b)
    other = mask.copy()
    other[0] = 1 - other[0]
    m.set_step(3, 20)
    r2 = m.local_posterior(x, mask=other, **kw)
    for n in range(1, N):
        for a, b in zip(image(r2, n), image(runs[0], n)):
            assert np.array_equal(a, b), n
    assert not np.array_equal(r2["mu"][0], runs[0]["mu"][0])


# ---------------------------------------------------------------- 8. the device's own noise
@pytest.mark.parametrize("objective", LQ.OBJECTIVES)
def test_device_noise_and_step_advance(gpu, objective):
    m, x, P = _net(64, 8, 48)
    N, S, T, E = 3, 7, 3, 2
    x = x[:N]
    mask = AM.mask_of("empty_full", N, 48)
    draws = []
    for step in range(9, 9 + T + E):
        m.set_step(step, 4)
        draws.append(m.debug_eps(N, S, 0))
    kw = dict(mask=mask, n_samples=S, n_iters=T, n_eval=E, objective=objective, lr=0.05, trace=True)
    m.set_step(9, 4)
    r = m.local_posterior(x, **kw)
    after = m.debug_eps(N, S, 0)
    m.set_step(9 + T + E, 4)
    assert np.array_equal(after, m.debug_eps(N, S, 0))             # the step advanced by T + E
    m.set_step(9 + T + E - 1, 4)
    assert not np.array_equal(after, m.debug_eps(N, S, 0))
    # the same draws as the caller's noise: the same bits, and the step is left alone
    m.set_step(9, 4)
    rn = m.local_posterior(x, noise=np.stack(draws), **kw)
    assert np.array_equal(m.debug_eps(N, S, 0), draws[0])
    _same(r, rn)


# ---------------------------------------------------------------- 10. errors
def _raw(m, x, mask, N, null=(), **fields):
    from iwae_amd import _capi
    o = _capi.LocalOptions()
    o.S, o.T, o.E, o.objective, o.lr, o.beta_1, o.beta_2, o.epsilon = 2, 1, 1, 0, 0.05, 0.9, 0.999, 1e-4
    for k, v in fields.items():
        setattr(o, k, v)
    elbo = np.zeros(max(N, 1), dtype=np.float64)
    outs = _capi.LocalOutputs()
    outs.elbo = None if "elbo" in null else elbo.ctypes.data
    return m.lib.iwae_local_posterior_masked(m.h, None if "x" in null else x.ctypes.data, None if mask is None else mask.ctypes.data, N, None if "opt" in null else C.byref(o),
                                             None if "out" in null else C.byref(outs)), elbo


def test_rejected_arguments_leave_the_step_alone(gpu):
    from iwae_amd.native import NativeModel
    m, x, P = _net(64, 8, 48)
    x = np.ascontiguousarray(x[:2])
    mask = AM.mask_of("dense95", 2, 48)
    m.set_step(17, 3)
    want = m.debug_eps(2, 2, 0)
    ok = dict(mask=mask, n_samples=2, n_iters=1, n_eval=1)
    bad = [dict(ok, n_samples=0), dict(ok, n_samples=65), dict(ok, n_samples=-1), dict(ok, n_iters=-1), dict(ok, n_eval=0), dict(ok, lr=-0.1),
           dict(ok, lr=np.nan), dict(ok, beta_1=1.0), dict(ok, beta_1=-0.1), dict(ok, beta_2=1.0), dict(ok, beta_2=-0.1), dict(ok, epsilon=0.0),
           dict(ok, epsilon=-1e-4), dict(ok, objective="dreg")]
    for kw in bad:
        with pytest.raises(ValueError):
            m.local_posterior(x, **kw)
    with pytest.raises(ValueError):
        m.local_posterior(x[:0], **dict(ok, mask=mask[:0]))
    with pytest.raises(ValueError):
        m.local_posterior(x, **dict(ok, mask=mask[:1]))            # (the binding: a mask of another shape)
    buf = np.ones(64, dtype=np.float32)
    for fields in (dict(mu0=buf.ctypes.data), dict(sigma0=buf.ctypes.data), dict(struct_size=56), dict(objective=2), dict(S=65), dict(E=0), dict(T=-1)):
        assert _raw(m, x, mask, 2, **fields)[0] == -1, fields
    for null in ("x", "opt", "out", "elbo"):
        assert _raw(m, x, mask, 2, null=(null,))[0] == -1, null
    assert _raw(m, x, mask, -1)[0] == -1 and _raw(m, x, mask, 0)[0] == -1
    assert _raw(m, x, mask, (1 << 21) + 1, S=64)[0] == -1          # N S > 2^27: rejected before x or the mask is read
    assert _raw(m, x, mask, 2, T=(1 << 24) + 1)[0] == -1 and _raw(m, x, mask, 2, E=(1 << 24) + 1)[0] == -1
    assert np.array_equal(m.debug_eps(2, 2, 0), want)             # none of them moved the noise step
    assert _raw(m, x, mask, 2)[0] == 0                             # the same call without a defect runs, and advances it by T + E
    m.set_step(17 + 2, 3)
    after = m.debug_eps(2, 2, 0)
    m.set_step(17, 3)
    rc, elbo = _raw(m, x, mask, 2)
    assert rc == 0 and np.array_equal(m.debug_eps(2, 2, 0), after)
    m.set_step(17, 3)
    assert np.array_equal(elbo, m.local_posterior(x, **ok)["elbo"])
    # mask == NULL through the C ABI is the unmasked call, and its refusals are the unmasked call's
    m.set_step(17, 3)
    rc, elbo0 = _raw(m, x, None, 2)
    m.set_step(17, 3)
    assert rc == 0 and np.array_equal(elbo0, m.local_posterior(x, **dict(ok, mask=None))["elbo"]) and not np.array_equal(elbo0, elbo)
    assert _raw(m, x, None, 2, S=65)[0] == -1 and _raw(m, x, None, 0)[0] == -1
    for make in (lambda: NativeModel(2, [16, 8], [4, 2], x_dim=48, seed=1), lambda: NativeModel(1, 16, 4, x_dim=48, seed=1, cond_dim=10),
                 lambda: NativeModel(1, 16, 4, x_dim=48, seed=1, cond_dim=10, cond_prior=True), lambda: NativeModel(1, 224, 4, x_dim=48, seed=1)):
        other = make()
        other.set_step(17, 3)
        before = other.debug_eps(2, 2, 0)
        with pytest.raises(ValueError):
            other.local_posterior(x, **ok)
        assert np.array_equal(other.debug_eps(2, 2, 0), before)
        other.close()
    edge = NativeModel(1, 208, 128, x_dim=48, seed=1)               # the limits themselves run
    assert np.all(np.isfinite(edge.local_posterior(x, **ok)["elbo"]))
    edge.close()


def test_shim(gpu):
    from iwae_amd import iwae1
    m, x, P = _net(64, 8, 48)
    model = iwae1.IWAE(64, 8, x_dim=48, seed=123)
    model._net.set_params(O.flatten_params(P))
    model._net.set_eval_precision("fp32")
    mask = AM.mask_of("sparse05", 3, 48)
    model._net.set_step(2, 0)
    a = model.local_posterior(x[:3], mask=mask, n_samples=4, n_iters=3, n_eval=1)
    m.set_step(2, 0)
    _same(a, m.local_posterior(x[:3], mask=mask, n_samples=4, n_iters=3, n_eval=1), keys=("mu", "sigma", "elbo", "iwae", "q_mu", "q_sigma", "log_w"))
    model._net.close()
