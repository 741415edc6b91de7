"""iwae_local_posterior (include/iwae_amd.h): per-image optimisation of a factorised Gaussian q against the decoder on the device, and the
inference-gap split built on it (Cremer, Li & Duvenaud 2018).

The expected values are the float64 restatement of tests/_local_q_ref.py on the DEVICE'S OWN q_mu, q_sigma and the noise passed in, so the
kernel is pinned independently of the encoder's precision.  Tolerances follow tests/test_gpu_ais.py's rule, set at run time: 8 x the largest
deviation of a float32 numpy run of the same restatement from its float64 run on the same inputs, floor 1e-5 -- the margin covers the
device's other summation order and its hardware exp / log.  Every test runs in the float32 eval precision.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import iwae_np as O
import make_golden as MG
import _ais_ref as R
import _local_q_ref as LQ
import _row_eval_bodies as RB

pytestmark = pytest.mark.gpu

SHAPES = [(64, 8, 48), (200, 100, 784), (37, 5, 53)]
NMAX = 5
_cache = {}


def _net(nh, nl, xd, precision="bf16"):
    """One handle per shape (and training precision) for the whole module (seed-fixed parameters, NMAX images)."""
    key = (nh, nl, xd, precision)
    if key not in _cache:
        from iwae_amd.native import NativeModel
        x, P, _ = MG.inputs(1, nh, nl, xd, NMAX, 1, 7 + nh)
        m = NativeModel(1, nh, nl, x_dim=xd, seed=123, precision=precision)
        m.set_params(O.flatten_params(P))
        m.set_eval_precision("fp32")
        _cache[key] = (m, x, P)
    return _cache[key]


_tol = RB._tol


KEYS = RB.LOCAL_KEYS
_compare = RB.local_compare


# ---------------------------------------------------------------- 1. per-iteration parity
@pytest.mark.parametrize("objective", LQ.OBJECTIVES)
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("N,S", [(1, 1), (1, 17), (3, 7), (5, 13), (2, 64)], ids=["row", "dead", "straddle", "two_wg", "one_image"])
@pytest.mark.parametrize("nh,nl,xd", SHAPES)
def test_iteration_parity(gpu, nh, nl, xd, N, S, T, objective):
    m, x, P = _net(nh, nl, xd)
    RB.local_iteration_parity(m, x, P, nl, N, S, T, objective)


@pytest.mark.parametrize("objective", LQ.OBJECTIVES)
def test_iteration_parity_from_the_callers_start(gpu, objective):
    m, x, P = _net(64, 8, 48)
    N, S, T, E = 3, 7, 3, 2
    x = x[:N]
    rng = np.random.default_rng(77)
    mu0 = (0.3 * rng.standard_normal((N, 8))).astype(np.float32)
    sg0 = np.exp(0.3 * rng.standard_normal((N, 8)) - 0.5).astype(np.float32)
    noise = rng.standard_normal((T + E, S, N, 8)).astype(np.float32)
    kw = dict(beta_1=0.8, beta_2=0.99, epsilon=1e-3)
    r = m.local_posterior(x, n_samples=S, n_iters=T, n_eval=E, objective=objective, lr=0.02, start=(mu0, sg0), noise=noise, trace=True, **kw)
    assert np.array_equal(r["q_mu"], mu0) and np.array_equal(r["q_sigma"], sg0)
    e64 = LQ.restate(P, x, mu0, sg0, noise, T, objective, lr=0.02, dtype=np.float64, **kw)
    e32 = LQ.restate(P, x, mu0, sg0, noise, T, objective, lr=0.02, dtype=np.float32, **kw)
    _compare(r, e64, e32)


# ---------------------------------------------------------------- 2. invariances, bitwise
@pytest.mark.parametrize("nh,nl,xd", [(64, 8, 48), (200, 100, 784)])
def test_chunking_position_and_repeat_are_bitwise(gpu, nh, nl, xd):
    m, x, P = _net(nh, nl, xd)
    RB.local_chunking_position_and_repeat_are_bitwise(m, x)


# ---------------------------------------------------------------- 3. anchors
def test_no_iterations_is_the_evaluator(gpu):
    m, x, P = _net(64, 8, 48, precision="fp32")
    N, S = 3, 7
    x = x[:N]
    m.set_step(5, 11)
    r = m.local_posterior(x, n_samples=S, n_iters=0, n_eval=1, trace=True)
    assert r["bound"].shape == (0, N) and "grad" not in r
    m.set_step(5, 11)
    _, per = m.eval_llh(x, k=S, per_image=True)
    print("iwae", r["iwae"], "eval_llh", per)
    assert np.max(np.abs(r["iwae"] - per.astype(np.float64))) <= 1e-4
    m.set_step(5, 11)
    eps = m.debug_eps(N, S, 0)
    f = m.forward(x, S, eps=eps, want=("log_w",))
    print("elbo", r["elbo"], "forward", f["log_w"].astype(np.float64).mean(axis=0))
    assert np.max(np.abs(r["elbo"] - f["log_w"].astype(np.float64).mean(axis=0))) <= 1e-4       # (float32 log-weights of ~35 nat, two kernels)
    assert np.array_equal(r["mu"], r["q_mu"])
    np.testing.assert_allclose(r["sigma"], r["q_sigma"], rtol=1e-6)                              # (through exp(log sigma))


@pytest.mark.parametrize("objective", LQ.OBJECTIVES)
def test_device_noise_and_step_advance(gpu, objective):
    m, x, P = _net(64, 8, 48)
    N, S, T, E = 3, 7, 2, 1
    x = x[:N]
    draws = []
    for step in (9, 10, 11):
        m.set_step(step, 4)
        draws.append(m.debug_eps(N, S, 0))
    m.set_step(9, 4)
    r = m.local_posterior(x, n_samples=S, n_iters=T, n_eval=E, objective=objective, lr=0.0, trace=True)
    after = m.debug_eps(N, S, 0)
    assert np.array_equal(r["mu"], r["q_mu"])                     # lr = 0: nothing moves, so iteration t sees the start on the draws of step 9 + t
    dec64, dec32 = R.decoder_of(P, np.float64), R.decoder_of(P, np.float32)
    for t in range(T):
        b64 = LQ.bound_and_grad(dec64, x.astype(np.float64), r["q_mu"].astype(np.float64), np.log(r["q_sigma"].astype(np.float64)), draws[t].astype(np.float64), objective)[0]
        b32 = LQ.bound_and_grad(dec32, x, r["q_mu"], np.log(r["q_sigma"]), draws[t], objective)[0]
        tol = _tol(b32, b64)
        err = float(np.max(np.abs(r["bound"][t] - b64)))
        print("bound[%d]: device error %.3g, tolerance %.3g" % (t, err, tol))
        assert err <= tol
    lw64 = LQ.log_weights(dec64, x.astype(np.float64), r["q_mu"].astype(np.float64), np.log(r["q_sigma"].astype(np.float64)), draws[2].astype(np.float64))[0]
    lw32 = LQ.log_weights(dec32, x, r["q_mu"], np.log(r["q_sigma"]), draws[2])[0]
    assert np.max(np.abs(r["log_w"] - lw64)) <= _tol(lw32, lw64)
    # the step advanced by T + E
    m.set_step(9 + T + E, 4)
    assert np.array_equal(after, m.debug_eps(N, S, 0))
    m.set_step(9 + T + E - 1, 4)
    assert not np.array_equal(after, m.debug_eps(N, S, 0))
    # the caller's noise leaves it alone
    m.set_step(9, 4)
    m.local_posterior(x, n_samples=S, n_iters=T, n_eval=E, objective=objective, noise=np.stack(draws))
    assert np.array_equal(m.debug_eps(N, S, 0), draws[0])


# ---------------------------------------------------------------- 4. ground truth on the device
def test_against_quadrature(gpu):
    from iwae_amd import iwae1, utils
    nh, nl, xd, N, S, T, E = 64, 2, 48, 4, 16, 200, 64
    x, P, _ = MG.inputs(1, nh, nl, xd, N, 1, 41)
    model = iwae1.IWAE(nh, nl, x_dim=xd, seed=123)
    m = model._net
    m.set_params(O.flatten_params(P))
    m.set_eval_precision("fp32")
    zg, lw = utils.latent_grid([(-8.0, 8.0)] * 2, 801)
    g = m.grid_posterior(x, zg, lw)
    log_px = g["log_px"]
    noise = np.concatenate([np.random.default_rng(5).standard_normal((T, S, N, nl)), np.random.default_rng(6).standard_normal((E, S, N, nl))]).astype(np.float32)
    r = m.local_posterior(x, n_samples=S, n_iters=T, n_eval=E, objective="elbo", lr=0.05, noise=noise)
    se = LQ.mean_se(r["log_w"])
    after = LQ.exact_elbo(P, x, r["mu"], r["sigma"])
    before = LQ.exact_elbo(P, x, r["q_mu"], r["q_sigma"])
    closed = (after - before) / (log_px - before)
    print("log_px", log_px, "elbo", r["elbo"], "exact", after, "se", se, "encoder gap", log_px - before, "gap left", log_px - after, "closed", closed)
    assert np.all(np.abs(r["elbo"] - after) <= 4 * se), (r["elbo"] - after, se)
    assert np.all(after <= log_px) and np.all(closed >= 0.5)
    # no iterations: log p(x) - ELBO[q_enc] is KL(q_enc || p(z|x))
    a = m.local_posterior(x, n_samples=S, n_iters=0, n_eval=E, noise=noise[T:])
    se_a = LQ.mean_se(a["log_w"])
    print("kl_q_post", g["kl_q_post"], "log_px - elbo", log_px - a["elbo"], "se", se_a)
    assert np.all(np.abs((log_px - a["elbo"]) - g["kl_q_post"]) <= 4 * se_a)
    # the split
    m.set_step(1, 0)
    gaps = model.inference_gaps(x, n_samples=S, n_iters=20, n_eval=4, ais=dict(n_chains=8, n_temps=20, leapfrog=2, step_size=0.3, adapt=False))
    assert np.max(np.abs(gaps["approximation_gap"] + gaps["amortization_gap"] - (gaps["log_px"] - gaps["elbo_amortized"]))) <= 1e-12
    assert np.array_equal(gaps["elbo_local"], gaps["local"]["elbo"]) and np.array_equal(gaps["elbo_amortized"], gaps["amortized"]["elbo"])
    assert gaps["elbo_local_se"].shape == (N,) and np.all(gaps["elbo_local_se"] > 0) and np.all(gaps["log_px_se"] > 0)
    model._net.close()


# ---------------------------------------------------------------- 5. errors
def _raw(m, x, N, null=(), extra_out=None, **fields):
    from iwae_amd import _capi
    o = _capi.LocalOptions()
    o.S, o.T, o.E, o.objective, o.lr, o.beta_1, o.beta_2, o.epsilon = 2, 1, 1, 0, 0.05, 0.9, 0.999, 1e-4
    for k, v in fields.items():
        setattr(o, k, v)
    elbo = np.zeros(max(N, 1), dtype=np.float64)
    outs = _capi.LocalOutputs()
    outs.elbo = None if "elbo" in null else elbo.ctypes.data
    for k, v in (extra_out or {}).items():
        setattr(outs, k, v.ctypes.data)
    return m.lib.iwae_local_posterior(m.h, None if "x" in null else x.ctypes.data, N, None if "opt" in null else C.byref(o),
                                      None if "out" in null else C.byref(outs))


def test_rejected_arguments_leave_the_step_alone(gpu):
    from iwae_amd.native import NativeModel
    m, x, P = _net(64, 8, 48)
    x = np.ascontiguousarray(x[:2])
    m.set_step(17, 3)
    want = m.debug_eps(2, 2, 0)
    ok = dict(n_samples=2, n_iters=1, n_eval=1)
    bad = [dict(ok, n_samples=0), dict(ok, n_samples=65), dict(ok, n_samples=-1), dict(ok, n_iters=-1), dict(ok, n_eval=0), dict(ok, lr=-0.1),
           dict(ok, lr=np.nan), dict(ok, beta_1=1.0), dict(ok, beta_1=-0.1), dict(ok, beta_2=1.0), dict(ok, beta_2=-0.1), dict(ok, epsilon=0.0),
           dict(ok, epsilon=-1e-4), dict(ok, objective="dreg")]
    for kw in bad:
        with pytest.raises(ValueError):
            m.local_posterior(x, **kw)
    with pytest.raises(ValueError):
        m.local_posterior(x[:0], **ok)
    buf = np.ones(64, dtype=np.float32)
    for fields in (dict(mu0=buf.ctypes.data), dict(sigma0=buf.ctypes.data), dict(struct_size=56), dict(objective=2), dict(S=65), dict(E=0), dict(T=-1)):
        assert _raw(m, x, 2, **fields) == -1, fields
    for null in ("x", "opt", "out", "elbo"):
        assert _raw(m, x, 2, null=(null,)) == -1, null
    assert _raw(m, x, -1) == -1 and _raw(m, x, 0) == -1
    assert _raw(m, x, (1 << 21) + 1, S=64) == -1                   # N S > 2^27: rejected before x is read
    assert _raw(m, x, 2, T=(1 << 24) + 1) == -1 and _raw(m, x, 2, E=(1 << 24) + 1) == -1
    assert np.array_equal(m.debug_eps(2, 2, 0), want)             # none of them moved the noise step
    assert _raw(m, x, 2) == 0                                      # the same call without a defect runs, and advances it by T + E
    m.set_step(17 + 2, 3)
    after = m.debug_eps(2, 2, 0)
    m.set_step(17, 3)
    assert _raw(m, x, 2) == 0
    assert np.array_equal(m.debug_eps(2, 2, 0), after)
    for make in (lambda: NativeModel(2, [16, 8], [4, 2], x_dim=48, seed=1), lambda: NativeModel(1, 16, 4, x_dim=48, seed=1, cond_dim=10),
                 lambda: NativeModel(1, 16, 4, x_dim=48, seed=1, cond_dim=10, cond_prior=True), lambda: NativeModel(1, 224, 4, x_dim=48, seed=1)):
        other = make()
        with pytest.raises(ValueError):
            other.local_posterior(x, **ok)
        other.close()
    with pytest.raises(ValueError):                                # (n_latent > 128: iwae_create already refuses the handle)
        NativeModel(1, 16, 130, x_dim=48, seed=1)
    edge = NativeModel(1, 208, 128, x_dim=48, seed=1)               # the limits themselves run
    r = edge.local_posterior(x, **ok)
    assert np.all(np.isfinite(r["elbo"]))
    edge.close()


def test_no_iterations_leaves_grad_and_bound_unwritten(gpu):
    """The raw ABI with every output pointer filled in, as a C wrapper would: T = 0 returns IWAE_OK and writes neither grad nor bound."""
    m, x, P = _net(64, 8, 48)
    x = np.ascontiguousarray(x[:2])
    grad, bound, log_w = np.full((2, 16), 7.0, np.float32), np.full((1, 2), 7.0, np.float32), np.full((2, 2), 7.0, np.float32)
    m.set_step(21, 0)
    assert _raw(m, x, 2, extra_out=dict(grad=grad, bound=bound, log_w=log_w), T=0) == 0
    assert np.all(grad == 7.0) and np.all(bound == 7.0) and np.all(log_w != 7.0)
    after = m.debug_eps(2, 2, 0)
    m.set_step(21 + 1, 0)
    assert np.array_equal(after, m.debug_eps(2, 2, 0))             # the step advanced by E = 1
    assert _raw(m, x, 2, extra_out=dict(grad=grad, bound=bound), T=1) == 0
    assert np.all(grad != 7.0) and np.all(bound != 7.0)


def test_shims(gpu):
    from iwae_amd import iwae2
    two = iwae2.IWAE([16, 8], [4, 2], x_dim=48)
    with pytest.raises(NotImplementedError):
        two.local_posterior(np.zeros((1, 48), np.float32))
    with pytest.raises(NotImplementedError):
        two.inference_gaps(np.zeros((1, 48), np.float32))
