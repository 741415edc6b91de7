"""iwae_ais (include/iwae_amd.h): annealed importance sampling log p(x) with HMC chains on the device (Neal 2001; Wu et al. 2017).

The expected values are the float64 restatement of tests/_ais_ref.py on the DEVICE'S OWN q_mu, q_sigma and the noise passed in, so the chain
kernel is pinned independently of the encoder's precision.  Tolerances are set at run time: 8 x the largest deviation of a float32 numpy run
of the same restatement from its float64 run on the same inputs, floor 1e-5 -- the margin covers the device's other summation order and its
hardware exp / log.  An accept decision whose float64 margin |log u + dH| is smaller than the arithmetic can resolve may legitimately fall
either way; what depends on it is compared only where the margin is resolved (single transitions: 1e-4; trajectories: see there).
"""
import ctypes as C

import numpy as np
import pytest

from oracle import iwae_np as O
import make_golden as MG
import _ais_ref as R
import _row_eval_bodies as RB

pytestmark = pytest.mark.gpu

SHAPES = [(64, 8, 48), (200, 100, 784), (37, 5, 53)]
NMAX = 5
_cache = {}


def _net(nh, nl, xd):
    """One handle per shape for the whole module (seed-fixed parameters, NMAX images)."""
    key = (nh, nl, xd)
    if key not in _cache:
        from iwae_amd.native import NativeModel
        x, P, _ = MG.inputs(1, nh, nl, xd, NMAX, 1, 7 + nh)
        m = NativeModel(1, nh, nl, x_dim=xd, seed=123)
        m.set_params(O.flatten_params(P))
        m.set_eval_precision("fp32")
        _cache[key] = (m, x, P)
    return _cache[key]


_tol = RB._tol


# ---------------------------------------------------------------- 1. one transition
@pytest.mark.parametrize("init", ["encoder", "prior"])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("N,Cn", [(1, 1), (1, 17), (3, 7), (5, 13)], ids=["row", "tile", "mixed", "workgroup"])
@pytest.mark.parametrize("nh,nl,xd", SHAPES)
def test_single_transition_parity(gpu, nh, nl, xd, N, Cn, L, init):
    m, x, P = _net(nh, nl, xd)
    RB.ais_single_transition(m, x, P, nl, N, Cn, L, init)


# ---------------------------------------------------------------- 2. trajectories
def _first(mask):
    """Per chain: index of the first True along axis 0, or T."""
    T = mask.shape[0]
    return np.where(mask.any(axis=0), mask.argmax(axis=0), T)


# (noise seeds for which the float64 restatement alone cuts under 5 % of the chains short; at h = 0.9 about one seed in ten does: the
# float32 deviation is the maximum over 864 chaotic leapfrog trajectories)
@pytest.mark.parametrize("nh,nl,xd,N,Cn,T,L,h,adapt,seed", [(64, 8, 48, 3, 24, 12, 4, 0.4, False, 216), (64, 8, 48, 3, 24, 12, 4, 0.9, False, 321),
                                                             (200, 100, 784, 2, 20, 6, 3, 0.3, False, 209), (64, 8, 48, 3, 24, 12, 4, 0.4, True, 301)],
                         ids=["h0.4", "h0.9", "full", "adapt"])
def test_trajectories(gpu, nh, nl, xd, N, Cn, T, L, h, adapt, seed):
    """A chain is compared with the float64 restatement up to its first decision whose float64 margin |log u + dH| is below delta = 64 x the
    float32-vs-float64 dH deviation measured here (floor 1e-4): beyond it the two may legitimately be different chains.  Deviations of dH
    are taken relative to max(1, |dH|): at h = 0.9 some leapfrog trajectories are unstable and end with dH in the hundreds (rejected by
    any arithmetic), where float32 resolves ~1e-5 of the value, not of 1."""
    m, x, P = _net(nh, nl, xd)
    x = x[:N]
    betas = np.linspace(0.0, 1.0, T + 1).astype(np.float32)
    eps0, mom, unif = R.noise(seed, T, Cn, N, nl)
    r = m.ais(x, n_chains=Cn, leapfrog=L, step_size=h, adapt=adapt, init="encoder", betas=betas, noise=(eps0, mom, unif), trace=True)
    mu, sg = r["q_mu"], r["q_sigma"]
    e64 = R.restate(P, x, mu, sg, betas, L, h, eps0, mom, unif, np.float64, adapt=adapt)
    e32 = R.restate(P, x, mu, sg, betas, L, h, eps0, mom, unif, np.float32, adapt=adapt)
    tt = np.arange(T)[:, None, None]
    # float32 vs float64 restatement while both are the same chain (up to and including their first differing decision)
    same = tt <= _first(e32["accepted"] != e64["accepted"])[None]
    scale = np.maximum(1.0, np.abs(e64["dH"]))
    dev_dH = float(np.max((np.abs(e32["dH"].astype(np.float64) - e64["dH"]) / scale)[same]))
    delta = max(64.0 * dev_dH, 1e-4)
    cut = _first(np.abs(e64["margin"]) < delta * scale)           # [C, N]
    frac = float(np.mean(cut < T))
    print("accept rate %.3f, float32 dH deviation %.3g, delta %.3g, chains cut short %.3f" % (r["accepted"].mean(), dev_dH, delta, frac))
    assert frac <= 0.10
    # the device's decisions follow its own dH
    logu = np.log(unif.astype(np.float64))
    clear = np.abs(logu + r["dH"]) > 1e-5
    assert np.array_equal(r["accepted"][clear] != 0, (logu < -r["dH"].astype(np.float64))[clear])
    np.testing.assert_allclose(r["accept_rate"], r["accepted"].reshape(T, -1).mean(axis=1), rtol=1e-6)
    if h == 0.9:
        assert 0.05 < 1.0 - r["accepted"].mean() < 0.95         # both branches of the accept step run
    tol = max(8.0 * dev_dH, 1e-5)
    upto = tt <= cut[None]
    err = float(np.max((np.abs(r["dH"].astype(np.float64) - e64["dH"]) / scale)[upto]))
    print("dH: device error %.3g, tolerance %.3g" % (err, tol))
    assert err <= tol
    before = tt < cut[None]
    assert np.array_equal(r["accepted"][before], e64["accepted"][before])
    whole = (cut == T) & (_first(e32["accepted"] != e64["accepted"]) == T)
    assert whole.any()
    for key in ("log_w", "z") + (("step_size",) if adapt else ()):
        k64 = "step" if key == "step_size" else key
        dev, w64, w32 = (np.asarray(a, dtype=np.float64)[whole] for a in (r[key], e64[k64], e32[k64]))
        tol = _tol(w32, w64)
        err = float(np.max(np.abs(dev - w64)))
        print("%s: device error %.3g, tolerance %.3g" % (key, err, tol))
        assert err <= tol, (key, err, tol)
    if adapt:
        assert len(np.unique(r["step_size"])) > 1 and np.all(r["step_size"] != np.float32(h))


# ---------------------------------------------------------------- 3. anchors
def test_one_temperature_is_eval_llh(gpu):
    m, x, P = _net(64, 8, 48)
    N, Cn = 3, 7
    x = x[:N]
    m.set_step(5, 11)
    r = m.ais(x, n_chains=Cn, leapfrog=1, step_size=0.1, adapt=False, betas=[0.0, 1.0])
    m.set_step(5, 11)
    _, per = m.eval_llh(x, k=Cn, per_image=True)
    print("ais", r["log_px"], "eval_llh", per)
    assert np.max(np.abs(r["log_px"] - per.astype(np.float64))) <= 1e-4
    # a vanishing step size: the chains stay where they start and any schedule telescopes to the same weight
    m.set_step(5, 11)
    b7 = np.array([0.0, 0.05, 0.1, 0.4, 0.45, 0.9, 1.0], dtype=np.float32)
    r7 = m.ais(x, n_chains=Cn, leapfrog=2, step_size=1e-30, adapt=False, betas=b7)
    np.testing.assert_allclose(r7["log_w"], r["log_w"], rtol=2e-6, atol=1e-9)


def test_device_noise_and_step_advance(gpu):
    m, x, P = _net(64, 8, 48)
    N, Cn, T = 3, 7, 6
    x = x[:N]
    m.set_step(9, 4)
    want = m.debug_eps(N, Cn, 0)
    r = m.ais(x, n_chains=Cn, leapfrog=1, step_size=1e-30, adapt=False, init="prior", betas=np.linspace(0, 1, T + 1))
    assert np.array_equal(r["z"], want)                           # prior init: z = e, and the chains never move
    after = m.debug_eps(N, Cn, 0)
    m.set_step(9 + T + 1, 4)
    assert np.array_equal(after, m.debug_eps(N, Cn, 0))
    m.set_step(9 + T, 4)
    assert not np.array_equal(after, m.debug_eps(N, Cn, 0))
    # the caller's noise leaves the step alone; z0 without noise still advances it
    m.set_step(9, 4)
    eps0, mom, unif = R.noise(3, T, Cn, N, 8)
    m.ais(x, n_chains=Cn, leapfrog=1, step_size=0.1, betas=np.linspace(0, 1, T + 1), noise=(eps0, mom, unif))
    assert np.array_equal(m.debug_eps(N, Cn, 0), want)
    rz = m.ais(x, n_chains=Cn, leapfrog=1, step_size=1e-30, adapt=False, betas=np.linspace(0, 1, T + 1), z0=eps0)
    np.testing.assert_allclose(rz["z"], eps0, rtol=1e-5, atol=1e-6)      # (z0 -> e -> z: two float32 roundings)
    assert np.array_equal(m.debug_eps(N, Cn, 0), after)


# ---------------------------------------------------------------- 4. invariances, bitwise
@pytest.mark.parametrize("nh,nl,xd", [(64, 8, 48), (200, 100, 784)])
def test_chunking_position_and_repeat_are_bitwise(gpu, nh, nl, xd):
    m, x, P = _net(nh, nl, xd)
    RB.ais_chunking_position_and_repeat_are_bitwise(m, x)


# ---------------------------------------------------------------- 5. ground truth on the device
def test_against_quadrature_and_bdmc(gpu):
    from iwae_amd import iwae1, utils
    nh, nl, xd, N, Cn, T = 64, 2, 48, 4, 64, 200
    x, P, _ = MG.inputs(1, nh, nl, xd, N, 1, 41)
    model = iwae1.IWAE(nh, nl, x_dim=xd, seed=123)
    m = model._net
    m.set_params(O.flatten_params(P))
    m.set_eval_precision("fp32")
    zg, lw = utils.latent_grid([(-8.0, 8.0)] * 2, 801)
    truth = m.grid_posterior(x, zg, lw)["log_px"]
    m.set_step(1, 0)
    r = m.ais(x, n_chains=Cn, n_temps=T, leapfrog=5, step_size=0.3, adapt=False, init="prior")
    se = R.log_mean_se(r["log_w"])
    print("truth", truth, "ais", r["log_px"], "se", se, "accept", r["accept_rate"].mean(), "ess", r["ess"])
    assert np.all(np.abs(r["log_px"] - truth) <= 4 * se), (r["log_px"] - truth, se)
    one = m.ais(x, n_chains=Cn, leapfrog=5, step_size=0.3, adapt=False, init="prior", betas=[0.0, 1.0])
    print("T = 1", one["log_px"])
    assert np.mean(np.abs(r["log_px"] - truth)) < np.mean(np.abs(one["log_px"] - truth))
    b = model.bdmc(4, n_chains=Cn, n_temps=T, seed=5, leapfrog=5, step_size=0.3, adapt=False, init="prior")
    truth_b = m.grid_posterior(b["x"], zg, lw)["log_px"]
    se_l, se_u = R.log_mean_se(b["forward"]["log_w"]), R.log_mean_se(b["reverse"]["log_w"])
    print("bdmc truth", truth_b, "lower", b["lower"], se_l, "upper", b["upper"], se_u, "gap", b["gap"])
    assert np.all(np.abs(b["lower"] - truth_b) <= 4 * se_l) and np.all(np.abs(b["upper"] - truth_b) <= 4 * se_u)
    assert np.all(b["lower"] - 4 * se_l <= truth_b) and np.all(truth_b <= b["upper"] + 4 * se_u)
    assert abs(b["gap"] - float(np.mean(b["upper"] - b["lower"]))) < 1e-12
    model._net.close()


# ---------------------------------------------------------------- 6. errors
def _raw(m, x, N, **fields):
    from iwae_amd import _capi
    betas = np.array([0.0, 1.0], dtype=np.float32)
    o = _capi.AisOptions()
    o.C, o.T, o.L, o.betas, o.step_size = 2, 1, 1, betas.ctypes.data, 0.1
    for k, v in fields.items():
        setattr(o, k, v)
    lpx = np.zeros(max(N, 1), dtype=np.float64)
    outs = _capi.AisOutputs()
    outs.log_px = lpx.ctypes.data
    return m.lib.iwae_ais(m.h, x.ctypes.data, N, C.byref(o), C.byref(outs)), betas


def test_rejected_arguments_leave_the_step_alone(gpu):
    from iwae_amd.native import NativeModel
    m, x, P = _net(64, 8, 48)
    x = np.ascontiguousarray(x[:2])
    m.set_step(17, 3)
    want = m.debug_eps(2, 2, 0)
    ok = dict(n_chains=2, leapfrog=1, step_size=0.1, betas=[0.0, 1.0])
    bad = [dict(ok, n_chains=0), dict(ok, n_chains=-3), dict(ok, leapfrog=0), dict(ok, betas=[0.5]), dict(ok, betas=[0.0, 1.5]),
           dict(ok, betas=[-0.1, 1.0]), dict(ok, betas=[0.0, np.nan]), dict(ok, step_size=0.0), dict(ok, step_size=-0.1)]
    for kw in bad:
        with pytest.raises(ValueError):
            m.ais(x, **kw)
    with pytest.raises(ValueError):
        m.ais(x[:0], **ok)
    buf = np.ones(64, dtype=np.float32)
    for fields in (dict(eps0=buf.ctypes.data), dict(mom=buf.ctypes.data, unif=buf.ctypes.data), dict(struct_size=64), dict(init=2),
                   dict(C=(1 << 26) + 1), dict(betas=None)):
        rc, _ = _raw(m, x, 2, **fields)
        assert rc == -1, fields
    assert np.array_equal(m.debug_eps(2, 2, 0), want)             # none of them moved the noise step
    assert _raw(m, x, 2)[0] == 0                                   # the same call without a defect runs, and advances it by T + 1
    m.set_step(17 + 2, 3)
    after = m.debug_eps(2, 2, 0)
    m.set_step(17, 3)
    assert _raw(m, x, 2)[0] == 0
    assert np.array_equal(m.debug_eps(2, 2, 0), after)
    two = NativeModel(2, [16, 8], [4, 2], x_dim=48, seed=1)
    with pytest.raises(ValueError):
        two.ais(x, **ok)
    two.close()
    cond = NativeModel(1, 16, 4, x_dim=48, seed=1, cond_dim=10)
    with pytest.raises(ValueError):
        cond.ais(x, **ok)
    cond.close()
    wide = NativeModel(1, 256, 4, x_dim=48, seed=1)
    with pytest.raises(ValueError):
        wide.ais(x, **ok)
    wide.close()


def test_shims(gpu):
    from iwae_amd import iwae2
    two = iwae2.IWAE([16, 8], [4, 2], x_dim=48)
    with pytest.raises(NotImplementedError):
        two.ais_log_likelihood(np.zeros((1, 48), np.float32))
    with pytest.raises(NotImplementedError):
        two.bdmc(2)
