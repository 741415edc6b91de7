"""iwae_ais_masked (include/iwae_amd.h): annealed importance sampling log p(x_obs) of incomplete images, HMC chains on p(z | x_obs).

The expected values are the float64 restatement of tests/_ais_masked_ref.py on the DEVICE'S OWN q_mu, q_sigma and the noise passed in.
Tolerances are tests/test_gpu_ais.py's, set at run time: 8 x the largest deviation of a float32 numpy run of the same restatement from its
float64 run on the same inputs, floor 1e-5; trajectories follow test_gpu_ais.py::test_trajectories.  The masks (tests/_ais_masked_ref.py
SHAPE_MASKS) are the smallest at which the output layer's epilogue can go wrong; the trajectory cases are the ones
tests/test_ais_masked_host.py holds admissible on the CPU."""
import ctypes as C

import numpy as np
import pytest

from oracle import iwae_np as O
import make_golden as MG
import _ais_ref as R
import _row_eval_bodies as RB
import _ais_masked_ref as AM
import _parity_common as PC

pytestmark = pytest.mark.gpu

NMAX = AM.NMAX
_cache = {}
_tol = RB._tol
AIS_KEYS = RB.AIS_KEYS + ("q_mu", "q_sigma")


def _net(nh, nl, xd):
    """One handle per shape for the whole module (test_gpu_ais.py's parameters and images)."""
    key = (nh, nl, xd)
    if key not in _cache:
        from iwae_amd.native import NativeModel
        x, P, _ = MG.inputs(1, nh, nl, xd, NMAX, 1, 7 + nh)
        m = NativeModel(1, nh, nl, x_dim=xd, seed=123)
        m.set_params(O.flatten_params(P))
        m.set_eval_precision("fp32")
        _cache[key] = (m, x, P)
    return _cache[key]


def _same(a, b, keys=AIS_KEYS):
    for key in keys:
        assert np.array_equal(a[key], b[key]), key


# ---------------------------------------------------------------- 1. one transition
@pytest.mark.parametrize("N,Cn", AM.SINGLE_CASES, ids=AM.SINGLE_IDS)
@pytest.mark.parametrize("shape,mname", [(s, n) for s in AM.SHAPES for n in AM.SHAPE_MASKS[s]], ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_single_transition_parity(gpu, shape, mname, N, Cn):
    """RB.ais_single_transition under a mask, both inits, L = 1 and 3."""
    nh, nl, xd = shape
    m, x, P = _net(nh, nl, xd)
    x = x[:N]
    mask = AM.mask_of(mname, N, xd)
    betas, h = AM.SINGLE_BETAS, AM.SINGLE_H
    for init in ("encoder", "prior"):
        for L in (1, 3):
            eps0, mom, unif = R.noise(AM.single_seed(shape, mname, N, Cn, L, init), 1, Cn, N, nl)
            r = m.ais(x, mask=mask, n_chains=Cn, leapfrog=L, step_size=h, adapt=False, init=init, betas=betas, noise=(eps0, mom, unif), trace=True)
            if init == "prior":
                assert np.array_equal(r["q_mu"], np.zeros((N, nl), np.float32)) and np.array_equal(r["q_sigma"], np.ones((N, nl), np.float32))
            mu, sg = r["q_mu"], r["q_sigma"]
            e64 = AM.restate_ais(P, x, mask, mu, sg, betas, L, h, eps0, mom, unif, np.float64)
            e32 = AM.restate_ais(P, x, mask, mu, sg, betas, L, h, eps0, mom, unif, np.float32)
            resolved = np.abs(e64["margin"][0]) > 1e-4
            for key in ("dH", "log_w", "z"):
                dev, w64, w32 = (np.asarray(a[key], dtype=np.float64) for a in (r, e64, e32))
                if key == "z":
                    dev, w64, w32 = dev[resolved], w64[resolved], w32[resolved]
                tol = _tol(w32, w64)
                err = float(np.max(np.abs(dev - w64))) if dev.size else 0.0
                print("%s L%d %s: device error %.3g, tolerance %.3g, ratio %.3f" % (init, L, key, err, tol, err / tol))
                assert err <= tol, (init, L, key, err, tol)
            assert np.array_equal(r["accepted"][0][resolved], e64["accepted"][0][resolved])
            np.testing.assert_allclose(r["log_px"], R.log_mean_exp(r["log_w"]), rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------- 2. trajectories
@pytest.mark.parametrize("name", sorted(AM.TRAJECTORIES))
def test_trajectories(gpu, name):
    """test_gpu_ais.py::test_trajectories under a mask, at the cases test_ais_masked_host.py holds admissible (the 10 % cap is a condition)."""
    nh, nl, xd, N, Cn, T, L, h, adapt, mname, seed = AM.TRAJECTORIES[name]
    m, x, P = _net(nh, nl, xd)
    x = x[:N]
    mask = AM.mask_of(mname, N, xd)
    betas = np.linspace(0.0, 1.0, T + 1).astype(np.float32)
    eps0, mom, unif = R.noise(seed, T, Cn, N, nl)
    r = m.ais(x, mask=mask, n_chains=Cn, leapfrog=L, step_size=h, adapt=adapt, init="encoder", betas=betas, noise=(eps0, mom, unif), trace=True)
    mu, sg = r["q_mu"], r["q_sigma"]
    e64 = AM.restate_ais(P, x, mask, mu, sg, betas, L, h, eps0, mom, unif, np.float64, adapt=adapt)
    e32 = AM.restate_ais(P, x, mask, mu, sg, betas, L, h, eps0, mom, unif, np.float32, adapt=adapt)
    tt = np.arange(T)[:, None, None]
    dev_dH, delta, cut, scale, whole = AM.trajectory_cut(e32, e64)
    frac = float(np.mean(cut < T))
    print("accept rate %.3f, float32 dH deviation %.3g, delta %.3g, chains cut short %.3f" % (r["accepted"].mean(), dev_dH, delta, frac))
    assert frac <= 0.10
    logu = np.log(unif.astype(np.float64))
    clear = np.abs(logu + r["dH"]) > 1e-5
    assert np.array_equal(r["accepted"][clear] != 0, (logu < -r["dH"].astype(np.float64))[clear])
    np.testing.assert_allclose(r["accept_rate"], r["accepted"].reshape(T, -1).mean(axis=1), rtol=1e-6)
    if h == 0.9:
        assert 0.05 < 1.0 - r["accepted"].mean() < 0.95
    tol = max(8.0 * dev_dH, 1e-5)
    upto = tt <= cut[None]
    err = float(np.max((np.abs(r["dH"].astype(np.float64) - e64["dH"]) / scale)[upto]))
    print("dH: device error %.3g, tolerance %.3g, ratio %.3f" % (err, tol, err / tol))
    assert err <= tol
    before = tt < cut[None]
    assert np.array_equal(r["accepted"][before], e64["accepted"][before])
    assert whole.any()
    for key in ("log_w", "z") + (("step_size",) if adapt else ()):
        k64 = "step" if key == "step_size" else key
        dev, w64, w32 = (np.asarray(a, dtype=np.float64)[whole] for a in (r[key], e64[k64], e32[k64]))
        tol = _tol(w32, w64)
        err = float(np.max(np.abs(dev - w64)))
        print("%s: device error %.3g, tolerance %.3g, ratio %.3f" % (key, err, tol, err / tol))
        assert err <= tol, (key, err, tol)
    if adapt:
        assert len(np.unique(r["step_size"])) > 1 and np.all(r["step_size"] != np.float32(h))


# ---------------------------------------------------------------- 3., 4. a mask of ones; NaN at the unobserved pixels
@pytest.mark.parametrize("nh,nl,xd", [(64, 8, 48), (200, 100, 784)])
def test_a_mask_of_ones_is_the_unmasked_call(gpu, nh, nl, xd):
    m, x, P = _net(nh, nl, xd)
    N, Cn, T = 5, 13, 4
    kw = dict(n_chains=Cn, leapfrog=2, step_size=0.35, adapt=True, betas=np.linspace(0, 1, T + 1), trace=True)
    ones = np.ones((N, xd), np.uint8)
    for extra in (dict(), dict(init="prior"), dict(noise=R.noise(7, T, Cn, N, nl))):
        m.set_step(3, 20)
        a = m.ais(x, **kw, **extra)
        m.set_step(3, 20)
        b = m.ais(x, mask=ones, **kw, **extra)
        _same(a, b)
        m.set_step(3, 20)
        _same(a, m.ais(x, mask=None, **kw, **extra))             # mask == NULL hands on to the unmasked call
    assert 0 < a["accepted"].mean()


@pytest.mark.parametrize("nh,nl,xd,mname", [(64, 8, 48, "sparse05"), (37, 5, 53, "last_only"), (200, 100, 784, "stripes64"), (200, 100, 784, "empty_full")])
def test_nan_at_unobserved_pixels_reaches_no_output(gpu, nh, nl, xd, mname):
    m, x, P = _net(nh, nl, xd)
    N, Cn, T = 5, 13, 4
    mask = AM.mask_of(mname, N, xd)
    xn = np.where(mask != 0, x, np.float32(np.nan)).astype(np.float32)
    xg = np.where(mask != 0, x, np.float32(-3e38)).astype(np.float32)
    assert np.isnan(xn).any()
    kw = dict(mask=mask, n_chains=Cn, leapfrog=2, step_size=0.35, adapt=True, betas=np.linspace(0, 1, T + 1), trace=True)
    for init in ("encoder", "prior"):
        runs = []
        for xx in (x, xn, xg):
            m.set_step(3, 20)
            runs.append(m.ais(xx, init=init, **kw))
        for other in runs[1:]:
            _same(runs[0], other)
        assert all(np.all(np.isfinite(runs[0][key])) for key in AIS_KEYS)


# ---------------------------------------------------------------- 5. anchors
def test_one_temperature_is_imputes_bound(gpu):
    m, x, P = _net(64, 8, 48)
    N, Cn = 3, 7
    x = x[:N]
    for mname in ("dense95", "sparse05", "empty_full"):
        mask = AM.mask_of(mname, N, 48)
        m.set_step(5, 11)
        r = m.ais(x, mask=mask, n_chains=Cn, leapfrog=1, step_size=0.1, adapt=False, betas=[0.0, 1.0])
        m.set_step(5, 11)
        imp = m.impute(x, mask=mask, n_samples=Cn, outputs=("log_px", "log_w", "q_mu", "q_sigma"))
        print(mname, "ais", r["log_px"], "impute", imp["log_px"])
        assert np.max(np.abs(r["log_px"] - imp["log_px"])) <= 1e-4
        assert np.array_equal(r["q_mu"], imp["q_mu"]) and np.array_equal(r["q_sigma"], imp["q_sigma"])
        # a vanishing step size: the chains stay where they start and any schedule telescopes to the same weight
        m.set_step(5, 11)
        b7 = np.array([0.0, 0.05, 0.1, 0.4, 0.45, 0.9, 1.0], dtype=np.float32)
        r7 = m.ais(x, mask=mask, n_chains=Cn, leapfrog=2, step_size=1e-30, adapt=False, betas=b7)
        np.testing.assert_allclose(r7["log_w"], r["log_w"], rtol=2e-6, atol=1e-6)


# ---------------------------------------------------------------- 6. nothing observed
@pytest.mark.parametrize("nh,nl,xd", AM.SHAPES)
def test_nothing_observed(gpu, nh, nl, xd):
    """The heads are those of the zero image, the target is the prior and log p(x_obs) = 0, for both inits."""
    m, x, P = _net(nh, nl, xd)
    N, Cn, T, L, h = 3, 7, 6, 2, 0.3
    x = x[:N]
    mask = np.zeros((N, xd), np.uint8)
    betas = np.linspace(0, 1, T + 1).astype(np.float32)
    eps0, mom, unif = R.noise(11, T, Cn, N, nl)
    zero = m.ais(np.zeros((N, xd), np.float32), n_chains=1, leapfrog=1, step_size=0.1, betas=[0.0, 1.0], noise=R.noise(1, 1, 1, N, nl))
    for init in ("encoder", "prior"):
        r = m.ais(x, mask=mask, n_chains=Cn, leapfrog=L, step_size=h, adapt=False, init=init, betas=betas, noise=(eps0, mom, unif))
        if init == "encoder":
            assert np.array_equal(r["q_mu"], zero["q_mu"]) and np.array_equal(r["q_sigma"], zero["q_sigma"])
        e64 = AM.restate_ais(P, x, mask, r["q_mu"], r["q_sigma"], betas, L, h, eps0, mom, unif, np.float64)
        e32 = AM.restate_ais(P, x, mask, r["q_mu"], r["q_sigma"], betas, L, h, eps0, mom, unif, np.float32)
        # prior init: every increment is (bt - bp) (lj - l0) with lj = l0 up to float32 rounding, so log_w is 0 within the run-time tolerance;
        # encoder init: log_w is the restatement's within it, and log_px is a (noisy, C = 7) estimate of log 1
        tol = _tol(e32["log_w"], e64["log_w"])
        err = float(np.max(np.abs(r["log_w"] - e64["log_w"])))
        print("%s: log_w device error %.3g, tolerance %.3g, ratio %.3f; log_px %s" % (init, err, tol, err / tol, r["log_px"]))
        assert err <= tol
        if init == "prior":
            assert np.max(np.abs(e64["log_w"])) <= 1e-12 and np.max(np.abs(r["log_px"])) <= tol
        else:
            assert np.max(np.abs(r["log_px"] - R.log_mean_exp(e64["log_w"]))) <= tol


# ---------------------------------------------------------------- 7. determinism, bitwise
@pytest.mark.parametrize("nh,nl,xd", [(64, 8, 48), (200, 100, 784)])
def test_chunking_position_masks_and_repeat_are_bitwise(gpu, nh, nl, xd):
    m, x, P = _net(nh, nl, xd)
    N, Cn, T = 5, 13, 5
    mask = AM.mask_of("dense95" if xd == 48 else "stripes64", N, xd)
    mask[3] = AM.mask_of("sparse05", N, xd)[3]
    kw = dict(n_chains=Cn, leapfrog=2, step_size=0.35, adapt=True, betas=np.linspace(0, 1, T + 1), trace=True)
    runs = []
    for chunk in (0, 1, 2, 0):
        m.set_option("ais_t_chunk", chunk)
        m.set_step(3, 20)
        runs.append(m.ais(x, mask=mask, **kw))
    m.set_option("ais_t_chunk", 0)
    for other in runs[1:]:
        _same(runs[0], other)
    assert 0 < runs[0]["accepted"].mean() and len(np.unique(runs[0]["step_size"])) > 1
    # image 2 alone, told its global index, against the same image inside N = 5
    m.set_step(3, 22)
    one = m.ais(x[2:3], mask=mask[2:3], **kw)

    def image(r, n):
        return [r[k][..., n] for k in ("log_w", "step_size", "log_px", "ess", "dH", "accepted")] + [r["z"][:, n], r["q_mu"][n], r["q_sigma"][n]]

    for a, b in zip(image(one, 0), image(runs[0], 2)):
        assert np.array_equal(a, b)
    # the other images' masks: changing only image 0's mask changes no bit of the other images' outputs, and changes image 0's
    other = mask.copy()
    other[0] = 1 - other[0]
    m.set_step(3, 20)
    r2 = m.ais(x, mask=other, **kw)
    for n in range(1, N):
        for a, b in zip(image(r2, n), image(runs[0], n)):
            assert np.array_equal(a, b), n
    assert not np.array_equal(r2["log_w"][:, 0], runs[0]["log_w"][:, 0])


# ---------------------------------------------------------------- 8. the device's own noise
def test_device_noise_and_step_advance(gpu):
    m, x, P = _net(64, 8, 48)
    N, Cn, T, nl = 3, 7, 6, 8
    x = x[:N]
    mask = AM.mask_of("empty_full", N, 48)
    betas = np.linspace(0, 1, T + 1)
    m.set_step(9, 4)
    want = m.debug_eps(N, Cn, 0)
    r = m.ais(x, mask=mask, n_chains=Cn, leapfrog=1, step_size=1e-30, adapt=False, init="prior", betas=betas)
    assert np.array_equal(r["z"], want)                           # prior init: z = e, and the chains never move
    after = m.debug_eps(N, Cn, 0)
    m.set_step(9 + T + 1, 4)
    assert np.array_equal(after, m.debug_eps(N, Cn, 0))
    m.set_step(9 + T, 4)
    assert not np.array_equal(after, m.debug_eps(N, Cn, 0))
    # the caller's noise leaves the step alone; passing the device's e_0 with momenta that never act (h = 1e-30) is the device-noise run
    m.set_step(9, 4)
    eps0, mom, unif = R.noise(3, T, Cn, N, nl)
    rn = m.ais(x, mask=mask, n_chains=Cn, leapfrog=1, step_size=1e-30, adapt=False, betas=betas, noise=(want, mom, unif))
    assert np.array_equal(m.debug_eps(N, Cn, 0), want)
    m.set_step(9, 4)
    rd = m.ais(x, mask=mask, n_chains=Cn, leapfrog=1, step_size=1e-30, adapt=False, betas=betas)
    for key in ("log_w", "log_px", "z", "ess", "q_mu", "q_sigma"):
        assert np.array_equal(rn[key], rd[key]), key


# ---------------------------------------------------------------- 9. ground truth on the device
def test_against_masked_quadrature_and_bdmc(gpu):
    """test_gpu_ais.py::test_against_quadrature_and_bdmc under a 50 % mask, at its model and margins."""
    from iwae_amd import iwae1
    nh, nl, xd, N, Cn, T = 64, 2, 48, 4, 64, 200
    x, P, _ = MG.inputs(1, nh, nl, xd, N, 1, 41)
    model = iwae1.IWAE(nh, nl, x_dim=xd, seed=123)
    m = model._net
    m.set_params(O.flatten_params(P))
    m.set_eval_precision("fp32")
    mask = (np.random.default_rng(45).random((N, xd)) < 0.5).astype(np.uint8)
    truth = AM.quadrature_log_px(P, x, mask)
    m.set_step(1, 0)
    r = m.ais(x, mask=mask, n_chains=Cn, n_temps=T, leapfrog=5, step_size=0.3, adapt=False, init="prior")
    se = R.log_mean_se(r["log_w"])
    print("truth", truth, "ais", r["log_px"], "se", se, "accept", r["accept_rate"].mean(), "ess", r["ess"])
    assert np.all(np.abs(r["log_px"] - truth) <= 4 * se), (r["log_px"] - truth, se)
    one = m.ais(x, mask=mask, n_chains=Cn, leapfrog=5, step_size=0.3, adapt=False, init="prior", betas=[0.0, 1.0])
    assert np.mean(np.abs(r["log_px"] - truth)) < np.mean(np.abs(one["log_px"] - truth))
    b = model.bdmc(4, n_chains=Cn, n_temps=T, seed=5, leapfrog=5, step_size=0.3, adapt=False, init="prior",
                   mask=lambda xs: np.random.default_rng(46).random(xs.shape) < 0.5)
    assert b["mask"].shape == b["x"].shape and 0.3 < b["mask"].mean() < 0.7
    truth_b = AM.quadrature_log_px(P, b["x"], b["mask"])
    se_l, se_u = R.log_mean_se(b["forward"]["log_w"]), R.log_mean_se(b["reverse"]["log_w"])
    print("bdmc truth", truth_b, "lower", b["lower"], se_l, "upper", b["upper"], se_u, "gap", b["gap"])
    assert np.all(np.abs(b["lower"] - truth_b) <= 4 * se_l) and np.all(np.abs(b["upper"] - truth_b) <= 4 * se_u)
    assert np.all(b["lower"] - 4 * se_l <= truth_b) and np.all(truth_b <= b["upper"] + 4 * se_u)
    model._net.close()


# ---------------------------------------------------------------- 10. errors
def _raw(m, x, mask, N, **fields):
    from iwae_amd import _capi
    betas = np.array([0.0, 1.0], dtype=np.float32)
    o = _capi.AisOptions()
    o.C, o.T, o.L, o.betas, o.step_size = 2, 1, 1, betas.ctypes.data, 0.1
    for k, v in fields.items():
        setattr(o, k, v)
    lpx = np.zeros(max(N, 1), dtype=np.float64)
    outs = _capi.AisOutputs()
    outs.log_px = lpx.ctypes.data
    return m.lib.iwae_ais_masked(m.h, x.ctypes.data, None if mask is None else mask.ctypes.data, N, C.byref(o), C.byref(outs)), lpx


def test_rejected_arguments_leave_the_step_alone(gpu):
    from iwae_amd.native import NativeModel
    m, x, P = _net(64, 8, 48)
    x = np.ascontiguousarray(x[:2])
    mask = AM.mask_of("dense95", 2, 48)
    m.set_step(17, 3)
    want = m.debug_eps(2, 2, 0)
    ok = dict(mask=mask, n_chains=2, leapfrog=1, step_size=0.1, betas=[0.0, 1.0])
    bad = [dict(ok, n_chains=0), dict(ok, n_chains=-3), dict(ok, leapfrog=0), dict(ok, betas=[0.5]), dict(ok, betas=[0.0, 1.5]),
           dict(ok, betas=[-0.1, 1.0]), dict(ok, betas=[0.0, np.nan]), dict(ok, step_size=0.0), dict(ok, step_size=-0.1)]
    for kw in bad:
        with pytest.raises(ValueError):
            m.ais(x, **kw)
    with pytest.raises(ValueError):
        m.ais(x[:0], **dict(ok, mask=mask[:0]))
    with pytest.raises(ValueError):
        m.ais(x, **dict(ok, mask=mask[:1]))                        # (the binding: a mask of another shape)
    buf = np.ones(64, dtype=np.float32)
    for fields in (dict(eps0=buf.ctypes.data), dict(mom=buf.ctypes.data, unif=buf.ctypes.data), dict(struct_size=64), dict(init=2),
                   dict(C=(1 << 26) + 1), dict(betas=None)):
        assert _raw(m, x, mask, 2, **fields)[0] == -1, fields
    assert np.array_equal(m.debug_eps(2, 2, 0), want)             # none of them moved the noise step
    assert _raw(m, x, mask, 2)[0] == 0                             # the same call without a defect runs, and advances it by T + 1
    m.set_step(17 + 2, 3)
    after = m.debug_eps(2, 2, 0)
    m.set_step(17, 3)
    rc, lpx = _raw(m, x, mask, 2)
    assert rc == 0 and np.array_equal(m.debug_eps(2, 2, 0), after)
    m.set_step(17, 3)
    assert np.array_equal(lpx, m.ais(x, **ok)["log_px"])
    # mask == NULL through the C ABI is the unmasked call, and its refusals are the unmasked call's
    m.set_step(17, 3)
    rc, lpx0 = _raw(m, x, None, 2)
    m.set_step(17, 3)
    assert rc == 0 and np.array_equal(lpx0, m.ais(x, **dict(ok, mask=None))["log_px"]) and not np.array_equal(lpx0, lpx)
    assert _raw(m, x, None, 2, init=2)[0] == -1 and _raw(m, x, None, 0)[0] == -1
    for make in (lambda: NativeModel(2, [16, 8], [4, 2], x_dim=48, seed=1), lambda: NativeModel(1, 16, 4, x_dim=48, seed=1, cond_dim=10),
                 lambda: NativeModel(1, 16, 4, x_dim=48, seed=1, cond_dim=10, cond_prior=True), lambda: NativeModel(1, 256, 4, x_dim=48, seed=1)):
        other = make()
        other.set_step(17, 3)
        before = other.debug_eps(2, 2, 0)
        with pytest.raises(ValueError):
            other.ais(x, **ok)
        assert np.array_equal(other.debug_eps(2, 2, 0), before)
        other.close()


# ---------------------------------------------------------------- 11. shims
def test_shims(gpu):
    from iwae_amd import iwae1, iwae2
    nh, nl, xd, N = 64, 8, 48, 4
    x, P, _ = MG.inputs(1, nh, nl, xd, N, 1, 7 + nh)
    model = iwae1.IWAE(nh, nl, x_dim=xd, seed=123)
    model._net.set_params(O.flatten_params(PC.spread_params(P, 1)))          # off its initialisation
    model._net.set_eval_precision("fp32")
    mask = AM.mask_of("empty_full", N, xd)
    mean, res = model.ais_log_likelihood(x, mask=mask, n_chains=8, n_temps=20, leapfrog=2, step_size=0.3, adapt=False)
    assert mean == float(np.mean(res["log_px"])) and res["log_px"].shape == (N,) and {"log_w", "ess", "accept_rate", "z", "step_size", "q_mu", "q_sigma", "betas"} <= set(res)
    model._net.set_step(1, 0)
    gaps = model.inference_gaps(x, mask=mask, n_samples=16, n_iters=20, n_eval=4, ais=dict(n_chains=8, n_temps=20, leapfrog=2, step_size=0.3, adapt=False))
    for key in ("log_px", "elbo_amortized", "elbo_local", "approximation_gap", "amortization_gap", "elbo_amortized_se", "elbo_local_se", "log_px_se"):
        assert gaps[key].shape == (N,) and np.all(np.isfinite(gaps[key])), key
    assert {"ais", "amortized", "local"} <= set(gaps)
    # the split is exact: (lp - el) + (el - ea) = lp - ea up to the float64 rounding of its three subtractions and one sum, each at most
    # half an ulp of a value no larger than 2 max(|lp|, |el|, |ea|) -- 4 ulp of that maximum in all
    big = np.maximum(np.maximum(np.abs(gaps["log_px"]), np.abs(gaps["elbo_local"])), np.abs(gaps["elbo_amortized"]))
    assert np.all(np.abs(gaps["approximation_gap"] + gaps["amortization_gap"] - (gaps["log_px"] - gaps["elbo_amortized"])) <= 4 * np.finfo(np.float64).eps * big)
    assert np.array_equal(gaps["approximation_gap"], gaps["log_px"] - gaps["elbo_local"]) and np.array_equal(gaps["amortization_gap"], gaps["elbo_local"] - gaps["elbo_amortized"])
    # all three runs took the mask: each starts from the heads of the masked input, which differ from the complete image's
    plain = model._net.local_posterior(x, n_samples=1, n_iters=0, n_eval=1)
    for run in ("ais", "amortized", "local"):
        assert np.array_equal(gaps[run]["q_mu"], gaps["amortized"]["q_mu"]) and not np.array_equal(gaps[run]["q_mu"][0], plain["q_mu"][0])
    assert np.array_equal(gaps["amortized"]["q_mu"][1], plain["q_mu"][1])      # (image 1 is fully observed)
    print("masked gaps: approximation", gaps["approximation_gap"], "amortization", gaps["amortization_gap"])
    b = model.bdmc(3, n_chains=8, n_temps=20, seed=5, leapfrog=2, step_size=0.3, adapt=False, mask=np.ones((3, xd)))
    assert {"x", "z", "lower", "upper", "gap", "forward", "reverse", "mask"} <= set(b) and b["lower"].shape == (3,)
    model._net.close()
    two = iwae2.IWAE([16, 8], [4, 2], x_dim=48)
    with pytest.raises(NotImplementedError):
        two.ais_log_likelihood(np.zeros((1, 48), np.float32), mask=np.ones((1, 48)))
    with pytest.raises(NotImplementedError):
        two.inference_gaps(np.zeros((1, 48), np.float32), mask=np.ones((1, 48)))
