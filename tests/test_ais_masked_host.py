"""iwae_ais_masked and iwae_local_posterior_masked (include/iwae_amd.h) without a GPU: the ABI, the masked restatements of
tests/_ais_masked_ref.py against the unmasked ones, tests/_impute_ref.py and quadrature, and the admissibility of every case the GPU modules
(tests/test_gpu_ais_masked.py, tests/test_gpu_local_masked.py) run."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import iwae_np as O  # noqa: E402
import make_golden as MG  # noqa: E402
import _ais_ref as R  # noqa: E402
import _local_q_ref as LQ  # noqa: E402
import _impute_ref as IM  # noqa: E402
import _row_eval_bodies as RB  # noqa: E402
import _ais_masked_ref as AM  # noqa: E402

ONE_ROUNDING_MAX = 1e-5      # tests/test_aspect_host.py's: the floor of the run-time tolerance


# ---------------------------------------------------------------- the ABI
def test_header_declares_and_capi_binds_the_masked_calls():
    import ctypes as C
    from iwae_amd import _capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "iwae_amd.h")).read(), flags=re.S)
    assert re.search(r"int iwae_ais_masked\(iwae_handle h, const float\* x, const uint8_t\* mask, int32_t N,\s*const iwae_ais_options\* opt, const iwae_ais_outputs\* out\);", src)
    assert re.search(r"int iwae_local_posterior_masked\(iwae_handle h, const float\* x, const uint8_t\* mask, int32_t N,\s*"
                     r"const iwae_local_options\* opt, const iwae_local_outputs\* out\);", src)
    assert _capi.SYMBOLS["iwae_ais_masked"][1][3:] == _capi.SYMBOLS["iwae_ais"][1][2:] and len(_capi.SYMBOLS["iwae_ais_masked"][1]) == 6
    assert _capi.SYMBOLS["iwae_local_posterior_masked"][1][3:] == _capi.SYMBOLS["iwae_local_posterior"][1][2:]
    assert C.sizeof(_capi.AisOptions) == 72 and C.sizeof(_capi.LocalOptions) == 64      # the structs are the unmasked calls', unchanged


def test_tool_and_section_are_documented():
    assert "dev/ais_masked_time.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "dev", "ais_masked_time.py"))
    assert "iwae_ais_masked" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"^## 22\.", open(os.path.join(ROOT, "DESIGN.md")).read(), flags=re.M)


def test_hole_code_has_one_definition():
    """MO_HOLE lives in device_helpers.h beside BF16_HOLE; no kernel file restates it."""
    csrc = os.path.join(ROOT, "iwae_amd", "csrc")
    defs = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")) and re.search(r"constexpr\s+uint32_t\s+MO_HOLE\s*=", open(os.path.join(csrc, f)).read())]
    assert defs == ["device_helpers.h"]


# ---------------------------------------------------------------- the restatements
def _small(nh, nl, xd, N, seed):
    x, P, _ = MG.inputs(1, nh, nl, xd, N, 1, seed)
    rng = np.random.default_rng(seed + 5)
    mu = 0.3 * rng.standard_normal((N, nl))
    sg = np.exp(0.3 * rng.standard_normal((N, nl)) - 0.5)
    mask = rng.random((N, xd)) < 0.5
    return x, P, mu, sg, mask


def test_a_mask_of_ones_is_the_unmasked_restatement():
    x, P, mu, sg, _ = _small(16, 4, 48, 3, 31)
    ones = np.ones(x.shape, np.uint8)
    T = 4
    betas = np.linspace(0, 1, T + 1)
    eps0, mom, unif = R.noise(32, T, 5, 3, 4)
    a, b = AM.restate_ais(P, x, ones, mu, sg, betas, 3, 0.3, eps0, mom, unif, adapt=True), R.restate(P, x, mu, sg, betas, 3, 0.3, eps0, mom, unif, adapt=True)
    assert sorted(a) == sorted(b)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    noise = RB.local_noise(3, 5, 3, 4)
    for objective in LQ.OBJECTIVES:
        a, b = AM.restate_local(P, x, ones, mu, sg, noise, 3, objective), LQ.restate(P, x, mu, sg, noise, 3, objective)
        assert sorted(a) == sorted(b)
        for key in a:
            assert np.array_equal(a[key], b[key]), (objective, key)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nan_at_unobserved_pixels_changes_nothing(dtype):
    x, P, mu, sg, mask = _small(16, 4, 48, 3, 35)
    xn = np.where(mask, x, np.nan).astype(np.float32)
    T = 3
    betas = np.linspace(0, 1, T + 1)
    eps0, mom, unif = R.noise(36, T, 5, 3, 4)
    a = AM.restate_ais(P, x, mask, mu, sg, betas, 2, 0.3, eps0, mom, unif, dtype)
    b = AM.restate_ais(P, xn, mask, mu, sg, betas, 2, 0.3, eps0, mom, unif, dtype)
    for key in a:
        assert np.array_equal(a[key], b[key]) and np.all(np.isfinite(b[key])), key
    noise = RB.local_noise(3, 5, 3, 4)
    a, b = AM.restate_local(P, x, mask, mu, sg, noise, 3, "iwae", dtype=dtype), AM.restate_local(P, xn, mask, mu, sg, noise, 3, "iwae", dtype=dtype)
    for key in a:
        assert np.array_equal(a[key], b[key]) and np.all(np.isfinite(b[key])), key
    P2 = MG.inputs(1, 16, 2, 48, 3, 1, 35)[1]                     # (two latent dimensions: the quadrature's model)
    q = AM.quadrature_log_px(P2, x, mask, n=101)
    assert np.all(np.isfinite(q)) and np.array_equal(q, AM.quadrature_log_px(P2, xn, mask, n=101))


def test_an_image_with_nothing_observed():
    """lp and its gradient are exactly 0: lj is log p(z) and g is -z; with prior init the AIS weight is 0 and the target the prior."""
    x, P, _, _, mask = _small(16, 4, 48, 3, 37)
    mask = mask.copy()
    mask[1] = False
    dec = R.decoder_of(P, np.float64)
    z = np.random.default_rng(1).standard_normal((3, 4))
    lj, g = AM.joint_and_grad(dec, np.asarray(x, np.float64), mask, z)
    assert lj[1] == -0.5 * np.sum(z[1] * z[1]) - 4 * R.HALF_LOG_2PI and np.array_equal(g[1], -z[1])
    assert lj[0] != -0.5 * np.sum(z[0] * z[0]) - 4 * R.HALF_LOG_2PI
    T = 5
    eps0, mom, unif = R.noise(38, T, 6, 3, 4)
    r = AM.restate_ais(P, x, mask, np.zeros((3, 4)), np.ones((3, 4)), np.linspace(0, 1, T + 1), 3, 0.3, eps0, mom, unif)
    assert np.max(np.abs(r["log_w"][:, 1])) <= 1e-13 and np.min(np.abs(r["log_w"][:, 0])) > 1.0
    assert np.max(np.abs(r["dH"][:, :, 1])) < 0.5          # (the leapfrog error of a standard normal target at h = 0.3)


def test_one_temperature_is_the_masked_importance_weight():
    x, P, mu, sg, mask = _small(16, 4, 48, 3, 31)
    eps0, mom, unif = R.noise(32, 1, 5, 3, 4)
    r = AM.restate_ais(P, x, mask, mu, sg, [0.0, 1.0], 3, 0.2, eps0, mom, unif)
    want = IM.restate(P, x, mask, mu, sg, eps0)
    np.testing.assert_allclose(r["log_w"], want["log_w"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(R.log_mean_exp(r["log_w"]), want["log_px"], rtol=1e-12, atol=1e-12)
    # the local posterior's evaluation pass from the same start and draws is the same weight
    lq = AM.restate_local(P, x, mask, mu, sg, eps0[None], 0)
    np.testing.assert_allclose(lq["log_w"], want["log_w"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(lq["iwae"], want["log_px"], rtol=1e-12, atol=1e-12)


def test_vanishing_step_telescopes_for_any_schedule():
    x, P, mu, sg, mask = _small(16, 4, 48, 3, 33)
    betas = np.array([0.2, 0.25, 0.6, 0.4, 0.9, 0.95, 0.7], dtype=np.float32)
    T = betas.size - 1
    eps0, mom, unif = R.noise(34, T, 5, 3, 4)
    r = AM.restate_ais(P, x, mask, mu, sg, betas, 2, 1e-30, eps0, mom, unif)
    want = np.float64(betas[-1] - betas[0]) * IM.restate(P, x, mask, mu, sg, eps0)["log_w"]
    np.testing.assert_allclose(r["log_w"], want, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(r["z"], mu[None] + sg[None] * eps0, rtol=0, atol=1e-25)


def test_masked_quadrature_is_imputes():
    _, P, _ = MG.inputs(1, 64, 2, 48, 4, 1, 41)
    rng = np.random.default_rng(3)
    x, mask = (rng.random((4, 48)) < 0.5).astype(np.float64), rng.random((4, 48)) < 0.5
    np.testing.assert_allclose(AM.quadrature_log_px(P, x, mask, n=401), IM.quadrature_log_px_obs(P, x, mask, n=401), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(AM.quadrature_log_px(P, x, np.ones_like(mask), n=401), R.quadrature_log_px(P, x, n=401), rtol=1e-12, atol=1e-12)
    assert np.max(np.abs(AM.quadrature_log_px(P, x, np.zeros_like(mask), n=401))) < 1e-9       # nothing observed: the prior's mass, log 1


def test_forward_and_reverse_masked_runs_bracket_masked_quadrature():
    """test_ais_host.py::test_forward_and_reverse_runs_bracket_quadrature under a 50 % mask: the simulated z is an exact posterior sample
    given x_obs too (x_obs is a marginal of x), so the reverse run from it bounds log p(x_obs) from above."""
    from iwae_amd.native import ais_schedule
    _, P, _ = MG.inputs(1, 64, 2, 48, 4, 1, 41)
    N, Cn, T, L, h = 4, 64, 200, 5, 0.3
    rng = np.random.default_rng(42)
    zt = rng.standard_normal((N, 2))
    probs = O.sigmoid(R.logits_of(R.decoder_of(P, np.float64), zt)[2])
    x = (rng.random(probs.shape) < probs).astype(np.float64)
    mask = np.random.default_rng(45).random(x.shape) < 0.5
    truth = AM.quadrature_log_px(P, x, mask)
    assert np.all(truth > R.quadrature_log_px(P, x) + 1.0)        # (fewer Bernoulli terms: another number)
    mu, sg = np.zeros((N, 2)), np.ones((N, 2))
    betas = ais_schedule(T, "sigmoid")
    eps0, mom, unif = R.noise(43, T, Cn, N, 2)
    fwd = AM.restate_ais(P, x, mask, mu, sg, betas, L, h, eps0, mom, unif)
    _, mom2, unif2 = R.noise(44, T, Cn, N, 2)
    rev = AM.restate_ais(P, x, mask, mu, sg, betas[::-1], L, h, eps0, mom2, unif2, z0=np.broadcast_to(zt[None], (Cn, N, 2)))
    lower, se_l = R.log_mean_exp(fwd["log_w"]), R.log_mean_se(fwd["log_w"])
    upper, se_u = -R.log_mean_exp(rev["log_w"]), R.log_mean_se(rev["log_w"])
    print("truth", truth, "lower", lower, "se", se_l, "upper", upper, "se", se_u, "accept", fwd["accepted"].mean(), rev["accepted"].mean())
    assert np.all(np.abs(lower - truth) <= 4 * se_l), (lower - truth, se_l)
    assert np.all(np.abs(upper - truth) <= 4 * se_u), (upper - truth, se_u)
    assert np.all(lower - 4 * se_l <= truth) and np.all(truth <= upper + 4 * se_u)


# ---------------------------------------------------------------- the masks do what their names say
def test_masks_hit_the_epilogue_edges():
    m = AM.mask_of("pass0", 2, 784)
    assert not m[:, :64].any() and m[:, 64:].all()
    m = AM.mask_of("tile1", 2, 48)
    assert not m[:, 16:32].any() and m[:, :16].all() and m[:, 32:].all()
    m = AM.mask_of("last_only", 2, 53)
    assert m[:, :48].all() and not m[:, 48:52].any() and m[:, 52].all()
    m = AM.mask_of("last_hole", 2, 53)
    assert m[:, :52].all() and not m[:, 52].any()
    for X in (48, 53, 784):
        m = AM.mask_of("empty_full", 3, X)
        assert not m[0].any() and m[1].all() and 0 < m[2].mean() < 1
    m = AM.mask_of("stripes64", 2, 784)
    assert m[:, :64].all() and not m[:, 64:128].any()
    assert 0.9 < AM.mask_of("dense95", 5, 784).mean() < 0.99 and 0.01 < AM.mask_of("sparse05", 5, 784).mean() < 0.1
    for shape, names in AM.SHAPE_MASKS.items():
        assert shape in AM.SHAPES and all(n in AM.MASKS for n in names)
    # every trajectory and local case names a mask its shape runs
    for c in list(AM.TRAJECTORIES.values()):
        assert c[9] in AM.MASKS
    assert {c[:3] for c in AM.TRAJECTORIES.values()} == {(64, 8, 48), (200, 100, 784)}
    assert {c[4] for c in AM.LOCAL_CASES} == {1, 13, 64} and max(c[5] for c in AM.LOCAL_CASES) <= 6 and max(c[3] for c in AM.LOCAL_CASES) <= AM.NMAX


# ---------------------------------------------------------------- admissibility of what the GPU modules run
def _heads(P, x, mask):
    mu, sg = IM.encoder_heads(P, x, mask)
    return mu.astype(np.float32), sg.astype(np.float32)


@pytest.mark.parametrize("shape,mname", [(s, n) for s in AM.SHAPES for n in AM.SHAPE_MASKS[s]], ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_single_transition_tolerances_resolve_the_energy(shape, mname):
    """Every single-transition case of the GPU module: finite, and its run-time dH tolerance (8 x the float32 restatement's deviation, floor
    1e-5) is no smaller than one float32 ulp of the largest energy U_t(e_0) among its chains -- below that the tolerance does not describe
    float32 arithmetic but one chain's luck in numpy (tests/_ais_masked_ref.py SINGLE_SEEDS) -- and far below what a wrong tile moves."""
    nh, nl, xd = shape
    xa, P, _ = MG.inputs(1, nh, nl, xd, AM.NMAX, 1, 7 + nh)
    dec = R.decoder_of(P, np.float64)
    bt = np.float64(np.float32(AM.SINGLE_BETAS[1]))
    for N, Cn in AM.SINGLE_CASES:
        x, mask = xa[:N], AM.mask_of(mname, N, xd)
        for init in ("encoder", "prior"):
            mu, sg = _heads(P, x, mask) if init == "encoder" else (np.zeros((N, nl), np.float32), np.ones((N, nl), np.float32))
            for L in (1, 3):
                eps0, mom, unif = R.noise(AM.single_seed(shape, mname, N, Cn, L, init), 1, Cn, N, nl)
                e64 = AM.restate_ais(P, x, mask, mu, sg, AM.SINGLE_BETAS, L, AM.SINGLE_H, eps0, mom, unif, np.float64)
                e32 = AM.restate_ais(P, x, mask, mu, sg, AM.SINGLE_BETAS, L, AM.SINGLE_H, eps0, mom, unif, np.float32)
                tol = RB._tol(e32["dH"], e64["dH"])
                e, mur, sgr = eps0.reshape(Cn * N, nl).astype(np.float64), np.tile(mu, (Cn, 1)).astype(np.float64), np.tile(sg, (Cn, 1)).astype(np.float64)
                lj, _ = AM.joint_and_grad(dec, np.tile(x, (Cn, 1)).astype(np.float64), np.tile(mask != 0, (Cn, 1)), mur + sgr * e)
                energy = float(np.max(np.abs((1.0 - bt) * R.base_density(e, sgr) + bt * lj)))
                ulp = float(np.spacing(np.float32(energy)))
                print("N%d C%d %s L%d: dH tolerance %.3g, one float32 ulp of |U| = %.1f is %.3g" % (N, Cn, init, L, tol, energy, ulp))
                assert np.all(np.isfinite(e64["dH"])) and np.all(np.isfinite(e64["log_w"])) and np.all(np.isfinite(e64["z"]))
                assert ulp <= tol < 1e-2, (N, Cn, init, L, tol, ulp)


@pytest.mark.parametrize("name", sorted(AM.TRAJECTORIES))
def test_trajectory_cases_are_admissible(name):
    """The float32 and float64 restatements alone, under test_gpu_ais.py::test_trajectories' cut rule (delta = 64 x the measured float32 dH
    deviation, floor 1e-4), cut at most 5 % of the chains short -- half the GPU test's 10 % cap -- and at least one whole chain survives."""
    nh, nl, xd, N, Cn, T, L, h, adapt, mname, seed = AM.TRAJECTORIES[name]
    x, P, _ = MG.inputs(1, nh, nl, xd, AM.NMAX, 1, 7 + nh)
    x = x[:N]
    mask = AM.mask_of(mname, N, xd)
    mu, sg = _heads(P, x, mask)
    betas = np.linspace(0.0, 1.0, T + 1).astype(np.float32)
    eps0, mom, unif = R.noise(seed, T, Cn, N, nl)
    e64 = AM.restate_ais(P, x, mask, mu, sg, betas, L, h, eps0, mom, unif, np.float64, adapt=adapt)
    e32 = AM.restate_ais(P, x, mask, mu, sg, betas, L, h, eps0, mom, unif, np.float32, adapt=adapt)
    dev_dH, delta, cut, scale, whole = AM.trajectory_cut(e32, e64)
    frac = float(np.mean(cut < T))
    print("%s seed %d: accept rate %.3f, float32 dH deviation %.3g, delta %.3g, chains cut short %.3f (<= 0.05), whole chains %d of %d"
          % (name, seed, e64["accepted"].mean(), dev_dH, delta, frac, int(whole.sum()), whole.size))
    assert np.all(np.isfinite(e64["log_w"])) and np.all(np.isfinite(e64["z"]))
    assert frac <= 0.05
    assert whole.any()
    if h == 0.9:
        assert 0.05 < 1.0 - e64["accepted"].mean() < 0.95


@pytest.mark.parametrize("case", AM.LOCAL_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_local_cases_do_not_amplify_a_float32_rounding(case):
    """tests/test_aspect_host.py::test_local_posterior_case_is_well_conditioned for the masked cases: finite, the run-time tolerance (8 x the
    float32 deviation) separates a wrong tile from rounding, and one float32 rounding of the weights moves no element of the gradient by
    more than the tolerance's floor."""
    nh, nl, xd, N, S, T, objective, mname = case
    x, P, _ = MG.inputs(1, nh, nl, xd, AM.NMAX, 1, 7 + nh)
    x = x[:N]
    mask = AM.mask_of(mname, N, xd)
    mu, sg = _heads(P, x, mask)
    noise = RB.local_noise(N, S, T, nl)
    e64 = AM.restate_local(P, x, mask, mu, sg, noise, T, objective, lr=0.05, dtype=np.float64)
    e32 = AM.restate_local(P, x, mask, mu, sg, noise, T, objective, lr=0.05, dtype=np.float32)
    dev = {key: float(np.max(np.abs(np.asarray(e32[key], dtype=np.float64) - e64[key]))) for key in ("grad", "mu", "log_w")}
    rng = np.random.default_rng(1)
    moved = 0.0
    for _ in range(6):
        Q = [(W * (1.0 + 6e-8 * rng.standard_normal(W.shape)), b * (1.0 + 6e-8 * rng.standard_normal(b.shape))) for W, b in P]
        moved = max(moved, float(np.max(np.abs(AM.restate_local(Q, x, mask, mu, sg, noise, T, objective, lr=0.05, dtype=np.float64)["grad"] - e64["grad"]))))
    print("one float32 rounding of the weights moves grad by %.3g (<= %.3g); float32 deviation grad %.3g, mu %.3g, log_w %.3g; |grad| max %.3g"
          % (moved, ONE_ROUNDING_MAX, dev["grad"], dev["mu"], dev["log_w"], float(np.max(np.abs(e64["grad"])))))
    assert all(np.all(np.isfinite(e64[key])) for key in ("grad", "bound", "mu", "sigma", "elbo", "iwae", "log_w"))
    assert 8.0 * dev["grad"] < 0.05 * float(np.max(np.abs(e64["grad"])))
    assert moved <= ONE_ROUNDING_MAX
