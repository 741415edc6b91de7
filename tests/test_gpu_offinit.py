"""Parity OFF the random initialisation: sharp posteriors (the sigma floor), saturated logits and tanh units, wide posteriors.

Every other parity module runs where sigma ~ 1 and |logit| <= ~6: there a kernel that dropped the `+ 1e-6` of sigma = exp(a) + 1e-6, took
the derivative through exp as sigma instead of sigma - 1e-6, or kept one of DReG's two floors moves every checked quantity by ~1e-6
relative, far below every bound.  Here the SAME operations run against the SAME oracle at the SAME tolerances (tests/_parity_common.py,
and the bounds of the tests named in the docstrings) on the case table of tests/_offinit_cases.py, whose parameters are built by
sharp_params / saturated_params; tests/test_offinit_host.py shows from the oracle alone that every case is well conditioned in the
arithmetic it runs in, and that each of those three defects moves a compared quantity by more than 3x its bound on every sharp case.

Sharp cases run in both arithmetics; saturated and wide ones in float32 mode and the float32 evaluator only (one bf16 rounding moves the
oracle by more than the bf16 bounds there).  Every test prints its worst figures next to their bounds (pytest -rP shows them)."""
import numpy as np
import pytest

from oracle import iwae_np as O, philox_np
import _ais_ref as R
import _impute_ref as IM
import _local_q_ref as LQ
import _offinit_cases as C
import _posterior_ref as PR
from _parity_common import (EMU_ROW_ATOL, EMU_SCALAR_ATOL, EMU_GRAD_REL, EXACT_SCALAR_ATOL, EXACT_GRAD_REL, F32_SCALAR_REL, F32_GRAD_REL,
                            F32_ROW_ATOL, _grad_rel_errors, _elementwise_ok, _densities_at_device_head, _densities_at_device_heads_2layer, sharp_params,
                            saturated_params)

pytestmark = pytest.mark.gpu

ROWS_1L = ("lpxz", "lpz", "lqzx")
ROWS_2L = (("lpxz", "lpxz1"), ("lpz", "lpz1z2"), ("lpz2", "lpz2"), ("lqzx", "lqz1x"), ("lqzx2", "lqz2z1"))


def _model(c, precision="bf16", options=None):
    from iwae_amd.native import NativeModel
    nh, nl, xd = c.widths
    nh, nl = (nh, nl) if c.layers == 1 else (list(nh), list(nl))
    return NativeModel(c.layers, nh, nl, x_dim=xd, seed=C.SEED, precision=precision, options=options, cond_dim=c.cond, cond_prior=bool(c.cond))


def _report(tag, **figs):
    print("%s: %s" % (tag, ", ".join("%s %.3g" % kv for kv in figs.items())))


def _adam_ref(P, g):
    ref, _, _ = O.adam_update(O.flatten_params(P), np.asarray(g, dtype=np.float64), 0.0, 0.0, 1, 1e-3)
    return ref


# ---------------------------------------------------------------- (i) the 1-layer bf16 step at sharp posteriors
def _bf16_step_1layer(c, options=None, tag=""):
    """The body of test_train_step_1layer_matches_oracle / test_large_row_count_kernels_match_oracle: rows at the device's own head,
    scalars against both oracles, the gradient per tensor and element-wise, then the fused train step on the Adam reference.  (Printed only: the
    sharpened units' sigma at the device's head relative to the rounding-aware oracle's -- a bf16 flip upstream moves a by ~1e-4.)"""
    nl = c.widths[1]
    x, _, P, eps, _ = C.inputs(c)
    res_e, g_e = C.oracle(c, "emu")
    res_x, g_x = C.oracle(c, "exact")
    m = _model(c, options=options)
    m.set_params(O.flatten_params(P))
    if c.noise == "device":
        m.set_step(C.NOISE_STEP, 0)
    dev_eps = None if c.noise == "device" else eps
    r = m.forward_backward(x, c.k, c.beta, c.obj, eps=dev_eps, want=ROWS_1L + ("al", "z"))
    g = m.get_grads()
    assert np.all(np.isfinite(g))
    at = _densities_at_device_head(m, P, x, eps, nl)
    keys = C.scalar_keys(c)
    errs_e, errs_x = _grad_rel_errors(g, g_e), _grad_rel_errors(g, g_x)
    units = [u for u in range(nl) if P[3][1][u] < -3.0]
    sig_rel = float(np.max(np.abs(at["sigma"] / (np.exp(res_e["a"][3]) + 1e-6) - 1.0)[:, units]))
    _report("1-layer bf16 %s%s" % (C.case_id(c), tag), rows_at_head=max(float(np.max(np.abs(r[key] - at[key]))) for key in ROWS_1L),
            rows_q98=max(float(np.quantile(np.abs(r[key] - res_e[key]), 0.98)) for key in ROWS_1L), rows_bound=EMU_ROW_ATOL,
            scalar_emu=max(abs(r[key] - res_e[key]) for key in keys), bound=EMU_SCALAR_ATOL,
            scalar_exact=max(abs(r[key] - res_x[key]) for key in keys), bound_x=EXACT_SCALAR_ATOL, grad_emu=max(errs_e), gbound=EMU_GRAD_REL,
            grad_exact=max(errs_x), gbound_x=EXACT_GRAD_REL, sharp_sigma_vs_oracle_rel=sig_rel, smallest_sigma=float(np.min(at["sigma"])))
    np.testing.assert_allclose(r["z"], res_e["z"], rtol=0, atol=1e-2)
    np.testing.assert_allclose(r["al"].sum(0), 1.0, atol=1e-5)
    for key in ROWS_1L:
        assert np.max(np.abs(r[key] - at[key])) < EMU_ROW_ATOL, key                      # every row, at the device's own encoder head
        assert np.quantile(np.abs(r[key] - res_e[key]), 0.98) < EMU_ROW_ATOL, key        # the typical row against the pure oracle
    for key in keys:
        assert abs(r[key] - res_e[key]) < EMU_SCALAR_ATOL, (key, r[key], res_e[key])
        assert abs(r[key] - res_x[key]) < EXACT_SCALAR_ATOL, (key, r[key], res_x[key])
    if c.obj == "dreg":
        assert abs(r["inference_loss"] - res_e["inference_loss"]) < 5e-3 * abs(res_e["inference_loss"]) + 0.05
    assert max(errs_e) < EMU_GRAD_REL, errs_e
    assert max(errs_x) < EXACT_GRAD_REL, errs_x
    worst = _elementwise_ok(g, g_e)
    if c.noise == "device":
        m.set_step(C.NOISE_STEP, 0)
    r2 = m.train_step(x, c.k, c.beta, 1e-3, c.obj, eps=dev_eps)
    assert abs(r2["iwae_elbo"] - r["iwae_elbo"]) < 1e-5
    np.testing.assert_array_equal(m.get_grads(), g)
    d_adam = float(np.max(np.abs(m.get_params() - _adam_ref(P, g))))
    _report("   ", elementwise=worst, bound=3e-2, adam=d_adam, abound=2e-6)
    assert d_adam < 2e-6
    m.close()


@pytest.mark.parametrize("c", C.BF16_1L, ids=C.case_id)
def test_train_step_sharp_posteriors_matches_oracle(gpu, c):
    _bf16_step_1layer(c)


@pytest.mark.parametrize("c", C.BF16_1L_QW, ids=C.case_id)
def test_train_step_sharp_posteriors_forced_200_row_decoder(gpu, c):
    """The 8 500-row cases once more with the 16-wave / 200-row shape of the pipelined decoder forced (bern_qw_force)."""
    _bf16_step_1layer(c, options={"bern_qw_force": 1}, tag=" bern_qw_force")


@pytest.mark.parametrize("c", C.NOISE_1L, ids=C.case_id)
def test_device_noise_step_sharp_posteriors_matches_oracle(gpu, c):
    """The device's own draws (no eps) against the oracle on their NumPy restatement."""
    _bf16_step_1layer(c, tag=" device noise")


# ---------------------------------------------------------------- (ii) the 2-layer bf16 step
@pytest.mark.parametrize("c", C.L2_BF16, ids=C.case_id)
def test_train_step_2layer_sharp_posteriors_matches_oracle(gpu, c):
    """The assertions and bounds of test_train_step_2layer_matches_oracle (few rows) and of its row-count class in
    test_gpu_sample_axis.py / test_gpu_ragged_widths.py (8 255 rows)."""
    nl = list(c.widths[1])
    B, k = c.B, c.k
    x, _, P, eps, _ = C.inputs(c)
    res_e, g_e = C.oracle(c, "emu")
    res_x, g_x = C.oracle(c, "exact")
    m = _model(c)
    m.set_params(O.flatten_params(P))
    r = m.forward_backward(x, k, 1.0, c.obj, eps=eps, want=("z", "z2", "al", "log_w", "lpxz", "lpz", "lqzx", "lpz2", "lqzx2"))
    g = m.get_grads()
    assert np.all(np.isfinite(g))
    at = _densities_at_device_heads_2layer(m, eps[0], eps[1], B, k, nl, P, x)
    worst_at = 0.0
    for a, b in ROWS_2L:
        d_at = float(np.max(np.abs(r[a] - at[b])))
        worst_at = max(worst_at, d_at / (EMU_ROW_ATOL if b == "lpxz1" else 2e-2))
        assert d_at < (EMU_ROW_ATOL if b == "lpxz1" else 2e-2), (b, d_at)
        err_e = np.abs(r[a] - res_e[b])
        if B * k <= 4096:
            assert err_e.max() < (0.4 if b == "lpz1z2" else 0.05), (b, err_e.max())
        elif b == "lpxz1":
            assert np.quantile(err_e, 0.98) < EMU_ROW_ATOL, (b, np.quantile(err_e, 0.98))
        else:
            assert np.quantile(err_e, 0.9) < 0.05, (b, np.quantile(err_e, 0.9))
    np.testing.assert_allclose(r["z"], res_e["z1"], rtol=0, atol=1e-2)
    errs_e, errs_x = _grad_rel_errors(g, g_e), _grad_rel_errors(g, g_x)
    s_tol, g_tol = (0.05, 2e-2) if B * k <= 4096 else (EMU_SCALAR_ATOL, EMU_GRAD_REL)
    keys = ("vae_elbo", "iwae_elbo", "iwae_eq14")
    _report("2-layer bf16 %s" % C.case_id(c), rows_at_heads_over_bound=worst_at, scalar_emu=max(abs(r[key] - res_e[key]) for key in keys), bound=s_tol,
            scalar_exact=max(abs(r[key] - res_x[key]) for key in keys), bound_x=0.3, grad_emu=max(errs_e), gbound=g_tol, grad_exact=max(errs_x), gbound_x=5e-2)
    for key in keys:
        assert abs(r[key] - res_e[key]) < s_tol, (key, r[key], res_e[key])
        assert abs(r[key] - res_x[key]) < 0.3, (key, r[key], res_x[key])
    lw = r["log_w"].astype(np.float64)
    assert abs(r["iwae_elbo"] - float(np.mean(O.logmeanexp(lw, axis=0)))) < 1e-3
    assert abs(r["vae_elbo"] - float(np.mean(lw))) < 1e-3
    assert max(errs_e) < g_tol, errs_e
    assert max(errs_x) < 5e-2, errs_x
    m.adam_step(1e-3)
    assert np.max(np.abs(m.get_params() - _adam_ref(P, g))) < 2e-6
    m.close()


# ---------------------------------------------------------------- (iii) the conditional-prior model, sharp on the encoder head
@pytest.mark.parametrize("c", C.COND_BF16, ids=C.case_id)
def test_conditional_prior_model_sharp_posteriors_matches_oracle(gpu, c):
    """The assertions and bounds of test_conditional_prior_model_matches_oracle."""
    x, _, P, eps, y = C.inputs(c)
    res_e, g_e = C.oracle(c, "emu")
    m = _model(c)
    assert m.n_params == sum(W.size + b.size for W, b in P)
    m.set_params(O.flatten_params(P))
    m.set_condition(y)
    r = m.forward_backward(x, c.k, c.beta, c.obj, eps=eps, want=ROWS_1L)
    errs = _grad_rel_errors(m.get_grads(), g_e)
    keys = ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14")
    _report("conditional prior %s" % C.case_id(c), lpxz=float(np.max(np.abs(r["lpxz"] - res_e["lpxz"]))), lqzx=float(np.max(np.abs(r["lqzx"] - res_e["lqzx"]))),
            rows_bound=EMU_ROW_ATOL, lpz=float(np.max(np.abs(r["lpz"] - res_e["lpz"]))), lpz_bound=0.2, scalar_emu=max(abs(r[key] - res_e[key]) for key in keys),
            bound=EMU_SCALAR_ATOL, grad_emu=max(errs), gbound=EMU_GRAD_REL)
    for key in ROWS_1L:
        assert np.max(np.abs(r[key] - res_e[key])) < (0.2 if key == "lpz" else EMU_ROW_ATOL), key
    for key in keys:
        assert abs(r[key] - res_e[key]) < EMU_SCALAR_ATOL, (key, r[key], res_e[key])
    assert max(errs) < EMU_GRAD_REL, errs
    m.close()


# ---------------------------------------------------------------- (iv) float32 mode against the exact oracle
def _head_restated(P4, x, dtype):
    """BasicBlock (src/iwae1.py:24-44) in NumPy at `dtype`: (mu, sigma)."""
    h = np.asarray(x, dtype=dtype)
    for W, b in P4[:2]:
        h = np.tanh(h @ W.astype(dtype) + b.astype(dtype))
    mu = h @ P4[2][0].astype(dtype) + P4[2][1].astype(dtype)
    sigma = np.exp(h @ P4[3][0].astype(dtype) + P4[3][1].astype(dtype)) + dtype(1e-6)
    return mu, sigma


def _check_head_sigma(m, P, x, D, tag):
    """enc.head's sigma per unit against the float64 head, relative: 8 x (float32 NumPy restatement - float64 restatement), floor 1e-6."""
    head = m.debug_tensor("enc.head").astype(np.float64)
    Dp = head.shape[1] // 2
    sig = head[:x.shape[0], Dp:Dp + D]
    _, s64 = _head_restated(P[0:4], x, np.float64)
    _, s32 = _head_restated(P[0:4], x, np.float32)
    tol = max(8.0 * float(np.max(np.abs(s32.astype(np.float64) - s64) / s64)), 1e-6)
    err = float(np.max(np.abs(sig - s64) / s64))
    _report("   enc.head sigma %s" % tag, rel_error=err, tolerance=tol, smallest_sigma=float(np.min(s64)), largest_sigma=float(np.max(s64)))
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("c", C.F32, ids=C.case_id)
def test_float32_step_off_init_matches_exact_oracle(gpu, c):
    """The body of test_float32_mode_matches_exact_oracle (without `logits` from 8 000 rows, as test_gpu_sample_axis.py runs it)."""
    layers = c.layers
    x, _, P, eps, _ = C.inputs(c)
    res, g = C.oracle(c, "exact")
    if layers == 1:
        rows = tuple((key, key) for key in ROWS_1L)
        keys = ("iwae_elbo",) if c.obj == "dreg" else ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14")
    else:
        rows, keys = ROWS_2L, ("vae_elbo", "iwae_elbo", "iwae_eq14")
    m = _model(c, precision="fp32")
    m.set_params(O.flatten_params(P))
    r = m.forward_backward(x, c.k, c.beta, c.obj, eps=eps, want=tuple(a for a, _ in rows) + ("al", "z"))
    flat = m.get_grads()
    assert np.all(np.isfinite(flat))
    errs = _grad_rel_errors(flat, g)
    d_il = abs(r["inference_loss"] - res["inference_loss"]) / (1e-4 * abs(res["inference_loss"]) + 1e-4) if c.obj == "dreg" else 0.0
    _report("float32 %s" % C.case_id(c), rows=max(float(np.max(np.abs(r[a] - res[b]))) for a, b in rows), rows_bound=F32_ROW_ATOL,
            scalar_over_bound=max(abs(r[key] - res[key]) / (F32_SCALAR_REL * abs(res[key]) + 2e-4) for key in keys), bound=1.0,
            inference_loss_over_bound=d_il, grad=max(errs), gbound=F32_GRAD_REL, max_logit=res["max_logit"])
    _check_head_sigma(m, P, x, c.widths[1] if layers == 1 else c.widths[1][0], C.case_id(c))
    for a, b in rows:
        assert np.max(np.abs(r[a] - res[b])) < F32_ROW_ATOL, (a, float(np.max(np.abs(r[a] - res[b]))))
    np.testing.assert_allclose(r["z"], res["z"] if layers == 1 else res["z1"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(r["al"], res["al"], atol=2e-4)
    for key in keys:
        assert abs(r[key] - res[key]) <= F32_SCALAR_REL * abs(res[key]) + 2e-4, (key, r[key], res[key])
    if c.obj == "dreg":
        assert d_il <= 1.0, (r["inference_loss"], res["inference_loss"])
    assert max(errs) < F32_GRAD_REL, errs
    r0 = m.forward(x, c.k, c.beta, eps=eps, want=("lpxz",))
    for key in keys:
        assert abs(r0[key] - r[key]) <= 1e-6 * abs(r[key]) + 1e-5
    d_fwd = float(np.max(np.abs(r0["lpxz"] - res[C.lpxz_key(c)])))
    assert d_fwd < F32_ROW_ATOL, d_fwd
    m.train_step(x, c.k, c.beta, 1e-3, c.obj, eps=eps)
    g2 = m.get_grads().astype(np.float64)
    assert np.linalg.norm(g2 - flat) / np.linalg.norm(flat) < 1e-5
    d_adam = float(np.max(np.abs(m.get_params() - _adam_ref(P, flat))))
    _report("   forward only / Adam", lpxz=d_fwd, rows_bound=F32_ROW_ATOL, adam=d_adam, abound=2e-6)
    assert d_adam < 2e-6
    m.close()


# ---------------------------------------------------------------- (v) clean saturation, forward only
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_clean_saturation_stays_finite(gpu, precision):
    """Pre-activations of 60 in the first encoder and decoder layers (e^{2|x|} = inf in float32) and logits of 120 (e^{|l|} = inf): every
    output and every gradient is finite; in float32 mode every row is within max(F32_ROW_ATOL, F32_SCALAR_REL |row|) of the exact oracle.
    The gradient is not compared: 1 - y^2 is 0 almost everywhere."""
    from iwae_amd.native import NativeModel
    nh, nl, xd = C.W1
    x, P, eps, fig = C.clean_saturation_inputs()
    k, B = eps.shape[:2]
    res = O.forward_1layer(P, x, eps)
    m = NativeModel(1, nh, nl, x_dim=xd, seed=C.SEED, precision=precision)
    m.set_params(O.flatten_params(P))
    for obj in ("iwae_elbo", "dreg", "vae_elbo_kl"):
        r = m.forward_backward(x, k, 1.0, obj, eps=eps, want=ROWS_1L + ("al", "z", "logits", "log_w", "snis_z"))
        for key, v in r.items():
            assert np.all(np.isfinite(v)), (obj, key)
        assert np.all(np.isfinite(m.get_grads())), obj
        np.testing.assert_allclose(r["al"].sum(0), 1.0, atol=1e-5)
    worst = max(float(np.max(np.abs(r[key] - res[key]) / np.maximum(F32_ROW_ATOL, F32_SCALAR_REL * np.abs(res[key])))) for key in ROWS_1L)
    _report("clean saturation %s" % precision, max_logit=fig["logit"], device_max_logit=float(np.max(np.abs(r["logits"]))), rows_over_bound=worst,
            bound=1.0, lpxz_mean=float(np.mean(res["lpxz"])), device_lpxz_mean=float(np.mean(r["lpxz"])))
    if precision == "fp32":
        assert worst <= 1.0, worst
    m.close()


# ---------------------------------------------------------------- (vi) iwae_eval_llh
@pytest.mark.parametrize("c,precs", C.EVAL, ids=lambda v: C.case_id(v) if isinstance(v, C.Case) else "+".join(v))
def test_eval_llh_off_init_matches_exact_oracle(gpu, c, precs):
    """Per image against the exact oracle on the restated draws; the bounds of test_trained_model_k5000_llh_within_north_star_tolerance:
    5e-3 nat for the float32 evaluator, 0.1 nat for the bf16 one."""
    x, _, P, _, _ = C.inputs(c)
    ref = np.array([float(O.forward_1layer(P, x[i:i + 1], philox_np.device_eps(C.SEED, C.EVAL_STEP, 1, c.k, c.widths[1], batch_offset=i))["iwae_elbo"])
                    for i in range(c.B)])
    m = _model(c)
    m.set_params(O.flatten_params(P))
    for prec in precs:
        m.set_eval_precision(prec)
        m.set_step(C.EVAL_STEP, 0)
        llh, per = m.eval_llh(x, c.k, per_image=True)
        d = float(np.max(np.abs(per - ref)))
        bound = 5e-3 if prec == "fp32" else 0.1
        _report("eval_llh %s %s" % (C.case_id(c), prec), per_image=d, bound=bound, mean_llh=float(ref.mean()))
        assert abs(llh - per.mean()) < 1e-3
        assert d <= bound, (prec, per, ref)
    m.close()


# ---------------------------------------------------------------- (vii) the analyses on one stressed handle per shape
# The analysis modules evaluate their float64 restatement AT the device's own q_mu, q_sigma: whether those heads carry the floor is seen there
# only by comparison at sigma ~ 1.  Here each shape has one handle with two sharp units (SHIFTS2) and saturated_params(.., *SAT) on top of the
# modules' own spread parameters, float32 eval precision; the restatements (_impute_ref, _posterior_ref, _local_q_ref, _ais_ref) and their
# run-time tolerance rule are the modules' own, and IN ADDITION every returned q_mu / q_sigma is held against the float64 head
# O._Block(P[0:4], O._id).fwd(x) -- q_mu by the same rule (absolute), q_sigma RELATIVE per unit with floor 1e-6 (an absolute floor of 1e-5
# would pass a head of 1.1e-7 where 1.11e-6 is due).
AN_SHAPES = [(64, 8, 48), (200, 100, 784)]
AN_CASES = [(3, 7), (2, 65)]
_an_cache = {}


def _an_net(nh, nl, xd):
    key = (nh, nl, xd)
    if key not in _an_cache:
        from iwae_amd.native import NativeModel
        x, Ps, mask = IM.shape_inputs(nh, nl, xd)
        P = saturated_params(sharp_params(Ps, 1, C.SHIFTS2, (3,)), 1, *C.SAT)
        m = NativeModel(1, nh, nl, x_dim=xd, seed=C.SEED)
        m.set_params(O.flatten_params(P))
        m.set_eval_precision("fp32")
        _an_cache[key] = (m, x, P, mask)
    return _an_cache[key]


def _tol(a32, a64, floor=1e-5):
    return max(8.0 * float(np.max(np.abs(np.asarray(a32, dtype=np.float64) - np.asarray(a64, dtype=np.float64)))), floor)


def _close(name, dev, w64, w32):
    dev, w64 = np.asarray(dev, dtype=np.float64), np.asarray(w64, dtype=np.float64)
    assert dev.shape == w64.shape, (name, dev.shape, w64.shape)
    tol = _tol(w32, w64)
    err = float(np.max(np.abs(dev - w64)))
    print("%s: device error %.3g, float32 restatement %.3g, tolerance %.3g" % (name, err, tol / 8.0, tol))
    assert err <= tol, (name, err, tol)


def _check_heads(tag, P, xin, q_mu, q_sigma):
    """The returned heads against the float64 encoder at the input the analysis feeds it (masked: m ? x : 0)."""
    mu64, s64 = O._Block(P[0:4], O._id).fwd(np.asarray(xin, dtype=np.float64))
    mu32, s32 = _head_restated(P[0:4], xin, np.float32)
    if q_mu is not None:
        _close("%s q_mu" % tag, q_mu, mu64, mu32)
    if q_sigma is not None:
        tol = max(8.0 * float(np.max(np.abs(s32.astype(np.float64) - s64) / s64)), 1e-6)
        err = float(np.max(np.abs(np.asarray(q_sigma, dtype=np.float64) - s64) / s64))
        print("%s q_sigma: relative device error %.3g, tolerance %.3g; sigma in [%.3g, %.3g]" % (tag, err, tol, float(s64.min()), float(s64.max())))
        assert err <= tol, (tag, err, tol)
        assert float(s64.min()) < 3e-6      # a unit on the floor is among them


@pytest.mark.parametrize("N,k", AN_CASES)
@pytest.mark.parametrize("nh,nl,xd", AN_SHAPES)
def test_impute_and_posterior_on_a_stressed_handle(gpu, nh, nl, xd, N, k):
    """test_gpu_impute.py's weight and imputation parity and test_gpu_posterior.py's moment parity and resampling checks."""
    m, x, P, mask = _an_net(nh, nl, xd)
    x, mask = x[:N], mask[:N]
    eps = IM.draws(N, k, nl)
    u = np.random.default_rng(500 + 10 * N + k).random((7, N)).astype(np.float32)
    r = m.impute(x, mask=mask, n_samples=k, noise=eps)
    e64 = IM.restate(P, x, mask, r["q_mu"], r["q_sigma"], eps, np.float64)
    e32 = IM.restate(P, x, mask, r["q_mu"], r["q_sigma"], eps, np.float32)
    for key in ("log_w", "log_px"):
        _close("impute " + key, r[key], e64[key], e32[key])
    al = PR.weights(r["log_w"], np.float64)
    # ess: always what the device's own log_w says it is (test_weight_parity's rtol); by the run-time rule where a float32 log_w can carry it --
    # C.ess_rounding_share: with |log_w| ~ 400 (ulp 3e-5) and two draws of nearly equal weight the output rounding of a PERFECT float32 log_w
    # alone moves ess by 4.2e-6 at (200, 100, 784), (2, 65), 40 % of the rule's floor and above the 1/8 every other admissibility condition
    # allows the inputs; test_offinit_host.py names the cases
    np.testing.assert_allclose(r["ess"], 1.0 / np.sum(al * al, axis=0), rtol=1e-6)
    share = C.ess_rounding_share(e64["log_w"], e64["ess"])
    if share <= 1.0 / 8:
        _close("impute ess", r["ess"], e64["ess"], e32["ess"])
    else:
        print("impute ess: device error %.3g, not held to the run-time rule: a correctly rounded float32 log_w alone takes %.3g of its floor"
              % (float(np.max(np.abs(r["ess"] - e64["ess"]))), share))
    want = np.sum(al[:, :, None] * e64["p"], axis=0)
    tol = _tol(e32["xhat"], e64["xhat"])
    err = float(np.max(np.abs(r["xhat"].astype(np.float64) - want)))
    print("impute xhat: device error %.3g, tolerance %.3g; largest |logit| behind it: p in [%.3g, %.3g]" % (err, tol, float(e64["p"].min()), float(e64["p"].max())))
    assert err <= tol, (err, tol)
    assert np.all(r["xhat"] >= 0.0) and np.all(r["xhat"] <= 1.0)
    _check_heads("impute", P, np.where(mask, x, 0.0), r["q_mu"], r["q_sigma"])
    p = m.posterior(x, mask=mask, n_samples=k, n_draws=7, noise=eps, uniforms=u)
    for key in ("log_w", "log_px", "ess", "q_mu", "q_sigma"):
        assert np.array_equal(p[key], r[key]), key      # (test_shared_outputs_are_imputes_bitwise)
    p64 = PR.restate(P, x, mask, p["q_mu"], p["q_sigma"], eps, np.float64)
    p32 = PR.restate(P, x, mask, p["q_mu"], p["q_sigma"], eps, np.float32)
    want = PR.moments(al, p["q_mu"], p["q_sigma"], eps, np.float64)
    for key in ("mean", "cov"):
        tol = _tol(p32[key], p64[key])
        err = float(np.max(np.abs(p[key].astype(np.float64) - want[key])))
        print("posterior %s: device error %.3g, float32 restatement %.3g, tolerance %.3g" % (key, err, tol / 8.0, tol))
        assert err <= tol, (key, err, tol)
    assert np.array_equal(p["idx"], PR.indices(p["log_w"], u))
    zw = p["q_mu"].astype(np.float64)[None] + p["q_sigma"].astype(np.float64)[None] * eps.astype(np.float64)[p["idx"], np.arange(N)[None]]
    np.testing.assert_allclose(p["z"], zw, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("objective", LQ.OBJECTIVES)
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("N,S", [(3, 7), (2, 64)])
@pytest.mark.parametrize("nh,nl,xd", AN_SHAPES)
def test_local_posterior_on_a_stressed_handle(gpu, nh, nl, xd, N, S, T, objective):
    """test_gpu_local_q.py::test_iteration_parity.  (2, 64) instead of the other analyses' (2, 65): iwae_local_posterior takes at most 64
    samples per image."""
    m, x, P, _ = _an_net(nh, nl, xd)
    x = x[:N]
    E = 2
    noise = np.random.default_rng(100 + 10 * N + S + T).standard_normal((T + E, S, N, nl)).astype(np.float32)
    r = m.local_posterior(x, n_samples=S, n_iters=T, n_eval=E, objective=objective, lr=0.05, noise=noise, trace=True)
    e64 = LQ.restate(P, x, r["q_mu"], r["q_sigma"], noise, T, objective, lr=0.05, dtype=np.float64)
    e32 = LQ.restate(P, x, r["q_mu"], r["q_sigma"], noise, T, objective, lr=0.05, dtype=np.float32)
    for key in ("grad", "bound", "mu", "sigma", "elbo", "iwae", "log_w"):
        _close("local_posterior " + key, r[key], e64[key], e32[key])
    _check_heads("local_posterior", P, x, r["q_mu"], r["q_sigma"])


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("N,Cn", AN_CASES)
@pytest.mark.parametrize("nh,nl,xd", AN_SHAPES)
def test_ais_single_transition_on_a_stressed_handle(gpu, nh, nl, xd, N, Cn, L):
    """test_gpu_ais.py::test_single_transition_parity, encoder initialisation."""
    m, x, P, _ = _an_net(nh, nl, xd)
    x = x[:N]
    betas, h = [0.3, 0.7], 0.3
    eps0, mom, unif = R.noise(100 + 10 * N + Cn + L, 1, Cn, N, nl)
    r = m.ais(x, n_chains=Cn, leapfrog=L, step_size=h, adapt=False, init="encoder", betas=betas, noise=(eps0, mom, unif), trace=True)
    mu, sg = r["q_mu"], r["q_sigma"]
    e64 = R.restate(P, x, mu, sg, betas, L, h, eps0, mom, unif, np.float64)
    e32 = R.restate(P, x, mu, sg, betas, L, h, eps0, mom, unif, np.float32)
    resolved = np.abs(e64["margin"][0]) > 1e-4
    for key in ("dH", "log_w", "z"):
        dev, w64, w32 = (np.asarray(a[key], dtype=np.float64) for a in (r, e64, e32))
        if key == "z":
            dev, w64, w32 = dev[resolved], w64[resolved], w32[resolved]
        tol = _tol(w32, w64)
        err = float(np.max(np.abs(dev - w64))) if dev.size else 0.0
        print("ais %s: device error %.3g, float32 restatement %.3g, tolerance %.3g" % (key, err, tol / 8.0, tol))
        assert err <= tol, (key, err, tol)
    assert np.array_equal(r["accepted"][0][resolved], e64["accepted"][0][resolved])
    _check_heads("ais", P, x, mu, sg)


@pytest.mark.parametrize("nh,nl,xd", AN_SHAPES)
def test_aggregate_posterior_and_latent_activity_heads_on_a_stressed_handle(gpu, nh, nl, xd):
    m, x, P, _ = _an_net(nh, nl, xd)
    eps = np.random.default_rng(3).standard_normal((2, x.shape[0], nl)).astype(np.float32)
    r = m.aggregate_posterior(x, n_samples=2, eps=eps)
    _check_heads("aggregate_posterior", P, x, r["q_mu"], r["q_sigma"])
    a = m.latent_activity(x, k=1, per_image=True)
    _check_heads("latent_activity post_mean", P, x, a["post_mean"][0], None)


def test_grid_posterior_heads_with_every_unit_sharp(gpu):
    """n_latent = 2 (the grid needs <= 4): both units are sharpened, one on the floor."""
    from iwae_amd.native import NativeModel
    nh, nl, xd = 64, 2, 48
    x, Ps, _ = IM.shape_inputs(nh, nl, xd)
    P = saturated_params(sharp_params(Ps, 1, C.SHIFTS2, (3,)), 1, *C.SAT)
    m = NativeModel(1, nh, nl, x_dim=xd, seed=C.SEED)
    m.set_params(O.flatten_params(P))
    m.set_eval_precision("fp32")
    g = np.linspace(-4.0, 4.0, 9)
    zg = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    r = m.grid_posterior(x, zg)
    _check_heads("grid_posterior", P, x, r["q_mu"], r["q_sigma"])
    m.close()
