"""Parity along the sample axis k, with importance weights that are spread over the samples.

The other GPU modules take their inputs at random initialisation, where one sample per image carries ~all of the weight over k (median
ESS/k = 1/k: tests/test_sample_axis_host.py prints it) -- the row weight G = -al / B of the iwae_elbo / iwae_eq14 / dreg steps is then one-hot
and the gradient comparison is blind to the other k - 1 samples -- and they cross none of the places where the code branches on k with a
step whose gradients are checked.  Here the SAME operations run against the SAME oracle at the SAME tolerances (tests/_parity_common.py)
on the case table of tests/_sample_axis_cases.py: spread parameters (spread_params), k on both sides of every such branch.

Two per-row checks are new, both derived (see _parity_common): log_w against the float64 sum of the device's OWN rows, and al against the
float64 softmax over k of the device's OWN log_w -- what the reductions over k do is held apart from what the bf16 operands do to the terms.

Every test prints its worst figures next to their bounds (pytest -rP shows them)."""
import numpy as np
import pytest

from oracle import iwae_np as O, philox_np
import make_golden as MG
import _sample_axis_cases as C
from _parity_common import (EMU_ROW_ATOL, EMU_SCALAR_ATOL, EMU_GRAD_REL, EXACT_SCALAR_ATOL, EXACT_GRAD_REL, F32_SCALAR_REL, F32_GRAD_REL,
                            F32_ROW_ATOL, LOGW_FROM_ROWS_ATOL, AL_RTOL, AL_ATOL, _grad_rel_errors, _elementwise_ok, _densities_at_device_head,
                            _densities_at_device_heads_2layer, al_excess, ess_fraction, softmax_over_k)

pytestmark = pytest.mark.gpu

ROWS_1L = ("lpxz", "lpz", "lqzx")
ROWS_2L = (("lpxz", "lpxz1"), ("lpz", "lpz1z2"), ("lpz2", "lpz2"), ("lqzx", "lqz1x"), ("lqzx2", "lqz2z1"))


def _model(c, precision="bf16", options=None):
    from iwae_amd.native import NativeModel
    nh, nl, xd = C.W1 if c.layers == 1 else C.W2
    return NativeModel(c.layers, nh, nl, x_dim=xd, seed=C.SEED, precision=precision, options=options)


def _report(tag, **figs):
    print("%s: %s" % (tag, ", ".join("%s %.3g" % kv for kv in figs.items())))


def _adam_ref(P, g):
    ref, _, _ = O.adam_update(O.flatten_params(P), np.asarray(g, dtype=np.float64), 0.0, 0.0, 1, 1e-3)
    return ref


def _check_sample_axis(c, r, tag):
    """The two per-row checks on the k axis and the normalisation, on the device's own outputs."""
    if c.layers == 1:
        lw = r["lpxz"].astype(np.float64) + c.beta * (r["lpz"].astype(np.float64) - r["lqzx"].astype(np.float64))      # iwae1.py:113
    else:
        lw = sum(s * r[key].astype(np.float64) for key, s in (("lpxz", 1), ("lpz", 1), ("lpz2", 1), ("lqzx", -1), ("lqzx2", -1)))      # iwae2.py:128
    d_lw = float(np.max(np.abs(r["log_w"] - lw)))
    ex = al_excess(r["al"], r["log_w"])
    d_one = float(np.max(np.abs(r["al"].astype(np.float64).sum(0) - 1.0)))
    _report("   k axis %s" % tag, log_w_from_rows=d_lw, bound=LOGW_FROM_ROWS_ATOL, al_over_bound=ex, al_bound=1.0, al_sum=d_one, sum_bound=1e-5,
            median_ess_over_k=float(np.median(ess_fraction(r["al"]))))
    assert d_lw <= LOGW_FROM_ROWS_ATOL, d_lw
    np.testing.assert_allclose(r["al"], softmax_over_k(r["log_w"]), rtol=AL_RTOL, atol=AL_ATOL)
    assert d_one <= 1e-5, d_one


def _scalar_keys(c):
    """The objective values a step reports next to its own: the DReG step beyond the few-row family reports iwae_elbo (as the row-count
    tests hold it); vae_elbo_kl needs the analytic KL, which every other step of the 1-layer model computes."""
    if c.obj == "dreg" and c.B * c.k > 1024:
        return ("iwae_elbo",)
    return ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14")


# ---------------------------------------------------------------- 1. the 1-layer bf16 step
def _bf16_step_1layer(c, options=None, tag=""):
    nl = C.W1[1]
    x, P, eps = C.inputs(c)
    res_e, g_e = C.oracle(c, True)
    res_x, g_x = C.oracle(c, False)
    m = _model(c, options=options)
    m.set_params(O.flatten_params(P))
    if c.noise == "device":
        m.set_step(C.NOISE_STEP, 0)
    dev_eps = None if c.noise == "device" else eps
    r = m.forward_backward(x, c.k, c.beta, c.obj, eps=dev_eps, want=ROWS_1L + ("log_w", "al", "z"))
    g = m.get_grads()
    assert np.all(np.isfinite(g))
    at = _densities_at_device_head(m, P, x, eps, nl)
    keys = _scalar_keys(c)
    errs_e, errs_x = _grad_rel_errors(g, g_e), _grad_rel_errors(g, g_x)
    q98 = max(float(np.quantile(np.abs(r[key] - res_e[key]), 0.98)) for key in ROWS_1L)
    _report("1-layer bf16 %s%s" % (C.case_id(c), tag), rows_at_head=max(float(np.max(np.abs(r[key] - at[key]))) for key in ROWS_1L),
            rows_q98=q98, rows_bound=EMU_ROW_ATOL, scalar_emu=max(abs(r[key] - res_e[key]) for key in keys), bound=EMU_SCALAR_ATOL,
            scalar_exact=max(abs(r[key] - res_x[key]) for key in keys), bound_x=EXACT_SCALAR_ATOL, grad_emu=max(errs_e), gbound=EMU_GRAD_REL,
            grad_exact=max(errs_x), gbound_x=EXACT_GRAD_REL)
    np.testing.assert_allclose(r["z"], res_e["z"], rtol=0, atol=1e-2)
    for key in ROWS_1L:
        assert np.max(np.abs(r[key] - at[key])) < EMU_ROW_ATOL, key                      # every row, at the device's own encoder head
        assert np.quantile(np.abs(r[key] - res_e[key]), 0.98) < EMU_ROW_ATOL, key        # the typical row against the pure oracle
        if c.noise == "device":
            assert np.max(np.abs(r[key] - res_e[key])) < 10 * EMU_ROW_ATOL, key
    _check_sample_axis(c, r, C.case_id(c))
    for key in keys:
        assert abs(r[key] - res_e[key]) < EMU_SCALAR_ATOL, (key, r[key], res_e[key])
        assert abs(r[key] - res_x[key]) < EXACT_SCALAR_ATOL, (key, r[key], res_x[key])
    if c.obj == "dreg":
        assert abs(r["inference_loss"] - res_e["inference_loss"]) < 5e-3 * abs(res_e["inference_loss"]) + 0.05
    assert max(errs_e) < EMU_GRAD_REL, errs_e
    assert max(errs_x) < EXACT_GRAD_REL, errs_x
    worst = _elementwise_ok(g, g_e)
    # the same step through iwae_train_step (Adam fused into the end of the step) gives the identical gradient and the Adam reference
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
def test_train_step_spread_weights_matches_oracle(gpu, c):
    _bf16_step_1layer(c)


@pytest.mark.parametrize("c", C.BF16_1L_QW, ids=C.case_id)
def test_train_step_spread_weights_forced_200_row_decoder(gpu, c):
    """The >= 8 192-row cases with k >= 32 once more with the 16-wave / 200-row shape of the pipelined decoder forced (bern_qw_force)."""
    _bf16_step_1layer(c, options={"bern_qw_force": 1}, tag=" bern_qw_force")


@pytest.mark.parametrize("c", C.BF16_1L_RANDOM, ids=C.case_id)
def test_train_step_one_hot_weights_matches_oracle(gpu, c):
    """Random initialisation at k > 64 and k > 256: one sample has ~all the weight -- the m = max path with exp underflow in every other lane."""
    _bf16_step_1layer(c)


@pytest.mark.parametrize("c", C.NOISE_1L, ids=C.case_id)
def test_device_noise_step_spread_weights_matches_oracle(gpu, c):
    """The device's own draws (no eps) against the oracle on their NumPy restatement: the assertions of
    test_device_noise_step_matches_oracle_on_the_same_draws, and the rest of the step's checks with them."""
    _bf16_step_1layer(c, tag=" device noise")


# ---------------------------------------------------------------- 2. float32 mode
def _float32_step(c, logits, options=None):
    layers = c.layers
    x, P, eps = C.inputs(c)
    res, g = C.oracle(c, False)
    if layers == 1:
        rows = tuple((key, key) for key in ROWS_1L)
        keys = ("iwae_elbo",) if c.obj == "dreg" else ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14")
    else:
        rows, keys = ROWS_2L, ("vae_elbo", "iwae_elbo", "iwae_eq14")
    m = _model(c, precision="fp32", options=options)
    m.set_params(O.flatten_params(P))
    r = m.forward_backward(x, c.k, c.beta, c.obj, eps=eps, want=tuple(a for a, _ in rows) + ("al", "z", "log_w") + (("logits",) if logits else ()))
    flat = m.get_grads()
    errs = _grad_rel_errors(flat, g)
    _report("float32 %s%s%s" % (C.case_id(c), "" if logits else " no logits", " %s" % (options,) if options else ""),
            rows=max(float(np.max(np.abs(r[a] - res[b]))) for a, b in rows), rows_bound=F32_ROW_ATOL,
            scalar_rel=max(abs(r[key] - res[key]) / (abs(res[key]) + 20.0) for key in keys), bound=F32_SCALAR_REL, grad=max(errs), gbound=F32_GRAD_REL)
    for a, b in rows:
        assert np.max(np.abs(r[a] - res[b])) < F32_ROW_ATOL, (a, float(np.max(np.abs(r[a] - res[b]))))
    np.testing.assert_allclose(r["z"], res["z"] if layers == 1 else res["z1"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(r["al"], res["al"], atol=2e-4)
    _check_sample_axis(c, r, C.case_id(c))
    for key in keys:
        assert abs(r[key] - res[key]) <= F32_SCALAR_REL * abs(res[key]) + 2e-4, (key, r[key], res[key])
    assert max(errs) < F32_GRAD_REL, errs
    # the forward-only call and the fused train step agree with the two-call path; Keras Adam from the device gradient
    # (without `logits` and from 4 096 rows the forward-only call is the one-launch decoder, dec_fwd_f32_kernel: its rows against the oracle too)
    r0 = m.forward(x, c.k, c.beta, eps=eps, want=("lpxz", "log_w", "al"))
    for key in keys:
        assert abs(r0[key] - r[key]) <= 1e-6 * abs(r[key]) + 1e-5
    d_fwd = float(np.max(np.abs(r0["lpxz"] - res["lpxz" if layers == 1 else "lpxz1"])))
    _report("   forward only", lpxz=d_fwd, rows_bound=F32_ROW_ATOL, al_over_bound=al_excess(r0["al"], r0["log_w"]), al_bound=1.0)
    assert d_fwd < F32_ROW_ATOL, d_fwd
    np.testing.assert_allclose(r0["al"], softmax_over_k(r0["log_w"]), rtol=AL_RTOL, atol=AL_ATOL)
    m.train_step(x, c.k, c.beta, 1e-3, c.obj, eps=eps)
    g2 = m.get_grads().astype(np.float64)
    assert np.linalg.norm(g2 - flat) / np.linalg.norm(flat) < 1e-5
    d_adam = float(np.max(np.abs(m.get_params() - _adam_ref(P, flat))))
    _report("   Adam", d=d_adam, bound=2e-6)
    assert d_adam < 2e-6
    m.close()


@pytest.mark.parametrize("c", C.F32_1L, ids=C.case_id)
def test_float32_step_spread_weights_matches_exact_oracle(gpu, c):
    """(1200, 7) runs without `logits`: the training step's output layer takes its fused epilogue, and the forward-only call inside
    _float32_step takes the one-launch float32 decoder, whose 16-row tiles hold 3 or 4 images each at k = 7."""
    _float32_step(c, logits=c.B * c.k < 8000)


def test_float32_step_one_launch_decoder_in_the_training_step(gpu):
    """(1200, 7) once more with option f32_dec_fused_train: the TRAINING step's decoder forward is dec_fwd_f32_kernel too (by default
    a training step takes three GEMM launches), so g1, g2 and s = x - sigmoid(l) of tiles on both sides of `x_in_lds` reach the gradients."""
    _float32_step(C.F32_1L[-1], logits=False, options={"f32_dec_fused_train": 1})


# ---------------------------------------------------------------- 3. the 2-layer model
@pytest.mark.parametrize("c", C.L2_BOTH + C.L2_BF16_ONLY, ids=C.case_id)
def test_train_step_2layer_spread_weights_matches_oracle(gpu, c):
    """The assertions and bounds of test_gpu_ragged_widths.py::test_train_step_2layer_matches_oracle for the same row-count class (its
    docstring explains them), plus the two checks on the k axis with log_w recomputed from the five device rows."""
    nl = C.W2[1]
    B, k = c.B, c.k
    x, P, eps = C.inputs(c)
    res_e, g_e = C.oracle(c, True)
    res_x, g_x = C.oracle(c, False)
    m = _model(c)
    m.set_params(O.flatten_params(P))
    r = m.forward_backward(x, k, 1.0, c.obj, eps=eps, want=("z", "z2", "al", "log_w", "lpxz", "lpz", "lqzx", "lpz2", "lqzx2"))
    g = m.get_grads()
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
    _check_sample_axis(c, r, C.case_id(c))
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


@pytest.mark.parametrize("c", C.L2_BOTH, ids=C.case_id)
def test_float32_step_2layer_spread_weights_matches_exact_oracle(gpu, c):
    _float32_step(c, logits=True)


# ---------------------------------------------------------------- 4. the multi-step noise buffers of the few-row step
# A 1-layer bf16 training step on few rows (dec_rows_step, step_bf16.hip) on the device's own noise takes its draws from two buffers that hold
# EPSM_STEPS = 8 consecutive steps each (plan_step: eps_multi; draw_eps_multi / epsm_find): one launch per 8 steps.  Option no_eps_multi
# draws every step on its own.  Both must see the same numbers: Philox is keyed by (seed, step, row), not by the launch.
EPSM_B, EPSM_K, EPSM_S0 = 20, 5, 41


def _epsm_inputs():
    nh, nl, xd = C.W1
    x, P, _ = MG.inputs(1, nh, nl, xd, EPSM_B, 1, 811)
    return x, P


def test_multi_step_noise_buffers_are_bitwise_the_per_step_draws(gpu):
    """20 consecutive train steps from iwae_set_step(41) on a default handle and on one with no_eps_multi: parameters and Adam state
    bitwise equal after EVERY call.  Read off forward_impl (step_bf16.hip): calls 0-2 take steps 41-43 from the group [41, 49) drawn at the
    first call; before call 3 iwae_set_step jumps into the middle of that group (step 46 = slot 5, no multiple of 8: a hit); step 48, the
    group's last, draws [49, 57) into the other buffer (a hand-over); call 12 runs at B = 12 (step 55, another batch shape: a miss that
    redraws the first buffer); call 13 returns to B = 20 at step 56 and hits slot 7 of the buffer the B = 12 call left alone, then hands
    over again; before call 16 iwae_set_step jumps far ahead to step 1 003 (a miss)."""
    x, P = _epsm_inputs()
    from iwae_amd.native import NativeModel
    nh, nl, xd = C.W1
    ms = [NativeModel(1, nh, nl, x_dim=xd, seed=C.SEED, options=opts) for opts in (None, {"no_eps_multi": 1})]
    for m in ms:
        m.set_params(O.flatten_params(P))
        m.set_step(EPSM_S0, 0)
    worst = 0.0
    for call in range(20):
        if call == 3:
            for m in ms:
                m.set_step(EPSM_S0 + 5, 0)
        if call == 16:
            for m in ms:
                m.set_step(1003, 0)
        xb = x[:12] if call == 12 else x
        out = []
        for m in ms:
            r = m.train_step(xb, EPSM_K, 1.0, 1e-3, "iwae_elbo")
            out.append((r["iwae_elbo"], m.get_params(), m.get_adam_state()))
        (la, pa, (ma, va, ta)), (lb, pb, (mb, vb, tb)) = out
        worst = max(worst, float(np.max(np.abs(pa - pb))))
        assert la == lb, (call, la, lb)
        assert ta == tb == call + 1
        for a, b, name in ((pa, pb, "parameters"), (ma, mb, "Adam m"), (va, vb, "Adam v")):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (call, name, float(np.max(np.abs(a - b))))
    _report("multi-step noise buffers vs per-step draws, 20 steps", max_param_difference=worst, bound=0.0)
    for m in ms:
        m.close()


def test_multi_step_noise_buffer_slot_holds_that_steps_draws(gpu):
    """Three train steps into a fresh group (steps 41, 42, 43: every iwae_train_step / iwae_forward_backward call ends with noise_step += 1,
    model.hip), then iwae_forward_backward at step 44 reads slot 3 of the group drawn at step 41: its z must be mu + sigma * the Philox
    draws OF STEP 44, mu and sigma the device's own encoder head.  float32 against float64 on the fast v_log / v_sin / v_cos draws
    (<= 2e-5 each, sigma ~ 1): 1e-4; a wrong slot or stride gives independent normals, differences of order 1."""
    x, P = _epsm_inputs()
    from iwae_amd.native import NativeModel
    nh, nl, xd = C.W1
    m = NativeModel(1, nh, nl, x_dim=xd, seed=C.SEED)
    m.set_params(O.flatten_params(P))
    m.set_step(EPSM_S0, 0)
    for _ in range(3):
        m.train_step(x, EPSM_K, 1.0, 1e-3, "iwae_elbo", scalars=False)
    r = m.forward_backward(x, EPSM_K, 1.0, "iwae_elbo", want=("z",))
    head = m.debug_tensor("enc.head").astype(np.float64)
    Dp = head.shape[1] // 2
    mu, sig = head[:EPSM_B, :nl], head[:EPSM_B, Dp:Dp + nl]
    d = {}
    for s in range(EPSM_S0, EPSM_S0 + 8):
        e = philox_np.device_eps(C.SEED, s, EPSM_B, EPSM_K, nl)
        d[s] = float(np.max(np.abs(r["z"] - (mu[None] + sig[None] * e))))
    _report("multi-step noise buffers, slot 3", z_vs_its_own_step=d[EPSM_S0 + 3], bound=1e-4, z_vs_nearest_other_step=min(v for s, v in d.items() if s != EPSM_S0 + 3))
    assert d[EPSM_S0 + 3] <= 1e-4, d
    m.close()
