"""Admissibility of the off-initialisation cases (tests/_offinit_cases.py) from the oracle alone -- no GPU -- and the negative controls
that show what the cases see.

The conditions are on the INPUTS, not measurements of the device:
  * a sharp case in bf16: per gradient tensor the rounding-aware oracle differs from the exact oracle by <= EMU_GRAD_REL and per row by
    <= half the bound the GPU test holds that row to against the rounding-aware oracle -- EMU_ROW_ATOL / 2, except the rows the existing
    bodies already hold to a wider bound because they divide by the sigma^2 of a head behind bf16 GEMMs: the 2-layer model's four latent
    rows (0.05) and the conditional prior's log p(z|y) (0.2) (the device is held to those bounds against the rounding-aware oracle; an
    input on which one bf16 rounding moves the result by more says nothing about a kernel); median ESS/k >= 0.10 (k > 1); on every image (row, for q(z2|z1)) of every sharpened
    head one sharpened unit has exp(a) <= 2e-6 (the floor is at least a third of sigma) and one has exp(a) in [5e-5, 2e-4] (the floor is
    ~1 % of sigma: a relative error the gradient bound sees, on a unit that still has a width);
  * a float32-mode case: the oracle with every OPERAND rounded to float32 differs from the exact oracle by <= 1/8 of the bound the GPU
    test uses -- rows, scalars, per-tensor gradient.  This proxy rounds operands only, not accumulations: it shows that the inputs do not
    amplify a float32 rounding, not what the device's float32 sums do;
  * a saturated case: max |logit| >= 15, >= 5 % of the decoder's second tanh layer at |y| >= 0.999, mean |log p(x|z)| <= 1 000 (so that
    F32_ROW_ATOL stays above 30 float32 ulps of a row).

Negative controls: three mutants of the oracle, patched in and restored inside the test --
  (a) the floor absent from the forward sigma (sigma = exp(a));
  (b) the derivative through exp taken as da = dsigma * sigma instead of dsigma * exp(a);
  (c) DReG with one floor instead of two (sig2 = sigma) -- DReG cases only.
On every sharp case each applicable mutant moves at least one quantity the GPU test compares (the objective values, DReG's inference
loss, a gradient tensor) by more than 3x that comparison's bound, and at the SAME case's spread parameters it moves every one of them by
less than a tenth of the bound: the evidence that the sharp cases see what no other parity case can.  All three are visible, (c)
through the encoder's gradient (120 .. 250 x EMU_GRAD_REL; DReG's inference loss itself moves by less than its bound).

Every test prints its figures next to their bounds (pytest -rP shows them)."""
import contextlib

import numpy as np
import pytest

from oracle import iwae_np as O
import _offinit_cases as C
from _parity_common import (EMU_GRAD_REL, EMU_ROW_ATOL, EMU_SCALAR_ATOL, F32_GRAD_REL, F32_ROW_ATOL, F32_SCALAR_REL, ess_fraction,
                            sharp_params, sharp_units, saturated_params)

ESS_MIN = 0.10
ON_FLOOR, NEAR_FLOOR = 2e-6, (5e-5, 2e-4)


def _rel(g_a, g_b):
    return [float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)) for pa, pb in zip(g_a, g_b) for a, b in zip(pa, pb)]


def _rows(c):
    return ("lpxz", "lpz", "lqzx") if c.layers == 1 else ("lpxz1", "lpz1z2", "lpz2", "lqz1x", "lqz2z1")


def _row_bound(c, key):
    """The bound the GPU test holds a row to against the rounding-aware oracle (test_conditional_prior_model_matches_oracle: 0.2 on lpz;
    test_train_step_2layer_matches_oracle and its large-row class: 0.05 on the latent rows -- 0.4 on lpz1z2 at few rows is not used here)."""
    if c.cond and key == "lpz":
        return 0.2
    if c.layers == 2 and key != "lpxz1":
        return 0.05
    return EMU_ROW_ATOL


def _f32_scalar_bound(v):
    return F32_SCALAR_REL * abs(v) + 2e-4      # the float32 bodies' check of an objective value


# ---------------------------------------------------------------- the constructors
def test_constructors_touch_only_what_they_name():
    x, P, eps = C.MG.inputs(2, [16, 8], [5, 3], 48, 2, 2, 1)
    S = sharp_params(P, 2, C.SHIFTS2, (3, 7))
    for i, ((W, b), (Ws, bs)) in enumerate(zip(P, S)):
        assert Ws.dtype == bs.dtype == np.float64 and Ws is not W and bs is not b
        np.testing.assert_array_equal(W, Ws)
        d = b - bs
        if i in (3, 7):
            assert sorted(np.nonzero(d)[0]) == [0, b.size - 1] and np.allclose(d[[0, b.size - 1]], C.SHIFTS2)
        else:
            assert not d.any()
    assert sharp_units(100, 4) == [0, 33, 66, 99] and sharp_units(5, 4) == [0, 1, 3, 4] and sharp_units(2, 2) == [0, 1]
    for bad in ((11,), (2,), (3, 11)):
        with pytest.raises(ValueError):
            sharp_params(P, 2, C.SHIFTS2, bad)
    with pytest.raises(ValueError):
        sharp_params(P[:7], 1, C.SHIFTS2, (7,))
    with pytest.raises(ValueError):
        sharp_params(P, 2, C.SHIFTS4, (7,))      # four units do not fit a head of width 3
    T = saturated_params(P, 2, 10.0, 3.0)
    for i, ((W, b), (Wt, bt)) in enumerate(zip(P, T)):
        np.testing.assert_array_equal(b, bt)
        np.testing.assert_allclose(Wt, W * (10.0 if i == 14 else 3.0 if i in (0, 1, 4, 5, 8, 9, 12, 13) else 1.0), rtol=1e-15)
    T1 = saturated_params(P[:7], 1, 10.0, 3.0)
    for i, ((W, b), (Wt, bt)) in enumerate(zip(P[:7], T1)):
        np.testing.assert_allclose(Wt, W * (10.0 if i == 6 else 3.0 if i in (0, 1, 4, 5) else 1.0), rtol=1e-15)


# ---------------------------------------------------------------- admissibility
@pytest.mark.parametrize("c", list(dict.fromkeys(C.SHARP_BF16)), ids=C.case_id)
def test_sharp_case_is_admissible_in_bf16(c):
    res_x, g_x = C.oracle(c, "exact")
    res_e, g_e = C.oracle(c, "emu")
    ess = float(np.median(ess_fraction(res_x["al"])))
    cond = max(_rel(g_e, g_x))
    rows = max(float(np.max(np.abs(res_e[key] - res_x[key]))) * (EMU_ROW_ATOL / _row_bound(c, key)) for key in _rows(c))
    units = sharp_units(c.widths[1] if c.layers == 1 else c.widths[1][0], c.sharp)
    on, near = [], []
    for h in c.heads:
        ea = np.exp(res_x["a"][h].reshape(-1, res_x["a"][h].shape[-1]))[:, sharp_units(res_x["a"][h].shape[-1], c.sharp)]
        on.append(float(np.max(np.min(ea, axis=1))))      # over images: the smallest sharpened exp(a) of the image
        near.append(bool(np.all(np.any((ea >= NEAR_FLOOR[0]) & (ea <= NEAR_FLOOR[1]), axis=1))))
    print("%s: median ESS/k %.3g (>= %.2f), rounding-aware vs exact rows, scaled to EMU_ROW_ATOL by each row's bound, %.3g (<= %.3g), gradient %.3g (<= %.3g), smallest exp(a) per image <= %.3g "
          "(<= %.1g), a unit in [%.0e, %.0e] on every image: %s" % (C.case_id(c), ess, ESS_MIN, rows, EMU_ROW_ATOL / 2, cond, EMU_GRAD_REL, max(on), ON_FLOOR,
                                                                    NEAR_FLOOR[0], NEAR_FLOOR[1], all(near)))
    assert units[-1] == (c.widths[1] if c.layers == 1 else c.widths[1][0]) - 1
    if c.k > 1:
        assert ess >= ESS_MIN, ess
    assert rows <= EMU_ROW_ATOL / 2, rows
    assert cond <= EMU_GRAD_REL, _rel(g_e, g_x)
    assert max(on) <= ON_FLOOR and all(near), (on, near)


@pytest.mark.parametrize("c", C.F32, ids=C.case_id)
def test_float32_case_is_admissible(c):
    res_x, g_x = C.oracle(c, "exact")
    res_f, g_f = C.oracle(c, "f32")
    rows = max(float(np.max(np.abs(res_f[key] - res_x[key]))) for key in _rows(c))
    scal = max(abs(res_f[key] - res_x[key]) / _f32_scalar_bound(res_x[key]) for key in C.scalar_keys(c))
    cond = max(_rel(g_f, g_x))
    mean_lpxz = float(np.mean(np.abs(res_x[C.lpxz_key(c)])))
    print("%s: float32-operand vs exact rows %.3g (<= %.3g), scalars %.3g x their bound (<= 0.125), gradient %.3g (<= %.3g); max |logit| %.3g, "
          "decoder layer 2 at |y| >= 0.999: %.3g, mean |lpxz| %.4g" % (C.case_id(c), rows, F32_ROW_ATOL / 8, scal, cond, F32_GRAD_REL / 8,
                                                                     res_x["max_logit"], res_x["sat_frac"], mean_lpxz))
    assert rows <= F32_ROW_ATOL / 8, rows
    assert scal <= 1.0 / 8, scal
    assert cond <= F32_GRAD_REL / 8, _rel(g_f, g_x)
    if c.sat:
        assert res_x["max_logit"] >= 15.0, res_x["max_logit"]
        assert res_x["sat_frac"] >= 0.05, res_x["sat_frac"]
        assert mean_lpxz <= 1000.0, mean_lpxz


def test_clean_saturation_inputs_overflow_the_fast_forms():
    """(v): the inputs reach e^{2|x|} = inf in both first layers and e^{|l|} = inf in the output layer, and the float32-operand oracle's rows
    stay within 1/8 of the GPU test's bound max(F32_ROW_ATOL, F32_SCALAR_REL |row|) of the exact oracle's."""
    x, P, eps, fig = C.clean_saturation_inputs()
    res_x = O.forward_1layer(P, x, eps)
    res_f = O.forward_1layer(P, x, eps, rnd=C.f32_round)
    worst = max(float(np.max(np.abs(res_f[key] - res_x[key]) / np.maximum(F32_ROW_ATOL, F32_SCALAR_REL * np.abs(res_x[key])))) for key in ("lpxz", "lpz", "lqzx"))
    print("clean saturation: max |pre-activation| encoder %.3g, decoder %.3g (> 45), max |logit| %.3g (> 90), mean lpxz %.4g, float32-operand vs exact "
          "rows %.3g x their bound (<= 0.125)" % (fig["enc_pre"], fig["dec_pre"], fig["logit"], float(np.mean(res_x["lpxz"])), worst))
    assert fig["enc_pre"] > 45.0 and fig["dec_pre"] > 45.0 and fig["logit"] > 90.0, fig
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(np.float32(2.0 * 45.0))) and np.isinf(np.exp(np.float32(90.0)))
    assert worst <= 1.0 / 8, worst


@pytest.mark.parametrize("c,precs", C.EVAL, ids=lambda v: C.case_id(v) if isinstance(v, C.Case) else "+".join(v))
def test_eval_llh_case_is_admissible(c, precs):
    """(vi): per image, the rounding-aware (float32-operand) oracle's log-mean-exp over k on the restated device draws is within half (an
    eighth) of the bound the GPU test holds the bf16 (float32) evaluator to."""
    from oracle import philox_np
    x, _, P, _, _ = C.inputs(c)
    worst = {}
    for i in range(c.B):
        e = philox_np.device_eps(C.SEED, C.EVAL_STEP, 1, c.k, c.widths[1], batch_offset=i)
        ref = float(O.forward_1layer(P, x[i:i + 1], e)["iwae_elbo"])
        for mode in ("f32",) + (("emu",) if "bf16" in precs else ()):
            worst[mode] = max(worst.get(mode, 0.0), abs(float(O.forward_1layer(P, x[i:i + 1], e, rnd=C.RND[mode])["iwae_elbo"]) - ref))
    print("%s: float32-operand vs exact per-image LLH %.3g (<= %.3g)%s" % (C.case_id(c), worst["f32"], 5e-3 / 8,
                                                                            ", rounding-aware %.3g (<= 0.05)" % worst["emu"] if "emu" in worst else ""))
    assert worst["f32"] <= 5e-3 / 8
    assert worst.get("emu", 0.0) <= 0.1 / 2


def test_ess_of_the_stressed_analysis_handle_by_the_run_time_rule():
    """(vii): test_gpu_offinit.py holds iwae_impute's ess to the analyses' run-time rule (8 x the float32 restatement's deviation, floor 1e-5)
    only where the output rounding of a perfect float32 log_w leaves it room -- at most 1/8 of the floor, the share every other condition
    of this module allows the inputs.  Heads: the float64 encoder's, rounded to float32 as the device returns them.  (64, 8, 48): 0.033 and
    0.013 of the floor; (200, 100, 784): 0.025 at (3, 7) and 0.42 at (2, 65), where |log_w| ~ 390 (ulp 3e-5) and one image has two draws of
    nearly equal weight (ess 2.02): that one is held to its own log_w only."""
    import _impute_ref as IM
    got = {}
    for nh, nl, xd in ((64, 8, 48), (200, 100, 784)):
        x, Ps, mask = IM.shape_inputs(nh, nl, xd)
        P = saturated_params(sharp_params(Ps, 1, C.SHIFTS2, (3,)), 1, *C.SAT)
        for N, k in ((3, 7), (2, 65)):
            mu, sg = IM.encoder_heads(P, x[:N], mask[:N])
            e64 = IM.restate(P, x[:N], mask[:N], mu.astype(np.float32), sg.astype(np.float32), IM.draws(N, k, nl), np.float64)
            got[(nh, N, k)] = C.ess_rounding_share(e64["log_w"], e64["ess"])
            print("stressed handle %d/%d/%d N = %d, k = %d: ess %s, a rounded log_w moves it by %.3g of the floor (<= 0.125 for the run-time rule), "
                  "max |log_w| %.4g" % (nh, nl, xd, N, k, np.round(e64["ess"], 3), got[(nh, N, k)], float(np.max(np.abs(e64["log_w"])))))
    assert sorted(key for key, v in got.items() if v > 1.0 / 8) == [(200, 2, 65)], got


# ---------------------------------------------------------------- negative controls
@contextlib.contextmanager
def _mutant(which):
    """The oracle with one defect, restored on exit."""
    fwd, bwd, floor = O._Block.fwd, O._Block.bwd, O.SIGMA_EPS

    def fwd_no_floor(self, x_r):
        fwd(self, x_r)
        self.sigma = np.exp(self.a)
        return self.mu, self.sigma

    def bwd_through_sigma(self, dmu, dsigma, need_dx=True):
        da = dsigma * self.sigma
        dh2 = self.lmu.bwd(dmu) + self.lstd.bwd(da)
        return self.l1.bwd(self.l2.bwd(dh2), need_dx=need_dx)

    def fwd_own_floor(self, x_r):
        fwd(self, x_r)
        self.sigma = np.exp(self.a) + floor      # the head keeps its floor while the module constant, which DReG's second floor reads, is 0
        return self.mu, self.sigma
    try:
        if which == "a":
            O._Block.fwd = fwd_no_floor
        elif which == "b":
            O._Block.bwd = bwd_through_sigma
        else:
            O._Block.fwd, O.SIGMA_EPS = fwd_own_floor, 0.0
        yield
    finally:
        O._Block.fwd, O._Block.bwd, O.SIGMA_EPS = fwd, bwd, floor


def _shift_over_bounds(c, P, which, f32):
    """The largest move, in units of the GPU test's bound, of a quantity the test compares: every objective value it checks, DReG's
    inference loss, every gradient tensor.  Exact oracle with and without the mutation."""
    res, g = C.run_oracle(c, P, "exact")
    with _mutant(which):
        res_m, g_m = C.run_oracle(c, P, "exact")
    out = {}
    for key in C.scalar_keys(c):
        out[key] = abs(res_m[key] - res[key]) / (_f32_scalar_bound(res[key]) if f32 else EMU_SCALAR_ATOL)
    if c.obj == "dreg":
        v = res["inference_loss"]
        out["inference_loss"] = abs(res_m["inference_loss"] - v) / ((1e-4 * abs(v) + 1e-4) if f32 else (5e-3 * abs(v) + 0.05))
    out["gradient"] = max(_rel(g_m, g)) / (F32_GRAD_REL if f32 else EMU_GRAD_REL)
    return out


CONTROL = [(c, False) for c in dict.fromkeys(C.SHARP_BF16)] + [(c, True) for c in C.F32 if c.sharp and c not in C.SHARP_BF16]
CONTROL = list(dict.fromkeys(CONTROL))


def _control_id(v):
    return C.case_id(v) if isinstance(v, C.Case) else v if isinstance(v, str) else ("f32" if v else "bf16")


@pytest.mark.parametrize("c,f32,which", [(c, f32, w) for c, f32 in CONTROL for w in ("a", "b") + (("c",) if c.obj == "dreg" else ())], ids=_control_id)
def test_control_mutant_is_seen_at_sharp_and_not_at_spread(c, f32, which):
    """Bounds: the bf16 tests' (EMU_SCALAR_ATOL, EMU_GRAD_REL, DReG's inference-loss bound) for a bf16 case, float32 mode's for a
    float32-only case.  "Spread parameters of the same case": the case without sharp_params (a saturated case keeps its saturation)."""
    x, Ps, P, eps, y = C.inputs(c)
    sharp = _shift_over_bounds(c, P, which, f32)
    spread = _shift_over_bounds(c, C.stress(c._replace(sharp=0), Ps), which, f32)
    print("%s %s mutant (%s): sharp %s; spread %s   [x the bound; sharp needs one > 3, spread all < 0.1]"
          % (C.case_id(c), "float32" if f32 else "bf16", which, ", ".join("%s %.3g" % kv for kv in sharp.items()),
             ", ".join("%s %.3g" % kv for kv in spread.items())))
    assert max(sharp.values()) > 3.0, sharp
    assert max(spread.values()) < 0.1, spread
