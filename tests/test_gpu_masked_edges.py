"""The masked float32 train step where tests/test_gpu_masked_step.py does not reach (case table: tests/_masked_cases.py; admissibility from
the oracle alone: tests/test_masked_edges_host.py):
  1. the route witness: every call's launch count of masked_out_f32_kernel (iwae_kernel_time "masked_out") against the route the test names;
     three shapes masked_out_f32_ok refuses are forced "fast" and must show 0 launches at full parity;
  2. fast-route shapes with an H the float4 strip load cannot take, a cut last pixel tile, TP of 7, 9, 12, 4 and 1, a pass at t0 & 3 == 0 that
     is not the first, K splits of 2 and 3 chunks at H not a multiple of 16, and the KSPLIT = false instantiation at few rows (f32_no_ksplit);
  3. row counts between 130 and 4 100 at 200 / 100 / 784: kslabs 5 and 7, and no split below 4 096 rows;
  4. the two routes bit for bit at every (shape, case) of 2 and 3;
  5. mask structures: columns no image observes (exact zeros in the gradient, whatever x holds there), dead tiles and passes, a batch of
     empty images, MCAR at 0.95 and 0.05, and raw mask bytes 2 / 0x80 / 255 through the raw binding;
  6. parameters off the initialisation under a mask (sharp, saturated, wide; the clean-saturation inputs);
  7. state across calls: a three-step trajectory at 4 100 rows (side-stream weight gradients, deferred decoder update) against the
     reference at the device's own parameters and float64 Adam, masked and unmasked calls alternated on one handle with B and k changing,
     device-resident x and mask (the mask also at an odd byte address).

The reference is tests/_masked_ref.py (masked_loss_grads).  Tolerances are float32 mode's own (tests/_parity_common.py), used as
test_gpu_masked_step.py's _check_parity and test_float32_step_off_init_matches_exact_oracle use them; route against route: bitwise in 4,
2e-6 / 1e-5 elsewhere; Adam from the device gradient 2e-6.  One handle per (shape, route) for the whole module; every test resets what it
reads.  Every test prints its worst figures next to their bounds (pytest -rP shows them).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import iwae_np as O
import _masked_cases as MC
import _masked_ref as MR
import _offinit_cases as OC
from _parity_common import F32_SCALAR_REL, F32_GRAD_REL, F32_ROW_ATOL, _grad_rel_errors

pytestmark = pytest.mark.gpu

SCALARS = ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14")
ROWS = ("lpxz", "lpz", "lqzx", "log_w", "al", "z")
_handles = {}


def _sid(v):
    return v if isinstance(v, str) else "%d_%d_%d" % v if len(v) == 3 else "B%d_k%d" % v


def _model(shape, route):
    """The module's handle of a shape on a route (MC.ROUTES; "default": no option): float32, 1-layer."""
    if (shape, route) not in _handles:
        from iwae_amd.native import NativeModel
        nh, nl, xd = shape
        _handles[(shape, route)] = NativeModel(1, nh, nl, x_dim=xd, seed=123, precision="fp32", options=MC.ROUTES.get(route, {}))
    return _handles[(shape, route)]


def _reset(m, P):
    m.set_params(O.flatten_params(P))
    m.set_adam_state(np.zeros(m.n_params, np.float32), np.zeros(m.n_params, np.float32), 0)
    m.set_step(0, 0)


def _report(tag, **figs):
    print("%s: %s" % (tag, ", ".join("%s %.3g" % kv for kv in figs.items())))


def _scalar_bound(v):
    return F32_SCALAR_REL * abs(v) + 2e-4


def _witnessed(m, route, rows, call):
    """call() with the launch count of masked_out_f32_kernel held to the route's expectation."""
    out, launches = MR.masked_out_launches(m, call)
    MR.expected_on_fast_route(route, launches, rows)
    return out


def _run(shape, case, route, obj, beta=1.0, structure="case"):
    """(result dict, flat gradient) of iwae_forward_backward_masked, once per (shape, case, route, objective, beta, mask structure); the
    witness is checked on every call."""
    return _run_once(shape, case, route, obj, float(beta), structure)


@functools.lru_cache(maxsize=None)
def _run_once(shape, case, route, obj, beta, structure):
    x, P, eps, mask = MC.struct_case(shape, case, structure)
    m = _model(shape, route)
    _reset(m, P)
    r = _witnessed(m, route, case[0] * case[1], lambda: m.forward_backward(x, case[1], beta, obj, eps=eps, want=ROWS, mask=mask))
    return r, m.get_grads().copy()


def _parity(r, flat, res, g, mask, obj, beta=1.0):
    """test_gpu_masked_step.py's _check_parity on given results; returns the figures (rows, scalars over their bound, gradient)."""
    rows = max(float(np.max(np.abs(r[a] - res[a]))) for a in ("lpxz", "lpz", "lqzx", "log_w"))
    keys = ("iwae_elbo",) if obj == "dreg" else SCALARS
    scal = max(abs(r[key] - res[key]) / _scalar_bound(res[key]) for key in keys)
    scal = max(scal, abs(r["mean_lpxz"] - res["lpxz"].mean()) / _scalar_bound(res["lpxz"].mean()))
    errs = _grad_rel_errors(flat, g)
    figs = dict(rows=rows, rows_bound=F32_ROW_ATOL, scalars_over_bound=scal, grad=max(errs), gbound=F32_GRAD_REL)
    for a in ("lpxz", "lpz", "lqzx", "log_w"):
        assert np.max(np.abs(r[a] - res[a])) < F32_ROW_ATOL, (a, float(np.max(np.abs(r[a] - res[a]))))
    np.testing.assert_allclose(r["z"], res["z"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(r["al"], res["al"], atol=2e-4)
    for key in keys:
        assert np.isfinite(r[key]) and abs(r[key] - res[key]) <= _scalar_bound(res[key]), (key, r[key], res[key])
    assert abs(r["mean_lpxz"] - res["lpxz"].mean()) <= _scalar_bound(res["lpxz"].mean()), (r["mean_lpxz"], res["lpxz"].mean())
    assert np.all(np.isfinite(flat))
    assert max(errs) < F32_GRAD_REL, errs
    # an image with nothing observed: log p(x_obs|z) = 0 exactly, log_w = log p(z) - log q(z|x) (at most three float32 roundings of terms of that size)
    for b in np.flatnonzero(mask.sum(axis=1) == 0):
        assert np.all(r["lpxz"][:, b] == 0.0)
        d = (r["lpz"][:, b].astype(np.float64) - r["lqzx"][:, b].astype(np.float64)) * beta
        ulp = 2.0 ** -23 * max(1.0, float(np.max(np.abs(r["lpz"][:, b]))), float(np.max(np.abs(r["lqzx"][:, b]))))
        assert np.max(np.abs(r["log_w"][:, b] - d)) <= 4 * ulp
    return figs


def _worst(acc, figs):
    for key, v in figs.items():
        acc[key] = max(acc.get(key, 0.0), v)


def _check(shape, case, route, obj, beta=1.0, structure="case"):
    x, P, eps, mask = MC.struct_case(shape, case, structure)
    res, g = MC.struct_reference(shape, case, structure, obj, beta)
    r, flat = _run(shape, case, route, obj, beta, structure)
    return _parity(r, flat, res, g, mask, obj, beta)


def _forward_and_train_agree(shape, case, route, obj, structure="case"):
    """The tail of test_masked_step_matches_the_restatement: the forward-only call agrees with the training call; iwae_train_step_masked =
    Keras Adam of the device gradient.  Both under the witness."""
    x, P, eps, mask = MC.struct_case(shape, case, structure)
    r, flat = _run(shape, case, route, obj, 1.0, structure)
    m = _model(shape, route)
    _reset(m, P)
    rows = case[0] * case[1]
    r0 = _witnessed(m, route, rows, lambda: m.forward(x, case[1], 1.0, eps=eps, want=("lpxz",), mask=mask))
    np.testing.assert_allclose(r0["lpxz"], r["lpxz"], rtol=1e-6, atol=1e-4)
    assert abs(r0["iwae_elbo"] - r["iwae_elbo"]) <= 1e-6 * abs(r["iwae_elbo"]) + 1e-5
    _witnessed(m, route, rows, lambda: m.train_step(x, case[1], 1.0, 1e-3, obj, eps=eps, mask=mask))
    g2 = m.get_grads().astype(np.float64)
    assert np.linalg.norm(g2 - flat) / max(np.linalg.norm(flat), 1e-30) < 1e-5
    ref, _, _ = O.adam_update(O.flatten_params(P), flat.astype(np.float64), 0.0, 0.0, 1, 1e-3)
    d = float(np.max(np.abs(m.get_params() - ref)))
    assert d < 2e-6, d
    return d


# ---------------------------------------------------------------- 1. shapes the fast route refuses, forced "fast"
@pytest.mark.parametrize("case", MC.EDGE_CASES, ids=_sid)
@pytest.mark.parametrize("shape", MC.FALLBACK_DIMS, ids=_sid)
def test_refused_shape_forced_fast_runs_the_general_route(gpu, shape, case):
    """masked_out_min_rows = 1 on a shape masked_out_f32_ok refuses (X % 4 == 1; W3 misaligned; H > 208): 0 launches of
    masked_out_f32_kernel on every call, and full parity."""
    x, P, eps, mask = MC.struct_case(shape, case, "case")
    m = _model(shape, "fast")
    worst = {}
    for obj in MR.OBJECTIVES:
        _reset(m, P)
        r, launches = MR.masked_out_launches(m, lambda: m.forward_backward(x, case[1], 1.0, obj, eps=eps, want=ROWS, mask=mask))
        assert launches == 0, (shape, obj, launches)
        res, g = MR.reference(*shape, *case, obj)
        _worst(worst, _parity(r, m.get_grads().copy(), res, g, mask, obj))
    _reset(m, P)
    _, launches = MR.masked_out_launches(m, lambda: m.train_step(x, case[1], 1.0, 1e-3, "iwae_elbo", eps=eps, mask=mask))
    assert launches == 0
    _report("refused %s B%d k%d forced fast: 0 launches" % (shape, *case), **worst)


# ---------------------------------------------------------------- 2. fast-route shapes
@pytest.mark.parametrize("case", MC.EDGE_CASES, ids=_sid)
@pytest.mark.parametrize("route", ["general", "fast"])
@pytest.mark.parametrize("shape", MC.EDGE_DIMS, ids=_sid)
def test_edge_shape_matches_the_restatement(gpu, shape, route, case):
    worst = {}
    for obj in MR.OBJECTIVES:
        _worst(worst, _check(shape, case, route, obj))
    worst["adam"] = _forward_and_train_agree(shape, case, route, MR.OBJECTIVES[-1])
    _report("edge %s %s B%d k%d" % (shape, route, *case), abound=2e-6, **worst)


@pytest.mark.parametrize("route", ["general_noksplit", "fast_noksplit"])
@pytest.mark.parametrize("shape", MC.EDGE_DIMS, ids=_sid)
def test_edge_shape_without_the_k_split(gpu, shape, route):
    """f32_no_ksplit = 1 at 65 rows: masked_out_f32_kernel<false> where the defaults would split K (H >= 96)."""
    worst = {}
    for obj in MR.OBJECTIVES:
        _worst(worst, _check(shape, (5, 13), route, obj))
    _report("edge %s %s B5 k13" % (shape, route), **worst)


# ---------------------------------------------------------------- 3. row counts between 130 and 4 100
@pytest.mark.parametrize("case", MC.MID_CASES, ids=_sid)
@pytest.mark.parametrize("route", ["general", "fast"])
def test_mid_row_counts_match_the_restatement(gpu, route, case):
    """200 / 100 / 784 at 450, 1 000 and 2 000 rows: the K split of the output layer in 3 chunks (kslabs 5), in 2 (kslabs 7), and none."""
    worst = {}
    for obj in MC.MID_OBJECTIVES:
        _worst(worst, _check(MC.WIDE, case, route, obj))
    _report("mid rows %s B%d k%d (K chunks %s)" % (route, *case, MC.MID_CHUNKS[case]), **worst)


# ---------------------------------------------------------------- 4. the two routes, bit for bit
BITWISE = [(s, c, "") for s in MC.EDGE_DIMS for c in MC.EDGE_CASES] + [(MC.WIDE, c, "") for c in MC.MID_CASES] + [(s, (5, 13), "_noksplit") for s in MC.EDGE_DIMS]


@pytest.mark.parametrize("shape,case,suffix", BITWISE, ids=lambda v: _sid(v) if v else "split")
def test_general_and_fast_route_are_bitwise_equal(gpu, shape, case, suffix):
    """masked_out_f32_kernel forms the general route's float32 numbers in the general route's order (kernel header):
    lpxz, log_w, the four scalars and the flat gradient are array_equal between the routes.  The figures are printed before they are held."""
    objs = MC.MID_OBJECTIVES if shape == MC.WIDE else MR.OBJECTIVES
    out = {}
    for obj in objs:
        (r1, g1), (r2, g2) = _run(shape, case, "general" + suffix, obj), _run(shape, case, "fast" + suffix, obj)
        out[obj] = (r1, g1, r2, g2)
        gn = float(np.linalg.norm(g1.astype(np.float64) - g2) / max(np.linalg.norm(g2.astype(np.float64)), 1e-30))
        print("routes %s B%d k%d %s%s: max |d lpxz| %.3g, max |d log_w| %.3g, scalars %.3g, gradient %.3g (unequal elements %d of %d)"
              % (shape, case[0], case[1], obj, suffix, float(np.max(np.abs(r1["lpxz"] - r2["lpxz"]))), float(np.max(np.abs(r1["log_w"] - r2["log_w"]))),
                 max(abs(r1[key] - r2[key]) for key in SCALARS), gn, int(np.sum(g1 != g2)), g1.size))
    for obj, (r1, g1, r2, g2) in out.items():
        np.testing.assert_array_equal(r1["lpxz"], r2["lpxz"], err_msg=obj)
        np.testing.assert_array_equal(r1["log_w"], r2["log_w"], err_msg=obj)
        for key in SCALARS:
            assert r1[key] == r2[key], (obj, key, r1[key], r2[key])
        np.testing.assert_array_equal(g1, g2, err_msg=obj)


# ---------------------------------------------------------------- 5. mask structures
STRUCT_ROUTES = [(s, r) for s in MC.STRUCT_SHAPES for r in ("general", "fast")]


def _tensor(flat, P, i):
    lo, hi = MC.tensor_slices(P)[i]
    shape = P[i // 2][i % 2].shape
    return flat[lo:hi].reshape(shape)


def _assert_zero_where_never_observed(flat, P, mask, tag):
    """Exactly 0.0 (-0.0 included) at W3[:, j], b3[j] and W1[j, :] for every pixel j no image of the batch observes."""
    nv = MC.never_observed(mask)
    assert nv.size > 0, tag
    assert np.all(_tensor(flat, P, 12)[:, nv] == 0.0), (tag, "W3")
    assert np.all(_tensor(flat, P, 13)[nv] == 0.0), (tag, "b3")
    assert np.all(_tensor(flat, P, 0)[nv, :] == 0.0), (tag, "W1")
    return nv.size


@pytest.mark.parametrize("case", MC.STRUCT_CASES, ids=_sid)
@pytest.mark.parametrize("structure", MC.STRUCTURES)
@pytest.mark.parametrize("shape,route", STRUCT_ROUTES, ids=_sid)
def test_mask_structure_matches_the_restatement(gpu, shape, route, structure, case):
    x, P, eps, mask = MC.struct_case(shape, case, structure)
    worst, nv = {}, 0
    for obj in MR.OBJECTIVES:
        _worst(worst, _check(shape, case, route, obj, 1.0, structure))
        r, flat = _run(shape, case, route, obj, 1.0, structure)
        if structure in MC.NEVER_OBSERVED:
            nv = _assert_zero_where_never_observed(flat, P, mask, (structure, obj))
        if structure == "none":      # every image empty: log p(x_obs|z) = 0, no decoder gradient, no gradient of the encoder's first kernel
            assert np.all(r["lpxz"] == 0.0) and r["mean_lpxz"] == 0.0
            for i in (0, 8, 9, 10, 11, 12, 13):
                assert np.all(_tensor(flat, P, i) == 0.0), (obj, i)
            for key in SCALARS:
                assert np.isfinite(r[key]), (obj, key)
    _report("structure %s %s %s B%d k%d: never-observed columns %d" % (structure, shape, route, *case, nv), **worst)


@pytest.mark.parametrize("fill", [np.nan, 1e30], ids=["nan", "1e30"])
@pytest.mark.parametrize("structure", MC.NEVER_OBSERVED)
@pytest.mark.parametrize("shape,route", STRUCT_ROUTES, ids=_sid)
def test_never_observed_columns_stay_exactly_zero_whatever_x_holds(gpu, shape, route, structure, fill):
    """NaN / 1e30 at every unobserved pixel of x: the results are bitwise those of the clean x, and the gradient at W3[:, j], b3[j], W1[j, :]
    of the never-observed pixels is exactly 0."""
    case = MC.STRUCT_CASES[0]
    x, P, eps, mask = MC.struct_case(shape, case, structure)
    xf = np.where(mask != 0, x, np.float32(fill)).astype(np.float32)
    m = _model(shape, route)
    for obj in MR.OBJECTIVES:
        r, flat = _run(shape, case, route, obj, 1.0, structure)
        _reset(m, P)
        rf = _witnessed(m, route, case[0] * case[1], lambda: m.forward_backward(xf, case[1], 1.0, obj, eps=eps, want=ROWS, mask=mask))
        gf = m.get_grads().copy()
        for key in r:
            np.testing.assert_array_equal(np.asarray(r[key]), np.asarray(rf[key]), err_msg=key)
        np.testing.assert_array_equal(flat, gf)
        _assert_zero_where_never_observed(gf, P, mask, (structure, obj, fill))


def _raw_calls(m, P, x, mask, k, eps, obj_id):
    """The three masked entry points through the raw binding on a uint8 mask passed as it is: (scalars x 3, gradient, parameters after the train step)."""
    from iwae_amd._capi import Scalars
    x, eps, mask = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(eps, np.float32), np.ascontiguousarray(mask, np.uint8)
    B = x.shape[0]
    out = []
    s = Scalars()
    _reset(m, P)
    assert m.lib.iwae_forward_masked(m.h, x.ctypes.data, mask.ctypes.data, B, k, 1.0, eps.ctypes.data, C.byref(s), None) == 0
    out.append([float(getattr(s, n)) for n in SCALARS + ("mean_lpxz",)])
    assert m.lib.iwae_forward_backward_masked(m.h, x.ctypes.data, mask.ctypes.data, B, k, 1.0, obj_id, eps.ctypes.data, C.byref(s), None) == 0
    out.append([float(getattr(s, n)) for n in SCALARS + ("mean_lpxz",)])
    out.append(m.get_grads().copy())
    assert m.lib.iwae_train_step_masked(m.h, x.ctypes.data, mask.ctypes.data, B, k, 1.0, 1e-3, obj_id, eps.ctypes.data, C.byref(s), None) == 0
    out.append([float(getattr(s, n)) for n in SCALARS + ("mean_lpxz",)])
    out.append(m.get_grads().copy())
    out.append(m.get_params().copy())
    return out


@pytest.mark.parametrize("shape,route", STRUCT_ROUTES, ids=_sid)
def test_any_non_zero_mask_byte_means_observed(gpu, shape, route):
    """The ABI's contract (include/iwae_amd.h: non-zero = observed) below NativeModel._mask_arg's coercion to 0 / 1: observed bytes 2, 0x80,
    255 and a mix of them give bitwise the 0 / 1 mask's results on all three entry points."""
    from iwae_amd.native import OBJECTIVES
    case = (5, 13)
    x, P, eps, mask = MC.struct_case(shape, case, "case")
    m = _model(shape, route)
    mix = (mask * np.random.default_rng(5).choice(np.array([1, 2, 0x80, 255], np.uint8), size=mask.shape)).astype(np.uint8)
    for obj in ("iwae_elbo", "dreg"):
        base = _witnessed(m, route, 65, lambda: _raw_calls(m, P, x, mask, 13, eps, OBJECTIVES[obj]))
        for name, mk in (("2", mask * np.uint8(2)), ("0x80", mask * np.uint8(0x80)), ("255", mask * np.uint8(255)), ("mixed", mix)):
            assert np.array_equal(mk != 0, mask != 0) and mk.dtype == np.uint8
            got = _raw_calls(m, P, x, mk, 13, eps, OBJECTIVES[obj])
            for i, (a, b) in enumerate(zip(base, got)):
                np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg="%s %s item %d" % (obj, name, i))
    assert np.all(np.isfinite(base[-1])) and np.any(base[2] != 0.0)


# ---------------------------------------------------------------- 6. off the random initialisation
def _offinit_body(c, structure, route, close=False):
    """The body of test_float32_step_off_init_matches_exact_oracle under a mask, at its bounds, on the module's handle of the route."""
    x, P, eps, mask = MC.offinit_inputs(c, structure)
    res, g = MC.offinit_reference(c, structure)
    keys = ("iwae_elbo",) if c.obj == "dreg" else SCALARS
    rows_n = c.B * c.k
    m = _model(tuple(c.widths), route)
    _reset(m, P)
    r = _witnessed(m, route, rows_n, lambda: m.forward_backward(x, c.k, c.beta, c.obj, eps=eps, want=("lpxz", "lpz", "lqzx", "al", "z"), mask=mask))
    flat = m.get_grads().copy()
    assert np.all(np.isfinite(flat))
    errs = _grad_rel_errors(flat, g)
    d_il = abs(r["inference_loss"] - res["inference_loss"]) / (1e-4 * abs(res["inference_loss"]) + 1e-4) if c.obj == "dreg" else 0.0
    _report("masked off-init %s %s %s" % (OC.case_id(c), structure, route), rows=max(float(np.max(np.abs(r[a] - res[a]))) for a in ("lpxz", "lpz", "lqzx")),
            rows_bound=F32_ROW_ATOL, scalar_over_bound=max(abs(r[key] - res[key]) / _scalar_bound(res[key]) for key in keys), bound=1.0,
            inference_loss_over_bound=d_il, grad=max(errs), gbound=F32_GRAD_REL, max_logit=float(np.max(np.abs(res["logits"]))))
    for a in ("lpxz", "lpz", "lqzx"):
        assert np.max(np.abs(r[a] - res[a])) < F32_ROW_ATOL, (a, float(np.max(np.abs(r[a] - res[a]))))
    np.testing.assert_allclose(r["z"], res["z"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(r["al"], res["al"], atol=2e-4)
    for key in keys:
        assert abs(r[key] - res[key]) <= _scalar_bound(res[key]), (key, r[key], res[key])
    if c.obj == "dreg":
        assert d_il <= 1.0, (r["inference_loss"], res["inference_loss"])
    assert max(errs) < F32_GRAD_REL, errs
    r0 = _witnessed(m, route, rows_n, lambda: m.forward(x, c.k, c.beta, eps=eps, want=("lpxz",), mask=mask))
    for key in keys:
        assert abs(r0[key] - r[key]) <= 1e-6 * abs(r[key]) + 1e-5
    d_fwd = float(np.max(np.abs(r0["lpxz"] - res["lpxz"])))
    assert d_fwd < F32_ROW_ATOL, d_fwd
    _witnessed(m, route, rows_n, lambda: m.train_step(x, c.k, c.beta, 1e-3, c.obj, eps=eps, mask=mask))
    g2 = m.get_grads().astype(np.float64)
    assert np.linalg.norm(g2 - flat) / np.linalg.norm(flat) < 1e-5
    ref, _, _ = O.adam_update(O.flatten_params(P), flat.astype(np.float64), 0.0, 0.0, 1, 1e-3)
    d_adam = float(np.max(np.abs(m.get_params() - ref)))
    _report("   forward only / Adam", lpxz=d_fwd, rows_bound=F32_ROW_ATOL, adam=d_adam, abound=2e-6)
    assert d_adam < 2e-6


@pytest.mark.parametrize("route", ["general", "fast"])
@pytest.mark.parametrize("structure", MC.OFFINIT_MASKS)
@pytest.mark.parametrize("c", MC.OFFINIT, ids=MC.offinit_id)
def test_masked_step_off_init_matches_the_restatement(gpu, c, structure, route):
    _offinit_body(c, structure, route)


def test_masked_step_off_init_at_8500_rows_default_options(gpu):
    """(170, 50), two sharp units, case_mask, the default options: the general route with the weight gradients on the side stream."""
    _offinit_body(MC.OFFINIT_BIG, "case", "default")


@pytest.mark.parametrize("route", ["general", "fast"])
def test_masked_clean_saturation_stays_finite(gpu, route):
    """test_clean_saturation_stays_finite under case_mask: pre-activations of 60 and logits of 120; every output and gradient is finite, every
    row within max(F32_ROW_ATOL, F32_SCALAR_REL |row|) of the reference.  The gradient is not compared: 1 - y^2 is 0 almost everywhere."""
    x, P, eps, fig = OC.clean_saturation_inputs()
    k, B = eps.shape[:2]
    mask = MR.case_mask(B, OC.W1[2], 17 + B + k)
    res, _ = MR.masked_loss_grads(P, x, mask, eps, 1.0, "iwae_elbo")
    m = _model(OC.W1, route)
    for obj in ("iwae_elbo", "dreg", "vae_elbo_kl"):
        _reset(m, P)
        r = _witnessed(m, route, B * k, lambda: m.forward_backward(x, k, 1.0, obj, eps=eps, want=("lpxz", "lpz", "lqzx", "al", "z", "log_w", "snis_z"), mask=mask))
        for key, v in r.items():
            assert np.all(np.isfinite(v)), (obj, key)
        assert np.all(np.isfinite(m.get_grads())), obj
        np.testing.assert_allclose(r["al"].sum(0), 1.0, atol=1e-5)
        worst = max(float(np.max(np.abs(r[key] - res[key]) / np.maximum(F32_ROW_ATOL, F32_SCALAR_REL * np.abs(res[key])))) for key in ("lpxz", "lpz", "lqzx"))
        _report("masked clean saturation %s %s" % (route, obj), max_logit=fig["logit"], rows_over_bound=worst, bound=1.0, lpxz_mean=float(np.mean(res["lpxz"])),
                device_lpxz_mean=float(np.mean(r["lpxz"])))
        assert worst <= 1.0, worst


# ---------------------------------------------------------------- 7. state across calls
_ref_cache = {}


def _reference_at(params, x, mask, eps, obj):
    """masked_loss_grads at the DEVICE's parameters (a flat float32 read), cached on the parameters' bytes: the two routes give the same
    numbers, so the second route's sequence finds its references made."""
    key = (params.tobytes(), x.shape, mask.tobytes(), eps.shape, float(eps.ravel()[0]), obj)
    if key not in _ref_cache:
        P = MC.unflatten(params, MR.case(*MC.WIDE, 5, 13)[1])
        res, g = MR.masked_loss_grads(P, x, mask, eps, 1.0, obj)
        _ref_cache[key] = ({name: v for name, v in res.items() if name in SCALARS + ("lpxz", "log_w")}, g)      # (not the [k, B, X] logits)
    return _ref_cache[key]


def _trajectory(m, route, x, eps, k, masks):
    """Three iwae_train_step_masked calls; before each the device's parameters are read, after each its gradient."""
    out = []
    for mask in masks:
        before = m.get_params().copy()
        r = _witnessed(m, route, x.shape[0] * k, lambda: m.train_step(x, k, 1.0, 1e-3, "iwae_elbo", eps=eps, mask=mask))
        out.append((before, r, m.get_grads().copy(), m.get_params().copy()))
    return out


def test_three_steps_at_4100_rows_follow_the_reference_and_adam(gpu):
    """From 4 096 rows the decoder's weight gradients and its deferred update run on the side stream and read s, g1, g2 and the row weights
    the next masked forward rewrites.  (82, 50), default options, host eps, another mask at every step: each step's gradient is within
    F32_GRAD_REL of the reference AT THE PARAMETERS THE DEVICE HELD, each step's parameters within 2e-6 of float64 Adam on the device
    gradients so far; the whole run repeats bitwise."""
    B, k = 82, 50
    x, P, eps, _ = MR.case(*MC.WIDE, B, k)
    masks = MC.step_masks(B, MC.WIDE[2], 3)
    assert not np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[1], masks[2])
    m = _model(MC.WIDE, "default")
    runs = []
    for _ in range(2):
        _reset(m, P)
        runs.append(_trajectory(m, "default", x, eps, k, masks))
    theta, mo, ve = runs[0][0][0].astype(np.float64), 0.0, 0.0
    for t, (before, r, g, after) in enumerate(runs[0]):
        res, gref = _reference_at(before, x, masks[t], eps, "iwae_elbo")
        errs = _grad_rel_errors(g, gref)
        theta, mo, ve = MC.adam_host(theta, g, mo, ve, t + 1)
        d_adam = float(np.max(np.abs(after - theta)))
        _report("trajectory step %d" % t, iwae_elbo_over_bound=abs(r["iwae_elbo"] - res["iwae_elbo"]) / _scalar_bound(res["iwae_elbo"]), grad=max(errs),
                gbound=F32_GRAD_REL, adam=d_adam, abound=2e-6)
        assert abs(r["iwae_elbo"] - res["iwae_elbo"]) <= _scalar_bound(res["iwae_elbo"])
        assert max(errs) < F32_GRAD_REL, (t, errs)
        assert d_adam < 2e-6, (t, d_adam)
        if t:
            assert not np.array_equal(before, runs[0][t - 1][0])
    for a, b in zip(runs[0], runs[1]):
        np.testing.assert_array_equal(a[0], b[0])
        assert a[1] == b[1]
        np.testing.assert_array_equal(a[2], b[2])
        np.testing.assert_array_equal(a[3], b[3])
    assert m.get_adam_state()[2] == 3


@pytest.mark.parametrize("route", ["default", "fast"])
def test_masked_and_unmasked_calls_alternate_on_one_handle(gpu, route):
    """Masked and unmasked steps share f32.logits and gx and flip keeps_s; B and k change, so xmask, mask and xcode regrow.  Six calls on one
    handle, each against the reference at the parameters the device held before it (an unmasked call: the reference with a mask of ones,
    which test_masked_host.py ties to the unmasked oracle)."""
    X = MC.WIDE[2]
    big, small, wide = MR.case(*MC.WIDE, 82, 50), MR.case(*MC.WIDE, 5, 13), MR.case(*MC.WIDE, 200, 50)
    other = MR.case_mask(200, X, 977)
    seq = [("train", big, big[3], True), ("train", big, None, False), ("forward", small, small[3], True), ("train", wide, other, True),
           ("forward_backward", small, None, False), ("train", small, small[3], True)]
    m = _model(MC.WIDE, route)
    _reset(m, big[1])
    for i, (kind, (x, _, eps, _), mask, masked) in enumerate(seq):
        k, B = eps.shape[:2]
        before = m.get_params().copy()
        res, gref = _reference_at(before, x, mask if masked else np.ones((B, X), np.uint8), eps, "iwae_elbo")
        kw = dict(eps=eps, want=("lpxz", "log_w"))
        if masked:
            kw["mask"] = mask
        if kind == "train":
            call = lambda: m.train_step(x, k, 1.0, 1e-3, "iwae_elbo", **kw)
        elif kind == "forward":
            call = lambda: m.forward(x, k, 1.0, **kw)
        else:
            call = lambda: m.forward_backward(x, k, 1.0, "iwae_elbo", **kw)
        r, launches = MR.masked_out_launches(m, call)
        if masked:
            MR.expected_on_fast_route(route, launches, B * k)
        else:
            assert launches == 0
        figs = dict(rows=max(float(np.max(np.abs(r[a] - res[a]))) for a in ("lpxz", "log_w")), rows_bound=F32_ROW_ATOL,
                    scalars_over_bound=max(abs(r[key] - res[key]) / _scalar_bound(res[key]) for key in SCALARS))
        assert figs["rows"] < F32_ROW_ATOL and figs["scalars_over_bound"] <= 1.0, (i, kind, figs)
        if kind != "forward":
            errs = _grad_rel_errors(m.get_grads(), gref)
            figs.update(grad=max(errs), gbound=F32_GRAD_REL)
            assert max(errs) < F32_GRAD_REL, (i, kind, errs)
        if kind == "train":
            assert not np.array_equal(m.get_params(), before)
        else:
            np.testing.assert_array_equal(m.get_params(), before)
        _report("alternation %s call %d %s%s B%d k%d" % (route, i, kind, " masked" if masked else "", B, k), **figs)


def _device_copy(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd_address"])
@pytest.mark.parametrize("shape,route", [((37, 5, 53), "general"), ((16, 4, 48), "general"), ((16, 4, 48), "fast"), (MC.WIDE, "general"), (MC.WIDE, "fast")], ids=_sid)
def test_device_resident_x_and_mask_give_the_host_pointers_results(gpu, shape, route, odd):
    """x and mask as device tensors -- what iwae_train_step_masked's resident entry and the timing tool pass -- through
    train_step_masked_devptr and the raw iwae_forward_backward_masked: bitwise the host-pointer call; the mask also at an odd byte address
    (the rows behind the first of a larger uint8 buffer); the caller's buffers unchanged."""
    import torch
    from iwae_amd._capi import Scalars
    from iwae_amd.native import OBJECTIVES
    B, k = 5, 13
    X = shape[2]
    x, P, eps, mask = MR.case(*shape, B, k)
    x, eps = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(eps, np.float32)
    m = _model(shape, route)
    xt = _device_copy(torch, x)
    lead = (X if X % 2 else X + 1) if odd else 256
    host_buf = np.concatenate([np.full(lead, 1, np.uint8), mask.ravel(), np.full(X, 1, np.uint8)])
    buf = _device_copy(torch, host_buf)
    mt = buf[lead:lead + B * X]
    assert mt.data_ptr() % 2 == (1 if odd else 0) and mt.data_ptr() == buf.data_ptr() + lead
    obj = OBJECTIVES["iwae_elbo"]
    # iwae_forward_backward_masked, host eps
    _reset(m, P)
    r_host = _witnessed(m, route, B * k, lambda: m.forward_backward(x, k, 1.0, "iwae_elbo", eps=eps, mask=mask))
    g_host = m.get_grads().copy()
    _reset(m, P)
    s = Scalars()
    rc = _witnessed(m, route, B * k, lambda: m.lib.iwae_forward_backward_masked(m.h, C.c_void_p(xt.data_ptr()), C.c_void_p(mt.data_ptr()), B, k, 1.0, obj,
                                                                               eps.ctypes.data, C.byref(s), None))
    assert rc == 0
    for key in SCALARS + ("mean_lpxz",):
        assert float(getattr(s, key)) == r_host[key], key
    np.testing.assert_array_equal(m.get_grads(), g_host)
    # iwae_train_step_masked, device noise
    _reset(m, P)
    m.train_step(x, k, 1.0, 1e-3, "iwae_elbo", mask=mask)
    want = (m.get_grads().copy(), m.get_params().copy(), m.get_adam_state())
    _reset(m, P)
    _witnessed(m, route, B * k, lambda: m.train_step_masked_devptr(xt.data_ptr(), mt.data_ptr(), B, k, 1.0, 1e-3, obj))
    np.testing.assert_array_equal(m.get_grads(), want[0])
    np.testing.assert_array_equal(m.get_params(), want[1])
    mo, ve, t = m.get_adam_state()
    np.testing.assert_array_equal(mo, want[2][0])
    np.testing.assert_array_equal(ve, want[2][1])
    assert t == want[2][2] == 1 and np.all(np.isfinite(want[1]))
    m.sync()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(xt.cpu().numpy(), x)
    np.testing.assert_array_equal(buf.cpu().numpy(), host_buf)
