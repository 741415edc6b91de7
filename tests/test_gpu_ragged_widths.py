"""Parity at odd and tile-straddling feature widths.

A lane owns four consecutive features of every 16 (iwae_amd/csrc/layout.h), so a width with F % 4 != 0 is the one case where a lane's
own float4 / quad straddles the end of the tensor; the 16-, 32- and 64-feature tile edges taken one feature too far or one short
move KT, the MG groups and Np32 / Kp32; and with one odd width the tensor offsets of the flat parameter / gradient vector stop being
multiples of 4 floats.  The other GPU modules take their widths from round numbers (every hidden width and x_dim a multiple of 4).
Here the SAME operations run against the SAME oracle at the SAME tolerances (tests/_parity_common.py) -- only the widths are new, and
no shape in this module is a multiple of 4 in all three dimensions.

Every test prints its worst errors next to their bounds (pytest -rP shows them).
"""
import numpy as np
import pytest

from oracle import iwae_np as O, philox_np
import make_golden as MG
import _activity_common as LA
import _aggregate_common as AP
import _grad_moments_common as GM
from _parity_common import (EMU_ROW_ATOL, EMU_SCALAR_ATOL, EMU_GRAD_REL, EXACT_SCALAR_ATOL, EXACT_GRAD_REL, F32_SCALAR_REL, F32_GRAD_REL,
                            F32_ROW_ATOL, _grad_rel_errors, _elementwise_ok, _densities_at_device_head, _densities_at_device_heads_2layer)

pytestmark = pytest.mark.gpu

SEED = 123      # the handles' noise seed (philox_np.device_eps restates the device stream for it)

# (n_hidden, n_latent, x_dim): what each shape cuts
S_ODD = (37, 5, 53)            # every width odd; the quad is cut at 1 of 4
S_REF_M1 = (199, 99, 783)      # the reference's widths minus one; the quad is cut at 3 of 4
S_REF_P1 = (201, 101, 785)     # the reference's widths plus one: one feature into a new quad and a new 16-tile (785 = 49 * 16 + 1)
S_63 = (63, 31, 63)            # one short of a full 32-step and 64-group
S_65 = (65, 33, 65)            # one past a full 32-step and 64-group (a second MG group with one live feature)
S_KT5 = (129, 3, 17)           # KT = 5 (no template instantiation); a 3-D latent; x_dim one past a 16-tile
S_MAX = (255, 127, 1023)       # the largest odd widths: run-time-KT fallbacks
S_ONE = (1, 1, 1)              # the smallest model the ABI accepts

L2_SMALL = ([67, 35], [33, 3], 61)
L2_REF_M1 = ([199, 99], [97, 49], 783)
L2_REF_P1 = ([201, 101], [101, 51], 785)


def _model(layers, nh, nl, xd, precision="bf16", **kw):
    from iwae_amd.native import NativeModel
    return NativeModel(layers, nh, nl, x_dim=xd, seed=SEED, precision=precision, **kw)


def _report(tag, **figs):
    print("%s: %s" % (tag, ", ".join("%s %.3g" % kv for kv in figs.items())))


def _oracle(layers, nh, nl, xd, B, k, seed, obj, beta, emu):
    """The seeded inputs and the oracle's step for them (emu: with the bf16 rounding points)."""
    x, P, eps = MG.inputs(layers, nh, nl, xd, B, k, seed)
    rnd = O.bf16_round if emu else None
    if layers == 1:
        res, g = O.loss_grads_1layer(P, x, eps, beta, obj, rnd=rnd)
    else:
        res, g = O.loss_grads_2layer(P, x, eps[0], eps[1], 1.0, obj, rnd=rnd)
    return x, P, eps, res, g


def _adam_ref(P, g):
    ref, _, _ = O.adam_update(O.flatten_params(P), np.asarray(g, dtype=np.float64), 0.0, 0.0, 1, 1e-3)
    return ref


# ---------------------------------------------------------------- 1. the 1-layer bf16 train step
CASES_1L = [  # (shape, B, k, objective, beta): B * k in 6 .. 40, B no multiple of 4, k = 1 and k > 1, the five objectives
    (S_ODD, 5, 3, "dreg", 1.0),                 # DReG at n_latent % 4 = 1
    (S_REF_M1, 7, 5, "vae_elbo_kl", 0.7),       # the analytic KL at n_latent % 4 = 3, beta != 1
    (S_REF_M1, 9, 1, "vae_elbo", 1.0),
    (S_REF_P1, 6, 5, "iwae_elbo", 1.0),
    (S_REF_P1, 7, 3, "dreg", 1.0),
    (S_63, 3, 7, "iwae_eq14", 1.0),
    (S_65, 10, 1, "vae_elbo", 1.0),
    (S_65, 5, 6, "vae_elbo_kl", 1.0),
    (S_KT5, 5, 8, "iwae_elbo", 1.0),
    (S_KT5, 9, 4, "dreg", 1.0),
    (S_MAX, 3, 2, "iwae_elbo", 1.0),
    (S_MAX, 7, 5, "iwae_eq14", 1.0),
    (S_ONE, 6, 5, "iwae_elbo", 1.0),
]


@pytest.mark.parametrize("shape,B,k,obj,beta", CASES_1L)
def test_train_step_1layer_matches_oracle(gpu, shape, B, k, obj, beta):
    """The body of test_gpu_parity.py::test_train_step_1layer_matches_oracle over the shape set.  S_ONE: a gradient tensor has one
    element and a single bf16 flip is the whole tensor -- finite, the scalars, and the gradient against the exact oracle only (its strict
    check is the float32 test below)."""
    nh, nl, xd = shape
    x, P, eps = MG.inputs(1, nh, nl, xd, B, k, 100 + B + k)
    res_e, g_e = O.loss_grads_1layer(P, x, eps, beta, obj, rnd=O.bf16_round)
    res_x, g_x = O.loss_grads_1layer(P, x, eps, beta, obj)
    m = _model(1, nh, nl, xd)
    m.set_params(O.flatten_params(P))
    r = m.forward_backward(x, k, beta, obj, eps=eps, want=("z", "snis_z", "al", "logits", "lpxz", "lpz", "lqzx"))
    g = m.get_grads()
    for key in ("z", "snis_z", "al", "logits", "lpxz", "lpz", "lqzx"):
        assert np.all(np.isfinite(r[key])), key
    assert np.all(np.isfinite(g))
    d_row = max(float(np.max(np.abs(r[key] - res_e[key]))) for key in ("lpxz", "lpz", "lqzx"))
    d_se = max(abs(r[key] - res_e[key]) for key in ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14"))
    d_sx = max(abs(r[key] - res_x[key]) for key in ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14"))
    e_e, e_x = max(_grad_rel_errors(g, g_e)), max(_grad_rel_errors(g, g_x))
    _report("1-layer bf16 %s B%d k%d %s" % (shape, B, k, obj), rows=d_row, rows_bound=EMU_ROW_ATOL, scalar_emu=d_se, bound=EMU_SCALAR_ATOL,
            scalar_exact=d_sx, bound_x=EXACT_SCALAR_ATOL, grad_emu=e_e, gbound=EMU_GRAD_REL, grad_exact=e_x, gbound_x=EXACT_GRAD_REL)
    strict = shape != S_ONE
    if strict:
        for key in ("lpxz", "lpz", "lqzx"):
            assert np.max(np.abs(r[key] - res_e[key])) < EMU_ROW_ATOL, key
        np.testing.assert_allclose(r["z"], res_e["z"], rtol=0, atol=1e-2)     # a bf16-ulp flip in h1/h2 moves mu by ~1e-3
        np.testing.assert_allclose(r["al"], res_e["al"], atol=2e-2)
        np.testing.assert_allclose(r["snis_z"], res_e["snis_z"], atol=5e-2)
        assert np.max(np.abs(r["logits"] - res_e["logits"])) < 2e-2
    np.testing.assert_allclose(r["al"].sum(0), 1.0, atol=1e-5)
    for key in ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14"):
        assert abs(r[key] - res_e[key]) < EMU_SCALAR_ATOL, (key, r[key], res_e[key])
        assert abs(r[key] - res_x[key]) < EXACT_SCALAR_ATOL, (key, r[key], res_x[key])
    if obj == "dreg":
        assert abs(r["inference_loss"] - res_e["inference_loss"]) < 5e-3 * abs(res_e["inference_loss"]) + 0.05
    if strict:
        assert e_e < EMU_GRAD_REL, _grad_rel_errors(g, g_e)
    assert e_x < EXACT_GRAD_REL, _grad_rel_errors(g, g_x)
    # Keras Adam, eps = 1e-4 (main.py:93): one step from the device gradient
    m.adam_step(1e-3)
    d_adam = float(np.max(np.abs(m.get_params() - _adam_ref(P, g))))
    _report("   Adam", d=d_adam, bound=2e-6)
    assert d_adam < 2e-6
    m.close()


# ---------------------------------------------------------------- 2. float32 mode
CASES_F32 = [  # (shape, B, k, objective, beta)
    (S_ODD, 5, 3, "dreg", 1.0),
    (S_ODD, 6, 5, "iwae_elbo", 0.7),
    (S_REF_M1, 7, 5, "vae_elbo_kl", 0.7),
    (S_REF_P1, 6, 5, "iwae_elbo", 1.0),
    (S_REF_P1, 7, 3, "dreg", 1.0),
    (S_63, 3, 7, "iwae_eq14", 1.0),
    (S_65, 10, 1, "vae_elbo", 1.0),
    (S_KT5, 5, 8, "iwae_elbo", 1.0),
    (S_MAX, 3, 2, "iwae_elbo", 1.0),
    (S_ONE, 6, 5, "iwae_elbo", 1.0),
    (S_ONE, 5, 1, "vae_elbo_kl", 0.7),
]


def _float32_body(layers, nh, nl, xd, B, k, obj, beta, seed, logits=True, tag=""):
    """The body of test_gpu_parity.py::test_float32_mode_matches_exact_oracle, incl. the forward / train_step agreement and the Adam
    step: these are what exercise odd offsets in the flat vector (16-byte transposed epilogues, the slab reduction with Adam inside)."""
    x, P, eps, res, g = _oracle(layers, nh, nl, xd, B, k, seed, obj, beta, False)
    if layers == 1:
        rows = (("lpxz", "lpxz"), ("lpz", "lpz"), ("lqzx", "lqzx"))
        keys = ("iwae_elbo",) if obj == "dreg" else ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14")
    else:
        rows = (("lpxz", "lpxz1"), ("lpz", "lpz1z2"), ("lpz2", "lpz2"), ("lqzx", "lqz1x"), ("lqzx2", "lqz2z1"))
        keys = ("vae_elbo", "iwae_elbo", "iwae_eq14")
    m = _model(layers, nh, nl, xd, precision="fp32")
    m.set_params(O.flatten_params(P))
    r = m.forward_backward(x, k, beta, obj, eps=eps, want=tuple(a for a, _ in rows) + ("al", "z") + (("logits",) if logits else ()))
    flat = m.get_grads()
    errs = _grad_rel_errors(flat, g)
    _report("float32 %s%s B%d k%d %s" % (tag, (nh, nl, xd), B, k, obj),
            rows=max(float(np.max(np.abs(r[a] - res[b]))) for a, b in rows), rows_bound=F32_ROW_ATOL,
            scalar_rel=max(abs(r[key] - res[key]) / (abs(res[key]) + 20.0) for key in keys), bound=F32_SCALAR_REL,
            grad=max(errs), gbound=F32_GRAD_REL)
    for a, b in rows:
        assert np.max(np.abs(r[a] - res[b])) < F32_ROW_ATOL, (a, float(np.max(np.abs(r[a] - res[b]))))
    if logits:
        assert np.max(np.abs(r["logits"] - res["logits"])) < 2e-4
    np.testing.assert_allclose(r["z"], res["z"] if layers == 1 else res["z1"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(r["al"], res["al"], atol=2e-4)
    for key in keys:
        assert abs(r[key] - res[key]) <= F32_SCALAR_REL * abs(res[key]) + 2e-4, (key, r[key], res[key])
    if obj == "dreg":
        assert abs(r["inference_loss"] - res["inference_loss"]) <= 1e-4 * abs(res["inference_loss"]) + 1e-4
    assert max(errs) < F32_GRAD_REL, errs
    # the forward-only call and the fused train step agree with the two-call path; Keras Adam from the device gradient
    r0 = m.forward(x, k, beta, eps=eps)
    for key in keys:
        assert abs(r0[key] - r[key]) <= 1e-6 * abs(r[key]) + 1e-5
    m.train_step(x, k, beta, 1e-3, obj, eps=eps)
    g2 = m.get_grads().astype(np.float64)
    assert np.linalg.norm(g2 - flat) / np.linalg.norm(flat) < 1e-5
    d_adam = float(np.max(np.abs(m.get_params() - _adam_ref(P, flat))))
    _report("   Adam", d=d_adam, bound=2e-6)
    assert d_adam < 2e-6
    m.close()


@pytest.mark.parametrize("shape,B,k,obj,beta", CASES_F32)
def test_float32_mode_matches_exact_oracle(gpu, shape, B, k, obj, beta):
    nh, nl, xd = shape
    _float32_body(1, nh, nl, xd, B, k, obj, beta, 300 + B + k)


# ---------------------------------------------------------------- 3. the row-count families of the step plan
ROWS = [(120, 50), (170, 50)]      # 6 000 rows: the middle family; 8 500: the pipelined decoder / fused dX family


@pytest.mark.parametrize("obj", ["iwae_elbo", "dreg"])
@pytest.mark.parametrize("B,k", ROWS)
@pytest.mark.parametrize("shape", [S_REF_M1, S_REF_P1])
def test_row_count_families_bf16(gpu, shape, B, k, obj):
    """The assertions of test_large_row_count_kernels_match_oracle and test_kernel_family_boundaries_match_oracle at the reference's
    widths -1 / +1: every row's densities against the oracle at the device's own encoder head and the typical row against the pure
    oracle, the encoder head itself, the scalars, every gradient tensor (norm and elementwise) against both oracles, and the same
    step through iwae_train_step (Adam fused into the slab reduction)."""
    nh, nl, xd = shape
    seed = 4242 + B
    x, P, eps, res_e, g_e = _oracle(1, nh, nl, xd, B, k, seed, obj, 1.0, True)
    m = _model(1, nh, nl, xd)
    m.set_params(O.flatten_params(P))
    r = m.forward_backward(x, k, 1.0, obj, eps=eps, want=("lpxz", "lqzx", "lpz"))
    g = m.get_grads()
    at = _densities_at_device_head(m, P, x, eps, nl)
    enc = O._Block(P[0:4], O.bf16_round)
    mu_o, sig_o = enc.fwd(O.bf16_round(np.asarray(x, dtype=np.float64)))
    assert np.max(np.abs(at["mu"] - mu_o)) < 1e-2 and np.max(np.abs(at["sigma"] / sig_o - 1.0)) < 1e-2
    keys = ("iwae_elbo",) if obj == "dreg" else ("vae_elbo", "iwae_elbo", "iwae_eq14")
    errs_e = _grad_rel_errors(g, g_e)
    _report("rows bf16 %s B%d k%d %s" % (shape, B, k, obj),
            rows_at_head=max(float(np.max(np.abs(r[key] - at[key]))) for key in ("lpxz", "lqzx", "lpz")), rows_bound=EMU_ROW_ATOL,
            scalar_emu=max(abs(r[key] - res_e[key]) for key in keys), bound=EMU_SCALAR_ATOL, grad_emu=max(errs_e), gbound=EMU_GRAD_REL)
    for key in ("lpxz", "lqzx", "lpz"):
        err = np.abs(r[key] - at[key])
        assert err.max() < EMU_ROW_ATOL, (key, err.max())
        err = np.abs(r[key] - res_e[key])       # and against the pure oracle: the typical row
        assert np.quantile(err, 0.98) < EMU_ROW_ATOL, (key, np.quantile(err, 0.98), err.max())
    for key in keys:
        assert abs(r[key] - res_e[key]) < EMU_SCALAR_ATOL, (key, r[key], res_e[key])
    if obj == "dreg":
        assert abs(r["inference_loss"] - res_e["inference_loss"]) < 5e-3 * abs(res_e["inference_loss"]) + 0.05
    assert max(errs_e) < EMU_GRAD_REL, errs_e
    worst = _elementwise_ok(g, g_e)
    _, _, _, res_x, g_x = _oracle(1, nh, nl, xd, B, k, seed, obj, 1.0, False)
    errs_x = _grad_rel_errors(g, g_x)
    _report("   ", elementwise=worst, bound=3e-2, grad_exact=max(errs_x), gbound_x=EXACT_GRAD_REL)
    assert max(errs_x) < EXACT_GRAD_REL, errs_x
    # the same step through iwae_train_step (Adam fused into the slab reduction) lands on the same parameters
    r2 = m.train_step(x, k, 1.0, 1e-3, obj, eps=eps)
    assert abs(r2["iwae_elbo"] - r["iwae_elbo"]) < 1e-5
    np.testing.assert_array_equal(m.get_grads(), g)
    assert np.max(np.abs(m.get_params() - _adam_ref(P, g))) < 2e-6
    m.close()


@pytest.mark.parametrize("logits", [True, False], ids=["logits", "fused-epilogue"])
@pytest.mark.parametrize("B,k", ROWS)
@pytest.mark.parametrize("shape", [S_REF_M1, S_REF_P1])
def test_row_count_families_float32(gpu, shape, B, k, logits):
    """float32 mode at 6 000 and 8 500 rows (row-split weight gradients; from ~8 000 rows the call without `logits` takes the output
    layer's fused epilogue -- the case with want=("logits",) does not)."""
    nh, nl, xd = shape
    _float32_body(1, nh, nl, xd, B, k, "iwae_elbo", 1.0, 4242 + B, logits=logits)


# ---------------------------------------------------------------- 4. the 2-layer model
CASES_2L = [(L2_SMALL, 5, 3, "iwae_elbo"), (L2_SMALL, 6, 5, "iwae_eq14"), (L2_REF_M1, 3, 7, "iwae_elbo"), (L2_REF_P1, 7, 5, "vae_elbo"),
            (L2_REF_M1, 170, 50, "iwae_elbo")]


@pytest.mark.parametrize("shape,B,k,obj", CASES_2L)
def test_train_step_2layer_matches_oracle(gpu, shape, B, k, obj):
    """The assertions of test_gpu_parity.py::test_train_step_2layer_matches_oracle (its bounds, unchanged), densities at the device's
    own three Gaussian heads; at 8 500 rows the fused chain kernels and the one-launch decoder, scalars and gradients against the
    rounding-aware oracle at EMU_SCALAR_ATOL / EMU_GRAD_REL as test_two_layer_large_row_count_matches_oracle holds them at that size.
    The MAXIMUM over rows against the PURE oracle (0.4 nat on log p(z1|z2), 0.05 on the others) is that test's statement for a few dozen
    rows.  At 8 500 rows it is not a property of the arithmetic: the oracle with the bf16 rounding points against the exact oracle -- its
    own sensitivity to one rounding -- differs at ([199, 99], [97, 49], 783), B = 170, k = 50 by up to 13.4 nat on log p(z1|z2) and 2.4 nat
    on log p(z2) (0.9-quantiles 0.70 / 0.24), and the device, which is within 2e-2 of the oracle at its own heads on EVERY row, measured
    0.83 nat there.  At that row count the pure oracle is held for the typical row, in the form the suite uses from 8 192 rows on
    (test_headline_size_step_matches_oracle: 0.9-quantile < 0.05 on the latent densities, 0.98-quantile < 0.03 on log p(x|z))."""
    nh, nl, xd = shape
    seed = 200 + B + k
    x, P, eps, res_e, g_e = _oracle(2, nh, nl, xd, B, k, seed, obj, 1.0, True)
    m = _model(2, nh, nl, xd)
    m.set_params(O.flatten_params(P))
    r = m.forward_backward(x, k, 1.0, obj, eps=eps, want=("z", "z2", "al", "lpxz", "lpz", "lqzx", "lpz2", "lqzx2", "snis_z", "snis_z2"))
    g = m.get_grads()
    at = _densities_at_device_heads_2layer(m, eps[0], eps[1], B, k, nl, P, x)
    worst_at = 0.0
    for a, b in (("lpxz", "lpxz1"), ("lpz", "lpz1z2"), ("lpz2", "lpz2"), ("lqzx", "lqz1x"), ("lqzx2", "lqz2z1")):
        d_at = float(np.max(np.abs(r[a] - at[b])))
        worst_at = max(worst_at, d_at / (EMU_ROW_ATOL if b == "lpxz1" else 2e-2))
        assert d_at < (EMU_ROW_ATOL if b == "lpxz1" else 2e-2), (b, d_at)
        err_e = np.abs(r[a] - res_e[b])
        if B * k <= 4096:
            assert err_e.max() < (0.4 if b == "lpz1z2" else 0.05), (b, err_e.max())      # (the pure oracle: loose, explained by the bound above)
        elif b == "lpxz1":     # 8 500 rows: the pure oracle holds for the typical row only, as in test_headline_size_step_matches_oracle
            assert np.quantile(err_e, 0.98) < EMU_ROW_ATOL, (b, np.quantile(err_e, 0.98))
        else:
            assert np.quantile(err_e, 0.9) < 0.05, (b, np.quantile(err_e, 0.9))
    np.testing.assert_allclose(r["z"], res_e["z1"], rtol=0, atol=1e-2)
    np.testing.assert_allclose(r["al"].sum(0), 1.0, atol=1e-5)
    errs_e = _grad_rel_errors(g, g_e)
    # (8 500 rows: the bounds test_two_layer_large_row_count_matches_oracle enforces at that size)
    s_tol, g_tol = (0.05, 2e-2) if B * k <= 4096 else (EMU_SCALAR_ATOL, EMU_GRAD_REL)
    _report("2-layer bf16 %s B%d k%d %s" % (shape, B, k, obj), rows_at_heads_over_bound=worst_at,
            scalar_emu=max(abs(r[key] - res_e[key]) for key in ("vae_elbo", "iwae_elbo", "iwae_eq14")), bound=s_tol,
            grad_emu=max(errs_e), gbound=g_tol)
    for key in ("vae_elbo", "iwae_elbo", "iwae_eq14"):
        assert abs(r[key] - res_e[key]) < s_tol, (key, r[key], res_e[key])
    lw = (r["lpxz"] + r["lpz"] + r["lpz2"] - r["lqzx"] - r["lqzx2"]).astype(np.float64)
    assert abs(r["iwae_elbo"] - float(np.mean(O.logmeanexp(lw, axis=0)))) < 1e-3
    assert abs(r["vae_elbo"] - float(np.mean(lw))) < 1e-3
    assert max(errs_e) < g_tol, errs_e
    _, _, _, res_x, g_x = _oracle(2, nh, nl, xd, B, k, seed, obj, 1.0, False)
    errs_x = _grad_rel_errors(g, g_x)
    _report("   ", scalar_exact=max(abs(r[key] - res_x[key]) for key in ("vae_elbo", "iwae_elbo", "iwae_eq14")), bound_x=0.3,
            grad_exact=max(errs_x), gbound_x=5e-2)
    for key in ("vae_elbo", "iwae_elbo", "iwae_eq14"):
        assert abs(r[key] - res_x[key]) < 0.3, (key, r[key], res_x[key])
    assert max(errs_x) < 5e-2, errs_x
    m.adam_step(1e-3)
    assert np.max(np.abs(m.get_params() - _adam_ref(P, g))) < 2e-6
    m.close()


@pytest.mark.parametrize("shape,B,k,obj", CASES_2L)
def test_float32_mode_2layer_matches_exact_oracle(gpu, shape, B, k, obj):
    nh, nl, xd = shape
    _float32_body(2, nh, nl, xd, B, k, obj, 1.0, 200 + B + k, logits=B * k < 1000, tag="2-layer ")


# ---------------------------------------------------------------- 5. conditional models: the condition sits in z's pad features
COND = [  # (n_hidden, n_latent, x_dim, cond_dim)
    (199, 21, 783, 10),      # 31 of 32: one pad feature left
    (65, 25, 65, 7),         # exactly fills 32
    (37, 5, 53, 3),
]


@pytest.mark.parametrize("prior", [False, True], ids=["n01-prior", "learned-prior"])
@pytest.mark.parametrize("nh,nl,xd,C", COND)
def test_conditional_models_match_oracle(gpu, nh, nl, xd, C, prior):
    """The assertions of test_conditional_model_matches_oracle / test_conditional_prior_model_matches_oracle."""
    B, k, obj, beta = (7, 6, "iwae_elbo", 1.0) if nl != 25 else (5, 4, "vae_elbo", 0.7)
    x, P, eps, y = MG.inputs(1, nh, nl, xd, B, k, 500 + nl, C, prior)
    res_e, g_e = O.loss_grads_1layer(P, x, eps, beta, obj, rnd=O.bf16_round, y=y)
    m = _model(1, nh, nl, xd, cond_dim=C, cond_prior=prior)
    assert m.n_params == sum(W.size + b.size for W, b in P)
    m.set_params(O.flatten_params(P))
    with pytest.raises(RuntimeError):
        m.forward_backward(x, k, beta, obj, eps=eps)            # no condition set yet: fails loudly
    m.set_condition(y)
    r = m.forward_backward(x, k, beta, obj, eps=eps, want=("lpxz", "lqzx", "lpz"))
    errs = _grad_rel_errors(m.get_grads(), g_e)
    _report("conditional bf16 (%d, %d, %d) C%d prior %d" % (nh, nl, xd, C, prior),
            lpxz=float(np.max(np.abs(r["lpxz"] - res_e["lpxz"]))), lqzx=float(np.max(np.abs(r["lqzx"] - res_e["lqzx"]))), rows_bound=EMU_ROW_ATOL,
            lpz=float(np.max(np.abs(r["lpz"] - res_e["lpz"]))), lpz_bound=0.2 if prior else EMU_ROW_ATOL,
            scalar_emu=max(abs(r[key] - res_e[key]) for key in ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14")), bound=EMU_SCALAR_ATOL,
            grad_emu=max(errs), gbound=EMU_GRAD_REL)
    for key in ("lpxz", "lqzx", "lpz"):
        # learned prior: lpz divides by sigma_p^2 of a head that comes out of bf16-fed GEMMs (as in test_conditional_prior_model_matches_oracle)
        assert np.max(np.abs(r[key] - res_e[key])) < (0.2 if key == "lpz" and prior else EMU_ROW_ATOL), key
    for key in ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14"):
        assert abs(r[key] - res_e[key]) < EMU_SCALAR_ATOL, (key, r[key], res_e[key])
    assert max(errs) < EMU_GRAD_REL, errs
    if prior:
        with pytest.raises(ValueError):
            m.forward_backward(x, k, beta, "dreg", eps=eps)
    # sample(z, y): the decoder on concat(z, y); with the learned prior z -> mu_p(y) + sigma_p(y) * z first
    n = 7
    rng = np.random.default_rng(nl)
    z = rng.standard_normal((n, nl)).astype(np.float32)
    yz = np.eye(C, dtype=np.float32)[np.full(n, C - 1)]
    m.set_condition(yz)
    dec = O._MLP3(P[4:7], O.bf16_round)
    zz = z.astype(np.float64)
    if prior:
        mu_p, sig_p = O._Block(P[7:11], O.bf16_round).fwd(O.bf16_round(yz.astype(np.float64)))
        zz = mu_p + sig_p * zz
    ref = O.sigmoid(dec.fwd(O.bf16_round(np.concatenate([zz, yz], axis=-1))))
    assert np.max(np.abs(m.decode(z) - ref)) < 2e-2
    # the k = 64 likelihood estimate walks the condition rows chunk by chunk
    m.set_condition(y)
    m.set_step(5, 0)
    a = m.eval_llh(x, k=64, chunk=0)
    m.set_step(5, 0)                                      # same noise keys: only the chunking differs
    b2 = m.eval_llh(x, k=64, chunk=max(1, B // 3))
    assert abs(a - b2) < 1e-3
    m.close()


@pytest.mark.parametrize("prior", [False, True], ids=["n01-prior", "learned-prior"])
@pytest.mark.parametrize("nh,nl,xd,C", COND)
def test_float32_mode_conditional_models_match_exact_oracle(gpu, nh, nl, xd, C, prior):
    """The assertions of test_gpu_parity.py::test_float32_mode_conditional_models_match_exact_oracle."""
    B, k, obj, beta = (7, 6, "iwae_elbo", 1.0) if nl != 25 else (5, 4, "vae_elbo", 0.7)
    x, P, eps, y = MG.inputs(1, nh, nl, xd, B, k, 500 + nl, C, prior)
    res, g = O.loss_grads_1layer(P, x, eps, beta, obj, y=y)
    m = _model(1, nh, nl, xd, precision="fp32", cond_dim=C, cond_prior=prior)
    m.set_params(O.flatten_params(P))
    m.set_condition(y)
    r = m.forward_backward(x, k, beta, obj, eps=eps, want=("lpxz", "lqzx", "lpz", "logits"))
    flat = m.get_grads()
    errs = _grad_rel_errors(flat, g)
    _report("conditional float32 (%d, %d, %d) C%d prior %d" % (nh, nl, xd, C, prior),
            rows=max(float(np.max(np.abs(r[key] - res[key]))) for key in ("lpxz", "lqzx", "lpz")), rows_bound=F32_ROW_ATOL,
            grad=max(errs), gbound=F32_GRAD_REL)
    for key in ("lpxz", "lqzx", "lpz"):
        assert np.max(np.abs(r[key] - res[key])) < F32_ROW_ATOL, (key, float(np.max(np.abs(r[key] - res[key]))))
    assert np.max(np.abs(r["logits"] - res["logits"])) < 2e-4
    for key in ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14"):
        assert abs(r[key] - res[key]) <= F32_SCALAR_REL * abs(res[key]) + 2e-4, (key, r[key], res[key])
    assert max(errs) < F32_GRAD_REL, errs
    m.train_step(x, k, beta, 1e-3, obj, eps=eps)
    assert np.max(np.abs(m.get_params() - _adam_ref(P, flat))) < 2e-6
    m.set_params(O.flatten_params(P))
    m.set_condition(y)
    m.set_step(5, 0)
    a = m.eval_llh(x, k=64, chunk=0)
    m.set_step(5, 0)
    b2 = m.eval_llh(x, k=64, chunk=max(1, B // 3))
    assert abs(a - b2) < 1e-4
    m.close()


# ---------------------------------------------------------------- 6. the device's own noise at odd latent widths
@pytest.mark.parametrize("B,k,nh,nl,xd,obj", [(7, 3, 37, 1, 53, "iwae_elbo"), (7, 3, 37, 3, 53, "dreg"), (5, 6, 37, 5, 53, "iwae_elbo"),
                                              (6, 5, 65, 33, 65, "dreg"), (6, 5, 201, 101, 785, "iwae_elbo"),
                                              (170, 50, 201, 101, 785, "iwae_elbo"),      # 8 500 rows: z is made inside the decoder kernel
                                              (170, 50, 199, 99, 783, "dreg")])
def test_device_noise_step_matches_oracle_on_the_same_draws(gpu, B, k, nh, nl, xd, obj):
    """The assertions of test_gpu_parity.py::test_device_noise_step_matches_oracle_on_the_same_draws: Philox gives four normals per
    call, so at D % 4 != 0 the last call's tail is dropped (a width-5 draw is the first 5 columns of the width-8 draw).
    n_latent = 1: the gradients of the two head biases are ONE number each, the sum over the B images of the head gradient t_b, and every
    tensor is held to the unchanged EMU_GRAD_REL.  With the input seed 601 the t_b of the mu head cancel (|sum t| = 0.055 sum |t|, read
    off the oracle alone) and the relative error of that one number is the terms' error times 18, whatever the arithmetic; the inputs
    of that case are seed 602, where neither sum cancels (|sum t| = 0.70 sum |t| for both heads)."""
    step = 9
    x, P, _ = MG.inputs(1, nh, nl, xd, B, 1, 602 if nl == 1 else 600 + nl)
    eps = philox_np.device_eps(SEED, step, B, k, nl)
    res_e, g_e = O.loss_grads_1layer(P, x, eps, 1.0, obj, rnd=O.bf16_round)
    m = _model(1, nh, nl, xd)
    m.set_params(O.flatten_params(P))
    m.set_step(step, 0)
    r = m.forward_backward(x, k, 1.0, obj, want=("lpxz", "lpz", "lqzx", "z"))
    np.testing.assert_allclose(r["z"], res_e["z"], rtol=0, atol=1e-2)
    at = _densities_at_device_head(m, P, x, eps, nl)
    keys = ("iwae_elbo",) if obj == "dreg" else ("vae_elbo", "iwae_elbo", "iwae_eq14")
    errs = _grad_rel_errors(m.get_grads(), g_e)
    _report("device noise (%d, %d, %d) B%d k%d %s" % (nh, nl, xd, B, k, obj),
            rows_at_head=max(float(np.max(np.abs(r[key] - at[key]))) for key in ("lpxz", "lpz", "lqzx")), rows_bound=EMU_ROW_ATOL,
            scalar_emu=max(abs(r[key] - res_e[key]) for key in keys), bound=EMU_SCALAR_ATOL, grad_emu=max(errs), gbound=EMU_GRAD_REL)
    for key in ("lpxz", "lpz", "lqzx"):
        assert np.max(np.abs(r[key] - at[key])) < EMU_ROW_ATOL, key
        assert np.quantile(np.abs(r[key] - res_e[key]), 0.98) < EMU_ROW_ATOL, key
        assert np.max(np.abs(r[key] - res_e[key])) < 10 * EMU_ROW_ATOL, key
    for key in keys:
        assert abs(r[key] - res_e[key]) < EMU_SCALAR_ATOL, (key, r[key], res_e[key])
    if obj == "dreg":
        assert abs(r["inference_loss"] - res_e["inference_loss"]) < 5e-3 * abs(res_e["inference_loss"]) + 0.05
    assert max(errs) < EMU_GRAD_REL, errs
    m.close()


def test_device_noise_step_2layer_matches_oracle_on_the_same_draws(gpu):
    """The 2-layer model with n_latent = [33, 3]: z1 from stream 0, z2 from stream 1 (the device-noise assertions of
    test_kernel_family_boundaries_match_oracle and, per row at the device's heads, of test_two_layer_kernel_variants_agree)."""
    nh, nl, xd = L2_SMALL
    B, k, step = 6, 5, 17
    x, P, _ = MG.inputs(2, nh, nl, xd, B, 1, 633)
    e1 = philox_np.device_eps(SEED, step, B, k, nl[0], stream=0, batch_offset=3)
    e2 = philox_np.device_eps(SEED, step, B, k, nl[1], stream=1, batch_offset=3)
    res_d, g_d = O.loss_grads_2layer(P, x, e1, e2, 1.0, "iwae_elbo", rnd=O.bf16_round)
    m = _model(2, nh, nl, xd)
    m.set_params(O.flatten_params(P))
    m.set_step(step, 3)
    r = m.forward_backward(x, k, 1.0, "iwae_elbo", want=("lpz", "lpz2", "lqzx", "lqzx2"))
    at = _densities_at_device_heads_2layer(m, e1, e2, B, k, nl)
    errs = _grad_rel_errors(m.get_grads(), g_d)
    _report("device noise 2-layer %s" % (L2_SMALL,),
            rows_at_heads=max(float(np.max(np.abs(r[a] - at[b]))) for a, b in (("lpz", "lpz1z2"), ("lpz2", "lpz2"), ("lqzx", "lqz1x"), ("lqzx2", "lqz2z1"))),
            rows_bound=2e-2, scalar_emu=abs(r["iwae_elbo"] - res_d["iwae_elbo"]), bound=EMU_SCALAR_ATOL, grad_emu=max(errs), gbound=EMU_GRAD_REL)
    for a, b in (("lpz", "lpz1z2"), ("lpz2", "lpz2"), ("lqzx", "lqz1x"), ("lqzx2", "lqz2z1")):
        assert np.max(np.abs(r[a] - at[b])) < 2e-2, b
    assert abs(r["iwae_elbo"] - res_d["iwae_elbo"]) < EMU_SCALAR_ATOL
    assert max(errs) < EMU_GRAD_REL, errs
    m.close()


@pytest.mark.parametrize("nl", [1, 3, 5, 33, 101])
def test_device_noise_matches_published_philox(gpu, nl):
    """iwae_debug_eps at odd widths against the NumPy restatement (fast v_log / v_sin / v_cos: abs err <= 2e-5), the batch offset, and the
    forward pass consuming exactly these draws -- as test_gpu_parity.py::test_device_noise_matches_published_philox does at width 100."""
    nh, xd = (37, 53) if nl < 33 else (65, 65)
    m = _model(1, nh, nl, xd)
    m.set_step(7, 0)
    e = m.debug_eps(5, 3, 0)
    ref = philox_np.device_eps(SEED, 7, 5, 3, nl)
    _report("debug_eps width %d" % nl, d=float(np.max(np.abs(e - ref))), bound=2e-5)
    assert e.shape == (3, 5, nl) and np.max(np.abs(e - ref)) < 2e-5
    wide = philox_np.device_eps(SEED, 7, 5, 3, 4 * ((nl + 3) // 4))
    np.testing.assert_array_equal(ref, wide[:, :, :nl])      # the restatement: a narrow draw is the head of the quad-wide draw
    m.set_step(7, 2)                       # batch_offset 2: same draws as images 2.. of the unsplit batch
    e2 = m.debug_eps(3, 3, 0)
    np.testing.assert_array_equal(e2, e[:, 2:5])
    x, _, _ = MG.inputs(1, nh, nl, xd, 5, 1, 3)
    m.set_step(9, 0)
    ed = m.debug_eps(5, 3, 0)
    r1 = m.forward(x, 3, want=("lpxz", "lpz"))
    r2 = m.forward(x, 3, eps=ed, want=("lpxz", "lpz"))
    np.testing.assert_allclose(r1["lpz"], r2["lpz"], atol=1e-4)
    np.testing.assert_allclose(r1["lpxz"], r2["lpxz"], atol=1e-3)
    m.close()


# ---------------------------------------------------------------- 7. the evaluator and decode
@pytest.mark.parametrize("k", [130, 1000])
@pytest.mark.parametrize("layers,shape", [(1, S_ODD), (1, S_REF_P1), (2, L2_SMALL)])
def test_eval_llh_matches_exact_oracle_per_image(gpu, layers, shape, k):
    """iwae_eval_llh (main.py:170-184) on 5 images, both evaluator precisions, per image against the exact float64 oracle on the device's
    Philox draws (image i: rows i * k .. of streams 0 / 1): float32 evaluator <= 5e-3 nat, bf16 evaluator <= 0.1 nat (the bounds of
    test_trained_model_k5000_llh_within_north_star_tolerance)."""
    nh, nl, xd = shape
    n, step = 5, 999
    x, P, _ = MG.inputs(layers, nh, nl, xd, n, 1, 700 + k)
    m = _model(layers, nh, nl, xd)
    m.set_params(O.flatten_params(P))
    m.set_step(step, 0)
    llh, per = m.eval_llh(x, k, chunk=n, per_image=True)
    m.set_eval_precision("bf16")
    m.set_step(step, 0)
    _, per_bf = m.eval_llh(x, k, chunk=2, per_image=True)
    m.close()
    if layers == 1:
        per_o = np.array([float(O.forward_1layer(P, x[i:i + 1], philox_np.device_eps(SEED, step, 1, k, nl, batch_offset=i))["iwae_elbo"]) for i in range(n)])
    else:
        per_o = np.array([float(O.forward_2layer(P, x[i:i + 1], philox_np.device_eps(SEED, step, 1, k, nl[0], stream=0, batch_offset=i),
                                                 philox_np.device_eps(SEED, step, 1, k, nl[1], stream=1, batch_offset=i))["iwae_elbo"]) for i in range(n)])
    d32, dbf = float(np.max(np.abs(per - per_o))), float(np.max(np.abs(per_bf - per_o)))
    _report("eval_llh %s k%d" % (shape, k), float32_per_image=d32, bound=5e-3, bf16_per_image=dbf, bound_bf=0.1)
    assert abs(llh - per.mean()) < 1e-3
    assert d32 <= 5e-3, (per, per_o)
    assert dbf <= 0.1, (per_bf, per_o)


@pytest.mark.parametrize("shape", [S_ODD, S_REF_P1])
def test_decode_matches_oracle(gpu, shape):
    nh, nl, xd = shape
    x, P, eps = MG.inputs(1, nh, nl, xd, 4, 2, 55)
    m = _model(1, nh, nl, xd)
    m.set_params(O.flatten_params(P))
    z = np.random.default_rng(0).standard_normal((37, nl)).astype(np.float32)
    probs = m.decode(z)
    ref = O.sigmoid(O._MLP3(P[4:7], O.bf16_round).fwd(O.bf16_round(z)))
    _report("decode %s" % (shape,), d=float(np.max(np.abs(probs - ref))), bound=5e-3)
    assert probs.shape == (37, xd) and np.max(np.abs(probs - ref)) < 5e-3
    m.close()


# ---------------------------------------------------------------- 8. three Adam steps
@pytest.mark.parametrize("shape,B,k", [(S_ODD, 7, 3), (S_REF_P1, 20, 5)])
def test_three_adam_steps_track_the_oracle_trajectory(gpu, shape, B, k):
    """The loop of test_training_reduces_loss_and_matches_oracle_trajectory: each step reads the bf16 weight images the previous step's
    update wrote -- a misplaced image chunk at a non-multiple width shows from step 2 on."""
    nh, nl, xd = shape
    steps, lr = 3, 1e-3
    x, P, _ = MG.inputs(1, nh, nl, xd, B, k, 77)
    m = _model(1, nh, nl, xd)
    m.set_params(O.flatten_params(P))
    flat = O.flatten_params(P)
    mo = vo = 0.0
    rng = np.random.default_rng(5)
    worst = 0.0
    for t in range(1, steps + 1):
        eps = rng.standard_normal((k, B, nl)).astype(np.float32)
        r = m.train_step(x, k, 1.0, lr, "iwae_elbo", eps=eps)
        Pt = O.unflatten_params(flat, 1, nh, nl, xd)
        res, g = O.loss_grads_1layer(Pt, x, eps, 1.0, "iwae_elbo", rnd=O.bf16_round)
        flat, mo, vo = O.adam_update(flat, O.flatten_grads(g), mo, vo, t, lr)
        worst = max(worst, abs(r["iwae_elbo"] - res["iwae_elbo"]))
        assert abs(r["iwae_elbo"] - res["iwae_elbo"]) < 0.05, (t, r["iwae_elbo"], res["iwae_elbo"])
    # Adam's step is ~lr whatever the gradient's size: an element whose gradient is near zero may take another sign on the device -- at most one lr per step
    d = np.abs(m.get_params() - flat)
    _report("trajectory %s" % (shape,), objective=worst, bound=0.05, param_max=d.max(), pbound=2.0 * lr * steps, param_mean=np.mean(d), mbound=0.05 * lr * steps)
    assert d.max() < 2.0 * lr * steps and np.mean(d) < 0.05 * lr * steps, (d.max(), np.mean(d))
    m.close()


# ---------------------------------------------------------------- 9. the statistics entry points, one odd shape each
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("layers,shape", [(1, S_ODD), (2, L2_SMALL)])
def test_latent_activity_matches_float64(gpu, layers, shape, prec):
    nh, nl, xd = shape
    N, k = 37, 50
    x, P, m, eps = LA._setup(layers, nh, nl, xd, N, k, 31 + N, prec)
    m.set_step(5, 0)
    r = m.latent_activity(x, k=k, eps=eps, per_image=True)
    LA._check(r, LA.reference(P, x, eps, rnd=None if prec == "fp32" else O.bf16_round), prec)
    m.close()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_aggregate_posterior_per_sample_parity_and_sums(gpu, prec):
    nh, nl, xd = S_ODD
    N, S = 130, 3
    x, m, eps = AP._setup(nh, nl, xd, N, S, 17 + N + S, prec)
    r = m.aggregate_posterior(x, n_samples=S, eps=eps, per_sample=True)
    m.close()
    assert r["q_mu"].shape == (N, nl) and r["unit_kl"].shape == (nl,)
    AP._check_sums(r, AP._parity(r, eps), N)
    assert np.all(r["unit_mi"] <= np.log(N) + 1e-4)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("obj", ["iwae_elbo", "dreg"])
def test_grad_moments_equal_the_host_fold(gpu, prec, obj):
    nh, nl, xd = S_ODD
    B, k, M, beta = 5, 3, 4, 0.8
    m, x, _, _ = GM._model(1, nh, nl, xd, prec, B, k)
    before = GM._state(m)
    m.set_step(GM.S0)
    mean, var = m.grad_moments(x, k, M, beta, obj)
    g_after = m.get_grads()
    GM._assert_state_equal(GM._state(m), before)
    ref_mean, ref_var, g_last = GM._host_fold(m, x, k, beta, obj, GM.S0, M)
    assert np.array_equal(g_after.view(np.uint32), g_last.view(np.uint32))
    assert np.all(var >= 0) and np.max(var) > 0
    GM._close(mean, ref_mean)
    GM._close(var, ref_var)
    m.close()


def test_dataset_gather_binarize_is_bit_exact(gpu):
    """x_dim = 53: the last Philox call of a row covers one pixel."""
    nh, nl, xd = S_ODD
    rng = np.random.default_rng(3)
    N = 300
    gray = (rng.random((N, xd)) * 256).astype(np.uint8)
    gray[:, :5] = 0
    gray[:, 48:] = 255
    _, P, _ = MG.inputs(1, nh, nl, xd, 1, 1, 5)
    m = _model(1, nh, nl, xd)
    m.set_params(O.flatten_params(P))
    m.dataset_upload(gray)
    order = rng.permutation(N).astype(np.int32)
    for epoch in (0, 7):
        m.dataset_begin_epoch(epoch, order)
        xb = m.dataset_get_batch(37, 150)
        ref = philox_np.device_binarize(SEED, epoch, gray, order[37:187])
        np.testing.assert_array_equal(xb, ref)
    assert xb[:, :5].sum() == 0 and xb[:, 48:].min() == 1
    # a train step fed from the resident dataset equals a train step fed the same batch through the host path
    m.dataset_begin_epoch(7, order)
    m.set_step(5, 0)
    a = m.train_step_dataset(37, 150, 5, 1.0, 1e-3, "iwae_elbo")
    pa = m.get_params()
    m.set_params(O.flatten_params(P)); m.set_adam_state(np.zeros(m.n_params), np.zeros(m.n_params), 0)
    m.set_step(5, 0)
    b = m.train_step(ref, 5, 1.0, 1e-3, "iwae_elbo")
    assert a["iwae_elbo"] == b["iwae_elbo"]
    np.testing.assert_array_equal(pa, m.get_params())
    m.close()
