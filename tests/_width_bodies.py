"""The bodies of the width-walking GPU parity tests, shared by tests/test_gpu_ragged_widths.py (odd and tile-straddling widths) and
tests/test_gpu_aspect.py (inverted and exact-tile widths): the SAME operations against the SAME oracle at the SAME tolerances
(tests/_parity_common.py) -- a module supplies only its shapes, row counts and seeds.  Not a test module.

Every body prints its worst errors next to their bounds (pytest -rP shows them).
"""
import numpy as np
import pytest

from oracle import iwae_np as O, philox_np
import make_golden as MG
from _parity_common import (EMU_ROW_ATOL, EMU_SCALAR_ATOL, EMU_GRAD_REL, EXACT_SCALAR_ATOL, EXACT_GRAD_REL, F32_SCALAR_REL, F32_GRAD_REL,
                            F32_ROW_ATOL, _grad_rel_errors, _elementwise_ok, _densities_at_device_head, _densities_at_device_heads_2layer)

SEED = 123      # the handles' noise seed (philox_np.device_eps restates the device stream for it)


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
def train_step_1layer(shape, B, k, obj, beta, seed, strict=True):
    """The body of test_gpu_parity.py::test_train_step_1layer_matches_oracle.  strict=False ((1, 1, 1): a gradient tensor has one element
    and a single bf16 flip is the whole tensor): finite, the scalars, and the gradient against the exact oracle only."""
    nh, nl, xd = shape
    x, P, eps = MG.inputs(1, nh, nl, xd, B, k, seed)
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
def float32_step(layers, nh, nl, xd, B, k, obj, beta, seed, logits=True, tag=""):
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


# ---------------------------------------------------------------- 3. the row-count families of the step plan
def row_count_family_bf16(shape, B, k, obj, seed):
    """The assertions of test_large_row_count_kernels_match_oracle and test_kernel_family_boundaries_match_oracle: every row's densities
    against the oracle at the device's own encoder head and the typical row against the pure oracle, the encoder head itself, the
    scalars, every gradient tensor (norm and elementwise) against both oracles, and the same step through iwae_train_step (Adam fused
    into the slab reduction)."""
    nh, nl, xd = shape
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


# ---------------------------------------------------------------- 4. the 2-layer model
def train_step_2layer(shape, B, k, obj, seed, exact_grad=True):
    """The assertions of test_gpu_parity.py::test_train_step_2layer_matches_oracle (its bounds, unchanged), densities at the device's
    own three Gaussian heads; at 8 500 rows the fused chain kernels and the one-launch decoder, scalars and gradients against the
    rounding-aware oracle at EMU_SCALAR_ATOL / EMU_GRAD_REL as test_two_layer_large_row_count_matches_oracle holds them at that size.
    The MAXIMUM over rows against the PURE oracle (0.4 nat on log p(z1|z2), 0.05 on the others) is that test's statement for a few dozen
    rows.  At 8 500 rows it is not a property of the arithmetic: the oracle with the bf16 rounding points against the exact oracle -- its
    own sensitivity to one rounding -- differs at ([199, 99], [97, 49], 783), B = 170, k = 50 by up to 13.4 nat on log p(z1|z2) and 2.4 nat
    on log p(z2) (0.9-quantiles 0.70 / 0.24), and the device, which is within 2e-2 of the oracle at its own heads on EVERY row, measured
    0.83 nat there.  At that row count the pure oracle is held for the typical row, in the form the suite uses from 8 192 rows on
    (test_headline_size_step_matches_oracle: 0.9-quantile < 0.05 on the latent densities, 0.98-quantile < 0.03 on log p(x|z)).
    exact_grad=False: a case whose inputs the host module has shown inadmissible for the gradient comparison with the EXACT oracle (the
    rounding-aware oracle itself is too far from it) keeps every other assertion and prints the figure."""
    nh, nl, xd = shape
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
    if exact_grad:
        assert max(errs_x) < 5e-2, errs_x
    m.adam_step(1e-3)
    assert np.max(np.abs(m.get_params() - _adam_ref(P, g))) < 2e-6
    m.close()


def two_layer_kernel_variants_agree(nh, nl, xd, B, k, seed):
    """The body of test_gpu_parity.py::test_two_layer_kernel_variants_agree: the per-sample blocks fused into one launch each way
    (chain2_fwd_kernel / chain2_bwd_kernel: every layer of q(z2|z1) and p(z1|z2), the z2 sampling, the three log-densities and their
    gradients without a round trip through HBM) against the same mathematics as separate launches (dense_kernel x 6, sample_kernel,
    gauss_lp_kernel, gauss_bwd_kernel x 2, dense_kernel<EPI_DX> x 6): values, per-row densities and all 26 gradient tensors, on host
    noise and on the device's own."""
    x, P, eps = MG.inputs(2, nh, nl, xd, B, k, seed)

    def run(opts, e):
        m = _model(2, nh, nl, xd, options=opts)
        m.set_params(O.flatten_params(P))
        m.set_step(9, 2)
        r = m.forward_backward(x, k, 1.0, "iwae_elbo", eps=e, want=("lpz", "lpz2", "lqzx", "lqzx2", "z2"))
        # round 4: every variant's per-row densities against the oracle evaluated at THAT run's own Gaussian heads -- no window for outliers
        e1, e2 = e if e is not None else (philox_np.device_eps(123, 9, B, k, nl[0], stream=0, batch_offset=2),
                                          philox_np.device_eps(123, 9, B, k, nl[1], stream=1, batch_offset=2))
        at = _densities_at_device_heads_2layer(m, e1, e2, B, k, nl)
        for a, b in (("lpz", "lpz1z2"), ("lpz2", "lpz2"), ("lqzx", "lqz1x"), ("lqzx2", "lqz2z1")):
            err = np.abs(r[a] - at[b])
            assert err.max() < (5e-3 if e is not None else 2e-2), (opts, b, err.max())      # (device noise: the host restates the float32 draws in float64, d eps ~ 1e-7, divided by sigma_p)
        g = m.get_grads().astype(np.float64)
        m.close()
        return r, g

    for e, ref_opts in ((eps, {"no_chain2": 1}), (None, {"no_chain2": 1}), (eps, {"no_chain2_bwd": 1})):
        r0, g0 = run(ref_opts, e)
        r1, g1 = run({}, e)
        # the fused kernels start their accumulators from the bias, the separate launches add it at the end: float32 sums in another
        # order, so a bf16 activation flips by an ulp here and there and moves the densities of THAT row (log p(z1|z2) of a row with a small
        # sigma_p by several 0.1 nat at random init, |lpz| ~ 200-400) -- the typical row agrees to float32 rounding; the rows that do not are
        # accounted for inside run(): each variant matches the oracle at its own heads on every row
        worst = {}
        for key in ("lpz", "lpz2", "lqzx2"):
            err = np.abs(r1[key] - r0[key])
            worst[key] = float(np.quantile(err, 0.9))
            assert np.quantile(err, 0.9) < 2e-3 and err.max() < 1.0, (key, np.quantile(err, 0.9), err.max())
        errz = np.abs(r1["z2"] - r0["z2"])
        assert np.quantile(errz, 0.98) < 2e-3 and errz.max() < 0.05
        assert abs(r1["iwae_elbo"] - r0["iwae_elbo"]) < 2e-2
        d_g = float(np.linalg.norm(g1 - g0) / np.linalg.norm(g0))
        _report("2-layer variants %s vs fused, %s noise" % (ref_opts, "host" if e is not None else "device"), rows_q90=max(worst.values()),
                rows_bound=2e-3, scalar=abs(r1["iwae_elbo"] - r0["iwae_elbo"]), bound=2e-2, grad=d_g, gbound=5e-3)
        assert d_g < 5e-3


# ---------------------------------------------------------------- 5. conditional models: the condition sits in z's pad features
def conditional_bf16(nh, nl, xd, C, prior, B, k, obj, beta, seed):
    """The assertions of test_conditional_model_matches_oracle / test_conditional_prior_model_matches_oracle."""
    x, P, eps, y = MG.inputs(1, nh, nl, xd, B, k, seed, C, prior)
    res_e, g_e = O.loss_grads_1layer(P, x, eps, beta, obj, rnd=O.bf16_round, y=y)
    m = _model(1, nh, nl, xd, cond_dim=C, cond_prior=prior)
    assert m.n_params == sum(W.size + b.size for W, b in P)
    m.set_params(O.flatten_params(P))
    with pytest.raises(RuntimeError):
        m.forward_backward(x, k, beta, obj, eps=eps)            # no condition set yet: fails loudly
    m.set_condition(y)
    r = m.forward_backward(x, k, beta, obj, eps=eps, want=("lpxz", "lqzx", "lpz"))
    errs = _grad_rel_errors(m.get_grads(), g_e)
    _report("conditional bf16 (%d, %d, %d) C%d prior %d B%d k%d" % (nh, nl, xd, C, prior, B, k),
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


def conditional_float32(nh, nl, xd, C, prior, B, k, obj, beta, seed):
    """The assertions of test_gpu_parity.py::test_float32_mode_conditional_models_match_exact_oracle."""
    x, P, eps, y = MG.inputs(1, nh, nl, xd, B, k, seed, C, prior)
    res, g = O.loss_grads_1layer(P, x, eps, beta, obj, y=y)
    m = _model(1, nh, nl, xd, precision="fp32", cond_dim=C, cond_prior=prior)
    m.set_params(O.flatten_params(P))
    m.set_condition(y)
    r = m.forward_backward(x, k, beta, obj, eps=eps, want=("lpxz", "lqzx", "lpz", "logits"))
    flat = m.get_grads()
    errs = _grad_rel_errors(flat, g)
    _report("conditional float32 (%d, %d, %d) C%d prior %d B%d k%d" % (nh, nl, xd, C, prior, B, k),
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


# ---------------------------------------------------------------- 6. the device's own noise
def device_noise_step(B, k, nh, nl, xd, obj, seed):
    """The assertions of test_gpu_parity.py::test_device_noise_step_matches_oracle_on_the_same_draws: Philox gives four normals per
    call, so at D % 4 != 0 the last call's tail is dropped (a width-5 draw is the first 5 columns of the width-8 draw)."""
    step = 9
    x, P, _ = MG.inputs(1, nh, nl, xd, B, 1, seed)
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


def device_noise_matches_philox(nh, nl, xd):
    """iwae_debug_eps against the NumPy restatement (fast v_log / v_sin / v_cos: abs err <= 2e-5), the batch offset, and the forward pass
    consuming exactly these draws -- as test_gpu_parity.py::test_device_noise_matches_published_philox does at width 100."""
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
def eval_llh_per_image(layers, shape, k, seed):
    """iwae_eval_llh (main.py:170-184) on 5 images, both evaluator precisions, per image against the exact float64 oracle on the device's
    Philox draws (image i: rows i * k .. of streams 0 / 1): float32 evaluator <= 5e-3 nat, bf16 evaluator <= 0.1 nat (the bounds of
    test_trained_model_k5000_llh_within_north_star_tolerance)."""
    nh, nl, xd = shape
    n, step = 5, 999
    x, P, _ = MG.inputs(layers, nh, nl, xd, n, 1, seed)
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


def decode_matches_oracle(shape):
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
def three_adam_steps(shape, B, k):
    """The loop of test_training_reduces_loss_and_matches_oracle_trajectory: each step reads the bf16 weight images the previous step's
    update wrote -- a misplaced image chunk shows from step 2 on."""
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
