"""The masked float32 train step (iwae_forward_masked / iwae_forward_backward_masked / iwae_train_step_masked, include/iwae_amd.h;
DESIGN.md section 19) against tests/_masked_ref.py, the float64 torch-autograd restatement that tests/test_masked_host.py ties to the
committed oracles.

Tolerances are the float32 mode's own (tests/_parity_common.py), used as test_float32_mode_matches_exact_oracle uses them: per-row
densities F32_ROW_ATOL, scalars F32_SCALAR_REL (+ 2e-4), every gradient tensor F32_GRAD_REL, Adam from the device gradient 2e-6.  The two
routes of the output layer against each other at the bounds of test_float32_mode_fused_output_layer_matches_exact_oracle (scalars 2e-6
relative, gradient norm 1e-5).  Every (B, k) case runs on the general route (option no_masked_out_fused) and, where the shape lets it, on
the fast route forced with masked_out_min_rows = 1.  One handle per (shape, route) for the whole module; every test resets what it reads.
Which route a call took is read off the launch count of masked_out_f32_kernel (_witnessed: iwae_kernel_time "masked_out"): more than 0 on
every "fast" call, 0 on every "general" one, and at the default options 0 below 25 600 rows.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from oracle import iwae_np as O
import _masked_ref as MR
from _parity_common import F32_SCALAR_REL, F32_GRAD_REL, F32_ROW_ATOL, _grad_rel_errors

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
SCALARS = ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14")
ROWS = ("lpxz", "lpz", "lqzx", "log_w", "al", "z")
SHAPE_ROUTES = [(s, r) for s in MR.SHAPES for r in ("general", "fast") if r == "general" or s in MR.FAST_SHAPES]
_handles = {}


def _model(shape, route):
    """The module's handle of a shape on a route ("general", "fast", "default"): float32, 1-layer."""
    if (shape, route) not in _handles:
        from iwae_amd.native import NativeModel
        nh, nl, xd = shape
        _handles[(shape, route)] = NativeModel(1, nh, nl, x_dim=xd, seed=123, precision="fp32", options=MR.ROUTES.get(route, {}))
    return _handles[(shape, route)]


def _reset(m, P):
    m.set_params(O.flatten_params(P))
    m.set_adam_state(np.zeros(m.n_params, np.float32), np.zeros(m.n_params, np.float32), 0)
    m.set_step(0, 0)


def _witnessed(m, route, rows, call):
    """call() with the launch count of masked_out_f32_kernel held to what the route's name promises (MR.expected_on_fast_route)."""
    out, launches = MR.masked_out_launches(m, call)
    MR.expected_on_fast_route(route, launches, rows)
    return out


@functools.lru_cache(maxsize=None)
def _run(shape, case, route, obj, beta=1.0):
    """(result dict, flat gradient) of iwae_forward_backward_masked on a case, once per (shape, case, route, objective)."""
    x, P, eps, mask = MR.case(*shape, *case)
    m = _model(shape, route)
    _reset(m, P)
    r = _witnessed(m, route, case[0] * case[1], lambda: m.forward_backward(x, case[1], beta, obj, eps=eps, want=ROWS, mask=mask))
    return r, m.get_grads().copy()


def _check_parity(shape, case, route, obj, beta=1.0):
    x, P, eps, mask = MR.case(*shape, *case)
    B, k = case
    res, g = MR.reference(*shape, B, k, obj, beta)
    r, flat = _run(shape, case, route, obj, beta)
    for a in ("lpxz", "lpz", "lqzx", "log_w"):
        assert np.max(np.abs(r[a] - res[a])) < F32_ROW_ATOL, (a, float(np.max(np.abs(r[a] - res[a]))))
    np.testing.assert_allclose(r["z"], res["z"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(r["al"], res["al"], atol=2e-4)
    for key in (("iwae_elbo",) if obj == "dreg" else SCALARS):
        assert abs(r[key] - res[key]) <= F32_SCALAR_REL * abs(res[key]) + 2e-4, (key, r[key], res[key])
    assert abs(r["mean_lpxz"] - res["lpxz"].mean()) <= F32_SCALAR_REL * abs(res["lpxz"].mean()) + 2e-4, (r["mean_lpxz"], res["lpxz"].mean())
    errs = _grad_rel_errors(flat, g)
    assert max(errs) < F32_GRAD_REL, errs
    # an image with nothing observed: log p(x_obs|z) = 0 exactly, log_w = log p(z) - log q(z|x) (at most three float32 roundings of terms of that size)
    for b in np.flatnonzero(mask.sum(axis=1) == 0):
        assert np.all(r["lpxz"][:, b] == 0.0)
        d = (r["lpz"][:, b].astype(np.float64) - r["lqzx"][:, b].astype(np.float64)) * beta
        ulp = 2.0 ** -23 * max(1.0, float(np.max(np.abs(r["lpz"][:, b]))), float(np.max(np.abs(r["lqzx"][:, b]))))
        assert np.max(np.abs(r["log_w"][:, b] - d)) <= 4 * ulp
    return r, flat


# ---------------------------------------------------------------- 1. parity with the restatement, both routes
@pytest.mark.parametrize("case", MR.CASES, ids=lambda c: "B%d_k%d" % c)
@pytest.mark.parametrize("shape,route", SHAPE_ROUTES, ids=lambda v: v if isinstance(v, str) else "%d_%d_%d" % v)
def test_masked_step_matches_the_restatement(gpu, shape, route, case):
    x, P, eps, mask = MR.case(*shape, *case)
    for obj in MR.OBJECTIVES:
        r, flat = _check_parity(shape, case, route, obj)
    # the forward-only call agrees with the training call; iwae_train_step_masked = Keras Adam of the device gradient
    m = _model(shape, route)
    _reset(m, P)
    obj = MR.OBJECTIVES[-1]
    r0 = _witnessed(m, route, case[0] * case[1], lambda: m.forward(x, case[1], 1.0, eps=eps, want=("lpxz",), mask=mask))
    np.testing.assert_allclose(r0["lpxz"], r["lpxz"], rtol=1e-6, atol=1e-4)
    assert abs(r0["iwae_elbo"] - r["iwae_elbo"]) <= 1e-6 * abs(r["iwae_elbo"]) + 1e-5
    _witnessed(m, route, case[0] * case[1], lambda: m.train_step(x, case[1], 1.0, 1e-3, obj, eps=eps, mask=mask))
    g2 = m.get_grads().astype(np.float64)
    assert np.linalg.norm(g2 - flat) / np.linalg.norm(flat) < 1e-5
    ref, _, _ = O.adam_update(O.flatten_params(P), flat.astype(np.float64), 0.0, 0.0, 1, 1e-3)
    assert np.max(np.abs(m.get_params() - ref)) < 2e-6


@pytest.mark.parametrize("route", ["general", "fast"])
def test_masked_vae_elbo_kl_at_beta(gpu, route):
    """IWAE_OBJ_VAE_ELBO_KL uses the masked mean of log p(x_obs|z); beta 0.7."""
    _check_parity(MR.SHAPES[0], (5, 13), route, "vae_elbo_kl", 0.7)


@pytest.mark.parametrize("case", MR.BIG_CASES, ids=lambda c: "B%d_k%d" % c)
def test_masked_step_at_training_row_counts_default_options(gpu, case):
    """4 100, 10 000 and 25 600 rows at the default options (row-split weight gradients on the side stream, the route the defaults pick: the
    general one at the first two, masked_out_f32_kernel at the third: _run holds the launch count to 0, 0 and more than 0)."""
    _check_parity(MR.SHAPES[0], case, "default", "iwae_elbo")


# ---------------------------------------------------------------- 2. the two routes against each other
@pytest.mark.parametrize("case", MR.CASES, ids=lambda c: "B%d_k%d" % c)
@pytest.mark.parametrize("shape", MR.FAST_SHAPES, ids=lambda s: "%d_%d_%d" % s)
def test_general_and_fast_route_agree(gpu, shape, case):
    """Scalars within 2e-6 relative, the gradient norm within 1e-5 (the test prints every figure).  masked_out_f32_kernel forms the general
    route's float32 numbers in the general route's order, so the figures are 0; with dec_fwd_f32_kernel's epilogue, which rounds log_w one
    or two float32 spacings elsewhere, the importance-weighted gradients at 208 / 128 / 800 differed by up to 3.4e-5."""
    figures = {}
    for obj in MR.OBJECTIVES:
        (r1, g1), (r2, g2) = _run(shape, case, "general", obj), _run(shape, case, "fast", obj)
        for key in (("iwae_elbo",) if obj == "dreg" else SCALARS):
            assert abs(r1[key] - r2[key]) <= 2e-6 * abs(r2[key]), (obj, key, r1[key], r2[key])
        g1, g2 = g1.astype(np.float64), g2.astype(np.float64)
        figures[obj] = np.linalg.norm(g1 - g2) / np.linalg.norm(g2)
        print("routes %s B%d k%d %s: gradient %.3g, max |d log_w| %.3g (float32 spacing at max |log_w| %.3g)"
              % (shape, case[0], case[1], obj, figures[obj], float(np.max(np.abs(r1["log_w"] - r2["log_w"]))),
                 float(np.spacing(np.float32(np.max(np.abs(r2["log_w"])))))))
    for obj in MR.OBJECTIVES:
        assert figures[obj] < 1e-5, (obj, figures)


# ---------------------------------------------------------------- 3. unobserved pixels are never read
def _step_state(m, P, x, mask, eps, k, obj, route):
    _reset(m, P)
    r = _witnessed(m, route, x.shape[0] * k, lambda: m.train_step(x, k, 1.0, 1e-3, obj, eps=eps, want=("log_w", "lpxz"), mask=mask))
    mo, ve, t = m.get_adam_state()
    return r, m.get_grads().copy(), m.get_params().copy(), mo, ve, t


@pytest.mark.parametrize("fill", [np.nan, 1e30], ids=["nan", "1e30"])
@pytest.mark.parametrize("shape,route", SHAPE_ROUTES, ids=lambda v: v if isinstance(v, str) else "%d_%d_%d" % v)
def test_unobserved_pixels_are_never_read(gpu, shape, route, fill):
    x, P, eps, mask = MR.case(*shape, 5, 13)
    xf = np.where(mask != 0, x, np.float32(fill)).astype(np.float32)
    assert (xf != x).any() or np.isnan(xf).any()
    m = _model(shape, route)
    for obj in ("iwae_elbo", "dreg"):
        a, b = _step_state(m, P, x, mask, eps, 13, obj, route), _step_state(m, P, xf, mask, eps, 13, obj, route)
        for key in a[0]:
            np.testing.assert_array_equal(np.asarray(a[0][key]), np.asarray(b[0][key]), err_msg=key)
        for u, v in zip(a[1:5], b[1:5]):
            assert np.all(np.isfinite(u))
            np.testing.assert_array_equal(u, v)
        assert a[5] == b[5] == 1


# ---------------------------------------------------------------- 4. no mask, a mask of ones
def _raw_train(m, x, mask_ptr, k, eps, obj_id):
    from iwae_amd._capi import Scalars
    s = Scalars()
    rc = m.lib.iwae_train_step_masked(m.h, x.ctypes.data, mask_ptr, x.shape[0], k, 1.0, 1e-3, obj_id, eps.ctypes.data, C.byref(s), None)
    assert rc == 0
    return {n: float(getattr(s, n)) for n in SCALARS}


@pytest.mark.parametrize("shape,route", SHAPE_ROUTES, ids=lambda v: v if isinstance(v, str) else "%d_%d_%d" % v)
def test_null_mask_is_the_unmasked_call_and_a_mask_of_ones_agrees_with_it(gpu, shape, route):
    """mask = NULL: bitwise the unmasked call.  A mask of ones: the unmasked call within the route-against-route bounds (the test prints
    the figure; log p(x|z) is bern_f32_kernel's term in its order on both routes)."""
    from iwae_amd.native import OBJECTIVES
    x, P, eps, _ = MR.case(*shape, 5, 13)
    x, eps = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(eps, np.float32)
    m = _model(shape, route)
    _reset(m, P)
    r_un = m.train_step(x, 13, 1.0, 1e-3, "iwae_elbo", eps=eps)
    g_un, p_un = m.get_grads().copy(), m.get_params().copy()
    _reset(m, P)
    r_null = _raw_train(m, x, None, 13, eps, OBJECTIVES["iwae_elbo"])
    for key in SCALARS:
        assert r_null[key] == r_un[key], key
    np.testing.assert_array_equal(m.get_grads(), g_un)
    np.testing.assert_array_equal(m.get_params(), p_un)
    _reset(m, P)
    r_one = _witnessed(m, route, 65, lambda: m.train_step(x, 13, 1.0, 1e-3, "iwae_elbo", eps=eps, mask=np.ones(x.shape, np.uint8)))
    for key in SCALARS:
        assert abs(r_one[key] - r_un[key]) <= 2e-6 * abs(r_un[key]), (key, r_one[key], r_un[key])
    g1 = m.get_grads().astype(np.float64)
    d = np.linalg.norm(g1 - g_un) / np.linalg.norm(g_un)
    print("ones %s %s: gradient %.3g" % (shape, route, d))
    assert d < 1e-5


# ---------------------------------------------------------------- 5. the same weights as iwae_impute's
@pytest.mark.parametrize("shape,route", [(s, r) for s, r in SHAPE_ROUTES if s[0] <= 208 and s[1] <= 128],
                         ids=lambda v: v if isinstance(v, str) else "%d_%d_%d" % v)
def test_log_w_gives_iwae_imputes_bound(gpu, shape, route):
    """LSE_s log_w - log k per image (float64 on the host) against iwae_impute's log_px on the same x, mask and draws: 1e-4, the bound
    tests/test_gpu_impute.py holds the same claim against the evaluator to."""
    B, k = 5, 13
    x, P, eps, mask = MR.case(*shape, B, k)
    m = _model(shape, route)
    _reset(m, P)
    lw = _witnessed(m, route, B * k, lambda: m.forward(x, k, 1.0, eps=eps, want=("log_w",), mask=mask))["log_w"].astype(np.float64)
    mx = lw.max(axis=0)
    lpx = mx + np.log(np.mean(np.exp(lw - mx[None]), axis=0))
    got = m.impute(x, mask=mask, n_samples=k, noise=eps, outputs=("log_px",))["log_px"]
    assert np.max(np.abs(lpx - got)) < 1e-4, (lpx, got)


# ---------------------------------------------------------------- 6. repeatability
@pytest.mark.parametrize("shape,route", SHAPE_ROUTES, ids=lambda v: v if isinstance(v, str) else "%d_%d_%d" % v)
def test_three_masked_steps_on_device_noise_repeat_bitwise(gpu, shape, route):
    x, P, _, mask = MR.case(*shape, 5, 13)
    m = _model(shape, route)
    outs = []
    for _ in range(2):
        _reset(m, P)
        rs = _witnessed(m, route, 65, lambda: [m.train_step(x, 13, 1.0, 1e-3, "iwae_elbo", mask=mask)["iwae_elbo"] for _ in range(3)])
        outs.append((rs, m.get_params().copy(), m.get_adam_state(), m.get_grads().copy()))
    assert outs[0][0] == outs[1][0] and np.all(np.isfinite(outs[0][0])) and len(set(outs[0][0])) == 3
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    np.testing.assert_array_equal(outs[0][2][0], outs[1][2][0])
    np.testing.assert_array_equal(outs[0][2][1], outs[1][2][1])
    np.testing.assert_array_equal(outs[0][3], outs[1][3])
    assert outs[0][2][2] == 3


# ---------------------------------------------------------------- 7. rejected calls
def _masked_calls(m, x, mask, B, k, want=None):
    """The three entry points' return codes for one argument set (raw binding: x / mask may be None)."""
    from iwae_amd._capi import Scalars
    s = Scalars()
    xp = None if x is None else x.ctypes.data
    mp = mask.ctypes.data
    w = None if want is None else C.byref(want)
    return (m.lib.iwae_forward_masked(m.h, xp, mp, B, k, 1.0, None, C.byref(s), w),
            m.lib.iwae_forward_backward_masked(m.h, xp, mp, B, k, 1.0, 1, None, C.byref(s), w),
            m.lib.iwae_train_step_masked(m.h, xp, mp, B, k, 1.0, 1e-3, 1, None, C.byref(s), w))


def _state(m):
    mo, ve, t = m.get_adam_state()
    return m.get_params().copy(), m.get_grads().copy(), mo, ve, t


def _same_state(a, b):
    for u, v in zip(a[:4], b[:4]):
        np.testing.assert_array_equal(u, v)
    assert a[4] == b[4]


def test_rejected_arguments_leave_the_handle_untouched(gpu):
    from iwae_amd.native import NativeModel
    from iwae_amd._capi import Tensors
    shape = MR.SHAPES[1]
    nh, nl, xd = shape
    x, P, eps, mask = MR.case(*shape, 5, 13)
    x = np.ascontiguousarray(x, np.float32)
    m = _model(shape, "general")
    _reset(m, P)
    m.train_step(x, 13, 1.0, 1e-3, "iwae_elbo", mask=mask)          # (a gradient and Adam moments to be left alone)
    m.set_step(7, 0)
    before = _state(m)
    expect = m.forward(x, 13, 1.0, mask=mask)                        # device noise at step 7
    m.set_step(7, 0)
    logits = np.empty((13, 5, xd), np.float32)
    t = Tensors()
    t.logits = logits.ctypes.data
    for args in ((x, mask, 0, 13), (x, mask, -1, 13), (x, mask, 5, 0), (x, mask, 5, -3), (None, mask, 5, 13)):
        assert _masked_calls(m, *args) == (ERR_ARG,) * 3, args
    assert _masked_calls(m, x, mask, 5, 13, want=t) == (ERR_ARG,) * 3
    _same_state(before, _state(m))
    again = m.forward(x, 13, 1.0, mask=mask)                         # the noise step is still 7
    for key in SCALARS:
        assert again[key] == expect[key]
    with pytest.raises(ValueError):
        m.train_step(x, 13, 1.0, 1e-3, "iwae_elbo", mask=mask[:, :-1])
    # a handle with communicators
    m.comm_init(NativeModel.comm_unique_id(), 1, 0)
    try:
        before = _state(m)
        assert _masked_calls(m, x, mask, 5, 13) == (ERR_ARG,) * 3
        _same_state(before, _state(m))
    finally:
        m.comm_destroy()
    # handles outside the scope: bf16, 2-layer, conditional
    for kw in (dict(n_layers=1, n_hidden=nh, n_latent=nl, precision="bf16"), dict(n_layers=2, n_hidden=[nh, 8], n_latent=[nl, 2], precision="fp32"),
               dict(n_layers=1, n_hidden=nh, n_latent=nl, precision="fp32", cond_dim=3)):
        o = NativeModel(x_dim=xd, seed=123, **kw)
        try:
            p0, (m0, v0, t0) = o.get_params().copy(), o.get_adam_state()
            assert _masked_calls(o, x, mask, 5, 13) == (ERR_ARG,) * 3, kw
            np.testing.assert_array_equal(o.get_params(), p0)
            m1, v1, t1 = o.get_adam_state()
            np.testing.assert_array_equal(m1, m0)
            np.testing.assert_array_equal(v1, v0)
            assert t1 == t0
        finally:
            o.close()


# ---------------------------------------------------------------- 8. the shim and the driver
def test_shim_passes_the_mask_through(gpu):
    from iwae_amd import iwae1, iwae2
    from iwae_amd.optimizers import Adam
    shape = MR.SHAPES[1]
    nh, nl, xd = shape
    x, P, eps, mask = MR.case(*shape, 5, 13)
    res, _ = MR.reference(*shape, 5, 13, "iwae_elbo")
    model = iwae1.IWAE(nh, nl, x_dim=xd, precision="fp32")
    model._net.set_params(O.flatten_params(P))
    opt = Adam(1e-3, epsilon=1e-4)
    v = model.val_step(x, 13, 1.0, mask=mask)
    assert np.isfinite(float(v["iwae_elbo"]))
    r = model.train_step(x, 13, 1.0, opt, objective="iwae_elbo", eps=eps, mask=mask)
    assert abs(float(r["iwae_elbo"]) - res["iwae_elbo"]) <= F32_SCALAR_REL * abs(res["iwae_elbo"]) + 2e-4
    assert opt.iterations == 1
    r2 = model(x, 13, 1.0, eps=eps, mask=mask)
    assert float(r2["iwae_elbo"]) != float(r["iwae_elbo"])          # (the step moved the weights)
    with pytest.raises(ValueError):
        model.train_step(x, 13, 1.0, opt, objective="iwae_elbo", mask=mask[:2])
    two = iwae2.IWAE([nh, 8], [nl, 2], x_dim=xd, precision="fp32")
    with pytest.raises(ValueError):
        two.train_step(x, 13, 1.0, opt, objective="iwae_elbo", mask=mask)
    with pytest.raises(ValueError):
        two(x, 13, 1.0, mask=mask)


def test_miwae_driver_trains_on_incomplete_images(gpu, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tasks"))
    try:
        import miwae
    finally:
        sys.path.pop(0)
    out = miwae.main(["--images", "64", "--test-images", "32", "--steps", "40", "--batch_size", "16", "--n_samples", "5", "--draws", "8"])
    assert set(out) == {"masked", "zero_filled"}
    for row in out.values():
        assert np.all(np.isfinite(row["trace"])) and len(row["trace"]) == 40
        assert np.isfinite(row["log_px"]) and np.isfinite(row["cross_entropy"]) and 0.0 <= row["abs_error"] <= 1.0
    tr = out["masked"]["trace"]
    assert np.mean(tr[-5:]) > np.mean(tr[:5])                        # the masked bound rises over the steps
    assert "log_px_obs" in capsys.readouterr().out
