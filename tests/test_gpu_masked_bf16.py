"""The masked train step on bf16 handles (iwae_forward_masked / iwae_forward_backward_masked / iwae_train_step_masked, include/iwae_amd.h;
DESIGN.md section 20) against the two references of tests/_masked_bf16_cases.py, whose admissibility tests/test_masked_bf16_host.py shows
on the CPU.

Tolerances are the bf16 mode's own (tests/_parity_common.py), used as test_train_step_1layer_matches_oracle uses them: per-row densities
against the oracle at the device's own encoder head EMU_ROW_ATOL, scalars EMU_SCALAR_ATOL, every gradient tensor EMU_GRAD_REL against the
rounding-aware oracle and EXACT_GRAD_REL against the exact one, Adam from the device gradient 2e-6.  A mask of ones against an unmasked
handle on the same plan (options no_bern_pipe + no_out_in_block): array_equal -- a live pixel runs the same instruction sequence.  One
handle per (shape, options) for the whole module; every test resets what it reads.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import iwae_np as O
import _masked_bf16_cases as BC
import _masked_cases as MC
import _masked_ref as MR
from _parity_common import EMU_GRAD_REL, EMU_ROW_ATOL, EMU_SCALAR_ATOL, EXACT_GRAD_REL, EXACT_SCALAR_ATOL, _grad_rel_errors

pytestmark = pytest.mark.gpu

ERR_ARG = -1
SCALARS = ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14")
ROWS = ("lpxz", "lpz", "lqzx", "log_w")
SAME_PLAN = (("no_bern_pipe", 1), ("no_out_in_block", 1))          # the plan a masked call takes, on an unmasked handle
_handles = {}


def _ids(v):
    return "%d_%d_%d" % v if isinstance(v, tuple) and len(v) == 3 else "B%d_k%d" % v if isinstance(v, tuple) else str(v)


def _new(shape, options=(), **kw):
    from iwae_amd.native import NativeModel
    nh, nl, xd = shape
    kw.setdefault("precision", "bf16")
    return NativeModel(kw.pop("n_layers", 1), kw.pop("n_hidden", nh), kw.pop("n_latent", nl), x_dim=xd, seed=123, options=dict(options), **kw)


def _model(shape, options=()):
    """The module's bf16 1-layer handle of a shape under a tuple of options."""
    if (shape, options) not in _handles:
        _handles[(shape, options)] = _new(shape, options)
    return _handles[(shape, options)]


def _reset(m, P, step=0):
    m.set_params(O.flatten_params(P))
    m.set_adam_state(np.zeros(m.n_params, np.float32), np.zeros(m.n_params, np.float32), 0)
    m.set_step(step, 0)


def _state(m):
    mo, ve, t = m.get_adam_state()
    return m.get_params().copy(), mo, ve, t


def _same_state(a, b):
    for u, v in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(u, v)
    assert a[3] == b[3]


# ---------------------------------------------------------------- 1. parity with the two references
def _check_parity(shape, bk, obj, beta=1.0):
    x, P, eps, mask = BC.case(shape, bk)
    B, k = bk
    res_x, g_x = BC.exact(shape, bk, obj, beta)
    res_e, g_e = BC.emulated(shape, bk, obj, beta)
    m = _model(shape)
    _reset(m, P)
    r = m.forward_backward(x, k, beta, obj, eps=eps, want=ROWS, mask=mask)
    flat = m.get_grads().copy()
    at = BC.densities_at_device_head(m, P, x, mask, eps, shape[1], beta)
    figs = {a: float(np.max(np.abs(r[a] - at[a]))) for a in ROWS}
    key = "iwae_elbo" if obj == "dreg" else obj
    d_e, d_x = abs(r[key] - res_e["value"]), abs(r[key] - BC.exact_value(res_x, obj))
    errs_e, errs_x = _grad_rel_errors(flat, g_e), _grad_rel_errors(flat, g_x)
    print("%s B%d k%d %s: rows at the device head %s (< %.3g); %s %.4g vs rounding-aware %.3g (< %.3g), vs exact %.3g (< %.3g); "
          "gradient per tensor vs rounding-aware %.3g (< %.3g), vs exact %.3g (< %.3g)"
          % (shape, B, k, obj, {a: "%.3g" % v for a, v in figs.items()}, EMU_ROW_ATOL, key, r[key], d_e, EMU_SCALAR_ATOL, d_x, EXACT_SCALAR_ATOL,
             max(errs_e), EMU_GRAD_REL, max(errs_x), EXACT_GRAD_REL))
    for a in ROWS:
        assert figs[a] < EMU_ROW_ATOL, (a, figs[a])
    assert d_e < EMU_SCALAR_ATOL, (key, r[key], res_e["value"])
    assert d_x < EXACT_SCALAR_ATOL, (key, r[key], BC.exact_value(res_x, obj))
    assert abs(r["mean_lpxz"] - float(np.mean(r["lpxz"].astype(np.float64)))) < 1e-3
    assert max(errs_e) < EMU_GRAD_REL, errs_e
    assert max(errs_x) < EXACT_GRAD_REL, errs_x
    return r, flat


@pytest.mark.parametrize("bk", BC.CASES, ids=_ids)
@pytest.mark.parametrize("shape", BC.DIMS, ids=_ids)
def test_masked_bf16_step_matches_the_references(gpu, shape, bk):
    x, P, eps, mask = BC.case(shape, bk)
    for obj in BC.OBJECTIVES:
        r, flat = _check_parity(shape, bk, obj)
    # the forward-only call agrees with the training call; iwae_train_step_masked = Keras Adam of the device gradient
    m = _model(shape)
    _reset(m, P)
    obj = BC.OBJECTIVES[-1]
    r0 = m.forward(x, bk[1], 1.0, eps=eps, want=("lpxz",), mask=mask)
    np.testing.assert_allclose(r0["lpxz"], r["lpxz"], rtol=1e-6, atol=1e-4)
    assert abs(r0["iwae_elbo"] - r["iwae_elbo"]) <= 1e-6 * abs(r["iwae_elbo"]) + 1e-5
    m.train_step(x, bk[1], 1.0, 1e-3, obj, eps=eps, mask=mask)
    g2 = m.get_grads().astype(np.float64)
    assert np.linalg.norm(g2 - flat) / np.linalg.norm(flat) < 1e-5
    ref, _, _ = O.adam_update(O.flatten_params(P), flat.astype(np.float64), 0.0, 0.0, 1, 1e-3)
    assert np.max(np.abs(m.get_params() - ref)) < 2e-6


def test_masked_bf16_vae_elbo_kl_at_beta(gpu):
    """IWAE_OBJ_VAE_ELBO_KL uses the masked mean of log p(x_obs|z); beta 0.7."""
    _check_parity(BC.WIDE, (5, 13), "vae_elbo_kl", 0.7)


@pytest.mark.parametrize("obj", BC.BIG_OBJECTIVES)
@pytest.mark.parametrize("bk", BC.BIG_CASES, ids=_ids)
def test_masked_bf16_step_at_training_row_counts(gpu, bk, obj):
    """4 100 and 10 000 rows at 200 / 100 / 784: either side of 8 192 rows the plan goes from per-pixel-group partial sums to whole rows,
    from sample_kernel to dense_kernel's sampled-input mode (iwae_elbo; DReG keeps sample_kernel) and from the 4-wave to the 8-wave shape of
    the hole-aware output layer.  (The block kernels and dec_bwd_rows_kernel are the small cases' path.)"""
    _check_parity(BC.WIDE, bk, obj)


# ---------------------------------------------------------------- 2. selected, never multiplied
def _step_state(m, P, x, mask, eps, k, obj):
    _reset(m, P)
    r = m.train_step(x, k, 1.0, 1e-3, obj, eps=eps, want=("log_w", "lpxz", "lpz", "lqzx"), mask=mask)
    mo, ve, t = m.get_adam_state()
    return r, m.get_grads().copy(), m.get_params().copy(), mo, ve, t


@pytest.mark.parametrize("fill", [np.nan, 1e30], ids=["nan", "1e30"])
@pytest.mark.parametrize("shape", BC.DIMS, ids=_ids)
def test_unobserved_pixels_are_never_read(gpu, shape, fill):
    """NaN / 1e30 at the unobserved pixels: every output is bitwise the clean call's.  The mask (case_mask with the first half of the pixels
    cleared) has an empty image and pixel columns no image observes: log p(x_obs|z) == 0 exactly there, the W3 / b3 gradient exactly 0 here."""
    B, k = 5, 13
    x, P, eps, _ = MR.case(*shape, B, k)
    mask = MC.mask_tophalf(B, shape[2], 17 + B + k)
    nv = MC.never_observed(mask)
    empty = np.flatnonzero(mask.sum(axis=1) == 0)
    assert nv.size and empty.size
    xf = np.where(mask != 0, x, np.float32(fill)).astype(np.float32)
    m = _model(shape)
    sl = MC.tensor_slices(P)
    for obj in ("iwae_elbo", "dreg"):
        a, b = _step_state(m, P, x, mask, eps, k, obj), _step_state(m, P, xf, mask, eps, k, obj)
        for key in a[0]:
            np.testing.assert_array_equal(np.asarray(a[0][key]), np.asarray(b[0][key]), err_msg=key)
        for u, v in zip(a[1:5], b[1:5]):
            assert np.all(np.isfinite(u))
            np.testing.assert_array_equal(u, v)
        assert a[5] == b[5] == 1
        g = b[1]
        dW3, db3 = g[sl[12][0]:sl[12][1]].reshape(P[6][0].shape), g[sl[13][0]:sl[13][1]]
        assert np.all(dW3[:, nv] == 0.0) and np.all(db3[nv] == 0.0)
        assert np.any(dW3 != 0.0)
        r = b[0]
        for e in empty:
            assert np.all(r["lpxz"][:, e] == 0.0)
            d = r["lpz"][:, e].astype(np.float64) - r["lqzx"][:, e].astype(np.float64)
            ulp = 2.0 ** -23 * max(1.0, float(np.max(np.abs(r["lpz"][:, e]))), float(np.max(np.abs(r["lqzx"][:, e]))))
            assert np.max(np.abs(r["log_w"][:, e] - d)) <= 4 * ulp


# ---------------------------------------------------------------- 3. a mask of ones, no mask
@pytest.mark.parametrize("shape,bk", [(s, (5, 13)) for s in BC.DIMS] + [(BC.WIDE, (200, 50))], ids=_ids)
def test_a_mask_of_ones_is_the_unmasked_step_on_the_same_plan(gpu, shape, bk):
    B, k = bk
    x, P, eps, _ = MR.case(*shape, B, k)
    ones = np.ones(x.shape, np.uint8)
    un, mk = _model(shape, SAME_PLAN), _model(shape)
    out = []
    for m, mask in ((un, None), (mk, ones)):
        _reset(m, P)
        r = m.train_step(x, k, 1.0, 1e-3, "iwae_elbo", eps=eps, want=("lpxz",), mask=mask)
        out.append((r, m.get_grads().copy(), m.get_params().copy()))
    (r_un, g_un, p_un), (r_mk, g_mk, p_mk) = out
    print("ones %s B%d k%d: max |d lpxz| %.3g, gradient %.3g" % (shape, B, k, float(np.max(np.abs(r_un["lpxz"] - r_mk["lpxz"]))),
                                                                  np.linalg.norm(g_un.astype(np.float64) - g_mk) / np.linalg.norm(g_un.astype(np.float64))))
    np.testing.assert_array_equal(r_mk["lpxz"], r_un["lpxz"])
    for key in SCALARS:
        assert r_mk[key] == r_un[key], key
    np.testing.assert_array_equal(g_mk, g_un)
    np.testing.assert_array_equal(p_mk, p_un)


def _raw_train(m, x, mask_ptr, k, eps, obj_id):
    from iwae_amd._capi import Scalars
    s = Scalars()
    rc = m.lib.iwae_train_step_masked(m.h, x.ctypes.data, mask_ptr, x.shape[0], k, 1.0, 1e-3, obj_id, eps.ctypes.data, C.byref(s), None)
    assert rc == 0
    return {n: float(getattr(s, n)) for n in SCALARS}


@pytest.mark.parametrize("shape", BC.DIMS[:1] + BC.DIMS[3:4], ids=_ids)
def test_null_mask_is_the_unmasked_call(gpu, shape):
    """mask = NULL at the default options: bitwise iwae_train_step (bern_pipe_kernel / block_fwd_kernel<.., OUT> included)."""
    from iwae_amd.native import OBJECTIVES
    x, P, eps, _ = MR.case(*shape, 5, 13)
    x, eps = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(eps, np.float32)
    m = _model(shape)
    _reset(m, P)
    r_un = m.train_step(x, 13, 1.0, 1e-3, "iwae_elbo", eps=eps)
    g_un, p_un = m.get_grads().copy(), m.get_params().copy()
    _reset(m, P)
    r_null = _raw_train(m, x, None, 13, eps, OBJECTIVES["iwae_elbo"])
    for key in SCALARS:
        assert r_null[key] == r_un[key], key
    np.testing.assert_array_equal(m.get_grads(), g_un)
    np.testing.assert_array_equal(m.get_params(), p_un)


# ---------------------------------------------------------------- 4. state across calls
def test_three_masked_steps_on_device_noise_repeat_bitwise(gpu):
    shape = BC.WIDE
    x, P, _, mask = MR.case(*shape, 5, 13)
    m = _model(shape)
    outs = []
    for _ in range(2):
        _reset(m, P)
        rs = [m.train_step(x, 13, 1.0, 1e-3, "iwae_elbo", mask=mask)["iwae_elbo"] for _ in range(3)]
        outs.append((rs, _state(m), m.get_grads().copy()))
    assert outs[0][0] == outs[1][0] and np.all(np.isfinite(outs[0][0])) and len(set(outs[0][0])) == 3
    _same_state(outs[0][1], outs[1][1])
    np.testing.assert_array_equal(outs[0][2], outs[1][2])
    assert outs[0][1][3] == 3


@pytest.mark.parametrize("bk", [(20, 5), (200, 50)], ids=_ids)
def test_masked_and_unmasked_steps_interleave_like_fresh_handles(gpu, bk):
    """masked, unmasked, masked on ONE handle, device noise: every step is bitwise the same step on a fresh handle started from the state in
    front of it (set_step aligns the noise).  (20, 5): the multi-step noise buffers; (200, 50): the speculative draw on a side stream and
    the deferred decoder update -- and between the steps the plan switches between bern_pipe_kernel / block_fwd_kernel<.., OUT> and the
    hole-aware dense_kernel."""
    shape = BC.WIDE
    B, k = bk
    x, P, _, _ = MR.case(*shape, 5, 13)
    x = np.ascontiguousarray(np.resize(x, (B, shape[2])), np.float32)
    masks = [MR.case_mask(B, shape[2], 301), None, MR.case_mask(B, shape[2], 308)]
    m = _model(shape)
    _reset(m, P, step=11)
    trail = []
    for i, mask in enumerate(masks):
        before = _state(m)
        r = m.train_step(x, k, 1.0, 1e-3, "iwae_elbo", mask=mask)
        trail.append((before, {key: r[key] for key in SCALARS}, _state(m)))
    assert trail[-1][2][3] == 3
    for i, mask in enumerate(masks):
        before, scal, after = trail[i]
        f = _new(shape)
        try:
            f.set_params(before[0])
            f.set_adam_state(before[1], before[2], before[3])
            f.set_step(11 + i, 0)
            r = f.train_step(x, k, 1.0, 1e-3, "iwae_elbo", mask=mask)
            for key in SCALARS:
                assert r[key] == scal[key], (i, key, r[key], scal[key])
            _same_state(_state(f), after)
        finally:
            f.close()


# ---------------------------------------------------------------- 5. refusals leave the handle untouched
def _masked_calls(m, x, mask, B, k, want=None):
    """The three entry points' return codes for one argument set (raw binding)."""
    from iwae_amd._capi import Scalars
    s = Scalars()
    w = None if want is None else C.byref(want)
    return (m.lib.iwae_forward_masked(m.h, x.ctypes.data, mask.ctypes.data, B, k, 1.0, None, C.byref(s), w),
            m.lib.iwae_forward_backward_masked(m.h, x.ctypes.data, mask.ctypes.data, B, k, 1.0, 1, None, C.byref(s), w),
            m.lib.iwae_train_step_masked(m.h, x.ctypes.data, mask.ctypes.data, B, k, 1.0, 1e-3, 1, None, C.byref(s), w))


def _refused_untouched(m, x, mask, k, want=None, cond=None):
    """All three masked calls return IWAE_ERR_ARG; parameters, Adam state and the noise step are what they were."""
    if cond is not None:
        m.set_condition(cond)
    m.train_step(x, k, 1.0, 1e-3, "iwae_elbo")                 # (Adam moments to be left alone)
    m.set_step(7, 0)
    expect = m.forward(x, k, 1.0)                              # device noise at step 7
    m.set_step(7, 0)
    before = _state(m)
    assert _masked_calls(m, x, mask, x.shape[0], k, want) == (ERR_ARG,) * 3
    _same_state(before, _state(m))
    again = m.forward(x, k, 1.0)                               # the noise step is still 7
    for key in SCALARS:
        assert again[key] == expect[key], key


@pytest.mark.parametrize("shape,kt", BC.REFUSED, ids=_ids)
def test_hidden_widths_without_a_stored_s_backward_are_refused(gpu, shape, kt):
    x, P, eps, mask = MR.case(*shape, 5, 13)
    m = _model(shape)
    _reset(m, P)
    _refused_untouched(m, np.ascontiguousarray(x, np.float32), mask, 13)


def test_out_of_scope_calls_are_refused(gpu):
    from iwae_amd._capi import Tensors
    shape = BC.DIMS[3]
    nh, nl, xd = shape
    x, P, eps, mask = MR.case(*shape, 5, 13)
    x = np.ascontiguousarray(x, np.float32)
    # the option that clears allow_s_mode
    o = _new(shape, (("out_recompute", 1),))
    try:
        o.set_params(O.flatten_params(P))
        _refused_untouched(o, x, mask, 13)
    finally:
        o.close()
    m = _model(shape)
    _reset(m, P)
    # want->logits
    t = Tensors()
    logits = np.empty((13, 5, xd), np.float32)
    t.logits = logits.ctypes.data
    _refused_untouched(m, x, mask, 13, want=t)
    # a handle with communicators
    from iwae_amd.native import NativeModel
    m.comm_init(NativeModel.comm_unique_id(), 1, 0)
    try:
        before = _state(m)
        assert _masked_calls(m, x, mask, 5, 13) == (ERR_ARG,) * 3
        _same_state(before, _state(m))
    finally:
        m.comm_destroy()
    # 2-layer and conditional bf16 handles
    for kw, cond in ((dict(n_layers=2, n_hidden=[nh, 32], n_latent=[nl, 2]), None), (dict(cond_dim=3), np.eye(3, dtype=np.float32)[np.arange(5) % 3])):
        o = _new(shape, **kw)
        try:
            _refused_untouched(o, x, mask, 13, cond=cond)
        finally:
            o.close()
    # ... and the accepted handle still takes a mask
    _reset(m, P)
    assert np.isfinite(m.train_step(x, 13, 1.0, 1e-3, "iwae_elbo", mask=mask)["iwae_elbo"])
