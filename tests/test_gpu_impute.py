"""iwae_impute (include/iwae_amd.h): the masked importance-weighted bound on log p(x_obs) and the self-normalised estimate of E[x | x_obs]
on the device (Mattei & Frellsen 2019).

The expected values are the float64 restatement of tests/_impute_ref.py on the DEVICE'S OWN q_mu, q_sigma and the noise passed in, so the
kernels are pinned independently of the encoder's precision.  Tolerances follow tests/test_gpu_local_q.py's rule, set at run time: 8 x the
largest deviation of a float32 numpy run of the same restatement from its float64 run on the same inputs, floor 1e-5.  The handles carry
SPREAD parameters (tests/_parity_common.py), so the weights over an image's draws are not one-hot (tests/test_impute_host.py checks that
from the restatement alone).  Every test runs in the float32 eval precision.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import iwae_np as O
import _impute_ref as IM
import _row_eval_bodies as RB

pytestmark = pytest.mark.gpu

KEYS = ("log_px", "xhat", "ess", "log_w", "q_mu", "q_sigma")
_cache = {}


def _net(nh, nl, xd):
    """One handle per shape for the whole module (seed-fixed spread parameters, NMAX images, a 50 % mask)."""
    key = (nh, nl, xd)
    if key not in _cache:
        from iwae_amd.native import NativeModel
        x, P, mask = IM.shape_inputs(nh, nl, xd)
        m = NativeModel(1, nh, nl, x_dim=xd, seed=123)
        m.set_params(O.flatten_params(P))
        m.set_eval_precision("fp32")
        _cache[key] = (m, x, P, mask)
    return _cache[key]


_runs = {}


def _run(nh, nl, xd, N, k):
    """The device's outputs and the two restatements at the device's heads, once per case."""
    key = (nh, nl, xd, N, k)
    if key not in _runs:
        m, x, P, mask = _net(nh, nl, xd)
        _runs[key] = RB.impute_run(m, x, P, mask, nl, N, k)
    return _runs[key]


_close = RB._close


def _same(a, b, keys=KEYS):
    RB.same(a, b, keys)


# ---------------------------------------------------------------- 1. parity of the weights
@pytest.mark.parametrize("N,k", IM.CASES, ids=IM.CASE_IDS)
@pytest.mark.parametrize("nh,nl,xd", IM.SHAPES)
def test_weight_parity(gpu, nh, nl, xd, N, k):
    RB.impute_weight_parity(_run(nh, nl, xd, N, k), N, k, xd)


# ---------------------------------------------------------------- 2. parity of the imputation
@pytest.mark.parametrize("N,k", IM.CASES, ids=IM.CASE_IDS)
@pytest.mark.parametrize("nh,nl,xd", IM.SHAPES)
def test_imputation_parity(gpu, nh, nl, xd, N, k):
    """xhat against sum_s softmax(DEVICE log_w)_s p64_s: the error of log_w (bounded above) is not charged to xhat."""
    RB.impute_imputation_parity(_run(nh, nl, xd, N, k))


def test_nothing_is_written_past_the_last_pixel(gpu):
    """x_dim = 53 (no multiple of the 16-pixel tile, nor of the 64-pixel pass): xhat into a device array with a guard row of sentinels behind
    it and a sentinel column range inside the padded width -- through the raw binding, both chunkings of the sum."""
    m, x, P, mask = _net(37, 5, 53)
    RB.impute_nothing_past_the_last_pixel(m, x, mask, 5, 53, lambda N, k: _run(37, 5, 53, N, k)[0])


# ---------------------------------------------------------------- 3. mask semantics
@pytest.mark.parametrize("N,k", [(5, 13), (2, 65)], ids=["one_chunk", "two_chunks"])
@pytest.mark.parametrize("nh,nl,xd", IM.SHAPES)
def test_unobserved_pixels_are_never_read(gpu, nh, nl, xd, N, k):
    m, x, P, mask = _net(nh, nl, xd)
    r = _run(nh, nl, xd, N, k)[0]
    xn = np.where(mask[:N], x[:N], np.float32(np.nan)).astype(np.float32)
    assert np.isnan(xn).any()
    _same(r, m.impute(xn, mask=mask[:N], n_samples=k, noise=IM.draws(N, k, nl)))


@pytest.mark.parametrize("nh,nl,xd", IM.SHAPES)
def test_no_mask_is_a_mask_of_ones_and_the_evaluator(gpu, nh, nl, xd):
    m, x, P, mask = _net(nh, nl, xd)
    N, k = 3, 7
    x = x[:N]
    m.set_step(5, 11)
    a = m.impute(x, mask=None, n_samples=k)
    m.set_step(5, 11)
    b = m.impute(x, mask=np.ones((N, xd), dtype=np.uint8), n_samples=k)
    _same(a, b)
    m.set_step(5, 11)
    _, per = m.eval_llh(x, k=k, per_image=True)
    print("log_px", a["log_px"], "eval_llh", per)
    diff = float(np.max(np.abs(a["log_px"] - per.astype(np.float64))))
    print("largest difference %.3g" % diff)
    assert diff <= 1e-4                                            # (tests/test_gpu_local_q.py's bound for the same claim)


def test_an_image_with_nothing_observed(gpu):
    m, x, P, mask = _net(64, 8, 48)
    N, k = 3, 7
    mk = mask[:N].copy()
    mk[1] = False
    eps = IM.draws(N, k, 8)
    r = m.impute(x[:N], mask=mk, n_samples=k, noise=eps)
    e64 = IM.restate(P, x[:N], mk, r["q_mu"], r["q_sigma"], eps, np.float64)
    e32 = IM.restate(P, x[:N], mk, r["q_mu"], r["q_sigma"], eps, np.float32)
    assert np.array_equal(e64["log_w"][:, 1], e64["lpz_minus_lq"][:, 1])       # (nothing observed: log p(x_obs|z) = 0)
    _close("log_w of the empty image", r["log_w"][:, 1], e64["lpz_minus_lq"][:, 1], e32["lpz_minus_lq"][:, 1])
    _close("log_w", r["log_w"], e64["log_w"], e32["log_w"])
    for key in KEYS:
        assert np.all(np.isfinite(r[key])), key


@pytest.mark.parametrize("nh,nl,xd", IM.SHAPES)
def test_heads_are_those_of_the_masked_input(gpu, nh, nl, xd):
    m, x, P, mask = _net(nh, nl, xd)
    r = _run(nh, nl, xd, 5, 13)[0]
    xin = np.where(mask, x, np.float32(0)).astype(np.float32)
    agg = m.aggregate_posterior(xin, n_samples=1, eps=np.zeros((1, 5, nl), np.float32))
    loc = m.local_posterior(xin, n_samples=1, n_iters=0, n_eval=1, noise=np.zeros((1, 1, 5, nl), np.float32))
    for other in (agg, loc):
        _same(r, other, keys=("q_mu", "q_sigma"))


# ---------------------------------------------------------------- 4. noise
def test_device_noise_and_step_advance(gpu):
    m, x, P, mask = _net(64, 8, 48)
    N, k = 3, 7
    x, mask = x[:N], mask[:N]
    m.set_step(9, 3)
    eps = m.debug_eps(N, k, 0)
    m.set_step(9, 3)
    a = m.impute(x, mask=mask, n_samples=k)
    after = m.debug_eps(N, k, 0)
    _same(a, m.impute(x, mask=mask, n_samples=k, noise=eps))
    assert np.array_equal(after, m.debug_eps(N, k, 0))             # the caller's noise leaves the step alone
    m.set_step(10, 3)
    assert np.array_equal(after, m.debug_eps(N, k, 0))             # the device's advanced it by exactly one
    assert not np.array_equal(after, eps)


# ---------------------------------------------------------------- 5. independence, bitwise
@pytest.mark.parametrize("k", [13, 70], ids=["one_chunk", "two_chunks"])
@pytest.mark.parametrize("nh,nl,xd", [(64, 8, 48), (200, 100, 784)])
def test_position_chunking_and_repeat_are_bitwise(gpu, nh, nl, xd, k):
    m, x, P, mask = _net(nh, nl, xd)
    RB.impute_position_chunking_and_repeat_are_bitwise(m, x, mask, nl, k, base=_run(nh, nl, xd, 5, k)[0] if (5, k) in IM.CASES else None)


# ---------------------------------------------------------------- 6. rejections
def _raw(m, x, N, null=(), **fields):
    from iwae_amd import _capi
    o = _capi.ImputeOptions()
    o.k = 2
    for key, v in fields.items():
        setattr(o, key, v)
    lpx = np.zeros(max(N, 1), dtype=np.float64)
    outs = _capi.ImputeOutputs()
    outs.log_px = None if "log_px" in null else lpx.ctypes.data
    return m.lib.iwae_impute(m.h, None if "x" in null else x.ctypes.data, N, None if "opt" in null else C.byref(o), None if "out" in null else C.byref(outs))


def test_rejected_arguments_leave_the_step_alone(gpu):
    from iwae_amd.native import NativeModel
    m, x, P, mask = _net(64, 8, 48)
    x = np.ascontiguousarray(x[:2])
    m.set_step(17, 3)
    want = m.debug_eps(2, 2, 0)
    for fields in (dict(k=0), dict(k=65537), dict(k=-1), dict(struct_size=16), dict(struct_size=32)):
        assert _raw(m, x, 2, **fields) == -1, fields
    for null in ("x", "opt", "out", "log_px"):
        assert _raw(m, x, 2, null=(null,)) == -1, null
    assert _raw(m, x, 0) == -1 and _raw(m, x, -1) == -1
    assert _raw(m, x, (1 << 11) + 1, k=65536) == -1                # N k > 2^27: rejected before x is read
    for kw in (dict(n_samples=0), dict(n_samples=65537)):
        with pytest.raises(ValueError):
            m.impute(x, **kw)
    with pytest.raises(ValueError):
        m.impute(x[:0], n_samples=2)
    with pytest.raises(ValueError):
        m.impute(x, mask=np.ones((2, 47)), n_samples=2)
    with pytest.raises(ValueError):
        m.impute(x, n_samples=2, noise=np.zeros((3, 2, 8), np.float32))
    assert np.array_equal(m.debug_eps(2, 2, 0), want)             # none of them moved the noise step
    assert _raw(m, x, 2) == 0                                      # the same call without a defect runs, and advances it by one
    m.set_step(18, 3)
    after = m.debug_eps(2, 2, 0)
    m.set_step(17, 3)
    assert _raw(m, x, 2) == 0
    assert np.array_equal(m.debug_eps(2, 2, 0), after)
    for make in (lambda: NativeModel(2, [16, 8], [4, 2], x_dim=48, seed=1), lambda: NativeModel(1, 16, 4, x_dim=48, seed=1, cond_dim=10),
                 lambda: NativeModel(1, 16, 4, x_dim=48, seed=1, cond_dim=10, cond_prior=True), lambda: NativeModel(1, 224, 4, x_dim=48, seed=1)):
        other = make()
        with pytest.raises(ValueError):
            other.impute(x, n_samples=2)
        other.close()
    edge = NativeModel(1, 208, 128, x_dim=48, seed=1)               # the limits themselves run, in one chunk and in two
    for k in (2, 65):
        r = edge.impute(x, mask=mask[:2], n_samples=k)
        assert np.all(np.isfinite(r["log_px"])) and np.all(np.isfinite(r["xhat"]))
    edge.close()


# ---------------------------------------------------------------- 7. shims
def test_shims(gpu):
    from iwae_amd import iwae1, iwae2
    x, P, mask = IM.shape_inputs(64, 8, 48)
    model = iwae1.IWAE(64, 8, x_dim=48, seed=123)
    model._net.set_params(O.flatten_params(P))
    model._net.set_eval_precision("fp32")
    eps = IM.draws(5, 13, 8)
    r = model.impute(x, mask, n_samples=13, noise=eps)
    assert np.array_equal(r["xhat"][mask], x[mask])                # observed pixels exactly as given
    assert np.array_equal(r["xhat"][~mask], r["xhat_raw"][~mask]) and np.all((r["xhat_raw"] > 0.0) & (r["xhat_raw"] < 1.0))
    assert np.array_equal(r["xhat_raw"], _run(64, 8, 48, 5, 13)[0]["xhat"]) and r["log_px"].shape == (5,) and r["ess"].shape == (5,)
    rec = model.reconstruct(x, n_samples=13, noise=eps)
    full = model.impute(x, np.ones_like(mask), n_samples=13, noise=eps)
    assert np.array_equal(rec["xhat"], full["xhat_raw"]) and np.array_equal(rec["log_px"], full["log_px"]) and np.array_equal(rec["ess"], full["ess"])
    assert np.array_equal(full["xhat"], x)
    model._net.close()
    two = iwae2.IWAE([16, 8], [4, 2], x_dim=48)
    with pytest.raises(ValueError):
        two.impute(np.zeros((1, 48), np.float32), None)
    with pytest.raises(ValueError):
        two.reconstruct(np.zeros((1, 48), np.float32))
