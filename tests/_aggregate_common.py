"""Helpers of the iwae_aggregate_posterior GPU tests (tests/test_gpu_aggregate_posterior.py, tests/test_gpu_ragged_widths.py): the seeded
set-up, the per-sample parity check with its run-time tolerance and the check of the sums.  Not a test module."""
import numpy as np

from oracle import iwae_np as O
import make_golden as MG
from _aggregate_ref import restate, sums

SUMMARY = ("mi", "tc", "dim_kl", "kl")


def _model(nh, nl, xd, layers=1, **kw):
    from iwae_amd.native import NativeModel
    return NativeModel(layers, nh, nl, x_dim=xd, seed=123, **kw)


def _setup(nh, nl, xd, N, S, seed, prec, edit=None):
    x, P, _ = MG.inputs(1, nh, nl, xd, N, 1, seed)
    if edit:
        P = edit(P, x)
    m = _model(nh, nl, xd)
    m.set_params(O.flatten_params(P))
    m.set_eval_precision(prec)
    eps = np.random.default_rng(seed + 9).standard_normal((S, N, nl)).astype(np.float32)
    return x, m, eps


def _parity(r, eps):
    """log_qz / log_qzd against float64 on the device's heads; returns the float64 restatement."""
    e64 = restate(r["q_mu"], r["q_sigma"], eps, np.float64)
    e32 = restate(r["q_mu"], r["q_sigma"], eps, np.float32)
    for key in ("log_qz", "log_qzd"):
        tol = max(8.0 * float(np.max(np.abs(e32[key].astype(np.float64) - e64[key]))), 1e-5)
        err = float(np.max(np.abs(r[key].astype(np.float64) - e64[key])))
        print("%s: device error %.3g, float32 restatement %.3g, tolerance %.3g" % (key, err, tol / 8.0, tol))
        assert r[key].dtype == np.float32 and r[key].shape == e64[key].shape
        assert err <= tol, (key, err, tol)
    return e64


def _check_sums(r, e64, N):
    want = sums(r["log_qz"], r["log_qzd"], e64["lq_own"], e64["lp"])
    for key in ("unit_kl", "unit_mi") + SUMMARY:
        np.testing.assert_allclose(r[key], want[key], rtol=1e-6, atol=1e-9, err_msg=key)
    mi, tc, dk, kl = (float(r[k]) for k in SUMMARY)
    assert abs(kl - (mi + tc + dk)) <= 1e-9 * (abs(mi) + abs(tc) + abs(dk) + abs(kl)) + 1e-12
    assert np.all(e64["lq_own"].sum(axis=2) - r["log_qz"].astype(np.float64) <= np.log(N) + 1e-4)
