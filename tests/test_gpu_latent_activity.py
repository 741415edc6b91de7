"""iwae_latent_activity (include/iwae_amd.h): the active-units statistic of Burda et al. section 5.2, A_u = Cov_x(E_q[u|x]), against a
float64 restatement, plus the device draws, its bitwise invariances, constructed activities, argument errors and the driver.

The restatement: E_q[z1|x] = mu1(x) (src/iwae1.py:39-42); E_q[z2|x] = mean over the k draws z1 = mu1 + sigma1 eps of mu2(z1), the q(z2|z1)
head (src/iwae2.py:61-65); A_u = population variance over the images.  rnd = O.bf16_round puts in the bf16 eval precision's rounding points.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import iwae_np as O
import make_golden as MG
from _activity_common import _model, reference, _setup, _check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF2 = ([200, 100], [100, 50], 784)        # the reference's 2-layer model: the fused bf16 kernel's shape
SMALL2 = ([64, 32], [16, 8], 48)            # composed path


NK = [(1, 1), (37, 50), (300, 200)]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("nh,nl,xd", [(64, 8, 48), (200, 100, 784)])
@pytest.mark.parametrize("N,k", NK)
def test_one_layer_matches_float64(gpu, prec, nh, nl, xd, N, k):
    x, P, m, _ = _setup(1, nh, nl, xd, N, k, 31 + N, prec)
    m.set_step(5, 0)
    r = m.latent_activity(x, k=k, per_image=True)
    assert len(r["activity"]) == 1 and r["activity"][0].shape == (nl,) and r["post_mean"][0].shape == (N, nl)
    _check(r, reference(P, x, rnd=None if prec == "fp32" else O.bf16_round), prec)
    m.close()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", [SMALL2, REF2], ids=["composed", "reference"])
@pytest.mark.parametrize("N,k", NK)
def test_two_layer_matches_float64(gpu, prec, shape, N, k):
    nh, nl, xd = shape
    x, P, m, eps = _setup(2, nh, nl, xd, N, k, 41 + N + k, prec)
    r = m.latent_activity(x, k=k, eps=eps, per_image=True)
    assert [a.shape for a in r["activity"]] == [(nl[0],), (nl[1],)]
    assert [p.shape for p in r["post_mean"]] == [(N, nl[0]), (N, nl[1])]
    _check(r, reference(P, x, eps, rnd=None if prec == "fp32" else O.bf16_round), prec)
    m.close()


@pytest.mark.parametrize("prec,shape", [("bf16", REF2), ("fp32", REF2), ("bf16", SMALL2)], ids=["fused", "fp32", "composed"])
def test_device_draws_are_the_evaluators(gpu, prec, shape):
    """eps=None draws what iwae_debug_eps (the evaluator's generator, latent stream 0, row (offset + i) k + s) gives at that step; a
    2-layer call advances the step by one."""
    nh, nl, xd = shape
    N, k = 37, 200
    x, P, m, _ = _setup(2, nh, nl, xd, N, k, 77, prec)
    m.set_step(11, 3)
    host = m.debug_eps(N, k, 0)
    m.set_step(11, 3)
    a = m.latent_activity(x, k=k, per_image=True)
    b = m.latent_activity(x, k=k, per_image=True)                # step 12 now
    m.set_step(11, 3)
    c = m.latent_activity(x, k=k, eps=host, per_image=True)
    for l in range(2):
        assert np.array_equal(a["post_mean"][l], c["post_mean"][l])
        assert np.array_equal(a["activity"][l], c["activity"][l]) and np.array_equal(a["data_mean"][l], c["data_mean"][l])
    assert not np.array_equal(a["post_mean"][1], b["post_mean"][1])
    assert np.array_equal(a["post_mean"][0], b["post_mean"][0])      # layer 1 draws nothing
    m.set_step(12, 3)
    d = m.latent_activity(x, k=k, per_image=True)
    assert np.array_equal(b["post_mean"][1], d["post_mean"][1])
    m.close()


def test_one_layer_call_ignores_k_and_leaves_the_step(gpu):
    x, P, m, _ = _setup(1, 64, 8, 48, 20, 1, 5, "fp32")
    m.set_step(3, 0)
    a = m.latent_activity(x, k=1, per_image=True)
    b = m.latent_activity(x, k=0, per_image=True)
    assert np.array_equal(a["post_mean"][0], b["post_mean"][0]) and np.array_equal(a["activity"][0], b["activity"][0])
    h1 = m.debug_eps(4, 2, 0)
    m.set_step(3, 0)
    assert np.array_equal(h1, m.debug_eps(4, 2, 0))
    m.close()


@pytest.mark.parametrize("prec,shape", [("bf16", REF2), ("fp32", REF2), ("bf16", SMALL2), ("fp32", SMALL2)],
                         ids=["fused", "fp32", "composed", "composed-fp32"])
def test_invariances_are_bitwise(gpu, prec, shape):
    """An image's post_mean does not depend on N, its position (same draws), the eval_rows chunking or the call."""
    nh, nl, xd = shape
    N, k = 300, 200
    x, P, m, _ = _setup(2, nh, nl, xd, N, k, 99, prec)
    m.set_step(21, 0)
    full = m.latent_activity(x, k=k, per_image=True)
    m.set_step(21, 0)
    again = m.latent_activity(x, k=k, per_image=True)
    for l in range(2):
        assert np.array_equal(full["post_mean"][l], again["post_mean"][l])
        assert np.array_equal(full["activity"][l], again["activity"][l])
    for j in (0, 1, 137, 299):
        m.set_step(21, j)                                          # image j alone at batch offset j: the same Philox rows
        one = m.latent_activity(x[j:j + 1], k=k, per_image=True)
        for l in range(2):
            assert np.array_equal(one["post_mean"][l][0], full["post_mean"][l][j]), (j, l)
    for rows in (128, 1000, 100000):                              # k split in 128-sample chunks / whole images, few or many per launch
        m.set_option("eval_rows", rows)
        m.set_step(21, 0)
        r = m.latent_activity(x, k=k, per_image=True)
        for l in range(2):
            assert np.array_equal(r["post_mean"][l], full["post_mean"][l]), (rows, l)
            assert np.array_equal(r["activity"][l], full["activity"][l])
    m.set_option("eval_rows", 0)
    # host draws: the same image at another position of another call, fed the same draws
    eps = np.random.default_rng(3).standard_normal((k, N, nl[0])).astype(np.float32)
    a = m.latent_activity(x, k=k, eps=eps, per_image=True)
    perm = np.array([5, 17, 0])
    b = m.latent_activity(x[perm], k=k, eps=np.ascontiguousarray(eps[:, perm]), per_image=True)
    for l in range(2):
        assert np.array_equal(b["post_mean"][l], a["post_mean"][l][perm])
    m.close()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("layers,shape", [(1, (200, 100, 784)), (2, REF2), (2, SMALL2)], ids=["1layer", "2layer", "2layer-small"])
def test_constructed_activity_counts(gpu, prec, layers, shape):
    """mu-head columns set to zero give A_u == 0.0 exactly; scaled-up columns are active; active_units counts exactly."""
    from iwae_amd import iwae1, iwae2
    nh, nl, xd = shape
    N, k = 64, 150
    x, P, _ = MG.inputs(layers, nh, nl, xd, N, 1, 123)
    D1 = nl if layers == 1 else nl[0]
    keep1 = [3, 5, 7]
    for which in ([1] if layers == 1 else [1, 2]):
        Q = [(W.copy(), b.copy()) for W, b in P]
        hi = 2 if which == 1 else 6                     # the mu head of q(z1|x) / of q(z2|z1)
        W = Q[hi][0]
        keep = keep1 if which == 1 else [1, 6]
        mask = np.zeros(W.shape[1], dtype=bool)
        mask[keep] = True
        W[:, ~mask] = 0.0
        W[:, mask] *= 30.0
        model = iwae1.IWAE(nh, nl, x_dim=xd) if layers == 1 else iwae2.IWAE(nh, nl, x_dim=xd)
        model._net.set_params(O.flatten_params(Q))
        model._net.set_eval_precision(prec)
        counts, act = (model.active_units(x) if layers == 1 else model.active_units(x, n_samples=k))
        a = act[which - 1]
        assert np.all(a[~mask] == 0.0), a[~mask]
        assert np.all(a[mask] > 1e-2), a[mask]
        assert counts[which - 1] == len(keep)
        assert counts == [int(np.sum(v > 1e-2)) for v in act]
        assert len(act) == layers and act[0].shape == (D1,)
        model._net.close()


def test_errors(gpu):
    from iwae_amd import _capi, task04, task05
    lib = _capi.load()
    x = np.zeros((4, 48), dtype=np.float32)
    act = np.zeros(64, dtype=np.float64)
    pa = act.ctypes.data_as(C.POINTER(C.c_double))
    m2 = _model(2, [64, 32], [16, 8], 48)
    assert lib.iwae_latent_activity(m2.h, x.ctypes.data, 4, 10, None, pa, None, None) == 0
    assert lib.iwae_latent_activity(m2.h, x.ctypes.data, 0, 10, None, pa, None, None) == -1
    assert lib.iwae_latent_activity(m2.h, x.ctypes.data, -3, 10, None, pa, None, None) == -1
    assert lib.iwae_latent_activity(m2.h, x.ctypes.data, 4, 0, None, pa, None, None) == -1
    assert lib.iwae_latent_activity(m2.h, x.ctypes.data, 4, -1, None, pa, None, None) == -1
    assert lib.iwae_latent_activity(m2.h, x.ctypes.data, 4, 10, None, None, None, None) == -1
    assert "activity" in lib.iwae_last_error().decode()
    m2.close()
    m1 = _model(1, 64, 8, 48)
    assert lib.iwae_latent_activity(m1.h, x.ctypes.data, 4, 0, None, pa, None, None) == 0      # (1 layer: k is not used)
    assert lib.iwae_latent_activity(m1.h, x.ctypes.data, 4, 1, None, None, None, None) == -1
    m1.close()
    for kw in ({"cond_dim": 10}, {"cond_dim": 10, "cond_prior": True}):
        mc = _model(1, 64, 8, 48, **kw)
        assert lib.iwae_latent_activity(mc.h, x.ctypes.data, 4, 1, None, pa, None, None) == -1
        with pytest.raises(ValueError):
            mc.latent_activity(x)
        mc.close()
    for cls in (task05.CIWAE, task04.CIWAE):
        model = cls(64, 8, x_dim=48)
        with pytest.raises(NotImplementedError):
            model.active_units(x)
        model._net.close()


def test_driver_prints_and_saves(gpu, monkeypatch, capsys, tmp_path):
    """main.py for one epoch on synthetic data, then tasks/active_units.py with the same flags: one line per layer, activity.npz next to the
    weights, counts equal to IWAE.active_units on the same test images."""
    import importlib
    import main
    from iwae_amd import utils, iwae2
    importlib.reload(main)
    monkeypatch.setattr(utils, "load_mnist", lambda path=None: None)
    monkeypatch.setattr(utils, "synthetic_mnist", lambda: (np.clip(np.tile(utils.synthetic_pixel_means(), (400, 1)), 0, 1),
                                                            np.clip(np.tile(utils.synthetic_pixel_means(), (60, 1)), 0, 1)))
    monkeypatch.setattr(main.iwae2.IWAE, "eval_llh", lambda self, x, L, chunk=0: self._net.eval_llh(x[:8], 100))
    argv = ["--stochastic_layers", "2", "--epochs", "1", "--batch_size", "100", "--n_samples", "5", "--objective", "iwae_elbo"]
    main.main(argv)
    capsys.readouterr()
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tasks"))
    for name in ("_common", "active_units"):
        sys.modules.pop(name, None)
    au = importlib.import_module("active_units")
    counts, act = au.main(argv)
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith("Active units, layer")]
    assert lines == ["Active units, layer 1: %d / 100" % counts[0], "Active units, layer 2: %d / 50" % counts[1]], out
    wdir = "/tmp/iwae/main_iwae_elbo_2_5"
    with np.load(os.path.join(wdir, "activity.npz")) as f:
        assert list(f["counts"]) == counts
        assert f["post_mean_1"].shape == (60, 100) and f["post_mean_2"].shape == (60, 50)
        assert np.array_equal(f["activity_2"], act[1])
    model = iwae2.IWAE([200, 100], [100, 50])
    model.load_weights(os.path.join(wdir, "final_weights.npz"))
    c2, a2 = model.active_units(au.load_test_set(), n_samples=au.N_SAMPLES)
    assert c2 == counts and all(np.array_equal(p, q) for p, q in zip(a2, act))
    model._net.close()
    for name in ("_common", "active_units"):
        sys.modules.pop(name, None)
