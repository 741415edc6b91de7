"""iwae_grad_moments on the GPU: the per-parameter mean and unbiased variance of M draws of the training gradient.

  * equal to a float64 Welford fold over get_grads() after forward_backward at set_step(s0 + j), in both precisions, on the 1- and
    2-layer and the conditional models, with the call's side effects (step, gradient buffer, parameters, Adam state);
  * against the float64 oracle fed each draw's own noise (float32 handle);
  * bitwise reproducible, host or device x and outputs;
  * properties of the estimators' distributions: the vae_elbo gradient's variance falls as 1/k, DReG's decoder moments are
    iwae_elbo's, DReG's encoder gradient has iwae_elbo's mean (and vae_elbo's does not);
  * argument errors and the tasks/gradient_snr.py driver.
"""
import os
import sys

import numpy as np
import pytest

from oracle import iwae_np as O
from _grad_moments_common import S0, _model, _Welford, _host_fold, _state, _assert_state_equal, _close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = {"vae_elbo": 0, "iwae_elbo": 1, "iwae_eq14": 2, "vae_elbo_kl": 3, "dreg": 4}
F32_GRAD_REL = 1e-4       # the float32 mode's per-draw gradient tolerance against the float64 oracle (tests/test_gpu_parity.py)


CASES = [  # id, layers, n_hidden, n_latent, x_dim, B, k, cond_dim, objectives
    ("tiny", 1, 16, 4, 48, 5, 3, 0, ("iwae_elbo", "vae_elbo", "dreg")),
    ("ref-B20-k5", 1, 200, 100, 784, 20, 5, 0, ("iwae_elbo", "vae_elbo", "dreg")),       # few rows: eight steps of noise per draw launch
    ("ref-B120-k50", 1, 200, 100, 784, 120, 50, 0, ("iwae_elbo", "vae_elbo", "dreg")),
    ("two-layer", 2, [16, 8], [4, 2], 48, 3, 5, 0, ("iwae_elbo", "vae_elbo")),
    ("conditional", 1, 200, 100, 784, 6, 5, 10, ("iwae_elbo", "vae_elbo")),
]
PARAMS = [(c[0], obj) for c in CASES for obj in c[8]]


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("case,obj", PARAMS, ids=["%s-%s" % p for p in PARAMS])
def test_equals_host_fold(gpu, prec, case, obj):
    _, layers, nh, nl, xd, B, k, cond, _ = next(c for c in CASES if c[0] == case)
    M, beta = 10, 0.8
    m, x, _, _ = _model(layers, nh, nl, xd, prec, B, k, cond)
    before = _state(m)
    m.set_step(S0)
    mean, var = m.grad_moments(x, k, M, beta, obj)
    assert mean.dtype == np.float64 and var.dtype == np.float64 and mean.shape == var.shape == (m.n_params,)
    g_after = m.get_grads()
    eps_after = [m.debug_eps(B, k, l) for l in range(layers)]
    _assert_state_equal(_state(m), before)                # parameters and Adam state (m, v, t) bitwise unchanged
    m.set_step(S0 + M)                                    # the call advanced the noise step by M
    for l in range(layers):
        assert np.array_equal(eps_after[l], m.debug_eps(B, k, l))
    ref_mean, ref_var, g_last = _host_fold(m, x, k, beta, obj, S0, M)
    assert np.array_equal(g_after.view(np.uint32), g_last.view(np.uint32))     # the gradient buffer holds the last draw's gradient
    assert np.all(var >= 0) and np.max(var) > 0
    _close(mean, ref_mean)
    _close(var, ref_var)
    if case == "ref-B20-k5" and prec == "bf16":
        # the same draws with one noise launch per step instead of one per eight steps (option no_eps_multi)
        m1, x1, _, _ = _model(layers, nh, nl, xd, prec, B, k, cond, options={"no_eps_multi": 1})
        ref1_mean, ref1_var, _ = _host_fold(m1, x1, k, beta, obj, S0, M)
        _close(mean, ref1_mean)
        _close(var, ref1_var)
        m1.close()
    m.close()


@pytest.mark.parametrize("layers,obj", [(1, "iwae_elbo"), (1, "vae_elbo"), (1, "dreg"), (2, "iwae_elbo"), (2, "vae_elbo")])
def test_matches_oracle_fold(gpu, layers, obj):
    """Each draw's noise read back with debug_eps, the float64 oracle's gradient of that draw folded the same way.  Tolerances from the
    per-draw float32 bound ||e_j|| <= eps ||g_j|| per tensor (eps = F32_GRAD_REL), G = max_j ||g_j||:
      mean: ||mean(e)|| <= max_j ||e_j|| <= eps G;
      var:  with u_j = g_j - mean(g), v_j = e_j - mean(e), ||v_j|| <= 2 eps G =: d, the elementwise (u + v)^2 - u^2 = 2 u v + v^2
            gives ||var' - var|| <= sum_j (2 ||u_j|| d + d^2) / (M - 1)."""
    nh, nl, xd, B, k = (16, 4, 48, 5, 3) if layers == 1 else ([16, 8], [4, 2], 48, 3, 5)
    M, beta = 10, 1.0 if layers == 2 or obj == "dreg" else 0.7
    m, x, P, _ = _model(layers, nh, nl, xd, "fp32", B, k, seed=300)
    table = m.tensor_table()
    m.set_step(S0)
    mean, var = m.grad_moments(x, k, M, beta, obj)
    draws = []
    for j in range(M):
        m.set_step(S0 + j)
        if layers == 1:
            _, g = O.loss_grads_1layer(P, x, m.debug_eps(B, k, 0).astype(np.float64), beta, obj)
        else:
            _, g = O.loss_grads_2layer(P, x, m.debug_eps(B, k, 0).astype(np.float64), m.debug_eps(B, k, 1).astype(np.float64), beta, obj)
        draws.append(O.flatten_grads(g).astype(np.float64))
    w = _Welford()
    for g in draws:
        w.add(g)
    ref_mean, ref_var = w.mean, w.var()
    for name, shape, off in table:
        sl = slice(off, off + int(np.prod(shape)))
        G = max(np.linalg.norm(g[sl]) for g in draws) + 1e-30
        d = 2 * F32_GRAD_REL * G
        tol_var = sum(2 * np.linalg.norm(g[sl] - ref_mean[sl]) * d + d * d for g in draws) / (M - 1)
        assert np.linalg.norm(mean[sl] - ref_mean[sl]) <= F32_GRAD_REL * G, name
        assert np.linalg.norm(var[sl] - ref_var[sl]) <= tol_var + 1e-30, name
    m.close()


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("B,k", [(20, 5), (120, 50)])
def test_bitwise_reproducible_host_and_device(gpu, prec, B, k):
    import torch
    m, x, _, _ = _model(1, 200, 100, 784, prec, B, k)
    M, P = 6, m.n_params
    m.set_step(S0)
    a = m.grad_moments(x, k, M, 1.0, "iwae_elbo")
    m.set_step(S0)
    b = m.grad_moments(x, k, M, 1.0, "iwae_elbo")
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint64), v.view(np.uint64))
    xd = torch.tensor(x, device="cuda")
    for x_ptr in (x.ctypes.data, xd.data_ptr()):
        md = torch.empty(P, dtype=torch.float64, device="cuda")
        vd = torch.empty(P, dtype=torch.float64, device="cuda")
        m.set_step(S0)
        m.grad_moments_devptr(x_ptr, B, k, M, 1.0, OBJ["iwae_elbo"], md.data_ptr(), vd.data_ptr())
        torch.cuda.synchronize()
        for u, v in zip(a, (md.cpu().numpy(), vd.cpu().numpy())):
            assert np.array_equal(u.view(np.uint64), v.view(np.uint64))
        mh, vh = np.empty(P), np.empty(P)
        m.set_step(S0)
        m.grad_moments_devptr(x_ptr, B, k, M, 1.0, OBJ["iwae_elbo"], mh.ctypes.data, vh.ctypes.data)
        for u, v in zip(a, (mh, vh)):
            assert np.array_equal(u.view(np.uint64), v.view(np.uint64))
    m.close()


def _group_sums(m, var):
    from iwae_amd import utils
    s = utils.gradient_snr_summary(np.zeros_like(var), var, m.tensor_table())
    return s["encoder"]["variance"], s["decoder"]["variance"]


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_vae_elbo_variance_falls_as_one_over_k(gpu, prec):
    """vae_elbo averages k iid reparameterised draws per image, so E[var_k] = var_1 / k exactly: sum var at k = 1 over k = 16 is 16."""
    B, M = 20, 1000
    m, x, _, _ = _model(1, 200, 100, 784, prec, B, 1)
    m.set_step(0)
    _, v1 = m.grad_moments(x, 1, M, 1.0, "vae_elbo")
    _, v16 = m.grad_moments(x, 16, M, 1.0, "vae_elbo")
    for a, b, name in zip(_group_sums(m, v1), _group_sums(m, v16), ("encoder", "decoder")):
        assert 12.8 <= a / b <= 20.0, (name, a / b)
    m.close()


def _t_stat(ma, va, mb, vb, M, idx):
    s = (va[idx] + vb[idx]) / M
    nz = s > 0
    return float(np.mean((ma[idx][nz] - mb[idx][nz]) ** 2 / s[nz]))


def test_dreg_decoder_moments_and_encoder_unbiasedness(gpu):
    B, k = 20, 5
    m, x, _, _ = _model(1, 200, 100, 784, "fp32", B, k)
    table = m.tensor_table()
    enc = np.concatenate([np.arange(off, off + int(np.prod(sh))) for n, sh, off in table if n.startswith("enc")])
    # the decoder's gradient is -iwae_elbo's under both (tasks/task02.py:95-96): same draws, same moments
    m.set_step(S0)
    md, vd = m.grad_moments(x, k, 50, 1.0, "dreg")
    m.set_step(S0)
    mi, vi = m.grad_moments(x, k, 50, 1.0, "iwae_elbo")
    for name, shape, off in table:
        if not name.startswith("dec"):
            continue
        sl = slice(off, off + int(np.prod(shape)))
        for a, b in ((md, mi), (vd, vi)):
            assert np.linalg.norm(a[sl] - b[sl]) <= 1e-5 * np.linalg.norm(b[sl]) + 1e-30, name
    # encoder: DReG is an unbiased estimator of the IWAE bound's gradient.  Disjoint step ranges, M draws each:
    # T = mean over encoder parameters of (m_a - m_b)^2 / ((v_a + v_b) / M), about 1 when the means agree
    M = 2000
    m.set_step(0)
    ma, va = m.grad_moments(x, k, M, 1.0, "dreg")
    mb, vb = m.grad_moments(x, k, M, 1.0, "iwae_elbo")
    mc, vc = m.grad_moments(x, k, M, 1.0, "vae_elbo")
    t_dreg = _t_stat(ma, va, mb, vb, M, enc)
    t_ctrl = _t_stat(mc, vc, mb, vb, M, enc)
    assert t_dreg <= 1.5, t_dreg
    assert t_ctrl >= 5.0, t_ctrl          # the control: the test can tell different means apart
    m.close()


def test_errors_leave_the_step(gpu):
    from iwae_amd.native import NativeModel
    m, x, _, _ = _model(1, 16, 4, 48, "bf16", 5, 3)
    P = m.n_params
    m.set_step(S0)
    m.forward_backward(x, 3, 1.0, "iwae_elbo")
    g0 = m.get_grads()
    m.set_step(S0)
    eps0 = m.debug_eps(5, 3, 0)
    mh, vh = np.empty(P), np.empty(P)
    bad = [dict(draws=1), dict(draws=0), dict(B=0), dict(k=0), dict(k=-2), dict(x=0), dict(mean=0), dict(var=0), dict(obj=7), dict(obj=-1)]
    for b in bad:
        a = dict(x=x.ctypes.data, B=5, k=3, draws=10, obj=1, mean=mh.ctypes.data, var=vh.ctypes.data)
        a.update(b)
        with pytest.raises(ValueError):
            m.grad_moments_devptr(a["x"], a["B"], a["k"], a["draws"], 1.0, a["obj"], a["mean"], a["var"])
        assert np.array_equal(m.debug_eps(5, 3, 0), eps0), b
    assert np.array_equal(m.get_grads().view(np.uint32), g0.view(np.uint32))
    with pytest.raises(ValueError):
        m.grad_moments(x, 3, 1)
    m.close()
    # objectives the model rejects: DReG and vae_elbo_kl on the 2-layer model, DReG on a conditional model
    m2, x2, _, _ = _model(2, [16, 8], [4, 2], 48, "bf16", 3, 5)
    m2.set_step(S0)
    e2 = m2.debug_eps(3, 5, 0)
    for obj in ("dreg", "vae_elbo_kl"):
        with pytest.raises(ValueError):
            m2.grad_moments(x2, 5, 4, 1.0, obj)
    assert np.array_equal(m2.debug_eps(3, 5, 0), e2)
    m2.close()
    mc = NativeModel(1, 200, 100, cond_dim=10, seed=123)
    mc.set_condition(np.eye(10, dtype=np.float32)[:4])
    with pytest.raises(ValueError):
        mc.grad_moments(np.zeros((4, 784), np.float32), 5, 4, 1.0, "dreg")
    mc.close()


def test_model_classes(gpu):
    from iwae_amd import iwae1, task02, task05
    x = O.synthetic_binarized(8, 3)
    a = iwae1.IWAE(200, 100, seed=5)
    r = a.gradient_snr(x, 5, n_draws=4)
    assert set(r) >= {"encoder", "decoder", "tensors", "mean", "var"}
    assert r["encoder"]["n"] + r["decoder"]["n"] == a._net.n_params
    d = task02.IWAEDReG(200, 100, seed=5)
    rd = d.gradient_snr(x, 5, n_draws=4)
    a._net.set_step(0)
    rr = a.gradient_snr(x, 5, n_draws=4, objective="dreg")
    assert np.array_equal(rd["mean"], rr["mean"]) and np.array_equal(rd["var"], rr["var"])     # IWAEDReG defaults to dreg
    c = task05.CIWAE(200, 100, seed=5)
    rc = c.gradient_snr(x, np.arange(8) % 10, 5, n_draws=4)
    assert rc["encoder"]["variance"] > 0


def test_driver_prints_and_saves(gpu, capsys, tmp_path):
    from iwae_amd import iwae1
    sys.path.insert(0, os.path.join(ROOT, "tasks"))
    try:
        sys.modules.pop("gradient_snr", None)
        import gradient_snr
    finally:
        sys.path.pop(0)
    w = str(tmp_path / "final_weights.npz")
    iwae1.IWAE(200, 100, seed=9).save_weights(w)
    for est in (None, "dreg"):
        argv = ["--weights", w, "--k_list", "1,5", "--draws", "8", "--batch_size", "10"] + (["--estimator", est] if est else [])
        rows = gradient_snr.main(argv)
        out = capsys.readouterr().out
        lines = [l for l in out.splitlines() if l.startswith("k = ")]
        assert len(lines) == 2 and lines[0].startswith("k =     1:") and lines[1].startswith("k =     5:"), out
        assert all("encoder SNR" in l and "decoder SNR" in l and "variance" in l for l in lines)
        with np.load(str(tmp_path / "gradient_snr.npz")) as f:
            assert list(f["k"]) == [1, 5] and int(f["draws"]) == 8 and int(f["batch_size"]) == 10
            assert str(f["estimator"]) == (est or "iwae_elbo")
            for g in ("encoder", "decoder"):
                for s in ("snr", "variance", "signal"):
                    assert f["%s_%s" % (g, s)].shape == (2,) and np.all(np.isfinite(f["%s_%s" % (g, s)]))
                    assert np.array_equal(f["%s_%s" % (g, s)], rows["%s_%s" % (g, s)])
            assert f["mean_k5"].dtype == np.float64 and f["var_k5"].shape == f["mean_k5"].shape
            assert np.all(f["encoder_variance"] > 0)
