"""iwae_grid_posterior (include/iwae_amd.h): the true posterior p(z|x) on a latent grid and log p(x) by quadrature
(tasks/plot_task01.py:31-78), against a float64 restatement built on the oracle's densities, plus its invariances, its use as ground
truth for the k-sample evaluator on a trained model, its argument errors, the Python level and the task01 / task03 drivers.

The restatement: lj(i, g) = sum_j bernoulli_log_prob(x_ij, l_gj) + sum_d normal_log_prob(z_gd, 0, 1) (src/iwae1.py:105-111),
log_px = logsumexp_g(lj + w_g); moments, q_mass and KL(q || p(z|x)) as the header defines them.
"""
import os
import sys

import numpy as np
import pytest

from oracle import iwae_np as O
import make_golden as MG
import _grid_common as GC
from _grid_common import _model, _lse, reference, _grid_case      # (shared with tests/test_gpu_aspect.py)

pytestmark = pytest.mark.gpu

EMU_ROW_ATOL = 0.03          # tests/test_gpu_parity.py: bf16 operands against the rounding-aware oracle


@pytest.mark.parametrize("nh,nl,xd", [(200, 2, 784), (64, 1, 784), (64, 4, 784), (64, 2, 48)])
def test_float32_matches_float64(gpu, nh, nl, xd):
    GC.float32_matches_float64(nh, nl, xd)


def test_bf16_eval_precision_matches_rounding_aware_restatement(gpu):
    N, G = 37, 1531
    x, P, _ = MG.inputs(1, 200, 2, 784, N, 1, 702)
    z, lw = _grid_case(N, G, 2, 13)
    m = _model(200, 2)
    m.set_params(O.flatten_params(P))
    m.set_eval_precision("bf16")
    r = m.grid_posterior(x, z, lw, log_joint=True)
    e = reference(P, x, z, lw, rnd=O.bf16_round)
    assert np.max(np.abs(r["log_joint"] - e["log_joint"])) < EMU_ROW_ATOL
    assert np.max(np.abs(r["log_px"] - e["log_px"])) < EMU_ROW_ATOL
    assert np.max(np.abs(r["kl_q_post"] - e["kl_q_post"])) < EMU_ROW_ATOL
    assert np.max(np.abs(r["post_mean"] - e["post_mean"])) < 1e-2
    np.testing.assert_allclose(r["q_mu"], e["q_mu"], atol=1e-2)
    m.close()


_KEYS = ("log_px", "post_mean", "post_cov", "q_mu", "q_sigma", "q_mass", "kl_q_post")


def test_per_image_independence_and_reproducibility(gpu):
    N, G, i = 300, 3001, 7
    x, P, _ = MG.inputs(1, 200, 2, 784, N, 1, 703)
    z, lw = _grid_case(N, G, 2, 17)
    m = _model(200, 2)
    m.set_params(O.flatten_params(P))
    full = m.grid_posterior(x, z, lw)
    alone = m.grid_posterior(x[i:i + 1], z, lw)
    first = m.grid_posterior(np.concatenate([x[i:i + 1], np.delete(x, i, 0)]), z, lw)
    last = m.grid_posterior(np.concatenate([np.delete(x, i, 0), x[i:i + 1]]), z, lw)
    again = m.grid_posterior(x, z, lw)
    for k in _KEYS:
        np.testing.assert_array_equal(alone[k][0], full[k][i], err_msg=k)
        np.testing.assert_array_equal(first[k][0], full[k][i], err_msg=k)
        np.testing.assert_array_equal(last[k][-1], full[k][i], err_msg=k)
        np.testing.assert_array_equal(again[k], full[k], err_msg=k)
    # chunking of G and the order of the grid points change summation orders only
    m.set_option("grid_chunk", 97)
    chunked = m.grid_posterior(x, z, lw)
    m.set_option("grid_chunk", 0)
    perm = np.random.default_rng(5).permutation(G)
    permuted = m.grid_posterior(x, z[perm], lw[perm])
    for other in (chunked, permuted):
        np.testing.assert_allclose(other["log_px"], full["log_px"], rtol=1e-5, atol=0)
        np.testing.assert_allclose(other["post_mean"], full["post_mean"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(other["post_cov"], full["post_cov"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(other["q_mass"], full["q_mass"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(other["kl_q_post"], full["kl_q_post"], rtol=1e-5, atol=2e-3)
    m.close()


def test_quadrature_is_the_limit_of_the_evaluator_on_a_trained_model(gpu):
    from iwae_amd import utils
    np.random.seed(0)
    m = _model(200, 2, precision="fp32")
    X = O.synthetic_binarized(4000, 21)
    m.set_output_bias(O.output_bias_from_mean(O.synthetic_pixel_means()))
    rng = np.random.default_rng(3)
    for step in range(300):
        m.train_step(X[rng.integers(0, X.shape[0], 100)], 5, 1.0, 1e-3, "iwae_elbo", scalars=False)
    Xt = O.synthetic_binarized(256, 99)
    # (a wider box than [-5, 5]^2: after 300 steps some q(z|x) here keeps ~0.2 % of its mass beyond it -- on 500^2 and 1000^2 points alike)
    z, lw = utils.latent_grid([(-8.0, 8.0)] * 2, 800)
    r = m.grid_posterior(Xt, z, lw)
    assert np.min(r["q_mass"]) > 0.999, np.min(r["q_mass"])
    lpx = float(np.mean(r["log_px"]))
    m.set_step(1000, 0)
    llh = [m.eval_llh(Xt, k) for k in (1, 50, 5000)]
    assert llh[0] < llh[1] < llh[2] <= lpx + 0.02, (llh, lpx)
    # log p(x) = ELBO + KL(q || p(z|x)): the grid's KL against log p(x) minus a k = 5000 Monte Carlo ELBO
    elbo = m.forward(Xt, 5000, 1.0)["vae_elbo"]
    assert abs(float(np.mean(r["kl_q_post"])) - (lpx - elbo)) < 0.05, (float(np.mean(r["kl_q_post"])), lpx - elbo)
    m.close()


def test_argument_errors_leave_the_handle_usable(gpu):
    from iwae_amd.native import NativeModel
    B, k = 8, 5
    x, P, eps = MG.inputs(1, 64, 2, 784, B, k, 704)
    z, lw = _grid_case(B, 200, 2, 19)
    m = _model(64, 2)
    m.set_params(O.flatten_params(P))
    grey = x.copy()
    grey[3, 100] = 0.5
    with pytest.raises(ValueError, match="binary"):
        m.grid_posterior(grey, z, lw)
    with pytest.raises(ValueError):
        m.grid_posterior(x, z[:, :1], lw)          # z of the wrong width
    with pytest.raises(ValueError):
        m.grid_posterior(x[:0], z, lw)             # N = 0
    r = m.train_step(x, k, 1.0, 1e-3, "iwae_elbo", eps=eps)
    fresh = _model(64, 2)
    fresh.set_params(O.flatten_params(P))
    rf = fresh.train_step(x, k, 1.0, 1e-3, "iwae_elbo", eps=eps)
    assert r["iwae_elbo"] == rf["iwae_elbo"]
    np.testing.assert_array_equal(m.get_params(), fresh.get_params())
    fresh.close()
    m.close()
    for model in (NativeModel(2, [64, 32], [2, 2], seed=123), NativeModel(1, 64, 2, seed=123, cond_dim=10), NativeModel(1, 64, 8, seed=123)):
        D = model.n_latent[0]
        with pytest.raises(ValueError):
            model.grid_posterior(x, np.zeros((10, D), np.float32))
        model.close()


def test_python_level(gpu):
    from iwae_amd import iwae1, iwae2, utils
    x, P, _ = MG.inputs(1, 200, 2, 784, 5, 1, 705)
    model = iwae1.IWAE(200, 2)
    model._net.set_params(O.flatten_params(P))
    n1, n2 = 30, 20
    grid, lw = utils.latent_grid([(-2.0, 2.0), (-1.0, 3.0)], (n1, n2))
    tp = model.true_posterior(x, grid, lw)
    np.testing.assert_allclose(_lse(tp["log_posterior"] + lw[None, :].astype(np.float64), 1), 0.0, atol=1e-4)
    assert tp["log_posterior"].shape == (5, n1 * n2) and tp["variational_posterior"].shape == (5, n1 * n2)
    img = tp["variational_posterior"][0].reshape(n2, n1)
    xs, ys = grid[:, 0].reshape(n2, n1), grid[:, 1].reshape(n2, n1)
    np.testing.assert_allclose(xs[0], np.linspace(-2, 2, n1), atol=1e-6)
    np.testing.assert_allclose(ys[:, 0], np.linspace(-1, 3, n2), atol=1e-6)
    mu, sd = tp["q_mu"][0].astype(np.float64), tp["q_sigma"][0].astype(np.float64)
    want = O.normal_log_prob(xs, mu[0], sd[0]) + O.normal_log_prob(ys, mu[1], sd[1])
    np.testing.assert_allclose(img, want, atol=1e-4)
    mean, per = model.true_log_likelihood(x, n_per_dim=60, batch=2)
    z, w = utils.latent_grid([(-5.0, 5.0)] * 2, 60)
    for i in range(5):
        assert per[i] == model._net.grid_posterior(x[i:i + 1], z, w)["log_px"][0]
    assert mean == pytest.approx(float(np.mean(per)))
    model._net.close()
    two = iwae2.IWAE([64, 32], [2, 2])
    with pytest.raises(NotImplementedError, match="nested integral"):
        two.true_posterior(x, grid)
    with pytest.raises(NotImplementedError):
        two.true_log_likelihood(x)
    two._net.close()
    from iwae_amd import task05
    cond = task05.CIWAE(64, 2)
    with pytest.raises(NotImplementedError):
        cond.true_posterior(x, grid)
    cond._net.close()


def _parity():
    import test_gpu_parity
    return test_gpu_parity


@pytest.mark.parametrize("B,k,obj", [(100, 5, "iwae_elbo"), (7, 50, "vae_elbo_kl")])
def test_train_step_at_task01_dims_matches_oracle(gpu, B, k, obj):
    _parity().test_train_step_1layer_matches_oracle(gpu, B, k, obj, 1.0, 200, 2, 784)


@pytest.mark.parametrize("B,k,obj,nl", [(20, 5, "iwae_elbo", [2, 2]), (6, 50, "vae_elbo", [4, 2])])
def test_train_step_at_task01_task03_dims_matches_oracle_2layer(gpu, B, k, obj, nl):
    _parity().test_train_step_2layer_matches_oracle(gpu, B, k, obj, [200, 100], nl, 784)


@pytest.mark.parametrize("task,argv", [("task01", ["--epochs", "1", "--stochastic_layers", "1"]),
                                       ("task01", ["--epochs", "1", "--stochastic_layers", "2", "--objective", "vae_elbo"]),
                                       ("task03", ["--epochs", "1", "--n_samples", "3"])])
def test_task01_task03_drivers_run_one_epoch(gpu, monkeypatch, capsys, task, argv):
    import importlib
    from iwae_amd import utils, _shim
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.syspath_prepend(os.path.join(root, "tasks"))
    for name in ("_common", task):
        sys.modules.pop(name, None)
    mod = importlib.import_module(task)
    monkeypatch.setattr(utils, "load_mnist", lambda path=None: None)
    monkeypatch.setattr(utils, "synthetic_mnist", lambda: (np.clip(np.tile(utils.synthetic_pixel_means(), (400, 1)), 0, 1),
                                                            np.clip(np.tile(utils.synthetic_pixel_means(), (60, 1)), 0, 1)))
    monkeypatch.setattr(_shim.BaseIWAE, "eval_llh", lambda self, x, L, chunk=0: self._net.eval_llh(x[:8], 100))
    if task == "task01":
        for name, value in (("N_EXAMPLES", 2), ("POST_GRID", 20), ("SIR_K", 100), ("SIR_DRAWS", 10), ("LLH_GRID", 50)):
            monkeypatch.setattr(mod, name, value)
    llh = mod.main(argv)
    out = capsys.readouterr().out
    assert "train ELBO" in out and "Test-set 5000 sample log likelihood estimate" in out and np.isfinite(llh)
    if task == "task01" and "1" == argv[argv.index("--stochastic_layers") + 1]:
        assert "Test-set grid-quadrature log likelihood" in out
        line = [l for l in out.splitlines() if "grid-quadrature" in l][0]
        assert np.isfinite(float(line.split()[-1]))
        with np.load("/tmp/iwae/task01_iwae_elbo_1_5/posteriors.npz") as f:
            assert f["log_posterior"].shape == (2, 20, 20) and f["variational_posterior"].shape == (2, 20, 20)
            assert f["sir_idx"].shape == (2, 10) and f["z"].shape == (2, 100, 2)
            lp = f["log_posterior"].astype(np.float64)
            np.testing.assert_allclose(_lse(lp.reshape(2, -1), 1), 0.0, atol=1e-4)
    for name in ("_common", task):
        sys.modules.pop(name, None)
