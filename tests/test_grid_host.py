"""Host-side pieces of the latent-grid quadrature (no GPU): utils.latent_grid's point order, weights and ranges
(tasks/plot_task01.py:22-29), and the argument parsers of the task01 / task03 drivers (the reference's tasks/task01.py:17-26,
tasks/task03.py:19-27)."""
import os
import sys

import numpy as np
import pytest

from iwae_amd import utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_latent_grid_order_weights_and_ranges():
    n1, n2 = 7, 5
    z, lw = utils.latent_grid([(-1.0, 2.0), (0.5, 1.5)], (n1, n2))
    assert z.shape == (n1 * n2, 2) and z.dtype == np.float32 and lw.shape == (n1 * n2,)
    # plot_task01.get_grid: X, Y = meshgrid(linspace(range1, n1), linspace(range2, n2)); points (X.ravel(), Y.ravel())
    X, Y = np.meshgrid(np.linspace(-1.0, 2.0, n1), np.linspace(0.5, 1.5, n2))
    np.testing.assert_allclose(z[:, 0], X.reshape(-1), atol=1e-7)
    np.testing.assert_allclose(z[:, 1], Y.reshape(-1), atol=1e-7)
    np.testing.assert_allclose(z[:, 0].reshape(n2, n1)[3], np.linspace(-1.0, 2.0, n1), atol=1e-7)      # reshape(n2, n1) is the image
    assert z[:, 0].min() == -1.0 and z[:, 0].max() == 2.0 and z[:, 1].min() == 0.5 and z[:, 1].max() == 1.5
    np.testing.assert_allclose(lw, np.log(3.0 / (n1 - 1) * 1.0 / (n2 - 1)), rtol=1e-6)
    # the weights make a Riemann sum: a standard normal density over a wide box integrates to ~1
    z, lw = utils.latent_grid([(-6.0, 6.0)] * 2, 241)
    logpdf = -0.5 * np.sum(z.astype(np.float64) ** 2, axis=1) - np.log(2 * np.pi)
    assert abs(np.sum(np.exp(logpdf + lw)) - 1.0) < 1e-6
    z1, lw1 = utils.latent_grid([(-3.0, 3.0)], 13)
    assert z1.shape == (13, 1)
    np.testing.assert_allclose(z1[:, 0], np.linspace(-3, 3, 13), atol=1e-7)
    np.testing.assert_allclose(lw1, np.log(0.5), rtol=1e-6)
    with pytest.raises(ValueError):
        utils.latent_grid([(-1.0, 1.0)], 1)


def _parsers():
    sys.path.insert(0, os.path.join(ROOT, "tasks"))
    try:
        import _common
        return _common
    finally:
        sys.path.pop(0)


def test_task01_parser_matches_the_reference_flags():
    c = _parsers()
    a = c.parser_task01().parse_args([])
    assert vars(a) == {"stochastic_layers": 1, "n_samples": 5, "batch_size": 20, "epochs": -1, "objective": "iwae_elbo", "gpu": "0"}
    a = c.parser_task01().parse_args(["--stochastic_layers", "2", "--n_samples", "50", "--objective", "vae_elbo_kl", "--gpu", "3"])
    assert (a.stochastic_layers, a.n_samples, a.objective, a.gpu) == (2, 50, "vae_elbo_kl", "3")
    with pytest.raises(SystemExit):
        c.parser_task01().parse_args(["--stochastic_layers", "3"])
    with pytest.raises(SystemExit):
        c.parser_task01().parse_args(["--objective", "dreg"])


def test_task03_parser_matches_the_reference_flags():
    c = _parsers()
    a = c.parser_task03().parse_args([])
    assert vars(a) == {"n_samples": 5, "batch_size": 20, "epochs": -1, "objective": "iwae_elbo", "gpu": "0"}
    with pytest.raises(SystemExit):
        c.parser_task03().parse_args(["--stochastic_layers", "1"])       # tasks/task03.py has no such flag
