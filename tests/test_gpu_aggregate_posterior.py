"""iwae_aggregate_posterior (include/iwae_amd.h): the split of mean_n KL(q(z|x_n) || p(z)) into mi + tc + dim_kl over the aggregate
posterior q(z) = (1/N) sum_m q(z|x_m) (Hoffman & Johnson 2016; Chen et al. 2018).

The expected values are the float64 restatement of tests/_aggregate_ref.py on the DEVICE'S OWN q_mu, q_sigma and the eps passed in, so the
kernels are pinned independently of the encoder's precision.  Per-sample tolerance: 8 x the largest deviation of a float32 numpy run of
the same restatement from the float64 run on the same inputs (computed here, at run time), floor 1e-5: the margin covers the device's
other summation order and its hardware exp / log.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from _aggregate_ref import restate, sums
from _aggregate_common import SUMMARY, _model, _setup, _parity, _check_sums

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(64, 8, 48), (200, 100, 784), (64, 128, 48)]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("N", [1, 37, 300])
@pytest.mark.parametrize("nh,nl,xd", SHAPES)
def test_per_sample_parity_and_sums(gpu, nh, nl, xd, N, S, prec):
    x, m, eps = _setup(nh, nl, xd, N, S, 17 + N + S, prec)
    r = m.aggregate_posterior(x, n_samples=S, eps=eps, per_sample=True)
    m.close()
    assert r["q_mu"].shape == (N, nl) and r["unit_kl"].shape == (nl,) and r["unit_kl"].dtype == np.float64
    assert r["log_n"] == np.log(N)
    e64 = _parity(r, eps)
    # the sums: double means of the device's own per-sample outputs and lq_own, lp in float64
    want = sums(r["log_qz"], r["log_qzd"], e64["lq_own"], e64["lp"])
    for key in ("unit_kl", "unit_mi") + SUMMARY:
        np.testing.assert_allclose(r[key], want[key], rtol=1e-6, atol=1e-9, err_msg=key)
    mi, tc, dk, kl = (float(r[k]) for k in SUMMARY)
    assert abs(kl - (mi + tc + dk)) <= 1e-9 * (abs(mi) + abs(tc) + abs(dk) + abs(kl)) + 1e-12
    assert np.all(e64["lq_own"].sum(axis=2) - r["log_qz"].astype(np.float64) <= np.log(N) + 1e-4)
    assert np.all(r["unit_mi"] <= np.log(N) + 1e-4)
    if N == 1:      # one component: q(z) = q(z|x_1), nothing to be informed about
        assert abs(mi) <= 1e-5 and np.all(np.abs(r["unit_mi"]) <= 1e-5)


@pytest.mark.parametrize("nl,N,S", [(8, 1100, 2), (8, 130, 127), (4, 513, 33)], ids=["ranges", "tiles", "both"])
def test_component_ranges_and_sample_tiles(gpu, nl, N, S):
    """The seams of the blocking: more than one range of 512 components with a partial last one (N = 1100: 3 ranges, 76 in the last;
    merged across ranges under a common maximum), more than one tile of 16 384 samples with a partial last one (130 x 127 = 16 510), and
    both at once with a padded unit width (513 x 33 = 16 929 samples, ranges of 512 + 1 components, D = 4 -> 16).  The smallest shapes
    that cross each seam: the float64 restatement is N^2 S D terms.  Same parity bound as above."""
    x, m, eps = _setup(64, nl, 48, N, S, 3 + N, "fp32")
    r = m.aggregate_posterior(x, n_samples=S, eps=eps, per_sample=True)
    e64 = _parity(r, eps)
    _check_sums(r, e64, N)
    # a draw alone equals the same draw inside the large call, also when it sat in the last tile / behind a tile boundary
    for s in sorted({0, S - 1, 16384 // N}):
        if s < S:
            one = m.aggregate_posterior(x, n_samples=1, eps=eps[s:s + 1], per_sample=True)
            assert np.array_equal(one["log_qz"][0], r["log_qz"][s]) and np.array_equal(one["log_qzd"][0], r["log_qzd"][s]), s
    m.close()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("nh,nl,xd", [(64, 8, 48), (200, 100, 784)])
def test_shared_heads_give_zero_information(gpu, nh, nl, xd, prec):
    """Head weight matrices zeroed: every image has mu = bias, sigma = exp(bias) + 1e-6, the mixture is one Gaussian."""
    def edit(P, x):
        Q = [(W.copy(), b.copy()) for W, b in P]
        Q[2] = (np.zeros_like(Q[2][0]), Q[2][1])
        Q[3] = (np.zeros_like(Q[3][0]), Q[3][1])
        return Q
    N, S = 37, 3
    x, m, eps = _setup(nh, nl, xd, N, S, 5, prec, edit)
    r = m.aggregate_posterior(x, n_samples=S, eps=eps, per_sample=True)
    m.close()
    assert np.all(r["q_mu"] == r["q_mu"][0]) and np.all(r["q_sigma"] == r["q_sigma"][0])
    e64 = restate(r["q_mu"], r["q_sigma"], eps)
    assert np.max(np.abs(r["log_qzd"] - e64["lq_own"])) <= 1e-5
    assert np.max(np.abs(r["log_qz"] - e64["lq_own"].sum(axis=2))) <= 1e-5
    assert abs(r["mi"]) <= 1e-5 and abs(r["tc"]) <= 1e-5 and np.all(np.abs(r["unit_mi"]) <= 1e-5)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_stress_sigma_spread_and_far_draws(gpu, prec):
    """log sigma over +-6 across the images and |eps| = 8: the edge of the numerical domain the header states."""
    nh, nl, xd, N, S = 64, 8, 48, 64, 3

    def edit(P, x):
        (W1, b1), (W2, b2) = P[0], P[1]
        h = np.tanh(np.tanh(np.asarray(x, dtype=np.float64) @ W1 + b1) @ W2 + b2)
        a = h @ P[3][0]
        f = 6.6 / min(a.max(), -a.min())
        Q = list(P)
        Q[3] = (P[3][0] * f, P[3][1])
        return Q
    x, m, eps = _setup(nh, nl, xd, N, S, 99, prec, edit)
    far = np.random.default_rng(3).random(eps.shape)
    eps[far < 0.05] = 8.0
    eps[far > 0.95] = -8.0
    r = m.aggregate_posterior(x, n_samples=S, eps=eps, per_sample=True)
    m.close()
    ls = np.log(r["q_sigma"].astype(np.float64))
    assert ls.min() <= -6.0 and ls.max() >= 6.0, (ls.min(), ls.max())        # the input is not silently benign
    assert np.abs(eps).max() == 8.0
    for key in ("log_qz", "log_qzd", "unit_kl", "unit_mi", "q_mu", "q_sigma") + SUMMARY:
        assert np.all(np.isfinite(r[key])), key
    _parity(r, eps)


def test_bitwise_invariances_and_device_draws(gpu):
    nh, nl, xd, N, S = 64, 8, 48, 37, 3
    x, m, eps = _setup(nh, nl, xd, N, S, 7, "fp32")
    keys = ("log_qz", "log_qzd", "unit_kl", "unit_mi", "q_mu", "q_sigma") + SUMMARY
    a = m.aggregate_posterior(x, n_samples=S, eps=eps, per_sample=True)
    b = m.aggregate_posterior(x, n_samples=S, eps=eps, per_sample=True)
    for key in keys:
        assert np.array_equal(a[key], b[key]), key
    one = m.aggregate_posterior(x, n_samples=1, eps=eps[1:2], per_sample=True)       # a sample's densities: not S, not its position
    assert np.array_equal(one["log_qz"][0], a["log_qz"][1]) and np.array_equal(one["log_qzd"][0], a["log_qzd"][1])
    # device draws = iwae_debug_eps(N, S, 0) at the same step and offset; they advance the step by one, explicit draws do not
    m.set_step(11, 3)
    host = m.debug_eps(N, S, 0)
    dev = m.aggregate_posterior(x, n_samples=S, per_sample=True)
    after = m.debug_eps(N, S, 0)
    m.set_step(12, 3)
    assert np.array_equal(after, m.debug_eps(N, S, 0)) and not np.array_equal(after, host)
    m.set_step(11, 3)
    exp = m.aggregate_posterior(x, n_samples=S, eps=host, per_sample=True)
    assert np.array_equal(m.debug_eps(N, S, 0), host)                            # still step 11
    for key in keys:
        assert np.array_equal(dev[key], exp[key]), key
    m.close()


def test_errors(gpu):
    from iwae_amd import _capi, iwae2, task04, task05
    lib = _capi.load()
    x = np.zeros((4, 48), dtype=np.float32)
    out = np.zeros(4, dtype=np.float64)
    ps = out.ctypes.data_as(C.POINTER(C.c_double))

    def call(m, N, S, summary):
        lib.iwae_set_step(m.h, 21, 5)
        before = m.debug_eps(4, 2, 0)
        rc = lib.iwae_aggregate_posterior(m.h, x.ctypes.data, N, S, None, summary, None, None, None, None, None, None)
        msg = lib.iwae_last_error().decode()
        assert np.array_equal(m.debug_eps(4, 2, 0), before) == (rc != 0)         # a rejected call leaves the noise step alone
        return rc, msg

    m1 = _model(64, 8, 48)
    assert call(m1, 4, 2, ps)[0] == 0
    for N, S, summary in ((0, 2, ps), (-3, 2, ps), (4, 0, ps), (4, -1, ps), (4, 2, None)):
        rc, msg = call(m1, N, S, summary)
        assert rc == -1 and msg, (N, S, summary)
    m1.close()
    m2 = _model([64, 32], [16, 8], 48, layers=2)
    rc, msg = call(m2, 4, 2, ps)
    assert rc == -1 and "1-layer" in msg
    m2.close()
    for kw in ({"cond_dim": 10}, {"cond_dim": 10, "cond_prior": True}):
        mc = _model(64, 8, 48, **kw)
        rc, msg = call(mc, 4, 2, ps)
        assert rc == -1 and msg
        with pytest.raises(ValueError):
            mc.aggregate_posterior(x)
        mc.close()
    for model in (task05.CIWAE(64, 8, x_dim=48), task04.CIWAE(64, 8, x_dim=48), iwae2.IWAE([64, 32], [16, 8], x_dim=48)):
        with pytest.raises(NotImplementedError):
            model.aggregate_posterior(x)
        model._net.close()


def test_driver_prints_the_decomposition(gpu, tmp_path):
    """tasks/elbo_surgery.py as a child process on a freshly saved model and the synthetic stand-in data (a small set, handed over as the
    mnist.npz the loader looks for): one line per unit, and sum_d (unit_kl + unit_mi) = kl."""
    from iwae_amd import iwae1, utils
    model = iwae1.IWAE(200, 100)
    wpath = str(tmp_path / "final_weights.npz")
    model.save_weights(wpath)
    model._net.close()
    Xtr, Xte = utils.synthetic_mnist(n_train=8, n_test=150)
    as_u8 = lambda a: np.round(a * 255).astype(np.uint8).reshape(-1, 28, 28)
    np.savez(str(tmp_path / "mnist.npz"), x_train=as_u8(Xtr), y_train=np.zeros(8, np.uint8), x_test=as_u8(Xte), y_test=np.zeros(150, np.uint8))
    env = dict(os.environ, IWAE_MNIST_PATH=str(tmp_path / "mnist.npz"))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tasks", "elbo_surgery.py"), "--weights", wpath, "--draws", "2"],
                       env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    vals = {ln.split()[0]: float(ln.split()[1]) for ln in lines if ln.split() and ln.split()[0] in SUMMARY}
    assert sorted(vals) == sorted(SUMMARY), p.stdout
    assert any(ln.startswith("images 150  draws 2  log N") for ln in lines), p.stdout
    units = [ln.split() for ln in lines if ln.startswith("unit ")]
    assert len(units) == 100 and [int(u[1]) for u in units] == list(range(100))
    total = sum(float(u[u.index("unit_kl") + 1]) + float(u[u.index("unit_mi") + 1]) for u in units)
    assert abs(total - vals["kl"]) <= 1e-6 * abs(vals["kl"]), (total, vals["kl"])
    assert all(float(u[u.index("A_u") + 1]) >= 0.0 for u in units)
