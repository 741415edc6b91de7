"""iwae_posterior (include/iwae_amd.h): the self-normalised latent mean and covariance and sampling importance resampling on the device,
on iwae_impute's weights.

The handles, images, masks and draws are tests/test_gpu_impute.py's (tests/_impute_ref.py: SPREAD parameters, a 50 % mask), float32 eval
precision throughout.  Tolerances follow its rule, set at run time: 8 x the largest deviation of a float32 numpy run of the restatement
(tests/_posterior_ref.py) from its float64 run on the same inputs, floor 1e-5; the moments are compared to the float64 restatement at
softmax(DEVICE log_w), so the error of log_w is not charged twice.  tests/test_posterior_host.py shows from the restatement alone that
these cases have weights that matter.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import iwae_np as O
import make_golden as MG
import _parity_common as PC
import _impute_ref as IM
import _posterior_ref as PR
import _row_eval_bodies as RB

pytestmark = pytest.mark.gpu

SHARED = ("log_px", "ess", "log_w", "q_mu", "q_sigma")
KEYS = ("log_px", "ess", "mean", "cov", "idx", "z", "u", "log_w", "q_mu", "q_sigma")
R0 = 7
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


unif = RB.unif

_runs = {}


def _run(nh, nl, xd, N, k):
    """The device's outputs (masked, the caller's draws and uniforms, R0 resampled draws) and the two restatements at the device's heads,
    once per case."""
    key = (nh, nl, xd, N, k)
    if key not in _runs:
        m, x, P, mask = _net(nh, nl, xd)
        _runs[key] = RB.posterior_run(m, x, P, mask, nl, N, k)
    return _runs[key]


def _same(a, b, keys=KEYS):
    RB.same(a, b, keys)


# ---------------------------------------------------------------- 1. the outputs shared with iwae_impute
@pytest.mark.parametrize("N,k", [(5, 13), (5, 70)], ids=["one_chunk", "two_chunks"])
@pytest.mark.parametrize("nh,nl,xd", IM.SHAPES)
def test_shared_outputs_are_imputes_bitwise(gpu, nh, nl, xd, N, k):
    m, x, P, mask = _net(nh, nl, xd)
    eps = IM.draws(N, k, nl)
    for mk in (mask[:N], None):
        _same(m.posterior(x[:N], mask=mk, n_samples=k, n_draws=R0, noise=eps, uniforms=unif(R0, N)), m.impute(x[:N], mask=mk, n_samples=k, noise=eps), keys=SHARED)
        m.set_step(21, 2)
        a = m.posterior(x[:N], mask=mk, n_samples=k, n_draws=R0)
        m.set_step(21, 2)
        _same(a, m.impute(x[:N], mask=mk, n_samples=k), keys=SHARED)


# ---------------------------------------------------------------- 2. parity of the moments
@pytest.mark.parametrize("N,k", IM.CASES, ids=IM.CASE_IDS)
@pytest.mark.parametrize("nh,nl,xd", IM.SHAPES)
def test_moment_parity(gpu, nh, nl, xd, N, k):
    m, x, P, mask = _net(nh, nl, xd)
    RB.posterior_moment_parity(m, x, mask, nl, N, k, _run(nh, nl, xd, N, k))


# ---------------------------------------------------------------- 3. ragged widths
def test_nothing_is_written_past_the_last_feature(gpu):
    """D = 5, x_dim = 53: cov [N, 5, 5], z [R, N, 5] and idx [R, N] into device arrays with a guard row of sentinels behind them, through
    the raw binding, one chunk per image and two."""
    m, x, P, mask = _net(37, 5, 53)
    RB.posterior_nothing_past_the_last_feature(m, x, mask, 5, lambda N, k: _run(37, 5, 53, N, k)[0])


# ---------------------------------------------------------------- 4. resampling
_small = {}


def _weights_run(k):
    """64/8/48, 3 images, k draws: log_w and the heads from a call without resampling (shared by the cases below)."""
    if k not in _small:
        m, x, P, mask = _net(64, 8, 48)
        eps = IM.draws(3, k, 8)
        _small[k] = (eps, m.posterior(x[:3], mask=mask[:3], n_samples=k, noise=eps, outputs=("log_w", "q_mu", "q_sigma")))
    return _small[k]


@pytest.mark.parametrize("R", [1, 7, 200])
@pytest.mark.parametrize("k", [1, 13, 65, 257])
def test_indices_and_draws(gpu, k, R):
    m, x, P, mask = _net(64, 8, 48)
    N = 3
    eps, w = _weights_run(k)
    RB.posterior_indices_and_draws(m, x, mask, 8, N, k, R, eps, w)


def test_edge_uniforms_take_the_first_and_the_last_weighted_draw(gpu):
    m, x, P, mask = _net(64, 8, 48)
    N, k = 3, 65
    eps, w = _weights_run(k)
    lo, hi = np.float32(2.0 ** -25), np.float32(1.0 - 2.0 ** -25)      # (the latter is 1 in float32: no c_s exceeds the target)
    u = np.stack([np.full(N, lo, np.float32), np.full(N, hi, np.float32)])
    r = m.posterior(x[:N], mask=mask[:N], n_samples=k, n_draws=2, noise=eps, uniforms=u, outputs=("idx", "log_w"))
    lw = r["log_w"]
    wt = np.exp((lw - lw.max(axis=0)[None]).astype(np.float64))
    for n in range(N):
        nz = np.nonzero(wt[:, n] > 0.0)[0]
        assert r["idx"][0, n] == nz[0] and r["idx"][1, n] == nz[-1], (n, r["idx"][:, n], nz[0], nz[-1])
    assert np.array_equal(r["idx"], PR.indices(lw, u))


# ---------------------------------------------------------------- 5. the device's noise
def test_device_noise_step_and_offset(gpu):
    m, x, P, mask = _net(64, 8, 48)
    N, k, R = 3, 70, 9
    x, mask = x[:N], mask[:N]
    m.set_step(9, 3)
    eps = m.debug_eps(N, k, 0)
    a = m.posterior(x, mask=mask, n_samples=k, n_draws=R)
    after = m.debug_eps(N, k, 0)
    assert np.all(a["u"] > 0.0) and np.all(a["u"] < 1.0) and len(np.unique(a["u"])) == R * N
    m.set_step(10, 3)
    assert np.array_equal(after, m.debug_eps(N, k, 0)) and not np.array_equal(after, eps)      # advanced by exactly one
    m.set_step(9, 3)
    _same(a, m.posterior(x, mask=mask, n_samples=k, n_draws=R, noise=eps, uniforms=a["u"]))
    assert np.array_equal(eps, m.debug_eps(N, k, 0))               # both the caller's: the step stays
    m.posterior(x, mask=mask, n_samples=k, noise=eps)             # nothing resampled, the caller's draws: it stays
    assert np.array_equal(eps, m.debug_eps(N, k, 0))
    b = m.posterior(x, mask=mask, n_samples=k, n_draws=R, noise=eps)      # the device's uniforms alone move it, and are the same ones
    assert np.array_equal(after, m.debug_eps(N, k, 0))
    _same(a, b)
    for n in range(N):                                             # u of image n at offset b is u of image 0 at offset b + n
        m.set_step(9, 3 + n)
        one = m.posterior(x[n:n + 1], mask=mask[n:n + 1], n_samples=k, n_draws=R, outputs=("u",))
        assert np.array_equal(one["u"][:, 0], a["u"][:, n]), n


# ---------------------------------------------------------------- 6. independence, bitwise
@pytest.mark.parametrize("k", [13, 70], ids=["one_chunk", "two_chunks"])
@pytest.mark.parametrize("nh,nl,xd", [(64, 8, 48), (200, 100, 784)])
def test_position_chunking_and_repeat_are_bitwise(gpu, nh, nl, xd, k):
    m, x, P, mask = _net(nh, nl, xd)
    RB.posterior_position_chunking_and_repeat_are_bitwise(m, x, mask, nl, k, _run(nh, nl, xd, 5, k)[0])


# ---------------------------------------------------------------- 7. ground truth on the device
def test_against_quadrature(gpu):
    """tests/test_posterior_host.py's 64/2/48 model, every pixel observed, k = 4 096: mean and cov within 4 delta-method standard errors
    (from the device's log_w and the draws given) of iwae_grid_posterior's moments on 401^2 points over [-8, 8]^2.  The float64
    restatement's gaps against quadrature, 1.13 and 1.7 standard errors, are the record that the bound is admissible."""
    from iwae_amd import utils
    from iwae_amd.native import NativeModel
    k = 4096
    x, P, eps = MG.inputs(1, 64, 2, 48, 4, k, 71)
    P = PC.spread_params(P, 1, head=0.1, dec_in=3.0)
    m = NativeModel(1, 64, 2, x_dim=48, seed=123)
    m.set_params(O.flatten_params(P))
    m.set_eval_precision("fp32")
    zg, lw = utils.latent_grid([(-8.0, 8.0)] * 2, 401)
    g = m.grid_posterior(x, zg, lw)
    r = m.posterior(x, n_samples=k, noise=eps)
    m.close()
    al = PR.weights(r["log_w"], np.float64)
    z = r["q_mu"].astype(np.float64)[None] + r["q_sigma"].astype(np.float64)[None] * eps.astype(np.float64)
    se_m, se_c = PR.standard_errors(al, z, r["mean"], r["cov"])
    gap_m, gap_c = np.max(np.abs(r["mean"] - g["post_mean"]) / se_m), np.max(np.abs(r["cov"] - g["post_cov"]) / se_c)
    print("mean %.3g se, cov %.3g se off the grid posterior; ESS/k %s" % (gap_m, gap_c, PC.ess_fraction(al)))
    assert gap_m <= 4.0 and gap_c <= 4.0


# ---------------------------------------------------------------- 8. rejections
def _raw(m, x, N, null=(), want=(), **fields):
    from iwae_amd import _capi
    o = _capi.PosteriorOptions()
    o.k = 2
    for key, v in fields.items():
        setattr(o, key, v)
    lpx = np.zeros(max(N, 1), dtype=np.float64)
    big = np.zeros(max(N, 1) * 64, dtype=np.float32)
    outs = _capi.PosteriorOutputs()
    outs.log_px = None if "log_px" in null else lpx.ctypes.data
    for name in want:
        setattr(outs, name, big.ctypes.data)
    return m.lib.iwae_posterior(m.h, None if "x" in null else x.ctypes.data, N, None if "opt" in null else C.byref(o), None if "out" in null else C.byref(outs))


def test_rejected_arguments_leave_the_step_alone(gpu):
    from iwae_amd.native import NativeModel
    m, x, P, mask = _net(64, 8, 48)
    x = np.ascontiguousarray(x[:2])
    m.set_step(17, 3)
    want = m.debug_eps(2, 2, 0)
    for fields in (dict(k=0), dict(k=65537), dict(k=-1), dict(R=-1), dict(R=65537), dict(struct_size=24), dict(struct_size=48), dict(reserved=1)):
        assert _raw(m, x, 2, **fields) == -1, fields
    for null in ("x", "opt", "out", "log_px"):
        assert _raw(m, x, 2, null=(null,)) == -1, null
    assert _raw(m, x, 0) == -1 and _raw(m, x, -1) == -1
    assert _raw(m, x, (1 << 11) + 1, k=65536) == -1                # N k > 2^27: rejected before x is read
    assert _raw(m, x, (1 << 11) + 1, k=2, R=65536) == -1           # N R > 2^27
    for name in ("idx", "z", "u"):
        assert _raw(m, x, 2, want=(name,)) == -1, name             # asked for with R = 0
    for kw in (dict(n_samples=0), dict(n_samples=65537), dict(n_samples=2, n_draws=-1), dict(n_samples=2, n_draws=65537),
               dict(n_samples=2, outputs=("z",)), dict(n_samples=2, outputs=("nothing",))):
        with pytest.raises(ValueError):
            m.posterior(x, **kw)
    with pytest.raises(ValueError):
        m.posterior(x[:0], n_samples=2)
    with pytest.raises(ValueError):
        m.posterior(x, mask=np.ones((2, 47)), n_samples=2)
    with pytest.raises(ValueError):
        m.posterior(x, n_samples=2, noise=np.zeros((3, 2, 8), np.float32))
    with pytest.raises(ValueError):
        m.posterior(x, n_samples=2, n_draws=3, uniforms=np.zeros((2, 2), np.float32))
    assert np.array_equal(m.debug_eps(2, 2, 0), want)             # none of them moved the noise step
    assert _raw(m, x, 2) == 0                                      # the same call without a defect runs, and advances it by one
    m.set_step(18, 3)
    after = m.debug_eps(2, 2, 0)
    m.set_step(17, 3)
    assert _raw(m, x, 2, R=3, want=("idx",)) == 0
    assert np.array_equal(m.debug_eps(2, 2, 0), after)
    for make in (lambda: NativeModel(2, [16, 8], [4, 2], x_dim=48, seed=1), lambda: NativeModel(1, 16, 4, x_dim=48, seed=1, cond_dim=10),
                 lambda: NativeModel(1, 16, 4, x_dim=48, seed=1, cond_dim=10, cond_prior=True), lambda: NativeModel(1, 224, 4, x_dim=48, seed=1)):
        other = make()
        with pytest.raises(ValueError):
            other.posterior(x, n_samples=2)
        other.close()
    edge = NativeModel(1, 208, 128, x_dim=48, seed=1)               # the limits themselves run, in one chunk and in two
    for k in (2, 65):
        r = edge.posterior(x, mask=mask[:2], n_samples=k, n_draws=3)
        for key in KEYS:
            assert np.all(np.isfinite(r[key])), (k, key)
        assert r["cov"].shape == (2, 128, 128) and np.array_equal(r["cov"], np.swapaxes(r["cov"], 1, 2))
    edge.close()


# ---------------------------------------------------------------- 9. shims
def test_shims(gpu):
    from iwae_amd import iwae1, iwae2
    x, P, mask = IM.shape_inputs(64, 8, 48)
    model = iwae1.IWAE(64, 8, x_dim=48, seed=123)
    model._net.set_params(O.flatten_params(P))
    model._net.set_eval_precision("fp32")
    eps, u = IM.draws(5, 13, 8), unif(R0, 5)
    r = model.posterior(x, mask, n_samples=13, n_draws=R0, noise=eps, uniforms=u)
    _same(r, _run(64, 8, 48, 5, 13)[0])
    mi = model.multiple_imputations(x, mask, n_samples=13, n_draws=4, seed=3)
    assert mi.shape == (4, 5, 48) and mi.dtype == np.float32 and set(np.unique(mi)) <= {0.0, 1.0}
    assert np.array_equal(mi[:, mask], np.broadcast_to(x[mask][None], (4, int(mask.sum()))))
    assert len(np.unique(mi.reshape(4, -1), axis=0)) > 1           # the unobserved pixels differ between imputations
    model._net.close()
    two = iwae2.IWAE([16, 8], [4, 2], x_dim=48)
    with pytest.raises(ValueError):
        two.posterior(np.zeros((1, 48), np.float32))
    with pytest.raises(ValueError):
        two.multiple_imputations(np.zeros((1, 48), np.float32), None)
