"""Host-side pieces of iwae_posterior (no GPU): the C declaration and its ctypes binding, the restatement of its formulas
(tests/_posterior_ref.py) against the direct formulas and against quadrature of p(z | x_obs) on a model with two latent dimensions, and --
from the restatement alone -- that the GPU parity cases of tests/test_gpu_posterior.py have weights that matter and tolerances that are
admissible."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden as MG  # noqa: E402
import _parity_common as PC  # noqa: E402
import _impute_ref as IM  # noqa: E402
import _posterior_ref as PR  # noqa: E402

OUTPUTS = ["log_px", "ess", "mean", "cov", "idx", "z", "u", "log_w", "q_mu", "q_sigma"]


# ---------------------------------------------------------------- 1. declaration, binding, build lists, documents
def _header():
    return open(os.path.join(ROOT, "include", "iwae_amd.h")).read()


def _typedef_fields(name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.search(r"(\w+)\s*$", f.strip()).group(1) for f in body.split(";") if f.strip()]


def test_declaration_and_binding(lib_built):
    from iwae_amd import _capi
    assert hasattr(C.CDLL(lib_built), "iwae_posterior")
    decl = re.search(r"int iwae_posterior\(([^;]*)\);", _header())
    assert decl, "iwae_posterior is not declared"
    assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == 5
    res, args = _capi.SYMBOLS["iwae_posterior"]
    assert res is C.c_int and len(args) == 5
    assert args[3] is C.POINTER(_capi.PosteriorOptions) and args[4] is C.POINTER(_capi.PosteriorOutputs)
    o = _capi.PosteriorOptions
    assert [f[0] for f in o._fields_] == _typedef_fields("iwae_posterior_options") == ["struct_size", "k", "R", "reserved", "mask", "eps", "unif"]
    assert [f[0] for f in _capi.PosteriorOutputs._fields_] == _typedef_fields("iwae_posterior_outputs") == OUTPUTS
    assert list(_capi.POSTERIOR_OUTPUT_FIELDS) == OUTPUTS
    # the numbers model.hip static_asserts
    assert C.sizeof(o) == 40 and [getattr(o, f).offset for f in ("struct_size", "k", "R", "reserved", "mask", "eps", "unif")] == [0, 4, 8, 12, 16, 24, 32]
    assert o().struct_size == 40 and o().reserved == 0             # the binding fills the ABI guard itself
    assert C.sizeof(_capi.PosteriorOutputs) == 10 * C.sizeof(C.c_void_p)
    src = open(os.path.join(ROOT, "iwae_amd", "csrc", "model.hip")).read()
    assert "sizeof(iwae_posterior_options) == 40" in src and "sizeof(iwae_posterior_outputs) == 10 * sizeof(void*)" in src


def test_build_lists_tool_driver_and_documents():
    from iwae_amd import _capi
    assert "posterior_kernels.hip" in _capi._ID_SOURCES
    b = open(os.path.join(ROOT, "iwae_amd", "csrc", "build.sh")).read()
    assert b.count("posterior_kernels.hip") >= 2 and b.count("posterior_kernels.o") >= 2      # the id list, the compile line and the link line
    listed = re.search(r"BUILD_ID=\$\(for f in (.*?); do", b).group(1).split()
    assert [os.path.basename(f) for f in listed] == [os.path.basename(f) for f in _capi._ID_SOURCES]
    readme = open(os.path.join(ROOT, "tools", "README.md")).read()
    assert '"posterior"' in readme and "dev/posterior_time.py" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "dev", "posterior_time.py"))
    for doc in ("DESIGN.md", "README.md"):
        assert "iwae_posterior" in open(os.path.join(ROOT, doc)).read(), doc
    assert '"posterior"' in _header()                              # the timer name
    import main
    sys.path.insert(0, os.path.join(ROOT, "tasks"))
    try:
        import posterior
    finally:
        sys.path.pop(0)
    before = sorted(a.dest for a in main.parser._actions)
    a = posterior.make_parser().parse_args([])
    assert vars(a) == dict(vars(main.parser.parse_args([])), weights=None, images=100, draws=5000, resamples=200, rate=0.0, mask_seed=0, out=None)
    assert sorted(a.dest for a in main.parser._actions) == before      # main.parser is not mutated


# ---------------------------------------------------------------- 2. the restatement against the direct formulas
def test_restatement_against_the_direct_formulas():
    x, P, mask = IM.shape_inputs(64, 8, 48)
    for N, k in ((3, 7), (5, 70), (1, 257)):
        eps = IM.draws(N, k, 8)
        mu, sigma = IM.encoder_heads(P, x[:N], mask[:N])
        base = IM.restate(P, x[:N], mask[:N], mu, sigma, eps)
        r = PR.restate(P, x[:N], mask[:N], mu, sigma, eps)
        assert np.array_equal(r["log_w"], base["log_w"]) and np.array_equal(r["log_px"], base["log_px"])
        assert np.max(np.abs(r["al"] - base["al"])) <= 1e-15
        m, c = PR.direct_moments(r["al"], r["z"])
        assert np.max(np.abs(r["mean"] - m)) <= 1e-10 and np.max(np.abs(r["cov"] - c)) <= 1e-10
        assert np.array_equal(r["cov"], np.swapaxes(r["cov"], 1, 2))


# ---------------------------------------------------------------- 3. weight edge cases of the index rule
def test_one_hot_weights_send_every_index_to_that_draw():
    k, hot = 37, [0, 11, 36]
    lw = np.full((k, 3), -1.0e4, dtype=np.float32)
    lw[hot, np.arange(3)] = 0.0
    u = np.concatenate([np.random.default_rng(0).random((50, 3)), np.full((1, 3), 2.0 ** -25), np.ones((1, 3))]).astype(np.float32)
    idx = PR.indices(lw, u)
    assert idx.dtype == np.int32 and np.array_equal(idx, np.broadcast_to(np.array(hot, dtype=np.int32)[None], u.shape))


def test_uniform_weights_and_the_midpoints_give_every_draw_once():
    k = 50
    u = ((np.arange(k) + 0.5) / k).astype(np.float32)
    idx = PR.indices(np.zeros((k, 2), np.float32), np.stack([u, u], axis=1))
    assert np.array_equal(idx[:, 0], np.arange(k)) and np.array_equal(idx[:, 1], np.arange(k))


# ---------------------------------------------------------------- 4. ground truth: quadrature of the posterior
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_moments_and_resampling_against_quadrature(masked):
    """64/2/48 model whose decoder depends strongly on z (dec_in = 3: the posterior is far from q), 4 images, k = 4 096 draws from the
    encoder's q: the SNIS mean and covariance against the float64 rectangle rule over [-8, 8]^2 at 801^2 points within 4 delta-method
    standard errors; the unweighted moments of the same draws at least 15 of those standard errors off (ignoring the weights fails); the mean of
    R = 512 SIR draws within 4 posterior standard deviations / sqrt(R).  Figures are the largest over images and entries.  Measured when
    written (unmasked, masked): SNIS mean 1.13, 1.01; SNIS cov 1.7, 1.7; unweighted mean 35.6, 31.3; unweighted cov 24.9, 20.9; SIR 2.41, 2.03."""
    k, Rn = 4096, 512
    x, P, eps = MG.inputs(1, 64, 2, 48, 4, k, 71)
    P = PC.spread_params(P, 1, head=0.1, dec_in=3.0)
    mask = np.random.default_rng(5).random((4, 48)) < 0.5 if masked else None
    mu, sigma = IM.encoder_heads(P, x, np.ones(x.shape, dtype=bool) if mask is None else mask)
    r = PR.restate(P, x, mask, mu, sigma, eps)
    qm, qc = PR.quadrature_posterior(P, x, mask)
    se_m, se_c = PR.standard_errors(r["al"], r["z"], r["mean"], r["cov"])
    gap_m, gap_c = np.max(np.abs(r["mean"] - qm) / se_m), np.max(np.abs(r["cov"] - qc) / se_c)
    flat = np.full_like(r["al"], 1.0 / k)
    um, uc = PR.direct_moments(flat, r["z"])
    ugap_m, ugap_c = np.max(np.abs(um - qm) / se_m), np.max(np.abs(uc - qc) / se_c)      # (in the SNIS estimate's standard errors)
    u = np.random.default_rng(9).random((Rn, 4)).astype(np.float32)
    idx = PR.indices(r["log_w"].astype(np.float32), u)
    zs = r["z"][idx, np.arange(4)[None]]
    sir = np.max(np.abs(zs.mean(axis=0) - qm) / (np.sqrt(qc[:, [0, 1], [0, 1]]) / np.sqrt(Rn)))
    print("SNIS mean %.3g se, cov %.3g se; unweighted mean %.3g se, cov %.3g se; SIR mean %.3g sd/sqrt(R); ESS/k %s"
          % (gap_m, gap_c, ugap_m, ugap_c, sir, PC.ess_fraction(r["al"])))
    assert gap_m <= 4.0 and gap_c <= 4.0
    assert ugap_m >= 15.0 and ugap_c >= 15.0
    assert sir <= 4.0


# ---------------------------------------------------------------- 5. the GPU parity cases, from the restatement alone
_case_cache = {}


def _case(nh, nl, xd, N, k):
    key = (nh, nl, xd, N, k)
    if key not in _case_cache:
        x, P, mask = IM.shape_inputs(nh, nl, xd)
        x, mask = x[:N], mask[:N]
        mu, sigma = IM.encoder_heads(P, x, mask)
        eps = IM.draws(N, k, nl)
        _case_cache[key] = (PR.restate(P, x, mask, mu, sigma, eps, np.float64), PR.restate(P, x, mask, mu.astype(np.float32), sigma.astype(np.float32), eps, np.float32))
    return _case_cache[key]


@pytest.mark.parametrize("N,k", IM.CASES, ids=IM.CASE_IDS)
@pytest.mark.parametrize("nh,nl,xd", IM.SHAPES)
def test_tolerances_are_admissible(nh, nl, xd, N, k):
    """The GPU tests allow 8 x (float32 restatement - float64 restatement), floor 1e-5: that figure stays small enough to mean something.
    (Measured when written: mean <= 2.9e-5, cov <= 9.0e-5, the worst at 200/100/784 with (N, k) = (3, 7).)"""
    r64, r32 = _case(nh, nl, xd, N, k)
    d_m, d_c = float(np.max(np.abs(r32["mean"] - r64["mean"]))), float(np.max(np.abs(r32["cov"] - r64["cov"])))
    print("float32 restatement off the float64 one: mean %.3g, cov %.3g" % (d_m, d_c))
    assert d_m <= 2e-4 and d_c <= 2e-4


@pytest.mark.parametrize("nh,nl,xd", IM.SHAPES)
def test_the_weights_matter_at_the_gpu_cases(nh, nl, xd):
    """N = 5, k = 70: mean and cov are at least 1e-2 (1 000 times the floor of the GPU test's tolerance) from the unweighted moments of the
    same draws, and the weights are spread (median ESS/k >= 0.3).  (Measured when written: mean >= 0.16, cov >= 0.19.)"""
    r, _ = _case(nh, nl, xd, 5, 70)
    um, uc = PR.direct_moments(np.full_like(r["al"], 1.0 / 70), r["z"])
    d_m, d_c = float(np.max(np.abs(r["mean"] - um))), float(np.max(np.abs(r["cov"] - uc)))
    frac = PC.ess_fraction(r["al"])
    print("from the unweighted moments: mean %.3g, cov %.3g; ESS/k %s" % (d_m, d_c, frac))
    assert d_m >= 1e-2 and d_c >= 1e-2
    assert np.median(frac) >= 0.3
