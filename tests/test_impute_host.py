"""Host-side pieces of iwae_impute (no GPU): the C declaration and its ctypes binding, the float64 restatement of its formulas
(tests/_impute_ref.py) against the oracle and against quadrature of log p(x_obs) on a model with two latent dimensions, and -- from the
restatement alone -- that the GPU parity cases of tests/test_gpu_impute.py have weights that matter and tolerances that are admissible."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import iwae_np as O  # noqa: E402
import make_golden as MG  # noqa: E402
import _ais_ref as R  # noqa: E402
import _parity_common as PC  # noqa: E402
import _impute_ref as IM  # noqa: E402


# ---------------------------------------------------------------- 1. declaration, binding, build lists, documents
def _header():
    return open(os.path.join(ROOT, "include", "iwae_amd.h")).read()


def _typedef_fields(name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.search(r"(\w+)\s*$", f.strip()).group(1) for f in body.split(";") if f.strip()]


def test_declaration_and_binding(lib_built):
    from iwae_amd import _capi
    assert hasattr(C.CDLL(lib_built), "iwae_impute")
    decl = re.search(r"int iwae_impute\(([^;]*)\);", _header())
    assert decl, "iwae_impute is not declared"
    assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == 5
    res, args = _capi.SYMBOLS["iwae_impute"]
    assert res is C.c_int and len(args) == 5
    assert args[3] is C.POINTER(_capi.ImputeOptions) and args[4] is C.POINTER(_capi.ImputeOutputs)
    o = _capi.ImputeOptions
    assert [f[0] for f in o._fields_] == _typedef_fields("iwae_impute_options") == ["struct_size", "k", "mask", "eps"]
    assert [f[0] for f in _capi.ImputeOutputs._fields_] == _typedef_fields("iwae_impute_outputs") == ["log_px", "xhat", "ess", "log_w", "q_mu", "q_sigma"]
    # the numbers model.hip static_asserts
    assert C.sizeof(o) == 24 and o.struct_size.offset == 0 and o.k.offset == 4 and o.mask.offset == 8 and o.eps.offset == 16
    assert o().struct_size == 24                                   # the binding fills the ABI guard itself
    assert C.sizeof(_capi.ImputeOutputs) == 6 * C.sizeof(C.c_void_p)
    src = open(os.path.join(ROOT, "iwae_amd", "csrc", "model.hip")).read()
    assert "sizeof(iwae_impute_options) == 24" in src and "sizeof(iwae_impute_outputs) == 6 * sizeof(void*)" in src


def test_build_lists_option_tool_and_driver():
    from iwae_amd import _capi
    assert "impute_kernels.hip" in _capi._ID_SOURCES
    b = open(os.path.join(ROOT, "iwae_amd", "csrc", "build.sh")).read()
    assert b.count("impute_kernels.hip") >= 2 and b.count("impute_kernels.o") >= 2      # the id list, the compile line and the link line
    listed = re.search(r"BUILD_ID=\$\(for f in (.*?); do", b).group(1).split()
    assert [os.path.basename(f) for f in listed] == [os.path.basename(f) for f in _capi._ID_SOURCES]
    readme = open(os.path.join(ROOT, "tools", "README.md")).read()
    assert "impute_rows" in readme and "dev/impute_time.py" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "dev", "impute_time.py"))
    assert "iwae_impute" in open(os.path.join(ROOT, "DESIGN.md")).read()
    import main
    sys.path.insert(0, os.path.join(ROOT, "tasks"))
    try:
        import impute
    finally:
        sys.path.pop(0)
    before = sorted(a.dest for a in main.parser._actions)
    a = impute.make_parser().parse_args([])
    assert vars(a) == dict(vars(main.parser.parse_args([])), weights=None, images=1000, draws=50, rates=[0.25, 0.5, 0.75], mask_seed=0)
    assert sorted(a.dest for a in main.parser._actions) == before      # main.parser is not mutated


def test_mcar_mask():
    from iwae_amd import utils
    m = utils.mcar_mask((200, 784), 0.5, seed=3)
    assert m.dtype == np.uint8 and m.shape == (200, 784) and set(np.unique(m)) == {0, 1}
    assert abs(m.mean() - 0.5) < 0.01                              # (156 800 fair coins: 4 standard errors are 0.005)
    assert np.array_equal(m, utils.mcar_mask((200, 784), 0.5, seed=3)) and not np.array_equal(m, utils.mcar_mask((200, 784), 0.5, seed=4))
    assert utils.mcar_mask((3, 4), 0.0).all() and not utils.mcar_mask((3, 4), 1.0).any()
    with pytest.raises(ValueError):
        utils.mcar_mask((3, 4), 1.5)


# ---------------------------------------------------------------- 2. nothing masked: the oracle's log-weights
def test_restatement_is_the_oracle_when_nothing_is_masked():
    x, P, eps = MG.inputs(1, 64, 8, 48, 4, 6, 51)
    mu, sigma = IM.encoder_heads(P, x, np.ones(x.shape, dtype=bool))
    res = O.forward_1layer(P, x, eps)
    want = res["lpxz"] + res["lpz"] - res["lqzx"]
    for mask in (np.ones(x.shape, dtype=bool), np.ones(x.shape, dtype=np.uint8), None):
        r = IM.restate(P, x, mask, mu, sigma, eps)
        assert np.max(np.abs(r["log_w"] - want)) <= 1e-10
        assert np.max(np.abs(r["al"] - res["al"])) <= 1e-10
        assert np.max(np.abs(r["xhat"] - np.sum(res["al"][:, :, None] * O.sigmoid(res["logits"]), axis=0))) <= 1e-10
        assert np.max(np.abs(r["log_px"] - O.logmeanexp(want, axis=0))) <= 1e-10


def test_restatement_never_reads_the_unobserved_pixels():
    x, P, mask = IM.shape_inputs(64, 8, 48)
    eps = IM.draws(3, 7, 8)
    mu, sigma = IM.encoder_heads(P, x[:3], mask[:3])
    a = IM.restate(P, x[:3], mask[:3], mu, sigma, eps)
    xn = np.where(mask[:3], x[:3], np.nan).astype(np.float32)
    mu2, sigma2 = IM.encoder_heads(P, xn, mask[:3])
    b = IM.restate(P, xn, mask[:3], mu2, sigma2, eps)
    for key in ("log_w", "log_px", "ess", "xhat"):
        assert np.array_equal(a[key], b[key]), key


# ---------------------------------------------------------------- 3. the formula estimates log p(x_obs)
def test_bound_against_quadrature_of_the_observed_pixels():
    """64/2/48 model, 4 images, 50 % mask, k = 2 000 draws from the encoder's q at the masked input: LSE_s log_w - log k against the
    float64 rectangle rule over [-8, 8]^2 at 401^2 points, within 4 delta-method standard errors on every image.  (Measured when written:
    gaps of 0.82, -1.52, 0.19 and 0.35 standard errors.)  A wrong mask sign, a missing -log k or the unobserved pixels left in each move
    the estimate by nats, hundreds of standard errors."""
    k = 2000
    x, P, eps = MG.inputs(1, 64, 2, 48, 4, k, 71)
    P = PC.spread_params(P, 1)
    mask = np.random.default_rng(5).random((4, 48)) < 0.5
    mu, sigma = IM.encoder_heads(P, x, mask)
    r = IM.restate(P, x, mask, mu, sigma, eps)
    truth = IM.quadrature_log_px_obs(P, x, mask)
    se = R.log_mean_se(r["log_w"])
    gap = (r["log_px"] - truth) / se
    print("log_px", r["log_px"], "quadrature", truth, "se", se, "gap in se", gap)
    assert np.all(np.abs(gap) <= 4.0), gap
    # what the three mistakes would give, for the record of the claim above
    full = IM.quadrature_log_px_obs(P, x, np.ones_like(mask))
    flipped = IM.quadrature_log_px_obs(P, x, ~mask)
    assert np.all(np.abs(r["log_px"] - full) > 100 * se) and np.all(np.abs(r["log_px"] - flipped) > 100 * se) and np.log(k) > 100 * se.max()


# ---------------------------------------------------------------- 4. / 5. the GPU parity cases, from the restatement alone
_case_cache = {}


def _case(nh, nl, xd, N, k):
    key = (nh, nl, xd, N, k)
    if key not in _case_cache:
        x, P, mask = IM.shape_inputs(nh, nl, xd)
        x, mask = x[:N], mask[:N]
        mu, sigma = IM.encoder_heads(P, x, mask)
        eps = IM.draws(N, k, nl)
        _case_cache[key] = (IM.restate(P, x, mask, mu, sigma, eps, np.float64), IM.restate(P, x, mask, mu.astype(np.float32), sigma.astype(np.float32), eps, np.float32))
    return _case_cache[key]


@pytest.mark.parametrize("nh,nl,xd", IM.SHAPES)
def test_the_weights_matter_at_the_gpu_cases(nh, nl, xd):
    """N = 5, k = 70: the weights are spread (median ESS/k >= 0.3, no draw holds more than half) and xhat is at least 1e-3 away from the
    unweighted mean of the decoder means -- 100 times the 1e-5 floor of the GPU test's tolerance, so a kernel that ignores the weights or
    takes the top-weight draw fails there."""
    r, _ = _case(nh, nl, xd, 5, 70)
    frac = r["ess"] / 70.0
    unweighted = float(np.max(np.abs(r["xhat"] - r["p"].mean(axis=0))))
    top = r["p"][np.argmax(r["al"], axis=0), np.arange(5)]
    print("ESS/k %s, max al %.3g, from the unweighted mean %.3g, from the top-weight draw %.3g" % (frac, r["al"].max(), unweighted, np.max(np.abs(r["xhat"] - top))))
    assert np.median(frac) >= 0.3 and r["al"].max() <= 0.5
    assert unweighted >= 1e-3 and np.max(np.abs(r["xhat"] - top)) >= 1e-3


@pytest.mark.parametrize("N,k", IM.CASES, ids=IM.CASE_IDS)
@pytest.mark.parametrize("nh,nl,xd", IM.SHAPES)
def test_tolerances_are_admissible(nh, nl, xd, N, k):
    """The GPU tests allow 8 x (float32 restatement - float64 restatement), floor 1e-5: that figure stays small enough to mean something."""
    r64, r32 = _case(nh, nl, xd, N, k)
    d_lw = float(np.max(np.abs(r32["log_w"].astype(np.float64) - r64["log_w"])))
    d_xh = float(np.max(np.abs(r32["xhat"].astype(np.float64) - r64["xhat"])))
    print("float32 restatement off the float64 one: log_w %.3g, xhat %.3g" % (d_lw, d_xh))
    assert d_lw <= 1e-4 and d_xh <= 2e-6
    assert np.all(r64["xhat"] >= 0.0) and np.all(r64["xhat"] <= 1.0)
