"""Host-side pieces of the gradient moments (no GPU): the C declaration of iwae_grad_moments and its ctypes binding, the new
translation unit in the build and the build id, utils.gradient_snr_summary on constructed moments, and the tasks/gradient_snr.py
driver's flags and default weights paths."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from iwae_amd import _capi, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_capi_binds_grad_moments():
    with open(os.path.join(ROOT, "include", "iwae_amd.h")) as f:
        h = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    decl = re.search(r"int iwae_grad_moments\(([^;]*)\);", h)
    assert decl, "iwae_grad_moments is not declared"
    params = [p.strip() for p in decl.group(1).split(",")]
    types = [" ".join(p.split()[:-1]) for p in params]
    assert types == ["iwae_handle", "const float*", "int32_t", "int32_t", "float", "int32_t", "int32_t", "double*", "double*"], types
    res, args = _capi.SYMBOLS["iwae_grad_moments"]
    assert res is C.c_int and len(args) == 9
    assert args[1] is C.c_void_p
    assert args[2] is C.c_int32 and args[3] is C.c_int32 and args[4] is C.c_float and args[5] is C.c_int32 and args[6] is C.c_int32
    assert args[7] == C.POINTER(C.c_double) and args[8] == C.POINTER(C.c_double)


def test_build_lists_moments_kernels():
    assert "moments_kernels.hip" in _capi._ID_SOURCES
    with open(os.path.join(ROOT, "iwae_amd", "csrc", "build.sh")) as f:
        b = f.read()
    assert "moments_kernels.hip" in b and "moments_kernels.o" in b
    ids = re.search(r"for f in ([^;]*); do", b).group(1).split()
    assert [os.path.basename(f) for f in ids] == [os.path.basename(f) for f in _capi._ID_SOURCES]     # same files, same order
    with open(os.path.join(ROOT, "iwae_amd", "csrc", "kernels.h")) as f:
        k = f.read()
    assert "launch_moments_fold" in k and "launch_moments_finalize" in k


TABLE = [("enc1.l1/kernel", (3, 2), 0), ("enc1.l1/bias", (2,), 6), ("enc2.l1/bias", (2,), 8),
         ("dec2.l1/bias", (1,), 10), ("dec1.d1/kernel", (2, 2), 11)]


def test_snr_summary_excludes_zero_variance_and_groups_by_prefix():
    n = 15
    mean = np.linspace(-2.0, 3.0, n)
    var = np.linspace(0.5, 4.0, n)
    var[[0, 7, 12]] = 0.0          # one zero-variance parameter in enc1.l1/kernel, enc1.l1/bias and dec1.d1/kernel each
    s = utils.gradient_snr_summary(mean, var, TABLE)
    enc, dec = np.arange(0, 10), np.arange(10, 15)
    for name, idx in (("encoder", enc), ("decoder", dec)):
        nz = idx[var[idx] > 0]
        assert s[name]["snr"] == pytest.approx(np.mean(np.abs(mean[nz]) / np.sqrt(var[nz])), rel=1e-14)
        assert s[name]["signal"] == pytest.approx(np.sum(mean[idx] ** 2), rel=1e-14)
        assert s[name]["variance"] == pytest.approx(np.sum(var[idx]), rel=1e-14)
        assert s[name]["n"] == idx.size
    assert s["encoder"]["n"] == 10                     # enc1 and enc2 both belong to the encoder
    assert set(s["tensors"]) == {t[0] for t in TABLE}
    t = s["tensors"]["enc1.l1/bias"]                   # [6, 8): parameter 7 has var 0
    assert t["n"] == 2 and t["snr"] == pytest.approx(abs(mean[6]) / np.sqrt(var[6]), rel=1e-14)
    s0 = utils.gradient_snr_summary(mean, np.zeros(n), TABLE)
    assert np.isnan(s0["encoder"]["snr"]) and s0["encoder"]["variance"] == 0.0
    with pytest.raises(ValueError):
        utils.gradient_snr_summary(mean[:-1], var, TABLE)


def test_snr_summary_of_a_known_distribution():
    rng = np.random.default_rng(0)
    mu = rng.standard_normal(4000)
    sd = rng.uniform(0.5, 2.0, 4000)
    s = utils.gradient_snr_summary(mu, sd ** 2, [("enc.l1/kernel", (4000,), 0)])
    assert s["encoder"]["snr"] == pytest.approx(np.mean(np.abs(mu) / sd), rel=1e-12)
    assert s["decoder"]["n"] == 0


def _driver():
    sys.path.insert(0, os.path.join(ROOT, "tasks"))
    try:
        sys.modules.pop("gradient_snr", None)
        import gradient_snr
        return gradient_snr
    finally:
        sys.path.pop(0)


def test_driver_parser_is_mains_plus_four_flags():
    import main
    d = _driver()
    before = sorted(a.dest for a in main.parser._actions)
    a = d.make_parser().parse_args([])
    want = dict(vars(main.parser.parse_args([])), weights=None, k_list="1,5,50,500,5000", draws=1000, estimator=None)
    assert vars(a) == want
    assert sorted(a.dest for a in main.parser._actions) == before      # main.parser is not mutated
    a = d.parse_args(["--n_samples", "50", "--k_list", "1,5", "--draws", "8", "--estimator", "dreg", "--weights", "/x/w.npz"])
    assert (a.n_samples, a.k_values, a.draws, d.estimator(a), a.weights) == (50, [1, 5], 8, "dreg", "/x/w.npz")


def test_driver_default_weights():
    d = _driver()
    a = d.parse_args(["--stochastic_layers", "2", "--n_samples", "50"])
    assert d.estimator(a) == "iwae_elbo"
    assert d.default_weights(a) == "/tmp/iwae/main_iwae_elbo_2_50/final_weights.npz"
    a = d.parse_args(["--objective", "vae_elbo"])
    assert d.default_weights(a) == "/tmp/iwae/main_vae_elbo_1_5/final_weights.npz"
    a = d.parse_args(["--n_samples", "50", "--estimator", "dreg"])
    assert d.default_weights(a) == "/tmp/iwae/task02_50/final_weights.npz"


def test_driver_rejects_dreg_with_two_layers_and_bad_lists():
    d = _driver()
    for argv in (["--stochastic_layers", "2", "--estimator", "dreg"], ["--k_list", "1,0"], ["--k_list", "a"], ["--draws", "1"],
                 ["--estimator", "stl"]):
        with pytest.raises(SystemExit):
            d.parse_args(argv)
