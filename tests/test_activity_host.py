"""Host-side pieces of the active-units statistic (no GPU): the C declaration and its ctypes binding, the tasks/active_units.py
driver's flags (main.py's plus --weights) and its default weights path, and the strict `> threshold` count (Burda et al. section 5.2)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from iwae_amd import _capi, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_capi_binds_latent_activity():
    with open(os.path.join(ROOT, "include", "iwae_amd.h")) as f:
        h = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    decl = re.search(r"int iwae_latent_activity\(([^;]*)\);", h)
    assert decl, "iwae_latent_activity is not declared"
    params = [p.strip() for p in decl.group(1).split(",")]
    types = [" ".join(p.split()[:-1]) for p in params]
    assert types == ["iwae_handle", "const float*", "int32_t", "int32_t", "const float*", "double*", "double*", "float*"], types
    res, args = _capi.SYMBOLS["iwae_latent_activity"]
    assert res is C.c_int and len(args) == 8
    assert args[2] is C.c_int32 and args[3] is C.c_int32
    assert args[5] == C.POINTER(C.c_double) and args[6] == C.POINTER(C.c_double)
    assert "activity_kernels.hip" in _capi._ID_SOURCES
    with open(os.path.join(ROOT, "iwae_amd", "csrc", "build.sh")) as f:
        b = f.read()
    assert "activity_kernels.hip" in b and "activity_kernels.o" in b


def _driver():
    sys.path.insert(0, os.path.join(ROOT, "tasks"))
    try:
        sys.modules.pop("active_units", None)
        import active_units
        return active_units
    finally:
        sys.path.pop(0)


def test_driver_parser_is_mains_plus_weights():
    import main
    d = _driver()
    before = sorted(a.dest for a in main.parser._actions)
    a = d.make_parser().parse_args([])
    want = dict(vars(main.parser.parse_args([])), weights=None)
    assert vars(a) == want
    assert sorted(a.dest for a in main.parser._actions) == before      # main.parser is not mutated
    a = d.make_parser().parse_args(["--stochastic_layers", "2", "--n_samples", "50", "--objective", "vae_elbo", "--weights", "/x/w.npz"])
    assert (a.stochastic_layers, a.n_samples, a.objective, a.weights) == (2, 50, "vae_elbo", "/x/w.npz")
    a = d.make_parser().parse_args(["--stochastic_layers", "2", "--n_samples", "50"])
    assert d.default_weights(a) == "/tmp/iwae/main_iwae_elbo_2_50/final_weights.npz"
    with pytest.raises(SystemExit):
        d.make_parser().parse_args(["--stochastic_layers", "3"])


def test_count_active_is_strict():
    a = np.array([0.0, 1e-2, np.nextafter(1e-2, 1.0), 0.5, 1e-3])
    assert utils.count_active(a) == 2
    assert utils.count_active(a, threshold=0.0) == 4
    assert utils.count_active(a, threshold=0.5) == 0
    assert utils.count_active([]) == 0
