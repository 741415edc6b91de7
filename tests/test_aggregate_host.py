"""Host-side pieces of the aggregate-posterior decomposition (no GPU): the C declaration and its ctypes binding, the build id's source
list, the tasks/elbo_surgery.py driver's flags (main.py's plus --weights and --draws), and the identities the float64 restatement
(tests/_aggregate_ref.py) must satisfy: kl = mi + tc + dim_kl and mi <= log N (Hoffman & Johnson 2016)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from iwae_amd import _capi
from _aggregate_ref import restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_capi_binds_aggregate_posterior():
    with open(os.path.join(ROOT, "include", "iwae_amd.h")) as f:
        h = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    decl = re.search(r"int iwae_aggregate_posterior\(([^;]*)\);", h)
    assert decl, "iwae_aggregate_posterior is not declared"
    params = [p.strip() for p in decl.group(1).split(",")]
    types = [" ".join(p.split()[:-1]) for p in params]
    assert types == ["iwae_handle", "const float*", "int32_t", "int32_t", "const float*", "double*", "double*", "double*",
                     "float*", "float*", "float*", "float*"], types
    res, args = _capi.SYMBOLS["iwae_aggregate_posterior"]
    assert res is C.c_int and len(args) == 12
    assert args[2] is C.c_int32 and args[3] is C.c_int32
    assert all(args[i] == C.POINTER(C.c_double) for i in (5, 6, 7))


def test_build_id_covers_the_new_source():
    assert "aggregate_kernels.hip" in _capi._ID_SOURCES
    with open(os.path.join(ROOT, "iwae_amd", "csrc", "build.sh")) as f:
        b = f.read()
    assert "aggregate_kernels.hip" in b and "aggregate_kernels.o" in b
    listed = re.search(r"BUILD_ID=\$\(for f in (.*?); do", b).group(1).split()
    assert [os.path.basename(f) for f in listed] == [os.path.basename(f) for f in _capi._ID_SOURCES]     # same files, same order
    assert re.fullmatch(r"[0-9a-f]{16}", _capi.source_build_id())


def _driver():
    sys.path.insert(0, os.path.join(ROOT, "tasks"))
    try:
        for name in ("elbo_surgery", "active_units"):
            sys.modules.pop(name, None)
        import elbo_surgery
        return elbo_surgery
    finally:
        sys.path.pop(0)


def test_driver_parser_is_mains_plus_weights_and_draws():
    import main
    d = _driver()
    before = sorted(a.dest for a in main.parser._actions)
    a = d.make_parser().parse_args([])
    assert vars(a) == dict(vars(main.parser.parse_args([])), weights=None, draws=1)
    assert sorted(a.dest for a in main.parser._actions) == before      # main.parser is not mutated
    a = d.make_parser().parse_args(["--n_samples", "50", "--objective", "vae_elbo", "--weights", "/x/w.npz", "--draws", "10"])
    assert (a.n_samples, a.objective, a.weights, a.draws) == (50, "vae_elbo", "/x/w.npz", 10)
    with pytest.raises(SystemExit):
        d.make_parser().parse_args(["--draws", "many"])


@pytest.mark.parametrize("N,S,D", [(1, 2, 5), (7, 1, 3), (40, 3, 9)])
def test_restatement_identities(N, S, D):
    rng = np.random.default_rng(10 * N + S)
    mu = rng.standard_normal((N, D))
    sigma = np.exp(0.7 * rng.standard_normal((N, D)))
    r = restate(mu, sigma, rng.standard_normal((S, N, D)))
    assert abs(r["kl"] - (r["mi"] + r["tc"] + r["dim_kl"])) <= 1e-12 * (abs(r["mi"]) + abs(r["tc"]) + abs(r["dim_kl"]) + abs(r["kl"])) + 1e-13
    assert r["mi"] <= np.log(N) + 1e-12
    assert np.all(r["lq_own"].sum(axis=2) - r["log_qz"] <= np.log(N) + 1e-12)      # q(z) >= q(z|x_n) / N at every sample
    assert np.all(r["unit_mi"] <= np.log(N) + 1e-12)
    np.testing.assert_allclose(np.sum(r["unit_kl"] + r["unit_mi"]), r["kl"], rtol=1e-12)
    if N == 1:
        assert abs(r["mi"]) <= 1e-12 and np.all(np.abs(r["unit_mi"]) <= 1e-12)
