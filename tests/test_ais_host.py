"""Host-side pieces of annealed importance sampling (no GPU): the C declaration and its ctypes binding, the build id's source list, the
annealing schedules, and identities the float64 restatement of iwae_ais's formulas (tests/_ais_ref.py) must satisfy: one temperature step
is the importance weight, a vanishing step size telescopes to it for any schedule, and on a model with two latent dimensions the forward
and the reverse run bracket the quadrature value of log p(x) (Grosse et al. 2015)."""
import ctypes as C
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import iwae_np as O  # noqa: E402
import make_golden as MG  # noqa: E402
import _ais_ref as R  # noqa: E402


def _header():
    return open(os.path.join(ROOT, "include", "iwae_amd.h")).read()


def test_header_declares_and_capi_binds_ais():
    from iwae_amd import _capi
    h = _header()
    decl = re.search(r"int iwae_ais\(([^;]*)\);", h)
    assert decl, "iwae_ais is not declared"
    assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == 5
    res, args = _capi.SYMBOLS["iwae_ais"]
    assert res is C.c_int and len(args) == 5
    assert args[3] is C.POINTER(_capi.AisOptions) and args[4] is C.POINTER(_capi.AisOutputs)


def _typedef_fields(name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.search(r"(\w+)\s*$", f.strip()).group(1) for f in body.split(";") if f.strip()]


def test_struct_layouts_match_binding():
    from iwae_amd import _capi
    o = _capi.AisOptions
    assert [f[0] for f in o._fields_] == _typedef_fields("iwae_ais_options")
    assert [f[0] for f in _capi.AisOutputs._fields_] == _typedef_fields("iwae_ais_outputs")
    # the numbers model.hip static_asserts
    assert C.sizeof(o) == 72 and o.struct_size.offset == 0 and o.C.offset == 4 and o.T.offset == 8 and o.L.offset == 12
    assert o.betas.offset == 16 and o.step_size.offset == 24 and o.adapt.offset == 28 and o.init.offset == 32
    assert o.z0.offset == 40 and o.eps0.offset == 48 and o.mom.offset == 56 and o.unif.offset == 64
    assert o().struct_size == 72
    assert C.sizeof(_capi.AisOutputs) == 10 * C.sizeof(C.c_void_p)
    src = open(os.path.join(ROOT, "iwae_amd", "csrc", "model.hip")).read()
    assert "sizeof(iwae_ais_options) == 72" in src and "sizeof(iwae_ais_outputs) == 10 * sizeof(void*)" in src
    assert _capi.AIS_INITS == {"encoder": 0, "prior": 1}
    assert re.search(r"IWAE_AIS_INIT_ENCODER = 0, IWAE_AIS_INIT_PRIOR = 1", _header())


def test_build_id_covers_ais_kernels():
    from iwae_amd import _capi
    assert "ais_kernels.hip" in _capi._ID_SOURCES
    b = open(os.path.join(ROOT, "iwae_amd", "csrc", "build.sh")).read()
    assert "ais_kernels.hip" in b and "ais_kernels.o" in b
    assert b.count("ais_kernels.hip") >= 2       # the id list and the compile line


def test_build_id_list_matches_build_sh():
    from iwae_amd import _capi
    b = open(os.path.join(ROOT, "iwae_amd", "csrc", "build.sh")).read()
    listed = re.search(r"BUILD_ID=\$\(for f in (.*?); do", b).group(1).split()
    assert [os.path.basename(f) for f in listed] == [os.path.basename(f) for f in _capi._ID_SOURCES]     # same files, same order


def test_driver_parser_is_mains_plus_the_samplers_flags():
    import main
    sys.path.insert(0, os.path.join(ROOT, "tasks"))
    try:
        for name in ("ais_llh", "active_units"):
            sys.modules.pop(name, None)
        import ais_llh
    finally:
        sys.path.pop(0)
    before = sorted(a.dest for a in main.parser._actions)
    a = ais_llh.make_parser().parse_args([])
    assert vars(a) == dict(vars(main.parser.parse_args([])), weights=None, images=1000, chains=16, temps=1000, leapfrog=10, step=0.1,
                           no_adapt=False, init="encoder", bdmc=16)
    assert sorted(a.dest for a in main.parser._actions) == before      # main.parser is not mutated
    a = ais_llh.make_parser().parse_args(["--temps", "50", "--init", "prior", "--no-adapt", "--bdmc", "0"])
    assert (a.temps, a.init, a.no_adapt, a.bdmc) == (50, "prior", True, 0)


def test_option_and_tool_are_documented():
    readme = open(os.path.join(ROOT, "tools", "README.md")).read()
    assert "ais_t_chunk" in readme and "dev/ais_time.py" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "dev", "ais_time.py"))
    assert "iwae_ais" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_schedules():
    from iwae_amd.native import ais_schedule
    for kind in ("sigmoid", "linear"):
        for T in (1, 2, 7, 1000):
            b = ais_schedule(T, kind)
            assert b.dtype == np.float32 and b.shape == (T + 1,)
            assert b[0] == 0.0 and b[-1] == 1.0
            assert np.all(np.diff(b.astype(np.float64)) > 0)
    np.testing.assert_allclose(ais_schedule(4, "linear"), [0, 0.25, 0.5, 0.75, 1.0])
    s = ais_schedule(1000, "sigmoid").astype(np.float64)
    assert s[500] == 0.5 or abs(s[500] - 0.5) < 1e-6
    assert s[100] < 0.1 * 0.9 and s[900] > 1 - 0.1 * 0.9       # slower than linear near both ends: Wu et al.'s point
    try:
        ais_schedule(5, "cosine")
    except ValueError:
        pass
    else:
        raise AssertionError("an unknown schedule must raise")


def _small(nh, nl, xd, N, seed):
    x, P, _ = MG.inputs(1, nh, nl, xd, N, 1, seed)
    rng = np.random.default_rng(seed + 5)
    mu = 0.3 * rng.standard_normal((N, nl))
    sg = np.exp(0.3 * rng.standard_normal((N, nl)) - 0.5)
    return x, P, mu, sg


def _importance_weight(P, x, mu, sg, e):
    """log p(x|z) + log p(z) - log q(z|x) at z = mu + sg e, from the oracle's own densities; e [C, N, D]."""
    dec = R.decoder_of(P, np.float64)
    z = mu[None] + sg[None] * e
    l = R.logits_of(dec, z.reshape(-1, z.shape[-1]))[2].reshape(z.shape[:2] + (-1,))
    lpx = O.bernoulli_log_prob(np.asarray(x, dtype=np.float64)[None], l).sum(-1)
    lpz = O.normal_log_prob(z, 0.0, 1.0).sum(-1)
    lq = O.normal_log_prob(z, mu[None], sg[None]).sum(-1)
    return lpx + lpz - lq


def test_one_temperature_is_the_importance_weight():
    x, P, mu, sg = _small(16, 4, 48, 3, 31)
    eps0, mom, unif = R.noise(32, 1, 5, 3, 4)
    r = R.restate(P, x, mu, sg, [0.0, 1.0], 3, 0.2, eps0, mom, unif)
    np.testing.assert_allclose(r["log_w"], _importance_weight(P, x, mu, sg, eps0.astype(np.float64)), rtol=1e-12, atol=1e-12)


def test_vanishing_step_telescopes_for_any_schedule():
    x, P, mu, sg = _small(16, 4, 48, 3, 33)
    betas = np.array([0.2, 0.25, 0.6, 0.4, 0.9, 0.95, 0.7], dtype=np.float32)
    T = betas.size - 1
    eps0, mom, unif = R.noise(34, T, 5, 3, 4)
    r = R.restate(P, x, mu, sg, betas, 2, 1e-30, eps0, mom, unif)
    want = np.float64(betas[-1] - betas[0]) * _importance_weight(P, x, mu, sg, eps0.astype(np.float64))
    np.testing.assert_allclose(r["log_w"], want, rtol=1e-6, atol=1e-6)       # (the float32 schedule's differences, summed, are off by ~1e-8 relative)
    np.testing.assert_allclose(r["z"], mu[None] + sg[None] * eps0, rtol=0, atol=1e-25)


def test_forward_and_reverse_runs_bracket_quadrature():
    """64/2/48 model, data simulated from the model so that the reverse run starts from exact posterior samples."""
    from iwae_amd.native import ais_schedule
    _, P, _ = MG.inputs(1, 64, 2, 48, 4, 1, 41)
    N, Cn, T, L, h = 4, 64, 200, 5, 0.3
    rng = np.random.default_rng(42)
    zt = rng.standard_normal((N, 2))
    probs = O.sigmoid(R.logits_of(R.decoder_of(P, np.float64), zt)[2])
    x = (rng.random(probs.shape) < probs).astype(np.float64)
    truth = R.quadrature_log_px(P, x)
    mu, sg = np.zeros((N, 2)), np.ones((N, 2))
    betas = ais_schedule(T, "sigmoid")
    eps0, mom, unif = R.noise(43, T, Cn, N, 2)
    fwd = R.restate(P, x, mu, sg, betas, L, h, eps0, mom, unif)
    _, mom2, unif2 = R.noise(44, T, Cn, N, 2)
    rev = R.restate(P, x, mu, sg, betas[::-1], L, h, eps0, mom2, unif2, z0=np.broadcast_to(zt[None], (Cn, N, 2)))
    lower, se_l = R.log_mean_exp(fwd["log_w"]), R.log_mean_se(fwd["log_w"])
    upper, se_u = -R.log_mean_exp(rev["log_w"]), R.log_mean_se(rev["log_w"])
    print("truth", truth, "lower", lower, "se", se_l, "upper", upper, "se", se_u, "accept", fwd["accepted"].mean(), rev["accepted"].mean())
    assert np.all(np.abs(lower - truth) <= 4 * se_l), (lower - truth, se_l)
    assert np.all(np.abs(upper - truth) <= 4 * se_u), (upper - truth, se_u)
    assert np.all(lower - 4 * se_l <= truth) and np.all(truth <= upper + 4 * se_u)
    # plain importance sampling from the same draws is the looser bound on average
    one = R.restate(P, x, mu, sg, [0.0, 1.0], L, h, eps0, mom[:1], unif[:1])
    assert np.mean(np.abs(R.log_mean_exp(one["log_w"]) - truth)) > np.mean(np.abs(lower - truth))
