"""Host-side pieces of the per-image posterior optimisation (no GPU): the float64 restatement of iwae_local_posterior's formulas
(tests/_local_q_ref.py) against torch autograd and the oracle's Adam, what the optimiser reaches on a model with two latent dimensions
against quadrature, and the C declaration, its ctypes binding, the build lists and the documents."""
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
import _local_q_ref as LQ  # noqa: E402


# ---------------------------------------------------------------- (a) the ascent direction is the gradient of the bound
def _torch_bound(P, x, mu, rho, e, objective):
    import torch
    (W1, b1), (W2, b2), (W3, b3) = [(torch.tensor(np.asarray(W, dtype=np.float64)), torch.tensor(np.asarray(b, dtype=np.float64))) for W, b in P[-3:]]
    x, e = torch.tensor(x), torch.tensor(e)
    z = mu[None] + torch.exp(rho)[None] * e
    l = torch.tanh(torch.tanh(z @ W1 + b1) @ W2 + b2) @ W3 + b3
    c = 0.5 * np.log(2.0 * np.pi)
    lpx = torch.sum(x[None] * l - torch.nn.functional.softplus(l), dim=-1)
    lpz = torch.sum(-0.5 * z * z - c, dim=-1)
    lq = torch.sum(-0.5 * e * e - rho[None] - c, dim=-1)
    lw = lpx + lpz - lq
    return lw.mean(dim=0) if objective == "elbo" else torch.logsumexp(lw, dim=0) - np.log(e.shape[0])


@pytest.mark.parametrize("objective", LQ.OBJECTIVES)
def test_grad_is_autograd_of_the_bound(objective):
    import torch
    x, P, _ = MG.inputs(1, 16, 4, 48, 3, 1, 31)
    rng = np.random.default_rng(7)
    N, D, S = 3, 4, 5
    mu, rho = 0.3 * rng.standard_normal((N, D)), 0.3 * rng.standard_normal((N, D)) - 0.5
    e = rng.standard_normal((S, N, D))
    x = x.astype(np.float64)
    bound, dmu, drho, _ = LQ.bound_and_grad(R.decoder_of(P, np.float64), x, mu, rho, e, objective)
    tm, tr = torch.tensor(mu, requires_grad=True), torch.tensor(rho, requires_grad=True)
    tb = _torch_bound(P, x, tm, tr, e, objective)
    tb.sum().backward()            # (an image's bound depends on its own mu, rho only)
    assert np.max(np.abs(bound - tb.detach().numpy())) <= 1e-10
    assert np.max(np.abs(dmu - tm.grad.numpy())) <= 1e-10
    assert np.max(np.abs(drho - tr.grad.numpy())) <= 1e-10


# ---------------------------------------------------------------- (b) Adam
def test_adam_is_the_oracles_with_the_sign_flipped():
    rng = np.random.default_rng(11)
    th, m, v = rng.standard_normal(40), np.zeros(40), np.zeros(40)
    tho, mo, vo = th.copy(), m.copy(), v.copy()
    for t in range(1, 6):
        g = rng.standard_normal(40)
        th, m, v = LQ.adam_ascent(th, g, m, v, t, 0.05)
        tho, mo, vo = O.adam_update(tho, -g, mo, vo, t, 0.05)
        assert np.array_equal(th, tho) and np.array_equal(m, -mo) and np.array_equal(v, vo)
    th2, _, _ = LQ.adam_ascent(th, g, m, v, 6, 0.01, beta_1=0.5, beta_2=0.9, epsilon=1e-3)
    tho2, _, _ = O.adam_update(tho, -g, mo, vo, 6, 0.01, beta1=0.5, beta2=0.9, eps=1e-3)
    assert np.array_equal(th2, tho2)


# ---------------------------------------------------------------- (c) what the optimiser reaches
def test_optimiser_closes_the_gap_to_quadrature():
    """64/2/48 model: ELBO, T = 200, S = 16, lr = 0.05 from the encoder heads.  The exact ELBO (quadrature) at the result closes at least
    half of each image's gap between the encoder's exact ELBO and quadrature log p(x), and never exceeds log p(x)."""
    x, P, _ = MG.inputs(1, 64, 2, 48, 4, 1, 41)
    mu0, sg0 = LQ.encoder_heads(P, x)
    eps = np.random.default_rng(5).standard_normal((200, 16, 4, 2))
    r = LQ.restate(P, x, mu0, sg0, eps, 200, "elbo", lr=0.05)
    truth = R.quadrature_log_px(P, x)
    before, after = LQ.exact_elbo(P, x, mu0, sg0), LQ.exact_elbo(P, x, r["mu"], r["sigma"])
    closed = (after - before) / (truth - before)
    print("log_px", truth, "encoder gap", truth - before, "gap left", truth - after, "closed", closed)
    assert np.all(after <= truth)
    assert np.all(closed >= 0.5)


# ---------------------------------------------------------------- (d) declaration, binding, build lists, documents
def _header():
    return open(os.path.join(ROOT, "include", "iwae_amd.h")).read()


def _typedef_fields(name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for f in body.split(";"):
        if f.strip():
            names += [re.search(r"(\w+)\s*$", part.strip()).group(1) for part in f.split(",")]
    return names


def test_struct_layouts_match_binding():
    from iwae_amd import _capi
    h = _header()
    decl = re.search(r"int iwae_local_posterior\(([^;]*)\);", h)
    assert decl, "iwae_local_posterior is not declared"
    assert len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == 5
    res, args = _capi.SYMBOLS["iwae_local_posterior"]
    assert res is C.c_int and len(args) == 5
    assert args[3] is C.POINTER(_capi.LocalOptions) and args[4] is C.POINTER(_capi.LocalOutputs)
    o = _capi.LocalOptions
    assert [f[0] for f in o._fields_] == _typedef_fields("iwae_local_options")
    assert [f[0] for f in _capi.LocalOutputs._fields_] == _typedef_fields("iwae_local_outputs")
    # the numbers model.hip static_asserts
    assert C.sizeof(o) == 64 and o.struct_size.offset == 0 and o.S.offset == 4 and o.T.offset == 8 and o.E.offset == 12 and o.objective.offset == 16
    assert o.lr.offset == 20 and o.beta_1.offset == 24 and o.beta_2.offset == 28 and o.epsilon.offset == 32
    assert o.mu0.offset == 40 and o.sigma0.offset == 48 and o.eps.offset == 56
    assert o().struct_size == 64
    assert C.sizeof(_capi.LocalOutputs) == 9 * C.sizeof(C.c_void_p)
    src = open(os.path.join(ROOT, "iwae_amd", "csrc", "model.hip")).read()
    assert "sizeof(iwae_local_options) == 64" in src and "sizeof(iwae_local_outputs) == 9 * sizeof(void*)" in src
    assert _capi.LOCAL_OBJECTIVES == {"elbo": 0, "iwae": 1}
    assert re.search(r"IWAE_LOCAL_ELBO = 0, IWAE_LOCAL_IWAE = 1", h)


def test_build_lists_cover_local_kernels():
    from iwae_amd import _capi
    assert "local_kernels.hip" in _capi._ID_SOURCES
    b = open(os.path.join(ROOT, "iwae_amd", "csrc", "build.sh")).read()
    assert b.count("local_kernels.hip") >= 2 and b.count("local_kernels.o") >= 2      # the id list, the compile line and the link line
    listed = re.search(r"BUILD_ID=\$\(for f in (.*?); do", b).group(1).split()
    assert [os.path.basename(f) for f in listed] == [os.path.basename(f) for f in _capi._ID_SOURCES]


def test_option_tool_and_driver_are_there():
    readme = open(os.path.join(ROOT, "tools", "README.md")).read()
    assert "local_t_chunk" in readme and "dev/local_q_time.py" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "dev", "local_q_time.py"))
    assert "iwae_local_posterior" in open(os.path.join(ROOT, "DESIGN.md")).read()
    import main
    sys.path.insert(0, os.path.join(ROOT, "tasks"))
    try:
        import inference_gaps
    finally:
        sys.path.pop(0)
    before = sorted(a.dest for a in main.parser._actions)
    a = inference_gaps.make_parser().parse_args([])
    assert vars(a) == dict(vars(main.parser.parse_args([])), weights=None, images=1000, draws=16, iters=500, eval_passes=64, local_lr=0.05,
                           chains=16, temps=1000, leapfrog=10, step=0.1)
    assert sorted(a.dest for a in main.parser._actions) == before      # main.parser is not mutated


def test_gap_split_sums():
    from iwae_amd import utils
    rng = np.random.default_rng(3)
    lp, ea, el = rng.standard_normal(7) - 80, rng.standard_normal(7) - 90, rng.standard_normal(7) - 85
    g = utils.inference_gap_split(lp, ea, el)
    assert np.max(np.abs(g["approximation_gap"] + g["amortization_gap"] - (lp - ea))) <= 1e-12
    lw = rng.standard_normal((50, 7))
    np.testing.assert_allclose(utils.mean_se(lw), LQ.mean_se(lw), rtol=1e-14)
    np.testing.assert_allclose(utils.log_mean_exp_se(lw), R.log_mean_se(lw), rtol=1e-14)
