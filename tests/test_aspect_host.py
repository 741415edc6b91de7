"""Admissibility of the aspect-ratio cases (tests/_aspect_cases.py) from the oracle alone -- no GPU.

The conditions are on the INPUTS and the SHAPES, not measurements of the device:
  * every oracle output is finite;
  * each shape has the property its comment claims (Dp > Hp, the k-step counts, no pad lane, the LDS request), computed from the widths
    with the rounding rules of layout.h / model.hip (iwae_create);
  * exact-oracle admissibility: a case whose GPU body holds the gradient to the EXACT float64 oracle must have the rounding-aware oracle
    within (that bound - the body's bound against the rounding-aware oracle) of the exact one, per tensor: EXACT_GRAD_REL - EMU_GRAD_REL =
    0.02 for the 1-layer bodies, 0.03 / 0.04 for the 2-layer body (_aspect_cases.admit_limit) -- that leaves the device what it is allowed
    against the rounding-aware oracle.  If a case misses, its seed changes, never a bound;
  * resolved accept decisions: in the float64 restatement of an AIS case at least 0.9 of the chains have |log u + dH| > 1e-4.

Every test prints its figures next to their bounds (pytest -rP shows them)."""
import os
import re

import numpy as np
import pytest

from oracle import iwae_np as O
import _ais_ref as R
import _local_q_ref as LQ
import _aspect_cases as A
import _row_eval_bodies as RB

RESOLVED_MIN = 0.9
ONE_ROUNDING_MAX = 1e-5      # the floor of the run-time tolerance of tests/test_gpu_local_q.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _finite(tree):
    if isinstance(tree, dict):
        return all(_finite(v) for v in tree.values())
    if isinstance(tree, (list, tuple)):
        return all(_finite(v) for v in tree)
    return bool(np.all(np.isfinite(np.asarray(tree, dtype=np.float64))))


@pytest.mark.parametrize("c", A.STEP_CASES, ids=A.case_id)
def test_step_case_is_admissible(c):
    res_x, g_x = A.oracle(c, False)
    res_e, g_e = A.oracle(c, True)
    assert _finite(res_x) and _finite(res_e) and _finite(g_x) and _finite(g_e)
    dist = A.grad_distance(g_e, g_x)
    limit = A.admit_limit(c)
    print("%s: rounding-aware vs exact gradient, worst tensor %.4f (<= %.3g%s)" % (A.case_id(c), max(dist), limit, "" if c.exact_grad else ": not held, no exact-oracle gradient check"))
    if c.exact_grad:
        assert max(dist) <= limit, dist


def test_shapes_have_the_properties_their_comments_claim():
    w = {name: A.widths(name) for name in A.SHAPES}
    for name, v in w.items():
        print(name, {k: v[k] for k in ("Hp", "Dp", "Xp32", "KT_H", "KT_D", "KT_X", "T16_H", "T16_D", "T16_X")})
    t = w["A_TILE"]       # one hidden 32-step under the widest latent, heads 256 wide, latent KT 4, all 8 latent tiles live, Dp > Hp
    assert t["KT_H"] == [1] and t["Dp"] == [128] and 2 * t["Dp"][0] == 256 and t["KT_D"] == [4] and t["T16_D"] == [A.AIS_DT] and t["D"][0] == 16 * A.AIS_DT
    assert t["Dp"][0] > t["Hp"][0]
    o = w["A_ODD"]        # every width odd, D > H > X, H one past a 32-step, the last latent quad cut at 3 of 4
    assert all(n % 2 == 1 for n in (o["H"][0], o["D"][0], o["X"])) and o["D"][0] > o["H"][0] > o["X"]
    assert o["H"][0] % 32 == 1 and o["D"][0] % 4 == 3 and o["Dp"][0] > o["Hp"][0] and o["T16_D"] == [A.AIS_DT]
    r = w["A_REF"]        # the reference's latent and pixels, hidden KT 2 < latent KT 4
    assert (r["D"][0], r["X"]) == (100, 784) and r["KT_H"] == [2] and r["KT_D"] == [4]
    f = w["A_FULL"]       # exact tiles, no pad lane anywhere; KT 7 as at (200, 100, 784)
    assert f["H"] == f["Hp"] and f["D"] == f["Dp"] and f["X"] == f["Xp32"] and f["KT_H"] == [7] and f["KT_H"] == [A.round_up(200, 32) // 32]
    assert f["Dp"] == [A.round_up(100, 32)]
    th = w["A_THIN"]      # x narrower than one 16-tile under a wider latent
    assert th["X"] < 16 and th["D"][0] > th["H"][0] > th["X"]
    mx = w["AN_MAX"]      # the row-evaluation maximum: 13 + 8 tiles, 155 904 bytes, the grid posterior's x limit
    assert mx["T16_H"] == [A.AIS_NT] and mx["T16_D"] == [A.AIS_DT] and mx["Xp32"] == 800 and A.round_up(801, 32) > 800
    assert A.row_eval_lds_bytes("ais", 128, 208) == 155904 and A.row_eval_lds_bytes("ais", 100, 200) == 151808
    for kern in ("ais", "local_q", "impute"):
        top = max(A.row_eval_lds_bytes(kern, D, H) for H in range(1, 209) for D in (1, 16, 64, 100, 127, 128))
        assert top == A.row_eval_lds_bytes(kern, 128, 208) <= 160 * 1024, (kern, top)      # the largest request is AN_MAX's, inside 160 KB of LDS
    # Dp > Hp (16-feature tiles here): local_q / impute widen their g strips to the latent, ais_chain_kernel does not
    for name in ("A_TILE", "A_ODD"):
        H, D = w[name]["H"][0], w[name]["D"][0]
        assert A.round_up(D, 16) > A.round_up(H, 16)
        assert A.row_eval_lds_bytes("local_q", D, H) > A.row_eval_lds_bytes("ais", D, H)
    i2 = w["L2_INV"]      # both hidden layers narrower than the latent they feed
    assert i2["H"][0] < i2["D"][0] and i2["H"][1] < i2["D"][1] and i2["H"][1] < i2["D"][0]
    f2 = w["L2_FULL"]     # the chain kernels' 4/4/2 with every latent lane live
    assert (f2["KT_D"][0], f2["KT_H"][1], f2["KT_D"][1]) == (4, 4, 2) and f2["D"] == f2["Dp"] and f2["H"] == f2["Hp"]
    assert (A.round_up(100, 32) // 32, A.round_up(100, 32) // 32, A.round_up(50, 32) // 32) == (4, 4, 2)      # ... reached through padding at the reference's widths
    c = w["C_INV"]
    assert c["D"][0] > c["H"][0] and c["D"][0] + A.C_INV_COND <= c["Dp"][0]


def test_constants_are_the_headers():
    src = open(os.path.join(ROOT, "iwae_amd", "csrc", "kernels.h")).read()
    for name in ("AIS_NT", "AIS_DT", "AIS_TPO", "AIS_SLABP"):
        assert int(re.search(r"#define %s (\d+)" % name, src).group(1)) == getattr(A, name), name
    ais = open(os.path.join(ROOT, "iwae_amd", "csrc", "ais_kernels.hip")).read()
    assert "ais_pz(Dp) + 2 * (Hp + 4)" in ais and "(Dp > 16 * AIS_TPO ? Dp : 16 * AIS_TPO) + 4" in ais
    for f, ph in (("local_kernels.hip", "lq_ph"), ("impute_kernels.hip", "im_ph")):
        assert re.search(r"int %s\(int Dp, int Hp\) \{ return \(Hp > Dp \? Hp : Dp\) \+ 4; \}" % ph, open(os.path.join(ROOT, "iwae_amd", "csrc", f)).read()), f


def test_case_table_covers_what_the_module_claims():
    assert all(c.B * c.k <= 40 and c.B % 4 for c in A.FEW_1L) and {c.shape for c in A.FEW_1L} == set(A.SHAPES_1L)
    assert {c.obj for c in A.FEW_1L} == {"iwae_elbo", "dreg", "iwae_eq14", "vae_elbo", "vae_elbo_kl"} and any(c.beta != 1.0 for c in A.FEW_1L)
    rows = sorted({c.B * c.k for c in A.ROWS_1L})
    assert 4096 < rows[0] < 4200 and rows[1:] == [6000, 8500] and max(c.B * c.k for c in A.STEP_CASES) <= 8500
    assert {c.shape for c in A.ROWS_1L} == {"A_TILE", "A_REF", "A_FULL", "A_ODD"} and {c.obj for c in A.ROWS_1L} == {"iwae_elbo", "dreg"}
    assert all(c.k <= 257 for c in A.STEP_CASES)


@pytest.mark.parametrize("init", ["encoder", "prior"])
@pytest.mark.parametrize("L", A.AIS_LS)
@pytest.mark.parametrize("N,Cn", A.AIS_CASES)
@pytest.mark.parametrize("name", A.ROW_EVAL)
def test_ais_accept_decisions_are_resolved(name, N, Cn, L, init):
    nh, nl, xd = A.SHAPES[name]
    x, P = A.analysis_inputs(name)
    x = x[:N]
    if init == "encoder":
        mu, sg = O._Block(P[0:4], O._id).fwd(np.asarray(x, dtype=np.float64))
    else:
        mu, sg = np.zeros((N, nl)), np.ones((N, nl))
    eps0, mom, unif = A.ais_noise(N, Cn, L, nl)
    e64 = R.restate(P, x, mu, sg, A.AIS_BETAS, L, A.AIS_H, eps0, mom, unif, np.float64)
    e32 = R.restate(P, x, mu.astype(np.float32), sg.astype(np.float32), A.AIS_BETAS, L, A.AIS_H, eps0, mom, unif, np.float32)
    share = float(np.mean(np.abs(e64["margin"][0]) > 1e-4))
    dev = float(np.max(np.abs(e32["dH"].astype(np.float64) - e64["dH"])))
    print("%s N%d C%d L%d %s: resolved share %.3f (>= %.1f), accept rate %.3f, float32 dH deviation %.3g" % (name, N, Cn, L, init, share, RESOLVED_MIN, e64["accepted"].mean(), dev))
    assert _finite(e64["dH"]) and _finite(e64["log_w"]) and _finite(e64["z"])
    assert share >= RESOLVED_MIN
    assert 1e-5 < 8.0 * dev < 1e-2      # the GPU test's run-time tolerance: above its floor, and far below what a mis-addressed tile moves (dH ~ 1)


@pytest.mark.parametrize("objective", LQ.OBJECTIVES)
@pytest.mark.parametrize("N,S", A.LOCAL_CASES)
@pytest.mark.parametrize("name", A.ROW_EVAL)
def test_local_posterior_case_is_well_conditioned(name, N, S, objective):
    """Finite; the float32 deviation the GPU test's run-time tolerance is built from stays far below a mis-addressed tile; and the case does
    not amplify: with the decoder's weights moved by ONE float32 rounding (6e-8 relative, 12 seeded draws, float64 arithmetic otherwise) no
    element of the last iteration's gradient moves by more than ONE_ROUNDING_MAX = 1e-5, the floor of that tolerance.  A case that misses
    changes its noise seed (tests/_aspect_cases.py LOCAL_SEEDS says which did)."""
    nh, nl, xd = A.SHAPES[name]
    x, P = A.analysis_inputs(name)
    x = x[:N]
    T = A.LOCAL_T
    mu, sg = (a.astype(np.float32) for a in O._Block(P[0:4], O._id).fwd(np.asarray(x, dtype=np.float64)))
    noise = RB.local_noise(N, S, T, nl, seed=A.local_seed(name, N, S))
    e64 = LQ.restate(P, x, mu, sg, noise, T, objective, lr=0.05, dtype=np.float64)
    e32 = LQ.restate(P, x, mu, sg, noise, T, objective, lr=0.05, dtype=np.float32)
    dev = {key: float(np.max(np.abs(np.asarray(e32[key], dtype=np.float64) - e64[key]))) for key in ("grad", "mu", "log_w")}
    rng = np.random.default_rng(1)
    moved = 0.0
    for _ in range(12):
        Q = [(W * (1.0 + 6e-8 * rng.standard_normal(W.shape)), b * (1.0 + 6e-8 * rng.standard_normal(b.shape))) for W, b in P]
        moved = max(moved, float(np.max(np.abs(LQ.restate(Q, x, mu, sg, noise, T, objective, lr=0.05, dtype=np.float64)["grad"] - e64["grad"]))))
    print("%s N%d S%d %s seed %d: one float32 rounding of the weights moves grad by %.3g (<= %.3g); float32 deviation grad %.3g, mu %.3g, log_w %.3g; |grad| max %.3g"
          % (name, N, S, objective, A.local_seed(name, N, S), moved, ONE_ROUNDING_MAX, dev["grad"], dev["mu"], dev["log_w"], float(np.max(np.abs(e64["grad"])))))
    assert all(_finite(e64[key]) for key in ("grad", "bound", "mu", "sigma", "elbo", "iwae", "log_w"))
    assert 8.0 * dev["grad"] < 0.05 * float(np.max(np.abs(e64["grad"])))      # the tolerance separates a wrong tile from rounding
    assert moved <= ONE_ROUNDING_MAX


@pytest.mark.parametrize("name", A.ROW_EVAL)
def test_impute_mask_leaves_an_image_nothing_in_the_last_tile(name):
    nh, nl, xd = A.SHAPES[name]
    x, P, mask = A.impute_inputs(name)
    last = 16 * ((xd - 1) // 16)
    assert not mask[1, last:].any() and mask[0, last:].any() or xd - last == 1      # (x_dim = 17: the last tile is one pixel wide)
    assert not mask[1, last:].any() and mask[1, :last].any() and mask.shape == (A.NMAX, xd)
    assert _finite(O.flatten_params(P))
