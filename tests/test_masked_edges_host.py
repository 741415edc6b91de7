"""Admissibility of the masked step's edge cases (tests/_masked_cases.py) from the oracle and the reference alone -- no GPU -- as
test_offinit_host.py does it for the off-initialisation family:
  1. the shape table's claims (H % 4, X % 16, pixel tiles / passes / TP, K chunks, the W3 offset from flatten_params) are the kernel's host
     arithmetic, and between them the accepted shapes hold every property the GPU module is there for;
  2. every mask structure is what its name says; where the GPU module asserts exact zeros (pixel columns no image observes, a batch of
     empty images) the float64 reference gives exact zeros;
  3. every parity case keeps its importance weights spread: median ESS/k >= 0.1 (saturated cases excluded, as in the existing family: they
     are one-hot by construction);
  4. every off-initialisation case under a mask: the NumPy oracle on the sliced models with every operand rounded to float32 is within HALF
     of each float32 bound of the exact one (rows F32_ROW_ATOL, scalars F32_SCALAR_REL + 2e-4, gradient F32_GRAD_REL per tensor);
  5. negative controls at the sharp case under a mask: dropping the sigma floor, or taking the exp derivative as sigma, moves a compared
     quantity by more than its bound.
Every test prints its figures next to their bounds (pytest -rP shows them)."""
import numpy as np
import pytest
import torch

from oracle import iwae_np as O
from oracle import iwae_torch as T
import make_golden as MG
import _masked_cases as MC
import _masked_ref as MR
import _offinit_cases as OC
from _parity_common import F32_GRAD_REL, F32_ROW_ATOL, F32_SCALAR_REL, ess_fraction
from test_offinit_host import _mutant

ESS_MIN = 0.10


def _rel(a, b):
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def _ids(v):
    return "%d_%d_%d" % v if isinstance(v, tuple) and len(v) == 3 else "B%d_k%d" % v if isinstance(v, tuple) else str(v)


# ---------------------------------------------------------------- 1. the shape table
@pytest.mark.parametrize("s", MC.EDGE_SHAPES, ids=lambda s: "%d_%d_%d" % s.dims)
def test_edge_shape_is_what_its_comment_says(s):
    H, L, X = s.dims
    assert (H % 4, X % 16) == (s.h_mod4, s.x_mod16)
    assert MC.pixel_plan(X) == (s.tiles, s.passes, s.tp, s.starts, s.last_cols)
    assert s.tiles == -(-X // 16) and s.passes == -(-s.tiles // 13) and s.tp * s.passes >= s.tiles > s.tp * (s.passes - 1) and s.tp <= 13
    for B, k in MC.EDGE_CASES:          # one split for every row count of the family (at most 130 rows: at most three 64-row tiles)
        assert MC.k_chunks(B * k, X, H) == s.chunks, (B, k)
        assert MC.k_chunks(B * k, X, H, ksplit=False) == (H,)
    assert sum(s.chunks) == H and all(c % 16 == 0 for c in s.chunks[:-1])
    assert (len(s.chunks) > 1) == (H >= 96)
    # the W3 offset: the closed form, the flat layout itself, and with the Keras layout 2 H^2 + 3 H L + 2 L (mod 4) once X % 4 == 0
    x, P, eps = MG.inputs(1, H, L, X, 2, 3, 1)
    off = sum(W.size + b.size for W, b in P[:6])
    assert off == MC.w3_offset(H, L, X) and O.flatten_params(P).size == off + H * X + X
    assert P[6][0].shape == (H, X)
    assert off % 4 == (2 * H * H + 3 * H * L + 2 * L) % 4 == 0
    assert MC.fast_route_accepts(H, L, X)
    print("%s: H %% 4 = %d, X %% 16 = %d, %d tiles in %d passes of %d at %s, last tile %d columns, K chunks %s (kslabs %d), W3 offset %d = 0 mod 4"
          % (s.dims, s.h_mod4, s.x_mod16, s.tiles, s.passes, s.tp, s.starts, s.last_cols, s.chunks, MC.kslabs(65, X, H), off))


def test_the_accepted_shapes_hold_every_property_between_them():
    S = MC.EDGE_SHAPES
    assert {s.h_mod4 for s in S} >= {0, 1, 2}                                   # an H the float4 strip load cannot take, odd and even
    assert any(s.h_mod4 and len(s.chunks) > 1 for s in S)                        # ... with the K split
    assert any(s.x_mod16 == 4 for s in S) and any(s.x_mod16 == 0 for s in S)
    assert {s.tp for s in S} >= {7, 9, 12} and 13 not in {s.tp for s in S}
    assert any(t0 > 0 and t0 & 3 == 0 for s in S for t0 in s.starts)
    assert {t0 & 3 for s in S for t0 in s.starts} == {0, 1, 2, 3}
    assert any(s.dims[2] == 4 for s in S) and min(s.dims[0] for s in S if len(s.chunks) > 1) == 96
    assert MC.k_chunks(1, 4, 95) == (95,)                                        # (96 is the smallest H that splits)
    # 200 / 100 / 784: the split by 64-row tiles
    H, L, X = MC.WIDE
    split = {rt: MC.k_chunks(64 * rt, X, H) for rt in range(1, 66)}
    assert all(split[rt] == (64, 64, 64, 8) for rt in range(1, 7))
    assert all(split[rt] == (80, 80, 40) for rt in range(7, 10))
    assert all(split[rt] == (112, 88) for rt in range(10, 20))
    assert all(split[rt] == (200,) for rt in range(20, 66))
    assert MC.k_chunks(4097, X, H) == (200,)
    for (B, k), chunks in MC.MID_CHUNKS.items():
        assert MC.k_chunks(B * k, X, H) == chunks and 130 < B * k < 4100
    assert [MC.kslabs(B * k, X, H) for B, k in MC.MID_CASES] == [5, 7, 0]
    assert {MC.kslabs(B * k, X, H) for B, k in MR.CASES} == {4} and {MC.kslabs(B * k, X, H) for B, k in MR.BIG_CASES} == {0}
    assert (20, 50) in MC.MID_CASES                                              # the reference's default batch


@pytest.mark.parametrize("dims,why", list(zip(MC.FALLBACK_DIMS, ("x", "w3", "h"))), ids=lambda v: v if isinstance(v, str) else "%d_%d_%d" % v)
def test_fallback_shape_is_refused_for_its_one_reason(dims, why):
    H, L, X = dims
    x, P, eps = MG.inputs(1, H, L, X, 2, 3, 1)
    off = sum(W.size + b.size for W, b in P[:6])
    assert off == MC.w3_offset(H, L, X)
    reasons = {"x": X % 4 != 0, "w3": X % 4 == 0 and off % 4 != 0, "h": H > MC.MO_MAX_H}
    assert reasons[why] and sum(reasons.values()) == 1, reasons
    assert not MC.fast_route_accepts(H, L, X)
    print("%s: X %% 4 = %d, W3 offset %% 4 = %d, H = %d (<= 208: %s)" % (dims, X % 4, off % 4, H, H <= 208))


def test_odd_h_is_aligned_only_at_l_2_mod_4():
    for H in (37, 101):
        for L in range(1, 13):
            assert MC.fast_route_accepts(H, L, 52) == (L % 4 == 2), (H, L)


# ---------------------------------------------------------------- 2. mask structures
@pytest.mark.parametrize("shape", MC.STRUCT_SHAPES, ids=_ids)
def test_mask_structures_are_what_their_names_say(shape):
    X = shape[2]
    for B, k in MC.STRUCT_CASES:
        seed = 17 + B + k
        base = MR.case_mask(B, X, seed)
        m = {name: MC.MASKS[name](B, X, seed) for name in MC.STRUCTURES}
        for name, v in m.items():
            assert v.dtype == np.uint8 and v.shape == (B, X) and set(np.unique(v)) <= {0, 1}, name
        assert not m["tophalf"][:, :X // 2].any() and np.array_equal(m["tophalf"][:, X // 2:], base[:, X // 2:])
        t = MC.dead_tile_index(X)
        assert 0 < t < (X + 15) // 16 - 1 and m["tile"].sum() == 16 * B and m["tile"][:, 16 * t:16 * t + 16].all()
        assert not m["none"].any()
        assert all(bool(m["stripes64"][b, j]) == ((j // 64) % 2 == 0) for b in (0, B - 1) for j in range(X))
        assert 0.90 < m["dense95"].mean() < 0.99 and 0.01 < m["sparse05"].mean() < 0.10
        nv = {name: MC.never_observed(v).size for name, v in m.items()}
        print("%s B = %d: never-observed columns %s" % (shape, B, nv))
        for name in MC.NEVER_OBSERVED:
            assert nv[name] > 0, name
        assert nv["tophalf"] >= X // 2 and nv["tile"] == X - 16 and nv["none"] == X      # (B = 2: case_mask's first image is empty, so more than half)
        # a whole pass of masked_out_f32_kernel is dead under `tile`
        nt, npass, tp, starts, _ = MC.pixel_plan(X)
        assert npass >= 2 and sum(1 for t0 in starts if not (t0 <= t < t0 + tp)) >= 1
    if X == 784:
        assert MC.never_observed(MC.mask_tophalf(5, X, 35)).size == 392 and MC.never_observed(MC.mask_tile(5, X, 35)).size == 768


@pytest.mark.parametrize("structure", MC.STRUCTURES)
@pytest.mark.parametrize("shape", MC.STRUCT_SHAPES, ids=_ids)
def test_reference_is_exactly_zero_where_nothing_is_observed_and_weights_stay_spread(shape, structure):
    case = MC.STRUCT_CASES[0]
    x, P, eps, mask = MC.struct_case(shape, case, structure)
    nv = MC.never_observed(mask)
    for obj in MR.OBJECTIVES:
        res, g = MC.struct_reference(shape, case, structure, obj)
        if nv.size:
            assert np.all(g[6][0][:, nv] == 0.0) and np.all(g[6][1][nv] == 0.0) and np.all(g[0][0][nv, :] == 0.0), obj
        if structure == "none":
            flat = [t for Wb in g for t in Wb]
            assert np.all(res["lpxz"] == 0.0)
            assert [i for i, t in enumerate(flat) if not np.any(t)] == [0, 8, 9, 10, 11, 12, 13], obj
    for c in MC.STRUCT_CASES:
        ess = float(np.median(ess_fraction(MC.struct_reference(shape, c, structure, "iwae_elbo")[0]["al"])))
        print("%s %s B%d k%d: never-observed columns %d, median ESS/k %.3g (>= %.2f)" % (shape, structure, c[0], c[1], nv.size, ess, ESS_MIN))
        assert ess >= ESS_MIN


def _float32_grads(P, x, mask, eps, objective):
    """masked_loss_grads at float32: the same torch graph on float32 tensors (what a device with plain float32 arithmetic would give)."""
    Pt = T.to_torch_params(P, torch.float32)
    flatP = [t for Wb in Pt for t in Wb]
    res = MR.masked_forward(Pt, torch.tensor(np.asarray(x), dtype=torch.float32), torch.tensor(np.asarray(mask) != 0),
                            torch.tensor(np.asarray(eps), dtype=torch.float32), 1.0, dreg=objective == "dreg")
    if objective == "dreg":
        g = list(torch.autograd.grad(res["inference_loss"], flatP[:8], retain_graph=True)) + list(torch.autograd.grad(-res["iwae_elbo"], flatP[8:], allow_unused=True))
    else:
        g = torch.autograd.grad(-res[objective], flatP, allow_unused=True)
    return [np.zeros(p.shape) if gi is None else gi.numpy().astype(np.float64) for gi, p in zip(g, flatP)]


@pytest.mark.parametrize("shape", MC.STRUCT_SHAPES, ids=_ids)
def test_empty_batch_leaves_a_well_conditioned_encoder_gradient(shape):
    """`none`: the encoder tensors 1 .. 7 are what the GPU module holds to F32_GRAD_REL; the float32 restatement is within half of it."""
    worst = 0.0
    for case in MC.STRUCT_CASES:
        x, P, eps, mask = MC.struct_case(shape, case, "none")
        for obj in MR.OBJECTIVES:
            g64 = [t for Wb in MC.struct_reference(shape, case, "none", obj)[1] for t in Wb]
            g32 = _float32_grads(P, x, mask, eps, obj)
            for i in (0, 8, 9, 10, 11, 12, 13):
                assert not np.any(g32[i]), (obj, i)
            worst = max(worst, max(_rel(g32[i], g64[i]) for i in range(1, 8)))
    print("%s none: float32 restatement vs float64, encoder tensors 1..7: %.3g (<= %.3g)" % (shape, worst, F32_GRAD_REL / 2))
    assert worst <= F32_GRAD_REL / 2


# ---------------------------------------------------------------- 3. the weights of every parity case stay spread
@pytest.mark.parametrize("shape", MC.EDGE_DIMS + MC.FALLBACK_DIMS, ids=_ids)
def test_edge_shape_cases_keep_spread_weights(shape):
    for B, k in MC.EDGE_CASES:
        if k == 1:
            continue
        ess = float(np.median(ess_fraction(MR.reference(*shape, B, k, "iwae_elbo")[0]["al"])))
        print("%s B%d k%d: median ESS/k %.3g (>= %.2f)" % (shape, B, k, ess, ESS_MIN))
        assert ess >= ESS_MIN


@pytest.mark.parametrize("case", MC.MID_CASES, ids=_ids)
def test_mid_row_count_cases_keep_spread_weights(case):
    ess = float(np.median(ess_fraction(MR.reference(*MC.WIDE, *case, "iwae_elbo")[0]["al"])))
    print("%s B%d k%d: median ESS/k %.3g (>= %.2f)" % (MC.WIDE, case[0], case[1], ess, ESS_MIN))
    assert ess >= ESS_MIN


# ---------------------------------------------------------------- 4. off the initialisation under a mask
def _f32_scalar_bound(v):
    return F32_SCALAR_REL * abs(v) + 2e-4


def _one_pixel_for_the_empty_image(mask):
    """The NumPy oracle cannot take an image of zero pixels (test_masked_host.py): the empty image gets one."""
    mask = mask.copy()
    for b in np.flatnonzero(mask.sum(axis=1) == 0):
        mask[b, 3] = 1
    return mask


@pytest.mark.parametrize("c,structure", [(c, s) for c in MC.OFFINIT for s in MC.OFFINIT_MASKS] + [(MC.OFFINIT_BIG, "case")], ids=MC.offinit_id)
def test_offinit_case_under_a_mask_is_admissible(c, structure):
    x, P, eps, mask = MC.offinit_inputs(c, structure)
    mask = _one_pixel_for_the_empty_image(mask)
    res_x, g_x = MR.sliced_oracle_grads(P, x, mask, eps, c.beta, c.obj)
    res_f, g_f = MR.sliced_oracle_grads(P, x, mask, eps, c.beta, c.obj, rnd=OC.f32_round)
    rows = max(float(np.max(np.abs(res_f[key] - res_x[key]))) for key in ("lpxz", "lpz", "lqzx"))
    scal = abs(res_f["value"] - res_x["value"]) / _f32_scalar_bound(res_x["value"])
    cond = max(_rel(a, b) for pa, pb in zip(g_f, g_x) for a, b in zip(pa, pb))
    ess = float(np.median(ess_fraction(res_x["al"])))
    print("%s %s: float32-operand vs exact rows %.3g (<= %.3g), scalar %.3g x its bound (<= 0.5), gradient %.3g (<= %.3g), median ESS/k %.3g%s"
          % (OC.case_id(c), structure, rows, F32_ROW_ATOL / 2, scal, cond, F32_GRAD_REL / 2, ess, " (saturated: not held)" if c.sat else " (>= %.2f)" % ESS_MIN))
    assert rows <= F32_ROW_ATOL / 2
    assert scal <= 0.5
    assert cond <= F32_GRAD_REL / 2
    if not c.sat:
        assert ess >= ESS_MIN


# ---------------------------------------------------------------- 5. negative controls at the sharp case under a mask
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("structure", MC.OFFINIT_MASKS)
@pytest.mark.parametrize("c", MC.OFFINIT[:2], ids=MC.offinit_id)
def test_control_mutant_is_seen_under_a_mask(c, structure, which):
    """(a) no floor in the forward sigma, (b) the exp derivative taken as sigma (test_offinit_host.py's mutants): at the sharp case each moves
    the objective value or a gradient tensor by more than the GPU test's float32 bound (by three orders of magnitude); at the same case's
    spread parameters it stays below the bound (the floor is 1e-6 of sigma ~ 1 there: 0.07 .. 0.7 of float32 mode's gradient bound)."""
    x, P, eps, mask = MC.offinit_inputs(c, structure)
    mask = _one_pixel_for_the_empty_image(mask)
    figs = {}
    for name, Pn in (("sharp", P), ("spread", OC.inputs(c)[1])):
        res, g = MR.sliced_oracle_grads(Pn, x, mask, eps, c.beta, c.obj)
        with _mutant(which):
            res_m, g_m = MR.sliced_oracle_grads(Pn, x, mask, eps, c.beta, c.obj)
        figs[name] = max(abs(res_m["value"] - res["value"]) / _f32_scalar_bound(res["value"]),
                         max(_rel(a, b) for pa, pb in zip(g_m, g) for a, b in zip(pa, pb)) / F32_GRAD_REL)
    print("%s %s mutant (%s): sharp %.3g, spread %.3g   [x the bound; sharp needs > 1, spread < 1]" % (OC.case_id(c), structure, which, figs["sharp"], figs["spread"]))
    assert figs["sharp"] > 1.0 and figs["spread"] < 1.0, figs
