"""Admissibility of the masked bf16 step's GPU cases (tests/_masked_bf16_cases.py, tests/test_gpu_masked_bf16.py) from the oracles alone
-- no GPU -- as test_masked_edges_host.py does it for the float32 step:
  1. the shape table's structural claims: the output layer's k-steps (KT in {2, 4, 7} for the accepted shapes, 1 and 8 for the refused
     ones), the 64-pixel groups and which of them is cut;
  2. the parity masks are case_mask with one pixel for the image it empties (the sliced oracle cannot take an empty image), and leave
     pixel columns no image observes;
  3. every parity case: the rounding-aware oracle (sliced_oracle_grads with rnd = O.bf16_round, the GPU module's bf16 reference) is within
     HALF of each EXACT bound of the exact float64 masked_loss_grads -- scalars and rows EXACT_SCALAR_ATOL / 2, every gradient tensor
     EXACT_GRAD_REL / 2 -- so a device within EMU_* of the first is within EXACT_* of the second with room to spare; and the importance
     weights stay spread, median ESS/k >= 0.125.
Every test prints its figures next to their bounds (pytest -rP shows them)."""
import numpy as np
import pytest

import _masked_bf16_cases as BC
import _masked_ref as MR
from _parity_common import EXACT_GRAD_REL, EXACT_SCALAR_ATOL, ess_fraction

ESS_MIN = 0.125


def _rel(a, b):
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def _ids(v):
    return "%d_%d_%d" % v if isinstance(v, tuple) and len(v) == 3 else "B%d_k%d" % v if isinstance(v, tuple) else str(v)


# ---------------------------------------------------------------- 1. the shape table
@pytest.mark.parametrize("s", BC.SHAPES, ids=lambda s: "%d_%d_%d" % s.dims)
def test_shape_is_what_its_comment_says(s):
    H, L, X = s.dims
    assert BC.kt_of(H) == s.kt and s.kt in BC.S_MODE_KT
    assert 32 * s.kt in (64, 128, 224)                          # the padded hidden widths a masked bf16 call takes
    assert BC.pixel_groups(X) == (s.groups, s.last)
    assert 64 * (s.groups - 1) + s.last == X and 1 <= s.last <= 64
    print("%s: output layer KT %d (hidden padded to %d), %d pixel groups, the last %d wide" % (s.dims, s.kt, 32 * s.kt, s.groups, s.last))


def test_the_shapes_hold_every_property_between_them():
    S = BC.SHAPES
    assert {s.kt for s in S} == set(BC.S_MODE_KT)
    assert S[0].dims == (200, 100, 784) and (S[0].groups, S[0].last) == (13, 16)      # the reference's widths: the last group cut to 16
    assert S[1].last == 32                                                             # ... a half
    assert any(s.last == 64 and s.groups > 1 for s in S)                               # whole groups only
    assert any(s.dims[2] % 2 == 1 and s.groups == 1 and s.last < 64 for s in S)        # odd x_dim, one cut group
    assert any(s.groups > 1 and s.last % 16 for s in S)                                # a last group cut inside a 16-pixel tile
    for dims, kt in BC.REFUSED:
        assert BC.kt_of(dims[0]) == kt and kt not in BC.S_MODE_KT
    assert [kt for _, kt in BC.REFUSED] == [1, 8]
    assert BC.CASES == [(1, 1), (3, 7), (20, 1), (5, 13), (2, 64)]
    # the two row counts at 200 / 100 / 784: either side of 8 192 rows, both beyond block_fwd_kernel's 4 096 and within the 10 000 the suite allows
    assert [B * k for B, k in BC.BIG_CASES] == [4100, 10000] and BC.BIG_CASES[0][0] * BC.BIG_CASES[0][1] < 8192 <= BC.BIG_CASES[1][0] * BC.BIG_CASES[1][1]


# ---------------------------------------------------------------- 2. the parity masks
@pytest.mark.parametrize("shape", BC.DIMS, ids=_ids)
def test_parity_masks_leave_no_image_empty(shape):
    X = shape[2]
    for B, k in BC.CASES + BC.BIG_CASES:
        x, P, eps, mask = BC.case(shape, (B, k)) if (B, k) in BC.CASES else (None, None, None, BC.parity_mask(B, X, 17 + B + k))
        base = MR.case_mask(B, X, 17 + B + k)
        assert mask.dtype == np.uint8 and mask.shape == (B, X) and set(np.unique(mask)) <= {0, 1}
        assert mask.sum(axis=1).min() >= 1 and mask[0, 0] == 1
        d = np.argwhere(mask != base)
        assert len(d) <= 1 and all(tuple(i) == (0, 0) for i in d)
        if B >= 2:
            assert mask[0].sum() == 1                       # the image case_mask empties: one pixel
        if B >= 3:
            assert mask[1].sum() == 1 and mask[1, X - 1] == 1
        if B >= 4:
            assert mask[B - 1].all()
        if shape != BC.WIDE:
            break          # (the large row counts run at the wide shape only)


# ---------------------------------------------------------------- 3. the two references against each other
@pytest.mark.parametrize("bk", BC.CASES, ids=_ids)
@pytest.mark.parametrize("shape", BC.DIMS, ids=_ids)
def test_rounding_aware_oracle_is_within_half_of_the_exact_bounds(shape, bk):
    B, k = bk
    for obj in BC.OBJECTIVES:
        res_x, g_x = BC.exact(shape, bk, obj)
        res_e, g_e = BC.emulated(shape, bk, obj)
        rows = max(float(np.max(np.abs(res_e[key] - res_x[key]))) for key in ("lpxz", "lpz", "lqzx"))
        scal = abs(res_e["value"] - BC.exact_value(res_x, obj))
        cond = max(_rel(a, b) for pa, pb in zip(g_e, g_x) for a, b in zip(pa, pb))
        ess = float(np.median(ess_fraction(res_x["al"])))
        print("%s B%d k%d %s: rounding-aware vs exact rows %.3g, scalar %.3g (<= %.3g), gradient %.3g (<= %.3g), median ESS/k %.3g (>= %.3g)"
              % (shape, B, k, obj, rows, scal, EXACT_SCALAR_ATOL / 2, cond, EXACT_GRAD_REL / 2, ess, ESS_MIN))
        assert rows <= EXACT_SCALAR_ATOL / 2
        assert scal <= EXACT_SCALAR_ATOL / 2
        assert cond <= EXACT_GRAD_REL / 2
        assert ess >= ESS_MIN


def test_vae_elbo_kl_case_is_admissible():
    """The one vae_elbo_kl case of the GPU module: beta 0.7 at the wide shape, (5, 13)."""
    res_x, g_x = BC.exact(BC.WIDE, (5, 13), "vae_elbo_kl", 0.7)
    res_e, g_e = BC.emulated(BC.WIDE, (5, 13), "vae_elbo_kl", 0.7)
    scal = abs(res_e["value"] - float(res_x["vae_elbo_kl"]))
    cond = max(_rel(a, b) for pa, pb in zip(g_e, g_x) for a, b in zip(pa, pb))
    print("vae_elbo_kl beta 0.7: scalar %.3g (<= %.3g), gradient %.3g (<= %.3g)" % (scal, EXACT_SCALAR_ATOL / 2, cond, EXACT_GRAD_REL / 2))
    assert scal <= EXACT_SCALAR_ATOL / 2 and cond <= EXACT_GRAD_REL / 2
