"""The case table of the masked float32 step's edge tests (test_masked_edges_host.py on the CPU, test_gpu_masked_edges.py on the GPU): the
shapes, row counts, mask structures and parameter states that tests/test_gpu_masked_step.py does not reach.  Not a test module.

The reference is tests/_masked_ref.py (masked_loss_grads, float64 torch autograd).  Every tolerance the GPU module uses is one the project
already holds float32 mode to (tests/_parity_common.py); no bound is introduced here.  If a case misses one, change its seed, its number of
sharp units or its scale -- never a bound -- and say so in its comment.

The tile arithmetic below restates masked_out_f32_kernel (masked_kernels.hip: MO_TP = 13 pixel tiles of 16 per pass, NT = ceil(X / 16),
npass = ceil(NT / 13), TP = ceil(NT / npass), pass p starts at tile t0 = p TP) and gemm_f32_fewrows_split (fp32_kernels.hip, default
options), which the kernel's KSPLIT instantiation follows; test_masked_edges_host.py holds the table to that arithmetic.
"""
import collections
import functools

import numpy as np

from oracle import iwae_np as O
import make_golden as MG
import _masked_ref as MR
import _offinit_cases as OC
from _parity_common import spread_params

MO_TP, MO_MAX_H = 13, 208


# ---------------------------------------------------------------- the kernel's host arithmetic, restated
def pixel_plan(X):
    """(tiles, passes, TP, first tile of every pass, live columns of the last tile) of masked_out_f32_kernel at x_dim X."""
    nt = (X + 15) // 16
    npass = (nt + MO_TP - 1) // MO_TP
    tp = (nt + npass - 1) // npass
    return nt, npass, tp, tuple(p * tp for p in range(npass)), X - 16 * (nt - 1)


def k_chunks(M, X, H, ksplit=True):
    """The widths of the K chunks launch_gemm_f32_fewrows gives the output layer's product [M, H] x [H, X] at the default options
    (gemm_f32_fewrows_split); one chunk: no split."""
    if not ksplit or M > 4096 or X % 4 or H < 96:
        return (H,)
    tiles = ((M + 63) // 64) * ((X + 63) // 64)
    if tiles >= 256:
        return (H,)
    ns = min(16 if tiles < 8 else 8, (256 + tiles - 1) // tiles, H // 48)
    if ns < 2:
        return (H,)
    kchunk = ((H + ns - 1) // ns + 15) // 16 * 16
    return tuple(min(kchunk, H - c) for c in range(0, H, kchunk))


def kslabs(M, X, H, ksplit=True):
    """MaskedOutF32Args::kslabs of forward_f32: 16-row weight slabs per K chunk; 0: the KSPLIT = false instantiation."""
    c = k_chunks(M, X, H, ksplit)
    return 0 if len(c) == 1 else c[0] // 16


def w3_offset(H, L, X):
    """The first float of W3 inside the flat parameters (Keras layout: W1 b1 W2 b2 Wmu bmu Wsd bsd D1 c1 D2 c2 W3 b3)."""
    return X * H + H + H * H + H + 2 * (H * L + L) + L * H + H + H * H + H


def fast_route_accepts(H, L, X):
    """masked_out_f32_ok: H <= 208, X a multiple of 4, W3 (and with it b3) 16-byte aligned inside the flat parameters."""
    return 1 <= H <= MO_MAX_H and X >= 4 and X % 4 == 0 and w3_offset(H, L, X) % 4 == 0


# ---------------------------------------------------------------- shapes
# dims; H % 4; X % 16; pixel tiles, passes, TP, pass starts, live columns of the last tile; K chunks of the output layer at <= 130 rows
Shape = collections.namedtuple("Shape", "dims h_mod4 x_mod16 tiles passes tp starts last_cols chunks")
EDGE_SHAPES = [
    # odd H: the scalar strip load of g2; three weight slabs, the last with 5 live rows of 16; no K split (H < 96).  14 pixel tiles in two
    # passes of 7, the second at t0 = 7 (t0 & 3 = 3); the last tile has 4 live columns
    Shape((37, 6, 212), 1, 4, 14, 2, 7, (0, 7), 4, (37,)),
    # odd H WITH the K split: chunks 64 + 37 (kslabs 4), the last slab 5 rows.  One pass of 4 tiles, the last 4 columns wide
    Shape((101, 6, 52), 1, 4, 4, 1, 4, (0,), 4, (64, 37)),
    # H = 2 mod 4: scalar load; chunks 64 / 64 / 22.  27 tiles: three passes of 9 at t0 = 0, 9, 18 (t0 & 3 = 0, 1, 2)
    Shape((150, 33, 420), 2, 4, 27, 3, 9, (0, 9, 18), 4, (64, 64, 22)),
    # two whole chunks of 64.  24 tiles: two passes of 12, the second at t0 = 12: t0 & 3 == 0 at a pass that is not the first; X whole tiles
    Shape((128, 16, 384), 0, 0, 24, 2, 12, (0, 12), 16, (64, 64)),
    # the smallest H that splits: 48 + 48 (kslabs 3).  The smallest X the predicate takes: one tile of 4 live columns
    Shape((96, 8, 4), 0, 4, 1, 1, 1, (0,), 4, (48, 48)),
]
EDGE_DIMS = [s.dims for s in EDGE_SHAPES]
# forced "fast", refused by masked_out_f32_ok: X % 4 == 1; W3 misaligned (offset = 1 mod 4) with X % 4 == 0; H > 208
FALLBACK_DIMS = [(37, 5, 53), (101, 7, 52), (224, 16, 48)]
WIDE = (200, 100, 784)
EDGE_CASES = [(1, 1), (3, 7), (20, 1), (5, 13), (2, 64)]          # MR.CASES without (1, 130)
# 200 / 100 / 784, rt = 64-row tiles: (9, 50) = 450 rows, rt 8: chunks 80 / 80 / 40, kslabs 5; (20, 50) = 1 000 rows, rt 16: 112 / 88, kslabs 7 (the
# reference's default batch); (40, 50) = 2 000 rows, rt 32: 416 tiles >= 256, no split below 4 096 rows
MID_CASES = [(9, 50), (20, 50), (40, 50)]
MID_CHUNKS = {(9, 50): (80, 80, 40), (20, 50): (112, 88), (40, 50): (200,)}
MID_OBJECTIVES = ("iwae_elbo", "dreg")
ROUTES = dict(MR.ROUTES)
ROUTES["general_noksplit"] = dict(MR.ROUTES["general"], f32_no_ksplit=1)
ROUTES["fast_noksplit"] = dict(MR.ROUTES["fast"], f32_no_ksplit=1)


# ---------------------------------------------------------------- mask structures
def dead_tile_index(X):
    """The one observed 16-pixel tile of `tile`: interior, a third of the way in (784: tile 16, so passes 0, 2 and 3 of the kernel are dead; 212: tile 4, pass 1 dead)."""
    return ((X + 15) // 16) // 3


def mask_tophalf(B, X, seed):
    """case_mask with pixels [0, X / 2) cleared in every image."""
    m = MR.case_mask(B, X, seed).copy()
    m[:, :X // 2] = 0
    return m


def mask_tile(B, X, seed):
    """Only one interior 16-pixel tile is observed, in every image."""
    m = np.zeros((B, X), np.uint8)
    t = dead_tile_index(X)
    m[:, 16 * t:16 * t + 16] = 1
    return m


def mask_none(B, X, seed):
    """Every image empty."""
    return np.zeros((B, X), np.uint8)


def mask_stripes64(B, X, seed):
    """A pixel is observed iff (j // 64) % 2 == 0: the general route's lane stride."""
    m = np.zeros((B, X), np.uint8)
    m[:, (np.arange(X) // 64) % 2 == 0] = 1
    return m


def mask_dense95(B, X, seed):
    from iwae_amd.utils import mcar_mask
    return mcar_mask((B, X), 0.05, seed=seed)


def mask_sparse05(B, X, seed):
    from iwae_amd.utils import mcar_mask
    return mcar_mask((B, X), 0.95, seed=seed)


MASKS = {"case": MR.case_mask, "tophalf": mask_tophalf, "tile": mask_tile, "none": mask_none, "stripes64": mask_stripes64,
         "dense95": mask_dense95, "sparse05": mask_sparse05}
STRUCTURES = ("tophalf", "tile", "none", "stripes64", "dense95", "sparse05")
STRUCT_SHAPES = [WIDE, (37, 6, 212)]
STRUCT_CASES = [(5, 13), (2, 64)]
NEVER_OBSERVED = ("tophalf", "tile", "none", "stripes64")          # structures with pixel columns no image of the batch observes


def never_observed(mask):
    """The pixel columns observed in no image of the batch."""
    return np.flatnonzero(np.asarray(mask).sum(axis=0) == 0)


@functools.lru_cache(maxsize=None)
def struct_case(shape, case, structure):
    """(x, P, eps, mask) of MR.case with the mask of a structure (the seed of MR.case's own mask)."""
    x, P, eps, _ = MR.case(*shape, *case)
    B, k = case
    return x, P, eps, MASKS[structure](B, shape[2], 17 + B + k)


@functools.lru_cache(maxsize=None)
def struct_reference(shape, case, structure, objective, beta=1.0):
    """masked_loss_grads of a structure's case, computed once and shared; read only."""
    x, P, eps, mask = struct_case(shape, case, structure)
    return MR.masked_loss_grads(P, x, mask, eps, beta, objective)


# ---------------------------------------------------------------- off the random initialisation (section 6)
# _offinit_cases.stress on spread_params, under case_mask and tophalf; B = 5, k = 8 at 200 / 100 / 784 unless named.  Sharp posteriors stay at
# the wide shape: at 37 / 6 / 212 a plain float32 restatement without the rounding-aware z - mu is off by up to 0.66 per gradient tensor.
OFFINIT = [
    OC.case(5, 8, "iwae_elbo"), OC.case(5, 8, "dreg"), OC.case(5, 8, "vae_elbo_kl", 0.7),                         # sharp, four units, SHIFTS4
    OC.case(5, 8, "iwae_elbo", sharp=0, sat=OC.SAT), OC.case(5, 8, "dreg", sharp=0, sat=OC.SAT),                   # saturated
    OC.case(5, 8, "iwae_elbo", sharp=0, wide=OC.WIDE),                                                            # wide
    OC.case(5, 8, "iwae_elbo", sat=OC.SAT),                                                                       # sharp + saturated
    OC.case(5, 8, "iwae_elbo", sharp=0, sat=OC.SAT, widths=(150, 33, 420)),                                        # saturated at an edge shape
]
OFFINIT_BIG = OC.case(170, 50, "iwae_elbo")          # 8 500 rows, two sharp units, default options
OFFINIT_MASKS = ("case", "tophalf")


def offinit_mask(c, structure):
    return MASKS[structure](c.B, c.widths[2], 17 + c.B + c.k)


@functools.lru_cache(maxsize=None)
def offinit_inputs(c, structure):
    """(x, P, eps, mask): _offinit_cases.inputs' stressed parameters and the structure's mask."""
    x, _, P, eps, _ = OC.inputs(c)
    return x, P, eps, offinit_mask(c, structure)


@functools.lru_cache(maxsize=None)
def offinit_reference(c, structure):
    x, P, eps, mask = offinit_inputs(c, structure)
    return MR.masked_loss_grads(P, x, mask, eps, c.beta, c.obj)


def offinit_id(v):
    return OC.case_id(v) if isinstance(v, OC.Case) else v


# ---------------------------------------------------------------- state across calls (section 7)
def step_masks(B, X, n, seed=301):
    """n different 50 % MCAR masks for the steps of a trajectory (case_mask: the special images included)."""
    return [MR.case_mask(B, X, seed + 7 * t) for t in range(n)]


@functools.lru_cache(maxsize=None)
def plain_inputs(shape, B, k, seed):
    """(x, P, eps): make_golden.inputs at spread_params."""
    x, P, eps = MG.inputs(1, *shape, B, k, seed)
    return x, spread_params(P, 1), eps


def unflatten(flat, P):
    """The flat device parameters as the oracle's [(W, b) ...] in float64, shaped like P."""
    out, off = [], 0
    flat = np.asarray(flat, dtype=np.float64)
    for W, b in P:
        w = flat[off:off + W.size].reshape(W.shape)
        off += W.size
        v = flat[off:off + b.size].reshape(b.shape)
        off += b.size
        out.append((w.copy(), v.copy()))
    assert off == flat.size
    return out


def tensor_slices(P):
    """(start, stop) of every tensor (W0, b0, W1, ...) in the flat parameters."""
    out, off = [], 0
    for W, b in P:
        for t in (W, b):
            out.append((off, off + t.size))
            off += t.size
    return out


def adam_host(theta, g, m, v, t, lr=1e-3):
    """One float64 Keras Adam step (oracle.adam_update) with the running moments kept by the caller: (theta, m, v)."""
    return O.adam_update(np.asarray(theta, np.float64), np.asarray(g, np.float64), m, v, t, lr)
