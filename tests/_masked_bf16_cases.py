"""The case table of the masked step on bf16 handles: test_masked_bf16_host.py on the CPU, test_gpu_masked_bf16.py on
the GPU.  Not a test module.

Two references, both committed: the exact one is tests/_masked_ref.py::masked_loss_grads (float64 torch autograd); the rounding-aware one is
_masked_ref.sliced_oracle_grads(..., rnd=O.bf16_round), the NumPy oracle on the sliced models with the device's bf16 rounding points.  The
sliced oracle cannot take an image with no observed pixel (its slice has zero columns), so the parity masks are case_mask with
mask[0, 0] = 1; the empty image is tested on the GPU without a reference (lpxz == 0 exactly).

The tile arithmetic restates the bf16 step's layout (layout.h, model.hip): a layer's input width is padded to 32 (KT = k-steps of 32), the
output layer's pixels run in groups of 64; a masked bf16 call needs the output layer's KT in {2, 4, 7} (out_bwd_has_s_mode, masked_bf16_ok).
"""
import collections
import functools

import numpy as np

from oracle import iwae_np as O
import _masked_ref as MR

S_MODE_KT = (2, 4, 7)
OBJECTIVES = MR.OBJECTIVES          # iwae_elbo, vae_elbo, dreg
CASES = [(1, 1), (3, 7), (20, 1), (5, 13), (2, 64)]
# dims (hidden, latent, x_dim); k-steps of the output layer; pixel groups of 64; live pixels of the last group
Shape = collections.namedtuple("Shape", "dims kt groups last")
SHAPES = [
    Shape((200, 100, 784), 7, 13, 16),      # the reference's widths: the last pixel group cut to 16
    Shape((208, 128, 800), 7, 13, 32),      # the last group a half
    Shape((128, 16, 384), 4, 6, 64),        # whole groups only
    Shape((64, 8, 100), 2, 2, 36),
    Shape((37, 5, 53), 2, 1, 53),           # odd x_dim, one cut group
]
DIMS = [s.dims for s in SHAPES]
WIDE = DIMS[0]
# refused on a bf16 handle: no stored-s backward pass at these hidden widths (KT = 1, KT = 8)
REFUSED = [((16, 4, 48), 1), ((256, 16, 64), 8)]
# 200 / 100 / 784 either side of 8 192 rows: 4 100 rows (log p(x|z) as per-pixel-group partial sums, sample_kernel, the 4-wave hole-aware output
# layer) and 10 000 rows (whole rows, dense_kernel's sampled-input mode unless DReG, the 8-wave shape).  Both lie beyond block_fwd_kernel's
# 4 096 rows and dec_bwd_rows_kernel's 1 024: those kernels are the small cases' path.
BIG_CASES = [(82, 50), (200, 50)]
BIG_OBJECTIVES = ("iwae_elbo", "dreg")


def kt_of(width):
    """k-steps of 32 of a layer whose input is `width` wide."""
    return (width + 31) // 32


def pixel_groups(X):
    """(64-pixel groups of the output layer, live pixels of the last one)."""
    g = (X + 63) // 64
    return g, X - 64 * (g - 1)


def parity_mask(B, X, seed):
    """case_mask with one pixel for the image it empties."""
    m = MR.case_mask(B, X, seed).copy()
    m[0, 0] = 1
    return m


@functools.lru_cache(maxsize=None)
def case(shape, bk):
    """(x, P, eps, mask): _masked_ref.case with parity_mask."""
    x, P, eps, _ = MR.case(*shape, *bk)
    return x, P, eps, parity_mask(bk[0], shape[2], 17 + bk[0] + bk[1])


@functools.lru_cache(maxsize=None)
def exact(shape, bk, objective, beta=1.0):
    """masked_loss_grads of a case (float64), computed once and shared; read only."""
    x, P, eps, mask = case(shape, bk)
    return MR.masked_loss_grads(P, x, mask, eps, beta, objective)


@functools.lru_cache(maxsize=None)
def emulated(shape, bk, objective, beta=1.0):
    """The rounding-aware oracle of a case, computed once and shared; read only."""
    x, P, eps, mask = case(shape, bk)
    return MR.sliced_oracle_grads(P, x, mask, eps, beta, objective, rnd=O.bf16_round)


def exact_value(res, objective):
    return float(res["iwae_elbo" if objective == "dreg" else objective])


def densities_at_device_head(m, P, x, mask, eps, nl, beta=1.0):
    """_parity_common._densities_at_device_head restated with the mask: log p(x_obs|z) sums the observed pixels only."""
    head = m.debug_tensor("enc.head").astype(np.float64)
    Dp = head.shape[1] // 2
    mu, sig = head[:, :nl], head[:, Dp:Dp + nl]
    z = mu[None] + sig[None] * np.asarray(eps, dtype=np.float64)
    dec = O._MLP3(P[4:7], O.bf16_round)
    terms = O.bernoulli_log_prob(np.where(mask != 0, np.asarray(x, dtype=np.float64), 0.0)[None], dec.fwd(O.bf16_round(z)))
    lpxz = np.sum(np.where((np.asarray(mask) != 0)[None], terms, 0.0), axis=-1)
    lpz = np.sum(O.normal_log_prob(z, 0.0, 1.0), axis=-1)
    lqzx = np.sum(O.normal_log_prob(z, mu[None], sig[None]), axis=-1)
    return {"lpxz": lpxz, "lpz": lpz, "lqzx": lqzx, "log_w": lpxz + beta * (lpz - lqzx)}
