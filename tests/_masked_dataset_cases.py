"""The case table of the resident per-image masks (iwae_dataset_set_mask / iwae_dataset_mcar_mask / iwae_dataset_get_mask and the masked
iwae_train_step_dataset, include/iwae_amd.h): test_masked_dataset_host.py shows its admissibility on the CPU,
test_gpu_masked_dataset.py runs it on the GPU.  Not a test module.

Shapes, data and batches are the smallest at which the word indexing (ceil(x_dim / 32) mask words per image, bit f & 31 of word f >> 5), the
pad rows and the range checks can go wrong.  Two things the table cannot hold literally, and how it holds them instead:
  * an image that observes everything and a pixel column nobody observes cannot share a batch, so the "full" images of the half mask observe
    every pixel BUT the dead column; the mask of ones is the fully observed case;
  * a batch of one image holds one image: (0, 1) holds an empty image, (299, 1) a full one (CLAIMS says which batch holds what).
The special images sit at fixed POSITIONS of the order, and both orders of the table keep those positions, so the claims hold in every epoch.
"""
import collections
import functools

import numpy as np

import _masked_ref as MR
import _masked_bf16_cases as BC
import _masked_cases as MC

N, K = 300, 5
# dims (hidden, latent, x_dim); mask words per image; pixels the last word holds
Shape = collections.namedtuple("Shape", "dims words last_fill")
SHAPES = [
    Shape((200, 100, 784), 25, 16),      # the last word half used
    Shape((37, 5, 53), 2, 21),           # odd x_dim: a cut last chunk, no 4-pixel group stores
    Shape((64, 8, 100), 4, 4),
    Shape((128, 16, 384), 12, 32),       # whole words and whole pixel groups
]
DIMS = [s.dims for s in SHAPES]
WIDE = DIMS[0]
# (start, B): ragged; the first image; the last image; a batch that ends on the set's last image
BATCHES = [(37, 150), (0, 1), (299, 1), (172, 128)]
EMPTY_AT, FULL_AT = (0, 40, 180), (299, 41, 181)      # positions of the order that hold an image with nothing / everything (but the dead column) observed
DEAD_COLUMN = 5
CLAIMS = {(37, 150): ("empty", "full", "dead"), (0, 1): ("empty", "dead"), (299, 1): ("full", "dead"), (172, 128): ("empty", "full", "dead")}
EPOCHS = (1, 6)      # the epoch of ORDERS[0] and of ORDERS[1]
MCAR_RATES, MCAR_SEEDS = (0.0, 0.3, 0.5, 1.0), (5, (1 << 40) + 77)
REFUSED_BF16 = [d for d, _ in BC.REFUSED]      # (16, 4, 48), (256, 16, 64): no stored-s backward pass at these hidden widths
OBJECTIVES5 = ("vae_elbo", "iwae_elbo", "iwae_eq14", "vae_elbo_kl", "dreg")


def mask_words(X):
    return (X + 31) // 32


def fast_route_accepts(dims):
    return MC.fast_route_accepts(*dims)


@functools.lru_cache(maxsize=None)
def gray(X):
    """uint8 grey levels [N, X], random, with columns of 0 and columns of 255 (a tenth of the width each)."""
    g = (np.random.default_rng(3).random((N, X)) * 256).astype(np.uint8)
    c = max(1, X // 10)
    g[:, :c] = 0
    g[:, c:2 * c] = 255
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def orders():
    """Two visiting orders that agree at the special positions and nowhere else on purpose."""
    rng = np.random.default_rng(11)
    a = rng.permutation(N).astype(np.int32)
    fixed = np.array(sorted(EMPTY_AT + FULL_AT))
    free = np.setdiff1d(np.arange(N), fixed)
    b = a.copy()
    b[free] = a[free][rng.permutation(free.size)]
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def half_mask(X):
    """50 % random [N, X] uint8 (1 = observed) with the empty images, the full images and the dead column of the table."""
    from iwae_amd.utils import mcar_mask
    m = mcar_mask((N, X), 0.5, seed=41)
    o = orders()[0]
    for p in EMPTY_AT:
        m[o[p]] = 0
    for p in FULL_AT:
        m[o[p]] = 1
    m[:, DEAD_COLUMN] = 0
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def ones_mask(X):
    m = np.ones((N, X), np.uint8)
    m.setflags(write=False)
    return m


MASKS = {"half": half_mask, "ones": ones_mask}


@functools.lru_cache(maxsize=None)
def params(dims):
    """Spread parameters of a shape (the masked tests' own: _masked_ref.case)."""
    return MR.case(*dims, 5, 13)[1]


def pack_bits(mask):
    """The resident form restated: uint32 [n, words], pixel f = bit f & 31 of word f >> 5."""
    n, X = mask.shape
    W = mask_words(X)
    padded = np.zeros((n, 32 * W), np.uint64)
    padded[:, :X] = mask != 0
    return (padded.reshape(n, W, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def unpack_bits(bits, X):
    n, W = bits.shape
    return ((bits[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).reshape(n, 32 * W)[:, :X].astype(np.uint8)
