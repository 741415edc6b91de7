"""The case table of the resident-dataset input path WITHOUT masks (iwae_dataset_upload / iwae_dataset_begin_epoch / iwae_dataset_get_batch /
iwae_dataset_get_labels and the unmasked iwae_train_step_dataset, include/iwae_amd.h): test_dataset_host.py shows its
admissibility on the CPU, test_gpu_dataset.py runs it on the GPU.  Not a test module.  (_masked_dataset_cases.py is the masked call's table.)

Everything the table feeds is integer or bitwise: grey levels, orders, labels, seeds and epochs.  Each shape names the property of
gather_binarize_kernel (row_kernels.hip) it cuts, each batch the block or pad boundary it sits on, and test_dataset_host.py asserts every claim.

Three things the table cannot hold literally, and how it holds them instead:
  * a shape narrower than six pixels cannot have a column of each special grey level: (1, 1, 1) cycles the six levels over the images of its one
    column, so the whole set holds each and a batch of one image holds one;
  * a batch of one image holds one label: (0, 1) holds label 0, (299, 1) label C - 1; every other batch holds both;
  * the negative controls of test_dataset_host.py differ from the restatement in at least one BIT of every (shape, batch, seed, epoch) -- but for
    the two batches of one image of (1, 1, 1), a single draw (CONTROL_EXEMPT, the arithmetic is beside it), and but for the threshold's rounding,
    which moves a threshold by one part in 2^24 (test_dataset_host.py says what holds it instead: PLANTED below).
The special images sit at fixed POSITIONS of the order, and both orders of the table keep those positions, so the claims hold in every epoch.
"""
import collections
import functools

import numpy as np

from oracle import iwae_np as O
from oracle import philox_np

N, K = 300, 5
SEEDS = (123, (1 << 40) + 77)            # the handle's seed (the Philox key): the second has a non-zero high word
EPOCHS = (0, 7, 2 ** 32 - 1)             # the Philox counter word c3: the last is the largest a uint32 holds
SPECIAL = (0, 255, 1, 127, 128, 254)     # grey levels of the columns 0 .. 5 of every set at least six pixels wide
C = 10                                   # cond_dim of the conditional shapes
PLANTED_X = 4096                         # the set that carries the planted pixels (planted() below)

# A model of the table.  nh, nl: ints (1-layer) or tuples (2-layer); C: cond_dim; prior: the learned prior p(z|y); step: False for the shapes
# whose train step is outside this table (inspection calls only).
Model = collections.namedtuple("Model", "nh nl X C prior step claim")


def _m(nh, nl, X, claim, C=0, prior=False, step=True):
    return Model(nh, nl, X, C, prior, step, claim)


ONE_LAYER = [
    _m(200, 100, 784, "reference"),
    _m(37, 5, 53, "cut"),                 # x_dim mod 4 = 1: the last Philox group is cut at one word
    _m(199, 99, 783, "cut"),              # x_dim mod 4 = 3
    _m(201, 101, 785, "cut"),             # x_dim mod 4 = 1, one past the reference
    _m(128, 16, 384, "nopad"),            # Xinp == x_dim: no pad column to zero
    _m(224, 128, 832, "nopad"),
    _m(1, 1, 1, "pixel"),                 # a single pixel
]
INSPECT = [
    _m(64, 8, 1029, "trips", step=False),     # Xinp / 8 = 132 > 128 chunks: the kernel's grid-stride loop takes a second trip (33 mask words)
    _m(64, 8, 4096, "trips", step=False),     # iwae_create's widest: 512 chunks, four trips
]
TWO_LAYER = [_m((200, 100), (100, 50), 784, "reference"), _m((40, 30), (24, 12), 61, "cut")]
COND = [_m(200, 100, 784, "reference", C, p) for p in (False, True)] + \
       [_m(64, 20, 783, "onehot_in_group", C, p) for p in (False, True)] + \
       [_m(64, 20, 795, "onehot_crosses_32", C, p) for p in (False, True)]   # 795 .. 804 crosses 800, a 16- and a 32-feature tile boundary
STEP_MODELS = ONE_LAYER + TWO_LAYER + COND
ALL_MODELS = STEP_MODELS + INSPECT
WIDE, WIDE2, WIDE_C, WIDE_CP = ONE_LAYER[0], TWO_LAYER[0], COND[0], COND[1]
WALK_MODELS = [WIDE, WIDE2, WIDE_C, WIDE_CP]

# (start, B) on N = 300, and the boundary each sits on: "lane64" gather_binarize_kernel's 64-lane row block (blockIdx.x * 64 + lane),
# "pad128" Bp = round_up(B, 128), "end" the batch ends on the set's last image, "one" a batch of one image, "all" the whole set.
BATCHES = collections.OrderedDict([
    ((37, 150), ("ragged",)), ((0, 1), ("one",)), ((299, 1), ("one", "end")), ((0, 300), ("all", "end")),
    ((0, 64), ("lane64_full",)), ((1, 65), ("lane64_over",)), ((0, 128), ("pad128_full",)), ((5, 129), ("pad128_over",)),
    ((172, 128), ("pad128_full", "end")),
])
WALK = [(0, 128), (128, 128), (256, 44)]          # one epoch at batch 128: the ragged last batch is 300 mod 128 = 44 images
DEFAULT_WALK = [(20 * i, 20) for i in range(15)]   # main.py's default batch: fifteen steps cross the eight-step noise buffer twice
LABEL0_AT, LABELC_AT = (0, 1, 40, 180, 260), (2, 41, 181, 261, 299)      # positions of the order whose image has label 0 / C - 1

# The large cases: either side of block_fwd_shape_ok's R <= 4 096 rows (kernels.hip), both above the 2 048 data rows of dec_rows_step
LARGE = _m(64, 8, 100, "rows")
LARGE_N, LARGE_K = 4200, 1
LARGE_BATCHES = [(0, 4096), (3, 4097)]
SIDE_K = 20                                       # on WIDE: B = 150 (128) at k = 20 is 3 000 (2 560) data rows: the side streams are live

OBJECTIVES5 = ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14", "dreg")
OBJECTIVES_2L = ("vae_elbo", "iwae_elbo", "iwae_eq14")

# One draw cannot disagree with five independent redraws (group, word, key, epoch twice) in each of six (seed, epoch) pairs: 2^-30 at p = 1/2.
CONTROL_EXEMPT = {((1, 1, 1), (0, 1)), ((1, 1, 1), (299, 1))}


def round_up(v, m):
    return (max(1, v) + m - 1) // m * m


def dims(m):
    return (m.nh, m.nl, m.X)


def model_id(m):
    w = lambda v: "x".join(str(e) for e in v) if isinstance(v, tuple) else str(v)
    return "%s_%s_%d%s" % (w(m.nh), w(m.nl), m.X, "" if not m.C else ("_cprior" if m.prior else "_cond"))


def layers(m):
    return 2 if isinstance(m.nh, tuple) else 1


def xinp(m):
    """model.hip (iwae_create): the row width of the encoder's input, concat(x, onehot(y)) padded to 32 features."""
    return round_up(m.X + m.C, 32)


def chunks(m):
    """gather_binarize_kernel walks a row in chunks of 8 features; its grid covers min(32, ceil(nchunk / 4)) * 4 = at most 128 of them per trip."""
    return xinp(m) // 8


def enc_block_fused(m, B, allow=True):
    """StepPlan::enc_takes_f32 restated (step_bf16.hip plan_step, model.hip block_fwd_shape, kernels.hip block_fwd_shape_ok with R = B, KT0 =
    Xinp / 32, KT1 = Hp / 32, NT1 = Hp / 16, NT2 = 2 Dp / 16): block_fwd_kernel converts a host-fed step's float32 rows itself; where this is False
    prep_rows_kernel writes the bf16 rows first.  A resident step reads gather_binarize_kernel's bf16 rows either way."""
    nh = m.nh[0] if layers(m) == 2 else m.nh
    nl = m.nl[0] if layers(m) == 2 else m.nl
    Hp, Dp, KT0 = round_up(nh, 32), round_up(nl, 32), xinp(m) // 32
    KT1, NT1, NT2 = Hp // 32, Hp // 16, 2 * Dp // 16
    shape_ok = B <= 4096 and KT1 <= 8 and NT1 <= 16 and NT2 <= 16 and NT1 == 2 * KT1 and (KT0 + 2 * KT1) * 1024 <= 150 * 1024
    return allow and m.C == 0 and shape_ok


@functools.lru_cache(maxsize=None)
def gray(X, n=N):
    """uint8 grey levels [n, X]: random, columns 0 .. 5 at the SPECIAL levels (narrower than six pixels: the levels cycle over the images of
    column 0), and the LAST column at 128 where the width allows it (a cut last Philox group then holds a pixel whose bit is a fair coin)."""
    g = (np.random.default_rng(3 + X).random((n, X)) * 256).astype(np.uint8)
    if X >= 6:
        for c, level in enumerate(SPECIAL):
            g[:, c] = level
        if X > 6:
            g[:, X - 1] = 128
    else:
        g[:, 0] = np.array(SPECIAL, np.uint8)[np.arange(n) % 6]
    if X == PLANTED_X and n == N:      # (the pixels at which the threshold's rounding shows in a bit: planted() below)
        for seed in SEEDS:
            for epoch in EPOCHS:
                for i, f, level in planted(seed, epoch):
                    g[i, f] = level
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def orders(n=N):
    """Two visiting orders that agree at the labelled positions and nowhere else on purpose; no image sits at its own position in the first
    (a generator keyed by the position instead of the image then draws every row from another counter)."""
    rng = np.random.default_rng(11 + n)
    a = np.roll(np.arange(n), 1 + int(rng.integers(0, n - 2)))[rng.permutation(n)].astype(np.int32)
    while np.any(a == np.arange(n)):
        a = rng.permutation(n).astype(np.int32)
    fixed = np.array(sorted(LABEL0_AT + LABELC_AT))
    free = np.setdiff1d(np.arange(n), fixed)
    b = a.copy()
    b[free] = a[free][rng.permutation(free.size)]
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def order_of(epoch, n=N):
    """The order the table visits the set in at an epoch: the first order at epochs 0 and 2^32 - 1, the second at 7."""
    return orders(n)[1 if epoch == 7 else 0]


@functools.lru_cache(maxsize=None)
def labels():
    """One class id per image, uint8 [N]: random, label 0 and label C - 1 at the images the fixed positions of the orders hold."""
    y = np.random.default_rng(17).integers(0, C, N).astype(np.uint8)
    o = orders()[0]
    y[o[list(LABEL0_AT)]] = 0
    y[o[list(LABELC_AT)]] = C - 1
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def set_mask(X):
    """A 50 % mask of the set [N, X] uint8 (the inspection of the masked gather kernel's second loop trip at x_dim 1 029)."""
    m = (np.random.default_rng(41).random((N, X)) < 0.5).astype(np.uint8)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=64)
def binarized(X, seed, epoch, n=N):
    """The restatement on the whole set in identity order, float32 [n, X], computed once: rows(...) below indexes it (a pixel's bit depends on
    (seed, epoch, image, pixel) only -- test_dataset_host.py holds that and rows() against philox_np.device_binarize on the batch's ids)."""
    out = philox_np.device_binarize(seed, epoch, gray(X, n), np.arange(n))
    out.setflags(write=False)
    return out


def rows(X, seed, epoch, ids, n=N):
    """philox_np.device_binarize(seed, epoch, gray(X, n), ids)"""
    return np.ascontiguousarray(binarized(X, seed, epoch, n)[np.asarray(ids)])


def one_hot(ids):
    from iwae_amd import task05
    return task05.one_hot(labels()[np.asarray(ids)], C)


@functools.lru_cache(maxsize=None)
def params(m):
    """Flat float32 parameters of a model at the random initialisation (oracle/iwae_np.init_params, seed 5) and the tensor list."""
    mean = np.resize(O.synthetic_pixel_means(m.X), m.X)      # (the synthetic means come on a square grid: repeated where x_dim is past the square)
    P = O.init_params(layers(m), list(m.nh) if layers(m) == 2 else m.nh, list(m.nl) if layers(m) == 2 else m.nl, 5,
                      x_mean=mean, x_dim=m.X, cond_dim=m.C, cond_prior=m.prior)
    assert all(b.shape == (W.shape[1],) for W, b in P)
    flat = np.asarray(O.flatten_params(P), dtype=np.float32)
    flat.setflags(write=False)
    return flat, P


# ---------------------------------------------------------------- the restatement pixel by pixel, and its mutants
def threshold(g, rounding=True):
    """T(g) = floor(g 2^24 / 255 + 1/2) as the kernel computes it, in integers; rounding=False: the mutant floor(g 2^24 / 255)."""
    return (int(g) * (1 << 25) + 255) // 510 if rounding else (int(g) << 24) // 255


def mutant(name, X, seed, epoch, order, start, B, n=N):
    """gather_binarize_kernel's rows [B, X] with ONE thing wrong (the negative controls of test_dataset_host.py).  Vectorised like
    philox_np.device_binarize, whose counters it restates: (image, 'BINA', pixel >> 2, epoch), key (seed lo, seed hi), word pixel & 3."""
    ids = np.asarray(order[start:start + B], dtype=np.int64)
    g = gray(X, n)[ids].astype(np.uint64)
    nd4 = (X + 3) // 4
    key = np.arange(start, start + B, dtype=np.int64) if name == "position" else ids
    grp = np.arange(nd4, dtype=np.uint32) + np.uint32(1 if name == "group" else 0)
    if name == "epoch":
        epoch = EPOCHS[(EPOCHS.index(epoch) + 1) % len(EPOCHS)]          # an epoch-blind generator returns another epoch's rows
    hi = 0 if name == "seed_hi" else (seed >> 32) & 0xFFFFFFFF
    c0 = np.broadcast_to(key[:, None].astype(np.uint32), (B, nd4))
    r = philox_np.philox4x32_10(c0, np.full((B, nd4), 0x42494E41, np.uint32), np.broadcast_to(grp[None, :], (B, nd4)),
                                np.full((B, nd4), epoch, np.uint32), seed & 0xFFFFFFFF, hi)
    if name == "word":
        r = r[::-1]
    u = np.stack([w >> np.uint32(8) for w in r], axis=-1).reshape(B, nd4 * 4)[:, :X].astype(np.uint64)
    if name == "threshold":
        thr = (g << np.uint64(24)) // np.uint64(255)
    else:
        thr = (g * np.uint64(1 << 25) + np.uint64(255)) // np.uint64(510)
    return (u < thr).astype(np.float32)


BIT_MUTANTS = ("group", "word", "position", "epoch", "seed_hi")      # seed_hi: on SEEDS[1] only (the first seed's high word IS zero)


def encoder_row(x, y, width):
    """The encoder's input rows as gather_binarize_kernel writes them: [B, width], pixels, then onehot(y) at X .. X + C - 1, then zeros."""
    out = np.zeros((x.shape[0], width), np.float32)
    out[:, :x.shape[1]] = x
    if y is not None:
        out[:, x.shape[1]:x.shape[1] + y.shape[1]] = y
    return out


def encoder_row_shifted(x, lab, width):
    """... with the one-hot written at X + lab + 1 (the seventh negative control)."""
    out = np.zeros((x.shape[0], width + 1), np.float32)
    out[:, :x.shape[1]] = x
    out[np.arange(x.shape[0]), x.shape[1] + np.asarray(lab, dtype=np.int64) + 1] = 1.0
    return out[:, :width]


# ---------------------------------------------------------------- planted pixels: where the threshold's rounding shows in a bit
# A pixel's 24-bit draw u gives bit (u < T(g)).  The rounding moves T(g) by one for the grey levels whose g 2^24 / 255 has a fraction >= 1/2, so
# it shows in a bit only where u == floor(g 2^24 / 255) exactly: one draw in 2^24 per level.  planted(seed, epoch) searches the draws of the
# images x pixels of the 4 096-wide set for such a (image, pixel, level); the 4 096-wide set of that (seed, epoch) carries the level there
# (gray_planted), so the inspection test on the GPU holds the rounding at those pixels.  The search is the restatement's own arithmetic.
@functools.lru_cache(maxsize=None)
def _floor_levels():
    lv = [g for g in range(256) if threshold(g) != threshold(g, False)]
    return np.array([threshold(g, False) for g in lv], np.int64), np.array(lv, np.int64)


@functools.lru_cache(maxsize=None)
def planted(seed, epoch, X=PLANTED_X):
    """[(image, pixel, grey level)] of the X-wide set at which u == floor(g 2^24 / 255) and the rounding lifts T(g) above it: bit 1 with the
    rounding, 0 without.  Columns 0 .. 5 and the last keep their levels."""
    nd4 = X // 4
    c0 = np.broadcast_to(np.arange(N, dtype=np.uint32)[:, None], (N, nd4))
    r = philox_np.philox4x32_10(c0, np.full((N, nd4), 0x42494E41, np.uint32), np.broadcast_to(np.arange(nd4, dtype=np.uint32)[None, :], (N, nd4)),
                                np.full((N, nd4), epoch, np.uint32), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u = np.stack([w >> np.uint32(8) for w in r], axis=-1).reshape(N, X).astype(np.int64)
    floors, levels = _floor_levels()
    hit = np.isin(u, floors)
    hit[:, :6] = False
    hit[:, X - 1] = False
    out = []
    for i, f in zip(*np.nonzero(hit)):
        out.append((int(i), int(f), int(levels[np.searchsorted(floors, u[i, f])])))
    return tuple(out)
