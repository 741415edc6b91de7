"""CPU side of the resident-dataset input path: the binarisation's definition in exact arithmetic, the restatement
oracle/philox_np.device_binarize every GPU check of that path leans on (Bernoulli(g / 255) per grey level, a function of (seed, epoch, image,
pixel) alone, pinned by a per-pixel scalar loop), the negative controls that show what the GPU equalities can see, and the admissibility of
tests/_dataset_cases.py from NumPy alone.  The GPU module test_gpu_dataset.py runs the table."""
import fractions
import math

import numpy as np
import pytest

from oracle import philox_np
import _dataset_cases as DC

SEED_IDS = ["seed123", "seed_hi"]


# ---------------------------------------------------------------- the definition
def test_threshold_is_the_rounded_rational_for_every_grey_level():
    """(g 2^25 + 255) // 510 == floor(g 2^24 / 255 + 1/2) in exact rational arithmetic for all 256 levels; monotone, 0 at 0 and 2^24 at 255."""
    t = [DC.threshold(g) for g in range(256)]
    for g in range(256):
        assert t[g] == (g * (1 << 25) + 255) // 510
        assert t[g] == math.floor(fractions.Fraction(g * (1 << 24), 255) + fractions.Fraction(1, 2))
        assert abs(fractions.Fraction(t[g], 1 << 24) - fractions.Fraction(g, 255)) <= fractions.Fraction(1, 1 << 25)
    assert t[0] == 0 and t[255] == 1 << 24 and all(a < b for a, b in zip(t, t[1:]))
    # the mutant without the rounding differs at the levels whose fraction is at least a half, by exactly one
    d = [t[g] - DC.threshold(g, False) for g in range(256)]
    assert set(d) == {0, 1} and d[0] == d[255] == 0 and d[128] == 1 and 100 < sum(d) < 156


@pytest.mark.parametrize("seed", DC.SEEDS, ids=SEED_IDS)
def test_device_binarize_is_bernoulli_of_the_grey_level(seed):
    """Per grey level 20 000 draws (2 000 images x 10 epochs, 2^32 - 1 among them): |frequency - g / 255| <= 5 sqrt(p (1 - p) / n), exactly 0
    at g = 0 and exactly 1 at g = 255."""
    n_img, epochs = 2000, (0, 1, 2, 3, 7, 100, 65536, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1)
    gray = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :], (n_img, 256))
    ones = np.zeros(256)
    for e in epochs:
        ones += philox_np.device_binarize(seed, e, gray, np.arange(n_img)).sum(axis=0, dtype=np.float64)
    n = n_img * len(epochs)
    assert n == 20000
    p = np.arange(256) / 255.0
    sigma = np.sqrt(p * (1.0 - p) / n)
    z = np.abs(ones / n - p) / np.where(sigma > 0, sigma, 1.0)
    print("seed %d: worst level %d at %.2f standard deviations" % (seed, int(np.argmax(z)), float(z.max())))
    assert ones[0] == 0 and ones[255] == n
    assert np.all(np.abs(ones / n - p) <= 5.0 * sigma)


@pytest.mark.parametrize("seed", DC.SEEDS, ids=SEED_IDS)
def test_a_pixels_bit_depends_on_seed_epoch_image_and_pixel_only(seed):
    X = 53
    g = DC.gray(X)
    full = philox_np.device_binarize(seed, 7, g, np.arange(DC.N))
    rng = np.random.default_rng(2)
    sub = rng.permutation(DC.N)[:77]                                   # a subset in another order: the same rows
    np.testing.assert_array_equal(philox_np.device_binarize(seed, 7, g, sub), full[sub])
    rep = np.array([5, 5, 299, 5, 0, 299])                             # repeated ids: equal rows
    got = philox_np.device_binarize(seed, 7, g, rep)
    np.testing.assert_array_equal(got, full[rep])
    np.testing.assert_array_equal(got[0], got[1])
    # rows() of the table is device_binarize on the batch's ids, at every batch and epoch
    for epoch in DC.EPOCHS:
        order = DC.order_of(epoch)
        for (s, B) in DC.BATCHES:
            np.testing.assert_array_equal(DC.rows(X, seed, epoch, order[s:s + B]), philox_np.device_binarize(seed, epoch, g, order[s:s + B]))
    # two epochs, and two images, agree on about half the pixels of a grey-128 column: |agreement - 1/2| <= 5 sigma (T(128) / 2^24 = 0.50196:
    # the agreement of two independent draws is 0.500008)
    col = np.full((4000, 4), 128, np.uint8)
    a, b = (philox_np.device_binarize(seed, e, col, np.arange(4000)) for e in (0, 2 ** 32 - 1))
    n = a.size
    tol = 5.0 * math.sqrt(0.25 / n)
    assert abs(float((a == b).mean()) - 0.5) <= tol
    assert abs(float((a[:2000] == a[2000:]).mean()) - 0.5) <= 5.0 * math.sqrt(0.25 / (n // 2))
    assert abs(float((a[:, 0] == a[:, 1]).mean()) - 0.5) <= 5.0 * math.sqrt(0.25 / 4000)      # ... and two pixels of one group


def _scalar_philox(c, k):
    """Philox4x32-10 on Python integers (Salmon et al., SC'11), one counter at a time."""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def test_scalar_restatement_pins_the_vectorised_one():
    """A per-pixel Python loop (no broadcasting) over (image, pixel, epoch) triples, the pixels of cut last groups among them."""
    assert _scalar_philox((0, 0, 0, 0), (0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]      # Random123's known answer
    for X in (53, 783, 1):
        g = DC.gray(X)
        pixels = sorted({0, X - 1, max(0, X - 2), X // 2, min(X - 1, 5), 4 * ((X - 1) // 4)})
        for seed in DC.SEEDS:
            for epoch in DC.EPOCHS:
                vec = philox_np.device_binarize(seed, epoch, g, np.arange(DC.N))
                for img in (0, 1, 150, 299):
                    for f in pixels:
                        r = _scalar_philox((img, 0x42494E41, f >> 2, epoch), (seed & 0xFFFFFFFF, seed >> 32))
                        bit = 1.0 if (r[f & 3] >> 8) < DC.threshold(int(g[img, f])) else 0.0
                        assert vec[img, f] == bit, (X, seed, epoch, img, f)


# ---------------------------------------------------------------- negative controls
@pytest.mark.parametrize("m", [m for m in DC.ALL_MODELS if not (m.C and m.prior)], ids=DC.model_id)      # (the prior changes no input row)
def test_every_mutant_of_the_restatement_shows_in_every_case(m):
    """Each mutant (tests/_dataset_cases.py mutant) differs from the restatement in at least one bit of every (batch, seed, epoch) of the
    shape: what the GPU module's array_equal can see.  seed_hi: on the second seed only.  CONTROL_EXEMPT: the two single draws."""
    X = m.X
    for (s, B) in DC.BATCHES:
        exempt = (DC.dims(m), (s, B)) in DC.CONTROL_EXEMPT
        for si, seed in enumerate(DC.SEEDS):
            for epoch in DC.EPOCHS:
                order = DC.order_of(epoch)
                ref = DC.rows(X, seed, epoch, order[s:s + B])
                for name in DC.BIT_MUTANTS:
                    if name == "seed_hi" and si == 0:
                        np.testing.assert_array_equal(DC.mutant(name, X, seed, epoch, order, s, B), ref)
                        continue
                    got = DC.mutant(name, X, seed, epoch, order, s, B)
                    if not exempt:
                        assert np.any(got != ref), (name, DC.model_id(m), (s, B), seed, epoch)
                assert B == 1 or X < 6 or (ref[:, 0].max() == 0 and ref[:, 1].min() == 1)
    if X == 1:      # the exempt draws' shape: every mutant shows on the whole set, and a mutant run unmutated is the restatement
        for seed in DC.SEEDS:
            np.testing.assert_array_equal(DC.mutant("none", X, seed, 7, DC.order_of(7), 0, DC.N), DC.rows(X, seed, 7, DC.order_of(7)))
    assert DC.CONTROL_EXEMPT == {((1, 1, 1), (0, 1)), ((1, 1, 1), (299, 1))}


@pytest.mark.parametrize("m", [m for m in DC.COND if not m.prior], ids=DC.model_id)
def test_a_shifted_one_hot_shows_in_the_encoders_input_row(m):
    """The one-hot written at X + lab + 1 moves a 1 of every row of the encoder's input (the label C - 1 falls off the live features and
    into a pad column, or off the row)."""
    for epoch in DC.EPOCHS:
        order = DC.order_of(epoch)
        for (s, B) in DC.BATCHES:
            ids = order[s:s + B]
            x = DC.rows(m.X, DC.SEEDS[0], epoch, ids)
            ref = DC.encoder_row(x, DC.one_hot(ids), DC.xinp(m))
            bad = DC.encoder_row_shifted(x, DC.labels()[ids], DC.xinp(m))
            assert np.all(np.any(ref != bad, axis=1))
            assert np.all(ref[:, m.X:m.X + m.C].sum(axis=1) == 1) and np.all(ref[:, m.X + m.C:] == 0)


def test_the_thresholds_rounding_shows_only_at_the_planted_pixels():
    """The mutant floor(g 2^24 / 255) gives the restatement's bits wherever no draw equals a floor exactly -- one draw in 2^24 per level, so no
    table of a few hundred images can show it in every batch.  What holds the rounding: the exact-arithmetic test above, and the pixels
    _dataset_cases.planted() found in the 4 096-wide set, where the draw IS the floor: bit 1 with the rounding, 0 without.  Every
    (seed, epoch) of the table has at least one, and the whole-set batch of that shape shows the mutant at exactly those pixels."""
    X = DC.PLANTED_X
    g = DC.gray(X)
    for seed in DC.SEEDS:
        for epoch in DC.EPOCHS:
            pl = [(i, f, lv) for i, f, lv in DC.planted(seed, epoch) if g[i, f] == lv]
            print("seed %d epoch %d: %d planted pixels" % (seed, epoch, len(pl)))
            assert len(pl) >= 1
            ident = np.arange(DC.N, dtype=np.int32)
            ref = DC.rows(X, seed, epoch, ident)
            mut = DC.mutant("threshold", X, seed, epoch, ident, 0, DC.N)
            where = set(zip(*[a.tolist() for a in np.nonzero(ref != mut)]))
            assert where >= {(i, f) for i, f, _ in pl}
            for i, f, lv in pl:
                assert ref[i, f] == 1.0 and mut[i, f] == 0.0 and DC.threshold(lv) == DC.threshold(lv, False) + 1
    # at the reference width the mutant is invisible: the figure the docstring states
    ident = np.arange(DC.N, dtype=np.int32)
    assert 784 * DC.N * 128 / 2.0 ** 24 < 2.0
    np.testing.assert_array_equal(DC.mutant("none", 784, 123, 0, ident, 0, DC.N), DC.rows(784, 123, 0, ident))


# ---------------------------------------------------------------- admissibility of the table
@pytest.mark.parametrize("m", DC.ALL_MODELS, ids=DC.model_id)
def test_shapes_have_the_property_they_claim(m):
    X, Xinp, nch = m.X, DC.xinp(m), DC.chunks(m)
    assert Xinp % 32 == 0 and Xinp >= X + m.C and nch * 8 == Xinp
    if m.claim == "cut":
        assert X % 4 in (1, 3) and Xinp > X
    if m.claim == "nopad":
        assert Xinp == X and X % 32 == 0
    if m.claim == "pixel":
        assert X == 1 and Xinp == 32
    if m.claim == "trips":
        assert nch > 128 and not m.step and X > 1023      # min(32, ceil(nch / 4)) * 4 = 128 chunks per trip of the grid-stride loop
    else:
        assert nch <= 128 and m.step
    if m.claim == "onehot_in_group":
        assert X % 4 != 0 and (X // 16 != (X + m.C - 1) // 16)
    if m.claim == "onehot_crosses_32":
        assert X // 32 != (X + m.C - 1) // 32 and X // 16 != (X + m.C - 1) // 16
    if m.C:
        nl = m.nl
        assert nl + m.C <= DC.round_up(nl, 32) and DC.layers(m) == 1      # iwae_create admits it
    assert 1 <= X <= 4096


def test_the_table_is_what_the_issue_lists():
    assert [DC.dims(m) for m in DC.ONE_LAYER] == [(200, 100, 784), (37, 5, 53), (199, 99, 783), (201, 101, 785), (128, 16, 384), (224, 128, 832), (1, 1, 1)]
    assert [m.X % 4 for m in DC.ONE_LAYER[1:4]] == [1, 3, 1]
    assert [DC.dims(m) for m in DC.INSPECT] == [(64, 8, 1029), (64, 8, 4096)]
    assert [DC.dims(m) for m in DC.TWO_LAYER] == [((200, 100), (100, 50), 784), ((40, 30), (24, 12), 61)]
    assert [(DC.dims(m), m.C, m.prior) for m in DC.COND] == [(d, 10, p) for d in ((200, 100, 784), (64, 20, 783), (64, 20, 795)) for p in (False, True)]
    assert list(DC.BATCHES) == [(37, 150), (0, 1), (299, 1), (0, 300), (0, 64), (1, 65), (0, 128), (5, 129), (172, 128)]
    assert DC.N == 300 and DC.K == 5 and DC.SEEDS == (123, (1 << 40) + 77) and DC.EPOCHS == (0, 7, 2 ** 32 - 1)
    assert DC.SEEDS[0] >> 32 == 0 and DC.SEEDS[1] >> 32 != 0
    assert DC.LARGE_N == 4200 and DC.dims(DC.LARGE) == (64, 8, 100) and DC.LARGE_K == 1 and DC.LARGE_BATCHES == [(0, 4096), (3, 4097)]
    assert max(B * DC.LARGE_K for _, B in DC.LARGE_BATCHES) <= 4100 and 150 * DC.SIDE_K <= 4100


def test_batches_sit_on_the_boundaries_they_claim():
    for (s, B), claim in DC.BATCHES.items():
        assert 0 <= s and B >= 1 and s + B <= DC.N
        assert ("end" in claim) == (s + B == DC.N)
        assert ("one" in claim) == (B == 1)
        if "lane64_full" in claim:
            assert B == 64
        if "lane64_over" in claim:
            assert B == 65 and s % 64 != 0
        if "pad128_full" in claim:
            assert B == 128 and DC.round_up(B, 128) == B
        if "pad128_over" in claim:
            assert B == 129 and DC.round_up(B, 128) == 256
        if "ragged" in claim:
            assert B % 64 != 0 and B % 128 != 0 and B > 128
    # the epoch walk: three batches tile the set, the ragged last one non-empty and smaller; the default batch's walk crosses 8 and 16 steps
    assert DC.WALK[0][1] == DC.WALK[1][1] == 128 and DC.WALK[2] == (256, DC.N % 128) and 0 < DC.WALK[2][1] < 128
    assert [s for s, _ in DC.WALK] == [0, 128, 256] and sum(B for _, B in DC.WALK) == DC.N
    assert len(DC.DEFAULT_WALK) == 15 and DC.DEFAULT_WALK[-1] == (280, 20) and 20 * DC.K <= 2048
    assert 128 * DC.SIDE_K > 2048 and 150 * DC.SIDE_K > 2048 and 44 * DC.SIDE_K <= 2048      # side streams on, off at the shrink, on again


def test_large_cases_fall_on_either_side_of_the_fused_encoders_row_limit():
    """enc_block_fused restates StepPlan::enc_takes_f32: (0, 4096) is the last batch whose host-fed twin lets block_fwd_kernel convert the
    float32 rows, (3, 4097) the first that goes through prep_rows_kernel; no_block_fused switches the conversion off at any size."""
    (s0, B0), (s1, B1) = DC.LARGE_BATCHES
    assert DC.enc_block_fused(DC.LARGE, B0) and not DC.enc_block_fused(DC.LARGE, B1)
    assert B0 * DC.LARGE_K > 2048 and s0 + B0 <= DC.LARGE_N and s1 + B1 <= DC.LARGE_N and s1 % 64 != 0
    assert DC.enc_block_fused(DC.WIDE, 150) and not DC.enc_block_fused(DC.WIDE, 150, allow=False)
    assert all(DC.enc_block_fused(m, B) for m in DC.ONE_LAYER + DC.TWO_LAYER for _, B in DC.BATCHES)
    assert not any(DC.enc_block_fused(m, 150) for m in DC.COND)             # conditional models: prep_rows_kernel concatenates
    g = DC.gray(DC.LARGE.X, DC.LARGE_N)
    o = DC.orders(DC.LARGE_N)[0]
    assert g.shape == (4200, 100) and sorted(o) == list(range(4200))


@pytest.mark.parametrize("X", sorted({m.X for m in DC.ALL_MODELS}))
def test_every_batch_holds_every_special_grey_level(X):
    g = DC.gray(X)
    assert g.shape == (DC.N, X) and g.dtype == np.uint8
    if X >= 6:
        for c, level in enumerate(DC.SPECIAL):
            assert np.all(g[:, c] == level)          # a column of the set is a column of every batch
        assert len(np.unique(g[:, 6:])) > 200 or X < 60
    else:
        assert set(np.unique(g[:, 0])) == set(DC.SPECIAL)      # (1, 1, 1): the whole set holds each level
        for epoch in DC.EPOCHS:
            for (s, B) in DC.BATCHES:
                if B >= 64:
                    assert set(np.unique(g[DC.order_of(epoch)[s:s + B], 0])) == set(DC.SPECIAL)
    assert sorted(DC.SPECIAL) == [0, 1, 127, 128, 254, 255]


def test_orders_and_labels_hold_what_they_claim_in_every_batch_and_epoch():
    a, b = DC.orders()
    assert sorted(a) == sorted(b) == list(range(DC.N)) and np.count_nonzero(a != b) > DC.N // 2
    assert not np.any(a == np.arange(DC.N))
    y = DC.labels()
    assert y.dtype == np.uint8 and y.max() == DC.C - 1 and y.min() == 0
    for epoch in DC.EPOCHS:
        order = DC.order_of(epoch)
        for (s, B) in list(DC.BATCHES) + DC.WALK:
            got = set(y[order[s:s + B]].tolist())
            if B == 1:
                assert got == ({0} if s == 0 else {DC.C - 1})
            else:
                assert {0, DC.C - 1} <= got, (epoch, s, B)
    oh = DC.one_hot(a[:5])
    assert oh.shape == (5, DC.C) and np.all(oh.sum(axis=1) == 1) and np.all(np.argmax(oh, axis=1) == y[a[:5]])
