"""CPU side of the resident per-image masks: the host restatement of the device mask generator against the committed
Philox, the admissibility of tests/_masked_dataset_cases.py from NumPy alone, the realised hidden fraction of the generator as a condition,
and tasks/miwae.py's parser.  The GPU module test_gpu_masked_dataset.py runs the table."""
import math
import os
import sys

import numpy as np
import pytest

from oracle import philox_np
from iwae_amd import utils
import _masked_dataset_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", DC.MCAR_SEEDS)
@pytest.mark.parametrize("X", [d[2] for d in DC.DIMS])
def test_device_mcar_mask_is_the_committed_philox_on_the_documented_counters(X, seed):
    """Pixel f of image i is hidden iff (philox4x32_10((i, 'MASK', f >> 2, 0), (seed lo, seed hi))[f & 3] >> 8) < floor(rate 2^24 + 0.5)."""
    n = 9
    nq = (X + 3) // 4
    i = np.broadcast_to(np.arange(n, dtype=np.uint32)[:, None], (n, nq))
    q = np.broadcast_to(np.arange(nq, dtype=np.uint32)[None, :], (n, nq))
    r = philox_np.philox4x32_10(i, np.full((n, nq), 0x4D41534B, np.uint32), q, np.zeros((n, nq), np.uint32), seed & 0xFFFFFFFF, seed >> 32)
    u = np.stack([w >> np.uint32(8) for w in r], axis=-1).reshape(n, 4 * nq)[:, :X].astype(np.int64)
    for rate in DC.MCAR_RATES:
        thr = int(math.floor(rate * 2.0 ** 24 + 0.5))
        assert utils.mcar_threshold(rate) == thr
        got = utils.device_mcar_mask(n, X, rate, seed)
        assert got.dtype == np.uint8 and got.shape == (n, X)
        np.testing.assert_array_equal(got, (u >= thr).astype(np.uint8))
    # the first n rows of a larger set are the same rows: the counter holds the image, not the set's size
    np.testing.assert_array_equal(utils.device_mcar_mask(n + 4, X, 0.5, seed)[:n], utils.device_mcar_mask(n, X, 0.5, seed))
    assert not np.array_equal(utils.device_mcar_mask(n, X, 0.5, seed), utils.device_mcar_mask(n, X, 0.5, seed + 1))


@pytest.mark.parametrize("rate", [-0.1, 1.5, float("nan")])
def test_rates_outside_the_unit_interval_are_refused(rate):
    with pytest.raises(ValueError):
        utils.device_mcar_mask(4, 8, rate, 0)


@pytest.mark.parametrize("seed", DC.MCAR_SEEDS)
def test_realised_hidden_fraction_of_the_generator(seed):
    """Over 300 x 784 draws the hidden fraction lies within 5 sqrt(p (1 - p) / (N X)) of thr / 2^24 (0.0047 at 0.3, 0.0052 at 0.5) for the
    two seeds the GPU module uses; rates 0 and 1 are exact."""
    X = 784
    for rate, bound in ((0.3, 0.0047), (0.5, 0.0052)):
        p = utils.mcar_threshold(rate) / 2.0 ** 24
        tol = 5.0 * math.sqrt(p * (1.0 - p) / (DC.N * X))
        assert abs(tol - bound) < 5e-5
        hidden = 1.0 - float(utils.device_mcar_mask(DC.N, X, rate, seed).mean())
        print("rate %.1f seed %d: hidden %.5f, |d| %.5f (< %.5f)" % (rate, seed, hidden, abs(hidden - p), tol))
        assert abs(hidden - p) < tol
    assert utils.device_mcar_mask(DC.N, X, 0.0, seed).min() == 1
    assert utils.device_mcar_mask(DC.N, X, 1.0, seed).max() == 0


@pytest.mark.parametrize("shape", DC.SHAPES, ids=lambda s: "%d_%d_%d" % s.dims)
def test_shapes_have_the_word_count_and_last_word_fill_they_claim(shape):
    X = shape.dims[2]
    assert DC.mask_words(X) == shape.words == -(-X // 32)
    assert X - 32 * (shape.words - 1) == shape.last_fill and 1 <= shape.last_fill <= 32
    # the 8 pixels of a P-layout chunk c (features 32 t + 16 h + 4 q + i, t = c >> 2, q = c & 3) lie in word t
    for c in range(4 * shape.words):
        t, q = c >> 2, c & 3
        assert {(32 * t + 16 * h + 4 * q + i) >> 5 for h in range(2) for i in range(4)} == {t}
    m = DC.half_mask(X)
    bits = DC.pack_bits(m)
    assert bits.shape == (DC.N, shape.words) and bits.dtype == np.uint32
    np.testing.assert_array_equal(DC.unpack_bits(bits, X), m)
    if shape.last_fill < 32:
        assert int(bits[:, -1].max()) < (1 << shape.last_fill)      # bits past the last pixel stay 0


def test_shapes_cover_what_the_issue_asks_for():
    assert DC.DIMS == [(200, 100, 784), (37, 5, 53), (64, 8, 100), (128, 16, 384)]
    assert [(s.words, s.last_fill) for s in DC.SHAPES] == [(25, 16), (2, 21), (4, 4), (12, 32)]
    assert DC.N == 300 and DC.K == 5 and DC.BATCHES == [(37, 150), (0, 1), (299, 1), (172, 128)]
    assert all(0 <= s and s + b <= DC.N for s, b in DC.BATCHES) and DC.BATCHES[-1][0] + DC.BATCHES[-1][1] == DC.N
    assert any(b % 64 for _, b in DC.BATCHES) and any(d[2] % 4 for d in DC.DIMS) and any(d[2] % 32 == 0 for d in DC.DIMS)
    # the float32 fused route takes three of the shapes; 37 / 5 / 53 (x_dim no multiple of 4) stays on the general route
    assert [DC.fast_route_accepts(d) for d in DC.DIMS] == [True, False, True, True]
    # every shape pads to a hidden width the bf16 masked step takes; the refused widths do not
    import _masked_bf16_cases as BC
    assert all(BC.kt_of(d[0]) in BC.S_MODE_KT for d in DC.DIMS)
    assert all(BC.kt_of(d[0]) not in BC.S_MODE_KT for d in DC.REFUSED_BF16)


@pytest.mark.parametrize("X", [d[2] for d in DC.DIMS])
def test_masks_hold_what_they_claim_in_every_batch_and_epoch(X):
    g = DC.gray(X)
    c = max(1, X // 10)
    assert g.shape == (DC.N, X) and g[:, :c].max() == 0 and g[:, c:2 * c].min() == 255 and 0 < g[:, 2 * c:].mean() < 255
    a, b = DC.orders()
    assert sorted(a) == sorted(b) == list(range(DC.N)) and np.count_nonzero(a != b) > DC.N // 2
    m = DC.half_mask(X)
    assert 0.45 < m.mean() < 0.55
    for order in (a, b):
        for (start, B) in DC.BATCHES:
            rows = m[order[start:start + B]]
            claim = DC.CLAIMS[(start, B)]
            per_image = rows.sum(axis=1)
            if "empty" in claim:
                assert np.any(per_image == 0)
            if "full" in claim:
                assert np.any(per_image == X - 1)      # everything but the dead column
            assert "dead" in claim and not rows[:, DC.DEAD_COLUMN].any()
            if B > 1:
                assert np.count_nonzero(rows.sum(axis=0) == 0) < X // 2 and set(claim) == {"empty", "full", "dead"}
    assert DC.ones_mask(X).min() == 1


def test_miwae_parser_with_and_without_resident():
    import main
    sys.path.insert(0, os.path.join(ROOT, "tasks"))
    try:
        import miwae
    finally:
        sys.path.pop(0)
    a = miwae.make_parser().parse_args([])
    assert not hasattr(a, "resident") and not miwae.resident_of(a)
    assert vars(a) == dict(vars(main.parser.parse_args([])), images=10000, test_images=1000, steps=2000, rate=0.5, draws=50, mask_seed=0, lr=1e-3)
    r = miwae.make_parser().parse_args(["--resident"])
    assert r.resident is True and miwae.resident_of(r)
    assert {k: v for k, v in vars(r).items() if k != "resident"} == vars(a)
    with pytest.raises(NotImplementedError):
        miwae.main(["--resident", "--stochastic_layers", "2"])
