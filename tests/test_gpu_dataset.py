"""The resident-dataset input path WITHOUT masks (iwae_dataset_upload / _begin_epoch / _get_batch / _get_labels and the unmasked
iwae_train_step_dataset; include/iwae_amd.h) on the case table of tests/_dataset_cases.py, whose admissibility
tests/test_dataset_host.py shows on the CPU.  (test_gpu_masked_dataset.py is the masked call's module.)

Everything compared here is integer or bitwise.  The inspection calls ARE the NumPy restatement (oracle/philox_np.device_binarize), and a
resident step IS the host-fed step on the restated rows -- the host-fed twin never sees a row the device produced, so a defect both device
paths share cannot hide -- from the same parameters, Adam state and noise step: scalars, gradient, parameters, Adam moments and the next
step's draws (iwae_debug_eps, the witness of the noise step) are compared with array_equal.  The only tolerances are the four anchors of
section 4, imported from the parity modules that hold the host-fed step of each family to the float64 oracle.

Sections: 1 inspection, 2 one step, 3 sequences, 4 oracle anchors, 5 the data-parallel handle at world size 1, 6 refusals, 7 the shim."""
import numpy as np
import pytest

from oracle import iwae_np as O
from oracle import philox_np
import _dataset_cases as DC
from _parity_common import EMU_GRAD_REL, EMU_SCALAR_ATOL, F32_DEVNOISE_GRAD_REL, F32_DEVNOISE_SCALAR_ATOL, _grad_rel_errors

pytestmark = pytest.mark.gpu

SEED, SEED_HI = DC.SEEDS
EPOCH = 7                     # the epoch of the step tests (the second order)
PRECISIONS = ("bf16", "fp32")
_handles = {}


def _new(m, precision="bf16", seed=SEED, options=()):
    from iwae_amd.native import NativeModel
    two = DC.layers(m) == 2
    return NativeModel(2 if two else 1, list(m.nh) if two else m.nh, list(m.nl) if two else m.nl, x_dim=m.X, seed=seed, cond_dim=m.C,
                       cond_prior=m.prior, precision=precision, options=dict(options))


def _model(m, precision="bf16", seed=SEED, options=(), tag=0):
    """The module's handles: one per (model, precision, seed, options, tag); every test resets what it reads."""
    key = (m, precision, seed, options, tag)
    if key not in _handles:
        _handles[key] = _new(m, precision, seed, options)
    return _handles[key]


def _upload(h, m, n=DC.N):
    h.dataset_upload(DC.gray(m.X, n))
    if m.C:
        h.dataset_set_labels(DC.labels())


def _reset(h, m, step=3):
    h.set_params(DC.params(m)[0])
    h.set_adam_state(np.zeros(h.n_params, np.float32), np.zeros(h.n_params, np.float32), 0)
    h.set_step(step, 0)


def _state(h, B=3, k=2):
    """Parameters, Adam m, v, t, the gradient buffer and the draws of the NEXT step (every layer's): all a later step depends on."""
    mo, ve, t = h.get_adam_state()
    return {"params": h.get_params().copy(), "m": mo, "v": ve, "t": t, "grads": h.get_grads().copy(),
            "eps": [h.debug_eps(B, k, l) for l in range(h.n_layers)]}


def _same_state(a, b, grads=True):
    assert a["t"] == b["t"]
    for key in ("params", "m", "v") + (("grads",) if grads else ()):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    for u, v in zip(a["eps"], b["eps"]):
        np.testing.assert_array_equal(u, v, err_msg="the next step's draws")


def _same_scalars(ra, rb):
    assert ra.keys() == rb.keys()
    for key in ra:
        assert ra[key] == rb[key] or (np.isnan(ra[key]) and np.isnan(rb[key])), (key, ra[key], rb[key])


def _host_step(h, m, seed, epoch, ids, k, beta=1.0, lr=1e-3, objective="iwae_elbo", n=DC.N):
    """The host-fed twin's step: the RESTATED rows of the images `ids` (never iwae_dataset_get_batch's) and, conditional models, their
    one-hot labels through iwae_set_condition."""
    if m.C:
        h.set_condition(DC.one_hot(ids))
    return h.train_step(DC.rows(m.X, seed, epoch, ids, n), k, beta, lr, objective)


# ---------------------------------------------------------------- 1. the inspection calls are the restatement
@pytest.mark.parametrize("seed", DC.SEEDS, ids=["seed123", "seed_hi"])
@pytest.mark.parametrize("m", [m for m in DC.ALL_MODELS if not (m.C and m.prior)], ids=DC.model_id)
def test_get_batch_is_the_restatement_bit_for_bit(gpu, m, seed):
    X = m.X
    h = _model(m, "bf16", seed)
    _upload(h, m)
    for epoch in DC.EPOCHS:
        order = DC.order_of(epoch)
        h.dataset_begin_epoch(epoch, order)
        for (s, B) in DC.BATCHES:
            got = h.dataset_get_batch(s, B)
            assert got.dtype == np.float32 and got.shape == (B, X)
            ids = order[s:s + B]
            np.testing.assert_array_equal(got, philox_np.device_binarize(seed, epoch, DC.gray(X), ids) if B <= 65 else DC.rows(X, seed, epoch, ids),
                                          err_msg="epoch %d (%d, %d)" % (epoch, s, B))
            if X >= 6:
                assert got[:, 0].max() == 0.0 and got[:, 1].min() == 1.0      # grey 0: never; grey 255: always
        if X == DC.PLANTED_X:      # the draws that equal floor(g 2^24 / 255): 1 with the threshold's rounding, 0 without
            whole = h.dataset_get_batch(0, DC.N)
            inv = np.argsort(order)
            pl = [(i, f) for i, f, lv in DC.planted(seed, epoch) if DC.gray(X)[i, f] == lv]
            assert pl and all(whole[inv[i], f] == 1.0 for i, f in pl)
    if m.C:
        for epoch in DC.EPOCHS:
            order = DC.order_of(epoch)
            h.dataset_begin_epoch(epoch, order)
            for (s, B) in DC.BATCHES:
                y = h.dataset_get_labels(s, B)
                np.testing.assert_array_equal(y, DC.one_hot(order[s:s + B]))
                assert (B == 1) or (y[:, 0].max() == 1.0 and y[:, DC.C - 1].max() == 1.0)
    if X == 1029:      # 33 mask words: the masked gather kernel's second loop trip
        mask = DC.set_mask(X)
        h.dataset_set_mask(mask)
        try:
            for epoch in DC.EPOCHS[:2]:
                order = DC.order_of(epoch)
                h.dataset_begin_epoch(epoch, order)
                for (s, B) in DC.BATCHES:
                    np.testing.assert_array_equal(h.dataset_get_mask(s, B), mask[order[s:s + B]])
                    np.testing.assert_array_equal(h.dataset_get_batch(s, B), DC.rows(X, seed, epoch, order[s:s + B]))
        finally:
            h.dataset_set_mask(None)


@pytest.mark.parametrize("m", [DC.WIDE, DC.ONE_LAYER[1], DC.INSPECT[0]], ids=DC.model_id)
def test_orders_with_repeats_and_epochs_that_keep_the_order(gpu, m):
    X = m.X
    h = _model(m, "bf16")
    _upload(h, m)
    h.dataset_begin_epoch(7, np.zeros(DC.N, np.int32))                   # repeats are allowed: only the range is checked
    got = h.dataset_get_batch(5, 129)
    np.testing.assert_array_equal(got, DC.rows(X, SEED, 7, np.zeros(129, np.int64)))
    assert np.all(got == got[0])
    order = DC.order_of(7)
    h.dataset_begin_epoch(7, order)
    a = h.dataset_get_batch(37, 150)
    h.dataset_begin_epoch(2 ** 32 - 1, None)                              # NULL keeps the order and changes the bits
    b = h.dataset_get_batch(37, 150)
    np.testing.assert_array_equal(a, DC.rows(X, SEED, 7, order[37:187]))
    np.testing.assert_array_equal(b, DC.rows(X, SEED, 2 ** 32 - 1, order[37:187]))
    assert np.any(a != b)


@pytest.mark.parametrize("m", [DC.WIDE, DC.COND[2]], ids=DC.model_id)
def test_a_second_upload_starts_over(gpu, m):
    """Another n: identity order, epoch 0, labels and masks dropped -- first a smaller set, then a larger one."""
    X = m.X
    h = _new(m, "bf16")
    try:
        _reset(h, m)
        _upload(h, m)
        if not m.C:
            h.dataset_set_mask(DC.set_mask(X))
        h.dataset_begin_epoch(7, DC.order_of(7))
        h.train_step_dataset(37, 150, DC.K)
        for n in (120, 500):
            g = DC.gray(X, n)
            h.dataset_upload(g)
            ident = np.arange(n)
            for (s, B) in ((0, n), (n - 1, 1), (7, 65)):
                np.testing.assert_array_equal(h.dataset_get_batch(s, B), philox_np.device_binarize(SEED, 0, g, ident[s:s + B]))
            with pytest.raises(ValueError):
                h.dataset_get_batch(n - 64, 65)
            with pytest.raises(ValueError):
                h.dataset_begin_epoch(1, DC.order_of(7))                  # the old set's order has the wrong length
            with pytest.raises(RuntimeError):
                h.dataset_get_mask(0, 1)                                  # no masks
            if m.C:
                before = _state(h)
                with pytest.raises(RuntimeError):
                    h.dataset_get_labels(0, 1)
                with pytest.raises(RuntimeError):
                    h.train_step_dataset(0, 20, DC.K)                     # IWAE_ERR_STATE until the labels are set again
                _same_state(before, _state(h))
                y = (np.arange(n) % DC.C).astype(np.uint8)
                h.dataset_set_labels(y)
                from iwae_amd import task05
                np.testing.assert_array_equal(h.dataset_get_labels(7, 65), task05.one_hot(y[7:72], DC.C))
            r = h.train_step_dataset(0, 20, DC.K)
            assert np.isfinite(r["iwae_elbo"])
    finally:
        h.close()


# ---------------------------------------------------------------- 2. one resident step is the host-fed step
def _pair(m, precision, seed=SEED, twin_options=(), n=DC.N, options=()):
    """(resident handle A with the set, host-fed handle B without one); options: of both, twin_options: of B on top"""
    a, b = _model(m, precision, seed, options), _model(m, precision, seed, options + twin_options, tag=1)
    _upload(a, m, n)
    return a, b


def _one_step(a, b, m, seed, epoch, order, s, B, k, beta=1.0, objective="iwae_elbo", n=DC.N, step=3):
    for h in (a, b):
        _reset(h, m, step)
    ra = a.train_step_dataset(s, B, k, beta, 1e-3, objective)
    rb = _host_step(b, m, seed, epoch, order[s:s + B], k, beta, 1e-3, objective, n)
    assert np.isfinite(ra["iwae_elbo"])
    _same_scalars(ra, rb)
    _same_state(_state(a, min(B, 3), k), _state(b, min(B, 3), k))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("m", DC.STEP_MODELS, ids=DC.model_id)
def test_one_resident_step_is_the_host_fed_step(gpu, m, precision):
    a, b = _pair(m, precision)
    order = DC.order_of(EPOCH)
    a.dataset_begin_epoch(EPOCH, order)
    for (s, B) in DC.BATCHES:
        _one_step(a, b, m, SEED, EPOCH, order, s, B, DC.K)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("m", [DC.WIDE, DC.TWO_LAYER[1], DC.COND[5]], ids=DC.model_id)
def test_one_resident_step_at_the_other_seed_and_the_last_epoch(gpu, m, precision):
    a, b = _pair(m, precision, SEED_HI)
    epoch = DC.EPOCHS[2]
    order = DC.order_of(epoch)
    a.dataset_begin_epoch(epoch, order)
    for (s, B) in ((37, 150), (299, 1), (5, 129)):
        _one_step(a, b, m, SEED_HI, epoch, order, s, B, DC.K, step=2 ** 32 - 2)


def _objective_cases():
    out = [(DC.WIDE, obj, 1.0) for obj in DC.OBJECTIVES5] + [(DC.WIDE2, obj, 1.0) for obj in DC.OBJECTIVES_2L]
    return out + [(DC.WIDE, "vae_elbo_kl", 0.7)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("m,objective,beta", _objective_cases(), ids=lambda v: DC.model_id(v) if isinstance(v, DC.Model) else str(v))
def test_every_objective_steps_from_the_resident_set(gpu, m, objective, beta, precision):
    a, b = _pair(m, precision)
    order = DC.order_of(EPOCH)
    a.dataset_begin_epoch(EPOCH, order)
    _one_step(a, b, m, SEED, EPOCH, order, 37, 150, DC.K, beta, objective)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("batch", DC.LARGE_BATCHES, ids=lambda v: "%d_%d" % v)
def test_large_batches_on_either_side_of_the_fused_encoders_row_limit(gpu, batch, precision):
    """4 096 images: the host-fed twin's block_fwd_kernel converts the float32 rows itself; 4 097: prep_rows_kernel writes them first
    (_dataset_cases.enc_block_fused).  Both are above 2 048 data rows: side streams carry the decoder's weight gradients and the update."""
    m, n = DC.LARGE, DC.LARGE_N
    s, B = batch
    assert DC.enc_block_fused(m, B) == (B <= 4096)
    a, b = _pair(m, precision, n=n)
    order = DC.orders(n)[0]
    a.dataset_begin_epoch(EPOCH, order)
    np.testing.assert_array_equal(a.dataset_get_batch(s, B), DC.rows(m.X, SEED, EPOCH, order[s:s + B], n))
    _one_step(a, b, m, SEED, EPOCH, order, s, B, DC.LARGE_K, n=n)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_step_of_three_thousand_rows_uses_the_side_streams(gpu, precision):
    m = DC.WIDE
    a, b = _pair(m, precision)
    order = DC.order_of(EPOCH)
    a.dataset_begin_epoch(EPOCH, order)
    _one_step(a, b, m, SEED, EPOCH, order, 37, 150, DC.SIDE_K)


def test_the_gather_kernels_rows_are_prep_rows_kernels_rows(gpu):
    """Both handles under no_block_fused (the option changes every block's kernels, so the twin alone would be another step, not another input
    path): the host-fed twin's prep_rows_kernel writes the bf16 rows that the resident step's gather kernel wrote itself, and the same
    dense_kernel launches read them."""
    m = DC.WIDE
    assert not DC.enc_block_fused(m, 150, allow=False)
    a, b = _pair(m, "bf16", options=(("no_block_fused", 1),))
    order = DC.order_of(EPOCH)
    a.dataset_begin_epoch(EPOCH, order)
    for (s, B) in DC.BATCHES:
        _one_step(a, b, m, SEED, EPOCH, order, s, B, DC.K)


# ---------------------------------------------------------------- 3. sequences
def _walk(a, b, m, plan, k, seed=SEED, between=None, objective="iwae_elbo"):
    """Handle A steps from the resident set, handle B is host-fed the restated rows, no reset in between; `plan` holds (start, B) batches and
    ("epoch", e) changes.  The scalars are compared step by step, the state at the end."""
    epoch, order = None, None
    last = None
    for i, item in enumerate(plan):
        if item[0] == "epoch":
            epoch = item[1]
            order = DC.order_of(epoch)
            a.dataset_begin_epoch(epoch, order)
            continue
        s, B = item
        if between:
            between(a, i)
        ra = a.train_step_dataset(s, B, k, 1.0, 1e-3, objective)
        rb = _host_step(b, m, seed, epoch, order[s:s + B], k, 1.0, 1e-3, objective)
        _same_scalars(ra, rb)
        last = B
    _same_state(_state(a, min(last, 3), k), _state(b, min(last, 3), k))
    return _state(a, min(last, 3), k)


EPOCH_WALK = [("epoch", 7)] + DC.WALK + [("epoch", 8)] + DC.WALK


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("m", DC.WALK_MODELS, ids=DC.model_id)
def test_two_epochs_of_resident_steps_are_the_host_fed_steps(gpu, m, precision):
    """(0, 128), (128, 128), the ragged (256, 44), a new epoch with another order, the same three again: consecutive steps, the speculative
    draw a step ahead, the shrinking last batch, stale pad rows behind a larger batch."""
    a, b = _pair(m, precision)
    for h in (a, b):
        _reset(h, m, step=11)
    st = _walk(a, b, m, EPOCH_WALK, DC.K)
    assert st["t"] == 6


def test_two_epochs_with_the_side_streams_live_across_the_shrink(gpu):
    m = DC.WIDE
    a, b = _pair(m, "bf16")
    for h in (a, b):
        _reset(h, m, step=11)
    _walk(a, b, m, EPOCH_WALK, DC.SIDE_K)


@pytest.mark.parametrize("mode", ["bf16", "fp32", "bf16-no_eps_multi"])
def test_fifteen_steps_of_the_default_batch(gpu, mode):
    """B = 20, k = 5: the eight-steps-per-launch noise buffers, crossed twice; once against a twin that draws every step on its own."""
    m = DC.WIDE
    precision = mode.split("-")[0]
    a, b = _pair(m, precision, twin_options=(("no_eps_multi", 1),) if "-" in mode else ())
    for h in (a, b):
        _reset(h, m, step=5)
    st = _walk(a, b, m, [("epoch", 7)] + DC.DEFAULT_WALK, DC.K)
    assert st["t"] == 15


@pytest.mark.parametrize("k", [DC.K, DC.SIDE_K], ids=lambda v: "k%d" % v)
@pytest.mark.parametrize("m,precision", [(DC.WIDE, "bf16"), (DC.WIDE, "fp32"), (DC.WIDE_C, "bf16"), (DC.WIDE_CP, "bf16"), (DC.WIDE_C, "fp32")],
                         ids=lambda v: DC.model_id(v) if isinstance(v, DC.Model) else str(v))
def test_inspection_between_steps_changes_nothing(gpu, m, precision, k):
    """iwae_dataset_get_batch and iwae_dataset_get_labels of ANOTHER range between the steps: get_batch overwrites the bf16 input rows,
    get_labels the condition rows, behind a step whose side-stream work may still be in flight (k = 20: 2 560 data rows)."""
    a, b = _pair(m, precision)
    for h in (a, b):
        _reset(h, m, step=11)

    def between(h, i):
        s, B = [(5, 129), (0, 300), (299, 1)][i % 3]
        order = DC.order_of(7 if i < 4 else 8)
        np.testing.assert_array_equal(h.dataset_get_batch(s, B), DC.rows(m.X, SEED, 7 if i < 4 else 8, order[s:s + B]))
        if m.C:
            np.testing.assert_array_equal(h.dataset_get_labels(s, B), DC.one_hot(order[s:s + B]))

    _walk(a, b, m, EPOCH_WALK, k, between=between)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("m", [DC.WIDE, DC.WIDE_C], ids=DC.model_id)
def test_resident_and_host_fed_steps_interleave(gpu, m, precision):
    """One handle alternates resident steps and host-fed steps of other batches; its twin is host-fed throughout."""
    a, b = _pair(m, precision)
    for h in (a, b):
        _reset(h, m, step=11)
    order = DC.order_of(EPOCH)
    a.dataset_begin_epoch(EPOCH, order)
    plan = [(0, 128), (37, 150), (256, 44), (5, 129), (128, 128), (299, 1)]
    for i, (s, B) in enumerate(plan):
        ids = order[s:s + B]
        ra = a.train_step_dataset(s, B, DC.K) if i % 2 == 0 else _host_step(a, m, SEED, EPOCH, ids, DC.K)
        rb = _host_step(b, m, SEED, EPOCH, ids, DC.K)
        _same_scalars(ra, rb)
    _same_state(_state(a), _state(b))


# ---------------------------------------------------------------- 4. anchors to the float64 oracle
@pytest.mark.parametrize("m,precision", [(DC.WIDE, "bf16"), (DC.WIDE, "fp32"), (DC.WIDE2, "bf16"), (DC.WIDE_C, "bf16")],
                         ids=lambda v: DC.model_id(v) if isinstance(v, DC.Model) else str(v))
def test_a_resident_step_against_the_float64_oracle(gpu, m, precision):
    """One resident step against oracle/iwae_np on device_binarize's rows and device_eps's draws, at the tolerances the host-fed
    device-noise step of the family is held to: bf16 at EMU_SCALAR_ATOL / EMU_GRAD_REL against the oracle with the bf16 rounding points
    (test_gpu_parity.py: test_device_noise_step_matches_oracle_on_the_same_draws, test_kernel_family_boundaries_match_oracle,
    test_conditional_model_matches_oracle), float32 at F32_DEVNOISE_SCALAR_ATOL / F32_DEVNOISE_GRAD_REL against the exact oracle
    (test_float32_mode_with_device_noise_and_dataset_pipeline)."""
    s, B, k, step = 37, 20, DC.K, 9
    h = _model(m, precision)
    _upload(h, m)
    _reset(h, m, step)
    order = DC.order_of(EPOCH)
    h.dataset_begin_epoch(EPOCH, order)
    ids = order[s:s + B]
    r = h.train_step_dataset(s, B, k, 1.0, 1e-3, "iwae_elbo")
    flat = h.get_grads().copy()
    x, P = DC.rows(m.X, SEED, EPOCH, ids), DC.params(m)[1]
    rnd = O.bf16_round if precision == "bf16" else None
    if DC.layers(m) == 2:
        e1 = philox_np.device_eps(SEED, step, B, k, m.nl[0], stream=0)
        e2 = philox_np.device_eps(SEED, step, B, k, m.nl[1], stream=1)
        res, grads = O.loss_grads_2layer(P, x, e1, e2, 1.0, "iwae_elbo", rnd=rnd)
    else:
        eps = philox_np.device_eps(SEED, step, B, k, m.nl)
        res, grads = O.loss_grads_1layer(P, x, eps, 1.0, "iwae_elbo", rnd=rnd, y=DC.one_hot(ids) if m.C else None)
    atol, rel = (EMU_SCALAR_ATOL, EMU_GRAD_REL) if precision == "bf16" else (F32_DEVNOISE_SCALAR_ATOL, F32_DEVNOISE_GRAD_REL)
    d, errs = abs(r["iwae_elbo"] - float(res["iwae_elbo"])), _grad_rel_errors(flat, grads)
    print("%s %s resident step vs float64: iwae_elbo %.5f, |d| %.3g (< %.3g); gradient per tensor %.3g (< %.3g)"
          % (DC.model_id(m), precision, r["iwae_elbo"], d, atol, max(errs), rel))
    assert d < atol, (r["iwae_elbo"], float(res["iwae_elbo"]))
    assert max(errs) < rel, errs


# ---------------------------------------------------------------- 5. the data-parallel handle at world size 1
@pytest.mark.parametrize("precision", PRECISIONS)
def test_data_parallel_handle_world1_walks_the_resident_set_like_the_plain_handle(gpu, precision):
    """iwae_comm_init with one rank (as test_in_library_data_parallel_step_world1_is_bitwise_the_single_gpu_step), then main.py's multi-GPU
    loop: iwae_train_step_dataset per batch.  The three-batch walk ends bitwise on the plain, host-fed handle's state."""
    from iwae_amd.native import NativeModel
    m = DC.WIDE
    a, b = _new(m, precision), _model(m, precision, tag=1)
    try:
        _upload(a, m)
        for h in (a, b):
            _reset(h, m, step=11)
        a.comm_init(NativeModel.comm_unique_id(), 1, 0)
        _walk(a, b, m, [("epoch", 7)] + DC.WALK, DC.K)
        a.comm_destroy()
    finally:
        a.close()


# ---------------------------------------------------------------- 6. refusals
def _refuses(h, exc, call, before):
    with pytest.raises(exc):
        call()
    _same_state(before, _state(h))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("m", [DC.WIDE, DC.WIDE_C], ids=DC.model_id)
def test_refused_calls_launch_nothing_and_leave_the_handle_alone(gpu, m, precision):
    n = DC.N
    a, b = _new(m, precision), _model(m, precision, tag=1)
    try:
        for h in (a, b):
            _reset(h, m, step=11)
        before = _state(a)
        calls = {"step": lambda s, B: a.train_step_dataset(s, B, DC.K), "get_batch": a.dataset_get_batch, "get_labels": a.dataset_get_labels,
                 "get_mask": a.dataset_get_mask}
        for name, call in calls.items():                                                  # no uploaded set
            _refuses(a, RuntimeError, lambda: call(0, 1), before)
        _refuses(a, RuntimeError, lambda: a.dataset_begin_epoch(1, None), before)
        a.dataset_upload(DC.gray(m.X))
        order = DC.order_of(EPOCH)
        a.dataset_begin_epoch(EPOCH, order)
        for name, call in calls.items():                                                  # ranges outside the set
            for (s, B) in ((-1, 5), (0, 0), (5, -3), (n - 149, 150), (n, 1)):
                assert s < 0 or B <= 0 or s + B == n + 1
                _refuses(a, ValueError, lambda: call(s, B), before)
        for bad in (order[:-1], np.where(np.arange(n) == 17, n, order), np.where(np.arange(n) == 17, -1, order)):
            _refuses(a, ValueError, lambda: a.dataset_begin_epoch(EPOCH + 1, bad.astype(np.int32)), before)
        np.testing.assert_array_equal(a.dataset_get_batch(37, 150), DC.rows(m.X, SEED, EPOCH, order[37:187]))      # epoch and order are the old ones
        if m.C:
            _refuses(a, RuntimeError, lambda: a.train_step_dataset(37, 150, DC.K), before)                         # no labels yet
            _refuses(a, RuntimeError, lambda: a.dataset_get_labels(37, 150), before)
            y = np.array(DC.labels())
            y[17] = DC.C
            _refuses(a, ValueError, lambda: a.dataset_set_labels(y), before)
            _refuses(a, ValueError, lambda: a.dataset_set_labels(DC.labels()[:-1]), before)
            _refuses(a, RuntimeError, lambda: a.dataset_get_labels(37, 150), before)                               # ... and none were kept
            a.dataset_set_labels(DC.labels())
            _refuses(a, RuntimeError, lambda: a.dataset_get_mask(0, 1), before)                                    # no masks on this model
        else:
            _refuses(a, RuntimeError, lambda: a.dataset_set_labels(DC.labels()), before)                           # cond_dim = 0
            _refuses(a, RuntimeError, lambda: a.dataset_get_labels(37, 150), before)
            _refuses(a, RuntimeError, lambda: a.dataset_get_mask(0, 1), before)                                    # no masks set
        # the next valid step is the twin's, at the same noise step
        ra = a.train_step_dataset(37, 150, DC.K)
        rb = _host_step(b, m, SEED, EPOCH, order[37:187], DC.K)
        _same_scalars(ra, rb)
        _same_state(_state(a), _state(b))
    finally:
        a.close()


# ---------------------------------------------------------------- 7. the shim
@pytest.mark.parametrize("precision", PRECISIONS)
def test_shim_set_dataset_quantises_and_trains_like_the_native_calls(gpu, precision):
    from iwae_amd import iwae1
    from iwae_amd.optimizers import Adam
    m = DC.WIDE
    nh, nl, X = DC.dims(m)
    xf = np.random.default_rng(23).random((DC.N, X)).astype(np.float32)      # float images in [0, 1]
    xf[:, 0], xf[:, 1] = 0.0, 1.0
    q = np.rint(xf.astype(np.float64) * 255.0).astype(np.uint8)
    assert q[:, 0].max() == 0 and q[:, 1].min() == 255 and len(np.unique(q)) == 256
    order = DC.order_of(EPOCH)
    model = iwae1.IWAE(nh, nl, x_dim=X, seed=SEED, precision=precision)
    opt = Adam(1e-3, epsilon=1e-4)
    model.set_dataset(xf)
    model.begin_epoch(EPOCH, order)
    for (s, B) in ((37, 150), (299, 1)):
        np.testing.assert_array_equal(model._net.dataset_get_batch(s, B), philox_np.device_binarize(SEED, EPOCH, q, order[s:s + B]))
    twin = _model(m, precision, tag=1)
    twin.set_params(model._net.get_params())
    twin.set_adam_state(np.zeros(twin.n_params, np.float32), np.zeros(twin.n_params, np.float32), 0)
    twin.dataset_upload(q)
    twin.dataset_begin_epoch(EPOCH, order)
    model._net.set_step(3, 0)
    twin.set_step(3, 0)
    for i, (s, B) in enumerate(DC.WALK):
        r = model.train_step_dataset(s, B, DC.K, 1.0, opt, objective="iwae_elbo")
        rt = twin.train_step_dataset(s, B, DC.K, 1.0, 1e-3, "iwae_elbo")
        assert opt.iterations == i + 1
        assert float(r["iwae_elbo"]) == rt["iwae_elbo"]
    np.testing.assert_array_equal(model._net.get_params(), twin.get_params())
    assert model._net.get_adam_state()[2] == 3
