"""The resident per-image masks and the masked train step from the device dataset (iwae_dataset_set_mask / iwae_dataset_mcar_mask /
iwae_dataset_get_mask, iwae_train_step_dataset with a mask set; include/iwae_amd.h) on the case table of
tests/_masked_dataset_cases.py, whose admissibility tests/test_masked_dataset_host.py shows on the CPU.

The contract is bitwise: a resident masked step IS iwae_train_step_masked on (iwae_dataset_get_batch, iwae_dataset_get_mask) of its rows,
so every comparison with the host-fed handle is array_equal.  One direct check per precision against the float64 restatement
(_masked_ref.masked_loss_grads) at the existing masked tests' own tolerances (_parity_common) keeps the module from resting on the host
route alone.  The route is read off the launch counters: "masked_input" counts gather_binarize_masked_kernel, "masked_out" the float32
fused output layer.  Sections 1-3 go through NativeModel, section 4 through the shim."""
import numpy as np
import pytest

from oracle import iwae_np as O
from oracle import philox_np
import _masked_dataset_cases as DC
import _masked_ref as MR
from _parity_common import EXACT_GRAD_REL, EXACT_SCALAR_ATOL, F32_GRAD_REL, F32_SCALAR_REL, _grad_rel_errors

pytestmark = pytest.mark.gpu

SEED = 123
FAST = (("masked_out_min_rows", 1),)
# (precision, options, name of the float32 route)
MODES = [("bf16", (), "bf16"), ("fp32", (), "general"), ("fp32", FAST, "fast")]
_handles = {}


def _ids(v):
    if isinstance(v, tuple) and len(v) == 3 and all(isinstance(e, int) for e in v):
        return "%d_%d_%d" % v
    if isinstance(v, tuple) and len(v) == 3 and isinstance(v[0], str):
        return v[2]
    if isinstance(v, tuple):
        return "-".join(str(e[0]) for e in v) or "default"
    return str(v)


def _new(dims, precision, options=(), **kw):
    from iwae_amd.native import NativeModel
    nh, nl, xd = dims
    return NativeModel(kw.pop("n_layers", 1), kw.pop("n_hidden", nh), kw.pop("n_latent", nl), x_dim=xd, seed=SEED, precision=precision,
                       options=dict(options), **kw)


def _model(dims, precision, options=(), tag=0):
    """The module's handles: one per (shape, precision, options, tag); every test resets what it reads."""
    key = (dims, precision, options, tag)
    if key not in _handles:
        _handles[key] = _new(dims, precision, options)
    return _handles[key]


def _reset(m, dims, step=3):
    m.set_params(O.flatten_params(DC.params(dims)))
    m.set_adam_state(np.zeros(m.n_params, np.float32), np.zeros(m.n_params, np.float32), 0)
    m.set_step(step, 0)


def _state(m):
    mo, ve, t = m.get_adam_state()
    return m.get_params().copy(), mo, ve, t


def _same_state(a, b):
    for u, v in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(u, v)
    assert a[3] == b[3]


def _same_step(ra, rb, a, b):
    """Scalars, gradient buffer, parameters, Adam moments and step count of two handles behind a step: bitwise."""
    assert ra.keys() == rb.keys()
    for key in ra:
        assert ra[key] == rb[key] or (np.isnan(ra[key]) and np.isnan(rb[key])), (key, ra[key], rb[key])
    np.testing.assert_array_equal(a.get_grads(), b.get_grads())
    _same_state(_state(a), _state(b))


def _launches(m, name):
    return m.kernel_time(name)[1]


# ---------------------------------------------------------------- 1. packing and gather
@pytest.mark.parametrize("dims", DC.DIMS, ids=_ids)
def test_get_mask_returns_the_images_rows_in_every_epoch(gpu, dims):
    X = dims[2]
    g = DC.gray(X)
    m = _model(dims, "fp32")
    m.dataset_upload(g)
    with pytest.raises(Exception):
        m.dataset_get_mask(0, 1)                                  # no mask yet
    plain = {}
    for epoch, order in zip(DC.EPOCHS, DC.orders()):
        m.dataset_begin_epoch(epoch, order)
        for (s, B) in DC.BATCHES:
            plain[(epoch, s, B)] = m.dataset_get_batch(s, B)
            np.testing.assert_array_equal(plain[(epoch, s, B)], philox_np.device_binarize(SEED, epoch, g, order[s:s + B]))
    for name, make in DC.MASKS.items():
        mask = make(X)
        m.dataset_set_mask(mask)
        for epoch, order in zip(DC.EPOCHS, DC.orders()):          # the mask belongs to the image: another epoch, another order, the same rows
            m.dataset_begin_epoch(epoch, order)
            for (s, B) in DC.BATCHES:
                got = m.dataset_get_mask(s, B)
                assert got.dtype == np.uint8 and got.shape == (B, X)
                np.testing.assert_array_equal(got, mask[order[s:s + B]], err_msg="%s epoch %d (%d, %d)" % (name, epoch, s, B))
                np.testing.assert_array_equal(m.dataset_get_batch(s, B), plain[(epoch, s, B)])      # the complete rows, mask or not
    with pytest.raises(ValueError):
        m.dataset_get_mask(200, 150)                              # range outside the set
    m.dataset_set_mask(None)
    with pytest.raises(Exception):
        m.dataset_get_mask(0, 1)
    m.dataset_set_mask(DC.half_mask(X))
    m.dataset_upload(g)                                           # a new set drops the masks
    with pytest.raises(Exception):
        m.dataset_get_mask(0, 1)


@pytest.mark.parametrize("dims", DC.DIMS, ids=_ids)
def test_mcar_mask_is_the_host_restatement_bit_for_bit(gpu, dims):
    from iwae_amd import utils
    X = dims[2]
    m = _model(dims, "fp32")
    m.dataset_upload(DC.gray(X))
    order = DC.orders()[1]
    for seed in DC.MCAR_SEEDS:
        for rate in DC.MCAR_RATES:
            m.dataset_mcar_mask(rate, seed)
            ref = utils.device_mcar_mask(DC.N, X, rate, seed)
            m.dataset_begin_epoch(0, np.arange(DC.N, dtype=np.int32))
            np.testing.assert_array_equal(m.dataset_get_mask(0, DC.N), ref, err_msg="rate %g seed %d" % (rate, seed))
            m.dataset_begin_epoch(2, order)
            np.testing.assert_array_equal(m.dataset_get_mask(37, 150), ref[order[37:187]])
    # keyed by the caller's seed, not the handle's: a handle with another weight seed draws the same masks
    from iwae_amd.native import NativeModel
    o = NativeModel(1, dims[0], dims[1], x_dim=X, seed=SEED + 1, precision="fp32")
    try:
        o.dataset_upload(DC.gray(X))
        o.dataset_mcar_mask(0.5, DC.MCAR_SEEDS[0])
        np.testing.assert_array_equal(o.dataset_get_mask(0, DC.N), utils.device_mcar_mask(DC.N, X, 0.5, DC.MCAR_SEEDS[0]))
    finally:
        o.close()


@pytest.mark.parametrize("dims", [DC.WIDE, (37, 5, 53)], ids=_ids)
def test_a_device_pointer_mask_uploads_like_a_host_one(gpu, dims):
    import torch
    X = dims[2]
    mask = DC.half_mask(X)
    m = _model(dims, "fp32")
    m.dataset_upload(DC.gray(X))
    m.dataset_begin_epoch(DC.EPOCHS[0], DC.orders()[0])
    t = torch.from_numpy(np.array(mask) * 3).to(torch.uint8).cuda()      # non-zero = observed
    torch.cuda.synchronize()
    m.dataset_set_mask(t)
    for (s, B) in DC.BATCHES:
        np.testing.assert_array_equal(m.dataset_get_mask(s, B), mask[DC.orders()[0][s:s + B]])
    out = torch.empty((150, X), dtype=torch.uint8, device="cuda")        # a device destination is written in place
    from iwae_amd._capi import check
    check(m.lib.iwae_dataset_get_mask(m.h, 37, 150, out.data_ptr()))
    np.testing.assert_array_equal(out.cpu().numpy(), mask[DC.orders()[0][37:187]])


# ---------------------------------------------------------------- 2. the step
def _pair(dims, precision, options):
    """(resident handle, host-fed handle) of a mode: same parameters, Adam state and step; both hold the set (the second to read batches)."""
    a, b = _model(dims, precision, options, 0), _model(dims, precision, options, 1)
    for m in (a, b):
        _reset(m, dims)
        m.dataset_upload(DC.gray(dims[2]))
    return a, b


def _run_steps(dims, precision, options, route, mask, objective="iwae_elbo", plan=None):
    """Resident masked steps on one handle against train_step(x = dataset_get_batch, mask = dataset_get_mask) on a second, bitwise after
    every step; an epoch change (another order) where the plan says so.  Returns the launches read off both handles."""
    plan = plan or [(37, 150), (0, 1), "epoch", (172, 128), (299, 1)]
    a, b = _pair(dims, precision, options)
    a.dataset_set_mask(mask)
    b.dataset_set_mask(mask)
    epochs = iter(zip(DC.EPOCHS, DC.orders()))
    epoch, order = next(epochs)
    for m in (a, b):
        m.dataset_begin_epoch(epoch, order)
        m.enable_timing(1)
    steps = 0
    try:
        for item in plan:
            if item == "epoch":
                epoch, order = next(epochs)
                for m in (a, b):
                    m.dataset_begin_epoch(epoch, order)
                continue
            s, B = item
            x, mk = b.dataset_get_batch(s, B), b.dataset_get_mask(s, B)
            np.testing.assert_array_equal(mk, mask[order[s:s + B]])
            ra = a.train_step_dataset(s, B, DC.K, 1.0, 1e-3, objective)
            rb = b.train_step(x, DC.K, 1.0, 1e-3, objective, mask=mk)
            steps += 1
            assert np.isfinite(ra["iwae_elbo"])
            _same_step(ra, rb, a, b)
        got = {"input_a": _launches(a, "masked_input"), "input_b": _launches(b, "masked_input"),
               "out_a": _launches(a, "masked_out"), "out_b": _launches(b, "masked_out")}
    finally:
        for m in (a, b):
            m.enable_timing(0)
            m.dataset_set_mask(None)
    # the route witness: one launch of the input kernel per resident masked step, none on the host-fed handle
    assert got["input_a"] == steps and got["input_b"] == 0, got
    if route == "fast":
        assert got["out_a"] == steps and got["out_b"] == steps, got
    else:
        assert got["out_a"] == 0 and got["out_b"] == 0, got
    assert _state(a)[3] == steps
    return got


def _mode_cases():
    out = []
    for dims in DC.DIMS:
        for mode in MODES:
            if mode[2] == "fast" and not DC.fast_route_accepts(dims):
                continue          # (37 / 5 / 53: x_dim no multiple of 4, masked_out_f32_ok refuses -- the general route is that shape's only one)
            out.append((dims, mode))
    return out


@pytest.mark.parametrize("dims,mode", _mode_cases(), ids=_ids)
def test_resident_masked_steps_are_the_host_fed_masked_steps(gpu, dims, mode):
    precision, options, route = mode
    _run_steps(dims, precision, options, route, DC.half_mask(dims[2]))


@pytest.mark.parametrize("objective", DC.OBJECTIVES5)
@pytest.mark.parametrize("mode", MODES, ids=_ids)
def test_every_objective_runs_from_the_resident_masked_set(gpu, mode, objective):
    precision, options, route = mode
    _run_steps(DC.WIDE, precision, options, route, DC.half_mask(DC.WIDE[2]), objective, plan=[(37, 150)])


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_resident_masked_step_against_the_float64_restatement(gpu, precision):
    """The gradient the resident step leaves and its bound against _masked_ref.masked_loss_grads on the batch, at the device's own draws
    (iwae_debug_eps at the step's counters): bf16 at EXACT_GRAD_REL / EXACT_SCALAR_ATOL, float32 at F32_GRAD_REL / F32_SCALAR_REL + 2e-4,
    as test_gpu_masked_bf16.py and test_gpu_masked_step.py hold the host-fed step."""
    dims = DC.WIDE
    X = dims[2]
    s, B = DC.BATCHES[0]
    mask, order = DC.half_mask(X), DC.orders()[0]
    m = _model(dims, precision)
    _reset(m, dims)
    m.dataset_upload(DC.gray(X))
    m.dataset_set_mask(mask)
    m.dataset_begin_epoch(DC.EPOCHS[0], order)
    try:
        x, mk = m.dataset_get_batch(s, B), m.dataset_get_mask(s, B)
        eps = m.debug_eps(B, DC.K, 0)
        r = m.train_step_dataset(s, B, DC.K, 1.0, 1e-3, "iwae_elbo")
        flat = m.get_grads().copy()
    finally:
        m.dataset_set_mask(None)
    res, grads = MR.masked_loss_grads(DC.params(dims), x, mk, eps, 1.0, "iwae_elbo")
    errs = _grad_rel_errors(flat, grads)
    d = abs(r["iwae_elbo"] - float(res["iwae_elbo"]))
    rel, atol = (F32_GRAD_REL, F32_SCALAR_REL * abs(float(res["iwae_elbo"])) + 2e-4) if precision == "fp32" else (EXACT_GRAD_REL, EXACT_SCALAR_ATOL)
    print("%s resident masked step vs float64: iwae_elbo %.5f, |d| %.3g (< %.3g); gradient per tensor %.3g (< %.3g)"
          % (precision, r["iwae_elbo"], d, atol, max(errs), rel))
    assert d < atol, (r["iwae_elbo"], float(res["iwae_elbo"]))
    assert max(errs) < rel, errs
    # an unobserved pixel column moves nothing: the dead column's rows of the first encoder kernel and columns of W3 / b3 have zero gradient
    P = DC.params(dims)
    gW1 = flat[:P[0][0].size].reshape(P[0][0].shape)
    assert np.all(gW1[DC.DEAD_COLUMN] == 0.0) and np.any(gW1 != 0.0)


# ---------------------------------------------------------------- 3. nothing else moved
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_a_dropped_mask_leaves_the_unmasked_step(gpu, precision):
    """A mask set and dropped (NULL), and a mask dropped by a fresh upload: the step is the step of a handle that never had one."""
    dims = DC.WIDE
    X = dims[2]
    s, B = DC.BATCHES[0]

    def run(prepare):
        m = _model(dims, precision)
        _reset(m, dims)
        m.dataset_upload(DC.gray(X))
        prepare(m)
        m.dataset_begin_epoch(DC.EPOCHS[0], DC.orders()[0])
        m.enable_timing(1)
        try:
            r = m.train_step_dataset(s, B, DC.K, 1.0, 1e-3, "iwae_elbo")
            assert _launches(m, "masked_input") == 0
        finally:
            m.enable_timing(0)
        return r, m.get_grads().copy(), _state(m)

    def dropped(m):
        m.dataset_set_mask(DC.half_mask(X))
        m.dataset_set_mask(None)

    def reuploaded(m):
        m.dataset_mcar_mask(0.5, 9)
        m.dataset_upload(DC.gray(X))

    never = run(lambda m: None)
    for other in (run(dropped), run(reuploaded)):
        assert other[0] == never[0]
        np.testing.assert_array_equal(other[1], never[1])
        _same_state(other[2], never[2])


@pytest.mark.parametrize("dims,mode", [(DC.WIDE, md) for md in MODES] + [((37, 5, 53), MODES[0]), ((37, 5, 53), MODES[1])], ids=_ids)
def test_a_mask_of_ones_is_the_host_fed_step_under_a_mask_of_ones(gpu, dims, mode):
    precision, options, route = mode
    _run_steps(dims, precision, options, route, DC.ones_mask(dims[2]), plan=[(37, 150), (299, 1)])


@pytest.mark.parametrize("bk", [(20, 5), (200, 50)], ids=lambda v: "B%d_k%d" % v)
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_resident_masked_and_host_unmasked_steps_interleave_like_fresh_handles(gpu, precision, bk):
    """resident masked, host unmasked, resident masked on ONE handle: every step is bitwise the same step on a fresh handle started from the
    state in front of it.  (20, 5): the multi-step noise buffers; (200, 50): the speculative draw on a side stream and the deferred decoder
    update (section 20's alternation test picks them the same way)."""
    dims = DC.WIDE
    X = dims[2]
    B, k = bk
    g, mask, order = DC.gray(X), DC.half_mask(X), DC.orders()[0]
    starts = (37, None, 100)

    def prepare(m):
        m.dataset_upload(g)
        m.dataset_set_mask(mask)
        m.dataset_begin_epoch(DC.EPOCHS[0], order)

    def step(m, i):
        if starts[i] is None:
            return m.train_step(xh, k, 1.0, 1e-3, "iwae_elbo")
        return m.train_step_dataset(starts[i], B, k, 1.0, 1e-3, "iwae_elbo")

    m = _model(dims, precision)
    _reset(m, dims, step=11)
    prepare(m)
    xh = m.dataset_get_batch(60, B)
    trail = []
    try:
        for i in range(3):
            before = _state(m)
            r = step(m, i)
            trail.append((before, r, _state(m), m.get_grads().copy()))
    finally:
        m.dataset_set_mask(None)
    assert trail[-1][2][3] == 3
    for i in range(3):
        before, r, after, grads = trail[i]
        f = _new(dims, precision)
        try:
            f.set_params(before[0])
            f.set_adam_state(before[1], before[2], before[3])
            f.set_step(11 + i, 0)
            prepare(f)
            rf = step(f, i)
            assert rf == r, (i, rf, r)
            np.testing.assert_array_equal(f.get_grads(), grads)
            _same_state(_state(f), after)
        finally:
            f.close()


def _refused_step(m, exc):
    """A resident masked step the handle refuses: raises, leaves parameters, Adam state and the noise step alone, and the next valid call (the
    unmasked resident step, the mask dropped) runs at the same noise step.  Returns (state before, that step's scalars, state after)."""
    s, B = DC.BATCHES[0]
    m.set_step(7, 0)
    before = _state(m)
    with pytest.raises(exc):
        m.train_step_dataset(s, B, DC.K, 1.0, 1e-3, "iwae_elbo")
    _same_state(before, _state(m))
    m.dataset_set_mask(None)
    r = m.train_step_dataset(s, B, DC.K, 1.0, 1e-3, "iwae_elbo")      # the noise step is still 7, ds_start was reset
    return before, r, _state(m)


def _fresh_unmasked(dims, precision, options, before):
    f = _new(dims, precision, options)
    try:
        f.set_params(before[0])
        f.set_adam_state(before[1], before[2], before[3])
        f.set_step(7, 0)
        f.dataset_upload(DC.gray(dims[2]))
        f.dataset_begin_epoch(DC.EPOCHS[0], DC.orders()[0])
        s, B = DC.BATCHES[0]
        return f.train_step_dataset(s, B, DC.K, 1.0, 1e-3, "iwae_elbo"), _state(f)
    finally:
        f.close()


@pytest.mark.parametrize("dims,options", [(DC.REFUSED_BF16[0], ()), (DC.REFUSED_BF16[1], ()), ((64, 8, 100), (("out_recompute", 1),))], ids=_ids)
def test_bf16_handles_the_masked_step_refuses_may_hold_a_mask_but_not_step(gpu, dims, options):
    X = dims[2]
    P = MR.case(*dims, 5, 13)[1]
    m = _new(dims, "bf16", options)
    try:
        m.set_params(O.flatten_params(P))
        m.dataset_upload(DC.gray(X))
        m.dataset_begin_epoch(DC.EPOCHS[0], DC.orders()[0])
        s, B = DC.BATCHES[0]
        m.train_step_dataset(s, B, DC.K, 1.0, 1e-3, "iwae_elbo")              # (Adam moments to be left alone)
        m.dataset_set_mask(DC.half_mask(X))                                    # held ...
        np.testing.assert_array_equal(m.dataset_get_mask(s, B), DC.half_mask(X)[DC.orders()[0][s:s + B]])
        before, r, after = _refused_step(m, ValueError)                  # ... the step is what refuses
        rf, sf = _fresh_unmasked(dims, "bf16", options, before)
        assert rf == r
        _same_state(sf, after)
    finally:
        m.close()


def test_mask_calls_refuse_other_models_bad_sizes_and_bad_rates(gpu):
    from iwae_amd._capi import IwaeError
    dims = (64, 8, 100)
    nh, nl, X = dims
    g, mask = DC.gray(X), DC.half_mask(X)
    # a 2-layer handle, a conditional handle: state errors, as iwae_dataset_set_labels refuses the wrong model
    for kw in (dict(n_layers=2, n_hidden=[nh, 32], n_latent=[nl, 2]), dict(cond_dim=3)):
        o = _new(dims, "bf16", **kw)
        try:
            o.dataset_upload(g)
            if kw.get("cond_dim"):
                o.dataset_set_labels(np.arange(DC.N) % 3)
            o.dataset_begin_epoch(DC.EPOCHS[0], DC.orders()[0])
            o.train_step_dataset(37, 20, DC.K, 1.0, 1e-3, "iwae_elbo")
            o.set_step(7, 0)
            before = _state(o)
            with pytest.raises(IwaeError):
                o.dataset_set_mask(mask)
            with pytest.raises(IwaeError):
                o.dataset_mcar_mask(0.5, 1)
            with pytest.raises(Exception):
                o.dataset_get_mask(0, 1)
            _same_state(before, _state(o))
            r = o.train_step_dataset(37, 20, DC.K, 1.0, 1e-3, "iwae_elbo")     # still the unmasked step, at step 7
            assert _launches(o, "masked_input") == 0
            f = _new(dims, "bf16", **kw)
            try:
                f.set_params(before[0])
                f.set_adam_state(before[1], before[2], before[3])
                f.set_step(7, 0)
                f.dataset_upload(g)
                if kw.get("cond_dim"):
                    f.dataset_set_labels(np.arange(DC.N) % 3)
                f.dataset_begin_epoch(DC.EPOCHS[0], DC.orders()[0])
                assert f.train_step_dataset(37, 20, DC.K, 1.0, 1e-3, "iwae_elbo") == r
                _same_state(_state(f), _state(o))
            finally:
                f.close()
        finally:
            o.close()
    for precision in ("bf16", "fp32"):
        m = _new(dims, precision)
        try:
            _reset(m, dims, step=7)
            # before any upload
            with pytest.raises(IwaeError):
                m.dataset_set_mask(mask)
            with pytest.raises(IwaeError):
                m.dataset_mcar_mask(0.5, 1)
            m.dataset_upload(g)
            m.dataset_begin_epoch(DC.EPOCHS[0], DC.orders()[0])
            # a wrong n; a rate outside [0, 1], NaN
            with pytest.raises(ValueError):
                m.dataset_set_mask(mask[:-1])
            for rate in (-0.1, 1.5, float("nan")):
                with pytest.raises(ValueError):
                    m.dataset_mcar_mask(rate, 1)
            with pytest.raises(Exception):
                m.dataset_get_mask(0, 1)                                       # none of them left a mask behind
            before = _state(m)
            # the next valid step is a fresh handle's: a resident masked step at step 7
            m.dataset_set_mask(mask)
            s, B = DC.BATCHES[0]
            r = m.train_step_dataset(s, B, DC.K, 1.0, 1e-3, "iwae_elbo")
            f = _new(dims, precision)
            try:
                _reset(f, dims, step=7)
                f.dataset_upload(g)
                f.dataset_set_mask(mask)
                f.dataset_begin_epoch(DC.EPOCHS[0], DC.orders()[0])
                assert f.train_step_dataset(s, B, DC.K, 1.0, 1e-3, "iwae_elbo") == r
                _same_state(_state(f), _state(m))
            finally:
                f.close()
        finally:
            m.close()


# ---------------------------------------------------------------- 4. the shim
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_shim_set_dataset_with_a_mask_trains_the_masked_step(gpu, precision):
    from iwae_amd import iwae1, iwae2
    from iwae_amd.optimizers import Adam
    dims = DC.WIDE
    nh, nl, X = dims
    g, mask, order = DC.gray(X), DC.half_mask(X), DC.orders()[0]
    s, B = DC.BATCHES[0]
    a, b = (iwae1.IWAE(nh, nl, x_dim=X, seed=SEED, precision=precision) for _ in range(2))
    oa, ob = Adam(1e-3, epsilon=1e-4), Adam(1e-3, epsilon=1e-4)
    a.set_dataset(g, mask)
    a.begin_epoch(DC.EPOCHS[0], order)
    b.set_dataset(g)
    b.begin_epoch(DC.EPOCHS[0], order)
    x, mk = b._net.dataset_get_batch(s, B), mask[order[s:s + B]]
    for m in (a, b):
        m._net.set_step(3, 0)
    ra = a.train_step_dataset(s, B, DC.K, 1.0, oa, objective="iwae_elbo")
    rb = b.train_step(x, DC.K, 1.0, ob, objective="iwae_elbo", mask=mk)
    assert oa.iterations == ob.iterations == 1
    for key in a.scalar_keys:
        assert float(ra[key]) == float(rb[key]), key
    for key in ("lpxz", "lpz", "lqzx"):                              # the step's means against the host-fed step's per-row tensors
        assert abs(float(ra[key]) - float(np.mean(rb[key]))) <= 1e-5 * abs(float(np.mean(rb[key]))) + 1e-3, key
    np.testing.assert_array_equal(a._net.get_params(), b._net.get_params())
    with pytest.raises(ValueError):
        iwae2.IWAE([nh, 32], [nl, 2], x_dim=X, seed=SEED).set_dataset(g, mask=mask)


def test_miwae_driver_trains_from_the_resident_set(gpu, capsys):
    """tasks/miwae.py --resident: both models train through set_dataset / begin_epoch / train_step_dataset (the masked one with its masks
    resident), finite traces of the right length, and the run prints what the host-fed run prints."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tasks"))
    try:
        import miwae
    finally:
        sys.path.pop(0)
    out = miwae.main(["--resident", "--images", "64", "--test-images", "32", "--steps", "40", "--batch_size", "16", "--n_samples", "5", "--draws", "8"])
    assert set(out) == {"masked", "zero_filled"}
    for name in out:
        tr = out[name]["trace"]
        assert len(tr) == 40 and np.all(np.isfinite(tr))
        assert np.isfinite(out[name]["log_px"]) and np.isfinite(out[name]["cross_entropy"]) and 0.0 <= out[name]["abs_error"] <= 1.0
    tr = out["masked"]["trace"]
    assert np.mean(tr[-5:]) > np.mean(tr[:5])                          # the masked bound rises over the steps
    assert out["masked"]["trace"] != out["zero_filled"]["trace"]
    assert "resident" in capsys.readouterr().out
