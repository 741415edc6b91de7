"""The Adam update of the training step, element by element against float64 (_adam_ref.py: reference, derived bounds, inputs, cases).

Three kernels apply the same adam_math: adam_kernel (iwae_adam_step, and every step that ends with the gradient joined),
reduce_grads_kernel with the update in its epilogue and wgrad_rows_kernel (the fused single-GPU step).  Each has its own element
addressing, its own AdamCoef and its own launcher for the betas and epsilon, and each refreshes the bf16 weight images behind the update.

  * injected gradients: a constructed gradient is written into the flat buffer (iwae_grad_devptr), so adam_kernel is held to the bounds on
    every element at hyper-parameters, step counts, gradient scales and magnitudes no training run reaches;
  * fused appliers: a fused train_step leaves the gradient it used in the flat buffer, so the same check applies to the other two kernels,
    off the default hyper-parameters and from a preloaded late state, together with the bitwise equality of the three appliers;
  * the weight images: a forward pass on the stepped handle against a fresh handle loaded with its parameters, bitwise;
  * checkpoint round trip, the reference-API shim's optimizer objects, rejected arguments.

The bounds are derived from the roundings of the update (see _adam_ref.py), not measured on the device; every test prints its figures
("figure / 1") before it asserts.
"""
import numpy as np
import pytest

import make_golden as MG
import _adam_ref as R

pytestmark = pytest.mark.gpu

SEED = 123
L2_SMALL = ([67, 35], [33, 3], 61)      # the ragged 2-layer shape of test_gpu_ragged_widths.py

# name -> (layers, n_hidden, n_latent, x_dim, cond_dim, precision): the smallest models that reach each layout of the layer table
MODELS = {
    "16/4/48": (1, 16, 4, 48, 0, "bf16"),
    "37/5/53": (1, 37, 5, 53, 0, "bf16"),                 # every layer ends in a partial 256-element block and a ragged head
    "200/100/784": (1, 200, 100, 784, 0, "bf16"),         # 455 k elements, many blocks per layer
    "2L-16,8/4,2/48": (2, [16, 8], [4, 2], 48, 0, "bf16"),
    "2L-ragged": (2,) + L2_SMALL + (0, "bf16"),
    "cond-prior-16/4/48": (1, 16, 4, 48, 10, "bf16"),     # the prior network's block sits behind the decoder's in the table
    "fp32-200/100/784": (1, 200, 100, 784, 0, "fp32"),
    "fp32-2L-16,8/4,2/48": (2, [16, 8], [4, 2], 48, 0, "fp32"),
    "2L-200,100/100,50/784": (2, [200, 100], [100, 50], 784, 0, "bf16"),
    "cond-prior-200/100/784": (1, 200, 100, 784, 10, "bf16"),
}


def _make(name, options=None):
    from iwae_amd.native import NativeModel
    layers, nh, nl, xd, C, prec = MODELS[name]
    return NativeModel(layers, nh, nl, x_dim=xd, seed=SEED, cond_dim=C, cond_prior=C > 0, precision=prec, options=options)


def _data(name, B, k, seed):
    """(x, flat seeded init, eps, y or None) of a model."""
    from oracle import iwae_np as O
    layers, nh, nl, xd, C, _ = MODELS[name]
    out = MG.inputs(layers, nh, nl, xd, B, k, seed, C, C > 0)
    return out[0], O.flatten_params(out[1]).astype(np.float32), out[2], (out[3] if C else None)


def _inject(m, g):
    """Write g into the handle's flat gradient buffer with torch (the pointer viewed as iwae_amd/parallel.py does).  The library runs on its
    own stream: it is idle before the write (sync) and the write is complete before the library is called again."""
    import torch
    from iwae_amd.parallel import _DevArray
    ptr, n = m.grad_devptr()
    assert n == g.size
    m.sync()
    torch.as_tensor(_DevArray(ptr, n), device="cuda").copy_(torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)))
    torch.cuda.synchronize()


def _state(m):
    mo, vo, t = m.get_adam_state()
    return m.get_params(), mo, vo, t


def _check(label, before, g, after, t, lr, b1, b2, eps, gscale):
    """The element check of one step: prints the three figures, then asserts them."""
    (w0, m0, v0), (w1, m1, v1) = before, after
    fm, fv, fw = R.adam_excess(w0, g, m0, v0, t, lr, b1, b2, eps, gscale, w1, m1, v1)
    print("adam_excess %s: m %.3f / 1, v %.3f / 1, w %.3f / 1" % (label, fm, fv, fw))
    assert fm <= 1.0 and fv <= 1.0 and fw <= 1.0, (label, fm, fv, fw)
    return fm, fv, fw


def _injected_step(m, c, w, g, mo, vo, label, exact=True):
    """set_params, set_adam_state, set_adam, adam_step on an injected gradient; read back; element check + exact rule (exact: the inputs
    hold elements the rule applies to)."""
    m.set_params(w)
    m.set_adam_state(mo, vo, c.t0)
    m.set_adam(c.b1, c.b2, c.eps)
    _inject(m, g)
    m.adam_step(c.lr, c.gscale)
    w1, m1, v1, t1 = _state(m)
    assert t1 == c.t0 + 1
    _check(label, (w, mo, vo), g, (w1, m1, v1), t1, c.lr, c.b1, c.b2, c.eps, c.gscale)
    n_still, n_bad = R.exact_rule_violations(w, g, mo, vo, w1, m1, v1)
    assert n_still >= int(exact) and n_bad == 0, (label, n_still, n_bad)
    return w1, m1, v1


INJECTED = [("37/5/53", c.id) for c in R.HYPER_CASES] + [(name, cid) for name in ("16/4/48", "200/100/784", "2L-16,8/4,2/48", "2L-ragged",
                                                                                  "cond-prior-16/4/48", "fp32-200/100/784", "fp32-2L-16,8/4,2/48")
                                                         for cid in ("B", "D")]


@pytest.mark.parametrize("name,cid", INJECTED)
def test_adam_kernel_on_injected_gradients(gpu, name, cid):
    """adam_kernel, every element of the table against float64 at the case's hyper-parameters, step count and gradient scale."""
    c = R.CASE[cid]
    m = _make(name)
    w, g, mo, vo = R.adam_inputs(m.n_params, 100 + ord(cid), c.fresh)
    w1, _, _ = _injected_step(m, c, w, g, mo, vo, "injected %s case %s" % (name, cid))
    if cid == "G":      # lr = 0: the parameters are bitwise what they were
        np.testing.assert_array_equal(w1.view(np.uint32), w.view(np.uint32))
    m.close()


def _forward_on_fresh_handle_is_bitwise(m, name, x, eps, y):
    """forward(x, k, eps) on the stepped handle m against a fresh handle loaded with m.get_params(): per-row densities and scalars, bitwise.
    The bf16 weight images and the bias blocks the stepped handle's kernels read were refreshed element by element behind the update; the
    fresh handle rebuilds all of them from the parameters."""
    k = (eps[0] if isinstance(eps, tuple) else eps).shape[0]
    want = ("lpxz", "lpz", "lqzx", "lpz2", "lqzx2", "log_w")
    f = _make(name)
    f.set_params(m.get_params())
    out = []
    for h in (m, f):
        if y is not None:
            h.set_condition(y)
        out.append(h.forward(x, k, 1.0, eps=eps, want=want))
    f.close()
    for key, a in out[0].items():
        if isinstance(a, np.ndarray) or key == "iwae_elbo":
            assert np.all(np.isfinite(a)), key
        np.testing.assert_array_equal(np.asarray(a), np.asarray(out[1][key]), err_msg=key)


@pytest.mark.parametrize("name,cid", [("37/5/53", "B"), ("37/5/53", "D"), ("16/4/48", "D"), ("200/100/784", "D"), ("2L-16,8/4,2/48", "D"),
                                      ("2L-ragged", "D"), ("cond-prior-16/4/48", "D")])
def test_weight_images_follow_an_injected_step(gpu, name, cid):
    """After adam_step the kernels' weight images are the new parameters': the seeded init stepped once on a constructed gradient and a
    plausible preloaded state (no weight moves by more than ~3 alpha, the model stays sane), then forward(x, k = 3, eps) against a fresh
    handle.  A bias element skipped at a layer's last partial block, or a weight written at the wrong (i, j) of an image, shows here."""
    c = R.CASE[cid]
    x, w, eps, y = _data(name, 5, 3, 41)
    m = _make(name)
    _, g, mo, vo = R.adam_inputs(m.n_params, 200 + ord(cid))
    mo, vo = R.plausible_state(mo, vo)
    w1, _, _ = _injected_step(m, c, w, g, mo, vo, "images %s case %s" % (name, cid), exact=False)
    assert np.count_nonzero(w1 != w) > 0.8 * w.size
    _forward_on_fresh_handle_is_bitwise(m, name, x, eps, y)
    m.close()


def test_hyper_parameters_are_per_handle(gpu):
    """Two handles with different hyper-parameters, stepped alternately on injected gradients: each matches its own reference."""
    hs = [(_make("37/5/53"), R.CASE["C"]), (_make("37/5/53"), R.CASE["D"])]
    n = hs[0][0].n_params
    for i, (m, c) in enumerate(hs):
        w, _, mo, vo = R.adam_inputs(n, 300 + i)
        m.set_params(w)
        m.set_adam_state(mo, vo, c.t0)
        m.set_adam(c.b1, c.b2, c.eps)
    for step in range(2):
        for i, (m, c) in enumerate(hs):
            w0, m0, v0, t0 = _state(m)
            _, g, _, _ = R.adam_inputs(n, 310 + 2 * step + i)
            _inject(m, g)
            m.adam_step(c.lr, c.gscale)
            w1, m1, v1, t1 = _state(m)
            assert t1 == t0 + 1 == c.t0 + step + 1
            _check("two handles, handle %d (case %s) step %d" % (i, c.id, step), (w0, m0, v0), g, (w1, m1, v1), t1, c.lr, c.b1, c.b2, c.eps, c.gscale)
    for m, _ in hs:
        m.close()


# ---- the fused appliers: reduce_grads_kernel with the update on, wgrad_rows_kernel ---------------------------------------------------
T_LATE = 99_999
FUSED = [  # (model, B, k): the shapes that reach each branch of the end-of-step plan (test_every_end_of_the_step_lands_on_the_same_parameters)
    ("200/100/784", 20, 5), ("200/100/784", 60, 50), ("200/100/784", 100, 50), ("200/100/784", 170, 50),
    ("2L-200,100/100,50/784", 170, 50),
    ("cond-prior-200/100/784", 6, 5),
    ("fp32-200/100/784", 20, 5), ("fp32-200/100/784", 100, 50),
    ("37/5/53", 5, 3), ("37/5/53", 170, 50),
]
FUSED_STEPS = [(R.CASE["B"], 1e-3), (R.CASE["D"], 1e-2)]      # (betas and epsilon of the case, lr); a fused step has grad_scale 1


def _two_steps(name, x, y, k, w, mo, vo, how):
    """Two steps from the preloaded late state, case B's hyper-parameters then case D's, on the device's own noise.
    how = "fused": train_step twice back to back, nothing read in between (at the large shapes the second step runs while the first one's
    deferred decoder update is the most recent work on the side stream, and set_adam falls in between);
    "fused_read": the same with parameters, state and the gradient read after every step; "split": forward_backward + adam_step, read.
    Returns the list of (w, m, v, t, g) after each step (only the last one for "fused")."""
    m = _make(name)
    m.set_params(w)
    m.set_adam_state(mo, vo, T_LATE)
    m.set_step(0, 0)
    seen = []
    for c, lr in FUSED_STEPS:
        m.set_adam(c.b1, c.b2, c.eps)
        if y is not None:
            m.set_condition(y)
        if how == "split":
            m.forward_backward(x, k, 1.0, "iwae_elbo")
            m.adam_step(lr)
        else:
            m.train_step(x, k, 1.0, lr, "iwae_elbo", scalars=False)
        if how != "fused":
            seen.append(_state(m) + (m.get_grads(),))
    if how == "fused":
        seen.append(_state(m) + (m.get_grads(),))
    return m, seen


@pytest.mark.parametrize("name,B,k", FUSED)
def test_fused_appliers_element_by_element(gpu, name, B, k):
    """The fused step's update against float64 on every element, from a preloaded state (v > 0, t = 99 999) and off the default
    hyper-parameters, and bitwise against forward_backward + adam_step (adam_kernel) on a second handle.
    The state is adam_inputs' made plausible (|m| <= sqrt(v)): the parameters are run through the model again in the second step."""
    x, w, _, y = _data(name, B, k, 17)
    _, _, mo, vo = R.adam_inputs(w.size, 400 + B)
    mo, vo = R.plausible_state(mo, vo)
    mr, read = _two_steps(name, x, y, k, w, mo, vo, "fused_read")
    mr.close()
    before = (w, mo, vo)
    for i, ((c, lr), (w1, m1, v1, t1, g)) in enumerate(zip(FUSED_STEPS, read)):
        assert t1 == T_LATE + 1 + i
        assert np.all(np.isfinite(g))
        _check("fused %s B=%d k=%d step %d (case %s)" % (name, B, k, i, c.id), before, g, (w1, m1, v1), t1, lr, c.b1, c.b2, c.eps, 1.0)
        before = (w1, m1, v1)
    ms, split = _two_steps(name, x, y, k, w, mo, vo, "split")
    ms.close()
    for i, (a, b) in enumerate(zip(read, split)):
        for what, p, q in zip(("parameters", "first moments", "second moments", "step count", "gradient"), a, b):
            np.testing.assert_array_equal(p, q, err_msg="%s after step %d, fused vs forward_backward + adam_step" % (what, i))
    mf, last = _two_steps(name, x, y, k, w, mo, vo, "fused")
    for what, p, q in zip(("parameters", "first moments", "second moments", "step count", "gradient"), read[-1], last[0]):
        np.testing.assert_array_equal(p, q, err_msg="%s after two steps, read in between vs back to back" % what)
    if name in ("2L-200,100/100,50/784", "cond-prior-200/100/784", "37/5/53"):
        xs, _, eps, ys = _data(name, 5, 3, 43)
        _forward_on_fresh_handle_is_bitwise(mf, name, xs, eps, ys)
    mf.close()


# ---- what belongs with it -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,k", [("37/5/53", 5, 3), ("200/100/784", 20, 5)])
def test_checkpoint_round_trip_under_non_default_hyper_parameters(gpu, name, B, k):
    """get_params + get_adam_state are the whole checkpoint EXCEPT the hyper-parameters (iwae_set_adam is per handle and not saved):
    a new handle given both and the same set_adam continues bitwise; one left at the default hyper-parameters does not."""
    c, lr = R.CASE["D"], 1e-3
    x, w, _, _ = _data(name, B, k, 19)

    def steps(m, first):
        for s in range(first, first + 3):
            m.set_step(s, 0)
            m.train_step(x, k, 1.0, lr, "iwae_elbo", scalars=False)

    a = _make(name)
    a.set_params(w)
    a.set_adam(c.b1, c.b2, c.eps)
    steps(a, 0)
    wa, ma, va, ta = _state(a)
    assert ta == 3
    b, d = _make(name), _make(name)
    for h in (b, d):
        h.set_params(wa)
        h.set_adam_state(ma, va, ta)
    b.set_adam(c.b1, c.b2, c.eps)
    for h in (a, b, d):
        steps(h, 3)
    sa, sb, sd = _state(a), _state(b), _state(d)
    for what, p, q in zip(("parameters", "first moments", "second moments", "step count"), sa, sb):
        np.testing.assert_array_equal(p, q, err_msg=what)
    assert sd[3] == 6 and np.any(sd[0] != sa[0])
    for h in (a, b, d):
        h.close()


@pytest.mark.parametrize("script", ["keras_defaults_and_assign", "swap_optimizer"])
def test_shim_optimizer_reaches_the_device(gpu, script):
    """IWAE.train_step with optimizers.Adam objects equals NativeModel + set_adam bitwise over two steps: Adam(1e-3) carries Keras's
    epsilon 1e-7 (not the reference's 1e-4) to the device, learning_rate.assign between the steps is honoured, and so is a second
    optimizer object with other hyper-parameters."""
    from iwae_amd import iwae1
    from iwae_amd.native import NativeModel
    from iwae_amd.optimizers import Adam
    from oracle import iwae_np as O
    x = O.synthetic_binarized(20, 7)
    if script == "keras_defaults_and_assign":
        o = Adam(1e-3)
        plan = [(o, None, (0.9, 0.999, 1e-7), 1e-3), (o, 5e-4, (0.9, 0.999, 1e-7), 5e-4)]
    else:
        plan = [(Adam(1e-2, beta_1=0.5, beta_2=0.9, epsilon=1e-7), None, (0.5, 0.9, 1e-7), 1e-2), (Adam(1e-3, epsilon=1e-4), None, (0.9, 0.999, 1e-4), 1e-3)]
    model = iwae1.IWAE(200, 100, seed=SEED)
    net = NativeModel(1, 200, 100, seed=SEED)
    np.testing.assert_array_equal(model._net.get_params(), net.get_params())
    for opt, assign, hyper, lr in plan:
        if assign is not None:
            opt.learning_rate.assign(assign)
        model.train_step(x, 5, 1.0, opt, objective="iwae_elbo")
        net.set_adam(*hyper)
        net.train_step(x, 5, 1.0, lr, "iwae_elbo", scalars=False)
    for what, p, q in zip(("parameters", "first moments", "second moments", "step count"), _state(model._net), _state(net)):
        np.testing.assert_array_equal(p, q, err_msg=what)
    assert _state(net)[3] == 2
    # ... and the hyper-parameters did matter: the same two steps at the device's defaults land elsewhere
    ref = NativeModel(1, 200, 100, seed=SEED)
    for _, _, _, lr in plan:
        ref.train_step(x, 5, 1.0, lr, "iwae_elbo", scalars=False)
    assert np.any(ref.get_params() != net.get_params())
    for h in (net, ref):
        h.close()


def test_rejected_arguments_change_nothing(gpu):
    """set_adam with beta = 1, a negative beta, epsilon = 0 or a NaN, set_adam_state with a wrong length or a negative step: an error, and
    parameters, state, t AND the hyper-parameters set before stay as they were -- a valid step afterwards passes the element check at them."""
    c = R.CASE["D"]
    m = _make("37/5/53")
    n = m.n_params
    w, g, mo, vo = R.adam_inputs(n, 500)
    m.set_params(w)
    m.set_adam_state(mo, vo, c.t0)
    m.set_adam(c.b1, c.b2, c.eps)
    nan = float("nan")
    for bad in ((1.0, 0.999, 1e-4), (0.9, 1.0, 1e-4), (-0.1, 0.999, 1e-4), (0.9, -1e-3, 1e-4), (0.9, 0.999, 0.0), (0.9, 0.999, -1e-4),
                (nan, 0.999, 1e-4), (0.9, nan, 1e-4), (0.9, 0.999, nan)):
        with pytest.raises(ValueError):
            m.set_adam(*bad)
    with pytest.raises(ValueError):
        m.set_adam_state(np.zeros(n - 1, dtype=np.float32), np.ones(n - 1, dtype=np.float32), 3)
    with pytest.raises(ValueError):
        m.set_adam_state(np.zeros(n + 1, dtype=np.float32), np.ones(n + 1, dtype=np.float32), 3)
    with pytest.raises(ValueError):
        m.set_adam_state(np.zeros(n, dtype=np.float32), np.ones(n, dtype=np.float32), -1)
    w0, m0, v0, t0 = _state(m)
    np.testing.assert_array_equal(w0.view(np.uint32), w.view(np.uint32))
    np.testing.assert_array_equal(m0.view(np.uint32), mo.view(np.uint32))
    np.testing.assert_array_equal(v0.view(np.uint32), vo.view(np.uint32))
    assert t0 == c.t0
    _inject(m, g)
    m.adam_step(c.lr, c.gscale)
    w1, m1, v1, t1 = _state(m)
    assert t1 == c.t0 + 1
    _check("after rejected calls, case D", (w, mo, vo), g, (w1, m1, v1), t1, c.lr, c.b1, c.b2, c.eps, c.gscale)
    m.close()
