"""The evaluation calls share one input workspace on the handle (iwae_model::EvalWs in csrc/model.h: the uploaded images, their bf16 rows and
the float32 encoder heads).  Nothing in it is read after the call that filled it, so a call must give bit for bit what it gives alone on a
fresh handle, whatever ran before it on the same handle.  The sizes below rise and fall, so the shared buffers regrow (N = 37 -> 64) and are
reused while larger than the call needs (N = 5, 3, 7 behind 37; N = 3 behind 64).

Every expected value comes from a fresh handle with the same parameters, noise step, batch offset and (train step) Adam state; the
comparison is bitwise (array bytes), no tolerance.
"""
import numpy as np
import pytest

from oracle import iwae_np as O
import make_golden as MG

pytestmark = pytest.mark.gpu

SMALL2 = ([64, 32], [16, 8], 48)        # the small 2-layer model of tests/test_gpu_latent_activity.py: the composed activity path


def _fresh(layers, nh, nl, xd, params, prec):
    from iwae_amd.native import NativeModel
    m = NativeModel(layers, nh, nl, x_dim=xd, seed=123)
    m.set_params(params)
    m.set_eval_precision(prec)
    return m


def _same(a, b, where):
    """Bitwise equality of two results of the Python layer (dicts, sequences, arrays, scalars)."""
    if isinstance(a, dict):
        assert set(a) == set(b), where
        for key in a:
            _same(a[key], b[key], "%s[%r]" % (where, key))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (u, v) in enumerate(zip(a, b)):
            _same(u, v, "%s[%d]" % (where, i))
    else:
        u, v = np.asarray(a), np.asarray(b)
        assert u.dtype == v.dtype and u.shape == v.shape, where
        assert u.tobytes() == v.tobytes(), "%s: %d of %d elements differ" % (where, int(np.sum(u != v)), u.size)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_calls_in_sequence_equal_calls_alone(gpu, prec):
    nh, nl, xd = 64, 2, 48
    x, P, _ = MG.inputs(1, nh, nl, xd, 64, 1, 31)
    params = O.flatten_params(P)
    rng = np.random.default_rng(5)
    z = rng.uniform(-3.0, 3.0, (1500, nl)).astype(np.float32)
    lw = rng.uniform(-1.0, 0.0, 1500).astype(np.float32)

    def state(m):
        mo, ve, t = m.get_adam_state()
        return {"params": m.get_params(), "mom": mo, "vel": ve, "t": t}

    # (name, noise step, batch offset, the call)
    calls = [
        ("grid N=37", 11, 0, lambda m: m.grid_posterior(x[:37], z, lw, log_joint=True)),
        ("aggregate N=5 S=3", 12, 3, lambda m: m.aggregate_posterior(x[:5], n_samples=3, per_sample=True)),
        ("ais encoder", 13, 5, lambda m: m.ais(x[:3], n_chains=7, n_temps=4, leapfrog=2, init="encoder", trace=True)),
        ("ais prior", 14, 5, lambda m: m.ais(x[:3], n_chains=7, n_temps=4, leapfrog=2, init="prior", trace=True)),
        ("activity N=64", 15, 0, lambda m: m.latent_activity(x, per_image=True)),
        ("eval_llh N=7 k=50", 16, 2, lambda m: m.eval_llh(x[:7], k=50, per_image=True)),
        ("train B=8 k=5", 17, 0, lambda m: m.train_step(x[:8], 5)),
        ("grid N=3", 18, 0, lambda m: m.grid_posterior(x[:3], z, lw, log_joint=True)),
    ]
    # each call alone on a fresh handle (the train step from the initial Adam state; the last grid call on the trained parameters)
    want, trained = [], None
    for name, step, offset, call in calls:
        alone = _fresh(1, nh, nl, xd, params if trained is None else trained["params"], prec)
        alone.set_step(step, offset)
        want.append(call(alone))
        if name.startswith("train"):
            trained = state(alone)
        alone.close()
    # ... and one behind the other on one handle, nothing read back in between: the train step's deferred decoder update is still on
    # the side stream when the last grid call begins
    shared = _fresh(1, nh, nl, xd, params, prec)
    for (name, step, offset, call), w in zip(calls, want):
        shared.set_step(step, offset)
        _same(call(shared), w, "%s (%s)" % (name, prec))
    _same(state(shared), trained, "state behind the train step (%s)" % prec)
    shared.close()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_two_layer_activity_between_evaluations(gpu, prec):
    """The composed 2-layer activity path keeps its own z1 rows and q(z2|z1) activations live beside the shared heads."""
    nh, nl, xd = SMALL2
    x, P, _ = MG.inputs(2, nh, nl, xd, 7, 1, 33)
    params = O.flatten_params(P)
    calls = [
        ("eval_llh before", 21, 0, lambda m: m.eval_llh(x, k=50, per_image=True)),
        ("activity N=5 k=200", 22, 1, lambda m: m.latent_activity(x[:5], k=200, per_image=True)),
        ("eval_llh after", 23, 0, lambda m: m.eval_llh(x, k=50, per_image=True)),
    ]
    shared = _fresh(2, nh, nl, xd, params, prec)
    for name, step, offset, call in calls:
        alone = _fresh(2, nh, nl, xd, params, prec)
        alone.set_step(step, offset)
        want = call(alone)
        alone.close()
        shared.set_step(step, offset)
        _same(call(shared), want, "%s (%s)" % (name, prec))
    shared.close()
