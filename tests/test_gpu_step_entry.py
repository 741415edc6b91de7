"""The null-mask path of the masked entry points (iwae_forward_masked / iwae_forward_backward_masked / iwae_train_step_masked with mask = NULL,
include/iwae_amd.h): the unmasked call, handed on before the masked scope check.  iwae_amd/native.py never passes a null mask, so the calls go
through the C ABI directly, on a handle and its twin (same seed, same noise step) that takes iwae_forward / iwae_forward_backward /
iwae_train_step: scalars, log_w, the gradient, and the parameters and Adam state after two train steps (the first hands out a tensor and ends
in a separate Adam pass, the second takes the fused update) are bitwise equal.  The 2-layer handles are ones the masked scope refuses: a null
mask never reaches it.
"""
import ctypes as C

import numpy as np
import pytest

from iwae_amd._capi import OBJECTIVES, Scalars, check

pytestmark = pytest.mark.gpu

B, K, XD = 5, 3, 48
MODELS = {"1layer": (1, [64], [8]), "2layer": (2, [64, 32], [8, 4])}
SCALARS = ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14", "inference_loss", "mean_lpxz", "mean_lpz", "mean_lqzx", "mean_kl")


def _calls(m, x, null_mask):
    """forward, forward_backward and two train steps through the C ABI -- the masked entry points with mask = NULL, or the unmasked ones --
    and every array they leave."""
    out = {}
    obj = OBJECTIVES["iwae_elbo"]

    def call(tag, name, tail, want):
        t, bufs = m._want(want, B, K)
        s = Scalars()
        tp = C.byref(t) if t is not None else None
        if null_mask:
            check(getattr(m.lib, name + "_masked")(m.h, x.ctypes.data, None, B, K, *tail, None, C.byref(s), tp))
        else:
            check(getattr(m.lib, name)(m.h, x.ctypes.data, B, K, *tail, None, C.byref(s), tp))
        out[tag + ".scalars"] = np.array([getattr(s, n) for n in SCALARS], np.float32)
        for n, a in bufs.items():
            out["%s.%s" % (tag, n)] = a

    m.set_step(7, 3)
    call("forward", "iwae_forward", (1.0,), ("log_w",))
    call("forward_backward", "iwae_forward_backward", (1.0, obj), ("log_w",))
    out["forward_backward.grads"] = m.get_grads().copy()
    call("train_step.0", "iwae_train_step", (1.0, 1e-3, obj), ("log_w",))
    call("train_step.1", "iwae_train_step", (1.0, 1e-3, obj), ())
    out["train_step.params"] = m.get_params().copy()
    out["train_step.adam_m"], out["train_step.adam_v"], t = m.get_adam_state()
    out["train_step.adam_t"] = np.array(t)
    return out


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_null_mask_is_the_unmasked_call(model, precision):
    from iwae_amd.native import NativeModel
    layers, nh, nl = MODELS[model]
    x = (np.random.default_rng(11).random((B, XD)) < 0.4).astype(np.float32)
    got, ref = (_run(NativeModel(layers, nh, nl, x_dim=XD, seed=123, precision=precision), x, null_mask) for null_mask in (True, False))
    assert sorted(got) == sorted(ref)
    for name in sorted(ref):
        assert np.all(np.isfinite(ref[name])), name
        assert np.array_equal(got[name], ref[name]), name
    assert np.any(ref["forward_backward.grads"] != 0.0) and np.any(ref["train_step.adam_v"] != 0.0)      # (the calls did their work)
    assert int(ref["train_step.adam_t"]) == 2


def _run(m, x, null_mask):
    try:
        return _calls(m, x, null_mask)
    finally:
        m.close()
