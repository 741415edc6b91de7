"""tests/_masked_ref.py -- the float64 restatement the GPU tests of the masked train step compare against -- checked on the host against
the committed oracles, so that what the device is held to is itself held to something:
  1. with a mask of ones it IS the torch oracle's unmasked step (1e-10);
  2. with real per-image masks it equals the NumPy oracle applied image by image to models that have lost their unobserved input rows and
     output columns (1e-9; the identity holds to ~5e-15 in float64);
  3. NaN at the unobserved pixels changes nothing, bitwise;
  4. negative control: the unmasked gradient is far from the masked one, so the cases see the mask.
"""
import numpy as np
import pytest

from oracle import iwae_np as O
import make_golden as MG
import _masked_ref as MR
from _parity_common import F32_GRAD_REL, spread_params

NH, NL, XD, B, K = 16, 4, 48, 5, 7


def _inputs():
    x, P, eps = MG.inputs(1, NH, NL, XD, B, K, 4242)
    P = spread_params(P, 1)
    mask = MR.case_mask(B, XD, 5)
    return x, P, eps, mask


def _rel(a, b):
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


@pytest.mark.parametrize("obj,beta", [("iwae_elbo", 1.0), ("vae_elbo", 1.0), ("dreg", 1.0), ("vae_elbo_kl", 0.7), ("iwae_eq14", 1.0)])
def test_mask_of_ones_is_the_unmasked_oracle(obj, beta):
    x, P, eps, _ = _inputs()
    res, g = O.loss_grads_1layer(P, x, eps, beta, obj)
    mres, mg = MR.masked_loss_grads(P, x, np.ones((B, XD), np.uint8), eps, beta, obj)
    for key in ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14"):
        assert abs(mres[key] - res[key]) <= 1e-10 * max(1.0, abs(res[key])), key
    for key in ("lpxz", "lpz", "lqzx", "al", "z"):
        np.testing.assert_allclose(mres[key], res[key], rtol=1e-10, atol=1e-10, err_msg=key)
    for (dW, db), (rW, rb) in zip(mg, g):
        assert _rel(dW, rW) < 1e-10 and _rel(db, rb) < 1e-10


@pytest.mark.parametrize("obj", MR.OBJECTIVES)
def test_masked_step_is_the_oracle_on_sliced_models(obj):
    x, P, eps, mask = _inputs()
    mask = mask.copy()
    assert not mask[0].any() and mask[1].sum() == 1 and mask[B - 1].all() and 0 < mask[2].sum() < XD
    mask[0, 3] = 1          # (the NumPy oracle cannot take an image of zero pixels: a zero-width reshape fails)
    sres, sg = MR.sliced_oracle_grads(P, x, mask, eps, 1.0, obj)
    mres, mg = MR.masked_loss_grads(P, x, mask, eps, 1.0, obj)
    key = "iwae_elbo" if obj == "dreg" else obj
    assert abs(mres[key] - sres["value"]) <= 1e-9 * max(1.0, abs(sres["value"]))
    np.testing.assert_allclose(mres["lpxz"], sres["lpxz"], rtol=1e-9, atol=1e-9)
    for i, ((dW, db), (rW, rb)) in enumerate(zip(mg, sg)):
        assert _rel(dW, rW) < 1e-9 and _rel(db, rb) < 1e-9, (i, _rel(dW, rW), _rel(db, rb))


@pytest.mark.parametrize("obj", MR.OBJECTIVES)
def test_nan_at_unobserved_pixels_changes_nothing(obj):
    x, P, eps, mask = _inputs()
    xn = np.where(mask != 0, x, np.nan)
    assert np.isnan(xn).any()
    a, ga = MR.masked_loss_grads(P, x, mask, eps, 1.0, obj)
    b, gb = MR.masked_loss_grads(P, xn, mask, eps, 1.0, obj)
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    for (dW, db), (rW, rb) in zip(ga, gb):
        np.testing.assert_array_equal(dW, rW)
        np.testing.assert_array_equal(db, rb)
    # an image with nothing observed: log p(x_obs|z) = 0 exactly, log_w = log p(z) - log q(z|x)
    assert np.all(a["lpxz"][:, 0] == 0.0)
    np.testing.assert_array_equal(a["log_w"][:, 0], (a["lpz"] - a["lqzx"])[:, 0])


@pytest.mark.parametrize("obj", MR.OBJECTIVES)
def test_unmasked_gradient_is_far_from_the_masked_one(obj):
    x, P, eps, mask = _inputs()
    _, g = O.loss_grads_1layer(P, x, eps, 1.0, obj)
    _, mg = MR.masked_loss_grads(P, x, mask, eps, 1.0, obj)
    for i, ((dW, db), (rW, rb)) in enumerate(zip(g, mg)):
        assert _rel(dW, rW) > 1e3 * F32_GRAD_REL and _rel(db, rb) > 1e3 * F32_GRAD_REL, (i, _rel(dW, rW), _rel(db, rb))


# ---------------------------------------------------------------- 5. header, binding, build list, options, driver
def test_header_binding_build_and_driver_agree():
    import os
    import re
    import sys
    from iwae_amd import _capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "iwae_amd.h")).read()
    for name, nargs in (("iwae_forward_masked", 9), ("iwae_forward_backward_masked", 10), ("iwae_train_step_masked", 11)):
        decl = re.search(r"int %s\((.*?)\);" % name, header, re.S).group(1)
        assert len(decl.split(",")) == nargs == len(_capi.SYMBOLS[name][1]), name
        assert "const uint8_t* mask" in decl
    assert '"masked_out"' in header and "SELECTED out" in header
    assert "masked_kernels.hip" in _capi._ID_SOURCES
    b = open(os.path.join(root, "iwae_amd", "csrc", "build.sh")).read()
    assert b.count("masked_kernels.hip") >= 2 and b.count("masked_kernels.o") >= 2      # the id list, the compile line and the link line
    readme = open(os.path.join(root, "tools", "README.md")).read()
    assert "no_masked_out_fused" in readme and "masked_out_min_rows" in readme and "dev/masked_step_time.py" in readme
    assert os.path.exists(os.path.join(root, "tools", "dev", "masked_step_time.py"))
    assert "masked_out_f32_kernel" in open(os.path.join(root, "DESIGN.md")).read()
    import main
    sys.path.insert(0, os.path.join(root, "tasks"))
    try:
        import miwae
    finally:
        sys.path.pop(0)
    before = sorted(a.dest for a in main.parser._actions)
    a = miwae.make_parser().parse_args([])
    assert vars(a) == dict(vars(main.parser.parse_args([])), images=10000, test_images=1000, steps=2000, rate=0.5, draws=50, mask_seed=0, lr=1e-3)
    assert sorted(a.dest for a in main.parser._actions) == before      # main.parser is not mutated
