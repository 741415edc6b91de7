"""Admissibility of the sample-axis cases (tests/_sample_axis_cases.py) from the oracle alone -- no GPU.

The conditions are on the INPUTS, not measurements of the device:
  * the importance weights over k are spread: median over images of ESS/k >= 0.10 and max al <= 0.7 (k = 1 and the cases that are at
    random initialisation on purpose excepted);
  * the comparison is well conditioned: per gradient tensor the rounding-aware oracle differs from the exact oracle by <= EMU_GRAD_REL
    (the device is held to that bound against the rounding-aware oracle; an input on which one bf16 rounding moves the gradient by more
    says nothing about a kernel);
  * a negative control: a device that dropped the samples s >= 64 of every image would be caught with spread weights, by the al check
    and by the gradient comparison -- and would NOT be caught by the gradient comparison at random initialisation, which is why the
    spread parameters exist.

Every test prints its figures next to their bounds (pytest -rP shows them)."""
import numpy as np
import pytest

from oracle import iwae_np as O
import _sample_axis_cases as C
from _parity_common import EMU_GRAD_REL, al_excess, ess_fraction, softmax_over_k

ESS_MIN, AL_MAX = 0.10, 0.7


def _rel(g_a, g_b):
    return [float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)) for pa, pb in zip(g_a, g_b) for a, b in zip(pa, pb)]


@pytest.mark.parametrize("c", C.UNIQUE, ids=C.case_id)
def test_case_is_admissible(c):
    res_x, g_x = C.oracle(c, False)
    res_e, g_e = C.oracle(c, True)
    ess = float(np.median(ess_fraction(res_x["al"])))
    top = float(np.max(res_x["al"]))
    cond = max(_rel(g_e, g_x))
    bound = EMU_GRAD_REL
    print("%s: median ESS/k %.3g (>= %.2f), max al %.3g (<= %.1f), rounding-aware vs exact gradient %.3g (<= %.3g)"
          % (C.case_id(c), ess, ESS_MIN, top, AL_MAX, cond, bound))
    np.testing.assert_allclose(softmax_over_k(C.log_w_of(c, res_x)), res_x["al"], rtol=1e-12, atol=1e-300)
    if c.init == "random":
        return      # the one-hot regime on purpose; its gradient is held against the rounding-aware oracle on the device only
    if c.k > 1:
        assert ess >= ESS_MIN and top <= AL_MAX, (ess, top)
    assert cond <= bound, _rel(g_e, g_x)


def _drop_from_64(c):
    """What a device that lost the samples s >= 64 of every image would give: al from the oracle's own log_w with those weights zeroed
    and the rest renormalised, and the iwae_elbo gradient that goes with it -- G = -al / B on the first 64 samples and 0 beyond, which is
    the oracle's gradient on the first 64 draws alone.  Returns (al check figure, worst per-tensor gradient shift)."""
    x, P, eps = C.inputs(c)
    res, g = C.oracle(c, True)
    al = softmax_over_k(C.log_w_of(c, res))
    al[64:] = 0.0
    al /= al.sum(axis=0, keepdims=True)
    _, g_cut = O.loss_grads_1layer(P, x, eps[:64], c.beta, "iwae_elbo", rnd=O.bf16_round)
    return al_excess(al, C.log_w_of(c, res)), max(_rel(g_cut, g))


def test_negative_control_dropping_samples_beyond_64():
    spread, random = C.case(3, 70, "iwae_elbo"), C.case(3, 70, "iwae_elbo", init="random")
    a_s, g_s = _drop_from_64(spread)
    a_r, g_r = _drop_from_64(random)
    print("samples s >= 64 dropped at (3, 70): spread al check %.3g x its bound, gradient shift %.3g; random init al check %.3g x, "
          "gradient shift %.3g; gradient bound %.3g" % (a_s, g_s, a_r, g_r, EMU_GRAD_REL))
    assert a_s > 100.0, a_s                  # the al check fails by a wide margin
    assert g_s > EMU_GRAD_REL, g_s           # and some tensor of the iwae_elbo gradient moves by more than its bound
    assert g_r <= EMU_GRAD_REL, g_r          # at random initialisation no tensor does: the gradient comparison is blind to it
