"""Shared by the GPU parity modules (test_gpu_parity.py, test_gpu_ragged_widths.py, test_gpu_sample_axis.py, test_gpu_offinit.py) and the
host modules test_sample_axis_host.py and test_offinit_host.py: the tolerance constants, the helpers that compare the device's flat
gradient with the oracle's tensors and its per-row densities with the oracle at the DEVICE's own heads, the inputs / checks of the sample
axis (spread_params, ess_fraction, softmax_over_k, al_excess) and the parameter constructors off the initialisation (sharp_params,
saturated_params).

Tolerances (the GEMM operands are bf16 with fp32 accumulation, BASELINE.json configs[1]):
  * against the oracle run with the SAME bf16 rounding points ("emu"): per-sample log densities |d| <= 0.03 nat, scalars
    |d| <= 0.02 nat, gradients relative L2 error <= 1e-2 per tensor (differences are single bf16-ulp flips from fp32 summation order);
  * against the exact float64 oracle: scalars |d| <= 0.15 nat at random init where |log_w| ~ 300-450, gradients relative L2 <= 3e-2;
  * float32 mode against the exact float64 oracle: scalars rel 1e-5, gradients rel 1e-4, per-row densities 2e-3.
"""
import numpy as np

from oracle import iwae_np as O

EMU_ROW_ATOL, EMU_SCALAR_ATOL, EMU_GRAD_REL = 0.03, 0.02, 1e-2
EXACT_SCALAR_ATOL, EXACT_GRAD_REL = 0.15, 3e-2
F32_SCALAR_REL, F32_GRAD_REL, F32_ROW_ATOL = 1e-5, 1e-4, 2e-3
# float32 mode on the DEVICE's own noise against the float64 oracle on the host restatement of the same draws (oracle/philox_np.device_eps):
# the figures test_gpu_parity.py::test_float32_mode_with_device_noise_and_dataset_pipeline holds that step to (float32 Box-Muller with fast
# sin / cos / log: eps differs by <= 2e-5), named here so that other modules hold the same step to the same numbers.
F32_DEVNOISE_SCALAR_ATOL, F32_DEVNOISE_GRAD_REL = 2e-2, 2e-3
# The two per-row checks on the sample axis (derived, not measured):
#   log_w against the float64 sum of the device's own rows: three (five) float32 terms of size <= ~600 are 3 ulp ~ 2e-4 -- the 1e-3 the
#   suite already holds reductions recomputed from device rows to;
#   al against the float64 softmax over k of the device's own log_w: v_exp_f32 after the log2(e) product errs by ~6e-8 |log_w - max|
#   relative, <= 2e-6 at a 30-nat spread, the sum adds the same order -- rtol 1e-4 is a margin of 50 that covers k = 2 048 terms; atol 1e-7
#   is below every weight that matters (1/k >= 5e-4) and above a flushed denormal.
LOGW_FROM_ROWS_ATOL = 1e-3
AL_RTOL, AL_ATOL = 1e-4, 1e-7


def _grad_rel_errors(flat, grads):
    out, off = [], 0
    for dW, db in grads:
        for g in (dW, db):
            got = flat[off:off + g.size].reshape(g.shape).astype(np.float64)
            off += g.size
            out.append(np.linalg.norm(got - g) / (np.linalg.norm(g) + 1e-30))
    return out


def _elementwise_ok(flat, grads):
    """|d| <= 3 % of the tensor's largest element, per tensor (a mis-addressed strip shows as a block of wrong columns, not in a norm)."""
    off, worst = 0, 0.0
    for dW, db in grads:
        for t in (dW, db):
            got = flat[off:off + t.size].reshape(t.shape).astype(np.float64)
            off += t.size
            d, top = float(np.max(np.abs(got - t))), float(np.max(np.abs(t)))
            assert d <= 3e-2 * top + 1e-9, (d, top)
            worst = max(worst, d / (top + 1e-30))
    return worst


def spread_params(P, layers, head=0.1, dec_in=0.1):
    """A benign reparametrisation under which the importance weights over the k samples of an image are SPREAD instead of one-hot.

    At random initialisation log_w = log p(x|z) + log p(z) - log q(z|x) differs between two samples of one image by tens of nats (the
    100 latent terms of log p(z) - log q do not cancel, and log p(x|z) follows z), so softmax over k puts ~all weight on one sample
    (median ESS/k = 1/k) and a gradient comparison says nothing about the other k - 1.  Returned is a NEW list in which
      * both tensors (weight and bias) of every Gaussian head's mu layer and log-sigma layer are scaled by `head` -- 1-layer: P[2], P[3];
        2-layer: P[2], P[3], P[6], P[7], P[10], P[11] -- so each q / p is close to N(0, 1) and log p(z) - log q nearly cancels;
      * the WEIGHT of the decoder's first layer is scaled by `dec_in` -- 1-layer: P[4][0]; 2-layer: P[12][0] -- so log p(x|z) varies
        little with z (its bias, and every other tensor, is untouched).
    Nothing is pushed to an extreme: no logit saturates and sigma ~ 1 stays far from its floor.  (sharp_params and saturated_params below
    are the constructors that DO push: a few posterior units down to the sigma floor, and the logits / tanh pre-activations into saturation.)"""
    out = [(np.array(W, dtype=np.float64), np.array(b, dtype=np.float64)) for W, b in P]
    heads, dec = ((2, 3), 4) if layers == 1 else ((2, 3, 6, 7, 10, 11), 12)
    for i in heads:
        out[i] = (out[i][0] * head, out[i][1] * head)
    out[dec] = (out[dec][0] * dec_in, out[dec][1])
    return out


def sharp_units(D, n):
    """The n units of a head of width D that sharp_params sharpens: spread evenly over the width, the first unit and the LAST unit D - 1
    always among them (the last quad of a ragged width is cut: its tail lanes must see a sharp unit too)."""
    if not 2 <= n <= D:
        raise ValueError("sharp_params: %d units do not fit a head of width %d" % (n, D))
    u = [int(round(j * (D - 1) / (n - 1))) for j in range(n)]
    assert len(set(u)) == n and u[-1] == D - 1
    return u


def sharp_params(P, layers, shifts, heads):
    """SHARP posteriors: in every named log-sigma layer (`heads`, indices into P: 3 = q(z|x) / q(z1|x) of either model, 7 = q(z2|z1) of the
    2-layer model) shifts[j] is subtracted from the BIAS of unit sharp_units(D, len(shifts))[j]; everything else is untouched.  Returns a
    NEW list, float64 in and out.  On spread_params the pre-activation a of every unit is ~0 (sigma ~ 1), so the sharpened unit has
    exp(a) ~ exp(-shift): shifts (4.6, 9.2, 12.5, 16) give sigma = exp(a) + 1e-6 of ~1e-2, ~1e-4, ~4.7e-6 and ~1.1e-6 -- the floor is 1 %,
    21 % and 90 % of the last three.  P[11], the head of p(z1|z2), is rejected: log p(z1|z2) divides by sigma_p^2, and at sigma_p ~ 1e-6
    one bf16 rounding of z1 moves a row by ~1e8 nat (oracle: 8e8) -- no comparison in bf16 arithmetic says anything there.

    What this makes visible (sigma = exp(a) + 1e-6: src/iwae1.py:34,42, iwae2.py:43,45) and spread_params cannot:
      * the floor in the forward sigma of every head epilogue: at sigma ~ 1 dropping it moves the worst gradient tensor by 7e-6 and
        iwae_elbo by 4e-6 nat (float64 oracle, (200, 100, 784), B = 5, k = 8) -- 14 times below even float32 mode's gradient bound.  At
        four sharp units it moves the gradient by 0.21 .. 0.54 (DReG: 35) and iwae_elbo by 1.8 .. 2.6 nat;
      * the derivative through exp, da = dsigma * exp(a) = dsigma * (sigma - 1e-6): taken as dsigma * sigma it moves the gradient by
        0.21 .. 0.54 at four sharp units, by ~1e-6 at sigma ~ 1;
      * DReG's second floor (tasks/task02.py:63: sigma + 1e-6 on a sigma that already holds one).
    The comparison stays well conditioned in BOTH arithmetics (tests/test_offinit_host.py holds every case to it): a sharp unit pins z_u
    to mu_u for every sample, so the weights over k stay spread (median ESS/k 0.16 .. 0.45 over the 1-layer cases of tests/_offinit_cases.py
    with four sharp units), the rounding-aware oracle's rows stay within 0.003 .. 0.012 nat of the exact oracle's and its gradient within
    0.0041 .. 0.0072 per tensor.  At k >= 50 four sharp units thin the weights too far (B = 3, k = 70: median ESS/k 0.048): two units,
    shifts (9.2, 13.8), are used there (0.11 .. 0.16; rows within 0.015, gradient within 0.0096)."""
    allowed = (3,) if layers == 1 else (3, 7)
    out = [(np.array(W, dtype=np.float64), np.array(b, dtype=np.float64)) for W, b in P]
    for h in heads:
        if h not in allowed:
            raise ValueError("sharp_params: P[%d] is not a log-sigma layer of an approximate posterior of the %d-layer model" % (h, layers))
        W, b = out[h]
        for u, s in zip(sharp_units(b.size, len(shifts)), shifts):
            b[u] -= float(s)
    return out


def saturated_params(P, layers, out, hidden):
    """SATURATED logits and tanh units: the WEIGHT of the output layer (1-layer: P[6]; 2-layer: P[14]) is multiplied by `out`, the weights
    of the tanh layers of every encoder and decoder network (1-layer: P[0], P[1], P[4], P[5]; 2-layer: P[0], P[1], P[4], P[5], P[8], P[9],
    P[12], P[13]) by `hidden`; biases are untouched.  Returns a NEW list, float64 in and out.

    At (10, 3) on spread_params the largest |logit| is ~17 (50 at (30, 3), mean log p(x|z) -2600) where every other parity case stays
    below ~6, and tanh units sit at |y| >= 0.999: the (x - 1/2) l - |l|/2 - log(1 + e^-|l|) form of the Bernoulli epilogues, the
    copysign(rcp(1 + e) - 1/2, l) form of x - sigmoid(l), and 1 - y^2 at y -> +-1.  NOT an input for a bf16 comparison: the weights over k
    become one-hot and one bf16 rounding of an operand moves the oracle's rows by 0.75 nat (bound 0.03; 3.5 nat at (30, 3)) -- the
    float32-operand oracle stays within 9e-6 (3e-5) of the exact one, so these parameters go through float32 mode and the float32 row
    evaluation only.  The case table (tests/_offinit_cases.py) runs (5, 8): under spread_params (10, 3) leaves NO unit of the decoder's second
    layer at |y| >= 0.999, (5, 8) has 34 % there at max |logit| 16.6 and mean |log p(x|z)| 621.  The same holds for WIDE posteriors (log-sigma bias + 1.5 on every unit: 0.096 nat against 1.7e-6)."""
    res = [(np.array(W, dtype=np.float64), np.array(b, dtype=np.float64)) for W, b in P]
    last, tanh = (6, (0, 1, 4, 5)) if layers == 1 else (14, (0, 1, 4, 5, 8, 9, 12, 13))
    res[last] = (res[last][0] * float(out), res[last][1])
    for i in tanh:
        res[i] = (res[i][0] * float(hidden), res[i][1])
    return res


def ess_fraction(al):
    """Effective sample size over k per image, 1 / (k sum_s al_s^2), for al of shape [k, B]: 1/k when one sample has all the weight,
    1 when the weights are uniform."""
    al = np.asarray(al, dtype=np.float64)
    return 1.0 / (al.shape[0] * np.sum(al * al, axis=0))


def softmax_over_k(log_w):
    """float64 softmax over axis 0 of log_w [k, B] (iwae1.py:128-137)."""
    lw = np.asarray(log_w, dtype=np.float64)
    w = np.exp(lw - lw.max(axis=0, keepdims=True))
    return w / w.sum(axis=0, keepdims=True)


def al_excess(al, log_w):
    """The al check of the sample-axis tests as one figure: max over [k, B] of |al - softmax_k(log_w)| / (AL_ATOL + AL_RTOL softmax);
    the check passes iff the figure is <= 1 (np.testing.assert_allclose(al, softmax, rtol=AL_RTOL, atol=AL_ATOL) restated)."""
    ref = softmax_over_k(log_w)
    return float(np.max(np.abs(np.asarray(al, dtype=np.float64) - ref) / (AL_ATOL + AL_RTOL * ref)))


def _densities_at_device_head(m, P, x, eps, nl):
    """Per-row log p(x|z), log p(z), log q(z|x) of the 1-layer model evaluated by the ORACLE at the DEVICE's own encoder head
    (mu, sigma as float32, iwae_debug_tensor "enc.head") and the given draws: removes the one sensitivity the per-row comparison with
    the pure oracle has -- a bf16 ulp flip of one encoder activation moves an image's mu, hence log p(z) of all its samples -- so the
    usual per-row bound holds for EVERY row (src/iwae1.py:59,105-111)."""
    head = m.debug_tensor("enc.head").astype(np.float64)
    Dp = head.shape[1] // 2
    mu, sig = head[:, :nl], head[:, Dp:Dp + nl]
    z = mu[None] + sig[None] * np.asarray(eps, dtype=np.float64)
    dec = O._MLP3(P[4:7], O.bf16_round)
    lpxz = np.sum(O.bernoulli_log_prob(np.asarray(x, dtype=np.float64)[None], dec.fwd(O.bf16_round(z))), axis=-1)
    lpz = np.sum(O.normal_log_prob(z, 0.0, 1.0), axis=-1)
    lqzx = np.sum(O.normal_log_prob(z, mu[None], sig[None]), axis=-1)
    return {"lpxz": lpxz, "lpz": lpz, "lqzx": lqzx, "mu": mu, "sigma": sig}


def _densities_at_device_heads_2layer(m, eps1, eps2, B, k, nl, P=None, x=None):
    """The 2-layer model's four latent log-densities (src/iwae2.py:118-124) evaluated by the oracle at the DEVICE's own three Gaussian
    heads (float32: "enc.head" on the images, "enc2.head" / "dec2.head" per sample; device rows are image-major, r = b*k + s) and the given
    draws.  A bf16 ulp flip in one hidden activation moves a head, and log p(z1|z2) divides by sigma_p^2: evaluated at the device's heads
    the comparison is free of that and holds per row at float32-level tolerances."""
    def split(name, D):
        h = m.debug_tensor(name).astype(np.float64)
        Dp = h.shape[1] // 2
        return h[:, :D], h[:, Dp:Dp + D]
    km = lambda a: a.reshape(B, k, -1).transpose(1, 0, 2)      # [M, D] image-major -> [k, B, D]
    mu1, sig1 = split("enc.head", nl[0])
    mu2, sig2 = [km(a) for a in split("enc2.head", nl[1])]
    mup, sigp = [km(a) for a in split("dec2.head", nl[0])]
    z1 = mu1[None] + sig1[None] * np.asarray(eps1, dtype=np.float64)
    z2 = mu2 + sig2 * np.asarray(eps2, dtype=np.float64)
    out = {"lpz2": np.sum(O.normal_log_prob(z2, 0.0, 1.0), axis=-1), "lqz2z1": np.sum(O.normal_log_prob(z2, mu2, sig2), axis=-1),
           "lpz1z2": np.sum(O.normal_log_prob(z1, mup, sigp), axis=-1), "lqz1x": np.sum(O.normal_log_prob(z1, mu1[None], sig1[None]), axis=-1)}
    if P is not None:      # log p(x|z1) through the oracle's decoder (the last three layers) at the device's own z1 (src/iwae2.py:96,121)
        dec = O._MLP3(P[-3:], O.bf16_round)
        out["lpxz1"] = np.sum(O.bernoulli_log_prob(np.asarray(x, dtype=np.float64)[None], dec.fwd(O.bf16_round(z1))), axis=-1)
    return out
