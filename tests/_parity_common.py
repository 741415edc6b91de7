"""Shared by the GPU parity modules (test_gpu_parity.py, test_gpu_ragged_widths.py, test_gpu_sample_axis.py) and the host module
test_sample_axis_host.py: the tolerance constants, the helpers that compare the device's flat gradient with the oracle's tensors and
its per-row densities with the oracle at the DEVICE's own heads, and the inputs / checks of the sample axis (spread_params,
ess_fraction, softmax_over_k, al_excess).

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
    Nothing is pushed to an extreme: no logit saturates and sigma ~ 1 stays far from its floor."""
    out = [(np.array(W, dtype=np.float64), np.array(b, dtype=np.float64)) for W, b in P]
    heads, dec = ((2, 3), 4) if layers == 1 else ((2, 3, 6, 7, 10, 11), 12)
    for i in heads:
        out[i] = (out[i][0] * head, out[i][1] * head)
    out[dec] = (out[dec][0] * dec_in, out[dec][1])
    return out


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
