"""The case table of the sample-axis parity tests (test_sample_axis_host.py on the CPU, test_gpu_sample_axis.py on the GPU).

The other GPU modules walk the feature widths and the row-count families; here the widths stay at the reference's -- (200, 100, 784) for
the 1-layer model, ([200, 100], [100, 50], 784) for the 2-layer model -- and the sample count k walks every value at which the code
changes path, as a TRAINING step whose gradients are compared with the oracle.  The parameters are spread_params of the seeded random
initialisation (tests/_parity_common.py) unless a case says init = "random": at random initialisation one sample per image has ~all
the weight over k (median ESS/k = 1/k), and the gradient says nothing about the other k - 1 samples.

Each case's comment names the branch it cuts (file and predicate).  test_sample_axis_host.py holds every case to the admissibility
conditions from the oracle alone and prints its figures (median ESS/k, max al, worst per-tensor relative difference of the rounding-aware
oracle's gradient against the exact oracle's: 0.39 .. 0.81, <= 0.64 and 0.0039 .. 0.0094 over this table).  If a new case misses one, change
its seed, never a bound, and record the oracle-only figures in its comment (as the (1200, 7) case does).
"""
import collections
import functools

import numpy as np

from oracle import iwae_np as O, philox_np
import make_golden as MG
from _parity_common import spread_params

SEED = 123            # the handles' noise seed (philox_np.device_eps restates the device stream for it)
NOISE_STEP = 9        # the device-noise cases: iwae_set_step(NOISE_STEP, 0) before the call
W1 = (200, 100, 784)
W2 = ([200, 100], [100, 50], 784)

Case = collections.namedtuple("Case", "layers B k obj beta init noise seed head")


def case(B, k, obj="iwae_elbo", beta=1.0, layers=1, init="spread", noise="host", seed=None, head=0.1):
    """seed: of make_golden.inputs; by default a function of the shape alone, so the cases of one shape share inputs.  head: spread_params'
    scale of the Gaussian heads."""
    return Case(layers, B, k, obj, beta, init, noise, 7000 + 13 * B + k if seed is None else seed, head)


def case_id(c):
    return "%dL-B%d-k%d-%s%s%s" % (c.layers, c.B, c.k, c.obj, "" if c.init == "spread" else "-" + c.init, "" if c.noise == "host" else "-devnoise")


# ---------------------------------------------------------------- 1-layer, bf16, spread weights, host draws
BF16_1L = [
    # -- few rows, M <= 1 024: the log-sum-exp sits inside dec_bwd_rows_kernel (kernels.hip, `lse_on`; plan LSE_BWD_ROWS), a wave per image
    #    in front of every 16-row workgroup
    case(1, 1, "vae_elbo"),                  # B = 1, M = 1: one workgroup in every per-image kernel, invB = 1
    case(1, 1, "iwae_elbo"),                 # the same through the softmax (al = 1)
    case(1, 65, "iwae_elbo"),                # one image over five 16-row workgroups, each recomputing it; lse_image `single = k <= 64` false: second pass
    case(7, 16, "iwae_elbo"),                # plan_step `lat_fuse` (step_bf16.hip: k <= 16): latent_image_part fused into block_bwd_kernel
    case(7, 17, "iwae_elbo"),                # ... and one past it: latent_bwd_kernel on its own
    case(3, 63, "iwae_eq14"),                # lse_image `single`: the last lane idle
    case(3, 64, "dreg"),                     # lse_image `single`: every lane holds a sample
    case(3, 65, "iwae_elbo"),                # lse_image: one sample in the second pass; latent_bwd_kernel's outer loop (UN * SG = 64) enters its second iteration, clamped tail
    case(3, 70, "dreg"),                     # the negative control's shape (test_sample_axis_host.py)
    case(5, 129, "vae_elbo_kl", 0.7),        # lse_image: three passes over a.logw, beta != 1
    case(3, 257, "iwae_elbo"),               # M = 771 <= 1 024: a WAVE walks 257 samples (launch_lse's block kernels are not used inside dec_bwd_rows_kernel)
    # -- 1 025 .. 4 096 rows: the separate launch_lse (row_kernels.hip: lse_block_kernel<4> for k > 256, <16> for k >= 2 048) in a training
    #    step -- the BlockRed reductions through the softmax, gx, cf, eq14 and DReG passes
    case(5, 256, "iwae_eq14"),               # launch_lse `k > 256` false: the last k of lse_kernel, a wave in four full passes
    case(5, 257, "iwae_elbo"),               # launch_lse `k > 256`: lse_block_kernel<4>
    case(4, 300, "dreg"),                    # lse_block_kernel<4>, the DReG pass
    case(1, 2047, "iwae_elbo"),              # B = 1, launch_lse `k >= 2048` false: still <4>
    case(2, 2048, "iwae_elbo"),              # launch_lse `k >= 2048`: lse_block_kernel<16>; the block-kernel decoder
    # -- 4 097 .. 8 191 rows
    case(3, 2048, "dreg"),                   # lse_block_kernel<16>, the DReG pass, the middle row-count family
    case(90, 65, "iwae_elbo"),               # 5 850 rows: lse_kernel at k > 64 in the middle family
    # -- >= 8 192 rows: the pipelined decoder (bern_pipe_kernel), z made in its prologue
    case(127, 65, "iwae_elbo"),              # lse_kernel behind the decoder kernel (bern_lse_ok: k does not divide 200) at k > 64: second pass; second outer iteration of latent_bwd_kernel
    case(127, 65, "dreg"),
    case(130, 64, "iwae_eq14"),              # lse_kernel, lse_image `single` with every lane holding a sample, behind the pipelined decoder
    case(265, 31, "iwae_elbo"),              # bern_pipe_ok (kernels.hip: (126 + k) / k + 1 <= BERN_XIMG_MAX needs k >= 32): falls back to dense_kernel<EPI_BERN>
    case(257, 32, "iwae_elbo"),              # ... the first k the pipelined kernel takes
    case(9, 1000, "iwae_elbo"),              # lse_block_kernel<4> behind the pipelined decoder
    case(5, 2048, "iwae_elbo"),              # lse_block_kernel<16>; every row of a workgroup belongs to one image
    case(170, 50, "iwae_elbo"),              # the headline shapes of the other modules, now with spread weights; k divides 200: with the 200-row shape (bern_qw_force) lse_image runs INSIDE the decoder kernel (bern_lse_ok)
    case(170, 50, "dreg"),
    case(340, 25, "iwae_eq14"),
]
# the >= 8 192-row cases with k >= 32 run a second time with options={"bern_qw_force": 1}
BF16_1L_QW = [c for c in BF16_1L if c.B * c.k >= 8192 and c.k >= 32]

# at random initialisation (the inputs of the other modules): the one-hot regime exercises the m = max path with exp underflow in the other lanes
BF16_1L_RANDOM = [case(3, 65, init="random"), case(5, 257, init="random"), case(127, 65, init="random")]

# ---------------------------------------------------------------- float32 mode (precision="fp32", exact oracle)
F32_1L = [
    case(1, 1), case(3, 65), case(5, 257), case(2, 2048), case(90, 65),
    # without `logits`: the one-launch float32 decoder's (dec_fwd_f32_kernel: forward-only calls, and the training step with option
    # f32_dec_fused_train) 16-row tiles hold 3 or 4 images each -- both sides of `x_in_lds = nimg <= 3` (fp32_kernels.hip) in one launch.  max al is here the largest of 7 weights over 1 200 images, an extreme value: with the heads scaled by 0.1 it is
    # 0.78 .. 0.91 at every one of 41 seeds tried (median ESS/k 0.64 .. 0.69) -- no seed admits the case, so its heads are scaled by 0.05
    # (oracle: median ESS/k 0.805, max al 0.619)
    case(1200, 7, head=0.05),
]

# ---------------------------------------------------------------- the 2-layer model
L2_BOTH = [case(1, 65, layers=2), case(7, 17, layers=2), case(3, 70, layers=2), case(3, 70, "vae_elbo", layers=2), case(5, 257, layers=2)]
L2_BF16_ONLY = [case(127, 65, layers=2)]      # 8 255 rows: the chain kernels (chain2_fwd_kernel / gblock_bwd) and the one-launch decoder

# ---------------------------------------------------------------- the device's own draws (iwae_set_step(NOISE_STEP, 0), no eps)
NOISE_1L = [case(3, 65, noise="device"), case(127, 65, "dreg", noise="device")]

ALL = BF16_1L + BF16_1L_RANDOM + F32_1L + L2_BOTH + L2_BF16_ONLY + NOISE_1L
UNIQUE = list(dict.fromkeys(ALL))      # (the float32 list repeats bf16 cases)


# ---------------------------------------------------------------- inputs and the oracle, computed once per case
@functools.lru_cache(maxsize=4)
def inputs(c):
    """(x, P, eps) of a case: make_golden.inputs at the case's seed, spread_params unless init = "random", and for noise = "device" the
    NumPy restatement of the device's Philox draws at NOISE_STEP."""
    nh, nl, xd = W1 if c.layers == 1 else W2
    x, P, eps = MG.inputs(c.layers, nh, nl, xd, c.B, c.k if c.noise == "host" else 1, c.seed)
    if c.init == "spread":
        P = spread_params(P, c.layers, head=c.head)
    if c.noise == "device":
        if c.layers == 1:
            eps = philox_np.device_eps(SEED, NOISE_STEP, c.B, c.k, nl)
        else:
            eps = tuple(philox_np.device_eps(SEED, NOISE_STEP, c.B, c.k, nl[l], stream=l) for l in range(2))
    return x, P, eps


@functools.lru_cache(maxsize=6)
def oracle(c, emu):
    """(res, grads) of the oracle's step for a case (emu: with the bf16 rounding points).  The [k, B, 784] logits are dropped from res:
    no test of these modules reads them, and at 10 240 rows they are 64 MB a call."""
    x, P, eps = inputs(c)
    rnd = O.bf16_round if emu else None
    if c.layers == 1:
        res, g = O.loss_grads_1layer(P, x, eps, c.beta, c.obj, rnd=rnd)
    else:
        res, g = O.loss_grads_2layer(P, x, eps[0], eps[1], 1.0, c.obj, rnd=rnd)
    res = {key: v for key, v in res.items() if key != "logits"}
    return res, g


def log_w_of(c, res):
    """The oracle's log_w [k, B] from its rows (iwae1.py:113, iwae2.py:128)."""
    if c.layers == 1:
        return res["lpxz"] + c.beta * (res["lpz"] - res["lqzx"])
    return res["lpxz1"] + res["lpz1z2"] + res["lpz2"] - res["lqz1x"] - res["lqz2z1"]
