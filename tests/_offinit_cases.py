"""The case table of the off-initialisation parity tests (test_offinit_host.py on the CPU, test_gpu_offinit.py on the GPU).

Every other parity module runs at the seeded random initialisation or at spread_params of it, where sigma ~ 1 and |logit| <= ~6: the
`+ 1e-6` of sigma = exp(a) + 1e-6 (src/iwae1.py:34,42, iwae2.py:43,45), the derivative through exp recovered as sigma - 1e-6, DReG's
second floor, and the saturated ends of the Bernoulli and tanh epilogues cannot be seen there.  Here the operations, the oracle and the
bounds are those of the other modules and only the PARAMETERS move: spread_params first, then
  * "sharp": sharp_params -- SHIFTS4 on four units (k < 50) or SHIFTS2 on two (k >= 50: four thin the weights over k too far, median
    ESS/k 0.048 at B = 3, k = 70) of the named posterior heads.  Admissible in BOTH arithmetics at the existing constants;
  * "sat": saturated_params(.., *SAT); "wide": + 1.5 on every bias of the posterior log-sigma layers.  Admissible in float32 mode ONLY:
    one bf16 rounding moves the oracle's rows by 0.75 / 0.096 nat (bound 0.03).
The head of p(z1|z2) is never sharpened (sharp_params rejects it).

test_offinit_host.py holds every case to its admissibility conditions from the oracle alone and prints the figures.  If a new case misses
one, change its seed, the number of sharp units or the scale -- never a bound -- and record the oracle-only figures in its comment.
"""
import collections
import functools

import numpy as np

from oracle import iwae_np as O, philox_np
import make_golden as MG
from _parity_common import sharp_params, saturated_params, spread_params

SEED = 123            # the handles' noise seed
NOISE_STEP = 9        # the device-noise cases: iwae_set_step(NOISE_STEP, 0) before the call
W1 = (200, 100, 784)
W2 = ([200, 100], [100, 50], 784)
WR = (37, 5, 53)      # every width ragged: the last quad of the 5-wide head is cut, and unit 4 is sharp
COND = 10
SHIFTS4, SHIFTS2 = (4.6, 9.2, 12.5, 16.0), (9.2, 13.8)
# (out, hidden) of saturated_params.  (10, 3) reaches max |logit| 18.6 but NO tanh unit of the decoder's second layer at |y| >= 0.999 (spread_params
# scales the decoder's first weight by 0.1, so its hidden units stay small), and (10, 6) has mean |log p(x|z)| 1 218; (5, 8): max |logit| 16.6, 34 % of
# the layer at |y| >= 0.999, mean |log p(x|z)| 621 (1-layer, B = 5, k = 8; 16.3, 35 %, 629 for the 2-layer model)
SAT = (5.0, 8.0)
WIDE = 1.5

Case = collections.namedtuple("Case", "layers widths B k obj beta sharp heads sat wide noise seed cond")


def case(B, k, obj="iwae_elbo", beta=1.0, layers=1, widths=None, sharp=None, heads=None, sat=None, wide=0.0, noise="host", seed=None, cond=0):
    """sharp: number of sharpened units per named head (default 4 below k = 50, 2 from there; 0: none).  heads: default every posterior
    head of the model.  seed: of make_golden.inputs; by default a function of the shape alone, so the cases of one shape share inputs."""
    if widths is None:
        widths = W1 if layers == 1 else (tuple(W2[0]), tuple(W2[1]), W2[2])
    if sharp is None:
        sharp = 4 if k < 50 else 2
    if heads is None:
        heads = (3,) if layers == 1 else (3, 7)
    return Case(layers, widths, B, k, obj, beta, sharp, tuple(heads), sat, wide, noise, 9000 + 13 * B + k if seed is None else seed, cond)


def case_id(c):
    kind = []
    if c.sharp:
        kind.append("sharp%d@%s" % (c.sharp, "+".join(str(h) for h in c.heads)))
    if c.sat:
        kind.append("sat")
    if c.wide:
        kind.append("wide")
    return "%dL%s%s-B%d-k%d-%s%s-%s%s" % (c.layers, "" if c.widths[2] == 784 else "-ragged", "-condprior" if c.cond else "", c.B, c.k, c.obj,
                                          "" if c.beta == 1.0 else "-beta%g" % c.beta, "+".join(kind), "" if c.noise == "host" else "-devnoise")


# ---------------------------------------------------------------- (i) 1-layer, bf16, sharp posteriors (oracle-only figures: test_offinit_host.py -rP)
BF16_1L = [
    # -- few rows (dec_rows_step): all five objectives, beta != 1 once
    case(5, 8, "vae_elbo"), case(5, 8, "iwae_elbo"), case(5, 8, "iwae_eq14"), case(5, 8, "vae_elbo_kl", 0.7), case(5, 8, "dreg"),
    case(7, 17, "dreg"),                      # latent_bwd_kernel on its own (k > 16)
    case(3, 70, "iwae_elbo"), case(3, 70, "dreg"),            # k > 64: the second pass of lse_image; two sharp units
    # -- 6 000 rows: the middle row-count family
    case(120, 50, "iwae_elbo"), case(120, 50, "dreg"),
    # -- 8 500 rows: the pipelined decoder, z made in its prologue; DReG there is the sampling prologue's sigma / (sigma + 1e-6)
    case(170, 50, "iwae_elbo"), case(170, 50, "dreg"),
    # -- every width ragged
    case(5, 8, "iwae_elbo", widths=WR), case(5, 8, "dreg", widths=WR),
]
BF16_1L_QW = [c for c in BF16_1L if c.B * c.k >= 8192]       # once more with options={"bern_qw_force": 1}
NOISE_1L = [case(5, 8, "iwae_elbo", noise="device")]

# ---------------------------------------------------------------- (ii) the 2-layer model, bf16: sharp on q(z1|x), on q(z2|z1), on both
L2_BF16 = [case(5, 8, obj, layers=2, heads=h) for h in ((3,), (7,), (3, 7)) for obj in ("iwae_elbo", "vae_elbo")] + [
    # 8 255 rows: the chain kernels.  One head at a time: with both sharp at k = 65 the weights thin out (oracle: median ESS/k 0.068; 0.093 at
    # 165 x 50) -- 0.111 and 0.120 here.  The rounding-aware oracle's latent rows differ from the exact oracle's by up to 0.020 (lpz1z2) and 0.016
    # (lpz2) at this row count at every one of 5 seeds tried (0.018 .. 0.022, 0.015 .. 0.018): the largest of 8 255 rows of a density that divides
    # by sigma_p^2, held by the GPU test to 0.05 against that oracle, not to EMU_ROW_ATOL (test_offinit_host.py takes half of each row's own bound)
    case(127, 65, "iwae_elbo", layers=2, heads=(3,)), case(127, 65, "iwae_elbo", layers=2, heads=(7,)),
]

# ---------------------------------------------------------------- (iii) the conditional-prior model: sharp on the encoder head only
COND_BF16 = [case(7, 6, "iwae_elbo", cond=COND)]

# ---------------------------------------------------------------- (iv) float32 mode against the exact oracle
F32 = [
    case(5, 8, "iwae_elbo"), case(5, 8, "dreg"), case(5, 8, "vae_elbo_kl", 0.7),
    case(5, 8, "iwae_elbo", sharp=0, sat=SAT), case(5, 8, "iwae_elbo", sharp=0, wide=WIDE), case(5, 8, "iwae_elbo", sat=SAT), case(5, 8, "dreg", sat=SAT),
    case(170, 50, "iwae_elbo"), case(170, 50, "iwae_elbo", sharp=0, sat=SAT), case(170, 50, "dreg", sat=SAT),
    case(5, 8, "iwae_elbo", layers=2), case(5, 8, "iwae_elbo", layers=2, sharp=0, sat=SAT), case(5, 8, "vae_elbo", layers=2, sat=SAT),
    case(5, 8, "iwae_elbo", layers=2, sharp=0, wide=WIDE),
]

SHARP_BF16 = BF16_1L + NOISE_1L + L2_BF16 + COND_BF16
ALL = SHARP_BF16 + F32
UNIQUE = list(dict.fromkeys(ALL))      # (the float32 list repeats bf16 cases)

# ---------------------------------------------------------------- (vi) iwae_eval_llh on the device's draws: (case, evaluators)
EVAL_N, EVAL_STEP = 3, 31
EVAL = [(case(EVAL_N, 65, noise="device"), ("fp32", "bf16")), (case(EVAL_N, 257, noise="device"), ("fp32", "bf16")),
        (case(EVAL_N, 65, noise="device", sat=SAT), ("fp32",)), (case(EVAL_N, 257, noise="device", sat=SAT), ("fp32",))]


def f32_round(a):
    """Operands as float32 (returned as float64): the oracle with this `rnd` is the float32-mode proxy of test_offinit_host.py."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


RND = {"exact": None, "emu": O.bf16_round, "f32": f32_round}


def stress(c, P):
    """The case's parameters from spread_params' output P."""
    if c.sharp:
        P = sharp_params(P, c.layers, SHIFTS4 if c.sharp == 4 else SHIFTS2, c.heads)
    if c.wide:
        P = [(W, b + c.wide) if i in ((3,) if c.layers == 1 else (3, 7)) else (W, b) for i, (W, b) in enumerate(P)]
    if c.sat:
        P = saturated_params(P, c.layers, *c.sat)
    return P


# ---------------------------------------------------------------- inputs and the oracle, computed once per case
@functools.lru_cache(maxsize=4)
def inputs(c, step=NOISE_STEP):
    """(x, P_spread, P, eps, y) of a case: make_golden.inputs at the case's seed, spread_params of it, the case's stressed parameters, and for
    noise = "device" the NumPy restatement of the device's Philox draws at `step`.  y: the one-hot condition (None without one)."""
    nh, nl, xd = c.widths
    nh, nl = (nh, nl) if c.layers == 1 else (list(nh), list(nl))
    got = MG.inputs(c.layers, nh, nl, xd, c.B, c.k if c.noise == "host" else 1, c.seed, cond=c.cond, cond_prior=bool(c.cond))
    x, P0, eps, y = got if c.cond else got + (None,)
    Ps = spread_params(P0, c.layers)
    if c.noise == "device":
        if c.layers == 1:
            eps = philox_np.device_eps(SEED, step, c.B, c.k, nl)
        else:
            eps = tuple(philox_np.device_eps(SEED, step, c.B, c.k, nl[l], stream=l) for l in range(2))
    return x, Ps, stress(c, Ps), eps, y


def run_oracle(c, P, mode):
    """(res, grads) of the oracle's step at parameters P.  res holds, next to the reference's entries (without the [k, B, X] logits):
    "a": the log-sigma pre-activations of the posterior heads by P index; "max_logit"; "sat_frac": the share of the decoder's second
    tanh layer with |y| >= 0.999."""
    x, _, _, eps, y = inputs(c)
    tape = {}
    if c.layers == 1:
        res, g = O.loss_grads_1layer(P, x, eps, c.beta, c.obj, rnd=RND[mode], tape=tape, y=y)
        a, d2 = {3: tape["enc"].a}, tape["dec"].d2.y
    else:
        res, g = O.loss_grads_2layer(P, x, eps[0], eps[1], 1.0, c.obj, rnd=RND[mode], tape=tape)
        a, d2 = {3: tape["enc1"].a, 7: tape["enc2"].a}, tape["dec1"].d2.y
    logits = res.pop("logits")
    res.update(a=a, max_logit=float(np.max(np.abs(logits))), sat_frac=float(np.mean(np.abs(d2) >= 0.999)))
    return res, g


@functools.lru_cache(maxsize=8)
def oracle(c, mode):
    """run_oracle at the case's own parameters; mode: "exact" (float64), "emu" (bf16 rounding points), "f32" (operands rounded to float32)."""
    return run_oracle(c, inputs(c)[2], mode)


def lpxz_key(c):
    return "lpxz" if c.layers == 1 else "lpxz1"


def scalar_keys(c):
    """The objective values the GPU tests compare for a case (the bodies of the existing parity tests)."""
    if c.layers == 2:
        return ("vae_elbo", "iwae_elbo", "iwae_eq14")
    if c.obj == "dreg" and c.B * c.k > 1024:
        return ("iwae_elbo",)
    return ("vae_elbo", "vae_elbo_kl", "iwae_elbo", "iwae_eq14")


# ---------------------------------------------------------------- (v) clean saturation
def clean_saturation_inputs(B=5, k=8, seed=9105):
    """(x, P, eps, figures): spread_params with the WEIGHT of the first encoder layer and of the first decoder layer scaled until the largest
    pre-activation is 60 (tanh through e^{2|x|} overflows float32 from |x| ~ 44.4) and the output layer's until the largest |logit| is 120
    (e^{|l|} overflows from 88.7).  Each factor is read off the float64 forward pass before it is applied, in network order."""
    nh, nl, xd = W1
    x, P0, eps = MG.inputs(1, nh, nl, xd, B, k, seed)
    P = [(np.array(W), np.array(b)) for W, b in spread_params(P0, 1)]

    def top(which):
        tape = {}
        O.forward_1layer(P, x, eps, _tape=tape)
        l = {"enc": tape["enc"].l1, "dec": tape["dec"].d1, "out": tape["dec"].out}[which]
        return float(np.max(np.abs(l.x @ l.W))), float(np.max(np.abs(l.x @ l.W + l.b)))
    for which, i, target in (("enc", 0, 60.0), ("dec", 4, 60.0), ("out", 6, 120.0)):
        P[i] = (P[i][0] * (target / top(which)[0]), P[i][1])      # (the factor from the weight's share alone: the bias does not scale)
    return x, P, eps, {"enc_pre": top("enc")[1], "dec_pre": top("dec")[1], "logit": top("out")[1]}


# ---------------------------------------------------------------- (vii) the analyses
def ess_rounding_share(log_w64, ess64, floor=1e-5):
    """How much of the floor of the analyses' run-time tolerance the OUTPUT rounding of log_w alone takes from ess: the float64 effective sample
    size of the float64 log_w [k, N] rounded once to float32 (what a device with perfect arithmetic returns) against ess64, over `floor`."""
    lw = np.asarray(log_w64, dtype=np.float64).astype(np.float32).astype(np.float64)
    w = np.exp(lw - lw.max(axis=0)[None])
    al = w / w.sum(axis=0)[None]
    return float(np.max(np.abs(1.0 / np.sum(al * al, axis=0) - np.asarray(ess64, dtype=np.float64)))) / floor
