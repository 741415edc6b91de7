"""Parity at odd and tile-straddling feature widths.

A lane owns four consecutive features of every 16 (iwae_amd/csrc/layout.h), so a width with F % 4 != 0 is the one case where a lane's
own float4 / quad straddles the end of the tensor; the 16-, 32- and 64-feature tile edges taken one feature too far or one short
move KT, the MG groups and Np32 / Kp32; and with one odd width the tensor offsets of the flat parameter / gradient vector stop being
multiples of 4 floats.  The other GPU modules take their widths from round numbers (every hidden width and x_dim a multiple of 4).
Here the SAME operations run against the SAME oracle at the SAME tolerances (tests/_parity_common.py) -- only the widths are new, and
no shape in this module is a multiple of 4 in all three dimensions.  The bodies are tests/_width_bodies.py's, shared with
tests/test_gpu_aspect.py.

Every test prints its worst errors next to their bounds (pytest -rP shows them).
"""
import numpy as np
import pytest

from oracle import iwae_np as O, philox_np
import make_golden as MG
import _activity_common as LA
import _aggregate_common as AP
import _grad_moments_common as GM
import _width_bodies as WB
from _width_bodies import SEED, _model, _report
from _parity_common import EMU_SCALAR_ATOL, EMU_GRAD_REL, _grad_rel_errors, _densities_at_device_heads_2layer

pytestmark = pytest.mark.gpu

# (n_hidden, n_latent, x_dim): what each shape cuts
S_ODD = (37, 5, 53)            # every width odd; the quad is cut at 1 of 4
S_REF_M1 = (199, 99, 783)      # the reference's widths minus one; the quad is cut at 3 of 4
S_REF_P1 = (201, 101, 785)     # the reference's widths plus one: one feature into a new quad and a new 16-tile (785 = 49 * 16 + 1)
S_63 = (63, 31, 63)            # one short of a full 32-step and 64-group
S_65 = (65, 33, 65)            # one past a full 32-step and 64-group (a second MG group with one live feature)
S_KT5 = (129, 3, 17)           # KT = 5 (no template instantiation); a 3-D latent; x_dim one past a 16-tile
S_MAX = (255, 127, 1023)       # the largest odd widths: run-time-KT fallbacks
S_ONE = (1, 1, 1)              # the smallest model the ABI accepts

L2_SMALL = ([67, 35], [33, 3], 61)
L2_REF_M1 = ([199, 99], [97, 49], 783)
L2_REF_P1 = ([201, 101], [101, 51], 785)


# ---------------------------------------------------------------- 1. the 1-layer bf16 train step
CASES_1L = [  # (shape, B, k, objective, beta): B * k in 6 .. 40, B no multiple of 4, k = 1 and k > 1, the five objectives
    (S_ODD, 5, 3, "dreg", 1.0),                 # DReG at n_latent % 4 = 1
    (S_REF_M1, 7, 5, "vae_elbo_kl", 0.7),       # the analytic KL at n_latent % 4 = 3, beta != 1
    (S_REF_M1, 9, 1, "vae_elbo", 1.0),
    (S_REF_P1, 6, 5, "iwae_elbo", 1.0),
    (S_REF_P1, 7, 3, "dreg", 1.0),
    (S_63, 3, 7, "iwae_eq14", 1.0),
    (S_65, 10, 1, "vae_elbo", 1.0),
    (S_65, 5, 6, "vae_elbo_kl", 1.0),
    (S_KT5, 5, 8, "iwae_elbo", 1.0),
    (S_KT5, 9, 4, "dreg", 1.0),
    (S_MAX, 3, 2, "iwae_elbo", 1.0),
    (S_MAX, 7, 5, "iwae_eq14", 1.0),
    (S_ONE, 6, 5, "iwae_elbo", 1.0),
]


@pytest.mark.parametrize("shape,B,k,obj,beta", CASES_1L)
def test_train_step_1layer_matches_oracle(gpu, shape, B, k, obj, beta):
    """The body of test_gpu_parity.py::test_train_step_1layer_matches_oracle over the shape set.  S_ONE: a gradient tensor has one
    element and a single bf16 flip is the whole tensor -- finite, the scalars, and the gradient against the exact oracle only (its strict
    check is the float32 test below)."""
    WB.train_step_1layer(shape, B, k, obj, beta, 100 + B + k, strict=shape != S_ONE)


# ---------------------------------------------------------------- 2. float32 mode
CASES_F32 = [  # (shape, B, k, objective, beta)
    (S_ODD, 5, 3, "dreg", 1.0),
    (S_ODD, 6, 5, "iwae_elbo", 0.7),
    (S_REF_M1, 7, 5, "vae_elbo_kl", 0.7),
    (S_REF_P1, 6, 5, "iwae_elbo", 1.0),
    (S_REF_P1, 7, 3, "dreg", 1.0),
    (S_63, 3, 7, "iwae_eq14", 1.0),
    (S_65, 10, 1, "vae_elbo", 1.0),
    (S_KT5, 5, 8, "iwae_elbo", 1.0),
    (S_MAX, 3, 2, "iwae_elbo", 1.0),
    (S_ONE, 6, 5, "iwae_elbo", 1.0),
    (S_ONE, 5, 1, "vae_elbo_kl", 0.7),
]


@pytest.mark.parametrize("shape,B,k,obj,beta", CASES_F32)
def test_float32_mode_matches_exact_oracle(gpu, shape, B, k, obj, beta):
    nh, nl, xd = shape
    WB.float32_step(1, nh, nl, xd, B, k, obj, beta, 300 + B + k)


# ---------------------------------------------------------------- 3. the row-count families of the step plan
ROWS = [(120, 50), (170, 50)]      # 6 000 rows: the middle family; 8 500: the pipelined decoder / fused dX family


@pytest.mark.parametrize("obj", ["iwae_elbo", "dreg"])
@pytest.mark.parametrize("B,k", ROWS)
@pytest.mark.parametrize("shape", [S_REF_M1, S_REF_P1])
def test_row_count_families_bf16(gpu, shape, B, k, obj):
    """The assertions of test_large_row_count_kernels_match_oracle and test_kernel_family_boundaries_match_oracle at the reference's
    widths -1 / +1: every row's densities against the oracle at the device's own encoder head and the typical row against the pure
    oracle, the encoder head itself, the scalars, every gradient tensor (norm and elementwise) against both oracles, and the same
    step through iwae_train_step (Adam fused into the slab reduction)."""
    WB.row_count_family_bf16(shape, B, k, obj, 4242 + B)


@pytest.mark.parametrize("logits", [True, False], ids=["logits", "fused-epilogue"])
@pytest.mark.parametrize("B,k", ROWS)
@pytest.mark.parametrize("shape", [S_REF_M1, S_REF_P1])
def test_row_count_families_float32(gpu, shape, B, k, logits):
    """float32 mode at 6 000 and 8 500 rows (row-split weight gradients; from ~8 000 rows the call without `logits` takes the output
    layer's fused epilogue -- the case with want=("logits",) does not)."""
    nh, nl, xd = shape
    WB.float32_step(1, nh, nl, xd, B, k, "iwae_elbo", 1.0, 4242 + B, logits=logits)


# ---------------------------------------------------------------- 4. the 2-layer model
CASES_2L = [(L2_SMALL, 5, 3, "iwae_elbo"), (L2_SMALL, 6, 5, "iwae_eq14"), (L2_REF_M1, 3, 7, "iwae_elbo"), (L2_REF_P1, 7, 5, "vae_elbo"),
            (L2_REF_M1, 170, 50, "iwae_elbo")]


@pytest.mark.parametrize("shape,B,k,obj", CASES_2L)
def test_train_step_2layer_matches_oracle(gpu, shape, B, k, obj):
    """The assertions of test_gpu_parity.py::test_train_step_2layer_matches_oracle (its bounds, unchanged), densities at the device's
    own three Gaussian heads; at 8 500 rows the fused chain kernels and the one-launch decoder (tests/_width_bodies.py: train_step_2layer
    says how the pure oracle is held at that row count)."""
    WB.train_step_2layer(shape, B, k, obj, 200 + B + k)


@pytest.mark.parametrize("shape,B,k,obj", CASES_2L)
def test_float32_mode_2layer_matches_exact_oracle(gpu, shape, B, k, obj):
    nh, nl, xd = shape
    WB.float32_step(2, nh, nl, xd, B, k, obj, 1.0, 200 + B + k, logits=B * k < 1000, tag="2-layer ")


# ---------------------------------------------------------------- 5. conditional models: the condition sits in z's pad features
COND = [  # (n_hidden, n_latent, x_dim, cond_dim)
    (199, 21, 783, 10),      # 31 of 32: one pad feature left
    (65, 25, 65, 7),         # exactly fills 32
    (37, 5, 53, 3),
]


@pytest.mark.parametrize("prior", [False, True], ids=["n01-prior", "learned-prior"])
@pytest.mark.parametrize("nh,nl,xd,C", COND)
def test_conditional_models_match_oracle(gpu, nh, nl, xd, C, prior):
    """The assertions of test_conditional_model_matches_oracle / test_conditional_prior_model_matches_oracle."""
    B, k, obj, beta = (7, 6, "iwae_elbo", 1.0) if nl != 25 else (5, 4, "vae_elbo", 0.7)
    WB.conditional_bf16(nh, nl, xd, C, prior, B, k, obj, beta, 500 + nl)


@pytest.mark.parametrize("prior", [False, True], ids=["n01-prior", "learned-prior"])
@pytest.mark.parametrize("nh,nl,xd,C", COND)
def test_float32_mode_conditional_models_match_exact_oracle(gpu, nh, nl, xd, C, prior):
    """The assertions of test_gpu_parity.py::test_float32_mode_conditional_models_match_exact_oracle."""
    B, k, obj, beta = (7, 6, "iwae_elbo", 1.0) if nl != 25 else (5, 4, "vae_elbo", 0.7)
    WB.conditional_float32(nh, nl, xd, C, prior, B, k, obj, beta, 500 + nl)


# ---------------------------------------------------------------- 6. the device's own noise at odd latent widths
@pytest.mark.parametrize("B,k,nh,nl,xd,obj", [(7, 3, 37, 1, 53, "iwae_elbo"), (7, 3, 37, 3, 53, "dreg"), (5, 6, 37, 5, 53, "iwae_elbo"),
                                              (6, 5, 65, 33, 65, "dreg"), (6, 5, 201, 101, 785, "iwae_elbo"),
                                              (170, 50, 201, 101, 785, "iwae_elbo"),      # 8 500 rows: z is made inside the decoder kernel
                                              (170, 50, 199, 99, 783, "dreg")])
def test_device_noise_step_matches_oracle_on_the_same_draws(gpu, B, k, nh, nl, xd, obj):
    """The assertions of test_gpu_parity.py::test_device_noise_step_matches_oracle_on_the_same_draws: Philox gives four normals per
    call, so at D % 4 != 0 the last call's tail is dropped (a width-5 draw is the first 5 columns of the width-8 draw).
    n_latent = 1: the gradients of the two head biases are ONE number each, the sum over the B images of the head gradient t_b, and every
    tensor is held to the unchanged EMU_GRAD_REL.  With the input seed 601 the t_b of the mu head cancel (|sum t| = 0.055 sum |t|, read
    off the oracle alone) and the relative error of that one number is the terms' error times 18, whatever the arithmetic; the inputs
    of that case are seed 602, where neither sum cancels (|sum t| = 0.70 sum |t| for both heads)."""
    WB.device_noise_step(B, k, nh, nl, xd, obj, 602 if nl == 1 else 600 + nl)


def test_device_noise_step_2layer_matches_oracle_on_the_same_draws(gpu):
    """The 2-layer model with n_latent = [33, 3]: z1 from stream 0, z2 from stream 1 (the device-noise assertions of
    test_kernel_family_boundaries_match_oracle and, per row at the device's heads, of test_two_layer_kernel_variants_agree)."""
    nh, nl, xd = L2_SMALL
    B, k, step = 6, 5, 17
    x, P, _ = MG.inputs(2, nh, nl, xd, B, 1, 633)
    e1 = philox_np.device_eps(SEED, step, B, k, nl[0], stream=0, batch_offset=3)
    e2 = philox_np.device_eps(SEED, step, B, k, nl[1], stream=1, batch_offset=3)
    res_d, g_d = O.loss_grads_2layer(P, x, e1, e2, 1.0, "iwae_elbo", rnd=O.bf16_round)
    m = _model(2, nh, nl, xd)
    m.set_params(O.flatten_params(P))
    m.set_step(step, 3)
    r = m.forward_backward(x, k, 1.0, "iwae_elbo", want=("lpz", "lpz2", "lqzx", "lqzx2"))
    at = _densities_at_device_heads_2layer(m, e1, e2, B, k, nl)
    errs = _grad_rel_errors(m.get_grads(), g_d)
    _report("device noise 2-layer %s" % (L2_SMALL,),
            rows_at_heads=max(float(np.max(np.abs(r[a] - at[b]))) for a, b in (("lpz", "lpz1z2"), ("lpz2", "lpz2"), ("lqzx", "lqz1x"), ("lqzx2", "lqz2z1"))),
            rows_bound=2e-2, scalar_emu=abs(r["iwae_elbo"] - res_d["iwae_elbo"]), bound=EMU_SCALAR_ATOL, grad_emu=max(errs), gbound=EMU_GRAD_REL)
    for a, b in (("lpz", "lpz1z2"), ("lpz2", "lpz2"), ("lqzx", "lqz1x"), ("lqzx2", "lqz2z1")):
        assert np.max(np.abs(r[a] - at[b])) < 2e-2, b
    assert abs(r["iwae_elbo"] - res_d["iwae_elbo"]) < EMU_SCALAR_ATOL
    assert max(errs) < EMU_GRAD_REL, errs
    m.close()


@pytest.mark.parametrize("nl", [1, 3, 5, 33, 101])
def test_device_noise_matches_published_philox(gpu, nl):
    """iwae_debug_eps at odd widths against the NumPy restatement (fast v_log / v_sin / v_cos: abs err <= 2e-5), the batch offset, and the
    forward pass consuming exactly these draws -- as test_gpu_parity.py::test_device_noise_matches_published_philox does at width 100."""
    nh, xd = (37, 53) if nl < 33 else (65, 65)
    WB.device_noise_matches_philox(nh, nl, xd)


# ---------------------------------------------------------------- 7. the evaluator and decode
@pytest.mark.parametrize("k", [130, 1000])
@pytest.mark.parametrize("layers,shape", [(1, S_ODD), (1, S_REF_P1), (2, L2_SMALL)])
def test_eval_llh_matches_exact_oracle_per_image(gpu, layers, shape, k):
    """iwae_eval_llh (main.py:170-184) on 5 images, both evaluator precisions, per image against the exact float64 oracle on the device's
    Philox draws (image i: rows i * k .. of streams 0 / 1): float32 evaluator <= 5e-3 nat, bf16 evaluator <= 0.1 nat (the bounds of
    test_trained_model_k5000_llh_within_north_star_tolerance)."""
    WB.eval_llh_per_image(layers, shape, k, 700 + k)


@pytest.mark.parametrize("shape", [S_ODD, S_REF_P1])
def test_decode_matches_oracle(gpu, shape):
    WB.decode_matches_oracle(shape)


# ---------------------------------------------------------------- 8. three Adam steps
@pytest.mark.parametrize("shape,B,k", [(S_ODD, 7, 3), (S_REF_P1, 20, 5)])
def test_three_adam_steps_track_the_oracle_trajectory(gpu, shape, B, k):
    """The loop of test_training_reduces_loss_and_matches_oracle_trajectory: each step reads the bf16 weight images the previous step's
    update wrote -- a misplaced image chunk at a non-multiple width shows from step 2 on."""
    WB.three_adam_steps(shape, B, k)


# ---------------------------------------------------------------- 9. the statistics entry points, one odd shape each
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("layers,shape", [(1, S_ODD), (2, L2_SMALL)])
def test_latent_activity_matches_float64(gpu, layers, shape, prec):
    nh, nl, xd = shape
    N, k = 37, 50
    x, P, m, eps = LA._setup(layers, nh, nl, xd, N, k, 31 + N, prec)
    m.set_step(5, 0)
    r = m.latent_activity(x, k=k, eps=eps, per_image=True)
    LA._check(r, LA.reference(P, x, eps, rnd=None if prec == "fp32" else O.bf16_round), prec)
    m.close()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_aggregate_posterior_per_sample_parity_and_sums(gpu, prec):
    nh, nl, xd = S_ODD
    N, S = 130, 3
    x, m, eps = AP._setup(nh, nl, xd, N, S, 17 + N + S, prec)
    r = m.aggregate_posterior(x, n_samples=S, eps=eps, per_sample=True)
    m.close()
    assert r["q_mu"].shape == (N, nl) and r["unit_kl"].shape == (nl,)
    AP._check_sums(r, AP._parity(r, eps), N)
    assert np.all(r["unit_mi"] <= np.log(N) + 1e-4)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("obj", ["iwae_elbo", "dreg"])
def test_grad_moments_equal_the_host_fold(gpu, prec, obj):
    nh, nl, xd = S_ODD
    B, k, M, beta = 5, 3, 4, 0.8
    m, x, _, _ = GM._model(1, nh, nl, xd, prec, B, k)
    before = GM._state(m)
    m.set_step(GM.S0)
    mean, var = m.grad_moments(x, k, M, beta, obj)
    g_after = m.get_grads()
    GM._assert_state_equal(GM._state(m), before)
    ref_mean, ref_var, g_last = GM._host_fold(m, x, k, beta, obj, GM.S0, M)
    assert np.array_equal(g_after.view(np.uint32), g_last.view(np.uint32))
    assert np.all(var >= 0) and np.max(var) > 0
    GM._close(mean, ref_mean)
    GM._close(var, ref_var)
    m.close()


def test_dataset_gather_binarize_is_bit_exact(gpu):
    """x_dim = 53: the last Philox call of a row covers one pixel."""
    nh, nl, xd = S_ODD
    rng = np.random.default_rng(3)
    N = 300
    gray = (rng.random((N, xd)) * 256).astype(np.uint8)
    gray[:, :5] = 0
    gray[:, 48:] = 255
    _, P, _ = MG.inputs(1, nh, nl, xd, 1, 1, 5)
    m = _model(1, nh, nl, xd)
    m.set_params(O.flatten_params(P))
    m.dataset_upload(gray)
    order = rng.permutation(N).astype(np.int32)
    for epoch in (0, 7):
        m.dataset_begin_epoch(epoch, order)
        xb = m.dataset_get_batch(37, 150)
        ref = philox_np.device_binarize(SEED, epoch, gray, order[37:187])
        np.testing.assert_array_equal(xb, ref)
    assert xb[:, :5].sum() == 0 and xb[:, 48:].min() == 1
    # a train step fed from the resident dataset equals a train step fed the same batch through the host path
    m.dataset_begin_epoch(7, order)
    m.set_step(5, 0)
    a = m.train_step_dataset(37, 150, 5, 1.0, 1e-3, "iwae_elbo")
    pa = m.get_params()
    m.set_params(O.flatten_params(P)); m.set_adam_state(np.zeros(m.n_params), np.zeros(m.n_params), 0)
    m.set_step(5, 0)
    b = m.train_step(ref, 5, 1.0, 1e-3, "iwae_elbo")
    assert a["iwae_elbo"] == b["iwae_elbo"]
    np.testing.assert_array_equal(pa, m.get_params())
    m.close()
