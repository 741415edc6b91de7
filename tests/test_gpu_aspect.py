"""Parity at inverted and exact-tile widths across the row families.

Every other model of the suite has n_hidden >= n_latent, the large row-count kernels only ever run at the reference's widths +-1, and the
row-evaluation kernels (ais_chain_kernel, local_q_kernel, impute_rows_kernel, posterior_moments_kernel) never at the widths that fill
their arrays.  The step plan's shape predicates are equalities of padded widths (step_bf16.hip plan_step, kernels.hip *_ok), some of which hold
trivially at H >= D; the row-evaluation kernels size their LDS strips by max(Hp, Dp).  Here the SAME operations run against the SAME
oracle at the SAME tolerances (tests/_parity_common.py; the run-time rule of tests/test_gpu_ais.py: 8 x the float32 restatement's deviation
from float64, floor 1e-5) at the shapes of tests/_aspect_cases.py -- each names the predicate or array bound it cuts, and
tests/test_aspect_host.py holds every case to its admissibility conditions from the oracle alone.  The bodies are those of the modules they
come from (tests/_width_bodies.py, tests/_row_eval_bodies.py, tests/_grid_common.py and the statistics' _common modules).

Every test prints its worst errors next to their bounds (pytest -rP shows them).
"""
import numpy as np
import pytest

from oracle import iwae_np as O
import _activity_common as LA
import _aggregate_common as AP
import _grad_moments_common as GM
import _grid_common as GC
import _impute_ref as IM
import _width_bodies as WB
import _row_eval_bodies as RB
import _aspect_cases as A

pytestmark = pytest.mark.gpu


def _shape(c):
    return A.SHAPES[c.shape]


# ---------------------------------------------------------------- 1. the training step, few rows
@pytest.mark.parametrize("c", A.FEW_1L, ids=A.case_id)
def test_train_step_1layer_matches_oracle(gpu, c):
    WB.train_step_1layer(_shape(c), c.B, c.k, c.obj, c.beta, c.seed)


@pytest.mark.parametrize("c", A.FEW_1L, ids=A.case_id)
def test_float32_mode_matches_exact_oracle(gpu, c):
    nh, nl, xd = _shape(c)
    WB.float32_step(1, nh, nl, xd, c.B, c.k, c.obj, c.beta, c.seed)


# ---------------------------------------------------------------- 2. the row-count families of the step plan
@pytest.mark.parametrize("c", A.ROWS_1L, ids=A.case_id)
def test_row_count_families_bf16(gpu, c):
    """4 100, 6 000 and 8 500 rows: the assertion set of tests/test_gpu_ragged_widths.py::test_row_count_families_bf16, incl. the same step
    through iwae_train_step landing on the Adam reference."""
    WB.row_count_family_bf16(_shape(c), c.B, c.k, c.obj, c.seed)


@pytest.mark.parametrize("c,logits", A.ROWS_F32, ids=lambda v: A.case_id(v) if isinstance(v, A.Case) else ("logits" if v else "fused-epilogue"))
def test_row_count_families_float32(gpu, c, logits):
    nh, nl, xd = _shape(c)
    WB.float32_step(1, nh, nl, xd, c.B, c.k, c.obj, c.beta, c.seed, logits=logits)


# ---------------------------------------------------------------- 3. the 2-layer model
@pytest.mark.parametrize("c", A.L2_ALL, ids=A.case_id)
def test_train_step_2layer_matches_oracle(gpu, c):
    WB.train_step_2layer(_shape(c), c.B, c.k, c.obj, c.seed, exact_grad=c.exact_grad)


@pytest.mark.parametrize("c", A.FEW_2L, ids=A.case_id)
def test_float32_mode_2layer_matches_exact_oracle(gpu, c):
    nh, nl, xd = _shape(c)
    WB.float32_step(2, nh, nl, xd, c.B, c.k, c.obj, 1.0, c.seed, tag="2-layer ")


def test_two_layer_kernel_variants_agree(gpu):
    """L2_FULL at 8 500 rows: chain2_fwd_kernel / gblock_bwd_kernel against the separate launches (options no_chain2, no_chain2_bwd) with
    every latent lane live -- at the reference's widths a quarter of each latent tile is padding in both."""
    nh, nl, xd = A.L2_FULL
    WB.two_layer_kernel_variants_agree(nh, nl, xd, 170, 50, 5150 + 170)


# ---------------------------------------------------------------- 4. conditional and conditional-prior models at D > H
@pytest.mark.parametrize("c", A.COND, ids=A.case_id)
def test_conditional_models_match_oracle(gpu, c):
    nh, nl, xd = _shape(c)
    WB.conditional_bf16(nh, nl, xd, c.cond, c.prior, c.B, c.k, c.obj, c.beta, c.seed)


@pytest.mark.parametrize("c", A.COND, ids=A.case_id)
def test_float32_mode_conditional_models_match_exact_oracle(gpu, c):
    nh, nl, xd = _shape(c)
    WB.conditional_float32(nh, nl, xd, c.cond, c.prior, c.B, c.k, c.obj, c.beta, c.seed)


# ---------------------------------------------------------------- 5. device noise, evaluator, decode, trajectory at A_TILE and A_ODD
WIDE = [A.A_TILE, A.A_ODD]


@pytest.mark.parametrize("B,k,shape,obj", [(6, 5, A.A_TILE, "iwae_elbo"), (7, 3, A.A_ODD, "dreg"),
                                           (170, 50, A.A_TILE, "dreg"),           # 8 500 rows: z is made in the decoder's prologue (fuse_z at KT 4)
                                           (170, 50, A.A_ODD, "iwae_elbo")])
def test_device_noise_step_matches_oracle_on_the_same_draws(gpu, B, k, shape, obj):
    nh, nl, xd = shape
    WB.device_noise_step(B, k, nh, nl, xd, obj, 600 + nl + B)


@pytest.mark.parametrize("shape", WIDE)
def test_device_noise_matches_published_philox(gpu, shape):
    nh, nl, xd = shape
    WB.device_noise_matches_philox(nh, nl, xd)


@pytest.mark.parametrize("k", [65, 257])
@pytest.mark.parametrize("shape", WIDE)
def test_eval_llh_matches_exact_oracle_per_image(gpu, shape, k):
    WB.eval_llh_per_image(1, shape, k, 700 + k)


@pytest.mark.parametrize("shape", WIDE)
def test_decode_matches_oracle(gpu, shape):
    WB.decode_matches_oracle(shape)


@pytest.mark.parametrize("shape,B,k", [(A.A_TILE, 7, 3), (A.A_ODD, 10, 5)])
def test_three_adam_steps_track_the_oracle_trajectory(gpu, shape, B, k):
    WB.three_adam_steps(shape, B, k)


# ---------------------------------------------------------------- 6. the row-evaluation analyses at A_TILE, A_ODD, AN_MAX
_nets, _inets, _iruns, _pruns = {}, {}, {}, {}


def _net(name):
    """One handle per shape for the AIS / local-posterior tests (random-init parameters, float32 eval precision)."""
    if name not in _nets:
        from iwae_amd.native import NativeModel
        nh, nl, xd = A.SHAPES[name]
        x, P = A.analysis_inputs(name)
        m = NativeModel(1, nh, nl, x_dim=xd, seed=A.SEED)
        m.set_params(O.flatten_params(P))
        m.set_eval_precision("fp32")
        _nets[name] = (m, x, P)
    return _nets[name]


def _inet(name):
    """One handle per shape for the impute / posterior tests (SPREAD parameters, the mask of _aspect_cases.impute_inputs)."""
    if name not in _inets:
        from iwae_amd.native import NativeModel
        nh, nl, xd = A.SHAPES[name]
        x, P, mask = A.impute_inputs(name)
        m = NativeModel(1, nh, nl, x_dim=xd, seed=A.SEED)
        m.set_params(O.flatten_params(P))
        m.set_eval_precision("fp32")
        _inets[name] = (m, x, P, mask)
    return _inets[name]


def _irun(name, N, k):
    if (name, N, k) not in _iruns:
        m, x, P, mask = _inet(name)
        _iruns[(name, N, k)] = RB.impute_run(m, x, P, mask, A.SHAPES[name][1], N, k)
    return _iruns[(name, N, k)]


def _prun(name, N, k):
    if (name, N, k) not in _pruns:
        m, x, P, mask = _inet(name)
        _pruns[(name, N, k)] = RB.posterior_run(m, x, P, mask, A.SHAPES[name][1], N, k)
    return _pruns[(name, N, k)]


@pytest.mark.parametrize("init", ["encoder", "prior"])
@pytest.mark.parametrize("L", A.AIS_LS)
@pytest.mark.parametrize("N,Cn", A.AIS_CASES)
@pytest.mark.parametrize("name", A.ROW_EVAL)
def test_ais_single_transition_parity(gpu, name, N, Cn, L, init):
    m, x, P = _net(name)
    RB.ais_single_transition(m, x, P, A.SHAPES[name][1], N, Cn, L, init)


@pytest.mark.parametrize("objective", RB.LQ.OBJECTIVES)
@pytest.mark.parametrize("N,S", A.LOCAL_CASES)
@pytest.mark.parametrize("name", A.ROW_EVAL)
def test_local_posterior_iteration_parity(gpu, name, N, S, objective):
    m, x, P = _net(name)
    RB.local_iteration_parity(m, x, P, A.SHAPES[name][1], N, S, A.LOCAL_T, objective, seed=A.local_seed(name, N, S))


@pytest.mark.parametrize("N,k", A.IMPUTE_CASES)
@pytest.mark.parametrize("name", A.ROW_EVAL)
def test_impute_weight_and_imputation_parity(gpu, name, N, k):
    run = _irun(name, N, k)
    RB.impute_weight_parity(run, N, k, A.SHAPES[name][2])
    RB.impute_imputation_parity(run)
    assert np.all(np.isfinite(run[0]["log_w"][:, 1]))      # the image with nothing observed in the last 16-pixel tile


@pytest.mark.parametrize("N,k", A.IMPUTE_CASES)
@pytest.mark.parametrize("name", A.ROW_EVAL)
def test_posterior_moment_parity_indices_and_draws(gpu, name, N, k):
    m, x, P, mask = _inet(name)
    nl = A.SHAPES[name][1]
    run = _prun(name, N, k)
    RB.posterior_moment_parity(m, x, mask, nl, N, k, run)
    RB.same(run[0], _irun(name, N, k)[0], ("log_px", "ess", "log_w", "q_mu", "q_sigma"))      # the outputs shared with iwae_impute, bitwise
    eps = IM.draws(N, k, nl)
    RB.posterior_indices_and_draws(m, x, mask, nl, N, k, 7, eps, run[0])


# ---- at A_TILE (all 8 latent tiles live, Dp > Hp): the bitwise invariances and the guard bands
def test_ais_chunking_position_and_repeat_are_bitwise(gpu):
    m, x, P = _net("A_TILE")
    RB.ais_chunking_position_and_repeat_are_bitwise(m, x)
    print("ais at %s: t-chunks 0 / 1 / 2, a repeat and image 2 alone are bitwise equal over %s (bound: 0 differing bits)" % (A.A_TILE, ", ".join(RB.AIS_KEYS)))


def test_local_posterior_chunking_position_and_repeat_are_bitwise(gpu):
    m, x, P = _net("A_TILE")
    RB.local_chunking_position_and_repeat_are_bitwise(m, x)
    print("local_posterior at %s: t-chunks 0 / 1 / 3, a repeat and image 2 alone are bitwise equal over %s (bound: 0 differing bits)" % (A.A_TILE, ", ".join(RB.LOCAL_KEYS)))


@pytest.mark.parametrize("k", [13, 70], ids=["one_chunk", "two_chunks"])
def test_impute_position_chunking_and_repeat_are_bitwise(gpu, k):
    m, x, P, mask = _inet("A_TILE")
    RB.impute_position_chunking_and_repeat_are_bitwise(m, x, mask, A.A_TILE[1], k)
    print("impute at %s k %d: a repeat, one image per launch and every image alone are bitwise equal over %s (bound: 0 differing bits)" % (A.A_TILE, k, ", ".join(RB.IMPUTE_KEYS)))


@pytest.mark.parametrize("k", [13, 70], ids=["one_chunk", "two_chunks"])
def test_posterior_position_chunking_and_repeat_are_bitwise(gpu, k):
    m, x, P, mask = _inet("A_TILE")
    RB.posterior_position_chunking_and_repeat_are_bitwise(m, x, mask, A.A_TILE[1], k, _prun("A_TILE", 5, k)[0])
    print("posterior at %s k %d: a repeat, one image per launch, every image alone and NaN at unobserved pixels are bitwise equal over %s (bound: 0 differing bits)"
          % (A.A_TILE, k, ", ".join(RB.POSTERIOR_KEYS)))


def test_impute_writes_nothing_past_the_last_pixel(gpu):
    m, x, P, mask = _inet("A_TILE")
    RB.impute_nothing_past_the_last_pixel(m, x, mask, A.A_TILE[1], A.A_TILE[2], lambda N, k: _irun("A_TILE", N, k)[0])
    print("impute at %s: the guard row behind xhat [N, %d] on the device is untouched at (N, k) = (5, 13) and (2, 65), xhat bitwise the Python level's" % (A.A_TILE, A.A_TILE[2]))


def test_posterior_writes_nothing_past_the_last_feature(gpu):
    m, x, P, mask = _inet("A_TILE")
    RB.posterior_nothing_past_the_last_feature(m, x, mask, A.A_TILE[1], lambda N, k: _prun("A_TILE", N, k)[0])
    print("posterior at %s: the guard rows behind cov, mean, z and idx on the device are untouched at (N, k) = (5, 13) and (2, 65), all four bitwise the Python level's" % (A.A_TILE,))


def _ais_guard(m, x, nl, N, Cn):
    """iwae_ais through the raw binding with DEVICE arrays for the outputs the kernels write in place (model.h staged_out: a device
    pointer is written in place, a host pointer is served from a workspace by a copy of the exact size): z [C, N, D], dH [T, C, N] and
    accepted [T, C, N], each with a guard row of sentinels behind it.  log_px, log_w, ess, step_out and accept_rate always go through
    copy_out from the workspace, so a guard cannot cover them; they are compared with the Python level's."""
    import ctypes as C
    import torch
    from iwae_amd import _capi
    import _ais_ref as R
    T, L = 2, 2
    betas = np.array([0.0, 0.5, 1.0], dtype=np.float32)
    eps0, mom, unif = R.noise(900 + N + Cn, T, Cn, N, nl)
    xs = np.ascontiguousarray(x[:N])
    o = _capi.AisOptions()
    o.C, o.T, o.L, o.betas, o.step_size, o.adapt = Cn, T, L, betas.ctypes.data, 0.3, 0
    o.eps0, o.mom, o.unif = eps0.ctypes.data, mom.ctypes.data, unif.ctypes.data
    rows = Cn * N
    z = torch.full((rows + 1, nl), -7.0, dtype=torch.float32, device="cuda")
    dH = torch.full((T * rows + 1,), -7.0, dtype=torch.float32, device="cuda")
    acc = torch.full((T * rows + 1,), 7, dtype=torch.uint8, device="cuda")
    lw, lpx = np.zeros(rows, dtype=np.float64), np.zeros(N, dtype=np.float64)
    outs = _capi.AisOutputs()
    outs.log_px, outs.log_w, outs.z, outs.dH, outs.accepted = lpx.ctypes.data, lw.ctypes.data, z.data_ptr(), dH.data_ptr(), acc.data_ptr()
    assert m.lib.iwae_ais(m.h, xs.ctypes.data, N, C.byref(o), C.byref(outs)) == 0
    torch.cuda.synchronize()
    r = m.ais(xs, n_chains=Cn, leapfrog=L, step_size=0.3, adapt=False, betas=betas, noise=(eps0, mom, unif), trace=True)
    zh, dh, ah = z.cpu().numpy(), dH.cpu().numpy(), acc.cpu().numpy()
    print("ais N%d C%d: guard rows behind z [%d, %d], dH [%d], accepted [%d] untouched: %s; accept rate %.3f"
          % (N, Cn, rows, nl, T * rows, T * rows, bool(np.all(zh[rows] == -7.0) and dh[T * rows] == -7.0 and ah[T * rows] == 7), r["accepted"].mean()))
    assert np.all(zh[rows] == -7.0) and dh[T * rows] == -7.0 and ah[T * rows] == 7
    assert np.array_equal(zh[:rows].reshape(Cn, N, nl), r["z"])
    assert np.array_equal(dh[:T * rows].reshape(T, Cn, N), r["dH"]) and np.array_equal(ah[:T * rows].reshape(T, Cn, N), r["accepted"])
    assert np.array_equal(lw.reshape(Cn, N), r["log_w"]) and np.array_equal(lpx, r["log_px"])


def test_ais_writes_nothing_past_the_last_feature(gpu):
    m, x, P = _net("A_TILE")
    for N, Cn in A.AIS_CASES:
        _ais_guard(m, x, A.A_TILE[1], N, Cn)


def _local_guard(m, x, nl, N, S):
    """iwae_local_posterior through the raw binding with DEVICE arrays for the outputs the kernels write in place (model.h staged_out):
    grad [N, 2 D], bound [T, N] and log_w [E S, N], each with a guard row of sentinels behind it.  elbo, iwae, mu, sigma, q_mu and q_sigma
    always go through copy_out from the workspace, so a guard cannot cover them; mu, sigma and elbo are compared with the Python level's."""
    import ctypes as C
    import torch
    from iwae_amd import _capi
    T, E = 2, 1
    noise = np.random.default_rng(950 + N + S).standard_normal((T + E, S, N, nl)).astype(np.float32)
    xs = np.ascontiguousarray(x[:N])
    o = _capi.LocalOptions()
    o.S, o.T, o.E, o.objective, o.lr, o.beta_1, o.beta_2, o.epsilon = S, T, E, 1, 0.05, 0.9, 0.999, 1e-4
    o.eps = noise.ctypes.data
    grad = torch.full((N + 1, 2 * nl), -7.0, dtype=torch.float32, device="cuda")
    bound = torch.full((T + 1, N), -7.0, dtype=torch.float32, device="cuda")
    lw = torch.full((E * S + 1, N), -7.0, dtype=torch.float32, device="cuda")
    mu, sg, elbo = np.zeros((N, nl), np.float32), np.zeros((N, nl), np.float32), np.zeros(N, np.float64)
    outs = _capi.LocalOutputs()
    outs.elbo, outs.mu, outs.sigma = elbo.ctypes.data, mu.ctypes.data, sg.ctypes.data
    outs.grad, outs.bound, outs.log_w = grad.data_ptr(), bound.data_ptr(), lw.data_ptr()
    assert m.lib.iwae_local_posterior(m.h, xs.ctypes.data, N, C.byref(o), C.byref(outs)) == 0
    torch.cuda.synchronize()
    r = m.local_posterior(xs, n_samples=S, n_iters=T, n_eval=E, objective="iwae", lr=0.05, noise=noise, trace=True)
    ok = True
    for name, got, rows in (("grad", grad, N), ("bound", bound, T), ("log_w", lw, E * S)):
        g = got.cpu().numpy()
        ok = ok and bool(np.all(g[rows] == -7.0))
        assert np.all(g[rows] == -7.0), name
        assert np.array_equal(g[:rows], r[name]), name
    print("local_posterior N%d S%d: guard rows behind grad [%d, %d], bound [%d, %d], log_w [%d, %d] untouched: %s" % (N, S, N, 2 * nl, T, N, E * S, N, ok))
    assert np.array_equal(mu, r["mu"]) and np.array_equal(sg, r["sigma"]) and np.array_equal(elbo, r["elbo"])


def test_local_posterior_writes_nothing_past_the_last_feature(gpu):
    m, x, P = _net("A_TILE")
    for N, S in A.LOCAL_CASES:
        _local_guard(m, x, A.A_TILE[1], N, S)


# ---------------------------------------------------------------- 7. the other analyses
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("layers,shape", [(1, A.A_TILE), (2, A.L2_FULL)], ids=["A_TILE", "L2_FULL"])
def test_latent_activity_matches_float64(gpu, layers, shape, prec):
    """L2_FULL in bf16: the fused act_chain path (activity_kernels.hip act_chain_ok: 4/4/2) with every latent lane live."""
    nh, nl, xd = shape
    N, k = 37, 50
    x, P, m, eps = LA._setup(layers, nh, nl, xd, N, k, 31 + N, prec)
    m.set_step(5, 0)
    r = m.latent_activity(x, k=k, eps=eps, per_image=True)
    LA._check(r, LA.reference(P, x, eps, rnd=None if prec == "fp32" else O.bf16_round), prec)
    m.close()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_aggregate_posterior_per_sample_parity_and_sums(gpu, prec):
    nh, nl, xd = A.A_TILE
    N, S = 130, 3
    x, m, eps = AP._setup(nh, nl, xd, N, S, 17 + N + S, prec)
    r = m.aggregate_posterior(x, n_samples=S, eps=eps, per_sample=True)
    m.close()
    assert r["q_mu"].shape == (N, nl) and r["unit_kl"].shape == (nl,)
    AP._check_sums(r, AP._parity(r, eps), N)
    print("aggregate posterior %s %s: sums against float64 of the device's rows at rtol 1e-6; max unit_mi %.4g (<= log N = %.4g)" % (A.A_TILE, prec, float(np.max(r["unit_mi"])), np.log(N)))
    assert np.all(r["unit_mi"] <= np.log(N) + 1e-4)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("obj", ["iwae_elbo", "dreg"])
def test_grad_moments_equal_the_host_fold(gpu, prec, obj):
    nh, nl, xd = A.A_TILE
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
    print("grad moments %s %s %s: mean off the host fold %.3g, variance %.3g, relative to the largest element (<= 1e-12)"
          % (A.A_TILE, prec, obj, float(np.max(np.abs(mean - ref_mean)) / np.max(np.abs(ref_mean))), float(np.max(np.abs(var - ref_var)) / np.max(np.abs(ref_var)))))
    GM._close(mean, ref_mean)
    GM._close(var, ref_var)
    m.close()


@pytest.mark.parametrize("nh,nl,xd", [(16, 4, 800), (64, 3, 799)])
def test_grid_posterior_float32_matches_float64(gpu, nh, nl, xd):
    """x_dim at iwae_grid_posterior's limit (analysis.hip: Xp32 <= GRID_XP_MAX = 800), exactly and through padding."""
    GC.float32_matches_float64(nh, nl, xd)


# ---------------------------------------------------------------- 8. limits
def test_limits_of_the_row_evaluation_analyses(gpu):
    """(209, 100, 784) rounds to 14 hidden tiles: refused by all four with IWAE_ERR_ARG (ValueError), the noise step unchanged and the
    handle still usable.  (208, 128, .) is accepted by iwae_ais -- that iwae_local_posterior, iwae_impute and iwae_posterior accept it is
    asserted by their own modules' test_rejected_arguments_leave_the_step_alone, as is the refusal of 224 (256 for iwae_ais); x_dim 801 is
    refused by iwae_grid_posterior."""
    from iwae_amd.native import NativeModel
    import make_golden as MG
    x, P, eps = MG.inputs(1, 209, 100, 784, 2, 3, 5)
    m = NativeModel(1, 209, 100, x_dim=784, seed=A.SEED)
    m.set_params(O.flatten_params(P))
    m.set_step(17, 3)
    want = m.debug_eps(2, 2, 0)
    calls = (lambda: m.ais(x, n_chains=2, leapfrog=1, step_size=0.1, betas=[0.0, 1.0]), lambda: m.local_posterior(x, n_samples=2, n_iters=1, n_eval=1),
             lambda: m.impute(x, n_samples=2), lambda: m.posterior(x, n_samples=2))
    for call in calls:
        with pytest.raises(ValueError, match="n_hidden <= 208"):
            call()
    assert np.array_equal(m.debug_eps(2, 2, 0), want)             # none of them moved the noise step
    r = m.forward_backward(x, 3, 1.0, "iwae_elbo", eps=eps)       # the handle is still usable
    fresh = NativeModel(1, 209, 100, x_dim=784, seed=A.SEED)
    fresh.set_params(O.flatten_params(P))
    rf = fresh.forward_backward(x, 3, 1.0, "iwae_elbo", eps=eps)
    assert r["iwae_elbo"] == rf["iwae_elbo"] and np.array_equal(m.get_grads(), fresh.get_grads())
    fresh.close()
    m.close()
    edge = NativeModel(1, 208, 128, x_dim=48, seed=1)
    r = edge.ais(x[:, :48], n_chains=2, leapfrog=1, step_size=0.1, betas=[0.0, 1.0])
    assert np.all(np.isfinite(r["log_px"]))
    edge.close()
    wide = NativeModel(1, 16, 2, x_dim=801, seed=1)
    with pytest.raises(ValueError, match="x_dim <= 800"):
        wide.grid_posterior(np.zeros((2, 801), np.float32), np.zeros((10, 2), np.float32))
    wide.close()
