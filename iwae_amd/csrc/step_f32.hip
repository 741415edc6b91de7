// The float32 step (iwae_config.precision = IWAE_PREC_FP32, and iwae_eval_llh / the analyses by default): host code; kernels in fp32_kernels.hip
// and, shared with the bf16 path, kernels.hip / row_kernels.hip / update_kernels.hip.  plan_step_f32 decides the step's kernels and streams once; forward_f32, backward_f32 and f32_dw
// execute what it decided.
#include <string.h>
#include <algorithm>
#include "model.h"       // (the HIP runtime, include/iwae_amd.h and kernels.h come with it)

using namespace iwae;

// =================================================================== float32 mode
// The reference's own arithmetic: Keras Dense layers in float32 (src/iwae1.py:31-34,72-75).  Same step structure as the bf16
// path with plain row-major float32 tensors and one generic MFMA GEMM (fp32_kernels.hip); the per-sample kernels that already
// work in float32 (sampling + densities, lse_kernel, latent_bwd_kernel, gauss_*_kernel, Adam) are shared.
namespace {

int f32_gemm(iwae_model* m, const float* A, long sam, long sak, const float* B, long sbk, long sbn, float* C, long ldc, int M, int N, int K,
             const float* bias, int epi, const float* ACT, long ldact, bool accumulate, const float* brow_scale = nullptr, const float* orow_scale = nullptr,
             hipStream_t st = nullptr, bool no_ksplit = false) {
    GemmF32Args a;
    memset(&a, 0, sizeof(a));
    a.A = A; a.sam = sam; a.sak = sak; a.B = B; a.sbk = sbk; a.sbn = sbn; a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K;
    a.bias = bias; a.epi = epi; a.ACT = ACT; a.ldact = ldact; a.accumulate = accumulate ? 1 : 0; a.kchunk = K; a.slab_stride = 0;
    a.brow_scale = brow_scale; a.orow_scale = orow_scale;
    {   // few rows (the encoder on the batch's images): K split + one reduction pass that carries the epilogue
        hipStream_t s_ = st ? st : m->stream;
        // (no_ksplit, iwae_eval_llh: the split depends on how many images a launch holds, and an image's estimate must not -- the evaluator's
        // encoder is 419 rows beside 2^21 decoder rows, nothing to gain there: test_eval_llh_images_per_launch_are_invisible)
        const int ns = no_ksplit ? 1 : gemm_f32_fewrows_split(m->opt.gemm_f32, M, N, K);
        if (ns > 1 && !brow_scale) {
            a.avec = a.bvec = 0;
            CHK(ensure(m->f32.kslab, (size_t)ns * M * N * 4, s_));
            launch_gemm_f32_fewrows(m->opt.gemm_f32, a, ptr<float>(m->f32.kslab), s_);
            HIPCHK(hipGetLastError());
            return IWAE_OK;
        }
    }
#ifdef IWAE_DENSE_STAMPS
    if (m->dstamp_epi == 12 && orow_scale && M >= 4096) {      // diagnostic (STAMPS=1 build, option dense_stamps_epi = 12): phase stamps of the output layer's dX product
        m->dstamp_waves = ((M + 63) / 64) * ((N + 223) / 224) * 4;
        CHK(ensure(m->dstamps, (size_t)m->dstamp_waves * 64, st ? st : m->stream));
        a.stamps = ptr<unsigned long long>(m->dstamps);
    }
#endif
    launch_gemm_f32(m->opt.gemm_f32, a, 1, st ? st : m->stream);
    HIPCHK(hipGetLastError());
    return IWAE_OK;
}
// DX (+)= (G W^T) * (1 - ACT^2)   (ACT = the stored tanh output of the layer below, or null)
// (rowscale: row r of G counts with weight rowscale[r] -- applied to the product's rows, in front of the tanh' factor)
int f32_dx(iwae_model* m, const KerasLayer& kl, const float* G, long ldg, int rows, float* DX, long lddx, const float* ACT, long ldact, bool accumulate,
           const float* rowscale = nullptr) {
    return f32_gemm(m, G, ldg, 1, m->param + kl.offW, 1, kl.Nout, DX, lddx, rows, kl.Kin, kl.Nout, nullptr, ACT ? GEMM_EPI_DTANH : GEMM_EPI_NONE, ACT, ldact, accumulate,
                    nullptr, rowscale);
}
// the queued slab sums of this step's float32 weight gradients, one launch per segment (f32_dw): seg 0 = the gradients made on the main stream,
// seg 1 = the decoder's, made on the side stream (backward_f32); seg < 0: whatever is queued, each segment on its own stream
int f32_flush_reductions(iwae_model* m, int seg = -1) {
    for (int sg = 0; sg < 2; ++sg) {
        if (seg >= 0 && sg != seg) continue;
        ReduceSlabsJobs jobs;
        memset(&jobs, 0, sizeof(jobs));
        for (const auto& p : m->f32_pending) {
            if (p.seg != sg) continue;
            ReduceSlabsJob& j = jobs.job[jobs.n++];
            j.slabs = ptr<float>(m->f32.slab) + p.off; j.stride = p.stride; j.n = p.n; j.out = p.out; j.nsplit = p.nsplit;
        }
        if (jobs.n > 0) {
            launch_reduce_slabs_multi_f32(jobs, sg == 1 ? m->side : m->stream);
            HIPCHK(hipGetLastError());
        }
    }
    if (seg < 0) m->f32_pending.clear();
    else m->f32_pending.erase(std::remove_if(m->f32_pending.begin(), m->f32_pending.end(), [seg](const iwae_model::F32Pending& p) { return p.seg == seg; }), m->f32_pending.end());
    if (m->f32_pending.empty()) m->f32_slab_used = 0;
    return IWAE_OK;
}
// grad W = X^T G, grad b = column sums of G: the row axis is split into fp32 slabs summed in a fixed order (deterministic)
// (rowscale: G's row r is multiplied by rowscale[r] as it is fetched -- the values the separate g_r s pass used to store)
int f32_dw(iwae_model* m, const KerasLayer& kl, const float* X, long ldx, const float* G, long ldg, int rows, const float* rowscale = nullptr, int seg = 0, int tile_mode = 0) {
    hipStream_t st = seg == 1 ? m->side : m->stream;
    // row splits: enough workgroups to fill the machine (~1 000 tiles of 64 x 64 or 128 x 128), at least 64 rows per split
    const int tiles = (int)gemm_f32_tiles(m->opt.gemm_f32, kl.Kin + 1, kl.Nout, tile_mode);      // (+ 1: the row of ones whose product row is the bias gradient)
    const int slots = std::min(m->opt.f32_dw_tiles, gemm_f32_slots(m->opt.gemm_f32, kl.Kin + 1, kl.Nout, tile_mode));
    int nsplit = std::max(1, std::min(std::min(256, rows / m->opt.f32_dw_min_rows), slots / tiles));      // (rounded DOWN: 1 027 workgroups on 1 024 slots are a second round of 3)
    while (nsplit > 8 && (tiles * nsplit) % 8 != 0) --nsplit;      // (a multiple of 8 workgroups: gemm_f32_v2_kernel then keeps a split's tiles on one XCD)
    const size_t nW = (size_t)kl.Kin * kl.Nout;
    // (round 5: the slabs of every gradient of the step stay until ONE reduction launch at the end of the backward pass; the buffer is sized for a
    // whole step -- a step that outgrows it falls back to the reduction per tensor, and the buffer grows for the next step)
    const size_t need = ((size_t)nsplit * (nW + kl.Nout) + 3) & ~(size_t)3;      // (a multiple of 4 floats: the next gradient's slabs stay 16-byte aligned)
    const bool queue = m->opt.allow_f32_multi_reduce && nsplit > 1 && (m->f32_slab_used + need) * 4 <= m->f32.slab.cap && m->f32_pending.size() + 2 <= REDUCE_SLABS_MAX_JOBS;
    if (!queue) {
        if (!m->f32_pending.empty()) CHK(f32_flush_reductions(m));      // (queued jobs still read the buffer ensure() may replace)
        if (m->f32_plan.side()) { HIPCHK(hipStreamSynchronize(m->side)); HIPCHK(hipStreamSynchronize(m->stream)); }      // (first steps only: the buffer is still growing)
        CHK(ensure(m->f32.slab, std::max(need, m->f32_slab_want) * 4, st));
    }
    m->f32_slab_want_step += need;
    float* slabW = ptr<float>(m->f32.slab) + (queue ? m->f32_slab_used : 0);
    float* slabB = slabW + (size_t)nsplit * nW;
    GemmF32Args a;
    memset(&a, 0, sizeof(a));
    a.A = X; a.sam = 1; a.sak = ldx; a.B = G; a.sbk = ldg; a.sbn = 1; a.M = kl.Kin; a.N = kl.Nout; a.K = rows;
    a.brow_scale = rowscale; a.tile_mode = tile_mode;
    a.kchunk = (rows + nsplit - 1) / nsplit; a.kchunk = (a.kchunk + 15) / 16 * 16;
    const int ns = (rows + a.kchunk - 1) / a.kchunk;
    // the bias gradient = the column sums of (weighted) G = the product row of a row of ONES appended to X^T (GemmF32Args.Cones): no pass of its own
    if (ns == 1) {
        a.C = m->grad + kl.offW; a.ldc = kl.Nout; a.slab_stride = 0; a.Cones = m->grad + kl.offb; a.cones_stride = 0;
        launch_gemm_f32(m->opt.gemm_f32, a, 1, st);
    } else {
        a.C = slabW; a.ldc = kl.Nout; a.slab_stride = nW; a.Cones = slabB; a.cones_stride = (size_t)kl.Nout;
#ifdef IWAE_DENSE_STAMPS
        if (m->dstamp_epi == 13 && rowscale) {      // diagnostic (STAMPS=1 build, option dense_stamps_epi = 13): phase stamps of the output layer's weight gradient
            m->dstamp_waves = ((kl.Kin + 1 + 223) / 224) * ((kl.Nout + 63) / 64) * ns * 4;
            CHK(ensure(m->dstamps, (size_t)m->dstamp_waves * 64, st));
            a.stamps = ptr<unsigned long long>(m->dstamps);
        }
#endif
        launch_gemm_f32(m->opt.gemm_f32, a, ns, st);
        if (queue) {
            m->f32_pending.push_back({(size_t)(slabW - ptr<float>(m->f32.slab)), nW, nW, m->grad + kl.offW, ns, seg});
            m->f32_pending.push_back({(size_t)(slabB - ptr<float>(m->f32.slab)), (size_t)kl.Nout, (size_t)kl.Nout, m->grad + kl.offb, ns, seg});
            m->f32_slab_used += need;
        } else {
            launch_reduce_slabs_f32(slabW, nW, ns, nW, m->grad + kl.offW, st);
            launch_reduce_slabs_f32(slabB, kl.Nout, ns, kl.Nout, m->grad + kl.offb, st);
            if (m->f32_plan.side()) { HIPCHK(hipStreamSynchronize(st)); }      // (the next unqueued gradient reuses the buffer's front from another stream)
        }
    }
    HIPCHK(hipGetLastError());
    return IWAE_OK;
}
// backward of a BasicBlock from dhead [R][2Dp] (d mu | d pre-exp): all four weight gradients, optionally dX [R][lddx]
int f32_block_bwd(iwae_model* m, int base, iwae_model::F32Block& w, const float* X, long ldx, int R, int Dp, float* dX, long lddx) {
    const KerasLayer *l1 = &m->klayers[base], *l2 = l1 + 1, *lmu = l1 + 2, *lsd = l1 + 3;
    const int H = l1->Nout;
    const float* dh = ptr<float>(w.dhead);
    CHK(ensure(w.d2, (size_t)R * H * 4, m->stream));
    CHK(ensure(w.d1, (size_t)R * H * 4, m->stream));
    CHK(f32_dw(m, *lmu, ptr<float>(w.h2), H, dh, 2 * Dp, R));
    CHK(f32_dw(m, *lsd, ptr<float>(w.h2), H, dh + Dp, 2 * Dp, R));
    CHK(f32_dx(m, *lmu, dh, 2 * Dp, R, ptr<float>(w.d2), H, ptr<float>(w.h2), H, false));
    CHK(f32_dx(m, *lsd, dh + Dp, 2 * Dp, R, ptr<float>(w.d2), H, ptr<float>(w.h2), H, true));
    CHK(f32_dw(m, *l2, ptr<float>(w.h1), H, ptr<float>(w.d2), H, R));
    CHK(f32_dx(m, *l2, ptr<float>(w.d2), H, R, ptr<float>(w.d1), H, ptr<float>(w.h1), H, false));
    CHK(f32_dw(m, *l1, X, ldx, ptr<float>(w.d1), H, R));
    if (dX) CHK(f32_dx(m, *l1, ptr<float>(w.d1), H, R, dX, lddx, nullptr, 0, false));
    return IWAE_OK;
}

// the masked step's output layer as masked_out_f32_kernel (the fused route): options, row count and the kernel's own predicate -- nothing of the staged input
bool masked_out_fused(const iwae_model* m, int M, int k) {
    const StepOptions& o = m->opt;
    const KerasLayer* d3 = &m->klayers[m->dec1[0].sub[0]] + 2;
    MaskedOutF32Args mo;
    memset(&mo, 0, sizeof(mo));
    mo.H = d3->Kin; mo.X = m->X; mo.k = k; mo.W3 = m->param + d3->offW; mo.b3 = m->param + d3->offb;
    return o.allow_masked_out_fused && M >= o.masked_out_min_rows && masked_out_f32_ok(mo);
}

// Which kernels a float32 call launches and on which streams, decided once from the options, the layer tables, the call's shape and the staged
// input xd.  As pure as plan_step: it touches no buffer, stream or event and fills p in place.  forward_f32 calls it behind stage_input:
// dec_fwd_f32_ok also asks for the alignment of x, and a caller's device pointer is read in place.
// A masked call (maskd: the staged mask; xd is then xin = m ? x : 0): always the three GEMM launches for the tanh layers and a stored s; the
// output layer is masked_out_f32_kernel where the options and its predicate allow (the fast route), else the logits GEMM + the masked passes.
void plan_step_f32(const iwae_model* m, int B, int k, int objective, bool bwd, const FwdCall& call, const iwae_tensors* want, const float* xd, const uint8_t* maskd, F32Plan& p) {
    const StepOptions& o = m->opt;
    const bool two = m->cfg.n_layers == 2, want_logits = want && want->logits;
    const int M = B * k, X = m->X;
    const int b_dec1 = m->dec1[0].sub[0];
    const KerasLayer *d1 = &m->klayers[b_dec1], *d2 = d1 + 1, *d3 = d1 + 2;
    p = F32Plan();
    p.x = xd;
    p.mask = maskd;
    p.want_dreg = !two && (objective == OBJ_DREG || (!bwd && !call.log_w_only));
    p.lme_only = !bwd && call.log_w_only && !want;
    // ---- the decoder forward
    // Round 4: the whole decoder forward in ONE launch where its shapes fit (dec_fwd_f32_kernel: rows stationary, activations in LDS, the
    // weights streamed from the float32 master parameters; log p(x|z) per row comes out whole) -- the k = 5000 evaluator's three GEMM launches
    // ran at 0.35 of the f32 MFMA peak between them.  A training step also keeps g1, g2 and s = x - sigmoid(l) for the backward pass.
    DecFwdF32Args df;      // (what dec_fwd_f32_ok reads: widths, k and the alignment of the weights and of x; forward_f32 fills the launch's own block)
    memset(&df, 0, sizeof(df));
    df.Din = m->D[0] + m->C; df.H = d1->Nout; df.X = X; df.k = k; df.XB = xd;
    df.W1 = m->param + d1->offW; df.b1 = m->param + d1->offb; df.W2 = m->param + d2->offW; df.b2 = m->param + d2->offb;
    df.W3 = m->param + d3->offW; df.b3 = m->param + d3->offb;
    // (round 5: a TRAINING step takes the three GEMM launches again -- with gemm_f32_v2_kernel they are faster than the fused kernel once g1, g2 and s
    // have to be stored anyway: 1.280 -> 1.248 ms; option f32_dec_fused_train = 1 for the fused kernel)
    const bool fused_dec = o.allow_f32_dec_fused && (!bwd || o.f32_dec_fused_train) && !want_logits && M >= 4096 && dec_fwd_f32_ok(df);
    // forward-only calls at large row counts (the k = 5000 evaluator): log p(x|z) in the epilogue of the output layer's GEMM -- the float32
    // logits (1.6 GB per launch of 2^19 rows) are neither written nor read back; per 64-column half tile a partial sum that lse_kernel adds
    // Round 3, training step: the same epilogue also leaves s = x - sigmoid(l) where the logits would have gone -- the backward pass reads s and
    // takes the row weight g_r inside its two consumers (f32_dw / f32_dx with rowscale) instead of a pass that rewrites 160 MB into dl = g_r s.
    const bool fuse_bern = !fused_dec && o.allow_f32_bern_fused && !want_logits && gemm_f32_takes_big(M, X, 1);
    p.dec_fwd = fused_dec ? F32_DEC_ONE_LAUNCH : F32_DEC_GEMMS;
    p.px_from = fused_dec ? F32_PX_DEC_KERNEL : fuse_bern ? F32_PX_GEMM_EPILOGUE : F32_PX_BERN_PASS;
    if (fuse_bern) p.px_parts = 2 * ((X + 127) / 128);
    p.keeps_s = bwd && (fused_dec || fuse_bern);
    if (maskd) {      // (never F32_DEC_ONE_LAUNCH / F32_PX_GEMM_EPILOGUE: neither kernel knows the mask; never dl_f32_kernel: it reads x at every pixel)
        const bool fast = masked_out_fused(m, M, k);
        p.dec_fwd = F32_DEC_GEMMS;
        p.px_from = fast ? F32_PX_MASKED_OUT : F32_PX_MASKED_PASS;
        p.px_parts = 1;
        p.keeps_s = bwd;
    }
    if (!bwd) return;
    // ---- the backward pass: where and in which order the decoder's three weight gradients are enqueued
    // (the conditional prior's block sits BEHIND the decoder in the flat parameters: its gradient is made on the main stream -- one stream for that model)
    const bool use_side = o.allow_f32_side && m->side && !m->has_prior && M >= 4096 && b_dec1 + 3 == (int)m->klayers.size();
    const bool dw_last = use_side && o.f32_dw_last > 0;      // option: every decoder weight gradient behind the dX chain, beside the main stream's few-row tail
    p.dw_order = !use_side ? F32_DW_ONE_STREAM : dw_last ? F32_DW_BEHIND_DX : o.f32_wout_first ? F32_DW_WOUT_FIRST : F32_DW_WOUT_LAST;
    if (dw_last) p.dw_tile_mode = o.f32_dw_last - 1;      // (1: tiles as picked, 2: 4-wave tiles, 3: 4-wave tiles at 3 waves per SIMD)
}

}  // namespace

// Y = epi(X W + b), W = the Keras kernel [in, out] of layer kl inside the flat float32 parameters
int f32_fwd(iwae_model* m, const KerasLayer& kl, const float* X, long ldx, int rows, float* Y, long ldy, int epi, bool no_ksplit) {
    return f32_gemm(m, X, ldx, 1, m->param + kl.offW, kl.Nout, 1, Y, ldy, rows, kl.Nout, kl.Kin, m->param + kl.offb, epi, nullptr, 0, false, nullptr, nullptr, nullptr, no_ksplit);
}
// BasicBlock (iwae1.py:36-44) on R rows: X [R][ldx] -> h1, h2 [R][H], head [R][2Dp] (mu at 0.., sigma = exp(.)+1e-6 at Dp..)
int f32_block_fwd(iwae_model* m, int base, iwae_model::F32Block& w, const float* X, long ldx, int R, float* head, int Dp, bool no_ksplit) {
    const KerasLayer *l1 = &m->klayers[base], *l2 = l1 + 1, *lmu = l1 + 2, *lsd = l1 + 3;
    const int H = l1->Nout;
    CHK(ensure(w.h1, (size_t)R * H * 4, m->stream));
    CHK(ensure(w.h2, (size_t)R * H * 4, m->stream));
    CHK(f32_fwd(m, *l1, X, ldx, R, ptr<float>(w.h1), H, GEMM_EPI_TANH, no_ksplit));
    CHK(f32_fwd(m, *l2, ptr<float>(w.h1), H, R, ptr<float>(w.h2), H, GEMM_EPI_TANH, no_ksplit));
    CHK(f32_fwd(m, *lmu, ptr<float>(w.h2), H, R, head, 2 * Dp, GEMM_EPI_NONE, no_ksplit));
    CHK(f32_fwd(m, *lsd, ptr<float>(w.h2), H, R, head + Dp, 2 * Dp, GEMM_EPI_EXP, no_ksplit));
    return IWAE_OK;
}

int forward_f32(iwae_model* m, const float* x, int B, int k, float beta, const float* eps, int objective, bool bwd, const iwae_tensors* want,
                const FwdCall& call) {
    const float* cond;      // conditional models (tasks/task05.py, tasks/task04.py): y of these images
    CHK(begin_forward(m, x, B, k, beta, call, &cond));
    const bool two = m->cfg.n_layers == 2, nks = call.no_ksplit;
    m->time_this = false;
    const int M = m->M, Mp = m->Mp, Bp = m->Bp, X = m->X;
    hipStream_t st = m->stream;
    if (m->bf16_side_used) {      // a bf16 call's deferred update / speculative draw may sit on either side stream
        CHK(join_side(m));
        if (m->side) HIPCHK(hipStreamSynchronize(m->side));
        if (m->side2) HIPCHK(hipStreamSynchronize(m->side2));
        m->bf16_side_used = false;
    }
    // (a float32 step's own deferred decoder update is joined in front of the decoder forward: the encoder and the sampling run beside it)
    m->user_eps = eps != nullptr;
    m->epsc_ptr[0] = m->epsc_ptr[1] = nullptr;
    if (!eps) {       // the step's draws, kept for the backward pass and the 2-layer densities (same generator as the bf16 path)
        const int np = (m->epsc_par + 1) % 3;
        CHK(draw_eps(m, np, m->noise_step, M, st));
        if (call.k_total > 0) m->eps_tag[np].valid = false;      // a k-chunk's draws: the tag (step, offset, rows) does not describe them
        if (bwd) m->epsc_par = np;      // (forward-only calls reuse one slot, as in forward_impl)
        for (int l = 0; l < m->cfg.n_layers; ++l) m->epsc_ptr[l] = ptr<float>(m->epsc[np][l]);
    } else {
        CHK(copy_in(m, m->epsbuf, eps, (size_t)M * (m->D[0] + (two ? m->D[1] : 0)) * 4));
    }
    const float* xd;
    const uint8_t* maskd = nullptr;
    bool xcode_staged = false;
    if (call.mask_resident) {      // the masked step from the resident set: xin, the mask bytes and, on the fused route, the hole-coded rows, one launch
        CHK(ensure(m->f32.xmask, (size_t)B * X * 4, st));
        CHK(ensure(m->f32.mask, (size_t)B * X, st));
        MaskedStage ms;
        ms.xin = ptr<float>(m->f32.xmask); ms.mask = ptr<uint8_t>(m->f32.mask);
        if (masked_out_fused(m, M, k)) {
            CHK(ensure(m->f32.xcode, (size_t)B * X * 4, st));
            ms.xcode = ptr<float>(m->f32.xcode);
            xcode_staged = true;
        }
        m->time_this = m->timing > 0;
        const int rc = stage_input(m, x, B, true, &xd, &ms);
        m->time_this = false;
        CHK(rc);
        maskd = ms.mask;
    } else CHK(stage_input(m, x, B, true, &xd));
    if (call.mask) {      // the masked step: xin = m ? x : 0 is the call's x from here on (the encoder, and the backward pass's encoder weight gradient)
        CHK(staged_in(m, call.mask, m->f32.mask, (size_t)B * m->X, &maskd));
        CHK(ensure(m->f32.xmask, (size_t)B * m->X * 4, m->stream));
        launch_impute_mask(xd, maskd, (long)B * m->X, ptr<float>(m->f32.xmask), m->stream);
        xd = ptr<float>(m->f32.xmask);
    }
    plan_step_f32(m, B, k, objective, bwd, call, want, xd, maskd, m->f32_plan);
    const F32Plan& p = m->f32_plan;
    // ---- encoder on the images (conditional models: on concat(x, y), tasks/task05.py:113-118)
    const int b_enc1 = m->enc1[0].sub[0];
    CHK(ensure(m->wenc1.head, (size_t)Bp * 2 * m->Dp[0] * 4, st));
    const float* xenc = xd;
    if (m->C > 0) {
        CHK(ensure(m->f32.xcat, (size_t)B * (X + m->C) * 4, st));
        launch_concat_f32(xd, X, cond, m->C, B, ptr<float>(m->f32.xcat), st);
        xenc = ptr<float>(m->f32.xcat);
    }
    CHK(f32_block_fwd(m, b_enc1, m->f32.enc1, xenc, X + m->C, B, ptr<float>(m->wenc1.head), m->Dp[0], nks));
    if (m->has_prior) {     // p(z|y) = N(mu_p(y), sigma_p(y)): the prior block on the B condition rows (tasks/task04.py:108,124)
        CHK(ensure(m->wprior.head, (size_t)Bp * 2 * m->Dp[0] * 4, st));
        CHK(f32_block_fwd(m, m->prior[0].sub[0], m->f32.prior, cond, m->C, B, ptr<float>(m->wprior.head), m->Dp[0], nks));
    }
    for (int i = 0; i < 6; ++i) CHK(ensure(m->rows[i], (size_t)Mp * 4, st));
    float* lpxz = ptr<float>(m->rows[0]);
    float* t1 = ptr<float>(m->rows[1]);
    float* t2 = ptr<float>(m->rows[2]);
    float* t3 = ptr<float>(m->rows[3]);
    float* t4 = ptr<float>(m->rows[4]);
    float* lqd = ptr<float>(m->rows[5]);
    // ---- z (z1) = mu + sigma*eps and its densities (iwae1.py:59,107,109)
    const int Dz = m->D[0] + m->C;      // row width of the decoder's input: z, or concat(z, y) (tasks/task05.py:185)
    if (m->left.z_pending) {      // the previous step's gradient of the decoder's first layer reads z on the side stream
        HIPCHK(hipStreamWaitEvent(st, m->ev_join, 0));
        m->left.z_pending = false;
    }
    CHK(ensure(m->f32.z[0], (size_t)Mp * Dz * 4, st));
    {
        SampleArgs s;
        memset(&s, 0, sizeof(s));
        s.head = ptr<float>(m->wenc1.head); s.ldH = 2 * m->Dp[0]; s.Dp = m->Dp[0]; s.D = m->D[0]; s.head_per_row = 0;
        s.M = M; s.Mp = Mp; s.k = k; s.B = B; s.eps = eps_src(m, 0);
        s.ZP = nullptr; s.ZF = ptr<float>(m->f32.z[0]); s.ldZF = Dz;
        s.cond = cond; s.C = m->C;      // (the sampling kernel writes y into features D .. D + C - 1 of every row)
        s.prior_head = m->has_prior ? ptr<float>(m->wprior.head) : nullptr;
        s.lp_prior = two ? nullptr : t1;
        s.lq = two ? t3 : t2;
        s.lq_dreg = p.want_dreg ? lqd : nullptr;
        launch_sample(s, st);
    }
    if (two) {       // q(z2|z1), z2, p(z1|z2)  (iwae2.py:63-65, :90, :118-124)
        const int b_enc2 = m->enc2[0].sub[0], b_dec2 = m->dec2[0].sub[0];
        CHK(ensure(m->wenc2.head, (size_t)Mp * 2 * m->Dp[1] * 4, st));
        CHK(f32_block_fwd(m, b_enc2, m->f32.enc2, ptr<float>(m->f32.z[0]), m->D[0], M, ptr<float>(m->wenc2.head), m->Dp[1], nks));
        CHK(ensure(m->f32.z[1], (size_t)Mp * m->D[1] * 4, st));
        SampleArgs s;
        memset(&s, 0, sizeof(s));
        s.head = ptr<float>(m->wenc2.head); s.ldH = 2 * m->Dp[1]; s.Dp = m->Dp[1]; s.D = m->D[1]; s.head_per_row = 1;
        s.M = M; s.Mp = Mp; s.k = k; s.B = B; s.eps = eps_src(m, 1);
        s.ZP = nullptr; s.ZF = ptr<float>(m->f32.z[1]); s.ldZF = m->D[1];
        s.lp_prior = t2; s.lq = t4; s.lq_dreg = nullptr;
        launch_sample(s, st);
        CHK(ensure(m->wdec2.head, (size_t)Mp * 2 * m->Dp[0] * 4, st));
        CHK(f32_block_fwd(m, b_dec2, m->f32.dec2, ptr<float>(m->f32.z[1]), m->D[1], M, ptr<float>(m->wdec2.head), m->Dp[0], nks));
        GaussLpArgs g;
        memset(&g, 0, sizeof(g));
        g.zhead = ptr<float>(m->wenc1.head); g.ldZH = 2 * m->Dp[0]; g.Dzp = m->Dp[0];
        g.phead = ptr<float>(m->wdec2.head); g.ldPH = 2 * m->Dp[0]; g.Dpp = m->Dp[0];
        g.D = m->D[0]; g.M = M; g.k = k; g.eps = eps_src(m, 0); g.out = t1;
        launch_gauss_lp(g, st);
    }
    // ---- decoder + Bernoulli log-likelihood (iwae1.py:81-83,111)
    const int b_dec1 = m->dec1[0].sub[0];
    const KerasLayer *d1 = &m->klayers[b_dec1], *d2 = d1 + 1, *d3 = d1 + 2;
    const int H = d1->Nout;
    CHK(join_side(m));      // the decoder's parameters (and g1, g2, s, which the previous step's weight gradients still read)
    // (one launch or three, and who makes log p(x|z): plan_step_f32)
    if (bwd || p.dec_fwd == F32_DEC_GEMMS) {
        CHK(ensure(m->f32.g1, (size_t)M * H * 4, st));
        CHK(ensure(m->f32.g2, (size_t)M * H * 4, st));
    }
    if (p.dec_fwd == F32_DEC_ONE_LAUNCH) {
        DecFwdF32Args df;
        memset(&df, 0, sizeof(df));
        df.Z = ptr<float>(m->f32.z[0]); df.ldz = Dz; df.Din = Dz; df.M = M; df.H = H; df.X = X;
        df.W1 = m->param + d1->offW; df.b1 = m->param + d1->offb; df.W2 = m->param + d2->offW; df.b2 = m->param + d2->offb;
        df.W3 = m->param + d3->offW; df.b3 = m->param + d3->offb;
        df.XB = xd; df.k = k; df.lpxz = lpxz; df.zero = m->d_zero; df.ldg = H; df.ldS = X;
        if (bwd) {
            CHK(ensure(m->f32.logits, (size_t)M * X * 4, st));
            df.G1 = ptr<float>(m->f32.g1); df.G2 = ptr<float>(m->f32.g2); df.S = ptr<float>(m->f32.logits);
        }
#ifdef IWAE_DENSE_STAMPS
        if (m->dstamp_epi == 11) {      // diagnostic (STAMPS=1 build, option dense_stamps_epi = 11): phase stamps of dec_fwd_f32_kernel
            m->dstamp_waves = ((M + 63) / 64) * 4;
            CHK(ensure(m->dstamps, (size_t)m->dstamp_waves * 64, st));
            df.stamps = ptr<unsigned long long>(m->dstamps);
        }
#endif
        launch_dec_fwd_f32(df, st);
    } else {
    CHK(f32_fwd(m, *d1, ptr<float>(m->f32.z[0]), Dz, M, ptr<float>(m->f32.g1), H, GEMM_EPI_TANH, nks));
    CHK(f32_fwd(m, *d2, ptr<float>(m->f32.g1), H, M, ptr<float>(m->f32.g2), H, GEMM_EPI_TANH, nks));
    if (p.px_from == F32_PX_GEMM_EPILOGUE) {
        CHK(ensure(m->px_part, (size_t)p.px_parts * Mp * 4, st));
        GemmF32Args ga;
        memset(&ga, 0, sizeof(ga));
        ga.A = ptr<float>(m->f32.g2); ga.sam = H; ga.sak = 1; ga.B = m->param + d3->offW; ga.sbk = d3->Nout; ga.sbn = 1; ga.M = M; ga.N = X; ga.K = H;
        ga.bias = m->param + d3->offb; ga.epi = GEMM_EPI_BERN; ga.kchunk = H;
        if (bwd) {      // (p.keeps_s)
            CHK(ensure(m->f32.logits, (size_t)M * X * 4, st));
            ga.C = ptr<float>(m->f32.logits); ga.ldc = X;
        }
        ga.XB = xd; ga.bern_k = k; ga.bern_X = X; ga.part = ptr<float>(m->px_part); ga.part_stride = (size_t)Mp;
        launch_gemm_f32(m->opt.gemm_f32, ga, 1, st);
    } else if (p.px_from == F32_PX_MASKED_OUT) {      // the masked step's fast route: no logits in memory, s stored once (training calls only)
        CHK(ensure(m->f32.xcode, (size_t)B * X * 4, st));
        if (!xcode_staged) launch_masked_code(xd, p.mask, (long)B * X, ptr<float>(m->f32.xcode), st);      // (a resident batch: stage_input wrote them)
        MaskedOutF32Args mo;
        memset(&mo, 0, sizeof(mo));
        mo.G2 = ptr<float>(m->f32.g2); mo.ldg = H; mo.M = M; mo.H = H; mo.X = X;
        mo.W3 = m->param + d3->offW; mo.b3 = m->param + d3->offb; mo.XC = ptr<float>(m->f32.xcode); mo.k = k;
        mo.lpxz = lpxz; mo.zero = m->d_zero;
        {   // (the K split f32_fwd would give the output layer's GEMM on the general route: the kernel's logits are that route's, bit for bit)
            const int ns = nks ? 1 : gemm_f32_fewrows_split(m->opt.gemm_f32, M, X, H);
            if (ns > 1) mo.kslabs = ((H + ns - 1) / ns + 15) / 16;
        }
        if (bwd) {      // (p.keeps_s)
            CHK(ensure(m->f32.logits, (size_t)M * X * 4, st));
            mo.S = ptr<float>(m->f32.logits); mo.ldS = X;
        }
        m->time_this = m->timing > 0;
        {
            ScopedTimer tm(m, T_MASKED_OUT, st);
            launch_masked_out_f32(mo, st);
        }
        m->time_this = false;
    } else {
    CHK(ensure(m->f32.logits, (size_t)M * X * 4, st));
    CHK(f32_fwd(m, *d3, ptr<float>(m->f32.g2), H, M, ptr<float>(m->f32.logits), X, GEMM_EPI_NONE, nks));
    if (p.px_from == F32_PX_MASKED_PASS) {      // the masked step's general route
        launch_masked_bern_f32(ptr<float>(m->f32.logits), X, xd, p.mask, X, M, k, lpxz, st);
        if (bwd) launch_masked_s_f32(ptr<float>(m->f32.logits), X, xd, p.mask, X, M, k, st);      // (p.keeps_s: the logits become s in place)
    } else launch_bern_f32(ptr<float>(m->f32.logits), X, xd, X, M, k, lpxz, st);
    }
    }      // (F32_DEC_GEMMS)
    if (want && want->logits) {      // reference [k,B,X] order
        CHK(ensure(m->scratch, (size_t)M * X * 4, st));
        launch_export_mat(ptr<float>(m->f32.logits), B, k, X, ptr<float>(m->scratch), st);
        CHK(copy_out(m, want->logits, m->scratch.p, (size_t)M * X * 4));
    }
    // ---- log_w, log-mean-exp over k, objectives (iwae1.py:113-139): the shared kernel
    CHK(ensure(m->logw, (size_t)Mp * 4, st));
    CHK(ensure(m->wn, (size_t)Mp * 4, st));
    {   // (as forward_impl: wgrad_rows_kernel's row-weighted path reads gx in whole 32-row stages -- 0 x a non-finite pad would be NaN)
        const void* before = m->gx.p;
        CHK(ensure(m->gx, (size_t)Mp * 4, st));
        if (m->gx.p != before) HIPCHK(hipMemsetAsync(m->gx.p, 0, m->gx.cap, st));
    }
    CHK(ensure(m->cf, (size_t)Mp * 16, st));
    CHK(ensure(m->per_b, (size_t)PB_COUNT * B * 4, st));
    {
        LseArgs a;
        memset(&a, 0, sizeof(a));
        if (!two) {
            a.term[0] = lpxz; a.coef[0] = 1.f; a.term[1] = t1; a.coef[1] = beta; a.term[2] = t2; a.coef[2] = -beta;
            a.head = ptr<float>(m->wenc1.head); a.ldH = 2 * m->Dp[0]; a.D = m->D[0]; a.Dp = m->Dp[0]; a.cz_on = 1.f;
        } else {
            a.term[0] = lpxz; a.coef[0] = 1.f; a.term[1] = t1; a.coef[1] = 1.f; a.term[2] = t2; a.coef[2] = 1.f;
            a.term[3] = t3; a.coef[3] = -1.f; a.term[4] = t4; a.coef[4] = -1.f; a.head = nullptr; a.cz_on = 0.f;
        }
        a.lq_dreg = p.want_dreg ? lqd : nullptr;
        a.B = B; a.k = k; a.beta = two ? 1.f : beta; a.objective = objective;
        a.lme_only = p.lme_only ? 1 : 0;
        a.logw = ptr<float>(m->logw); a.wn = ptr<float>(m->wn); a.gx = ptr<float>(m->gx);
        a.cf = ptr<float4>(m->cf); a.per_b = ptr<float>(m->per_b);
        a.n_px_part = p.px_parts; a.px_stride = (size_t)Mp; a.term0_out = lpxz;
        if (p.px_parts > 1) a.term[0] = ptr<float>(m->px_part);      // (the fused Bernoulli epilogue's per-half-tile partial sums)
        launch_lse(a, st);
        launch_scalars(ptr<float>(m->per_b), B, two ? 1.f : beta, m->d_scalars, st);
    }
    HIPCHK(hipGetLastError());
    m->have_forward = true;
    m->fwd_was_f32 = true;
    return IWAE_OK;
}

// closed-form backward in float32: leaves the flat gradient in m->grad
// Round 5: two streams.  The decoder's three weight gradients (58 % of the backward pass's FLOPs, needed by nobody until the update) go to the
// side stream: the hidden layers' behind the dX product that makes their operand, the output layer's LAST -- it needs only s, g2 and the
// row weights, so it is what runs beside the main stream's few-row tail (dz, the latent sums, the encoder's seven launches on the batch's
// images: 64 workgroups each on 256 CUs).  END_UPDATE (the single-GPU train step): the update is part of it -- the encoder's
// layers on the main stream, the decoder's on the side stream behind its own slab reduction, DEFERRED: the next step's encoder forward
// and sampling run beside the output layer's gradient, and forward_f32 joins (ev_dec) in front of the decoder forward.
// (end: END_GRAD or END_UPDATE; this path leaves no segment of the gradient unjoined for a caller, so the split ends are END_GRAD)
int backward_f32(iwae_model* m, int objective, StepEnd end, float lr) {
    const bool update = end == END_UPDATE;
    m->f32_slab_want_step = 0;
    if (!m->have_forward || !m->fwd_was_f32) return fail(IWAE_ERR_STATE, "backward without a float32 forward");
    const bool two = m->cfg.n_layers == 2;
    const int B = m->B, k = m->k, M = m->M, Mp = m->Mp, X = m->X;
    hipStream_t st = m->stream;
    const int b_dec1 = m->dec1[0].sub[0];
    const KerasLayer *d1 = &m->klayers[b_dec1], *d2 = d1 + 1, *d3 = d1 + 2;
    const int H = d1->Nout, D0 = m->D[0], Dp0 = m->Dp[0];
    const F32Plan& p = m->f32_plan;
    float* dl = ptr<float>(m->f32.logits);
    const float* rw = nullptr;      // the row weight g_r, where the forward pass kept s instead of the logits (forward_f32): taken by the two consumers
    if (p.keeps_s) rw = ptr<float>(m->gx);
    else launch_dl_f32(dl, X, p.x, X, M, k, ptr<float>(m->gx), st);        // dl = g_r (x - sigmoid(l)), in place
    CHK(ensure(m->f32.d2, (size_t)M * H * 4, st));
    CHK(ensure(m->f32.d1, (size_t)M * H * 4, st));
    CHK(ensure(m->wdec1.dz, (size_t)Mp * Dp0 * 4, st));
    if (m->descs_dirty) CHK(build_descs(m));
    // ---- the decoder: the dX chain on the main stream, each layer's weight gradient where the plan's order puts it
    const int tm = p.dw_tile_mode;
    auto dx3 = [&]() { return f32_dx(m, *d3, dl, X, M, ptr<float>(m->f32.d2), H, ptr<float>(m->f32.g2), H, false, rw); };
    auto dx2 = [&]() { return f32_dx(m, *d2, ptr<float>(m->f32.d2), H, M, ptr<float>(m->f32.d1), H, ptr<float>(m->f32.g1), H, false); };
    auto dx1 = [&]() { return f32_dx(m, *d1, ptr<float>(m->f32.d1), H, M, ptr<float>(m->wdec1.dz), Dp0, nullptr, 0, false); };
    auto dw3 = [&](int seg) { return f32_dw(m, *d3, ptr<float>(m->f32.g2), H, dl, X, M, rw, seg, tm); };      // (seg 1: on the side stream)
    auto dw2 = [&](int seg) { return f32_dw(m, *d2, ptr<float>(m->f32.g1), H, ptr<float>(m->f32.d2), H, M, nullptr, seg, tm); };
    auto dw1 = [&](int seg) { return f32_dw(m, *d1, ptr<float>(m->f32.z[0]), D0 + m->C, ptr<float>(m->f32.d1), H, M, nullptr, seg, tm); };
    auto fork = [&](hipEvent_t ev) {      // the side stream goes on behind what the main stream has enqueued so far
        HIPCHK(hipEventRecord(ev, st));
        HIPCHK(hipStreamWaitEvent(m->side, ev, 0));
        return (int)IWAE_OK;
    };
    auto z_free = [&]() { HIPCHK(hipEventRecord(m->ev_join, m->side)); return (int)IWAE_OK; };      // (behind dw1, z's last reader: z is free for the next step's sampling -- StepLeft::z_pending)
    switch (p.dw_order) {
    case F32_DW_ONE_STREAM:
        CHK(dw3(0)); CHK(dx3()); CHK(dw2(0)); CHK(dx2()); CHK(dw1(0)); CHK(dx1());
        break;
    case F32_DW_WOUT_FIRST:
        CHK(fork(m->ev_fork));      // s, g1, g2, z, the row weights
        CHK(dw3(1)); CHK(dx3());
        CHK(fork(m->ev_fork2)); CHK(dw2(1)); CHK(dx2());
        CHK(fork(m->ev_blk)); CHK(dw1(1)); CHK(z_free());
        CHK(dx1());
        break;
    case F32_DW_WOUT_LAST:
        CHK(fork(m->ev_fork));
        CHK(dx3());
        CHK(fork(m->ev_fork2)); CHK(dw2(1)); CHK(dx2());
        CHK(fork(m->ev_blk)); CHK(dw1(1)); CHK(z_free()); CHK(dw3(1));
        CHK(dx1());
        break;
    case F32_DW_BEHIND_DX:      // (in the plan's tile mode)
        CHK(fork(m->ev_fork));
        CHK(dx3()); CHK(dx2()); CHK(dx1());
        CHK(fork(m->ev_blk)); CHK(dw1(1)); CHK(z_free()); CHK(dw2(1)); CHK(dw3(1));
        break;
    }
    const float *dz1_b = nullptr, *dz1_c = nullptr;
    if (two) {
        const int b_enc2 = m->enc2[0].sub[0], b_dec2 = m->dec2[0].sub[0];
        const int Dp1 = m->Dp[1];
        CHK(ensure(m->dzdir, (size_t)Mp * Dp0 * 4, st));
        CHK(ensure(m->f32.dec2.dhead, (size_t)Mp * 2 * Dp0 * 4, st));
        CHK(ensure(m->f32.dec2.dx, (size_t)Mp * Dp1 * 4, st));
        CHK(ensure(m->f32.enc2.dhead, (size_t)Mp * 2 * Dp1 * 4, st));
        CHK(ensure(m->f32.enc2.dx, (size_t)Mp * Dp0 * 4, st));
        HIPCHK(hipMemsetAsync(m->f32.dec2.dhead.p, 0, (size_t)Mp * 2 * Dp0 * 4, st));      // (pad columns are read by the weight-gradient GEMMs' strided views: keep them zero)
        HIPCHK(hipMemsetAsync(m->f32.enc2.dhead.p, 0, (size_t)Mp * 2 * Dp1 * 4, st));
        GaussBwdArgs g;
        memset(&g, 0, sizeof(g));
        g.mode = 0; g.G = ptr<float>(m->gx);
        g.head = ptr<float>(m->wdec2.head); g.ldH = 2 * Dp0; g.D = D0; g.Dp = Dp0;
        g.zhead = ptr<float>(m->wenc1.head); g.ldZH = 2 * Dp0; g.Dzp = Dp0;
        g.dz_direct = ptr<float>(m->dzdir); g.ldDZ = Dp0;
        g.eps = eps_src(m, 0); g.M = M; g.Mp = Mp; g.k = k;
        g.DHP = nullptr; g.DHF = ptr<float>(m->f32.dec2.dhead);
        launch_gauss_bwd(g, st);
        CHK(f32_block_bwd(m, b_dec2, m->f32.dec2, ptr<float>(m->f32.z[1]), m->D[1], M, Dp0, ptr<float>(m->f32.dec2.dx), Dp1));
        memset(&g, 0, sizeof(g));
        g.mode = 1; g.G = ptr<float>(m->gx);
        g.head = ptr<float>(m->wenc2.head); g.ldH = 2 * Dp1; g.D = m->D[1]; g.Dp = Dp1;
        g.dz_in = ptr<float>(m->f32.dec2.dx); g.ldDZ = Dp1;
        g.eps = eps_src(m, 1); g.M = M; g.Mp = Mp; g.k = k;
        g.DHP = nullptr; g.DHF = ptr<float>(m->f32.enc2.dhead);
        launch_gauss_bwd(g, st);
        CHK(f32_block_bwd(m, b_enc2, m->f32.enc2, ptr<float>(m->f32.z[0]), D0, M, Dp1, ptr<float>(m->f32.enc2.dx), Dp0));
        dz1_b = ptr<float>(m->dzdir); dz1_c = ptr<float>(m->f32.enc2.dx);
    }
    {
        CHK(ensure(m->f32.enc1.dhead, (size_t)m->Bp * 2 * Dp0 * 4, st));
        HIPCHK(hipMemsetAsync(m->f32.enc1.dhead.p, 0, (size_t)m->Bp * 2 * Dp0 * 4, st));
        LatentBwdArgs a;
        memset(&a, 0, sizeof(a));
        a.dz = ptr<float>(m->wdec1.dz); a.dz2 = dz1_b; a.dz3 = dz1_c; a.ldDZ = Dp0;
        a.head = ptr<float>(m->wenc1.head); a.ldH = 2 * Dp0; a.D = D0; a.Dp = Dp0;
        a.cf = ptr<float4>(m->cf); a.eps = eps_src(m, 0);
        a.B = B; a.Bp = m->Bp; a.k = k;
        a.kmu = a.ksig = (objective == OBJ_VAE_ELBO_KL) ? m->beta / (float)B : 0.f;
        a.DHP = nullptr; a.DHF = ptr<float>(m->f32.enc1.dhead);
        if (m->has_prior) {      // gradient of the conditional prior's head, summed over the image's samples (tasks/task04.py:124-130)
            CHK(ensure(m->f32.prior.dhead, (size_t)m->Bp * 2 * Dp0 * 4, st));
            HIPCHK(hipMemsetAsync(m->f32.prior.dhead.p, 0, (size_t)m->Bp * 2 * Dp0 * 4, st));
            a.prior_head = ptr<float>(m->wprior.head); a.DHF2 = ptr<float>(m->f32.prior.dhead);
        }
        launch_latent_bwd(a, st);
    }
    if (m->has_prior)
        CHK(f32_block_bwd(m, m->prior[0].sub[0], m->f32.prior, ptr<float>(m->cond) + (size_t)m->call.cond_row0 * m->C, m->C, B, Dp0, nullptr, 0));
    CHK(f32_block_bwd(m, m->enc1[0].sub[0], m->f32.enc1, m->C > 0 ? ptr<float>(m->f32.xcat) : p.x, X + m->C, B, Dp0, nullptr, 0));
    m->f32_slab_want = std::max(m->f32_slab_want, m->f32_slab_want_step);
    // what the step leaves: nothing for a caller's own all-reduce (split_offset = n: the data-parallel step exchanges the whole gradient at once);
    // with the side stream, the decoder's sums [+ update] there (join_side: whoever reads the decoder's gradient or parameters next)
    m->left = StepLeft{p.side(), false, BlockRange(), m->nparam, ON_SIDE, p.side()};
    if (!p.side()) {
        CHK(f32_flush_reductions(m));      // every row-split gradient's slabs -> the flat gradient, one launch
        if (update) CHK(adam_impl(m, lr, 1.0f));
        HIPCHK(hipGetLastError());
        return IWAE_OK;
    }
    const int b0 = m->tb.dec1.e;
    const float alpha = update ? adam_alpha(m, lr) : 0.0f;
    CHK(f32_flush_reductions(m, 0));       // the slabs of the main stream's gradients (every block but the decoder)
    // (the decoder's update rewrites W1 .. W3, which the main stream's dX chain reads, and only F32_DW_BEHIND_DX puts the side stream's work behind
    // that chain: the update waits for the encoder's, the main stream's last launch of the step.  ev_fork2 is free again by now and rides on that
    // launch's dispatch packet -- no record on the main stream.  Without the wait a side stream that the host had just waited for (f32_dw while the
    // slab buffer grows) ran the update beside the dX product of the decoder's first layer: the fused end then missed the other ends by rounding)
    if (update) adam_blocks(m, st, 0, b0, alpha, 1.0f, m->ev_fork2);
    CHK(f32_flush_reductions(m, 1));       // the decoder's, on the side stream
    if (update) {
        HIPCHK(hipStreamWaitEvent(m->side, m->ev_fork2, 0));
        adam_blocks(m, m->side, b0, m->tb.end.e - b0, alpha, 1.0f);
    }
    HIPCHK(hipEventRecord(m->ev_dec, m->side));
    HIPCHK(hipGetLastError());
    return IWAE_OK;
}
