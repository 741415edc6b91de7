// iwae_grid_posterior, iwae_latent_activity, iwae_aggregate_posterior, iwae_ais, iwae_local_posterior (both with their _masked forms), iwae_impute and iwae_posterior: the analyses that start
// from the encoder heads of N images (host code; kernels in the seven *_kernels.hip).  Each reads in five parts: argument checks, eval_begin, its own buffers and launches, its own copy-outs, eval_end.
#include <math.h>
#include <string.h>
#include <algorithm>
#include <new>
#include "model.h"       // (the HIP runtime, include/iwae_amd.h and kernels.h come with it)
#include "layout.h"

using namespace iwae;

namespace {

// st: the handle's main stream (the whole call runs there); xd: the images [N][x_dim] on the device (the caller's, or the handle's copy);
// head, ldh (eval_heads): mu_i at head[i * ldh], sigma_i at Dp[0] further; f32: the eval precision is float32
struct EvalCall { iwae_model* m; hipStream_t st; const float* xd; const float* head; int ldh; bool f32; };

// Device, the parameters a deferred update may still be writing (both side streams idle), the images on the device
int eval_begin(iwae_model* m, const float* x, int N, EvalCall& c) {
    HIPCHK(hipSetDevice(m->cfg.device));
    CHK(join_side(m));
    if (m->side) HIPCHK(hipStreamSynchronize(m->side));
    if (m->side2) HIPCHK(hipStreamSynchronize(m->side2));
    c.m = m; c.st = m->stream; c.head = nullptr; c.ldh = 0; c.f32 = m->eval_precision == IWAE_PREC_FP32;
    return staged_in(m, x, m->ev.x, (size_t)N * m->X * 4, &c.xd);
}

// Encoder heads mu | sigma (src/iwae1.py:39-42) of the call's N images in the eval precision.  float32: f32_block_fwd into the shared head
// buffer; bf16: block_fwd on the bf16 rows into the handle's own encoder workspace (c.head points there).
int eval_heads(EvalCall& c, int N) {
    iwae_model* m = c.m;
    const int X = m->X, Xp = m->Xp32, Dp = m->Dp[0];
    if (c.f32) {
        CHK(ensure(m->ev.head, (size_t)N * 2 * Dp * 4, c.st));
        CHK(f32_block_fwd(m, m->enc1[0].sub[0], m->f32.enc1, c.xd, X, N, ptr<float>(m->ev.head), Dp, true));      // (no K split of the few-row products: an image's heads must not depend on N)
        c.head = ptr<float>(m->ev.head); c.ldh = 2 * Dp;
    } else {
        const int Nbp = round_up(N, 128);
        CHK(ensure(m->ev.xP, (size_t)Nbp * Xp * 2, c.st));
        launch_prep_rows(c.xd, nullptr, N, X, 0, Xp, Nbp, ptr<uint16_t>(m->ev.xP), c.st);
        CHK(block_alloc(m, m->enc1, m->wenc1, N, Nbp, false, false));
        CHK(block_fwd(m, m->enc1, m->wenc1, ptr<uint16_t>(m->ev.xP), N));
        c.head = ptr<float>(m->wenc1.head); c.ldh = m->enc1[2].Np32;
    }
    return IWAE_OK;
}

// q_mu, q_sigma [N][D] of the heads, to wherever the caller's arrays live (either may be null)
int eval_copy_heads(const EvalCall& c, int N, float* q_mu, float* q_sigma) {
    const int D = c.m->D[0];
    if (q_mu) HIPCHK(hipMemcpy2DAsync(q_mu, (size_t)D * 4, c.head, (size_t)c.ldh * 4, (size_t)D * 4, N, hipMemcpyDefault, c.st));
    if (q_sigma) HIPCHK(hipMemcpy2DAsync(q_sigma, (size_t)D * 4, c.head + c.m->Dp[0], (size_t)c.ldh * 4, (size_t)D * 4, N, hipMemcpyDefault, c.st));
    return IWAE_OK;
}

// The call's results are with the caller; its forward-pass leftovers are no longer what iwae_debug_tensor would name
int eval_end(EvalCall& c) {
    HIPCHK(hipStreamSynchronize(c.st));
    c.m->have_forward = false;
    return IWAE_OK;
}

// ws [S][N][D] = what iwae_debug_eps(N, S, 0) returns at the handle's step and offset
int dump_eps(iwae_model* m, int N, int S, int D, DevBuf& ws) {
    CHK(ensure(ws, (size_t)S * N * D * 4, m->stream));
    EpsSrc e;
    e.user = nullptr; e.B = N; e.seed = m->cfg.seed; e.row_offset = (uint64_t)m->batch_offset * (uint64_t)S; e.step = m->noise_step; e.stream = 0;
    launch_eps_dump(e, N, S, D, ptr<float>(ws), m->stream);
    HIPCHK(hipGetLastError());
    return IWAE_OK;
}

// Grid points per chunk of iwae_grid_posterior: ~8 KB of chunk-sized buffers per point at 784 pixels (logits, L_hi + L_lo, two hidden layers
// in float32), so 32 768 points keep them near 256 MB whatever G is.
#define GRID_CHUNK_DEFAULT 32768

// Transitions per launch of ais_chain_kernel (option ais_t_chunk).  Measured at the timing workload (N = 1 000, C = 16, L = 10, reference
// dims; profiles/ais_time.txt): one transition takes 4.37 ms there, a launch of 4 takes 17.5 ms -- well under the 50 ms a launch may hold a
// shared machine -- and the 125 launches of a T = 500 run cost nothing measurable (2.187 s in the kernel of 2.188 s wall).
#define AIS_T_CHUNK_DEFAULT 4

// Passes per launch of local_q_kernel (option local_t_chunk).  Measured at the timing workload (N = 1 000, S = 16, T = 500, E = 8, reference
// dims; profiles/local_q_time.txt): one pass takes 0.404 ms there (one row evaluation of 16 000 rows; an AIS transition at L = 10 is eleven:
// 4.38 ms), a full launch of 32 takes 32 x 0.404 = 12.9 ms (the file's 12.84 ms averages in the shorter last launch) -- well under the 50 ms a launch may hold a shared machine -- and launches of 8 change nothing
// measurable (0.207 s in the kernel against 0.205 s), so nothing is gained by going lower and nothing by going higher.
#define LOCAL_T_CHUNK_DEFAULT 32
#define LOCAL_PASSES_MAX (1 << 24)      // T and E each: T + E and the step-size table stay far inside int and host memory

// Rows (images x draws, whole images) per launch of impute_rows_kernel (option impute_rows).  Measured at the timing workload (reference dims,
// 50 % mask; profiles/impute_time.txt): a launch of 500 000 rows (N = 10 000, k = 50) takes 8.26 ms, one of 520 000 (104 images at k = 5 000)
// 6.65 ms, each the mean of passes (a) and (c) -- well under the 50 ms a launch may hold a shared machine -- and the 194 launches
// (97 per pass) of the N = 10 000, k = 5 000 call cost nothing measurable (1.290 s in the kernel of 1.297 s wall), so nothing is gained by going higher.
#define IMPUTE_ROWS_DEFAULT (1 << 19)
#define IMPUTE_K_MAX 65536
#define POSTERIOR_R_MAX 65536
// iwae_posterior: floats of chunk moments per launch of posterior_moments_kernel (256 MB): at the reference dims (D' = 112, k = 5 000) an image
// takes 79 x 12 656 floats, so a launch holds 67 images; the sums do not depend on where the launches are cut.
#define POSTERIOR_PART_FLOATS ((size_t)1 << 26)

// The decoder's weights in both orientations, padded to multiples of 16 (src/iwae1.py:72-75; Keras kernels [in][out]), into m->ais.wpad
struct DecPad { const float *W1, *W1T, *W2, *W2T, *W3, *W3T, *b1, *b2, *b3; };
int pad_decoder(iwae_model* m, hipStream_t st, int Dp, int Hp, int Xp, DecPad& p) {
    const int D = m->D[0], H = m->H[0], X = m->X;
    const KerasLayer* d1 = &m->klayers[m->dec1[0].sub[0]];
    const size_t nW1 = (size_t)Dp * Hp, nW2 = (size_t)Hp * Hp, nW3 = (size_t)Hp * Xp;
    CHK(ensure(m->ais.wpad, (2 * (nW1 + nW2 + nW3) + 2 * Hp + Xp) * 4, st));
    float* W1 = ptr<float>(m->ais.wpad); float* W1T = W1 + nW1; float* W2 = W1T + nW1; float* W2T = W2 + nW2; float* W3 = W2T + nW2; float* W3T = W3 + nW3;
    float* b1 = W3T + nW3; float* b2 = b1 + Hp; float* b3 = b2 + Hp;
    const AisPrepArgs jobs[6] = {{m->param + d1[0].offW, D, H, Dp, Hp, W1, W1T}, {m->param + d1[1].offW, H, H, Hp, Hp, W2, W2T},
                                 {m->param + d1[2].offW, H, X, Hp, Xp, W3, W3T}, {m->param + d1[0].offb, 1, H, 1, Hp, b1, nullptr},
                                 {m->param + d1[1].offb, 1, H, 1, Hp, b2, nullptr}, {m->param + d1[2].offb, 1, X, 1, Xp, b3, nullptr}};
    for (const AisPrepArgs& j : jobs) launch_ais_pad(j, st);
    HIPCHK(hipGetLastError());
    p = DecPad{W1, W1T, W2, W2T, W3, W3T, b1, b2, b3};
    return IWAE_OK;
}

// The pixel rows of a masked chain call (iwae_ais_masked, iwae_local_posterior_masked): the mask on the device (the
// caller's, or a copy in maskbuf), xin = m ? x : 0 for the encoder (c.xd points there from here on) and xc = m ? x : the hole code, which the
// HOLES instantiations of the row evaluation read in place of x (*xcode).
int mask_rows(EvalCall& c, int N, const uint8_t* mask, DevBuf& maskbuf, DevBuf& xin, DevBuf& xc, const float** xcode) {
    iwae_model* m = c.m;
    const long n = (long)N * m->X;
    const uint8_t* maskd = nullptr;
    CHK(staged_in(m, mask, maskbuf, (size_t)n, &maskd));
    CHK(ensure(xin, (size_t)n * 4, c.st));
    CHK(ensure(xc, (size_t)n * 4, c.st));
    launch_impute_mask(c.xd, maskd, n, ptr<float>(xin), c.st);
    launch_masked_code(c.xd, maskd, n, ptr<float>(xc), c.st);
    HIPCHK(hipGetLastError());
    c.xd = ptr<float>(xin);
    *xcode = ptr<float>(xc);
    return IWAE_OK;
}

// What iwae_impute and iwae_posterior share.  First the models and sizes both accept (who: the caller's name, for the message) ...
int impute_scope(iwae_model* m, const char* who, int N, int k) {
    const std::string w(who);
    if (N <= 0 || k < 1 || k > IMPUTE_K_MAX) return fail(IWAE_ERR_ARG, w + ": needs N > 0 and 1 <= k <= " + std::to_string(IMPUTE_K_MAX));
    if (m->cfg.n_layers != 1) return fail(IWAE_ERR_ARG, w + ": only the 1-layer model");
    if (m->C != 0 || m->has_prior) return fail(IWAE_ERR_ARG, w + ": only the unconditional model (cond_dim = 0, no learned prior)");
    if ((int64_t)N * k > (int64_t)1 << 27) return fail(IWAE_ERR_ARG, w + ": too large (N * k > 2^27 rows)");
    if (round_up(m->H[0], 16) > 16 * AIS_NT || round_up(m->D[0], 16) > 16 * AIS_DT) return fail(IWAE_ERR_ARG, w + ": needs n_hidden <= " + std::to_string(16 * AIS_NT) + " and n_latent <= " + std::to_string(16 * AIS_DT));
    return IWAE_OK;
}

// ... and the weights: the masked input, the encoder heads (copied to q_mu / q_sigma), pass (a) in launches of whole images of at most
// `impute_rows` rows, and pass (b).  Leaves in m->imp log_w (or in the caller's device array: iw.logwd), wstat, lpx and (want_ess) ess; iw.ia
// is ready for further launches of impute_rows_kernel (xhat and part unset) and carries the call's noise keys.  Switches the kernel
// timing on for the call: the caller switches it off after its own timed launches.
struct ImputeWeights { ImputeArgs ia; float* logwd; int nbmax, nchunk; };
int impute_weights(EvalCall& c, int N, int S, const uint8_t* mask, const float* eps, float* log_w, bool want_ess, float* q_mu, float* q_sigma, ImputeWeights& iw) {
    iwae_model* m = c.m;
    hipStream_t st = c.st;
    iwae_model::ImputeWs& w = m->imp;
    const int D = m->D[0], H = m->H[0], X = m->X, Dp = round_up(D, 16), Hp = round_up(H, 16), Xp = round_up(X, 16), Dh = m->Dp[0];
    // ---- the masked input xin = m ? x : 0 into the call's own buffer: what the encoder and the rows read from here on
    const uint8_t* maskd = nullptr;
    if (mask) {
        CHK(staged_in(m, mask, w.mask, (size_t)N * X, &maskd));
        CHK(ensure(w.xin, (size_t)N * X * 4, st));
        launch_impute_mask(c.xd, maskd, (long)N * X, ptr<float>(w.xin), st);
        HIPCHK(hipGetLastError());
        c.xd = ptr<float>(w.xin);
    }
    // ---- encoder heads mu, sigma of the masked input (src/iwae1.py:39-42), in the eval precision
    CHK(eval_heads(c, N));
    CHK(eval_copy_heads(c, N, q_mu, q_sigma));
    ImputeArgs& ia = iw.ia;
    memset(&ia, 0, sizeof(ia));
    {
        DecPad p;
        CHK(pad_decoder(m, st, Dp, Hp, Xp, p));
        ia.W1 = p.W1; ia.W2 = p.W2; ia.W3 = p.W3; ia.b1 = p.b1; ia.b2 = p.b2; ia.b3 = p.b3;
    }
    const float* epsd = nullptr;
    if (eps) CHK(staged_in(m, eps, w.eps, (size_t)S * N * D * 4, &epsd));
    float* logwd = nullptr;
    CHK(staged_out(m, log_w, w.logw, (size_t)S * N * 4, &logwd));      // (always computed: the later passes read it)
    CHK(ensure(w.wstat, (size_t)N * 8, st));
    CHK(ensure(w.lpx, (size_t)N * 8, st));
    if (want_ess) CHK(ensure(w.ess, (size_t)N * 4, st));
    // ---- launches of whole images, at most `cap` rows each
    const int cap = m->opt.impute_rows > 0 ? m->opt.impute_rows : IMPUTE_ROWS_DEFAULT;
    const int nbmax = std::min((int)N, std::max(1, cap / S)), nchunk = S > 64 ? (S + 63) / 64 : 1;
    ia.D = D; ia.H = H; ia.X = X; ia.Dp = Dp; ia.Hp = Hp; ia.Xp = Xp;
    ia.x = c.xd; ia.mask = maskd; ia.head = c.head; ia.ldh = c.ldh; ia.soff = Dh;
    ia.N = N; ia.S = S; ia.ipw = S <= 64 ? 64 / S : 1; ia.nchunk = nchunk;
    ia.eps = epsd; ia.seed = m->cfg.seed; ia.row_offset = (uint64_t)m->batch_offset * (uint64_t)S; ia.step = m->noise_step;
    ia.log_w = logwd; ia.wstat = ptr<float2>(w.wstat);
    m->time_this = m->timing > 0;
    // pass (a): log_w of every row
    for (int i0 = 0; i0 < N; i0 += nbmax) {
        ia.img0 = i0; ia.nimg = std::min(nbmax, (int)N - i0);
        ScopedTimer tm(m, T_IMPUTE, st);
        launch_impute_rows(ia, false, st);
        HIPCHK(hipGetLastError());
    }
    // pass (b): per image the maximum, the sum, log_px and ess, in sample order
    ImputeStatsArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.log_w = logwd; sa.N = N; sa.S = S; sa.log_px = ptr<double>(w.lpx); sa.ess = want_ess ? ptr<float>(w.ess) : nullptr; sa.wstat = ptr<float2>(w.wstat);
    launch_impute_stats(sa, st);
    HIPCHK(hipGetLastError());
    iw.logwd = logwd; iw.nbmax = nbmax; iw.nchunk = nchunk;
    return IWAE_OK;
}

}  // namespace

extern "C" {

int iwae_grid_posterior(iwae_handle m, const float* x, int32_t N, const float* z, const float* log_wq, int32_t G, double* log_px,
                        float* post_mean, float* post_cov, float* q_mu, float* q_sigma, float* q_mass, float* kl_q_post, float* log_joint) {
    if (!m || !x || !z || !log_px) return fail(IWAE_ERR_ARG, "grid_posterior: need x, z and log_px");
    if (N <= 0 || G <= 0) return fail(IWAE_ERR_ARG, "grid_posterior: N and G must be positive");
    if (m->cfg.n_layers != 1) return fail(IWAE_ERR_ARG, "grid_posterior: only the 1-layer model (the 2-layer model needs a nested integral over z1)");
    if (m->C != 0) return fail(IWAE_ERR_ARG, "grid_posterior: only the unconditional model (cond_dim = 0)");
    if (m->D[0] > GRID_D_MAX) return fail(IWAE_ERR_ARG, "grid_posterior: needs n_latent <= 4 (got " + std::to_string(m->D[0]) + ")");
    if (m->Xp32 > GRID_XP_MAX) return fail(IWAE_ERR_ARG, "grid_posterior: needs x_dim <= " + std::to_string(GRID_XP_MAX));
    EvalCall c;
    CHK(eval_begin(m, x, N, c));
    hipStream_t st = c.st;
    iwae_model::GridWs& w = m->grid;
    const int D = m->D[0], Dp = m->Dp[0], X = m->X, Xp = m->Xp32, Np = round_up(N, 64);
    // ---- images: bf16 copy for the score kernel + the binary check (the scores rely on x being exact in bf16)
    CHK(ensure(w.xb, (size_t)Np * Xp * 2, st));
    CHK(ensure(w.flag, 4, st));
    HIPCHK(hipMemsetAsync(w.flag.p, 0, 4, st));
    launch_grid_prep_x(c.xd, N, X, Np, Xp, ptr<uint16_t>(w.xb), ptr<int>(w.flag), st);
    HIPCHK(hipGetLastError());
    int nonbinary = 0;
    HIPCHK(hipMemcpyAsync(&nonbinary, w.flag.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (nonbinary) return fail(IWAE_ERR_ARG, "grid_posterior: x must be binary (every value 0 or 1)");
    // ---- encoder heads mu, sigma of the N images (src/iwae1.py:39-42), in the eval precision
    CHK(eval_heads(c, N));
    CHK(eval_copy_heads(c, N, q_mu, q_sigma));
    const float* head = c.head; const int ldh = c.ldh;
    // ---- G in chunks: decoder logits -> prep -> score -> merge into the running per-image state
    const int chunk = m->opt.grid_chunk > 0 ? m->opt.grid_chunk : GRID_CHUNK_DEFAULT;
    const int gmax = std::min(chunk, (int)G), gmaxp = round_up(gmax, 128), H = m->H[0], Hp = m->dec1[0].Np32;
    CHK(ensure(w.run, (size_t)N * GRID_ST * 8, st));
    CHK(ensure(w.lpx, (size_t)N * 8, st));
    CHK(ensure(w.mean, (size_t)N * D * 4, st));
    CHK(ensure(w.cov, (size_t)N * D * D * 4, st));
    CHK(ensure(w.qmass, (size_t)N * 4, st));
    CHK(ensure(w.kl, (size_t)N * 4, st));
    CHK(ensure(w.z, (size_t)gmax * D * 4, st));
    if (log_wq) CHK(ensure(w.lw, (size_t)gmax * 4, st));
    CHK(ensure(w.logits, (size_t)gmaxp * Xp * 4, st));
    CHK(ensure(w.lhi, (size_t)gmaxp * Xp * 2, st));
    CHK(ensure(w.llo, (size_t)gmaxp * Xp * 2, st));
    CHK(ensure(w.c, (size_t)gmaxp * 4, st));
    CHK(ensure(w.zc, (size_t)gmaxp * 16, st));
    CHK(ensure(w.w, (size_t)gmaxp * 4, st));
    if (c.f32) {
        CHK(ensure(w.h1, (size_t)gmax * H * 4, st));
        CHK(ensure(w.h2, (size_t)gmax * H * 4, st));
    } else {
        CHK(ensure(w.zP, (size_t)gmaxp * Dp * 2, st));
        CHK(ensure(w.h1, (size_t)gmaxp * Hp * 2, st));
        CHK(ensure(w.h2, (size_t)gmaxp * Hp * 2, st));
    }
    const int nsplit_max = (gmax + GRID_RANGE - 1) / GRID_RANGE;
    CHK(ensure(w.part, (size_t)nsplit_max * N * GRID_ST * 4, st));
    float* lj = nullptr;
    if (log_joint) CHK(staged_out(m, log_joint, w.lj, (size_t)N * G * 4, &lj));
    const KerasLayer* d1 = &m->klayers[m->dec1[0].sub[0]];
    for (int c0 = 0; c0 < G; c0 += chunk) {
        const int Gc = std::min(chunk, (int)G - c0), Gcp = round_up(Gc, 128);
        HIPCHK(hipMemcpyAsync(w.z.p, z + (size_t)c0 * D, (size_t)Gc * D * 4, hipMemcpyDefault, st));
        if (log_wq) HIPCHK(hipMemcpyAsync(w.lw.p, log_wq + c0, (size_t)Gc * 4, hipMemcpyDefault, st));
        // decoder logits l_g (src/iwae1.py:72-75), as iwae_decode / forward_f32 compute them
        if (c.f32) {
            CHK(f32_fwd(m, d1[0], ptr<float>(w.z), D, Gc, ptr<float>(w.h1), H, GEMM_EPI_TANH, false));
            CHK(f32_fwd(m, d1[1], ptr<float>(w.h1), H, Gc, ptr<float>(w.h2), H, GEMM_EPI_TANH, false));
            CHK(f32_fwd(m, d1[2], ptr<float>(w.h2), H, Gc, ptr<float>(w.logits), Xp, GEMM_EPI_NONE, false));
        } else {
            launch_prep_rows(ptr<float>(w.z), nullptr, Gc, D, 0, Dp, Gcp, ptr<uint16_t>(w.zP), st);
            CHK(dense_fwd(m, m->dec1[0], EPI_TANH, ptr<uint16_t>(w.zP), Gc, ptr<uint16_t>(w.h1), nullptr, 0));
            CHK(dense_fwd(m, m->dec1[1], EPI_TANH, ptr<uint16_t>(w.h1), Gc, ptr<uint16_t>(w.h2), nullptr, 0));
            // (EPI_HEAD on the output layer: fp32 logits with the bias -- its exp split lies beyond the one-sub-layer map; EPI_F32 adds no bias)
            CHK(dense_fwd(m, m->dec1[2], EPI_HEAD, ptr<uint16_t>(w.h2), Gc, nullptr, ptr<float>(w.logits), Xp));
        }
        GridPrepArgs pa;
        memset(&pa, 0, sizeof(pa));
        pa.logits = ptr<float>(w.logits); pa.ldl = Xp; pa.z = ptr<float>(w.z); pa.lw = log_wq ? ptr<float>(w.lw) : nullptr;
        pa.Gc = Gc; pa.Gcp = round_up(Gc, 16); pa.X = X; pa.Xp = Xp; pa.D = D;
        pa.Lhi = ptr<uint16_t>(w.lhi); pa.Llo = ptr<uint16_t>(w.llo); pa.c = ptr<float>(w.c); pa.zc = ptr<float4>(w.zc); pa.w = ptr<float>(w.w);
        launch_grid_prep(pa, st);
        HIPCHK(hipGetLastError());
        GridScoreArgs sa;
        memset(&sa, 0, sizeof(sa));
        sa.XB = ptr<uint16_t>(w.xb); sa.Xp = Xp; sa.Lhi = pa.Lhi; sa.Llo = pa.Llo; sa.c = pa.c; sa.zc = pa.zc; sa.w = pa.w;
        sa.head = head; sa.ldh = ldh; sa.soff = Dp; sa.N = N; sa.Gc = Gc; sa.nsplit = (Gc + GRID_RANGE - 1) / GRID_RANGE;
        sa.part = ptr<float>(w.part); sa.log_joint = lj; sa.ldlj = G; sa.lj_col = c0;
        launch_grid_score(sa, D, st);
        HIPCHK(hipGetLastError());
        GridMergeArgs ma;
        memset(&ma, 0, sizeof(ma));
        ma.part = sa.part; ma.nsplit = sa.nsplit; ma.N = N; ma.D = D; ma.run = ptr<double>(w.run);
        ma.first = c0 == 0; ma.last = c0 + Gc >= G; ma.head = head; ma.ldh = ldh;
        ma.log_px = ptr<double>(w.lpx); ma.mean = ptr<float>(w.mean); ma.cov = ptr<float>(w.cov); ma.qmass = ptr<float>(w.qmass); ma.kl = ptr<float>(w.kl);
        launch_grid_merge(ma, st);
        HIPCHK(hipGetLastError());
    }
    CHK(copy_out(m, log_px, w.lpx.p, (size_t)N * 8));
    if (post_mean) CHK(copy_out(m, post_mean, w.mean.p, (size_t)N * D * 4));
    if (post_cov) CHK(copy_out(m, post_cov, w.cov.p, (size_t)N * D * D * 4));
    if (q_mass) CHK(copy_out(m, q_mass, w.qmass.p, (size_t)N * 4));
    if (kl_q_post) CHK(copy_out(m, kl_q_post, w.kl.p, (size_t)N * 4));
    CHK(finish_out(m, log_joint, lj, (size_t)N * G * 4));
    return eval_end(c);
}

int iwae_latent_activity(iwae_handle m, const float* x, int32_t N, int32_t k, const float* eps, double* activity, double* data_mean, float* post_mean) {
    if (!m || !x) return fail(IWAE_ERR_ARG, "latent_activity: need x");
    if (!activity) return fail(IWAE_ERR_ARG, "latent_activity: activity is required");
    if (N <= 0) return fail(IWAE_ERR_ARG, "latent_activity: N must be positive");
    if (m->C != 0) return fail(IWAE_ERR_ARG, "latent_activity: only the unconditional models (cond_dim = 0)");
    const bool two = m->cfg.n_layers == 2;
    if (two && k <= 0) return fail(IWAE_ERR_ARG, "latent_activity: k must be positive for the 2-layer model");
    EvalCall c;
    CHK(eval_begin(m, x, N, c));
    hipStream_t st = c.st;
    iwae_model::ActWs& w = m->act;
    const int D0 = m->D[0], Dp0 = m->Dp[0], D1 = two ? m->D[1] : 0, Dt = D0 + D1;
    // ---- layer 1: E_q[z1|x] = mu1(x), the encoder head
    CHK(eval_heads(c, N));
    const float* head = c.head; const int ldh = c.ldh;
    CHK(ensure(w.pm, (size_t)N * Dt * 4, st));
    CHK(ensure(w.act, (size_t)Dt * 8, st));
    CHK(ensure(w.dm, (size_t)Dt * 8, st));
    ActStatsArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.src = head; sa.ld_img = ldh; sa.ld_blk = 0; sa.nblk = 1; sa.kdiv = 1.0; sa.N = N; sa.D = D0;
    sa.post_mean = ptr<float>(w.pm); sa.ldpm = Dt; sa.col = 0; sa.activity = ptr<double>(w.act); sa.data_mean = ptr<double>(w.dm);
    launch_act_stats(sa, st);
    HIPCHK(hipGetLastError());
    if (two) {
        // ---- layer 2: E_q[z2|x] = E_{z1 ~ q(z1|x)}[mu2(z1)], summed per (image, ACT_BLOCK-sample block), launches of at most eval_rows rows:
        // whole images while k fits (kc = k), else one image at a time in sample chunks of a multiple of ACT_BLOCK -- so a block never
        // straddles two launches and an image's partials do not depend on the chunking.
        const Linear* e2 = m->enc2;
        const bool fused = !c.f32 && act_chain_ok(e2[0].KT, e2[1].KT, m->Dp[1] / 32) && e2[0].Kp32 == Dp0 && e2[0].Np32 == 32 * e2[1].KT &&
                           e2[1].Np32 == e2[0].Np32 && e2[2].KT == e2[1].KT && e2[2].Np32 == 2 * m->Dp[1] && ldh == 2 * Dp0;
        const int eval_rows = m->opt.eval_rows > 0 ? m->opt.eval_rows : 1 << 19;
        // (bf16 composed path: at most 4096 rows, where block_fwd is one block_fwd_kernel launch on any row count -- a row's mu2 does not
        // depend on how many rows share its launch)
        const int cap = (!c.f32 && !fused) ? std::min(eval_rows, 4096) : eval_rows;
        const int kc = k <= cap ? k : std::max(ACT_BLOCK, cap / ACT_BLOCK * ACT_BLOCK);
        const int nbmax = kc == k ? std::max(1, std::min(32768, cap / k)) : 1;
        const int nblk = (k + ACT_BLOCK - 1) / ACT_BLOCK;
        CHK(ensure(w.part, (size_t)N * nblk * D1 * 4, st));
        const size_t rows_max = (size_t)std::min(nbmax, (int)N) * kc, rows_maxp = round_up((int)rows_max, 128);
        CHK(ensure(w.eps, rows_max * D0 * 4, st));
        if (!fused) {
            CHK(ensure(w.rows, rows_maxp * 4, st));
            if (c.f32) {
                const int H = m->klayers[e2[0].sub[0]].Nout;
                CHK(ensure(w.z, rows_maxp * D0 * 4, st));
                CHK(ensure(w.f32.h1, rows_maxp * H * 4, st));
                CHK(ensure(w.f32.h2, rows_maxp * H * 4, st));
                CHK(ensure(w.blk.head, rows_maxp * D1 * 4, st));
            } else {
                CHK(ensure(w.z, rows_maxp * Dp0 * 2, st));
                CHK(block_alloc(m, m->enc2, w.blk, (int)rows_max, (int)rows_maxp, false, false));
            }
        }
        const uint32_t step = m->noise_step;
        for (int i0 = 0; i0 < N; i0 += nbmax) {
            const int nb = std::min(nbmax, (int)N - i0);
            for (int s0 = 0; s0 < k; s0 += kc) {
                const int kn = std::min(kc, (int)k - s0), M = nb * kn, Mp = round_up(M, 128);
                EpsSrc e;
                e.seed = m->cfg.seed; e.step = step; e.stream = 0;
                e.row_offset = (uint64_t)(m->batch_offset + (uint32_t)i0) * (uint64_t)k;     // iwae_eval_llh's Philox rows: (offset + i) k + s
                e.k_total = k; e.s_off = s0; e.kc = kn;
                if (eps) {      // the caller's [k][N][D0] draws of this chunk -> [kn][nb][D0]
                    HIPCHK(hipMemcpy2DAsync(w.eps.p, (size_t)nb * D0 * 4, eps + ((size_t)s0 * N + i0) * D0, (size_t)N * D0 * 4, (size_t)nb * D0 * 4, kn, hipMemcpyDefault, st));
                    e.user = ptr<float>(w.eps);
                }
                e.B = nb;
                const float* hd = head + (size_t)i0 * ldh;
                if (fused) {
                    ActChainArgs c;
                    memset(&c, 0, sizeof(c));
                    c.img1 = e2[0].imgF; c.img2 = e2[1].imgF; c.imgh = e2[2].imgF;
                    c.head1 = hd; c.ldH1 = ldh; c.eps1 = e; c.kn = kn; c.D0 = D0; c.D1 = D1;
                    c.part = ptr<float>(w.part); c.nblk = nblk; c.img0 = i0; c.blk0 = s0 / ACT_BLOCK;
                    launch_act_chain(c, nb, st);
                } else {
                    SampleArgs sm;
                    memset(&sm, 0, sizeof(sm));
                    sm.head = hd; sm.ldH = ldh; sm.Dp = Dp0; sm.D = D0; sm.head_per_row = 0;
                    sm.M = M; sm.Mp = Mp; sm.k = kn; sm.B = nb; sm.eps = e;
                    sm.lq = ptr<float>(w.rows);
                    const float* mu2;
                    int ldm;
                    if (c.f32) {      // z1 rows in float32 -> the q(z2|z1) block's two tanh layers and its mu head (the sigma head is not needed)
                        sm.ZF = ptr<float>(w.z); sm.ldZF = D0;
                        launch_sample(sm, st);
                        const KerasLayer* l1 = &m->klayers[e2[0].sub[0]];
                        const int H = l1->Nout;
                        // (no K split of few-row products: an image's mu2 must not depend on how many share the launch)
                        CHK(f32_fwd(m, l1[0], ptr<float>(w.z), D0, M, ptr<float>(w.f32.h1), H, GEMM_EPI_TANH, true));
                        CHK(f32_fwd(m, l1[1], ptr<float>(w.f32.h1), H, M, ptr<float>(w.f32.h2), H, GEMM_EPI_TANH, true));
                        CHK(f32_fwd(m, l1[2], ptr<float>(w.f32.h2), H, M, ptr<float>(w.blk.head), D1, GEMM_EPI_NONE, true));
                        mu2 = ptr<float>(w.blk.head); ldm = D1;
                    } else {
                        sm.ZP = ptr<uint16_t>(w.z);
                        launch_sample(sm, st);
                        CHK(block_fwd(m, m->enc2, w.blk, ptr<uint16_t>(w.z), M));
                        mu2 = ptr<float>(w.blk.head); ldm = e2[2].Np32;
                    }
                    ActPartialArgs pa;
                    memset(&pa, 0, sizeof(pa));
                    pa.head = mu2; pa.ldh = ldm; pa.nb = nb; pa.kn = kn; pa.D1 = D1;
                    pa.part = ptr<float>(w.part); pa.nblk = nblk; pa.img0 = i0; pa.blk0 = s0 / ACT_BLOCK;
                    launch_act_partial(pa, st);
                }
                HIPCHK(hipGetLastError());
            }
        }
        sa.src = ptr<float>(w.part); sa.ld_img = (long)nblk * D1; sa.ld_blk = D1; sa.nblk = nblk; sa.kdiv = (double)k; sa.D = D1; sa.col = D0;
        launch_act_stats(sa, st);
        HIPCHK(hipGetLastError());
        m->noise_step += 1;
    }
    CHK(copy_out(m, activity, w.act.p, (size_t)Dt * 8));
    if (data_mean) CHK(copy_out(m, data_mean, w.dm.p, (size_t)Dt * 8));
    if (post_mean) CHK(copy_out(m, post_mean, w.pm.p, (size_t)N * Dt * 4));
    return eval_end(c);
}

// Aggregate-posterior decomposition (Hoffman & Johnson 2016; Chen et al. 2018): the samples z = mu_n + sigma_n eps_{s,n} of every image
// against the mixture of all N encoder posteriors, in sample tiles of AGG_TILE; DESIGN.md section 14
int iwae_aggregate_posterior(iwae_handle m, const float* x, int32_t N, int32_t S, const float* eps, double* summary, double* unit_kl, double* unit_mi,
                             float* q_mu, float* q_sigma, float* log_qz, float* log_qzd) {
    if (!m || !x || !summary) return fail(IWAE_ERR_ARG, "aggregate_posterior: need x and summary");
    if (N <= 0 || S <= 0) return fail(IWAE_ERR_ARG, "aggregate_posterior: N and S must be positive");
    if (m->cfg.n_layers != 1) return fail(IWAE_ERR_ARG, "aggregate_posterior: only the 1-layer model (the 2-layer q(z2|x) is not Gaussian, its p(z1) not N(0,1))");
    if (m->C != 0) return fail(IWAE_ERR_ARG, "aggregate_posterior: only the unconditional model (cond_dim = 0)");
    if (N > 1 << 24 || (int64_t)N * S > (int64_t)1 << 27) return fail(IWAE_ERR_ARG, "aggregate_posterior: too large (N > 2^24 images or N * S > 2^27 samples)");
    EvalCall c;
    CHK(eval_begin(m, x, N, c));
    hipStream_t st = c.st;
    iwae_model::AggWs& w = m->agg;
    const int D = m->D[0], Dp = m->Dp[0], Dpad = round_up(D, AGG_DC);
    const long SN = (long)S * N;
    const int P = (N + AGG_RANGE - 1) / AGG_RANGE, Tmax = (int)std::min<long>(SN, AGG_TILE);
    // ---- encoder heads mu, sigma of the N images (src/iwae1.py:39-42), in the eval precision
    CHK(eval_heads(c, N));
    CHK(eval_copy_heads(c, N, q_mu, q_sigma));
    const float* head = c.head; const int ldh = c.ldh;
    // ---- the draws [S][N][D]: the caller's, or what iwae_debug_eps(N, S, 0) returns at this step and offset
    const float* ed;
    if (eps) CHK(staged_in(m, eps, w.eps, (size_t)SN * D * 4, &ed));
    else { CHK(dump_eps(m, N, S, D, w.eps)); ed = ptr<float>(w.eps); }
    CHK(ensure(w.mu, (size_t)N * Dpad * 4, st));
    CHK(ensure(w.inv, (size_t)N * Dpad * 4, st));
    CHK(ensure(w.nls, (size_t)N * Dpad * 4, st));
    CHK(ensure(w.invd, (size_t)N * Dpad * 8, st));
    CHK(ensure(w.nls_sum, (size_t)N * 8, st));
    CHK(ensure(w.zT, (size_t)Dpad * Tmax * 4, st));
    CHK(ensure(w.shT, (size_t)Dpad * Tmax * 4, st));
    CHK(ensure(w.dim_part, (size_t)P * Dpad * Tmax * 4, st));
    CHK(ensure(w.jmax, (size_t)P * Tmax * 8, st));
    CHK(ensure(w.jsum, (size_t)P * Tmax * 4, st));
    CHK(ensure(w.lqz, (size_t)SN * 4, st));
    CHK(ensure(w.lqzdT, (size_t)Dpad * SN * 4, st));
    CHK(ensure(w.part, (size_t)(D + 1) * 5 * 8, st));
    CHK(ensure(w.out, (size_t)(4 + 2 * D) * 8, st));
    AggCompArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.head = head; ca.ldh = ldh; ca.soff = Dp; ca.N = N; ca.D = D; ca.Dpad = Dpad;
    ca.mu = ptr<float>(w.mu); ca.inv = ptr<float>(w.inv); ca.nls = ptr<float>(w.nls);
    ca.invd = ptr<double>(w.invd); ca.nls_sum = ptr<double>(w.nls_sum);
    launch_agg_comp(ca, st);
    HIPCHK(hipGetLastError());
    for (long i0 = 0; i0 < SN; i0 += AGG_TILE) {
        const int T = (int)std::min<long>(AGG_TILE, SN - i0);
        AggSampleArgs sa;
        memset(&sa, 0, sizeof(sa));
        sa.head = head; sa.ldh = ldh; sa.soff = Dp; sa.N = N; sa.D = D; sa.Dpad = Dpad; sa.eps = ed;
        sa.mu = ca.mu; sa.inv = ca.inv; sa.nls = ca.nls; sa.i0 = i0; sa.T = T; sa.zT = ptr<float>(w.zT); sa.shT = ptr<float>(w.shT);
        launch_agg_sample(sa, st);
        AggMainArgs ma;
        memset(&ma, 0, sizeof(ma));
        ma.mu = ca.mu; ma.inv = ca.inv; ma.nls = ca.nls; ma.invd = ca.invd; ma.nls_sum = ca.nls_sum; ma.N = N; ma.Dpad = Dpad;
        ma.zT = sa.zT; ma.shT = sa.shT; ma.T = T;
        ma.dim_part = ptr<float>(w.dim_part); ma.joint_max = ptr<double>(w.jmax); ma.joint_sum = ptr<float>(w.jsum);
        launch_agg_main(ma, st);
        AggMergeArgs ga;
        memset(&ga, 0, sizeof(ga));
        ga.dim_part = ma.dim_part; ga.joint_max = ma.joint_max; ga.joint_sum = ma.joint_sum; ga.shT = sa.shT; ga.P = P; ga.Dpad = Dpad; ga.T = T;
        ga.log_n = log((double)N); ga.log_qz = ptr<float>(w.lqz); ga.log_qzdT = ptr<float>(w.lqzdT); ga.ldo = SN; ga.i0 = i0;
        launch_agg_merge(ga, st);
        HIPCHK(hipGetLastError());
    }
    AggReduceArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.head = head; ra.ldh = ldh; ra.soff = Dp; ra.N = N; ra.D = D; ra.eps = ed; ra.SN = SN;
    ra.log_qz = ptr<float>(w.lqz); ra.log_qzdT = ptr<float>(w.lqzdT); ra.part = ptr<double>(w.part);
    ra.summary = ptr<double>(w.out); ra.unit_kl = ra.summary + 4; ra.unit_mi = ra.unit_kl + D;
    launch_agg_reduce(ra, st);
    HIPCHK(hipGetLastError());
    CHK(copy_out(m, summary, ra.summary, 4 * 8));
    if (unit_kl) CHK(copy_out(m, unit_kl, ra.unit_kl, (size_t)D * 8));
    if (unit_mi) CHK(copy_out(m, unit_mi, ra.unit_mi, (size_t)D * 8));
    if (log_qz) CHK(copy_out(m, log_qz, w.lqz.p, (size_t)SN * 4));
    if (log_qzd) {
        float* dst;
        CHK(staged_out(m, log_qzd, w.lqzd, (size_t)SN * D * 4, &dst));
        launch_agg_untranspose(ptr<float>(w.lqzdT), SN, D, dst, st);
        HIPCHK(hipGetLastError());
        CHK(finish_out(m, log_qzd, dst, (size_t)SN * D * 4));
    }
    CHK(eval_end(c));
    if (!eps) m->noise_step += 1;
    return IWAE_OK;
}

// Annealed importance sampling with HMC chains (Neal 2001; Wu et al. 2017): DESIGN.md section 15
// (mask null: iwae_ais; else iwae_ais_masked -- the same checks, launches and copy-outs, the pixel rows coded and the HOLES kernel)
static int ais_call(iwae_handle m, const float* x, const uint8_t* mask, int32_t N, const iwae_ais_options* o, const iwae_ais_outputs* out) {
    if (!m || !x || !o || !out) return fail(IWAE_ERR_ARG, "ais: need x, options and outputs");
    if (o->struct_size != sizeof(iwae_ais_options)) return fail(IWAE_ERR_ARG, "ais: iwae_ais_options.struct_size must be sizeof(iwae_ais_options) = " + std::to_string(sizeof(iwae_ais_options)));
    if (!out->log_px || !o->betas) return fail(IWAE_ERR_ARG, "ais: betas and log_px are required");
    if (N <= 0 || o->C <= 0 || o->T <= 0 || o->L <= 0) return fail(IWAE_ERR_ARG, "ais: N, C, T and L must be positive");
    if (!(o->step_size > 0.0f)) return fail(IWAE_ERR_ARG, "ais: step_size must be positive");
    if (o->init != IWAE_AIS_INIT_ENCODER && o->init != IWAE_AIS_INIT_PRIOR) return fail(IWAE_ERR_ARG, "ais: init must be IWAE_AIS_INIT_ENCODER or IWAE_AIS_INIT_PRIOR");
    const int given = (o->eps0 != nullptr) + (o->mom != nullptr) + (o->unif != nullptr);
    if (given != 0 && given != 3) return fail(IWAE_ERR_ARG, "ais: eps0, mom and unif come all three or not at all");
    if (m->cfg.n_layers != 1) return fail(IWAE_ERR_ARG, "ais: only the 1-layer model");
    if (m->C != 0 || m->has_prior) return fail(IWAE_ERR_ARG, "ais: only the unconditional model (cond_dim = 0, no learned prior)");
    if ((int64_t)N * o->C > (int64_t)1 << 27) return fail(IWAE_ERR_ARG, "ais: too large (N * C > 2^27 chains)");
    const int D = m->D[0], H = m->H[0], X = m->X, Dp = round_up(D, 16), Hp = round_up(H, 16), Xp = round_up(X, 16), Dh = m->Dp[0];
    if (Hp > 16 * AIS_NT || Dp > 16 * AIS_DT) return fail(IWAE_ERR_ARG, "ais: needs n_hidden <= " + std::to_string(16 * AIS_NT) + " and n_latent <= " + std::to_string(16 * AIS_DT));
    HIPCHK(hipSetDevice(m->cfg.device));
    const int T = o->T, C = o->C;
    const long R = (long)N * C;
    std::vector<float> betas(T + 1);
    HIPCHK(hipMemcpy(betas.data(), o->betas, (size_t)(T + 1) * 4, hipMemcpyDefault));
    for (float b : betas) if (!(b >= 0.0f && b <= 1.0f)) return fail(IWAE_ERR_ARG, "ais: every beta must lie in [0, 1]");
    EvalCall c;
    CHK(eval_begin(m, x, N, c));      // (behind the schedule's check: a bad schedule leaves the handle's streams untouched)
    hipStream_t st = c.st;
    iwae_model::AisWs& w = m->ais;
    const bool user_noise = given == 3, prior = o->init == IWAE_AIS_INIT_PRIOR;
    const float* xrows = c.xd;        // what the chains read: the images, or their coded rows
    if (mask) CHK(mask_rows(c, N, mask, w.mask, w.xin, w.xc, &xrows));
    // ---- base density: the encoder heads in the eval precision, or N(0, I) (head stays null)
    if (!prior) {
        CHK(eval_heads(c, N));
        CHK(eval_copy_heads(c, N, out->q_mu, out->q_sigma));
    } else if (out->q_mu || out->q_sigma) {
        DevBuf& hb = m->ev.head;      // (no heads computed: the constants go out through the head buffer)
        CHK(ensure(hb, (size_t)N * D * 4, st));
        if (out->q_mu) { HIPCHK(hipMemsetAsync(hb.p, 0, (size_t)N * D * 4, st)); CHK(copy_out(m, out->q_mu, hb.p, (size_t)N * D * 4)); }
        if (out->q_sigma) { HIPCHK(hipMemsetD32Async((hipDeviceptr_t)hb.p, 0x3f800000, (size_t)N * D, st)); CHK(copy_out(m, out->q_sigma, hb.p, (size_t)N * D * 4)); }
    }
    const float* head = c.head; const int ldh = c.ldh;
    // ---- the decoder's weights in both orientations, padded to multiples of 16
    AisChainArgs ca;
    memset(&ca, 0, sizeof(ca));
    {
        DecPad p;
        CHK(pad_decoder(m, st, Dp, Hp, Xp, p));
        ca.W1 = p.W1; ca.W1T = p.W1T; ca.W2 = p.W2; ca.W2T = p.W2T; ca.W3 = p.W3; ca.W3T = p.W3T; ca.b1 = p.b1; ca.b2 = p.b2; ca.b3 = p.b3;
    }
    // ---- chain state: e_0 = the caller's draws, (z0 - mu) / sigma, or what iwae_debug_eps(N, C, 0) returns at this step and offset
    CHK(ensure(w.e, (size_t)R * D * 4, st));
    CHK(ensure(w.logw, (size_t)R * 8, st));
    CHK(ensure(w.h, (size_t)R * 4, st));
    CHK(ensure(w.nacc, (size_t)R * 4, st));
    CHK(ensure(w.lpx, (size_t)N * 8, st));
    CHK(copy_in(m, w.betas, betas.data(), (size_t)(T + 1) * 4));
    const float* z0d = nullptr;
    if (o->z0) CHK(staged_in(m, o->z0, w.z0, (size_t)R * D * 4, &z0d));
    else if (user_noise) HIPCHK(hipMemcpyAsync(w.e.p, o->eps0, (size_t)R * D * 4, hipMemcpyDefault, st));
    else CHK(dump_eps(m, N, C, D, w.e));
    AisInitArgs ia;
    memset(&ia, 0, sizeof(ia));
    ia.z0 = z0d; ia.head = head; ia.ldh = ldh; ia.soff = Dh; ia.N = N; ia.D = D; ia.R = R; ia.step = o->step_size;
    ia.e = ptr<float>(w.e); ia.log_w = ptr<double>(w.logw); ia.h = ptr<float>(w.h); ia.nacc = ptr<int>(w.nacc);
    launch_ais_init(ia, st);
    HIPCHK(hipGetLastError());
    const float *momd = nullptr, *unifd = nullptr;
    if (user_noise) {
        CHK(staged_in(m, o->mom, w.mom, (size_t)T * R * D * 4, &momd));
        CHK(staged_in(m, o->unif, w.unif, (size_t)T * R * 4, &unifd));
    }
    float* dHd = nullptr; uint8_t* accd = nullptr;
    if (out->dH) CHK(staged_out(m, out->dH, w.dH, (size_t)T * R * 4, &dHd));
    if (out->accepted || out->accept_rate) CHK(staged_out(m, out->accepted, w.acc, (size_t)T * R, &accd));      // (the rates alone: the flags stay in the workspace)
    ca.D = D; ca.H = H; ca.X = X; ca.Dp = Dp; ca.Hp = Hp; ca.Xp = Xp;
    ca.x = xrows; ca.holes = mask != nullptr; ca.head = head; ca.ldh = ldh; ca.soff = Dh; ca.N = N; ca.C = C; ca.R = R;
    ca.betas = ptr<float>(w.betas); ca.L = o->L; ca.adapt = o->adapt != 0;
    ca.mom = momd; ca.unif = unifd;
    ca.seed = m->cfg.seed; ca.row_offset = (uint64_t)m->batch_offset * (uint64_t)C; ca.step0 = m->noise_step;
    ca.e = ia.e; ca.log_w = ia.log_w; ca.h = ia.h; ca.nacc = ia.nacc; ca.dH = dHd; ca.accepted = accd;
    const int chunk = m->opt.ais_t_chunk > 0 ? m->opt.ais_t_chunk : AIS_T_CHUNK_DEFAULT;
    m->time_this = m->timing > 0;
    for (int t0 = 0; t0 < T; t0 += chunk) {
        ca.t0 = t0; ca.t1 = std::min(T, t0 + chunk);
        ScopedTimer tm(m, T_AIS_CHAIN, st);
        launch_ais_chain(ca, st);
        HIPCHK(hipGetLastError());
    }
    m->time_this = false;
    AisFinishArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.head = head; fa.ldh = ldh; fa.soff = Dh; fa.N = N; fa.C = C; fa.D = D; fa.R = R; fa.e = ia.e; fa.log_w = ia.log_w;
    fa.log_px = ptr<double>(w.lpx);
    if (out->ess) { CHK(ensure(w.ess, (size_t)N * 4, st)); fa.ess = ptr<float>(w.ess); }
    if (out->z) CHK(staged_out(m, out->z, w.z, (size_t)R * D * 4, &fa.z));
    launch_ais_finish(fa, st);
    HIPCHK(hipGetLastError());
    if (out->accept_rate) {
        CHK(ensure(w.rate, (size_t)T * 4, st));
        launch_ais_accept_rate(accd, T, R, ptr<float>(w.rate), st);
        HIPCHK(hipGetLastError());
        CHK(copy_out(m, out->accept_rate, w.rate.p, (size_t)T * 4));
    }
    CHK(copy_out(m, out->log_px, w.lpx.p, (size_t)N * 8));
    if (out->log_w) CHK(copy_out(m, out->log_w, w.logw.p, (size_t)R * 8));
    if (out->ess) CHK(copy_out(m, out->ess, w.ess.p, (size_t)N * 4));
    if (out->step_out) CHK(copy_out(m, out->step_out, w.h.p, (size_t)R * 4));
    CHK(finish_out(m, out->z, fa.z, (size_t)R * D * 4));
    CHK(finish_out(m, out->dH, dHd, (size_t)T * R * 4));
    CHK(finish_out(m, out->accepted, accd, (size_t)T * R));
    CHK(eval_end(c));
    if (!user_noise) m->noise_step += (uint32_t)T + 1u;
    return IWAE_OK;
}
int iwae_ais(iwae_handle m, const float* x, int32_t N, const iwae_ais_options* o, const iwae_ais_outputs* out) { return ais_call(m, x, nullptr, N, o, out); }
// AIS estimate of log p(x_obs) of incomplete images: DESIGN.md section 22
int iwae_ais_masked(iwae_handle m, const float* x, const uint8_t* mask, int32_t N, const iwae_ais_options* o, const iwae_ais_outputs* out) {
    return ais_call(m, x, mask, N, o, out);
}

// Per-image optimisation of a factorised Gaussian q and its evaluation (Cremer, Li & Duvenaud 2018): DESIGN.md section 16
// (mask null: iwae_local_posterior; else iwae_local_posterior_masked, as ais_call)
static int local_call(iwae_handle m, const float* x, const uint8_t* mask, int32_t N, const iwae_local_options* o, const iwae_local_outputs* out) {
    if (!m || !x || !o || !out) return fail(IWAE_ERR_ARG, "local_posterior: need x, options and outputs");
    if (o->struct_size != sizeof(iwae_local_options)) return fail(IWAE_ERR_ARG, "local_posterior: iwae_local_options.struct_size must be sizeof(iwae_local_options) = " + std::to_string(sizeof(iwae_local_options)));
    if (!out->elbo) return fail(IWAE_ERR_ARG, "local_posterior: elbo is required");
    if (N <= 0 || o->S < 1 || o->S > LOCAL_S_MAX || o->T < 0 || o->E < 1) return fail(IWAE_ERR_ARG, "local_posterior: needs N > 0, 1 <= S <= " + std::to_string(LOCAL_S_MAX) + ", T >= 0 and E >= 1");
    if (o->T > LOCAL_PASSES_MAX || o->E > LOCAL_PASSES_MAX) return fail(IWAE_ERR_ARG, "local_posterior: too many passes (T or E > 2^24)");
    if (o->objective != IWAE_LOCAL_ELBO && o->objective != IWAE_LOCAL_IWAE) return fail(IWAE_ERR_ARG, "local_posterior: objective must be IWAE_LOCAL_ELBO or IWAE_LOCAL_IWAE");
    if (!(o->lr >= 0.0f) || !(o->beta_1 >= 0.0f && o->beta_1 < 1.0f) || !(o->beta_2 >= 0.0f && o->beta_2 < 1.0f) || !(o->epsilon > 0.0f))
        return fail(IWAE_ERR_ARG, "local_posterior: needs lr >= 0, beta_1 and beta_2 in [0, 1) and epsilon > 0");
    if ((o->mu0 != nullptr) != (o->sigma0 != nullptr)) return fail(IWAE_ERR_ARG, "local_posterior: mu0 and sigma0 come both or not at all");
    if (m->cfg.n_layers != 1) return fail(IWAE_ERR_ARG, "local_posterior: only the 1-layer model");
    if (m->C != 0 || m->has_prior) return fail(IWAE_ERR_ARG, "local_posterior: only the unconditional model (cond_dim = 0, no learned prior)");
    if ((int64_t)N * o->S > (int64_t)1 << 27) return fail(IWAE_ERR_ARG, "local_posterior: too large (N * S > 2^27 rows)");
    const int D = m->D[0], H = m->H[0], X = m->X, Dp = round_up(D, 16), Hp = round_up(H, 16), Xp = round_up(X, 16), Dh = m->Dp[0];
    if (Hp > 16 * AIS_NT || Dp > 16 * AIS_DT) return fail(IWAE_ERR_ARG, "local_posterior: needs n_hidden <= " + std::to_string(16 * AIS_NT) + " and n_latent <= " + std::to_string(16 * AIS_DT));
    const int S = o->S, T = o->T, E = o->E;
    std::vector<float> alpha;
    try { alpha.resize(T); } catch (const std::bad_alloc&) { return fail(IWAE_ERR_NOMEM, "local_posterior: no host memory for the step sizes of " + std::to_string(T) + " iterations"); }
    EvalCall c;
    CHK(eval_begin(m, x, N, c));
    hipStream_t st = c.st;
    iwae_model::LocalWs& w = m->loc;
    const float* xrows = c.xd;        // what the rows read: the images, or their coded rows
    if (mask) CHK(mask_rows(c, N, mask, w.mask, w.xin, w.xc, &xrows));
    // ---- the start: the caller's, or the encoder heads in the eval precision
    const float *mu0d = nullptr, *sg0d = nullptr;
    if (o->mu0) {
        CHK(staged_in(m, o->mu0, w.mu0, (size_t)N * D * 4, &mu0d));
        CHK(staged_in(m, o->sigma0, w.sg0, (size_t)N * D * 4, &sg0d));
    } else {
        CHK(eval_heads(c, N));
    }
    LocalArgs la;
    memset(&la, 0, sizeof(la));
    {
        DecPad p;
        CHK(pad_decoder(m, st, Dp, Hp, Xp, p));
        la.W1 = p.W1; la.W1T = p.W1T; la.W2 = p.W2; la.W2T = p.W2T; la.W3 = p.W3; la.W3T = p.W3T; la.b1 = p.b1; la.b2 = p.b2; la.b3 = p.b3;
    }
    // ---- per-image state, Adam's step sizes (the bias correction in double, rounded once)
    CHK(ensure(w.st, (size_t)N * 6 * D * 4, st));
    CHK(ensure(w.acc, (size_t)N * 3 * 8, st));
    CHK(ensure(w.qmu, (size_t)N * D * 4, st));
    CHK(ensure(w.qsg, (size_t)N * D * 4, st));
    CHK(ensure(w.mu, (size_t)N * D * 4, st));
    CHK(ensure(w.sg, (size_t)N * D * 4, st));
    CHK(ensure(w.elbo, (size_t)N * 8, st));
    CHK(ensure(w.iwae, (size_t)N * 8, st));
    for (int t = 1; t <= T; ++t) alpha[t - 1] = (float)((double)o->lr * sqrt(1.0 - pow((double)o->beta_2, t)) / (1.0 - pow((double)o->beta_1, t)));
    if (T > 0) CHK(copy_in(m, w.alpha, alpha.data(), (size_t)T * 4));      // (alpha lives until eval_end has synchronised)
    const float* epsd = nullptr;
    if (o->eps) CHK(staged_in(m, o->eps, w.eps, (size_t)(T + E) * S * N * D * 4, &epsd));
    LocalInitArgs ia;
    memset(&ia, 0, sizeof(ia));
    ia.head = c.head; ia.ldh = c.ldh; ia.soff = Dh; ia.mu0 = mu0d; ia.sigma0 = sg0d; ia.N = N; ia.D = D;
    ia.st = ptr<float>(w.st); ia.acc = ptr<double>(w.acc); ia.q_mu = ptr<float>(w.qmu); ia.q_sigma = ptr<float>(w.qsg);
    launch_local_init(ia, st);
    HIPCHK(hipGetLastError());
    float *boundd = nullptr, *gradd = nullptr, *logwd = nullptr;
    if (out->bound && T > 0) CHK(staged_out(m, out->bound, w.bound, (size_t)T * N * 4, &boundd));
    if (out->grad && T > 0) CHK(staged_out(m, out->grad, w.grad, (size_t)N * 2 * D * 4, &gradd));
    if (out->log_w) CHK(staged_out(m, out->log_w, w.logw, (size_t)E * S * N * 4, &logwd));
    la.D = D; la.H = H; la.X = X; la.Dp = Dp; la.Hp = Hp; la.Xp = Xp;
    la.x = xrows; la.holes = mask != nullptr; la.N = N; la.S = S; la.ipw = 64 / S; la.T = T; la.objective = o->objective;
    la.alpha = ptr<float>(w.alpha); la.beta1 = o->beta_1; la.beta2 = o->beta_2; la.epsilon = o->epsilon;
    la.inv_S = 1.0f / (float)S; la.log_S = logf((float)S);
    la.eps = epsd; la.seed = m->cfg.seed; la.row_offset = (uint64_t)m->batch_offset * (uint64_t)S; la.step0 = m->noise_step;
    la.st = ia.st; la.acc = ia.acc; la.bound = boundd; la.grad = gradd; la.log_w = logwd;
    const int chunk = m->opt.local_t_chunk > 0 ? m->opt.local_t_chunk : LOCAL_T_CHUNK_DEFAULT;
    m->time_this = m->timing > 0;
    for (int t0 = 0; t0 < T + E; t0 += chunk) {
        la.t0 = t0; la.t1 = std::min(T + E, t0 + chunk);
        ScopedTimer tm(m, T_LOCAL_Q, st);
        launch_local_q(la, st);
        HIPCHK(hipGetLastError());
    }
    m->time_this = false;
    LocalFinishArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.st = ia.st; fa.acc = ia.acc; fa.N = N; fa.D = D; fa.ES = E * S;
    fa.mu = ptr<float>(w.mu); fa.sigma = ptr<float>(w.sg); fa.elbo = ptr<double>(w.elbo); fa.iwae = ptr<double>(w.iwae);
    launch_local_finish(fa, st);
    HIPCHK(hipGetLastError());
    CHK(copy_out(m, out->elbo, w.elbo.p, (size_t)N * 8));
    if (out->iwae) CHK(copy_out(m, out->iwae, w.iwae.p, (size_t)N * 8));
    if (out->mu) CHK(copy_out(m, out->mu, w.mu.p, (size_t)N * D * 4));
    if (out->sigma) CHK(copy_out(m, out->sigma, w.sg.p, (size_t)N * D * 4));
    if (out->q_mu) CHK(copy_out(m, out->q_mu, w.qmu.p, (size_t)N * D * 4));
    if (out->q_sigma) CHK(copy_out(m, out->q_sigma, w.qsg.p, (size_t)N * D * 4));
    if (boundd) CHK(finish_out(m, out->bound, boundd, (size_t)T * N * 4));      // (T = 0: neither was staged, neither is written)
    if (gradd) CHK(finish_out(m, out->grad, gradd, (size_t)N * 2 * D * 4));
    if (logwd) CHK(finish_out(m, out->log_w, logwd, (size_t)E * S * N * 4));
    CHK(eval_end(c));
    if (!o->eps) m->noise_step += (uint32_t)(T + E);
    return IWAE_OK;
}
int iwae_local_posterior(iwae_handle m, const float* x, int32_t N, const iwae_local_options* o, const iwae_local_outputs* out) { return local_call(m, x, nullptr, N, o, out); }
// The best factorised Gaussian for p(z | x_obs) of incomplete images: DESIGN.md section 22
int iwae_local_posterior_masked(iwae_handle m, const float* x, const uint8_t* mask, int32_t N, const iwae_local_options* o, const iwae_local_outputs* out) {
    return local_call(m, x, mask, N, o, out);
}

// Masked importance-weighted bound on log p(x_obs) and the SNIS estimate of E[x | x_obs] (Mattei & Frellsen 2019): DESIGN.md section 17
int iwae_impute(iwae_handle m, const float* x, int32_t N, const iwae_impute_options* o, const iwae_impute_outputs* out) {
    if (!m || !x || !o || !out) return fail(IWAE_ERR_ARG, "impute: need x, options and outputs");
    if (o->struct_size != sizeof(iwae_impute_options)) return fail(IWAE_ERR_ARG, "impute: iwae_impute_options.struct_size must be sizeof(iwae_impute_options) = " + std::to_string(sizeof(iwae_impute_options)));
    if (!out->log_px) return fail(IWAE_ERR_ARG, "impute: log_px is required");
    CHK(impute_scope(m, "impute", N, o->k));
    const int X = m->X, Xp = round_up(X, 16), S = o->k;
    EvalCall c;
    CHK(eval_begin(m, x, N, c));
    hipStream_t st = c.st;
    iwae_model::ImputeWs& w = m->imp;
    ImputeWeights iw;
    CHK(impute_weights(c, N, S, o->mask, o->eps, out->log_w, out->ess != nullptr, out->q_mu, out->q_sigma, iw));
    ImputeArgs& ia = iw.ia;
    const int nbmax = iw.nbmax, nchunk = iw.nchunk;
    float* xhatd = nullptr;
    if (out->xhat) CHK(staged_out(m, out->xhat, w.xhat, (size_t)N * X * 4, &xhatd));
    if (xhatd && nchunk > 1) CHK(ensure(w.part, (size_t)nbmax * nchunk * Xp * 4, st));
    ia.xhat = xhatd; ia.part = nchunk > 1 ? ptr<float>(w.part) : nullptr;
    // pass (c): the decoder once more with the weights final (only when xhat is wanted)
    for (int i0 = 0; xhatd && i0 < N; i0 += nbmax) {
        ia.img0 = i0; ia.nimg = std::min(nbmax, (int)N - i0);
        {
            ScopedTimer tm(m, T_IMPUTE, st);
            launch_impute_rows(ia, true, st);
        }
        if (nchunk > 1) {
            ImputeMergeArgs ma;
            memset(&ma, 0, sizeof(ma));
            ma.part = ia.part; ma.nimg = ia.nimg; ma.nchunk = nchunk; ma.X = X; ma.Xp = Xp; ma.img0 = i0; ma.xhat = xhatd;
            launch_impute_merge(ma, st);
        }
        HIPCHK(hipGetLastError());
    }
    m->time_this = false;
    CHK(copy_out(m, out->log_px, w.lpx.p, (size_t)N * 8));
    if (out->ess) CHK(copy_out(m, out->ess, w.ess.p, (size_t)N * 4));
    CHK(finish_out(m, out->log_w, iw.logwd, (size_t)S * N * 4));
    CHK(finish_out(m, out->xhat, xhatd, (size_t)N * X * 4));
    CHK(eval_end(c));
    if (!o->eps) m->noise_step += 1;
    return IWAE_OK;
}

// SNIS latent mean and covariance and sampling importance resampling on iwae_impute's weights: DESIGN.md section 18
int iwae_posterior(iwae_handle m, const float* x, int32_t N, const iwae_posterior_options* o, const iwae_posterior_outputs* out) {
    if (!m || !x || !o || !out) return fail(IWAE_ERR_ARG, "posterior: need x, options and outputs");
    if (o->struct_size != sizeof(iwae_posterior_options)) return fail(IWAE_ERR_ARG, "posterior: iwae_posterior_options.struct_size must be sizeof(iwae_posterior_options) = " + std::to_string(sizeof(iwae_posterior_options)));
    if (o->reserved != 0) return fail(IWAE_ERR_ARG, "posterior: iwae_posterior_options.reserved must be 0");
    if (!out->log_px) return fail(IWAE_ERR_ARG, "posterior: log_px is required");
    CHK(impute_scope(m, "posterior", N, o->k));
    if (o->R < 0 || o->R > POSTERIOR_R_MAX) return fail(IWAE_ERR_ARG, "posterior: needs 0 <= R <= " + std::to_string(POSTERIOR_R_MAX));
    if ((int64_t)N * o->R > (int64_t)1 << 27) return fail(IWAE_ERR_ARG, "posterior: too large (N * R > 2^27 draws)");
    if (o->R == 0 && (out->idx || out->z || out->u)) return fail(IWAE_ERR_ARG, "posterior: idx, z and u need R > 0");
    const int D = m->D[0], Dp = round_up(D, 16), S = o->k, R = o->R;
    const bool want_mom = out->mean || out->cov, want_sir = R > 0 && (out->idx || out->z || out->u);
    EvalCall c;
    CHK(eval_begin(m, x, N, c));
    hipStream_t st = c.st;
    iwae_model::ImputeWs& w = m->imp;
    iwae_model::PosteriorWs& pw = m->post;
    ImputeWeights iw;
    CHK(impute_weights(c, N, S, o->mask, o->eps, out->log_w, out->ess != nullptr, out->q_mu, out->q_sigma, iw));
    const ImputeArgs& ia = iw.ia;
    // ---- the moments: launches of whole images, cut by pass (a)'s cap and by the size of the chunk sums
    float *meand = nullptr, *covd = nullptr;
    if (want_mom) {
        const int nchunk = (S + 63) / 64;
        const size_t stride = posterior_part_floats(Dp);
        const int nbm = (int)std::min<size_t>((size_t)iw.nbmax, std::max<size_t>(1, POSTERIOR_PART_FLOATS / ((size_t)nchunk * stride)));
        if (out->mean) CHK(staged_out(m, out->mean, pw.mean, (size_t)N * D * 4, &meand));
        if (out->cov) CHK(staged_out(m, out->cov, pw.cov, (size_t)N * D * D * 4, &covd));
        CHK(ensure(pw.part, (size_t)nbm * nchunk * stride * 4, st));
        PosteriorMomArgs pa;
        memset(&pa, 0, sizeof(pa));
        pa.D = D; pa.Dp = Dp; pa.N = N; pa.S = S; pa.nchunk = nchunk; pa.want_cov = covd ? 1 : 0;
        pa.eps = ia.eps; pa.seed = ia.seed; pa.row_offset = ia.row_offset; pa.step = ia.step;
        pa.log_w = iw.logwd; pa.wstat = ia.wstat; pa.part = ptr<float>(pw.part);
        PosteriorMergeArgs ma;
        memset(&ma, 0, sizeof(ma));
        ma.part = pa.part; ma.nchunk = nchunk; ma.D = D; ma.Dp = Dp; ma.head = c.head; ma.ldh = c.ldh; ma.soff = ia.soff; ma.mean = meand; ma.cov = covd;
        for (int i0 = 0; i0 < N; i0 += nbm) {
            pa.img0 = ma.img0 = i0; pa.nimg = ma.nimg = std::min(nbm, (int)N - i0);
            ScopedTimer tm(m, T_POSTERIOR, st);
            launch_posterior_moments(pa, st);
            launch_posterior_merge(ma, st);
            HIPCHK(hipGetLastError());
        }
    }
    m->time_this = false;
    // ---- the resampling: per launch the running sums of its images, the picks, the picked draws' z
    int32_t* idxd = nullptr;
    float *zd = nullptr, *ud = nullptr;
    if (want_sir) {
        const float* unifd = nullptr;
        if (o->unif) CHK(staged_in(m, o->unif, pw.unif, (size_t)R * N * 4, &unifd));
        CHK(staged_out(m, out->idx, pw.idx, (size_t)R * N * 4, &idxd));      // (always computed: the gather reads it)
        if (out->z) CHK(staged_out(m, out->z, pw.z, (size_t)R * N * D * 4, &zd));
        if (out->u) CHK(staged_out(m, out->u, pw.u, (size_t)R * N * 4, &ud));
        CHK(ensure(pw.cdf, (size_t)iw.nbmax * S * 8, st));
        PosteriorCdfArgs ca;
        memset(&ca, 0, sizeof(ca));
        ca.log_w = iw.logwd; ca.wstat = ia.wstat; ca.N = N; ca.S = S; ca.cdf = ptr<double>(pw.cdf);
        PosteriorPickArgs ka;
        memset(&ka, 0, sizeof(ka));
        ka.cdf = ca.cdf; ka.N = N; ka.S = S; ka.R = R; ka.top = 1;
        while (2 * ka.top <= S) ka.top *= 2;
        ka.unif = unifd; ka.seed = ia.seed; ka.batch_offset = m->batch_offset; ka.step = m->noise_step; ka.idx = idxd; ka.u = ud;
        PosteriorGatherArgs ga;
        memset(&ga, 0, sizeof(ga));
        ga.idx = idxd; ga.D = D; ga.Dp = Dp; ga.N = N; ga.S = S; ga.R = R; ga.head = c.head; ga.ldh = c.ldh; ga.soff = ia.soff;
        ga.eps = ia.eps; ga.seed = ia.seed; ga.row_offset = ia.row_offset; ga.step = ia.step; ga.z = zd;
        for (int i0 = 0; i0 < N; i0 += iw.nbmax) {
            ca.img0 = ka.img0 = ga.img0 = i0; ca.nimg = ka.nimg = ga.nimg = std::min(iw.nbmax, (int)N - i0);
            launch_posterior_cdf(ca, st);
            launch_posterior_pick(ka, st);
            if (zd) launch_posterior_gather(ga, st);
            HIPCHK(hipGetLastError());
        }
    }
    CHK(copy_out(m, out->log_px, w.lpx.p, (size_t)N * 8));
    if (out->ess) CHK(copy_out(m, out->ess, w.ess.p, (size_t)N * 4));
    CHK(finish_out(m, out->log_w, iw.logwd, (size_t)S * N * 4));
    CHK(finish_out(m, out->mean, meand, (size_t)N * D * 4));
    CHK(finish_out(m, out->cov, covd, (size_t)N * D * D * 4));
    CHK(finish_out(m, out->idx, idxd, (size_t)R * N * 4));
    CHK(finish_out(m, out->z, zd, (size_t)R * N * D * 4));
    CHK(finish_out(m, out->u, ud, (size_t)R * N * 4));
    CHK(eval_end(c));
    if (!o->eps || (want_sir && !o->unif)) m->noise_step += 1;
    return IWAE_OK;
}

}  // extern "C"
