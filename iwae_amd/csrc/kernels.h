// Argument blocks and launch wrappers of the kernel files, one section per file (internal; the public ABI is include/iwae_amd.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace iwae {

#define IWAE_DENSE_G1_DEFAULT 29u     // TANH | DX | F32 | BERN (measured: 0.339 -> 0.328 ms/step at B=1024, k=50)
enum { EPI_TANH = 0, EPI_HEAD = 1, EPI_DX = 2, EPI_F32 = 3, EPI_BERN = 4, EPI_SIGMOID = 5 };
enum { OBJ_VAE_ELBO = 0, OBJ_IWAE_ELBO = 1, OBJ_IWAE_EQ14 = 2, OBJ_VAE_ELBO_KL = 3, OBJ_DREG = 4 };
// per-image reductions written by lse_kernel
enum { PB_LME = 0, PB_MEAN, PB_EQ14, PB_KL, PB_PX, PB_T1, PB_T2, PB_DREG, PB_COUNT };
// scalar outputs (device float[16]); must match iwae_scalars in include/iwae_amd.h
enum { SC_VAE_ELBO = 0, SC_VAE_ELBO_KL, SC_IWAE_ELBO, SC_IWAE_EQ14, SC_INFERENCE_LOSS, SC_MEAN_LPXZ, SC_MEAN_T1, SC_MEAN_T2, SC_KL, SC_COUNT = 16 };

// done (in the launchers below): a completion event that rides on the launch's dispatch packet (cheaper on both streams than hipEventRecord behind
// the kernel: LAUNCH_EV in step_helpers.h); launch_out_bwd gives it to its LAST kernel.  A launcher without the argument cannot carry one.

// ---- bf16 step, what walks rows or elements once (row_kernels.hip; iwae_forward, iwae_train_step, iwae_eval_llh): input conversion, noise,
// sampling, log-densities, log-mean-exp, exports.  EpsSrc, LseArgs and SampleArgs are members of the later sections' argument blocks too.
struct EpsSrc {
    const float* user = nullptr;     // [k][B][D] host-supplied draws (reference order) or null -> Philox
    const float* cache = nullptr;    // [rows][ldC] draws eps_gen_kernel made ahead of the step (Philox costs ~40 quarter-rate
    int ldC = 0;                     //   integer multiplies per 4 draws; re-reading 16 B is cheaper than redrawing) or null
    int B = 0;
    uint64_t seed = 0;
    uint64_t row_offset = 0;   // global index of this rank's first data row (batch_offset * k)
    uint32_t step = 0;
    uint32_t stream = 0;       // 0: first latent layer, 1: second
    // k-chunked calls (iwae_eval_llh at large k): this call holds samples [s_off, s_off + kc) of k_total per image; the Philox row
    // index is that of the unchunked call, (image)*k_total + sample, so chunking does not change the draws.  k_total = 0: off.
    int k_total = 0, s_off = 0, kc = 0;
};

struct LseArgs {
    const float* term[5]; float coef[5];
    const float* lq_dreg;
    int B, k; float beta; int objective;
    float cz_on;                         // 1: prior term -z reaches dz (1-layer); 0: 2-layer (handled per row)
    const float* head; int ldH, D, Dp;   // for KL (1-layer) or null
    float* logw; float* wn; float* gx; float4* cf; float* per_b;
    int n_px_part; size_t px_stride;     // term[0] arrives as n partial sums [n][stride] (n <= 1: a plain array)
    float* term0_out;                    // [M] total of term[0] (== term[0] when n_px_part <= 1)
    int lme_only;                        // iwae_eval_llh's launches: only the per-image log-mean-exp and the means are wanted -- no softmax weights / gradient coefficients pass (28 B of stores per row)
    float* gx_local; int gx_r0, gx_n;    // optional: the row weights of rows [gx_r0, gx_r0 + gx_n) also go to gx_local[row - gx_r0] (kernels that do lse_image's work for their own rows: dec_bwd_rows_kernel, bern_pipe_kernel)
};

struct SampleArgs {
    const float* head; int ldH; int Dp; int D; int head_per_row;
    int M, Mp, k, B;
    EpsSrc eps;
    uint16_t* ZP;                     // z as bf16 P-layout [M][Dp], or null
    float* ZF; int ldZF;              // z as float32 rows [M][ldZF] (float32 mode), or null
    const float* prior_head;          // conditional prior: per-image head [B][ldH] (mu_p | sigma_p) scoring z, or null = N(0,1)
    const float* cond; int C;         // conditional model: y [B][C] goes into features D..D+C-1 of the z rows (decoder input concat(z, y))
    float* lp_prior; float* lq; float* lq_dreg;
};

struct GaussLpArgs {
    const float* zhead; int ldZH; int Dzp;   // head that generated z (per image)
    const float* phead; int ldPH; int Dpp;   // head that scores z (per row)
    int D, M, k;
    EpsSrc eps;
    float* out;
};
void launch_prep_rows(const float* x, const float* cond, int B, int X, int C, int Xp, int Bp, uint16_t* XP, hipStream_t st);
void launch_gather_binarize(const uint8_t* data, const int32_t* order, int start, int N, int B, int X, int Xp, int Bp, uint64_t seed,
                            uint32_t epoch, uint16_t* XP, float* xf, hipStream_t st,
                            const uint8_t* labels = nullptr, int C = 0, float* cond_out = nullptr);      // labels: class ids of the resident set (conditional models)
void launch_eps_gen(const EpsSrc& e, int M, int D, int ld, float* out, hipStream_t st, int max_blocks = 0);   // max_blocks > 0: grid-stride over at most that many blocks
void launch_eps_gen_multi(const EpsSrc& e, int M, int D, int ld, float* out, int nsteps, size_t step_stride, hipStream_t st);   // steps e.step .. e.step + nsteps - 1, step s at out + s * step_stride
void launch_sample(const SampleArgs& a, hipStream_t st);
void launch_gauss_lp(const GaussLpArgs& a, hipStream_t st);
void launch_lse(const LseArgs& a, hipStream_t st, hipEvent_t done = nullptr);
void launch_export_rows(const float* in, int B, int k, float* out, hipStream_t st);
void launch_export_z(const SampleArgs& a, float* zout, hipStream_t st);
void launch_snis(const float* z, const float* wn, int B, int k, int D, float* out, hipStream_t st);
void launch_unpack_p(const uint16_t* P, int rows, int F, int Fp, float* out, hipStream_t st);
void launch_eps_dump(const EpsSrc& e, int B, int k, int D, float* out, hipStream_t st);

// ---- bf16 step, forward (kernels.hip, its forward part; iwae_forward, iwae_train_step, iwae_eval_llh): activations and the Bernoulli term; launch_dense also
// launches the dx pass's EPI_DX / EPI_F32 products
struct DenseArgs {
    const uint16_t* X; int ldX;       // P-layout rows [M][ldX], ldX = 32*KT
    const char* img;                  // MG-major A-image of the weight
    int split;                        // EPI_HEAD: out-features >= split are the sigma head (exp + 1e-6)
    int M, KT, MG, mg_per_block;
    int stage_all;                    // run-time K path: stage every window's weights up front (needs mg_per_block * windows <= 4)
    unsigned g1_mask;                 // EPI bit mask: launches (M >= 8192) that take the 8-wave x 16-row shape
    int Np32;                         // out-features that are stored (multiple of 32)
    uint16_t* YP; int ldYP;           // bf16 P-layout out
    float* YF; int ldYF;              // fp32 natural out
    const uint16_t* ACT; int ldACT;   // EPI_DX: stored activation of the out-features (P-layout)
    // EPI_BERN
    const uint16_t* XB; int ldXB; int k; int B; int Xdim;
    // sampled-input mode (dense_kernel<..., ZIN>): z = mu + sigma*eps made in place of reading X (X's layout: ldX = 32*KT)
    const float* zhead; int ldZH;     // encoder head per image [B][ldZH] (mu | sigma at zDp)
    const float* zeps; int zldE; int zD, zDp;   // the step's draws fp32 [rows][zldE]; latent width and its 32-padding (head layout, z rows)
    uint16_t* ZPout;                  // z as bf16 P-layout [M][ldX] (kept for the weight gradient)
    float* zlp; float* zlq;           // per-row log p(z), log q(z|x)
    float* zlq_dreg;                  // DReG (tasks/task02.py:63-65): log q(z|x) with sigma + 1e-6 as the scale, or null (bern_pipe_kernel's prologue only)
    float* lpxz; size_t lpxz_stride;  // log p(x|z) per row; stride > 0: block row y of the grid writes its partial sum to lpxz[y*stride + row]
    float* logits_out;
    int pipe;                         // EPI_BERN: take bern_pipe_kernel where it exists (option no_bern_pipe clears it)
    // bern_pipe_kernel<.., PRE>: the two tanh layers in front of the output layer run inside the same launch (pre_img1 != null)
    const char* pre_img1; int pre_KT1;   // first decoder layer: forward image, k-steps of its input (latent, <= 4)
    const char* pre_img2;                // second decoder layer (KT k-steps in and out)
    const uint16_t* pre_Z;               // z rows, P-layout [M][32*pre_KT1] (when zhead == null; else z is made in the kernel, see ZIN fields)
    uint16_t *pre_G1, *pre_G2;           // the layers' activations, P-layout [M][32*KT], kept for the backward pass (null: forward only, not stored)
    unsigned long long* stamps;       // diagnostic build (IWAE_DENSE_STAMPS) only: [blocks*4 waves][8] phase cycle sums, else null
    // bern_pipe_kernel<.., PRE, QW>, k a divisor of its 200 rows: the workgroup's rows are whole images, so what lse_kernel would do for
    // them (log_w, log-mean-exp, row weights, per-image values: `lse`) runs at the end of the workgroup -- no launch between the decoder
    // forward and the backward pass (lse.term[0] is ignored: log p(x|z) comes from the kernel's own sums)
    int lse_on;
    LseArgs lse;
    // ... and with the row weights in hand it leaves g2w = bf16(g_r * g2) [M][32*KT] (P-layout) for the output layer's weight gradient, which then
    // needs NO row weighting (dW3 = g2w^T s; feature g2w_feat -- a pad column of the hidden width -- carries g_r itself: its product row is the
    // bias gradient).  null: not wanted.
    uint16_t* G2W; int g2w_feat;
    int dbg;                          // DIAG builds only (option fake_s): 32 = the Bernoulli epilogue does not store s
};
// holes (EPI_BERN of a masked call, pipe = 0, a hidden width with out_bwd_has_s_mode): a.XB carries launch_masked_code_bf16's hole codes and the
// epilogue selects those pixels out (dense_kernel<EPI_BERN, .., HOLES>)
void launch_dense(int epi, const DenseArgs& a, hipStream_t st, hipEvent_t done = nullptr, bool holes = false);
bool bern_pipe_ok(const DenseArgs& a);  // shapes bern_pipe_kernel covers (launch_dense falls back to dense_kernel<EPI_BERN> otherwise)
bool bern_lse_ok(const DenseArgs& a);   // ... and can take lse_kernel's work for its rows (DenseArgs.lse_on)

struct BlockFwdArgs {                 // block_fwd_kernel: one BasicBlock on R <= 4096 rows
    const uint16_t* X; int ldX;       // input rows, P-layout [R][32*KT0]
    const float* Xf; int Xdim; uint16_t* XPout;   // or (Xf != null) fp32 rows [R][Xdim], converted on the way in and kept in XPout (P-layout, ldX)
    const char *img0, *img1, *img2;   // MG-major forward images of l1 (KT0 k-steps), l2 and the head (KT1 k-steps each)
    int KT0, KT1;
    int NT1, NT2;                     // stored 16-feature tiles of the hidden layers (= 2*KT1) and of the head (<= 16 each)
    int R;
    uint16_t *H1, *H2; int ldH;       // hidden activations, P-layout [R][32*KT1]
    float* YF; int ldYF; int split;   // head, fp32 [R][ldYF]; out-features >= split are the sigma head
    int sample; SampleArgs S;         // sample != 0: the input rows are z = mu + sigma*eps made HERE (sample_kernel's job, without its launch): S.Dp = 32*KT0
    // oimg != null (decoder on few rows, NT2 = 0): the Bernoulli output layer follows in the same launch -- logits = h2 W3 + c3 from the MG-major
    // image oimg (KT1 k-steps), log p(x|z) per row -> olpxz, s = x - sigmoid(l) -> oSP (P-layout [R][oldS], or null: forward-only call)
    const char* oimg; int oXdim, oH;  // pixels, 32-pixel halves that hold real pixels
    const uint16_t* oXB; int oldXB; int ok;   // x as bf16 P-layout [B][oldXB]; samples per image (row r belongs to image r / ok)
    uint16_t* oSP; int oldS; float* olpxz;
};
bool block_fwd_ok(const BlockFwdArgs& a);
bool block_fwd_shape_ok(const BlockFwdArgs& a);      // block_fwd_ok's shape part: reads no buffer pointer
void launch_block_fwd(const BlockFwdArgs& a, hipStream_t st);

struct Chain2FwdArgs {                // chain2_fwd_kernel: the 2-layer model's per-sample blocks (q(z2|z1) and p(z1|z2)) on M rows, one launch
    uint16_t* Z1P;                    // z1 rows, bf16 P-layout [M][32*KT0]: MADE here (z1 = mu1 + sigma1*eps1, iwae2.py:61) and kept for the decoder and the weight gradient
    float* lqz1x;                     // log q(z1|x) per row (iwae2.py:123)
    const char *e_img1, *e_img2, *e_imgh;     // MG-major forward images of encode_z1_to_z2: l1 (KT0 k-steps), l2, head (KTH k-steps each)
    const char *d_img1, *d_img2, *d_imgh;     // ... of decode_z2_to_z1: l1 (KT1 k-steps), l2, head (KTH k-steps each)
    int M, k, B, D0, D1;              // data rows, samples per image, images; latent widths of z1 and z2
    uint16_t *EH1, *EH2;              // encode block's tanh activations, P-layout [M][32*KTH], kept for the backward pass (null: forward only)
    float* EHEAD;                     // its head, fp32 [M][64*KT1] (mu2 | sigma2), or null
    uint16_t* Z2P;                    // z2 rows, P-layout [M][32*KT1], or null
    uint16_t *DH1, *DH2;              // decode block's tanh activations, or null
    float* DHEAD;                     // its head, fp32 [M][64*KT0] (mu_p | sigma_p), or null
    const float* head1; int ldH1;     // head of q(z1|x) per image [B][ldH1] (mu1 | sigma1 at 32*KT0): z1 in float32 for log p(z1|z2)
    EpsSrc eps1, eps2;                // the draws of z1 and z2
    float *lpz1z2, *lpz2, *lqz2z1;    // per-row log-densities (iwae2.py:122-124)
};
bool chain2_fwd_ok(int KT0, int KTH, int KT1, int M);
void launch_chain2_fwd(const Chain2FwdArgs& a, hipStream_t st);

// ---- bf16 step, dx (kernels.hip, its dX part; iwae_train_step, iwae_forward_backward): gradients back through the activations
struct DecBwdRowsArgs {               // dec_bwd_rows_kernel: the decoder's dX chain on few rows (16-row workgroups, weights straight from L2)
    const uint16_t* SP; int ldS; int KTX;     // s = x - sigmoid(l), P-layout [M][ldS], KTX = ldS/32 pixel k-steps
    const char* imgK3; int MT3;               // K-major image of the output layer's W (block (pixel k-step, hidden tile)), MT3 hidden tiles per k-step
    const char *imgB2, *imgB1;                // backward images of the second / first tanh layer (MG-major, KT k-steps each)
    int KT, NT1, NT3;                         // hidden k-steps, hidden tiles (= 2*KT), latent tiles of dz
    int M;
    const uint16_t *G2, *G1; int ldH;         // stored tanh activations, P-layout [M][32*KT]
    const float* gx;                          // [M] row weights
    uint16_t *D2P, *D1P;                      // dpre2, dpre1 out, P-layout [M][32*KT]
    float* DZ; uint16_t* DZH; int ldDZ;       // dz out: float32 or (DZH != null) bf16, [M][ldDZ]
    // lse_on: the workgroup first does lse_kernel's work (log_w, log-mean-exp over k, row weights, per-image values) for the images its 16 rows
    // belong to -- a wave per image, beside the first weight fragments' round trip -- and takes its rows' weights from LDS: no lse launch
    // between the decoder forward and this kernel (few rows: the step is a chain of dependent launches).  Images that straddle workgroups are
    // done by each of them (identical values).
    int lse_on;
    LseArgs lse;
};
bool dec_bwd_rows_ok(const DecBwdRowsArgs& a);
void launch_dec_bwd_rows(const DecBwdRowsArgs& a, hipStream_t st, hipEvent_t done = nullptr);

struct LatentBwdArgs {
    const float* dz; int ldDZ;
    const uint16_t* dzh;              // dz as bf16 [rows][ldDZ] instead of `dz` (dec_bwd_kernel's output), or null
    const float* dz2; const float* dz3;   // optional further terms of dz (same layout), added on load; both or neither
    const float* head; int ldH; int D, Dp;
    const float4* cf;
    EpsSrc eps;
    int B, Bp, k;
    float kmu, ksig;
    uint16_t* DHP;                    // dhead bf16, P-layout [B][2Dp] (or null)
    float* DHF;                       // float32 mode: dhead as float32 [B][2Dp] (d mu at f, d pre-exp at Dp + f), or null
    const float* prior_head;          // conditional prior p(z|y) (tasks/task04.py:124-130): per-image head [B][ldH] like `head`, or null = N(0,1)
    uint16_t* DHP2;                   // its dhead, P-layout [B][2Dp] (written when prior_head != null)
    float* DHF2;                      // float32 mode: the same as float32 [B][2Dp]
};
void launch_latent_bwd(const LatentBwdArgs& a, hipStream_t st);
struct BlockBwdArgs {                 // block_bwd_kernel: the dX chain of a BasicBlock on R <= 4096 rows
    const uint16_t* DH; int ldDH;     // dhead, bf16 P-layout [R][32*KTH]
    const char *imgH, *imgL2;         // backward images (MG-major: out-feature groups over hidden) of the head (KTH k-steps) and of l2 (KT1)
    int KTH, KT1, NT1;                // NT1 = hidden tiles = 2*KT1
    int R;
    const uint16_t *H2, *H1; int ldH; // stored tanh activations, P-layout [R][32*KT1]
    uint16_t *D2, *D1;                // outputs: dpre of l2 and of l1, P-layout [R][32*KT1]
    // lat_on (the image encoder on few rows): the block's dhead rows are MADE here -- latent_bwd_kernel's per-image sums over the k samples
    // (d mu, d sigma: `lat`), a wave per image in front of the dX chain -- instead of being read from DH; they are also stored to lat.DHP
    // for the head's weight gradient.  One dependent launch less per step.
    int lat_on;
    LatentBwdArgs lat;
    int rows_per_wg;                  // 16, or 4 with lat_on (many samples per image: four waves per image, four times the workgroups)
};
bool block_bwd_ok(const BlockBwdArgs& a);
void launch_block_bwd(const BlockBwdArgs& a, hipStream_t st);

struct OutBwdArgs {
    const uint16_t* G2; int ldG;      // last hidden activation, P-layout [M][32*KT]
    const char* img1;                 // MG-major image of W^T (out = pixels, k = hidden)
    const char* img2;                 // K-major image of W   (out = hidden, k = pixels)
    int Xdim; int Xp32;
    const float* gx;                  // [M] dLoss/dlpxz
    const uint16_t* XB; int ldXB; int k;
    int M, KT, NG;
    uint16_t* DLP;                    // dlogits, P-layout [M][Xp32] or null
    const uint16_t* SP;               // s = x - sigmoid(l) kept by the forward pass, P-layout [M][Xp32]: no recompute (else null)
    float* part; int gpb;             // SP mode, small row counts: block row y handles gpb pixel groups, fp32 partial dg2 in part[y][M][ldG]
    uint16_t* DPP;                    // dpre of the last hidden layer, P-layout [M][32*KT]
    unsigned long long* stamps;       // diagnostic build only: [blocks*4 waves][8] phase cycle sums, else null
    int dbg;                          // DIAG builds only (option fake_s; timing only -- results are wrong): 32 = s rows read from the first 32 rows (no HBM stream)
};
void launch_out_bwd(const OutBwdArgs& a, hipStream_t st, hipEvent_t done = nullptr);

struct DecBwdArgs {                  // dec_bwd_kernel: out_bwd_s + dX of the two tanh layers in one launch
    OutBwdArgs o;                     // SP (s), G2, gx, img1 (W3^T image), M, KT, NG, Xp32, ldG, DPP (dpre2 out); part = null
    const char* imgB2;                // backward image of the second tanh layer ((KT+1)/2 64-out-feature groups over hidden, KT k-steps each)
    const uint16_t* G1;               // stored first-layer activation, P-layout [M][32*KT]
    uint16_t* D1P;                    // dpre1 out, P-layout [M][32*KT]
    const char* imgB1; int MG1;       // backward image of the first decoder layer (out = latent groups, k = hidden)
    float* DZ; int ldDZ;              // dz fp32 [M][ldDZ] (or null)
    uint16_t* DZH;                    // dz as bf16 [M][ldDZ], natural feature order (1-layer model: latent_bwd_kernel is its only reader), or null
    int nw;                           // 8: the 8-wave x 16-row shape (KT = 7 only), else 4 waves x 32 rows
};
bool out_bwd_has_s_mode(int KT);      // hidden widths with a compiled out_bwd_s_kernel / dec_bwd_kernel
void launch_dec_bwd(const DecBwdArgs& d, hipStream_t st, hipEvent_t done = nullptr);

struct GBlockBwdArgs {                // gblock_bwd_kernel: backward of a per-sample BasicBlock of the 2-layer model from its Gaussian head, one launch
    const char* imgH;                 // FORWARD image of the head (KTH k-steps, KTL groups: mu groups then sigma groups): the head is recomputed
    const char *imgBh, *imgB2, *imgB1;   // backward images (MG-major) of the head (2*KTL k-steps), l2 and l1 (KTH k-steps each)
    const uint16_t *H2, *H1;          // the block's stored tanh activations, P-layout [M][32*KTH]
    const float* gx;                  // [M] dLoss/dlog_w of the row
    int M, k, B, D;                   // D: real width of the head's latent
    EpsSrc eps;                       // MODE 0: the draws of z1; MODE 1: the draws of z2
    const float* head1; int ldH1;     // MODE 0: head of q(z1|x) per image (z1 = mu1 + sigma1*eps1 in float32)
    const float* DZIN;                // MODE 1: dz2 from the decode block, float32 [M][32*KTL]
    uint16_t* DHP;                    // dhead, P-layout [M][64*KTL] (for the head's weight gradient)
    uint16_t *D2P, *D1P;              // dpre of l2 / l1, P-layout [M][32*KTH]
    float* DZ2;                       // MODE 0: dz2 out, float32 [M][32*KTIN]
    uint16_t* DZD;                    // MODE 0: out, MODE 1: in -- the direct term of dz1 (-dm), bf16 [M][128] natural feature order
    const float* DZDEC;               // MODE 1: dz1 from the z1 -> x decoder, float32 [M][ldDZDEC]
    int ldDZDEC;
    uint16_t* DZOUT;                  // MODE 1: the three terms of dz1 summed, bf16 [M][32*KTIN] natural feature order (latent_bwd_kernel's input)
};
bool gblock_bwd_ok(int KT0, int KTH, int KT1, int M);
void launch_gblock_bwd(int mode, const GBlockBwdArgs& a, hipStream_t st, hipEvent_t done = nullptr);

struct GaussBwdArgs {
    int mode;
    const float* G;
    const float* head; int ldH; int D, Dp;       // per-row head
    const float* zhead; int ldZH; int Dzp;       // mode 0: head generating z1 (per image)
    const float* dz_in; float* dz_direct; int ldDZ;
    EpsSrc eps;
    int M, Mp, k;
    uint16_t* DHP;                    // dhead bf16 P-layout [M][2Dp], or null
    float* DHF;                       // float32 mode: dhead float32 [M][2Dp], or null
};
void launch_gauss_bwd(const GaussBwdArgs& a, hipStream_t st);

// ---- bf16 step, weight gradients (wgrad_kernels.hip; iwae_train_step, iwae_forward_backward): activations x gradients -> fp32 slabs per row split
struct WgradPArgs {
    const uint16_t* X; int ldX; int IT;     // layer input, P-layout [rows][ldX]; IT = ldX/16 i-tiles
    const uint16_t* G; int ldG; int JT;     // dpre of layer output, P-layout [rows][ldG]
    int M, rows_per_split;                  // valid rows; rows per split (multiple of 64)
    float* slabW;                           // [nsplit][IT*16][JT*16]
    float* slabB;                           // [nsplit][JT*16]
    const char* zero;                       // >= 512 B of zeros (source of rows >= M and of unused slots)
    const float* rowscale;                  // optional [M]: G rows are multiplied by it (rounded to bf16) on the way in, else null
    int dbg;                                // diagnostic ablations (DIAG build, option wg_debug; timing only -- results are wrong): 1 no DMA in the loop, 2 no A reads / MFMAs, 4 no bias sums, 8 no row scaling
    unsigned long long* stamps;             // diagnostic build (STAMPS=1) only: wgradws_kernel's per-wave phase cycle sums [workgroups * waves][8], else null
};
void launch_wgradp(const WgradPArgs& a, int nsplit, int shape, hipStream_t st, hipEvent_t done = nullptr);      // shape: see wgradp_strip
int wgradp_strip(int shape);          // j-tiles (16 out-features each) per block of a shape: 8 -> 8, 16 / 7 -> 16
struct WgradPGroup {                        // up to 3 independent 8-wave weight gradients in one launch
    WgradPArgs a[3];
    int n;
    int gx[3], gy[3];                       // j-blocks / i-blocks of each
    int zbeg[4];                            // first blockIdx.z of each (zbeg[n] = total)
};
void launch_wgradp_group(const WgradPGroup& g, hipStream_t st);
void launch_wgradws_group(const WgradPGroup& g, hipStream_t st);     // shape-7 (specialised waves) gradients, non-row-weighted, in one launch

// ---- bf16 step, update (update_kernels.hip; iwae_train_step, iwae_forward_backward): slabs -> flat gradient -> Adam and the weight images;
// the step's batch means
struct LayerDesc {
    int Kin, Nout, joff;
    size_t offW, offb;                // offsets into the flat parameter / gradient buffers
    char* imgF; int KT_F;             // forward image (rows = out-features)
    char* imgB; int KT_B; int MT_B; int imgB_kmajor;   // backward image (rows = in-features) or null
    const float* slabW; const float* slabB; int nsplit; int slab_ld; size_t slab_stride;
    size_t slabB_stride;              // distance between the row splits' bias sums (0: slab_ld, the usual [nsplit][slab_ld] array; the pre-weighted output layer keeps them as a row of slabW)
    int block_begin;                  // first block of this layer in the flat elementwise grid (256 elements per block)
    int rblock_begin;                 // same for the slab-reduce grid (64 elements per block)
};
// Sums the slabs of reduce blocks [first_block, first_block + nblocks) of the layer table into the flat gradient.
// per_b != null: one extra block turns the per-image values into the batch means (scalars) of the step.
// fuse_adam: the Adam update (grad_scale 1) + weight-image refresh of each element follows its slab sum in the same thread.
void launch_reduce_grads(const LayerDesc* layers, int nlayers, int first_block, int nblocks, float* grad, float* param, float* mom, float* vel,
                         float alpha, float beta1, float beta2, float eps, int fuse_adam, const float* per_b, int B, float beta, float* scalars, hipStream_t st,
                         int first_block2 = 0, int nblocks2 = 0, hipEvent_t done = nullptr);      // (optional second block range of the same launch)
void launch_scalars(const float* per_b, int B, float beta, float* out, hipStream_t st);
void launch_adam(const LayerDesc* layers, int nlayers, int nblocks, float* param, const float* grad, float* mom, float* vel,
                 float alpha, float gscale, float beta1, float beta2, float eps, int do_update, hipStream_t st, int first_block = 0, hipEvent_t done = nullptr);   // blocks [first_block, first_block + nblocks) of the elementwise grid

// wgrad_rows_kernel (round 4): weight gradient of one linear map on FEW rows (<= 2 048) with the whole row reduction inside the workgroup
// and the optimizer update in its epilogue -- no slabs, no reduction launch
#define WGR_MAX_JOBS 6
struct WgradRowsJob {
    const uint16_t* X; int ldX;             // layer input, P-layout [R][ldX]
    const uint16_t* G; int ldG;             // dpre of the layer's outputs, P-layout [R][ldG]
    int R;                                  // valid rows
    const float* rowscale;                  // optional [>= R rounded up to 32]: G rows are multiplied by it on the way in (the output layer: G = the stored s), else null
    int sub0, sub1, split;                  // layer-table index of out-features < split and (merged mu | sigma head) >= split; sub1 = -1: none
    int ib, jb, wg_begin;                   // filled by launch_wgrad_rows: 64-feature blocks of the in / out space, first workgroup
};
// fuse_adam: Keras Adam (grad_scale 1) + image refresh in the epilogue; per_b != null: one extra block makes the step's batch means
void launch_wgrad_rows(const WgradRowsJob* jobs, int njobs, const LayerDesc* layers, float* grad, float* param, float* mom, float* vel, float alpha,
                       float beta1, float beta2, float eps, int fuse_adam, const float* per_b, int B, float beta, float* scalars, const char* zero, hipStream_t st);

// ---- float32 mode (fp32_kernels.hip)
enum { GEMM_EPI_NONE = 0, GEMM_EPI_TANH = 1, GEMM_EPI_EXP = 2, GEMM_EPI_DTANH = 3, GEMM_EPI_BERN = 4 };
struct GemmF32Args {
    const float* A; long sam, sak;        // element (m,k) of op(A) at A[m*sam + k*sak]
    const float* B; long sbk, sbn;        // element (k,n) of op(B) at B[k*sbk + n*sbn]
    float* C; long ldc;                   // C[m*ldc + n]
    int M, N, K;
    const float* bias;                    // [N] or null
    int epi;                              // GEMM_EPI_*: none | tanh | exp(.)+1e-6 | times (1 - ACT^2)
    const float* ACT; long ldact;         // GEMM_EPI_DTANH: stored tanh activation of the outputs
    int accumulate;                       // C += instead of C =
    int kchunk; size_t slab_stride;       // K split over blockIdx.z: split z covers kchunk k's and writes C + z*slab_stride
    int avec, bvec;                       // set by launch_gemm_f32: the operand's quads may be fetched as float4
    int cvec;                             // ... and C (bias, ACT, Cones) may be accessed as float4 (gemm_f32_v2_kernel's transposed epilogue)
    // GEMM_EPI_BERN (128-tile kernel only, forward-only calls): the logits are not stored; every 64-column half tile leaves its partial
    // log p(x|z) = sum_n x_n l_n - softplus(l_n) per row in part[(2 * column tile + half) * part_stride + m]; lse_kernel adds them in fixed order
    const float* XB; int bern_k, bern_X;  // x [B][bern_X] float32 in {0,1}; row m belongs to image m / bern_k
    float* part; size_t part_stride;
    // training step (round 3): GEMM_EPI_BERN with C != null also keeps s = x - sigmoid(l) there (the gradient of that sum wrt l; what the
    // backward pass reads instead of logits), and its consumers take the row weight g_r on the fly instead of a pass that makes dl = g_r s:
    const float* brow_scale;              // element (k,n) of op(B) is multiplied by brow_scale[k] as it is fetched (the weight gradient X^T (g_r s)), or null
    const float* orow_scale;              // row m of the product is multiplied by orow_scale[m] in front of the epilogue (dX = g_r (s W^T) ...), or null
    // weight gradients: op(A) = X^T gets one more row m == M of ONES, whose product row -- the column sums of op(B), i.e. the bias gradient --
    // goes to Cones[z * cones_stride + n] instead of C (round 3: no separate pass over G for the bias gradients)
    float* Cones; size_t cones_stride;
    unsigned long long* stamps;           // diagnostic build (STAMPS=1) only: [workgroups * 4 waves][8] phase cycle sums of gemm_f32_v2_kernel, else null
    int tile_mode;                        // 0: launch_gemm_f32 picks the tile; 1: 4-wave tiles only; 2: 4-wave tiles at <= 3 waves per SIMD (a slot per SIMD stays free for few-row kernels beside it)
    int dbg;                              // diagnostic builds (DIAG=1) only: timing ablations of gemm_f32_v2_kernel (option f32_gemm_dbg; results wrong)
};
// dec_fwd_f32_kernel: the decoder forward in float32 in ONE launch (z -> tanh -> tanh -> logits -> log p(x|z)), rows stationary
struct DecFwdF32Args {
    const float* Z; int ldz; int Din;      // decoder input rows [M][ldz] (z, or concat(z, y)), Din features
    int M, H, X;                           // data rows, hidden width, pixels
    const float *W1, *b1, *W2, *b2, *W3, *b3;      // Keras kernels [in][out] and biases inside the float32 master parameters
    float *G1, *G2; int ldg;               // the tanh activations [M][ldg], kept for the backward pass (null: forward only)
    float* S; int ldS;                     // s = x - sigmoid(l) [M][ldS] for the backward pass, or null
    const float* XB; int k;                // x [B][X] float32 in {0,1}; row m belongs to image m / k
    float* lpxz;                           // [M] log p(x|z) per row
    const char* zero;                      // >= 1 KiB of zeros
    unsigned long long* stamps;            // diagnostic build (STAMPS=1) only: [workgroups * 4 waves][8] phase cycle sums, else null
};
bool dec_fwd_f32_ok(const DecFwdF32Args& a);
void launch_dec_fwd_f32(const DecFwdF32Args& a, hipStream_t st);
// kernel choice of the float32 GEMM launchers: one per handle (iwae_set_option f32_*), handed to every launcher that reads it
struct GemmF32Opts {
    bool v2 = true;                  // false (option f32_gemm_v1 = 1): gemm_f32_big_kernel (the round-3 k loop) instead of gemm_f32_v2_kernel, for A/B measurements
    bool w8 = true;                  // false (option f32_gemm_w4 = 1): no 8-wave tiles
    bool v2_small = true;            // false (option f32_gemm_small_v1 = 1): the round-3 64-tile kernel for every 64 x 64-tiled product
    bool ksplit = true;              // false (option f32_no_ksplit = 1): few-row products as one 64-tile launch walking K alone
    int ksplit_min_tiles = 1;        // option f32_ksplit_min_tiles: 8 = round-5 first version: B >= 100 images only
    int v2_small_min = 1;            // option f32_gemm_small_min: workgroups from which the 64 x 64 launch takes the v2 loop
    int dbg = 0;                     // option f32_gemm_dbg (DIAG builds): timing ablations of gemm_f32_v2_kernel
};
long gemm_f32_tiles(const GemmF32Opts& o, int M, int N, int tile_mode = 0);      // output tiles of the kernel launch_gemm_f32 takes for an M x N product
bool gemm_f32_takes_big(int M, int N, int nsplit);      // launch_gemm_f32's kernel choice (GEMM_EPI_BERN needs the 128-tile kernel)
void launch_gemm_f32(const GemmF32Opts& o, const GemmF32Args& a, int nsplit, hipStream_t st);
int gemm_f32_fewrows_split(const GemmF32Opts& o, int M, int N, int K);      // > 1: launch_gemm_f32_fewrows splits K that many ways (scratch: split * M * N floats)
void launch_gemm_f32_fewrows(const GemmF32Opts& o, const GemmF32Args& a, float* slabs, hipStream_t st);
int gemm_f32_slots(const GemmF32Opts& o, int M, int N, int tile_mode = 0);       // workgroups of launch_gemm_f32's kernel for an M x N product the chip holds at once
void launch_reduce_slabs_f32(const float* slabs, size_t stride, int nsplit, size_t n, float* out, hipStream_t st);
// every slab sum of a float32 step in one launch (round 5): out[i] = sum over the job's slabs, i < n; block_begin is filled by the launcher
#define REDUCE_SLABS_MAX_JOBS 40
struct ReduceSlabsJob { const float* slabs; size_t stride; size_t n; float* out; int nsplit; int block_begin; };
struct ReduceSlabsJobs { ReduceSlabsJob job[REDUCE_SLABS_MAX_JOBS]; int n; };
void launch_reduce_slabs_multi_f32(ReduceSlabsJobs& jobs, hipStream_t st);
void launch_bern_f32(const float* logits, size_t ld, const float* x, int X, int M, int k, float* lpxz, hipStream_t st);
void launch_dl_f32(float* logits, size_t ld, const float* x, int X, int M, int k, const float* gx, hipStream_t st);
// ---- the masked float32 step (masked_kernels.hip): mask [B][X] uint8, non-zero = observed; what x holds elsewhere is never an operand
void launch_masked_bern_f32(const float* logits, size_t ld, const float* x, const uint8_t* mask, int X, int M, int k, float* lpxz, hipStream_t st);      // log p(x_obs|z) per row
void launch_masked_s_f32(float* logits, size_t ld, const float* x, const uint8_t* mask, int X, int M, int k, hipStream_t st);      // in place: s = m ? x - sigmoid(l) : 0
void launch_masked_code(const float* x, const uint8_t* mask, long n, float* xc, hipStream_t st);      // xc = m ? x : the hole code masked_out_f32_kernel compares against
// the masked bf16 step: XC = bf16 P-layout rows [Bp][Xp] of m ? bf16(x) : BF16_HOLE (pad pixels and pad rows 0), what dense_kernel<EPI_BERN, .., HOLES> reads as XB
void launch_masked_code_bf16(const float* x, const uint8_t* mask, int B, int X, int Xp, int Bp, uint16_t* XC, hipStream_t st);
// masked_out_f32_kernel: the output layer g2 W3 + b3 with the masked likelihood [+ s] in its epilogue, rows stationary; no logits in memory
struct MaskedOutF32Args {
    const float* G2; int ldg;              // the second tanh layer's activations [M][ldg]
    int M, H, X;                           // data rows, hidden width, pixels
    const float *W3, *b3;                  // the Keras kernel [H][X] and bias inside the float32 master parameters
    const float* XC; int k;                // launch_masked_code's [B][X]; row m belongs to image m / k
    float* S; int ldS;                     // s = m ? x - sigmoid(l) : 0 [M][ldS] for the backward pass, or null (forward only)
    float* lpxz;                           // [M] log p(x_obs|z) per row
    const char* zero;                      // >= 1 KiB of zeros
    int kslabs;                            // > 0: the general route's output-layer GEMM splits K into chunks of 16 kslabs in-features (launch_gemm_f32_fewrows); the kernel adds its partial chains the same way
};
bool masked_out_f32_ok(const MaskedOutF32Args& a);      // reads H, X, k, W3, b3
void launch_masked_out_f32(const MaskedOutF32Args& a, hipStream_t st);
// ---- the resident per-image masks: bits [n][W], W = ceil(X / 32) words per image, pixel f = bit f & 31 of word f >> 5, set = observed
inline int mask_words(int X) { return (X + 31) / 32; }
void launch_mask_pack(const uint8_t* mask, int n, int X, uint32_t* bits, hipStream_t st);      // a device [n][X] byte mask (non-zero = observed) -> bits
void launch_mask_mcar(int n, int X, uint32_t thr, uint64_t key, uint32_t* bits, hipStream_t st);      // pixel f of image i hidden iff (philox((i, 'MASK', f / 4, 0), key)[f % 4] >> 8) < thr
// gather_binarize_masked_kernel: gather_binarize_kernel's batch (rows start.. of the order, the same binarised bits) under the images' masks, in
// one launch every form of it a masked step reads; a null output is not written
struct GatherMaskedArgs {
    const uint8_t* data; const int32_t* order; const uint32_t* bits;      // the resident set [N][X], the epoch's order, the masks [N][W]
    int start, B, X, Xp, Bp;
    uint64_t seed; uint32_t epoch;
    uint16_t* XP;                          // bf16 P-layout rows [B][Xp] of xin = m ? bit : 0 (the encoder's input)
    uint16_t* XC;                          // bf16 P-layout rows [Bp][Xp] of m ? bf16(bit) : BF16_HOLE, pad pixels and pad rows 0 (launch_masked_code_bf16's)
    float* xin;                            // float32 xin [B][X]
    uint8_t* mask;                         // the batch's mask bytes [B][X], 0 / 1
    float* xcode;                          // float32 m ? bit : the hole code [B][X] (launch_masked_code's)
};
void launch_gather_binarize_masked(const GatherMaskedArgs& a, hipStream_t st);
void launch_sigmoid_f32(float* v, size_t n, hipStream_t st);
void launch_export_mat(const float* in, int B, int k, int X, float* out, hipStream_t st);
void launch_concat_f32(const float* a, int na, const float* b, int nb, int rows, float* out, hipStream_t st);

// ---- latent-grid quadrature (grid_kernels.hip; iwae_grid_posterior): the true posterior p(z|x) of a model with a few latent
// dimensions on a grid of points z_g with log weights w_g, and log p(x) = LSE_g (log p(x|z_g) + log p(z_g) + w_g)
#define GRID_D_MAX 4            // latent dimensions
#define GRID_XP_MAX 800         // padded pixels: the score kernel keeps an image's 25 k-steps of x in registers
#define GRID_RANGE 1024         // grid rows per partial state: a chunk of Gc rows is cut into ceil(Gc / GRID_RANGE) ranges (depends on Gc only)
// per-image partial state: [0] running max m, [1] sum s = sum exp(t - m), [2..5] S1_d = sum e (z - mu)_d, [6..15] S2 (packed upper
// triangle, grid_tri(d, e)) = sum e (z - mu)_d (z - mu)_e, [16] Q = sum exp(lq + w), [17] A = sum exp(lq + w) (lq - lj)
enum { GRID_ST = 18, GRID_S1 = 2, GRID_S2 = 6, GRID_Q = 16, GRID_A = 17 };
__host__ __device__ inline int grid_tri(int d, int e) { return d * GRID_D_MAX - d * (d - 1) / 2 + (e - d); }
struct GridPrepArgs {
    const float* logits; int ldl;          // decoder logits of the chunk's points, fp32 [Gc][ldl]
    const float* z; const float* lw;       // the chunk's points [Gc][D] and log weights [Gc] (null: 0)
    int Gc, Gcp, X, Xp, D;                 // rows, rows written (a multiple of 16; rows >= Gc are zero), pixels, padded pixels, latent dims
    uint16_t *Lhi, *Llo;                   // out: bf16(l), bf16(l - bf16(l)) [Gcp][Xp], pixels >= X zero
    float* c; float4* zc; float* w;        // out: c_g = log p(z_g) - sum_j softplus(l_gj) + w_g, z_g padded to 4, w_g   [Gcp]
};
struct GridScoreArgs {
    const uint16_t* XB; int Xp;            // images as bf16 [round_up(N, 64)][Xp] (exact: x in {0,1}), pad rows / pixels zero
    const uint16_t *Lhi, *Llo; const float* c; const float4* zc; const float* w;      // grid_prep_kernel's outputs
    const float* head; int ldh, soff;      // encoder heads: mu_id at head[i*ldh + d], sigma_id at head[i*ldh + soff + d]
    int N, Gc, nsplit;
    float* part;                           // out: [nsplit][N][GRID_ST]
    float* log_joint; long ldlj; long lj_col;      // out (or null): log p(x_i|z_g) + log p(z_g) at [i*ldlj + lj_col + g]
};
struct GridMergeArgs {
    const float* part; int nsplit, N, D;
    double* run;                           // [N][GRID_ST] running state across the chunks of G
    int first, last;                       // first chunk: start from the empty state; last chunk: finalise into the outputs
    const float* head; int ldh;            // mu (the moments are taken about it)
    double* log_px; float *mean, *cov, *qmass, *kl;     // [N], [N][D], [N][D][D], [N], [N]
};
void launch_grid_prep_x(const float* x, int N, int X, int Np, int Xp, uint16_t* XB, int* nonbinary, hipStream_t st);
void launch_grid_prep(const GridPrepArgs& a, hipStream_t st);
void launch_grid_score(const GridScoreArgs& a, int D, hipStream_t st);
void launch_grid_merge(const GridMergeArgs& a, hipStream_t st);

// ---- active units (activity_kernels.hip; iwae_latent_activity): per-unit Cov_x(E_q[u|x]).  An image's mu2 rows are summed per block of
// ACT_BLOCK samples into a partial [image][block][D1]; the statistics kernel folds the partials and reduces over the images in double
#define ACT_BLOCK 128
struct ActChainArgs {                 // act_chain_kernel: the 2-layer model's q(z2|z1) mean on nb images x kn samples, summed per block
    const char *img1, *img2, *imgh;   // MG-major forward images of encode_z1_to_z2: l1 (KT0 k-steps), l2, head (KTH k-steps each; mu groups first)
    const float* head1; int ldH1;     // q(z1|x) heads of this launch's images [nb][ldH1] (mu1 | sigma1 at 32*KT0)
    EpsSrc eps1;                      // the draws of z1 (user [k][B][D0] at this launch's first sample and image, or Philox with k_total set)
    int kn, D0, D1;                   // samples per image in this launch, latent widths of z1 and z2
    float* part; int nblk;            // out: [N][nblk][D1] partial sums of mu2, nblk = ceil(k / ACT_BLOCK)
    int img0, blk0;                   // this launch's first image and first block
};
struct ActPartialArgs {               // act_partial_kernel: the same partials from mu2 rows [nb * kn][ldh] that composed launches made
    const float* head; int ldh;
    int nb, kn, D1;
    float* part; int nblk, img0, blk0;
};
struct ActStatsArgs {                 // act_stats_kernel: one unit per workgroup
    const float* src; long ld_img; int ld_blk, nblk;   // image i's partials of unit u at src[i*ld_img + j*ld_blk + u], j < nblk
    double kdiv;                      // per-image mean = (sum of the partials, double) / kdiv
    int N, D;                         // images, units of this layer
    float* post_mean; int ldpm, col;  // out: [N][ldpm], this layer's units from column col
    double *activity, *data_mean;     // out: [.] from index col
};
bool act_chain_ok(int KT0, int KTH, int KT1);
void launch_act_chain(const ActChainArgs& a, int nb, hipStream_t st);
void launch_act_partial(const ActPartialArgs& a, hipStream_t st);
void launch_act_stats(const ActStatsArgs& a, hipStream_t st);

// ---- gradient moments (moments_kernels.hip; iwae_grad_moments): per-parameter Welford fold of M gradient draws, in double
struct MomentsFoldArgs {              // moments_fold_kernel: draw j (1-based) of the flat gradient g [n] into mean [n] and M2 [n]
    const float* g;
    double *mean, *m2;
    size_t n;
    int j;
};
struct MomentsFinalizeArgs {          // moments_finalize_kernel: out_var = M2 / (M - 1); out_mean = mean unless null (mean already in place)
    const double *mean, *m2;
    double *out_mean, *out_var;
    size_t n;
    int M;
};
void launch_moments_fold(const MomentsFoldArgs& a, hipStream_t st);
void launch_moments_finalize(const MomentsFinalizeArgs& a, hipStream_t st);

// ---- aggregate posterior (aggregate_kernels.hip; iwae_aggregate_posterior): log q(z) and its per-unit marginals at the samples of q(z|x_n).
// Sample i = s N + n; a launch group handles samples [i0, i0 + T) against all N components, cut into ranges of AGG_RANGE components (their
// number depends on N only) and, for the per-unit sums, into groups of AGG_DC units.  Dpad = round_up(D, AGG_DC) <= 128.
#define AGG_DC 16               // units per agg_dim_kernel block; the padded unit width
#define AGG_RANGE 512           // components per partial
#define AGG_TILE 16384          // samples per launch group (bounds the partial buffers)
struct AggCompArgs {                  // agg_comp_kernel: heads [N][ldh] (mu | sigma at soff) -> tables [N][Dpad] in log2 units
    const float* head; int ldh, soff, N, D, Dpad;
    float *mu, *inv, *nls;            // mu, sqrt(log2(e)/2) / sigma, -log2(e) (log sigma + log(2 pi)/2)
    double *invd, *nls_sum;           // the scale in double; [N] sum_d -log2(e) (log sigma + log(2 pi)/2) in double (the joint density's)
};
struct AggSampleArgs {                // agg_sample_kernel: z and the own-component term of samples [i0, i0 + T), transposed [Dpad][T]
    const float* head; int ldh, soff, N, D, Dpad;
    const float* eps;                 // [S][N][D]
    const float *mu, *inv, *nls;
    long i0; int T;
    float *zT, *shT;
};
struct AggMainArgs {                  // agg_dim_kernel + agg_joint_kernel
    const float *mu, *inv, *nls; const double *invd, *nls_sum; int N, Dpad;
    const float *zT, *shT; int T;
    float* dim_part;                  // [P][Dpad][T] per-unit sums of exp2(term - own term)
    double* joint_max; float* joint_sum;   // [P][T] running maximum (log2 units) and sum of the joint density
};
struct AggMergeArgs {                 // agg_merge_kernel: partials of P ranges -> log_qz [SN] and log_qzdT [Dpad][ldo] at column i0
    const float* dim_part; const double* joint_max; const float *joint_sum, *shT; int P, Dpad, T;
    double log_n;
    float* log_qz; float* log_qzdT; long ldo, i0;
};
struct AggReduceArgs {                // agg_reduce_kernel + agg_finish_kernel
    const float* head; int ldh, soff, N, D;
    const float* eps; long SN;
    const float *log_qz, *log_qzdT;   // [SN], [Dpad][SN]
    double* part;                     // [(D + 1)][5] block sums
    double *summary, *unit_kl, *unit_mi;
};
void launch_agg_comp(const AggCompArgs& a, hipStream_t st);
void launch_agg_sample(const AggSampleArgs& a, hipStream_t st);
void launch_agg_main(const AggMainArgs& a, hipStream_t st);
void launch_agg_merge(const AggMergeArgs& a, hipStream_t st);
void launch_agg_untranspose(const float* src, long SN, int D, float* dst, hipStream_t st);
void launch_agg_reduce(const AggReduceArgs& a, hipStream_t st);

// ---- annealed importance sampling (ais_kernels.hip; iwae_ais): C HMC chains per image through T temperatures, float32.  Chain row
// r = c N + n (the reference's [C, N] order) keeps its state e [R][D], log_w [R] (double), step size h [R] and accept count [R] in HBM between
// launches; ais_chain_kernel runs transitions [t0, t1) of 64 rows per workgroup, a wave owning 16 rows.  Philox row of chain (n, c):
// row_offset + n C + c (iwae_eval_llh's at k = C).
#define AIS_NT 13               // out-feature tiles (16 each) a wave accumulates: hidden width <= 208
#define AIS_DT 8                // latent tiles: n_latent <= 128
#define AIS_TPO 4               // pixel tiles per pass of the output layer (the residual tile that feeds s W3^T)
#define AIS_SLABP 212           // weight slab pitch in floats (16 in-features x <= 208 out-features)
struct AisPrepArgs {                  // ais_pad_kernel: src [K][N] (Keras kernel inside the master parameters) -> dst [Kp][Np] and dstT [Np][Kp], pads zero
    const float* src; int K, N, Kp, Np;
    float *dst, *dstT;                // dstT null: not wanted (biases: K = 1)
};
struct AisInitArgs {                  // ais_init_kernel: log_w = 0, h = step, accepts = 0; with z0: e = (z0 - mu) / sigma
    const float* z0;                  // [R][D] or null (e already holds the draws)
    const float* head; int ldh, soff; // encoder heads per image, or null (prior init: mu = 0, sigma = 1)
    int N, D; long R;
    float step;
    float* e; double* log_w; float* h; int* nacc;
};
struct AisChainArgs {
    const float *W1, *W1T, *W2, *W2T, *W3, *W3T, *b1, *b2, *b3;      // padded to multiples of 16 (ais_pad_kernel): W [in][out], WT [out][in]
    int D, H, X, Dp, Hp, Xp;
    const float* x;                   // [N][X]
    const float* head; int ldh, soff; // mu at head[n ldh + d], sigma soff further; null: prior init
    int N, C; long R;
    const float* betas;               // [T + 1] on the device
    int t0, t1, L, adapt;
    const float* mom; const float* unif;      // the caller's noise [T][R][D], [T][R] or null: Philox streams 3 / 4 at step0 + t
    uint64_t seed, row_offset; uint32_t step0;
    float* e; double* log_w; float* h; int* nacc;
    float* dH; uint8_t* accepted;     // [T][R] or null
    int holes;                        // != 0 (iwae_ais_masked): x holds launch_masked_code's rows m ? x : the hole code, the launch takes ais_chain_kernel<true>
};
struct AisFinishArgs {                // ais_finish_kernel: z = mu + sigma e; per image log_px = LSE_c log_w - log C and the effective sample size
    const float* head; int ldh, soff;
    int N, C, D; long R;
    const float* e; const double* log_w;
    float* z; double* log_px; float* ess;      // z, ess: null = not wanted
};
size_t ais_chain_lds_bytes(int Dp, int Hp);
void launch_ais_pad(const AisPrepArgs& a, hipStream_t st);
void launch_ais_init(const AisInitArgs& a, hipStream_t st);
void launch_ais_chain(const AisChainArgs& a, hipStream_t st);
void launch_ais_finish(const AisFinishArgs& a, hipStream_t st);
void launch_ais_accept_rate(const uint8_t* accepted, int T, long R, float* rate, hipStream_t st);

// ---- per-image posterior optimisation (local_kernels.hip; iwae_local_posterior): S draws per image and pass, float32, ais_chain_kernel's
// blocking and row evaluation.  A workgroup (4 waves x 16 rows) owns ipw = 64 / S whole images, rows image-major (local row i S + s), the rest
// dead; between passes an image's state st [N][6][D] = mu | rho = log sigma | Adam's m, v of mu | m, v of rho lives in HBM / L2.  Pass t < T
// is an Adam iteration on the draws of step0 + t; pass T + j evaluation pass j (no update): log_w summed into acc [N][3] (double).
#define LOCAL_S_MAX 64
struct LocalInitArgs {                // local_init_kernel: the start (the caller's, else the encoder heads), m = v = 0, acc = (0, -inf, 0)
    const float* head; int ldh, soff; // encoder heads per image (used where mu0 is null)
    const float *mu0, *sigma0;        // [N][D] or null
    int N, D;
    float* st; double* acc;
    float *q_mu, *q_sigma;            // [N][D]: where it started
};
struct LocalArgs {
    const float *W1, *W1T, *W2, *W2T, *W3, *W3T, *b1, *b2, *b3;      // padded to multiples of 16 (ais_pad_kernel): W [in][out], WT [out][in]
    int D, H, X, Dp, Hp, Xp;
    const float* x;                   // [N][X]
    int N, S, ipw;
    int t0, t1, T, objective;         // passes [t0, t1) of this launch; T iterations in all; iwae_local_objective
    const float* alpha;               // [T] on the device: lr sqrt(1 - beta_2^t) / (1 - beta_1^t), t = pass + 1
    float beta1, beta2, epsilon, inv_S, log_S;
    const float* eps;                 // the caller's draws [T + E][S][N][D] or null: Philox stream 0 at step0 + pass, row row_offset + n S + s
    uint64_t seed, row_offset; uint32_t step0;
    float* st; double* acc;
    float* bound;                     // [T][N] or null
    float* grad;                      // [N][2 D] or null: the ascent direction of iteration T - 1
    float* log_w;                     // [E S][N] or null
    int holes;                        // != 0 (iwae_local_posterior_masked): x holds launch_masked_code's rows m ? x : the hole code, the launch takes local_q_kernel<true>
};
struct LocalFinishArgs {              // local_finish_kernel: mu, sigma = exp(rho); elbo = sum / (E S), iwae = max + log(sum exp) - log(E S)
    const float* st; const double* acc;
    int N, D, ES;
    float *mu, *sigma; double *elbo, *iwae;
};
size_t local_q_lds_bytes(int Dp, int Hp);
void launch_local_init(const LocalInitArgs& a, hipStream_t st);
void launch_local_q(const LocalArgs& a, hipStream_t st);
void launch_local_finish(const LocalFinishArgs& a, hipStream_t st);

// ---- masked importance-weighted bound and SNIS imputation (impute_kernels.hip; iwae_impute): S draws per image, float32, local_q_kernel's
// blocking and the forward half of its row evaluation.  Rows image-major; S <= 64: a workgroup owns ipw = 64 / S whole images (nchunk = 1),
// S > 64: chunk c of nchunk = ceil(S / 64) of one image.  A launch holds the whole images [img0, img0 + nimg).
struct ImputeArgs {                   // impute_rows_kernel<false>: pass (a), writes log_w; <true>: pass (c), reads log_w and wstat, writes xhat / part
    const float *W1, *W2, *W3, *b1, *b2, *b3;      // padded to multiples of 16 (ais_pad_kernel): W [in][out]
    int D, H, X, Dp, Hp, Xp;
    const float* x;                   // [N][X]: the masked input m ? x : 0 (the caller's x where mask is null)
    const uint8_t* mask;              // [N][X], non-zero = observed, or null: every pixel observed
    const float* head; int ldh, soff; // mu at head[n ldh + d], sigma soff further
    int N, S, ipw, nchunk;            // N: the call's images (the stride of eps and log_w)
    int img0, nimg;                   // this launch's images
    const float* eps;                 // the caller's draws [S][N][D] or null: Philox stream 0 at `step`, row row_offset + n S + s
    uint64_t seed, row_offset; uint32_t step;
    float* log_w;                     // [S][N]
    const float2* wstat;              // [N]: (max_s log_w, 1 / sum_s exp(log_w - max)) of impute_stats_kernel
    float* xhat;                      // [N][X] (nchunk == 1)
    float* part;                      // [nimg][nchunk][Xp] (nchunk > 1): the chunks' sums, for impute_merge_kernel
};
struct ImputeStatsArgs {              // impute_stats_kernel: per image, in sample order: log_px = LSE_s log_w - log S and ess (double), wstat
    const float* log_w; int N, S;
    double* log_px; float* ess;       // ess: null = not wanted
    float2* wstat;
};
struct ImputeMergeArgs {              // impute_merge_kernel: xhat[img0 + i] = min(1, sum_c part[i][c]) in chunk order
    const float* part; int nimg, nchunk, X, Xp, img0;
    float* xhat;
};
size_t impute_lds_bytes(int Dp, int Hp);
void launch_impute_mask(const float* x, const uint8_t* mask, long n, float* xin, hipStream_t st);      // xin = mask ? x : 0
void launch_impute_rows(const ImputeArgs& a, bool xhat, hipStream_t st);
void launch_impute_stats(const ImputeStatsArgs& a, hipStream_t st);
void launch_impute_merge(const ImputeMergeArgs& a, hipStream_t st);

// ---- SNIS latent moments and posterior resampling (posterior_kernels.hip; iwae_posterior): on the log_w [S][N] and wstat of iwae_impute's
// passes (a) and (b).  The moments are taken in the standardised variable e (z = mu + sigma e): a workgroup owns chunk c of
// nchunk = ceil(S / 64) of one image; a launch holds the whole images [img0, img0 + nimg).  A draw is regenerated from its index, never stored.
struct PosteriorMomArgs {             // posterior_moments_kernel: per chunk m1[d] = sum_s al_s e_sd and (cov wanted) m2[d][d'] = sum_s (al_s e_sd) e_sd', d-tile <= d'-tile
    int D, Dp;
    int N, S, nchunk;                 // N: the call's images (the stride of eps and log_w)
    int img0, nimg;                   // this launch's images
    int want_cov;
    const float* eps;                 // the caller's draws [S][N][D] or null: Philox stream 0 at `step`, row row_offset + n S + s
    uint64_t seed, row_offset; uint32_t step;
    const float* log_w;               // [S][N]
    const float2* wstat;              // [N]: (max_s log_w, 1 / sum_s exp(log_w - max))
    float* part;                      // [nimg][nchunk][Dp Dp + Dp]: m2 (row-major, the upper tiles only), then m1
};
struct PosteriorMergeArgs {           // posterior_merge_kernel: the chunks in chunk order in double -> mean [N][D], cov [N][D][D]
    const float* part; int nimg, nchunk, D, Dp, img0;
    const float* head; int ldh, soff;
    float *mean, *cov;                // either may be null
};
struct PosteriorCdfArgs {             // posterior_expw_kernel, then posterior_cdf_kernel: c[s][i] = sum_{j <= s} exp((double)(log_w_j - max)), image img0 + i, sample order
    const float* log_w; const float2* wstat; int N, S, img0, nimg;
    double* cdf;                      // [S][nimg]
};
struct PosteriorPickArgs {            // posterior_pick_kernel: idx[r][n] = the smallest s with c_s > u c_{S-1} (u = 1: the first s that reaches c_{S-1})
    const double* cdf; int N, S, R, img0, nimg, top;      // top: the largest power of two <= S
    const float* unif;                // the caller's uniforms [R][N] or null: Philox stream 5 at `step`, row (batch_offset + n) R + r, word 0
    uint64_t seed, batch_offset; uint32_t step;
    int32_t* idx;                     // [R][N]
    float* u;                         // [R][N] or null: the uniforms used
};
struct PosteriorGatherArgs {          // posterior_gather_kernel: z[r][n] = mu + exp(log sigma) e_idx, e regenerated (or gathered from the caller's eps)
    const int32_t* idx; int D, Dp, N, S, R, img0, nimg;
    const float* head; int ldh, soff;
    const float* eps; uint64_t seed, row_offset; uint32_t step;
    float* z;                         // [R][N][D]
};
size_t posterior_lds_bytes(int Dp);
size_t posterior_part_floats(int Dp);      // per (image, chunk)
void launch_posterior_moments(const PosteriorMomArgs& a, hipStream_t st);
void launch_posterior_merge(const PosteriorMergeArgs& a, hipStream_t st);
void launch_posterior_cdf(const PosteriorCdfArgs& a, hipStream_t st);
void launch_posterior_pick(const PosteriorPickArgs& a, hipStream_t st);
void launch_posterior_gather(const PosteriorGatherArgs& a, hipStream_t st);

}  // namespace iwae
