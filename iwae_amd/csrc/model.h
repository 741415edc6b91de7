// What the host translation units of libiwae_amd.so share: the handle (iwae_model), its workspaces, the helpers model.hip defines and
// analysis.hip, step_bf16.hip and step_f32.hip call, and the two steps' entry points (step_bf16.hip, step_f32.hip).  Internal to the
// library -- everything here has hidden visibility, the exported surface is include/iwae_amd.h alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <type_traits>
#include <vector>
#include <rccl/rccl.h>       // types only: RCCL is loaded with dlopen at iwae_comm_init, the library does not link against it
#include "../../include/iwae_amd.h"
#include "kernels.h"

#pragma GCC visibility push(hidden)

int fail(int code, const std::string& msg);      // keeps msg for iwae_last_error (this thread's) and returns code
#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail(e_ == hipErrorOutOfMemory ? IWAE_ERR_NOMEM : IWAE_ERR_HIP,                     \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                            \
    } while (0)
#define CHK(expr) do { int rc_ = (expr); if (rc_ != IWAE_OK) return rc_; } while (0)

struct DevBuf { void* p = nullptr; size_t cap = 0; };
struct KerasLayer { std::string name; int Kin, Nout; size_t offW, offb; };

// one GEMM-able linear map; the mu|sigma head merges two Keras layers into one (joff = 0 / Dp)
struct Linear {
    int Kin = 0, Nspace = 0;          // in-features, out-feature space (heads: 2*Dp)
    int Kp32 = 0, Np32 = 0, KT = 0, MG = 0;
    int nsub = 0, sub[2] = {0, 0}, joff[2] = {0, 0};
    char* imgF = nullptr; size_t imgF_bytes = 0;
    char* imgB = nullptr; size_t imgB_bytes = 0; int KT_B = 0, MG_B = 0, MT_B = 0, kmajor = 0;
    DevBuf slabW, slabB;
    int IT = 0, JT = 0, nsplit = 1;
};

struct BlockWs { DevBuf h1P, h2P, head, dheadP, d2P, d1P, dx; };   // activations / gradients of one BasicBlock applied to R rows
struct MlpWs {     // decode_z_to_x applied to M rows
    DevBuf g1P, g2P, dlP, d2P, d1P, dz;
    DevBuf g2wP;      // g2 times the row weight (bf16, P-layout; pad feature H = the row weight): the pre-weighted operand of the output layer's weight gradient
};

void free_buf(DevBuf& b);
// A workspace struct (BlockWs, MlpWs, the nested *Ws / F32* structs of iwae_model) is DevBufs and nothing else, so iwae_destroy frees it as
// the array of DevBufs it is laid out as: a buffer added to a struct needs no second edit there
template <class Ws> void free_all(Ws& ws) {
    static_assert(std::is_standard_layout<Ws>::value && std::is_trivially_destructible<Ws>::value && sizeof(Ws) % sizeof(DevBuf) == 0, "a workspace struct holds DevBufs only");
    DevBuf* b = reinterpret_cast<DevBuf*>(&ws);
    for (size_t i = 0; i < sizeof(Ws) / sizeof(DevBuf); ++i) free_buf(b[i]);
}

// kernels iwae_enable_timing brackets with HIP events (on the stream each is launched on); names: iwae_kernel_time
enum TimedKernel { T_OUT_BWD = 0, T_DEC_FWD, T_WGRAD_OUT, T_DX_HID, T_DX_LAT, T_WGRAD_HID, T_WGRAD_LAT, T_LATENT_BWD, T_ENC_FWD, T_REDUCE, T_DEC_BWD, T_AR_ENC, T_AR_DEC, T_AIS_CHAIN, T_LOCAL_Q, T_IMPUTE, T_POSTERIOR, T_MASKED_OUT, T_MASKED_INPUT, T_COUNT };

// What a forward pass is told by its caller beyond the ABI's arguments.  Ordinary calls: FwdCall{m->batch_offset}; iwae_eval_llh walks
// images and samples in chunks and needs log_w only.
struct FwdCall {
    uint32_t batch_offset = 0;        // Philox row offset of the call's first image (iwae_set_step, plus the chunk's first image)
    int cond_row0 = 0;                // first row of iwae_model::cond the call's images use
    int k_total = 0, s_off = 0;       // k_total > 0: the call holds samples [s_off, s_off + k) of k_total per image and draws the unchunked call's Philox rows
    bool log_w_only = false;          // forward-only call: no second (DReG) density per sample (round 5: ~14 % of the sampling pass); the log-mean-exp alone when no tensor is wanted
    bool no_ksplit = false;           // float32: no K split of few-row products (an image's result must not depend on how many images share the launch)
    const uint8_t* mask = nullptr;    // the masked step of either precision (iwae_*_masked): the caller's [B, x_dim] mask, host or device, non-zero = observed; null: every pixel observed
    bool mask_resident = false;       // ... or the masks of the resident set's images (iwae_train_step_dataset behind iwae_dataset_set_mask / _mcar_mask; `mask` is null then):
                                      // stage_input writes every form of the batch the masked step reads in its one launch (MaskedStage)
    bool masked() const { return mask != nullptr || mask_resident; }
};
// Where stage_input leaves a resident masked batch (FwdCall::mask_resident): the caller has sized the buffers its plan reads and leaves the rest null
struct MaskedStage {
    uint16_t* xP = nullptr;           // bf16 rows of xin = m ? x : 0 (m->xP)
    uint16_t* xcP = nullptr;          // the hole-coded bf16 pixel rows (mk.xcP)
    float* xin = nullptr;             // float32 xin [B][X] (f32.xmask)
    uint8_t* mask = nullptr;          // the batch's mask bytes [B][X] (f32.mask)
    float* xcode = nullptr;           // float32 hole-coded rows [B][X] (f32.xcode: the fused route of the output layer)
};

// Every switch and tuning value iwae_set_option writes (defaults: the measured best).  plan_step reads the switches that choose kernels and streams; the
// launch code reads only the values that size a launch already chosen (wg_target*, wout_wg*, eps_blocks, dense_g1_mask, dec_bwd_nw).
struct StepOptions {
    bool allow_s_mode = true;   // option out_recompute switches back to recomputing the logits in out_bwd (A/B measurements)
    bool allow_zin = true;      // option no_zin: always the separate sampling kernel (A/B measurements)
    bool allow_zin_eval = false; // option zin_eval (round 4, measured and NOT the default): forward-only calls on many rows take their draws from eps_gen_kernel and let the decoder
                                 // kernel make z in its prologue instead of sample_kernel (inline Philox) in front of it -- bf16 evaluator 146 k vs 158 k images/s: the prologue's 20 MB of
                                 // float32 draws cost the vector-issue-bound kernel more than the separate pass
    bool allow_eps_multi = true;   // option no_eps_multi: one draw launch per step there too
    int eps_blocks = 512;      // blocks of the ahead-of-time noise draw (option eps_blocks; 0 = one block per 256 threads of work)
    bool allow_block_fused = true;   // option no_block_fused: a BasicBlock on few rows stays three dense_kernel launches (A/B measurements)
    bool allow_out_in_block = true;  // option no_out_in_block: the output layer of a few-row decoder stays a dense_kernel<EPI_BERN> launch (A/B measurements)
    bool allow_dec_fused = true;     // option no_dec_fused: the two tanh layers of the decoder stay dense_kernel launches (A/B measurements)
    bool allow_bern_pipe = true;   // option no_bern_pipe: the Bernoulli forward stays on dense_kernel<EPI_BERN> (A/B measurements)
    bool bern_qw = true;             // option no_bern_qw: the decoder kernel's 8-wave / 128-row shape instead of 16 waves / 200 rows (A/B measurements)
    bool bern_qw_force = false;      // option bern_qw_force: that shape at every row count it exists for (tests)
    bool allow_lse_fused = true;  // the decoder kernel does lse_kernel's work for its rows (option no_lse_fused)
    bool allow_lse_dup = true;      // option no_lse_dup: one lse_kernel, the side stream forks behind it (A/B measurements)
    bool allow_lse_in_bwd = true;      // few rows: this step's lse_kernel work is left to dec_bwd_rows_kernel (option no_lse_in_bwd)
    bool allow_early_wout = true;    // option no_early_wout: the output layer's weight gradient forks behind out_bwd with the others (A/B measurements)
    // Option g2w (round 4, measured and NOT the default): the decoder kernel leaves g2w = bf16(g_r g2) and the output layer's weight gradient runs
    // unweighted on it (no 870 cycles of row weighting per loader stage).  That kernel got faster (107 -> 97 us in the step) and the step SLOWER
    // (0.2044 -> 0.2154 ms, interleaved A/B): the decoder kernel pays 4 us for 23 MB more writes and the backward phase is bound by its bytes, not
    // by that kernel's instruction stream.
    bool allow_g2w = false;
    bool allow_chain2 = true;   // option no_chain2: the 2-layer model's per-sample blocks as dense_kernel launches + sample_kernel + gauss_lp_kernel (A/B measurements, variant tests)
    bool allow_chain2_bwd = true;      // option no_chain2_bwd: the per-sample blocks' backward as gauss_bwd_kernel + dense_kernel launches
    unsigned dense_g1_mask = IWAE_DENSE_G1_DEFAULT;   // option dense_g1 = <mask> (tuning aid, kernels.h)
    bool allow_dec_bwd = true;  // option no_dec_bwd: out_bwd_s + the two dX kernels stay three launches (A/B measurements)
    bool small_dec_bwd = true; int small_rows = 8191;   // the one-launch dX chain also below 8 192 rows (option no_small_dec_bwd: the per-pixel-group out_bwd + finish + two dX launches
                                                        // there).  Measured: B=20,k=1 0.1417 -> 0.1383 ms/step, B=100,k=5 150.7 -> 144.6 us, B=160,k=50 189.1 -> 165.7 us
    int dec_rows_max = 1024;    // dec_bwd_rows_kernel up to this many rows (option dec_rows), dec_bwd_kernel beyond
    int dec_bwd_nw = 8;         // option dec_bwd_nw: dec_bwd_kernel's shape (8 waves x 16 rows, round 4 | 4 waves x 32 rows)
    bool allow_dz_half = true;  // option dz_f32: dec_bwd_kernel leaves dz as float32 (A/B measurements)
    bool allow_wg3 = true;                           // few rows: the decoder's three weight gradients as one grouped launch (option no_wg3)
    bool allow_dec_rows = true;                      // ... and, with <= 2 048 DATA rows, the decoder's in the same launch (dec_rows_step; option no_dec_rows)
    bool allow_wgrad_rows = true;                    // few rows (<= 2 048): the image encoder's weight gradients + Adam in ONE launch, whole row reduction per workgroup (wgrad_rows_kernel; option no_wgrad_rows)
    bool allow_lat_rows4 = false;                    // option lat_rows4 (round 5, measured and NOT the default): beyond 16 samples per image the sums inside block_bwd_kernel<4> (4 images per
                                                     // workgroup, an image's samples over four waves, 256 workgroups).  In the step it takes 32.6 us where latent_bwd_kernel + block_bwd_kernel
                                                     // take 18.7 + 10.1: its 1024-thread / 101-register workgroups need a whole CU each and only ~96 CUs are free beside the weight
                                                     // gradients (three rounds), where latent_bwd_kernel's small workgroups fit anywhere: c1 0.1965 vs 0.1962 ms, c2 0.3856 vs 0.3802
    bool allow_lat_in_block = true;                  // few images: latent_bwd_kernel's sums inside the encoder's block_bwd_kernel (option no_lat_in_block)
    bool use_side2 = true;             // option no_side2: the hidden layers' weight gradients behind the output layer's on `side`, not beside it on `side2`
    bool allow_wg_group = false;       // option wg_group: the hidden layers' gradients as ONE grouped launch (measured: 0.2450 vs 0.2384 ms/step as two launches --
                                       // both at once take more of the machine from the output layer's gradient, which is what the step waits for)
    int wout_split = 0, wout_wg1 = 56, wout_wg2 = 128;      // option wout_split (percent of the rows, 0 = off; round 5): the output layer's weight gradient as an EARLY launch on few
                                // workgroups beside dec_bwd_kernel (rows [0, R1)) and a LATE one behind it (the rest, beside the hidden layers' gradients)
    bool defer_split = false;   // option defer_split (round 5): 1-layer step, each side stream sums + updates the decoder layers whose gradients IT carried
    bool allow_defer = true;    // option no_defer: always join at the end of the step (A/B measurements)
    bool allow_defer2 = true;   // option no_defer2
    bool allow_defer2_split = true;      // ... one deferred update per side stream (option no_defer2_split: one, on `tail`)
    int wg_target16 = 0;       // workgroups aimed at per 16-wave weight-gradient launch (option wg16; 0 = the model's default: 96 for the 1-layer model, 64 (round 5; 128 before) for
                               // the 2-layer one -- round 3, with the output layer's gradient starting right behind the decoder kernel: 80 / 88 / 96 / 104 / 112 / 128
                               // -> 0.2192 / 0.2168 / 0.2132 / 0.2164 / 0.2206 / 0.2175 ms, 24 row splits write 17 MB of slabs instead of 22.5; the 2-layer
                               // step: 0.3932 vs 0.3916): these are one-per-CU
                               // workgroups (128 KB of LDS); 256 of them lock every CU against the kernels running beside them on the main
                               // stream (256 -> 0.294, 192 -> 0.280, 160 -> 0.279 ms/step while the gradient forked behind out_bwd; forked
                               // behind lse_kernel, beside out_bwd: 96 -> 0.268, 112 -> 0.262, 128 -> 0.258, 144 -> 0.261, 160 -> 0.265)
    int wg_target16_1 = 64;    // same, for layers that are a single block wide (option wg16_1): the hidden layers' gradients -- with the specialised-wave kernel 64 row splits (12.8 MB of slabs each) beat 128 (0.259 -> 0.249-0.254 ms/step); 48 and 32 are slower again
    int wg_target8 = 128;      // same for the 8-wave launches on many rows (narrow layers of the 2-layer model; option wg8): 128 row splits halve the 109 MB of fp32 slabs 256 wrote per step (c2: 0.4193 -> 0.4176 ms; 64: 0.462)
    int wg_target8_few = 32;   // 8-wave launches on < 8 192 rows (the encoder's layers on the batch's images; option wg8_few): the 784-wide first layer in 4 row
                               // splits instead of 16 (10.6 -> 2.7 MB of slabs each way): 0.2439 -> 0.2351 ms/step at B = 1 024; 8 / 16 / 48: 0.2374 / 0.2374 / 0.2360
    int wg_shape9 = 0;          // option wg9 (bit mask, see wgradp_plan): layers that take the 8 + 8-wave / 128-feature shape of wgradws_kernel
    bool allow_wg7 = true;      // option no_wg7: the 16-wave weight-gradient shapes also where the 8-wave 7 x 4 shape exists (A/B measurements)
    bool dp_concurrent = false;        // option dp_concurrent: the two all-reduces of a step may run at the same time (see dp_finish)
    iwae::GemmF32Opts gemm_f32;                     // kernel choice of the float32 GEMM launchers (options f32_gemm_*, f32_no_ksplit, f32_ksplit_min_tiles)
    bool allow_f32_multi_reduce = true;      // option no_f32_multi_reduce: a slab reduction launch per gradient tensor instead of one per step
    bool allow_f32_side = true, f32_wout_first = true;      // float32 step: the decoder's weight gradients + update on the side stream (options no_f32_side, f32_wout_first)
    int f32_dw_last = 0;        // option f32_dw_last: all decoder weight gradients behind the dX chain (1: tiles as picked, 2: 4-wave tiles, 3: ... at 3 waves per SIMD)
    int f32_dw_min_rows = 32;   // float32 weight gradients: a row split covers at least this many rows (option f32_dw_min_rows; 64 until round 5)
    int f32_dw_tiles = 1024;    // float32 weight gradients: workgroups aimed at per launch (row splits = this / output tiles; option f32_dw_tiles)
    bool f32_dec_fused_train = false;
    bool allow_f32_dec_fused = true;                           // float32 mode: the decoder forward as one launch (dec_fwd_f32_kernel; option no_f32_dec_fused)
    bool allow_f32_bern_fused = true;      // float32 mode: log p(x|z) (and, in a training step, s) in the output layer's GEMM epilogue (option no_f32_bern_fused)
    int eval_rows = 0;                        // data rows per evaluator launch (option eval_rows): images x samples, k chunked beyond it; 0 = eval_rows_auto()
    int grid_chunk = 0;                       // iwae_grid_posterior: grid points per chunk (option grid_chunk; 0 = GRID_CHUNK_DEFAULT)
    int ais_t_chunk = 0;                      // iwae_ais: transitions per launch of ais_chain_kernel (option ais_t_chunk; 0 = AIS_T_CHUNK_DEFAULT)
    int local_t_chunk = 0;                    // iwae_local_posterior: passes per launch of local_q_kernel (option local_t_chunk; 0 = LOCAL_T_CHUNK_DEFAULT)
    bool allow_masked_out_fused = true;       // masked float32 step: the output layer + masked likelihood as masked_out_f32_kernel where its predicate holds (option no_masked_out_fused)
    int masked_out_min_rows = 25600;          // ... from this many data rows on (option masked_out_min_rows; 1: wherever the predicate holds).  Measured at 784 / 200 / 100, k = 50,
                                              // masked step / unmasked step, general | fast: 8 200 rows 1.006 | 1.178, 16 400 1.140 | 1.254, 25 600 1.156 | 1.128, 40 000 1.179 | 1.172,
                                              // 51 200 1.184 | 1.182, 102 400 1.247 | 1.144 (profiles/masked_step_time.txt): from 25 600 rows on the kernel never loses
    int impute_rows = 0;                      // iwae_impute: rows (images x draws, whole images) per launch of impute_rows_kernel (option impute_rows; 0 = IMPUTE_ROWS_DEFAULT)
};

// The kernels and streams of one bf16 step.  plan_step decides all of it from shapes and options before forward_impl launches or allocates
// anything; forward_impl, backward_impl and the entry points behind them read it and decide nothing themselves, so the forward pass never
// predicts what the backward pass will do -- both follow the same plan.  Every bf16 forward, a forward-only one too, writes m->plan anew: the
// backward half is valid only from a training forward to the entry points of that same step (backward_impl, dp_finish, the split step's halves).
enum ZFrom { Z_SAMPLE = 0, Z_DENSE_ZIN, Z_DEC_PROLOGUE, Z_BLOCK, Z_CHAIN2 };      // who makes z (z1): sample_kernel | dense_kernel's sampled-input mode | the decoder kernel's prologue | block_fwd_kernel | chain2_fwd_kernel
enum DecFwd { DEC_DENSE = 0, DEC_BLOCK2, DEC_BLOCK_OUT, DEC_PIPE };              // the decoder's tanh layers: dense_kernel launches | block_fwd_kernel | block_fwd_kernel with the output layer | inside the one-launch bern_pipe_kernel
enum LseAt { LSE_FWD = 0, LSE_DECODER, LSE_BWD_ROWS };                           // the log-mean-exp: lse_kernel in the forward pass | the decoder kernel | dec_bwd_rows_kernel
enum DxPath { DX_THREE = 0, DX_DEC_BWD, DX_ROWS };                               // the decoder's dX chain: out_bwd + two dense launches | dec_bwd_kernel | dec_bwd_rows_kernel
enum OnStream { ON_MAIN = 0, ON_SIDE, ON_SIDE2 };
struct StepPlan {
    // ---- forward
    bool zin_eval = false;      // forward-only call whose decoder kernel makes z from eps_gen_kernel's draws (option zin_eval)
    bool keep_eps = false;      // the draws come from eps_gen_kernel's buffers (later kernels of the call read them again)
    bool eps_multi = false;     // ... from the multi-step buffers (few data rows, single-stream backward)
    bool enc_takes_f32 = false; // the encoder's block_fwd_kernel converts float32 input rows itself (else prep_rows runs first)
    ZFrom z_from = Z_SAMPLE;
    bool chain = false;         // 2-layer model: both per-sample blocks in chain2_fwd_kernel
    bool chain2_bwd = false;    // ... and their backward as gblock_bwd_kernel
    DecFwd dec_fwd = DEC_DENSE;
    iwae::DenseArgs bern;             // shape half of the output layer's / decoder kernel's argument block (pipe: bern_pipe's shape 1 or 2); forward_impl adds the buffers
    iwae::BlockFwdArgs dec_blk;       // ... of block_fwd_kernel on the decoder (DEC_BLOCK2, DEC_BLOCK_OUT)
    int px_parts = 1;           // > 1: log p(x|z) of this forward arrives in px_part as that many partial sums per row
    bool s_mode = false;        // the forward keeps s = x - sigmoid(l) in wdec1.dlP
    bool holes = false;         // a masked call (FwdCall::mask): the output layer reads the hole-coded pixel rows xcP and selects unobserved pixels out (dense_kernel<EPI_BERN, .., HOLES>)
    bool early_wout = false;    // the output layer's weight gradient forks behind the decoder forward / lse_kernel, not behind out_bwd
    bool lse_fused = false;     // the decoder kernel does lse_kernel's work for its rows
    bool lse_dup = false;       // a second lse_kernel on the side stream makes the output layer's row weights
    bool g2w = false;           // the decoder kernel leaves g2w = bf16(g_r g2) (option g2w)
    LseAt lse_at = LSE_FWD;
    bool want_dreg = false;     // the call wants the second (DReG) log q per sample
    OnStream draw_on = ON_SIDE; // the stream of the speculative draw of the next step's noise
    // ---- backward (filled when the forward is a training step's)
    bool dec_rows = false;      // the decoder's weight gradients ride in the encoder's wgrad_rows_kernel launch: no side-stream work at all
    DxPath dx = DX_THREE;
    iwae::DecBwdRowsArgs rows;        // shape half of dec_bwd_rows_kernel's argument block (DX_ROWS)
    bool out_parts = false;     // DX_THREE: out_bwd_s_kernel per pixel group, partial sums + finish kernel
    bool dz_half = false;       // the dX kernel leaves dz as bf16
    bool lat_fuse = false;      // latent_bwd_kernel's sums inside the encoder's block_bwd_kernel
    bool rows_enc = false;      // the encoder's weight gradients + update as wgrad_rows_kernel
    bool group3 = false;        // the decoder's three weight gradients as one grouped launch on `side2`
    bool wout_two_part = false; // the output layer's weight gradient as an early and a late launch (option wout_split)
    bool hid_group = false;     // the hidden layers' weight gradients as one grouped launch (option wg_group)
    OnStream hid_on = ON_SIDE;  // the stream of the hidden layers' weight gradients (the output layer's: `side`, or `side2` in group3)
    OnStream tail = ON_SIDE;    // the side stream that finishes last (carries the decoder's reduction / exchange / update)
};

// The kernels and streams of one float32 step, as StepPlan is the bf16 step's.  plan_step_f32 decides all of it from shapes, options and the
// staged input (the one-launch decoder reads x in 16-byte segments, and a caller's device pointer is read in place: dec_fwd_f32_ok); forward_f32,
// backward_f32 and f32_dw read it and decide nothing themselves.  Every float32 forward writes m->f32_plan anew (fwd_was_f32 says which of the
// two plans is the valid one); the backward half is valid only from a training forward to the backward_f32 of that same step.
enum F32DecFwd { F32_DEC_GEMMS = 0, F32_DEC_ONE_LAUNCH };                    // the decoder forward: three GEMM launches | dec_fwd_f32_kernel
enum F32PxFrom { F32_PX_BERN_PASS = 0, F32_PX_GEMM_EPILOGUE, F32_PX_DEC_KERNEL, F32_PX_MASKED_PASS, F32_PX_MASKED_OUT };      // log p(x|z): bern_f32_kernel over the stored logits | the output layer's GEMM epilogue (px_parts partial sums per row) | dec_fwd_f32_kernel (whole)
// (a masked call, F32Plan::mask: masked_bern_f32_kernel over the stored logits [+ masked_s_f32_kernel] | masked_out_f32_kernel in place of the output layer's GEMM)
// the host enqueue order of the decoder's three weight gradients among its dX products (backward_f32)
enum F32DwOrder {
    F32_DW_ONE_STREAM = 0,      // each in front of its layer's dX product, on the main stream
    F32_DW_WOUT_FIRST,          // side stream: the output layer's first, the hidden layers' each behind the dX product that makes its operand
    F32_DW_WOUT_LAST,           // ... the output layer's behind the hidden layers' (option f32_wout_last)
    F32_DW_BEHIND_DX            // ... all three behind the whole dX chain, first layer first (option f32_dw_last)
};
struct F32Plan {
    const float* x = nullptr;   // device x [B][X] of the call (stage_input): the backward pass reads it again.  A masked call: xin = m ? x : 0
    const uint8_t* mask = nullptr;      // device mask [B][X] of a masked call (iwae_*_masked), else null
    // ---- forward
    F32DecFwd dec_fwd = F32_DEC_GEMMS;
    F32PxFrom px_from = F32_PX_BERN_PASS;
    int px_parts = 1;           // > 1: log p(x|z) arrives in px_part as that many partial sums per row
    bool keeps_s = false;       // the forward left s = x - sigmoid(l) where the logits would have gone (the backward pass takes the row weight in its two consumers)
    bool want_dreg = false;     // the call wants the second (DReG) log q per sample
    bool lme_only = false;      // forward-only call that hands out no tensor: lse_kernel makes the log-mean-exp alone
    // ---- backward (filled when the forward is a training step's)
    F32DwOrder dw_order = F32_DW_ONE_STREAM;
    int dw_tile_mode = 0;       // tile mode of the decoder's weight gradients (F32_DW_BEHIND_DX; 0: tiles as picked, 1: 4-wave tiles, 2: ... at 3 waves per SIMD)
    bool side() const { return dw_order != F32_DW_ONE_STREAM; }      // the decoder's weight gradients + sums [+ update] run on the side stream
};

// How a training step ends: what becomes of the weight-gradient slabs once every layer's are written.
enum StepEnd {
    END_GRAD = 0,           // the flat gradient, every stream joined (iwae_forward_backward, iwae_grad_moments, the train step that hands out tensors)
    END_GRAD_SPLIT,         // ... the decoder's segment left on the side stream, unjoined (iwae_forward_backward_split)
    END_GRAD_SPLIT_HELD,    // ... and its slab reduction not launched either: dp_finish does, behind the wait that orders the step's two all-reduces
    END_UPDATE              // Adam in the epilogue of the slab sums (the single-GPU iwae_train_step)
};
struct BlockRange { int first = 0, count = 0; };
// Where each block of layers begins in the layer table (order enc1 | enc2 | dec2 | dec1 | prior): .r in the slab-reduce grid, .e in the
// elementwise grid.  build_descs computes them; nothing else looks a boundary up.
struct TableBounds {
    struct At { int r = 0, e = 0; };
    At enc1_end, enc2, dec2;      // (1-layer model: all three are where the image encoder ends)
    At dec1, dec1_out, dec1_end;  // the decoder's first layer, its output layer, the first entry behind it
    At end;                       // the whole table: the grids' sizes
};
// What a step left behind on the side streams: planned by plan_step_end, written once at the end of backward_impl / backward_f32, consumed by
// join_side and dp_finish, reported by iwae_forward_backward_split.
// Single-GPU train step: the decoder's slab reduction + Adam (90 % of the slab bytes) stays on the side stream and is
// NOT joined at the end of the step -- nothing needs the decoder's new weights before the next step's d1 layer, so it
// runs beside the next encoder forward.  join_side() waits for it, and every entry point that touches parameters, gradients or the decoder calls that.
struct StepLeft {
    bool dec = false;           // ev_dec (recorded behind the tail stream's reduction / update) has not been waited for yet
    bool dec2 = false;          // ... ev_dec2 (the other side stream's own deferred update)
    BlockRange held;            // count > 0: the decoder's slab reduction over these blocks is not launched yet: dp_finish does
    size_t split_offset = 0;    // first float of the flat gradient that was left on the side stream (nparam: none)
    OnStream on = ON_SIDE;      // the stream that carries it
    bool z_pending = false;     // float32 step: ev_join (recorded on the side stream behind the gradient of the decoder's first layer, which reads z) has not been
                                // waited for yet: the next forward of either precision waits in front of its sampling
};
// The end of one bf16 step, decided by plan_step_end from the plan, the options, the layer table and the caller's StepEnd; backward_impl
// executes it.  A side stream sums (and, `update`, updates) the layers whose weight gradients it carried, in ONE launch of up to two ranges.
// EARLY: gradient only, the decoder's sums on the tail stream, joined behind the main stream's | _SPLIT: not joined | _HELD: not even launched
enum EndCase { ENDS_JOINED = 0, ENDS_DEC_ROWS, ENDS_EARLY, ENDS_EARLY_SPLIT, ENDS_EARLY_HELD, ENDS_DEFER, ENDS_SPLIT_UPD, ENDS_DEFER2, ENDS_DEFER2_SPLIT };
enum SideWait { WAIT_NONE = 0, WAIT_FORK2, WAIT_SIDE };      // what a side stream waits for in front of its sums: nothing more | the dX chain's event | `side` (ev_join2, recorded there)
struct SideSum { OnStream on = ON_SIDE; BlockRange a, b; SideWait behind = WAIT_NONE; bool second_event = false; };      // (second_event: completes ev_dec2, not ev_dec)
struct StepEndPlan {
    EndCase how = ENDS_JOINED;
    bool update = false;        // Adam in every reduction's epilogue
    bool join_both = false;     // ENDS_JOINED: the main stream waits for `side` as well as for the tail stream
    BlockRange main_a, main_b;  // the main stream's share of the table
    int nside = 0;
    SideSum side[2];            // in host enqueue order
    StepLeft left;              // what the step will have left behind when all of this is enqueued
};

struct iwae_model {
    iwae_config cfg;
    int X, Xp32;
    int C = 0, Xinp = 0;       // conditional model: condition width; row width of the encoder input concat(x, y) (= Xp32 without)
    DevBuf cond; int cond_n = 0;   // y [cond_n][C] fp32 for the next call (iwae_set_condition)
    int H[2], D[2], Hp[2], Dp[2];
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::vector<KerasLayer> klayers;
    size_t nparam = 0;
    // Linear maps.  1-layer: enc{l1,l2,head}, dec{d1,d2,out}.  2-layer adds enc2, dec2 blocks.
    Linear enc1[3], enc2[3], dec2[3], dec1[3];
    Linear prior[3];           // conditional prior network p(z|y) (cfg.cond_prior, tasks/task04.py:108): BasicBlock on y
    bool has_prior = false;
    DevBuf condP;              // y as bf16 P-layout [Bp][32*ceil(C/32)] (the prior block's input)
    float *param = nullptr, *grad = nullptr, *mom = nullptr, *vel = nullptr;
    int64_t adam_t = 0;
    // float32 mode (iwae_config.precision / iwae_set_eval_precision): row-major float32 activations, GEMMs on v_mfma_f32_16x16x4_f32
    struct F32Block { DevBuf h1, h2, dhead, d2, d1, dx; };
    struct F32State { F32Block enc1, enc2, dec2, prior; DevBuf z[2], g1, g2, logits, d2, d1, slab, bpart, xcat, kslab, xmask, mask, xcode; } f32;
    // float32 weight gradients of a step keep their row-split slabs (each in its own region of f32.slab) and are summed by ONE launch at the end of
    // backward_f32 (reduce_slabs_multi_f32_kernel): jobs queued by f32_dw, slab offsets in floats (the buffer may still grow while they queue)
    struct F32Pending { size_t off; size_t stride; size_t n; float* out; int nsplit; int seg; };
    std::vector<F32Pending> f32_pending; size_t f32_slab_used = 0;
    bool bf16_side_used = false;      // a bf16 call may have left a speculative draw on a side stream (forward_f32 waits for it on the host)
    size_t f32_slab_want = 0, f32_slab_want_step = 0;      // floats of slabs the last whole step asked for (the buffer's target size) / this step so far
    // An evaluation call's images when they arrive on the host, their bf16 rows and float32 encoder heads (analysis.hip): nothing is read after the call that filled it, so all calls share
    struct EvalWs { DevBuf x, xP, head; } ev;
    DevBuf eval_lme;                          // iwae_eval_llh: the per-image log-mean-exps of every launch
    int eval_precision = IWAE_PREC_FP32;      // arithmetic of iwae_eval_llh and the analyses (iwae_set_eval_precision)
    // iwae_grid_posterior's buffers
    struct GridWs { DevBuf xb, flag, z, lw, zP, h1, h2, logits, lhi, llo, c, zc, w, part, run, lpx, mean, cov, qmass, kl, lj; } grid;
    // iwae_latent_activity's buffers: the chunk's draws, z1 rows and q(z2|z1) activations of the composed paths, the block partials
    // of mu2 [N][blocks][D2] and the outputs
    struct ActWs { DevBuf eps, z, rows, part, pm, act, dm; BlockWs blk; F32Block f32; } act;
    // iwae_grad_moments' buffers: the Welford mean and M2 [nparam] in double
    struct MomWs { DevBuf mean, m2; } mom_ws;
    // iwae_aggregate_posterior's buffers: the draws, the component tables, a sample tile's z / own terms and range partials,
    // the per-sample densities (log_qzd transposed [Dpad][S N]) and the double sums
    struct AggWs { DevBuf eps, mu, inv, invd, nls, nls_sum, zT, shT, dim_part, jmax, jsum, lqz, lqzdT, lqzd, part, out; } agg;
    // iwae_ais's buffers: the decoder's padded weights, the schedule, the chain state (e, log_w, h, accept counts), the
    // caller's noise and initial states when they arrive on the host, and the outputs; iwae_ais_masked's mask copy, masked input and coded rows
    struct AisWs { DevBuf wpad, betas, e, logw, h, nacc, z0, mom, unif, dH, acc, rate, z, lpx, ess, mask, xin, xc; } ais;
    // iwae_local_posterior's buffers (the padded weights are ais.wpad): the per-image state and double sums, Adam's step sizes, the
    // caller's start and noise when they arrive on the host, and the outputs; iwae_local_posterior_masked's mask copy, masked input and coded rows
    struct LocalWs { DevBuf st, acc, alpha, mu0, sg0, eps, qmu, qsg, mu, sg, elbo, iwae, bound, grad, logw, mask, xin, xc; } loc;
    // iwae_impute's buffers (the padded weights are ais.wpad): the masked input, the caller's mask and noise when they arrive on the host,
    // the log-weights, per image (max, 1 / sum), the chunk sums of xhat (more than 64 draws per image) and the outputs
    struct ImputeWs { DevBuf xin, mask, eps, logw, wstat, part, lpx, ess, xhat; } imp;
    // iwae_posterior's buffers beyond those (it shares imp with iwae_impute): the chunk moments and the running sums of a launch, the
    // caller's uniforms when they arrive on the host, and the outputs
    struct PosteriorWs { DevBuf part, cdf, unif, mean, cov, idx, z, u; } post;
    bool fwd_was_f32 = false;                 // the last forward ran in float32 mode (its backward must too)
    // data-parallel training inside the library (iwae_comm_init): one communicator per stream that carries a collective
    ncclComm_t comm_main = nullptr, comm_side = nullptr;
    int comm_world = 1, comm_rank = 0;
    float adam_b1 = 0.9f, adam_b2 = 0.999f, adam_eps = 1e-4f;   // keras Adam(lr, epsilon=1e-4) of main.py:93 unless iwae_set_adam says otherwise
    uint32_t noise_step = 0, batch_offset = 0;
    // layer descriptor table
    std::vector<iwae::LayerDesc> descs;
    iwae::LayerDesc* d_descs = nullptr;
    TableBounds tb;
    bool descs_dirty = true;
    StepOptions opt;
    StepPlan plan;             // the kernels and streams of the step in flight: written by plan_step (forward_impl), read by the backward pass and the entry points behind it
    StepEndPlan end;           // ... and how it ends: written by plan_step_end (backward_impl)
    F32Plan f32_plan;          // the float32 step in flight: written by plan_step_f32 (forward_f32), read by backward_f32 and f32_dw
    StepLeft left;
    // per-call state: written by begin_forward only (the backward pass and eps_src read the forward's copy)
    FwdCall call;
    int B = 0, k = 0, M = 0, Mp = 0, Bp = 0;
    float beta = 1.0f;
    bool have_forward = false, user_eps = false;
    DevBuf dg2_part;            // small row counts: out_bwd_s_kernel's per-pixel-group partial sums
    DevBuf px_part;
    DevBuf xin, xP, epsbuf, zP[2];
    // the masked bf16 step: the hole-coded pixel rows beside xP (which then holds xin = m ? x : 0), xin as float32, the caller's mask when it arrives on the host
    struct MaskedWs { DevBuf xcP, xin, mask; } mk;
    DevBuf rows[6];            // lpxz, t1, t2, t3, t4, lq_dreg   (per data row)
    DevBuf logw, wn, gx, cf, per_b, dzdir;
    // lse_kernel's outputs once more, written by the copy of it that runs on the side stream (see forward_impl): the output layer's
    // weight gradient takes its row weights from there
    DevBuf logw2, wn2, gx2, cf2, per_b2;
    bool g2w_descs = false;     // the layer table was built for a step with plan.g2w
    BlockWs wenc1, wenc2, wdec2, wprior;
    MlpWs wdec1;
    DevBuf scratch;            // exports
    // resident dataset (iwae_dataset_*): uint8 grey levels [N][X] + the epoch's visiting order
    DevBuf ds_data, ds_order;
    DevBuf ds_labels; bool ds_has_labels = false;   // class id per image of the resident set (iwae_dataset_set_labels; conditional models)
    DevBuf ds_mask; bool ds_has_mask = false;       // one fixed mask per image of the resident set, bit-packed [ds_N][mask_words(X)] (iwae_dataset_set_mask / _mcar_mask): iwae_train_step_dataset takes the masked step
    int ds_N = 0;
    // N(0,1) draws of a step, fp32 [Mp][Dp] per latent layer, made by eps_gen_kernel and read by the sampling / decoder and
    // backward kernels.  A training step draws the NEXT step's noise during its forward pass on the side stream, idle then
    // (speculating step+1, same batch shape); it is ordered by the join the main stream performs anyway, and a forward
    // whose counters do not match the speculation draws on its own stream first.  Three ring slots: this step's draws, the
    // previous step's (its backward pass may still read them) and the next step's.
    DevBuf epsc[3][2];          // [ring slot][layer]: the step's draws, the previous step's (its backward may still read them
                                // when the next step's are requested) and the next step's (drawn during this step's forward)
    struct EpsTag { bool valid = false; uint32_t step = 0; uint64_t row_offset = 0; int M = 0; } eps_tag[3];
    int epsc_par = 0;
    // Few data rows (the single-stream regime of dec_rows_step, round 5): the draws of EPSM_STEPS consecutive steps in ONE launch, two buffers taking turns
    // (the next group is drawn during the forward pass of the current group's last step: the buffer it overwrites was last read a whole group ago, in stream order)
    DevBuf epsm[2][2];          // [buffer][layer]: [EPSM_STEPS][Mp][eps_ld]
    struct EpsMTag { bool valid = false; uint32_t step0 = 0; uint64_t row_offset = 0; int M = 0; } epsm_tag[2];
    const float* epsc_ptr[2] = {nullptr, nullptr};
    char* d_zero = nullptr;    // 1 KiB of zeros (wgradp_kernel's source for rows >= M)
    uint32_t ds_epoch = 0;
    int ds_start = -1;         // >= 0: the next forward gathers + binarises rows ds_start.. from the dataset instead of reading x
    DevBuf stamps;             // diagnostic (option stamps, DIAG builds)
    DevBuf dstamps; int dstamp_epi = -1, dstamp_kt = -1, dstamp_waves = 0;   // diagnostic (options dense_stamps_epi / dense_stamps_kt, STAMPS builds)
    // optional HIP-event timing of the dominant kernels (iwae_enable_timing): pairs recorded on m->stream
    // fork/join of the decoder weight-gradient GEMMs (independent of the dz -> encoder chain) onto a side stream
    hipStream_t side = nullptr;
    hipStream_t side2 = nullptr;       // the hidden layers' weight gradients beside the output layer's (option no_side2: behind it on `side`)
    hipEvent_t ev_s2 = nullptr;
    hipEvent_t ev_ar = nullptr;        // data-parallel step: recorded behind the encoder segment's all-reduce (dp_finish)
    hipEvent_t ev_lse = nullptr;
    hipEvent_t ev_fork = nullptr, ev_fork2 = nullptr, ev_blk = nullptr, ev_join = nullptr, ev_join2 = nullptr, ev_dec = nullptr;
    int fake_s = 0;             // DIAG builds: byte ablations of s (option fake_s)
    int abl_skip = 0;           // DIAG builds: launch ablations of the full-size step (option abl_skip; timing only, results wrong): 1 no output-layer weight gradient,
                                // 2 no hidden-layer weight gradients, 4 no deferred decoder reduction + update, 8 no latent_bwd_kernel, 16 no noise draw ahead
    int wg_debug = 0;           // option wg_debug (DIAG builds): diagnostic ablations of wgradp_kernel (kernels.h)
    int num_cus = 256;               // compute units of the device (hipDeviceProp_t::multiProcessorCount)
    hipEvent_t ev_dec2 = nullptr;
    int timing = 0;            // 0 off, n > 0: time every n-th forward (event records cost a few us of stream bubble each)
    int64_t timing_calls = 0;
    bool time_this = false;
    std::vector<hipEvent_t> ev_start[T_COUNT], ev_stop[T_COUNT];   // per timed kernel (enum TimedKernel)
    size_t ev_used[T_COUNT] = {};
    bool want_stamps = false;
    float* d_scalars = nullptr;
    float* h_scalars = nullptr;   // pinned
};

template <class T>
T* ptr(const DevBuf& b) { return (T*)b.p; }

struct ScopedTimer {     // records a start/stop event pair around a launch when timing is enabled
    iwae_model* m; int id; bool on; hipStream_t ts;
    ScopedTimer(iwae_model* m_, int id_, hipStream_t s_ = nullptr) : m(m_), id(id_), on(m_->time_this), ts(s_ ? s_ : m_->stream) {
        if (!on) return;
        if (m->ev_used[id] == m->ev_start[id].size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
            m->ev_start[id].push_back(a); m->ev_stop[id].push_back(b);
        }
        (void)hipEventRecord(m->ev_start[id][m->ev_used[id]], ts);
    }
    ~ScopedTimer() {
        if (!on) return;
        (void)hipEventRecord(m->ev_stop[id][m->ev_used[id]], ts);
        m->ev_used[id] += 1;
    }
};

// ---- defined in model.hip
int ensure(DevBuf& b, size_t bytes, hipStream_t st);      // at least `bytes`; regrowing synchronises st and frees the old allocation
bool is_device_ptr(const void* p, int device);
int copy_in(iwae_model* m, DevBuf& dst, const void* src, size_t bytes);
int copy_out(iwae_model* m, void* dst, const void* src, size_t bytes);
int join_side(iwae_model* m);
int dense_fwd(iwae_model* m, Linear& L, int epi, const uint16_t* XP, int rows, uint16_t* YP, float* YF, int ldYF, const iwae::SampleArgs* zin = nullptr);
int block_alloc(iwae_model* m, Linear* blk, BlockWs& w, int R, int Rp, bool bwd, bool need_dx);
int block_fwd(iwae_model* m, Linear* blk, BlockWs& w, const uint16_t* XP, int R, const float* xf = nullptr, int xdim = 0);
// (the float32 step's share)
int begin_forward(iwae_model* m, const float* x, int B, int k, float beta, const FwdCall& call, const float** cond);
int stage_input(iwae_model* m, const float* x, int B, bool keep_f32, const float** xd, const MaskedStage* masked = nullptr);
int draw_eps(iwae_model* m, int par, uint32_t step, int M, hipStream_t gs, int max_blocks = 0);
iwae::EpsSrc eps_src(iwae_model* m, int layer);
int build_descs(iwae_model* m);
float adam_alpha(iwae_model* m, float lr);
void adam_blocks(iwae_model* m, hipStream_t st, int first, int count, float alpha, float grad_scale, hipEvent_t done = nullptr, bool update = true);
int adam_impl(iwae_model* m, float lr, float gscale);
// (the bf16 step's share)
void reduce_blocks(iwae_model* m, hipStream_t st, BlockRange a, BlockRange b, float alpha, bool update, hipEvent_t done, bool with_means);
int attach_dense_stamps(iwae_model* m, int epi, iwae::DenseArgs& a);
bool block_fwd_shape(const iwae_model* m, const Linear* blk, int R, iwae::BlockFwdArgs& a);
// row stride of the cached draws: the latent width rounded to 4, NOT the 32-padded operand width -- D = 100: 400 B instead of 512 B per row,
// 5.7 MB less per pass over the k = 50, B = 1 024 step's draws (written once, read by the decoder kernel and by latent_bwd_kernel)
inline int eps_ld(const iwae_model* m, int layer) { return 4 * ((m->D[layer] + 3) / 4); }
inline hipStream_t on_stream(const iwae_model* m, OnStream s) { return s == ON_SIDE2 ? m->side2 : s == ON_SIDE ? m->side : m->stream; }
// (the step driver: the forward / backward pass of the given / the handle's precision -- nothing else chooses between forward_f32 / forward_impl
// and backward_f32 / backward_impl)
int step_forward(iwae_model* m, int precision, const float* x, int B, int k, float beta, const float* eps, int objective, bool bwd, const iwae_tensors* want,
                 const FwdCall& call);
int step_backward(iwae_model* m, int objective, StepEnd end, float lr = 0.0f);

// ---- defined in step_f32.hip
int f32_fwd(iwae_model* m, const KerasLayer& kl, const float* X, long ldx, int rows, float* Y, long ldy, int epi, bool no_ksplit);
int f32_block_fwd(iwae_model* m, int base, iwae_model::F32Block& w, const float* X, long ldx, int R, float* head, int Dp, bool no_ksplit);
int forward_f32(iwae_model* m, const float* x, int B, int k, float beta, const float* eps, int objective, bool bwd, const iwae_tensors* want, const FwdCall& call);
int backward_f32(iwae_model* m, int objective, StepEnd end, float lr = 0.0f);

// ---- defined in step_bf16.hip
int forward_impl(iwae_model* m, const float* x, int B, int k, float beta, const float* eps, int objective, bool bwd, const iwae_tensors* want, const FwdCall& call);
int backward_impl(iwae_model* m, int objective, StepEnd end, float lr = 0.0f);

// ---- a caller's array may live on the host or on the handle's device.  Input: a device pointer is read in place, host memory is uploaded into ws
template <class T> int staged_in(iwae_model* m, const T* user, DevBuf& ws, size_t bytes, const T** dev) {
    const bool in_place = is_device_ptr(user, m->cfg.device);
    if (!in_place) CHK(copy_in(m, ws, user, bytes));
    *dev = in_place ? user : ptr<T>(ws);
    return IWAE_OK;
}
// output: a device pointer is written in place; else (host memory, or null: only later kernels want it) into ws, finish_out copies it out
template <class T> int staged_out(iwae_model* m, T* user, DevBuf& ws, size_t bytes, T** dev) {
    const bool in_place = user && is_device_ptr(user, m->cfg.device);
    if (!in_place) CHK(ensure(ws, bytes, m->stream));
    *dev = in_place ? user : ptr<T>(ws);
    return IWAE_OK;
}
inline int finish_out(iwae_model* m, void* user, const void* staged, size_t bytes) { return user && staged != user ? copy_out(m, user, staged, bytes) : IWAE_OK; }

#pragma GCC visibility pop
