/* iwae_amd -- C ABI of the MI355X-native IWAE train / eval step.
 *
 * Drop-in boundary for the hot path of nbip/IWAE (a pure-Python TF2 repo with no FFI of its
 * own): each entry point replaces the Python-level call named next to it (file:line under
 * /root/reference).  Plain C types only; every function returns IWAE_OK (0) or a negative
 * iwae_status, the message is available from iwae_last_error().  No C++ exceptions cross
 * this boundary.  A handle is bound to one GPU and one HIP stream; calls on one handle are
 * stream-ordered and not thread-safe, different handles are independent.
 *
 * Pointers named `x`, `eps`, `flat`, `out` may be host OR device pointers (the copy uses
 * hipMemcpyDefault); host results are valid when the call returns.
 * Tensor order at this boundary is the reference's: sample axis first, [k, B, ...]
 * (src/iwae1.py:59,107-125), C-contiguous float32.
 */
#ifndef IWAE_AMD_H
#define IWAE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct iwae_model* iwae_handle;

typedef enum {
    IWAE_OK = 0,
    IWAE_ERR_ARG = -1,      /* bad argument (the Python shim maps it to ValueError / KeyError) */
    IWAE_ERR_HIP = -2,      /* HIP runtime error */
    IWAE_ERR_NOMEM = -3,    /* device allocation failed */
    IWAE_ERR_STATE = -4     /* call order (e.g. backward without forward) */
} iwae_status;

/* --objective choices of main.py:23, plus the DReG estimator of tasks/task02.py:87-101 */
typedef enum {
    IWAE_OBJ_VAE_ELBO = 0,     /* src/iwae1.py:120 */
    IWAE_OBJ_IWAE_ELBO = 1,    /* src/iwae1.py:125 */
    IWAE_OBJ_IWAE_EQ14 = 2,    /* src/iwae1.py:128-134 */
    IWAE_OBJ_VAE_ELBO_KL = 3,  /* src/iwae1.py:121 (1-layer only; a KeyError for the 2-layer model, src/iwae2.py:154-167) */
    IWAE_OBJ_DREG = 4          /* tasks/task02.py:61-101 (1-layer only) */
} iwae_objective;

/* arithmetic of the GEMMs.  The reference computes everything in float32 (Keras Dense defaults, src/iwae1.py:31-34,72-75);
 * BASELINE.json configs[1] asks for bf16 operands. */
typedef enum {
    IWAE_PREC_BF16 = 0,        /* bf16 GEMM operands, fp32 accumulation (v_mfma_f32_16x16x32_bf16): the fast training path */
    IWAE_PREC_FP32 = 1         /* exact float32 GEMMs (v_mfma_f32_16x16x4_f32): every product as the reference's float32 graph */
} iwae_precision;

/* iwae1.IWAE(n_hidden, n_latent) src/iwae1.py:89-96 / iwae2.IWAE(n_hidden[2], n_latent[2]) src/iwae2.py:100-107.
 * struct_size MUST be set to sizeof(iwae_config) by the caller: iwae_create rejects any other value, so a binding
 * compiled against an older or newer layout fails loudly instead of reading past its struct. */
typedef struct {
    uint32_t struct_size;      /* = sizeof(iwae_config) (64); ABI guard */
    int32_t n_layers;          /* 1 or 2 stochastic layers (main.py:17) */
    int32_t n_hidden[2];       /* main.py:86,90 : {200} / {200,100}; each <= 256 */
    int32_t n_latent[2];       /* main.py:85,89 : {100} / {100,50};  each <= 128 */
    int32_t x_dim;             /* 784 */
    int32_t device;            /* HIP device ordinal */
    uint64_t seed;             /* Philox key for the reparameterisation noise (main.py:40-41 seeds TF) */
    int32_t world_size;        /* data-parallel ranks (1 = single GPU); iwae_comm_init must be given the same values */
    int32_t rank;              /* this process's rank (checked against iwae_comm_init).  The library does NOT derive noise keys from it:
                                  the caller passes the global index of the shard's first image, rank*B, through iwae_set_step */
    int32_t cond_dim;          /* 0, or C > 0: the conditional model of tasks/task05.py:101-168 (1-layer only): the encoder
                                  sees concat(x, y), the decoder concat(z, y), y [B, C] set with iwae_set_condition
                                  (one-hot labels there, C = 10); needs n_latent + C <= round_up(n_latent, 32) */
    int32_t cond_prior;        /* with cond_dim > 0: 1 = the learned conditional prior p(z|y) of tasks/task04.py:101-173 (a BasicBlock on y,
                                  created after the decoder) replaces N(0,1) in lpz; sample(z, y) maps z through it (:190-196) */
    int32_t precision;         /* iwae_precision of forward / train calls (iwae_eval_llh: iwae_set_eval_precision) */
    int32_t reserved;          /* 0 */
} iwae_config;

/* scalar entries of the result dict (src/iwae1.py:141-144, tasks/task02.py:78-79) and the
 * means that IWAE.write_to_tensorboard logs (src/iwae1.py:228-232) */
typedef struct {
    float vae_elbo;
    float vae_elbo_kl;
    float iwae_elbo;
    float iwae_eq14;
    float inference_loss;      /* DReG only */
    float mean_lpxz;           /* mean over [k,B] of lpxz (lpxz1) */
    float mean_lpz;            /* 1-layer: lpz ; 2-layer: lpz1z2 */
    float mean_lqzx;           /* 1-layer: lqzx ; 2-layer: lpz2 */
    float mean_kl;
    float reserved[7];
} iwae_scalars;

/* optional tensor outputs (NULL = not wanted, then never materialised).  1-layer names;
 * for the 2-layer model z=z1, z2=z2, lpz=lpz1z2, lpz2=lpz2, lqzx=lqz1x, lqzx2=lqz2z1 */
typedef struct {
    float* z;        /* [k,B,D1]  src/iwae1.py:145 */
    float* z2;       /* [k,B,D2]  src/iwae2.py:158 */
    float* snis_z;   /* [B,D1]    src/iwae1.py:146 */
    float* snis_z2;  /* [B,D2]    src/iwae2.py:160 */
    float* al;       /* [k,B]     src/iwae1.py:147 */
    float* logits;   /* [k,B,X]   src/iwae1.py:148 */
    float* lpxz;     /* [k,B]     src/iwae1.py:149 */
    float* lpz;      /* [k,B]     src/iwae1.py:150 */
    float* lqzx;     /* [k,B]     src/iwae1.py:151 */
    float* lpz2;     /* [k,B]     src/iwae2.py:165 */
    float* lqzx2;    /* [k,B]     src/iwae2.py:167 */
    float* log_w;    /* [k,B]     src/iwae1.py:113 */
} iwae_tensors;

const char* iwae_last_error(void);
int iwae_version(void);
/* 16 hex digits of the sha256 over the sources this binary was built from (iwae_amd/csrc/build.sh; "-diag" appended for diagnostic
 * builds): ties a shipped .so to a source tree -- the test suite rebuilds on mismatch, bench.py stamps its line with it and drops
 * profile artefacts (profiles/ *_kernel_traffic.json) taken on another build.  No reference counterpart. */
const char* iwae_build_id(void);

/* model construction: iwae1.IWAE(...) / iwae2.IWAE(...) ; weights glorot-uniform / zero-bias
 * (Keras Dense defaults, src/iwae1.py:31-34,72-75) drawn from `seed`; set the data-mean output
 * bias (src/utils.py:11-23) with iwae_set_params or iwae_set_output_bias. */
int iwae_create(const iwae_config* cfg, iwae_handle* out);
void iwae_destroy(iwae_handle h);
int iwae_set_stream(iwae_handle h, void* hip_stream);        /* run on the caller's stream (e.g. torch's) */
int iwae_sync(iwae_handle h);

/* model.trainable_weights (Keras creation order, kernel [in,out] then bias [out] per Dense) */
int iwae_param_count(iwae_handle h, size_t* n);
int iwae_num_tensors(iwae_handle h, int32_t* n);
int iwae_tensor_info(iwae_handle h, int32_t idx, char* name, size_t name_cap, int32_t* rows, int32_t* cols, size_t* offset);
int iwae_set_params(iwae_handle h, const float* flat, size_t n);   /* model.load_weights / set_weights */
int iwae_get_params(iwae_handle h, float* flat, size_t n);         /* model.save_weights (main.py:165) */
int iwae_set_output_bias(iwae_handle h, const float* bias, size_t n);  /* utils.get_bias(), src/utils.py:11-23 */
int iwae_get_grads(iwae_handle h, float* flat, size_t n);          /* tape.gradient result, src/iwae1.py:159 */
int iwae_get_adam_state(iwae_handle h, float* m, float* v, size_t n, int64_t* step);
int iwae_set_adam_state(iwae_handle h, const float* m, const float* v, size_t n, int64_t step);

/* model(x, n_samples, beta) / val_step : src/iwae1.py:98-151,164-166 (main.py:152,176).
 * x [B, x_dim] in {0,1}; eps NULL (device Philox) or the N(0,1) draws of qzx.sample:
 * 1-layer [k,B,D1]; 2-layer eps = [k,B,D1] followed by [k,B,D2]. */
int iwae_forward(iwae_handle h, const float* x, int32_t B, int32_t k, float beta, const float* eps,
                 iwae_scalars* scalars, const iwae_tensors* want);

/* model.train_step(x, n_samples, beta, optimizer, objective) : src/iwae1.py:153-162 (main.py:143),
 * tasks/task02.py:87-101 for IWAE_OBJ_DREG.  lr = optimizer.learning_rate (main.py:93,128-133). */
int iwae_train_step(iwae_handle h, const float* x, int32_t B, int32_t k, float beta, float lr, int32_t objective,
                    const float* eps, iwae_scalars* scalars, const iwae_tensors* want);

/* the two halves of train_step, for data-parallel training: forward+backward leaves the flat fp32
 * gradient of THIS rank's shard (mean over its B images) on the device; the caller all-reduces
 * iwae_grad_devptr() (RCCL) and applies Adam with grad_scale = 1/world_size. */
int iwae_forward_backward(iwae_handle h, const float* x, int32_t B, int32_t k, float beta, int32_t objective,
                          const float* eps, iwae_scalars* scalars, const iwae_tensors* want);
int iwae_grad_devptr(iwae_handle h, void** dev_ptr, size_t* n);
/* iwae_forward_backward for a data-parallel step that overlaps its exchange with the backward pass: the gradient of the
 * decoder's layers -- floats [*side_offset, n) of the flat buffer, final long before the encoder's -- is completed on the
 * library's side stream (*side_stream, a hipStream_t) and NOT joined into the main stream: the caller orders its
 * all-reduce of that segment behind *side_stream and of [0, *side_offset) behind the main stream, makes the main stream
 * wait for both and calls iwae_adam_step.  Models without such a segment return *side_offset = n (nothing left on the
 * side stream: float32 mode, and steps on <= 2 048 data rows, whose weight gradients all run on the main stream).  No reference counterpart (the reference is
 * single-device, main.py:32). */
int iwae_forward_backward_split(iwae_handle h, const float* x, int32_t B, int32_t k, float beta, int32_t objective,
                                const float* eps, void** side_stream, size_t* side_offset);
int iwae_adam_step(iwae_handle h, float lr, float grad_scale);      /* keras Adam(lr, epsilon=1e-4), main.py:93 */

/* Training on incomplete images (Mattei & Frellsen 2019, MIWAE, arXiv 1902.02102): iwae_forward / iwae_forward_backward /
 * iwae_train_step with a per-pixel mask.  No reference counterpart.  DESIGN.md section 19.
 * mask [B, x_dim], host or device, non-zero = observed: exactly iwae_impute_options.mask.  mask == NULL delegates to the unmasked
 * call, bitwise.  With a mask the step differs in three places: the encoder reads xin = m ? x : 0 (iwae_impute's convention),
 * log p(x|z) sums the Bernoulli terms of the observed pixels only, and the backward pass starts from s = m ? x - sigmoid(l) : 0
 * (the encoder's first-layer weight gradient is taken against xin).  Unobserved pixels are SELECTED out, never multiplied out:
 * what x holds where m = 0 (NaN, garbage) reaches no scalar, tensor, gradient, parameter or Adam moment, bitwise -- iwae_impute's
 * contract.  An image with nothing observed has log p(x_obs|z) = 0 exactly, log_w = log p(z) - log q(z|x).
 * iwae_scalars.mean_lpxz and want->lpxz / log_w / al / z / snis_z / lpz / lqzx are those of the masked weights; IWAE_OBJ_VAE_ELBO_KL
 * uses the masked mean_lpxz.  Noise (eps, the handle's step) and the step's semantics are the unmasked calls'.  Bitwise repeatable.
 * Models: the 1-layer unconditional model, all five 1-layer objectives.  precision = IWAE_PREC_FP32: every width (DESIGN.md section 19;
 * options no_masked_out_fused / masked_out_min_rows, tools/README.md, pick between the two routes of the output layer).
 * precision = IWAE_PREC_BF16: handles whose hidden width pads to 64, 128 or 224 (n_hidden 33 .. 64, 97 .. 128,
 * 193 .. 224: the widths with a stored-s backward pass), option out_recompute off; the mask rides in the bf16 pixel rows as a hole code
 * (bits 0xFFFF) that the output layer's Bernoulli epilogue selects on, and the step is the unmasked bf16 step's plan under
 * no_bern_pipe + no_out_in_block.  The two precisions compute DIFFERENT numbers -- bf16 operands with float32 accumulation against
 * float32 throughout, as the unmasked calls do -- each bitwise repeatable; on one handle masked and unmasked calls may alternate freely.
 * A bf16 handle of any other hidden width or with out_recompute set, a 2-layer handle, cond_dim > 0, a handle with communicators
 * (iwae_comm_init), want->logits != NULL (no masked route materialises logits), B <= 0, k <= 0 or x NULL: IWAE_ERR_ARG before any
 * launch; the noise step, parameters, gradient buffer and Adam state are unchanged. */
int iwae_forward_masked(iwae_handle h, const float* x, const uint8_t* mask, int32_t B, int32_t k, float beta, const float* eps,
                        iwae_scalars* scalars, const iwae_tensors* want);
int iwae_forward_backward_masked(iwae_handle h, const float* x, const uint8_t* mask, int32_t B, int32_t k, float beta,
                                 int32_t objective, const float* eps, iwae_scalars* scalars, const iwae_tensors* want);
int iwae_train_step_masked(iwae_handle h, const float* x, const uint8_t* mask, int32_t B, int32_t k, float beta, float lr,
                           int32_t objective, const float* eps, iwae_scalars* scalars, const iwae_tensors* want);
/* keras.optimizers.Adam(learning_rate, beta_1, beta_2, epsilon) hyper-parameters of this handle's optimizer; the default
 * is what the reference trains with: Adam(lr, epsilon=1e-4) = (0.9, 0.999, 1e-4), main.py:93.  Keras form: epsilon is
 * added to sqrt(v) outside the bias correction.  They take effect with the next update and are NOT part of the saved
 * state: iwae_get_adam_state / iwae_set_adam_state carry m, v and the step count only, so whoever resumes from a checkpoint
 * calls iwae_set_adam again (a new handle starts at the default).  A rejected call (beta outside [0, 1), epsilon <= 0,
 * NaN) changes nothing. */
int iwae_set_adam(iwae_handle h, float beta_1, float beta_2, float epsilon);
/* conditional model (cond_dim > 0): y [n, cond_dim] (host or device) for the NEXT forward / train step / eval_llh / decode
 * of n images -- tasks/task05.py:108-118 (y_onehot), :185-190 (sample(z, y)).  Stays set until replaced. */
int iwae_set_condition(iwae_handle h, const float* y, int32_t n);
int iwae_set_step(iwae_handle h, uint32_t noise_step, uint32_t batch_offset); /* Philox counter words */

/* Data-parallel training INSIDE the library (BASELINE configs[4]; no reference counterpart, main.py:32 is single-device): one
 * process per GPU, every rank holds a handle created with the same seed / parameters and iwae_config.world_size / rank.
 * Rank 0 obtains an opaque id blob (iwae_comm_unique_id: RCCL ncclGetUniqueId, one per internal communicator), the caller
 * ships it to the other ranks by any means (MPI, a file, torch.distributed's store), and EVERY rank calls iwae_comm_init
 * with it (collective: ncclCommInitRank).  From then on iwae_train_step / iwae_train_step_dataset take the rank's shard
 * of the global batch (B = global batch / world_size images) and all-reduce the flat fp32 gradient with ncclAllReduce on the
 * library's own streams before Adam.  NOISE KEYS ARE THE CALLER'S JOB: the draws of an image are keyed by its global index,
 * batch_offset + row, and the library never adds rank * B itself -- every rank must call
 * iwae_set_step(step, global_batch_offset + rank * B) before each step (main.py and iwae_amd/parallel.py do), otherwise all ranks
 * draw the same noise and N ranks no longer reproduce what one rank would compute on the whole batch.  Adam runs with
 * grad_scale 1/world_size, identical on every rank (replicas stay bit-identical): the decoder's segment (done early, on the
 * side stream) is exchanged and applied there, beside the encoder's backward pass and the next encoder forward, exactly as
 * the single-GPU step defers it; the encoder's segment follows on the main stream.  RCCL is loaded at run time (dlopen):
 * the library itself does not link against it.  iwae_comm_destroy (or iwae_destroy) releases the communicators. */
int iwae_comm_unique_id(void* id_out, size_t cap, size_t* id_bytes);
int iwae_comm_init(iwae_handle h, const void* unique_id, size_t id_bytes, int32_t world_size, int32_t rank);
/* The checks of iwae_comm_init that need no other rank (arguments, handle state, RCCL loadable), without the rendezvous: ncclCommInitRank
 * blocks until every rank has entered it, so a multi-process caller runs this first, agrees on the outcome over its own channel, and only
 * then lets every rank call iwae_comm_init (no reference counterpart: the reference is single-device, main.py:24,32). */
int iwae_comm_preflight(iwae_handle h, const void* unique_id, size_t id_bytes, int32_t world_size, int32_t rank);
int iwae_comm_destroy(iwae_handle h);
/* what RCCL itself reports for the handle's communicators (ncclCommCount / ncclCommUserRank): *world_size = 0, *rank = -1 when
 * the handle has none.  bench.py records it so a multi-GPU line shows which exchange path ran and over how many ranks. */
int iwae_comm_info(iwae_handle h, int32_t* world_size, int32_t* rank);

/* test-set LLH loop of main.py:170-184: mean over N images of iwae_elbo(k samples, B=1), images
 * batched `chunk` at a time on the device (chunk <= 0: as many as the row cap per launch allows -- option eval_rows; by default 2^21 rows
 * where the whole decoder forward is ONE launch for the evaluator's precision (1-layer model, hidden width 200, unconditional, the fused
 * decoder kernels not switched off), 2^19 otherwise; beyond it an image's k samples are walked in chunks and merged with a running
 * log-sum-exp).
 * x: host or device pointer, [N, x_dim]; a host batch is uploaded once.  The launches' per-image estimates stay on the device until one
 * copy at the end: the call returns after one synchronisation.  An image's estimate does not depend on the launch it rode in (the draws are
 * keyed by the global image index: iwae_set_step).  llh_per_image may be NULL. */
int iwae_eval_llh(iwae_handle h, const float* x, int32_t N, int32_t k, int32_t chunk, double* llh, float* llh_per_image);
/* arithmetic of iwae_eval_llh, independent of iwae_config.precision: IWAE_PREC_FP32 by default (the reference evaluates in
 * float32, main.py:176; 10 000 images x k = 5000 take well under a second either way), IWAE_PREC_BF16 for the fast path. */
int iwae_set_eval_precision(iwae_handle h, int32_t precision);

/* IWAE.sample(z): decoder only -> probs [n, x_dim].  1-layer: src/iwae1.py:168-178, z [n,D1].  2-layer:
 * src/iwae2.py:184-196, z = z2 [n,D2]: z1 ~ p(z1|z2) is drawn on the device (Philox), then decoded. */
int iwae_decode(iwae_handle h, const float* z, int32_t n, float* probs);

/* tasks/plot_task01.py:31-78 (true posterior on a latent grid) and the exact log p(x) of a low-dimensional latent model by quadrature.
 * For image x_i and grid point z_g with log quadrature weight w_g (log_wq[g], or 0 when log_wq is NULL), l_g = decoder(z_g) in the eval
 * precision (iwae_set_eval_precision) and
 *   lj(i,g)   = sum_j [x_ij l_gj - softplus(l_gj)] + sum_d (-z_gd^2/2 - log(2 pi)/2)       (lpxz + lpz, src/iwae1.py:105-111)
 *   log_px[i] = LSE_g (lj(i,g) + w_g)                                                      (merged in double)
 *   post_mean, post_cov: mean and covariance of z under pi(i,g) = exp(lj + w_g - log_px[i])
 *   q_mu, q_sigma: the encoder heads (src/iwae1.py:39-42); lq(i,g) = sum_d log N(z_gd; mu_id, sigma_id)
 *   q_mass[i]    = sum_g exp(lq + w_g)               (near 1: the grid covers and resolves q(z|x_i))
 *   kl_q_post[i] = sum_g exp(lq + w_g) (lq - lj + log_px[i])   = KL(q(z|x) || p(z|x)) on the grid (log p(x) = ELBO + KL)
 *   log_joint    = lj [N, G], only materialised when asked.
 * 1-layer unconditional models with n_latent <= 4 and x_dim <= 800 only; x must be binary (checked on the device); N, G > 0: otherwise
 * IWAE_ERR_ARG.  G is processed in chunks (option grid_chunk, default 32 768 points, ~256 MB of chunk-sized buffers); an image's results
 * depend on G, the grid and the chunk size only (not on N, its position or the other images) and are bitwise reproducible.
 * x, z, log_wq: host or device; every output: host or device, [N], [N,D], [N,D,D] as named, or NULL (log_px is required). */
int iwae_grid_posterior(iwae_handle h, const float* x, int32_t N,          /* [N, x_dim], values in {0,1}; host or device */
                        const float* z, const float* log_wq, int32_t G,     /* grid [G, D]; log quadrature weight per point [G] or NULL (= 0) */
                        double* log_px,                                     /* [N]            required */
                        float* post_mean, float* post_cov,                  /* [N, D], [N, D, D]   or NULL */
                        float* q_mu, float* q_sigma,                        /* [N, D] encoder heads (src/iwae1.py:39-42) or NULL */
                        float* q_mass, float* kl_q_post,                    /* [N]            or NULL */
                        float* log_joint);                                  /* [N, G] or NULL (only materialised when asked) */

/* Active units (Burda et al. section 5.2; the reference's README TODO): for unit u of stochastic layer l, A_u = Cov_x(E_q[u|x]), the
 * population variance over the N images (divide by N), in double; the unit is active if A_u > 1e-2.
 *   layer 1: E_q[z1|x] = mu1(x), the encoder head (src/iwae1.py:39-42, src/iwae2.py:58-60): no sampling.
 *   layer 2: E_q[z2|x] = E_{z1 ~ q(z1|x)}[mu2(z1)] (mu2: the q(z2|z1) head, src/iwae2.py:61-65), estimated from k draws of
 *            z1 = mu1 + sigma1 eps; z2 is never sampled (the Rao-Blackwellised estimate).  The Monte Carlo error adds about
 *            E_x Var(mu2)/k to A_u, negligible at k = 5000.
 * Arithmetic in the eval precision (iwae_set_eval_precision).  Device draws (eps == NULL) are exactly those iwae_eval_llh would use at
 * the same step, offset, N and k (latent stream 0, row (batch_offset + i) k + s); a 2-layer call advances the noise step by one, a
 * 1-layer call ignores k and eps, draws nothing and leaves the step alone.  No launch holds more than eval_rows per-sample rows.
 * An image's post_mean depends only on the weights, the image, k and its draws (not on N, its position, eval_rows or the other
 * images) and is bitwise reproducible; activity and data_mean come from the per-image means in an order fixed by N.
 * Conditional models, N <= 0, k <= 0 (2-layer) or activity == NULL: IWAE_ERR_ARG. */
int iwae_latent_activity(iwae_handle h, const float* x, int32_t N,   /* [N, x_dim], host or device, any values in [0,1] */
                         int32_t k, const float* eps,                /* 2-layer: z1 draws per image; eps [k, N, D1] (reference order) or NULL */
                         double* activity,                           /* [D1 (+ D2)] required: A_u, layer 1's units first */
                         double* data_mean,                          /* [D1 (+ D2)] or NULL: mean over x of E_q[u|x] */
                         float* post_mean);                          /* [N, D1 (+ D2)] or NULL: E_q[u|x] per image */

/* Aggregate-posterior decomposition of the KL term the model trains on (Hoffman & Johnson 2016, "ELBO surgery"; Chen et al. 2018,
 * beta-TCVAE; no reference counterpart).  With q(z) = (1/N) sum_m q(z|x_m) over the N images given,
 *   (1/N) sum_n KL(q(z|x_n) || p(z)) = I_q(n; z) + KL(q(z) || prod_d q(z_d)) + sum_d KL(q(z_d) || p(z_d)) = mi + tc + dim_kl,
 * estimated exactly in the components (all N, the own one included) from S draws per image, z_{s,n} = mu_n + sigma_n eps_{s,n}; the heads
 * mu, sigma (src/iwae1.py:39-42) in the eval precision (iwae_set_eval_precision).  With c = log(2 pi)/2 and
 *   l(s,n|m,d)     = -((z_{s,n,d} - mu_{m,d}) / sigma_{m,d})^2 / 2 - log sigma_{m,d} - c
 *   log_qzd[s,n,d] = LSE_m l(s,n|m,d) - log N              log_qz[s,n] = LSE_m sum_d l(s,n|m,d) - log N
 *   lq_own[s,n,d]  = -eps^2/2 - log sigma_{n,d} - c         lp[s,n,d]   = -z^2/2 - c
 *   unit_mi[d] = mean_{s,n}(lq_own_d - log_qzd_d)           unit_kl[d]  = mean_{s,n}(log_qzd_d - lp_d)
 *   summary = { mi = mean(sum_d lq_own - log_qz), tc = mean(log_qz - sum_d log_qzd), dim_kl = sum_d unit_kl[d], kl = mean(sum_d lq_own - sum_d lp) }
 * (kl is summed on its own; kl = mi + tc + dim_kl holds to double rounding).  The N^2 S D per-unit terms l(s,n|m,d) behind log_qzd are
 * float32; behind log_qz the difference z - mu is float32 and its scaling, square and the sum over d are double (a float32 sum of 100 unit
 * terms is off by ~1e-5, more than mi = 0 at N = 1 allows); lq_own, lp and every sum over samples are double; log_qz and log_qzd are
 * returned and summed as float32.  mi <= log N; a collapsed unit has unit_kl and unit_mi near 0.
 * Models: 1-layer unconditional only (the 2-layer q(z2|x) is not Gaussian and its p(z1) not N(0,1)): a 2-layer handle or cond_dim > 0 is
 * IWAE_ERR_ARG.  N <= 0, S <= 0, x or summary NULL, or N > 2^24 or N * S > 2^27 (the launch grids' index range, not a memory bound):
 * IWAE_ERR_ARG, nothing launched, the noise step unchanged.  The workspace is about 4 (2 Dpad + 1) N S + 4 (ceil(N/512) + 2) (Dpad + 3) min(N S, 16 384)
 * + 20 N Dpad bytes, Dpad = D rounded up to 16 (0.1 GB at N = 10 000, S = 1, D = 100; 1 GB at S = 10); a call that does not fit fails with
 * IWAE_ERR_NOMEM like any other.
 * Draws: eps == NULL uses exactly what iwae_debug_eps(N, S, 0) returns at the current step and offset (latent stream 0, row
 * (batch_offset + n) S + s) and then advances the noise step by one; with eps given the step is left alone.
 * Determinism: a sample's log_qz / log_qzd depend only on the N heads (in their order) and that sample's eps -- not on S, the sample's
 * position or the other draws -- and repeat bitwise; summary, unit_kl and unit_mi are reduced in double in an order fixed by (N, S).
 * Numerical domain: finite and accurate for |eps| <= 8 and log sigma spread over +-6 across the images: the joint density carries a running
 * maximum, a unit's density is shifted by the sample's own component (its sum is >= 1, its largest term exp(eps^2/2 + log(sigma_own/sigma_m))
 * <= e^44).  x, eps: host or device; every output: host or device, NULL = not wanted (log_qz / log_qzd: only copied out when asked). */
int iwae_aggregate_posterior(iwae_handle h, const float* x, int32_t N,   /* [N, x_dim], host or device */
                             int32_t S, const float* eps,                /* draws per image; eps [S, N, D] (reference order) or NULL */
                             double* summary,                            /* [4] required: mi, tc, dim_kl, kl */
                             double* unit_kl, double* unit_mi,           /* [D] each or NULL */
                             float* q_mu, float* q_sigma,                /* [N, D] encoder heads or NULL */
                             float* log_qz, float* log_qzd);             /* [S, N] / [S, N, D] or NULL: only materialised when asked */

/* Gradient moments of the training estimator (Rainforth et al. 2018, arXiv 1802.04537; Tucker et al. 2019, arXiv 1810.04152): the
 * per-parameter mean and unbiased (M - 1) variance, in double, of M draws of the flat float32 gradient.  Draw j (0 <= j < M) is exactly
 * the gradient iwae_forward_backward(h, x, B, k, beta, objective, NULL, ...) leaves after iwae_set_step(s0 + j, batch_offset), s0 the
 * handle's current step: the gradient of the handle's loss, the mean over the B images (IWAE_OBJ_DREG: the encoder's part is the
 * gradient of inference_loss, tasks/task02.py:88-99).  The call advances the noise step by M, leaves the parameters and the Adam state
 * (m, v, t) bitwise unchanged and the last draw's gradient in the gradient buffer, uploads x once, uses the condition of
 * iwae_set_condition for every draw and never communicates (also on a data-parallel handle).  Welford fold per draw on the device, no
 * host sync between draws; mean and var bitwise reproducible.  Same objectives as iwae_forward_backward.
 * M < 2, B <= 0, k <= 0, x, mean or var NULL, or a rejected objective: IWAE_ERR_ARG, nothing launched, the step unchanged. */
int iwae_grad_moments(iwae_handle h, const float* x, int32_t B, int32_t k, float beta, int32_t objective,   /* x [B, x_dim], host or device */
                      int32_t M,                                         /* draws, >= 2 */
                      double* mean, double* var);                        /* [P] each, host or device */

/* Annealed importance sampling estimate of log p(x) with HMC transitions (Neal 2001; Wu, Burda, Salakhutdinov & Grosse 2017, "On the
 * quantitative analysis of decoder-based generative models"; no reference counterpart -- its README points to an annealed-IWAE repository).
 * Image n has C chains.  Base density p0 = q(z|x_n) (IWAE_AIS_INIT_ENCODER; heads mu, sigma of src/iwae1.py:39-42 in the eval precision) or
 * N(0, I) (IWAE_AIS_INIT_PRIOR: mu = 0, sigma = 1).  The chain state is the standardised e, z = mu + sigma e, so HMC runs with the identity
 * mass matrix at unit scale whatever sigma is.  With c = log(2 pi)/2,
 *   lj(e) = log p(x|z) + sum_d (-z_d^2/2 - c)   (src/iwae1.py:105-111)        l0(e) = sum_d (-e_d^2/2 - log sigma_d - c)
 *   for t = 1..T:  log_w += (betas[t] - betas[t-1]) (lj - l0)(e)               (float32 product terms, double accumulator per chain)
 *                  one HMC transition that leaves f_t ~ exp(-U_t) invariant, U_t(e) = -[(1 - b) l0(e) + b lj(e)], b = betas[t]:
 *                  grad U_t = (1 - b) e - b sigma (grad_z log p(x|z) - z)
 *                  p ~ N(0, I);  p -= (h/2) grad U;  L times { e += h p;  p -= h grad U (the last: h/2) }
 *                  dH = ((U_t(e') + |p'|^2/2) - U_t(e)) - |p|^2/2  (float32);  accept iff logf(u) < -dH  (a NaN dH rejects)
 *   log_px[n] = LSE_c log_w[c,n] - log C  (double)        ess[n] = (sum_c w)^2 / sum_c w^2
 * betas: any T + 1 values in [0,1]; ascending 0 -> 1 is the forward run (log_px is a stochastic lower bound of log p(x) in expectation),
 * descending 1 -> 0 started from exact posterior samples (z0) the reverse run of bidirectional Monte Carlo (Grosse et al. 2015), whose
 * E[exp(log_w)] = 1/p(x).  T = 1, betas = {0, 1}, encoder init: log_w is exactly the importance weight of iwae_eval_llh at k = C.
 * step_size h > 0; adapt != 0: each chain keeps its own h, multiplied after every transition by 1.02 if the chain's running acceptance
 * mean (accepts so far / transitions so far) exceeds 0.65, else by 0.98, and clamped to [1e-4, 0.5] (Wu et al.'s rule).  ADAPTATION MAKES
 * THE TRANSITION DEPEND ON THE CHAIN'S HISTORY: the kernel is then no longer Markov and the estimator's unbiasedness argument holds only
 * approximately; adapt = 0 is the exact scheme.
 * Noise: with eps0 = mom = unif = NULL the device Philox generator, counter (row lo, row hi, stream << 24 | d4, step), row = (batch_offset + n) C + c,
 * s0 = the handle's noise step: e_0 stream 0 at step s0 (exactly what iwae_debug_eps(N, C, 0) returns and iwae_eval_llh uses at k = C), the
 * momentum of transition t stream 3 at step s0 + t, its accept uniform stream 4 at step s0 + t (d4 = 0, word 0, u = ((r >> 8) + 0.5) 2^-24);
 * the call advances the noise step by T + 1.  With z0 [C,N,D] given, e_0 = (z0 - mu) / sigma and nothing is drawn at step s0 (the step still
 * advances by T + 1).  The caller's noise: eps0 [C,N,D], mom [T,C,N,D], unif [T,C,N] in the reference's order, all three or none (eps0 is
 * ignored beside z0), the step is left alone.
 * Models: the 1-layer unconditional model with n_hidden <= 208 only; a 2-layer handle, cond_dim > 0 or cond_prior: IWAE_ERR_ARG.  N, C, T or
 * L <= 0, a beta outside [0,1], step_size <= 0, some but not all noise pointers, a wrong struct_size, x / opt / out / betas / log_px NULL or
 * N C > 2^27: IWAE_ERR_ARG before any launch, the noise step unchanged.
 * Arithmetic: the chain is float32 (v_mfma_f32_16x16x4_f32) whatever iwae_set_eval_precision says; only the heads follow it.
 * Workspace: 4 N C (D + 4) bytes of chain state, two padded copies of the decoder's weights (about 2 x 4 (D H + H H + H X) bytes), and per
 * output asked for its own size (accept_rate: N C T bytes of flags; with the caller's noise on the host its copy, 4 T N C (D + 1) bytes).
 * Determinism: a chain's results depend only on the weights, its image and that image's heads, its own noise and the schedule -- not on N,
 * C, its position, the other chains or the launch chunking (option ais_t_chunk: transitions per launch) -- and repeat bitwise; log_px and
 * ess are reduced over an image's chains in chain order.
 * x, betas, z0, eps0, mom, unif: host or device.  Outputs: each host or device, NULL = not wanted and never materialised. */
typedef enum { IWAE_AIS_INIT_ENCODER = 0, IWAE_AIS_INIT_PRIOR = 1 } iwae_ais_init;
typedef struct {
    uint32_t struct_size;      /* = sizeof(iwae_ais_options) (72); ABI guard like iwae_config's */
    int32_t C;                 /* chains per image */
    int32_t T;                 /* transitions (temperatures beyond the first) */
    int32_t L;                 /* leapfrog steps per transition */
    const float* betas;        /* [T + 1] */
    float step_size;           /* h */
    int32_t adapt;             /* 0: fixed h; else per-chain adaptation (see above) */
    int32_t init;              /* iwae_ais_init */
    int32_t reserved;          /* 0 */
    const float* z0;           /* [C,N,D] initial states in z space, or NULL */
    const float* eps0;         /* [C,N,D]   the caller's noise: all three or none */
    const float* mom;          /* [T,C,N,D] */
    const float* unif;         /* [T,C,N]   in (0,1) */
} iwae_ais_options;
typedef struct {
    double* log_px;            /* [N]      required */
    double* log_w;             /* [C,N] */
    float* ess;                /* [N] */
    float* accept_rate;        /* [T]      mean over the N C chains */
    float* z;                  /* [C,N,D]  final states mu + sigma e */
    float* step_out;           /* [C,N]    final step sizes */
    float* q_mu;               /* [N,D]    (prior init: 0) */
    float* q_sigma;            /* [N,D]    (prior init: 1) */
    float* dH;                 /* [T,C,N] */
    uint8_t* accepted;         /* [T,C,N]  0 / 1 */
} iwae_ais_outputs;
int iwae_ais(iwae_handle h, const float* x, int32_t N,                     /* [N, x_dim], host or device, any values in [0,1] */
             const iwae_ais_options* opt, const iwae_ais_outputs* out);

/* Per-image optimisation of the variational posterior and what the inference-gap split needs from it (Cremer, Li & Duvenaud 2018,
 * "Inference Suboptimality in Variational Autoencoders"; Kim et al. 2018, semi-amortised VAEs -- the reference's README lists
 * harvardnlp/sa-vae; no reference counterpart).  Image n gets its own factorised Gaussian q_n = N(mu_n, sigma_n^2), sigma = exp(rho),
 * started at the caller's mu0 / sigma0 or at the encoder heads (src/iwae1.py:39-42, in the eval precision) and moved by T Adam
 * iterations that ASCEND a bound of S draws; E evaluation passes of S fresh draws each then score the result.  With e_s ~ N(0, I),
 * z_s = mu + sigma e_s and c = log(2 pi)/2,
 *   lj_s    = log p(x|z_s) + sum_d (-z_sd^2/2 - c)   (src/iwae1.py:105-111)      lq_s = sum_d (-e_sd^2/2 - rho_d - c)
 *   log_w_s = lj_s - lq_s                                                        g_s  = grad_z log p(x|z_s) - z_s
 *   wt_s    = 1/S (IWAE_LOCAL_ELBO)  or  softmax_s(log_w) (IWAE_LOCAL_IWAE)
 *   d/dmu_d = sum_s wt_s g_sd                     d/drho_d = sum_s wt_s g_sd (sigma_d e_sd) + 1
 * -- the reparameterised path derivative with the entropy term (sum_d rho_d) taken analytically; for IWAE_LOCAL_IWAE the gradient of
 * LSE_s log_w - log S (the + 1 is sum_s wt_s d(-lq_s)/drho).  bound[t] = mean_s log_w (ELBO) or LSE_s log_w - log S (IWAE) on the draws
 * of iteration t, before its update.  Adam in Keras form (epsilon outside the bias correction), per image, both moments zero at the
 * start: m = beta_1 m + (1 - beta_1) d, v = beta_2 v + (1 - beta_2) d^2, theta += lr sqrt(1 - beta_2^t) / (1 - beta_1^t) m / (sqrt(v) + epsilon),
 * t = 1..T.  After the last iteration: elbo[n] = mean over the E S evaluation draws of log_w, iwae[n] = LSE over them - log(E S), both
 * accumulated in double from float32 log_w in pass order, then sample order.
 * Arithmetic: the row products are float32 (v_mfma_f32_16x16x4_f32) as in iwae_ais, whatever iwae_set_eval_precision says (only the
 * encoder start follows it); an image's sums over s run in sample order in float32.
 * Noise: with eps == NULL iteration t (0-based) uses exactly what iwae_debug_eps(N, S, 0) returns at step s0 + t, s0 the handle's noise
 * step (latent stream 0, row (batch_offset + n) S + s), evaluation pass j the draws of step s0 + T + j, and the call advances the step by
 * T + E; so T = 0, E = 1 from the encoder start gives iwae[n] = iwae_eval_llh's per-image value at k = S on the same step.  With the
 * caller's eps [T + E, S, N, D] (the first T blocks: the iterations; the last E: the evaluation) the step is left alone.
 * Determinism: an image's outputs depend only on the weights, the image, its start, its draws and the options -- not on N, its position,
 * the other images or the launch chunking (option local_t_chunk: passes per launch) -- and repeat bitwise.
 * Models: the 1-layer unconditional model with n_hidden <= 208 and n_latent <= 128 (the chain kernel's limits); a 2-layer handle,
 * cond_dim > 0 or cond_prior: IWAE_ERR_ARG.  N <= 0, S outside 1..64, T < 0, E < 1, lr < 0, a beta outside [0, 1), epsilon <= 0, an
 * objective other than the two, exactly one of mu0 / sigma0, a wrong struct_size, x / opt / out / elbo NULL, N S > 2^27 or T or E > 2^24: IWAE_ERR_ARG
 * before any launch, the noise step unchanged.  sigma0 > 0 is the caller's precondition (rho = log sigma0 is not checked).
 * Workspace: 24 N D + 24 N bytes of state, two padded copies of the decoder's weights (as iwae_ais), per output asked for its own size and,
 * with the caller's eps on the host, its copy (4 (T + E) S N D bytes).
 * x, mu0, sigma0, eps: host or device.  Outputs: each host or device, NULL = not wanted. */
typedef enum { IWAE_LOCAL_ELBO = 0, IWAE_LOCAL_IWAE = 1 } iwae_local_objective;
typedef struct {
    uint32_t struct_size;      /* = sizeof(iwae_local_options) (64); ABI guard like iwae_ais_options' */
    int32_t S;                 /* draws per image per pass, 1..64 */
    int32_t T;                 /* Adam iterations, >= 0 */
    int32_t E;                 /* evaluation passes after the last iteration, >= 1, S fresh draws each */
    int32_t objective;         /* iwae_local_objective: what the iterations ascend */
    float lr, beta_1, beta_2, epsilon;   /* Adam (the shims default to 0.9, 0.999, 1e-4 as the project trains, main.py:93) */
    const float* mu0;          /* [N,D] start; both or none; NULL = the encoder heads in the eval precision */
    const float* sigma0;       /* [N,D] > 0 */
    const float* eps;          /* [T+E,S,N,D] the caller's N(0,1) draws, or NULL */
} iwae_local_options;
typedef struct {
    double* elbo;              /* [N]      required: mean over the E S evaluation draws of log_w */
    double* iwae;              /* [N]      LSE over the E S draws - log(E S) */
    float* mu;                 /* [N,D]    optimised */
    float* sigma;              /* [N,D]    optimised */
    float* q_mu;               /* [N,D]    where it started */
    float* q_sigma;            /* [N,D]    where it started */
    float* bound;              /* [T,N]    the S-draw objective of each iteration, before its update; T = 0: not written */
    float* grad;               /* [N,2D]   the last iteration's ascent direction (d/dmu | d/drho); T = 0: not written */
    float* log_w;              /* [E S,N]  evaluation log-weights, pass-major (the caller's standard errors) */
} iwae_local_outputs;
int iwae_local_posterior(iwae_handle h, const float* x, int32_t N,        /* [N, x_dim], host or device, any values in [0,1] */
                         const iwae_local_options* opt, const iwae_local_outputs* out);

/* iwae_ais and iwae_local_posterior for incomplete images (Mattei & Frellsen 2019): the AIS estimate of log p(x_obs), HMC draws from
 * p(z | x_obs), and the best factorised Gaussian for p(z | x_obs) -- the tight counterparts of iwae_impute's k-sample bound.  mask
 * [N, x_dim] marks the observed pixels (non-zero): exactly iwae_impute_options.mask.  The option and output structs are the unmasked calls'.
 * mask == NULL hands on to the unmasked call before any check of its own, bit for bit (the convention of the iwae_*_masked step calls).
 * Encoder: wherever the unmasked call uses the encoder heads (the encoder init of AIS; the encoder start and q_mu / q_sigma of the local
 * posterior) they are the heads of xin_nj = m_nj ? x_nj : 0 in the eval precision, as in iwae_impute.
 * Definitions: every formula of iwae_ais and iwae_local_posterior holds with
 *   log p(x|z)  ->  sum_{j: m_nj != 0} [x_nj l_j - softplus(l_j)]        and its gradient started from  s_j = m_nj ? x_nj - sigmoid(l_j) : 0
 * so the HMC target is p(z | x_obs) ~ p(x_obs | z) p(z), log_px estimates log p(x_obs), and the Adam ascent finds the factorised Gaussian
 * closest to p(z | x_obs).
 * Unobserved pixels are SELECTED out, not multiplied out (iwae_impute's contract): what x holds at a pixel with m = 0, NaN or garbage,
 * reaches no output, bitwise.  The kernels read rows xc = m ? x : a hole code (all ones, compared as bits; an observed x with exactly those
 * bits is stored one bit off, still a NaN) and the value of an unobserved pixel is only ever the unchosen side of a select.
 * An image with nothing observed has log p(x_obs|z) = 0 and a zero likelihood gradient: its AIS target is the prior and log p(x_obs) = 0;
 * its local posterior moves towards N(0, I).
 * Noise and determinism: the noise keys, the step advance (T + 1; T + E), the caller-noise rules, the chunking options (ais_t_chunk,
 * local_t_chunk), determinism and the reduction orders are the unmasked calls'; a chain's or image's outputs additionally depend on that
 * image's mask row and on nothing else.  With a mask of ones every output equals the unmasked call's, bitwise.
 * Hence: T = 1, betas = {0, 1}, encoder init: log_px is iwae_impute's log_px at k = C on the same step and offset (both draw
 * iwae_debug_eps(N, C, 0)); iwae_local_posterior_masked with T = 0, E = 1 from the encoder start: iwae[n] is iwae_impute's log_px at k = S
 * (each up to the other call's float32 kernels).
 * Models and refusals: the unmasked calls' (1-layer unconditional, n_hidden <= 208, n_latent <= 128, the same argument checks):
 * IWAE_ERR_ARG before any launch, the noise step unchanged.
 * Workspace: the unmasked calls', plus 4 N x_dim bytes for xin, 4 N x_dim for the coded rows and N x_dim for the mask's copy when it
 * arrives on the host.
 * mask: host or device. */
int iwae_ais_masked(iwae_handle h, const float* x, const uint8_t* mask, int32_t N,   /* x, mask [N, x_dim], host or device */
                    const iwae_ais_options* opt, const iwae_ais_outputs* out);
int iwae_local_posterior_masked(iwae_handle h, const float* x, const uint8_t* mask, int32_t N,
                                const iwae_local_options* opt, const iwae_local_outputs* out);

/* Masked importance-weighted bound on log p(x_obs) and the self-normalised importance-sampling (SNIS) estimate of E[x | x_obs] (Mattei &
 * Frellsen 2019, "MIWAE: Deep Generative Modelling and Imputation of Incomplete Data Sets"; the snis_z idea of src/iwae1.py:139 carried
 * through the decoder; no reference counterpart).  m [N, x_dim] marks the observed pixels (non-zero), NULL = every pixel observed: the call
 * is then the importance-weighted reconstruction.  The encoder sees xin_nj = m_nj ? x_nj : 0; (mu_n, sigma_n) are its heads
 * (src/iwae1.py:39-42) of xin_n in the eval precision.  Image n has k draws e_s ~ N(0, I); with z_s = mu + sigma e_s, l_s = decoder(z_s)
 * (src/iwae1.py:72-75, logits) and c = log(2 pi)/2,
 *   lpx_s   = sum_{j: m_nj != 0} [x_nj l_sj - softplus(l_sj)]       (src/iwae1.py:105-111 restricted to the observed pixels)
 *   log_w_s = lpx_s + sum_d (-z_sd^2/2 - c) - sum_d (-e_sd^2/2 - log sigma_d - c)
 *   al_s    = softmax_s(log_w)              log_px[n] = LSE_s log_w - log k              ess[n] = 1 / sum_s al_s^2
 *   xhat[n,j] = sum_s al_s sigmoid(l_sj)    for EVERY pixel j, the observed ones too (the caller puts the observed values back)
 * log_px is the k-sample IWAE bound on log p(x_obs): the unobserved pixels are marginalised by leaving them out of log p(x|z).
 * Unobserved pixels are SELECTED out, not multiplied out: what x holds at a pixel with m = 0 is never read into any result -- NaN or
 * garbage there changes nothing, bitwise.  Observed x may be any value in [0,1], as in iwae_ais.
 * Arithmetic: the row products are float32 (v_mfma_f32_16x16x4_f32) whatever iwae_set_eval_precision says, exactly as iwae_ais and
 * iwae_local_posterior (only the heads follow it); sigma enters z as exp(log sigma), as in iwae_local_posterior.  float32: a lane's sums
 * over the pixels of one pass of the output layer (16 ceil(n_hidden/16) pixels) and over its latent features, al_s = exp(log_w_s - max) * (float)(1 / sum), and xhat -- an image's
 * al_s sigmoid(l_sj) added in sample order within a 64-draw chunk, then the chunks in chunk order, then clamped to 1 (a convex
 * combination, the clamp takes the rounding of sum_s al_s).  double: a row's log_w -- the passes in pass order per lane, the three terms,
 * then the row's 16 lanes by a butterfly -- rounded to float32 once; and per image, over its float32 log_w in sample order,
 * sum_s exp(log_w_s - max) and its squares, hence log_px and ess.
 * Noise: with eps == NULL the draws are exactly what iwae_debug_eps(N, k, 0) returns at the handle's step and offset (latent stream 0, row
 * (batch_offset + n) k + s), and the call advances the noise step by one; so with mask == NULL, log_px[n] is iwae_eval_llh's per-image
 * value at the same k and step (up to the evaluator's other float32 kernels).  With the caller's eps [k, N, D] the step is left alone.
 * Determinism: an image's outputs depend only on the weights, the image, its mask, k and its draws -- not on N, its position, the other
 * images or the launch chunking (option impute_rows: rows per launch, whole images) -- and repeat bitwise.  No atomics; every reduction
 * has a fixed order.
 * Models: the 1-layer unconditional model with n_hidden <= 208 and n_latent <= 128 (the chain kernel's limits); a 2-layer handle,
 * cond_dim > 0 or cond_prior: IWAE_ERR_ARG.  N <= 0, k outside 1..65536, N k > 2^27, x / opt / out / log_px NULL or a wrong struct_size:
 * IWAE_ERR_ARG before any launch, the noise step unchanged.
 * Workspace: 4 k N bytes of log-weights and 16 N of per-image sums; with a mask 4 N x_dim for the masked input (and N x_dim for the mask's
 * copy when it arrives on the host); with xhat, for k > 64, 4 ceil(k / 64) x_dim' bytes per image of a launch (x_dim' = x_dim rounded up to
 * 16; at most impute_rows / 64 chunks: 26 MB at the defaults and 784 pixels); two padded copies of the decoder's weights (as iwae_ais);
 * per output asked for on the host its own size and, with the caller's eps on the host, its copy (4 k N D bytes).
 * x, mask, eps: host or device.  Outputs: each host or device, NULL = not wanted and never materialised (xhat == NULL: the second pass
 * over the decoder does not run). */
typedef struct {
    uint32_t struct_size;      /* = sizeof(iwae_impute_options) (24); ABI guard like iwae_local_options' */
    int32_t k;                 /* draws per image, 1..65536 */
    const uint8_t* mask;       /* [N, x_dim], non-zero = observed; NULL = every pixel observed */
    const float* eps;          /* [k, N, D] the caller's N(0,1) draws (reference order), or NULL */
} iwae_impute_options;
typedef struct {
    double* log_px;            /* [N]      required: LSE_s log_w - log k, the k-sample bound on log p(x_obs) */
    float* xhat;               /* [N, X]   sum_s al_s sigmoid(l_s): every pixel, observed ones too */
    float* ess;                /* [N]      1 / sum_s al_s^2 */
    float* log_w;              /* [k, N] */
    float* q_mu;               /* [N, D]   heads of the masked input */
    float* q_sigma;            /* [N, D] */
} iwae_impute_outputs;
int iwae_impute(iwae_handle h, const float* x, int32_t N,                  /* [N, x_dim], host or device, observed values in [0,1] */
                const iwae_impute_options* opt, const iwae_impute_outputs* out);

/* The two uses of the self-normalised importance weights beyond a pixel mean, on the device at scale: the SNIS estimate of the posterior's
 * mean and covariance in latent space, and sampling importance resampling (SIR) of R latent vectors per image from p(z | x_obs)
 * (the reference's tasks/task01.py:52-58 and tasks/plot_task01.py:74-88 do both on the host per image; the covariance is what the
 * approximation gap of iwae_local_posterior is made of, Cremer et al. 2018; the SIR draws are Mattei & Frellsen's multiple imputation).
 * The proposal, the mask semantics, log_w_s and al_s are iwae_impute's: image n has k draws e_s ~ N(0, I), z_s = mu + sigma e_s.
 * (1) Shared outputs.  log_w [k, N], log_px, ess, q_mu, q_sigma are bit for bit what iwae_impute returns on the same x, mask, k and noise:
 * both calls run the same heads step, pass (a) and pass (b) (and honour the same launch cap, option impute_rows).
 * (2) Moments, taken in the standardised variable e (q's own mean is the pilot, so one pass suffices):
 *   ebar_d = sum_s al_s e_sd        M2_dd' = sum_s (al_s e_sd) e_sd'        Ce = M2 - ebar ebar^T
 *   mean[n,d] = mu_d + sigma_d ebar_d        cov[n,d,d'] = sigma_d sigma_d' Ce_dd'
 * float32: al_s = exp(log_w_s - max) * (float)(1 / sum), and the sums over each 64-draw chunk of an image in sample order (M2 on
 * v_mfma_f32_16x16x4_f32, four draws per instruction).  double: the chunks in chunk order, Ce, and the products with mu and sigma, each
 * output rounded to float32 once.  cov is bitwise symmetric (one triangle is computed, the other mirrors it) and its diagonal is clamped
 * at 0.  With cov == NULL the second-moment product does not run; with mean == NULL too, no moment kernel runs.
 * (3) Resampling with replacement by the inverse CDF.  w_s = exp((double)(log_w_s - max)) (pass (b)'s exponential), c_s = sum_{j <= s} w_j
 * in double in sample order (c_{k-1} is pass (b)'s sum); draw r takes
 *   idx[r,n] = the smallest s with c_s > (double)u_{r,n} c_{k-1}          z[r,n,:] = mu + exp(log sigma) e_idx  (fmaf, pass (a)'s arithmetic)
 * and u = 1 (no such s) takes the first s whose c_s reaches c_{k-1}: the last draw of non-zero weight.  Passing unif with
 * u_{r,n} = (r + u0_n) / R, u0_n in [0,1), gives systematic resampling.  e_idx is regenerated from the index at the proposal's own Philox
 * row (batch_offset + n) k + idx (with the caller's eps: gathered from there): no [k, N, D] array of z ever exists.  u [R, N] returns the
 * uniforms used.  R = 0: no resampling; asking for idx, z or u then is IWAE_ERR_ARG.  R > 0 with none of the three asked for draws nothing.
 * (4) Noise.  eps == NULL: iwae_impute's draws (latent stream 0 at the handle's step).  unif == NULL: Philox stream 5 at the same step,
 * counter (row lo, row hi, 5 << 24, step) with row = (batch_offset + n) R + r, the uniform ((word 0 >> 8) + 0.5) 2^-24 as iwae_ais forms
 * its accept uniforms.  The call advances the noise step by one if and only if it drew anything on the device (eps, or uniforms that a
 * wanted idx, z or u needed); with both the caller's it is left alone.
 * Determinism: iwae_impute's contract.  An image's outputs depend only on the weights, the image, its mask, k, R and its own draws and
 * uniforms -- not on N, its position, the other images or the launch chunking -- and repeat bitwise.  No atomics; every reduction has a
 * fixed order and every trip count is known on the host; workgroups never communicate.  What x holds at an unobserved pixel reaches nothing.
 * Models and limits: iwae_impute's (1-layer, unconditional, n_hidden <= 208, n_latent <= 128).  IWAE_ERR_ARG before any launch, the noise
 * step unchanged: k outside 1..65536, R outside 0..65536, N <= 0, N k > 2^27, N R > 2^27, a wrong struct_size, reserved != 0, x / opt /
 * out / log_px NULL, idx / z / u with R = 0.
 * Workspace: iwae_impute's without xhat; for the moments 4 ceil(k / 64) (D'^2 + D') bytes per image of a launch (D' = n_latent rounded up
 * to 16; launches are cut so that this stays under 256 MB); for the resampling 8 k bytes per image of a launch (never 8 k N) and 4 R N of
 * indices; per output asked for on the host its own size.
 * x, mask, eps, unif: host or device.  Outputs: each host or device, NULL = not wanted and never materialised. */
typedef struct {
    uint32_t struct_size;      /* = sizeof(iwae_posterior_options) (40) */
    int32_t k;                 /* importance draws per image, 1..65536 */
    int32_t R;                 /* resampled draws per image, 0..65536 */
    int32_t reserved;          /* 0 */
    const uint8_t* mask;       /* [N, x_dim], non-zero = observed; NULL = every pixel observed */
    const float* eps;          /* [k, N, D] the caller's N(0,1) draws, or NULL */
    const float* unif;         /* [R, N] the caller's uniforms in [0,1], or NULL */
} iwae_posterior_options;
typedef struct {
    double* log_px;            /* [N]        required: as iwae_impute */
    float* ess;                /* [N] */
    float* mean;               /* [N, D]     SNIS estimate of E[z | x_obs] */
    float* cov;                /* [N, D, D]  SNIS estimate of Cov[z | x_obs] */
    int32_t* idx;              /* [R, N]     the resampled draws' indices into the k proposals */
    float* z;                  /* [R, N, D]  the resampled latent vectors */
    float* u;                  /* [R, N]     the uniforms used */
    float* log_w;              /* [k, N] */
    float* q_mu;               /* [N, D]     heads of the masked input */
    float* q_sigma;            /* [N, D] */
} iwae_posterior_outputs;
int iwae_posterior(iwae_handle h, const float* x, int32_t N,               /* [N, x_dim], host or device, observed values in [0,1] */
                   const iwae_posterior_options* opt, const iwae_posterior_outputs* out);

/* Data pipeline on the device (main.py:59-65,117-120 + src/utils.py:26-27): the grey-level training set
 * stays resident in HBM as uint8 [n, x_dim]; every epoch gets a visiting order (tf.data shuffle) and a
 * fresh dynamic binarisation, x = 1 iff (philox(seed, epoch, image, pixel/4) >> 8) < floor(g*2^24/255 + 0.5),
 * i.e. Bernoulli(g/255), one draw per image per epoch like the reference's per-epoch bernoullisample.
 * iwae_train_step_dataset takes rows [start, start+B) of the current order; gather + binarise are fused
 * into the input kernel, no host traffic.  iwae_dataset_get_batch returns the same batch for inspection.
 * The step and the inspection calls (get_batch, get_labels, get_mask): no uploaded set IWAE_ERR_STATE; a range outside
 * [0, n] (compared in 64 bits), B <= 0 or a null pointer IWAE_ERR_ARG.  A refused call launches nothing. */
int iwae_dataset_upload(iwae_handle h, const uint8_t* gray, int32_t n);
int iwae_dataset_begin_epoch(iwae_handle h, uint32_t epoch, const int32_t* order /* NULL keeps the order */, int32_t n);
int iwae_dataset_get_batch(iwae_handle h, int32_t start, int32_t B, float* x_out);
/* Conditional models (cond_dim > 0; tasks/task05.py:296-322 trains on (x, y) batches of a labelled set): one class id per image of the
 * uploaded set, each < cond_dim; kept resident next to the images.  iwae_train_step_dataset then feeds onehot(y) of the batch's images
 * wherever a host-fed step takes iwae_set_condition's rows (the encoder's input concat(x, onehot(y)), the decoder's concat(z, onehot(y)),
 * the prior network of tasks/task04.py) -- gathered by the same input kernel, no host traffic.  A new iwae_dataset_upload drops the labels.
 * iwae_dataset_get_labels returns the batch's one-hot rows [B, cond_dim] for inspection. */
int iwae_dataset_set_labels(iwae_handle h, const uint8_t* labels, int32_t n);
int iwae_dataset_get_labels(iwae_handle h, int32_t start, int32_t B, float* y_out);
/* Incomplete images on the resident set (MIWAE, Mattei & Frellsen 2019; the 1-layer unconditional model): one fixed mask per image, kept
 * resident bit-packed -- ceil(x_dim / 32) 32-bit words per image, pixel f = bit f & 31 of word f >> 5 (5.9 MB for 60 000 x 784).  The mask
 * belongs to the IMAGE: row i is image i of the uploaded set, not position i of the epoch's order, and no epoch changes it.
 * iwae_dataset_set_mask: mask [n, x_dim] bytes, host or device, non-zero = observed (the convention of iwae_impute_options.mask and
 * iwae_*_masked); n must be the uploaded set's size.  mask == NULL drops the masks; a new iwae_dataset_upload drops them too.
 * iwae_dataset_mcar_mask draws them on the device, missing completely at random: pixel f of image i is hidden iff
 * (philox4x32_10(counter = (i, 0x4D41534B 'MASK', f >> 2, 0), key = (mask_seed lo, hi))[f & 3] >> 8) < thr, thr = floor(rate 2^24 + 0.5)
 * computed once on the host in double (rate 0 hides nothing, rate 1 everything); keyed by the caller's mask_seed, not the handle's seed, so
 * models with different weight seeds can share one incomplete set.  iwae_amd/utils.py::device_mcar_mask restates it bit for bit.
 * iwae_dataset_get_mask returns the mask rows of a batch, [B, x_dim] bytes of 0 / 1 (host or device), rows order[start .. start + B), for
 * inspection; iwae_dataset_get_batch stays what it is, the complete binarised rows.
 * With masks set, iwae_train_step_dataset is exactly iwae_train_step_masked(h, x = what iwae_dataset_get_batch(start, B) returns, mask =
 * what iwae_dataset_get_mask(start, B) returns, ..., eps = NULL, want = NULL) from the same handle state -- scalars, gradient, parameters,
 * Adam moments, step count and noise step bitwise, in both precisions and on both routes of the float32 output layer -- with the batch
 * fed by ONE input kernel (gather, binarisation and every masked form of the rows; timed name "masked_input") and no host traffic.  Its
 * scope and refusals are iwae_train_step_masked's (IWAE_ERR_ARG before any launch, the handle unchanged): the 1-layer unconditional model,
 * no communicators, on a bf16 handle a hidden width that pads to 64, 128 or 224 with option out_recompute off.  Without masks the call
 * runs what it ran before masks existed, bit for bit.
 * Errors of iwae_dataset_set_mask / iwae_dataset_mcar_mask: a 2-layer or conditional handle, or no uploaded set: IWAE_ERR_STATE (as
 * iwae_dataset_set_labels); a wrong n, a rate outside [0, 1] or NaN: IWAE_ERR_ARG.  A bf16 handle of a width the masked step refuses may
 * hold masks: the step is what refuses.  iwae_dataset_get_mask: a bad range IWAE_ERR_ARG, no masks IWAE_ERR_STATE. */
int iwae_dataset_set_mask(iwae_handle h, const uint8_t* mask, int32_t n);
int iwae_dataset_mcar_mask(iwae_handle h, double rate, uint64_t mask_seed);
int iwae_dataset_get_mask(iwae_handle h, int32_t start, int32_t B, uint8_t* mask_out);
int iwae_train_step_dataset(iwae_handle h, int32_t start, int32_t B, int32_t k, float beta, float lr, int32_t objective,
                            iwae_scalars* scalars);

/* HIP-event timing of the step's heavy kernels, each on the stream it is launched on (used by bench.py's roofline
 * object): enable, run steps, then read the average launch duration.  enable = n > 0 brackets the kernels of every n-th
 * step (an event record costs a few us of stream bubble, so bench.py samples rather than timing every launch); 0 switches
 * it off.  name: "decoder_fwd" (whole decoder forward + log-likelihood), "out_bwd" (output-layer backward), "decoder_bwd" (the decoder's whole dX chain where it is one launch), "wgrad_out",
 * "dx_hidden", "dx_latent", "wgrad_hidden", "wgrad_latent" (the decoder's other backward kernels), "latent_bwd",
 * "encoder_fwd", "reduce_adam" (main-stream slab reduction + Adam), "ais_chain" (every launch of iwae_ais's chain kernel while timing is on), "local_q" (likewise iwae_local_posterior's local_q_kernel), "impute" (likewise both passes of iwae_impute's impute_rows_kernel, and pass (a) of iwae_posterior), "posterior" (likewise iwae_posterior's moments and merge launches), "masked_out" (likewise the masked float32 step's masked_out_f32_kernel), "masked_input" (likewise gather_binarize_masked_kernel, the input kernel of a masked iwae_train_step_dataset).  A kernel a configuration does not launch reports 0 launches. */
int iwae_enable_timing(iwae_handle h, int32_t enable);
int iwae_kernel_time(iwae_handle h, const char* name, double* avg_us, int64_t* launches);

/* Kernel-selection switches of a handle, for A/B measurements and for the parity tests that compare kernel variants of the same
 * mathematics (names and meanings: tools/README.md; the defaults are the measured best).  This call is the ONLY way to steer the
 * library: it never reads the environment.  Synchronises the handle's streams.  Unknown names fail with IWAE_ERR_ARG. */
int iwae_set_option(iwae_handle h, const char* name, int64_t value);

/* debugging: fetch an internal activation / gradient as float32 [rows, feat] (names in DESIGN.md) */
int iwae_debug_tensor(iwae_handle h, const char* name, float* out, size_t cap, int32_t* rows, int32_t* cols);
/* the N(0,1) draws the device generator produces for (B,k): [k,B,D] */
int iwae_debug_eps(iwae_handle h, int32_t B, int32_t k, int32_t layer, float* out);

#ifdef __cplusplus
}
#endif
#endif
