// Host side of libiwae_amd.so: error state, RCCL loading, the handle and its layer table, buffers, the step driver and the C ABI of
// include/iwae_amd.h.  The two steps' host paths are step_bf16.hip and step_f32.hip, the analyses analysis.hip.
// Step structure follows the reference's train_step (src/iwae1.py:153-162): forward (IWAE.call,
// :98-151), backward (closed form of tape.gradient), Adam (main.py:93).
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <stddef.h>
#include <stdlib.h>
#include <algorithm>
#include <random>
#include <memory>
#include <dlfcn.h>
#include "model.h"       // (the HIP runtime, RCCL's types, include/iwae_amd.h and kernels.h come with it)
#include "layout.h"

using namespace iwae;

static_assert(sizeof(iwae_config) == 64 && offsetof(iwae_config, struct_size) == 0 && offsetof(iwae_config, seed) == 32 && offsetof(iwae_config, cond_dim) == 48 &&
              offsetof(iwae_config, cond_prior) == 52 && offsetof(iwae_config, precision) == 56, "iwae_config layout is part of the ABI (iwae_amd/_capi.py)");
static_assert(sizeof(iwae_scalars) == 64 && sizeof(iwae_tensors) == 12 * sizeof(void*), "ABI struct layout");
static_assert(sizeof(iwae_ais_options) == 72 && offsetof(iwae_ais_options, betas) == 16 && offsetof(iwae_ais_options, step_size) == 24 && offsetof(iwae_ais_options, z0) == 40 &&
              offsetof(iwae_ais_options, unif) == 64 && sizeof(iwae_ais_outputs) == 10 * sizeof(void*), "iwae_ais_options / iwae_ais_outputs layout is part of the ABI (iwae_amd/_capi.py)");
static_assert(sizeof(iwae_local_options) == 64 && offsetof(iwae_local_options, objective) == 16 && offsetof(iwae_local_options, lr) == 20 && offsetof(iwae_local_options, epsilon) == 32 &&
              offsetof(iwae_local_options, mu0) == 40 && offsetof(iwae_local_options, eps) == 56 && sizeof(iwae_local_outputs) == 9 * sizeof(void*), "iwae_local_options / iwae_local_outputs layout is part of the ABI (iwae_amd/_capi.py)");
static_assert(sizeof(iwae_impute_options) == 24 && offsetof(iwae_impute_options, k) == 4 && offsetof(iwae_impute_options, mask) == 8 && offsetof(iwae_impute_options, eps) == 16 &&
              sizeof(iwae_impute_outputs) == 6 * sizeof(void*), "iwae_impute_options / iwae_impute_outputs layout is part of the ABI (iwae_amd/_capi.py)");
static_assert(sizeof(iwae_posterior_options) == 40 && offsetof(iwae_posterior_options, k) == 4 && offsetof(iwae_posterior_options, R) == 8 && offsetof(iwae_posterior_options, reserved) == 12 &&
              offsetof(iwae_posterior_options, mask) == 16 && offsetof(iwae_posterior_options, eps) == 24 && offsetof(iwae_posterior_options, unif) == 32 &&
              sizeof(iwae_posterior_outputs) == 10 * sizeof(void*), "iwae_posterior_options / iwae_posterior_outputs layout is part of the ABI (iwae_amd/_capi.py)");

static thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

// RCCL entry points, resolved at run time (the process may already hold torch's copy of librccl: that one is reused)
struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
static RcclApi g_rccl;
static int load_rccl() {
    if (g_rccl.lib) return IWAE_OK;
    const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
    void* lib = nullptr;
    for (const char* n : names) if ((lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD)) != nullptr) break;       // already in the process (e.g. torch's)
    if (!lib) for (const char* n : names) if ((lib = dlopen(n, RTLD_NOW | RTLD_LOCAL)) != nullptr) break;
    if (!lib) return fail(IWAE_ERR_STATE, std::string("RCCL not found (dlopen librccl.so): ") + (dlerror() ? dlerror() : ""));
    RcclApi r;
    r.lib = lib;
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(lib, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(lib, "ncclCommInitRank");
    r.AllReduce = (decltype(r.AllReduce))dlsym(lib, "ncclAllReduce");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(lib, "ncclCommDestroy");
    r.CommCount = (decltype(r.CommCount))dlsym(lib, "ncclCommCount");
    r.CommUserRank = (decltype(r.CommUserRank))dlsym(lib, "ncclCommUserRank");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(lib, "ncclGetErrorString");
    if (!r.GetUniqueId || !r.CommInitRank || !r.AllReduce || !r.CommDestroy || !r.CommCount || !r.CommUserRank || !r.GetErrorString) return fail(IWAE_ERR_STATE, "librccl.so lacks an expected symbol");
    g_rccl = r;
    return IWAE_OK;
}
#define NCCLCHK(expr)                                                                                              \
    do {                                                                                                           \
        ncclResult_t r_ = (expr);                                                                                  \
        if (r_ != ncclSuccess) return fail(IWAE_ERR_HIP, std::string(#expr) + ": " + g_rccl.GetErrorString(r_));    \
    } while (0)

static const char* const kTimedNames[T_COUNT] = {"out_bwd", "decoder_fwd", "wgrad_out", "dx_hidden", "dx_latent", "wgrad_hidden", "wgrad_latent",
                                                 "latent_bwd", "encoder_fwd", "reduce_adam", "decoder_bwd",
                                                 "allreduce_enc", "allreduce_dec",       // (the data-parallel step's two ncclAllReduce calls, each on its own stream)
                                                 "ais_chain",                            // (iwae_ais: every launch of ais_chain_kernel while timing is enabled)
                                                 "local_q",                              // (iwae_local_posterior: likewise local_q_kernel)
                                                 "impute",                               // (iwae_impute: likewise both passes of impute_rows_kernel)
                                                 "posterior",                            // (iwae_posterior: likewise its moments and merge launches)
                                                 "masked_out",                           // (the masked float32 step: likewise masked_out_f32_kernel)
                                                 "masked_input"};                        // (the masked step from the resident set: likewise gather_binarize_masked_kernel)

namespace {

void init_linear(Linear& L, int Kin, int Nspace, bool need_B, bool kmajor) {
    L.Kin = Kin;
    L.Nspace = Nspace;
    L.Kp32 = round_up(Kin, 32);
    L.Np32 = round_up(Nspace, 32);
    L.KT = L.Kp32 / 32;
    L.MG = (L.Np32 + 63) / 64;
    L.imgF_bytes = (size_t)L.MG * img_mg_group_bytes(L.KT);
    L.kmajor = kmajor ? 1 : 0;
    if (need_B) {
        if (kmajor) {
            L.MT_B = L.Kp32 / 16;                      // rows = in-features (hidden)
            L.imgB_bytes = (size_t)L.MG * 2 * L.MT_B * 1024;   // one k-group per 64 out-features
        } else {
            L.KT_B = L.Np32 / 32;
            L.MG_B = (L.Kp32 + 63) / 64;
            L.imgB_bytes = (size_t)L.MG_B * img_mg_group_bytes(L.KT_B);
        }
    }
    L.IT = L.Kp32 / 16;
    L.JT = L.Np32 / 16;
}

int alloc_linear(Linear& L) {
    HIPCHK(hipMalloc((void**)&L.imgF, L.imgF_bytes));
    HIPCHK(hipMemset(L.imgF, 0, L.imgF_bytes));
    if (L.imgB_bytes) {
        HIPCHK(hipMalloc((void**)&L.imgB, L.imgB_bytes));
        HIPCHK(hipMemset(L.imgB, 0, L.imgB_bytes));
    }
    return IWAE_OK;
}

void free_linear(Linear& L) {
    if (L.imgF) (void)hipFree(L.imgF);
    if (L.imgB) (void)hipFree(L.imgB);
    free_buf(L.slabW);
    free_buf(L.slabB);
}

// Keras creation order: a BasicBlock is l1, l2, lmu, lstd
void add_block(iwae_model* m, Linear* blk, const char* prefix, int Kin, int H, int D, bool need_dx_first) {
    const int base = (int)m->klayers.size();
    const char* nm[4] = {"l1", "l2", "lmu", "lstd"};
    const int kin[4] = {Kin, H, H, H}, nout[4] = {H, H, D, D};
    for (int i = 0; i < 4; ++i) {
        KerasLayer kl;
        kl.name = std::string(prefix) + "." + nm[i];
        kl.Kin = kin[i];
        kl.Nout = nout[i];
        kl.offW = m->nparam;
        m->nparam += (size_t)kin[i] * nout[i];
        kl.offb = m->nparam;
        m->nparam += nout[i];
        m->klayers.push_back(kl);
    }
    const int Dp = round_up(D, 32);
    init_linear(blk[0], Kin, H, need_dx_first, false);
    blk[0].nsub = 1; blk[0].sub[0] = base;
    init_linear(blk[1], H, H, true, false);
    blk[1].nsub = 1; blk[1].sub[0] = base + 1;
    init_linear(blk[2], H, 2 * Dp, true, false);
    blk[2].nsub = 2; blk[2].sub[0] = base + 2; blk[2].sub[1] = base + 3; blk[2].joff[1] = Dp;
}

void add_mlp3(iwae_model* m, Linear* mlp, const char* prefix, int D, int H, int X) {
    const int base = (int)m->klayers.size();
    const char* nm[3] = {"d1", "d2", "out"};
    const int kin[3] = {D, H, H}, nout[3] = {H, H, X};
    for (int i = 0; i < 3; ++i) {
        KerasLayer kl;
        kl.name = std::string(prefix) + "." + nm[i];
        kl.Kin = kin[i];
        kl.Nout = nout[i];
        kl.offW = m->nparam;
        m->nparam += (size_t)kin[i] * nout[i];
        kl.offb = m->nparam;
        m->nparam += nout[i];
        m->klayers.push_back(kl);
    }
    init_linear(mlp[0], D, H, true, false);
    mlp[0].nsub = 1; mlp[0].sub[0] = base;
    init_linear(mlp[1], H, H, true, false);
    mlp[1].nsub = 1; mlp[1].sub[0] = base + 1;
    init_linear(mlp[2], H, X, true, true);
    mlp[2].nsub = 1; mlp[2].sub[0] = base + 2;
}

std::vector<Linear*> all_linears(iwae_model* m) {
    std::vector<Linear*> v;
    for (int i = 0; i < 3; ++i) v.push_back(&m->enc1[i]);
    if (m->cfg.n_layers == 2) {
        for (int i = 0; i < 3; ++i) v.push_back(&m->enc2[i]);
        for (int i = 0; i < 3; ++i) v.push_back(&m->dec2[i]);
    }
    for (int i = 0; i < 3; ++i) v.push_back(&m->dec1[i]);
    if (m->has_prior) for (int i = 0; i < 3; ++i) v.push_back(&m->prior[i]);
    return v;
}

}  // namespace

// ---------------------------------------------------------------- helpers the step files and analysis.hip call too (declared in model.h)
// the layer table
int build_descs(iwae_model* m) {
    m->descs.assign(m->klayers.size(), LayerDesc());
    for (Linear* L : all_linears(m)) {
        for (int s = 0; s < L->nsub; ++s) {
            const KerasLayer& kl = m->klayers[L->sub[s]];
            LayerDesc& d = m->descs[L->sub[s]];
            d.Kin = kl.Kin; d.Nout = kl.Nout; d.joff = L->joff[s];
            d.offW = kl.offW; d.offb = kl.offb;
            d.imgF = L->imgF; d.KT_F = L->KT;
            d.imgB = L->imgB; d.KT_B = L->KT_B; d.MT_B = L->MT_B; d.imgB_kmajor = L->kmajor;
            d.slabW = ptr<float>(L->slabW); d.slabB = ptr<float>(L->slabB);
            d.nsplit = L->nsplit; d.slab_ld = L->JT * 16; d.slab_stride = (size_t)L->IT * 16 * L->JT * 16;
            d.slabB_stride = 0;
            if (m->plan.g2w && L == &m->dec1[2]) {      // pre-weighted output layer: the bias gradient is product row H (the pad feature that carries g_r) of every slab
                d.slabB = ptr<float>(L->slabW) + (size_t)kl.Kin * d.slab_ld;
                d.slabB_stride = d.slab_stride;
            }
        }
    }
    int blocks = 0, rblocks = 0;
    for (auto& d : m->descs) {
        d.block_begin = blocks;
        d.rblock_begin = rblocks;
        blocks += (d.Kin * d.Nout + d.Nout + 255) / 256;
        rblocks += ((d.Kin + 1) * ((d.Nout + 3) / 4) + 63) / 64;     // float4 groups: (Kin weight rows + bias row) x ceil(Nout/4)
    }
    auto at = [&](int i) { return i < (int)m->descs.size() ? TableBounds::At{m->descs[i].rblock_begin, m->descs[i].block_begin} : TableBounds::At{rblocks, blocks}; };
    const bool two = m->cfg.n_layers == 2;
    TableBounds& t = m->tb;      // (table order: enc1, enc2, dec2, dec1, prior)
    t.enc1_end = at(m->enc1[2].sub[m->enc1[2].nsub - 1] + 1);
    t.enc2 = two ? at(m->enc2[0].sub[0]) : t.enc1_end;
    t.dec2 = two ? at(m->dec2[0].sub[0]) : t.enc1_end;
    t.dec1 = at(m->dec1[0].sub[0]); t.dec1_out = at(m->dec1[2].sub[0]); t.dec1_end = at(m->dec1[2].sub[0] + 1);
    t.end = at((int)m->descs.size());
    if (!m->d_descs) HIPCHK(hipMalloc((void**)&m->d_descs, sizeof(LayerDesc) * m->descs.size()));
    HIPCHK(hipMemcpyAsync(m->d_descs, m->descs.data(), sizeof(LayerDesc) * m->descs.size(), hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (m->side) HIPCHK(hipStreamSynchronize(m->side));      // a deferred decoder update may still be reading the old table
    if (m->side2) HIPCHK(hipStreamSynchronize(m->side2));
    m->descs_dirty = false;
    m->g2w_descs = m->plan.g2w;
    return IWAE_OK;
}

// The two kernels that walk the layer table, with the handle's constants filled in.
// reduce_blocks: the slabs of reduce blocks a (and b, same launch) summed into the flat gradient on st; update: Adam (alpha) + the weight-image
// refresh in the epilogue; done: its completion event, riding on the dispatch packet; with_means: one extra block makes the step's batch means
void reduce_blocks(iwae_model* m, hipStream_t st, BlockRange a, BlockRange b, float alpha, bool update, hipEvent_t done, bool with_means) {
    const float* per_b = with_means ? ptr<float>(m->per_b) : nullptr;
    launch_reduce_grads(m->d_descs, (int)m->descs.size(), a.first, a.count, m->grad, m->param, m->mom, m->vel, alpha, m->adam_b1, m->adam_b2, m->adam_eps, update ? 1 : 0,
                        per_b, per_b ? m->B : 0, !per_b ? 0.f : m->cfg.n_layers == 2 ? 1.f : m->beta, per_b ? m->d_scalars : nullptr, st, b.first, b.count, done);
}
// adam_blocks: Adam on elementwise blocks [first, first + count) of the flat gradient times grad_scale; done as above (update = false: the weight images only)
void adam_blocks(iwae_model* m, hipStream_t st, int first, int count, float alpha, float grad_scale, hipEvent_t done, bool update) {
    launch_adam(m->d_descs, (int)m->descs.size(), count, m->param, m->grad, m->mom, m->vel, alpha, grad_scale, m->adam_b1, m->adam_b2, m->adam_eps, update ? 1 : 0, st, first, done);
}

// where a kernel of the call in flight finds the N(0,1) draws of a latent layer
EpsSrc eps_src(iwae_model* m, int layer) {
    EpsSrc e;
    e.user = nullptr;
    e.cache = m->epsc_ptr[layer];
    e.ldC = eps_ld(m, layer);
    if (m->user_eps) e.user = ptr<float>(m->epsbuf) + (layer == 0 ? 0 : (size_t)m->k * m->B * m->D[0]);
    e.B = m->B;
    e.seed = m->cfg.seed;
    e.row_offset = (uint64_t)m->call.batch_offset * (uint64_t)m->k;
    e.step = m->noise_step;
    e.stream = (uint32_t)layer;
    if (m->call.k_total > 0) {      // k-chunked evaluation: the unchunked call's Philox rows
        e.k_total = m->call.k_total; e.s_off = m->call.s_off; e.kc = m->k;
        e.row_offset = (uint64_t)m->call.batch_offset * (uint64_t)m->call.k_total;
    }
    return e;
}

// diagnostic (STAMPS=1 build + options dense_stamps_epi / dense_stamps_kt): record the phase stamps of the matching dense launch
int attach_dense_stamps(iwae_model* m, int epi, DenseArgs& a) {
    if (m->dstamp_epi != epi || m->dstamp_kt != a.KT || (a.M < 4096 && a.KT <= 8)) return IWAE_OK;
    m->dstamp_waves = std::max(((a.M + 127) / 128) * ((a.MG + a.mg_per_block - 1) / a.mg_per_block) * 4, epi == EPI_BERN ? ((a.M + 127) / 128) * 16 : 0);      // (bern_pipe_kernel: <= 16 waves per 128+ rows)
    CHK(ensure(m->dstamps, (size_t)m->dstamp_waves * 64, m->stream));
    a.stamps = ptr<unsigned long long>(m->dstamps);
    return IWAE_OK;
}

// Does block_fwd_kernel take the whole block on R rows (few rows: the encoder on the batch's images)?  Fills the shape half of its argument block.
bool block_fwd_shape(const iwae_model* m, const Linear* blk, int R, BlockFwdArgs& a) {
    memset(&a, 0, sizeof(a));
    a.ldX = blk[0].Kp32; a.img0 = blk[0].imgF; a.img1 = blk[1].imgF; a.img2 = blk[2].imgF;
    a.KT0 = blk[0].KT; a.KT1 = blk[1].KT; a.NT1 = blk[0].Np32 / 16; a.NT2 = blk[2].Np32 / 16; a.R = R;
    a.ldH = blk[0].Np32; a.ldYF = blk[2].Np32; a.split = (blk[2].nsub == 2) ? blk[2].joff[1] : (1 << 30);
    return m->opt.allow_block_fused && blk[1].Np32 == blk[0].Np32 && blk[2].KT == blk[1].KT && blk[1].Kp32 == blk[0].Np32 && block_fwd_ok(a);
}

// fills eps buffer `par` with the draws of (step, current batch offset) for M data rows on stream gs
int draw_eps(iwae_model* m, int par, uint32_t step, int M, hipStream_t gs, int max_blocks) {
    const int Mp = round_up(M, 128);
    iwae_model::EpsTag& tg = m->eps_tag[par];
    tg.valid = false;
    for (int l = 0; l < m->cfg.n_layers; ++l) {
        CHK(ensure(m->epsc[par][l], (size_t)Mp * m->Dp[l] * 4, m->stream));
        EpsSrc e = eps_src(m, l);
        e.user = nullptr; e.cache = nullptr; e.step = step;
        if (!(m->abl_skip & 16)) launch_eps_gen(e, M, m->D[l], eps_ld(m, l), ptr<float>(m->epsc[par][l]), gs, max_blocks);
    }
    HIPCHK(hipGetLastError());
    tg.valid = true; tg.step = step; tg.row_offset = (uint64_t)m->call.batch_offset * (uint64_t)m->k; tg.M = M;
    return IWAE_OK;
}

// What both forward passes start with: the argument checks, the conditional model's y rows of these images (*cond, null without) and the
// handle's per-call state.  A call that is refused leaves that state as it was.
int begin_forward(iwae_model* m, const float* x, int B, int k, float beta, const FwdCall& call, const float** cond) {
    const bool from_ds = m->ds_start >= 0;
    if ((!x && !from_ds) || B <= 0 || k <= 0) return fail(IWAE_ERR_ARG, "forward: need x, B > 0, k > 0");
    if ((int64_t)B * k > (int64_t)1 << 30) return fail(IWAE_ERR_ARG, "forward: B*k too large");
    const int row0 = from_ds ? 0 : call.cond_row0;
    *cond = nullptr;
    if (m->C > 0) {
        if (from_ds) {      // (x, y) from the resident set: the input kernel writes onehot(y) of the batch's images into m->cond (tasks/task05.py:296-322)
            if (!m->ds_has_labels) return fail(IWAE_ERR_STATE, "conditional model on the resident dataset: call iwae_dataset_set_labels first");
            CHK(ensure(m->cond, (size_t)B * m->C * 4, m->stream));
            m->cond_n = B;
        }
        if (row0 + B > m->cond_n) return fail(IWAE_ERR_STATE, "conditional model: call iwae_set_condition with y for these images first");
        *cond = ptr<float>(m->cond) + (size_t)row0 * m->C;
    }
    m->call = call; m->call.cond_row0 = row0;
    m->B = B; m->k = k; m->M = B * k; m->beta = beta;
    m->Mp = round_up(m->M, 128); m->Bp = round_up(B, 128);
    return IWAE_OK;
}

// The batch on the device: rows ds_start.. of the resident set, gathered by the epoch's order and binarised on the fly (main.py:117-120) into the
// bf16 rows m->xP -- and, keep_f32, into the float32 rows m->xin -- or the caller's x (host batches are staged in m->xin, device batches read in
// place).  *xd: the float32 rows, null where none were kept.
// masked (a resident masked batch, FwdCall::mask_resident): the same rows under the images' masks, in the one launch of
// gather_binarize_masked_kernel every form of them the caller's plan reads (MaskedStage; *xd: its float32 xin, null where the caller kept none).
int stage_input(iwae_model* m, const float* x, int B, bool keep_f32, const float** xd, const MaskedStage* masked) {
    *xd = x;
    if (masked) {
        if (m->ds_start < 0 || !m->ds_has_mask) return fail(IWAE_ERR_STATE, "forward: a resident masked batch without a resident set and its masks");
        GatherMaskedArgs g;
        memset(&g, 0, sizeof(g));
        g.data = ptr<uint8_t>(m->ds_data); g.order = ptr<int32_t>(m->ds_order); g.bits = ptr<uint32_t>(m->ds_mask);
        g.start = m->ds_start; g.B = B; g.X = m->X; g.Xp = m->Xinp; g.Bp = m->Bp; g.seed = m->cfg.seed; g.epoch = m->ds_epoch;
        g.XP = masked->xP; g.XC = masked->xcP; g.xin = masked->xin; g.mask = masked->mask; g.xcode = masked->xcode;
        {
            ScopedTimer tm(m, T_MASKED_INPUT);
            launch_gather_binarize_masked(g, m->stream);
        }
        m->ds_start = -1;
        *xd = masked->xin;
    } else if (m->ds_start >= 0) {
        CHK(ensure(m->xP, (size_t)m->Bp * m->Xinp * 2, m->stream));
        if (keep_f32) CHK(ensure(m->xin, (size_t)B * m->X * 4, m->stream));
        float* xf = keep_f32 ? ptr<float>(m->xin) : nullptr;
        launch_gather_binarize(ptr<uint8_t>(m->ds_data), ptr<int32_t>(m->ds_order), m->ds_start, m->ds_N, B, m->X, m->Xinp, m->Bp, m->cfg.seed, m->ds_epoch,
                               ptr<uint16_t>(m->xP), xf, m->stream, m->C > 0 ? ptr<uint8_t>(m->ds_labels) : nullptr, m->C, m->C > 0 ? ptr<float>(m->cond) : nullptr);
        m->ds_start = -1;
        *xd = xf;
    } else CHK(staged_in(m, x, m->xin, (size_t)B * m->X * 4, xd));
    return IWAE_OK;
}

float adam_alpha(iwae_model* m, float lr) {      // keras Adam: lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t); advances t
    m->adam_t += 1;
    const double t = (double)m->adam_t;
    return (float)((double)lr * sqrt(1.0 - pow((double)m->adam_b2, t)) / (1.0 - pow((double)m->adam_b1, t)));
}

int adam_impl(iwae_model* m, float lr, float gscale) {
    if (m->descs_dirty) CHK(build_descs(m));
    const float alpha = adam_alpha(m, lr);
    adam_blocks(m, m->stream, 0, m->tb.end.e, alpha, gscale);
    HIPCHK(hipGetLastError());
    return IWAE_OK;
}

// buffers, streams, the dense layers' launches
int ensure(DevBuf& b, size_t bytes, hipStream_t st) {
    if (bytes <= b.cap) return IWAE_OK;
    if (b.p) {
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    const size_t want = bytes + bytes / 8 + 256;
    HIPCHK(hipMalloc(&b.p, want));
    b.cap = want;
    return IWAE_OK;
}
void free_buf(DevBuf& b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

// orders the main stream behind a deferred decoder update (and the noise prefetch in front of it) still on the side stream
int join_side(iwae_model* m) {
    if (m->left.dec2) HIPCHK(hipStreamWaitEvent(m->stream, m->ev_dec2, 0));      // (the first side stream's own deferred update)
    if (m->left.dec) HIPCHK(hipStreamWaitEvent(m->stream, m->ev_dec, 0));
    m->left.dec = m->left.dec2 = false;
    return IWAE_OK;
}

int dense_fwd(iwae_model* m, Linear& L, int epi, const uint16_t* XP, int rows, uint16_t* YP, float* YF, int ldYF, const SampleArgs* zin) {
    DenseArgs a;
    memset(&a, 0, sizeof(a));
    a.X = XP; a.ldX = L.Kp32; a.img = L.imgF;
    a.split = (L.nsub == 2) ? L.joff[1] : (1 << 30);
    a.M = rows; a.KT = L.KT; a.MG = L.MG; a.mg_per_block = (rows <= 8192) ? 1 : L.MG; a.Np32 = L.Np32; a.g1_mask = m->opt.dense_g1_mask;
    a.stage_all = (a.mg_per_block == 1 && L.KT > 8 && (L.KT + 7) / 8 <= 4) ? 1 : 0;
    if (zin) {      // sampled-input mode: the layer makes its own input rows z = mu + sigma*eps (and keeps them in zin->ZP)
        a.zhead = zin->head; a.ldZH = zin->ldH; a.zeps = zin->eps.cache; a.zldE = zin->eps.ldC; a.zD = zin->D; a.zDp = zin->Dp;
        a.ZPout = zin->ZP; a.zlp = zin->lp_prior; a.zlq = zin->lq; a.k = zin->k;
        a.mg_per_block = L.MG;          // one block owns all out-feature groups of its rows (the z rows are made once)
    }
    a.YP = YP; a.ldYP = L.Np32; a.YF = YF; a.ldYF = ldYF;
    CHK(attach_dense_stamps(m, epi, a));
    launch_dense(epi, a, m->stream);
    HIPCHK(hipGetLastError());
    return IWAE_OK;
}

int block_alloc(iwae_model* m, Linear* blk, BlockWs& w, int R, int Rp, bool bwd, bool need_dx) {
    const int Hp = blk[0].Np32, N2 = blk[2].Np32;
    CHK(ensure(w.h1P, (size_t)Rp * Hp * 2, m->stream));
    CHK(ensure(w.h2P, (size_t)Rp * Hp * 2, m->stream));
    CHK(ensure(w.head, (size_t)Rp * N2 * 4, m->stream));
    if (bwd) {
        CHK(ensure(w.dheadP, (size_t)Rp * N2 * 2, m->stream));
        CHK(ensure(w.d2P, (size_t)Rp * Hp * 2, m->stream));
        CHK(ensure(w.d1P, (size_t)Rp * Hp * 2, m->stream));
        if (need_dx) CHK(ensure(w.dx, (size_t)Rp * blk[0].Kp32 * 4, m->stream));
    }
    (void)R;
    return IWAE_OK;
}

// xf != null: the input rows are still fp32 [R][xdim] and the fused kernel converts them into XP itself -- only where block_fwd_shape says
// that kernel runs (StepPlan::enc_takes_f32); elsewhere the caller runs prep_rows first
int block_fwd(iwae_model* m, Linear* blk, BlockWs& w, const uint16_t* XP, int R, const float* xf, int xdim) {
    BlockFwdArgs a;
    if (block_fwd_shape(m, blk, R, a)) {       // few rows: the whole block in one launch
        a.X = XP; a.H1 = ptr<uint16_t>(w.h1P); a.H2 = ptr<uint16_t>(w.h2P); a.YF = ptr<float>(w.head);
        if (xf) { a.Xf = xf; a.Xdim = xdim; a.XPout = const_cast<uint16_t*>(XP); }
        launch_block_fwd(a, m->stream);
        HIPCHK(hipGetLastError());
        return IWAE_OK;
    }
    if (xf) return fail(IWAE_ERR_STATE, "block_fwd: float32 input rows on a shape block_fwd_kernel does not cover");
    CHK(dense_fwd(m, blk[0], EPI_TANH, XP, R, ptr<uint16_t>(w.h1P), nullptr, 0));
    CHK(dense_fwd(m, blk[1], EPI_TANH, ptr<uint16_t>(w.h1P), R, ptr<uint16_t>(w.h2P), nullptr, 0));
    CHK(dense_fwd(m, blk[2], EPI_HEAD, ptr<uint16_t>(w.h2P), R, nullptr, ptr<float>(w.head), blk[2].Np32));
    return IWAE_OK;
}

bool is_device_ptr(const void* p, int device) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // plain host memory
    return at.type == hipMemoryTypeDevice && at.device == device;
}

int copy_in(iwae_model* m, DevBuf& dst, const void* src, size_t bytes) {
    CHK(ensure(dst, bytes, m->stream));
    HIPCHK(hipMemcpyAsync(dst.p, src, bytes, hipMemcpyDefault, m->stream));
    return IWAE_OK;
}

int copy_out(iwae_model* m, void* dst, const void* src, size_t bytes) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, m->stream));
    return IWAE_OK;
}

// ---------------------------------------------------------------- the step driver: what the step entry points of the C ABI share
// The only two places that choose between the precisions' passes.  iwae_eval_llh hands the forward m->eval_precision, everything else
// m->cfg.precision; the backward pass follows the handle's (and refuses a forward of the other precision).
int step_forward(iwae_model* m, int precision, const float* x, int B, int k, float beta, const float* eps, int objective, bool bwd, const iwae_tensors* want,
                 const FwdCall& call) {
    return precision == IWAE_PREC_FP32 ? forward_f32(m, x, B, k, beta, eps, objective, bwd, want, call) : forward_impl(m, x, B, k, beta, eps, objective, bwd, want, call);
}
int step_backward(iwae_model* m, int objective, StepEnd end, float lr) {
    return m->cfg.precision == IWAE_PREC_FP32 ? backward_f32(m, objective, end, lr) : backward_impl(m, objective, end, lr);
}

namespace {

int refresh_images(iwae_model* m) {   // rebuild bf16 A-images from the fp32 master weights
    if (m->descs_dirty) CHK(build_descs(m));
    adam_blocks(m, m->stream, 0, m->tb.end.e, 0.f, 1.f, nullptr, false);
    HIPCHK(hipGetLastError());
    return IWAE_OK;
}

int fetch_outputs(iwae_model* m, iwae_scalars* scalars, const iwae_tensors* want) {
    hipStream_t st = m->stream;
    const int B = m->B, k = m->k, M = m->M;
    const bool two = m->cfg.n_layers == 2;
    if (want) {
        const float* rowsrc[6] = {ptr<float>(m->rows[0]), ptr<float>(m->rows[1]), ptr<float>(m->rows[2]),
                                  ptr<float>(m->rows[3]), ptr<float>(m->rows[4]), ptr<float>(m->logw)};
        float* dsts[7];
        const float* srcs[7];
        int n = 0;
        if (want->lpxz) { dsts[n] = want->lpxz; srcs[n++] = rowsrc[0]; }
        if (want->lpz) { dsts[n] = want->lpz; srcs[n++] = rowsrc[1]; }
        if (want->lqzx) { dsts[n] = want->lqzx; srcs[n++] = two ? rowsrc[3] : rowsrc[2]; }
        if (want->lpz2 && two) { dsts[n] = want->lpz2; srcs[n++] = rowsrc[2]; }
        if (want->lqzx2 && two) { dsts[n] = want->lqzx2; srcs[n++] = rowsrc[4]; }
        if (want->log_w) { dsts[n] = want->log_w; srcs[n++] = rowsrc[5]; }
        if (want->al) { dsts[n] = want->al; srcs[n++] = ptr<float>(m->wn); }
        const size_t zmax = (size_t)M * std::max(m->D[0], two ? m->D[1] : 0);
        CHK(ensure(m->scratch, std::max((size_t)M * 4, zmax * 4 + (size_t)B * 256 * 4), st));
        for (int i = 0; i < n; ++i) {
            launch_export_rows(srcs[i], B, k, ptr<float>(m->scratch), st);
            CHK(copy_out(m, dsts[i], m->scratch.p, (size_t)M * 4));
        }
        for (int layer = 0; layer < (two ? 2 : 1); ++layer) {
            float* zdst = layer == 0 ? want->z : want->z2;
            float* sdst = layer == 0 ? want->snis_z : want->snis_z2;
            if (!zdst && !sdst) continue;
            SampleArgs s;
            memset(&s, 0, sizeof(s));
            BlockWs& hw = layer == 0 ? m->wenc1 : m->wenc2;
            s.head = ptr<float>(hw.head); s.ldH = 2 * m->Dp[layer]; s.Dp = m->Dp[layer]; s.D = m->D[layer];
            s.head_per_row = layer; s.M = M; s.Mp = m->Mp; s.k = k; s.B = B; s.eps = eps_src(m, layer);
            float* zdev = ptr<float>(m->scratch);
            launch_export_z(s, zdev, st);
            if (zdst) CHK(copy_out(m, zdst, zdev, (size_t)M * m->D[layer] * 4));
            if (sdst) {
                float* sdev = zdev + zmax;
                launch_snis(zdev, ptr<float>(m->wn), B, k, m->D[layer], sdev, st);
                CHK(copy_out(m, sdst, sdev, (size_t)B * m->D[layer] * 4));
            }
        }
        HIPCHK(hipGetLastError());
    }
    if (scalars) {
        HIPCHK(hipMemcpyAsync(m->h_scalars, m->d_scalars, SC_COUNT * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const float* s = m->h_scalars;
        memset(scalars, 0, sizeof(*scalars));
        scalars->vae_elbo = s[SC_VAE_ELBO];
        scalars->vae_elbo_kl = s[SC_VAE_ELBO_KL];
        scalars->iwae_elbo = s[SC_IWAE_ELBO];
        scalars->iwae_eq14 = s[SC_IWAE_EQ14];
        scalars->inference_loss = s[SC_INFERENCE_LOSS];
        scalars->mean_lpxz = s[SC_MEAN_LPXZ];
        scalars->mean_lpz = s[SC_MEAN_T1];
        scalars->mean_lqzx = s[SC_MEAN_T2];
        scalars->mean_kl = s[SC_KL];
    } else if (want) {
        HIPCHK(hipStreamSynchronize(st));
    }
    return IWAE_OK;
}

int check_objective(iwae_model* m, int objective) {
    if (objective < 0 || objective > 4) return fail(IWAE_ERR_ARG, "unknown objective");
    if (m->cfg.n_layers == 2 && (objective == OBJ_VAE_ELBO_KL || objective == OBJ_DREG))
        return fail(IWAE_ERR_ARG, "objective not defined for the 2-layer model (KeyError in src/iwae2.py:154-173)");
    if (m->C > 0 && objective == OBJ_DREG) return fail(IWAE_ERR_ARG, "the DReG estimator is defined for the unconditional 1-layer model (tasks/task02.py)");
    return IWAE_OK;
}

// Data-parallel step, second half (the gradient of this rank's shard is in m->grad; the backward pass, END_GRAD_SPLIT_HELD, left the decoder's
// segment to the side stream, its slabs not yet summed): all-reduce + Adam(grad_scale 1/N) of the decoder's layers on the SIDE stream -- they run
// beside the encoder's backward pass and the next encoder forward, as the single-GPU step's deferred update does -- and of the
// encoder's layers on the main stream.  Models without such a segment: one all-reduce + Adam on the main stream.
int dp_finish(iwae_model* m, float lr) {
    const float alpha = adam_alpha(m, lr);
    const float gs = 1.0f / (float)m->comm_world;
    if (m->descs_dirty) CHK(build_descs(m));
    const size_t n = m->nparam, off = m->left.split_offset;
    if (m->left.held.count > 0) {      // (set only with a segment, off < n, that nothing has joined: iwae_train_step calls nothing that joins between backward_impl and here)
        hipStream_t tail = on_stream(m, m->left.on);
        const int b0 = m->tb.dec1.e;
        // Two communicators, one per stream.  Until an N > 1 run has shown that the two collectives may be co-resident, they are ORDERED
        // on the device, and in the order in which their inputs become ready: the encoder's segment first (main stream: its gradient is
        // complete ~30 us before the decoder's, whose reduction waits for the hidden layers' weight gradients), the decoder's behind an
        // event recorded after it -- a wait that is normally already satisfied.  (Round 3 first had them the other way round: the main
        // stream's update and the next encoder forward then waited for the decoder's reduction, +22 us per step in the one-rank
        // rehearsal.)  Every rank enqueues them in this order.  Option dp_concurrent = 1 drops the wait.
        { ScopedTimer tm(m, T_AR_ENC); NCCLCHK(g_rccl.AllReduce(m->grad, m->grad, off, ncclFloat32, ncclSum, m->comm_main, m->stream)); }
        // Round 5: the order costs (almost) nothing.  The event rides on the dispatch packet of the encoder's update (the kernel right behind
        // the all-reduce: no record bubble on the main stream), and the tail stream waits for it IN FRONT of the decoder's slab reduction --
        // which backward_impl left to this function (StepLeft::held) -- i.e. right behind the wait for the output layer's gradient it performs
        // there anyway, ~15 us before the decoder's exchange instead of directly in front of it (a barrier packet costs its 6-10 us wherever
        // its event stands; here it falls into the shadow of the hidden layers' gradients).  Measured in the one-rank rehearsal: see DESIGN.md 8.
        adam_blocks(m, m->stream, 0, b0, alpha, gs, m->opt.dp_concurrent ? nullptr : m->ev_ar);
        if (!m->opt.dp_concurrent) HIPCHK(hipStreamWaitEvent(tail, m->ev_ar, 0));
        reduce_blocks(m, tail, m->left.held, BlockRange(), 0.0f, false, nullptr, false);
        m->left.held = BlockRange();
        { ScopedTimer tm(m, T_AR_DEC, tail); NCCLCHK(g_rccl.AllReduce(m->grad + off, m->grad + off, n - off, ncclFloat32, ncclSum, m->comm_side, tail)); }
        adam_blocks(m, tail, b0, m->tb.end.e - b0, alpha, gs, m->ev_dec);           // join_side() now waits for the decoder's UPDATE, not just its gradient
    } else {
        CHK(join_side(m));
        { ScopedTimer tm(m, T_AR_ENC); NCCLCHK(g_rccl.AllReduce(m->grad, m->grad, n, ncclFloat32, ncclSum, m->comm_main, m->stream)); }
        adam_blocks(m, m->stream, 0, m->tb.end.e, alpha, gs);
    }
    HIPCHK(hipGetLastError());
    return IWAE_OK;
}

// The bodies behind iwae_forward / iwae_forward_backward / iwae_train_step and their masked and resident-set twins: the entry point has made
// its checks and hands in the FwdCall (the caller's mask, the resident set's, or neither).  noise_step advances on success only.
int forward_call(iwae_model* m, const float* x, int B, int k, float beta, const float* eps, iwae_scalars* scalars, const iwae_tensors* want, const FwdCall& call) {
    CHK(step_forward(m, m->cfg.precision, x, B, k, beta, eps, OBJ_IWAE_ELBO, false, want, call));
    CHK(fetch_outputs(m, scalars, want));
    m->noise_step += 1;
    return IWAE_OK;
}
int forward_backward_call(iwae_model* m, const float* x, int B, int k, float beta, int objective, const float* eps, iwae_scalars* scalars, const iwae_tensors* want,
                          const FwdCall& call) {
    CHK(step_forward(m, m->cfg.precision, x, B, k, beta, eps, objective, true, want, call));
    CHK(step_backward(m, objective, END_GRAD));
    CHK(fetch_outputs(m, scalars, want));
    m->noise_step += 1;
    return IWAE_OK;
}
// The train step ends in one of three ways.  Data-parallel (iwae_comm_init): the exchange stands between gradient and update (dp_finish).  Tensors
// wanted: they refer to the forward before the update (src/iwae1.py:162), so the gradient is joined, the tensors fetched, and Adam follows as its
// own pass -- behind join_side, which waits for the float32 step's side stream and finds nothing to wait for behind a bf16 END_GRAD.  Else Adam
// rides in the epilogue of the gradient sums, the decoder's share deferred on the side stream.
int train_step_call(iwae_model* m, const float* x, int B, int k, float beta, float lr, int objective, const float* eps, iwae_scalars* scalars, const iwae_tensors* want,
                    const FwdCall& call) {
    CHK(step_forward(m, m->cfg.precision, x, B, k, beta, eps, objective, true, want, call));
    const StepEnd end = m->comm_main ? END_GRAD_SPLIT_HELD : want ? END_GRAD : END_UPDATE;
    CHK(step_backward(m, objective, end, lr));
    if (want) CHK(fetch_outputs(m, nullptr, want));
    if (m->comm_main) CHK(dp_finish(m, lr));
    else if (want) { CHK(join_side(m)); CHK(adam_impl(m, lr, 1.0f)); }
    CHK(fetch_outputs(m, scalars, nullptr));
    m->noise_step += 1;
    return IWAE_OK;
}

// A bf16 handle takes a mask where its backward pass starts from the stored s = m ? x - sigmoid(l) : 0: the kernels that recompute x - sigmoid(l)
// from the pixel rows (out_bwd_kernel / out_bwd_pair_kernel) know no mask.  Padded hidden widths 64, 128 and 224, option out_recompute off.
bool masked_bf16_ok(const iwae_model* m) { return m->opt.allow_s_mode && out_bwd_has_s_mode(m->dec1[2].KT); }
// what a masked call takes; refused before anything of the handle changes
int masked_scope(iwae_model* m, const char* who, const float* x, int B, int k, const iwae_tensors* want, bool resident = false) {
    const std::string w(who);
    if (m->cfg.n_layers != 1 || m->C > 0 || m->has_prior) return fail(IWAE_ERR_ARG, w + ": the masked step takes the 1-layer unconditional model only");
    if (m->comm_main) return fail(IWAE_ERR_ARG, w + ": the masked step is single-device (the handle has communicators)");
    if (m->cfg.precision != IWAE_PREC_FP32 && !masked_bf16_ok(m))
        return fail(IWAE_ERR_ARG, w + ": on a bf16 handle the masked step needs a hidden width that pads to 64, 128 or 224 and the stored-s backward pass (option out_recompute off); "
                                      "other handles: precision = IWAE_PREC_FP32");
    if (want && want->logits) return fail(IWAE_ERR_ARG, w + ": the masked step hands out no logits");
    if ((!x && !resident) || B <= 0 || k <= 0) return fail(IWAE_ERR_ARG, w + ": need x, B > 0, k > 0");
    if ((int64_t)B * k > (int64_t)1 << 30) return fail(IWAE_ERR_ARG, w + ": B*k too large");
    return IWAE_OK;
}
}  // namespace

// =================================================================== C ABI
extern "C" {

const char* iwae_last_error(void) { return g_err.c_str(); }
int iwae_version(void) { return 1; }
#ifndef IWAE_BUILD_ID
#define IWAE_BUILD_ID "unknown"
#endif
static const char kBuildIdMarker[] = "IWAE_BUILD_ID=" IWAE_BUILD_ID;      // (the marker lets a checker read the id from the file without loading it)
const char* iwae_build_id(void) { return kBuildIdMarker + 14; }

int iwae_create(const iwae_config* cfg, iwae_handle* out) {
    if (!cfg || !out) return fail(IWAE_ERR_ARG, "iwae_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(iwae_config))
        return fail(IWAE_ERR_ARG, "iwae_create: iwae_config.struct_size is " + std::to_string(cfg->struct_size) + ", this library's iwae_config has " +
                                      std::to_string(sizeof(iwae_config)) + " bytes (binding built against another include/iwae_amd.h?)");
    if (cfg->reserved != 0) return fail(IWAE_ERR_ARG, "iwae_config.reserved must be 0");
    if (cfg->precision != IWAE_PREC_BF16 && cfg->precision != IWAE_PREC_FP32) return fail(IWAE_ERR_ARG, "precision must be IWAE_PREC_BF16 or IWAE_PREC_FP32");
    if (cfg->world_size < 1 || cfg->rank < 0 || cfg->rank >= cfg->world_size) return fail(IWAE_ERR_ARG, "need world_size >= 1 and 0 <= rank < world_size");
    if (cfg->n_layers != 1 && cfg->n_layers != 2) return fail(IWAE_ERR_ARG, "n_layers must be 1 or 2 (main.py:17)");
    for (int i = 0; i < cfg->n_layers; ++i) {
        if (cfg->n_hidden[i] < 1 || cfg->n_hidden[i] > 256) return fail(IWAE_ERR_ARG, "n_hidden must be in [1,256]");
        if (cfg->n_latent[i] < 1 || cfg->n_latent[i] > 128) return fail(IWAE_ERR_ARG, "n_latent must be in [1,128]");
    }
    if (cfg->x_dim < 1 || cfg->x_dim > 4096) return fail(IWAE_ERR_ARG, "x_dim must be in [1,4096]");
    if (cfg->cond_dim < 0 || cfg->cond_dim > 64) return fail(IWAE_ERR_ARG, "cond_dim must be in [0,64]");
    if (cfg->cond_dim > 0 && cfg->n_layers != 1) return fail(IWAE_ERR_ARG, "the conditional model is 1-layer (tasks/task05.py:101)");
    if (cfg->cond_prior != 0 && cfg->cond_dim <= 0) return fail(IWAE_ERR_ARG, "cond_prior needs cond_dim > 0 (tasks/task04.py)");
    if (cfg->cond_dim > 0 && cfg->n_latent[0] + cfg->cond_dim > round_up(cfg->n_latent[0], 32))
        return fail(IWAE_ERR_ARG, "conditional model: n_latent + cond_dim must fit the 32-feature padding of z");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(IWAE_ERR_HIP, "no HIP device: the IWAE hot path needs an AMD GPU (there is no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(IWAE_ERR_ARG, "device " + std::to_string(cfg->device) + " out of range (" + std::to_string(ndev) + " HIP devices)");
    HIPCHK(hipSetDevice(cfg->device));
    // the half-built model is owned by `guard` until the very end: every failing path below (HIPCHK / CHK return) frees
    // its streams, events and device memory through iwae_destroy
    std::unique_ptr<iwae_model, void (*)(iwae_model*)> guard(new iwae_model(), iwae_destroy);
    iwae_model* m = guard.get();
    m->cfg = *cfg;
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && ncu > 0) m->num_cus = ncu;
    }

    m->X = cfg->x_dim;
    m->Xp32 = round_up(cfg->x_dim, 32);
    m->C = cfg->cond_dim;
    m->Xinp = round_up(cfg->x_dim + cfg->cond_dim, 32);
    for (int i = 0; i < 2; ++i) {
        m->H[i] = cfg->n_hidden[i]; m->D[i] = cfg->n_latent[i];
        m->Hp[i] = round_up(std::max(1, m->H[i]), 32); m->Dp[i] = round_up(std::max(1, m->D[i]), 32);
    }
    HIPCHK(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    m->own_stream = true;
    {   // the side stream carries work with slack (weight gradients, next step's noise, the deferred decoder update): lowest
        // priority, so the main stream's dependency chain gets the CUs first whenever both have workgroups ready
        int least = 0, greatest = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        int prio = least;
        HIPCHK(hipStreamCreateWithPriority(&m->side, hipStreamNonBlocking, prio));
        prio = least;
        HIPCHK(hipStreamCreateWithPriority(&m->side2, hipStreamNonBlocking, prio));
        HIPCHK(hipEventCreateWithFlags(&m->ev_s2, hipEventDisableTiming));
    }
    HIPCHK(hipEventCreateWithFlags(&m->ev_lse, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&m->ev_fork2, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&m->ev_join, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&m->ev_join2, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&m->ev_dec, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&m->ev_blk, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&m->ev_dec2, hipEventDisableTiming));
    if (cfg->n_layers == 1) {
        add_block(m, m->enc1, "enc", m->X + m->C, m->H[0], m->D[0], false);      // tasks/task05.py:113-118 when C > 0
        add_mlp3(m, m->dec1, "dec", m->D[0] + m->C, m->H[0], m->X);
        m->has_prior = cfg->cond_prior != 0;
        if (m->has_prior) add_block(m, m->prior, "prior", m->C, m->H[0], m->D[0], false);      // tasks/task04.py:108 (after the decoder)
    } else {
        add_block(m, m->enc1, "enc1", m->X, m->H[0], m->D[0], false);
        add_block(m, m->enc2, "enc2", m->D[0], m->H[1], m->D[1], true);
        add_block(m, m->dec2, "dec2", m->D[1], m->H[1], m->D[0], true);
        add_mlp3(m, m->dec1, "dec1", m->D[0], m->H[0], m->X);
    }
    for (Linear* L : all_linears(m)) CHK(alloc_linear(*L));
    const size_t nb = m->nparam * 4;
    HIPCHK(hipMalloc((void**)&m->param, nb));
    HIPCHK(hipMalloc((void**)&m->grad, nb));
    HIPCHK(hipMalloc((void**)&m->mom, nb));
    HIPCHK(hipMalloc((void**)&m->vel, nb));
    HIPCHK(hipMemset(m->grad, 0, nb));
    HIPCHK(hipMemset(m->mom, 0, nb));
    HIPCHK(hipMemset(m->vel, 0, nb));
    HIPCHK(hipMalloc((void**)&m->d_zero, 1024));
    HIPCHK(hipMemset(m->d_zero, 0, 1024));
    HIPCHK(hipMalloc((void**)&m->d_scalars, SC_COUNT * 4));
    HIPCHK(hipMemset(m->d_scalars, 0, SC_COUNT * 4));
    HIPCHK(hipHostMalloc((void**)&m->h_scalars, SC_COUNT * 4));
    // Keras Dense defaults: glorot-uniform kernels, zero biases (src/iwae1.py:31-34,72-75)
    std::vector<float> init(m->nparam, 0.f);
    std::mt19937_64 rng(cfg->seed ^ 0x9E3779B97F4A7C15ull);
    for (const KerasLayer& kl : m->klayers) {
        const double lim = sqrt(6.0 / (double)(kl.Kin + kl.Nout));
        std::uniform_real_distribution<double> U(-lim, lim);
        for (size_t i = 0; i < (size_t)kl.Kin * kl.Nout; ++i) init[kl.offW + i] = (float)U(rng);
    }
    HIPCHK(hipMemcpy(m->param, init.data(), nb, hipMemcpyHostToDevice));
    CHK(refresh_images(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    *out = guard.release();
    return IWAE_OK;
}

void iwae_destroy(iwae_handle m) {
    if (!m) return;
    (void)hipSetDevice(m->cfg.device);
    if (m->side) (void)hipStreamSynchronize(m->side);
    if (m->side2) (void)hipStreamSynchronize(m->side2);      // the decoder's all-reduce + Adam run on `tail`, which may be side2
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    if (m->comm_main && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(m->comm_main);
    if (m->comm_side && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(m->comm_side);
    for (Linear* L : all_linears(m)) free_linear(*L);
    DevBuf* bufs[] = {&m->xin, &m->xP, &m->epsbuf, &m->zP[0], &m->zP[1], &m->rows[0], &m->rows[1],
                      &m->rows[2], &m->rows[3], &m->rows[4], &m->rows[5], &m->logw, &m->wn, &m->gx, &m->cf, &m->per_b, &m->logw2, &m->wn2, &m->gx2, &m->cf2, &m->per_b2,
                      &m->dzdir, &m->scratch, &m->ds_data, &m->ds_order, &m->dstamps, &m->px_part, &m->dg2_part, &m->cond, &m->condP, &m->epsc[0][0], &m->epsc[0][1], &m->epsc[1][0], &m->epsc[1][1], &m->epsc[2][0], &m->epsc[2][1], &m->eval_lme,
                      &m->ds_labels, &m->ds_mask, &m->epsm[0][0], &m->epsm[0][1], &m->epsm[1][0], &m->epsm[1][1], &m->stamps};
    for (DevBuf* b : bufs) free_buf(*b);
    free_all(m->ev);
    free_all(m->grid);
    free_all(m->act);
    free_all(m->mom_ws);
    free_all(m->agg);
    free_all(m->ais);
    free_all(m->loc);
    free_all(m->imp);
    free_all(m->post);
    free_all(m->mk);
    for (BlockWs* w : {&m->wenc1, &m->wenc2, &m->wdec2, &m->wprior}) free_all(*w);
    free_all(m->wdec1);
    free_all(m->f32);
    if (m->param) (void)hipFree(m->param);
    if (m->grad) (void)hipFree(m->grad);
    if (m->mom) (void)hipFree(m->mom);
    if (m->vel) (void)hipFree(m->vel);
    if (m->d_descs) (void)hipFree(m->d_descs);
    if (m->d_zero) (void)hipFree(m->d_zero);
    if (m->d_scalars) (void)hipFree(m->d_scalars);
    if (m->h_scalars) (void)hipHostFree(m->h_scalars);
    for (int i = 0; i < T_COUNT; ++i) {
        for (hipEvent_t e : m->ev_start[i]) (void)hipEventDestroy(e);
        for (hipEvent_t e : m->ev_stop[i]) (void)hipEventDestroy(e);
    }
    if (m->side2) { (void)hipStreamSynchronize(m->side2); (void)hipStreamDestroy(m->side2); }
    if (m->ev_s2) (void)hipEventDestroy(m->ev_s2);
    if (m->ev_ar) (void)hipEventDestroy(m->ev_ar);
    if (m->side) { (void)hipStreamSynchronize(m->side); (void)hipStreamDestroy(m->side); }
    if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
    if (m->ev_fork2) (void)hipEventDestroy(m->ev_fork2);
    if (m->ev_join) (void)hipEventDestroy(m->ev_join);
    if (m->ev_join2) (void)hipEventDestroy(m->ev_join2);
    if (m->ev_dec) (void)hipEventDestroy(m->ev_dec);
    if (m->ev_lse) (void)hipEventDestroy(m->ev_lse);
    if (m->ev_dec2) (void)hipEventDestroy(m->ev_dec2);
    if (m->ev_blk) (void)hipEventDestroy(m->ev_blk);
    if (m->own_stream && m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
}

int iwae_set_stream(iwae_handle m, void* s) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    CHK(join_side(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (m->own_stream) { HIPCHK(hipStreamDestroy(m->stream)); m->own_stream = false; }
    if (s) {
        m->stream = (hipStream_t)s;
    } else {
        HIPCHK(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
        m->own_stream = true;
    }
    return IWAE_OK;
}

int iwae_sync(iwae_handle m) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    CHK(join_side(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    return IWAE_OK;
}

int iwae_param_count(iwae_handle m, size_t* n) {
    if (!m || !n) return fail(IWAE_ERR_ARG, "null argument");
    *n = m->nparam;
    return IWAE_OK;
}
int iwae_num_tensors(iwae_handle m, int32_t* n) {
    if (!m || !n) return fail(IWAE_ERR_ARG, "null argument");
    *n = (int32_t)m->klayers.size() * 2;
    return IWAE_OK;
}
int iwae_tensor_info(iwae_handle m, int32_t idx, char* name, size_t cap, int32_t* rows, int32_t* cols, size_t* offset) {
    if (!m || idx < 0 || idx >= (int32_t)m->klayers.size() * 2) return fail(IWAE_ERR_ARG, "tensor index out of range");
    const KerasLayer& kl = m->klayers[idx / 2];
    const bool bias = idx & 1;
    if (name && cap) snprintf(name, cap, "%s/%s", kl.name.c_str(), bias ? "bias" : "kernel");
    if (rows) *rows = bias ? kl.Nout : kl.Kin;
    if (cols) *cols = bias ? 1 : kl.Nout;
    if (offset) *offset = bias ? kl.offb : kl.offW;
    return IWAE_OK;
}

int iwae_set_params(iwae_handle m, const float* flat, size_t n) {
    if (!m || !flat || n != m->nparam) return fail(IWAE_ERR_ARG, "set_params: size mismatch");
    CHK(join_side(m));
    HIPCHK(hipMemcpyAsync(m->param, flat, n * 4, hipMemcpyDefault, m->stream));
    CHK(refresh_images(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    return IWAE_OK;
}
int iwae_get_params(iwae_handle m, float* flat, size_t n) {
    if (!m || !flat || n != m->nparam) return fail(IWAE_ERR_ARG, "get_params: size mismatch");
    CHK(join_side(m));
    HIPCHK(hipMemcpyAsync(flat, m->param, n * 4, hipMemcpyDefault, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return IWAE_OK;
}
int iwae_set_output_bias(iwae_handle m, const float* bias, size_t n) {
    if (!m || !bias || n != (size_t)m->X) return fail(IWAE_ERR_ARG, "set_output_bias: need x_dim values");
    CHK(join_side(m));
    HIPCHK(hipMemcpyAsync(m->param + m->klayers[m->dec1[2].sub[0]].offb, bias, n * 4, hipMemcpyDefault, m->stream));
    CHK(refresh_images(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    return IWAE_OK;
}
int iwae_get_grads(iwae_handle m, float* flat, size_t n) {
    if (!m || !flat || n != m->nparam) return fail(IWAE_ERR_ARG, "get_grads: size mismatch");
    CHK(join_side(m));
    HIPCHK(hipMemcpyAsync(flat, m->grad, n * 4, hipMemcpyDefault, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return IWAE_OK;
}
int iwae_get_adam_state(iwae_handle m, float* mo, float* ve, size_t n, int64_t* step) {
    if (!m || n != m->nparam) return fail(IWAE_ERR_ARG, "get_adam_state: size mismatch");
    CHK(join_side(m));
    if (mo) HIPCHK(hipMemcpyAsync(mo, m->mom, n * 4, hipMemcpyDefault, m->stream));
    if (ve) HIPCHK(hipMemcpyAsync(ve, m->vel, n * 4, hipMemcpyDefault, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (step) *step = m->adam_t;
    return IWAE_OK;
}
int iwae_set_adam_state(iwae_handle m, const float* mo, const float* ve, size_t n, int64_t step) {
    if (!m || !mo || !ve || n != m->nparam || step < 0) return fail(IWAE_ERR_ARG, "set_adam_state: bad argument");
    CHK(join_side(m));
    HIPCHK(hipMemcpyAsync(m->mom, mo, n * 4, hipMemcpyDefault, m->stream));
    HIPCHK(hipMemcpyAsync(m->vel, ve, n * 4, hipMemcpyDefault, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->adam_t = step;
    return IWAE_OK;
}

int iwae_forward(iwae_handle m, const float* x, int32_t B, int32_t k, float beta, const float* eps, iwae_scalars* scalars,
                 const iwae_tensors* want) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(m->cfg.device));
    return forward_call(m, x, B, k, beta, eps, scalars, want, FwdCall{m->batch_offset});
}

int iwae_forward_backward(iwae_handle m, const float* x, int32_t B, int32_t k, float beta, int32_t objective, const float* eps,
                          iwae_scalars* scalars, const iwae_tensors* want) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(m->cfg.device));
    CHK(check_objective(m, objective));
    return forward_backward_call(m, x, B, k, beta, objective, eps, scalars, want, FwdCall{m->batch_offset});
}

int iwae_forward_backward_split(iwae_handle m, const float* x, int32_t B, int32_t k, float beta, int32_t objective, const float* eps,
                                void** side_stream, size_t* side_offset) {
    if (!m || !side_stream || !side_offset) return fail(IWAE_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(m->cfg.device));
    CHK(check_objective(m, objective));
    CHK(step_forward(m, m->cfg.precision, x, B, k, beta, eps, objective, true, nullptr, FwdCall{m->batch_offset}));
    CHK(step_backward(m, objective, END_GRAD_SPLIT));
    if (m->cfg.precision == IWAE_PREC_FP32) CHK(join_side(m));      // float32 mode: nothing is left on the side stream (*side_offset = n)
    *side_stream = (void*)on_stream(m, m->left.on);
    *side_offset = m->left.split_offset;
    m->noise_step += 1;
    return IWAE_OK;
}

int iwae_grad_devptr(iwae_handle m, void** p, size_t* n) {
    if (!m || !p || !n) return fail(IWAE_ERR_ARG, "null argument");
    CHK(join_side(m));
    *p = m->grad;
    *n = m->nparam;
    return IWAE_OK;
}

int iwae_adam_step(iwae_handle m, float lr, float grad_scale) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(m->cfg.device));
    CHK(join_side(m));
    return adam_impl(m, lr, grad_scale);
}

// Kernel-selection switches of a handle (A/B measurements and the parity tests that compare kernel variants; the defaults are the
// measured best).  The library never reads the environment: this call is the only way to steer it.  Names: tools/README.md.
int iwae_set_option(iwae_handle m, const char* name, int64_t value) {
    if (!m || !name) return fail(IWAE_ERR_ARG, "set_option: null argument");
    HIPCHK(hipSetDevice(m->cfg.device));
    // a switch changes which kernels the next call launches: nothing of the previous calls may still be in flight
    CHK(join_side(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (m->side) HIPCHK(hipStreamSynchronize(m->side));
    if (m->side2) HIPCHK(hipStreamSynchronize(m->side2));
    m->have_forward = false;
    const bool on = value != 0;
    const int iv = (int)value;
    const std::string n(name);
    if (n == "out_recompute") m->opt.allow_s_mode = !on;                  // recompute the logits in out_bwd instead of keeping s
    else if (n == "no_defer") m->opt.allow_defer = !on;                   // join the decoder update at the end of every step
    else if (n == "wout_split") m->opt.wout_split = std::max(0, std::min(95, iv));      // percent of the rows in the output layer's EARLY gradient launch (0: one launch)
    else if (n == "wout_wg1") m->opt.wout_wg1 = std::max(1, iv);          // ... its workgroups / those of the late launch
    else if (n == "wout_wg2") m->opt.wout_wg2 = std::max(1, iv);
    else if (n == "defer_split") m->opt.defer_split = on;                 // 1-layer step: one deferred decoder update per side stream
    else if (n == "no_eps_multi") m->opt.allow_eps_multi = !on;           // few rows: one noise-draw launch per step instead of one per 8 steps
    else if (n == "no_zin") m->opt.allow_zin = !on;                       // always the separate sampling kernel
    else if (n == "zin_eval") m->opt.allow_zin_eval = on;                 // forward-only calls: z made in the decoder kernel's prologue (measured slower)
    else if (n == "no_chain2_bwd") m->opt.allow_chain2_bwd = !on;         // ... only their backward unfused
    else if (n == "no_chain2") m->opt.allow_chain2 = !on;                 // 2-layer model: the per-sample blocks unfused
    else if (n == "no_dec_bwd") m->opt.allow_dec_bwd = !on;               // the decoder's dX chain as three launches
    else if (n == "no_defer2_split") m->opt.allow_defer2_split = !on;     // ... one deferred update on `tail` instead of one per side stream
    else if (n == "no_defer2") m->opt.allow_defer2 = !on;                 // 2-layer step: one reduction + update of all layers on the main stream
    else if (n == "f32_dw_tiles") m->opt.f32_dw_tiles = std::max(1, iv);
    else if (n == "f32_dw_min_rows") m->opt.f32_dw_min_rows = std::max(16, iv);
    else if (n == "f32_gemm_dbg") m->opt.gemm_f32.dbg = iv;                // DIAG builds: timing ablations of gemm_f32_v2_kernel (1 no fetch, 2 no stash, 4 no MFMAs, 16 no barrier)
    else if (n == "f32_gemm_small_min") m->opt.gemm_f32.v2_small_min = std::max(1, iv);
    else if (n == "f32_ksplit_min_tiles") m->opt.gemm_f32.ksplit_min_tiles = std::max(1, iv);     // ... only from that many 64 x 64 output tiles on
    else if (n == "f32_no_ksplit") m->opt.gemm_f32.ksplit = !on;           // ... few-row products as one 64-tile launch
    else if (n == "f32_gemm_small_v1") m->opt.gemm_f32.v2_small = !on;     // ... the round-3 64-tile kernel for every 64 x 64-tiled product
    else if (n == "f32_gemm_w4") m->opt.gemm_f32.w8 = !on;                 // ... without the 8-wave tiles (A/B only)
    else if (n == "f32_gemm_v1") m->opt.gemm_f32.v2 = !on;                 // float32 GEMMs with the round-3 k loop (A/B only)
    else if (n == "no_f32_side") m->opt.allow_f32_side = !on;             // float32 step on one stream (no side-stream weight gradients, no deferred decoder update)
    else if (n == "f32_dw_last") m->opt.f32_dw_last = iv;                 // float32 step: all decoder weight gradients behind the dX chain (1: tiles as picked, 2: 4-wave tiles, 3: ... at 3 waves per SIMD)
    else if (n == "f32_wout_last") m->opt.f32_wout_first = !on;           // ... with the output layer's gradient last on the side stream (beside the encoder's few-row kernels) instead of first (beside the dX chain)
    else if (n == "no_f32_multi_reduce") m->opt.allow_f32_multi_reduce = !on;      // float32 mode: a slab reduction launch per gradient tensor instead of one per step
    else if (n == "f32_dec_fused_train") m->opt.f32_dec_fused_train = on;   // float32 training step: the decoder forward as dec_fwd_f32_kernel (round 4) instead of three GEMM launches
    else if (n == "no_f32_dec_fused") m->opt.allow_f32_dec_fused = !on;   // float32 mode: the decoder forward as three GEMM launches
    else if (n == "no_f32_bern_fused") m->opt.allow_f32_bern_fused = !on; // float32 mode: logits to memory, bern_f32_kernel / dl_f32_kernel as their own passes
    else if (n == "no_dec_rows") m->opt.allow_dec_rows = !on;             // few data rows: the decoder's weight gradients as the grouped launch on the side stream + deferred reduction
    else if (n == "no_wgrad_rows") m->opt.allow_wgrad_rows = !on;         // few rows: the encoder's weight gradients as the grouped launch + slabs + reduce_grads_kernel
    else if (n == "no_wg3") m->opt.allow_wg3 = !on;                       // few rows: the decoder's weight gradients as three launches on two streams
    else if (n == "g2w") m->opt.allow_g2w = on;                           // the decoder kernel leaves bf16(g_r g2); the output layer's weight gradient runs unweighted on it (measured slower)
    else if (n == "lat_rows4") m->opt.allow_lat_rows4 = on;               // many samples per image: latent_bwd_kernel's sums inside block_bwd_kernel<4> (measured no faster)
    else if (n == "no_lat_in_block") m->opt.allow_lat_in_block = !on;     // few images: latent_bwd_kernel as its own launch in front of the encoder's backward pass
    else if (n == "no_lse_in_bwd") m->opt.allow_lse_in_bwd = !on;         // few rows: lse_kernel as its own launch between decoder forward and backward
    else if (n == "no_lse_fused") m->opt.allow_lse_fused = !on;           // lse_kernel as its own launch behind the decoder kernel
    else if (n == "no_lse_dup") m->opt.allow_lse_dup = !on;               // one lse_kernel, the side stream forks behind it
    else if (n == "dz_f32") m->opt.allow_dz_half = !on;                   // dec_bwd_kernel leaves dz as float32
    else if (n == "no_small_dec_bwd") m->opt.small_dec_bwd = !on;         // per-pixel-group out_bwd + finish + two dX launches below 8 192 rows
    else if (n == "small_rows") m->opt.small_rows = iv;
    else if (n == "dec_rows") m->opt.dec_rows_max = iv;                   // dec_bwd_rows_kernel up to this many rows
    else if (n == "no_wg7") m->opt.allow_wg7 = !on;                       // the 16-wave weight-gradient shapes everywhere
    else if (n == "wg9") m->opt.wg_shape9 = iv;                           // bit mask: layers that take the 8 + 8-wave / 128-feature wgradws shape
    else if (n == "grid_chunk") m->opt.grid_chunk = iv > 0 ? std::max(16, iv) : 0;      // iwae_grid_posterior: grid points per chunk (0: the default)
    else if (n == "ais_t_chunk") m->opt.ais_t_chunk = iv > 0 ? iv : 0;                 // iwae_ais: transitions per launch (0: the default)
    else if (n == "local_t_chunk") m->opt.local_t_chunk = iv > 0 ? iv : 0;             // iwae_local_posterior: passes per launch (0: the default)
    else if (n == "no_masked_out_fused") m->opt.allow_masked_out_fused = !on;          // masked float32 step: always the general route (logits to memory, masked_bern_f32_kernel / masked_s_f32_kernel)
    else if (n == "masked_out_min_rows") m->opt.masked_out_min_rows = std::max(1, iv); // ... masked_out_f32_kernel from this many data rows on (1: wherever masked_out_f32_ok holds)
    else if (n == "impute_rows") m->opt.impute_rows = iv > 0 ? iv : 0;                 // iwae_impute: rows per launch, whole images (0: the default)
    else if (n == "eval_rows") m->opt.eval_rows = iv > 0 ? std::max(64, iv) : 0;       // data rows per evaluator launch
    else if (n == "no_bern_pipe") m->opt.allow_bern_pipe = !on;           // the Bernoulli forward on dense_kernel<EPI_BERN>
    else if (n == "no_block_fused") m->opt.allow_block_fused = !on;       // a BasicBlock on few rows as three dense_kernel launches
    else if (n == "no_out_in_block") m->opt.allow_out_in_block = !on;     // the few-row decoder's output layer as its own launch
    else if (n == "no_dec_fused") m->opt.allow_dec_fused = !on;           // the decoder's tanh layers as dense_kernel launches
    else if (n == "no_bern_qw") m->opt.bern_qw = !on;                     // the decoder kernel's 8-wave / 128-row shape
    else if (n == "bern_qw_force") m->opt.bern_qw_force = on;             // the 16-wave / 200-row shape at every row count
    else if (n == "dense_g1") m->opt.dense_g1_mask = (unsigned)iv;        // EPI bit mask of the 8-wave x 16-row dense shape
    else if (n == "wg8") m->opt.wg_target8 = std::max(1, iv);             // workgroup targets of the weight-gradient launches
    else if (n == "wg8_few") m->opt.wg_target8_few = std::max(1, iv);
    else if (n == "wg16") m->opt.wg_target16 = std::max(1, iv);
    else if (n == "wg16_1") m->opt.wg_target16_1 = std::max(1, iv);
    else if (n == "eps_blocks") m->opt.eps_blocks = std::max(0, iv);      // blocks of the ahead-of-time noise draw
    else if (n == "dec_bwd_nw") m->opt.dec_bwd_nw = iv == 8 ? 8 : 4;
    else if (n == "no_side2") m->opt.use_side2 = !on;                     // the hidden layers' weight gradients behind the output layer's
    else if (n == "wg_group") m->opt.allow_wg_group = on;                 // ... as one grouped launch
    else if (n == "no_early_wout") m->opt.allow_early_wout = !on;         // the output layer's weight gradient forks behind out_bwd
    else if (n == "dp_concurrent") m->opt.dp_concurrent = on;             // data-parallel step: no device-side order between its two all-reduces
#ifdef IWAE_DIAG
    // diagnostic builds only (DIAG=1 ./build.sh): in-kernel phase stamps and the weight-gradient ablations -- results are wrong or slower
    else if (n == "stamps") { m->want_stamps = on; if (on) { m->opt.allow_s_mode = false; m->opt.allow_bern_pipe = false; m->opt.allow_block_fused = false; m->opt.allow_dec_fused = false; } }
    else if (n == "dense_stamps_epi") m->dstamp_epi = iv;
    else if (n == "dense_stamps_kt") m->dstamp_kt = iv;
    else if (n == "wg_debug") m->wg_debug = iv;
    else if (n == "abl_skip") m->abl_skip = iv;      // launch ablations of the full-size step (timing only)
    else if (n == "fake_s") m->fake_s = iv;          // byte ablations (timing only): 1 dec_bwd_kernel reads s from 32 rows, 2 the output layer's gradient likewise, 4 the decoder kernel does not store s, 8 ... nor z / g1 / g2
#endif
    else return fail(IWAE_ERR_ARG, "set_option: unknown option '" + n + "'");
    return IWAE_OK;
}

int iwae_set_eval_precision(iwae_handle m, int32_t precision) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    if (precision != IWAE_PREC_BF16 && precision != IWAE_PREC_FP32) return fail(IWAE_ERR_ARG, "precision must be IWAE_PREC_BF16 or IWAE_PREC_FP32");
    m->eval_precision = precision;
    return IWAE_OK;
}

int iwae_set_adam(iwae_handle m, float beta1, float beta2, float epsilon) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(epsilon > 0.f)) return fail(IWAE_ERR_ARG, "set_adam: need 0 <= beta < 1, epsilon > 0");
    m->adam_b1 = beta1; m->adam_b2 = beta2; m->adam_eps = epsilon;
    return IWAE_OK;
}

int iwae_train_step(iwae_handle m, const float* x, int32_t B, int32_t k, float beta, float lr, int32_t objective, const float* eps,
                    iwae_scalars* scalars, const iwae_tensors* want) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(m->cfg.device));
    CHK(check_objective(m, objective));
    return train_step_call(m, x, B, k, beta, lr, objective, eps, scalars, want, FwdCall{m->batch_offset});
}

// ---- the masked step (DESIGN.md sections 19, 20): the unmasked entry points' bodies with FwdCall::mask set.  A null mask is the unmasked
// call, on every handle: it is handed on before the scope check
int iwae_forward_masked(iwae_handle m, const float* x, const uint8_t* mask, int32_t B, int32_t k, float beta, const float* eps, iwae_scalars* scalars,
                        const iwae_tensors* want) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    if (!mask) return iwae_forward(m, x, B, k, beta, eps, scalars, want);
    HIPCHK(hipSetDevice(m->cfg.device));
    CHK(masked_scope(m, "forward_masked", x, B, k, want));
    FwdCall call{m->batch_offset};
    call.mask = mask;
    return forward_call(m, x, B, k, beta, eps, scalars, want, call);
}

int iwae_forward_backward_masked(iwae_handle m, const float* x, const uint8_t* mask, int32_t B, int32_t k, float beta, int32_t objective, const float* eps,
                                 iwae_scalars* scalars, const iwae_tensors* want) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    if (!mask) return iwae_forward_backward(m, x, B, k, beta, objective, eps, scalars, want);
    HIPCHK(hipSetDevice(m->cfg.device));
    CHK(masked_scope(m, "forward_backward_masked", x, B, k, want));
    CHK(check_objective(m, objective));
    FwdCall call{m->batch_offset};
    call.mask = mask;
    return forward_backward_call(m, x, B, k, beta, objective, eps, scalars, want, call);
}

int iwae_train_step_masked(iwae_handle m, const float* x, const uint8_t* mask, int32_t B, int32_t k, float beta, float lr, int32_t objective,
                           const float* eps, iwae_scalars* scalars, const iwae_tensors* want) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    if (!mask) return iwae_train_step(m, x, B, k, beta, lr, objective, eps, scalars, want);
    HIPCHK(hipSetDevice(m->cfg.device));
    CHK(masked_scope(m, "train_step_masked", x, B, k, want));
    CHK(check_objective(m, objective));
    FwdCall call{m->batch_offset};
    call.mask = mask;
    return train_step_call(m, x, B, k, beta, lr, objective, eps, scalars, want, call);
}

int iwae_comm_unique_id(void* id_out, size_t cap, size_t* id_bytes) {
    if (!id_out || !id_bytes || cap < 2 * sizeof(ncclUniqueId)) return fail(IWAE_ERR_ARG, "comm_unique_id: need a buffer of >= 256 bytes");
    CHK(load_rccl());
    ncclUniqueId ids[2];
    NCCLCHK(g_rccl.GetUniqueId(&ids[0]));
    NCCLCHK(g_rccl.GetUniqueId(&ids[1]));
    memcpy(id_out, ids, sizeof(ids));
    *id_bytes = sizeof(ids);
    return IWAE_OK;
}

// Everything iwae_comm_init can refuse WITHOUT talking to another rank: arguments, handle state, RCCL loadable.  ncclCommInitRank is itself
// a blocking rendezvous: a rank that fails one of these checks must not leave the others inside it, so callers agree on the preflight's
// outcome first (iwae_amd/parallel.py::init_in_library_exchange) and only then enter iwae_comm_init together.
int iwae_comm_preflight(iwae_handle m, const void* unique_id, size_t id_bytes, int32_t world_size, int32_t rank) {
    if (!m || !unique_id || id_bytes != 2 * sizeof(ncclUniqueId)) return fail(IWAE_ERR_ARG, "comm_init: bad id blob (iwae_comm_unique_id makes it)");
    if (world_size < 1 || rank < 0 || rank >= world_size) return fail(IWAE_ERR_ARG, "comm_init: need 0 <= rank < world_size");
    if (world_size != m->cfg.world_size || rank != m->cfg.rank)
        return fail(IWAE_ERR_ARG, "comm_init: world_size / rank differ from the iwae_config this handle was created with");
    if (m->comm_main) return fail(IWAE_ERR_STATE, "comm_init: communicators already exist (iwae_comm_destroy first)");
    CHK(load_rccl());
    return IWAE_OK;
}

int iwae_comm_init(iwae_handle m, const void* unique_id, size_t id_bytes, int32_t world_size, int32_t rank) {
    CHK(iwae_comm_preflight(m, unique_id, id_bytes, world_size, rank));
    HIPCHK(hipSetDevice(m->cfg.device));
    CHK(join_side(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    ncclUniqueId ids[2];
    memcpy(ids, unique_id, sizeof(ids));
    // both communicators or neither: a half-initialised pair would send the next train step into ncclAllReduce with a null
    // communicator, and could not be retried ("communicators already exist")
    if (!m->ev_ar) HIPCHK(hipEventCreateWithFlags(&m->ev_ar, hipEventDisableTiming));
    ncclComm_t cm = nullptr, cs = nullptr;
    ncclResult_t r1 = g_rccl.CommInitRank(&cm, world_size, ids[0], rank);
    ncclResult_t r2 = r1 == ncclSuccess ? g_rccl.CommInitRank(&cs, world_size, ids[1], rank) : r1;
    if (r1 != ncclSuccess || r2 != ncclSuccess) {
        if (r1 == ncclSuccess && cm) (void)g_rccl.CommDestroy(cm);
        return fail(IWAE_ERR_HIP, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r1 != ncclSuccess ? r1 : r2));
    }
    m->comm_main = cm; m->comm_side = cs;
    m->comm_world = world_size; m->comm_rank = rank;
    return IWAE_OK;
}

int iwae_comm_destroy(iwae_handle m) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    CHK(join_side(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (m->side) HIPCHK(hipStreamSynchronize(m->side));
    if (m->side2) HIPCHK(hipStreamSynchronize(m->side2));      // `tail` (the decoder's exchange + update) may be either side stream
    if (m->comm_main) { NCCLCHK(g_rccl.CommDestroy(m->comm_main)); m->comm_main = nullptr; }
    if (m->comm_side) { NCCLCHK(g_rccl.CommDestroy(m->comm_side)); m->comm_side = nullptr; }
    m->comm_world = 1; m->comm_rank = 0;
    return IWAE_OK;
}

int iwae_comm_info(iwae_handle m, int32_t* world_size, int32_t* rank) {
    if (!m || !world_size || !rank) return fail(IWAE_ERR_ARG, "comm_info: null argument");
    *world_size = 0; *rank = -1;
    if (!m->comm_main) return IWAE_OK;            // no communicator: the handle trains alone
    int n = 0, r = -1, n2 = 0;
    NCCLCHK(g_rccl.CommCount(m->comm_main, &n));
    NCCLCHK(g_rccl.CommUserRank(m->comm_main, &r));
    NCCLCHK(g_rccl.CommCount(m->comm_side, &n2));
    if (n2 != n) return fail(IWAE_ERR_STATE, "comm_info: the two communicators disagree about the world size");
    *world_size = n; *rank = r;
    return IWAE_OK;
}

int iwae_set_condition(iwae_handle m, const float* y, int32_t n) {
    if (!m || !y || n <= 0) return fail(IWAE_ERR_ARG, "set_condition: bad argument");
    if (m->C <= 0) return fail(IWAE_ERR_STATE, "set_condition: the model was created with cond_dim = 0");
    HIPCHK(hipSetDevice(m->cfg.device));
    CHK(copy_in(m, m->cond, y, (size_t)n * m->C * 4));
    HIPCHK(hipStreamSynchronize(m->stream));       // y may be a temporary of the caller
    m->cond_n = n;
    return IWAE_OK;
}

int iwae_set_step(iwae_handle m, uint32_t noise_step, uint32_t batch_offset) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    m->noise_step = noise_step;
    m->batch_offset = batch_offset;
    return IWAE_OK;
}

int iwae_eval_llh(iwae_handle m, const float* x, int32_t N, int32_t k, int32_t chunk, double* llh, float* per_image) {
    if (!m || !x || N <= 0 || k <= 0 || !llh) return fail(IWAE_ERR_ARG, "eval_llh: bad argument");
    HIPCHK(hipSetDevice(m->cfg.device));
    // Launches of at most eval_rows data rows: `chunk` images x kc samples.  k <= eval_rows: whole images (kc = k).  Larger k: the
    // samples of an image are walked in chunks of kc and the per-chunk log-mean-exps are merged with a running log-sum-exp
    // (src/utils.py:6-8 is associative in that form) -- the activations of ALL k samples never exist at once.
    // (2^21 rows per launch at the reference's hidden width -- the single-launch decoder kernels keep nothing per pixel, ~0.4 KiB of HBM per row, and
    // the per-launch costs (image encoder on ~100 images, log-mean-exp, launch boundaries) are a quarter of what they are at 2^19: bf16 186 -> 205 k
    // images/s, float32 35.0 -> 36.7 k; other shapes, whose fallback paths may keep float32 logits, stay at 2^19)
    // (advisor, round 4: the large cap only where the single-launch decoder really runs for the evaluator's precision -- 1-layer model, the reference's
    // hidden width, and neither of the fused paths switched off; the 2-layer model and the unfused float32 path keep per-row tensors: 2^19)
    const bool eval_f32 = m->eval_precision == IWAE_PREC_FP32;
    const bool one_launch_dec = m->cfg.n_layers == 1 && m->dec1[2].KT == 7 && m->C == 0 && !m->has_prior &&
                                (eval_f32 ? (m->opt.allow_f32_dec_fused && m->opt.allow_f32_bern_fused) : (m->opt.allow_bern_pipe && m->opt.allow_dec_fused));
    const int eval_rows = m->opt.eval_rows > 0 ? m->opt.eval_rows : (one_launch_dec ? 1 << 21 : 1 << 19);
    const int kc = std::min(k, eval_rows);
    if (chunk <= 0) chunk = std::max(1, eval_rows / kc);
    chunk = std::min(chunk, N);
    // Round 4: no host round trip per launch.  The images go to the device once, every launch leaves its per-image log-mean-exps in one device
    // array [k-chunks][N], and ONE copy + synchronisation at the end feeds the same host arithmetic in the same order (the results are bitwise
    // what the per-launch copies gave); the k = 5000 evaluator's launches used to sit ~50 us apart (10 % of the bf16 evaluator's time).
    const int ns = (k + kc - 1) / kc;
    const float* xd = x;
    const size_t xbytes = (size_t)N * m->X * 4;
    if (xbytes <= ((size_t)1 << 31)) CHK(staged_in(m, x, m->ev.x, xbytes, &xd));      // (a larger host array is passed on as it is)
    CHK(ensure(m->eval_lme, (size_t)ns * N * 4, m->stream));
    int rc = IWAE_OK;
    for (int i0 = 0; i0 < N && rc == IWAE_OK; i0 += chunk) {
        const int nb = std::min(chunk, N - i0);
        FwdCall call{m->batch_offset + (uint32_t)i0, i0};
        call.log_w_only = call.no_ksplit = true;
        for (int si = 0; si < ns && rc == IWAE_OK; ++si) {
            const int s0 = si * kc, kn = std::min(kc, k - s0);
            call.k_total = kc < k ? k : 0; call.s_off = s0;
            rc = step_forward(m, m->eval_precision, xd + (size_t)i0 * m->X, nb, kn, 1.0f, nullptr, OBJ_IWAE_ELBO, false, nullptr, call);
            if (rc == IWAE_OK && hipMemcpyAsync(ptr<float>(m->eval_lme) + (size_t)si * N + i0, ptr<float>(m->per_b) + (size_t)PB_LME * nb, (size_t)nb * 4,
                                                hipMemcpyDeviceToDevice, m->stream) != hipSuccess)
                rc = fail(IWAE_ERR_HIP, "eval_llh: keeping the per-image estimates failed");
        }
    }
    if (rc != IWAE_OK) { (void)hipStreamSynchronize(m->stream); return rc; }
    std::vector<float> lme((size_t)ns * N);
    if (hipMemcpyAsync(lme.data(), m->eval_lme.p, lme.size() * 4, hipMemcpyDeviceToHost, m->stream) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess)
        return fail(IWAE_ERR_HIP, "eval_llh: copying the per-image estimates failed");
    double total = 0.0;
    for (int i = 0; i < N; ++i) {
        double run = 0.0;
        for (int si = 0; si < ns; ++si) {
            const int kn = std::min(kc, k - si * kc);
            const double part = (double)lme[(size_t)si * N + i] + log((double)kn);       // log sum_s exp(log_w) over this chunk of samples
            if (si == 0) run = part;
            else { const double hi = std::max(run, part), lo = std::min(run, part); run = hi + log1p(exp(lo - hi)); }
        }
        const double v = run - log((double)k);
        total += v;                    // MyMetric: sum / count (src/utils.py:39-41)
        if (per_image) per_image[i] = (float)v;
    }
    m->noise_step += 1;
    *llh = total / (double)N;
    return IWAE_OK;
}

int iwae_decode(iwae_handle m, const float* z, int32_t n, float* probs) {
    if (!m || !z || !probs || n <= 0) return fail(IWAE_ERR_ARG, "decode: bad argument");
    HIPCHK(hipSetDevice(m->cfg.device));
    CHK(join_side(m));
    hipStream_t st = m->stream;
    const bool two = m->cfg.n_layers == 2;
    const int np = round_up(n, 128), D0 = m->D[0], Dp0 = m->Dp[0], Hp = m->dec1[0].Np32, Xp = m->Xp32;
    MlpWs& w = m->wdec1;
    const int Din = two ? m->D[1] : D0, Dinp = two ? m->Dp[1] : Dp0;       // the caller's z is the LAST latent (z for 1 layer, z2 for 2)
    CHK(copy_in(m, m->xin, z, (size_t)n * Din * 4));
    CHK(ensure(m->zP[0], (size_t)np * Dp0 * 2, st));
    CHK(ensure(w.g1P, (size_t)np * Hp * 2, st));
    CHK(ensure(w.g2P, (size_t)np * Hp * 2, st));
    CHK(ensure(m->scratch, (size_t)np * Xp * 4, st));
    if (two) {
        // src/iwae2.py:184-196: pz1z2 = decode_z2_to_z1(z2); z1 = pz1z2.sample(); logits = decode_z1_to_x(z1)
        CHK(ensure(m->zP[1], (size_t)np * Dinp * 2, st));
        launch_prep_rows(ptr<float>(m->xin), nullptr, n, Din, 0, Dinp, np, ptr<uint16_t>(m->zP[1]), st);
        CHK(block_alloc(m, m->dec2, m->wdec2, n, np, false, false));
        CHK(block_fwd(m, m->dec2, m->wdec2, ptr<uint16_t>(m->zP[1]), n));
        for (int i = 0; i < 2; ++i) CHK(ensure(m->rows[i], (size_t)np * 4, st));
        SampleArgs s;
        memset(&s, 0, sizeof(s));
        s.head = ptr<float>(m->wdec2.head); s.ldH = 2 * Dp0; s.Dp = Dp0; s.D = D0; s.head_per_row = 1;
        s.M = n; s.Mp = np; s.k = 1; s.B = n;
        s.eps.user = nullptr; s.eps.B = n; s.eps.seed = m->cfg.seed; s.eps.row_offset = 0; s.eps.step = m->noise_step; s.eps.stream = 2;
        s.ZP = ptr<uint16_t>(m->zP[0]);
        s.lp_prior = ptr<float>(m->rows[0]); s.lq = ptr<float>(m->rows[1]); s.lq_dreg = nullptr;
        launch_sample(s, st);
        m->noise_step += 1;
    } else {
        if (m->C > 0 && n > m->cond_n) return fail(IWAE_ERR_STATE, "conditional model: call iwae_set_condition with y for these rows first");
        if (m->has_prior) {
            // tasks/task04.py:190-196: z_new = pzy.loc + pzy.scale * z with pzy the conditional prior of the label rows
            const int Cp = round_up(m->C, 32);
            CHK(ensure(m->condP, (size_t)np * Cp * 2, st));
            launch_prep_rows(ptr<float>(m->cond), nullptr, n, m->C, 0, Cp, np, ptr<uint16_t>(m->condP), st);
            CHK(block_alloc(m, m->prior, m->wprior, n, np, false, false));
            CHK(block_fwd(m, m->prior, m->wprior, ptr<uint16_t>(m->condP), n));
            for (int i = 0; i < 2; ++i) CHK(ensure(m->rows[i], (size_t)np * 4, st));
            SampleArgs s;
            memset(&s, 0, sizeof(s));
            s.head = ptr<float>(m->wprior.head); s.ldH = 2 * Dp0; s.Dp = Dp0; s.D = D0; s.head_per_row = 1;
            s.M = n; s.Mp = np; s.k = 1; s.B = n;
            s.eps.user = ptr<float>(m->xin); s.eps.B = n;          // the caller's z plays the role of the N(0,1) draw
            s.ZP = ptr<uint16_t>(m->zP[0]);
            s.cond = ptr<float>(m->cond); s.C = m->C;
            s.lp_prior = ptr<float>(m->rows[0]); s.lq = ptr<float>(m->rows[1]); s.lq_dreg = nullptr;
            launch_sample(s, st);
        } else {
            launch_prep_rows(ptr<float>(m->xin), m->C > 0 ? ptr<float>(m->cond) : nullptr, n, D0, m->C, Dp0, np, ptr<uint16_t>(m->zP[0]), st);
        }
    }
    CHK(dense_fwd(m, m->dec1[0], EPI_TANH, ptr<uint16_t>(m->zP[0]), n, ptr<uint16_t>(w.g1P), nullptr, 0));
    CHK(dense_fwd(m, m->dec1[1], EPI_TANH, ptr<uint16_t>(w.g1P), n, ptr<uint16_t>(w.g2P), nullptr, 0));
    CHK(dense_fwd(m, m->dec1[2], EPI_SIGMOID, ptr<uint16_t>(w.g2P), n, nullptr, ptr<float>(m->scratch), Xp));
    HIPCHK(hipMemcpy2DAsync(probs, (size_t)m->X * 4, m->scratch.p, (size_t)Xp * 4, (size_t)m->X * 4, n, hipMemcpyDefault, st));
    HIPCHK(hipStreamSynchronize(st));
    m->have_forward = false;
    return IWAE_OK;
}

// M draws of the training gradient (Rainforth et al. 2018): draw j is what iwae_forward_backward leaves after iwae_set_step(s0 + j, offset),
// folded into a per-parameter mean and M2 by moments_fold_kernel after each draw, in stream order; one host sync at the end
int iwae_grad_moments(iwae_handle m, const float* x, int32_t B, int32_t k, float beta, int32_t objective, int32_t M, double* mean, double* var) {
    if (!m || !x || !mean || !var || B <= 0 || k <= 0 || M < 2) return fail(IWAE_ERR_ARG, "grad_moments: need x, mean, var, B > 0, k > 0, M >= 2");
    if ((int64_t)B * k > (int64_t)1 << 30) return fail(IWAE_ERR_ARG, "grad_moments: B*k too large");
    CHK(check_objective(m, objective));
    HIPCHK(hipSetDevice(m->cfg.device));
    const size_t n = m->nparam;
    hipStream_t st = m->stream;
    iwae_model::MomWs& w = m->mom_ws;
    const float* xd;
    CHK(staged_in(m, x, m->ev.x, (size_t)B * m->X * 4, &xd));        // uploaded once: every draw reads the images in place
    CHK(ensure(w.mean, n * 8, st));
    CHK(ensure(w.m2, n * 8, st));
    for (int j = 0; j < M; ++j) {
        CHK(step_forward(m, m->cfg.precision, xd, B, k, beta, nullptr, objective, true, nullptr, FwdCall{m->batch_offset}));
        CHK(step_backward(m, objective, END_GRAD));
        m->noise_step += 1;
        CHK(join_side(m));               // the fold reads the whole gradient: behind every stream that wrote part of it
        MomentsFoldArgs a;
        a.g = m->grad; a.mean = ptr<double>(w.mean); a.m2 = ptr<double>(w.m2); a.n = n; a.j = j + 1;
        launch_moments_fold(a, st);
    }
    // var replaces M2 in the workspace unless the caller's buffer is on the device; the mean is copied only to a device buffer
    MomentsFinalizeArgs f;
    f.mean = ptr<double>(w.mean); f.m2 = ptr<double>(w.m2); f.n = n; f.M = M;
    double* mean_d;
    CHK(staged_out(m, mean, w.mean, n * 8, &mean_d));
    CHK(staged_out(m, var, w.m2, n * 8, &f.out_var));
    f.out_mean = mean_d != f.mean ? mean_d : nullptr;
    launch_moments_finalize(f, st);
    HIPCHK(hipGetLastError());
    CHK(finish_out(m, mean, mean_d, n * 8));
    CHK(finish_out(m, var, f.out_var, n * 8));
    HIPCHK(hipStreamSynchronize(st));
    return IWAE_OK;
}

int iwae_dataset_upload(iwae_handle m, const uint8_t* gray, int32_t n) {
    if (!m || !gray || n <= 0) return fail(IWAE_ERR_ARG, "dataset_upload: bad argument");
    HIPCHK(hipSetDevice(m->cfg.device));
    CHK(ensure(m->ds_data, (size_t)n * m->X, m->stream));
    CHK(ensure(m->ds_order, (size_t)n * 4, m->stream));
    HIPCHK(hipMemcpyAsync(m->ds_data.p, gray, (size_t)n * m->X, hipMemcpyDefault, m->stream));
    std::vector<int32_t> ident(n);
    for (int i = 0; i < n; ++i) ident[i] = i;
    HIPCHK(hipMemcpyAsync(m->ds_order.p, ident.data(), (size_t)n * 4, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->ds_N = n;
    m->ds_epoch = 0;
    m->ds_has_labels = false;      // (a new set: its labels, if any, follow)
    m->ds_has_mask = false;        // (... and its masks)
    return IWAE_OK;
}

int iwae_dataset_set_labels(iwae_handle m, const uint8_t* labels, int32_t n) {
    if (!m || !labels) return fail(IWAE_ERR_ARG, "dataset_set_labels: null argument");
    if (m->C <= 0) return fail(IWAE_ERR_STATE, "dataset_set_labels: the model was created with cond_dim = 0");
    if (m->ds_N <= 0) return fail(IWAE_ERR_STATE, "dataset_set_labels: no dataset uploaded");
    if (n != m->ds_N) return fail(IWAE_ERR_ARG, "dataset_set_labels: one label per image of the uploaded set");
    HIPCHK(hipSetDevice(m->cfg.device));
    if (!is_device_ptr(labels, m->cfg.device))
        for (int i = 0; i < n; ++i)
            if ((int)labels[i] >= m->C) return fail(IWAE_ERR_ARG, "dataset_set_labels: label " + std::to_string((int)labels[i]) + " at " + std::to_string(i) + " is not below cond_dim");
    CHK(ensure(m->ds_labels, (size_t)n, m->stream));
    HIPCHK(hipMemcpyAsync(m->ds_labels.p, labels, (size_t)n, hipMemcpyDefault, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->ds_has_labels = true;
    return IWAE_OK;
}

int iwae_dataset_begin_epoch(iwae_handle m, uint32_t epoch, const int32_t* order, int32_t n) {
    if (!m || m->ds_N <= 0) return fail(IWAE_ERR_STATE, "dataset_begin_epoch: no dataset uploaded");
    if (order) {
        if (n != m->ds_N) return fail(IWAE_ERR_ARG, "dataset_begin_epoch: order must have one entry per image");
        for (int i = 0; i < n; ++i)
            if (order[i] < 0 || order[i] >= m->ds_N) return fail(IWAE_ERR_ARG, "dataset_begin_epoch: index out of range");
        HIPCHK(hipMemcpyAsync(m->ds_order.p, order, (size_t)n * 4, hipMemcpyHostToDevice, m->stream));
        HIPCHK(hipStreamSynchronize(m->stream));
    }
    m->ds_epoch = epoch;
    return IWAE_OK;
}

int iwae_dataset_get_batch(iwae_handle m, int32_t start, int32_t B, float* x_out) {
    if (!m || !x_out) return fail(IWAE_ERR_ARG, "dataset_get_batch: null argument");
    if (m->ds_N <= 0) return fail(IWAE_ERR_STATE, "dataset_get_batch: no dataset uploaded");
    if (start < 0 || B <= 0 || (int64_t)start + B > (int64_t)m->ds_N) return fail(IWAE_ERR_ARG, "dataset_get_batch: bad range");
    HIPCHK(hipSetDevice(m->cfg.device));
    const int Bp = round_up(B, 128);
    CHK(ensure(m->xP, (size_t)Bp * m->Xinp * 2, m->stream));
    CHK(ensure(m->scratch, (size_t)B * m->X * 4, m->stream));
    launch_gather_binarize(ptr<uint8_t>(m->ds_data), ptr<int32_t>(m->ds_order), start, m->ds_N, B, m->X, m->Xinp, Bp, m->cfg.seed, m->ds_epoch,
                           ptr<uint16_t>(m->xP), ptr<float>(m->scratch), m->stream);
    HIPCHK(hipMemcpyAsync(x_out, m->scratch.p, (size_t)B * m->X * 4, hipMemcpyDefault, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->have_forward = false;
    return IWAE_OK;
}

int iwae_dataset_get_labels(iwae_handle m, int32_t start, int32_t B, float* y_out) {
    if (!m || !y_out) return fail(IWAE_ERR_ARG, "dataset_get_labels: null argument");
    if (m->ds_N <= 0) return fail(IWAE_ERR_STATE, "dataset_get_labels: no dataset uploaded");
    if (start < 0 || B <= 0 || (int64_t)start + B > (int64_t)m->ds_N) return fail(IWAE_ERR_ARG, "dataset_get_labels: bad range");
    if (m->C <= 0 || !m->ds_has_labels) return fail(IWAE_ERR_STATE, "dataset_get_labels: no labels (iwae_dataset_set_labels on a conditional model)");
    HIPCHK(hipSetDevice(m->cfg.device));
    CHK(join_side(m));
    const int Bp = round_up(B, 128);
    CHK(ensure(m->xP, (size_t)Bp * m->Xinp * 2, m->stream));
    CHK(ensure(m->cond, (size_t)B * m->C * 4, m->stream));
    launch_gather_binarize(ptr<uint8_t>(m->ds_data), ptr<int32_t>(m->ds_order), start, m->ds_N, B, m->X, m->Xinp, Bp, m->cfg.seed, m->ds_epoch,
                           ptr<uint16_t>(m->xP), nullptr, m->stream, ptr<uint8_t>(m->ds_labels), m->C, ptr<float>(m->cond));
    HIPCHK(hipMemcpyAsync(y_out, m->cond.p, (size_t)B * m->C * 4, hipMemcpyDefault, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->cond_n = 0;                 // (the buffer no longer holds what iwae_set_condition put there)
    m->have_forward = false;
    return IWAE_OK;
}

// The resident per-image masks: one fixed mask per image of the uploaded set, bit-packed; with one set
// iwae_train_step_dataset takes the masked step.  The 1-layer unconditional model only (a bf16 handle of a width the masked step refuses may
// hold a mask: the step refuses, options can change in between).
namespace {
int dataset_mask_scope(iwae_model* m, const char* who) {
    const std::string w(who);
    if (m->cfg.n_layers != 1 || m->C > 0 || m->has_prior) return fail(IWAE_ERR_STATE, w + ": per-image masks belong to the 1-layer unconditional model (the masked step's)");
    if (m->ds_N <= 0) return fail(IWAE_ERR_STATE, w + ": no dataset uploaded");
    return IWAE_OK;
}
}  // namespace

int iwae_dataset_set_mask(iwae_handle m, const uint8_t* mask, int32_t n) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    if (!mask) { m->ds_has_mask = false; return IWAE_OK; }
    CHK(dataset_mask_scope(m, "dataset_set_mask"));
    if (n != m->ds_N) return fail(IWAE_ERR_ARG, "dataset_set_mask: one mask row per image of the uploaded set");
    HIPCHK(hipSetDevice(m->cfg.device));
    const int W = mask_words(m->X);
    CHK(ensure(m->ds_mask, (size_t)n * W * 4, m->stream));
    if (is_device_ptr(mask, m->cfg.device)) {
        launch_mask_pack(mask, n, m->X, ptr<uint32_t>(m->ds_mask), m->stream);
        HIPCHK(hipGetLastError());
    } else {
        std::vector<uint32_t> bits((size_t)n * W, 0u);
        for (int i = 0; i < n; ++i)
            for (int f = 0; f < m->X; ++f)
                if (mask[(size_t)i * m->X + f] != 0) bits[(size_t)i * W + (f >> 5)] |= 1u << (f & 31);
        HIPCHK(hipMemcpyAsync(m->ds_mask.p, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, m->stream));
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    m->ds_has_mask = true;
    return IWAE_OK;
}

int iwae_dataset_mcar_mask(iwae_handle m, double rate, uint64_t mask_seed) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    CHK(dataset_mask_scope(m, "dataset_mcar_mask"));
    if (!(rate >= 0.0 && rate <= 1.0)) return fail(IWAE_ERR_ARG, "dataset_mcar_mask: rate must lie in [0, 1]");
    HIPCHK(hipSetDevice(m->cfg.device));
    const uint32_t thr = (uint32_t)floor(rate * 16777216.0 + 0.5);
    CHK(ensure(m->ds_mask, (size_t)m->ds_N * mask_words(m->X) * 4, m->stream));
    launch_mask_mcar(m->ds_N, m->X, thr, mask_seed, ptr<uint32_t>(m->ds_mask), m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(m->stream));
    m->ds_has_mask = true;
    return IWAE_OK;
}

int iwae_dataset_get_mask(iwae_handle m, int32_t start, int32_t B, uint8_t* mask_out) {
    if (!m || !mask_out) return fail(IWAE_ERR_ARG, "dataset_get_mask: null argument");
    if (m->ds_N <= 0) return fail(IWAE_ERR_STATE, "dataset_get_mask: no dataset uploaded");
    if (start < 0 || B <= 0 || (int64_t)start + B > (int64_t)m->ds_N) return fail(IWAE_ERR_ARG, "dataset_get_mask: bad range");
    if (!m->ds_has_mask) return fail(IWAE_ERR_STATE, "dataset_get_mask: no masks (iwae_dataset_set_mask / iwae_dataset_mcar_mask)");
    HIPCHK(hipSetDevice(m->cfg.device));
    CHK(ensure(m->scratch, (size_t)B * m->X, m->stream));
    GatherMaskedArgs g;
    memset(&g, 0, sizeof(g));
    g.data = ptr<uint8_t>(m->ds_data); g.order = ptr<int32_t>(m->ds_order); g.bits = ptr<uint32_t>(m->ds_mask);
    g.start = start; g.B = B; g.X = m->X; g.Xp = m->Xinp; g.Bp = round_up(B, 128); g.seed = m->cfg.seed; g.epoch = m->ds_epoch;
    g.mask = ptr<uint8_t>(m->scratch);      // (the mask bytes alone: no row of the step's buffers is touched)
    launch_gather_binarize_masked(g, m->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(mask_out, m->scratch.p, (size_t)B * m->X, hipMemcpyDefault, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return IWAE_OK;
}

int iwae_train_step_dataset(iwae_handle m, int32_t start, int32_t B, int32_t k, float beta, float lr, int32_t objective, iwae_scalars* scalars) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    if (m->ds_N <= 0) return fail(IWAE_ERR_STATE, "train_step_dataset: no dataset uploaded");
    if (start < 0 || B <= 0 || (int64_t)start + B > (int64_t)m->ds_N) return fail(IWAE_ERR_ARG, "train_step_dataset: batch range outside the dataset");
    HIPCHK(hipSetDevice(m->cfg.device));
    FwdCall call{m->batch_offset};
    if (m->ds_has_mask) {      // iwae_train_step_masked on (iwae_dataset_get_batch, iwae_dataset_get_mask) of these rows, fed on the device
        CHK(masked_scope(m, "train_step_dataset", nullptr, B, k, nullptr, true));
        call.mask_resident = true;
    }
    CHK(check_objective(m, objective));
    m->ds_start = start;      // (-1 outside this call: set behind the last check, reset on every path)
    const int rc = train_step_call(m, nullptr, B, k, beta, lr, objective, nullptr, scalars, nullptr, call);
    m->ds_start = -1;
    return rc;
}

int iwae_enable_timing(iwae_handle m, int32_t enable) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    HIPCHK(hipStreamSynchronize(m->stream));
    m->timing = enable > 0 ? enable : 0;
    m->timing_calls = 0;
    m->time_this = false;
    for (int i = 0; i < T_COUNT; ++i) m->ev_used[i] = 0;
    return IWAE_OK;
}

int iwae_kernel_time(iwae_handle m, const char* name, double* avg_us, int64_t* launches) {
    if (!m || !name || !avg_us) return fail(IWAE_ERR_ARG, "kernel_time: null argument");
    int id = -1;
    for (int i = 0; i < T_COUNT; ++i)
        if (!strcmp(name, kTimedNames[i])) id = i;
    if (!strcmp(name, "bernoulli_fwd")) id = T_DEC_FWD;      // round-1 name of the decoder forward kernel
    if (id < 0) {
        std::string all;
        for (int i = 0; i < T_COUNT; ++i) all += std::string(i ? " | " : "") + kTimedNames[i];
        return fail(IWAE_ERR_ARG, "kernel_time: unknown kernel (" + all + ")");
    }
    CHK(join_side(m));
    HIPCHK(hipStreamSynchronize(m->stream));
    if (m->side) HIPCHK(hipStreamSynchronize(m->side));      // the weight gradients are timed on the side streams
    if (m->side2) HIPCHK(hipStreamSynchronize(m->side2));
    double tot = 0.0;
    for (size_t i = 0; i < m->ev_used[id]; ++i) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, m->ev_start[id][i], m->ev_stop[id][i]));
        tot += ms;
    }
    *avg_us = m->ev_used[id] ? tot * 1e3 / (double)m->ev_used[id] : 0.0;
    if (launches) *launches = (int64_t)m->ev_used[id];
    return IWAE_OK;
}

int iwae_debug_eps(iwae_handle m, int32_t B, int32_t k, int32_t layer, float* out) {
    if (!m || !out || B <= 0 || k <= 0 || layer < 0 || layer >= m->cfg.n_layers) return fail(IWAE_ERR_ARG, "debug_eps: bad argument");
    HIPCHK(hipSetDevice(m->cfg.device));
    const int D = m->D[layer];
    CHK(ensure(m->scratch, (size_t)B * k * D * 4, m->stream));
    EpsSrc e;
    e.user = nullptr; e.B = B; e.seed = m->cfg.seed; e.row_offset = (uint64_t)m->batch_offset * k; e.step = m->noise_step; e.stream = layer;
    launch_eps_dump(e, B, k, D, ptr<float>(m->scratch), m->stream);
    HIPCHK(hipMemcpyAsync(out, m->scratch.p, (size_t)B * k * D * 4, hipMemcpyDefault, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return IWAE_OK;
}

int iwae_debug_tensor(iwae_handle m, const char* name, float* out, size_t cap, int32_t* rows, int32_t* cols) {
    if (!m || !name) return fail(IWAE_ERR_ARG, "debug_tensor: null argument");
    if (!m->have_forward) return fail(IWAE_ERR_STATE, "debug_tensor: no forward pass yet");
    HIPCHK(hipSetDevice(m->cfg.device));
    CHK(join_side(m));
    struct Ent { const char* nm; int kind; const DevBuf* buf; int R; int F; int Fp; };   // kind 0: bf16 P-layout, 2: fp32
    const int B = m->B, M = m->M, Mp = m->Mp;
    const int H0 = m->H[0], Hp0 = m->Hp[0], D0 = m->D[0], Dp0 = m->Dp[0];
    std::vector<Ent> ents = {
        {"x", 0, &m->xP, B, m->X, m->Xinp},
        {"enc.h1", 0, &m->wenc1.h1P, B, H0, Hp0},
        {"enc.h2", 0, &m->wenc1.h2P, B, H0, Hp0},
        {"enc.head", 2, &m->wenc1.head, B, 2 * Dp0, 2 * Dp0},
        {"enc.dhead", 0, &m->wenc1.dheadP, B, 2 * Dp0, 2 * Dp0},
        {"enc.d2", 0, &m->wenc1.d2P, B, H0, Hp0}, {"enc.d1", 0, &m->wenc1.d1P, B, H0, Hp0},
        {"z", 0, &m->zP[0], M, D0, Dp0},
        {"dec.g1", 0, &m->wdec1.g1P, M, H0, Hp0},
        {"dec.g2", 0, &m->wdec1.g2P, M, H0, Hp0},
        {"dec.dl", 0, &m->wdec1.dlP, M, m->X, m->Xp32},
        {"dec.d2", 0, &m->wdec1.d2P, M, H0, Hp0},
        {"dec.d1", 0, &m->wdec1.d1P, M, H0, Hp0},
        {"dec.dz", 2, &m->wdec1.dz, M, Dp0, Dp0},
        {"gx", 2, &m->gx, M, 1, 1}, {"wn", 2, &m->wn, M, 1, 1}, {"log_w", 2, &m->logw, M, 1, 1},
    };
    if (m->cfg.n_layers == 2) {
        const int H1 = m->H[1], Hp1 = m->Hp[1], D1 = m->D[1], Dp1 = m->Dp[1];
        std::vector<Ent> e2 = {
            {"enc2.h1", 0, &m->wenc2.h1P, M, H1, Hp1}, {"enc2.h2", 0, &m->wenc2.h2P, M, H1, Hp1},
            {"enc2.head", 2, &m->wenc2.head, M, 2 * Dp1, 2 * Dp1}, {"enc2.dhead", 0, &m->wenc2.dheadP, M, 2 * Dp1, 2 * Dp1},
            {"enc2.dx", 2, &m->wenc2.dx, M, Dp0, Dp0},
            {"z2", 0, &m->zP[1], M, D1, Dp1},
            {"dec2.h1", 0, &m->wdec2.h1P, M, H1, Hp1}, {"dec2.h2", 0, &m->wdec2.h2P, M, H1, Hp1},
            {"dec2.head", 2, &m->wdec2.head, M, 2 * Dp0, 2 * Dp0}, {"dec2.dhead", 0, &m->wdec2.dheadP, M, 2 * Dp0, 2 * Dp0},
            {"dec2.dx", 2, &m->wdec2.dx, M, Dp1, Dp1},
            {"dz1_direct", 2, &m->dzdir, M, Dp0, Dp0},
        };
        ents.insert(ents.end(), e2.begin(), e2.end());
    }
    if (strcmp(name, "dense_stamps") == 0) {   // diagnostic: [waves][8] phase cycle sums of the selected dense launch
        if (rows) *rows = m->dstamp_waves;
        if (cols) *cols = 8;
        if (!out) return IWAE_OK;
        if (!m->dstamps.p) return fail(IWAE_ERR_STATE, "dense stamps not enabled (STAMPS=1 build + options dense_stamps_epi / dense_stamps_kt)");
        std::vector<unsigned long long> h((size_t)m->dstamp_waves * 8);
        HIPCHK(hipStreamSynchronize(m->stream));
        HIPCHK(hipMemcpy(h.data(), m->dstamps.p, h.size() * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < h.size(); ++i) out[i] = (float)h[i];
        return IWAE_OK;
    }
    if (strcmp(name, "stamps") == 0) {   // diagnostic: [waves][8] phase cycle sums of out_bwd, as float
        const int nw = (Mp / 64) * 4;
        if (rows) *rows = nw;
        if (cols) *cols = 8;
        if (!out) return IWAE_OK;
        if (!m->stamps.p) return fail(IWAE_ERR_STATE, "stamps not enabled (DIAG=1 build + option stamps)");
        std::vector<unsigned long long> h((size_t)nw * 8);
        HIPCHK(hipStreamSynchronize(m->stream));
        HIPCHK(hipMemcpy(h.data(), m->stamps.p, h.size() * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < h.size(); ++i) out[i] = (float)h[i];
        return IWAE_OK;
    }
    for (const Ent& e : ents) {
        if (strcmp(e.nm, name) != 0) continue;
        if (rows) *rows = e.R;
        if (cols) *cols = e.F;
        if (!out) return IWAE_OK;
        if (!e.buf->p) return fail(IWAE_ERR_STATE, std::string("debug_tensor: buffer not populated: ") + name);
        const size_t n = (size_t)e.R * e.F;
        if (cap < n) return fail(IWAE_ERR_ARG, "debug_tensor: output too small");
        if (e.kind == 2) {
            HIPCHK(hipMemcpyAsync(out, e.buf->p, n * 4, hipMemcpyDefault, m->stream));
        } else {
            CHK(ensure(m->scratch, n * 4, m->stream));
            launch_unpack_p(ptr<uint16_t>(*e.buf), e.R, e.F, e.Fp, ptr<float>(m->scratch), m->stream);
            HIPCHK(hipMemcpyAsync(out, m->scratch.p, n * 4, hipMemcpyDefault, m->stream));
        }
        HIPCHK(hipStreamSynchronize(m->stream));
        return IWAE_OK;
    }
    return fail(IWAE_ERR_ARG, std::string("debug_tensor: unknown name ") + name);
}

}  // extern "C"
