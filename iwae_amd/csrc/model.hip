// Host side of libiwae_amd.so: device memory, launch sequencing and the C ABI of include/iwae_amd.h.
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

namespace {      // (closed and reopened around each helper that model.h declares for step_f32.hip; what is added in between stays internal)

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

// table order enc1 | enc2 | dec2 | dec1 [| prior]: are the decoder's three layers (one table entry each) the tail of the table / does the
// 2-layer model's share of it start with the per-sample encoder?  (plan_step_end asks: only then do TableBounds::dec1 / enc2 open a side stream's range)
bool dec_layers_last(const iwae_model* m) {
    const int d0 = m->dec1[0].sub[0];
    return m->dec1[0].nsub == 1 && m->dec1[1].nsub == 1 && m->dec1[2].nsub == 1 && m->dec1[1].sub[0] == d0 + 1 && m->dec1[2].sub[0] == d0 + 2 && d0 + 3 == (int)m->klayers.size();
}
bool side_layers_from_enc2(const iwae_model* m) { return m->cfg.n_layers == 2 && m->enc2[0].nsub >= 1; }

}  // namespace -- build_descs: external (hidden) linkage, declared in model.h, step_f32.hip calls it too
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
namespace {      // (internal linkage again)

// The two kernels that walk the layer table, with the handle's constants filled in.
// reduce_blocks: the slabs of reduce blocks a (and b, same launch) summed into the flat gradient on st; update: Adam (alpha) + the weight-image
// refresh in the epilogue; done: its completion event, riding on the dispatch packet; with_means: one extra block makes the step's batch means
void reduce_blocks(iwae_model* m, hipStream_t st, BlockRange a, BlockRange b, float alpha, bool update, hipEvent_t done, bool with_means) {
    const float* per_b = with_means ? ptr<float>(m->per_b) : nullptr;
    launch_reduce_grads(m->d_descs, (int)m->descs.size(), a.first, a.count, m->grad, m->param, m->mom, m->vel, alpha, m->adam_b1, m->adam_b2, m->adam_eps, update ? 1 : 0,
                        per_b, per_b ? m->B : 0, !per_b ? 0.f : m->cfg.n_layers == 2 ? 1.f : m->beta, per_b ? m->d_scalars : nullptr, st, b.first, b.count, done);
}
}  // namespace -- adam_blocks: external (hidden) linkage, declared in model.h, step_f32.hip calls it too
// adam_blocks: Adam on elementwise blocks [first, first + count) of the flat gradient times grad_scale; done as above (update = false: the weight images only)
void adam_blocks(iwae_model* m, hipStream_t st, int first, int count, float alpha, float grad_scale, hipEvent_t done, bool update) {
    launch_adam(m->d_descs, (int)m->descs.size(), count, m->param, m->grad, m->mom, m->vel, alpha, grad_scale, m->adam_b1, m->adam_b2, m->adam_eps, update ? 1 : 0, st, first, done);
}
namespace {      // (internal linkage again)

int refresh_images(iwae_model* m) {   // rebuild bf16 A-images from the fp32 master weights
    if (m->descs_dirty) CHK(build_descs(m));
    adam_blocks(m, m->stream, 0, m->tb.end.e, 0.f, 1.f, nullptr, false);
    HIPCHK(hipGetLastError());
    return IWAE_OK;
}

// row stride of the cached draws: the latent width rounded to 4, NOT the 32-padded operand width -- D = 100: 400 B instead of 512 B per row,
// 5.7 MB less per pass over the k = 50, B = 1 024 step's draws (written once, read by the decoder kernel and by latent_bwd_kernel)
static inline int eps_ld(const iwae_model* m, int layer) { return 4 * ((m->D[layer] + 3) / 4); }
}  // namespace -- eps_src: external (hidden) linkage, declared in model.h, step_f32.hip calls it too
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
namespace {      // (internal linkage again)

// diagnostic (STAMPS=1 build + options dense_stamps_epi / dense_stamps_kt): record the phase stamps of the matching dense launch
int attach_dense_stamps(iwae_model* m, int epi, DenseArgs& a) {
    if (m->dstamp_epi != epi || m->dstamp_kt != a.KT || (a.M < 4096 && a.KT <= 8)) return IWAE_OK;
    m->dstamp_waves = std::max(((a.M + 127) / 128) * ((a.MG + a.mg_per_block - 1) / a.mg_per_block) * 4, epi == EPI_BERN ? ((a.M + 127) / 128) * 16 : 0);      // (bern_pipe_kernel: <= 16 waves per 128+ rows)
    CHK(ensure(m->dstamps, (size_t)m->dstamp_waves * 64, m->stream));
    a.stamps = ptr<unsigned long long>(m->dstamps);
    return IWAE_OK;
}

// ---------------------------------------------------------------- forward pieces
// Does block_fwd_kernel take the whole block on R rows (few rows: the encoder on the batch's images)?  Fills the shape half of its argument block.
bool block_fwd_shape(const iwae_model* m, const Linear* blk, int R, BlockFwdArgs& a) {
    memset(&a, 0, sizeof(a));
    a.ldX = blk[0].Kp32; a.img0 = blk[0].imgF; a.img1 = blk[1].imgF; a.img2 = blk[2].imgF;
    a.KT0 = blk[0].KT; a.KT1 = blk[1].KT; a.NT1 = blk[0].Np32 / 16; a.NT2 = blk[2].Np32 / 16; a.R = R;
    a.ldH = blk[0].Np32; a.ldYF = blk[2].Np32; a.split = (blk[2].nsub == 2) ? blk[2].joff[1] : (1 << 30);
    return m->opt.allow_block_fused && blk[1].Np32 == blk[0].Np32 && blk[2].KT == blk[1].KT && blk[1].Kp32 == blk[0].Np32 && block_fwd_ok(a);
}

// ---------------------------------------------------------------- backward pieces
// weight gradient from the P-layout operands (wgradp_kernel); XP/GP row-major bf16, `rows` valid rows.
// wgradp_plan sizes the row splits and the slabs and fills the argument block; nw = the kernel shape (launch_wgradp:
// 8 = small, 16 = 16 waves, 7 = 8 waves with 7 x 4 accumulator tiles each, for inputs <= 224 features wide).
// the shape part: the kernel shape, the row splits and the 64-row chunks per split (no allocation: plan_step asks for the shape alone)
void wgradp_shape(const iwae_model* m, const Linear& L, int rows, int& nsplit, int& nw, int& cps) {
    const int chunks = (rows + 63) / 64;
    nw = (L.JT > 8 && chunks >= 128) ? 16 : 8;
    if (nw == 16 && L.IT <= 14 && m->opt.allow_wg7) nw = (m->opt.wg_shape9 & (L.JT > 16 ? 1 : 2)) ? 9 : 7;      // option wg9: bit 0 the output layer, bit 1 the hidden layers
    const int blocks = ((L.JT + wgradp_strip(nw) - 1) / wgradp_strip(nw)) * ((L.IT + 15) / 16);
    // Workgroup targets (measured at k=50, B=1024).  Early builds, the weight gradients alone on the machine: 64 -> 0.501,
    // 128 -> 0.425, 256 -> 0.406, 384 -> 0.443 ms/step (fewer leaves CUs idle, more pays a full fp32 slab per extra split).
    // Since they run beside the dX chain and with the register-blocked kernel: 160 (see wg_target16); the
    // single-block-wide hidden layers prefer 128.
    // (round 5: the 2-layer step's MAIN stream is its long chain and its side streams have slack: 64 workgroups for the output layer's gradient leave the
    // main chain's kernels more CUs -- 128 / 96 / 72 / 64 / 56 / 48 -> 0.3915 / 0.3834 / 0.3896 / 0.3769 / 0.3805 / 0.3852 ms, interleaved)
    const int target16 = m->opt.wg_target16 > 0 ? m->opt.wg_target16 : (m->cfg.n_layers == 2 ? 64 : 96);
    const int target = (nw != 8) ? (blocks == 1 ? m->opt.wg_target16_1 : target16) : (chunks < 128 ? m->opt.wg_target8_few : m->opt.wg_target8);
    nsplit = std::max(1, std::min(chunks, target / std::max(1, blocks)));
    cps = (chunks + nsplit - 1) / nsplit;
    nsplit = (chunks + cps - 1) / cps;
}
int wgradp_plan(iwae_model* m, Linear& L, const uint16_t* XP, const uint16_t* GP, int rows, WgradPArgs& a, int& nsplit, int& nw) {
    int cps;
    wgradp_shape(m, L, rows, nsplit, nw, cps);
    const size_t needW = (size_t)nsplit * L.IT * 16 * L.JT * 16 * 4, needB = (size_t)nsplit * L.JT * 16 * 4;
    void* oldW = L.slabW.p; void* oldB = L.slabB.p;
    CHK(ensure(L.slabW, needW, m->stream));
    CHK(ensure(L.slabB, needB, m->stream));
    if (oldW != L.slabW.p || oldB != L.slabB.p || nsplit != L.nsplit) { L.nsplit = nsplit; m->descs_dirty = true; }
    a.X = XP; a.ldX = L.Kp32; a.IT = L.IT; a.G = GP; a.ldG = L.Np32; a.JT = L.JT; a.M = rows; a.rows_per_split = cps * 64;
    a.slabW = ptr<float>(L.slabW); a.slabB = ptr<float>(L.slabB); a.zero = m->d_zero; a.rowscale = nullptr;
    a.dbg = m->wg_debug;
    a.stamps = nullptr;
    return IWAE_OK;
}

int wgradp(iwae_model* m, Linear& L, const uint16_t* XP, const uint16_t* GP, int rows, hipStream_t st = nullptr,
           const float* rowscale = nullptr, hipEvent_t done = nullptr) {
    WgradPArgs a;
    int nsplit = 1, nw = 8;
    CHK(wgradp_plan(m, L, XP, GP, rows, a, nsplit, nw));
    a.rowscale = rowscale;
    if (rowscale && (m->fake_s & 2)) a.dbg |= 32;
#ifdef IWAE_DENSE_STAMPS
    if (m->dstamp_epi == 10 && rowscale && nw == 7) {      // diagnostic (STAMPS=1 build, option dense_stamps_epi = 10): phase stamps of the output layer's weight gradient
        m->dstamp_waves = ((L.JT + 15) / 16) * nsplit * 12;
        CHK(ensure(m->dstamps, (size_t)m->dstamp_waves * 64, m->stream));
        a.stamps = ptr<unsigned long long>(m->dstamps);
    }
#endif
    launch_wgradp(a, nsplit, nw, st ? st : m->stream, done);
    HIPCHK(hipGetLastError());
    return IWAE_OK;
}

// dX (times tanh' of the stored activation, or raw fp32) of a layer: X = dpre of the layer's outputs
// The output layer's gradient in two launches over disjoint row ranges (option wout_split): slabs [0, n1) come from rows [0, R1), slabs
// [n1, n1 + n2) from the rest -- the reduction sums them in that fixed order whichever launch ends first.
int wgradp_two_plan(iwae_model* m, Linear& L, const uint16_t* XP, const uint16_t* GP, int rows, const float* rowscale, WgradPArgs& a1, int& n1, WgradPArgs& a2, int& n2) {
    const int blocks = (L.JT + 15) / 16;
    const int chunks = (rows + 63) / 64;
    const int c1 = std::min(chunks - 1, std::max(1, (int)((long)chunks * m->opt.wout_split / 100)));
    const int c2 = chunks - c1;
    auto split = [&](int ch, int target, int& n, int& cps) { n = std::max(1, std::min(ch, target / std::max(1, blocks))); cps = (ch + n - 1) / n; n = (ch + cps - 1) / cps; };
    int cps1, cps2;
    split(c1, m->opt.wout_wg1, n1, cps1);
    split(c2, m->opt.wout_wg2, n2, cps2);
    const int ns = n1 + n2;
    const size_t stride = (size_t)L.IT * 16 * L.JT * 16;
    void* oldW = L.slabW.p; void* oldB = L.slabB.p;
    CHK(ensure(L.slabW, (size_t)ns * stride * 4, m->stream));
    CHK(ensure(L.slabB, (size_t)ns * L.JT * 16 * 4, m->stream));
    if (oldW != L.slabW.p || oldB != L.slabB.p || ns != L.nsplit) { L.nsplit = ns; m->descs_dirty = true; }
    const int R1 = c1 * 64;
    memset(&a1, 0, sizeof(a1));
    a1.X = XP; a1.ldX = L.Kp32; a1.IT = L.IT; a1.G = GP; a1.ldG = L.Np32; a1.JT = L.JT; a1.M = R1; a1.rows_per_split = cps1 * 64;
    a1.slabW = ptr<float>(L.slabW); a1.slabB = ptr<float>(L.slabB); a1.zero = m->d_zero; a1.rowscale = rowscale;
    a2 = a1;
    a2.X = XP + (size_t)R1 * L.Kp32; a2.G = GP + (size_t)R1 * L.Np32; a2.M = rows - R1; a2.rows_per_split = cps2 * 64;
    a2.slabW = a1.slabW + (size_t)n1 * stride; a2.slabB = a1.slabB + (size_t)n1 * L.JT * 16; a2.rowscale = rowscale + R1;
    return IWAE_OK;
}

int dense_dx(iwae_model* m, Linear& L, const uint16_t* GP, int rows, const uint16_t* ACT, uint16_t* YP, float* YF, hipEvent_t done = nullptr) {
    DenseArgs a;
    memset(&a, 0, sizeof(a));
    a.X = GP; a.ldX = L.Np32; a.img = L.imgB;
    a.split = 1 << 30;
    a.M = rows; a.KT = L.KT_B; a.MG = L.MG_B; a.mg_per_block = (rows <= 8192) ? 1 : L.MG_B; a.Np32 = L.Kp32; a.g1_mask = m->opt.dense_g1_mask;
    a.YP = YP; a.ldYP = L.Kp32; a.YF = YF; a.ldYF = L.Kp32;
    a.ACT = ACT; a.ldACT = L.Kp32;
    CHK(attach_dense_stamps(m, ACT ? EPI_DX : EPI_F32, a));
    launch_dense(ACT ? EPI_DX : EPI_F32, a, m->stream, done);
    HIPCHK(hipGetLastError());
    return IWAE_OK;
}

// backward of one BasicBlock over R rows: the dX chain first, then the three weight gradients -- they only feed the
// slab reduction, so for small R (latency-bound 8-wave kernels) they go out as ONE grouped launch
// dx_done: the dX chain (dhead -> d2 -> d1 -> dx) has been computed already (gblock_bwd_kernel): only the weight gradients are left
// Does block_bwd_kernel take both dX products of the block on R rows?  Fills the shape half of its argument block.
bool block_bwd_shape(const iwae_model* m, const Linear* blk, int R, BlockBwdArgs& b) {
    memset(&b, 0, sizeof(b));
    b.ldDH = blk[2].Np32; b.imgH = blk[2].imgB; b.imgL2 = blk[1].imgB;
    b.KTH = blk[2].KT_B; b.KT1 = blk[1].KT_B; b.NT1 = blk[0].Np32 / 16; b.R = R; b.ldH = blk[0].Np32;
    return m->opt.allow_block_fused && !blk[2].kmajor && !blk[1].kmajor && blk[1].Np32 == blk[0].Np32 && blk[1].Kp32 == blk[0].Np32 && blk[2].Kp32 == blk[0].Np32 && block_bwd_ok(b);
}
// ... and can that launch make the head's gradient rows of a latent Dp wide itself (no conditional prior, bf16 rows)?
bool lat_in_block_ok(const Linear* blk, int Dp, bool prior, bool f32_rows) { return Dp <= 128 && Dp == blk[2].Np32 / 2 && !prior && !f32_rows; }
// lat != null: the block's dhead rows are made inside block_bwd_kernel (latent_bwd_kernel's sums, a wave per image) -- only where
// block_bwd_shape and lat_in_block_ok say so (StepPlan::lat_fuse); elsewhere the caller launches latent_bwd_kernel first
int block_bwd(iwae_model* m, Linear* blk, BlockWs& w, const uint16_t* inP, int R, bool need_dx, bool wgrad_on_side, bool dx_done = false, hipStream_t side_st = nullptr,
              bool skip_wgrad = false, const LatentBwdArgs* lat = nullptr) {
    bool chain_fused = dx_done;
    if (dx_done) need_dx = false;
    BlockBwdArgs b;
    if (!dx_done && block_bwd_shape(m, blk, R, b)) {      // few rows (the encoder on the batch's images): both dX products in one launch
        b.DH = ptr<uint16_t>(w.dheadP); b.H2 = ptr<uint16_t>(w.h2P); b.H1 = ptr<uint16_t>(w.h1P);
        b.D2 = ptr<uint16_t>(w.d2P); b.D1 = ptr<uint16_t>(w.d1P);
        if (lat) {
            if (!lat_in_block_ok(blk, lat->Dp, lat->prior_head != nullptr, lat->DHF != nullptr)) return fail(IWAE_ERR_STATE, "block_bwd: latent sums on a shape block_bwd_kernel does not cover");
            b.lat_on = 1; b.lat = *lat;
            b.rows_per_wg = lat->k > 16 ? 4 : 16;      // (many samples per image: four waves per image, 4 images per workgroup -- block_bwd_kernel<4>)
        }
        launch_block_bwd(b, m->stream); chain_fused = true;
    } else if (lat) return fail(IWAE_ERR_STATE, "block_bwd: latent sums on a shape block_bwd_kernel does not cover");
    if (!chain_fused) {
        CHK(dense_dx(m, blk[2], ptr<uint16_t>(w.dheadP), R, ptr<uint16_t>(w.h2P), ptr<uint16_t>(w.d2P), nullptr));
        CHK(dense_dx(m, blk[1], ptr<uint16_t>(w.d2P), R, ptr<uint16_t>(w.h1P), ptr<uint16_t>(w.d1P), nullptr));
    }
    if (need_dx) CHK(dense_dx(m, blk[0], ptr<uint16_t>(w.d1P), R, nullptr, nullptr, ptr<float>(w.dx)));
    if (skip_wgrad) { HIPCHK(hipGetLastError()); return IWAE_OK; }      // (the caller takes the weight gradients: block_wgrad_rows)
    const uint16_t* xs[3] = {ptr<uint16_t>(w.h2P), ptr<uint16_t>(w.h1P), inP};
    const uint16_t* gs[3] = {ptr<uint16_t>(w.dheadP), ptr<uint16_t>(w.d2P), ptr<uint16_t>(w.d1P)};
    Linear* ls[3] = {&blk[2], &blk[1], &blk[0]};
    // The weight gradients only feed the slab reduction.  For the per-sample blocks of the 2-layer model (R = B*k rows)
    // they go to the side stream, ordered behind this block's dX chain, so the main stream's dependency chain does not
    // wait for them; the small encoder block (R = B) stays on the main stream (it is the tail of the step anyway).
    hipStream_t ws = m->stream;
    if (wgrad_on_side) {
        ws = side_st ? side_st : m->side;
        if (!dx_done) HIPCHK(hipEventRecord(m->ev_blk, m->stream));      // (dx_done: the event rode on gblock_bwd_kernel's dispatch packet)
        HIPCHK(hipStreamWaitEvent(ws, m->ev_blk, 0));
    }
    WgradPGroup g;
    memset(&g, 0, sizeof(g));
    int nsplit[3], nw[3];
    bool small = true;
    for (int i = 0; i < 3; ++i) {
        CHK(wgradp_plan(m, *ls[i], xs[i], gs[i], R, g.a[i], nsplit[i], nw[i]));
        small = small && nw[i] == 8;
    }
    if (small) {
        g.n = 3;
        for (int i = 0; i < 3; ++i) {
            g.gx[i] = (ls[i]->JT + 7) / 8; g.gy[i] = (ls[i]->IT + 15) / 16;
            g.zbeg[i + 1] = g.zbeg[i] + nsplit[i];
        }
        launch_wgradp_group(g, ws);
    } else {
        for (int i = 0; i < 3; ++i) launch_wgradp(g.a[i], nsplit[i], nw[i], ws);
    }
    HIPCHK(hipGetLastError());
    return IWAE_OK;
}

// Few rows (the image encoder: R = batch size): the block's three weight gradients with the whole row reduction inside each workgroup and
// (fuse) the Adam update in the epilogue -- one launch instead of the grouped weight gradient + slabs + reduce_grads_kernel (round 4).
// with_means: one extra block turns the step's per-image values into its batch means (what reduce_grads_kernel's extra block did).
bool wgrad_rows_ok(const iwae_model* m, const Linear* blk, int R) {
    return m->opt.allow_wgrad_rows && R <= 2048 && blk[0].nsub == 1 && blk[1].nsub == 1 && blk[2].nsub <= 2 && !blk[0].kmajor && !blk[1].kmajor && !blk[2].kmajor;      // (its epilogue writes MG-major images)
}
// Few DATA rows too (M = B * k <= 2 048: the reference's default regime, B = 20): the decoder's three weight gradients join the encoder's in the
// SAME launch (six jobs; the output layer's G = the stored s takes its row weights on the way in) -- no side-stream launches, no slabs, no
// deferred reduction, no cross-stream events in the whole backward pass.  1-layer model only (the 2-layer model's per-sample blocks keep their path).
bool dec_rows_step(const iwae_model* m, int M, int B) {
    return m->opt.allow_dec_rows && m->cfg.n_layers == 1 && M <= 2048 && wgrad_rows_ok(m, m->enc1, B) && m->dec1[0].nsub == 1 && m->dec1[1].nsub == 1 &&
           m->dec1[2].nsub == 1 && !m->dec1[0].kmajor && !m->dec1[1].kmajor;
}
int block_wgrad_rows(iwae_model* m, Linear* blk, BlockWs& w, const uint16_t* inP, int R, float alpha, bool fuse, bool with_means, bool with_decoder = false) {
    if (m->descs_dirty) CHK(build_descs(m));
    const uint16_t* xs[6] = {ptr<uint16_t>(w.h2P), ptr<uint16_t>(w.h1P), inP, ptr<uint16_t>(m->wdec1.g2P), ptr<uint16_t>(m->wdec1.g1P), ptr<uint16_t>(m->zP[0])};
    const uint16_t* gs[6] = {ptr<uint16_t>(w.dheadP), ptr<uint16_t>(w.d2P), ptr<uint16_t>(w.d1P), ptr<uint16_t>(m->wdec1.dlP), ptr<uint16_t>(m->wdec1.d2P), ptr<uint16_t>(m->wdec1.d1P)};
    Linear* ls[6] = {&blk[2], &blk[1], &blk[0], &m->dec1[2], &m->dec1[1], &m->dec1[0]};
    const int njobs = with_decoder ? 6 : 3;
    WgradRowsJob jobs[6];
    memset(jobs, 0, sizeof(jobs));
    for (int i = 0; i < njobs; ++i) {
        jobs[i].X = xs[i]; jobs[i].ldX = ls[i]->Kp32; jobs[i].G = gs[i]; jobs[i].ldG = ls[i]->Np32; jobs[i].R = i < 3 ? R : m->M;
        jobs[i].sub0 = ls[i]->sub[0];
        jobs[i].sub1 = ls[i]->nsub == 2 ? ls[i]->sub[1] : -1;
        jobs[i].split = ls[i]->nsub == 2 ? ls[i]->joff[1] : (1 << 30);
    }
    if (with_decoder && m->plan.s_mode) jobs[3].rowscale = ptr<float>(m->gx);      // the forward pass kept s: dl = g_r s is made on the way in (else dlP already holds dl)
    const bool two = m->cfg.n_layers == 2;
    launch_wgrad_rows(jobs, njobs, m->d_descs, m->grad, m->param, m->mom, m->vel, alpha, m->adam_b1, m->adam_b2, m->adam_eps, fuse ? 1 : 0,
                      with_means ? ptr<float>(m->per_b) : nullptr, m->B, two ? 1.f : m->beta, m->d_scalars, m->d_zero, m->stream);
    HIPCHK(hipGetLastError());
    return IWAE_OK;
}

// ---------------------------------------------------------------- the forward pass
}  // namespace -- draw_eps: external (hidden) linkage, declared in model.h, step_f32.hip calls it too
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
namespace {      // (internal linkage again)

#define EPSM_STEPS 8
// few rows: draws of steps [step0, step0 + EPSM_STEPS) into multi-step buffer `buf` (stream order on gs protects the buffer: see iwae_model::epsm)
int draw_eps_multi(iwae_model* m, int buf, uint32_t step0, int M, hipStream_t gs) {
    const int Mp = round_up(M, 128);
    iwae_model::EpsMTag& tg = m->epsm_tag[buf];
    tg.valid = false;
    for (int l = 0; l < m->cfg.n_layers; ++l) {
        const size_t stride = (size_t)Mp * eps_ld(m, l);
        CHK(ensure(m->epsm[buf][l], (size_t)EPSM_STEPS * stride * 4, m->stream));
        EpsSrc e = eps_src(m, l);
        e.user = nullptr; e.cache = nullptr; e.step = step0;
        launch_eps_gen_multi(e, M, m->D[l], eps_ld(m, l), ptr<float>(m->epsm[buf][l]), EPSM_STEPS, stride, gs);
    }
    HIPCHK(hipGetLastError());
    tg.valid = true; tg.step0 = step0; tg.row_offset = (uint64_t)m->call.batch_offset * (uint64_t)m->k; tg.M = M;
    return IWAE_OK;
}
// the multi-step buffer that holds the draws of `step` for this batch shape, or -1
int epsm_find(const iwae_model* m, uint32_t step, int M) {
    const uint64_t ro = (uint64_t)m->call.batch_offset * (uint64_t)m->k;
    for (int i = 0; i < 2; ++i) {
        const iwae_model::EpsMTag& t = m->epsm_tag[i];
        if (t.valid && t.M == M && t.row_offset == ro && step - t.step0 < (uint32_t)EPSM_STEPS) return i;      // (unsigned: step >= step0)
    }
    return -1;
}

inline hipStream_t on_stream(const iwae_model* m, OnStream s) { return s == ON_SIDE2 ? m->side2 : s == ON_SIDE ? m->side : m->stream; }

// ---------------------------------------------------------------- the step's plan
// Which kernels a bf16 call launches and on which streams, decided once from the options, the layer tables and the call's shape.  A pure host
// function: it touches no buffer, stream or event, and forward_impl calls it before it launches or allocates anything.  Every shape predicate
// is asked here, on the shape half of the launch's own argument block; the launch code adds the buffers and asks nothing again.
StepPlan plan_step(const iwae_model* m, int B, int k, int objective, bool bwd, const FwdCall& call, const iwae_tensors* want, bool host_eps) {
    const StepOptions& o = m->opt;
    StepPlan p = StepPlan();
    const bool two = m->cfg.n_layers == 2;
    const int M = B * k, Mp = round_up(M, 128), X = m->X, Xp = m->Xp32;
    const Linear* d1 = m->dec1;
    const Linear& L = m->dec1[2];
    // A masked call (a mask is staged, the caller's or the resident set's: FwdCall::masked(), DESIGN.md sections 20, 21) takes the plan of the options no_bern_pipe + no_out_in_block: the output
    // layer stays a dense_kernel<EPI_BERN> launch, the one kernel whose epilogue knows the hole code -- never bern_pipe_kernel (so no DEC_PIPE,
    // lse_fused, g2w, Z_DEC_PROLOGUE), never block_fwd_kernel<.., OUT> (DEC_BLOCK_OUT).  Everything else follows from the predicates below.
    p.holes = call.masked();
    const bool allow_bern_pipe = o.allow_bern_pipe && !p.holes, allow_out_in_block = o.allow_out_in_block && !p.holes;
    BlockFwdArgs bf;
    p.enc_takes_f32 = m->C == 0 && block_fwd_shape(m, m->enc1, B, bf);
    p.dec_rows = bwd && dec_rows_step(m, M, B);
    p.want_dreg = !two && (objective == OBJ_DREG || (!bwd && !call.log_w_only));    // tasks/task02.py:63-65
    // ---- the step's N(0,1) draws
    // (round 4: a forward-only call on many rows -- the k = 5000 evaluator on bf16 operands -- also takes its draws from eps_gen_kernel, so that the
    // decoder kernel makes z itself in its prologue instead of sample_kernel drawing inline and writing z out: option zin_eval, off by default -- measured slower)
    p.zin_eval = !bwd && !two && m->C == 0 && o.allow_zin && o.allow_zin_eval && (int64_t)B * k >= 8192 && o.allow_dec_fused && allow_bern_pipe;
    p.keep_eps = !host_eps && (bwd || two || p.zin_eval);
    // few data rows, training step, single-stream backward (dec_rows_step): the draws come from the multi-step buffers (one launch per EPSM_STEPS steps)
    p.eps_multi = p.keep_eps && bwd && !two && o.allow_eps_multi && call.k_total == 0 && p.dec_rows;
    // ---- who would make z
    // 1-layer training step on the device's own noise: the first decoder layer makes z itself (dense_kernel ZIN mode, or the decoder kernel's prologue,
    // which also sums the DReG step's second log q)
    const bool fuse_z = o.allow_zin && !two && m->C == 0 && (bwd || p.zin_eval) && p.keep_eps && M >= 8192 && (d1[0].KT == 4 || d1[0].KT == 2) && d1[0].Kp32 == m->Dp[0];
    // few rows: block_fwd_kernel (the decoder's two tanh layers in one launch) makes z itself -- one latency-bound launch less
    const bool sample_in_block = o.allow_block_fused && o.allow_zin && !two && !fuse_z && M <= 4096 && d1[0].Kp32 == m->Dp[0];
    // 2-layer model at large row counts, the reference's dims: chain2_fwd_kernel makes z1 itself, as its first layer's operand
    if (two) {
        const Linear *e2 = m->enc2, *d2 = m->dec2;
        p.chain = o.allow_chain2 && chain2_fwd_ok(e2[0].KT, e2[1].KT, d2[0].KT, M) && e2[0].Kp32 == m->Dp[0] && e2[0].Np32 == 32 * e2[1].KT &&
                  e2[1].Np32 == e2[0].Np32 && e2[2].KT == e2[1].KT && e2[2].Np32 == 2 * m->Dp[1] && d2[0].Kp32 == m->Dp[1] && d2[0].Np32 == e2[0].Np32 &&
                  d2[1].KT == e2[1].KT && d2[1].Np32 == d2[0].Np32 && d2[2].KT == e2[1].KT && d2[2].Np32 == 2 * m->Dp[0];
        p.chain2_bwd = p.chain && bwd && o.allow_chain2_bwd && gblock_bwd_ok(e2[0].KT, e2[1].KT, d2[0].KT, M) && e2[0].imgB && d2[0].imgB;
    }
    // ---- the output layer's block
    DenseArgs& a = p.bern;
    a.ldX = L.Kp32; a.img = L.imgF;
    a.split = 1 << 30;
    a.M = M; a.KT = L.KT; a.MG = L.MG; a.mg_per_block = L.MG; a.Np32 = L.Np32; a.g1_mask = o.dense_g1_mask;
    // few rows: the output layer runs inside block_fwd_kernel, behind the two tanh layers of the same 16-row tile (one launch for the
    // whole decoder; log p(x|z) per row comes out whole, not as per-group partial sums)
    const bool out_in_block = o.allow_block_fused && allow_out_in_block && !fuse_z && M <= 4096 && !(want && want->logits) && !m->want_stamps &&
                              d1[1].Np32 == d1[0].Np32 && d1[1].Kp32 == d1[0].Np32 && L.Kp32 == d1[1].Np32 && L.KT == d1[1].KT && L.KT <= 8;
    // small row counts (the reference's default B = 20, k = 5): a handful of workgroups walking all 13 pixel groups
    // in turn is 40 us of latency -- one pixel group per block instead, log p(x|z) as per-group partial sums that
    // lse_kernel adds up in fixed order
    if (M < 8192 && L.MG > 1 && !out_in_block) { a.mg_per_block = 1; p.px_parts = L.MG; }
    a.ldXB = m->Xinp; a.k = k; a.B = B; a.Xdim = X;
    a.lpxz_stride = p.px_parts > 1 ? (size_t)Mp : 0;
    // training step: keep s = x - sigmoid(l) for the backward pass (out_bwd_s_kernel, output-layer weight gradient)
    p.s_mode = bwd && o.allow_s_mode && out_bwd_has_s_mode(L.KT);
    if (p.s_mode) {
        a.ldYP = Xp;
        if (m->fake_s & 4) a.dbg = 32;
        if (m->fake_s & 16) a.dbg |= 64;      // (the decoder kernel's tanh layers without their weight DMA)
        if (m->fake_s & 32) a.dbg |= 128;     // (phase exits of the decoder kernel, for instruction counters: behind the prologue,
        if (m->fake_s & 64) a.dbg |= 256;     //  behind both tanh layers,
        if (m->fake_s & 128) a.dbg |= 512;    //  behind the first)
    }
    a.pipe = allow_bern_pipe ? 1 : 0;
    if (a.pipe && o.bern_qw) {      // the 16-wave / 200-row shape is one workgroup per CU: only where its last round is nearly full
        const int nwg = (M + 199) / 200, ncu = std::max(1, m->num_cus);
        const int rounds = (nwg + ncu - 1) / ncu;
        if ((double)nwg >= 0.9 * (double)rounds * ncu || o.bern_qw_force) a.pipe = 2;
    }
    // ---- the decoder's tanh layers
    // The whole decoder in one launch (bern_pipe_kernel<.., PRE>) where that kernel exists: the two tanh layers' activations
    // stay in registers from layer to layer (z made in the kernel when the step runs on the device's noise).
    if (o.allow_dec_fused && a.pipe && m->C == 0 && d1[0].KT <= 4 && d1[0].Kp32 == m->Dp[0] && d1[0].Np32 == L.Kp32 && d1[1].Kp32 == L.Kp32 && d1[1].Np32 == L.Kp32) {
        DenseArgs pre = a;
        pre.pre_img1 = d1[0].imgF; pre.pre_KT1 = d1[0].KT; pre.pre_img2 = d1[1].imgF;
        pre.logits_out = want ? want->logits : nullptr;      // (only "logits are written", in this local copy: the predicate refuses it, so the plan's block never holds the caller's pointer)
        if (bern_pipe_ok(pre)) { a = pre; p.dec_fwd = DEC_PIPE; }
    }
    // few rows: the two tanh layers as ONE launch of block_fwd_kernel (a BasicBlock without its head: 16-row workgroups,
    // weights straight from the L2-resident images) instead of two latency-bound dense_kernel launches
    if (p.dec_fwd != DEC_PIPE && o.allow_block_fused && !fuse_z && M <= 4096 && d1[1].Np32 == d1[0].Np32 && d1[1].Kp32 == d1[0].Np32) {
        BlockFwdArgs& b = p.dec_blk;
        b.ldX = d1[0].Kp32; b.img0 = d1[0].imgF; b.img1 = d1[1].imgF; b.img2 = d1[1].imgF;
        b.KT0 = d1[0].KT; b.KT1 = d1[1].KT; b.NT1 = d1[0].Np32 / 16; b.NT2 = 0; b.R = M;
        b.ldH = d1[0].Np32; b.split = 1 << 30;
        if (sample_in_block) { b.sample = 1; b.S.Dp = m->Dp[0]; b.S.M = M; }      // (forward_impl puts the whole sampling block there)
        if (out_in_block) { b.oimg = L.imgF; b.oXdim = X; b.oH = L.Np32 >> 5; b.oldXB = m->Xinp; b.ok = k; b.oldS = Xp; }
        if (block_fwd_shape_ok(b)) p.dec_fwd = out_in_block ? DEC_BLOCK_OUT : DEC_BLOCK2;
    }
    const bool in_block = p.dec_fwd == DEC_BLOCK2 || p.dec_fwd == DEC_BLOCK_OUT;
    // (dense_kernel's sampled-input mode has no DReG sum; a block kernel that does not run cannot sample either: sample_kernel then)
    p.z_from = p.chain ? Z_CHAIN2 : (fuse_z && p.dec_fwd == DEC_PIPE) ? Z_DEC_PROLOGUE : (fuse_z && !p.want_dreg) ? Z_DENSE_ZIN : (sample_in_block && in_block) ? Z_BLOCK : Z_SAMPLE;
    // ---- log-mean-exp and the output layer's weight gradient
    p.early_wout = bwd && p.s_mode && o.allow_early_wout && !p.dec_rows;      // (few data rows: no side-stream work in the backward pass at all)      // (round 3: the 2-layer model too -- its weight gradients are 220 us of kernels, on ONE side stream behind dec_bwd they ended 100 us after the main stream)
    // Round 3: where the decoder kernel's workgroups own whole images (16-wave / 200-row shape, k a divisor of 200) it also does
    // lse_kernel's work for them -- the backward pass starts right behind it: one launch (7 us) and one dispatch gap (6 us) less
    // on the loop that sets the step, and no second lse_kernel on the side stream.
    if (p.dec_fwd == DEC_PIPE && o.allow_lse_fused && !m->want_stamps) {
        DenseArgs lse = a;      // (shapes only; forward_impl asks again on the filled block, where z made in the prologue brings its term pointers)
        lse.lse_on = 1; lse.lse.n_px_part = 1;
        if (bern_lse_ok(lse)) { a.lse_on = 1; p.lse_fused = true; }
    }
    // round 4: with the row weights made inside the decoder kernel, it also leaves g2w = bf16(g_r g2) -- the output layer's weight gradient
    // (forked right behind this kernel) then needs no row weighting.  Needs a pad column in the hidden width for g_r itself (the bias gradient).
    p.g2w = p.lse_fused && p.early_wout && o.allow_g2w && p.s_mode && L.Kin < L.Kp32 && !two;
    if (p.g2w) a.g2w_feat = L.Kin;
    // s-mode training step: the output layer's weight gradient needs s, g2 and the row weights -- not out_bwd -- so the
    // side stream forks early.  Round 2: it forks behind the decoder kernel (event on its dispatch packet) and runs its own copy of
    // lse_kernel (7 us, a few waves) for the row weights, instead of forking behind the main stream's lse_kernel: the ~12 us
    // a cross-stream hand-off takes now pass beside the main stream's lse_kernel, not behind it.
    p.lse_dup = p.early_wout && o.allow_lse_dup && p.px_parts == 1 && p.dec_fwd != DEC_BLOCK_OUT && !p.lse_fused;
    if (p.lse_fused) p.lse_at = LSE_DECODER;
    if (!bwd) return p;

    // ---- the backward pass
    // One launch for out_bwd + dX of d2 + dX of d1 (dec_bwd_kernel) where it exists: s kept by the forward pass, hidden width with an
    // instantiation, large row counts or (small_dec_bwd) few; dpre2 / dpre1 stay in registers from product to product.
    const bool small_fused = o.small_dec_bwd && o.allow_dec_bwd && p.s_mode && M <= o.small_rows && out_bwd_has_s_mode(L.KT) && !m->want_stamps;
    p.out_parts = p.s_mode && M < 8192 && L.MG > 1 && !small_fused;      // small row counts: one pixel group per block, partial sums + finish kernel
    const bool fused_dx = o.allow_dec_bwd && p.s_mode && !p.out_parts && (M >= 8192 || small_fused) && !(m->want_stamps && L.KT == 7) && L.kmajor && L.imgB &&
                          d1[1].KT_B == L.KT && d1[1].MG_B == (L.KT + 1) / 2 && d1[0].KT_B == L.KT && d1[1].Kp32 == L.Kp32 && d1[0].Np32 == L.Kp32;
    // 1-layer model: dz has one reader (latent_bwd_kernel): bf16 halves its 26 MB each way (the 2-layer model adds two more
    // float32 terms to it there and keeps float32)
    p.dz_half = fused_dx && !two && o.allow_dz_half;
    DecBwdRowsArgs& r = p.rows;      // few rows: 16-row workgroups, weights straight from L2
    r.ldS = Xp; r.KTX = Xp / 32; r.imgK3 = L.imgB; r.MT3 = L.MT_B;
    r.imgB2 = d1[1].imgB; r.imgB1 = d1[0].imgB; r.KT = L.KT; r.NT1 = L.Kp32 / 16; r.NT3 = d1[0].Kp32 / 16; r.M = M;
    r.ldH = L.Kp32; r.ldDZ = d1[0].Kp32;
    p.dx = !fused_dx ? DX_THREE : (M <= o.dec_rows_max && o.allow_block_fused && dec_bwd_rows_ok(r)) ? DX_ROWS : DX_DEC_BWD;
    // Few rows (round 4): the training step's log-mean-exp is done by the backward pass's first kernel (dec_bwd_rows_kernel, a wave per
    // image in front of its own work): one dependent launch less on a chain of ~10 us launches.  1-layer model below small_rows only: the
    // kernel has never taken the 2-layer model's five terms, nor the log-mean-exp of a step of 8 192 rows or more
    if (!p.lse_fused && o.allow_lse_in_bwd && !p.lse_dup && !p.early_wout && p.dx == DX_ROWS && small_fused && !two) { p.lse_at = LSE_BWD_ROWS; r.lse_on = 1; }
    // ---- the side streams: the decoder's weight gradients only need what the dX chain produced plus forward activations
    // Few rows (round 3): the three as ONE grouped launch on `side2` behind the dX chain (the B = 20 step is bound by the host's
    // launches and the streams' hand-offs, not by these kernels: 13 -> 11 launches, two events less)
    // (early_wout says: stored s, and not the single-stream dec_rows step)
    const bool few_side2 = p.early_wout && o.allow_wg3 && o.use_side2 && M <= 4096;
    int ns[3], nw[3], cps;
    for (int i = 0; i < 3; ++i) wgradp_shape(m, d1[i], M, ns[i], nw[i], cps);
    p.group3 = few_side2 && fused_dx && nw[0] == 8 && nw[1] == 8 && nw[2] == 8;
    p.wout_two_part = !p.dec_rows && !p.group3 && o.wout_split > 0 && p.s_mode && !p.g2w && p.early_wout && o.use_side2 && fused_dx && M >= 8192 && L.IT <= 14 && o.allow_wg7 && !(m->abl_skip & 1);
    // The hidden layers' weight gradients need dpre2 / dpre1, not the output layer's gradient: forked early, that one keeps `side` busy well
    // past the end of the dX chain, so they go to a second side stream and run beside it.  They finish last, so that stream is the `tail`.
    p.hid_on = p.dec_rows ? ON_MAIN : (p.group3 || (p.early_wout && o.use_side2)) ? ON_SIDE2 : ON_SIDE;
    p.hid_group = nw[1] == 7 && nw[0] == 7 && o.allow_wg_group && (p.early_wout || fused_dx);      // (both inputs ready: one launch)
    p.tail = p.dec_rows ? ON_SIDE : p.hid_on;
    // The NEXT step's noise is drawn on a stream that this backward pass orders behind the main stream and whose last event the next forward
    // joins: `side`; few rows, where `side2` carries the group (or the hidden layers' gradients) and the decoder update in front of that
    // event: `side2`; the dec_rows step touches no side stream at all: the draw stays in stream order
    p.draw_on = p.dec_rows ? ON_MAIN : few_side2 ? ON_SIDE2 : ON_SIDE;
    // ---- the encoder
    // Few images and samples (round 4): latent_bwd_kernel's per-image sums are made inside the encoder's block_bwd_kernel (a wave per image in
    // front of its dX chain) -- one dependent launch less; the separate kernel (256 threads per image) stays for many samples per image
    // (measured, end-to-end us per step with / without: B = 20, k = 1: 67.7 / 70.0; B = 20, k = 5: 67.5 / 69.3; B = 100, k = 5: 72.1 / 73.4; B = 20, k = 50: 88.2 / 78.5 --
    // one wave walking 50 samples is slower than latent_bwd_kernel's 256 threads: up to 16 samples per image)
    // (round 5, option lat_rows4: beyond 16 samples per image block_bwd_kernel<4> -- 4 images per workgroup, an image's samples over four waves --
    // can take the sums on 4 x the workgroups; measured no faster than the two launches in the step, see allow_lat_rows4)
    BlockBwdArgs bb;
    p.lat_fuse = o.allow_lat_in_block && B <= 1024 && (k <= 16 || (o.allow_lat_rows4 && B >= 64)) && block_bwd_shape(m, m->enc1, B, bb) &&
                 lat_in_block_ok(m->enc1, m->Dp[0], m->has_prior, false);
    // Round 4: on few rows the image encoder's weight gradients, their sum over ALL rows and (fused step) the Adam update are one launch
    // (wgrad_rows_kernel) -- the encoder's layers (the head of the table) then need no slabs and no share of reduce_grads_kernel
    p.rows_enc = wgrad_rows_ok(m, m->enc1, B);
    return p;
}

// How that step ends, from its plan and the caller's StepEnd: who sums which weight-gradient slabs, on which stream, behind which wait, with or without
// Adam, and what that leaves behind.  As pure as plan_step: it reads the plan, the options and the layer table (TableBounds) and touches no stream,
// event or buffer; it fills e in place.
void plan_step_end(const iwae_model* m, const StepPlan& p, StepEnd mode, StepEndPlan& e) {
    const StepOptions& o = m->opt;
    const TableBounds& t = m->tb;
    const bool two = m->cfg.n_layers == 2;
    const bool fuse = mode == END_UPDATE, split = mode == END_GRAD_SPLIT || mode == END_GRAD_SPLIT_HELD;
    const bool dec_own = !two && !p.dec_rows && dec_layers_last(m);      // the decoder's layers can be summed apart from the rest: by the stream that carried their gradients
    // the decoder's slab sums + Adam stay on the side stream and are NOT joined at the end of the step (join_side)
    const bool defer = fuse && o.allow_defer && dec_own;      // (2-layer: the main stream needs the side-stream block gradients anyway)
    // ... as one deferred update per side stream, each behind the weight gradients it carried (option defer_split)
    const bool split_upd = defer && o.defer_split && p.hid_on == ON_SIDE2 && !p.group3 && p.early_wout;
    // gradient only: the decoder's layers are summed into the flat gradient on the side stream, right behind their weight gradients
    const bool early = !fuse && dec_own;
    // 2-layer training step at large row counts (round 3): every layer behind the image encoder has its weight gradients on the side
    // streams; their slab sums + Adam follow there, instead of the main stream waiting for both side streams and then summing all 94 MB itself
    const bool defer2 = fuse && two && o.allow_defer && o.allow_defer2 && side_layers_from_enc2(m) && p.chain2_bwd && p.early_wout && o.use_side2 && !split;
    // ... one update per side stream, each for the layers whose weight gradients IT carried
    const bool defer2_split = defer2 && p.tail == ON_SIDE2 && o.allow_defer2_split && m->dec2[0].nsub == 1 && m->dec1[0].nsub == 1 && m->dec1[2].nsub == 1;
    e = StepEndPlan();
    e.update = fuse;
    e.how = early ? (mode == END_GRAD_SPLIT_HELD ? ENDS_EARLY_HELD : split ? ENDS_EARLY_SPLIT : ENDS_EARLY) : defer2 ? (defer2_split ? ENDS_DEFER2_SPLIT : ENDS_DEFER2) :
            p.dec_rows ? ENDS_DEC_ROWS : defer ? (split_upd ? ENDS_SPLIT_UPD : ENDS_DEFER) : ENDS_JOINED;
    // joined: every weight gradient launched on a side stream is in its slabs before the main stream sums them -- the 2-layer model's per-sample
    // blocks' went to `side` behind the output layer's, so where that is not the tail both side streams join.  (early / defer: the side stream
    // sums its own; defer2: likewise, nothing to join; dec_rows: nothing ran on a side stream)
    e.join_both = e.how == ENDS_JOINED && two && p.tail != ON_SIDE;
    // the main stream's share of the table: [lo, hi) -- empty when wgrad_rows_kernel took the encoder and everything else is
    // deferred to the side streams (the full-size 1- and 2-layer steps) or rode in the same launch (few data rows: p.dec_rows, where
    // the decoder's three layers drop out of the range and leave two)
    const int lo = p.rows_enc ? t.enc1_end.r : 0, hi = (defer || early) ? t.dec1.r : defer2 ? t.enc2.r : t.end.r;
    const int d0 = p.dec_rows ? t.dec1.r : hi, d1 = p.dec_rows ? t.dec1_end.r : hi;
    e.main_a = BlockRange{lo, std::max(0, std::min(d0, hi) - lo)};
    e.main_b = BlockRange{d1, std::max(0, hi - d1)};
    e.left.split_offset = early && split ? m->klayers[m->dec1[0].sub[0]].offW : m->nparam;
    e.left.on = p.tail;
    if (e.how == ENDS_JOINED || e.how == ENDS_DEC_ROWS) return;
    // the side streams' shares, in the order they are enqueued
    auto sum = [&](OnStream on, TableBounds::At a0, TableBounds::At a1, TableBounds::At b0, TableBounds::At b1, SideWait behind = WAIT_NONE, bool second = false) {
        e.side[e.nside++] = SideSum{on, BlockRange{a0.r, a1.r - a0.r}, BlockRange{b0.r, b1.r - b0.r}, behind, second};
    };
    if (e.how == ENDS_DEFER2_SPLIT) {
        // each side stream sums and updates the layers whose weight gradients IT carried, as soon as its own chain ends: the second one the
        // encode block q(z2|z1) and the decoder's two tanh layers, the first one the decode block p(z1|z2) and the output layer (two block
        // ranges per launch: table order enc2 | dec2 | dec1).  The next forward waits for both events (join_side).
        sum(ON_SIDE2, t.enc2, t.dec2, t.dec1, t.dec1_out);
        sum(ON_SIDE, t.dec2, t.dec1, t.dec1_out, t.end, WAIT_NONE, true);
    } else if (e.how == ENDS_DEFER2) {
        sum(p.tail, t.enc2, t.end, t.end, t.end, p.tail != ON_SIDE ? WAIT_SIDE : WAIT_NONE);
    } else if (e.how == ENDS_SPLIT_UPD) {
        // Round 5: one deferred update per side stream, each behind the weight gradients it carried -- no hand-off between the two side
        // streams in front of the update, and the output layer's share (54 % of the decoder's slabs) is done ~20 us before the hidden layers'
        // gradients end.  The output layer's gradient forked behind the decoder FORWARD: its update rewrites the W3 image dec_bwd_kernel
        // reads, so `side` waits for that kernel's event first (long complete by then).
        sum(ON_SIDE, t.dec1_out, t.end, t.end, t.end, WAIT_FORK2, true);
        sum(ON_SIDE2, t.dec1, t.dec1_out, t.end, t.end);
    } else {      // ENDS_DEFER and the three ENDS_EARLY cases
        // The decoder's layers (90 % of the slab bytes): slab sums [+ Adam] on the side stream, behind its weight gradients
        // (which wait for ev_fork2, i.e. for dX of d1, the last reader of the decoder's weight images -- without that order
        // the trajectory test caught a stale-image race), joined by the next user of the decoder (join_side): it runs beside
        // the encoder's backward pass / update and the next step's encoder forward.  (held: planned here, launched by dp_finish)
        sum(p.tail, t.dec1, t.end, t.end, t.end);
        if (e.how == ENDS_EARLY_HELD) e.left.held = e.side[0].a;
    }
    e.left.dec = e.how != ENDS_EARLY;      // (ENDS_EARLY: the main stream has waited for ev_dec itself by the end of the step)
    e.left.dec2 = e.nside == 2;
}

// log_w / log-mean-exp arguments of the call in flight (lse_kernel, or the kernel that does its work: StepPlan::lse_at); the buffers exist (lse_alloc)
void lse_args(iwae_model* m, int objective, bool bwd, const iwae_tensors* want, LseArgs& a) {
    const bool two = m->cfg.n_layers == 2;
    float* lpxz = ptr<float>(m->rows[0]);
    memset(&a, 0, sizeof(a));
    if (!two) {
        a.term[0] = lpxz; a.coef[0] = 1.f;
        a.term[1] = ptr<float>(m->rows[1]); a.coef[1] = m->beta;
        a.term[2] = ptr<float>(m->rows[2]); a.coef[2] = -m->beta;
        a.head = ptr<float>(m->wenc1.head); a.ldH = 2 * m->Dp[0]; a.D = m->D[0]; a.Dp = m->Dp[0];
        a.cz_on = 1.f;
    } else {
        a.term[0] = lpxz; a.coef[0] = 1.f;    // iwae2.py:128 (beta unused there)
        a.term[1] = ptr<float>(m->rows[1]); a.coef[1] = 1.f;
        a.term[2] = ptr<float>(m->rows[2]); a.coef[2] = 1.f;
        a.term[3] = ptr<float>(m->rows[3]); a.coef[3] = -1.f;
        a.term[4] = ptr<float>(m->rows[4]); a.coef[4] = -1.f;
        a.head = nullptr;
        a.cz_on = 0.f;
    }
    a.lq_dreg = m->plan.want_dreg ? ptr<float>(m->rows[5]) : nullptr;
    a.B = m->B; a.k = m->k; a.beta = two ? 1.f : m->beta; a.objective = objective;
    a.lme_only = (!bwd && m->call.log_w_only && !want) ? 1 : 0;
    a.logw = ptr<float>(m->logw); a.wn = ptr<float>(m->wn); a.gx = ptr<float>(m->gx);
    a.cf = ptr<float4>(m->cf); a.per_b = ptr<float>(m->per_b);
    a.n_px_part = 1; a.px_stride = (size_t)m->Mp; a.term0_out = lpxz;
}
// ... with log p(x|z) taken from the per-pixel-group partial sums where the forward left those (lse_kernel, dec_bwd_rows_kernel)
void lse_args_parts(iwae_model* m, int objective, bool bwd, const iwae_tensors* want, LseArgs& a) {
    lse_args(m, objective, bwd, want, a);
    if (m->plan.px_parts > 1) a.term[0] = ptr<float>(m->px_part);
    a.n_px_part = m->plan.px_parts;
}
int lse_alloc(iwae_model* m) {
    hipStream_t st = m->stream;
    CHK(ensure(m->logw, (size_t)m->Mp * 4, st));
    CHK(ensure(m->wn, (size_t)m->Mp * 4, st));
    {   // the row weights are also read 64 at a time by the output layer's weight gradient: pad rows must stay finite
        const void* before = m->gx.p;
        CHK(ensure(m->gx, (size_t)m->Mp * 4, st));
        if (m->gx.p != before) HIPCHK(hipMemsetAsync(m->gx.p, 0, m->gx.cap, st));
    }
    CHK(ensure(m->cf, (size_t)m->Mp * 16, st));
    CHK(ensure(m->per_b, (size_t)PB_COUNT * m->B * 4, st));
    return IWAE_OK;
}

}  // namespace -- begin_forward, stage_input: external (hidden) linkage, declared in model.h, step_f32.hip calls them too
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
namespace {      // (internal linkage again)

int forward_impl(iwae_model* m, const float* x, int B, int k, float beta, const float* eps, int objective, bool bwd,
                 const iwae_tensors* want, const FwdCall& call) {
    const float* cond;
    CHK(begin_forward(m, x, B, k, beta, call, &cond));
    m->plan = plan_step(m, B, k, objective, bwd, call, want, eps != nullptr);
    const StepPlan& p = m->plan;
    const bool two = m->cfg.n_layers == 2;
    m->bf16_side_used = true;
    if (m->left.z_pending) { HIPCHK(hipStreamWaitEvent(m->stream, m->ev_join, 0)); m->left.z_pending = false; }      // (ev_join is this path's too)
    m->time_this = m->timing > 0 && (m->timing_calls++ % m->timing) == 0;
    const int M = m->M, Mp = m->Mp, Bp = m->Bp, X = m->X, Xp = m->Xp32, Xinp = m->Xinp;
    hipStream_t st = m->stream;
    m->user_eps = eps != nullptr;
    // ---- the step's N(0,1) draws: normally already there (prefetched by the previous training step), else drawn now
    m->epsc_ptr[0] = m->epsc_ptr[1] = nullptr;
    if (p.eps_multi) {      // few data rows: from the multi-step buffers (one launch per EPSM_STEPS steps)
        int bi = epsm_find(m, m->noise_step, M);
        if (bi < 0) {      // (first step, another batch shape, a jump of iwae_set_step: drawn now, in stream order)
            bi = (m->epsm_tag[0].valid && !m->epsm_tag[1].valid) ? 1 : 0;
            CHK(draw_eps_multi(m, bi, m->noise_step, M, st));
        }
        const size_t soff = (size_t)(m->noise_step - m->epsm_tag[bi].step0) * (size_t)round_up(M, 128);
        for (int l = 0; l < m->cfg.n_layers; ++l) m->epsc_ptr[l] = ptr<float>(m->epsm[bi][l]) + soff * eps_ld(m, l);
    } else
    if (p.keep_eps) {
        const int np = (m->epsc_par + 1) % 3;
        const uint64_t ro = (uint64_t)call.batch_offset * (uint64_t)k;
        iwae_model::EpsTag& tg = m->eps_tag[np];
        if (call.k_total > 0 || !(tg.valid && tg.step == m->noise_step && tg.row_offset == ro && tg.M == M)) {
            CHK(join_side(m));          // a speculative draw into this slot may still be on a side stream
            if (m->side) HIPCHK(hipStreamSynchronize(m->side));
            if (m->side2) HIPCHK(hipStreamSynchronize(m->side2));
            CHK(draw_eps(m, np, m->noise_step, M, st));
            if (call.k_total > 0) tg.valid = false;      // (a k-chunk's draws: the tag does not describe them)
        }
        if (bwd) m->epsc_par = np;      // (forward-only calls -- the evaluator's launches -- reuse ONE slot: stream order protects it, and three slots of 2^21 rows are 2.5 GB grown inside the first calls)
        for (int l = 0; l < m->cfg.n_layers; ++l) m->epsc_ptr[l] = ptr<float>(m->epsc[np][l]);
    }
    if (eps) CHK(copy_in(m, m->epsbuf, eps, (size_t)M * (m->D[0] + (two ? m->D[1] : 0)) * 4));
    CHK(ensure(m->xP, (size_t)Bp * Xinp * 2, st));
    const float *xd, *xf_pending = nullptr;
    if (call.mask_resident) {      // the masked step from the resident set: xin as bf16 in m->xP and the hole-coded pixel rows, one launch
        CHK(ensure(m->mk.xcP, (size_t)Bp * Xinp * 2, st));
        MaskedStage ms;
        ms.xP = ptr<uint16_t>(m->xP); ms.xcP = ptr<uint16_t>(m->mk.xcP);
        CHK(stage_input(m, x, B, false, &xd, &ms));      // (xd: null -- the rows are in m->xP already)
    } else CHK(stage_input(m, x, B, p.holes, &xd));
    if (p.holes && !call.mask_resident) {      // the masked step on the caller's mask: the hole-coded pixel rows for the output layer; xin = m ? x : 0 is the call's x from here on (m->xP: the encoder, its backward and weight gradient)
        if (!xd) return fail(IWAE_ERR_STATE, "forward: the masked step has no float32 rows of this batch");
        const uint8_t* maskd;
        CHK(staged_in(m, call.mask, m->mk.mask, (size_t)B * X, &maskd));
        CHK(ensure(m->mk.xcP, (size_t)Bp * Xinp * 2, st));
        CHK(ensure(m->mk.xin, (size_t)B * X * 4, st));
        launch_masked_code_bf16(xd, maskd, B, X, Xinp, Bp, ptr<uint16_t>(m->mk.xcP), st);
        launch_impute_mask(xd, maskd, (long)B * X, ptr<float>(m->mk.xin), st);
        xd = ptr<float>(m->mk.xin);
    }
    if (p.holes && (p.dec_fwd == DEC_PIPE || p.dec_fwd == DEC_BLOCK_OUT || (bwd && !p.s_mode)))      // (masked_bf16_ok and plan_step rule all three out)
        return fail(IWAE_ERR_STATE, "forward: the masked step was planned onto a kernel that knows no mask");
    if (xd) {      // (the resident set's rows are in m->xP already)
        if (p.enc_takes_f32) xf_pending = xd;      // the fused encoder kernel converts the rows itself
        else launch_prep_rows(xd, cond, B, X, m->C, Xinp, Bp, ptr<uint16_t>(m->xP), st);
    }

    // ---- encoder over images (iwae1.py:57 / iwae2.py:59)
    CHK(block_alloc(m, m->enc1, m->wenc1, B, Bp, bwd, false));
    {
    ScopedTimer tm_enc(m, T_ENC_FWD);
    CHK(block_fwd(m, m->enc1, m->wenc1, ptr<uint16_t>(m->xP), B, xf_pending, X));
    }

    for (int i = 0; i < 6; ++i) CHK(ensure(m->rows[i], (size_t)Mp * 4, st));
    float* lpxz = ptr<float>(m->rows[0]);
    float* t1 = ptr<float>(m->rows[1]);   // 1-layer lpz   | 2-layer lpz1z2
    float* t2 = ptr<float>(m->rows[2]);   // 1-layer lqzx  | 2-layer lpz2
    float* t3 = ptr<float>(m->rows[3]);   //               | 2-layer lqz1x
    float* t4 = ptr<float>(m->rows[4]);   //               | 2-layer lqz2z1
    float* lqd = ptr<float>(m->rows[5]);

    // ---- z (z1) = mu + sigma*eps and its densities (iwae1.py:59,107,109)
    // the draws are kept when later kernels of this call need them again (backward, 2-layer densities)
    CHK(ensure(m->zP[0], (size_t)Mp * m->Dp[0] * 2, st));
    CHK(join_side(m));      // from here on: the prefetched noise, then the decoder's weights
    SampleArgs zin;      // the sampling of z (z1): sample_kernel's arguments, or the prologue's of the kernel that makes z itself (p.z_from)
    memset(&zin, 0, sizeof(zin));
    if (m->has_prior) {     // p(z|y) = N(mu_p(y), sigma_p(y)) (tasks/task04.py:124): the prior block on the B condition rows
        const int Cp = round_up(m->C, 32);
        CHK(ensure(m->condP, (size_t)Bp * Cp * 2, st));
        launch_prep_rows(cond, nullptr, B, m->C, 0, Cp, Bp, ptr<uint16_t>(m->condP), st);
        CHK(block_alloc(m, m->prior, m->wprior, B, Bp, bwd, false));
        CHK(block_fwd(m, m->prior, m->wprior, ptr<uint16_t>(m->condP), B));
    }
    {
        SampleArgs s;
        memset(&s, 0, sizeof(s));
        s.head = ptr<float>(m->wenc1.head); s.ldH = 2 * m->Dp[0]; s.Dp = m->Dp[0]; s.D = m->D[0]; s.head_per_row = 0;
        s.M = M; s.Mp = Mp; s.k = k; s.B = B; s.eps = eps_src(m, 0);
        s.ZP = ptr<uint16_t>(m->zP[0]);
        s.cond = cond; s.C = m->C;
        s.prior_head = m->has_prior ? ptr<float>(m->wprior.head) : nullptr;
        s.lp_prior = two ? nullptr : t1;
        s.lq = two ? t3 : t2;
        s.lq_dreg = p.want_dreg ? lqd : nullptr;
        zin = s;
        if (p.z_from == Z_SAMPLE) launch_sample(s, st);
    }
    if (two) {
        // ---- q(z2|z1), z2, p(z1|z2)  (iwae2.py:63-65, :90, :118-124)
        CHK(block_alloc(m, m->enc2, m->wenc2, M, Mp, bwd, true));
        CHK(ensure(m->zP[1], (size_t)Mp * m->Dp[1] * 2, st));
        CHK(block_alloc(m, m->dec2, m->wdec2, M, Mp, bwd, true));
        // large row counts, the reference's dims: the z1 sampling, both per-sample blocks, the z2 sampling and the four log-densities in ONE launch
        const Linear *e2 = m->enc2, *d2 = m->dec2;
        if (p.chain) {
            Chain2FwdArgs c;
            memset(&c, 0, sizeof(c));
            c.Z1P = ptr<uint16_t>(m->zP[0]); c.lqz1x = t3;
            c.e_img1 = e2[0].imgF; c.e_img2 = e2[1].imgF; c.e_imgh = e2[2].imgF;
            c.d_img1 = d2[0].imgF; c.d_img2 = d2[1].imgF; c.d_imgh = d2[2].imgF;
            c.M = M; c.k = k; c.B = B; c.D0 = m->D[0]; c.D1 = m->D[1];
            // the backward pass reads the blocks' tanh activations; the float32 heads only where something still reads THEM: the unfused
            // backward kernels (gauss_bwd_kernel) and the z2 / snis exports -- gblock_bwd_kernel recomputes them from h2
            const bool heads = want != nullptr || (bwd && !p.chain2_bwd);
            c.EH1 = bwd ? ptr<uint16_t>(m->wenc2.h1P) : nullptr; c.EH2 = bwd ? ptr<uint16_t>(m->wenc2.h2P) : nullptr;
            c.EHEAD = heads ? ptr<float>(m->wenc2.head) : nullptr;
            c.Z2P = ptr<uint16_t>(m->zP[1]);
            c.DH1 = bwd ? ptr<uint16_t>(m->wdec2.h1P) : nullptr; c.DH2 = bwd ? ptr<uint16_t>(m->wdec2.h2P) : nullptr;
            c.DHEAD = heads ? ptr<float>(m->wdec2.head) : nullptr;
            c.head1 = ptr<float>(m->wenc1.head); c.ldH1 = 2 * m->Dp[0];
            c.eps1 = eps_src(m, 0); c.eps2 = eps_src(m, 1);
            c.lpz1z2 = t1; c.lpz2 = t2; c.lqz2z1 = t4;
            launch_chain2_fwd(c, st);
        } else {
        CHK(block_fwd(m, m->enc2, m->wenc2, ptr<uint16_t>(m->zP[0]), M));
        SampleArgs s;
        memset(&s, 0, sizeof(s));
        s.head = ptr<float>(m->wenc2.head); s.ldH = 2 * m->Dp[1]; s.Dp = m->Dp[1]; s.D = m->D[1]; s.head_per_row = 1;
        s.M = M; s.Mp = Mp; s.k = k; s.B = B; s.eps = eps_src(m, 1);
        s.ZP = ptr<uint16_t>(m->zP[1]);
        s.lp_prior = t2; s.lq = t4; s.lq_dreg = nullptr;
        launch_sample(s, st);
        CHK(block_fwd(m, m->dec2, m->wdec2, ptr<uint16_t>(m->zP[1]), M));
        GaussLpArgs g;
        memset(&g, 0, sizeof(g));
        g.zhead = ptr<float>(m->wenc1.head); g.ldZH = 2 * m->Dp[0]; g.Dzp = m->Dp[0];
        g.phead = ptr<float>(m->wdec2.head); g.ldPH = 2 * m->Dp[0]; g.Dpp = m->Dp[0];
        g.D = m->D[0]; g.M = M; g.k = k; g.eps = eps_src(m, 0); g.out = t1;
        launch_gauss_lp(g, st);
        }
    }

    // ---- decoder + Bernoulli log-likelihood (iwae1.py:81-83,111)
    MlpWs& w = m->wdec1;
    const int Hp = m->dec1[0].Np32;
    CHK(ensure(w.g1P, (size_t)Mp * Hp * 2, st));
    CHK(ensure(w.g2P, (size_t)Mp * Hp * 2, st));
    {
        DenseArgs a = p.bern;      // the plan's shapes; the buffers follow
        a.X = ptr<uint16_t>(w.g2P);
        if (p.px_parts > 1) CHK(ensure(m->px_part, (size_t)p.px_parts * Mp * 4, st));
        a.XB = ptr<uint16_t>(p.holes ? m->mk.xcP : m->xP);
        a.lpxz = p.px_parts > 1 ? ptr<float>(m->px_part) : lpxz;
        if (p.s_mode) {      // s = x - sigmoid(l) stays for the backward pass (out_bwd_s_kernel, output-layer weight gradient)
            CHK(ensure(m->wdec1.dlP, (size_t)Mp * Xp * 2, st));
            a.YP = ptr<uint16_t>(m->wdec1.dlP);
        }
        a.logits_out = nullptr;
        if (want && want->logits) {
            CHK(ensure(m->scratch, (size_t)M * X * 4, st));
            a.logits_out = ptr<float>(m->scratch);
        }
        if (p.dec_fwd == DEC_PIPE) {      // the whole decoder in one launch
            a.pre_Z = ptr<uint16_t>(m->zP[0]);
            // g1, g2 are kept for the backward pass only: a forward-only call (val_step, the k = 5000 evaluator) never reads them back
            a.pre_G1 = (bwd && !(m->fake_s & 8)) ? ptr<uint16_t>(w.g1P) : nullptr; a.pre_G2 = (bwd && !(m->fake_s & 8)) ? ptr<uint16_t>(w.g2P) : nullptr;      // (fake_s & 8, DIAG builds: timing without the activation stores)
            if (p.z_from == Z_DEC_PROLOGUE) {
                a.zhead = zin.head; a.ldZH = zin.ldH; a.zeps = zin.eps.cache; a.zldE = zin.eps.ldC; a.zD = zin.D; a.zDp = zin.Dp;
                a.ZPout = (bwd && !(m->fake_s & 8)) ? zin.ZP : nullptr; a.zlp = zin.lp_prior; a.zlq = zin.lq; a.zlq_dreg = zin.lq_dreg;      // (a forward-only call never reads z back)
            }
        } else if (p.dec_fwd == DEC_DENSE) {
            CHK(dense_fwd(m, m->dec1[0], EPI_TANH, ptr<uint16_t>(m->zP[0]), M, ptr<uint16_t>(w.g1P), nullptr, 0, p.z_from == Z_DENSE_ZIN ? &zin : nullptr));
            CHK(dense_fwd(m, m->dec1[1], EPI_TANH, ptr<uint16_t>(w.g1P), M, ptr<uint16_t>(w.g2P), nullptr, 0));
        } else {      // few rows: block_fwd_kernel on the two tanh layers, with z made in front and the output layer behind where the plan says so
            BlockFwdArgs bf = p.dec_blk;
            bf.X = ptr<uint16_t>(m->zP[0]); bf.H1 = ptr<uint16_t>(w.g1P); bf.H2 = ptr<uint16_t>(w.g2P);
            if (p.z_from == Z_BLOCK) bf.S = zin;
            if (p.dec_fwd == DEC_BLOCK_OUT) { bf.oXB = ptr<uint16_t>(m->xP); bf.oSP = p.s_mode ? ptr<uint16_t>(m->wdec1.dlP) : nullptr; bf.olpxz = lpxz; }
            if (!block_fwd_ok(bf)) return fail(IWAE_ERR_STATE, "forward: the decoder's block_fwd_kernel launch lacks a buffer");
            ScopedTimer tm(m, T_DEC_FWD);
            launch_block_fwd(bf, st);
        }
        CHK(attach_dense_stamps(m, EPI_BERN, a));
        CHK(lse_alloc(m));
        if (p.lse_fused) {      // the decoder kernel does lse_kernel's work for its rows
            lse_args(m, objective, bwd, want, a.lse);
            // (the launch's guard, like block_fwd_ok above: the plan asked on shapes; the terms the prologue writes must be the ones lse_args names)
            if (!bern_lse_ok(a)) return fail(IWAE_ERR_STATE, "forward: the decoder kernel's log-mean-exp terms are not the ones its prologue writes");
        }
        if (p.g2w) {
            CHK(ensure(w.g2wP, (size_t)Mp * Hp * 2, st));
            a.G2W = ptr<uint16_t>(w.g2wP);
        }
        if (bwd && p.g2w != m->g2w_descs) m->descs_dirty = true;      // (the layer table says where the output layer's bias sums are)
        // The side stream of an early output-layer weight gradient forks behind THIS kernel (event on its dispatch packet) where the row
        // weights come from it or from the side stream's own copy of lse_kernel
        const bool fork_here = p.lse_dup || (p.lse_fused && p.early_wout);
        if (p.dec_fwd != DEC_BLOCK_OUT) { ScopedTimer tm(m, T_DEC_FWD); launch_dense(EPI_BERN, a, st, (fork_here && !m->time_this) ? m->ev_lse : nullptr, p.holes); }
        if (fork_here && m->time_this) HIPCHK(hipEventRecord(m->ev_lse, st));      // (a timed step: the timer's stop event sits behind the kernel)
        HIPCHK(hipGetLastError());
        // The NEXT step's noise (speculating step + 1 with the same batch shape; the tag is checked on use): drawn now, on the stream the plan
        // names (idle until the backward pass forks) -- enqueued behind the decoder kernel so that its dispatch does not delay that one
        if (p.eps_multi) {      // the next GROUP of steps, once per group: into the buffer the current step does not read (main stream: this regime touches no other)
            if (epsm_find(m, m->noise_step + 1, M) < 0) CHK(draw_eps_multi(m, 1 - epsm_find(m, m->noise_step, M), m->noise_step + 1, M, st));
        } else
        if (bwd && p.keep_eps && m->side)
            CHK(draw_eps(m, (m->epsc_par + 1) % 3, m->noise_step + 1, M, on_stream(m, p.draw_on), m->opt.eps_blocks));
        if (want && want->logits) CHK(copy_out(m, want->logits, m->scratch.p, (size_t)M * X * 4));
    }

    // ---- log_w, log-mean-exp over k, objectives (iwae1.py:113-139)
    if (p.lse_at == LSE_DECODER) {      // the decoder kernel did it; the side stream (output layer's weight gradient) forks behind that kernel
        if (p.early_wout) HIPCHK(hipStreamWaitEvent(m->side, m->ev_lse, 0));
    } else {
        LseArgs a;
        lse_args_parts(m, objective, bwd, want, a);
        // s-mode training step: the output layer's weight gradient needs s, g2 and the row weights lse_kernel leaves -- not
        // out_bwd -- so the side stream forks here (ev_lse on this kernel's dispatch packet), one kernel earlier, and the
        // gradient runs beside out_bwd (both read s)
        if (p.lse_at == LSE_FWD) launch_lse(a, st, (p.early_wout && !p.lse_dup) ? m->ev_lse : nullptr);      // (LSE_BWD_ROWS: the backward pass's first kernel does it)
        if (p.lse_dup) {       // the side stream's copy: same inputs, its own outputs
            CHK(ensure(m->logw2, (size_t)Mp * 4, st));
            CHK(ensure(m->wn2, (size_t)Mp * 4, st));
            {
                const void* before = m->gx2.p;
                CHK(ensure(m->gx2, (size_t)Mp * 4, st));
                if (m->gx2.p != before) { HIPCHK(hipMemsetAsync(m->gx2.p, 0, m->gx2.cap, st)); HIPCHK(hipStreamSynchronize(st)); }
            }
            CHK(ensure(m->cf2, (size_t)Mp * 16, st));
            CHK(ensure(m->per_b2, (size_t)PB_COUNT * B * 4, st));
            LseArgs a2 = a;
            a2.logw = ptr<float>(m->logw2); a2.wn = ptr<float>(m->wn2); a2.gx = ptr<float>(m->gx2);
            a2.cf = ptr<float4>(m->cf2); a2.per_b = ptr<float>(m->per_b2);
            HIPCHK(hipStreamWaitEvent(m->side, m->ev_lse, 0));
            launch_lse(a2, m->side);
        }
    }
    // batch means: a training step folds them into its last kernel (backward_impl), a forward-only call takes them here
    if (!bwd) launch_scalars(ptr<float>(m->per_b), B, two ? 1.f : beta, m->d_scalars, st);
    HIPCHK(hipGetLastError());
    m->have_forward = true;
    m->fwd_was_f32 = false;
    return IWAE_OK;
}

// ---------------------------------------------------------------- the backward pass
}  // namespace -- adam_alpha: external (hidden) linkage, declared in model.h, step_f32.hip calls it too
float adam_alpha(iwae_model* m, float lr) {      // keras Adam: lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t); advances t
    m->adam_t += 1;
    const double t = (double)m->adam_t;
    return (float)((double)lr * sqrt(1.0 - pow((double)m->adam_b2, t)) / (1.0 - pow((double)m->adam_b1, t)));
}
namespace {      // (internal linkage again)

// end: how the step ends (StepEnd); lr: Adam's learning rate where that is END_UPDATE.  plan_step_end decides everything about it up front
int backward_impl(iwae_model* m, int objective, StepEnd end, float lr = 0.0f) {
    if (!m->have_forward) return fail(IWAE_ERR_STATE, "backward without forward");
    if (m->fwd_was_f32) return fail(IWAE_ERR_STATE, "the last forward ran in float32 mode");
    const StepPlan& p = m->plan;
    const StepOptions& o = m->opt;
    const bool two = m->cfg.n_layers == 2;
    const int B = m->B, k = m->k, M = m->M, Mp = m->Mp, Bp = m->Bp, X = m->X, Xp = m->Xp32;
    // (planned up front although build_descs may still run below: TableBounds depends on the layers' Kin, Nout and table positions alone, fixed at
    // creation -- a rebuild for new row splits or slab pointers moves no block boundary)
    plan_step_end(m, p, end, m->end);
    const StepEndPlan& e = m->end;
    hipStream_t st = m->stream, tail = on_stream(m, p.tail);
    MlpWs& w = m->wdec1;
    const int Hp = m->dec1[0].Np32;
    CHK(ensure(w.dlP, (size_t)Mp * Xp * 2, st));
    CHK(ensure(w.d2P, (size_t)Mp * Hp * 2, st));
    CHK(ensure(w.d1P, (size_t)Mp * Hp * 2, st));
    CHK(ensure(w.dz, (size_t)Mp * m->Dp[0] * 4, st));
    const bool fused_dx = p.dx != DX_THREE;
    const float* gx_out = ptr<float>(p.lse_dup ? m->gx2 : m->gx);      // the output layer's row weights on `side`: from the side stream's own lse_kernel where it ran one
    {
        Linear& L = m->dec1[2];
        OutBwdArgs a;
        memset(&a, 0, sizeof(a));
        a.G2 = ptr<uint16_t>(w.g2P); a.ldG = L.Kp32; a.img1 = L.imgF; a.img2 = L.imgB;
        a.Xdim = X; a.Xp32 = Xp;
        a.gx = ptr<float>(m->gx); a.XB = ptr<uint16_t>(m->xP); a.ldXB = m->Xinp; a.k = k;
        a.M = M; a.KT = L.KT; a.NG = L.MG;
        a.DPP = ptr<uint16_t>(w.d2P);
        if (p.s_mode) a.SP = ptr<uint16_t>(w.dlP);     // dlP holds s: one product, no recompute
        if (m->fake_s & 1) a.dbg = 32;
        if (p.out_parts) {         // small row counts: one pixel group per block, partial sums + finish kernel
            a.gpb = 1;
            CHK(ensure(m->dg2_part, (size_t)L.MG * M * L.Kp32 * 4, st));
            a.part = ptr<float>(m->dg2_part);
        }
        else a.DLP = ptr<uint16_t>(w.dlP);                // recompute mode: out_bwd writes dl = gx * s there
        if (m->want_stamps && L.KT == 7) {
            CHK(ensure(m->stamps, (size_t)(Mp / 64) * 4 * 8 * 8, st));
            a.stamps = ptr<unsigned long long>(m->stamps);
        }
        if (p.dx == DX_ROWS) {      // few rows: 16-row workgroups, weights straight from L2
            DecBwdRowsArgs r = p.rows;
            r.SP = ptr<uint16_t>(w.dlP); r.G2 = ptr<uint16_t>(w.g2P); r.G1 = ptr<uint16_t>(w.g1P); r.gx = ptr<float>(m->gx);
            r.D2P = ptr<uint16_t>(w.d2P); r.D1P = ptr<uint16_t>(w.d1P);
            r.DZ = ptr<float>(w.dz); r.DZH = p.dz_half ? (uint16_t*)w.dz.p : nullptr;
            if (p.lse_at == LSE_BWD_ROWS) lse_args_parts(m, objective, true, nullptr, r.lse);      // (the forward pass left the log-mean-exp to this kernel)
            ScopedTimer tm(m, T_DEC_BWD);
            launch_dec_bwd_rows(r, st, p.dec_rows ? nullptr : m->ev_fork2);
        } else if (p.dx == DX_DEC_BWD) {      // out_bwd + dX of d2 + dX of d1 in one launch
            DecBwdArgs d;
            memset(&d, 0, sizeof(d));
            d.o = a;
            d.imgB2 = m->dec1[1].imgB; d.G1 = ptr<uint16_t>(w.g1P); d.D1P = ptr<uint16_t>(w.d1P);
            d.imgB1 = m->dec1[0].imgB; d.MG1 = m->dec1[0].MG_B; d.DZ = ptr<float>(w.dz); d.ldDZ = m->dec1[0].Kp32;
            if (p.dz_half) d.DZH = (uint16_t*)w.dz.p;
            d.nw = o.dec_bwd_nw;
            if (m->dstamp_epi == 9) {      // diagnostic (STAMPS=1 build, option dense_stamps_epi = 9): phase stamps of dec_bwd_kernel
                m->dstamp_waves = ((M + 127) / 128) * (L.KT == 7 ? o.dec_bwd_nw : 4);
                CHK(ensure(m->dstamps, (size_t)m->dstamp_waves * 64, st));
                d.o.stamps = ptr<unsigned long long>(m->dstamps);
            }
            ScopedTimer tm(m, T_DEC_BWD);
            launch_dec_bwd(d, st, p.dec_rows ? nullptr : m->ev_fork2);          // dpre2, dpre1 and the last read of the decoder's weight images: one event
        } else {
            // (forked behind lse_kernel already: the side stream then needs nothing from the main stream until dX of d1 is done)
            { ScopedTimer tm(m, T_OUT_BWD); launch_out_bwd(a, st, p.early_wout ? nullptr : m->ev_fork); }
        }
        HIPCHK(hipGetLastError());
    }
    // fork: the decoder weight gradients only need what out_bwd produced (dl, dpre2) plus forward activations, so
    // they start on the side stream right behind it and fill the machine next to the dz -> encoder chain; the
    // first decoder layer's gradient additionally waits for dpre1 (second event).
    hipStream_t sd = m->side;
    if (p.dec_rows) {
        if (!fused_dx) {      // (the dX chain as three launches; their weight gradients follow in wgrad_rows_kernel, further down the main stream)
            { ScopedTimer tm(m, T_DX_HID); CHK(dense_dx(m, m->dec1[1], ptr<uint16_t>(w.d2P), M, ptr<uint16_t>(w.g1P), ptr<uint16_t>(w.d1P), nullptr)); }
            { ScopedTimer tm(m, T_DX_LAT); CHK(dense_dx(m, m->dec1[0], ptr<uint16_t>(w.d1P), M, nullptr, nullptr, ptr<float>(w.dz))); }
        }
    } else if (p.group3) {      // few rows: the decoder's three weight gradients as ONE grouped launch behind the dX chain
        WgradPGroup g3;
        memset(&g3, 0, sizeof(g3));
        Linear* ls[3] = {&m->dec1[2], &m->dec1[1], &m->dec1[0]};
        const uint16_t* xs[3] = {ptr<uint16_t>(w.g2P), ptr<uint16_t>(w.g1P), ptr<uint16_t>(m->zP[0])};
        const uint16_t* gs[3] = {ptr<uint16_t>(w.dlP), ptr<uint16_t>(w.d2P), ptr<uint16_t>(w.d1P)};
        int ns[3], nw[3];
        for (int i = 0; i < 3; ++i) {
            CHK(wgradp_plan(m, *ls[i], xs[i], gs[i], M, g3.a[i], ns[i], nw[i]));
            g3.gx[i] = (ls[i]->JT + 7) / 8; g3.gy[i] = (ls[i]->IT + 15) / 16;
            g3.zbeg[i + 1] = g3.zbeg[i] + ns[i];
        }
        g3.n = 3;
        g3.a[0].rowscale = ptr<float>(m->gx);      // (the main stream's row weights: this group waits for ev_fork2, i.e. for the main stream -- never the side stream's copy)
        HIPCHK(hipStreamWaitEvent(m->side2, m->ev_fork2, 0));
        { ScopedTimer tm(m, T_WGRAD_OUT, m->side2); launch_wgradp_group(g3, m->side2); }
        HIPCHK(hipGetLastError());
    } else {
    const bool wout_beside = p.early_wout && p.hid_on == ON_SIDE2;      // the output layer's gradient on `side`, the hidden layers' beside it on `side2`
    if (p.early_wout && (p.lse_dup || p.lse_fused)) {}                            // forked behind the decoder kernel already (forward_impl)
    else if (p.early_wout) HIPCHK(hipStreamWaitEvent(m->side, m->ev_lse, 0));            // forked behind lse_kernel (forward_impl)
    else HIPCHK(hipStreamWaitEvent(m->side, fused_dx ? m->ev_fork2 : m->ev_fork, 0));  // the event rode on out_bwd's / dec_bwd's dispatch packet
    {   // (its completion event ev_s2 rides on the dispatch packet: the stream that later picks `side` up waits ~8 us less than behind a record)
        ScopedTimer tm(m, T_WGRAD_OUT, sd);
        if (p.wout_two_part) {
            WgradPArgs a1, a2;
            int n1 = 1, n2 = 1;
            CHK(wgradp_two_plan(m, m->dec1[2], ptr<uint16_t>(w.g2P), ptr<uint16_t>(w.dlP), M, gx_out, a1, n1, a2, n2));
            launch_wgradp(a1, n1, 7, sd);
            HIPCHK(hipStreamWaitEvent(sd, m->ev_fork2, 0));      // (the late part starts behind dec_bwd_kernel, beside the hidden layers' gradients)
            launch_wgradp(a2, n2, 7, sd, m->ev_s2);
            HIPCHK(hipGetLastError());
        } else if (m->abl_skip & 1) {      // (DIAG builds, timing only: slabs allocated, the reduction still reads them)
            if (wout_beside) HIPCHK(hipEventRecord(m->ev_s2, sd));
            WgradPArgs a0; int n0 = 1, w0 = 8; CHK(wgradp_plan(m, m->dec1[2], ptr<uint16_t>(w.g2P), ptr<uint16_t>(w.dlP), M, a0, n0, w0));
        } else {
            const hipEvent_t done = wout_beside ? m->ev_s2 : nullptr;
            if (p.g2w) CHK(wgradp(m, m->dec1[2], ptr<uint16_t>(w.g2wP), ptr<uint16_t>(w.dlP), M, sd, nullptr, done));      // (pre-weighted X operand: the unweighted kernel)
            else CHK(wgradp(m, m->dec1[2], ptr<uint16_t>(w.g2P), ptr<uint16_t>(w.dlP), M, sd, p.s_mode ? gx_out : nullptr, done));
        }
    }
    if (!fused_dx) {
        { ScopedTimer tm(m, T_DX_HID); CHK(dense_dx(m, m->dec1[1], ptr<uint16_t>(w.d2P), M, ptr<uint16_t>(w.g1P), ptr<uint16_t>(w.d1P), nullptr)); }
        { ScopedTimer tm(m, T_DX_LAT); CHK(dense_dx(m, m->dec1[0], ptr<uint16_t>(w.d1P), M, nullptr, nullptr, ptr<float>(w.dz), m->ev_fork2)); }
    }
    // ONE event (ev_fork2) behind the whole dX chain -- the last of its kernels carries it on its dispatch packet (every separate
    // record costs the main stream a ~6 us bubble): the hidden layers' weight gradients need dpre2 and dpre1, and the deferred
    // decoder update further down the side stream must come after dX of d1, the last reader of the decoder's weight images.
    // Forked early, the side stream is busy with the output layer's gradient until after that: ONE wait then covers everything,
    // and out_bwd carries no event at all -- one bubble less on the main stream, one wait less on the side stream.
    // The hidden layers' weight gradients go to the stream the plan names (p.hid_on: beside the output layer's on `side2`, or behind it) -- as
    // ONE grouped launch where both take the specialised-wave shape.  They finish last, so that stream (`tail`) also carries what follows the
    // weight gradients (the decoder's slab reduction [+ exchange] + Adam): it picks up `side` (ev_s2, recorded behind the output
    // layer's gradient, long complete by then) instead of `side` picking up the later of the two.
    hipStream_t ws = on_stream(m, p.hid_on);
    if (p.early_wout) HIPCHK(hipStreamWaitEvent(ws, m->ev_fork2, 0));
    {
        WgradPArgs ah, al;
        int nsh = 1, nsl = 1, shh = 8, shl = 8;
        CHK(wgradp_plan(m, m->dec1[1], ptr<uint16_t>(w.g1P), ptr<uint16_t>(w.d2P), M, ah, nsh, shh));
        CHK(wgradp_plan(m, m->dec1[0], ptr<uint16_t>(m->zP[0]), ptr<uint16_t>(w.d1P), M, al, nsl, shl));
        if (p.hid_group) {
            WgradPGroup g;
            memset(&g, 0, sizeof(g));
            g.n = 2; g.a[0] = ah; g.a[1] = al;
            g.gx[0] = (m->dec1[1].JT + 15) / 16; g.gx[1] = (m->dec1[0].JT + 15) / 16; g.gy[0] = g.gy[1] = 1;
            g.zbeg[0] = 0; g.zbeg[1] = nsh; g.zbeg[2] = nsh + nsl;
            ScopedTimer tm(m, T_WGRAD_HID, ws);
            launch_wgradws_group(g, ws);
        } else {
            if (!(m->abl_skip & 2)) { ScopedTimer tm(m, T_WGRAD_HID, ws); launch_wgradp(ah, nsh, shh, ws); }
            if (!p.early_wout && !fused_dx) HIPCHK(hipStreamWaitEvent(m->side, m->ev_fork2, 0));
            if (!(m->abl_skip & 2)) { ScopedTimer tm(m, T_WGRAD_LAT, ws); launch_wgradp(al, nsl, shl, ws); }
        }
        HIPCHK(hipGetLastError());
    }
    if (p.hid_on == ON_SIDE2 && e.how != ENDS_SPLIT_UPD) HIPCHK(hipStreamWaitEvent(m->side2, m->ev_s2, 0));
    }      // (!group3)
    const float alpha = e.update ? adam_alpha(m, lr) : 0.0f;
    if (m->descs_dirty) CHK(build_descs(m));

    const float* dz1 = ptr<float>(w.dz);
    const float *dz1_b = nullptr, *dz1_c = nullptr;
    bool dz_sum_half = false;      // 2-layer model, fused block backward: the three terms of dz1 arrive summed, as bf16, in dzdir
    if (two) {
        // ---- p(z1|z2) head, dec2, q(z2|z1) head, enc2
        CHK(ensure(m->dzdir, (size_t)Mp * m->Dp[0] * 4, st));
        if (p.chain2_bwd) {
            // one launch per block: the head recomputed from h2, its gradient, the block's dX chain (gblock_bwd_kernel); the second one
            // also sums the three terms of dz1 (bf16, in dzdir) -- latent_bwd_kernel reads that like the 1-layer step's dz
            GBlockBwdArgs gb;
            memset(&gb, 0, sizeof(gb));
            gb.imgH = m->dec2[2].imgF; gb.imgBh = m->dec2[2].imgB; gb.imgB2 = m->dec2[1].imgB; gb.imgB1 = m->dec2[0].imgB;
            gb.H2 = ptr<uint16_t>(m->wdec2.h2P); gb.H1 = ptr<uint16_t>(m->wdec2.h1P); gb.gx = ptr<float>(m->gx);
            gb.M = M; gb.k = k; gb.B = B; gb.D = m->D[0]; gb.eps = eps_src(m, 0);
            gb.head1 = ptr<float>(m->wenc1.head); gb.ldH1 = 2 * m->Dp[0];
            gb.DHP = ptr<uint16_t>(m->wdec2.dheadP); gb.D2P = ptr<uint16_t>(m->wdec2.d2P); gb.D1P = ptr<uint16_t>(m->wdec2.d1P);
            gb.DZ2 = ptr<float>(m->wdec2.dx); gb.DZD = (uint16_t*)m->wenc2.dx.p;
            launch_gblock_bwd(0, gb, st, m->ev_blk);
            CHK(block_bwd(m, m->dec2, m->wdec2, ptr<uint16_t>(m->zP[1]), M, false, true, true));
            memset(&gb, 0, sizeof(gb));
            gb.imgH = m->enc2[2].imgF; gb.imgBh = m->enc2[2].imgB; gb.imgB2 = m->enc2[1].imgB; gb.imgB1 = m->enc2[0].imgB;
            gb.H2 = ptr<uint16_t>(m->wenc2.h2P); gb.H1 = ptr<uint16_t>(m->wenc2.h1P); gb.gx = ptr<float>(m->gx);
            gb.M = M; gb.k = k; gb.B = B; gb.D = m->D[1]; gb.eps = eps_src(m, 1);
            gb.DZIN = ptr<float>(m->wdec2.dx);
            gb.DHP = ptr<uint16_t>(m->wenc2.dheadP); gb.D2P = ptr<uint16_t>(m->wenc2.d2P); gb.D1P = ptr<uint16_t>(m->wenc2.d1P);
            gb.DZD = (uint16_t*)m->wenc2.dx.p; gb.DZDEC = ptr<float>(w.dz); gb.ldDZDEC = m->dec1[0].Kp32; gb.DZOUT = (uint16_t*)m->dzdir.p;
            launch_gblock_bwd(1, gb, st, m->ev_blk);
            // (the encode block's weight gradients on the second side stream, free by now: beside the decode block's, not behind them)
            CHK(block_bwd(m, m->enc2, m->wenc2, ptr<uint16_t>(m->zP[0]), M, false, true, true, p.hid_on == ON_SIDE2 ? m->side2 : nullptr));
            HIPCHK(hipGetLastError());
            dz1 = nullptr; dz_sum_half = true;
        } else {
        GaussBwdArgs g;
        memset(&g, 0, sizeof(g));
        g.mode = 0; g.G = ptr<float>(m->gx);
        g.head = ptr<float>(m->wdec2.head); g.ldH = 2 * m->Dp[0]; g.D = m->D[0]; g.Dp = m->Dp[0];
        g.zhead = ptr<float>(m->wenc1.head); g.ldZH = 2 * m->Dp[0]; g.Dzp = m->Dp[0];
        g.dz_direct = ptr<float>(m->dzdir); g.ldDZ = m->Dp[0];
        g.eps = eps_src(m, 0); g.M = M; g.Mp = Mp; g.k = k;
        g.DHP = ptr<uint16_t>(m->wdec2.dheadP);
        launch_gauss_bwd(g, st);
        CHK(block_bwd(m, m->dec2, m->wdec2, ptr<uint16_t>(m->zP[1]), M, true, true));
        memset(&g, 0, sizeof(g));
        g.mode = 1; g.G = ptr<float>(m->gx);
        g.head = ptr<float>(m->wenc2.head); g.ldH = 2 * m->Dp[1]; g.D = m->D[1]; g.Dp = m->Dp[1];
        g.dz_in = ptr<float>(m->wdec2.dx); g.ldDZ = m->Dp[1];
        g.eps = eps_src(m, 1); g.M = M; g.Mp = Mp; g.k = k;
        g.DHP = ptr<uint16_t>(m->wenc2.dheadP);
        launch_gauss_bwd(g, st);
        CHK(block_bwd(m, m->enc2, m->wenc2, ptr<uint16_t>(m->zP[0]), M, true, true));
        dz1_b = ptr<float>(m->dzdir); dz1_c = ptr<float>(m->wenc2.dx);     // summed inside latent_bwd_kernel
        }
    }
    LatentBwdArgs lat_args;
    {
        LatentBwdArgs a;
        memset(&a, 0, sizeof(a));
        a.dz = dz1; a.dz2 = dz1_b; a.dz3 = dz1_c; a.ldDZ = m->Dp[0];
        if (p.dz_half) a.dzh = (const uint16_t*)w.dz.p;
        if (dz_sum_half) a.dzh = (const uint16_t*)m->dzdir.p;
        a.head = ptr<float>(m->wenc1.head); a.ldH = 2 * m->Dp[0]; a.D = m->D[0]; a.Dp = m->Dp[0];
        a.cf = ptr<float4>(m->cf); a.eps = eps_src(m, 0);
        a.B = B; a.Bp = Bp; a.k = k;
        a.kmu = a.ksig = (objective == OBJ_VAE_ELBO_KL) ? m->beta / (float)B : 0.f;
        a.DHP = ptr<uint16_t>(m->wenc1.dheadP);
        if (m->has_prior) { a.prior_head = ptr<float>(m->wprior.head); a.DHP2 = ptr<uint16_t>(m->wprior.dheadP); }
        lat_args = a;
        // (few images and samples: the encoder's block_bwd_kernel makes these sums itself, below)
        if (!p.lat_fuse && !(m->abl_skip & 8)) { ScopedTimer tm(m, T_LATENT_BWD); launch_latent_bwd(a, st); }
    }
    if (m->has_prior) CHK(block_bwd(m, m->prior, m->wprior, ptr<uint16_t>(m->condP), B, false, false));
    CHK(block_bwd(m, m->enc1, m->wenc1, ptr<uint16_t>(m->xP), B, false, false, false, nullptr, p.rows_enc, p.lat_fuse ? &lat_args : nullptr));
    if (m->descs_dirty) CHK(build_descs(m));      // (the encoder's splits were planned after the first build)
    // ---- the end of the step, as planned (StepEndPlan): optional join, the main stream's sums, per side stream at most one wait and one launch
    // split (data-parallel step, iwae_forward_backward_split): the decoder's layers are summed into the flat gradient on the
    // side stream, right behind their weight gradients, and NOT joined here -- the caller's all-reduce of that segment is
    // ordered behind the side stream and runs beside the encoder's backward pass; join_side() (every later entry point) joins.
    // Without split (iwae_forward_backward: gradient only, e.g. the one-message data-parallel step) the same early decoder
    // reduction runs on the side stream and the main stream joins it behind its own, shorter, encoder reduction.
    // (2-layer deferred update: the next forward joins in front of z1 (join_side).  The image rewrite is safe for the same reason as in the 1-layer
    // step: the side streams' weight gradients wait for the events behind the dX chains (ev_fork2, ev_blk), the last readers of those images.)
    const bool side_first = e.how == ENDS_EARLY || e.how == ENDS_EARLY_SPLIT;      // (gradient only: the decoder's slabs are ready first, its sums are enqueued first)
    auto side_sums = [&]() -> int {
        for (int i = 0; i < e.nside; ++i) {
            const SideSum& s = e.side[i];
            hipStream_t ss = on_stream(m, s.on);
            if (s.behind == WAIT_FORK2) HIPCHK(hipStreamWaitEvent(ss, m->ev_fork2, 0));
            if (s.behind == WAIT_SIDE) { HIPCHK(hipEventRecord(m->ev_join2, m->side)); HIPCHK(hipStreamWaitEvent(ss, m->ev_join2, 0)); }
            if (e.how == ENDS_DEFER && (m->abl_skip & 4)) HIPCHK(hipEventRecord(m->ev_dec, ss));      // (DIAG builds, timing only: no deferred reduction + update)
            else reduce_blocks(m, ss, s.a, s.b, alpha, e.update, s.second_event ? m->ev_dec2 : m->ev_dec, false);
        }
        return IWAE_OK;
    };
    if (e.how == ENDS_JOINED) {
        HIPCHK(hipEventRecord(m->ev_join, tail));
        HIPCHK(hipStreamWaitEvent(st, m->ev_join, 0));
        if (e.join_both) { HIPCHK(hipEventRecord(m->ev_join2, m->side)); HIPCHK(hipStreamWaitEvent(st, m->ev_join2, 0)); }
    }
    if (side_first) CHK(side_sums());
    {   // (wgrad_rows_kernel's extra block makes the batch means whenever it runs, else the reduction's)
        ScopedTimer tm_red(m, T_REDUCE);
        if (p.rows_enc) CHK(block_wgrad_rows(m, m->enc1, m->wenc1, ptr<uint16_t>(m->xP), B, alpha, e.update, true, p.dec_rows));
        if (!p.rows_enc || e.main_a.count + e.main_b.count > 0) reduce_blocks(m, st, e.main_a, e.main_b, alpha, e.update, nullptr, !p.rows_enc);
    }
    if (e.how == ENDS_EARLY) HIPCHK(hipStreamWaitEvent(st, m->ev_dec, 0));
    if (!side_first && e.how != ENDS_EARLY_HELD) CHK(side_sums());
    m->left = e.left;
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

}  // namespace -- adam_impl: external (hidden) linkage, declared in model.h, step_f32.hip calls it too
int adam_impl(iwae_model* m, float lr, float gscale) {
    if (m->descs_dirty) CHK(build_descs(m));
    const float alpha = adam_alpha(m, lr);
    adam_blocks(m, m->stream, 0, m->tb.end.e, alpha, gscale);
    HIPCHK(hipGetLastError());
    return IWAE_OK;
}
namespace {      // (internal linkage again)

// Data-parallel step, second half (the gradient of this rank's shard is in m->grad; backward_impl(END_GRAD_SPLIT_HELD) left the decoder's
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

}  // namespace

// ---------------------------------------------------------------- helpers analysis.hip calls too (declared in model.h)
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
    if (m->cfg.precision == IWAE_PREC_FP32) CHK(forward_f32(m, x, B, k, beta, eps, OBJ_IWAE_ELBO, false, want, FwdCall{m->batch_offset}));
    else CHK(forward_impl(m, x, B, k, beta, eps, OBJ_IWAE_ELBO, false, want, FwdCall{m->batch_offset}));
    CHK(fetch_outputs(m, scalars, want));
    m->noise_step += 1;
    return IWAE_OK;
}

int iwae_forward_backward(iwae_handle m, const float* x, int32_t B, int32_t k, float beta, int32_t objective, const float* eps,
                          iwae_scalars* scalars, const iwae_tensors* want) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    HIPCHK(hipSetDevice(m->cfg.device));
    CHK(check_objective(m, objective));
    if (m->cfg.precision == IWAE_PREC_FP32) {
        CHK(forward_f32(m, x, B, k, beta, eps, objective, true, want, FwdCall{m->batch_offset}));
        CHK(backward_f32(m, objective, END_GRAD));
    } else {
        CHK(forward_impl(m, x, B, k, beta, eps, objective, true, want, FwdCall{m->batch_offset}));
        CHK(backward_impl(m, objective, END_GRAD));
    }
    CHK(fetch_outputs(m, scalars, want));
    m->noise_step += 1;
    return IWAE_OK;
}

int iwae_forward_backward_split(iwae_handle m, const float* x, int32_t B, int32_t k, float beta, int32_t objective, const float* eps,
                                void** side_stream, size_t* side_offset) {
    if (!m || !side_stream || !side_offset) return fail(IWAE_ERR_ARG, "null argument");
    HIPCHK(hipSetDevice(m->cfg.device));
    CHK(check_objective(m, objective));
    if (m->cfg.precision == IWAE_PREC_FP32) {       // float32 mode: nothing is left on the side stream (*side_offset = n)
        CHK(forward_f32(m, x, B, k, beta, eps, objective, true, nullptr, FwdCall{m->batch_offset}));
        CHK(backward_f32(m, objective, END_GRAD_SPLIT));
        CHK(join_side(m));
    } else {
        CHK(forward_impl(m, x, B, k, beta, eps, objective, true, nullptr, FwdCall{m->batch_offset}));
        CHK(backward_impl(m, objective, END_GRAD_SPLIT));
    }
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
    if (m->cfg.precision == IWAE_PREC_FP32) {   // float32 mode: forward, closed-form backward, [exchange,] Adam -- all in float32
        CHK(forward_f32(m, x, B, k, beta, eps, objective, true, want, FwdCall{m->batch_offset}));
        if (m->comm_main || want) {
            CHK(backward_f32(m, objective, m->comm_main ? END_GRAD_SPLIT_HELD : END_GRAD));
            if (want) CHK(fetch_outputs(m, nullptr, want));      // tensors refer to the pre-update forward (src/iwae1.py:162)
            if (m->comm_main) CHK(dp_finish(m, lr));
            else { CHK(join_side(m)); CHK(adam_impl(m, lr, 1.0f)); }
        } else {
            CHK(backward_f32(m, objective, END_UPDATE, lr));   // the update rides behind the gradients, the decoder's on the side stream (deferred)
        }
        CHK(fetch_outputs(m, scalars, nullptr));
        m->noise_step += 1;
        return IWAE_OK;
    }
    CHK(forward_impl(m, x, B, k, beta, eps, objective, true, want, FwdCall{m->batch_offset}));
    if (m->comm_main) {                         // data-parallel step: exchange between gradient and update (iwae_comm_init)
        CHK(backward_impl(m, objective, END_GRAD_SPLIT_HELD));
        if (want) CHK(fetch_outputs(m, nullptr, want));
        CHK(dp_finish(m, lr));
    } else if (want) {
        CHK(backward_impl(m, objective, END_GRAD));
        CHK(fetch_outputs(m, nullptr, want));   // tensors refer to the pre-update forward (src/iwae1.py:162)
        CHK(adam_impl(m, lr, 1.0f));
    } else {
        CHK(backward_impl(m, objective, END_UPDATE, lr));   // Adam fused into the gradient reduction
    }
    CHK(fetch_outputs(m, scalars, nullptr));
    m->noise_step += 1;
    return IWAE_OK;
}

// ---- the masked step (DESIGN.md sections 19, 20): the unmasked entry points' branches of either precision with FwdCall::mask set
namespace {
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
int train_step_masked_call(iwae_model* m, const float* x, int B, int k, float beta, float lr, int objective, const float* eps, iwae_scalars* scalars,
                           const iwae_tensors* want, const FwdCall& call);
}  // namespace

int iwae_forward_masked(iwae_handle m, const float* x, const uint8_t* mask, int32_t B, int32_t k, float beta, const float* eps, iwae_scalars* scalars,
                        const iwae_tensors* want) {
    if (!m) return fail(IWAE_ERR_ARG, "null handle");
    if (!mask) return iwae_forward(m, x, B, k, beta, eps, scalars, want);
    HIPCHK(hipSetDevice(m->cfg.device));
    CHK(masked_scope(m, "forward_masked", x, B, k, want));
    FwdCall call{m->batch_offset};
    call.mask = mask;
    if (m->cfg.precision == IWAE_PREC_FP32) CHK(forward_f32(m, x, B, k, beta, eps, OBJ_IWAE_ELBO, false, want, call));
    else CHK(forward_impl(m, x, B, k, beta, eps, OBJ_IWAE_ELBO, false, want, call));
    CHK(fetch_outputs(m, scalars, want));
    m->noise_step += 1;
    return IWAE_OK;
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
    if (m->cfg.precision == IWAE_PREC_FP32) {
        CHK(forward_f32(m, x, B, k, beta, eps, objective, true, want, call));
        CHK(backward_f32(m, objective, END_GRAD));
    } else {
        CHK(forward_impl(m, x, B, k, beta, eps, objective, true, want, call));
        CHK(backward_impl(m, objective, END_GRAD));
    }
    CHK(fetch_outputs(m, scalars, want));
    m->noise_step += 1;
    return IWAE_OK;
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
    return train_step_masked_call(m, x, B, k, beta, lr, objective, eps, scalars, want, call);
}

namespace {
// the masked train step behind its checks: the caller's mask (iwae_train_step_masked) or the resident set's (iwae_train_step_dataset)
int train_step_masked_call(iwae_model* m, const float* x, int B, int k, float beta, float lr, int objective, const float* eps, iwae_scalars* scalars,
                           const iwae_tensors* want, const FwdCall& call) {
    if (m->cfg.precision != IWAE_PREC_FP32) {      // iwae_train_step's single-device bf16 branch
        CHK(forward_impl(m, x, B, k, beta, eps, objective, true, want, call));
        if (want) {
            CHK(backward_impl(m, objective, END_GRAD));
            CHK(fetch_outputs(m, nullptr, want));   // tensors refer to the pre-update forward (src/iwae1.py:162)
            CHK(adam_impl(m, lr, 1.0f));
        } else {
            CHK(backward_impl(m, objective, END_UPDATE, lr));   // Adam fused into the gradient reduction
        }
        CHK(fetch_outputs(m, scalars, nullptr));
        m->noise_step += 1;
        return IWAE_OK;
    }
    CHK(forward_f32(m, x, B, k, beta, eps, objective, true, want, call));
    if (want) {
        CHK(backward_f32(m, objective, END_GRAD));
        CHK(fetch_outputs(m, nullptr, want));      // tensors refer to the pre-update forward (src/iwae1.py:162)
        CHK(join_side(m));
        CHK(adam_impl(m, lr, 1.0f));
    } else {
        CHK(backward_f32(m, objective, END_UPDATE, lr));
    }
    CHK(fetch_outputs(m, scalars, nullptr));
    m->noise_step += 1;
    return IWAE_OK;
}
}  // namespace

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
            rc = eval_f32 ? forward_f32(m, xd + (size_t)i0 * m->X, nb, kn, 1.0f, nullptr, OBJ_IWAE_ELBO, false, nullptr, call)
                          : forward_impl(m, xd + (size_t)i0 * m->X, nb, kn, 1.0f, nullptr, OBJ_IWAE_ELBO, false, nullptr, call);
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
    const bool f32 = m->cfg.precision == IWAE_PREC_FP32;
    const size_t n = m->nparam;
    hipStream_t st = m->stream;
    iwae_model::MomWs& w = m->mom_ws;
    const float* xd;
    CHK(staged_in(m, x, m->ev.x, (size_t)B * m->X * 4, &xd));        // uploaded once: every draw reads the images in place
    CHK(ensure(w.mean, n * 8, st));
    CHK(ensure(w.m2, n * 8, st));
    for (int j = 0; j < M; ++j) {
        if (f32) {
            CHK(forward_f32(m, xd, B, k, beta, nullptr, objective, true, nullptr, FwdCall{m->batch_offset}));
            CHK(backward_f32(m, objective, END_GRAD));
        } else {
            CHK(forward_impl(m, xd, B, k, beta, nullptr, objective, true, nullptr, FwdCall{m->batch_offset}));
            CHK(backward_impl(m, objective, END_GRAD));
        }
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
    if (!m || !x_out || m->ds_N <= 0 || start < 0 || B <= 0 || start + B > m->ds_N) return fail(IWAE_ERR_ARG, "dataset_get_batch: bad range");
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
    if (!m || !y_out || m->ds_N <= 0 || start < 0 || B <= 0 || start + B > m->ds_N) return fail(IWAE_ERR_ARG, "dataset_get_labels: bad range");
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
    if (!m || !mask_out || m->ds_N <= 0 || start < 0 || B <= 0 || start + B > m->ds_N) return fail(IWAE_ERR_ARG, "dataset_get_mask: bad range");
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
    if (start < 0 || B <= 0 || start + B > m->ds_N) return fail(IWAE_ERR_ARG, "train_step_dataset: batch range outside the dataset");
    int rc;
    if (m->ds_has_mask) {      // iwae_train_step_masked on (iwae_dataset_get_batch, iwae_dataset_get_mask) of these rows, fed on the device
        HIPCHK(hipSetDevice(m->cfg.device));
        CHK(masked_scope(m, "train_step_dataset", nullptr, B, k, nullptr, true));
        CHK(check_objective(m, objective));
        FwdCall call{m->batch_offset};
        call.mask_resident = true;
        m->ds_start = start;
        rc = train_step_masked_call(m, nullptr, B, k, beta, lr, objective, nullptr, scalars, nullptr, call);
    } else {
        m->ds_start = start;
        rc = iwae_train_step(m, nullptr, B, k, beta, lr, objective, nullptr, scalars, nullptr);
    }
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
