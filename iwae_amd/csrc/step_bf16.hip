// The bf16 step (iwae_config.precision = IWAE_PREC_BF16): host code; kernels in kernels.hip (forward and dX), wgrad_kernels.hip, update_kernels.hip
// and row_kernels.hip.  plan_step decides the step's kernels and streams once and plan_step_end how it ends; forward_impl and backward_impl
// execute what they decided.  The step driver in model.hip (step_forward / step_backward) is their only caller.
#include <string.h>
#include <algorithm>
#include "model.h"       // (the HIP runtime, include/iwae_amd.h and kernels.h come with it)
#include "layout.h"

using namespace iwae;

namespace {

// table order enc1 | enc2 | dec2 | dec1 [| prior]: are the decoder's three layers (one table entry each) the tail of the table / does the
// 2-layer model's share of it start with the per-sample encoder?  (plan_step_end asks: only then do TableBounds::dec1 / enc2 open a side stream's range)
bool dec_layers_last(const iwae_model* m) {
    const int d0 = m->dec1[0].sub[0];
    return m->dec1[0].nsub == 1 && m->dec1[1].nsub == 1 && m->dec1[2].nsub == 1 && m->dec1[1].sub[0] == d0 + 1 && m->dec1[2].sub[0] == d0 + 2 && d0 + 3 == (int)m->klayers.size();
}
bool side_layers_from_enc2(const iwae_model* m) { return m->cfg.n_layers == 2 && m->enc2[0].nsub >= 1; }

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

}  // namespace

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

// end: how the step ends (StepEnd); lr: Adam's learning rate where that is END_UPDATE.  plan_step_end decides everything about it up front
int backward_impl(iwae_model* m, int objective, StepEnd end, float lr) {
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
