// What more than one kernel file of the bf16 train / eval step needs (kernels.hip, row_kernels.hip, wgrad_kernels.hip, update_kernels.hip): no
// kernels; include it after device_helpers.h.
// bern_pipe_kernel, dec_bwd_rows_kernel and lse_kernel must produce the same log-mean-exp bit for bit (lse_image), and every kernel that
// makes z runs the same sample_step: each exists once, here.  They take LseArgs / SampleArgs / EpsSrc and are of no use to the analysis
// kernels, hence not device_helpers.h.  Also here: the counted vector-memory wait (wgradws_kernel in wgrad_kernels.hip, wgrad_rows_kernel in
// update_kernels.hip) and the launch helper that puts a completion event on a kernel's dispatch packet (host side).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include "kernels.h"
#include "layout.h"
#include "device_helpers.h"

// diagnostic ablations of the weight-gradient kernels (WgradPArgs.dbg: timing only, results are wrong) exist in DIAG=1 builds only;
// in the shipped kernels the conditions fold to false at compile time
#ifdef IWAE_DIAG
#define WG_DBG(a, bit) (((a).dbg & (bit)) != 0)
#else
#define WG_DBG(a, bit) false
#endif

// diagnostic build only (./build.sh with STAMPS=1): per-phase s_memtime sums per wave -> a.stamps[wave][8]
#ifdef IWAE_DENSE_STAMPS
#define DS_STAMP(slot)                                                                 \
    {                                                                                  \
        unsigned long long t_;                                                         \
        __builtin_amdgcn_sched_barrier(0);                                             \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");     \
        __builtin_amdgcn_sched_barrier(0);                                             \
        ds_sum[slot] += t_ - ds_prev;                                                  \
        ds_prev = t_;                                                                  \
    }
#else
#define DS_STAMP(slot)
#endif

namespace iwae {

// 4 consecutive eps values for features 4*d4 .. 4*d4+3 of data row (b,s)
__device__ __forceinline__ void eps4(const EpsSrc& e, int b, int s, int row, int d4, int D, float n[4]) {
    if (e.cache) {
        const float4 v = *(const float4*)(e.cache + (size_t)row * e.ldC + 4 * d4);
        n[0] = v.x; n[1] = v.y; n[2] = v.z; n[3] = v.w;
    } else if (e.user) {
        const float* p = e.user + ((size_t)s * e.B + b) * D + 4 * d4;
#pragma unroll
        for (int i = 0; i < 4; ++i) n[i] = (4 * d4 + i < D) ? p[i] : 0.0f;
    } else {
        const uint64_t grow = e.k_total ? e.row_offset + (uint64_t)b * (uint64_t)e.k_total + (uint64_t)(e.s_off + s) : e.row_offset + (uint64_t)row;
        normal4(grow, (uint32_t)d4, e.stream, e.step, e.seed, n);
    }
}

// One 32-feature step t of z = mu + sigma*eps for the lane's (row, quad): the lane's 8 features of P-layout chunk 4t+q (features
// 32t+4q..+3 and 32t+16+4q..+3) and their contributions to the row's log-densities (sample_kernel; block_fwd_kernel's sampling mode)
__device__ __forceinline__ void sample_step(const SampleArgs& a, int t, int q, int rowc, int b, int s, const float* hd, float z8[8], float& lp, float& lq, float& lq2) {
    // Round 5: the density arithmetic in the decoder kernel's new form -- a density scored at its own sample has (z - mu)/sigma = eps, the
    // chunks that straddle or lie beyond the latent width take a wave-uniform masked path instead of a branch per element, and the
    // log-scales are summed as log2 of pair products (one v_log per 2 elements; __logf was ~12 instructions per element).  The k = 5000
    // evaluator's sampling pass is this function behind Philox + Box-Muller: 107 us per 520 k rows before.
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int f0 = 32 * t + 16 * h + 4 * q;
        float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        float4 mu4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), sg4 = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        float4 pm4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), ps4 = make_float4(1.0f, 1.0f, 1.0f, 1.0f);     // prior: N(0,1) unless a head is given
        if (f0 < a.D) {
            eps4(a.eps, b, s, rowc, f0 >> 2, a.D, e);
            mu4 = *(const float4*)(hd + f0);
            sg4 = *(const float4*)(hd + a.Dp + f0);
            if (a.prior_head) {      // learned conditional prior p(z|y) of tasks/task04.py:124-130, one head per image
                pm4 = *(const float4*)(a.prior_head + (size_t)b * a.ldH + f0);
                ps4 = *(const float4*)(a.prior_head + (size_t)b * a.ldH + a.Dp + f0);
            }
        }
        float muv[4] = {mu4.x, mu4.y, mu4.z, mu4.w}, sgv[4] = {sg4.x, sg4.y, sg4.z, sg4.w};
        float pmv[4] = {pm4.x, pm4.y, pm4.z, pm4.w}, psv[4] = {ps4.x, ps4.y, ps4.z, ps4.w};
        float cnt = 4.0f;                                     // valid features of this chunk
        const bool ragged = 32 * t + 16 * h + 16 > a.D;      // wave-uniform where t is (sample_kernel, block_fwd_kernel's sampling mode)
        if (ragged) {
            cnt = (float)max(0, min(4, a.D - f0));
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool in = f0 + i < a.D;
                e[i] = in ? e[i] : 0.0f; muv[i] = in ? muv[i] : 0.0f; sgv[i] = in ? sgv[i] : 1.0f;
                pmv[i] = in ? pmv[i] : 0.0f; psv[i] = in ? psv[i] : 1.0f;
            }
        }
        float sz = 0.0f, se = 0.0f, su = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float z = muv[i] + sgv[i] * e[i];                  // iwae1.py:59 (pad features: exactly 0)
            se = fmaf(e[i], e[i], se);                               // iwae1.py:109: (z - mu)/sigma = eps
            if (a.prior_head) {
                const float up = (z - pmv[i]) * __builtin_amdgcn_rcpf(psv[i]);
                sz = fmaf(up, up, sz);                               // task04.py:130
            } else sz = fmaf(z, z, sz);                              // iwae1.py:107
            if (a.lq_dreg) {                                         // tasks/task02.py:63-65: scale sigma + 1e-6
                const float u2 = (sgv[i] * __builtin_amdgcn_rcpf(sgv[i] + 1e-6f)) * e[i];
                su = fmaf(u2, u2, su);
            }
            z8[4 * h + i] = z;
        }
        if (a.cond && ragged) {      // decoder input = concat(z, y): the condition sits in the pad features behind D
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (f0 + i >= a.D && f0 + i < a.D + a.C) z8[4 * h + i] = a.cond[(size_t)b * a.C + (f0 + i - a.D)];
        }
        const float c0 = -0.5f * LOG2PI_F * cnt;
        lp += fmaf(-0.5f, sz, c0) - (a.prior_head ? LN2_F * (log2_raw(psv[0] * psv[1]) + log2_raw(psv[2] * psv[3])) : 0.0f);
        lq += fmaf(-0.5f, se, c0) - LN2_F * (log2_raw(sgv[0] * sgv[1]) + log2_raw(sgv[2] * sgv[3]));
        if (a.lq_dreg) {
            const float s20 = sgv[0] + 1e-6f, s21 = sgv[1] + 1e-6f, s22 = sgv[2] + 1e-6f, s23 = sgv[3] + 1e-6f;
            const float m0 = ragged && !(f0 + 0 < a.D) ? 1.0f : s20, m1 = ragged && !(f0 + 1 < a.D) ? 1.0f : s21;
            const float m2 = ragged && !(f0 + 2 < a.D) ? 1.0f : s22, m3 = ragged && !(f0 + 3 < a.D) ? 1.0f : s23;
            lq2 += fmaf(-0.5f, su, c0) - LN2_F * (log2_raw(m0 * m1) + log2_raw(m2 * m3));
        }
    }
}

// Wave-wide sum / max through the DPP path (row_shr 1, 2, 4, 8, then row_bcast 15 and 31: the total arrives in lane 63 and is handed to
// every lane through an SGPR): six vector instructions of ~10 cycles each, where the ds_bpermute butterfly of __shfl_xor is six LDS
// round trips of ~100 -- lse_image is four such reductions deep, on the tail of the decoder kernel.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ float dpp_or(float old, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL, ROWMASK, 0xf, false));
}
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp_or<0x111, 0xf>(0.0f, v); v += dpp_or<0x112, 0xf>(0.0f, v); v += dpp_or<0x114, 0xf>(0.0f, v); v += dpp_or<0x118, 0xf>(0.0f, v);
    v += dpp_or<0x142, 0xa>(0.0f, v);
    v += dpp_or<0x143, 0xc>(0.0f, v);
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp_or<0x111, 0xf>(-INFINITY, v)); v = fmaxf(v, dpp_or<0x112, 0xf>(-INFINITY, v));
    v = fmaxf(v, dpp_or<0x114, 0xf>(-INFINITY, v)); v = fmaxf(v, dpp_or<0x118, 0xf>(-INFINITY, v));
    v = fmaxf(v, dpp_or<0x142, 0xa>(-INFINITY, v));
    v = fmaxf(v, dpp_or<0x143, 0xc>(-INFINITY, v));
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// What one wave does for image b: log_w over its k samples, logmeanexp / softmax / objective gradients (iwae1.py:113-139).  `src` says where
// the rows' terms come from: LseGlobalSrc (lse_kernel: the arrays of LseArgs) or the LDS copies bern_pipe_kernel keeps of what it made itself.
struct LseGlobalSrc {
    __device__ __forceinline__ float px(const LseArgs& a, int, int r) const {
        float px = a.term[0][r];
        if (a.n_px_part > 1) {      // log p(x|z) as partial sums over pixel groups (small row counts): fixed order
            // (all partials requested at once: as a loop of dependent adds each load waited for the one before it -- 13 L2 round
            // trips, most of this kernel's 10 us at B = 20)
            float part[16];
#pragma unroll
            for (int i = 1; i < 16; ++i) part[i] = (i < a.n_px_part) ? a.term[0][(size_t)i * a.px_stride + r] : 0.0f;
#pragma unroll
            for (int i = 1; i < 16; ++i) px += part[i];
            for (int i = 16; i < a.n_px_part; ++i) px += a.term[0][(size_t)i * a.px_stride + r];
            a.term0_out[r] = px;
        }
        return px;
    }
    __device__ __forceinline__ float px_total(const LseArgs& a, int, int r) const { return a.term0_out[r]; }      // (total log p(x|z), written by px() above)
    __device__ __forceinline__ float term(const LseArgs& a, int t, int, int r) const { return a.term[t][r]; }
    __device__ __forceinline__ float lq_dreg(const LseArgs& a, int, int r) const { return a.lq_dreg[r]; }
};

// RED = the team working on one image: a wave (WaveRed: the training step's k) or a whole workgroup (BlockRed<NW>: the k = 5000 evaluator, where a wave
// per image is ~100 waves on the machine walking 5 000 samples each: 26 % of the bf16 evaluator's time in round 3's profile).  `lane` = index in the team.
struct WaveRed {
    static constexpr int NT = 64;
    __device__ __forceinline__ float sum(float v) const { return wave_sum(v); }
    __device__ __forceinline__ float max(float v) const { return wave_max(v); }
};
template <int NW>
struct BlockRed {      // (every thread of the workgroup calls sum / max the same number of times: they hold barriers)
    static constexpr int NT = 64 * NW;
    float* slots;      // NW floats of LDS
    __device__ __forceinline__ float sum(float v) const {
        const float w = wave_sum(v);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = w;
        __syncthreads();
        float t = 0.0f;
#pragma unroll
        for (int i = 0; i < NW; ++i) t += slots[i];
        return t;
    }
    __device__ __forceinline__ float max(float v) const {
        const float w = wave_max(v);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = w;
        __syncthreads();
        float t = -INFINITY;
#pragma unroll
        for (int i = 0; i < NW; ++i) t = fmaxf(t, slots[i]);
        return t;
    }
};

template <class SRC, class RED = WaveRed>
__device__ __forceinline__ void lse_image(const LseArgs& a, const int b, const int lane, const SRC& src, const RED red = RED()) {
    constexpr int NT = RED::NT;
    const int k = a.k;
    const bool single = NT == 64 && k <= 64;          // one sample per lane: log_w stays in a register between the passes
    // the image's head (for the KL term at the end): requested first, so that its round trip runs beside the log_w terms' instead of
    // behind the whole kernel
    float kmu[2] = {0.0f, 0.0f}, ksg[2] = {1.0f, 1.0f};
    if (a.head) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int f = lane + NT * i;
            if (f < a.D) { kmu[i] = a.head[(size_t)b * a.ldH + f]; ksg[i] = a.head[(size_t)b * a.ldH + a.Dp + f]; }
        }
    }
    float lw_reg = 0.0f;
    float m = -INFINITY, sum_lw = 0.0f, sum_px = 0.0f, sum_t1 = 0.0f, sum_t2 = 0.0f;
    for (int s = lane; s < k; s += NT) {
        const int r = b * k + s;
        const float px = src.px(a, s, r);
        float lw = a.coef[0] * px;
#pragma unroll
        for (int t = 1; t < 5; ++t)
            if (a.term[t]) lw += a.coef[t] * src.term(a, t, s, r);
        a.logw[r] = lw;
        lw_reg = lw;
        m = fmaxf(m, lw);
        sum_lw += lw;
        sum_px += px;
        if (a.term[1]) sum_t1 += src.term(a, 1, s, r);
        if (a.term[2]) sum_t2 += src.term(a, 2, s, r);
    }
    m = red.max(m); sum_lw = red.sum(sum_lw); sum_px = red.sum(sum_px); sum_t1 = red.sum(sum_t1); sum_t2 = red.sum(sum_t2);
    float se = 0.0f;
    for (int s = lane; s < k; s += NT) se += __expf((single ? lw_reg : a.logw[b * k + s]) - m);
    se = red.sum(se);
    const float inv_se = 1.0f / se;
    const float invB = 1.0f / (float)a.B, invkB = invB / (float)k;
    float eq14 = 0.0f, dreg = 0.0f;
    if (!a.lme_only)
    for (int s = lane; s < k; s += NT) {
        const int r = b * k + s;
        const float lw = single ? lw_reg : a.logw[r];
        const float wn = __expf(lw - m) * inv_se;       // iwae1.py:128-131 == softmax over k (:137)
        eq14 += wn * lw;
        a.wn[r] = wn;
        float G;                                         // dLoss/dlog_w, loss = -objective (iwae1.py:157)
        float4 cf = make_float4(1.0f, 0.0f, 0.0f, 0.0f); // (ca, cz, cq, cs) for latent_bwd_kernel
        if (a.objective == OBJ_VAE_ELBO) {
            G = -invkB; cf.y = -G * a.beta * a.cz_on; cf.w = G * a.beta;
        } else if (a.objective == OBJ_VAE_ELBO_KL) {
            G = -invkB;
        } else if (a.objective == OBJ_DREG) {            // tasks/task02.py:61-76,95-96
            G = -wn * invB;
            const float c2 = wn * wn * invB;
            cf.x = wn; cf.y = c2; cf.z = -c2;
        } else {                                         // iwae_elbo, iwae_eq14 (same gradient)
            G = -wn * invB; cf.y = -G * a.beta * a.cz_on; cf.w = G * a.beta;
        }
        if (a.lq_dreg) dreg += wn * wn * (src.term(a, 1, s, r) + src.px_total(a, s, r) - src.lq_dreg(a, s, r));   // tasks/task02.py:70-73
        a.gx[r] = G;
        if (a.gx_local && r >= a.gx_r0 && r < a.gx_r0 + a.gx_n) a.gx_local[r - a.gx_r0] = G;
        a.cf[r] = cf;
    }
    eq14 = red.sum(eq14); dreg = red.sum(dreg);
    // KL(q(z|x) || N(0,1)) per image (iwae1.py:116), TFP closed form
    float kl = 0.0f;
    if (a.head) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (lane + NT * i < a.D) {
                const float ls = __logf(ksg[i]);
                kl += 0.5f * kmu[i] * kmu[i] + 0.5f * expm1f(2.0f * ls) - ls;
            }
        }
        for (int f = lane + 2 * NT; f < a.D; f += NT) {      // (latent widths beyond 128)
            const float mu = a.head[(size_t)b * a.ldH + f], sg = a.head[(size_t)b * a.ldH + a.Dp + f];
            const float ls = __logf(sg);
            kl += 0.5f * mu * mu + 0.5f * expm1f(2.0f * ls) - ls;
        }
        kl = red.sum(kl);
    }
    if (lane == 0) {
        float* pb = a.per_b;
        const int B = a.B;
        pb[PB_LME * B + b] = m + __logf(se / (float)k);          // utils.py:6-8
        pb[PB_MEAN * B + b] = sum_lw / (float)k;
        pb[PB_EQ14 * B + b] = eq14;
        pb[PB_KL * B + b] = kl;
        pb[PB_PX * B + b] = sum_px / (float)k;
        pb[PB_T1 * B + b] = sum_t1 / (float)k;
        pb[PB_T2 * B + b] = sum_t2 / (float)k;
        pb[PB_DREG * B + b] = dreg;
    }
}

// counted wait for any count 0..24 (wave-uniform)
__device__ __forceinline__ void wait_vmem_but_ws(int n) {
#define IWAE_WS_CASE(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
    switch (n) {
        IWAE_WS_CASE(0) IWAE_WS_CASE(1) IWAE_WS_CASE(2) IWAE_WS_CASE(3) IWAE_WS_CASE(4) IWAE_WS_CASE(5) IWAE_WS_CASE(6) IWAE_WS_CASE(7)
        IWAE_WS_CASE(8) IWAE_WS_CASE(9) IWAE_WS_CASE(10) IWAE_WS_CASE(11) IWAE_WS_CASE(12) IWAE_WS_CASE(13) IWAE_WS_CASE(14) IWAE_WS_CASE(15)
        IWAE_WS_CASE(16) IWAE_WS_CASE(17) IWAE_WS_CASE(18) IWAE_WS_CASE(19) IWAE_WS_CASE(20) IWAE_WS_CASE(21) IWAE_WS_CASE(22) IWAE_WS_CASE(23)
        default: asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); break;
    }
#undef IWAE_WS_CASE
}

// Completion event riding on a kernel's own dispatch packet (hipExtLaunchKernelGGL stop event) instead of a separate
// hipEventRecord behind it.  Measured on MI355X (tools/probe/event_latency.hip): the record puts a 5.5-7 us bubble in
// front of the recording stream's next kernel and the waiting stream starts 12 us after the kernel ended; with the event
// on the dispatch packet these are 2.2 and 7.6 us, and a join back 6.2 instead of 10.  `done` is the launcher's own
// trailing argument (null: a plain launch); a launcher without one cannot carry an event.
#define LAUNCH_EV(done, kern, grid, block, lds, st, ...)                                                  \
    do {                                                                                                  \
        hipEvent_t ev_ = (done);                                                                          \
        if (ev_) hipExtLaunchKernelGGL(kern, grid, block, lds, st, nullptr, ev_, 0, __VA_ARGS__);         \
        else hipLaunchKernelGGL(kern, grid, block, lds, st, __VA_ARGS__);                                 \
    } while (0)
static inline dim3 grid1(size_t n, int bs) { return dim3((unsigned)((n + bs - 1) / bs)); }

}  // namespace iwae
