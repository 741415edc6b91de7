// Per-image optimisation of a factorised Gaussian q(z|x_n) = N(mu_n, exp(rho_n)^2) against the decoder (iwae_local_posterior,
// include/iwae_amd.h; Cremer, Li & Duvenaud 2018; Kim et al. 2018): DESIGN.md section 16.
//   local_init_kernel     state per image: mu, rho = log sigma from the caller's start or the encoder heads, Adam's m = v = 0, the double sums
//   local_q_kernel        passes [t0, t1) of 64 rows per workgroup: the draws, the row evaluation (decoder forward, log p(x|z), dz), one
//                         barrier, then one thread per (image, d) sums the image's S rows in sample order and applies Adam; evaluation
//                         passes run the same evaluation with the update switched off and sum log_w in double
//   local_finish_kernel   mu, sigma = exp(rho), elbo and iwae out of the double sums
// The row evaluation is ais_chain_kernel's, restated here in the same arithmetic (lq_wg_gemm, lq_row_eval): shared through a header it
// cost ais_chain_kernel two spilled registers (12 bytes of scratch per lane), so ais_kernels.hip stays as it is.  A row's numbers are
// float32 fmaf chains in k order (v_mfma_f32_16x16x4_f32) and do not depend on the rows beside it.  Every loop has a host-known trip
// count; workgroups never communicate; no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"

namespace iwae {
namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4v;
#define LQ_LOG2E 1.4426950408889634f
#define LQ_LN2 0.6931471805599453f
#define LQ_HALF_LOG_2PI 0.9189385332046727f
constexpr int LQ_THREADS = 256;

__host__ __device__ inline int lq_pz(int Dp) { return (Dp > 16 * AIS_TPO ? Dp : 16 * AIS_TPO) + 4; }      // pitch of the z strip (also holds a residual tile)

// tanh through one hardware exp2 (fp32_kernels.hip's tanh_f32): absolute error <= ~1.5e-7
__device__ __forceinline__ float lq_tanh(float x) {
    const float t = __expf(2.0f * fabsf(x));
    return __builtin_copysignf(1.0f - 2.0f * __builtin_amdgcn_rcpf(t + 1.0f), x);
}

// Philox4x32-10 + Box-Muller exactly as kernels.hip draws them: counter = (row_lo, row_hi, (stream << 24) | d4, step), key = seed
__device__ __forceinline__ void lq_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)c0 * 0xD2511F53ull, p1 = (unsigned long long)c2 * 0xCD9E8D57ull;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ void lq_normal4(uint64_t grow, uint32_t d4, uint32_t stream, uint32_t step, uint64_t seed, float n[4]) {
    uint32_t r[4];
    lq_philox((uint32_t)grow, (uint32_t)(grow >> 32), (stream << 24) | d4, step, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const float s24 = 5.9604644775390625e-08f;   // 2^-24
    const float u0 = ((float)(r[0] >> 8) + 0.5f) * s24, u1 = ((float)(r[1] >> 8) + 0.5f) * s24;
    const float u2 = ((float)(r[2] >> 8) + 0.5f) * s24, u3 = ((float)(r[3] >> 8) + 0.5f) * s24;
    const float ra = __builtin_amdgcn_sqrtf(-2.0f * __logf(u0)), rb = __builtin_amdgcn_sqrtf(-2.0f * __logf(u2));
    n[0] = ra * __builtin_amdgcn_cosf(u1); n[1] = ra * __builtin_amdgcn_sinf(u1);
    n[2] = rb * __builtin_amdgcn_cosf(u3); n[3] = rb * __builtin_amdgcn_sinf(u3);
}
__device__ __forceinline__ float lq_rowsum(float v) {      // over the 16 lanes n16 of a quad group: every lane gets the same bits
    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
    return v;
}

// acc[t] += strip[16 rows][16 nkb] * W[16 nkb rows][16 cnt columns], t < cnt: W row-major with ldw floats per row, already at its first row and
// column.  Whole workgroup: the slab of 16 weight rows goes global -> registers (one slab ahead) -> LDS between two barriers.
__device__ __forceinline__ void lq_wg_gemm(const float* strip, int pa, int nkb, const float* W, int ldw, int cnt, float* slab,
                                            f32x4v (&acc)[AIS_NT], int tid, int n16, int q) {
    const int gpr = 4 * cnt;                     // 16-byte granules per slab row
    int goff[4], soff[4];
    bool ok[4];
    float4 pre[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int g = tid + LQ_THREADS * u, r = g / gpr, cq = g - r * gpr;
        ok[u] = r < 16;
        goff[u] = r * ldw + 4 * cq;
        soff[u] = r * AIS_SLABP + 4 * cq;
        pre[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok[u]) pre[u] = *(const float4*)(W + goff[u]);
    }
    for (int kb = 0; kb < nkb; ++kb) {
        __syncthreads();          // every wave has left the previous slab (and the strips of the layer before are written)
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (ok[u]) *(float4*)(slab + soff[u]) = pre[u];
        __syncthreads();
        if (kb + 1 < nkb) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (ok[u]) pre[u] = *(const float4*)(W + (size_t)(kb + 1) * 16 * ldw + goff[u]);
        }
        const float4 av = *(const float4*)(strip + n16 * pa + 16 * kb + 4 * q);      // row n16, k = 16 kb + 4 q + j at .j
        const float a4[4] = {av.x, av.y, av.z, av.w};
        const float* sl = slab + 4 * q * AIS_SLABP + n16;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < AIS_NT; ++t)
                if (t < cnt) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[j], sl[j * AIS_SLABP + 16 * t], acc[t], 0, 0, 0);
    }
}

// The row evaluation: the wave's 16 rows of z are in its strip zs (columns [0, 16 dt), pads zero).  Adds each lane's share of log p(x|z) of
// its four rows 4q + r to lp (lq_rowsum completes it) and leaves dz = grad_z log p(x|z) in acc[t][r], t < dt (row 4q + r, feature
// 16 t + n16).  Overwrites all three strips: g1s ends as dpre1, g2s as dpre2, zs as the last residual tile.  PH: pitch of g1s / g2s; xrow[r]: the image of row 4q + r.  Whole workgroup.
__device__ __forceinline__ void lq_row_eval(const LocalArgs& a, float* zs, float* g1s, float* g2s, float* slab, int PZ, int PH, int dt, int ht, int xt,
                                            int npass, const float* const (&xrow)[4], f32x4v (&acc)[AIS_NT], float (&lp)[4], int tid, int n16, int q) {
    f32x4v dg2[AIS_NT];
    // ---- g1 = tanh(z W1 + b1), g2 = tanh(g1 W2 + b2)
#pragma unroll
    for (int t = 0; t < AIS_NT; ++t) acc[t] = (f32x4v){0.f, 0.f, 0.f, 0.f};
    lq_wg_gemm(zs, PZ, dt, a.W1, a.Hp, ht, slab, acc, tid, n16, q);
#pragma unroll
    for (int t = 0; t < AIS_NT; ++t) {
        if (t < ht) {
            const float b = a.b1[16 * t + n16];
#pragma unroll
            for (int r = 0; r < 4; ++r) g1s[(4 * q + r) * PH + 16 * t + n16] = lq_tanh(acc[t][r] + b);
            acc[t] = (f32x4v){0.f, 0.f, 0.f, 0.f};
        }
    }
    lq_wg_gemm(g1s, PH, ht, a.W2, a.Hp, ht, slab, acc, tid, n16, q);
#pragma unroll
    for (int t = 0; t < AIS_NT; ++t) {
        if (t < ht) {
            const float b = a.b2[16 * t + n16];
#pragma unroll
            for (int r = 0; r < 4; ++r) g2s[(4 * q + r) * PH + 16 * t + n16] = lq_tanh(acc[t][r] + b);
        }
        dg2[t] = (f32x4v){0.f, 0.f, 0.f, 0.f};
    }
    // ---- output layer, 64 pixels at a time: logits -> log p(x|z) and s = x - sigmoid(l) -> dg2 += s W3^T (s never leaves the workgroup)
    for (int pass = 0; pass < npass; ++pass) {
        const int c0 = 16 * AIS_TPO * pass, cnt = min(AIS_TPO, xt - AIS_TPO * pass);
#pragma unroll
        for (int t = 0; t < AIS_TPO; ++t) acc[t] = (f32x4v){0.f, 0.f, 0.f, 0.f};
        lq_wg_gemm(g2s, PH, ht, a.W3 + c0, a.Xp, cnt, slab, acc, tid, n16, q);
        // sum_n x l - softplus(l) = sum_n (x - 1/2) l - |l| / 2 - log(1 + e^-|l|), the logarithms as one log2 of the product (dec_fwd_f32_kernel's form)
        float s_xl[4] = {0.f, 0.f, 0.f, 0.f}, s_al[4] = {0.f, 0.f, 0.f, 0.f}, prod[4] = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
        for (int t = 0; t < AIS_TPO; ++t) {
            if (t < cnt) {
                const int col = c0 + 16 * t + n16;
                const bool in = col < a.X;
                const float b = a.b3[col];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float x1 = in ? xrow[r][col] : 0.0f;
                    const float l = in ? acc[t][r] + b : 0.0f, xm = in ? x1 - 0.5f : 0.0f;
                    const float ex = __builtin_amdgcn_exp2f(-fabsf(l) * LQ_LOG2E);      // exp(-|l|)
                    s_xl[r] = fmaf(xm, l, s_xl[r]);
                    s_al[r] += fabsf(l);
                    prod[r] = in ? fmaf(prod[r], ex, prod[r]) : prod[r];
                    zs[(4 * q + r) * PZ + 16 * t + n16] = in ? xm - __builtin_copysignf(__builtin_amdgcn_rcpf(1.0f + ex) - 0.5f, l) : 0.0f;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) lp[r] += s_xl[r] - 0.5f * s_al[r] - LQ_LN2 * __builtin_amdgcn_logf(prod[r]);
        lq_wg_gemm(zs, PZ, cnt, a.W3T + (size_t)c0 * a.Hp, a.Hp, ht, slab, dg2, tid, n16, q);
    }
    // ---- dpre2 = dg2 (1 - g2^2) over g2; dpre1 = (dpre2 W2^T)(1 - g1^2) over g1; dz = dpre1 W1^T
#pragma unroll
    for (int t = 0; t < AIS_NT; ++t) {
        if (t < ht) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float* at = g2s + (4 * q + r) * PH + 16 * t + n16;
                const float y = *at;
                *at = dg2[t][r] * (1.0f - y * y);
            }
        }
        acc[t] = (f32x4v){0.f, 0.f, 0.f, 0.f};
    }
    lq_wg_gemm(g2s, PH, ht, a.W2T, a.Hp, ht, slab, acc, tid, n16, q);
#pragma unroll
    for (int t = 0; t < AIS_NT; ++t) {
        if (t < ht) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float* at = g1s + (4 * q + r) * PH + 16 * t + n16;
                const float y = *at;
                *at = acc[t][r] * (1.0f - y * y);
            }
            acc[t] = (f32x4v){0.f, 0.f, 0.f, 0.f};
        }
    }
    lq_wg_gemm(g1s, PH, ht, a.W1T, a.Dp, dt, slab, acc, tid, n16, q);
}

__host__ __device__ inline int lq_ph(int Dp, int Hp) { return (Hp > Dp ? Hp : Dp) + 4; }      // pitch of the g1 / g2 strips (g1's later holds a row of g sigma e)

__global__ __launch_bounds__(LQ_THREADS) void local_init_kernel(LocalInitArgs a) {
    const long idx = (long)blockIdx.x * LQ_THREADS + threadIdx.x;
    if (idx >= (long)a.N * a.D) return;
    const int n = (int)(idx / a.D), d = (int)(idx - (long)n * a.D);
    const float mu = a.mu0 ? a.mu0[idx] : a.head[(size_t)n * a.ldh + d];
    const float sg = a.sigma0 ? a.sigma0[idx] : a.head[(size_t)n * a.ldh + a.soff + d];
    float* sp = a.st + (size_t)n * 6 * a.D + d;
    sp[0] = mu;
    sp[a.D] = logf(sg);
#pragma unroll
    for (int j = 2; j < 6; ++j) sp[j * a.D] = 0.0f;
    a.q_mu[idx] = mu;
    a.q_sigma[idx] = sg;
    if (d == 0) { a.acc[3 * (size_t)n] = 0.0; a.acc[3 * (size_t)n + 1] = -INFINITY; a.acc[3 * (size_t)n + 2] = 0.0; }
}

__global__ __launch_bounds__(LQ_THREADS, 1) void local_q_kernel(LocalArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem_lq[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n16 = lane & 15, q = lane >> 4;
    const int PZ = lq_pz(a.Dp), PH = lq_ph(a.Dp, a.Hp), WST = 16 * (PZ + 2 * PH);
    float* zs = smem_lq + wave * WST;             // z rows, then residual tiles, at the end g = dz - z and (column PZ - 4) the row's log_w
    float* g1s = zs + 16 * PZ;                    // g1, then dpre1, at the end g sigma e
    float* g2s = g1s + 16 * PH;                   // g2, then dpre2
    float* slab = smem_lq + 4 * WST;
    const int dt = a.Dp >> 4, ht = a.Hp >> 4, xt = a.Xp >> 4, npass = (xt + AIS_TPO - 1) / AIS_TPO;
    const int S = a.S, D = a.D;
    const int img0 = blockIdx.x * a.ipw, nimg = min(a.ipw, a.N - img0), rows = nimg * S;      // the workgroup's images and live rows (image-major)

    // the lane's four rows 4q + r: local row (a dead one repeats the last live row and stores nothing), image, sample
    bool live[4]; int img[4], smp[4]; const float* xrow[4]; const float* srow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int lr = wave * 16 + 4 * q + r, lc = min(lr, rows - 1);
        live[r] = lr < rows;
        const int i = lc / S;
        img[r] = img0 + i;
        smp[r] = lc - i * S;
        xrow[r] = a.x + (size_t)img[r] * a.X;
        srow[r] = a.st + (size_t)img[r] * 6 * D;
    }
    const float dc = (float)D * LQ_HALF_LOG_2PI;

    for (int t = a.t0; t < a.t1; ++t) {
        // ---- the draws of pass t: the caller's, or Philox stream 0 at step0 + t (iwae_debug_eps(N, S, 0)'s keying) -- one draw of four
        // features per lane and turn, handed to the lanes that own them through the wave's z strip
        float e[AIS_DT][4];
        if (!a.eps) {
            const int dq = a.Dp >> 2;
#pragma unroll 1
            for (int idx = lane; idx < 16 * dq; idx += 64) {
                const int rr = idx / dq, d4 = idx - rr * dq;
                const int lc = min(wave * 16 + rr, rows - 1), i = lc / S;
                float nrm[4];
                lq_normal4(a.row_offset + (uint64_t)(img0 + i) * (uint64_t)S + (uint64_t)(lc - i * S), (uint32_t)d4, 0u, a.step0 + (uint32_t)t, a.seed, nrm);
                *(float4*)(zs + rr * PZ + 4 * d4) = make_float4(nrm[0], nrm[1], nrm[2], nrm[3]);
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < AIS_DT; ++k) {
            const int col = 16 * k + n16;
            const bool in = k < dt && col < D;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = 0.0f;
                if (in) v = a.eps ? a.eps[(((size_t)t * S + smp[r]) * a.N + img[r]) * D + col] : zs[(4 * q + r) * PZ + col];
                e[k][r] = v;
            }
        }
        // ---- z = mu + sigma e into the strip; the sums of log p(z) and log q(z)
        f32x4v acc[AIS_NT];
        float sz[4] = {0.f, 0.f, 0.f, 0.f}, se[4] = {0.f, 0.f, 0.f, 0.f}, sr[4] = {0.f, 0.f, 0.f, 0.f}, lp[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < AIS_DT; ++k) {
            if (k < dt) {
                const int col = 16 * k + n16;
                const bool in = col < D;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float rho = in ? srow[r][D + col] : 0.0f;
                    const float z = in ? fmaf(expf(rho), e[k][r], srow[r][col]) : 0.0f;
                    zs[(4 * q + r) * PZ + col] = z;
                    sz[r] = fmaf(z, z, sz[r]);
                    se[r] = fmaf(e[k][r], e[k][r], se[r]);
                    sr[r] += rho;
                }
            }
        }
        lq_row_eval(a, zs, g1s, g2s, slab, PZ, PH, dt, ht, xt, npass, xrow, acc, lp, tid, n16, q);      // acc: dz = grad_z log p(x|z)
        // ---- g = dz - z and g sigma e into the wave's own (now dead) strips, the row's log_w beside them
#pragma unroll
        for (int k = 0; k < AIS_DT; ++k) {
            if (k < dt) {
                const int col = 16 * k + n16;
                if (col < D) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float sg = expf(srow[r][D + col]), z = fmaf(sg, e[k][r], srow[r][col]);
                        const float g = acc[k][r] - z;
                        zs[(4 * q + r) * PZ + col] = g;
                        g1s[(4 * q + r) * PH + col] = g * (sg * e[k][r]);
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float lj = lq_rowsum(lp[r]) + (-0.5f * lq_rowsum(sz[r]) - dc);
            const float lqz = -0.5f * lq_rowsum(se[r]) - lq_rowsum(sr[r]) - dc;
            const float lw = lj - lqz;
            if (n16 == 0) {
                zs[(4 * q + r) * PZ + PZ - 4] = lw;
                if (a.log_w && t >= a.T && live[r]) a.log_w[((size_t)(t - a.T) * S + smp[r]) * a.N + img[r]] = lw;
            }
        }
        __syncthreads();
        auto lw_at = [&](int lr) { return smem_lq[(lr >> 4) * WST + (lr & 15) * PZ + PZ - 4]; };
        if (t < a.T) {
            // ---- one thread per (image, d): the image's S rows in sample order (across waves where S does not divide 16), then Adam
            const float alpha = a.alpha[t];
            for (int idx = tid; idx < nimg * D; idx += LQ_THREADS) {
                const int i = idx / D, d = idx - i * D, r0 = i * S;
                float mx = -INFINITY, sum = 0.0f, inv = a.inv_S;
                if (a.objective == 1) {
                    for (int s = 0; s < S; ++s) mx = fmaxf(mx, lw_at(r0 + s));
                    for (int s = 0; s < S; ++s) sum += expf(lw_at(r0 + s) - mx);
                    inv = 1.0f / sum;
                } else {
                    for (int s = 0; s < S; ++s) sum += lw_at(r0 + s);
                }
                float dmu = 0.0f, drho = 0.0f;
                for (int s = 0; s < S; ++s) {
                    const int lr = r0 + s;
                    const float* wv = smem_lq + (lr >> 4) * WST;      // the strips of the wave that owns the row
                    const float w = a.objective == 1 ? expf(wv[(lr & 15) * PZ + PZ - 4] - mx) * inv : inv;
                    dmu = fmaf(w, wv[(lr & 15) * PZ + d], dmu);
                    drho = fmaf(w, wv[16 * PZ + (lr & 15) * PH + d], drho);      // (g sigma e: the g1 strip)
                }
                drho += 1.0f;
                const size_t n = (size_t)(img0 + i);
                if (d == 0 && a.bound) a.bound[(size_t)t * a.N + n] = a.objective == 1 ? mx + logf(sum) - a.log_S : sum * a.inv_S;
                if (a.grad && t == a.T - 1) { a.grad[n * 2 * D + d] = dmu; a.grad[n * 2 * D + D + d] = drho; }
                float* sp = a.st + n * 6 * D + d;
                const float gr[2] = {dmu, drho};
#pragma unroll
                for (int j = 0; j < 2; ++j) {      // Keras Adam, ascending: epsilon outside the bias correction (alpha carries it)
                    const float m = a.beta1 * sp[(2 + 2 * j) * D] + (1.0f - a.beta1) * gr[j];
                    const float v = a.beta2 * sp[(3 + 2 * j) * D] + (1.0f - a.beta2) * gr[j] * gr[j];
                    sp[(2 + 2 * j) * D] = m;
                    sp[(3 + 2 * j) * D] = v;
                    sp[j * D] += alpha * m / (sqrtf(v) + a.epsilon);
                }
            }
        } else {
            // ---- evaluation pass: one thread per image, its S log-weights in sample order into the double sums (sum, running maximum,
            // sum of exp against it)
            for (int i = tid; i < nimg; i += LQ_THREADS) {
                double* ap = a.acc + 3 * (size_t)(img0 + i);
                double sum = ap[0], mx = ap[1], sx = ap[2];
                for (int s = 0; s < S; ++s) {
                    const double lw = (double)lw_at(i * S + s);
                    sum += lw;
                    if (lw > mx) { sx = sx * exp(mx - lw) + 1.0; mx = lw; }
                    else sx += exp(lw - mx);
                }
                ap[0] = sum; ap[1] = mx; ap[2] = sx;
            }
        }
        __syncthreads();          // the state is written (the next pass reads it) and the strips are free again
    }
}

__global__ __launch_bounds__(LQ_THREADS) void local_finish_kernel(LocalFinishArgs a) {
    const long idx = (long)blockIdx.x * LQ_THREADS + threadIdx.x;
    if (idx >= (long)a.N * a.D) return;
    const int n = (int)(idx / a.D), d = (int)(idx - (long)n * a.D);
    const float* sp = a.st + (size_t)n * 6 * a.D + d;
    a.mu[idx] = sp[0];
    a.sigma[idx] = expf(sp[a.D]);
    if (d == 0) {
        const double* ap = a.acc + 3 * (size_t)n;
        a.elbo[n] = ap[0] / (double)a.ES;
        a.iwae[n] = ap[1] + log(ap[2]) - log((double)a.ES);
    }
}

}  // namespace

size_t local_q_lds_bytes(int Dp, int Hp) { return ((size_t)4 * 16 * (lq_pz(Dp) + 2 * lq_ph(Dp, Hp)) + (size_t)16 * AIS_SLABP) * 4; }
void launch_local_init(const LocalInitArgs& a, hipStream_t st) {
    const long n = (long)a.N * a.D;
    hipLaunchKernelGGL(local_init_kernel, dim3((unsigned)((n + LQ_THREADS - 1) / LQ_THREADS)), dim3(LQ_THREADS), 0, st, a);
}
void launch_local_q(const LocalArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(local_q_kernel, dim3((unsigned)((a.N + a.ipw - 1) / a.ipw)), dim3(LQ_THREADS), local_q_lds_bytes(a.Dp, a.Hp), st, a);
}
void launch_local_finish(const LocalFinishArgs& a, hipStream_t st) {
    const long n = (long)a.N * a.D;
    hipLaunchKernelGGL(local_finish_kernel, dim3((unsigned)((n + LQ_THREADS - 1) / LQ_THREADS)), dim3(LQ_THREADS), 0, st, a);
}

}  // namespace iwae
