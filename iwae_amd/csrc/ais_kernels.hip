// Annealed importance sampling with HMC transitions (iwae_ais, include/iwae_amd.h; Neal 2001; Wu, Burda, Salakhutdinov & Grosse 2017): DESIGN.md section 15.
//   ais_pad_kernel      a Keras kernel of the float32 master parameters -> both orientations, padded to multiples of 16 with zeros
//   ais_init_kernel     chain state: e_0 (from z0 when given), log_w = 0, h = step_size, accept count = 0
//   ais_chain_kernel    transitions [t0, t1) of 64 chain rows per workgroup, everything between two launches in one: per leapfrog step the
//                       decoder forward, log p(x|z), the residual s = x - sigmoid(l) consumed at once into s W3^T, the two tanh-derivative
//                       products, W1^T and the leapfrog update; Philox momenta and uniforms, accept step, log_w increment, step adaptation
//   ais_finish_kernel   z = mu + sigma e, log_px = LSE_c log_w - log C (double), effective sample size
//   ais_accept_rate_kernel   mean of the accept flags per transition, fixed order
// Blocking: a wave owns 16 chain rows through every layer, forward and backward (v_mfma_f32_16x16x4_f32: the products are float32 fmaf chains
// in k order, so a row's numbers do not depend on the rows beside it); its activations z, g1, g2 live in a private LDS strip each and are
// overwritten in place by the backward pass (d2 over g2, d1 over g1, the residual tile over z); the workgroup's four waves share the weight
// slabs (16 in-features x <= 208 out-features), fetched from L2 into registers one slab ahead and handed over through LDS between two
// barriers.  Every loop has a host-known trip count; rows beyond R repeat row R - 1 and store nothing.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "device_helpers.h"

namespace iwae {
namespace {

constexpr int AIS_THREADS = 256;

__host__ __device__ inline int ais_pz(int Dp) { return (Dp > 16 * AIS_TPO ? Dp : 16 * AIS_TPO) + 4; }      // pitch of the z strip (also holds a residual tile)

// one accept uniform per chain row and transition: Philox stream 4, the first word of the draw
__device__ __forceinline__ float ais_uniform(uint64_t grow, uint32_t step, uint64_t seed) {
    uint32_t r[4];
    philox4x32_10_mul((uint32_t)grow, (uint32_t)(grow >> 32), 4u << 24, step, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    return ((float)(r[0] >> 8) + 0.5f) * 5.9604644775390625e-08f;
}

__global__ __launch_bounds__(AIS_THREADS) void ais_pad_kernel(AisPrepArgs a) {
    const long idx = (long)blockIdx.x * AIS_THREADS + threadIdx.x;
    if (idx >= (long)a.Kp * a.Np) return;
    const int k = (int)(idx / a.Np), n = (int)(idx - (long)k * a.Np);
    const float v = (k < a.K && n < a.N) ? a.src[(size_t)k * a.N + n] : 0.0f;
    a.dst[idx] = v;
    if (a.dstT) a.dstT[(size_t)n * a.Kp + k] = v;
}

__global__ __launch_bounds__(AIS_THREADS) void ais_init_kernel(AisInitArgs a) {
    const long r = (long)blockIdx.x * AIS_THREADS + threadIdx.x;
    if (r >= a.R) return;
    a.log_w[r] = 0.0;
    a.h[r] = a.step;
    a.nacc[r] = 0;
    if (a.z0) {
        const int n = (int)(r % a.N);
        for (int d = 0; d < a.D; ++d) {
            const float z = a.z0[(size_t)r * a.D + d];
            a.e[(size_t)r * a.D + d] = a.head ? (z - a.head[(size_t)n * a.ldh + d]) / a.head[(size_t)n * a.ldh + a.soff + d] : z;
        }
    }
}

// HOLES (iwae_ais_masked): a.x holds launch_masked_code's rows m ? x : MO_HOLE; a pixel with the hole's bits is selected
// out of log p(x|z) and of s like a pad column
template <bool HOLES>
__global__ __launch_bounds__(AIS_THREADS, 1) void ais_chain_kernel(AisChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem_ais[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n16 = lane & 15, q = lane >> 4;
    const int PZ = ais_pz(a.Dp), PH = a.Hp + 4, WST = 16 * (PZ + 2 * PH);
    float* zs = smem_ais + wave * WST;            // z rows, later a 64-pixel tile of the residual s
    float* g1s = zs + 16 * PZ;                    // g1, later dpre1
    float* g2s = g1s + 16 * PH;                   // g2, later dpre2
    float* slab = smem_ais + 4 * WST;
    const int dt = a.Dp >> 4, ht = a.Hp >> 4, xt = a.Xp >> 4, npass = (xt + AIS_TPO - 1) / AIS_TPO;
    const long m0 = (long)blockIdx.x * 64 + wave * 16;

    // the lane's four rows 4q + r: storage row (clamped) and image.  e and p stay in registers in the accumulator layout (row 4q + r,
    // feature 16 t + n16); mu and sigma are re-read where they are used (the heads of <= 16 images: L1 hits) -- 64 registers the MFMA
    // accumulators need more
    long row[4]; bool live[4]; const float* xrow[4]; const float* hrow[4];
    float e[AIS_DT][4], p[AIS_DT][4];
    float lsum[4], hstep[4]; int nacc[4];
    auto mu_at = [&](int r, int col) { return a.head ? hrow[r][col] : 0.0f; };
    auto sg_at = [&](int r, int col) { return a.head ? hrow[r][a.soff + col] : 1.0f; };
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long rr = m0 + 4 * q + r;
        live[r] = rr < a.R;
        row[r] = live[r] ? rr : a.R - 1;
        const int n = (int)(row[r] % a.N);
        xrow[r] = a.x + (size_t)n * a.X;
        hrow[r] = a.head + (size_t)n * a.ldh;
        float ls = 0.0f;
#pragma unroll
        for (int t = 0; t < AIS_DT; ++t) {
            const int col = 16 * t + n16;
            const bool in = t < dt && col < a.D;
            e[t][r] = in ? a.e[(size_t)row[r] * a.D + col] : 0.0f;
            p[t][r] = 0.0f;
            if (in) ls += __logf(sg_at(r, col));
        }
        lsum[r] = rowsum16(ls);                 // sum_d log sigma_d
        hstep[r] = a.h[row[r]];
        nacc[r] = a.nacc[row[r]];
    }
    const float dc = (float)a.D * HALF_LOG_2PI_F;

    // lj = log p(x|z) + log p(z) and l0 = log N(e; 0, I) - sum log sigma at z = mu + sigma e, then the kick p -= hh grad U_t with
    // grad U_t = (1 - bt) e - bt sigma (grad_z log p(x|z) - z)
    auto eval_kick = [&](float (&lj)[4], float (&l0)[4], const float bt, const float (&hh)[4]) {
        f32x4 acc[AIS_NT], dg2[AIS_NT];
        float sz[4] = {0.f, 0.f, 0.f, 0.f}, se[4] = {0.f, 0.f, 0.f, 0.f}, lp[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < AIS_DT; ++t) {
            if (t < dt) {
                const int col = 16 * t + n16;
                const bool in = col < a.D;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float z = in ? fmaf(sg_at(r, col), e[t][r], mu_at(r, col)) : 0.0f;
                    zs[(4 * q + r) * PZ + col] = z;
                    sz[r] = fmaf(z, z, sz[r]);
                    se[r] = fmaf(e[t][r], e[t][r], se[r]);
                }
            }
        }
        // ---- g1 = tanh(z W1 + b1), g2 = tanh(g1 W2 + b2)
#pragma unroll
        for (int t = 0; t < AIS_NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        wg_gemm_f32(zs, PZ, dt, a.W1, a.Hp, ht, slab, acc, tid, n16, q);
#pragma unroll
        for (int t = 0; t < AIS_NT; ++t) {
            if (t < ht) {
                const float b = a.b1[16 * t + n16];
#pragma unroll
                for (int r = 0; r < 4; ++r) g1s[(4 * q + r) * PH + 16 * t + n16] = tanh_f32(acc[t][r] + b);
                acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
        wg_gemm_f32(g1s, PH, ht, a.W2, a.Hp, ht, slab, acc, tid, n16, q);
#pragma unroll
        for (int t = 0; t < AIS_NT; ++t) {
            if (t < ht) {
                const float b = a.b2[16 * t + n16];
#pragma unroll
                for (int r = 0; r < 4; ++r) g2s[(4 * q + r) * PH + 16 * t + n16] = tanh_f32(acc[t][r] + b);
            }
            dg2[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        // ---- output layer, 64 pixels at a time: logits -> log p(x|z) and s = x - sigmoid(l) -> dg2 += s W3^T (s never leaves the workgroup)
        for (int pass = 0; pass < npass; ++pass) {
            const int c0 = 16 * AIS_TPO * pass, cnt = min(AIS_TPO, xt - AIS_TPO * pass);
#pragma unroll
            for (int t = 0; t < AIS_TPO; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            wg_gemm_f32(g2s, PH, ht, a.W3 + c0, a.Xp, cnt, slab, acc, tid, n16, q);
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
                        const bool ob = in && (!HOLES || __float_as_uint(x1) != MO_HOLE);      // counts: inside the image and observed
                        const float l = ob ? acc[t][r] + b : 0.0f, xm = ob ? x1 - 0.5f : 0.0f;
                        const float ex = __builtin_amdgcn_exp2f(-fabsf(l) * LOG2E_F);      // exp(-|l|)
                        s_xl[r] = fmaf(xm, l, s_xl[r]);
                        s_al[r] += fabsf(l);
                        prod[r] = ob ? fmaf(prod[r], ex, prod[r]) : prod[r];
                        zs[(4 * q + r) * PZ + 16 * t + n16] = ob ? xm - __builtin_copysignf(__builtin_amdgcn_rcpf(1.0f + ex) - 0.5f, l) : 0.0f;
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) lp[r] += s_xl[r] - 0.5f * s_al[r] - LN2_F * __builtin_amdgcn_logf(prod[r]);
            wg_gemm_f32(zs, PZ, cnt, a.W3T + (size_t)c0 * a.Hp, a.Hp, ht, slab, dg2, tid, n16, q);
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
            acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        wg_gemm_f32(g2s, PH, ht, a.W2T, a.Hp, ht, slab, acc, tid, n16, q);
#pragma unroll
        for (int t = 0; t < AIS_NT; ++t) {
            if (t < ht) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float* at = g1s + (4 * q + r) * PH + 16 * t + n16;
                    const float y = *at;
                    *at = acc[t][r] * (1.0f - y * y);
                }
                acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
        wg_gemm_f32(g1s, PH, ht, a.W1T, a.Dp, dt, slab, acc, tid, n16, q);
#pragma unroll
        for (int t = 0; t < AIS_DT; ++t) {
            if (t < dt) {
                const int col = 16 * t + n16;
                if (col < a.D) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float sg = sg_at(r, col), z = fmaf(sg, e[t][r], mu_at(r, col));
                        p[t][r] -= hh[r] * ((1.0f - bt) * e[t][r] - bt * (sg * (acc[t][r] - z)));
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            lj[r] = rowsum16(lp[r]) + (-0.5f * rowsum16(sz[r]) - dc);
            l0[r] = -0.5f * rowsum16(se[r]) - lsum[r] - dc;
        }
    };
    auto kinetic = [&](float (&kin)[4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float s = 0.0f;
#pragma unroll
            for (int t = 0; t < AIS_DT; ++t) s = fmaf(p[t][r], p[t][r], s);
            kin[r] = 0.5f * rowsum16(s);
        }
    };

    for (int tt = a.t0; tt < a.t1; ++tt) {
        const float bt = a.betas[tt + 1], bp = a.betas[tt];
        float lj[4], l0[4], u0[4], k0[4], half[4];
        // momentum of transition tt + 1: the caller's, or Philox stream 3 at step0 + tt + 1 -- one draw of four features per lane and turn,
        // handed to the lanes that own them through the wave's z strip (free between two evaluations)
        if (!a.mom) {
            const int dq = a.Dp >> 2;
#pragma unroll 1
            for (int idx = lane; idx < 16 * dq; idx += 64) {
                const int rr = idx / dq, d4 = idx - rr * dq;
                const long rw = min(m0 + rr, a.R - 1);
                float nrm[4];
                normal4_mul(a.row_offset + (uint64_t)(rw % a.N) * (uint64_t)a.C + (uint64_t)(rw / a.N), (uint32_t)d4, 3u, a.step0 + (uint32_t)tt + 1u, a.seed, nrm);
                *(float4*)(zs + rr * PZ + 4 * d4) = make_float4(nrm[0], nrm[1], nrm[2], nrm[3]);
            }
        }
#pragma unroll
        for (int t = 0; t < AIS_DT; ++t) {
            const int col = 16 * t + n16;
            const bool in = t < dt && col < a.D;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = 0.0f;
                if (in) v = a.mom ? a.mom[((size_t)tt * a.R + row[r]) * a.D + col] : zs[(4 * q + r) * PZ + col];
                p[t][r] = v;
            }
        }
        kinetic(k0);
#pragma unroll
        for (int r = 0; r < 4; ++r) half[r] = 0.5f * hstep[r];
        // evaluation 0 at the transition's start (weight increment, U_t(e), first half kick), then L leapfrog steps
        for (int l = 0; l <= a.L; ++l) {
            if (l > 0) {
#pragma unroll
                for (int t = 0; t < AIS_DT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) e[t][r] = fmaf(hstep[r], p[t][r], e[t][r]);
            }
            float hh[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) hh[r] = (l == 0 || l == a.L) ? half[r] : hstep[r];
            eval_kick(lj, l0, bt, hh);
            if (l == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (live[r] && n16 == 0) a.log_w[row[r]] += (double)(bt - bp) * (double)(lj[r] - l0[r]);
                    u0[r] = -((1.0f - bt) * l0[r] + bt * lj[r]);
                }
            }
        }
        float k1[4];
        kinetic(k1);
        if (!a.unif && lane < 16) {      // the accept uniforms of the wave's 16 rows (Philox stream 4), one per lane, through the strip
            const long rw = min(m0 + lane, a.R - 1);
            zs[lane * PZ] = ais_uniform(a.row_offset + (uint64_t)(rw % a.N) * (uint64_t)a.C + (uint64_t)(rw / a.N), a.step0 + (uint32_t)tt + 1u, a.seed);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float u1 = -((1.0f - bt) * l0[r] + bt * lj[r]);
            const float dH = ((u1 + k1[r]) - u0[r]) - k0[r];
            const float un = a.unif ? a.unif[(size_t)tt * a.R + row[r]] : zs[(4 * q + r) * PZ];
            const bool take = logf(un) < -dH;             // (a NaN dH rejects)
            if (live[r] && n16 == 0) {
                if (a.dH) a.dH[(size_t)tt * a.R + row[r]] = dH;
                if (a.accepted) a.accepted[(size_t)tt * a.R + row[r]] = take ? 1 : 0;
            }
            // the state in HBM is the chain's position between transitions: stored on accept, read back on reject
#pragma unroll
            for (int t = 0; t < AIS_DT; ++t) {
                const int col = 16 * t + n16;
                if (t < dt && col < a.D) {
                    float* at = a.e + (size_t)row[r] * a.D + col;
                    if (take) { if (live[r]) *at = e[t][r]; }
                    else e[t][r] = *at;
                }
            }
            nacc[r] += take ? 1 : 0;
            if (a.adapt) {
                const float mean = (float)nacc[r] / (float)(tt + 1);
                hstep[r] = fminf(fmaxf(hstep[r] * (mean > 0.65f ? 1.02f : 0.98f), 1e-4f), 0.5f);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (live[r] && n16 == 0) { a.h[row[r]] = hstep[r]; a.nacc[row[r]] = nacc[r]; }
    }
}

__global__ __launch_bounds__(AIS_THREADS) void ais_z_kernel(AisFinishArgs a) {
    const long idx = (long)blockIdx.x * AIS_THREADS + threadIdx.x;
    if (idx >= a.R * a.D) return;
    const long r = idx / a.D;
    const int d = (int)(idx - r * a.D), n = (int)(r % a.N);
    const float ev = a.e[idx];
    a.z[idx] = a.head ? fmaf(a.head[(size_t)n * a.ldh + a.soff + d], ev, a.head[(size_t)n * a.ldh + d]) : ev;
}
// one thread per image, its C chains in chain order
__global__ __launch_bounds__(AIS_THREADS) void ais_finish_kernel(AisFinishArgs a) {
    const int n = blockIdx.x * AIS_THREADS + threadIdx.x;
    if (n >= a.N) return;
    double mx = -INFINITY;
    for (int c = 0; c < a.C; ++c) mx = fmax(mx, a.log_w[(size_t)c * a.N + n]);
    double s1 = 0.0, s2 = 0.0;
    for (int c = 0; c < a.C; ++c) {
        const double w = exp(a.log_w[(size_t)c * a.N + n] - mx);
        s1 += w; s2 += w * w;
    }
    a.log_px[n] = mx + log(s1) - log((double)a.C);
    if (a.ess) a.ess[n] = (float)(s1 * s1 / s2);
}
// one workgroup per transition: the R flags summed as integers (exact, so the order is immaterial), then one division
__global__ __launch_bounds__(AIS_THREADS) void ais_accept_rate_kernel(const uint8_t* accepted, long R, float* rate) {
    __shared__ int part[AIS_THREADS];
    const uint8_t* f = accepted + (size_t)blockIdx.x * R;
    int s = 0;
    for (long i = threadIdx.x; i < R; i += AIS_THREADS) s += f[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = AIS_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) rate[blockIdx.x] = (float)part[0] / (float)R;
}

}  // namespace

size_t ais_chain_lds_bytes(int Dp, int Hp) { return ((size_t)4 * 16 * (ais_pz(Dp) + 2 * (Hp + 4)) + (size_t)16 * AIS_SLABP) * 4; }
void launch_ais_pad(const AisPrepArgs& a, hipStream_t st) {
    const long n = (long)a.Kp * a.Np;
    hipLaunchKernelGGL(ais_pad_kernel, dim3((unsigned)((n + AIS_THREADS - 1) / AIS_THREADS)), dim3(AIS_THREADS), 0, st, a);
}
void launch_ais_init(const AisInitArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(ais_init_kernel, dim3((unsigned)((a.R + AIS_THREADS - 1) / AIS_THREADS)), dim3(AIS_THREADS), 0, st, a);
}
void launch_ais_chain(const AisChainArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)((a.R + 63) / 64));
    if (a.holes) hipLaunchKernelGGL(ais_chain_kernel<true>, grid, dim3(AIS_THREADS), ais_chain_lds_bytes(a.Dp, a.Hp), st, a);
    else hipLaunchKernelGGL(ais_chain_kernel<false>, grid, dim3(AIS_THREADS), ais_chain_lds_bytes(a.Dp, a.Hp), st, a);
}
void launch_ais_finish(const AisFinishArgs& a, hipStream_t st) {
    if (a.z) hipLaunchKernelGGL(ais_z_kernel, dim3((unsigned)((a.R * a.D + AIS_THREADS - 1) / AIS_THREADS)), dim3(AIS_THREADS), 0, st, a);
    hipLaunchKernelGGL(ais_finish_kernel, dim3((a.N + AIS_THREADS - 1) / AIS_THREADS), dim3(AIS_THREADS), 0, st, a);
}
void launch_ais_accept_rate(const uint8_t* accepted, int T, long R, float* rate, hipStream_t st) {
    hipLaunchKernelGGL(ais_accept_rate_kernel, dim3(T), dim3(AIS_THREADS), 0, st, accepted, R, rate);
}

}  // namespace iwae
