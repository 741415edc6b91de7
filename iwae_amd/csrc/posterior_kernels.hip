// Self-normalised latent moments and sampling importance resampling on the weights of iwae_impute's passes (a) and (b) (iwae_posterior,
// include/iwae_amd.h): DESIGN.md section 18.
//   posterior_moments_kernel  one workgroup per 64-draw chunk of one image: the chunk's draws e [64][Dp] in LDS (regenerated from their
//                             Philox rows, or the caller's), al_s from log_w and the image's (max, 1 / sum); m1 = sum_s al_s e_s per column in
//                             sample order, m2 = (al e)^T e on v_mfma_f32_16x16x4_f32, the tiles with tile-row <= tile-column only
//   posterior_merge_kernel    one thread per (image, d, d'): the chunks in chunk order in double -> mean, cov (mirrored: bitwise symmetric)
//   posterior_expw_kernel     one thread per (draw, image of the launch): exp((double)(log_w - max))
//   posterior_cdf_kernel      one thread per image of the launch: the running sum of those in sample order
//   posterior_pick_kernel     one thread per (draw r, image): its uniform (the caller's, or Philox stream 5) and the inverse CDF by bisection
//   posterior_gather_kernel   one thread per (r, image, four features): e of the picked index regenerated (or gathered) -> z
// Every loop has a host-known trip count; workgroups never communicate; no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "device_helpers.h"

namespace iwae {
namespace {

constexpr int PO_THREADS = 256;

__host__ __device__ inline int po_pe(int Dp) { return Dp + 4; }                                            // pitch of the e tile
__host__ __device__ inline size_t po_stride(int Dp) { return (size_t)Dp * Dp + Dp; }                       // floats per (image, chunk) of part

// one resampling uniform per (image, draw r): Philox stream 5, the first word of the draw, as ais_uniform forms it
__device__ __forceinline__ float po_uniform(uint64_t grow, uint32_t step, uint64_t seed) {
    uint32_t r[4];
    philox4x32_10((uint32_t)grow, (uint32_t)(grow >> 32), 5u << 24, step, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    return ((float)(r[0] >> 8) + 0.5f) * 5.9604644775390625e-08f;
}

__global__ __launch_bounds__(PO_THREADS) void posterior_moments_kernel(PosteriorMomArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem_po[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n16 = lane & 15, q = lane >> 4;
    const int PE = po_pe(a.Dp), D = a.D, Dp = a.Dp;
    float* es = smem_po;                  // e [64][PE]: columns >= D and rows >= SC are zero
    float* als = es + 64 * PE;            // al [64]: rows >= SC are zero
    const int bi = (int)blockIdx.x / a.nchunk, chunk = (int)blockIdx.x - bi * a.nchunk;      // image, counted from the launch's first
    const int img = a.img0 + bi, s0 = 64 * chunk, SC = min(64, a.S - s0);
    // ---- the chunk's draws, four features per thread and turn: the caller's, or impute_rows_kernel's Philox rows (stream 0 at the call's step)
    const int dq = Dp >> 2;
    for (int idx = tid; idx < 64 * dq; idx += PO_THREADS) {
        const int rr = idx / dq, d4 = idx - rr * dq;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (rr < SC) {
            if (a.eps) {
                const float* src = a.eps + ((size_t)(s0 + rr) * a.N + img) * D;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * d4 + j < D) v[j] = src[4 * d4 + j];
            } else {
                normal4(a.row_offset + (uint64_t)img * (uint64_t)a.S + (uint64_t)(s0 + rr), (uint32_t)d4, 0u, a.step, a.seed, v);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * d4 + j >= D) v[j] = 0.0f;
            }
        }
        *(float4*)(es + rr * PE + 4 * d4) = make_float4(v[0], v[1], v[2], v[3]);
    }
    // ---- al_s = exp(log_w_s - max) / sum: pass (c) of iwae_impute forms the same
    if (tid < 64) {
        float al = 0.0f;
        if (tid < SC) {
            const float2 st = a.wstat[img];
            al = expf(a.log_w[(size_t)(s0 + tid) * a.N + img] - st.x) * st.y;
        }
        als[tid] = al;
    }
    __syncthreads();
    float* out = a.part + ((size_t)bi * a.nchunk + chunk) * po_stride(Dp);
    // ---- first moment: one thread per column, the 64 rows in sample order (dead rows add exact zeros)
    if (tid < Dp) {
        float sum = 0.0f;
        for (int s = 0; s < 64; ++s) sum += als[s] * es[s * PE + tid];
        out[(size_t)Dp * Dp + tid] = sum;
    }
    // ---- second moment A^T B over the draw axis, A = al_s e_sd, B = e_sd', four draws per instruction in sample order.  Lane (n16, q)
    // hands row d = 16 ti + n16 of A and column d' = 16 tj + n16 of B at draw 4 sb + q, and holds m2[16 ti + 4 q + r][16 tj + n16] in
    // acc[r] (wg_gemm_f32's layout, device_helpers.h).  The upper tiles are dealt round the four waves in row-major order.
    if (a.want_cov) {
        const int dt = Dp >> 4, ntile = dt * (dt + 1) / 2;
        for (int t = wave; t < ntile; t += 4) {
            int ti = 0, rem = t;
            for (int i = 0; i < dt; ++i) {            // (row ti of the triangle holds dt - ti tiles)
                const bool past = ti == i && rem >= dt - i;
                rem = past ? rem - (dt - i) : rem;
                ti = past ? i + 1 : ti;
            }
            const int tj = ti + rem;
            f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int sb = 0; sb < 16; ++sb) {
                const int s = 4 * sb + q;
                const float ea = als[s] * es[s * PE + 16 * ti + n16];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ea, es[s * PE + 16 * tj + n16], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(size_t)(16 * ti + 4 * q + r) * Dp + 16 * tj + n16] = acc[r];
        }
    }
}

// mean[n][d] = mu_d + sigma_d ebar_d; cov[n][d][d'] = sigma_d sigma_d' (M2[d][d'] - ebar_d ebar_d').  The thread of (d, d'), d <= d', reads
// its entry of the upper triangle (consecutive d': consecutive addresses) and writes cov[d][d'] and cov[d'][d] -- the same float32, so cov
// equals its transpose bit for bit; a thread below the diagonal has nothing to do.  Each output is rounded to float32 once.  cov null: one
// thread per (image, d).
__global__ __launch_bounds__(PO_THREADS) void posterior_merge_kernel(PosteriorMergeArgs a) {
    const int D = a.D, Dp = a.Dp, DD = a.cov ? D : 1;
    const long idx = (long)blockIdx.x * PO_THREADS + threadIdx.x;
    if (idx >= (long)a.nimg * D * DD) return;
    const int i = (int)(idx / ((long)D * DD)), rem = (int)(idx - (long)i * D * DD), d = rem / DD, e = rem - d * DD;
    if (a.cov && e < d) return;
    const size_t stride = po_stride(Dp);
    const float* p = a.part + (size_t)i * a.nchunk * stride;
    const float* h = a.head + (size_t)(a.img0 + i) * a.ldh;
    double md = 0.0;
    for (int c = 0; c < a.nchunk; ++c) md += (double)p[c * stride + (size_t)Dp * Dp + d];
    if ((!a.cov || e == d) && a.mean) a.mean[(size_t)(a.img0 + i) * D + d] = (float)((double)h[d] + (double)h[a.soff + d] * md);
    if (a.cov) {
        double me = 0.0, m2 = 0.0;
        for (int c = 0; c < a.nchunk; ++c) me += (double)p[c * stride + (size_t)Dp * Dp + e];
        for (int c = 0; c < a.nchunk; ++c) m2 += (double)p[c * stride + (size_t)d * Dp + e];
        double ce = m2 - md * me;
        if (d == e) ce = fmax(ce, 0.0);
        const float v = (float)(((double)h[a.soff + d] * (double)h[a.soff + e]) * ce);
        float* cv = a.cov + (size_t)(a.img0 + i) * D * D;
        cv[(size_t)d * D + e] = v;
        cv[(size_t)e * D + d] = v;
    }
}

// w[s][i] = exp((double)(log_w_s - max)) of the launch's images, one thread each: impute_stats_kernel's exponential, out of the chain of sums
__global__ __launch_bounds__(PO_THREADS) void posterior_expw_kernel(PosteriorCdfArgs a) {
    const long t = (long)blockIdx.x * PO_THREADS + threadIdx.x;
    if (t >= (long)a.S * a.nimg) return;
    const int s = (int)(t / a.nimg), i = (int)(t - (long)s * a.nimg), img = a.img0 + i;
    a.cdf[t] = exp((double)(a.log_w[(size_t)s * a.N + img] - a.wstat[img].x));
}

// One thread per image of the launch: the running sum of its w in sample order, in place -- impute_stats_kernel's additions in its order,
// so c[S - 1] is that kernel's sum.  Eight loads go ahead of the eight additions that need them.
__global__ __launch_bounds__(PO_THREADS) void posterior_cdf_kernel(PosteriorCdfArgs a) {
    const int i = blockIdx.x * PO_THREADS + threadIdx.x;
    if (i >= a.nimg) return;
    double* p = a.cdf + i;
    const size_t ld = (size_t)a.nimg;
    double c = 0.0;
    int s = 0;
    for (; s + 8 <= a.S; s += 8) {
        double w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = p[(size_t)(s + j) * ld];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            c += w[j];
            p[(size_t)(s + j) * ld] = c;
        }
    }
    for (; s < a.S; ++s) {
        c += p[(size_t)s * ld];
        p[(size_t)s * ld] = c;
    }
}

// One thread per (r, image).  The bisection walks the powers of two from `top` down: pos ends as the number of leading c_s that fail the
// test, which (c never falls) is the index of the first that passes.  u c_{S-1} >= c_{S-1} (u = 1, or not a number in [0, 1)): no s
// passes, and the draw takes the first s whose c_s reaches c_{S-1}, the last draw of non-zero weight.  The result is always inside [0, S).
__global__ __launch_bounds__(PO_THREADS) void posterior_pick_kernel(PosteriorPickArgs a) {
    const long t = (long)blockIdx.x * PO_THREADS + threadIdx.x;
    if (t >= (long)a.R * a.nimg) return;
    const int r = (int)(t / a.nimg), i = (int)(t - (long)r * a.nimg), img = a.img0 + i;
    const size_t o = (size_t)r * a.N + img;
    const float u = a.unif ? a.unif[o] : po_uniform((a.batch_offset + (uint64_t)img) * (uint64_t)a.R + (uint64_t)r, a.step, a.seed);
    if (a.u) a.u[o] = u;
    const double* c = a.cdf + i;
    const double last = c[(size_t)(a.S - 1) * a.nimg], target = (double)u * last;
    int pos = 0;
    for (int b = a.top; b > 0; b >>= 1) {
        const int nx = pos + b;
        if (nx <= a.S && !(c[(size_t)(nx - 1) * a.nimg] > target)) pos = nx;
    }
    if (pos >= a.S) {
        pos = 0;
        for (int b = a.top; b > 0; b >>= 1) {
            const int nx = pos + b;
            if (nx <= a.S && c[(size_t)(nx - 1) * a.nimg] < last) pos = nx;
        }
        pos = min(pos, a.S - 1);
    }
    a.idx[o] = pos;
}

// One thread per (r, image, four features): z = fmaf(exp(log sigma), e, mu), impute_rows_kernel's arithmetic, e from the picked draw's own
// Philox row (batch_offset + n) S + idx (or the caller's eps at that index)
__global__ __launch_bounds__(PO_THREADS) void posterior_gather_kernel(PosteriorGatherArgs a) {
    const int dq = a.Dp >> 2;
    const long t = (long)blockIdx.x * PO_THREADS + threadIdx.x;
    if (t >= (long)a.R * a.nimg * dq) return;
    const int d4 = (int)(t % dq);
    const long ri = t / dq;
    const int r = (int)(ri / a.nimg), i = (int)(ri - (long)r * a.nimg), img = a.img0 + i;
    if (4 * d4 >= a.D) return;
    const int s = min(max(a.idx[(size_t)r * a.N + img], 0), a.S - 1);
    float e[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.eps) {
        const float* src = a.eps + ((size_t)s * a.N + img) * a.D;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (4 * d4 + j < a.D) e[j] = src[4 * d4 + j];
    } else {
        normal4(a.row_offset + (uint64_t)img * (uint64_t)a.S + (uint64_t)s, (uint32_t)d4, 0u, a.step, a.seed, e);
    }
    const float* h = a.head + (size_t)img * a.ldh;
    float* z = a.z + ((size_t)r * a.N + img) * a.D;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = 4 * d4 + j;
        if (col < a.D) z[col] = fmaf(expf(logf(h[a.soff + col])), e[j], h[col]);
    }
}

}  // namespace

size_t posterior_lds_bytes(int Dp) { return ((size_t)64 * po_pe(Dp) + 64) * 4; }
size_t posterior_part_floats(int Dp) { return po_stride(Dp); }
void launch_posterior_moments(const PosteriorMomArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(posterior_moments_kernel, dim3((unsigned)a.nimg * (unsigned)a.nchunk), dim3(PO_THREADS), posterior_lds_bytes(a.Dp), st, a);
}
void launch_posterior_merge(const PosteriorMergeArgs& a, hipStream_t st) {
    const long n = (long)a.nimg * a.D * (a.cov ? a.D : 1);
    hipLaunchKernelGGL(posterior_merge_kernel, dim3((unsigned)((n + PO_THREADS - 1) / PO_THREADS)), dim3(PO_THREADS), 0, st, a);
}
void launch_posterior_cdf(const PosteriorCdfArgs& a, hipStream_t st) {
    const long n = (long)a.S * a.nimg;
    hipLaunchKernelGGL(posterior_expw_kernel, dim3((unsigned)((n + PO_THREADS - 1) / PO_THREADS)), dim3(PO_THREADS), 0, st, a);
    hipLaunchKernelGGL(posterior_cdf_kernel, dim3((unsigned)((a.nimg + PO_THREADS - 1) / PO_THREADS)), dim3(PO_THREADS), 0, st, a);
}
void launch_posterior_pick(const PosteriorPickArgs& a, hipStream_t st) {
    const long n = (long)a.R * a.nimg;
    hipLaunchKernelGGL(posterior_pick_kernel, dim3((unsigned)((n + PO_THREADS - 1) / PO_THREADS)), dim3(PO_THREADS), 0, st, a);
}
void launch_posterior_gather(const PosteriorGatherArgs& a, hipStream_t st) {
    const long n = (long)a.R * a.nimg * (a.Dp >> 2);
    hipLaunchKernelGGL(posterior_gather_kernel, dim3((unsigned)((n + PO_THREADS - 1) / PO_THREADS)), dim3(PO_THREADS), 0, st, a);
}

}  // namespace iwae
