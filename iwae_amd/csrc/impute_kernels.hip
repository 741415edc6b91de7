// Masked importance-weighted log p(x_obs) and the self-normalised estimate of E[x | x_obs] (iwae_impute, include/iwae_amd.h; Mattei &
// Frellsen 2019, MIWAE): DESIGN.md section 17.
//   impute_mask_kernel     xin = m ? x : 0, the encoder's input (a select: what x holds at an unobserved pixel goes nowhere)
//   impute_rows_kernel<0>  pass (a): 64 rows per workgroup -- the draws, z, the decoder forward, log p(x_obs|z) over the observed pixels, log_w
//   impute_stats_kernel    pass (b): one thread per image, its S log-weights in sample order: maximum, sum, log_px, ess
//   impute_rows_kernel<1>  pass (c): the same forward again with the weights final; per pixel pass the tile al_s sigmoid(l_s) goes to the
//                          waves' strips and one thread per (image, pixel) sums the image's rows of this chunk in sample order
//   impute_merge_kernel    S > 64 only: an image's chunk sums in chunk order -> xhat
// Rows are image-major.  S <= 64: a workgroup (4 waves x 16 rows) owns ipw = 64 / S whole images; S > 64: one 64-row chunk of one image.  The
// forward half of the row evaluation is local_q_kernel's (lq_row_eval), restated here for the reason local_kernels.hip gives: a row's products
// are float32 fmaf chains in k order (v_mfma_f32_16x16x4_f32) and do not depend on the rows beside it.  Unlike there, a row's log_w is
// summed in double across the pixel passes, the row's 16 lanes and its three terms and rounded to float32 once: a single row at 784 pixels
// then lands within a float32 rounding of the float64 value.  Every loop has a host-known trip count; workgroups never communicate; no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"

namespace iwae {
namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4v;
#define IM_LOG2E 1.4426950408889634f
#define IM_LN2 0.6931471805599453f
constexpr int IM_THREADS = 256;

__host__ __device__ inline int im_pz(int Dp) { return Dp + 4; }                                            // pitch of the z strip
__host__ __device__ inline int im_ph(int Dp, int Hp) { return (Hp > Dp ? Hp : Dp) + 4; }                   // pitch of the g1 / g2 strips

// tanh through one hardware exp2 (fp32_kernels.hip's tanh_f32): absolute error <= ~1.5e-7
__device__ __forceinline__ float im_tanh(float x) {
    const float t = __expf(2.0f * fabsf(x));
    return __builtin_copysignf(1.0f - 2.0f * __builtin_amdgcn_rcpf(t + 1.0f), x);
}

// Philox4x32-10 + Box-Muller exactly as kernels.hip draws them: counter = (row_lo, row_hi, (stream << 24) | d4, step), key = seed
__device__ __forceinline__ void im_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
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
__device__ __forceinline__ void im_normal4(uint64_t grow, uint32_t d4, uint32_t stream, uint32_t step, uint64_t seed, float n[4]) {
    uint32_t r[4];
    im_philox((uint32_t)grow, (uint32_t)(grow >> 32), (stream << 24) | d4, step, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const float s24 = 5.9604644775390625e-08f;   // 2^-24
    const float u0 = ((float)(r[0] >> 8) + 0.5f) * s24, u1 = ((float)(r[1] >> 8) + 0.5f) * s24;
    const float u2 = ((float)(r[2] >> 8) + 0.5f) * s24, u3 = ((float)(r[3] >> 8) + 0.5f) * s24;
    const float ra = __builtin_amdgcn_sqrtf(-2.0f * __logf(u0)), rb = __builtin_amdgcn_sqrtf(-2.0f * __logf(u2));
    n[0] = ra * __builtin_amdgcn_cosf(u1); n[1] = ra * __builtin_amdgcn_sinf(u1);
    n[2] = rb * __builtin_amdgcn_cosf(u3); n[3] = rb * __builtin_amdgcn_sinf(u3);
}
__device__ __forceinline__ double im_rowsum_d(double v) {      // over the 16 lanes n16 of a quad group: every lane gets the same bits
    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
    return v;
}

// acc[t] += strip[16 rows][16 nkb] * W[16 nkb rows][16 cnt columns], t < cnt: W row-major with ldw floats per row, already at its first row and
// column.  Whole workgroup: the slab of 16 weight rows goes global -> registers (one slab ahead) -> LDS between two barriers.
__device__ __forceinline__ void im_wg_gemm(const float* strip, int pa, int nkb, const float* W, int ldw, int cnt, float* slab,
                                            f32x4v (&acc)[AIS_NT], int tid, int n16, int q) {
    const int gpr = 4 * cnt;                     // 16-byte granules per slab row
    int goff[4], soff[4];
    bool ok[4];
    float4 pre[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int g = tid + IM_THREADS * u, r = g / gpr, cq = g - r * gpr;
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

__global__ __launch_bounds__(IM_THREADS) void impute_mask_kernel(const float* x, const uint8_t* mask, long n, float* xin) {
    const long idx = (long)blockIdx.x * IM_THREADS + threadIdx.x;
    if (idx >= n) return;
    float v = 0.0f;
    if (mask[idx] != 0) v = x[idx];          // (x at an unobserved pixel is not even loaded)
    xin[idx] = v;
}

// XHAT = false: pass (a), writes log_w.  XHAT = true: pass (c), reads log_w and the image's (max, 1 / sum) and writes xhat (S <= 64) or the
// chunk's partial sums (S > 64).
template <bool XHAT>
__global__ __launch_bounds__(IM_THREADS, 1) void impute_rows_kernel(ImputeArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem_im[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n16 = lane & 15, q = lane >> 4;
    const int PZ = im_pz(a.Dp), PH = im_ph(a.Dp, a.Hp), WST = 16 * (PZ + 2 * PH);
    float* zs = smem_im + wave * WST;             // z rows
    float* g1s = zs + 16 * PZ;                    // g1, then (pass (c)) the pixel tiles of al sigmoid(l)
    float* g2s = g1s + 16 * PH;
    float* slab = smem_im + 4 * WST;
    const int dt = a.Dp >> 4, ht = a.Hp >> 4, xt = a.Xp >> 4;
    const int tpo = ht, npass = (xt + tpo - 1) / tpo;      // pixel tiles per pass of the output layer: as many as a strip of g1 is wide
    const int S = a.S, D = a.D;
    // the workgroup's images and live rows (image-major): ipw whole images, or chunk `chunk` of one image
    const int bi = a.nchunk > 1 ? (int)blockIdx.x / a.nchunk : (int)blockIdx.x * a.ipw;      // first image, counted from the launch's first
    const int chunk = a.nchunk > 1 ? (int)blockIdx.x - bi * a.nchunk : 0;
    const int nimg = a.nchunk > 1 ? 1 : min(a.ipw, a.nimg - bi);
    const int SC = a.nchunk > 1 ? min(64, S - 64 * chunk) : S;                                // rows per image in this workgroup
    const int rows = nimg * SC, img0 = a.img0 + bi, s0 = 64 * chunk;

    // the lane's four rows 4q + r: local row (a dead one repeats the last live row and stores nothing), image, sample
    bool live[4], same[4]; int img[4], smp[4]; const float* xrow[4]; const uint8_t* mrow[4]; const float* hrow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int lr = wave * 16 + 4 * q + r, lc = min(lr, rows - 1);
        live[r] = lr < rows;
        const int i = lc / SC;
        img[r] = img0 + i;
        smp[r] = s0 + lc - i * SC;
        same[r] = r > 0 && img[r] == img[r - 1];
        xrow[r] = a.x + (size_t)img[r] * a.X;
        mrow[r] = a.mask ? a.mask + (size_t)img[r] * a.X : nullptr;
        hrow[r] = a.head + (size_t)img[r] * a.ldh;
    }

    // ---- the draws: the caller's, or Philox stream 0 at the call's step (iwae_debug_eps(N, S, 0)'s keying) -- one draw of four features per
    // lane and turn, handed to the lanes that own them through the wave's z strip
    float e[AIS_DT][4];
    if (!a.eps) {
        const int dq = a.Dp >> 2;
#pragma unroll 1
        for (int idx = lane; idx < 16 * dq; idx += 64) {
            const int rr = idx / dq, d4 = idx - rr * dq;
            const int lc = min(wave * 16 + rr, rows - 1), i = lc / SC;
            float nrm[4];
            im_normal4(a.row_offset + (uint64_t)(img0 + i) * (uint64_t)S + (uint64_t)(s0 + lc - i * SC), (uint32_t)d4, 0u, a.step, a.seed, nrm);
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
            if (in) v = a.eps ? a.eps[((size_t)smp[r] * a.N + img[r]) * D + col] : zs[(4 * q + r) * PZ + col];
            e[k][r] = v;
        }
    }
    // ---- z = mu + sigma e into the strip (sigma as exp(rho), rho = log sigma: local_q_kernel's arithmetic); the sums of log p(z) and log q(z)
    f32x4v acc[AIS_NT];
    float sz[4] = {0.f, 0.f, 0.f, 0.f}, se[4] = {0.f, 0.f, 0.f, 0.f}, sr[4] = {0.f, 0.f, 0.f, 0.f};
    double lp[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < AIS_DT; ++k) {
        if (k < dt) {
            const int col = 16 * k + n16;
            const bool in = col < D;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float rho = in ? logf(hrow[r][a.soff + col]) : 0.0f;
                const float z = in ? fmaf(expf(rho), e[k][r], hrow[r][col]) : 0.0f;
                zs[(4 * q + r) * PZ + col] = z;
                sz[r] = fmaf(z, z, sz[r]);
                se[r] = fmaf(e[k][r], e[k][r], se[r]);
                sr[r] += rho;
            }
        }
    }
    // ---- g1 = tanh(z W1 + b1), g2 = tanh(g1 W2 + b2)
#pragma unroll
    for (int t = 0; t < AIS_NT; ++t) acc[t] = (f32x4v){0.f, 0.f, 0.f, 0.f};
    im_wg_gemm(zs, PZ, dt, a.W1, a.Hp, ht, slab, acc, tid, n16, q);
#pragma unroll
    for (int t = 0; t < AIS_NT; ++t) {
        if (t < ht) {
            const float b = a.b1[16 * t + n16];
#pragma unroll
            for (int r = 0; r < 4; ++r) g1s[(4 * q + r) * PH + 16 * t + n16] = im_tanh(acc[t][r] + b);
            acc[t] = (f32x4v){0.f, 0.f, 0.f, 0.f};
        }
    }
    im_wg_gemm(g1s, PH, ht, a.W2, a.Hp, ht, slab, acc, tid, n16, q);
#pragma unroll
    for (int t = 0; t < AIS_NT; ++t) {
        if (t < ht) {
            const float b = a.b2[16 * t + n16];
#pragma unroll
            for (int r = 0; r < 4; ++r) g2s[(4 * q + r) * PH + 16 * t + n16] = im_tanh(acc[t][r] + b);
        }
    }
    // ---- pass (c): the rows' final weights al_s = exp(log_w_s - max) / sum (a dead row: 0)
    float al[4] = {0.f, 0.f, 0.f, 0.f};
    if (XHAT) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (live[r]) {
                const float2 st = a.wstat[img[r]];
                al[r] = expf(a.log_w[(size_t)smp[r] * a.N + img[r]] - st.x) * st.y;
            }
        }
    }
    // ---- output layer, 16 tpo pixels at a time (local_q_kernel walks 64: its residual tile must fit the z strip; here a slab of W3 feeds up
    // to 13 tiles between its two barriers instead of 4)
    for (int pass = 0; pass < npass; ++pass) {
        const int c0 = 16 * tpo * pass, cnt = min(tpo, xt - tpo * pass);
#pragma unroll
        for (int t = 0; t < AIS_NT; ++t) acc[t] = (f32x4v){0.f, 0.f, 0.f, 0.f};
        im_wg_gemm(g2s, PH, ht, a.W3 + c0, a.Xp, cnt, slab, acc, tid, n16, q);
        if (!XHAT) {
            // sum_n x l - softplus(l) over the observed pixels = sum_n (x - 1/2) l - |l| / 2 - log(1 + e^-|l|), the logarithms as one log2 of the
            // product (dec_fwd_f32_kernel's form); an image's mask byte of a pixel is loaded once for the lane's rows of that image
            float s_xl[4] = {0.f, 0.f, 0.f, 0.f}, s_al[4] = {0.f, 0.f, 0.f, 0.f}, prod[4] = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
            for (int t = 0; t < AIS_NT; ++t) {
                if (t < cnt) {
                    const int col = c0 + 16 * t + n16;
                    const bool inx = col < a.X;
                    const float b = a.b3[col];
                    bool ob = inx;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (a.mask && !same[r]) ob = inx && mrow[r][inx ? col : 0] != 0;
                        const bool in = ob;
                        const float x1 = in ? xrow[r][col] : 0.0f;
                        const float l = in ? acc[t][r] + b : 0.0f, xm = in ? x1 - 0.5f : 0.0f;
                        const float ex = __builtin_amdgcn_exp2f(-fabsf(l) * IM_LOG2E);      // exp(-|l|)
                        s_xl[r] = fmaf(xm, l, s_xl[r]);
                        s_al[r] += fabsf(l);
                        prod[r] = in ? fmaf(prod[r], ex, prod[r]) : prod[r];
                    }
                }
            }
            // (across the passes in double: a row's log_w is rounded to float32 once, at the end)
#pragma unroll
            for (int r = 0; r < 4; ++r) lp[r] += ((double)s_xl[r] - 0.5 * (double)s_al[r]) - (double)IM_LN2 * (double)__builtin_amdgcn_logf(prod[r]);
        } else {
            // the tile al_s sigmoid(l_s) into the waves' g1 strips (dead since g2), then one thread per (image, pixel): the image's rows of this
            // chunk in sample order
#pragma unroll
            for (int t = 0; t < AIS_NT; ++t) {
                if (t < cnt) {
                    const int col = c0 + 16 * t + n16;
                    const float b = a.b3[col];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float l = acc[t][r] + b;
                        const float ex = __builtin_amdgcn_exp2f(-fabsf(l) * IM_LOG2E);      // exp(-|l|)
                        const float rc = __builtin_amdgcn_rcpf(1.0f + ex);
                        g1s[(4 * q + r) * PH + 16 * t + n16] = al[r] * (l >= 0.0f ? rc : ex * rc);
                    }
                }
            }
            __syncthreads();
            const int wd = 16 * cnt;
            for (int idx = tid; idx < nimg * wd; idx += IM_THREADS) {
                const int i = idx / wd, c = idx - i * wd, col = c0 + c;
                if (col < a.X) {
                    float sum = 0.0f;
                    for (int s = 0; s < SC; ++s) {
                        const int lr = i * SC + s;
                        sum += smem_im[(lr >> 4) * WST + 16 * PZ + (lr & 15) * PH + c];
                    }
                    if (a.nchunk > 1) a.part[((size_t)bi * a.nchunk + chunk) * a.Xp + col] = sum;
                    else a.xhat[(size_t)(img0 + i) * a.X + col] = fminf(sum, 1.0f);      // (a convex combination: the clamp takes the rounding of sum al)
                }
            }
            // (the next pass's product starts with a barrier before any strip is written again)
        }
    }
    if (!XHAT) {
        // log_w = log p(x_obs|z) + sum_d (-z^2/2 - c) - sum_d (-e^2/2 - log sigma - c): the lane's float32 sums meet in double (the c's
        // cancel), the row's 16 lanes are added in double, and the result is rounded to float32 once
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double lw = im_rowsum_d(lp[r] + 0.5 * ((double)se[r] - (double)sz[r]) + (double)sr[r]);
            if (n16 == 0 && live[r]) a.log_w[(size_t)smp[r] * a.N + img[r]] = (float)lw;
        }
    }
}

// One thread per image: the S float32 log-weights in sample order -- the maximum, then sum exp(log_w - max) and its squares in double
__global__ __launch_bounds__(IM_THREADS) void impute_stats_kernel(ImputeStatsArgs a) {
    const int n = blockIdx.x * IM_THREADS + threadIdx.x;
    if (n >= a.N) return;
    float mx = -INFINITY;
    for (int s = 0; s < a.S; ++s) mx = fmaxf(mx, a.log_w[(size_t)s * a.N + n]);
    double sum = 0.0, sq = 0.0;
    for (int s = 0; s < a.S; ++s) {
        const double w = exp((double)(a.log_w[(size_t)s * a.N + n] - mx));      // (the float32 difference is exact enough: both are float32 values of one magnitude)
        sum += w;
        sq = fma(w, w, sq);
    }
    a.log_px[n] = (double)mx + log(sum) - log((double)a.S);
    if (a.ess) a.ess[n] = (float)(sum * sum / sq);
    a.wstat[n] = make_float2(mx, (float)(1.0 / sum));
}

__global__ __launch_bounds__(IM_THREADS) void impute_merge_kernel(ImputeMergeArgs a) {
    const long idx = (long)blockIdx.x * IM_THREADS + threadIdx.x;
    if (idx >= (long)a.nimg * a.X) return;
    const int i = (int)(idx / a.X), col = (int)(idx - (long)i * a.X);
    float sum = 0.0f;
    for (int c = 0; c < a.nchunk; ++c) sum += a.part[((size_t)i * a.nchunk + c) * a.Xp + col];
    a.xhat[(size_t)(a.img0 + i) * a.X + col] = fminf(sum, 1.0f);
}

}  // namespace

size_t impute_lds_bytes(int Dp, int Hp) { return ((size_t)4 * 16 * (im_pz(Dp) + 2 * im_ph(Dp, Hp)) + (size_t)16 * AIS_SLABP) * 4; }
void launch_impute_mask(const float* x, const uint8_t* mask, long n, float* xin, hipStream_t st) {
    hipLaunchKernelGGL(impute_mask_kernel, dim3((unsigned)((n + IM_THREADS - 1) / IM_THREADS)), dim3(IM_THREADS), 0, st, x, mask, n, xin);
}
void launch_impute_rows(const ImputeArgs& a, bool xhat, hipStream_t st) {
    const unsigned grid = a.nchunk > 1 ? (unsigned)a.nimg * (unsigned)a.nchunk : (unsigned)((a.nimg + a.ipw - 1) / a.ipw);
    if (xhat) hipLaunchKernelGGL(impute_rows_kernel<true>, dim3(grid), dim3(IM_THREADS), impute_lds_bytes(a.Dp, a.Hp), st, a);
    else hipLaunchKernelGGL(impute_rows_kernel<false>, dim3(grid), dim3(IM_THREADS), impute_lds_bytes(a.Dp, a.Hp), st, a);
}
void launch_impute_stats(const ImputeStatsArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(impute_stats_kernel, dim3((unsigned)((a.N + IM_THREADS - 1) / IM_THREADS)), dim3(IM_THREADS), 0, st, a);
}
void launch_impute_merge(const ImputeMergeArgs& a, hipStream_t st) {
    const long n = (long)a.nimg * a.X;
    hipLaunchKernelGGL(impute_merge_kernel, dim3((unsigned)((n + IM_THREADS - 1) / IM_THREADS)), dim3(IM_THREADS), 0, st, a);
}

}  // namespace iwae
