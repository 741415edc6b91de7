// Masked importance-weighted log p(x_obs) and the self-normalised estimate of E[x | x_obs] (iwae_impute, include/iwae_amd.h; Mattei &
// Frellsen 2019, MIWAE): DESIGN.md section 17.
//   impute_mask_kernel     xin = m ? x : 0, the encoder's input (a select: what x holds at an unobserved pixel goes nowhere)
//   impute_rows_kernel<0>  pass (a): 64 rows per workgroup -- the draws, z, the decoder forward, log p(x_obs|z) over the observed pixels, log_w
//   impute_stats_kernel    pass (b): one thread per image, its S log-weights in sample order: maximum, sum, log_px, ess
//   impute_rows_kernel<1>  pass (c): the same forward again with the weights final; per pixel pass the tile al_s sigmoid(l_s) goes to the
//                          waves' strips and one thread per (image, pixel) sums the image's rows of this chunk in sample order
//   impute_merge_kernel    S > 64 only: an image's chunk sums in chunk order -> xhat
// Rows are image-major.  S <= 64: a workgroup (4 waves x 16 rows) owns ipw = 64 / S whole images; S > 64: one 64-row chunk of one image.  The
// forward half of the row evaluation is local_q_kernel's (device_helpers.h, dec_row_tanh_layers): a row's products
// are float32 fmaf chains in k order (v_mfma_f32_16x16x4_f32) and do not depend on the rows beside it.  Unlike there, a row's log_w is
// summed in double across the pixel passes, the row's 16 lanes and its three terms and rounded to float32 once: a single row at 784 pixels
// then lands within a float32 rounding of the float64 value.  Every loop has a host-known trip count; workgroups never communicate; no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "device_helpers.h"

namespace iwae {
namespace {

constexpr int IM_THREADS = 256;

__host__ __device__ inline int im_pz(int Dp) { return Dp + 4; }                                            // pitch of the z strip
__host__ __device__ inline int im_ph(int Dp, int Hp) { return (Hp > Dp ? Hp : Dp) + 4; }                   // pitch of the g1 / g2 strips

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
            normal4(a.row_offset + (uint64_t)(img0 + i) * (uint64_t)S + (uint64_t)(s0 + lc - i * SC), (uint32_t)d4, 0u, a.step, a.seed, nrm);
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
    f32x4 acc[AIS_NT];
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
    dec_row_tanh_layers(a, zs, g1s, g2s, slab, PZ, PH, dt, ht, acc, tid, n16, q);
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
        for (int t = 0; t < AIS_NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        wg_gemm_f32(g2s, PH, ht, a.W3 + c0, a.Xp, cnt, slab, acc, tid, n16, q);
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
                        const float ex = __builtin_amdgcn_exp2f(-fabsf(l) * LOG2E_F);      // exp(-|l|)
                        s_xl[r] = fmaf(xm, l, s_xl[r]);
                        s_al[r] += fabsf(l);
                        prod[r] = in ? fmaf(prod[r], ex, prod[r]) : prod[r];
                    }
                }
            }
            // (across the passes in double: a row's log_w is rounded to float32 once, at the end)
#pragma unroll
            for (int r = 0; r < 4; ++r) lp[r] += ((double)s_xl[r] - 0.5 * (double)s_al[r]) - (double)LN2_F * (double)__builtin_amdgcn_logf(prod[r]);
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
                        const float ex = __builtin_amdgcn_exp2f(-fabsf(l) * LOG2E_F);      // exp(-|l|)
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
            const double lw = rowsum16(lp[r] + 0.5 * ((double)se[r] - (double)sz[r]) + (double)sr[r]);
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
