// Per-image optimisation of a factorised Gaussian q(z|x_n) = N(mu_n, exp(rho_n)^2) against the decoder (iwae_local_posterior,
// include/iwae_amd.h; Cremer, Li & Duvenaud 2018; Kim et al. 2018): DESIGN.md section 16.
//   local_init_kernel     state per image: mu, rho = log sigma from the caller's start or the encoder heads, Adam's m = v = 0, the double sums
//   local_q_kernel        passes [t0, t1) of 64 rows per workgroup: the draws, the row evaluation (decoder forward, log p(x|z), dz), one
//                         barrier, then one thread per (image, d) sums the image's S rows in sample order and applies Adam; evaluation
//                         passes run the same evaluation with the update switched off and sum log_w in double
//   local_finish_kernel   mu, sigma = exp(rho), elbo and iwae out of the double sums
// The row evaluation is device_helpers.h's dec_row_eval (ais_chain_kernel's arithmetic).  A row's numbers are float32 fmaf chains in k
// order (v_mfma_f32_16x16x4_f32) and do not depend on the rows beside it.  Every loop has a host-known trip count; workgroups never
// communicate; no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "device_helpers.h"

namespace iwae {
namespace {

constexpr int LQ_THREADS = 256;

__host__ __device__ inline int lq_pz(int Dp) { return (Dp > 16 * AIS_TPO ? Dp : 16 * AIS_TPO) + 4; }      // pitch of the z strip (also holds a residual tile)
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

// HOLES (iwae_local_posterior_masked): a.x holds launch_masked_code's rows m ? x : MO_HOLE, which dec_row_eval<true> selects out
template <bool HOLES>
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
    const float dc = (float)D * HALF_LOG_2PI_F;

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
                normal4(a.row_offset + (uint64_t)(img0 + i) * (uint64_t)S + (uint64_t)(lc - i * S), (uint32_t)d4, 0u, a.step0 + (uint32_t)t, a.seed, nrm);
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
        f32x4 acc[AIS_NT];
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
        dec_row_eval<HOLES>(a, zs, g1s, g2s, slab, PZ, PH, dt, ht, xt, npass, xrow, acc, lp, tid, n16, q);      // acc: dz = grad_z log p(x|z)
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
            const float lj = rowsum16(lp[r]) + (-0.5f * rowsum16(sz[r]) - dc);
            const float lqz = -0.5f * rowsum16(se[r]) - rowsum16(sr[r]) - dc;
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
    const dim3 grid((unsigned)((a.N + a.ipw - 1) / a.ipw));
    if (a.holes) hipLaunchKernelGGL(local_q_kernel<true>, grid, dim3(LQ_THREADS), local_q_lds_bytes(a.Dp, a.Hp), st, a);
    else hipLaunchKernelGGL(local_q_kernel<false>, grid, dim3(LQ_THREADS), local_q_lds_bytes(a.Dp, a.Hp), st, a);
}
void launch_local_finish(const LocalFinishArgs& a, hipStream_t st) {
    const long n = (long)a.N * a.D;
    hipLaunchKernelGGL(local_finish_kernel, dim3((unsigned)((n + LQ_THREADS - 1) / LQ_THREADS)), dim3(LQ_THREADS), 0, st, a);
}

}  // namespace iwae
