// Latent-grid quadrature of a model with a few latent dimensions (iwae_grid_posterior, include/iwae_amd.h):
// the true posterior p(z|x) on a grid and the exact log p(x) (tasks/plot_task01.py:31-78).
//   grid_prep_x_kernel   x -> bf16 once per call, binary check
//   grid_prep_kernel     decoder logits of a chunk of grid points -> bf16 hi/lo split + row constant c_g
//   grid_score_kernel    S = X (L_hi + L_lo)^T on v_mfma_f32_16x16x32_bf16, online log-sum-exp + moments per image
//   grid_merge_kernel    partial states in fixed order -> running state (double) -> log p(x), moments, KL
// Numerics: x in {0,1} is exact in bf16 and l = L_hi + L_lo up to ~2^-17 |l|, so S is float32-grade;
// the softplus sum of c_g is taken in double; every reduction runs in a fixed order, so an image's results depend on the grid
// and the chunk size only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "layout.h"
#include "device_helpers.h"

namespace iwae {
namespace {

#define GRID_LOG2PI 1.8378770664093453

// x [N][X] fp32 -> XB [Np][Xp] bf16 (pad rows / pixels zero); *nonbinary = 1 if any x is not 0 or 1
__global__ __launch_bounds__(256) void grid_prep_x_kernel(const float* x, int N, int X, int Np, int Xp, uint16_t* XB, int* nonbinary) {
    const int nq = Xp / 8;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)Np * nq) return;
    const int row = (int)(idx / nq), c8 = (int)(idx - (long)row * nq) * 8;
    float v[8];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int col = c8 + j;
        v[j] = (row < N && col < X) ? x[(size_t)row * X + col] : 0.0f;
        bad |= !(v[j] == 0.0f || v[j] == 1.0f);
    }
    *(uint4*)(XB + (size_t)row * Xp + c8) = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
    if (bad) atomicOr(nonbinary, 1);
}

// one wave per grid row: bf16 hi/lo split of the logits, c_g = -1/2 |z|^2 - D/2 log 2 pi - sum_j softplus(l_j) + w_g (src/iwae1.py:105-111)
__global__ __launch_bounds__(256) void grid_prep_kernel(GridPrepArgs a) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= a.Gcp) return;
    const bool valid = g < a.Gc;
    double sp = 0.0;
    for (int c8 = lane * 8; c8 < a.Xp; c8 += 512) {
        float l[8], lo[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int col = c8 + j;
            l[j] = (valid && col < a.X) ? a.logits[(size_t)g * a.ldl + col] : 0.0f;
            if (valid && col < a.X) sp += (double)(fmaxf(l[j], 0.0f) + log1pf(expf(-fabsf(l[j]))));
        }
        uint32_t h[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            h[j] = pack2(l[2 * j], l[2 * j + 1]);
            lo[2 * j] = l[2 * j] - bflo(h[j]);
            lo[2 * j + 1] = l[2 * j + 1] - bfhi(h[j]);
        }
        *(uint4*)(a.Lhi + (size_t)g * a.Xp + c8) = make_uint4(h[0], h[1], h[2], h[3]);
        *(uint4*)(a.Llo + (size_t)g * a.Xp + c8) = make_uint4(pack2(lo[0], lo[1]), pack2(lo[2], lo[3]), pack2(lo[4], lo[5]), pack2(lo[6], lo[7]));
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sp += __shfl_xor(sp, off);      // butterfly: every lane holds the same sum
    if (lane == 0) {
        float zz[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        double lpz = 0.0;
        for (int d = 0; d < a.D; ++d) {
            zz[d] = valid ? a.z[(size_t)g * a.D + d] : 0.0f;
            lpz += -0.5 * (double)zz[d] * (double)zz[d] - 0.5 * GRID_LOG2PI;
        }
        const float w = (valid && a.lw) ? a.lw[g] : 0.0f;
        a.c[g] = valid ? (float)(lpz - sp + (double)w) : 0.0f;
        a.zc[g] = make_float4(zz[0], zz[1], zz[2], zz[3]);
        a.w[g] = w;
    }
}

template <int D>
struct GridState {
    float m, s, S1[D], S2[D * (D + 1) / 2], Q, A;
};
template <int D>
__device__ __forceinline__ int tri(int d, int e) { return d * D - d * (d - 1) / 2 + (e - d); }

// merge the state of the lane `off` away into this lane's (both about the same mu)
template <int D>
__device__ __forceinline__ void merge_xor(GridState<D>& st, int off) {
    const float m2 = __shfl_xor(st.m, off);
    const float M = fmaxf(st.m, m2);
    const float a1 = st.m == -INFINITY ? 0.0f : __expf(st.m - M);
    const float a2 = m2 == -INFINITY ? 0.0f : __expf(m2 - M);
    st.s = st.s * a1 + __shfl_xor(st.s, off) * a2;
#pragma unroll
    for (int d = 0; d < D; ++d) st.S1[d] = st.S1[d] * a1 + __shfl_xor(st.S1[d], off) * a2;
#pragma unroll
    for (int t = 0; t < D * (D + 1) / 2; ++t) st.S2[t] = st.S2[t] * a1 + __shfl_xor(st.S2[t], off) * a2;
    st.Q += __shfl_xor(st.Q, off);
    st.A += __shfl_xor(st.A, off);
    st.m = M;
}

// Workgroup = 4 waves x 16 images (wave w: images 64 blockIdx.x + 16 w ..), one range of GRID_RANGE grid rows (blockIdx.y).
// A wave keeps the B operand (x of its 16 images, all k-steps) in registers; the A operand (16 grid rows of L_hi and L_lo) is
// staged in LDS in fragment order once per 16-row tile for the four waves.  Accumulator: lane (r = lane & 15, q = lane >> 4)
// reg i = S[grid row 4q + i][image r], so a lane scores ONE image against 4 grid rows per tile and keeps that image's online
// state; the four lanes of an image merge theirs at the end of the range (lane xor 16, then xor 32: the same order for every image).
template <int D>
__global__ __launch_bounds__(256) void grid_score_kernel(GridScoreArgs a) {
    extern __shared__ uint4 lfrag[];      // [2 (hi, lo)][KT][64 lanes]
    constexpr int KTM = GRID_XP_MAX / 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4;
    const int KT = a.Xp / 32;
    const int img = blockIdx.x * 64 + wave * 16 + (lane & 15);
    const int g_begin = blockIdx.y * GRID_RANGE, g_end = min(a.Gc, g_begin + GRID_RANGE);
    uint4 xf[KTM];
#pragma unroll
    for (int s = 0; s < KTM; ++s)
        xf[s] = s < KT ? *(const uint4*)(a.XB + (size_t)img * a.Xp + 32 * s + 8 * q) : make_uint4(0, 0, 0, 0);
    const int ic = min(img, a.N - 1);      // (pad images score image N-1's heads; their results are never written)
    float mu[D], isg[D], lqc = -0.5f * (float)D * (float)GRID_LOG2PI;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        mu[d] = a.head[(size_t)ic * a.ldh + d];
        const float sg = a.head[(size_t)ic * a.ldh + a.soff + d];
        isg[d] = 1.0f / sg;
        lqc -= logf(sg);
    }
    GridState<D> st;
    st.m = -INFINITY; st.s = 0.0f; st.Q = 0.0f; st.A = 0.0f;
#pragma unroll
    for (int d = 0; d < D; ++d) st.S1[d] = 0.0f;
#pragma unroll
    for (int t = 0; t < D * (D + 1) / 2; ++t) st.S2[t] = 0.0f;
    const int nfrag = 2 * KT * 64;
    for (int t0 = g_begin; t0 < g_end; t0 += 16) {
        __syncthreads();      // the previous tile's fragments are consumed
        for (int f = threadIdx.x; f < nfrag; f += 256) {
            const int hl = f >= KT * 64, r = hl ? f - KT * 64 : f, s = r >> 6, l = r & 63;
            const uint16_t* src = (hl ? a.Llo : a.Lhi) + (size_t)(t0 + (l & 15)) * a.Xp + 32 * s + 8 * (l >> 4);
            lfrag[f] = *(const uint4*)src;
        }
        __syncthreads();
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < KTM; ++s) {
            if (s < KT) {
                acc = mfma16(lfrag[s * 64 + lane], xf[s], acc);
                acc = mfma16(lfrag[(KT + s) * 64 + lane], xf[s], acc);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int g = t0 + 4 * q + i;
            if (g >= g_end) continue;
            const float t = acc[i] + a.c[g];      // lj + w
            if (!(t > -INFINITY)) continue;       // zero-weight point (w = -inf)
            const float wg = a.w[g];
            const float4 z4 = a.zc[g];
            const float zv[4] = {z4.x, z4.y, z4.z, z4.w};
            float dz[D], lq = lqc;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                dz[d] = zv[d] - mu[d];
                const float u = dz[d] * isg[d];
                lq -= 0.5f * u * u;
            }
            const float lj = t - wg;
            if (a.log_joint && img < a.N) a.log_joint[(size_t)img * a.ldlj + a.lj_col + g] = lj;
            const float eq = __expf(lq + wg);
            st.Q += eq;
            st.A += eq * (lq - lj);
            if (t > st.m) {
                const float sc = __expf(st.m - t);      // (0 for the first point: m = -inf)
                st.s *= sc;
#pragma unroll
                for (int d = 0; d < D; ++d) st.S1[d] *= sc;
#pragma unroll
                for (int u = 0; u < D * (D + 1) / 2; ++u) st.S2[u] *= sc;
                st.m = t;
            }
            const float e = __expf(t - st.m);
            st.s += e;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const float ed = e * dz[d];
                st.S1[d] += ed;
#pragma unroll
                for (int f = d; f < D; ++f) st.S2[tri<D>(d, f)] += ed * dz[f];
            }
        }
    }
    merge_xor(st, 16);
    merge_xor(st, 32);
    if (q == 0 && img < a.N) {
        float o[GRID_ST];
#pragma unroll
        for (int j = 0; j < GRID_ST; ++j) o[j] = 0.0f;      // (slots of latent dimensions >= D stay 0)
        o[0] = st.m; o[1] = st.s; o[GRID_Q] = st.Q; o[GRID_A] = st.A;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            o[GRID_S1 + d] = st.S1[d];
#pragma unroll
            for (int f = d; f < D; ++f) o[GRID_S2 + grid_tri(d, f)] = st.S2[tri<D>(d, f)];
        }
        float* dst = a.part + ((size_t)blockIdx.y * a.N + img) * GRID_ST;
#pragma unroll
        for (int j = 0; j < GRID_ST; ++j) dst[j] = o[j];
    }
}

// one thread per image: the chunk's partial states in split order into the running state (double); the last chunk finalises
__global__ __launch_bounds__(256) void grid_merge_kernel(GridMergeArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    double st[GRID_ST];
    double* run = a.run + (size_t)i * GRID_ST;
    if (a.first) {
        for (int j = 0; j < GRID_ST; ++j) st[j] = 0.0;
        st[0] = -INFINITY;
    } else {
        for (int j = 0; j < GRID_ST; ++j) st[j] = run[j];
    }
    for (int sp = 0; sp < a.nsplit; ++sp) {
        const float* p = a.part + ((size_t)sp * a.N + i) * GRID_ST;
        const double m2 = p[0];
        if (m2 == -INFINITY) continue;      // (a range with no finite point)
        const double M = fmax(st[0], m2);
        const double a1 = st[0] == -INFINITY ? 0.0 : exp(st[0] - M), a2 = exp(m2 - M);
        for (int j = 1; j < GRID_Q; ++j) st[j] = st[j] * a1 + (double)p[j] * a2;
        st[GRID_Q] += p[GRID_Q];
        st[GRID_A] += p[GRID_A];
        st[0] = M;
    }
    if (!a.last) {
        for (int j = 0; j < GRID_ST; ++j) run[j] = st[j];
        return;
    }
    const double lpx = st[0] + log(st[1]);
    a.log_px[i] = lpx;
    const double inv = 1.0 / st[1];
    for (int d = 0; d < a.D; ++d) {
        const double md = st[GRID_S1 + d] * inv;
        if (a.mean) a.mean[(size_t)i * a.D + d] = (float)((double)a.head[(size_t)i * a.ldh + d] + md);
        if (a.cov)
            for (int e = 0; e < a.D; ++e) {
                const int lo = d < e ? d : e, hi = d < e ? e : d;
                const double me = st[GRID_S1 + e] * inv;
                a.cov[((size_t)i * a.D + d) * a.D + e] = (float)(st[GRID_S2 + grid_tri(lo, hi)] * inv - md * me);
            }
    }
    if (a.qmass) a.qmass[i] = (float)st[GRID_Q];
    if (a.kl) a.kl[i] = (float)(st[GRID_A] + st[GRID_Q] * lpx);      // sum q w (lq - lj + log p(x)) = KL(q || p(z|x)) on the grid
}

}  // namespace

void launch_grid_prep_x(const float* x, int N, int X, int Np, int Xp, uint16_t* XB, int* nonbinary, hipStream_t st) {
    const long n = (long)Np * (Xp / 8);
    hipLaunchKernelGGL(grid_prep_x_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, N, X, Np, Xp, XB, nonbinary);
}

void launch_grid_prep(const GridPrepArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(grid_prep_kernel, dim3((unsigned)((a.Gcp + 3) / 4)), dim3(256), 0, st, a);
}

void launch_grid_score(const GridScoreArgs& a, int D, hipStream_t st) {
    const dim3 grid((unsigned)((a.N + 63) / 64), (unsigned)a.nsplit);
    const size_t lds = (size_t)2 * (a.Xp / 32) * 64 * sizeof(uint4);
    switch (D) {
        case 1: hipLaunchKernelGGL(grid_score_kernel<1>, grid, dim3(256), lds, st, a); break;
        case 2: hipLaunchKernelGGL(grid_score_kernel<2>, grid, dim3(256), lds, st, a); break;
        case 3: hipLaunchKernelGGL(grid_score_kernel<3>, grid, dim3(256), lds, st, a); break;
        default: hipLaunchKernelGGL(grid_score_kernel<4>, grid, dim3(256), lds, st, a); break;
    }
}

void launch_grid_merge(const GridMergeArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(grid_merge_kernel, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, st, a);
}

}  // namespace iwae
