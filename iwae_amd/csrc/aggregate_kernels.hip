// Aggregate-posterior decomposition of the KL term (iwae_aggregate_posterior, include/iwae_amd.h; Hoffman & Johnson 2016, Chen et al. 2018):
// the densities of the samples z_i = mu_n + sigma_n eps_{s,n} (i = s N + n) under q(z) = (1/N) sum_m q(z|x_m) and under its per-unit marginals.
//   agg_comp_kernel     heads -> component tables [N][Dpad]: mu, a / sigma (float and double), -log2(e) (log sigma + c), and the latter's sum
//                       over d in double (log2 units, a^2 = log2(e)/2)
//   agg_sample_kernel   heads + eps -> z and the own-component term of every unit, transposed [Dpad][T] so that a lane = a sample reads them coalesced
//   agg_dim_kernel      per-unit sums   sum_m exp2(l2(i|m,d) - l2(i|own,d))   over one component range and 16 units, a lane = a sample
//   agg_joint_kernel    running (max, sum) of   sum_d l2(i|m,d)   over one component range, a lane = a sample
//   agg_merge_kernel    component ranges folded in range order -> log_qz [T], log_qzd [Dpad][T]
//   agg_reduce_kernel / agg_finish_kernel   the per-unit and summary sums in double; lq_own and lp are evaluated in double there
// Blocking and determinism: a lane owns one sample and walks the components in index order, so the accumulators of
// a sample exist once (not once per lane) and no cross-lane merge is needed; the component values are wave-uniform and arrive through the
// scalar cache.  A sample's results depend on N (which fixes the ranges), the N heads and its own eps only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "kernels.h"
#include "device_helpers.h"

namespace iwae {
namespace {

#define AGG_LOG2E 1.4426950408889634
#define AGG_LN2 0.6931471805599453
#define AGG_HALF_LOG_2PI 0.9189385332046727
constexpr int AGG_THREADS = 256;

// component tables: a pad unit (d >= D) gets mu = 0, inv = 0, nls = 0 and therefore the term l2 = 0 for every sample (whose pad z is 0)
__global__ __launch_bounds__(AGG_THREADS) void agg_comp_kernel(AggCompArgs a) {
    const int m = blockIdx.x * AGG_THREADS + threadIdx.x;
    if (m >= a.N) return;
    const float* h = a.head + (size_t)m * a.ldh;
    const double ascale_d = 0.8493218002880191;       // sqrt(log2(e) / 2)
    const float ascale = (float)ascale_d;
    double tot = 0.0;
    for (int d = 0; d < a.Dpad; ++d) {
        float mu = 0.0f, inv = 0.0f, nls = 0.0f;
        double invd = 0.0;
        if (d < a.D) {
            const float sg = h[a.soff + d];
            mu = h[d];
            inv = ascale / sg;
            nls = -(float)AGG_LOG2E * (logf(sg) + (float)AGG_HALF_LOG_2PI);
            invd = ascale_d / (double)sg;
            tot -= AGG_LOG2E * (log((double)sg) + AGG_HALF_LOG_2PI);
        }
        const size_t o = (size_t)m * a.Dpad + d;
        a.mu[o] = mu; a.inv[o] = inv; a.nls[o] = nls; a.invd[o] = invd;
    }
    a.nls_sum[m] = tot;
}

// the one expression every kernel evaluates a term with (log2 units): the own-component shift of agg_sample_kernel equals bit for bit the
// term agg_dim_kernel finds at m = n, so that term contributes exactly exp2(0) = 1
__device__ __forceinline__ float agg_term(float z, float mu, float inv, float nls) {
    const float t = (z - mu) * inv;
    return fmaf(-t, t, nls);
}

// samples i0 .. i0 + T - 1 of the call: zT[d][j], shT[d][j], j = i - i0; the thread index runs over j first (coalesced stores)
__global__ __launch_bounds__(AGG_THREADS) void agg_sample_kernel(AggSampleArgs a) {
    const long idx = (long)blockIdx.x * AGG_THREADS + threadIdx.x;
    if (idx >= (long)a.T * a.Dpad) return;
    const int j = (int)(idx % a.T), d = (int)(idx / a.T);
    float z = 0.0f, sh = 0.0f;
    if (d < a.D) {
        const long i = a.i0 + j;
        const int n = (int)(i % a.N);
        const float* h = a.head + (size_t)n * a.ldh;
        z = fmaf(h[a.soff + d], a.eps[(size_t)i * a.D + d], h[d]);
        const size_t o = (size_t)n * a.Dpad + d;
        sh = agg_term(z, a.mu[o], a.inv[o], a.nls[o]);
    }
    a.zT[(size_t)d * a.T + j] = z;
    a.shT[(size_t)d * a.T + j] = sh;
}

// agg_dim_kernel: block (x, y, z) = (256 samples, component range y, units 16 z .. 16 z + 15).  The component index is uniform over the
// block, so mu / inv / nls are scalar loads; per term: sub, mul, fma, sub, exp2, add.  A lane past T computes on a clamped sample and
// stores nothing.
__global__ __launch_bounds__(AGG_THREADS) void agg_dim_kernel(AggMainArgs a) {
    const int j = blockIdx.x * AGG_THREADS + threadIdx.x;
    const int jc = min(j, a.T - 1);
    const int d0 = blockIdx.z * AGG_DC;
    const int m0 = blockIdx.y * AGG_RANGE, m1 = min(a.N, m0 + AGG_RANGE);
    float z[AGG_DC], sh[AGG_DC], acc[AGG_DC];
#pragma unroll
    for (int q = 0; q < AGG_DC; ++q) {
        z[q] = a.zT[(size_t)(d0 + q) * a.T + jc];
        sh[q] = a.shT[(size_t)(d0 + q) * a.T + jc];
        acc[q] = 0.0f;
    }
    const float* __restrict__ mu = a.mu + d0;
    const float* __restrict__ inv = a.inv + d0;
    const float* __restrict__ nls = a.nls + d0;
    for (int m = m0; m < m1; ++m) {
        const size_t o = (size_t)m * a.Dpad;
#pragma unroll
        for (int q = 0; q < AGG_DC; ++q)
            acc[q] += __builtin_amdgcn_exp2f(agg_term(z[q], mu[o + q], inv[o + q], nls[o + q]) - sh[q]);
    }
    if (j < a.T) {
#pragma unroll
        for (int q = 0; q < AGG_DC; ++q) a.dim_part[((size_t)blockIdx.y * a.Dpad + d0 + q) * a.T + j] = acc[q];
    }
}

// agg_joint_kernel: block (x, y) = (256 samples, component range y); the sample's z stays in registers (NCH * 16 units).  The joint
// term of a component is a sum of up to 128 unit terms of magnitude ~1 whose total is ~-150: summed in float32 its rounding alone (~1e-5)
// would exceed what mi = 0 for a single component demands, so z - mu (float32) is widened and scaled, squared and accumulated in double
// in two chains (what that costs is measured, not assumed: DESIGN.md section 14).  The result is folded into a running (max, sum); the maximum starts at a
// finite floor, so no inf - inf can arise.
template <int NCH>
__global__ __launch_bounds__(AGG_THREADS) void agg_joint_kernel(AggMainArgs a) {
    constexpr int DP = NCH * AGG_DC;
    const int j = blockIdx.x * AGG_THREADS + threadIdx.x;
    const int jc = min(j, a.T - 1);
    const int m0 = blockIdx.y * AGG_RANGE, m1 = min(a.N, m0 + AGG_RANGE);
    float z[DP];
#pragma unroll
    for (int d = 0; d < DP; ++d) z[d] = a.zT[(size_t)d * a.T + jc];
    const float* __restrict__ mu = a.mu;
    const double* __restrict__ inv = a.invd;
    double mx = -3.0e38;
    float sum = 0.0f;
    for (int m = m0; m < m1; ++m) {
        const size_t o = (size_t)m * DP;
        double c[2] = {0.0, 0.0};
#pragma unroll
        for (int d = 0; d < DP; ++d) {
            const double t = (double)(z[d] - mu[o + d]) * inv[o + d];
            c[d & 1] = fma(-t, t, c[d & 1]);
        }
        const double J = (c[0] + c[1]) + a.nls_sum[m];
        const double nm = fmax(mx, J);
        sum = fmaf(sum, __builtin_amdgcn_exp2f((float)(mx - nm)), __builtin_amdgcn_exp2f((float)(J - nm)));
        mx = nm;
    }
    if (j < a.T) {
        a.joint_max[(size_t)blockIdx.y * a.T + j] = mx;
        a.joint_sum[(size_t)blockIdx.y * a.T + j] = sum;
    }
}

// agg_merge_kernel: thread = (row r, sample j); rows 0 .. Dpad-1 are the units (range sums added in range order: they share the sample's
// fixed shift), row Dpad the joint density (ranges merged under their common maximum, in range order).  The logarithm of the sum, log2 -> nat
// and - log N are in double: the hardware log2's error is the same for every sample with the same sum (all of them when the components
// coincide), and tc adds it up over D units.
__global__ __launch_bounds__(AGG_THREADS) void agg_merge_kernel(AggMergeArgs a) {
    const long idx = (long)blockIdx.x * AGG_THREADS + threadIdx.x;
    if (idx >= (long)a.T * (a.Dpad + 1)) return;
    const int j = (int)(idx % a.T), r = (int)(idx / a.T);
    if (r < a.Dpad) {
        float s = 0.0f;
        for (int p = 0; p < a.P; ++p) s += a.dim_part[((size_t)p * a.Dpad + r) * a.T + j];
        const double v = ((double)a.shT[(size_t)r * a.T + j] + log2((double)s)) * AGG_LN2 - a.log_n;
        a.log_qzdT[(size_t)r * a.ldo + a.i0 + j] = (float)v;
    } else {
        double mx = a.joint_max[j];
        for (int p = 1; p < a.P; ++p) mx = fmax(mx, a.joint_max[(size_t)p * a.T + j]);
        float s = 0.0f;
        for (int p = 0; p < a.P; ++p) s = fmaf(a.joint_sum[(size_t)p * a.T + j], __builtin_amdgcn_exp2f((float)(a.joint_max[(size_t)p * a.T + j] - mx)), s);
        const double v = (mx + log2((double)s)) * AGG_LN2 - a.log_n;
        a.log_qz[a.i0 + j] = (float)v;
    }
}

// [Dpad][SN] -> the caller's [SN][D]
__global__ __launch_bounds__(AGG_THREADS) void agg_untranspose_kernel(const float* src, long SN, int D, float* dst) {
    const long idx = (long)blockIdx.x * AGG_THREADS + threadIdx.x;
    if (idx >= SN * D) return;
    const long i = idx / D;
    const int d = (int)(idx % D);
    dst[idx] = src[(size_t)d * SN + i];
}

// agg_reduce_kernel: block d < D sums over the samples of unit d, in double: lq_own - log_qzd, log_qzd - lp, lq_own - lp, lq_own, log_qzd
// (lq_own = -eps^2/2 - log sigma - c and lp = -z^2/2 - c, z = mu + sigma eps, evaluated in double from the float32 heads and draws);
// block D sums log_qz.  Thread t takes samples t, t + 256, ...; the 256 thread sums are folded by a fixed tree: the order depends on (N, S).
__global__ __launch_bounds__(AGG_THREADS) void agg_reduce_kernel(AggReduceArgs a) {
    __shared__ double sh[AGG_THREADS];
    const int d = blockIdx.x;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (d < a.D) {
        for (long i = threadIdx.x; i < a.SN; i += AGG_THREADS) {
            const int n = (int)(i % a.N);
            const float* h = a.head + (size_t)n * a.ldh;
            const double mu = (double)h[d], sg = (double)h[a.soff + d], e = (double)a.eps[(size_t)i * a.D + d];
            const double z = mu + sg * e;
            const double lq = -0.5 * e * e - log(sg) - AGG_HALF_LOG_2PI;
            const double lp = -0.5 * z * z - AGG_HALF_LOG_2PI;
            const double qd = (double)a.log_qzdT[(size_t)d * a.SN + i];
            s[0] += lq - qd; s[1] += qd - lp; s[2] += lq - lp; s[3] += lq; s[4] += qd;
        }
    } else {
        for (long i = threadIdx.x; i < a.SN; i += AGG_THREADS) s[0] += (double)a.log_qz[i];
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const double r = tree_sum_256(s[q], sh);
        if (threadIdx.x == 0) a.part[(size_t)d * 5 + q] = r;
    }
}

// agg_finish_kernel (one thread): the block sums -> unit_mi, unit_kl [D] and summary = {mi, tc, dim_kl, kl}, units in index order
__global__ void agg_finish_kernel(AggReduceArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double cnt = (double)a.SN;
    double dim_kl = 0.0, k = 0.0, lq = 0.0, qd = 0.0;
    for (int d = 0; d < a.D; ++d) {
        const double* p = a.part + (size_t)d * 5;
        a.unit_mi[d] = p[0] / cnt;
        a.unit_kl[d] = p[1] / cnt;
        dim_kl += p[1] / cnt;
        k += p[2]; lq += p[3]; qd += p[4];
    }
    const double qz = a.part[(size_t)a.D * 5];
    a.summary[0] = (lq - qz) / cnt;
    a.summary[1] = (qz - qd) / cnt;
    a.summary[2] = dim_kl;
    a.summary[3] = k / cnt;
}

}  // namespace

void launch_agg_comp(const AggCompArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(agg_comp_kernel, dim3((a.N + AGG_THREADS - 1) / AGG_THREADS), dim3(AGG_THREADS), 0, st, a);
}
void launch_agg_sample(const AggSampleArgs& a, hipStream_t st) {
    const long n = (long)a.T * a.Dpad;
    hipLaunchKernelGGL(agg_sample_kernel, dim3((unsigned)((n + AGG_THREADS - 1) / AGG_THREADS)), dim3(AGG_THREADS), 0, st, a);
}
void launch_agg_main(const AggMainArgs& a, hipStream_t st) {
    const int nx = (a.T + AGG_THREADS - 1) / AGG_THREADS, P = (a.N + AGG_RANGE - 1) / AGG_RANGE, nch = a.Dpad / AGG_DC;
    hipLaunchKernelGGL(agg_dim_kernel, dim3(nx, P, nch), dim3(AGG_THREADS), 0, st, a);
    const dim3 g(nx, P), b(AGG_THREADS);
    switch (nch) {
        case 1: hipLaunchKernelGGL(agg_joint_kernel<1>, g, b, 0, st, a); break;
        case 2: hipLaunchKernelGGL(agg_joint_kernel<2>, g, b, 0, st, a); break;
        case 3: hipLaunchKernelGGL(agg_joint_kernel<3>, g, b, 0, st, a); break;
        case 4: hipLaunchKernelGGL(agg_joint_kernel<4>, g, b, 0, st, a); break;
        case 5: hipLaunchKernelGGL(agg_joint_kernel<5>, g, b, 0, st, a); break;
        case 6: hipLaunchKernelGGL(agg_joint_kernel<6>, g, b, 0, st, a); break;
        case 7: hipLaunchKernelGGL(agg_joint_kernel<7>, g, b, 0, st, a); break;
        default: hipLaunchKernelGGL(agg_joint_kernel<8>, g, b, 0, st, a); break;
    }
}
void launch_agg_merge(const AggMergeArgs& a, hipStream_t st) {
    const long n = (long)a.T * (a.Dpad + 1);
    hipLaunchKernelGGL(agg_merge_kernel, dim3((unsigned)((n + AGG_THREADS - 1) / AGG_THREADS)), dim3(AGG_THREADS), 0, st, a);
}
void launch_agg_untranspose(const float* src, long SN, int D, float* dst, hipStream_t st) {
    hipLaunchKernelGGL(agg_untranspose_kernel, dim3((unsigned)((SN * D + AGG_THREADS - 1) / AGG_THREADS)), dim3(AGG_THREADS), 0, st, src, SN, D, dst);
}
void launch_agg_reduce(const AggReduceArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(agg_reduce_kernel, dim3(a.D + 1), dim3(AGG_THREADS), 0, st, a);
    hipLaunchKernelGGL(agg_finish_kernel, dim3(1), dim3(1), 0, st, a);
}

}  // namespace iwae
