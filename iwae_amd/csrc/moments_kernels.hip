// Per-parameter gradient moments (iwae_grad_moments, include/iwae_amd.h; Rainforth et al. 2018, Tucker et al. 2019): the mean and the
// unbiased variance of the flat float32 gradient over M draws of the training estimator.
//   moments_fold_kernel      one Welford update per draw, in double: draw 1 sets mean = g, M2 = 0; draw j > 1 applies
//                            mean += (g - mean) / j and M2 += (g - mean_old)(g - mean_new)
//   moments_finalize_kernel  var = M2 / (M - 1); mean copied out when the caller's buffer is not the workspace
// Every element is independent and no atomics are used: the results are bitwise reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace iwae {
namespace {

#define MOM_THREADS 256
#define MOM_MAX_BLOCKS 1024      // 256 CUs x 4 workgroups; larger gradients are walked grid-stride

__device__ __forceinline__ void welford(double g, double& mean, double& m2, bool first, double j) {
    if (first) { mean = g; m2 = 0.0; return; }
    const double d = g - mean;
    const double mn = mean + d / j;      // (a true division, as the float64 reference fold does)
    m2 += d * (g - mn);
    mean = mn;
}

__global__ __launch_bounds__(MOM_THREADS) void moments_fold_kernel(MomentsFoldArgs a) {
    const bool first = a.j == 1;
    const double j = (double)a.j;
    const size_t n4 = a.n / 4;
    const size_t stride = (size_t)gridDim.x * MOM_THREADS;
    for (size_t i = (size_t)blockIdx.x * MOM_THREADS + threadIdx.x; i < n4; i += stride) {
        const float4 g = reinterpret_cast<const float4*>(a.g)[i];          // 16-B loads of the gradient and of the two double arrays
        double2* mp = reinterpret_cast<double2*>(a.mean) + 2 * i;
        double2* qp = reinterpret_cast<double2*>(a.m2) + 2 * i;
        double2 m0 = first ? make_double2(0.0, 0.0) : mp[0], m1 = first ? make_double2(0.0, 0.0) : mp[1];
        double2 q0 = first ? make_double2(0.0, 0.0) : qp[0], q1 = first ? make_double2(0.0, 0.0) : qp[1];
        welford(g.x, m0.x, q0.x, first, j);
        welford(g.y, m0.y, q0.y, first, j);
        welford(g.z, m1.x, q1.x, first, j);
        welford(g.w, m1.y, q1.y, first, j);
        mp[0] = m0; mp[1] = m1;
        qp[0] = q0; qp[1] = q1;
    }
    // the last n % 4 elements
    const size_t t = (size_t)blockIdx.x * MOM_THREADS + threadIdx.x;
    if (t < a.n - 4 * n4) {
        const size_t e = 4 * n4 + t;
        double m = first ? 0.0 : a.mean[e], q = first ? 0.0 : a.m2[e];
        welford(a.g[e], m, q, first, j);
        a.mean[e] = m; a.m2[e] = q;
    }
}

__global__ __launch_bounds__(MOM_THREADS) void moments_finalize_kernel(MomentsFinalizeArgs a) {
    const double den = (double)(a.M - 1);
    const size_t stride = (size_t)gridDim.x * MOM_THREADS;
    for (size_t i = (size_t)blockIdx.x * MOM_THREADS + threadIdx.x; i < a.n; i += stride) {
        if (a.out_mean) a.out_mean[i] = a.mean[i];
        a.out_var[i] = a.m2[i] / den;
    }
}

unsigned mom_blocks(size_t work) {
    const size_t b = (work + MOM_THREADS - 1) / MOM_THREADS;
    return (unsigned)(b < 1 ? 1 : b > MOM_MAX_BLOCKS ? MOM_MAX_BLOCKS : b);
}

}  // namespace

void launch_moments_fold(const MomentsFoldArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(moments_fold_kernel, dim3(mom_blocks(a.n / 4 > 0 ? a.n / 4 : 1)), dim3(MOM_THREADS), 0, st, a);
}
void launch_moments_finalize(const MomentsFinalizeArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(moments_finalize_kernel, dim3(mom_blocks(a.n)), dim3(MOM_THREADS), 0, st, a);
}

}  // namespace iwae
