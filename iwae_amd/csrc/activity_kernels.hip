// Active units (iwae_latent_activity, include/iwae_amd.h; Burda et al. section 5.2): A_u = Cov_x(E_q[u|x]) per latent unit.
//   act_chain_kernel     2-layer model, bf16 eval precision, the reference's shape: z1 draws -> q(z2|z1) block -> mu2, summed over
//                        each (image, 128-sample block) in the workgroup; only the block's partial sum reaches HBM
//   act_partial_kernel   the same partials from mu2 rows that composed launches made (other shapes, float32 mode)
//   act_stats_kernel     partials -> per-image means (double) -> data mean and centred second moment per unit, fixed order
// Determinism: a partial depends only on its image, its samples' draws and the weights; the per-image
// fold runs in block order and the statistics in an order fixed by N alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>
#include "kernels.h"
#include "layout.h"
#include "device_helpers.h"

namespace iwae {
namespace {

// 4 draws for features 4*d4 .. +3 of sample s of image b: the user's [k][B][D] draws or Philox keyed as iwae_eval_llh keys them
// (k_total set: row = row_offset + b * k_total + s_off + s)
__device__ __forceinline__ void aeps4(const EpsSrc& e, int b, int s, int d4, int D, float n[4]) {
    if (e.user) {
        const float* p = e.user + ((size_t)s * e.B + b) * D + 4 * d4;
#pragma unroll
        for (int i = 0; i < 4; ++i) n[i] = (4 * d4 + i < D) ? p[i] : 0.0f;
    } else {
        normal4(e.row_offset + (uint64_t)b * (uint64_t)e.k_total + (uint64_t)(e.s_off + s), (uint32_t)d4, e.stream, e.step, e.seed, n);
    }
}

// ---------------------------------------------------------------------------------
// act_chain_kernel: one workgroup = one (image, ACT_BLOCK-sample block); wave w owns samples 16w .. 16w+15 of the block, lane
// (rho, q) sample rho and the features layout.h gives it.  z1 = mu1 + sigma1*eps1 (iwae2.py:61) goes straight into the q(z2|z1)
// block's first layer (iwae2.py:63-64), the tanh layers' converted accumulators are the next layer's operand, and the mu2 head
// accumulators (the sigma head is not needed) are summed over the block's valid samples: across the 16 lanes of a quad with
// shuffles, then across the 8 waves in LDS in wave order.  The weights stream through two LDS buffers one 64-out-feature group at a
// time, as in chain2_fwd_kernel, whose arithmetic (z1 in fp32 -> bf16, tanh_fast -> bf16, fp32 head) this restates.
// ---------------------------------------------------------------------------------
template <int KT0, int KTH, int KT1>
__global__ __launch_bounds__(512, 4) void act_chain_kernel(ActChainArgs a) {
    static_assert(KT0 % 2 == 0 && KT1 % 2 == 0 && KT0 <= 4 && KTH <= 4 && KT1 <= 4, "64-feature latent groups, <= 128 features everywhere");
    static_assert(ACT_BLOCK == 128, "8 waves x 16 samples");
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    constexpr int NWV = 8;
    constexpr int KTMAX = KT0 > KTH ? KT0 : KTH;
    constexpr int UNIT = KTMAX * 4096 + 1024, NIDX = (4 * KTMAX + 1 + NWV - 1) / NWV;
    constexpr int MGH = (KTH + 1) / 2;                       // 64-feature groups of a hidden layer
    constexpr int NG = KT1 / 2;                              // 64-feature groups of mu2 (the head's first NG groups)
    constexpr int U_E2 = MGH, U_EH = 2 * MGH, NUNITS = U_EH + NG;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rho = lane & 15, q = lane >> 4;
    const int b = blockIdx.y, blk = blockIdx.x;
    const int s = blk * ACT_BLOCK + wave * 16 + rho;          // the lane's sample inside this launch's kn
    const bool valid = s < a.kn;
    const int sc = min(s, a.kn - 1);
    const int a_off = rho * 64 + ((q ^ hperm(rho >> 2)) * 16);
    float* red = (float*)(smem + 2 * UNIT);                  // [NWV][64 * NG] per-wave sums

    auto dma_unit = [&](int uu, int buf) {                 // uu wave-uniform
        const char* src; int kt;
        if (uu < U_E2) { src = a.img1 + (size_t)uu * img_mg_group_bytes(KT0); kt = KT0; }
        else if (uu < U_EH) { src = a.img2 + (size_t)(uu - U_E2) * img_mg_group_bytes(KTH); kt = KTH; }
        else { src = a.imgh + (size_t)(uu - U_EH) * img_mg_group_bytes(KTH); kt = KTH; }
        const int npc = 4 * kt + 1;
#pragma unroll
        for (int idx = 0; idx < NIDX; ++idx) {
            const int p = wave + NWV * idx;
            if (p < npc)
                glds16(src + (size_t)p * 1024 + lane * 16, (uint32_t)__builtin_amdgcn_readfirstlane((int)(lds_addr_of(smem + buf * UNIT) + (uint32_t)p * 1024u)));
        }
    };
    dma_unit(0, 0);
    // ---- z1 = mu1 + sigma1 * eps1 of this sample (iwae2.py:61) as bf16 B-operand fragments
    uint4 zf[KT0];
    {
        const float* hz = a.head1 + (size_t)b * a.ldH1;
#pragma unroll
        for (int ks = 0; ks < KT0; ++ks) {
            float z8[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int f0 = 32 * ks + 16 * h + 4 * q;
                float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (f0 < a.D0) aeps4(a.eps1, b, sc, f0 >> 2, a.D0, e);
                const float4 mu4 = *(const float4*)(hz + f0), sg4 = *(const float4*)(hz + 32 * KT0 + f0);   // (inside the padded head row)
                float muv[4] = {mu4.x, mu4.y, mu4.z, mu4.w}, sgv[4] = {sg4.x, sg4.y, sg4.z, sg4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const bool in = f0 + i < a.D0;
                    z8[4 * h + i] = in ? fmaf(sgv[i], e[i], muv[i]) : 0.0f;
                }
            }
            zf[ks] = make_uint4(pack2(z8[0], z8[1]), pack2(z8[2], z8[3]), pack2(z8[4], z8[5]), pack2(z8[6], z8[7]));
        }
    }
    int u = 0;
    auto unit_mfma = [&](auto kt_tag, const uint4* bin, f32x4 (&acc)[4]) {
        constexpr int KTin = decltype(kt_tag)::value;
        const int buf = u & 1;
        wait_all_vmem();
        __syncthreads();
        if (u + 1 < NUNITS) dma_unit(u + 1, buf ^ 1);
        const char* lb = smem + buf * UNIT + a_off;
        const char* lbias = smem + buf * UNIT + KTin * 4096 + q * 16;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float4 c = *(const float4*)(lbias + 64 * t);
            acc[t] = (f32x4){c.x, c.y, c.z, c.w};
        }
        uint4 av[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) av[i] = *(const uint4*)(lb + i * 1024);
#pragma unroll
        for (int i = 0; i < KTin * 4; ++i) {
            acc[i & 3] = mfma16(av[i & 3], bin[i >> 2], acc[i & 3]);
            if (i + 4 < KTin * 4) av[i & 3] = *(const uint4*)(lb + (i + 4) * 1024);
        }
        ++u;
    };
    auto tanh_layer = [&](auto kt_tag, const uint4* bin, uint4 (&bout)[KTH]) {
#pragma unroll
        for (int mg = 0; mg < MGH; ++mg) {
            f32x4 acc[4];
            unit_mfma(kt_tag, bin, acc);
#pragma unroll
            for (int p2 = 0; p2 < 2; ++p2) {
                const int kso = 2 * mg + p2;
                if (kso < KTH) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = tanh_fast(acc[2 * p2 + (j >> 2)][j & 3]);
                    bout[kso] = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
                }
            }
        }
    };
    uint4 h1f[KTH], h2f[KTH];
    tanh_layer(std::integral_constant<int, KT0>{}, zf, h1f);
    tanh_layer(std::integral_constant<int, KTH>{}, h1f, h2f);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        f32x4 mu2[4];
        unit_mfma(std::integral_constant<int, KTH>{}, h2f, mu2);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v = valid ? mu2[t][i] : 0.0f;           // (tail samples of a partial block carry a clamped sample's values)
                v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
                if (rho == 0) red[wave * (64 * NG) + 64 * g + 16 * t + 4 * q + i] = v;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 64 * NG && (int)threadIdx.x < a.D1) {
        float acc = 0.0f;
#pragma unroll
        for (int w = 0; w < NWV; ++w) acc += red[w * (64 * NG) + threadIdx.x];
        a.part[((size_t)(a.img0 + b) * a.nblk + a.blk0 + blk) * a.D1 + threadIdx.x] = acc;
    }
}

// act_partial_kernel: the same partials from materialised mu2 rows [nb * kn][ldh] (row = b * kn + s), one thread per
// (image, block, unit), samples in index order in fp32
__global__ __launch_bounds__(256) void act_partial_kernel(ActPartialArgs a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int nbl = (a.kn + ACT_BLOCK - 1) / ACT_BLOCK;
    if (idx >= (long)a.nb * nbl * a.D1) return;
    const int uu = (int)(idx % a.D1);
    const long r = idx / a.D1;
    const int blk = (int)(r % nbl), b = (int)(r / nbl);
    const int s0 = blk * ACT_BLOCK, s1 = min(a.kn, s0 + ACT_BLOCK);
    const float* p = a.head + ((size_t)b * a.kn + s0) * a.ldh + uu;
    float acc = 0.0f;
    for (int s = s0; s < s1; ++s, p += a.ldh) acc += *p;
    a.part[((size_t)(a.img0 + b) * a.nblk + a.blk0 + blk) * a.D1 + uu] = acc;
}

// act_stats_kernel: one workgroup per unit.  Thread t takes images t, t + 256, ... in turn; the 256 thread sums are folded by a
// fixed pairwise tree.  Pass 1: the per-image means (block partials folded in order, in double, / kdiv) -> post_mean and their sum;
// pass 2: the centred second moment about the data mean.  Both orders depend on N only.
constexpr int ACT_STAT_THREADS = 256;
__global__ __launch_bounds__(ACT_STAT_THREADS) void act_stats_kernel(ActStatsArgs a) {
    __shared__ double sh[ACT_STAT_THREADS];
    const int uu = blockIdx.x;
    auto image_mean = [&](int i) {
        const float* p = a.src + (size_t)i * a.ld_img + uu;
        double s = 0.0;
        for (int j = 0; j < a.nblk; ++j) s += (double)p[(size_t)j * a.ld_blk];
        return s / a.kdiv;
    };
    double s1 = 0.0;
    for (int i = threadIdx.x; i < a.N; i += ACT_STAT_THREADS) {
        const double v = image_mean(i);
        a.post_mean[(size_t)i * a.ldpm + a.col + uu] = (float)v;
        s1 += v;
    }
    const double mean = tree_sum_256(s1, sh) / (double)a.N;
    double s2 = 0.0;
    for (int i = threadIdx.x; i < a.N; i += ACT_STAT_THREADS) {
        const double d = image_mean(i) - mean;
        s2 += d * d;
    }
    const double var = tree_sum_256(s2, sh) / (double)a.N;
    if (threadIdx.x == 0) { a.data_mean[a.col + uu] = mean; a.activity[a.col + uu] = var; }
}

}  // namespace

bool act_chain_ok(int KT0, int KTH, int KT1) { return KT0 == 4 && KTH == 4 && KT1 == 2; }
void launch_act_chain(const ActChainArgs& a, int nb, hipStream_t st) {
    const int nbl = (a.kn + ACT_BLOCK - 1) / ACT_BLOCK;
    hipLaunchKernelGGL((act_chain_kernel<4, 4, 2>), dim3(nbl, nb), dim3(512), 2 * (4 * 4096 + 1024) + 8 * 64 * 4, st, a);
}
void launch_act_partial(const ActPartialArgs& a, hipStream_t st) {
    const long n = (long)a.nb * ((a.kn + ACT_BLOCK - 1) / ACT_BLOCK) * a.D1;
    hipLaunchKernelGGL(act_partial_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
}
void launch_act_stats(const ActStatsArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(act_stats_kernel, dim3(a.D), dim3(ACT_STAT_THREADS), 0, st, a);
}

}  // namespace iwae
