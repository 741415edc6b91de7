// gfx950 kernels of the IWAE train / eval step that walk rows or elements once: input conversion, noise, sampling, log-densities,
// log-mean-exp, exports.  Kernel -> reference mapping: top of kernels.hip.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <algorithm>
#include "kernels.h"
#include "layout.h"
#include "device_helpers.h"
#include "step_helpers.h"

namespace iwae {

// ---------------------------------------------------------------------------------
// elementwise / reduction kernels
// ---------------------------------------------------------------------------------
// x fp32 [B][X] -> bf16 P-layout [B][Xp] (pads written as zero).
// block = 64 rows (lanes) x 4 chunk-waves; a thread converts one 8-feature P chunk of one row.
// cond != null: C more features per row taken from cond [B][C] (conditional model: concat(x, y), tasks/task05.py:113).
__global__ __launch_bounds__(256) void prep_rows_kernel(const float* x, const float* cond, int B, int X, int C, int Xp, int Bp, uint16_t* XP) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 64 + lane;
    const int nchunk = Xp / 8;
    if (b >= Bp) return;
    for (int c = blockIdx.y * 4 + (threadIdx.x >> 6); c < nchunk; c += gridDim.y * 4) {
        const int t = c >> 2, qq = c & 3;
        float v[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int f0 = 32 * t + 16 * h + 4 * qq;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int f = f0 + i;
                float t = 0.0f;
                if (b < B && f < X) t = x[(size_t)b * X + f];
                else if (b < B && f < X + C) t = cond[(size_t)b * C + (f - X)];
                v[4 * h + i] = t;
            }
        }
        if (b < B) *(uint4*)(XP + (size_t)b * Xp + 8 * c) = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
    }
}

// Fused batch gather + dynamic binarisation (main.py:117-120 + src/utils.py:26-27 done per batch on the
// device): row b of the batch is image idx[start+b] of the uint8 dataset resident in HBM; pixel f is
// 1 iff (philox(seed, epoch, image, f/4)[f%4] >> 8) < T(gray), T(g) = floor(g * 2^24 / 255 + 0.5), i.e.
// Bernoulli(gray/255) with an integer threshold (bit-exactly reproducible on the host).  Keyed by
// (epoch, image): one binarisation per image per epoch, as in the reference.  Same block shape and
// output as prep_rows_kernel (P-layout) + optional float32 copy.
// labels != null (conditional models, tasks/task05.py:296-322: the training set is (x, y) pairs): the image's class y rides along -- features
// X .. X + C - 1 of the row are onehot(y) (the encoder's input concat(x, onehot(y)), task05.py:113), and cond_out [B][C] gets the same
// one-hot row as float32 (what iwae_set_condition would have been handed for a host-fed batch).
__global__ __launch_bounds__(256) void gather_binarize_kernel(const uint8_t* data, const int32_t* order, int start, int N, int B, int X, int Xp,
                                                              int Bp, uint64_t seed, uint32_t epoch, uint16_t* XP, float* xf,
                                                              const uint8_t* labels, int C, float* cond_out) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 64 + lane;
    const int nchunk = Xp / 8;
    if (b >= Bp) return;
    const int img = (b < B) ? order[start + b] : 0;
    const int lab = (labels && b < B) ? (int)labels[img] : -1;
    if (cond_out && blockIdx.y == 0 && threadIdx.x < 64 && b < B)
        for (int j = 0; j < C; ++j) cond_out[(size_t)b * C + j] = (j == lab) ? 1.0f : 0.0f;
    for (int c = blockIdx.y * 4 + (threadIdx.x >> 6); c < nchunk; c += gridDim.y * 4) {
        const int t = c >> 2, qq = c & 3;
        float v[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int f0 = 32 * t + 16 * h + 4 * qq;
            uint32_t r[4];
            philox4x32_10((uint32_t)img, 0x42494E41u /* 'BINA' */, (uint32_t)(f0 >> 2), epoch, (uint32_t)seed, (uint32_t)(seed >> 32), r);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float bit = 0.0f;
                if (b < B && f0 + i < X) {
                    const uint32_t g = data[(size_t)img * X + f0 + i];
                    const uint32_t thr = (uint32_t)(((uint64_t)g * 16777216ull * 2ull + 255ull) / 510ull);   // floor(g*2^24/255 + 0.5)
                    bit = ((r[i] >> 8) < thr) ? 1.0f : 0.0f;
                    if (xf) xf[(size_t)b * X + f0 + i] = bit;
                } else if (lab >= 0 && f0 + i == X + lab) bit = 1.0f;
                v[4 * h + i] = bit;
            }
        }
        if (b < B) *(uint4*)(XP + (size_t)b * Xp + 8 * c) = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
    }
}

// The N(0,1) draws of one latent layer for a whole step, fp32 [rows][ld] (4 per thread).  They depend on nothing but
// the counters, so the host launches this a whole step ahead, on the side stream beside the forward pass: the ~40
// quarter-rate integer multiplies per Philox call are off every dependency chain.
// Grid-stride: drawn ahead (a whole step early, beside the forward pass) the launch is a few hundred small blocks that
// take their time in a corner of every CU; as 5 000 blocks it filled the machine for 11 us and the forward's large
// workgroups queued behind it.
// The draws of `nsteps` consecutive steps in one launch (few rows: a step's 2 000 draws are a 4.5 us launch on a chain of 9-17 us kernels; eight steps'
// worth cost the same): step e.step + s goes to out + s * step_stride, each value exactly what eps_gen_kernel would draw for that step.
__global__ __launch_bounds__(256) void eps_gen_multi_kernel(EpsSrc e, int M, int nd4, int ld, float* out, int nsteps, size_t step_stride) {
    const size_t per = (size_t)M * nd4, total = per * nsteps;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int s = (int)(idx / per);
        const size_t r = idx - (size_t)s * per;
        const int row = (int)(r / nd4), d4 = (int)(r - (size_t)row * nd4);
        float n[4];
        normal4(e.row_offset + (uint64_t)row, (uint32_t)d4, e.stream, e.step + (uint32_t)s, e.seed, n);
        *(float4*)(out + (size_t)s * step_stride + (size_t)row * ld + 4 * d4) = make_float4(n[0], n[1], n[2], n[3]);
    }
}
__global__ __launch_bounds__(256) void eps_gen_kernel(EpsSrc e, int M, int nd4, int ld, float* out) {
    const size_t total = (size_t)M * nd4;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int row = (int)(idx / nd4), d4 = (int)(idx - (size_t)row * nd4);
        float n[4];
        uint64_t grow = e.row_offset + (uint64_t)row;
        if (e.k_total) { const int b = row / e.kc; grow = e.row_offset + (uint64_t)b * (uint64_t)e.k_total + (uint64_t)(e.s_off + row - b * e.kc); }
        normal4(grow, (uint32_t)d4, e.stream, e.step, e.seed, n);
        *(float4*)(out + (size_t)row * ld + 4 * d4) = make_float4(n[0], n[1], n[2], n[3]);
    }
}

// z = mu + sigma*eps, prior/posterior log-densities, z written bf16 P-layout.
// wave = 16 data rows x 4 quads.  In every 32-feature step t lane (r, q) owns P-layout chunk 4t+q, i.e. features
// 32t+4q..+3 and 32t+16+4q..+3: float4 loads of eps / mu / sigma, one 16-byte store per step, and the row sums
// meet across the 4 quads with two shuffles -- no LDS, no barrier, 800 small blocks instead of 800 of 1024 threads.
__global__ __launch_bounds__(256) void sample_kernel(SampleArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int row = (blockIdx.x * 4 + wave) * 16 + r;
    const bool valid = row < a.M;
    const int rowc = valid ? row : a.M - 1;        // loads come from a clamped row, results are masked
    const int b = rowc / a.k, s = rowc - b * a.k;
    const float* hd = a.head + (size_t)(a.head_per_row ? rowc : b) * a.ldH;
    float lp = 0.0f, lq = 0.0f, lq2 = 0.0f;
    const int nt = a.Dp / 32;
    for (int t = 0; t < nt; ++t) {
        float z8[8];
        sample_step(a, t, q, rowc, b, s, hd, z8, lp, lq, lq2);
        if (valid && a.ZP)
            *(uint4*)(a.ZP + (size_t)row * a.Dp + 8 * (4 * t + q)) = make_uint4(pack2(z8[0], z8[1]), pack2(z8[2], z8[3]), pack2(z8[4], z8[5]), pack2(z8[6], z8[7]));
        if (valid && a.ZF) {       // float32 mode: z in natural feature order, unrounded
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int f0 = 32 * t + 16 * h + 4 * q;
                // (one 16-byte store per lane where the row pitch allows it: as four dword stores under four conditions the evaluator's sampling
                // kernel took 225 us for 416 k rows -- 64 scattered 4-byte pieces per instruction)
                if ((a.ldZF & 3) == 0 && f0 + 3 < a.ldZF) {
                    *(float4*)(a.ZF + (size_t)row * a.ldZF + f0) = make_float4(z8[4 * h], z8[4 * h + 1], z8[4 * h + 2], z8[4 * h + 3]);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (f0 + i < a.ldZF) a.ZF[(size_t)row * a.ldZF + f0 + i] = z8[4 * h + i];
                }
            }
        }
    }
    lp += __shfl_xor(lp, 16); lp += __shfl_xor(lp, 32);
    lq += __shfl_xor(lq, 16); lq += __shfl_xor(lq, 32);
    lq2 += __shfl_xor(lq2, 16); lq2 += __shfl_xor(lq2, 32);
    if (q == 0 && valid) {
        if (a.lp_prior) a.lp_prior[row] = lp;
        a.lq[row] = lq;
        if (a.lq_dreg) a.lq_dreg[row] = lq2;
    }
}

// thread per data row: sum_d log N(z1; mup[row], sigp[row]) with z1 recomputed from the encoder head
// and eps (iwae2.py:122); also the per-row gradients wrt the dec2 head when G != null is done in
// gauss_bwd_kernel.
__global__ __launch_bounds__(256) void gauss_lp_kernel(GaussLpArgs a) {
    // wave = 16 data rows x 4 quads: quad q takes feature groups d4 = q, q+4, ... (float4 loads), two shuffles add them up
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int row = (blockIdx.x * 4 + wave) * 16 + r;
    const bool valid = row < a.M;
    const int rowc = valid ? row : a.M - 1;
    const int b = rowc / a.k, s = rowc - b * a.k;
    const float* hz = a.zhead + (size_t)b * a.ldZH;           // generating head (per image)
    const float* hp = a.phead + (size_t)rowc * a.ldPH;        // evaluating head (per row)
    float lp = 0.0f;
    const int nd4 = (a.D + 3) / 4;
    for (int d4 = q; d4 < nd4; d4 += 4) {
        float e[4];
        eps4(a.eps, b, s, rowc, d4, a.D, e);
        const float4 zm = *(const float4*)(hz + 4 * d4), zs = *(const float4*)(hz + a.Dzp + 4 * d4);
        const float4 pm = *(const float4*)(hp + 4 * d4), ps = *(const float4*)(hp + a.Dpp + 4 * d4);
        const float zmv[4] = {zm.x, zm.y, zm.z, zm.w}, zsv[4] = {zs.x, zs.y, zs.z, zs.w};
        const float pmv[4] = {pm.x, pm.y, pm.z, pm.w}, psv[4] = {ps.x, ps.y, ps.z, ps.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (4 * d4 + i < a.D) {
                const float z = zmv[i] + zsv[i] * e[i];
                const float u = (z - pmv[i]) * __builtin_amdgcn_rcpf(psv[i]);
                lp += -0.5f * u * u - 0.5f * LOG2PI_F - __logf(psv[i]);
            }
        }
    }
    lp += __shfl_xor(lp, 16);
    lp += __shfl_xor(lp, 32);
    if (q == 0 && valid) a.out[row] = lp;
}

// one wave per image b
__global__ void lse_kernel(LseArgs a) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= a.B) return;
    lse_image(a, b, lane, LseGlobalSrc{});
}
// one workgroup of NW waves per image (many samples per image: the evaluator's k)
template <int NW>
__global__ __launch_bounds__(64 * NW) void lse_block_kernel(LseArgs a) {
    __shared__ float slots[NW];
    lse_image(a, (int)blockIdx.x, (int)threadIdx.x, LseGlobalSrc{}, BlockRed<NW>{slots});
}

// ---------------------------------------------------------------------------------
// exports in the reference's [k, B, ...] order (iwae1.py:141-151), debug dumps
// ---------------------------------------------------------------------------------
__global__ void export_rows_kernel(const float* in, int B, int k, float* out) {   // [B*k] row order -> [k][B]
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B * k) return;
    const int b = r / k, s = r - b * k;
    out[(size_t)s * B + b] = in[r];
}
__global__ void export_z_kernel(SampleArgs a, float* zout, const float* wn, float* snis) {
    // thread per (row, d4): z[k][B][D]; snis_z via atomics-free second kernel below
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int nd4 = (a.D + 3) / 4;
    const int row = idx / nd4, d4 = idx % nd4;
    if (row >= a.M) return;
    const int b = row / a.k, s = row - b * a.k;
    const float* hd = a.head + (size_t)(a.head_per_row ? row : b) * a.ldH;
    float e[4];
    eps4(a.eps, b, s, row, d4, a.D, e);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int f = 4 * d4 + i;
        if (f < a.D) zout[((size_t)s * a.B + b) * a.D + f] = hd[f] + hd[a.Dp + f] * e[i];
    }
}
__global__ void snis_kernel(const float* z, const float* wn, int B, int k, int D, float* out) {   // iwae1.py:139
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * D) return;
    const int b = idx / D, d = idx % D;
    float s = 0.0f;
    for (int i = 0; i < k; ++i) s += wn[b * k + i] * z[((size_t)i * B + b) * D + d];
    out[idx] = s;
}
__global__ void unpack_p_kernel(const uint16_t* P, int rows, int F, int Fp, float* out) {   // P-layout bf16 -> [rows][F] fp32
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * F) return;
    const int r = idx / F, f = idx % F;
    out[idx] = __uint_as_float((uint32_t)P[(size_t)r * Fp + p_pos(f)] << 16);
}
__global__ void eps_dump_kernel(EpsSrc e, int B, int k, int D, float* out) {   // [k][B][D]
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int nd4 = (D + 3) / 4;
    const int row = idx / nd4, d4 = idx % nd4;
    if (row >= B * k) return;
    const int b = row / k, s = row - b * k;
    float n[4];
    eps4(e, b, s, row, d4, D, n);
    for (int i = 0; i < 4; ++i)
        if (4 * d4 + i < D) out[((size_t)s * B + b) * D + 4 * d4 + i] = n[i];
}

// ---- launch wrappers (plain C++ callers in model.hip / step_f32.hip / analysis.hip)
void launch_prep_rows(const float* x, const float* cond, int B, int X, int C, int Xp, int Bp, uint16_t* XP, hipStream_t st) {
    const int nchunk = Xp / 8;
    hipLaunchKernelGGL(prep_rows_kernel, dim3(Bp / 64, std::min(32, (nchunk + 3) / 4)), dim3(256), 0, st, x, cond, B, X, cond ? C : 0, Xp, Bp, XP);
}
void launch_gather_binarize(const uint8_t* data, const int32_t* order, int start, int N, int B, int X, int Xp, int Bp, uint64_t seed,
                            uint32_t epoch, uint16_t* XP, float* xf, hipStream_t st, const uint8_t* labels, int C, float* cond_out) {
    const int nchunk = Xp / 8;
    hipLaunchKernelGGL(gather_binarize_kernel, dim3(Bp / 64, std::min(32, (nchunk + 3) / 4)), dim3(256), 0, st, data, order, start, N, B, X, Xp,
                       Bp, seed, epoch, XP, xf, labels, labels ? C : 0, cond_out);
}
void launch_eps_gen_multi(const EpsSrc& e, int M, int D, int ld, float* out, int nsteps, size_t step_stride, hipStream_t st) {
    const int nd4 = (D + 3) / 4;
    hipLaunchKernelGGL(eps_gen_multi_kernel, grid1((size_t)nsteps * M * nd4, 256), dim3(256), 0, st, e, M, nd4, ld, out, nsteps, step_stride);
}
void launch_eps_gen(const EpsSrc& e, int M, int D, int ld, float* out, hipStream_t st, int max_blocks) {
    const int nd4 = (D + 3) / 4;
    dim3 grid = grid1((size_t)M * nd4, 256);
    if (max_blocks > 0 && (int)grid.x > max_blocks) grid.x = max_blocks;
    hipLaunchKernelGGL(eps_gen_kernel, grid, dim3(256), 0, st, e, M, nd4, ld, out);
}
void launch_sample(const SampleArgs& a, hipStream_t st) { hipLaunchKernelGGL(sample_kernel, dim3((a.M + 63) / 64), dim3(256), 0, st, a); }
void launch_gauss_lp(const GaussLpArgs& a, hipStream_t st) { hipLaunchKernelGGL(gauss_lp_kernel, dim3((a.M + 63) / 64), dim3(256), 0, st, a); }
void launch_lse(const LseArgs& a, hipStream_t st, hipEvent_t done) {
    if (a.k >= 2048) LAUNCH_EV(done, lse_block_kernel<16>, dim3(a.B), dim3(1024), 0, st, a);
    else if (a.k > 256) LAUNCH_EV(done, lse_block_kernel<4>, dim3(a.B), dim3(256), 0, st, a);
    else LAUNCH_EV(done, lse_kernel, grid1((size_t)a.B * 64, 256), dim3(256), 0, st, a);
}
void launch_export_rows(const float* in, int B, int k, float* out, hipStream_t st) {
    hipLaunchKernelGGL(export_rows_kernel, grid1((size_t)B * k, 256), dim3(256), 0, st, in, B, k, out);
}
void launch_export_z(const SampleArgs& a, float* zout, hipStream_t st) {
    hipLaunchKernelGGL(export_z_kernel, grid1((size_t)a.M * ((a.D + 3) / 4), 256), dim3(256), 0, st, a, zout, (const float*)nullptr, (float*)nullptr);
}
void launch_snis(const float* z, const float* wn, int B, int k, int D, float* out, hipStream_t st) {
    hipLaunchKernelGGL(snis_kernel, grid1((size_t)B * D, 256), dim3(256), 0, st, z, wn, B, k, D, out);
}
void launch_unpack_p(const uint16_t* P, int rows, int F, int Fp, float* out, hipStream_t st) {
    hipLaunchKernelGGL(unpack_p_kernel, grid1((size_t)rows * F, 256), dim3(256), 0, st, P, rows, F, Fp, out);
}
void launch_eps_dump(const EpsSrc& e, int B, int k, int D, float* out, hipStream_t st) {
    hipLaunchKernelGGL(eps_dump_kernel, grid1((size_t)B * k * ((D + 3) / 4), 256), dim3(256), 0, st, e, B, k, D, out);
}

}  // namespace iwae
