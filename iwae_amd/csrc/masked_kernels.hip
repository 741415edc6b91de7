// The masked float32 train step (iwae_forward_masked / iwae_forward_backward_masked / iwae_train_step_masked, include/iwae_amd.h; Mattei &
// Frellsen 2019, MIWAE): DESIGN.md section 19.  Host side: step_f32.hip.  Unobserved pixels are SELECTED out: what x holds there is never
// an operand of any arithmetic.
//   masked_bern_f32_kernel   general route: log p(x_obs|z) per row from the stored logits, the observed pixels only (one wave per row, fixed order)
//   masked_s_f32_kernel      general route: the logits in place -> s = m ? x - sigmoid(l) : 0
//   masked_code_kernel       fast route: xc = m ? x : HOLE, one float per pixel that carries value and mask (HOLE: a bit pattern, compared as bits)
//   masked_out_f32_kernel    fast route: the output layer g2 W3 + b3 with the masked likelihood [+ s] in its epilogue, rows stationary; the
//                            output-layer section of dec_fwd_f32_kernel (fp32_kernels.hip) with the mask as one more term of its `ok` predicate
//   masked_code_bf16_kernel  the masked bf16 step: the same code at bf16 width, in the bf16 step's P-layout pixel rows
//   gather_binarize_masked_kernel   the masked step fed from the resident set: gather, binarisation and every masked form of
//                            the batch's rows (xin as bf16 and float32, both hole codes, the mask bytes) in one launch, from the bit-packed
//                            per-image masks mask_pack_kernel / mask_mcar_kernel leave
// The two routes are the SAME float32 numbers: masked_out_f32_kernel forms each logit, each Bernoulli term, each row sum and each s with the
// general route's operations in the general route's order (see the kernel), so which route a call takes shows in no result.
// Every loop has a host-known trip count; workgroups never communicate; no atomics: results are bitwise repeatable.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include "kernels.h"
#include "device_helpers.h"

namespace iwae {
namespace {

// (the code of an unobserved pixel, MO_HOLE, is device_helpers.h's: the row evaluation of the masked analyses compares against it too)

// s = x - sigmoid(l) = (x - 1/2) - sign(l) (1 / (1 + e^-|l|) - 1/2) through one hardware exp2 and one reciprocal (dec_fwd_f32_kernel's form; absolute
// error ~1e-7).  Both routes call this one function: adds and single products only, nothing for the compiler to contract differently in two places.
// (Unlike log p(x_obs|z), s feeds no exponential: its last bits move a gradient by 1e-7, so it need not be dl_f32_kernel's expf and division.)
__device__ __forceinline__ float mo_s(float x, float l) {
    const float e = __builtin_amdgcn_exp2f(-fabsf(l) * LOG2E_F);
    return (x - 0.5f) - __builtin_copysignf(__builtin_amdgcn_rcpf(1.0f + e) - 0.5f, l);
}

__global__ __launch_bounds__(256) void masked_bern_f32_kernel(const float* logits, size_t ld, const float* x, const uint8_t* mask, int X, int M, int k, float* lpxz) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* l = logits + (size_t)row * ld;
    const float* xr = x + (size_t)(row / k) * X;
    const uint8_t* mr = mask + (size_t)(row / k) * X;
    float s = 0.0f;
    for (int j = lane; j < X; j += 64) {
        if (mr[j] != 0) {
            const float v = l[j];
            s += xr[j] * v - (fmaxf(v, 0.0f) + log1pf(expf(-fabsf(v))));      // iwae1.py:111, bern_f32_kernel's form
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) lpxz[row] = s;
}

__global__ __launch_bounds__(256) void masked_s_f32_kernel(float* logits, size_t ld, const float* x, const uint8_t* mask, int X, int M, int k) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)M * X) return;
    const int row = (int)(idx / X), j = (int)(idx - (size_t)row * X);
    float* p = logits + (size_t)row * ld + j;
    const size_t xi = (size_t)(row / k) * X + j;
    float s = 0.0f;
    if (mask[xi] != 0) s = mo_s(x[xi], *p);
    *p = s;
}

__global__ __launch_bounds__(256) void masked_code_kernel(const float* x, const uint8_t* mask, long n, float* xc) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    uint32_t b = MO_HOLE;
    if (mask[idx] != 0) {          // (x at an unobserved pixel is not even loaded)
        b = __float_as_uint(x[idx]);
        if (b == MO_HOLE) b = MO_HOLE - 1u;
    }
    xc[idx] = __uint_as_float(b);
}

// The masked bf16 step's pixel rows: prep_rows_kernel's block shape, chunks and P-layout, each pixel m ? bf16(x) :
// BF16_HOLE.  The mask byte is tested first: x at an unobserved pixel is not loaded.  An observed x whose bf16 is exactly the hole's bits is
// stored one bit off (still a NaN, still observed).  Pad pixels are 0 and pad rows are written too (0): the reader selects on bits alone.
__global__ __launch_bounds__(256) void masked_code_bf16_kernel(const float* x, const uint8_t* mask, int B, int X, int Xp, int Bp, uint16_t* XC) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 64 + lane;
    const int nchunk = Xp / 8;
    if (b >= Bp) return;
    for (int c = blockIdx.y * 4 + (threadIdx.x >> 6); c < nchunk; c += gridDim.y * 4) {
        const int t = c >> 2, qq = c & 3;
        uint32_t v[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int f0 = 32 * t + 16 * h + 4 * qq;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int f = f0 + i;
                uint32_t bits = 0u;
                if (b < B && f < X) {
                    bits = BF16_HOLE;
                    if (mask[(size_t)b * X + f] != 0) {
                        bits = pack2(x[(size_t)b * X + f], 0.0f) & 0xffffu;
                        if (bits == BF16_HOLE) bits = BF16_HOLE - 1u;
                    }
                }
                v[4 * h + i] = bits;
            }
        }
        *(uint4*)(XC + (size_t)b * Xp + 8 * c) = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
    }
}

// ---- the resident per-image masks (iwae_dataset_set_mask / iwae_dataset_mcar_mask): one thread per (image, word)
__global__ __launch_bounds__(256) void mask_pack_kernel(const uint8_t* mask, int n, int X, int W, uint32_t* bits) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n * W) return;
    const int i = (int)(idx / W), w = (int)(idx - (size_t)i * W);
    uint32_t v = 0u;
    for (int j = 0; j < 32; ++j) {
        const int f = 32 * w + j;
        if (f < X && mask[(size_t)i * X + f] != 0) v |= 1u << j;
    }
    bits[idx] = v;
}
// missing completely at random, keyed like the binarisation (counter (image, 'MASK', pixel / 4, 0), the caller's key): integer work,
// iwae_amd/utils.py::device_mcar_mask restates it bit for bit.  Bits past the last pixel stay 0.
__global__ __launch_bounds__(256) void mask_mcar_kernel(int n, int X, int W, uint32_t thr, uint64_t key, uint32_t* bits) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n * W) return;
    const int i = (int)(idx / W), w = (int)(idx - (size_t)i * W);
    uint32_t v = 0u;
    for (int j = 0; j < 8; ++j) {
        uint32_t r[4];
        philox4x32_10((uint32_t)i, 0x4D41534Bu /* 'MASK' */, (uint32_t)(8 * w + j), 0u, (uint32_t)key, (uint32_t)(key >> 32), r);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int f = 32 * w + 4 * j + e;
            if (f < X && !((r[e] >> 8) < thr)) v |= 1u << (4 * j + e);
        }
    }
    bits[idx] = v;
}

// The masked step's input from the resident set: gather_binarize_kernel's block shape, chunk walk, P-layout and Philox
// call -- counter, key and threshold are its own, so a pixel's binarised bit is the bit iwae_dataset_get_batch returns -- under the image's
// mask.  A chunk's 8 pixels lie in the 32-pixel group t = c >> 2: one word of the image's mask serves them.  Written, where the pointer is
// not null: XP = bf16(m ? bit : 0) (prep_rows_kernel on impute_mask_kernel's rows), XC = m ? bf16(bit) : BF16_HOLE with pad pixels and pad rows
// 0 (masked_code_bf16_kernel), and as [B][X] rows xin = m ? bit : 0 (impute_mask_kernel), the mask bytes and xcode = m ? bit : MO_HOLE
// (masked_code_kernel).  The grey level of an unobserved pixel is loaded (the set is the library's own memory); the bit it binarises to reaches
// an output only as the unchosen side of a select.  vec4 (X a multiple of 4: a group of 4 pixels is whole or absent): the [B][X] rows in 16-byte / 4-byte stores.
__global__ __launch_bounds__(256) void gather_binarize_masked_kernel(GatherMaskedArgs a, int W, int vec4) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 64 + lane;
    const int nchunk = a.Xp / 8;
    if (b >= a.Bp) return;
    const bool row = b < a.B;
    const int img = row ? a.order[a.start + b] : 0;
    for (int c = blockIdx.y * 4 + (threadIdx.x >> 6); c < nchunk; c += gridDim.y * 4) {
        const int t = c >> 2, qq = c & 3;
        const uint32_t word = (row && t < W) ? a.bits[(size_t)img * W + t] : 0u;
        float v[8];
        uint32_t hc[8];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int f0 = 32 * t + 16 * h + 4 * qq;
            uint32_t r[4];
            philox4x32_10((uint32_t)img, 0x42494E41u /* 'BINA' */, (uint32_t)(f0 >> 2), a.epoch, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), r);
            float xi[4], xc[4];
            uint32_t mb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int f = f0 + i;
                xi[i] = 0.0f; xc[i] = 0.0f; mb[i] = 0u;
                uint32_t code = 0u;
                if (row && f < a.X) {
                    const bool obs = ((word >> (f & 31)) & 1u) != 0u;
                    const uint32_t g = a.data[(size_t)img * a.X + f];
                    const uint32_t thr = (uint32_t)(((uint64_t)g * 16777216ull * 2ull + 255ull) / 510ull);   // floor(g*2^24/255 + 0.5)
                    const float bit = ((r[i] >> 8) < thr) ? 1.0f : 0.0f;
                    xi[i] = obs ? bit : 0.0f;
                    xc[i] = obs ? bit : __uint_as_float(MO_HOLE);
                    mb[i] = obs ? 1u : 0u;
                    code = obs ? (pack2(bit, 0.0f) & 0xffffu) : BF16_HOLE;
                }
                v[4 * h + i] = xi[i];
                hc[4 * h + i] = code;
            }
            if (row && f0 < a.X) {
                const size_t o = (size_t)b * a.X + f0;
                if (vec4) {
                    if (a.xin) *(float4*)(a.xin + o) = make_float4(xi[0], xi[1], xi[2], xi[3]);
                    if (a.mask) *(uint32_t*)(a.mask + o) = mb[0] | (mb[1] << 8) | (mb[2] << 16) | (mb[3] << 24);
                    if (a.xcode) *(float4*)(a.xcode + o) = make_float4(xc[0], xc[1], xc[2], xc[3]);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (f0 + i < a.X) {
                            if (a.xin) a.xin[o + i] = xi[i];
                            if (a.mask) a.mask[o + i] = (uint8_t)mb[i];
                            if (a.xcode) a.xcode[o + i] = xc[i];
                        }
                    }
                }
            }
        }
        if (a.XP && row) *(uint4*)(a.XP + (size_t)b * a.Xp + 8 * c) = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
        if (a.XC) *(uint4*)(a.XC + (size_t)b * a.Xp + 8 * c) = make_uint4(hc[0] | (hc[1] << 16), hc[2] | (hc[3] << 16), hc[4] | (hc[5] << 16), hc[6] | (hc[7] << 16));
    }
}

// ---------------------------------------------------------------------------------
// masked_out_f32_kernel: logits = g2 W3 + b3 -> log p(x_obs|z) per row [+ s], the logits never leave the registers.
//   * a wave owns 16 data rows; a workgroup = 4 waves = 64 rows; the wave's g2 rows sit in its private LDS strip (a lane's four k values of a
//     16-block are one ds_read_b128), W3 is streamed 16 in-features at a time through two shared slabs by LDS-DMA
//     from the float32 master parameters; <= 13 pixel tiles (208 pixels) of accumulators per pass: 80.9 KB of LDS, two workgroups per CU;
//   * v_mfma_f32_16x16x4_f32: lane quad q contracts k = 4 q + j of the 16-block in step j (a slab's rows are stored permuted for that: row 4 j + q
//     holds in-feature 4 q + j, so quads q, q + 1 read rows one pitch apart, 16 banks, as in dec_fwd_f32_kernel); accumulator tile t: lane (n16, q) reg r = row 4q + r, pixel c0 + 16 t + n16;
//   * the epilogue's operands (b3 and xc of the wave's images at the pass's pixels) are one 16-byte request per lane and segment, parked in the
//     slab the last k-step left free; more than three images in a wave (k < 8): xc straight from memory;
//   * a pixel counts iff it is inside the layer AND observed (`live`): only then do x and the logit enter a sum, and s is stored as 0
//     elsewhere (the weight gradient and the dX product read every column of s);
//   * bit for bit the general route.  (First the epilogue was dec_fwd_f32_kernel's: (x - 1/2) l - |l| / 2 and one log2 of a product of
//     (1 + e) per 13 pixels.  That is as accurate, but it rounds log p(x_obs|z) one or two float32 spacings away from the general route's
//     value, 3e-5 at |log_w| ~ 300; softmax over k turns that into a relative error of the importance weights, and at a handful of rows the
//     two routes' gradients differed by up to 3.4e-5.)  Three things make the numbers equal:
//       - the logit: gemm_f32_v2_kernel's chain -- per 16-block of in-features four MFMA steps, step j over k = j, 4 + j, 8 + j, 12 + j -- plus the
//         bias; where the general route's output-layer GEMM splits K
//         (launch_gemm_f32_fewrows, few rows: partial chains of kchunk in-features, added in chunk order, then the bias) the KSPLIT
//         instantiation keeps a second set of accumulators and does the same (a.kslabs = kchunk / 16 slabs per chunk);
//       - the term: masked_bern_f32_kernel's expression (bern_f32_kernel's: library expf / log1pf); s: mo_s, shared with masked_s_f32_kernel;
//       - the row sum: masked_bern_f32_kernel's lane L adds pixels L, L + 64, ... in turn, then the lanes are added as a tree (xor 32, 16, 8
//         .. 1).  Pixel 16 T + n16 of tile T belongs to lane 16 (T & 3) + n16: this kernel's lane (n16, q) keeps four running sums per row,
//         one per T & 3, over the passes, adds (p0 + p2) + (p1 + p3) and finishes with the same xor 8 .. 1 over n16.
// ---------------------------------------------------------------------------------
#define MO_TP 13                    // pixel tiles (16 each) a wave accumulates per pass
#define MO_PA 212                   // strip pitch in floats (= 4 * 53: rows fall into different bank quads for ds_read_b128)
#define MO_SLAB (16 * 16 * MO_TP)   // floats per weight slab: 16 in-features x 208 pixels
template <bool KSPLIT>
__global__ __launch_bounds__(256, 2) void masked_out_f32_kernel(MaskedOutF32Args a) {
    extern __shared__ __attribute__((aligned(1024))) char smem_mo[];
    float* strip_all = (float*)smem_mo;                                  // [4 waves][16 rows][MO_PA]
    float* slab_all = (float*)(smem_mo + 4 * 16 * MO_PA * 4);            // [2][16][208]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n16 = lane & 15, q = lane >> 4;
    const int m0 = blockIdx.x * 64 + wave * 16;                          // the wave's first data row
    float* strip = strip_all + wave * 16 * MO_PA;
    const uint32_t slab_lds = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)slab_all;
    const char* zsrc = a.zero + lane * 16;
    const int K = a.H, N = a.X;

    // ---- the wave's 16 rows of g2 into its strip (pad columns and rows >= M zero): float4 requests, all in flight before the first store
    {
        const int Kp = (K + 15) & ~15, Q = Kp >> 2;                      // quads per row (<= 52)
        const bool vec = (K & 3) == 0 && (a.ldg & 3) == 0 && (((uintptr_t)a.G2) & 15) == 0;
        float4 gq[13];                                                     // 16 rows x <= 52 quads = <= 832 quads = 13 per lane
        int gpos[13];
#pragma unroll
        for (int it = 0; it < 13; ++it) {
            const int idx = lane + 64 * it;
            gq[it] = make_float4(0.f, 0.f, 0.f, 0.f);
            gpos[it] = -1;
            if (idx < 16 * Q) {
                const int r = idx / Q, c = 4 * (idx - r * Q);
                gpos[it] = r * MO_PA + c;
                if (m0 + r < a.M && c < K) {
                    const float* src = a.G2 + (size_t)(m0 + r) * a.ldg + c;
                    if (vec) gq[it] = *(const float4*)src;
                    else { gq[it].x = src[0]; if (c + 1 < K) gq[it].y = src[1]; if (c + 2 < K) gq[it].z = src[2]; if (c + 3 < K) gq[it].w = src[3]; }
                }
            }
        }
#pragma unroll
        for (int it = 0; it < 13; ++it) {
            if (gpos[it] >= 0) {
                *(float4*)(strip + gpos[it]) = gq[it];
            }
        }
    }
    // the images of the lane's four rows (4q + r): base of their xc rows, once
    const float* xrow[4];
    const int img0 = min(m0, a.M - 1) / a.k, nimg = min(m0 + 15, a.M - 1) / a.k - img0 + 1;      // (wave-uniform)
    const bool x_in_lds = nimg <= 3;
    int xslot[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int im = min(m0 + 4 * q + r, a.M - 1) / a.k;
        xrow[r] = a.XC + (size_t)im * a.X;
        xslot[r] = x_in_lds ? im - img0 : 0;
    }
    float part[4][4];      // [row 4q + r][T & 3]: masked_bern_f32_kernel's lane sums of lanes 16 (T & 3) + n16
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) part[r][i] = 0.0f;
    auto rotate = [&](int n) {      // part[r][i] <- part[r][(i + n) & 3], n wave-uniform: the epilogue indexes the slots with constants
        for (int it = 0; it < n; ++it) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float f = part[r][0]; part[r][0] = part[r][1]; part[r][1] = part[r][2]; part[r][2] = part[r][3]; part[r][3] = f; }
        }
    };

    const int NT = (N + 15) >> 4, npass = (NT + MO_TP - 1) / MO_TP, TP = (NT + npass - 1) / npass, nkb = (K + 15) >> 4;
    for (int pass = 0; pass < npass; ++pass) {
        const int t0 = pass * TP, cnt = min(TP, NT - t0), c0 = 16 * t0;
        // DMA of a slab: granule g = tid + 256 u (16 bytes) of the [16][208] slab <- W3[16 kb + g / 52][c0 + 4 (g % 52)]: a running pointer and a
        // stride per piece (the zero line / 0 for granules outside the layer)
        const char* gcur[4]; unsigned gstep[4]; int grow[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int g = tid + 256 * u, rd = g / (4 * MO_TP), cq = g - rd * (4 * MO_TP);
            const int r = 4 * (rd & 3) + (rd >> 2);       // slab row 4 j + q holds in-feature 4 q + j of the block: the k order of gemm_f32_v2_kernel's MFMA steps (see the header)
            const bool ok = rd < 16 && cq < 4 * cnt && c0 + 4 * cq < N;      // (N is a multiple of 4: a granule is all in or all out)
            grow[u] = ok ? r : (1 << 20);
            gcur[u] = ok ? (const char*)(a.W3 + (size_t)r * N + c0 + 4 * cq) : zsrc;
            gstep[u] = ok ? (unsigned)(16 * N * 4) : 0u;
        }
        auto issue = [&](int kb, int buf) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (256 * u + 64 * wave < 16 * 4 * MO_TP) {          // (wave-uniform: pieces past the slab's 832 granules are never issued)
                    const char* src = (16 * kb + grow[u] >= K) ? zsrc : gcur[u];      // (rows past K of the last slab, and granules outside: the zero line)
                    glds16(src, (uint32_t)__builtin_amdgcn_readfirstlane((int)(slab_lds + (uint32_t)buf * (MO_SLAB * 4) + (uint32_t)(256 * u + 64 * wave) * 16u)));
                    gcur[u] += gstep[u];
                }
            }
        };
        f32x4 acc[MO_TP];
        f32x4 tot[KSPLIT ? MO_TP : 1];      // KSPLIT: the sum of the K chunks finished so far
#pragma unroll
        for (int t = 0; t < MO_TP; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        __syncthreads();              // every wave is done with both slabs of the pass before (and the strip is written)
        issue(0, 0);
        const int segcol = c0 + 4 * lane;
        const bool segok = lane < 4 * MO_TP && lane < 4 * cnt && segcol < N;
        float4 pb = make_float4(0.f, 0.f, 0.f, 0.f), px[3] = {pb, pb, pb};
        for (int kb = 0; kb < nkb; ++kb) {
            const int buf = kb & 1;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();          // slab kb has landed for everyone; everyone has left slab kb - 1
            if (kb + 1 < nkb) issue(kb + 1, buf ^ 1);
            if (kb == nkb - 1 && segok) {
                pb = *(const float4*)(a.b3 + segcol);
                if (x_in_lds) {
#pragma unroll
                    for (int si = 0; si < 3; ++si)
                        if (si < nimg) px[si] = *(const float4*)(a.XC + (size_t)(img0 + si) * a.X + segcol);
                }
            }
            const float4 av = *(const float4*)(strip + n16 * MO_PA + 16 * kb + 4 * q);      // row n16 of the wave: k = 16 kb + 4 q + j at .j
            const float a4[4] = {av.x, av.y, av.z, av.w};
            const float* sl = slab_all + buf * MO_SLAB + q * (16 * MO_TP) + n16;
            // 52 MFMAs (step j = i / 13, tile t = i % 13), their B operands through an explicit 8-deep read pipeline
            constexpr int NM = 4 * MO_TP, PD = 8;
            float bq[PD];
#pragma unroll
            for (int i = 0; i < PD; ++i) bq[i] = sl[(4 * (i / MO_TP)) * (16 * MO_TP) + 16 * (i % MO_TP)];
#pragma unroll
            for (int i = 0; i < NM; ++i) {
                acc[i % MO_TP] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[i / MO_TP], bq[i % PD], acc[i % MO_TP], 0, 0, 0);      // (all 13 tiles, branch-free: the slab columns of tiles >= cnt are zeros)
                if (i + PD < NM) bq[i % PD] = sl[(4 * ((i + PD) / MO_TP)) * (16 * MO_TP) + 16 * ((i + PD) % MO_TP)];
            }
            __builtin_amdgcn_sched_group_barrier(0x100, PD + 1, 0);      // (+ the A operand's ds_read_b128)
#pragma unroll
            for (int i = 0; i < NM; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                if (i + PD < NM) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            if constexpr (KSPLIT) {      // the end of a K chunk: its partial chain joins the chunks before it, in chunk order
                if ((kb + 1) % a.kslabs == 0 || kb == nkb - 1) {
                    const bool first = kb < a.kslabs;
#pragma unroll
                    for (int t = 0; t < MO_TP; ++t) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) tot[t][r] = first ? acc[t][r] : tot[t][r] + acc[t][r];
                        acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    }
                }
            }
        }
        if constexpr (KSPLIT) {
#pragma unroll
            for (int t = 0; t < MO_TP; ++t) acc[t] = tot[t];
        }
        // park the epilogue operands in the slab the last k-step did not use (wave-private quarter: the wave's own LDS order is all the ordering needed)
        float* scr = slab_all + (nkb & 1) * MO_SLAB + wave * (16 * 4 * MO_TP);
        if (lane < 4 * MO_TP) {
            *(float4*)(scr + 4 * lane) = pb;
#pragma unroll
            for (int si = 0; si < 3; ++si) *(float4*)(scr + 16 * MO_TP * (1 + si) + 4 * lane) = px[si];
        }
        // log p(x_obs|z) += sum over the pass's live pixels of x l - softplus(l) (iwae1.py:111): masked_bern_f32_kernel's term, into the running sum of
        // the pixel's tile index mod 4 (slot i holds T & 3 = (i + t0) & 3 during the pass)
        rotate(t0 & 3);
#pragma unroll
        for (int t = 0; t < MO_TP; ++t) {
            const int col = c0 + 16 * t + n16;
            const bool ok = t < cnt && col < N;
            const float bvt = scr[16 * t + n16];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float x1 = x_in_lds ? scr[16 * MO_TP * (1 + xslot[r]) + 16 * t + n16] : (ok ? xrow[r][col] : 0.0f);
                const bool live = ok && __float_as_uint(x1) != MO_HOLE;
                const float v = acc[t][r] + bvt;
                if (live) part[r][t & 3] += x1 * v - (fmaxf(v, 0.0f) + log1pf(expf(-fabsf(v))));
                if (a.S && ok && m0 + 4 * q + r < a.M) {      // training step: s = m ? x - sigmoid(l) : 0 (masked_s_f32_kernel's expression)
                    float sv = 0.0f;
                    if (live) sv = mo_s(x1, v);
                    a.S[(size_t)(m0 + 4 * q + r) * a.ldS + col] = sv;
                }
            }
        }
        rotate((4 - (t0 & 3)) & 3);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float v = (part[r][0] + part[r][2]) + (part[r][1] + part[r][3]);      // (masked_bern_f32_kernel's xor 32, then xor 16)
        v += __shfl_xor(v, 8); v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);      // (... its xor 8 .. 1 over n16)
        if (n16 == 0 && m0 + 4 * q + r < a.M) a.lpxz[m0 + 4 * q + r] = v;
    }
}

}  // namespace

void launch_masked_bern_f32(const float* logits, size_t ld, const float* x, const uint8_t* mask, int X, int M, int k, float* lpxz, hipStream_t st) {
    hipLaunchKernelGGL(masked_bern_f32_kernel, dim3((M + 3) / 4), dim3(256), 0, st, logits, ld, x, mask, X, M, k, lpxz);
}
void launch_masked_s_f32(float* logits, size_t ld, const float* x, const uint8_t* mask, int X, int M, int k, hipStream_t st) {
    hipLaunchKernelGGL(masked_s_f32_kernel, dim3((unsigned)(((size_t)M * X + 255) / 256)), dim3(256), 0, st, logits, ld, x, mask, X, M, k);
}
void launch_masked_code(const float* x, const uint8_t* mask, long n, float* xc, hipStream_t st) {
    hipLaunchKernelGGL(masked_code_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, mask, n, xc);
}
void launch_masked_code_bf16(const float* x, const uint8_t* mask, int B, int X, int Xp, int Bp, uint16_t* XC, hipStream_t st) {
    const int nchunk = Xp / 8;
    hipLaunchKernelGGL(masked_code_bf16_kernel, dim3(Bp / 64, std::min(32, (nchunk + 3) / 4)), dim3(256), 0, st, x, mask, B, X, Xp, Bp, XC);
}
void launch_mask_pack(const uint8_t* mask, int n, int X, uint32_t* bits, hipStream_t st) {
    const int W = mask_words(X);
    hipLaunchKernelGGL(mask_pack_kernel, dim3((unsigned)(((size_t)n * W + 255) / 256)), dim3(256), 0, st, mask, n, X, W, bits);
}
void launch_mask_mcar(int n, int X, uint32_t thr, uint64_t key, uint32_t* bits, hipStream_t st) {
    const int W = mask_words(X);
    hipLaunchKernelGGL(mask_mcar_kernel, dim3((unsigned)(((size_t)n * W + 255) / 256)), dim3(256), 0, st, n, X, W, thr, key, bits);
}
void launch_gather_binarize_masked(const GatherMaskedArgs& a, hipStream_t st) {
    const int nchunk = a.Xp / 8;
    hipLaunchKernelGGL(gather_binarize_masked_kernel, dim3(a.Bp / 64, std::min(32, (nchunk + 3) / 4)), dim3(256), 0, st, a, mask_words(a.X), (a.X & 3) == 0 ? 1 : 0);
}
// widths and alignment masked_out_f32_kernel takes: the hidden width within one strip, pixel rows in whole 16-byte granules (W3's rows, b3 and
// xc are read as float4 / by LDS-DMA)
bool masked_out_f32_ok(const MaskedOutF32Args& a) {
    return a.H >= 1 && a.H <= 16 * MO_TP && a.X >= 4 && a.X % 4 == 0 && a.k >= 1 &&
           ((uintptr_t)a.W3 & 15) == 0 && ((uintptr_t)a.b3 & 15) == 0;
}
void launch_masked_out_f32(const MaskedOutF32Args& a, hipStream_t st) {
    const size_t lds = (size_t)4 * 16 * MO_PA * 4 + (size_t)2 * MO_SLAB * 4;
    if (a.kslabs > 0) hipLaunchKernelGGL(masked_out_f32_kernel<true>, dim3((a.M + 63) / 64), dim3(256), lds, st, a);
    else hipLaunchKernelGGL(masked_out_f32_kernel<false>, dim3((a.M + 63) / 64), dim3(256), lds, st, a);
}

}  // namespace iwae
