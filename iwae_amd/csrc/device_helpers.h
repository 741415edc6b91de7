// Leaf device helpers shared by the kernel files (device code only: no kernels, launchers or host code); include it after kernels.h and
// layout.h.  A helper that two kernels must agree on bit for bit -- the bf16 pack, the two tanh forms, Philox + Box-Muller, the float32
// slab GEMM, the decoder row evaluation -- exists once, here, so the parity of those kernels does not rest on copies kept equal by eye.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "layout.h"

namespace iwae {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define LOG2PI_F 1.8378770664093453f
#define HALF_LOG_2PI_F 0.9189385332046727f

// ---------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pack2(float a, float b) {
    bf16x2_t v;
    v[0] = (__bf16)a;
    v[1] = (__bf16)b;   // hipcc emits v_cvt_pk_bf16_f32 (round-to-nearest-even, NaN-safe)
    return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ float bflo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bfhi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ float bf_at(const uint4& u, int j) {
    const uint32_t w = (j < 2) ? u.x : (j < 4) ? u.y : (j < 6) ? u.z : u.w;
    return (j & 1) ? bfhi(w) : bflo(w);
}
// the bits of that bf16 (the masked bf16 step compares them with the hole code, never the value)
__device__ __forceinline__ uint32_t bf_bits_at(const uint4& u, int j) {
    const uint32_t w = (j < 2) ? u.x : (j < 4) ? u.y : (j < 6) ? u.z : u.w;
    return (j & 1) ? (w >> 16) : (w & 0xffffu);
}
// The code of an unobserved pixel in the bf16 pixel rows of a masked call (masked_code_bf16_kernel writes it, bern8<.., HOLES> compares against it):
// all ones, a NaN no arithmetic produces -- the float32 step's MO_HOLE at bf16 width (DESIGN.md sections 19, 20)
constexpr uint32_t BF16_HOLE = 0xFFFFu;
// The code of an unobserved pixel in float32 pixel rows (masked_code_kernel writes xc = m ? x : the code; masked_out_f32_kernel and the HOLES
// instantiations of the row evaluation compare against it, as bits): all ones, a NaN no arithmetic produces.  An observed x with exactly these
// bits is stored one bit off, still a NaN: it stays observed and poisons its image as any observed NaN does.
constexpr uint32_t MO_HOLE = 0xFFFFFFFFu;
__device__ __forceinline__ f32x4 mfma16(const uint4& a, const uint4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ float rcp_fast(float x) { return __builtin_amdgcn_rcpf(x); }
#define LOG2E_F 1.4426950408889634f
#define LN2_F 0.6931471805599453f
// raw v_exp_f32 / v_log_f32 (base 2, ~1 ulp, no denormal fix-up code: arguments here never need it)
__device__ __forceinline__ float exp2_raw(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float log2_raw(float x) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float tanh_fast(float x) {
    // 1 - 2/(e^{2x}+1): exact limits at +-inf, abs error ~1e-7 (the result is rounded to bf16 anyway)
    return 1.0f - 2.0f * rcp_fast(exp2_raw(x * (2.0f * LOG2E_F)) + 1.0f);
}
__device__ __forceinline__ float sigmoid_fast(float l) { return rcp_fast(1.0f + exp2_raw(-l * LOG2E_F)); }
// tanh through one hardware exp2: 1 - 2/(1 + e^{2|x|}), sign restored.  Absolute error <= ~1.5e-7 (one ulp of 1.0; saturates cleanly: e^{2|x|} = inf
// gives exactly 1) -- the library tanhf is ~50 instructions per value, 20 million values per tanh layer of the full-size step.
__device__ __forceinline__ float tanh_f32(float x) {
    const float t = __expf(2.0f * fabsf(x));
    return __builtin_copysignf(1.0f - 2.0f * __builtin_amdgcn_rcpf(t + 1.0f), x);
}

// async global -> LDS copy (LDS-DMA), 16 B per lane; LDS destination = M0 (wave-uniform byte address)
// + lane*16.  Issued through inline asm on purpose: with the builtin, hipcc cannot prove that the
// DMA does not alias later ds_reads and drains it (s_waitcnt vmcnt(0)) before every k-step, which
// serialises the weight prefetch with the MFMAs.  Completion is ordered by the explicit
// "s_waitcnt vmcnt(0)" + barrier at the top of each group (cdna_hip_programming.md 5.7).
__device__ __forceinline__ uint32_t lds_addr_of(const char* p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}
__device__ __forceinline__ void glds16(const char* g, uint32_t lds_wave_base) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(g), "s"(lds_wave_base) : "memory");
}

// stream `bytes` (multiple of 1 KiB) of an A-image into LDS with the whole workgroup (wave must be
// wave-uniform, e.g. readfirstlane(threadIdx.x >> 6))
template <int NWAVES>
__device__ __forceinline__ void stage_image(const char* src, char* lds, int bytes, int wave, int lane) {
    const uint32_t base = lds_addr_of(lds);
    for (int off = wave * 1024; off < bytes; off += NWAVES * 1024)
        glds16(src + off + lane * 16, (uint32_t)__builtin_amdgcn_readfirstlane((int)(base + (uint32_t)off)));
}

// Group boundary wait.  The builtin tells hipcc's waitcnt pass that every vector-memory op it knows
// about has retired (otherwise it re-waits vmcnt(0) in front of the first MFMA of the group, which
// also drains the LDS-DMA just issued for the NEXT group); the asm form is the one that must stay:
// it also covers the asm-issued LDS-DMA, which the pass cannot see.
__device__ __forceinline__ void wait_all_vmem() {
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0), expcnt/lgkmcnt untouched
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// A-fragment stream with P ds_read_b128 in flight: rd(i) -> uint4, use(i, frag).  Without this the
// compiler emits read -> lgkmcnt(0) -> 2 MFMA per fragment and a lone wave pays the LDS latency
// (~64-128 cycles) for every 32 cycles of MFMA.
template <int N, int P, class RD, class USE, class SIDE>
__device__ __forceinline__ void lds_pipeline(RD rd, USE use, SIDE side) {
    uint4 av[P];
#pragma unroll
    for (int i = 0; i < P; ++i)
        if (i < N) av[i] = rd(i);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        use(i, av[i % P]);
        if (i + P < N) av[i % P] = rd(i + P);
        side(i);       // e.g. one LDS-DMA piece of the NEXT group: drains under the MFMAs instead of in front of them
    }
}
template <int N, int P, class RD, class USE>
__device__ __forceinline__ void lds_pipeline(RD rd, USE use) {
    lds_pipeline<N, P>(rd, use, [](int) {});
}

// ---------------------------------------------------------------------------------
// Philox4x32-10 + Box-Muller.  counter = (row_lo, row_hi, (stream<<24)|d4, step), key = seed
// ---------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        // both halves of a 32 x 32 product from ONE v_mad_u64_u32 (as __umulhi + a 32-bit multiply the compiler issued two quarter-rate multiplies each)
        unsigned long long p0, p1;
        asm("v_mad_u64_u32 %0, vcc, %1, %2, 0" : "=v"(p0) : "v"(c0), "v"(0xD2511F53u) : "vcc");
        asm("v_mad_u64_u32 %0, vcc, %1, %2, 0" : "=v"(p1) : "v"(c2), "v"(0xCD9E8D57u) : "vcc");
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// The plain 64-bit-multiply form (the same bits): ais_chain_kernel alone keeps it -- on the asm form that kernel, at the register limit, ran 1.0 % slower (17.49 -> 17.67 ms per launch).
__device__ __forceinline__ void philox4x32_10_mul(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
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
// four standard normals from the four words of one draw
__device__ __forceinline__ void box_muller4(const uint32_t (&r)[4], float n[4]) {
    const float s24 = 5.9604644775390625e-08f;   // 2^-24
    const float u0 = ((float)(r[0] >> 8) + 0.5f) * s24, u1 = ((float)(r[1] >> 8) + 0.5f) * s24;
    const float u2 = ((float)(r[2] >> 8) + 0.5f) * s24, u3 = ((float)(r[3] >> 8) + 0.5f) * s24;
    // v_log/v_sqrt/v_sin/v_cos (v_sin/v_cos take revolutions: sin(2*pi*u) = v_sin(u)); abs error ~1e-6
    const float ra = __builtin_amdgcn_sqrtf(-2.0f * __logf(u0)), rb = __builtin_amdgcn_sqrtf(-2.0f * __logf(u2));
    n[0] = ra * __builtin_amdgcn_cosf(u1); n[1] = ra * __builtin_amdgcn_sinf(u1);
    n[2] = rb * __builtin_amdgcn_cosf(u3); n[3] = rb * __builtin_amdgcn_sinf(u3);
}
__device__ __forceinline__ void normal4(uint64_t grow, uint32_t d4, uint32_t stream, uint32_t step, uint64_t seed, float n[4]) {
    uint32_t r[4];
    philox4x32_10((uint32_t)grow, (uint32_t)(grow >> 32), (stream << 24) | d4, step, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    box_muller4(r, n);
}
__device__ __forceinline__ void normal4_mul(uint64_t grow, uint32_t d4, uint32_t stream, uint32_t step, uint64_t seed, float n[4]) {
    uint32_t r[4];
    philox4x32_10_mul((uint32_t)grow, (uint32_t)(grow >> 32), (stream << 24) | d4, step, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    box_muller4(r, n);
}

// ---------------------------------------------------------------------------------
// fixed-order sums
// ---------------------------------------------------------------------------------
// over the 16 lanes n16 of a quad group: every lane gets the same bits
__device__ __forceinline__ float rowsum16(float v) {
    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
    return v;
}
__device__ __forceinline__ double rowsum16(double v) {
    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
    return v;
}
// the sum of one double per thread of a 256-thread workgroup by a fixed pairwise tree (sh: 256 doubles of LDS); every thread gets it
__device__ __forceinline__ double tree_sum_256(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int w = 256 / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// ---------------------------------------------------------------------------------
// The float32 decoder of the row kernels (ais_chain_kernel, local_q_kernel, impute_rows_kernel): 256 threads, a wave owns 16 rows, lane
// (n16 = lane & 15, q = lane >> 4).  A row's numbers are float32 fmaf chains in k order (v_mfma_f32_16x16x4_f32) and do not depend on
// the rows beside it.
// ---------------------------------------------------------------------------------
constexpr int WG_GEMM_THREADS = 256;

// acc[t] += strip[16 rows][16 nkb] * W[16 nkb rows][16 cnt columns], t < cnt: W row-major with ldw floats per row, already at its first row and
// column.  Whole workgroup: the slab of 16 weight rows goes global -> registers (one slab ahead) -> LDS between two barriers.
__device__ __forceinline__ void wg_gemm_f32(const float* strip, int pa, int nkb, const float* W, int ldw, int cnt, float* slab,
                                            f32x4 (&acc)[AIS_NT], int tid, int n16, int q) {
    const int gpr = 4 * cnt;                     // 16-byte granules per slab row
    int goff[4], soff[4];
    bool ok[4];
    float4 pre[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int g = tid + WG_GEMM_THREADS * u, r = g / gpr, cq = g - r * gpr;
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

// The forward half of the row evaluation: the wave's 16 rows of z are in its strip zs (columns [0, 16 dt), pads zero); g1 = tanh(z W1 + b1) goes
// to g1s and g2 = tanh(g1 W2 + b2) to g2s (pitch PH).  Reads a.W1, a.W2, a.b1, a.b2, a.Hp.  Whole workgroup; acc is scratch.
template <class Args>
__device__ __forceinline__ void dec_row_tanh_layers(const Args& a, const float* zs, float* g1s, float* g2s, float* slab, int PZ, int PH, int dt, int ht,
                                                    f32x4 (&acc)[AIS_NT], int tid, int n16, int q) {
#pragma unroll
    for (int t = 0; t < AIS_NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    wg_gemm_f32(zs, PZ, dt, a.W1, a.Hp, ht, slab, acc, tid, n16, q);
#pragma unroll
    for (int t = 0; t < AIS_NT; ++t) {
        if (t < ht) {
            const float b = a.b1[16 * t + n16];
#pragma unroll
            for (int r = 0; r < 4; ++r) g1s[(4 * q + r) * PH + 16 * t + n16] = tanh_f32(acc[t][r] + b);
            acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    }
    wg_gemm_f32(g1s, PH, ht, a.W2, a.Hp, ht, slab, acc, tid, n16, q);
#pragma unroll
    for (int t = 0; t < AIS_NT; ++t) {
        if (t < ht) {
            const float b = a.b2[16 * t + n16];
#pragma unroll
            for (int r = 0; r < 4; ++r) g2s[(4 * q + r) * PH + 16 * t + n16] = tanh_f32(acc[t][r] + b);
        }
    }
}

// The row evaluation: the wave's 16 rows of z are in its strip zs (columns [0, 16 dt), pads zero).  Adds each lane's share of log p(x|z) of
// its four rows 4q + r to lp (rowsum16 completes it) and leaves dz = grad_z log p(x|z) in acc[t][r], t < dt (row 4q + r, feature
// 16 t + n16).  Overwrites all three strips: g1s ends as dpre1, g2s as dpre2, zs as the last residual tile.  PH: pitch of g1s / g2s;
// xrow[r]: the image of row 4q + r.  Reads a.W1 .. a.W3T, a.b1 .. a.b3, a.Hp, a.Xp, a.X, a.Dp.  Whole workgroup.
// ais_chain_kernel's eval_kick lambda is the single deliberate restatement of this function: called from there it cost that kernel, which
// sits at the register limit, 12 bytes of scratch per lane (256 VGPR / 246 AGPR / 0 -> 256 / 256 / 12).
// HOLES (the masked calls): xrow[r] is a row of launch_masked_code's xc = m ? x : MO_HOLE.  A pixel whose bits are the
// hole code is SELECTED out like a pad column: it adds exactly nothing to lp and its residual is exactly 0, whatever x held there.
template <bool HOLES, class Args>
__device__ __forceinline__ void dec_row_eval(const Args& a, float* zs, float* g1s, float* g2s, float* slab, int PZ, int PH, int dt, int ht, int xt,
                                             int npass, const float* const (&xrow)[4], f32x4 (&acc)[AIS_NT], float (&lp)[4], int tid, int n16, int q) {
    f32x4 dg2[AIS_NT];
    // ---- g1 = tanh(z W1 + b1), g2 = tanh(g1 W2 + b2)
    dec_row_tanh_layers(a, zs, g1s, g2s, slab, PZ, PH, dt, ht, acc, tid, n16, q);
#pragma unroll
    for (int t = 0; t < AIS_NT; ++t) dg2[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // ---- output layer, 64 pixels at a time: logits -> log p(x|z) and s = x - sigmoid(l) -> dg2 += s W3^T (s never leaves the workgroup)
    for (int pass = 0; pass < npass; ++pass) {
        const int c0 = 16 * AIS_TPO * pass, cnt = min(AIS_TPO, xt - AIS_TPO * pass);
#pragma unroll
        for (int t = 0; t < AIS_TPO; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        wg_gemm_f32(g2s, PH, ht, a.W3 + c0, a.Xp, cnt, slab, acc, tid, n16, q);
        // sum_n x l - softplus(l) = sum_n (x - 1/2) l - |l| / 2 - log(1 + e^-|l|), the logarithms as one log2 of the product (dec_fwd_f32_kernel's form)
        float s_xl[4] = {0.f, 0.f, 0.f, 0.f}, s_al[4] = {0.f, 0.f, 0.f, 0.f}, prod[4] = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
        for (int t = 0; t < AIS_TPO; ++t) {
            if (t < cnt) {
                const int col = c0 + 16 * t + n16;
                const bool in = col < a.X;
                const float b = a.b3[col];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float x1 = in ? xrow[r][col] : 0.0f;
                    const bool ob = in && (!HOLES || __float_as_uint(x1) != MO_HOLE);      // counts: inside the image and observed
                    const float l = ob ? acc[t][r] + b : 0.0f, xm = ob ? x1 - 0.5f : 0.0f;
                    const float ex = __builtin_amdgcn_exp2f(-fabsf(l) * LOG2E_F);      // exp(-|l|)
                    s_xl[r] = fmaf(xm, l, s_xl[r]);
                    s_al[r] += fabsf(l);
                    prod[r] = ob ? fmaf(prod[r], ex, prod[r]) : prod[r];
                    zs[(4 * q + r) * PZ + 16 * t + n16] = ob ? xm - __builtin_copysignf(__builtin_amdgcn_rcpf(1.0f + ex) - 0.5f, l) : 0.0f;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) lp[r] += s_xl[r] - 0.5f * s_al[r] - LN2_F * __builtin_amdgcn_logf(prod[r]);
        wg_gemm_f32(zs, PZ, cnt, a.W3T + (size_t)c0 * a.Hp, a.Hp, ht, slab, dg2, tid, n16, q);
    }
    // ---- dpre2 = dg2 (1 - g2^2) over g2; dpre1 = (dpre2 W2^T)(1 - g1^2) over g1; dz = dpre1 W1^T
#pragma unroll
    for (int t = 0; t < AIS_NT; ++t) {
        if (t < ht) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float* at = g2s + (4 * q + r) * PH + 16 * t + n16;
                const float y = *at;
                *at = dg2[t][r] * (1.0f - y * y);
            }
        }
        acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    wg_gemm_f32(g2s, PH, ht, a.W2T, a.Hp, ht, slab, acc, tid, n16, q);
#pragma unroll
    for (int t = 0; t < AIS_NT; ++t) {
        if (t < ht) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float* at = g1s + (4 * q + r) * PH + 16 * t + n16;
                const float y = *at;
                *at = acc[t][r] * (1.0f - y * y);
            }
            acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    }
    wg_gemm_f32(g1s, PH, ht, a.W1T, a.Dp, dt, slab, acc, tid, n16, q);
}

}  // namespace iwae
