// gfx950 (CDNA4, MI355X) kernels of the bf16 train step's update: gradient slabs -> flat gradient -> Adam and the weight images, the batch means
// of the step's scalars, and wgrad_rows_kernel, whose epilogue is that update; the launchers are at the end of the file.
// Layout rules: layout.h.  Kernel -> reference mapping (file:line in the reference, as at the top of kernels.hip):
//   reduce_grads_kernel / wgrad_rows_kernel
//                                    tape.gradient(loss, w)   src/iwae1.py:155-159
//   adam_kernel                      Adam(eps=1e-4)           main.py:93, src/iwae1.py:160
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "kernels.h"
#include "layout.h"
#include "device_helpers.h"
#include "step_helpers.h"

namespace iwae {
// Batch means of the per-image values (the scalar entries of the reference's result dict), one 256-thread block.
// A cross-XCD "last wave reduces" inside lse_kernel would need agent-scope release/acquire fences, i.e. an L2
// write-back per wave (measured: 7 -> 71 us); a kernel boundary does that once, so the means are taken either by
// this tiny kernel (forward-only calls) or by an extra block of the step's last kernel (reduce_grads_kernel).
__device__ __forceinline__ void batch_means_block(const float* per_b, int B, float beta, float* out) {
    __shared__ float red[PB_COUNT][4];
    float acc[PB_COUNT];
#pragma unroll
    for (int t = 0; t < PB_COUNT; ++t) acc[t] = 0.0f;
    for (int b = threadIdx.x; b < B; b += 256)
#pragma unroll
        for (int t = 0; t < PB_COUNT; ++t) acc[t] += per_b[t * B + b];
#pragma unroll
    for (int t = 0; t < PB_COUNT; ++t) {
        float v = acc[t];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((threadIdx.x & 63) == 0) red[t][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s[PB_COUNT];
        for (int t = 0; t < PB_COUNT; ++t) s[t] = (red[t][0] + red[t][1] + red[t][2] + red[t][3]) / (float)B;
        out[SC_IWAE_ELBO] = s[PB_LME];
        out[SC_VAE_ELBO] = s[PB_MEAN];
        out[SC_IWAE_EQ14] = s[PB_EQ14];
        out[SC_VAE_ELBO_KL] = s[PB_PX] - beta * s[PB_KL];      // iwae1.py:121
        out[SC_MEAN_LPXZ] = s[PB_PX];
        out[SC_MEAN_T1] = s[PB_T1];
        out[SC_MEAN_T2] = s[PB_T2];
        out[SC_INFERENCE_LOSS] = -s[PB_DREG];                  // tasks/task02.py:76
        out[SC_KL] = s[PB_KL];
    }
}
__global__ __launch_bounds__(256) void scalars_kernel(const float* per_b, int B, float beta, float* out) { batch_means_block(per_b, B, beta, out); }

// single block: means over the batch -> scalars[16]

// ---------------------------------------------------------------------------------
// gradient slab reduce and Adam (+ bf16 A-image refresh)
// ---------------------------------------------------------------------------------
struct AdamCoef { float alpha, gscale, beta1, beta2, eps; int on; };

// Keras Adam (epsilon outside the square root, main.py:93) on one element + refresh of the bf16 weight images /
// the fp32 bias block the GEMM kernels read.  is_bias: element j of the bias, else weight (in-feature i, out-feature j).
// The update's arithmetic with its roundings spelled out (explicit fused multiply-adds): the same function is inlined into
// reduce_grads_kernel, adam_kernel and wgrad_rows_kernel, and the single-GPU step must land on bit-identical parameters whichever of them
// applies it (left to -ffp-contract, the compiler fused a different product of b1*m + (1-b1)*g in one of the three contexts).
__device__ __forceinline__ void adam_math(float& w, float& m, float& v, float g, const AdamCoef& c) {
    g *= c.gscale;
    m = __builtin_fmaf(c.beta1, m, (1.0f - c.beta1) * g);
    v = __builtin_fmaf(c.beta2, v, ((1.0f - c.beta2) * g) * g);
    const float q = (c.alpha * m) / (sqrtf(v) + c.eps);
    w = w - q;
}
// refresh of the bf16 weight images / the fp32 bias block the GEMM kernels read, from the (new) master value w
__device__ __forceinline__ void image_refresh(const LayerDesc& L, bool is_bias, int i, int j, float w) {
    if (is_bias) {
        *(float*)(L.imgF + img_mg_bias_byte(L.joff + j, L.KT_F)) = w;
    } else {
        const uint16_t h = (uint16_t)(pack2(w, 0.0f) & 0xffffu);
        *(uint16_t*)(L.imgF + img_mg_byte(L.joff + j, i, L.KT_F)) = h;
        if (L.imgB) {
            if (L.imgB_kmajor) *(uint16_t*)(L.imgB + img_k_byte(i, L.joff + j, L.MT_B)) = h;
            else *(uint16_t*)(L.imgB + img_mg_byte(i, L.joff + j, L.KT_B)) = h;
        }
    }
}
__device__ __forceinline__ void adam_element(const LayerDesc& L, bool is_bias, int i, int j, size_t idx, float g, bool update,
                                             float* param, float* mom, float* vel, const AdamCoef& c) {
    float w = param[idx];
    if (update) {
        float m = mom[idx], v = vel[idx];
        adam_math(w, m, v, g, c);
        mom[idx] = m;
        vel[idx] = v;
        param[idx] = w;
    }
    image_refresh(L, is_bias, i, j, w);
}

// Sums the per-split fp32 slabs of every layer into the flat gradient; with c.on the Adam update of the same
// elements follows in the same thread (single-GPU train step: no all-reduce sits between the two).
struct MeansArgs { const float* per_b; int B; float beta; float* out; };     // per_b == null: no extra block

// The grid covers reduce blocks [first_block, first_block + n) of the layer table: the whole table, or -- single-GPU
// train step -- the decoder's layers on the side stream and the rest on the main stream (see backward_impl).
__global__ __launch_bounds__(256) void reduce_grads_kernel(const LayerDesc* layers, int nlayers, float* grad, float* param, float* mom,
                                                           float* vel, AdamCoef c, MeansArgs mn, int first_block, int n1, int first_block2) {
    if (mn.per_b && blockIdx.x == gridDim.x - 1) {      // the one extra block of the grid: batch means of this step
        batch_means_block(mn.per_b, mn.B, mn.beta, mn.out);
        return;
    }
    // (two block ranges: the layers whose weight gradients ran on one side stream need not be neighbours in the table)
    const int bid = (int)blockIdx.x < n1 ? (int)blockIdx.x + first_block : (int)blockIdx.x - n1 + first_block2;
    // block = 64 groups of 4 consecutive out-features (float4 loads) x 4 split groups; partial sums meet in LDS.
    // A group never straddles a weight row: rblock counts are computed per row of 4-float groups (Nout4 = ceil(Nout/4)).
    __shared__ float4 red[4][64];
    int l = 0;
    while (l + 1 < nlayers && bid >= layers[l + 1].rblock_begin) ++l;
    const LayerDesc L = layers[l];
    const int n4 = (L.Nout + 3) >> 2;                       // float4 groups per weight row
    const int g = (bid - L.rblock_begin) * 64 + (threadIdx.x & 63);
    const int sg = threadIdx.x >> 6;
    const int ngroups = (L.Kin + 1) * n4;                   // Kin weight rows + 1 bias row
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    int i = 0, j = 0;
    const bool ok = g < ngroups;
    if (ok) {
        i = g / n4;
        j = (g - i * n4) * 4;
        const bool is_b = i == L.Kin;
        const float* p = is_b ? (L.slabB + L.joff + j) : (L.slabW + (size_t)i * L.slab_ld + L.joff + j);
        const size_t stride = is_b ? (L.slabB_stride ? L.slabB_stride : (size_t)L.slab_ld) : L.slab_stride;
        // slab rows start 16-byte aligned (joff, slab_ld multiples of 16 floats): float4 loads; columns >= Nout are pads (zeros / ignored)
        // 8 slabs' loads in flight per thread, summed in slab order (a 64-split layer was 4 round trips of 4 loads: the kernel's time
        // was this chain, not its bytes)
        if (L.nsplit <= 16) {      // few row splits (the encoder's layers): at most 4 loads per thread, all in flight
#pragma unroll 4
            for (int sp = sg; sp < L.nsplit; sp += 4) {
                const float4 v = *(const float4*)(p + (size_t)sp * stride);
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
        } else
        for (int sp0 = sg; sp0 < L.nsplit; sp0 += 32) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int sp = sp0 + 4 * u;
                v[u] = *(const float4*)(p + (size_t)(sp < L.nsplit ? sp : sg) * stride);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (sp0 + 4 * u < L.nsplit) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
        }
    }
    red[sg][threadIdx.x & 63] = s;
    __syncthreads();
    if (sg == 0 && ok) {
        const int t = threadIdx.x;
        float r[4] = {red[0][t].x + red[1][t].x + red[2][t].x + red[3][t].x, red[0][t].y + red[1][t].y + red[2][t].y + red[3][t].y,
                      red[0][t].z + red[1][t].z + red[2][t].z + red[3][t].z, red[0][t].w + red[1][t].w + red[2][t].w + red[3][t].w};
        float* dst = (i == L.Kin) ? (grad + L.offb + j) : (grad + L.offW + (size_t)i * L.Nout + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (j + e < L.Nout) {
                dst[e] = r[e];
                if (c.on) adam_element(L, i == L.Kin, i, j + e, (size_t)(dst - grad) + e, r[e], true, param, mom, vel, c);
            }
        }
    }
}

// Keras Adam (main.py:93): theta -= lr*sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps), eps = 1e-4;
// then refresh the bf16 A-images the GEMM kernels stream (forward W^T and backward W).
__global__ void adam_kernel(const LayerDesc* layers, int nlayers, float* param, const float* grad, float* mom, float* vel, AdamCoef c, int first_block) {
    const int bid = (int)blockIdx.x + first_block;       // the grid covers blocks [first_block, first_block + gridDim.x) of the layer table
    int l = 0;
    while (l + 1 < nlayers && bid >= layers[l + 1].block_begin) ++l;
    const LayerDesc L = layers[l];
    const int e = (bid - L.block_begin) * blockDim.x + threadIdx.x;
    const int nW = L.Kin * L.Nout;
    if (e >= nW + L.Nout) return;
    const bool is_b = e >= nW;
    const size_t idx = is_b ? (L.offb + (e - nW)) : (L.offW + e);
    adam_element(L, is_b, is_b ? 0 : e / L.Nout, is_b ? e - nW : e % L.Nout, idx, c.on ? grad[idx] : 0.0f, c.on != 0, param, mom, vel, c);
}
// ---------------------------------------------------------------------------------
// wgrad_rows_kernel (round 4): the weight gradients of a BasicBlock applied to FEW rows (the image encoder: R = batch size <= 2 048)
// with the WHOLE row reduction inside one workgroup -- no row splits, no fp32 slabs, no reduction launch -- and the Keras Adam update
// (+ weight-image refresh) of the workgroup's 64 x 64 block of the weight matrix in its epilogue.  Before: wgradp_group_kernel (32 - 48
// workgroups of 256 x 128 features walking row splits: 18.6 us alone) -> slabs -> reduce_grads_kernel (+ Adam: 14.6 us), two dependent
// launches at the END of the step's main chain, in front of the next encoder forward.
//   grid: one workgroup per (linear map, 64 in-features, 64 out-features) [+ one block for the step's batch means]
//   wave w of 4: data rows [w*RW, (w+1)*RW) -- its own ring of 4 stages x 32 rows x (128 B of X + 128 B of G) filled by its own LDS-DMA and
//   read back through ds_read_b64_tr_b16 (the P-layout operands are row-major; the contraction index is the data row): no workgroup
//   barrier in the loop, a wave waits only for its own vmcnt.  16 accumulator tiles (4 i-tiles x 4 j-tiles) per wave + the bias
//   gradient through the matrix pipe (ones x G).  The four waves' partial sums meet in LDS (fixed order: deterministic), then every
//   thread owns 16 elements: gradient -> flat buffer, and (c.on) m, v, theta, the bf16 images.  Reference: tape.gradient + apply_gradients,
//   src/iwae1.py:159-160 (Adam: main.py:93).
// ---------------------------------------------------------------------------------
struct WgradRowsArgs {
    WgradRowsJob job[WGR_MAX_JOBS];
    int njobs;
    const LayerDesc* layers;
    float *grad, *param, *mom, *vel;
    AdamCoef c;
    MeansArgs mn;              // per_b != null: the last block of the grid makes the step's batch means
    const char* zero;          // >= 1 KiB of zeros
};
#define WGR_NST 4
#define WGR_STAGE 8192         // bytes per stage and wave: 32 rows x 128 B of X, 32 rows x 128 B of G
__global__ __launch_bounds__(256, 1) void wgrad_rows_kernel(WgradRowsArgs a) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    typedef __attribute__((ext_vector_type(4))) short v4s;
    if (a.mn.per_b && blockIdx.x == gridDim.x - 1) {
        batch_means_block(a.mn.per_b, a.mn.B, a.mn.beta, a.mn.out);
        return;
    }
    int jn = 0;
#pragma unroll
    for (int t = 1; t < WGR_MAX_JOBS; ++t)
        if (t < a.njobs && (int)blockIdx.x >= a.job[t].wg_begin) jn = t;
    const WgradRowsJob J = a.job[jn];
    const int wl = (int)blockIdx.x - J.wg_begin;
    const int bi = wl / J.jb, bj = wl - bi * J.jb;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane >> 4, l16 = lane & 15, qp = l16 >> 2, p = l16 & 3;
    const int RW = ((J.R + 3) / 4 + 31) & ~31;                  // data rows per wave (multiple of the 32-row stage)
    const int rbeg = wave * RW, rend = min(J.R, rbeg + RW);
    const int nstage = rend > rbeg ? (rend - rbeg + 31) / 32 : 0;
    char* ring = smem + wave * (WGR_NST * WGR_STAGE);
    // 16-byte slot s of row r lands at slot s ^ swz(r) (applied on the SOURCE address): at a 128-byte row pitch odd rows are half a bank
    // cycle apart by themselves, row bit 1 picks the other half (the narrow strip of wgradws_kernel)
    auto swz = [](int r) { return ((r >> 1) & 1) << 2; };
    // DMA pieces of a stage: 4 of X (8 rows x 128 B each), 4 of G; a lane fetches the same (row in stage, slot) in every stage
    const int prl = lane >> 3, psl = lane & 7;
    const char* zsrc = a.zero + lane * 16;
    const char* xsrc[4]; const char* gsrc[4]; int xlim[4], glim[4];
#pragma unroll
    for (int pc = 0; pc < 4; ++pc) {
        const int rl = 8 * pc + prl;
        const int cx = bi * 64 + ((psl ^ swz(rl)) * 8), cg = bj * 64 + ((psl ^ swz(rl)) * 8);
        xsrc[pc] = (const char*)J.X + ((size_t)(rbeg + rl) * J.ldX + cx) * 2;
        gsrc[pc] = (const char*)J.G + ((size_t)(rbeg + rl) * J.ldG + cg) * 2;
        xlim[pc] = cx < J.ldX ? rend - rbeg - rl : -(1 << 30);      // the piece's row is valid in stage c iff 32*c < lim
        glim[pc] = cg < J.ldG ? rend - rbeg - rl : -(1 << 30);
    }
    const size_t xstride = (size_t)32 * J.ldX * 2, gstride = (size_t)32 * J.ldG * 2;
    auto issue = [&](int c) {
        const uint32_t base = lds_addr_of(ring + (c % WGR_NST) * WGR_STAGE);
#pragma unroll
        for (int pc = 0; pc < 4; ++pc)
            glds16(32 * c < xlim[pc] ? xsrc[pc] + (size_t)c * xstride : zsrc, (uint32_t)__builtin_amdgcn_readfirstlane((int)(base + (uint32_t)pc * 1024u)));
#pragma unroll
        for (int pc = 0; pc < 4; ++pc)
            glds16(32 * c < glim[pc] ? gsrc[pc] + (size_t)c * gstride : zsrc, (uint32_t)__builtin_amdgcn_readfirstlane((int)(base + 4096u + (uint32_t)pc * 1024u)));
    };
    f32x4 acc[4][4], accb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        accb[u] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t][u] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    }
    const uint4 ones = make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u);      // bf16 1.0 x 8
    const bool do_bias = bi == 0;
    for (int c = 0; c < min(nstage, WGR_NST - 1); ++c) issue(c);
    const int row_off = (4 * q + qp) * 128;
    for (int c = 0; c < nstage; ++c) {
        wait_vmem_but_ws(8 * min(WGR_NST - 2, nstage - 1 - c));     // stage c has landed; the (<= 2) younger stages may still fly
        if (c + WGR_NST - 1 < nstage) issue(c + WGR_NST - 1);        // into the buffer stage c - 1 has left (its reads fed MFMAs already issued)
        const char* xb = ring + (c % WGR_NST) * WGR_STAGE + row_off;
        const char* gb = xb + 4096;
        auto frag = [&](const char* base, int t) {       // tile t of the 64-feature block: P chunk 4*(t>>1)+p (swizzled by the row), half t&1
            const char* p0 = base + ((((4 * (t >> 1)) ^ swz(qp)) + p) * 16) + 8 * (t & 1);
            const v4s r0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)p0);
            const v4s r1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(p0 + 16 * 128));
            const uint2 lo = __builtin_bit_cast(uint2, r0), hi = __builtin_bit_cast(uint2, r1);
            return make_uint4(lo.x, lo.y, hi.x, hi.y);
        };
        uint4 g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) g[u] = frag(gb, u);
        if (J.rowscale) {      // row-weighted G (workgroup-uniform): a fragment's 8 data rows are 4q..4q+3 and 16+4q..16+4q+3 of the stage; dl = bf16(g_r * s), one rounding
            const float* rs = J.rowscale + rbeg + 32 * c + 4 * q;
            const float4 s0 = *(const float4*)rs, s1 = *(const float4*)(rs + 16);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                g[u] = make_uint4(pack2(bflo(g[u].x) * s0.x, bfhi(g[u].x) * s0.y), pack2(bflo(g[u].y) * s0.z, bfhi(g[u].y) * s0.w),
                                  pack2(bflo(g[u].z) * s1.x, bfhi(g[u].z) * s1.y), pack2(bflo(g[u].w) * s1.z, bfhi(g[u].w) * s1.w));
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint4 av = frag(xb, t);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[t][u] = mfma16(av, g[u], acc[t][u]);
        }
        if (do_bias) {
#pragma unroll
            for (int u = 0; u < 4; ++u) accb[u] = mfma16(ones, g[u], accb[u]);
        }
    }
    // the waves' partial sums meet in LDS: each wave writes its 16 tiles into its own ring (conflict-free 16-byte stores), the bias row behind them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) *(f32x4*)(ring + ((t * 4 + u) * 64 + lane) * 16) = acc[t][u];
    if (q == 0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) *(float*)(ring + 16384 + (u * 16 + l16) * 4) = accb[u][0];
    }
    __syncthreads();
    // Epilogue.  Thread (wave, lane) owns, of the 64 x 64 block, the i-tiles t = 2s, 2s+1 (s = wave >> 1: one 32-in-feature k-step) and the
    // j-tiles u = 2(wave & 1), +1 with the accumulator's lane map: i = 64 bi + 16t + 4q + ii, j = 64 bj + 16u + l16 -- 16 elements, of which
    // the 8 of one u (two tiles x four in-features) are ONE 16-byte chunk of the forward weight image (layout.h: a lane's 8 values of a
    // k-step).  All sums first, then theta / m / v requested in one batch, the arithmetic, the stores; the new weights go into the images as
    // 16-byte stores -- the forward image straight from registers, the backward image (rows = in-features) through a bf16 tile in LDS.
    // (Element by element with 2-byte image stores the epilogue was 16 dependent round trips and ~100 scattered stores per thread: 15 of
    // the kernel's 18 us.)
    const int jg = bj * 64;
    const LayerDesc L0 = a.layers[J.sub0];
    const LayerDesc L1 = a.layers[J.sub1 >= 0 ? J.sub1 : J.sub0];
    const int s2 = wave >> 1, u0 = 2 * (wave & 1);
    float gsum[16], pw[16], pm[16], pv[16];
    size_t eidx[16];
    bool eok[16];
    char* tileB = smem + 20480;                 // bf16 [64 in-features][64 out-features], pitch 144 B (behind wave 0's tiles and bias row)
    constexpr int TB_PITCH = 144;
#pragma unroll
    for (int uu = 0; uu < 2; ++uu) {
        const int u = u0 + uu;
        const bool second = J.sub1 >= 0 && jg + 16 * u >= J.split;       // (wave-uniform: the split is a multiple of 32 features)
        const int joff = second ? L1.joff : L0.joff, Nout = second ? L1.Nout : L0.Nout, Kin = second ? L1.Kin : L0.Kin;
        const size_t offW = second ? L1.offW : L0.offW;
        const int jj = jg + 16 * u + l16 - joff;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int n = (2 * s2 + tt) * 4 + u;
            f32x4 v = *(const f32x4*)(smem + (n * 64 + lane) * 16);
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const f32x4 o = *(const f32x4*)(smem + w * (WGR_NST * WGR_STAGE) + (n * 64 + lane) * 16);
                v[0] += o[0]; v[1] += o[1]; v[2] += o[2]; v[3] += o[3];
            }
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
                const int i = bi * 64 + 32 * s2 + 16 * tt + 4 * q + ii, e = 8 * uu + 4 * tt + ii;
                eok[e] = jj >= 0 && jj < Nout && i < Kin;
                eidx[e] = eok[e] ? offW + (size_t)i * Nout + jj : offW;
                gsum[e] = v[ii];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        pw[e] = a.param[eidx[e]];
        if (a.c.on) { pm[e] = a.mom[eidx[e]]; pv[e] = a.vel[eidx[e]]; }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        if (eok[e]) {
            a.grad[eidx[e]] = gsum[e];
            if (a.c.on) {
                adam_math(pw[e], pm[e], pv[e], gsum[e], a.c);
                a.mom[eidx[e]] = pm[e];
                a.vel[eidx[e]] = pv[e];
                a.param[eidx[e]] = pw[e];
            }
        } else {
            pw[e] = 0.0f;          // pad rows / columns of the images stay zero
        }
    }
    if (a.c.on) {
        // forward image (rows = out-features): this lane's 8 in-features of k-step (64 bi + 32 s2) / 32 for out-feature j
#pragma unroll
        for (int uu = 0; uu < 2; ++uu) {
            const int jl = 16 * (u0 + uu) + l16, j = jg + jl;
            const int kf0 = bi * 64 + 32 * s2 + 4 * q;
            const uint4 ch = make_uint4(pack2(pw[8 * uu + 0], pw[8 * uu + 1]), pack2(pw[8 * uu + 2], pw[8 * uu + 3]),
                                        pack2(pw[8 * uu + 4], pw[8 * uu + 5]), pack2(pw[8 * uu + 6], pw[8 * uu + 7]));
            if (j < J.ldG && kf0 < 32 * L0.KT_F) *(uint4*)(L0.imgF + img_mg_byte(j, kf0, L0.KT_F)) = ch;
            if (L0.imgB) {
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {      // tile [in-feature 32 s2 + 16 tt + 4q + ii][out-feature jl]
#pragma unroll
                    for (int ii = 0; ii < 4; ++ii)
                        *(uint16_t*)(tileB + (32 * s2 + 16 * tt + 4 * q + ii) * TB_PITCH + jl * 2) = (uint16_t)(pack2(pw[8 * uu + 4 * tt + ii], 0.0f) & 0xffffu);
                }
            }
        }
        if (L0.imgB) {      // backward image (rows = in-features, k = out-feature space): 512 chunks of 16 bytes per block, two per thread
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int c = tid + 256 * r, il = c >> 3, sp = (c >> 2) & 1, qq = c & 3;
                const int i = bi * 64 + il, kf0 = jg + 32 * sp + 4 * qq;
                const uint2 lo = *(const uint2*)(tileB + il * TB_PITCH + (32 * sp + 4 * qq) * 2);
                const uint2 hi = *(const uint2*)(tileB + il * TB_PITCH + (32 * sp + 16 + 4 * qq) * 2);
                // (MG-major or K-major: the 16-byte chunk of (row i, k-step quarter) holds the same 8 out-features either way, layout.h)
                if (i < J.ldX && kf0 < J.ldG)
                    *(uint4*)(L0.imgB + (L0.imgB_kmajor ? img_k_byte(i, kf0, L0.MT_B) : img_mg_byte(i, kf0, L0.KT_B))) = make_uint4(lo.x, lo.y, hi.x, hi.y);
            }
        }
    }
    if (do_bias && tid < 64) {
        float b = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) b += *(const float*)(smem + w * (WGR_NST * WGR_STAGE) + 16384 + tid * 4);
        const int j = jg + tid;
        const bool second = J.sub1 >= 0 && j >= J.split;
        const LayerDesc L = second ? a.layers[J.sub1] : L0;
        const int jj = j - L.joff;
        if (jj >= 0 && jj < L.Nout) {
            const size_t idx = L.offb + jj;
            a.grad[idx] = b;
            if (a.c.on) adam_element(L, true, 0, jj, idx, b, true, a.param, a.mom, a.vel, a.c);
        }
    }
}

// ---------------------------------------------------------------------------------
// launch wrappers (plain C++ callers in model.hip; LAUNCH_EV: step_helpers.h)
// ---------------------------------------------------------------------------------
void launch_reduce_grads(const LayerDesc* layers, int nlayers, int first_block, int nblocks, float* grad, float* param, float* mom, float* vel,
                         float alpha, float beta1, float beta2, float eps, int fuse_adam, const float* per_b, int B, float beta, float* scalars, hipStream_t st,
                         int first_block2, int nblocks2, hipEvent_t done) {
    const AdamCoef c = {alpha, 1.0f, beta1, beta2, eps, fuse_adam};
    const MeansArgs mn = {per_b, B, beta, scalars};
    LAUNCH_EV(done, reduce_grads_kernel, dim3(nblocks + nblocks2 + (per_b ? 1 : 0)), dim3(256), 0, st, layers, nlayers, grad, param, mom, vel, c, mn, first_block, nblocks,
              first_block2);
}
void launch_scalars(const float* per_b, int B, float beta, float* out, hipStream_t st) {
    hipLaunchKernelGGL(scalars_kernel, dim3(1), dim3(256), 0, st, per_b, B, beta, out);
}
void launch_adam(const LayerDesc* layers, int nlayers, int nblocks, float* param, const float* grad, float* mom, float* vel,
                 float alpha, float gscale, float beta1, float beta2, float eps, int do_update, hipStream_t st, int first_block, hipEvent_t done) {
    const AdamCoef c = {alpha, gscale, beta1, beta2, eps, do_update};
    LAUNCH_EV(done, adam_kernel, dim3(nblocks), dim3(256), 0, st, layers, nlayers, param, grad, mom, vel, c, first_block);
}
void launch_wgrad_rows(const WgradRowsJob* jobs, int njobs, const LayerDesc* layers, float* grad, float* param, float* mom, float* vel, float alpha,
                       float beta1, float beta2, float eps, int fuse_adam, const float* per_b, int B, float beta, float* scalars, const char* zero, hipStream_t st) {
    WgradRowsArgs a;
    memset(&a, 0, sizeof(a));
    int wgs = 0;
    for (int i = 0; i < njobs && i < WGR_MAX_JOBS; ++i) {
        a.job[i] = jobs[i];
        a.job[i].ib = (jobs[i].ldX + 63) / 64;
        a.job[i].jb = (jobs[i].ldG + 63) / 64;
        a.job[i].wg_begin = wgs;
        wgs += a.job[i].ib * a.job[i].jb;
    }
    a.njobs = njobs;
    a.layers = layers; a.grad = grad; a.param = param; a.mom = mom; a.vel = vel;
    a.c = AdamCoef{alpha, 1.0f, beta1, beta2, eps, fuse_adam};
    a.mn = MeansArgs{per_b, B, beta, scalars};
    a.zero = zero;
    hipLaunchKernelGGL(wgrad_rows_kernel, dim3(wgs + (per_b ? 1 : 0)), dim3(256), (size_t)4 * WGR_NST * WGR_STAGE, st, a);
}

}  // namespace iwae
