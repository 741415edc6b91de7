// gfx950 (CDNA4, MI355X) kernels of the bf16 train step that turn activations and their gradients into weight-gradient slabs
// (reduce_grads_kernel in update_kernels.hip sums the slabs); the launchers are at the end of the file.
// Layout rules: layout.h.  Kernel -> reference mapping (file:line in the reference, as at the top of kernels.hip):
//   wgradp_kernel / wgradws_kernel / the *_group*_kernel
//                                    tape.gradient(loss, w)   src/iwae1.py:155-159
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
// wgradp_kernel: weight gradient straight from the ROW-major P-layout activations (no feature-major copies):
//   out[i][j] = sum_r X[r][i] * G[r][j],   X: bf16 [rows][ldX], G: bf16 [rows][ldG]  (both P-layout)
// The contraction index (data row) is the strided one in memory, so both MFMA operands are produced by the
// hardware-transposing LDS read: per 64-row chunk the X tile (<=256 features) and the G strip (NW*16
// features) are DMA'd row-major into LDS (16-byte slot s of row r lands at slot s ^ ((r&3)<<2), the swizzle
// is applied on the per-lane SOURCE address), and a fragment is two ds_read_b64_tr_b16 (4 rows x 16 features
// each; 2-way bank conflict by construction: every lane uses one half of a 16-byte slot).  P-layout's feature
// permutation is undone for free by which 8-byte piece a lane addresses.  Rows >= M read a zero line.
// grid = (j-blocks of NW*16 features, i-blocks of 256 features, row splits); fp32 slabs as before.
// ---------------------------------------------------------------------------------
// Register blocking: the NW waves form a WI x (NW/WI) grid; a wave owns 16/WI i-tiles x WI j-tiles (16 accumulator tiles
// either way) and reads 16/WI + WI fragments per 32-row step instead of 16 + 1 -- the transposing LDS reads (2-way bank
// conflict by construction) were what a 64-row chunk waited for (4 352 LDS cycles per chunk against 2 048 MFMA cycles per
// SIMD at 16 x 1).  The row-weighted variant scales every G fragment it reads, so it takes the 8 x 2 shape.
// counted wait: all but the wave's n youngest vector-memory operations (here: LDS-DMA pieces, issued in stage order) are done
__device__ __forceinline__ void wait_vmem_but(int n) {      // n wave-uniform, 0..12
    switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
        case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
        case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
        case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
        case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    }
}

// Staging: the operands move through a RING of WG_NST LDS stages of WG_SR = 32 data rows each; while stage c is multiplied the
// DMA of stage c + 3 is issued (pieces spread between the MFMAs), and the top of stage c + 1 waits only for ITS pieces
// (s_waitcnt vmcnt(n) with the two younger stages' pieces still in flight).  Round 1 double-buffered 64-row chunks and
// waited for chunk c + 1 right after issuing its last piece: every chunk exposed one full HBM round trip (~1.5-2 us under
// load against ~1 us of MFMA + LDS work; 3.9 us per chunk measured on the output layer's gradient = 0.13 of the HBM peak).
#define WG_SR 32
#define WG_NST 4
// diagnostic ablations of the weight-gradient kernels (WgradPArgs.dbg: timing only, results are wrong) exist in DIAG=1 builds only;
// in the shipped kernels the conditions fold to false at compile time
// (WG_DBG: defined in step_helpers.h)
// Shapes <NW waves, IGC i-groups, AI x BJ accumulator tiles per wave>: the waves form an IGC x (NW/IGC) grid, the workgroup's
// output tile is IGC*AI i-tiles x (NW/IGC)*BJ j-tiles.  A 32-row stage costs a wave AI + BJ fragment reads for AI*BJ MFMAs:
//   <16, 4, 4, 4>  256 x 256 features, 0.50 reads per MFMA (round 1's shape; the hidden layers at large row counts)
//   <16, 2, 8, 2>  the same tile for the row-weighted variant (scales its 2 G fragments), 0.63
//   < 8, 2, 7, 4>  224 x 256 features with EIGHT waves (two per SIMD, 28 accumulator tiles each): 0.39 reads per MFMA -- below the
//                  0.5 at which the LDS (2-way conflict of the transposing reads: 128 B/clk) keeps up with the MFMA pipes -- and
//                  half the waves at every barrier; for layers whose input is <= 224 features wide (the decoder's)
//   < 8, 4, 4, 4>  256 x 128 features, 8 waves: small row counts (grouped launch for an encoder block)
template <int NW, int IGC, int AI, int BJ, bool SC>     // SC: G rows carry a per-row weight (a.rowscale), staged through LDS with the tiles
__device__ __forceinline__ void wgradp_body(const WgradPArgs& a, const int bx, const int by, const int bz) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    constexpr int XT_BYTES = WG_SR * 512;              // X tile: 32 rows x 512 B (256 features)
    constexpr int JGC = NW / IGC, STRIP = JGC * BJ;    // j-tiles of the workgroup's G strip
    constexpr int GROW = STRIP * 32;                   // G strip row bytes (512 for 16 j-tiles, 256 for 8)
    constexpr int GT_BYTES = WG_SR * GROW;
    constexpr int BUF = XT_BYTES + GT_BYTES + (SC ? 1024 : 0);
    constexpr int XP = XT_BYTES / 1024, GP = GT_BYTES / 1024, NPC = XP + GP + (SC ? 1 : 0), NIDX = (NPC + NW - 1) / NW;
    typedef __attribute__((ext_vector_type(4))) short v4s;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane >> 4, l16 = lane & 15, qp = l16 >> 2, p = l16 & 3;
    const int ig = wave % IGC, jg = wave / IGC;        // the wave's i-tiles ig*AI .. +AI-1, local j-tiles jg*BJ .. +BJ-1
    const int it0 = by * 16;
    const int nit = min(IGC * AI, a.IT - it0);
    const int split = bz;
    const int rbeg = split * a.rows_per_split;
    const int rend = min(a.M, rbeg + a.rows_per_split);
    const int nstage = (rend - rbeg + WG_SR - 1) / WG_SR;
    const int xcol0 = it0 * 16, gcol0 = bx * STRIP * 16;    // first feature (= P position, both multiples of 32) of the tiles
    int my_pieces = 0;                                       // DMA pieces this wave issues per stage (wave-uniform)
#pragma unroll
    for (int idx = 0; idx < NIDX; ++idx) my_pieces += (wave + NW * idx < NPC) ? 1 : 0;

    // one DMA piece = 1 KiB of LDS = 2 X rows (32 slots each) or 1024/GROW G rows.  A lane fetches the same (row in stage,
    // 16-byte chunk) of its pieces in every stage: the source address is a per-lane base + stage * (32 rows of bytes), both
    // precomputed (as per-stage 64-bit index arithmetic it was ~25 vector instructions per piece, 96 per wave and stage in
    // all against 16 MFMAs -- SQ_INSTS_VALU of the round-2 profile).
    const char* zsrc = a.zero + (lane & 31) * 16;
    const char* pbase[NIDX];       // lane's source at stage 0
    int plim[NIDX];                // the piece's row is valid in stage c iff c * WG_SR < plim
    int pstride[NIDX];             // bytes per stage (wave-uniform)
#pragma unroll
    for (int idx = 0; idx < NIDX; ++idx) {
        const int pc = wave + NW * idx;               // wave-uniform
        pbase[idx] = zsrc; plim[idx] = -(1 << 30); pstride[idx] = 0;
        if (pc < XP) {
            const int rl = 2 * pc + (lane >> 5), sl = lane & 31;
            const int col = xcol0 + (sl ^ ((rl & 3) << 2)) * 8;           // source 16-byte chunk of this LDS slot
            pbase[idx] = (const char*)a.X + ((size_t)(rbeg + rl) * a.ldX + col) * 2;
            plim[idx] = col < a.ldX ? rend - rbeg - rl : -(1 << 30);
            pstride[idx] = WG_SR * a.ldX * 2;
        } else if (SC && pc == XP + GP) {                                // the stage's 32 row weights (128 B; the pad rows of gx are finite)
            pbase[idx] = (const char*)(a.rowscale + rbeg) + (lane & 7) * 16;
            plim[idx] = lane < WG_SR / 4 ? (1 << 30) : -(1 << 30);
            pstride[idx] = WG_SR * 4;
        } else if (pc < NPC) {
            constexpr int SPR = GROW / 16, RPP = 1024 / GROW;            // slots per row, rows per piece
            const int rl = RPP * (pc - XP) + lane / SPR, sl = lane % SPR;
            const int col = gcol0 + (sl ^ ((rl & 3) << 2)) * 8;
            pbase[idx] = (const char*)a.G + ((size_t)(rbeg + rl) * a.ldG + col) * 2;
            plim[idx] = col < a.ldG ? rend - rbeg - rl : -(1 << 30);
            pstride[idx] = WG_SR * a.ldG * 2;
        }
    }
    auto dma_piece = [&](int c, int idx) {
        const int pc = wave + NW * idx;               // wave-uniform
        if (pc >= NPC) return;
        const char* src = (c * WG_SR < plim[idx]) ? pbase[idx] + (size_t)c * (size_t)pstride[idx] : zsrc;
        glds16(src, (uint32_t)__builtin_amdgcn_readfirstlane((int)(lds_addr_of(smem + (c % WG_NST) * BUF) + (uint32_t)pc * 1024u)));
    };

    f32x4 acc[AI][BJ];
#pragma unroll
    for (int t = 0; t < AI; ++t)
#pragma unroll
        for (int u = 0; u < BJ; ++u) acc[t][u] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    float bsum[BJ];
#pragma unroll
    for (int u = 0; u < BJ; ++u) bsum[u] = 0.0f;
    for (int c = 0; c < min(nstage, WG_NST - 1); ++c) {
#pragma unroll
        for (int idx = 0; idx < NIDX; ++idx) dma_piece(c, idx);
    }
    // lane-constant parts of the transposing-read addresses: row 4q+q' of a 16-row half-step, piece p
    const int xrow_off = (4 * q + qp) * 512, grow_off = (4 * q + qp) * GROW;

    for (int c = 0; c < nstage; ++c) {
        const int buf = c % WG_NST;
        wait_vmem_but(my_pieces * min(WG_NST - 2, nstage - 1 - c));      // stage c has landed; the (<= 2) younger stages may still fly
        __syncthreads();                                                 // ... for every wave; and everyone is done reading stage c - 1
        const bool more = c + WG_NST - 1 < nstage && !WG_DBG(a, 1);       // stage c + 3 goes into the buffer stage c - 1 has just left
        int dma_idx = 0;
        auto dma_next = [&]() {
            if (more && dma_idx < NIDX) dma_piece(c + WG_NST - 1, dma_idx);
            ++dma_idx;
        };
        const char* xb = smem + buf * BUF + xrow_off + p * 16;
        const char* gbase = smem + buf * BUF + XT_BYTES + grow_off;
        {
            // B fragments: 8 data rows (two 4-row blocks) of each of this wave's BJ j-tiles (local tile jl -> chunk 4*(jl>>1)+p, half jl&1)
            uint4 g[BJ];
#pragma unroll
            for (int u = 0; u < BJ; ++u) {
                const int jl = jg * BJ + u;
                const char* gb = gbase + ((((4 * (jl >> 1)) ^ (qp << 2)) + p) * 16) + 8 * (jl & 1);
                const v4s g0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)gb);
                const v4s g1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(gb + 16 * GROW));
                const uint2 glo = __builtin_bit_cast(uint2, g0), ghi = __builtin_bit_cast(uint2, g1);
                g[u] = make_uint4(glo.x, glo.y, ghi.x, ghi.y);
            }
            if (SC && !WG_DBG(a, 8)) {      // the lane's 8 data rows: 4q..4q+3 and 16+4q..16+4q+3 of this 32-row stage (output layer: G = s, weight = dLoss/dlpxz)
                const float* scl = (const float*)(smem + buf * BUF + XT_BYTES + GT_BYTES) + 4 * q;
                const float4 s0 = *(const float4*)scl, s1 = *(const float4*)(scl + 16);
#pragma unroll
                for (int u = 0; u < BJ; ++u)
                    g[u] = make_uint4(pack2(bflo(g[u].x) * s0.x, bfhi(g[u].x) * s0.y), pack2(bflo(g[u].y) * s0.z, bfhi(g[u].y) * s0.w),
                                      pack2(bflo(g[u].z) * s1.x, bfhi(g[u].z) * s1.y), pack2(bflo(g[u].w) * s1.z, bfhi(g[u].w) * s1.w));
            }
            if (ig == 0 && !WG_DBG(a, 4)) {       // bias gradient = column sums of G: one wave per j-tile (wave-uniform branch)
#pragma unroll
                for (int u = 0; u < BJ; ++u)
                    bsum[u] += bflo(g[u].x) + bfhi(g[u].x) + bflo(g[u].y) + bfhi(g[u].y) + bflo(g[u].z) + bfhi(g[u].z) + bflo(g[u].w) + bfhi(g[u].w);
            }
            if (!WG_DBG(a, 2)) lds_pipeline<AI, (AI < 3 ? AI : 3)>(
                [&](int t) {       // A fragment of i-tile i: P chunk 4*(i>>1)+p (swizzled by the row), half i&1
                    const int i = ig * AI + t;
                    const char* p0 = xb + ((((4 * (i >> 1)) ^ (qp << 2))) * 16) + 8 * (i & 1);
                    const v4s r0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)p0);
                    const v4s r1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(p0 + 16 * 512));
                    const uint2 lo = __builtin_bit_cast(uint2, r0), hi = __builtin_bit_cast(uint2, r1);
                    return make_uint4(lo.x, lo.y, hi.x, hi.y);
                },
                [&](int t, const uint4& av) {
                    if (ig * AI + t < nit) {
#pragma unroll
                        for (int u = 0; u < BJ; ++u) acc[t][u] = mfma16(av, g[u], acc[t][u]);
                    }
                },
                [&](int t) { if (t == 0 || (AI > 1 && t == AI / 2) || (AI > 3 && t == AI - 1)) dma_next(); });
        }
        while (dma_idx < NIDX) dma_next();
    }

    // D: lane(col j = lane&15, quad q) reg ii -> out[i = 16*it + 4q + ii][j]
    float* slab = a.slabW + (size_t)split * a.IT * 16 * a.JT * 16;
    if (WG_DBG(a, 16)) return;
#pragma unroll
    for (int u = 0; u < BJ; ++u) {
        const int jt = bx * STRIP + jg * BJ + u;
        if (jt < a.JT) {
#pragma unroll
            for (int t = 0; t < AI; ++t) {
                const int it = ig * AI + t;
                if (it < nit) {
#pragma unroll
                    for (int ii = 0; ii < 4; ++ii)
                        slab[(size_t)((it0 + it) * 16 + 4 * q + ii) * (a.JT * 16) + jt * 16 + l16] = acc[t][u][ii];
                }
            }
            if (by == 0 && ig == 0) {
                float v = bsum[u];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if (q == 0) a.slabB[(size_t)split * a.JT * 16 + jt * 16 + l16] = v;
            }
        }
    }
}

template <int NW, int IGC, int AI, int BJ, bool SC>
__global__ __launch_bounds__(NW * 64, (AI * BJ > 16) ? 2 : NW / 4) void wgradp_kernel(WgradPArgs a) {
    // XCD-aware block order: the hardware deals workgroups round-robin to the 8 XCDs (private L2 each).  Renumber
    // so that blocks which share operands -- the j-blocks / i-blocks of one row split -- sit on ONE XCD and are
    // dispatched back to back: the shared X tile then comes from HBM once instead of once per j-block.
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    const int gx = gridDim.x, gy = gridDim.y, nb = gx * gy * (int)gridDim.z;
    if ((nb & 7) == 0) {
        const int L = bx + gx * (by + gy * bz);
        const int V = (L & 7) * (nb >> 3) + (L >> 3);
        bx = V % gx; by = (V / gx) % gy; bz = V / (gx * gy);
    }
    wgradp_body<NW, IGC, AI, BJ, SC>(a, bx, by, bz);
}

// ---------------------------------------------------------------------------------
// wgradws_kernel: the weight gradient of a layer whose input is <= 224 features wide (the decoder's three layers) at large
// row counts, with SPECIALISED waves.  Ablations of wgradp_kernel on the output layer (alone on the machine, 90 us): without its
// MFMAs and A-fragment reads 92 us, without the DMA 73, without the row scaling 74, without the bias sums 82, with none of the
// four 29 -- every wave's own instruction stream (DMA issue ~14 instructions per 1 KiB piece, 80 vector instructions of row
// scaling, 64 of bias sums, ~100 scalar ones of loop skeleton, per 28 MFMAs) is what a 32-row stage takes, run in sequence by
// waves that a barrier keeps in lockstep; the MFMA pipe idles 3/4 of the time.  Here:
//   * 8 COMPUTE waves (2 x 4 grid, 7 x 4 accumulator tiles each = 224 x 256 features) only read fragments and multiply; the bias
//     gradient (column sums of G) comes out of the matrix pipe too (one MFMA per G fragment against an all-ones A fragment);
//   * 4 LOADER waves issue all LDS-DMA of the stage ring (3 stages ahead); in the row-weighted variant (the output layer: G = the
//     stored s, weight = dLoss/dlpxz of the row) the G strip travels through the loaders' REGISTERS instead and is multiplied by
//     the row weight on the way into LDS (bf16, one rounding: dl = bf16(g_r * s)) -- see the loader branch below.
// One barrier per stage: behind it the compute waves own stage c + 1 (landed, weighted) and the loaders own the buffer of
// stage c (to refill).
// ---------------------------------------------------------------------------------
// (wait_vmem_but_ws, the counted wait for any count 0..24: step_helpers.h -- wgrad_rows_kernel in update_kernels.hip waits with it too)
// <SC, BJ, NLW>: BJ = j-tiles per compute wave (the workgroup's G strip is 4*BJ tiles wide), NLW = loader waves.
//   <.., 4, 4>: 224 x 256 features per workgroup, 8 + 4 waves at <= 168 registers (three per SIMD)
//   <.., 2, 8>: 224 x 128 features, 8 + 8 waves at <= 128 registers (four per SIMD): a third of the DMA issues and a quarter of the
//               scaling per loader and stage -- the loaders' instruction stream is what a stage takes (see above) -- for 1.75x the
//               X-tile traffic out of L2 (seven column blocks instead of four)
#ifdef IWAE_DENSE_STAMPS      // diagnostic build: cycles per phase and wave -> a.stamps[workgroup * waves + wave][8]
#define WS_STAMP(slot)                                                                 \
    {                                                                                  \
        unsigned long long t_;                                                         \
        __builtin_amdgcn_sched_barrier(0);                                             \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");     \
        __builtin_amdgcn_sched_barrier(0);                                             \
        ws_sum[slot] += t_ - ws_prev;                                                  \
        ws_prev = t_;                                                                  \
    }
#define WS_STAMP_OUT()                                                                                                         \
    if (a.stamps && lane == 0) {                                                                                               \
        for (int i_ = 0; i_ < 8; ++i_) a.stamps[((size_t)sid * (NCW + NLW) + wave) * 8 + i_] = ws_sum[i_];                     \
    }
#else
#define WS_STAMP(slot)
#define WS_STAMP_OUT()
#endif
// XCD-aware block order (see wgradp_kernel): the j-blocks of one row split share an XCD's L2
__device__ __forceinline__ void wgradws_block(int& bx, int& bz, const int gx, const int nz) {
    const int nb = gx * nz;
    if ((nb & 7) == 0) {
        const int L = bx + gx * bz;
        const int V = (L & 7) * (nb >> 3) + (L >> 3);
        bx = V % gx; bz = V / gx;
    }
}
// jt0: first j-tile (16 out-features) of the workgroup's G strip, bz: its row split, sid: its slot in the diagnostic stamp buffer
template <bool SC, int BJ, int NLW>
__device__ __forceinline__ void wgradws_body(const WgradPArgs& a, const int jt0, const int bz, const int sid) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
#ifdef IWAE_DENSE_STAMPS
    unsigned long long ws_sum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ws_prev = 0;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(ws_prev)::"memory");
#endif
    constexpr int AI = 7, IGC = 2, NCW = 8, STRIP = 4 * BJ;
    constexpr int XT_BYTES = WG_SR * 512, GROW = STRIP * 32, GT_BYTES = WG_SR * GROW, BUF = XT_BYTES + GT_BYTES;
    constexpr int XP = XT_BYTES / 1024, GP = GT_BYTES / 1024, XPL = XP / NLW, GPL = GP / NLW, PPL = XPL + GPL;      // pieces per loader and stage
    constexpr int SPR = GROW / 16, RPP = 1024 / GROW;                   // G strip: 16-byte slots per row, rows per 1 KiB piece
    static_assert(XP % NLW == 0 && GP % NLW == 0 && GPL >= 1 && GPL <= 4, "loader split");
    typedef __attribute__((ext_vector_type(4))) short v4s;
    // G strip in LDS: 16-byte slot s of row r sits at slot s ^ gswz(r), so that the four rows a transposing read touches per quad fall
    // into four different 64-byte bank windows (row pitch 512 / 256 B: rows are bank-aligned, the two low row bits pick the window;
    // pitch 128 B -- the narrow strip -- : odd rows are half a bank cycle further by themselves, row bit 1 picks the other half)
    auto gswz = [](int r) { return SPR >= 16 ? ((r & 3) << 2) : (((r >> 1) & 1) << 2); };
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rbeg = bz * a.rows_per_split;
    const int rend = min(a.M, rbeg + a.rows_per_split);
    const int nstage = (rend - rbeg + WG_SR - 1) / WG_SR;
    const int gcol0 = jt0 * 16;

    if (SC && wave >= NCW) {
        // ------------------------------------------------------------------ loader waves, row-weighted variant (round 3)
        // The G strip (the stored s of the output layer) does NOT go through LDS-DMA here: a loader fetches its pieces into REGISTERS
        // (plain 16-byte loads, three stages ahead, four register sets), multiplies them by the row weight on the way -- one weight per
        // lane and piece: a lane's 16 bytes are 8 features of ONE data row -- and stores them into the stage's buffer (ds_write_b128),
        // one stage ahead of the compute waves.  Round 2 DMA'd the strip and then scaled it IN PLACE in LDS (ds_read, 20 vector
        // instructions, ds_write, behind a wait for the DMA it had just issued around): that read-modify-write sat on the loaders'
        // serial path, which is what a stage took (60 us alone against 31 for the unweighted kernel on the same shape).  Now the
        // multiplies ride in the issue slots the compute waves' MFMAs leave free, nothing is read back from LDS, and a loader waits for
        // nothing younger than two stages.  Same arithmetic as before: dl = bf16(g_r * s), one rounding.
        typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
        // The loaders' stream (8 memory instructions, ~90 vector instructions of weighting, 4 LDS stores per stage) is what a stage waits
        // for, and as the youngest waves of their SIMDs they lose every issue arbitration against the two compute waves beside them
        // (phase stamps: 870 cycles for the weighting): issued first, they are out of the way instead.
        __builtin_amdgcn_s_setprio(3);
        const int lw = wave - NCW;
        const char* zsrc = a.zero + (lane & 31) * 16;
        const int xstride = WG_SR * a.ldX * 2, gstride = WG_DBG(a, 32) ? 0 : WG_SR * a.ldG * 2;
        const char* xbase[XPL]; int xlim[XPL];
#pragma unroll
        for (int i = 0; i < XPL; ++i) {
            const int pc = lw * XPL + i, rl = 2 * pc + (lane >> 5);
            const int col = ((lane & 31) ^ ((rl & 3) << 2)) * 8;                 // source 16-byte chunk of this LDS slot
            xbase[i] = (const char*)a.X + ((size_t)(rbeg + rl) * a.ldX + col) * 2;
            xlim[i] = col < a.ldX ? rend - rbeg - rl : -(1 << 30);
        }
        const char* gbase[GPL]; int glim[GPL];
#pragma unroll
        for (int i = 0; i < GPL; ++i) {
            const int pc = lw * GPL + i, rl = RPP * pc + lane / SPR;
            const int col = gcol0 + ((lane % SPR) ^ gswz(rl)) * 8;
            const bool ok = col < a.ldG;                                          // (a last column block narrower than its strip)
            gbase[i] = (const char*)a.G + ((size_t)(rbeg + rl) * a.ldG + (ok ? col : 0)) * 2;
            glim[i] = ok ? rend - rbeg - rl : -(1 << 30);
        }
        // What a stage costs a CU is the NUMBER of vector-memory wave-instructions, not their bytes (phase stamps of this kernel: 12
        // instructions per loader and stage took 1 430 cycles, ~30 per instruction and CU whatever the width -- the "60-70 GB/s per CU"
        // of DESIGN item 5 is 1 KiB per ~31 cycles).  So the row weights do NOT come by vector loads (4 dword loads per loader and stage
        // = a third of all its instructions for 32 bytes): a loader's G pieces cover NR consecutive data rows, whose weights are ONE
        // scalar load (s_load_dwordx8 through the scalar cache, no vector-memory slot), requested at the top of the iteration that
        // uses them and waited for behind the stage's vector-memory wait.
        constexpr int NR = RPP * GPL;           // data rows of a stage this loader's G pieces cover: rows NR*lw .. NR*lw + NR - 1
        static_assert(NR == 8 || NR == 4, "row weights of a loader and stage are one s_load_dwordx8 / x4");
        typedef __attribute__((ext_vector_type(NR))) float wvec_t;
        auto load_w = [&](int st, wvec_t& w) {
            const uint64_t ad = (uint64_t)(a.rowscale + (rbeg + st * WG_SR + NR * lw));      // (< Mp: the pad rows of gx are finite)
            const uint64_t au = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(ad >> 32)) << 32) |
                                (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)ad);
            if constexpr (NR == 8) asm volatile("s_load_dwordx8 %0, %1, 0x0" : "=s"(w) : "s"(au) : "memory");
            else asm volatile("s_load_dwordx4 %0, %1, 0x0" : "=s"(w) : "s"(au) : "memory");
        };
        auto wsel = [&](const wvec_t& w, int i) {       // the weight of the lane's row in piece i: row RPP * i + lane / SPR of the loader's NR
            float f = w[RPP * i];
#pragma unroll
            for (int r = 1; r < RPP; ++r) f = (lane / SPR == r) ? w[RPP * i + r] : f;
            return f;
        };
        constexpr int PER = GPL + XPL;          // vector-memory operations per loader and stage: GPL strip pieces, XPL DMA pieces
        u32x4 gq0[GPL], gq1[GPL], gq2[GPL], gq3[GPL];
        // rows beyond the split (and the columns beyond the layer) read a valid address and are multiplied by zero in put_piece
        auto issue_g = [&](int st, int i, u32x4& dst) {
            const char* pg = (st * WG_SR < glim[i]) ? gbase[i] + (size_t)st * (size_t)gstride : (const char*)a.G;
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(pg) : "memory");
        };
        auto issue_x = [&](int st, int i) {
            if (WG_DBG(a, 1)) return;
            const char* src = (st * WG_SR < xlim[i]) ? xbase[i] + (size_t)st * (size_t)xstride : zsrc;
            glds16(src, (uint32_t)__builtin_amdgcn_readfirstlane((int)(lds_addr_of(smem + (st % WG_NST) * BUF) + (uint32_t)(lw * XPL + i) * 1024u)));
        };
        auto put_piece = [&](int st, int i, const u32x4& v, const wvec_t& w) {
            const float f = (st * WG_SR < glim[i]) ? (WG_DBG(a, 8) ? 1.0f : wsel(w, i)) : 0.0f;
            *(uint4*)(smem + (st % WG_NST) * BUF + (XP + lw * GPL + i) * 1024 + lane * 16) =
                make_uint4(pack2(bflo(v.x) * f, bfhi(v.x) * f), pack2(bflo(v.y) * f, bfhi(v.y) * f),
                           pack2(bflo(v.z) * f, bfhi(v.z) * f), pack2(bflo(v.w) * f, bfhi(v.w) * f));
        };
        constexpr int XDMA = XPL;
        auto per_stage = [&](int st) { return (st < nstage) ? (WG_DBG(a, 1) ? PER - XDMA : PER) : 0; };
        // prologue: stages 0, 1, 2 requested; stage 0 in its buffer behind the first barrier.  Stage st lives in register set st & 3.
        wvec_t wcur;
        load_w(0, wcur);
        auto issue_all = [&](int st, u32x4 (&gs)[GPL]) {
#pragma unroll
            for (int i = 0; i < GPL; ++i) issue_g(st, i, gs[i]);
#pragma unroll
            for (int i = 0; i < XPL; ++i) issue_x(st, i);
        };
        if (0 < nstage) issue_all(0, gq0);
        if (1 < nstage) issue_all(1, gq1);
        if (2 < nstage) issue_all(2, gq2);
        wait_vmem_but_ws(per_stage(1) + per_stage(2));
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(wcur) : : "memory");
        if (0 < nstage) {
#pragma unroll
            for (int i = 0; i < GPL; ++i) { asm volatile("" : "+v"(gq0[i])); put_piece(0, i, gq0[i], wcur); }
        }
        __syncthreads();
        WS_STAMP(0)      // prologue
        // Iteration c: the buffer stage c - 1 has left is requested again (stage c + 3), then stage c + 1 (requested two iterations ago) is
        // weighted and stored into its buffer.  (Taking the two in turns, one memory instruction then one piece's weighting, was measured
        // and is slower: 53 us alone against 51, the loaders' iteration 3 080 cycles against 2 030 in the stamped build.)
        auto iter = [&](int c, u32x4 (&gn)[GPL], u32x4 (&gc)[GPL]) {      // n: register set of stage c + 3, c: of stage c + 1
            const bool next = c + 1 < nstage;
            if (next) load_w(c + 1, wcur);
            if (c + 3 < nstage) issue_all(c + 3, gn);
            WS_STAMP(1)      // requests of stage c + 3
            if (next) {
                wait_vmem_but_ws(per_stage(c + 2) + per_stage(c + 3));
                asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(wcur) : : "memory");
            }
            WS_STAMP(2)      // wait for stage c + 1
            if (next) {
#pragma unroll
                for (int i = 0; i < GPL; ++i) { asm volatile("" : "+v"(gc[i])); put_piece(c + 1, i, gc[i], wcur); }
            }
            WS_STAMP(3)      // weighting + LDS stores of stage c + 1
            __syncthreads();
            WS_STAMP(4)      // barrier
        };
        for (int c = 0; c < nstage; c += 4) {
            iter(c, gq3, gq1);
            if (c + 1 < nstage) iter(c + 1, gq0, gq2);
            if (c + 2 < nstage) iter(c + 2, gq1, gq3);
            if (c + 3 < nstage) iter(c + 3, gq2, gq0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        WS_STAMP_OUT()
        return;
    }
    if (wave >= NCW) {
        // ------------------------------------------------------------------ loader waves
        const int lw = wave - NCW;
        const char* zsrc = a.zero + (lane & 31) * 16;
        const char* pbase[PPL];
        int plim[PPL];
        const int xstride = WG_SR * a.ldX * 2, gstride = WG_SR * a.ldG * 2;
#pragma unroll
        for (int i = 0; i < PPL; ++i) {
            const bool isx = i < XPL;
            int rl, col, ld;
            if (isx) {
                const int pc = lw * XPL + i;
                rl = 2 * pc + (lane >> 5);
                col = ((lane & 31) ^ ((rl & 3) << 2)) * 8;               // source 16-byte chunk of this LDS slot
                ld = a.ldX;
            } else {
                const int pc = lw * GPL + (i - XPL);
                rl = RPP * pc + lane / SPR;
                col = gcol0 + ((lane % SPR) ^ gswz(rl)) * 8;
                ld = a.ldG;
            }
            pbase[i] = (const char*)(isx ? a.X : a.G) + ((size_t)(rbeg + rl) * ld + col) * 2;
            plim[i] = col < ld ? rend - rbeg - rl : -(1 << 30);
        }
        auto issue = [&](int st) {
#pragma unroll
            for (int i = 0; i < PPL; ++i) {
                const bool isx = i < XPL;
                const int pc = isx ? lw * XPL + i : XP + lw * GPL + (i - XPL);
                const char* src = (st * WG_SR < plim[i]) ? pbase[i] + (size_t)st * (size_t)(isx ? xstride : gstride) : zsrc;
                glds16(src, (uint32_t)__builtin_amdgcn_readfirstlane((int)(lds_addr_of(smem + (st % WG_NST) * BUF) + (uint32_t)pc * 1024u)));
            }
        };
        // prologue: P(0) P(1) P(2); stage 0 landed behind the first barrier
        if (0 < nstage) issue(0);
        if (1 < nstage) issue(1);
        if (2 < nstage) issue(2);
        wait_vmem_but_ws((1 < nstage ? PPL : 0) + (2 < nstage ? PPL : 0));
        __syncthreads();
        // iteration c: the buffer stage c - 1 has left is refilled with stage c + 3; the wait for stage c + 1 leaves P(c+2), P(c+3) in flight
        for (int c = 0; c < nstage; ++c) {
            const bool refill = c + 3 < nstage && !WG_DBG(a, 1);
            if (refill) issue(c + 3);
            if (c + 1 < nstage) wait_vmem_but_ws((c + 2 < nstage ? PPL : 0) + (refill ? PPL : 0));
            __syncthreads();
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        return;
    }

    // ---------------------------------------------------------------------- compute waves
    const int q = lane >> 4, l16 = lane & 15, qp = l16 >> 2, p = l16 & 3;
    const int ig = wave % IGC, jg = wave / IGC;        // the wave's i-tiles ig*7 .. +6, local j-tiles jg*BJ .. +BJ-1
    f32x4 acc[AI][BJ], accb[BJ];
#pragma unroll
    for (int u = 0; u < BJ; ++u) {
        accb[u] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int t = 0; t < AI; ++t) acc[t][u] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    }
    const int xrow_off = (4 * q + qp) * 512, grow_off = (4 * q + qp) * GROW;
    const uint4 ones = make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u);      // bf16 1.0 x 8
    const bool do_bias = ig == 0 && !WG_DBG(a, 4);
    __syncthreads();
    WS_STAMP(0)          // prologue
    for (int c = 0; c < nstage; ++c) {
        const int buf = c % WG_NST;
        const char* xb = smem + buf * BUF + xrow_off + p * 16;
        const char* gbase = smem + buf * BUF + XT_BYTES + grow_off;
        uint4 g[BJ];
#pragma unroll
        for (int u = 0; u < BJ; ++u) {
            const int jl = jg * BJ + u;
            const char* gb = gbase + ((((4 * (jl >> 1)) ^ gswz(qp)) + p) * 16) + 8 * (jl & 1);
            const v4s g0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)gb);
            const v4s g1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(gb + 16 * GROW));
            const uint2 glo = __builtin_bit_cast(uint2, g0), ghi = __builtin_bit_cast(uint2, g1);
            g[u] = make_uint4(glo.x, glo.y, ghi.x, ghi.y);
        }
        WS_STAMP(1)      // G fragments read
        if (!WG_DBG(a, 2)) {
            lds_pipeline<AI, 3>(
                [&](int t) {       // A fragment of i-tile i: P chunk 4*(i>>1)+p (swizzled by the row), half i&1
                    const int i = ig * AI + t;
                    const char* p0 = xb + ((((4 * (i >> 1)) ^ (qp << 2))) * 16) + 8 * (i & 1);
                    const v4s r0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)p0);
                    const v4s r1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(p0 + 16 * 512));
                    const uint2 lo = __builtin_bit_cast(uint2, r0), hi = __builtin_bit_cast(uint2, r1);
                    return make_uint4(lo.x, lo.y, hi.x, hi.y);
                },
                [&](int t, const uint4& av) {
#pragma unroll
                    for (int u = 0; u < BJ; ++u) acc[t][u] = mfma16(av, g[u], acc[t][u]);
                });
        }
        if (do_bias) {      // column sums of G through the matrix pipe: every row of ones x G is sum_r G[r][j] (wave-uniform branch)
#pragma unroll
            for (int u = 0; u < BJ; ++u) accb[u] = mfma16(ones, g[u], accb[u]);
        }
        WS_STAMP(2)      // A fragments + MFMAs issued
        __syncthreads();
        WS_STAMP(3)      // barrier
    }
    if (WG_DBG(a, 16)) return;
    // D: lane(col j = lane&15, quad q) reg ii -> out[i = 16*it + 4q + ii][j]
    float* slab = a.slabW + (size_t)bz * a.IT * 16 * a.JT * 16;
#pragma unroll
    for (int u = 0; u < BJ; ++u) {
        const int jt = jt0 + jg * BJ + u;
        if (jt < a.JT) {
#pragma unroll
            for (int t = 0; t < AI; ++t) {
                const int it = ig * AI + t;
                if (it < a.IT) {
#pragma unroll
                    for (int ii = 0; ii < 4; ++ii)
                        slab[(size_t)(it * 16 + 4 * q + ii) * (a.JT * 16) + jt * 16 + l16] = acc[t][u][ii];
                }
            }
            if (ig == 0 && q == 0) a.slabB[(size_t)bz * a.JT * 16 + jt * 16 + l16] = accb[u][0];
        }
    }
    WS_STAMP(4)          // slab stores issued
    WS_STAMP_OUT()
}

template <bool SC, int BJ, int NLW>
__global__ __launch_bounds__((8 + NLW) * 64, NLW == 8 ? 4 : 3) void wgradws_kernel(WgradPArgs a) {
    int bx = blockIdx.x, bz = blockIdx.z;
    wgradws_block(bx, bz, gridDim.x, gridDim.z);
    const int sid = bz * (int)gridDim.x + bx;
    if constexpr (BJ == 4) {
        // a last column block of <= 64 real out-features (the reference's 784 pixels = 3 x 256 + 64, padded to 832): its workgroups
        // take the 64-wide strip shape -- 4 instead of 16 G pieces per stage, 7 instead of 28 MFMAs per wave -- instead of fetching and
        // multiplying 192 columns of zeros (workgroup-uniform branch)
        // (round 4: the unweighted kernel too, where it is a remainder block of a wider layer: the pre-weighted output layer)
        if (bx == (int)gridDim.x - 1 && a.JT - bx * 16 <= 4 && (SC || gridDim.x > 1)) { wgradws_body<SC, 1, NLW>(a, bx * 16, bz, sid); return; }
    }
    wgradws_body<SC, BJ, NLW>(a, bx * 4 * BJ, bz, sid);
}
// two (or three) of them in one launch: blockIdx.z runs over the concatenated row splits
__global__ __launch_bounds__(768, 3) void wgradws_group_kernel(WgradPGroup g) {
    int l = 0;
    while (l + 1 < g.n && (int)blockIdx.z >= g.zbeg[l + 1]) ++l;
    if ((int)blockIdx.x >= g.gx[l]) return;          // (uniform per workgroup: no barrier is skipped by part of a workgroup)
    int bx = blockIdx.x, bz = blockIdx.z - g.zbeg[l];
    wgradws_block(bx, bz, g.gx[l], g.zbeg[l + 1] - g.zbeg[l]);
    wgradws_body<false, 4, 4>(g.a[l], bx * 16, bz, 0);
}

// Several small weight gradients in ONE launch (the three layers of an encoder block over B rows are ~30-130 blocks
// each and latency-bound): blockIdx.z runs over the concatenated row splits of the layers.
__global__ __launch_bounds__(512, 2) void wgradp_group_kernel(WgradPGroup g) {
    int l = 0;
    while (l + 1 < g.n && (int)blockIdx.z >= g.zbeg[l + 1]) ++l;
    if ((int)blockIdx.x >= g.gx[l] || (int)blockIdx.y >= g.gy[l]) return;
    wgradp_body<8, 4, 4, 4, false>(g.a[l], blockIdx.x, blockIdx.y, blockIdx.z - g.zbeg[l]);
}
// ... with row weights on member 0 (the decoder's three layers at small row counts: the output layer's gradient is g2^T (g_r s))
__global__ __launch_bounds__(512, 2) void wgradp_group_sc_kernel(WgradPGroup g) {
    int l = 0;
    while (l + 1 < g.n && (int)blockIdx.z >= g.zbeg[l + 1]) ++l;
    if ((int)blockIdx.x >= g.gx[l] || (int)blockIdx.y >= g.gy[l]) return;
    if (l == 0) wgradp_body<8, 4, 4, 4, true>(g.a[0], blockIdx.x, blockIdx.y, blockIdx.z);
    else wgradp_body<8, 4, 4, 4, false>(g.a[l], blockIdx.x, blockIdx.y, blockIdx.z - g.zbeg[l]);
}

// ---------------------------------------------------------------------------------
// launch wrappers (plain C++ callers in model.hip; LAUNCH_EV: step_helpers.h)
// ---------------------------------------------------------------------------------
void launch_wgradws_group(const WgradPGroup& g, hipStream_t st) {
    int mx = 0;
    for (int l = 0; l < g.n; ++l) mx = std::max(mx, g.gx[l]);
    hipLaunchKernelGGL(wgradws_group_kernel, dim3(mx, 1, g.zbeg[g.n]), dim3(768), WG_NST * (WG_SR * 512 + WG_SR * 512), st, g);
}
void launch_wgradp_group(const WgradPGroup& g, hipStream_t st) {
    int mx = 0, my = 0;
    for (int l = 0; l < g.n; ++l) { mx = std::max(mx, g.gx[l]); my = std::max(my, g.gy[l]); }
    if (g.a[0].rowscale) hipLaunchKernelGGL(wgradp_group_sc_kernel, dim3(mx, my, g.zbeg[g.n]), dim3(512), WG_NST * (WG_SR * 512 + WG_SR * 256 + 1024), st, g);
    else hipLaunchKernelGGL(wgradp_group_kernel, dim3(mx, my, g.zbeg[g.n]), dim3(512), WG_NST * (WG_SR * 512 + WG_SR * 256), st, g);
}
// shape: 8 = 8 waves / 8 j-tiles per block (small), 16 = 16 waves / 16 j-tiles; specialised waves (IT <= 14): 7 = 8 + 4 waves / 16 j-tiles,
// 9 = 8 + 8 waves / 8 j-tiles
int wgradp_strip(int shape) { return (shape == 8 || shape == 9) ? 8 : 16; }
void launch_wgradp(const WgradPArgs& a, int nsplit, int shape, hipStream_t st, hipEvent_t done) {
    dim3 grid((a.JT + wgradp_strip(shape) - 1) / wgradp_strip(shape), (a.IT + 15) / 16, nsplit);
    const size_t sc = a.rowscale ? 1024 : 0;
    if (shape == 7) {        // specialised waves: 8 compute + 4 loader (needs IT <= 14, one i-block)
        const size_t lds = WG_NST * (WG_SR * 512 + WG_SR * 512);
        if (a.rowscale) LAUNCH_EV(done, (wgradws_kernel<true, 4, 4>), grid, dim3(768), lds, st, a);
        else LAUNCH_EV(done, (wgradws_kernel<false, 4, 4>), grid, dim3(768), lds, st, a);
    } else if (shape == 9) { // specialised waves: 8 compute + 8 loader, 128-feature column blocks
        const size_t lds = WG_NST * (WG_SR * 512 + WG_SR * 256);
        if (a.rowscale) LAUNCH_EV(done, (wgradws_kernel<true, 2, 8>), grid, dim3(1024), lds, st, a);
        else LAUNCH_EV(done, (wgradws_kernel<false, 2, 8>), grid, dim3(1024), lds, st, a);
    } else if (shape == 16) {
        const size_t lds = WG_NST * (WG_SR * 512 + WG_SR * 512 + sc);
        if (a.rowscale) LAUNCH_EV(done, (wgradp_kernel<16, 2, 8, 2, true>), grid, dim3(1024), lds, st, a);
        else LAUNCH_EV(done, (wgradp_kernel<16, 4, 4, 4, false>), grid, dim3(1024), lds, st, a);
    } else {
        const size_t lds = WG_NST * (WG_SR * 512 + WG_SR * 256 + sc);
        if (a.rowscale) LAUNCH_EV(done, (wgradp_kernel<8, 4, 4, 4, true>), grid, dim3(512), lds, st, a);
        else LAUNCH_EV(done, (wgradp_kernel<8, 4, 4, 4, false>), grid, dim3(512), lds, st, a);
    }
}

}  // namespace iwae
