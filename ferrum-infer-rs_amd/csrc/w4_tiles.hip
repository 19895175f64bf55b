// INT4 GEMMs over 32- to 256-row tiles with the activations staged in LDS: the MoE prefill grouped GEMM (w4_gemm_tile_kernel),
// the dense prefill GEMM (w4_gemm_tilep_kernel) and the scale-folded big tiles (w4_gemm_big_kernel).  Layout and arithmetic: w4_gemm.h.
#include "w4_gemm.h"

namespace fh {

// ── MoE prefill grouped GEMM: 64-row tiles, activations through LDS, 4 waves × 64 columns ──────────────────────
// For blocks of 64 sorted pairs the skinny kernels re-fetch their A fragments from L2 for every 64-column supertile and
// spend half their time on it.  Here a workgroup owns 64 rows × 256 columns: every 128-k group's 64×128 activation tile is
// gathered once (pair rows through sorted_token_ids) into a double-buffered fragment-major LDS tile, each wave streams
// the INT4 group of ITS 64-column supertile straight to registers, expands it once and runs it against all four 16-row
// tiles (80 MFMAs per 4 KiB of weights instead of 20).  MODE 1 plain, 2 gate_up with the fused silu·mul epilogue.  Same
// arithmetic as w4_consume_group (exact integer-valued products, fp32 scale), restructured k-pair-major to hold 250 VGPRs.
// (The dense M ≥ 64 GEMM uses the hand-pipelined w4_gemm_tilep_kernel below.)
// MTN = 16-row tiles per block: 4 (64-pair align blocks, ≥ 32 pairs per expert) or 2 (32-pair blocks: a few hundred
// tokens, e.g. a fresh prompt riding along with the decode batch — half the MFMA padding and the LDS traffic per block).
template <bool HAS_ZP, int MODE, int MTN = 4>
__global__ __launch_bounds__(256, 2) void w4_gemm_tile_kernel(W4Args p) {
    constexpr int ROWS = 16 * MTN;
    static_assert(MODE == 1 || MODE == 2, "grouped-GEMM modes only");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    half8* lds_a = reinterpret_cast<half8*>(lds_raw);          // [2][MTN mt][4 s][64] half8 = 2 × MTN·4 KiB
    constexpr int FR = MTN * 256;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int a = lane >> 4, b = lane & 15;
    // XCD-aware tile order: workgroups are dealt to the 8 XCDs round-robin by launch index; here each XCD walks a contiguous
    // range of (column tile, row block) with the row block fastest, so the row blocks of one expert meet its weight slice in
    // ONE XCD's L2 instead of four
    const int nwg = gridDim.x * gridDim.y, lin = blockIdx.x + gridDim.x * blockIdx.y;
    const int xcd = lin & 7, virt = xcd * (nwg >> 3) + min(xcd, nwg & 7) + (lin >> 3);      // XCD x owns nwg/8 (+1 if x < nwg%8) tiles
    const int st_raw = (virt / (int)gridDim.y) * 4 + wave;
    const bool st_ok = st_raw < p.n64;
    const int st = st_ok ? st_raw : p.n64 - 1;
    const int rb = virt % (int)gridDim.y;

    const uint32_t* qw = p.qw;
    const __half* sc = p.sc;
    const __half* zp = p.zp;
    // rows of this tile: fragment loads are split by wave (k-step s = wave), so every thread needs the 4 rows
    // mt·16 + b of its lane; the epilogue needs rows mt·16 + 4a + r
    int row_in[MTN], row_out_l[MTN];
    {
        // (independent reads, in bounds for every launched row block: requested together — one round trip, not three)
        const int total = *p.total_post_pad;
        const int e = p.block_ids[rb];
        int ids[MTN];
#pragma unroll
        for (int mt = 0; mt < MTN; mt++) ids[mt] = p.sorted_token_ids[rb * ROWS + mt * 16 + b];
        if (rb * ROWS >= total) return;
        qw += (long)e * p.expert_stride_qw;
        sc += (long)e * p.expert_stride_sc;
        if (HAS_ZP) zp += (long)e * p.expert_stride_sc;
#pragma unroll
        for (int mt = 0; mt < MTN; mt++) {
            const int id = ids[mt];
            row_out_l[mt] = id < p.M ? id : -1;
            row_in[mt] = id < p.M ? id / p.top_k : 0;
        }
    }
    const __half* asrc[MTN];
#pragma unroll
    for (int mt = 0; mt < MTN; mt++) asrc[mt] = p.x + (long)row_in[mt] * p.K + 32 * wave + 8 * a;

    const u32x4* qw_lane = reinterpret_cast<const u32x4*>(qw) + ((long)st * p.G * 4) * 64 + lane;
    const uint2* sc_lane = reinterpret_cast<const uint2*>(sc) + ((long)st * p.G) * 16 + b;
    const uint2* zp_lane = HAS_ZP ? reinterpret_cast<const uint2*>(zp) + ((long)st * p.G) * 16 + b : nullptr;

    float4v acc[MTN][4];
#pragma unroll
    for (int mt = 0; mt < MTN; mt++)
#pragma unroll
        for (int nt = 0; nt < 4; nt++) acc[mt][nt] = (float4v){0.f, 0.f, 0.f, 0.f};

    u32x4 wq[2][4];
    uint2 scv[2], zpv[2];
    half8 areg[MTN];
    auto issue_w = [&](int slot, int g) {
#pragma unroll
        for (int nt = 0; nt < 4; nt++) wq[slot][nt] = __builtin_nontemporal_load(qw_lane + ((long)g * 4 + nt) * 64);
        scv[slot] = sc_lane[(long)g * 16];
        if (HAS_ZP) zpv[slot] = zp_lane[(long)g * 16];
    };
    auto issue_a = [&](int g) {
#pragma unroll
        for (int mt = 0; mt < MTN; mt++) areg[mt] = *reinterpret_cast<const half8*>(asrc[mt] + (long)g * 128);
    };
    auto store_a = [&](int buf) {   // fragment (mt, s = wave, lane)
#pragma unroll
        for (int mt = 0; mt < MTN; mt++) lds_a[buf * FR + (mt * 4 + wave) * 64 + lane] = areg[mt];
    };
    // low nibbles land in mantissa bits 0-3 of 0x6400 (1024 + n), high nibbles in bits 4-7 of 0x5400 (64 + n): both
    // expansions are integer-valued, so no operand needs rescaling (the vector issue port is what bounds this kernel)
    const uint32_t magic = opaque_vgpr(0x64006400u), magic_hi = opaque_vgpr(0x54005400u);
    const uint32_t m_lo = opaque_sgpr(0x000F000Fu), m_hi = opaque_sgpr(0x00F000F0u);
    const half8 b_lo = splat_half8(HAS_ZP ? -1024.0f : -1032.0f), b_hi = splat_half8(HAS_ZP ? -64.0f : -72.0f);
    const half8 ones = splat_half8(1.0f);
    auto consume = [&](int slot, int abuf) {
        const half8* at = lds_a + abuf * FR;
        // expand the group once (16 B-operand fragments), then one 16-row tile at a time: 4 offset MFMAs seed the
        // tile's 4 chains, 16 MFMAs extend them, the fp32 scale folds them into acc
        half8 lo[2][4], hi[2][4];
#pragma unroll
        for (int pr = 0; pr < 2; pr++)
#pragma unroll
            for (int nt = 0; nt < 4; nt++) {
                const uint32_t d0 = wq[slot][nt][2 * pr], d1 = wq[slot][nt][2 * pr + 1];
                const uint32_t d0s = d0 >> 8, d1s = d1 >> 8;
                lo[pr][nt] = pack_half8(and_or(d0, m_lo, magic), and_or(d0s, m_lo, magic), and_or(d1, m_lo, magic), and_or(d1s, m_lo, magic));
                hi[pr][nt] = pack_half8(and_or(d0, m_hi, magic_hi), and_or(d0s, m_hi, magic_hi), and_or(d1, m_hi, magic_hi), and_or(d1s, m_hi, magic_hi));
            }
        const unsigned long long sb = ((unsigned long long)scv[slot].y << 32) | scv[slot].x;
        const unsigned long long zb = HAS_ZP ? (((unsigned long long)zpv[slot].y << 32) | zpv[slot].x) : 0ull;
#pragma unroll
        for (int mt = 0; mt < MTN; mt++) {
            half8 af[4];
#pragma unroll
            for (int s = 0; s < 4; s++) af[s] = at[(mt * 4 + s) * 64 + lane];
            float4v t = {0.f, 0.f, 0.f, 0.f}, u = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 4; s++) {
                t = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[s], (s & 1) ? b_hi : b_lo, t, 0, 0, 0);
                if (HAS_ZP) u = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[s], ones, u, 0, 0, 0);
            }
            float4v tmp[4];
#pragma unroll
            for (int nt = 0; nt < 4; nt++) tmp[nt] = t;
#pragma unroll
            for (int pr = 0; pr < 2; pr++) {
#pragma unroll
                for (int nt = 0; nt < 4; nt++) tmp[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[2 * pr], lo[pr][nt], tmp[nt], 0, 0, 0);
#pragma unroll
                for (int nt = 0; nt < 4; nt++) tmp[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[2 * pr + 1], hi[pr][nt], tmp[nt], 0, 0, 0);
            }
#pragma unroll
            for (int nt = 0; nt < 4; nt++) {
                const float s_f = (float)half_at(sb, nt);                  // packed fp32 FMAs: two accumulators per issue slot
                const float4v s4 = {s_f, s_f, s_f, s_f};
                if (HAS_ZP) {
                    const float z_f = (float)half_at(zb, nt);
                    const float4v nz4 = {-z_f, -z_f, -z_f, -z_f};
                    acc[mt][nt] = __builtin_elementwise_fma(s4, __builtin_elementwise_fma(nz4, u, tmp[nt]), acc[mt][nt]);
                } else {
                    acc[mt][nt] = __builtin_elementwise_fma(s4, tmp[nt], acc[mt][nt]);
                }
            }
        }
    };
    const int gz0 = 0, gz1 = p.G;
    {
        const int gl = gz1 - 1;
        issue_w(0, gz0);
        issue_a(gz0);
        FH_PIN();
        store_a(0);
        issue_a(min(gz0 + 1, gl));
        __syncthreads();
        int g = gz0;
        for (; g + 2 <= gz1; g += 2) {              // two groups per trip: static buffer indices, no conditional loads
            issue_w(1, min(g + 1, gl));
            store_a(1);                              // A(g+1), requested one group ago
            issue_a(min(g + 2, gl));
            FH_PIN();
            consume(0, 0);
            FH_PIN();
            __syncthreads();
            issue_w(0, min(g + 2, gl));
            store_a(0);                              // A(g+2)
            issue_a(min(g + 3, gl));
            FH_PIN();
            consume(1, 1);
            FH_PIN();
            __syncthreads();
        }
        if (g < gz1) consume(0, 0);                  // odd group count: the last group is already staged
    }
    if (!st_ok) return;
    // epilogue: D row 4a + r of tile mt ↔ tile row mt·16 + 4a + r, whose routing lives in lane (·, b = 4a + r)
#pragma unroll
    for (int mt = 0; mt < MTN; mt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int orow = __shfl(row_out_l[mt], 4 * a + r, 64);
            if (orow < 0) continue;
            if (MODE == 2) {
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const float gt = acc[mt][j][r], up = acc[mt][2 + j][r];
                    const float v = (gt / (1.0f + __expf(-gt))) * up;
                    const int col = st * 32 + j * 16 + b;
                    if (col < p.ldo) p.out[(long)orow * p.ldo + col] = __float2half(v);
                }
            } else {
#pragma unroll
                for (int nt = 0; nt < 4; nt++) {
                    const int col = st * 64 + nt * 16 + b;
                    if (col < p.N) {
                        float v = acc[mt][nt][r];
                        p.out[(long)orow * p.ldo + col] = __float2half(v);
                    }
                }
            }
        }
}

// ── dense prefill GEMM (M ≥ 64): 64-row tiles, software-pipelined by hand ──────────────────────────────────────────
// Same tile as the MoE kernel above (64 rows × 256 columns per workgroup, activations through a double-buffered
// fragment-major LDS tile, each wave streaming the INT4 group of its own 64-column supertile), but every phase of a wave is
// interleaved with its MFMA stream explicitly instead of running as separate phases (SQ_VALU_MFMA_BUSY_CYCLES of the phased
// kernel: ≈ 45 % of wall):
//   * a quant group is consumed as two k-halves; while the MFMAs of one half run, the OTHER half's B operands are expanded,
//     two VALU behind each MFMA (an MFMA holds the SIMD's vector issue for 8 of its 16 cycles);
//   * one "step" = one 16-row tile × one k-half (2 offset + 8 product MFMAs).  The A fragments of step i+1 are read from LDS
//     during step i; the chain result of step i−1 is folded into the accumulators (fp32 FMA with the group scale) just
//     before step i overwrites the chain registers;
//   * activation staging (global → registers → LDS, one group ahead) and the weight loads (two groups ahead) are issued one
//     instruction per step; every global address is a scalar base + a 32-bit lane offset (no 64-bit address registers —
//     a spill inside this loop costs a vmcnt(0) drain of the prefetches).
// Same arithmetic as w4_consume_group except that the fp32 scale is applied per k-half (two roundings per group instead of
// one).  Measured against the phased kernel (tools/exp_prefill_gemm.py): 4096→28672 at M = 8192 745 → 937 TFLOP/s,
// 4096→6144 at M = 2048 746 → 806, 2048→5120 at M = 2048 636 → 676; M = 64…512 +3…8 %.  A 128-row variant (one wave per
// SIMD, 128 accumulators) was tried and rejected: the fp32 fold needs the accumulators in arch VGPRs, the compiler shuttles
// them through AGPRs (≈ 840 v_accvgpr moves per two groups) and it ran at 264–471 TFLOP/s.  The MoE modes gain nothing
// from this schedule at K = 2048 / 768 (158.6 → 157.1 µs, 101.2 → 103.4 µs at 2048 tokens: padding and the short K bound
// them), so the grouped GEMM keeps the phased kernel.
template <bool HAS_ZP>
__global__ __launch_bounds__(256, 2) void w4_gemm_tilep_kernel(W4Args p) {
    constexpr int MTN = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    half8* lds_a = reinterpret_cast<half8*>(lds_raw);          // [2][MTN mt][4 s][64] half8 = 2 × MTN·4 KiB
    constexpr int FR = MTN * 256, ROWS = MTN * 16;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;   // wave-uniform: scalar bases
    const int a = lane >> 4, b = lane & 15;
    const int st_raw = blockIdx.x * 4 + wave;
    const bool st_ok = st_raw < p.n64;
    const int st = st_ok ? st_raw : p.n64 - 1;
    const int rb = blockIdx.y;

    const uint32_t* qw = p.qw;
    const __half* sc = p.sc;
    const __half* zp = p.zp;
    uint32_t aoff[MTN];                                        // BYTE offset of this thread's staging rows (mt·16 + b): scalar base + 32-bit lane offset
#pragma unroll
    for (int mt = 0; mt < MTN; mt++) {
        const int r = rb * ROWS + mt * 16 + b;
        aoff[mt] = ((uint32_t)(r < p.M ? r : p.M - 1) * (uint32_t)p.K + 32 * wave + 8 * a) * 2u;
    }
    const char* qw_wave = reinterpret_cast<const char*>(qw) + ((long)st * p.G * 4) * 64 * 16;     // scalar
    const char* sc_wave = reinterpret_cast<const char*>(sc) + ((long)st * p.G) * 16 * 8;
    const char* zp_wave = HAS_ZP ? reinterpret_cast<const char*>(zp) + ((long)st * p.G) * 16 * 8 : nullptr;
    const char* x_base = reinterpret_cast<const char*>(p.x);
    const uint32_t lane16 = lane * 16, b8 = b * 8;

    float4v acc[MTN][4];
#pragma unroll
    for (int mt = 0; mt < MTN; mt++)
#pragma unroll
        for (int nt = 0; nt < 4; nt++) acc[mt][nt] = (float4v){0.f, 0.f, 0.f, 0.f};
    u32x4 wq[2][4];                 // raw words, groups of parity 0 / 1
    uint2 scv[2], zpv[2];
    half8 areg[MTN];                  // activation staging
    u32x4 bw[2][4][2];              // expanded B operands [k-half][column tile][lo, hi]
    half8 af[2][2];                  // A fragments of the current / next step
    float4v tmp[4], usum[2];         // chain results: folded into acc just before the next step overwrites them
    float sf[2][4], zf[2][4];

    const uint32_t magic = opaque_vgpr(0x64006400u), magic_hi = opaque_vgpr(0x54005400u);
    const uint32_t m_lo = opaque_sgpr(0x000F000Fu), m_hi = opaque_sgpr(0x00F000F0u);
    const half8 b_lo = splat_half8(HAS_ZP ? -1024.0f : -1032.0f), b_hi = splat_half8(HAS_ZP ? -64.0f : -72.0f);
    const half8 ones = splat_half8(1.0f);
    const float4v zero4 = {0.f, 0.f, 0.f, 0.f};
    auto half_at = [](uint2 v, int i) {
        union { uint16_t u; _Float16 h; } c;
        c.u = (uint16_t)((i < 2 ? v.x : v.y) >> (16 * (i & 1)));
        return c.h;
    };
    const int gz0 = (int)((long)p.G * blockIdx.z / p.S), gz1 = (int)((long)p.G * (blockIdx.z + 1) / p.S);
    const int gl = gz1 - 1;
    auto issue_w = [&](int sl, int nt, int g) __attribute__((always_inline)) {
        wq[sl][nt] = *reinterpret_cast<const u32x4*>(qw_wave + ((uint32_t)g * 4096u + lane16) + nt * 1024);   // scalar base + 32-bit offset
    };
    auto issue_s = [&](int sl, int g) __attribute__((always_inline)) {
        scv[sl] = *reinterpret_cast<const uint2*>(sc_wave + ((uint32_t)g * 128u + b8));
        if (HAS_ZP) zpv[sl] = *reinterpret_cast<const uint2*>(zp_wave + ((uint32_t)g * 128u + b8));
    };
    auto issue_a = [&](int mt, int g) __attribute__((always_inline)) {
        areg[mt] = *reinterpret_cast<const half8*>(x_base + (aoff[mt] + (uint32_t)g * 256u));
    };
    // expansion of column tile nt of k-half pr_t from words (2·pr_t, 2·pr_t + 1) of wq[sl_src][nt]: lo (6 VALU) or hi (6)
    auto expand = [&](int pr_t, int sl_src, int nt, int part, int piece) __attribute__((always_inline)) {
        const uint32_t d0 = wq[sl_src][nt][2 * pr_t], d1 = wq[sl_src][nt][2 * pr_t + 1];
        const uint32_t ml = part == 0 ? m_lo : m_hi, mg = part == 0 ? magic : magic_hi;
        u32x4& dst = bw[pr_t][nt][part];
        if (piece == 0) { dst[0] = and_or(d0, ml, mg); dst[1] = and_or(d0 >> 8, ml, mg); }
        else { dst[2] = and_or(d1, ml, mg); dst[3] = and_or(d1 >> 8, ml, mg); }
    };
    // fold the chain result of the previous step (row tile pm, scales of group parity psl) into the accumulators
    auto fold = [&](int pp, int pm, int psl, int nt) __attribute__((always_inline)) {   // pp: parity of usum
        const float s_f = sf[psl][nt];
        const float4v s4 = {s_f, s_f, s_f, s_f};
        if (HAS_ZP) {
            const float z_f = zf[psl][nt];
            const float4v nz4 = {-z_f, -z_f, -z_f, -z_f};
            acc[pm][nt] = __builtin_elementwise_fma(s4, __builtin_elementwise_fma(nz4, usum[pp], tmp[nt]), acc[pm][nt]);
        } else {
            acc[pm][nt] = __builtin_elementwise_fma(s4, tmp[nt], acc[pm][nt]);
        }
    };
    // one step: row tile mt × k-half pr of group g (register/LDS parity sl)
    auto step = [&](int pr, int mt, int sl, int g) __attribute__((always_inline)) {
        const int cp = mt & 1, np = cp ^ 1;
        const half8* at = lds_a + sl * FR;
        // next step's A fragments (after the group's barrier when they belong to the next group)
        if (pr == 1 && mt == MTN - 1) {
            __syncthreads();
            const half8* atn = lds_a + (sl ^ 1) * FR;
            af[np][0] = atn[lane];
            af[np][1] = atn[64 + lane];
        } else {
            const int nmt = (mt + 1) % MTN, npr = mt == MTN - 1 ? 1 : pr;
            af[np][0] = at[(nmt * 4 + 2 * npr) * 64 + lane];
            af[np][1] = at[(nmt * 4 + 2 * npr + 1) * 64 + lane];
        }
        if (pr == 0) {                       // activations: A(g+1) → LDS, A(g+2) requested
            lds_a[(sl ^ 1) * FR + (mt * 4 + wave) * 64 + lane] = areg[mt];
            issue_a(mt, min(g + 2, gl));
        } else if (mt < 4) {                 // weights of group g+2 into the words this group has consumed
            issue_w(sl, mt, min(g + 2, gl));
        }
        if (pr == 0 && mt == 0) {            // this group's scales; their words are then free for group g+2
#pragma unroll
            for (int nt = 0; nt < 4; nt++) {
                sf[sl][nt] = (float)half_at(scv[sl], nt);
                if (HAS_ZP) zf[sl][nt] = (float)half_at(zpv[sl], nt);
            }
        }
        if (pr == 0 && mt == 1) issue_s(sl, min(g + 2, gl));
        float4v t = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[cp][0], b_lo, zero4, 0, 0, 0);
        FH_PIN();
        t = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[cp][1], b_hi, t, 0, 0, 0);
        FH_PIN();
        if (HAS_ZP) {
            float4v u1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[cp][0], ones, zero4, 0, 0, 0);
            usum[cp] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[cp][1], ones, u1, 0, 0, 0);
            FH_PIN();
        }
        const int pm = (mt + MTN - 1) % MTN, psl = (pr == 0 && mt == 0) ? (sl ^ 1) : sl;
        const int xpr = pr ^ 1, xsl = pr == 0 ? sl : (sl ^ 1);
        constexpr int PPS = 16 / MTN;          // expansion pieces (2 VALU each) per step
#pragma unroll
        for (int nt = 0; nt < 4; nt++) {
            fold(np, pm, psl, nt);
            tmp[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[cp][0], __builtin_bit_cast(half8, bw[pr][nt][0]), t, 0, 0, 0);
            FH_PIN();
        }
#pragma unroll
        for (int nt = 0; nt < 4; nt++) {
            if (nt < PPS) { const int pc = mt * PPS + nt; expand(xpr, xsl, pc >> 2, (pc >> 1) & 1, pc & 1); }
            tmp[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[cp][1], __builtin_bit_cast(half8, bw[pr][nt][1]), tmp[nt], 0, 0, 0);
            FH_PIN();
        }
    };
    auto group = [&](int sl, int g) __attribute__((always_inline)) {
#pragma unroll
        for (int pr = 0; pr < 2; pr++)
#pragma unroll
            for (int mt = 0; mt < MTN; mt++) step(pr, mt, sl, g);
    };
    // prologue: weights of the first two groups, A(gz0) staged, B operands of (gz0, k-half 0), an empty "previous step"
#pragma unroll
    for (int nt = 0; nt < 4; nt++) { issue_w(0, nt, gz0); issue_w(1, nt, min(gz0 + 1, gl)); }
    issue_s(0, gz0);
    issue_s(1, min(gz0 + 1, gl));
#pragma unroll
    for (int mt = 0; mt < MTN; mt++) issue_a(mt, gz0);
#pragma unroll
    for (int mt = 0; mt < MTN; mt++) lds_a[(mt * 4 + wave) * 64 + lane] = areg[mt];
#pragma unroll
    for (int mt = 0; mt < MTN; mt++) issue_a(mt, min(gz0 + 1, gl));
#pragma unroll
    for (int nt = 0; nt < 4; nt++) {
        expand(0, 0, nt, 0, 0); expand(0, 0, nt, 0, 1); expand(0, 0, nt, 1, 0); expand(0, 0, nt, 1, 1);
        tmp[nt] = zero4;
        sf[1][nt] = 0.f;
        zf[1][nt] = 0.f;
    }
    usum[1] = zero4;
    __syncthreads();
    af[0][0] = lds_a[lane];
    af[0][1] = lds_a[64 + lane];
    FH_PIN();
    int g = gz0;
    for (; g + 2 <= gz1; g += 2) {
        group(0, g);
        group(1, g + 1);
    }
    int lsl = 1;
    if (g < gz1) { group(0, g); lsl = 0; }
    // the last step's chain result is still pending
    if (lsl == 0) {
#pragma unroll
        for (int nt = 0; nt < 4; nt++) fold(1, MTN - 1, 0, nt);
    } else {
#pragma unroll
        for (int nt = 0; nt < 4; nt++) fold(1, MTN - 1, 1, nt);
    }
    if (!st_ok) return;
    if (p.partial) {                                 // split-K: fp32 slab, summed by the reduce launch
        float* slab = p.partial + (long)blockIdx.z * p.rows_pad * p.n_pad;
#pragma unroll
        for (int mt = 0; mt < MTN; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = rb * ROWS + mt * 16 + 4 * a + r;
#pragma unroll
                for (int nt = 0; nt < 4; nt++) slab[(long)row * p.n_pad + st * 64 + nt * 16 + b] = acc[mt][nt][r];
            }
        return;
    }
#pragma unroll
    for (int mt = 0; mt < MTN; mt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = rb * ROWS + mt * 16 + 4 * a + r;
            if (row >= p.M) continue;
#pragma unroll
            for (int nt = 0; nt < 4; nt++) {
                const int col = st * 64 + nt * 16 + b;
                if (col < p.N) {
                    float v = acc[mt][nt][r];
                    if (p.bias) v += __half2float(p.bias[col]);
                    p.out[(long)row * p.ldo + col] = __float2half(v);
                }
            }
        }
}

// ── prefill GEMM, 128- or 256-row tiles: group scale and zero folded into the B operand ───────────────────────────────
// The 64-row kernels above are bound by vector issue, not by the matrix pipe: every 4-KiB weight group costs a wave ≈ 80
// VALU of nibble expansion plus one fp32 FMA per accumulator (the per-group scale is applied to a chain result), and the
// offset removal adds 2 MFMAs to every 8 — all of it amortised over only four row tiles.  Here the expanded nibbles are
// finished as fp16 weights in registers — (1024 + q) − (1024 + zero) is an exact fp16 integer (v_pk_add_f16), × the group
// scale is one rounding (v_pk_mul_f16): the fp16 weight the reference's own dequantisation produces — so the MFMAs accumulate
// straight into their final registers: no chain results, no fold, no offset MFMAs, and the MT·16 accumulators of a wave
// can live in AGPRs.  With MT = 8 (128 rows) a group costs a wave ≈ 210 VALU against 128 MFMAs, with MT = 16 against 256:
// the matrix pipe (16 cycles per MFMA, 8 of them holding the issue port) is the bound.  One wave per SIMD; the next
// k-half's operands are expanded between the MFMAs of the current one; activations global → registers → LDS one group ahead,
// weights two groups ahead.
// MODE 0 dense; 1 / 2 the MoE grouped GEMM over MT·16-row align blocks (rows gathered through sorted_token_ids, the block's
// expert from block_ids; 2 = gate_up with the silu·mul epilogue), tiles dealt to the XCDs like w4_gemm_tile_kernel's.
template <int MT, bool HAS_ZP, int MODE = 0>
__global__ __launch_bounds__(256, MT <= 6 ? 2 : 1) void w4_gemm_big_kernel(W4Args p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    half8* lds_a = reinterpret_cast<half8*>(lds_raw);          // [2][MT][4 s][64] half8
    constexpr int FR = MT * 256, ROWS = MT * 16;
    typedef _Float16 half2v_ __attribute__((ext_vector_type(2)));
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int a = lane >> 4, b = lane & 15;
    int ct = blockIdx.x, rb = blockIdx.y;
    if (MODE != 0) {        // each XCD walks a contiguous range of (column tile, row block), row block fastest: one expert's blocks meet its weights in one L2
        const int nwg = gridDim.x * gridDim.y, lin = blockIdx.x + gridDim.x * blockIdx.y;
        const int xcd = lin & 7, virt = xcd * (nwg >> 3) + min(xcd, nwg & 7) + (lin >> 3);
        ct = virt / (int)gridDim.y;
        rb = virt % (int)gridDim.y;
    }
    const int st_raw = ct * 4 + wave;
    const bool st_ok = st_raw < p.n64;
    const int st = st_ok ? st_raw : p.n64 - 1;
    const uint32_t* qw = p.qw;
    const __half* sc = p.sc;
    const __half* zp = p.zp;
    uint32_t aoff[MT];                                          // byte offset of this thread's staging rows: scalar base + 32-bit offset
    int row_out_l[MODE != 0 ? MT : 1];                          // MoE: output row (pair id) of tile row mt·16 + b, −1 = padding
    if (MODE != 0) {
        // the three reads a tile starts with are independent and in bounds for every launched row block (padding blocks hold
        // sentinels): request them together, then decide — one memory round trip instead of three before the first A row
        const int total = *p.total_post_pad;
        const int e = p.block_ids[rb];
        int ids[MT];
#pragma unroll
        for (int mt = 0; mt < MT; mt++) ids[mt] = p.sorted_token_ids[rb * ROWS + mt * 16 + b];
        if (rb * ROWS >= total) return;
        qw += (long)e * p.expert_stride_qw;
        sc += (long)e * p.expert_stride_sc;
        if (HAS_ZP) zp += (long)e * p.expert_stride_sc;
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const int id = ids[mt];
            row_out_l[mt] = id < p.M ? id : -1;
            aoff[mt] = ((uint32_t)(id < p.M ? id / p.top_k : 0) * (uint32_t)p.K + 32 * wave + 8 * a) * 2u;
        }
    } else {
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const int r = rb * ROWS + mt * 16 + b;
            aoff[mt] = ((uint32_t)(r < p.M ? r : p.M - 1) * (uint32_t)p.K + 32 * wave + 8 * a) * 2u;
        }
    }
    // MoE: the valid rows of an align block are a prefix; 16-row tiles that hold only padding are skipped (their MFMAs, not the
    // side work riding behind them): at ≈ 512 pairs per expert 96-row blocks carry ≈ 19 % padding rows, 16-row granularity ≈ 2 %
    int mt_valid = MT;
    if (MODE != 0) {
        mt_valid = 0;
#pragma unroll
        for (int mt = 0; mt < MT; mt++) mt_valid += __ballot(row_out_l[mt] >= 0) != 0 ? 1 : 0;
        mt_valid = __builtin_amdgcn_readfirstlane(mt_valid);
    }
    const char* qw_wave = reinterpret_cast<const char*>(qw) + ((long)st * p.G * 4) * 64 * 16;
    const char* sc_wave = reinterpret_cast<const char*>(sc) + ((long)st * p.G) * 16 * 8;
    const char* zp_wave = HAS_ZP ? reinterpret_cast<const char*>(zp) + ((long)st * p.G) * 16 * 8 : nullptr;
    const char* x_base = reinterpret_cast<const char*>(p.x);
    const uint32_t lane16 = lane * 16, b8 = b * 8;

    float4v acc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < 4; nt++) acc[mt][nt] = (float4v){0.f, 0.f, 0.f, 0.f};
    u32x4 wq[2][4];
    uint2 scv[2], zpv[2];
    half8 areg[MT];
    u32x4 bq[2][4];                                            // finished fp16 B operands [k-step parity][column tile]
    const uint32_t magic = opaque_vgpr(0x64006400u), magic_hi = opaque_vgpr(0x54005400u);
    const uint32_t m_lo = opaque_sgpr(0x000F000Fu), m_hi = opaque_sgpr(0x00F000F0u);
    const int gz0 = (int)((long)p.G * blockIdx.z / p.S), gz1 = (int)((long)p.G * (blockIdx.z + 1) / p.S);
    const int gl = gz1 - 1;
    auto issue_w = [&](int sl, int g) __attribute__((always_inline)) {
#pragma unroll
        for (int nt = 0; nt < 4; nt++)
            wq[sl][nt] = *reinterpret_cast<const u32x4*>(qw_wave + ((uint32_t)g * 4096u + lane16) + nt * 1024);
        scv[sl] = *reinterpret_cast<const uint2*>(sc_wave + ((uint32_t)g * 128u + b8));
        if (HAS_ZP) zpv[sl] = *reinterpret_cast<const uint2*>(zp_wave + ((uint32_t)g * 128u + b8));
    };
    auto issue_a = [&](int mt, int g) __attribute__((always_inline)) {
        areg[mt] = *reinterpret_cast<const half8*>(x_base + (aoff[mt] + (uint32_t)g * 256u));
    };
    auto h2 = [](uint2 v, int i) __attribute__((always_inline)) {   // packed half i of four → both lanes of a half2
        const uint32_t w = i < 2 ? v.x : v.y;
        const uint32_t h = (i & 1) ? (w >> 16) : (w & 0xFFFFu);
        return __builtin_bit_cast(half2v_, h | (h << 16));
    };
    // B operands of column tile nt, k-half pr of the group in slot sl — part 0: the lo nibbles (k-step 2·pr), part 1: the hi
    // nibbles (k-step 2·pr + 1): expand (5 VALU per 8 nibbles), remove the offset (exact), scale (one rounding).  Cut into eight
    // micro-steps of ≤ 2 VALU so that each rides behind one MFMA (an MFMA holds the issue port for 8 of its 16 cycles).
    half2v_ s2v[2][4], zlo[2][4], zhi[2][4];
    const uint32_t off_lo = opaque_vgpr(0xE408E408u), off_hi = opaque_vgpr(0xD480D480u);   // −1032, −72 as half2 in VGPRs (an SGPR operand
                                                                                           // with op_sel costs a wait state before the multiply)
    auto prep_scales = [&](int sl) __attribute__((always_inline)) {
#pragma unroll
        for (int nt = 0; nt < 4; nt++) {
            s2v[sl][nt] = h2(scv[sl], nt);
            if (HAS_ZP) {
                const half2v_ z2 = h2(zpv[sl], nt);
                zlo[sl][nt] = (half2v_){(_Float16)-1024.0f, (_Float16)-1024.0f} - z2;      // exact: integers ≤ 2048
                zhi[sl][nt] = (half2v_){(_Float16)-64.0f, (_Float16)-64.0f} - z2;
            }
        }
    };
    auto micro = [&](int pr, int sl, int nt, int part, int step, uint32_t (&tt)[4]) __attribute__((always_inline)) {
        const uint32_t d0 = wq[sl][nt][2 * pr], d1 = wq[sl][nt][2 * pr + 1];
        const half2v_ s2 = s2v[sl][nt];
        half2v_ off;
        if (HAS_ZP) off = part ? zhi[sl][nt] : zlo[sl][nt];
        else off = __builtin_bit_cast(half2v_, part ? off_hi : off_lo);
        const uint32_t ml = part ? m_hi : m_lo, mg = part ? magic_hi : magic;
        auto addo = [&](uint32_t v) { return __builtin_bit_cast(uint32_t, __builtin_bit_cast(half2v_, v) + off); };
        auto muls = [&](uint32_t v) { return __builtin_bit_cast(uint32_t, __builtin_bit_cast(half2v_, v) * s2); };
        u32x4& dst = bq[part][nt];             // k-step 2·pr + part: parity = part
        switch (step) {
            case 0: tt[0] = and_or(d0, ml, mg); tt[1] = d0 >> 8; break;
            case 1: tt[0] = addo(tt[0]); tt[1] = and_or(tt[1], ml, mg); break;
            case 2: dst[0] = muls(tt[0]); tt[1] = addo(tt[1]); break;
            case 3: dst[1] = muls(tt[1]); tt[2] = and_or(d1, ml, mg); break;
            case 4: tt[2] = addo(tt[2]); tt[3] = d1 >> 8; break;
            case 5: dst[2] = muls(tt[2]); tt[3] = and_or(tt[3], ml, mg); break;
            case 6: tt[3] = addo(tt[3]); break;
            default: dst[3] = muls(tt[3]); break;
        }
    };
    auto finish = [&](int pr, int sl, int nt, int part) __attribute__((always_inline)) {
        uint32_t tt[4];
#pragma unroll
        for (int s = 0; s < 8; s++) micro(pr, sl, nt, part, s, tt);
    };
#define FH_MFMA(ACC, A, B, T) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(ACC) : "v"(A), "v"(B))
    // one k-step (32 k) of one group: MT × 4 MFMAs, in place in AGPRs (hipcc otherwise picks three-address MFMAs whose results
    // drift through the register file and permutes all MT·16 accumulators back at the loop edge: ≈ 90 v_accvgpr moves per group).
    // Dependent MFMAs are MT·4 issue slots apart, B operands were finished one k-step earlier, A fragments come from ds_read.
    // Side work of k-step s: the four operand parts of k-step s + 1 (32 micro-steps spread over the MT·4 MFMAs); k-steps 0 / 1 also
    // move A(g+1) from its staging registers to LDS and request A(g+2).
    uint32_t tt[4];
    half8 af[2];
    // AT = row tiles that hold real rows (MoE: the valid rows of an align block are a prefix; at ≈ 512 pairs per expert 96-row
    // blocks carry ≈ 19 % padding rows — a block whose tail tiles are all padding runs the 2- or 4-tile body instead)
    auto k_step = [&](auto at_c, int ks, int sl, int g) __attribute__((always_inline)) {
        constexpr int AT = decltype(at_c)::value;
        static_assert(AT % 2 == 0 && AT <= MT, "the A-fragment ping-pong returns to slot 0 at every k-step");
        const half8* at = lds_a + sl * FR;
        constexpr int NM = AT * 4;                   // MFMAs per k-step
        const int nks = (ks + 1) & 3, npr = nks >> 1, nsl = ks == 3 ? (sl ^ 1) : sl;     // the k-step whose operands are built now
        if (ks == 0) af[0] = at[lane];               // (the group's barrier has just been passed)
#pragma unroll
        for (int mt = 0; mt < AT; mt++) {
            const int cp = mt & 1;
#pragma unroll
            for (int nt = 0; nt < 4; nt++) {
                const int q = mt * 4 + nt;
                FH_MFMA(acc[mt][nt], af[cp], bq[ks & 1][nt], tt);
                if (nt == 0) {
                    if (mt + 1 < AT) af[cp ^ 1] = at[((mt + 1) * 4 + ks) * 64 + lane];
                    else if (ks < 3) af[cp ^ 1] = at[(ks + 1) * 64 + lane];          // first fragment of the next k-step
                    if (ks < 2) {                    // staging rows mt' = ks·AT/2 … of this k-step's share
                        constexpr int HM = (AT + 1) / 2;
                        const int smt = ks * HM + mt;
                        if (mt < HM && smt < AT) {
                            lds_a[(sl ^ 1) * FR + (smt * 4 + wave) * 64 + lane] = areg[smt];   // A(g+1) → LDS
                            issue_a(smt, min(g + 2, gl));                                      // A(g+2) requested
                        }
                    }
                }
#pragma unroll
                for (int ms = q * 32 / NM; ms < (q + 1) * 32 / NM; ms++)
                    micro(npr, nsl, ms >> 3, nks & 1, ms & 7, tt);      // part ms/8 = column tile, of k-step nks (lo / hi nibbles)
                FH_PIN();
            }
        }
    };
    auto group = [&](auto at_c, int sl, int g) __attribute__((always_inline)) {
        k_step(at_c, 0, sl, g);
        k_step(at_c, 1, sl, g);
        k_step(at_c, 2, sl, g);
        prep_scales(sl ^ 1);
        issue_w(sl, min(g + 2, gl));            // this slot's words are all expanded: group g+2
        FH_PIN();
        k_step(at_c, 3, sl, g);
        __syncthreads();                        // A(g+1) is in LDS; every wave is done with A(g)
    };
    // prologue
    issue_w(0, gz0);
    issue_w(1, min(gz0 + 1, gl));
#pragma unroll
    for (int mt = 0; mt < MT; mt++) issue_a(mt, gz0);
#pragma unroll
    for (int mt = 0; mt < MT; mt++) lds_a[(mt * 4 + wave) * 64 + lane] = areg[mt];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) issue_a(mt, min(gz0 + 1, gl));
    prep_scales(0);
#pragma unroll
    for (int nt = 0; nt < 4; nt++) finish(0, 0, nt, 0);            // operands of k-step 0 of the first group
    __syncthreads();
    FH_PIN();
    auto run = [&](auto at_c) __attribute__((always_inline)) {
        for (int g = gz0; g < gz1; g += 2) {   // an even number of groups per split (the launcher checks)
            group(at_c, 0, g);
            group(at_c, 1, g + 1);
        }
    };
    run(std::integral_constant<int, MT>{});
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");      // the last MFMAs' results before any VALU reads them
    if (!st_ok) return;
    // epilogue: every accumulator leaves its AGPR through an explicit read at its point of use (left to the allocator, all
    // MT·16 of them move to VGPRs at the loop exit and the 256-row form spills 250 registers)
    auto acc_get = [&](int mt, int nt) __attribute__((always_inline)) {
        float4v v;
        asm volatile("v_accvgpr_read_b32 %0, %4\n\tv_accvgpr_read_b32 %1, %5\n\tv_accvgpr_read_b32 %2, %6\n\tv_accvgpr_read_b32 %3, %7"
                     : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3])
                     : "a"(acc[mt][nt][0]), "a"(acc[mt][nt][1]), "a"(acc[mt][nt][2]), "a"(acc[mt][nt][3]));
        return v;
    };
    if (MODE != 0) {        // D row 4a + r of tile mt ↔ block row mt·16 + 4a + r, whose pair id lives in lane (·, b = 4a + r)
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            int orow[4];
#pragma unroll
            for (int r = 0; r < 4; r++) orow[r] = __shfl(row_out_l[mt], 4 * a + r, 64);
            if (MODE == 2) {
#pragma unroll
                for (int jj = 0; jj < 2; jj++) {
                    const float4v gt = acc_get(mt, jj), up = acc_get(mt, 2 + jj);
                    const int col = st * 32 + jj * 16 + b;
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (orow[r] >= 0 && col < p.ldo)
                            p.out[(long)orow[r] * p.ldo + col] = __float2half((gt[r] / (1.0f + __expf(-gt[r]))) * up[r]);
                }
            } else {
#pragma unroll
                for (int nt = 0; nt < 4; nt++) {
                    const float4v v = acc_get(mt, nt);
                    const int col = st * 64 + nt * 16 + b;
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (orow[r] >= 0 && col < p.N) p.out[(long)orow[r] * p.ldo + col] = __float2half(v[r]);
                }
            }
        }
        return;
    }
    if (p.partial) {
        float* slab = p.partial + (long)blockIdx.z * p.rows_pad * p.n_pad + (long)(rb * ROWS + 4 * a) * p.n_pad + st * 64 + b;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int nt = 0; nt < 4; nt++) {
                const float4v v = acc_get(mt, nt);
#pragma unroll
                for (int r = 0; r < 4; r++) slab[(long)(mt * 16 + r) * p.n_pad + nt * 16] = v[r];
            }
        return;
    }
    __half* out_lane = p.out + (long)(rb * ROWS + 4 * a) * p.ldo + st * 64 + b;
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < 4; nt++) {
            const float4v v = acc_get(mt, nt);
            const int col = st * 64 + nt * 16 + b;
            const float bias = (p.bias && col < p.N) ? __half2float(p.bias[col]) : 0.f;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = rb * ROWS + mt * 16 + 4 * a + r;
                if (row < p.M && col < p.N) out_lane[(long)(mt * 16 + r) * p.ldo + nt * 16] = __float2half(v[r] + bias);
            }
        }
}

template <int MT, int MODE>
static int launch_big_t(const W4Args& a, bool has_zp, dim3 grid, hipStream_t stream) {
    const size_t lds = (size_t)2 * MT * 256 * 16;
    with_zp(has_zp, [&](auto zp) { hipLaunchKernelGGL((w4_gemm_big_kernel<MT, decltype(zp)::value, MODE>), grid, dim3(256), lds, stream, a); });
    FH_CHECK_LAUNCH();
    return 0;
}

// dense (mode 0): 96-, 128- or 256-row tiles; grouped (modes 1, 2): 96- or 128-row align blocks
int launch_big(const W4Args& a, int mt, int mode, bool has_zp, dim3 grid, hipStream_t stream) {
    if (mode == 0) {
        if (mt == 6) return launch_big_t<6, 0>(a, has_zp, grid, stream);
        return mt == 16 ? launch_big_t<16, 0>(a, has_zp, grid, stream) : launch_big_t<8, 0>(a, has_zp, grid, stream);
    }
    if (mt == 8) return mode == 2 ? launch_big_t<8, 2>(a, has_zp, grid, stream) : launch_big_t<8, 1>(a, has_zp, grid, stream);
    return mode == 2 ? launch_big_t<6, 2>(a, has_zp, grid, stream) : launch_big_t<6, 1>(a, has_zp, grid, stream);
}

int launch_tilep(const W4Args& a, bool has_zp, dim3 grid, hipStream_t stream) {
    const size_t lds = (size_t)2 * 1024 * 16;
    with_zp(has_zp, [&](auto zp) { hipLaunchKernelGGL((w4_gemm_tilep_kernel<decltype(zp)::value>), grid, dim3(256), lds, stream, a); });
    FH_CHECK_LAUNCH();
    return 0;
}

template <int MODE, int MTN>
static int launch_tile(const W4Args& a, bool has_zp, dim3 grid, hipStream_t stream) {
    const size_t lds = (size_t)2 * MTN * 256 * 16;
    with_zp(has_zp, [&](auto zp) { hipLaunchKernelGGL((w4_gemm_tile_kernel<decltype(zp)::value, MODE, MTN>), grid, dim3(256), lds, stream, a); });
    FH_CHECK_LAUNCH();
    return 0;
}

// Dense projection for ≥ 64 rows as S fp32 slabs through the pipelined tile kernel (S as w4_gemm_dense would pick it); the
// consumer kernel sums the slabs in order, so the reduce launch disappears (short prefills: o_proj → add + norm + route).
int w4_gemm_dense_slabs_tile(const W4Device& w, const __half* x, float* slabs, size_t slab_bytes, int m, int* S_out,
                             int* rows_pad_out, int* n_pad_out, hipStream_t stream) {
    if (m <= 0) return 0;
    FH_REQUIRE(m >= 64 && w.perm == nullptr && w.bias == nullptr, "w4_gemm_dense_slabs_tile: m=%d / act-order / bias use the direct path", m);
    W4Args a = dense_args(w, x, m);
    const int cols = cdiv(w.n64, 4), rts = cdiv(m, 64);
    int S = 1;
    while ((long)cols * rts * S < 256 && w.G / (S * 2) >= 8) S *= 2;
    while (S > 1 && (size_t)S * rts * 64 * w.n64 * 64 * sizeof(float) > slab_bytes) S /= 2;
    if (int rc = slab_output(a, S, rts * 64, slabs, slab_bytes, "w4_gemm_dense_slabs_tile", rows_pad_out, n_pad_out)) return rc;
    *S_out = S;
    form_hit(FORM_W4_SLABS_TILE);
    return launch_tilep(a, w.zp != nullptr, dim3(cols, rts, S), stream);
}

// MoE grouped GEMM over 64-row blocks (moe_align_block_size with block 64): prefill-sized batches, where an expert sees
// tens to hundreds of pairs and the 16-row kernel would re-stream its weights once per 16 pairs.
int w4_gemm_moe_tile(const W4Device& w, const __half* x, __half* out, const int32_t* sorted_token_ids, const int32_t* block_ids,
                     const int32_t* total_post_pad, int num_valid_pairs, int max_blocks, int block_rows, int top_k, int fused_silu,
                     hipStream_t stream) {
    if (num_valid_pairs <= 0 || max_blocks <= 0) return 0;
    FH_REQUIRE(block_rows == 128 || block_rows == 96 || block_rows == 64 || block_rows == 32, "w4_gemm_moe_tile: block_rows=%d (128, 96, 64 or 32)", block_rows);
    FH_REQUIRE(block_rows < 96 || w.G % 2 == 0, "w4_gemm_moe_tile: 96- / 128-row blocks need an even number of quant groups (K=%d)", w.k);
    W4Args a = moe_args(w, x, out, num_valid_pairs, top_k, fused_silu);
    a.sorted_token_ids = sorted_token_ids; a.block_ids = block_ids; a.total_post_pad = total_post_pad;
    dim3 grid(cdiv(w.n64, 4), max_blocks, 1);
    const bool zp = w.zp != nullptr;
    form_hit(block_rows >= 96 ? FORM_MOE_TILE_BIG : (block_rows == 64 ? FORM_MOE_TILE64 : FORM_MOE_TILE32));
    if (block_rows >= 96) return launch_big(a, block_rows / 16, fused_silu ? 2 : 1, zp, grid, stream);
    if (block_rows == 64) return fused_silu ? launch_tile<2, 4>(a, zp, grid, stream) : launch_tile<1, 4>(a, zp, grid, stream);
    return fused_silu ? launch_tile<2, 2>(a, zp, grid, stream) : launch_tile<1, 2>(a, zp, grid, stream);
}

}  // namespace fh
