// Paged-KV prefill attention for gfx950 with K/V staged in LDS: the flash form with 32-key steps (head_dim 64 and 256), the
// flash form with 64-key steps (head_dim 128) and the resident-K/V form for short prompts (head_dim 128, kv ≤ 256).  Three
// kernels with three main loops; what is the same in all of them is a helper below.  Entry points: attention.hip; which form a
// shape takes: attn_plan.h; the forms that read K/V straight from the pool: attention_decode.hip.
#include "attn_common.h"
#include "kv_layout.h"

namespace fh {

// ── what the three forms share: a row tile's masks and Q fragments, the LDS stash of a tile, the transposing epilogue ──────
// One 16-row tile as its wave sees it; lane column b ↔ query row tile·16 + b.
template <int KS>
struct RowTile {
    int row_pos, win_lo;     // this lane's row attends keys [win_lo, row_pos]
    bool row_ok;
    int vis_hi, vis_lo;      // keys in [vis_lo, vis_hi] are visible to EVERY row of the tile (vis_hi = −1: never take the fast path)
    half8 qf[KS];
};

// divmod(rho, t, g): row → (token, head of the GQA group).  Returns the position of the tile's last token.
template <int HD, typename DivMod>
__device__ __forceinline__ int row_tile_setup(const AttnArgs& p, RowTile<HD / 32>& rt, int tile, int rows_total, int tok0, int pos0,
                                              int kvh, int G, int lane, DivMod divmod) {
    const int a = lane >> 4, b = lane & 15;
    const bool full = tile * 16 + 15 < rows_total;
    int t0, t1, g;
    divmod(tile * 16, t0, g);
    divmod(min(tile * 16 + 15, rows_total - 1), t1, g);
    const int tmin = pos0 + t0, tmax = pos0 + t1;     // first / last token position of the tile
    rt.vis_hi = full ? tmin : -1;
    rt.vis_lo = p.sliding_window > 0 ? max(0, tmax + 1 - p.sliding_window) : 0;
    const int rho = tile * 16 + b;
    rt.row_ok = rho < rows_total;
    int t_local;
    divmod(rt.row_ok ? rho : 0, t_local, g);
    rt.row_pos = pos0 + t_local;
    rt.win_lo = p.sliding_window > 0 ? max(0, rt.row_pos + 1 - p.sliding_window) : 0;
    const long q_off = ((long)(tok0 + t_local) * p.nq + kvh * G + g) * HD;
#pragma unroll
    for (int s = 0; s < HD / 32; s++) rt.qf[s] = *reinterpret_cast<const half8*>(p.q + q_off + 32 * s + 8 * a);
    return tmax;
}

// the lane's KS fragments of one tile → LDS, in fragment order (`dst` includes the lane's 16 bytes)
template <int KS>
__device__ __forceinline__ void stash_tile(__half* dst, const half8 (&st)[KS]) {
#pragma unroll
    for (int s = 0; s < KS; s++) *reinterpret_cast<half8*>(dst + s * 512) = st[s];
}
// … of a V tile, interleaved with the other block of its pair so that the PV operand of d-tile 2·ld + sub — the 8-byte half `sub`
// of the lane's fragment of block 0 followed by the same half of block 1 — is ONE conflict-free ds_read_b128: 16-byte slot
// ((sub·KS + ld)·64 + lane) of the pair's V region, block i in its half i (`dst` includes the lane's slot and 8·i bytes)
template <int KS>
__device__ __forceinline__ void stash_v_interleaved(__half* dst, const half8 (&st)[KS]) {
#pragma unroll
    for (int s = 0; s < KS; s++) {
        const uint4 w4 = __builtin_bit_cast(uint4, st[s]);
        *reinterpret_cast<uint2*>(dst + s * 512) = make_uint2(w4.x, w4.y);                 // sub 0
        *reinterpret_cast<uint2*>(dst + (KS + s) * 512) = make_uint2(w4.z, w4.w);          // sub 1
    }
}

// Epilogue of one row tile of the Oᵀ forms: wave-private transposition through `lo` (HD floats per row, 16 rows: the wave's
// share of the now idle stage memory; LDS operations of one wave execute in order), then rows of 64-byte pieces divided by
// the row sums (lane b holds row b's in `l_lane`).
template <int HD>
__device__ __forceinline__ void store_tile_transposed(const AttnArgs& p, float* lo, const float4v (&o_acc)[HD / 16], float l_lane,
                                                      int tile, int rows_total, int tok0, int kvh, int G, int lane) {
    const int a = lane >> 4, b = lane & 15, row = lane >> 2, dl = lane & 3;
    constexpr int DPL = HD / 4;
#pragma unroll
    for (int dt = 0; dt < HD / 16; dt++) *reinterpret_cast<float4v*>(&lo[b * HD + dt * 16 + 4 * a]) = o_acc[dt];
    const float l_row = __shfl(l_lane, row, 64);
    const int rho_o = tile * 16 + row;
    if (rho_o < rows_total) {
        const float inv = l_row > 0.f ? 1.0f / l_row : 0.f;
        __half* o = p.out + ((long)(tok0 + rho_o / G) * p.nq + kvh * G + rho_o % G) * HD + dl * DPL;
#pragma unroll
        for (int i = 0; i < DPL; i += 8) {
            half8 h;
#pragma unroll
            for (int j = 0; j < 8; j++) h[j] = (_Float16)(lo[row * HD + dl * DPL + i + j] * inv);
            *reinterpret_cast<half8*>(o + i) = h;
        }
    }
}

// ── prefill attention with the K/V tiles of a block pair staged ONCE per workgroup in LDS (flash form) ───────────────────
// The forms of attention_decode.hip pull every K/V fragment from L2 once per 16-row tile: at long prompts that is the whole cost (one 8192-token
// prompt: 2.6 ms per layer, ≈ 210 TFLOP/s).  Here a workgroup owns NW·MT = 8 (HD ≤ 128) consecutive row tiles of one sequence
// and one kv head — 128 query rows, i.e. 16 tokens × 8 heads of the GQA group — and walks their common key range pair by pair:
// wave w copies tile w of the pair (K block 0, K block 1, V block 0, V block 1: one 16·HD-element tile each, the same
// fragment-shaped bytes the other forms load) into a double-buffered LDS stage while the previous pair is consumed; every wave
// then reads the fragments with ds_read_b128 and runs them against ITS MT row tiles (the per-row arithmetic is the KV-split
// form's: Sᵀ = K·Qᵀ, lane-local online softmax, Oᵀ += Vᵀ·Pᵀ).  One barrier per pair; L2 traffic per query row ÷ 8.
template <int HD, int MT>
__global__ __launch_bounds__(256, HD <= 128 ? 2 : 1) void paged_prefill_attn_kernel(AttnArgs p) {
    constexpr int NW = 4, DT = HD / 16, KS = HD / 32, TILE = 16 * HD;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __half* lds_kv = reinterpret_cast<__half*>(smem);          // [2 stages][K0, K1, V0, V1][TILE]; reused by the epilogue
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int a = lane >> 4;
    const int kvh = blockIdx.y;
    const int G = p.nq / p.nkv;
    // (sequence, unit of NW·MT row tiles) of this workgroup: scan of cu_seqlens_q, 64 sequences per pass.  Its own copy of
    // attn_find_unit (attn_common.h): through the helper, hipcc allots the head_dim-64 instance 140 registers instead of
    // 128, one workgroup per CU fewer
    int seq = -1, unit = 0;
    {
        const int w = blockIdx.x;
        int base = 0;
        for (int s0 = 0; s0 < p.num_seqs; s0 += 64) {
            const int s = s0 + lane;
            int units = 0;
            if (s < p.num_seqs) {
                const int tiles = ((int)(p.cu_seqlens_q[s + 1] - p.cu_seqlens_q[s]) * G + 15) >> 4;
                units = (tiles + NW * MT - 1) / (NW * MT);
            }
            int incl = units;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int t = __shfl_up(incl, off, 64);
                if (lane >= off) incl += t;
            }
            const int total = __shfl(incl, 63, 64);
            if (w < base + total) {
                const unsigned long long hit = __ballot(w < base + incl);
                const int src = __ffsll((long long)hit) - 1;
                seq = s0 + src;
                unit = w - (base + __shfl(incl - units, src, 64));
                break;
            }
            base += total;
        }
        if (seq < 0) return;                       // whole workgroup (the scan is wave-uniform and identical in every wave)
    }
    const int tok0 = (int)p.cu_seqlens_q[seq];
    const int q_len = (int)p.cu_seqlens_q[seq + 1] - tok0;
    const int rows_total = q_len * G, tiles_s = (rows_total + 15) >> 4;
    const int pos0 = (int)p.pos_offsets[seq];

    const auto divmod_g = [G](int rho, int& t, int& g) { t = rho / G; g = rho % G; };
    RowTile<KS> rt[MT];              // this wave's MT row tiles
#pragma unroll
    for (int mt = 0; mt < MT; mt++) row_tile_setup<HD>(p, rt[mt], (unit * NW + wave) * MT + mt, rows_total, tok0, pos0, kvh, G, lane, divmod_g);
    // key range common to the workgroup's rows
    const int tile_first = unit * NW * MT, tile_last = min(tile_first + NW * MT, tiles_s) - 1;
    const int t_first = (tile_first * 16) / G, t_last = min(q_len - 1, (tile_last * 16 + 15) / G);
    const int kv_end = pos0 + t_last + 1;
    const int kv_begin = p.sliding_window > 0 ? max(0, pos0 + t_first + 1 - p.sliding_window) : 0;
    const int pair_lo = (kv_begin / KV_BLOCK) / 2, pair_hi = (cdiv_dev(kv_end, KV_BLOCK) + 1) / 2;
    const int nblocks = cdiv_dev(kv_end, KV_BLOCK);

    // staging: wave w moves tile w of a pair (0: K block 0, 1: K block 1, 2: V block 0, 3: V block 1)
    const int32_t* bt = p.block_tables + (long)seq * p.max_blocks;
    int bt_lo = 2 * pair_lo;
    int btv = bt[min(bt_lo + lane, p.max_blocks - 1)];
    const __half* pool = wave < 2 ? p.k_pool : p.v_pool;
    half8 st[KS];
    auto issue = [&](int pr) {
        int blk = 2 * pr + (wave & 1);
        if (blk >= nblocks) blk = 2 * pr;                // odd tail: a copy of block 0, masked below
        if (2 * pr + 1 - bt_lo >= 64) {                  // wave-uniform: next chunk of the table
            bt_lo = 2 * pr;
            btv = bt[min(bt_lo + lane, p.max_blocks - 1)];
        }
        const long phys = __builtin_amdgcn_readlane(btv, blk - bt_lo);
        const __half* src = pool + (phys * p.nkv + kvh) * (long)TILE + lane * 8;
#pragma unroll
        for (int s = 0; s < KS; s++) st[s] = *reinterpret_cast<const half8*>(src + s * 512);
    };
    auto stash = [&](int stage) {
        stash_tile<KS>(lds_kv + (stage * 4 + wave) * TILE + lane * 8, st);
    };

    const float sl2 = p.scale * 1.4426950408889634f;
    float m_run[MT], l_run[MT];            // running maximum (log2 units) and sum per row
    float4v o_acc[MT][DT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        m_run[mt] = -INFINITY;
        l_run[mt] = 0.f;
#pragma unroll
        for (int dt = 0; dt < DT; dt++) o_acc[mt][dt] = (float4v){0.f, 0.f, 0.f, 0.f};
    }
    if (pair_lo < pair_hi) {
        issue(pair_lo);
        stash(0);
    }
    __syncthreads();
    for (int pr = pair_lo; pr < pair_hi; pr++) {
        const int cur = (pr - pair_lo) & 1;
        const bool more = pr + 1 < pair_hi;
        if (more) issue(pr + 1);
        __builtin_amdgcn_sched_barrier(0);               // keep the global requests ahead of this pair's work
        const __half* kb = lds_kv + (cur * 4) * TILE + lane * 8;
        const int blk0 = 2 * pr, blk1 = 2 * pr + 1;
        const bool has1 = blk1 < nblocks;
        // Sᵀ[key][row] of both blocks for every row tile; K fragments are read once per k-step
        float4v s0[MT], s1[MT];
#pragma unroll
        for (int mt = 0; mt < MT; mt++) { s0[mt] = (float4v){0.f, 0.f, 0.f, 0.f}; s1[mt] = (float4v){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int s = 0; s < KS; s++) {
            const half8 k0 = *reinterpret_cast<const half8*>(kb + s * 512);
            const half8 k1 = *reinterpret_cast<const half8*>(kb + TILE + s * 512);
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                s0[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(k0, rt[mt].qf[s], s0[mt], 0, 0, 0);
                s1[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(k1, rt[mt].qf[s], s1[mt], 0, 0, 0);
            }
        }
        half8 pf[MT];
        float alpha[MT];
        bool rescale[MT];
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            // probabilities as exp2(s·scale·log₂e − m): one FMA per score feeds the native exp2
            const bool clear = blk1 * KV_BLOCK + KV_BLOCK - 1 <= rt[mt].vis_hi && blk0 * KV_BLOCK >= rt[mt].vis_lo;
            float sc[8];
            float mx = -INFINITY;
            if (clear) {
                // both blocks lie below the causal diagonal (and inside the window) of every row of the tile: no masks
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    sc[r] = s0[mt][r];
                    sc[4 + r] = s1[mt][r];
                    mx = fmaxf(mx, fmaxf(sc[r], sc[4 + r]));
                }
                mx *= sl2;                                   // sl2 > 0: the maximum commutes with the scaling
            } else {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int kp0 = blk0 * KV_BLOCK + 4 * a + r, kp1 = blk1 * KV_BLOCK + 4 * a + r;
                    const bool ok0 = rt[mt].row_ok && kp0 <= rt[mt].row_pos && kp0 >= rt[mt].win_lo;
                    const bool ok1 = rt[mt].row_ok && has1 && kp1 <= rt[mt].row_pos && kp1 >= rt[mt].win_lo;
                    sc[r] = ok0 ? s0[mt][r] : -INFINITY;
                    sc[4 + r] = ok1 ? s1[mt][r] : -INFINITY;
                    mx = fmaxf(mx, fmaxf(sc[r], sc[4 + r]));
                }
                mx *= sl2;
            }
            mx = rows_reduce_max(mx);
            const float m_new = fmaxf(m_run[mt], mx);
            const float m_safe = m_new == -INFINITY ? 0.f : m_new;
            alpha[mt] = __builtin_amdgcn_exp2f(m_run[mt] - m_safe);
            rescale[mt] = __ballot(m_new != m_run[mt]) != 0;     // wave-uniform: some row's maximum moved
            float psum = 0.f;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[j], sl2, -m_safe));      // masked: −inf·sl2 − m = −inf → 0
                psum += pv;
                pf[mt][j] = (_Float16)pv;
            }
            psum = rows_reduce_sum(psum);
            l_run[mt] = l_run[mt] * alpha[mt] + psum;
            m_run[mt] = m_new;
        }
        // Oᵀ[d][row] += Vᵀ[d][key]·Pᵀ[key][row]; V fragments are read once per d-tile pair
        // (the A operand of d-tile 2·ld + sub is the 8-byte half `sub` of the lane's V fragment of block 0 followed by the same
        // half of block 1: two ds_read_b64 straight into the operand registers, no element moves; a missing block 1 has P = 0)
        typedef uint32_t u32x4a __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int ld = 0; ld < KS; ld++) {
#pragma unroll
            for (int sub = 0; sub < 2; sub++) {
                const uint2 v0 = *reinterpret_cast<const uint2*>(kb + 2 * TILE + ld * 512 + 4 * sub);
                const uint2 v1 = *reinterpret_cast<const uint2*>(kb + 3 * TILE + ld * 512 + 4 * sub);
                const half8 vfrag = __builtin_bit_cast(half8, (u32x4a){v0.x, v0.y, v1.x, v1.y});
                const int dt = 2 * ld + sub;
#pragma unroll
                for (int mt = 0; mt < MT; mt++) {
                    if (rescale[mt]) {
#pragma unroll
                        for (int r = 0; r < 4; r++) o_acc[mt][dt][r] *= alpha[mt];
                    }
                    o_acc[mt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vfrag, pf[mt], o_acc[mt][dt], 0, 0, 0);
                }
            }
        }
        if (more) stash(cur ^ 1);
        __syncthreads();
    }
    float* lo = reinterpret_cast<float*>(smem) + wave * 16 * HD;
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
        store_tile_transposed<HD>(p, lo, o_acc[mt], l_run[mt], (unit * NW + wave) * MT + mt, rows_total, tok0, kvh, G, lane);
}

// ── flash form, 64 keys per step ─────────────────────────────────────────────────────────────────────────────────────
// paged_prefill_attn_kernel above pays its softmax bookkeeping (row maximum and its cross-lane reduce, α, the rescale test, the
// row sum and ITS reduce, one barrier) once per 32 keys, and that vector work — not its 32 MFMAs — sets its pace.  Here a step is
// TWO block pairs (64 keys): one maximum / α / rescale per 64 keys, the row sums come out of the matrix pipe (an all-ones A
// operand against Pᵀ: every lane's accumulator then holds Σ_keys P of its query row, rescaled by α like O), and steps whose 64
// keys are visible to every row of a tile (all but the diagonal ones) run a mask-free body.  Same staging, tile layout and
// per-row arithmetic otherwise (Sᵀ = K·Qᵀ, lane-local exp2, Oᵀ += Vᵀ·Pᵀ); l is the sum of the fp16 P the numerator uses.
template <int HD>
__global__ __launch_bounds__(256, 2) void paged_prefill_attn64_kernel(AttnArgs p) {
    constexpr int NW = 4, MT = 2, DT = HD / 16, KS = HD / 32, TILE = 16 * HD;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __half* lds_kv = reinterpret_cast<__half*>(smem);          // [2 stages][2 pairs][K0, K1, V0, V1][TILE]; reused by the epilogue
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int a = lane >> 4;
    const int kvh = blockIdx.y;
    const int G = p.nq / p.nkv;
    int seq, unit;
    // launch order reversed: the longest key ranges (last units of a causal prompt) start first
    attn_find_unit<NW * MT>(p.cu_seqlens_q, p.num_seqs, G, gridDim.x - 1 - blockIdx.x, lane, seq, unit);
    if (seq < 0) return;
    seq = __builtin_amdgcn_readfirstlane(seq);              // wave-uniform by construction: scalar table reads below
    unit = __builtin_amdgcn_readfirstlane(unit);
    const int tok0 = (int)p.cu_seqlens_q[seq];
    const int q_len = (int)p.cu_seqlens_q[seq + 1] - tok0;
    const int rows_total = q_len * G, tiles_s = (rows_total + 15) >> 4;
    const int pos0 = (int)p.pos_offsets[seq];

    const auto divmod_g = [G](int rho, int& t, int& g) { t = rho / G; g = rho % G; };
    RowTile<KS> rt[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) row_tile_setup<HD>(p, rt[mt], (unit * NW + wave) * MT + mt, rows_total, tok0, pos0, kvh, G, lane, divmod_g);
    const int tile_first = unit * NW * MT, tile_last = min(tile_first + NW * MT, tiles_s) - 1;
    const int t_first = (tile_first * 16) / G, t_last = min(q_len - 1, (tile_last * 16 + 15) / G);
    const int kv_end = pos0 + t_last + 1;
    const int kv_begin = p.sliding_window > 0 ? max(0, pos0 + t_first + 1 - p.sliding_window) : 0;
    const int nblocks = cdiv_dev(kv_end, KV_BLOCK);
    const int step_lo = (kv_begin / KV_BLOCK) / 4, step_hi = (nblocks + 3) / 4;       // steps of four blocks

    // staging: wave w moves tile w (0: K block 0, 1: K block 1, 2: V block 0, 3: V block 1) of both pairs of a step.  No load
    // sits under a condition (a conditional load makes hipcc drain vmcnt at the next use of ANY loaded register — here the Q
    // fragments, i.e. a full memory round trip inside every step): the prefetch index is clamped to the last step instead, and
    // the block ids are scalar loads (uniform address: lgkmcnt, not vmcnt).
    const int32_t* bt = p.block_tables + (long)seq * p.max_blocks;
    const __half* pool = wave < 2 ? p.k_pool : p.v_pool;
    half8 st[2][KS];
    int phys_next[2];                                    // physical blocks of the step to be requested next (read one step ahead)
    auto lookup = [&](int sp) {
#pragma unroll
        for (int j = 0; j < 2; j++)
            phys_next[j] = bt[min(4 * sp + 2 * j + (wave & 1), nblocks - 1)];    // past the end: a copy of the last block (finite data), masked below
    };
    auto issue = [&]() {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const __half* src = pool + ((long)phys_next[j] * p.nkv + kvh) * (long)TILE + lane * 8;
#pragma unroll
            for (int s = 0; s < KS; s++) st[j][s] = *reinterpret_cast<const half8*>(src + s * 512);
        }
    };
    // K tiles keep their fragment order; the two V tiles of a pair are interleaved (stash_v_interleaved)
    auto stash = [&](int stage) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            if (wave < 2) stash_tile<KS>(lds_kv + ((stage * 2 + j) * 4 + wave) * TILE + lane * 8, st[j]);
            else stash_v_interleaved<KS>(lds_kv + ((stage * 2 + j) * 4 + 2) * TILE + lane * 8 + (wave & 1) * 4, st[j]);
        }
    };

    const float sl2 = p.scale * 1.4426950408889634f;
    float m_run[MT];
    float4v o_acc[MT][DT], l_acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        m_run[mt] = -INFINITY;
        l_acc[mt] = (float4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dt = 0; dt < DT; dt++) o_acc[mt][dt] = (float4v){0.f, 0.f, 0.f, 0.f};
    }
    const half8 ones = {(_Float16)1.f, (_Float16)1.f, (_Float16)1.f, (_Float16)1.f, (_Float16)1.f, (_Float16)1.f, (_Float16)1.f, (_Float16)1.f};
    if (step_lo < step_hi) {
        lookup(step_lo);
        issue();
        lookup(min(step_lo + 1, step_hi - 1));
        stash(0);
    }
    __syncthreads();
    for (int sp = step_lo; sp < step_hi; sp++) {
        const int cur = (sp - step_lo) & 1;
        issue();                                         // step sp + 1 (clamped), whose block ids arrived during the previous step
        lookup(min(sp + 2, step_hi - 1));
        __builtin_amdgcn_sched_barrier(0);
        const __half* kb = lds_kv + (cur * 8) * TILE + lane * 8;
        // Sᵀ[key][row]: s[mt][2·j + i] = block i of pair j
        float4v sv[MT][4];
        const float4v zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; s++) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const half8 kf = *reinterpret_cast<const half8*>(kb + ((q >> 1) * 4 + (q & 1)) * TILE + s * 512);
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
                    sv[mt][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, rt[mt].qf[s], s == 0 ? zero4 : sv[mt][q], 0, 0, 0);
            }
        }
        half8 pf[MT][2];
        const int key0 = sp * 4 * KV_BLOCK;
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const bool clear = key0 + 4 * KV_BLOCK - 1 <= rt[mt].vis_hi && key0 >= rt[mt].vis_lo;      // wave-uniform
            if (!clear) {
#pragma unroll
                for (int q = 0; q < 4; q++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int kp = key0 + q * KV_BLOCK + 4 * a + r;
                        const bool ok = rt[mt].row_ok && kp <= rt[mt].row_pos && kp >= rt[mt].win_lo;
                        sv[mt][q][r] = ok ? sv[mt][q][r] : -INFINITY;
                    }
            }
            float mx = fmaxf(fmaxf(sv[mt][0][0], sv[mt][0][1]), fmaxf(sv[mt][0][2], sv[mt][0][3]));
#pragma unroll
            for (int q = 1; q < 4; q++) mx = fmaxf(mx, fmaxf(fmaxf(sv[mt][q][0], sv[mt][q][1]), fmaxf(sv[mt][q][2], sv[mt][q][3])));
            mx = rows_reduce_max(mx * sl2);                       // sl2 > 0: the maximum commutes with the scaling
            const float m_new = fmaxf(m_run[mt], mx);
            const float m_safe = m_new == -INFINITY ? 0.f : m_new;
            if (__ballot(m_new != m_run[mt]) != 0) {              // wave-uniform: some row's maximum moved
                const float alpha = __builtin_amdgcn_exp2f(m_run[mt] - m_safe);
#pragma unroll
                for (int dt = 0; dt < DT; dt++)
#pragma unroll
                    for (int r = 0; r < 4; r++) o_acc[mt][dt][r] *= alpha;
#pragma unroll
                for (int r = 0; r < 4; r++) l_acc[mt][r] *= alpha;
                m_run[mt] = m_new;
            }
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        pf[mt][j][4 * i + r] = (_Float16)__builtin_amdgcn_exp2f(__builtin_fmaf(sv[mt][2 * j + i][r], sl2, -m_safe));
        }
        // Oᵀ[d][row] += Vᵀ[d][key]·Pᵀ[key][row]; the row sums ride along as one more "d tile" whose A operand is all ones
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const __half* vb = kb + (j * 4 + 2) * TILE;
#pragma unroll
            for (int mt = 0; mt < MT; mt++) l_acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones, pf[mt][j], l_acc[mt], 0, 0, 0);
#pragma unroll
            for (int ld = 0; ld < KS; ld++) {
#pragma unroll
                for (int sub = 0; sub < 2; sub++) {
                    const half8 vfrag = *reinterpret_cast<const half8*>(vb + (sub * KS + ld) * 512);
                    const int dt = 2 * ld + sub;
#pragma unroll
                    for (int mt = 0; mt < MT; mt++)
                        o_acc[mt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vfrag, pf[mt][j], o_acc[mt][dt], 0, 0, 0);
                }
            }
        }
        stash(cur ^ 1);
        __syncthreads();
    }
    float* lo = reinterpret_cast<float*>(smem) + wave * 16 * HD;
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
        store_tile_transposed<HD>(p, lo, o_acc[mt], l_acc[mt][0], (unit * NW + wave) * MT + mt, rows_total, tok0, kvh, G, lane);
}

// ── short prompts: the sequence's whole K/V resident in LDS ─────────────────────────────────────────────────────────────
// A 256-token prompt is ≤ 4 steps of 64 keys per workgroup of the flash form, most of them on the diagonal: its prologue (unit
// scan, Q, first stage, barrier) and epilogue are most of its time (32 × 256 tokens: 79 µs for 17 GFLOP).  When a sequence's
// keys fit — kv ≤ 256 at head_dim 128: 2 × 64 KiB — ONE copy of its K/V tiles is staged per workgroup (pairs of V tiles
// interleaved as in the 64-key form), one barrier, and then the 8 waves walk the sequence's row tiles two at a time with
// no further synchronisation: wave w of workgroup j ∈ {0, 1} takes tile pairs 2·(w + 8·i) + j … (interleaved, so the causal
// work is balanced).  PV runs with the operands swapped — A = P (the lane's row b, keys (a, j)), B = the V fragment (the very
// registers that serve as A for Oᵀ) — so the result is O[row 4a + r][d = b]: output rows are stored straight from the
// accumulators, no transposition through LDS (there is none left).  Row maxima live in the S layout (lane column b = row); α
// reaches the O layout (row 4a + r) by four lane broadcasts, only when a maximum moved.
template <int HD>
__global__ __launch_bounds__(512, 1) void paged_prefill_attn_resident_kernel(AttnArgs p) {
    constexpr int NW = 8, MT = 2, DT = HD / 16, KS = HD / 32, TILE = 16 * HD, MAXB = 256 / KV_BLOCK;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __half* lds_k = reinterpret_cast<__half*>(smem);            // [MAXB][TILE]
    __half* lds_v = lds_k + MAXB * TILE;                        // [MAXB / 2 pairs][2·TILE], interleaved
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int a = lane >> 4, b = lane & 15;
    const int seq = blockIdx.x >> 1, jpar = blockIdx.x & 1, kvh = blockIdx.y;
    const int G = p.nq / p.nkv;
    // row → (token, head of the group): a shift when the GQA group is a power of two (an emulated integer division costs ≈ 20
    // VALU, and the pass set-up and the row stores do ten of them per pass)
    const int gsh = (G & (G - 1)) == 0 ? __builtin_ctz(G) : -1;
    auto divmod_g = [&](int rho, int& t, int& g) {
        if (gsh >= 0) { t = rho >> gsh; g = rho & (G - 1); }
        else { t = rho / G; g = rho - t * G; }
    };
    const int tok0 = (int)p.cu_seqlens_q[seq];
    const int q_len = (int)p.cu_seqlens_q[seq + 1] - tok0;
    const int rows_total = q_len * G, tiles_s = (rows_total + 15) >> 4;
    const int pos0 = (int)p.pos_offsets[seq];
    const int kv_end = pos0 + q_len;
    const int nblocks = cdiv_dev(kv_end, KV_BLOCK);             // ≤ MAXB (the launcher checks)
    // stage K and V of every block: tile t of the pool → LDS (V: 8-byte halves of a pair's two blocks side by side)
    {
        // (every load of the wave requested before the first LDS write: one memory round trip, not one per tile)
        const int32_t* bt = p.block_tables + (long)seq * p.max_blocks;
        constexpr int NT = 2 * MAXB / NW;                       // tile copies per wave (K and V of MAXB blocks over NW waves)
        long phys[NT];
#pragma unroll
        for (int i = 0; i < NT; i++) phys[i] = bt[min((wave + NW * i) >> 1, nblocks - 1)];
        half8 st[NT][KS];
#pragma unroll
        for (int i = 0; i < NT; i++) {
            const int t = wave + NW * i, isv = t & 1;
            const __half* src = (isv ? p.v_pool : p.k_pool) + (phys[i] * p.nkv + kvh) * (long)TILE + lane * 8;
#pragma unroll
            for (int s = 0; s < KS; s++) st[i][s] = *reinterpret_cast<const half8*>(src + s * 512);
        }
#pragma unroll
        for (int i = 0; i < NT; i++) {
            const int t = wave + NW * i, blk = t >> 1, isv = t & 1;
            if (blk < nblocks) {
                if (!isv) stash_tile<KS>(lds_k + blk * TILE + lane * 8, st[i]);
                else stash_v_interleaved<KS>(lds_v + (blk >> 1) * 2 * TILE + lane * 8 + (blk & 1) * 4, st[i]);
            }
        }
        // a step spans four blocks: V of the blocks between the context's end and the step boundary must read as zeros (their
        // P is 0, but 0 × a stale Inf / NaN is NaN); stale K only yields scores that the masks discard
        for (int blk = nblocks + wave; blk < min(MAXB, (nblocks + 3) & ~3); blk += NW) {
            __half* dst = lds_v + (blk >> 1) * 2 * TILE + lane * 8 + (blk & 1) * 4;
#pragma unroll
            for (int s = 0; s < 2 * KS; s++) *reinterpret_cast<uint2*>(dst + s * 512) = make_uint2(0u, 0u);
        }
    }
    __syncthreads();
    const float sl2 = p.scale * 1.4426950408889634f;
    const half8 ones = {(_Float16)1.f, (_Float16)1.f, (_Float16)1.f, (_Float16)1.f, (_Float16)1.f, (_Float16)1.f, (_Float16)1.f, (_Float16)1.f};
    const float4v zero4 = {0.f, 0.f, 0.f, 0.f};
    // this wave's passes: tile pair index tp = jpar + 2·(wave + NW·i) → tiles 2·tp, 2·tp + 1
    for (int tp = jpar + 2 * wave; 2 * tp < tiles_s; tp += 2 * NW) {
        RowTile<KS> rt[MT];
        int t_last = 0;
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const int tile = 2 * tp + mt;
            const int tmax = row_tile_setup<HD>(p, rt[mt], tile, rows_total, tok0, pos0, kvh, G, lane, divmod_g);
            if (tile * 16 < rows_total) t_last = max(t_last, tmax);
        }
        const int kv_hi = t_last + 1;                                           // keys [0, kv_hi) matter to this pass
        int tw0, gw_;
        divmod_g(2 * tp * 16, tw0, gw_);
        const int kv_lo = p.sliding_window > 0 ? max(0, pos0 + tw0 + 1 - p.sliding_window) : 0;
        const int step_lo = (kv_lo / KV_BLOCK) / 4, step_hi = (cdiv_dev(kv_hi, KV_BLOCK) + 3) / 4;
        float m_run[MT];
        float4v o_acc[MT][DT], l_acc[MT];                                       // O[row 4a + r][d = dt·16 + b], Σ P in the same layout
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            m_run[mt] = -INFINITY;
            l_acc[mt] = zero4;
#pragma unroll
            for (int dt = 0; dt < DT; dt++) o_acc[mt][dt] = zero4;
        }
        for (int sp = step_lo; sp < step_hi; sp++) {
            // (the element offset of the step is made opaque so that the 16 K reads use 16-bit immediates off ONE per-step base;
            // left alone, hipcc keeps a loop-wide base and spends a VALU add per ds_read on offsets beyond 64 KiB)
            int koff = (sp * 4) * TILE + lane * 8;
            asm volatile("" : "+v"(koff));
            const __half* kb = lds_k + koff;
            float4v sv[MT][4];
#pragma unroll
            for (int s = 0; s < KS; s++) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const half8 kf = *reinterpret_cast<const half8*>(kb + q * TILE + s * 512);     // (blocks past the end: stale LDS, masked below)
#pragma unroll
                    for (int mt = 0; mt < MT; mt++)
                        sv[mt][q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, rt[mt].qf[s], s == 0 ? zero4 : sv[mt][q], 0, 0, 0);
                }
            }
            half8 pf[MT][2];
            const int key0 = sp * 4 * KV_BLOCK;
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                const bool clear = key0 + 4 * KV_BLOCK - 1 <= rt[mt].vis_hi && key0 >= rt[mt].vis_lo;      // wave-uniform
                if (!clear) {
#pragma unroll
                    for (int q = 0; q < 4; q++)
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const int kp = key0 + q * KV_BLOCK + 4 * a + r;
                            const bool ok = rt[mt].row_ok && kp <= rt[mt].row_pos && kp >= rt[mt].win_lo;
                            sv[mt][q][r] = ok ? sv[mt][q][r] : -INFINITY;
                        }
                }
                float mx = fmaxf(fmaxf(sv[mt][0][0], sv[mt][0][1]), fmaxf(sv[mt][0][2], sv[mt][0][3]));
#pragma unroll
                for (int q = 1; q < 4; q++) mx = fmaxf(mx, fmaxf(fmaxf(sv[mt][q][0], sv[mt][q][1]), fmaxf(sv[mt][q][2], sv[mt][q][3])));
                mx = rows_reduce_max(mx * sl2);
                const float m_new = fmaxf(m_run[mt], mx);
                const float m_safe = m_new == -INFINITY ? 0.f : m_new;
                if (__ballot(m_new != m_run[mt]) != 0) {                        // wave-uniform: some row's maximum moved
                    const float alpha = __builtin_amdgcn_exp2f(m_run[mt] - m_safe);      // lane column b ↔ row b
                    float al[4];
#pragma unroll
                    for (int r = 0; r < 4; r++) al[r] = __shfl(alpha, 4 * a + r, 64);   // O layout: row 4a + r
#pragma unroll
                    for (int dt = 0; dt < DT; dt++)
#pragma unroll
                        for (int r = 0; r < 4; r++) o_acc[mt][dt][r] *= al[r];
#pragma unroll
                    for (int r = 0; r < 4; r++) l_acc[mt][r] *= al[r];
                    m_run[mt] = m_new;
                }
#pragma unroll
                for (int j = 0; j < 2; j++)
#pragma unroll
                    for (int i = 0; i < 2; i++)
#pragma unroll
                        for (int r = 0; r < 4; r++)
                            pf[mt][j][4 * i + r] = (_Float16)__builtin_amdgcn_exp2f(__builtin_fmaf(sv[mt][2 * j + i][r], sl2, -m_safe));
            }
            // O[row][d] += P[row][key]·V[key][d]: A = P fragment, B = V fragment (operands swapped against the Oᵀ forms)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                int voff = (sp * 2 + j) * 2 * TILE + lane * 8;
                asm volatile("" : "+v"(voff));
                const __half* vb = lds_v + voff;
#pragma unroll
                for (int mt = 0; mt < MT; mt++) l_acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pf[mt][j], ones, l_acc[mt], 0, 0, 0);
#pragma unroll
                for (int ld = 0; ld < KS; ld++)
#pragma unroll
                    for (int sub = 0; sub < 2; sub++) {
                        const half8 vfrag = *reinterpret_cast<const half8*>(vb + (sub * KS + ld) * 512);
                        const int dt = 2 * ld + sub;
#pragma unroll
                        for (int mt = 0; mt < MT; mt++)
                            o_acc[mt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pf[mt][j], vfrag, o_acc[mt][dt], 0, 0, 0);
                    }
            }
        }
        // rows straight from the accumulators: lane (a, b) holds O[row 4a + r][dt·16 + b]
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int rho_o = (2 * tp + mt) * 16 + 4 * a + r;
                if (rho_o < rows_total) {
                    const float l_row = l_acc[mt][r];
                    const float inv = l_row > 0.f ? 1.0f / l_row : 0.f;
                    int to, go;
                    divmod_g(rho_o, to, go);
                    __half* o = p.out + ((long)(tok0 + to) * p.nq + kvh * G + go) * HD + b;
#pragma unroll
                    for (int dt = 0; dt < DT; dt++) o[dt * 16] = __float2half(o_acc[mt][dt][r] * inv);
                }
            }
    }
}

// every form here sizes its LDS at launch: the kernel's dynamic-LDS limit is raised once (it stays with the function)
template <void (*KERNEL)(AttnArgs)>
static int launch_with_lds(const AttnPlan& pl, const AttnArgs& a, hipStream_t s) {
    static bool attr_set = false;
    if (!attr_set) {
        FH_CHECK_HIP(hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes));
        attr_set = true;
    }
    hipLaunchKernelGGL(KERNEL, dim3(pl.grid_x, pl.grid_y, pl.grid_z), dim3(pl.block), pl.lds_bytes, s, a);
    FH_CHECK_LAUNCH();
    return 0;
}

int paged_attn_prefill_launch(const AttnPlan& plan, const AttnArgs& a, int head_dim, hipStream_t s) {
    if (plan.kernel == ATTN_KERNEL_RESIDENT) return launch_with_lds<paged_prefill_attn_resident_kernel<128>>(plan, a, s);
    if (plan.kernel == ATTN_KERNEL_FLASH64) return launch_with_lds<paged_prefill_attn64_kernel<128>>(plan, a, s);
    return head_dim == 64 ? launch_with_lds<paged_prefill_attn_kernel<64, 2>>(plan, a, s)
                          : launch_with_lds<paged_prefill_attn_kernel<256, 1>>(plan, a, s);
}

}  // namespace fh
