// Paged-KV attention for gfx950, the family that reads K/V straight from the pool: one kernel for decode (q_len = 1), chunked
// prefill and mixed batches — KV-split, row-split, fused-qkv decode — and the reduce of its grid.z partials.  Entry points and
// reference ops: attention.hip; which form a shape takes: attn_plan.h; the LDS-staged prefill forms: attention_prefill.hip.
//
// Design (HBM-bound in decode):
//  * a workgroup owns (sequence, kv_head, 16 query rows) where a "row" is a (token, q-head of the
//    GQA group) pair — at decode the 16 rows are the nq/nkv heads of the single new token, so K/V
//    of a kv head are read ONCE for the whole group (the reference's CUDA lane reads them once per
//    q head, kernels/paged_decode_attention.cu:177-179);
//  * K/V tiles are stored MFMA-fragment shaped (kv_layout.h): every wave load is 1 KiB contiguous,
//    goes HBM → VGPR with no LDS staging, and is directly the A operand of v_mfma_f32_16x16x32_f16;
//  * Sᵀ = K·Qᵀ puts one query row per lane column, so softmax statistics are lane-local plus two
//    xor-shuffles; Oᵀ = Vᵀ·Pᵀ keeps the same column ↔ row map, so no cross-lane traffic for the
//    rescale and P feeds the second MFMA straight from the accumulator registers;
//  * the 4 waves of a workgroup split the KV range, and grid.z splits it further for long
//    contexts (flash-decode); partial (m, l, O) are merged in fixed order (deterministic);
//  * prefill (RS, ≥ 4 row tiles per sequence): the waves of a workgroup take 4 CONSECUTIVE row tiles instead and each
//    walks its whole KV range — no cross-wave merge, a loop long enough to amortise the prologue (at 256-token prompts
//    the KV-split form gives a wave 1–2 block pairs), and the four waves request the same K/V lines at about the same
//    time (L1 hits instead of 4× the L2 traffic).
#include "attn_common.h"
#include "kernels.h"
#include "kv_layout.h"
#include "rope_rows.h"

namespace fh {

// FUSED_QKV (decode, q_len = 1): the workgroup of (sequence, kv head) first does what
// split_qkv_norm_rope_into_paged_cache_varlen does for ITS rows of the new token — the G query heads of the
// group, the kv head's key (both per-head RMSNorm + RoPE per qk_mode) and value — into LDS, with the same
// float operations in the same order (bit-identical fp16 results).  The split that owns the last KV block
// writes the new K/V into the paged cache and every wave patches the new token's slot into the fragments it
// loaded from that block, so nothing depends on the visibility of the cache store inside the launch.
template <int HD, bool FUSED_QKV, int NW, bool RS = false>
__global__ __launch_bounds__(NW * 64) void paged_attn_kernel(AttnArgs p) {
    static_assert(!(RS && FUSED_QKV), "row-split is the prefill form");
    constexpr int DT = HD / 16;      // output d-tiles
    constexpr int KS = HD / 32;      // QKᵀ k-steps (= 1-KiB loads per K tile = per V tile)
    constexpr int OSTRIDE = HD + 4;  // padded LDS row (floats)
    __shared__ __attribute__((aligned(16))) float lds_o[NW * 16 * OSTRIDE];
    __shared__ float lds_m[NW * 16], lds_l[NW * 16];

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int a = lane >> 4, b = lane & 15;
    const int kvh = blockIdx.y, z = RS ? 0 : blockIdx.z;
    const int G = p.nq / p.nkv;
    int seq, unit;                   // unit: row tile (KV-split form) or group of NW row tiles (row-split form) in the sequence
    if (p.compact) {
        // ragged batches (31 decode tokens + one 256-token prompt): a grid of num_seqs × max tiles launches thousands of
        // workgroups that only find out they are empty (≈ 15 ns each, 70 µs per layer); here grid.x is an upper bound of
        // the REAL work units and every wave finds its (sequence, unit) by a scan of cu_seqlens_q, 64 sequences per pass
        attn_find_unit<RS ? NW : 1>(p.cu_seqlens_q, p.num_seqs, G, blockIdx.x, lane, seq, unit);
        if (seq < 0) return;
    } else {
        const int tpw = RS ? (p.tiles_per_seq + NW - 1) / NW : p.tiles_per_seq;      // workgroups per sequence
        seq = blockIdx.x / tpw;
        unit = blockIdx.x % tpw;
    }
    const int tok0 = p.cu_seqlens_q ? (int)p.cu_seqlens_q[seq] : seq;
    const int q_len = p.cu_seqlens_q ? (int)p.cu_seqlens_q[seq + 1] - tok0 : 1;
    const int rows_total = q_len * G;
    // a row-split launch still serves its single-tile sequences (the decode tokens of a mixed batch) KV-split: one wave
    // alone would walk the whole context
    const bool rs = RS && rows_total > 16;
    const int tile = rs ? unit * NW + wave : unit;
    if (tile * 16 >= rows_total) return;
    const int pos0 = p.kv_lens ? (int)p.kv_lens[seq] - 1 : (int)p.pos_offsets[seq];

    // this lane's query row (column b of every MFMA)
    const int rho = tile * 16 + b;
    const bool row_ok = rho < rows_total;
    const int t_local = row_ok ? rho / G : 0;
    const int g = row_ok ? rho % G : 0;
    const int row_pos = pos0 + t_local;                 // attends keys [win_lo, row_pos]
    const int win_lo = p.sliding_window > 0 ? max(0, row_pos + 1 - p.sliding_window) : 0;
    const long q_off = ((long)(tok0 + t_local) * p.nq + kvh * G + g) * HD;

    // tile-wide key range
    const int t_first = (tile * 16) / G;
    const int t_last = min(q_len - 1, (tile * 16 + 15) / G);
    const int kv_end = pos0 + t_last + 1;
    const int kv_begin = p.sliding_window > 0 ? max(0, pos0 + t_first + 1 - p.sliding_window) : 0;
    const int pair_lo = (kv_begin / KV_BLOCK) / 2;
    const int pair_hi = (cdiv_dev(kv_end, KV_BLOCK) + 1) / 2;       // exclusive
    const int npairs = pair_hi - pair_lo;
    const int per_split = RS ? npairs : (npairs + p.nsplit - 1) / p.nsplit;      // (a row-split launch has nsplit = 1)
    const int my_lo = pair_lo + z * per_split;
    const int my_hi = min(pair_hi, my_lo + per_split);
    const int STEP = rs ? 1 : NW;                       // row-split: every wave walks the whole range of ITS tile
    const int first = my_lo + (rs ? 0 : wave);
    const int nblocks = cdiv_dev(kv_end, KV_BLOCK);

    // Block-table entries of this split are fetched once (64 per wave, re-fetched every 32 pairs) and the K/V
    // fragments of a wave's NEXT pair are requested before the current pair is consumed, so a wave exposes one
    // memory round trip, not one (table) + one (tiles) per pair.
    const int32_t* bt = p.block_tables + (long)seq * p.max_blocks;
    const long tile_elems = kv_tile_elems(HD);
    int bt_lo = 2 * my_lo;
    int btv = bt[min(bt_lo + lane, p.max_blocks - 1)];
    struct Frags { half8 k0[KS], k1[KS], v0[KS], v1[KS]; };
    auto issue = [&](int pr, Frags& f) {
        const int blk0 = 2 * pr, blk1 = 2 * pr + 1;
        const bool has1 = blk1 < nblocks;
        if (blk1 - bt_lo >= 64) {                        // wave-uniform: next chunk of the table
            bt_lo = blk0;
            btv = bt[min(bt_lo + lane, p.max_blocks - 1)];
        }
        const long phys0 = __builtin_amdgcn_readlane(btv, blk0 - bt_lo);
        const long phys1 = has1 ? __builtin_amdgcn_readlane(btv, blk1 - bt_lo) : phys0;
        const __half* k0 = p.k_pool + (phys0 * p.nkv + kvh) * tile_elems + lane * 8;
        const __half* k1 = p.k_pool + (phys1 * p.nkv + kvh) * tile_elems + lane * 8;
        const __half* v0 = p.v_pool + (phys0 * p.nkv + kvh) * tile_elems + lane * 8;
        const __half* v1 = p.v_pool + (phys1 * p.nkv + kvh) * tile_elems + lane * 8;
#pragma unroll
        for (int s = 0; s < KS; s++) {
            f.k0[s] = __builtin_nontemporal_load(reinterpret_cast<const half8*>(k0 + s * 512));
            f.k1[s] = __builtin_nontemporal_load(reinterpret_cast<const half8*>(k1 + s * 512));
        }
#pragma unroll
        for (int s = 0; s < KS; s++) {
            f.v0[s] = __builtin_nontemporal_load(reinterpret_cast<const half8*>(v0 + s * 512));
            f.v1[s] = __builtin_nontemporal_load(reinterpret_cast<const half8*>(v1 + s * 512));
        }
    };
    Frags cur, nxt;
    if (first < my_hi) issue(first, cur);

    half8 qf[KS];
    __shared__ __attribute__((aligned(16))) __half lds_q[FUSED_QKV ? 16 * HD : 8];
    __shared__ __attribute__((aligned(16))) __half lds_kv[FUSED_QKV ? 2 * HD : 8];
    const int last_blk = pos0 / KV_BLOCK, slot_new = pos0 % KV_BLOCK;
    if (FUSED_QKV) {
        // 16 quarter-wave rows cover the G query heads, the key (row G), the value (row G + 1); rows ≥ G of lds_q are zero
        constexpr int HALF = HD / 2;
        const int q_dim = p.nq * HD, kv_dim = p.nkv * HD;
        const __half* qrow = p.qkv + (long)seq * (q_dim + 2 * kv_dim);
        const int r16 = threadIdx.x >> 4, q16 = threadIdx.x & 15;
        const int rc = r16 < G + 2 ? r16 : G + 1;     // clamped: loads stay unconditional (r16 < 16·NW/4)
        const __half* src = rc < G ? qrow + (kvh * G + rc) * HD
                                   : rc == G ? qrow + q_dim + kvh * HD : qrow + q_dim + kv_dim + kvh * HD;
        const RopeRow<HD> rr = rope_row16<HD>(src, rc < G ? p.q_norm_w : p.k_norm_w, p.cos_t + (long)pos0 * HALF,
                                              p.sin_t + (long)pos0 * HALF, rc <= G ? p.qk_mode : 0, p.qk_mode == 1,
                                              p.qk_mode != 0, p.eps, q16);
        using hv = typename RopeRow<HD>::hv;
        hv z0, z1;
#pragma unroll
        for (int k = 0; k < HD / 32; k++) { z0[k] = (_Float16)0.f; z1[k] = (_Float16)0.f; }
        _Float16* lq = reinterpret_cast<_Float16*>(lds_q) + r16 * HD;
        if (r16 < 16) {
            *reinterpret_cast<hv*>(lq + rr.off0) = r16 < G ? rr.out0 : z0;
            *reinterpret_cast<hv*>(lq + rr.off1) = r16 < G ? rr.out1 : z1;
        }
        if (r16 == G || r16 == G + 1) {
            _Float16* lk = reinterpret_cast<_Float16*>(lds_kv) + (r16 - G) * HD;
            *reinterpret_cast<hv*>(lk + rr.off0) = rr.out0;
            *reinterpret_cast<hv*>(lk + rr.off1) = rr.out1;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < KS; s++) qf[s] = *reinterpret_cast<const half8*>(lds_q + b * HD + 32 * s + 8 * a);
        // the split that owns the last block stores the new token's K (wave 0) and V (wave 1) into the cache
        const int last_pair = last_blk >> 1;
        if (last_pair >= my_lo && last_pair < my_hi && wave < 2) {
            const long phys = p.block_tables[(long)seq * p.max_blocks + last_blk];
            const long toff = (phys * p.nkv + kvh) * kv_tile_elems(HD);
            for (int d = lane; d < HD; d += 64) {
                if (wave == 0) p.k_pool_w[toff + k_tile_off(slot_new, d)] = lds_kv[d];
                else p.v_pool_w[toff + v_tile_off(slot_new, d)] = lds_kv[HD + d];
            }
        }
    } else {
#pragma unroll
        for (int s = 0; s < KS; s++) qf[s] = *reinterpret_cast<const half8*>(p.q + q_off + 32 * s + 8 * a);
    }

    float m_run = -INFINITY, l_run = 0.f;
    float4v o_acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; dt++) o_acc[dt] = (float4v){0.f, 0.f, 0.f, 0.f};


    for (int pr = first; pr < my_hi; pr += STEP) {
        const int blk0 = 2 * pr, blk1 = 2 * pr + 1;
        const bool has1 = blk1 < nblocks;
        if (pr + STEP < my_hi) issue(pr + STEP, nxt);
        __builtin_amdgcn_sched_barrier(0);               // keep the prefetch ahead of this pair's MFMAs
        half8 (&kf0)[KS] = cur.k0, (&kf1)[KS] = cur.k1, (&vf0)[KS] = cur.v0, (&vf1)[KS] = cur.v1;
        if (FUSED_QKV && (blk0 == last_blk || blk1 == last_blk)) {
            // patch the new token's slot (key slot_new of block last_blk) into the loaded fragments
            const bool in1 = blk1 == last_blk;
#pragma unroll
            for (int s = 0; s < KS; s++) {
                const half8 nk = *reinterpret_cast<const half8*>(lds_kv + 32 * s + 8 * a);
                if (b == slot_new) { if (in1) kf1[s] = nk; else kf0[s] = nk; }
            }
            const bool a_hit = a == (slot_new >> 2);
            const int jn = slot_new & 3;
#pragma unroll
            for (int ld = 0; ld < KS; ld++) {
#pragma unroll
                for (int sub = 0; sub < 2; sub++) {
                    const _Float16 nv = (_Float16)lds_kv[HD + 32 * ld + 16 * sub + b];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if (a_hit && j == jn) { if (in1) vf1[ld][4 * sub + j] = nv; else vf0[ld][4 * sub + j] = nv; }
                    }
                }
            }
        }
        // Sᵀ[key][row] for the two blocks: lane (a,b) ← keys 4a+r of each block, query row b
        float4v s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; s++) {
            s0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf0[s], qf[s], s0, 0, 0, 0);
            s1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf1[s], qf[s], s1, 0, 0, 0);
        }
        float sc[8];
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            int kp0 = blk0 * KV_BLOCK + 4 * a + r, kp1 = blk1 * KV_BLOCK + 4 * a + r;
            bool ok0 = row_ok && kp0 <= row_pos && kp0 >= win_lo;
            bool ok1 = row_ok && has1 && kp1 <= row_pos && kp1 >= win_lo;
            sc[r] = ok0 ? s0[r] * p.scale : -INFINITY;
            sc[4 + r] = ok1 ? s1[r] * p.scale : -INFINITY;
            mx = fmaxf(mx, fmaxf(sc[r], sc[4 + r]));
        }
        mx = rows_reduce_max(mx);
        const float m_new = fmaxf(m_run, mx);
        const float m_safe = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = __expf(m_run - m_safe);      // m_run = -inf → 0
        float psum = 0.f;
        half8 pf;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            float pv = __expf(sc[j] - m_safe);            // masked → 0
            psum += pv;
            pf[j] = (_Float16)pv;
        }
        psum = rows_reduce_sum(psum);
        l_run = l_run * alpha + psum;
        m_run = m_new;
        // Oᵀ[d][row] += Vᵀ[d][key]·Pᵀ[key][row]; contraction index (a,j): j<4 block0 key 4a+j, else block1
        typedef uint32_t u32x4a __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int dt = 0; dt < DT; dt++) {
            // 8-byte half `dt & 1` of the lane's V fragment of block 0, then of block 1 (whole dwords: register selection, no
            // element moves); a missing block 1 is a copy of block 0 whose P is 0
            const int ld = dt >> 1, sub = (dt & 1) * 2;
            const u32x4a w0 = __builtin_bit_cast(u32x4a, vf0[ld]), w1 = __builtin_bit_cast(u32x4a, vf1[ld]);
            const half8 vfrag = __builtin_bit_cast(half8, (u32x4a){w0[sub], w0[sub + 1], w1[sub], w1[sub + 1]});
#pragma unroll
            for (int r = 0; r < 4; r++) o_acc[dt][r] *= alpha;
            o_acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vfrag, pf, o_acc[dt], 0, 0, 0);
        }
        cur = nxt;
    }

    if (rs) {
        // wave-private transposition through LDS (Oᵀ[d][row] → rows of 64-byte pieces); LDS ops of one wave execute in order
        float* lo = lds_o + wave * 16 * OSTRIDE;
#pragma unroll
        for (int dt = 0; dt < DT; dt++) *reinterpret_cast<float4v*>(&lo[b * OSTRIDE + dt * 16 + 4 * a]) = o_acc[dt];
        const int row = lane >> 2, dl = lane & 3;
        const float l_row = __shfl(l_run, row, 64);       // lane `row` (a = 0, b = row) holds that row's sum
        const int rho_o = tile * 16 + row;
        if (rho_o >= rows_total) return;
        const float inv = l_row > 0.f ? 1.0f / l_row : 0.f;
        constexpr int DPL = HD / 4;
        __half* o = p.out + ((long)(tok0 + rho_o / G) * p.nq + kvh * G + rho_o % G) * HD + dl * DPL;
#pragma unroll
        for (int i = 0; i < DPL; i += 8) {
            half8 h;
#pragma unroll
            for (int j = 0; j < 8; j++) h[j] = (_Float16)(lo[row * OSTRIDE + dl * DPL + i + j] * inv);
            *reinterpret_cast<half8*>(o + i) = h;
        }
        return;
    }
    // merge the NW waves' partial states through LDS
    if (a == 0) {
        lds_m[wave * 16 + b] = m_run;
        lds_l[wave * 16 + b] = l_run;
    }
#pragma unroll
    for (int dt = 0; dt < DT; dt++)
        *reinterpret_cast<float4v*>(&lds_o[(wave * 16 + b) * OSTRIDE + dt * 16 + 4 * a]) = o_acc[dt];
    __syncthreads();

    // thread → (row = tid / TPR, DPT dims)
    constexpr int TPR = NW * 4;
    const int row = threadIdx.x / TPR, dl = threadIdx.x % TPR;
    float mw[NW], M = -INFINITY;
#pragma unroll
    for (int w = 0; w < NW; w++) { mw[w] = lds_m[w * 16 + row]; M = fmaxf(M, mw[w]); }
    const float Ms = M == -INFINITY ? 0.f : M;
    float fw[NW], L = 0.f;
#pragma unroll
    for (int w = 0; w < NW; w++) { fw[w] = __expf(mw[w] - Ms); L += lds_l[w * 16 + row] * fw[w]; }

    const int rho_o = tile * 16 + row;
    const bool ok_o = rho_o < rows_total;
    const int t_o = ok_o ? rho_o / G : 0, g_o = ok_o ? rho_o % G : 0;
    constexpr int DPT = HD / TPR;    // dims per thread
    float ov[DPT];
#pragma unroll
    for (int i = 0; i < DPT; i++) {
        int d = dl * DPT + i;
        float acc = 0.f;
#pragma unroll
        for (int w = 0; w < NW; w++) acc += lds_o[(w * 16 + row) * OSTRIDE + d] * fw[w];
        ov[i] = acc;
    }
    if (p.nsplit > 1) {
        float* dst = p.partial + (((long)blockIdx.x * p.nkv + kvh) * p.nsplit + z) * 16 * (HD + 2) + row * (HD + 2);
#pragma unroll
        for (int i = 0; i < DPT; i++) dst[dl * DPT + i] = ov[i];
        if (dl == 0) { dst[HD] = M; dst[HD + 1] = L; }
        return;
    }
    if (!ok_o) return;
    const float inv = L > 0.f ? 1.0f / L : 0.f;
    if (p.out_scatter) {
        __half* orow = p.out + (long)(tok0 + t_o) * p.nq * HD;
        const int32_t* sc = p.out_scatter + (kvh * G + g_o) * HD + dl * DPT;
#pragma unroll
        for (int i = 0; i < DPT; i++) orow[sc[i]] = __float2half(ov[i] * inv);
        return;
    }
    __half* o = p.out + ((long)(tok0 + t_o) * p.nq + kvh * G + g_o) * HD + dl * DPT;
#pragma unroll
    for (int i = 0; i < DPT; i++) o[i] = __float2half(ov[i] * inv);
}

// merge grid.z partials: one thread per (row, dim)
template <int HD>
__global__ void paged_attn_reduce_kernel(AttnArgs p) {
    const int seq = blockIdx.x / p.tiles_per_seq, tile = blockIdx.x % p.tiles_per_seq;
    const int kvh = blockIdx.y;
    const int G = p.nq / p.nkv;
    const int tok0 = p.cu_seqlens_q ? (int)p.cu_seqlens_q[seq] : seq;
    const int q_len = p.cu_seqlens_q ? (int)p.cu_seqlens_q[seq + 1] - tok0 : 1;
    const int rows_total = q_len * G;
    const int row = threadIdx.x / (HD / 8), dl = threadIdx.x % (HD / 8);
    const int rho = tile * 16 + row;
    if (rho >= rows_total) return;
    const float* base = p.partial + ((long)blockIdx.x * p.nkv + kvh) * p.nsplit * 16 * (HD + 2) + row * (HD + 2);
    float M = -INFINITY;
    for (int z = 0; z < p.nsplit; z++) M = fmaxf(M, base[(long)z * 16 * (HD + 2) + HD]);
    const float Ms = M == -INFINITY ? 0.f : M;
    float L = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int z = 0; z < p.nsplit; z++) {
        const float* src = base + (long)z * 16 * (HD + 2);
        float f = __expf(src[HD] - Ms);
        L += src[HD + 1] * f;
#pragma unroll
        for (int i = 0; i < 8; i++) acc[i] += src[dl * 8 + i] * f;
    }
    const float inv = L > 0.f ? 1.0f / L : 0.f;
    const int t_o = rho / G, g_o = rho % G;
    if (p.out_scatter) {
        __half* orow = p.out + (long)(tok0 + t_o) * p.nq * HD;
        const int32_t* sc = p.out_scatter + (kvh * G + g_o) * HD + dl * 8;
#pragma unroll
        for (int i = 0; i < 8; i++) orow[sc[i]] = __float2half(acc[i] * inv);
        return;
    }
    __half* o = p.out + ((long)(tok0 + t_o) * p.nq + kvh * G + g_o) * HD + dl * 8;
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = __float2half(acc[i] * inv);
}

template <int HD>
static int launch_hd(const AttnPlan& pl, const AttnArgs& a, bool fused_qkv, hipStream_t s) {
    const dim3 grid(pl.grid_x, pl.grid_y, pl.grid_z), block(pl.block);
    const bool wide = pl.waves == 8;
    if (fused_qkv && wide) hipLaunchKernelGGL((paged_attn_kernel<HD, true, 8>), grid, block, 0, s, a);
    else if (fused_qkv) hipLaunchKernelGGL((paged_attn_kernel<HD, true, 4>), grid, block, 0, s, a);
    else if (pl.kernel == ATTN_KERNEL_ROW_SPLIT) hipLaunchKernelGGL((paged_attn_kernel<HD, false, 4, true>), grid, block, 0, s, a);
    else if (wide) hipLaunchKernelGGL((paged_attn_kernel<HD, false, 8>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((paged_attn_kernel<HD, false, 4>), grid, block, 0, s, a);
    FH_CHECK_LAUNCH();
    if (pl.reduce) {
        hipLaunchKernelGGL(paged_attn_reduce_kernel<HD>, dim3(pl.reduce_grid_x, pl.reduce_grid_y), dim3(pl.reduce_block), 0, s, a);
        FH_CHECK_LAUNCH();
    }
    return 0;
}

int paged_attn_decode_launch(const AttnPlan& plan, const AttnArgs& a, int head_dim, bool fused_qkv, hipStream_t s) {
    return head_dim == 128 ? launch_hd<128>(plan, a, fused_qkv, s)
                           : head_dim == 64 ? launch_hd<64>(plan, a, fused_qkv, s) : launch_hd<256>(plan, a, fused_qkv, s);
}

}  // namespace fh
