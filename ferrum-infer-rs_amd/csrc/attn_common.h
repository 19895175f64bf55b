// What the two paged-attention kernel families (attention_decode.hip, attention_prefill.hip) and their dispatcher
// (attention.hip) share: the kernel argument block, the launch functions, and the work-unit lookup of a ragged batch.
#pragma once
#include "attn_plan.h"
#include "common.h"

namespace fh {

struct AttnArgs {
    const __half* q;        // [total_q, nq, hd]
    const __half* k_pool;   // [blocks, nkv, tile]
    const __half* v_pool;
    __half* out;            // [total_q, nq, hd]
    const uint32_t* cu_seqlens_q;   // [num_seqs+1] or null (decode: token i ↔ seq i)
    const uint32_t* pos_offsets;    // [num_seqs] kv position of each seq's first q token
    const uint32_t* kv_lens;        // decode form: [num_seqs] kv length incl. the new token (pos = len-1)
    const int32_t* block_tables;    // [num_seqs, max_blocks]
    float* partial;         // [tiles][nsplit][16][hd+2] when nsplit > 1
    int num_seqs, nq, nkv, tiles_per_seq, max_blocks, sliding_window, nsplit;
    int compact;            // grid.x enumerates real work units of a ragged batch (see the kernel), not num_seqs × tiles_per_seq
    float scale;
    // fused decode form (FUSED_QKV): q / new K / new V come straight from the qkv projection output
    const __half* qkv;      // [num_seqs, (nq + 2·nkv)·hd]
    const __half* q_norm_w;
    const __half* k_norm_w;
    const float* cos_t;
    const float* sin_t;
    __half* k_pool_w;
    __half* v_pool_w;
    float eps;
    int qk_mode;
    // decode forms: the consumer is an act-order o_proj — channel c of a row is stored at out_scatter[c] (inverse of the
    // projection's row permutation), so no gather launch sits between attention and the GEMM
    const int32_t* out_scatter;
};

// Launch what the plan names (attn_plan.h) on `a`; the decode family's launch adds the reduce launch of a KV-split plan.
int paged_attn_decode_launch(const AttnPlan& plan, const AttnArgs& a, int head_dim, bool fused_qkv, hipStream_t s);
int paged_attn_prefill_launch(const AttnPlan& plan, const AttnArgs& a, int head_dim, hipStream_t s);

// (sequence, unit) of work unit `w` of a ragged batch, where a unit is UNIT_TILES consecutive 16-row tiles of a sequence: every wave
// scans cu_seqlens_q, 64 sequences per pass (wave-uniform, and identical in every wave of a workgroup).  seq = −1: `w` lies
// past the last unit (grid.x is an upper bound of the real units).
template <int UNIT_TILES>
__device__ __forceinline__ void attn_find_unit(const uint32_t* cu_seqlens_q, int num_seqs, int G, int w, int lane, int& seq, int& unit) {
    int base = 0;
    seq = -1;
    unit = 0;
    for (int s0 = 0; s0 < num_seqs; s0 += 64) {
        const int s = s0 + lane;
        int units = 0;
        if (s < num_seqs) {
            const int tiles = ((int)(cu_seqlens_q[s + 1] - cu_seqlens_q[s]) * G + 15) >> 4;
            units = (tiles + UNIT_TILES - 1) / UNIT_TILES;
        }
        int incl = units;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        const int total = __shfl(incl, 63, 64);
        if (w < base + total) {
            const unsigned long long hit = __ballot(w < base + incl);      // first lane whose inclusive sum passes w
            const int src = __ffsll((long long)hit) - 1;
            seq = s0 + src;
            unit = w - (base + __shfl(incl - units, src, 64));
            break;
        }
        base += total;
    }
}

}  // namespace fh
