// Launch plan of paged attention: which kernel form a shape takes, with which grid.  Host-only (knobs.h and the standard
// library, nothing else) and pure integer arithmetic over the shape and the knobs, so every threshold is checked on the CPU
// (tests/cpp/attn_plan_check.cc); attention.hip fills AttnArgs from a plan and hands it to the launch function of the kernel
// family (attention_decode.hip, attention_prefill.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "knobs.h"

namespace fh {

constexpr int ATTN_KV_BLOCK = 16;      // = KV_BLOCK (kv_layout.h; attention.hip asserts it)

struct AttnShape {
    int num_seqs, total_q_tokens;
    int max_q_len;                     // ≤ 0: unknown, bounded by total_q_tokens − (num_seqs − 1)
    int max_kv_len, num_heads, num_kv_heads, head_dim;
};

enum AttnKernel : int {
    ATTN_KERNEL_KV_SPLIT,              // paged_attn_kernel: the waves of a workgroup (and grid.z) split the KV range of one row tile
    ATTN_KERNEL_ROW_SPLIT,             // paged_attn_kernel<…, RS>: the waves take consecutive row tiles
    ATTN_KERNEL_FLASH32,               // paged_prefill_attn_kernel (head_dim 64 and 256)
    ATTN_KERNEL_FLASH64,               // paged_prefill_attn64_kernel (head_dim 128)
    ATTN_KERNEL_RESIDENT,              // paged_prefill_attn_resident_kernel (head_dim 128)
};

struct AttnPlan {
    AttnKernel kernel;
    int waves;                         // per workgroup: 4 or 8
    int mt;                            // FLASH32: row tiles per wave (2; 1 at head_dim 256)
    unsigned grid_x, grid_y, grid_z;
    int block;                         // threads per workgroup
    size_t lds_bytes;                  // dynamic LDS
    int nsplit, compact, tiles_per_seq;
    bool reduce;                       // nsplit > 1: paged_attn_reduce_kernel follows on (reduce_grid_x, reduce_grid_y) × reduce_block
    unsigned reduce_grid_x, reduce_grid_y;
    int reduce_block;
    size_t workspace_need;             // bytes of partials the chosen split count wants (before the fallback to one split)
    Form form;                         // counted per launch; FORM_ATTN_SPLIT_REDUCE as well when `reduce`
};

static inline int attn_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

static inline int choose_splits(int num_tiles_total, int nkv, int max_kv_len) {
    // enough workgroups to cover the 256 CUs; at least 4 block pairs (128 keys) per wave per split
    long wgs = (long)num_tiles_total * nkv;
    int pairs = attn_cdiv(attn_cdiv(max_kv_len, ATTN_KV_BLOCK), 2);
    int s = 1;
    // a split costs a second (reduce) launch ≈ 5 µs: only worth it for ≥ 512 keys per split
    while (wgs * s < 256 && pairs / (s * 2) >= 16 && s < 32) s *= 2;
    return s;
}

static inline size_t attn_workspace_bytes(int total_q_tokens, int num_heads, int head_dim) {
    // worst case: every (token, head) row in its own tile slot, 32 splits
    long rows = (long)total_q_tokens * num_heads + 16L * 4096;
    return (size_t)rows * 32 * (head_dim + 2) * sizeof(float);
}

// `varlen`: the caller gave cu_seqlens_q (otherwise token i ↔ sequence i); `fused_qkv`: the decode form with QK-norm + RoPE + KV
// write in its prologue; `workspace_bytes`: room for KV-split partials (0: none).  The shape is valid (the entry points check).
static inline AttnPlan attn_plan(AttnShape sh, const Knobs& kn, bool varlen, bool fused_qkv, size_t workspace_bytes) {
    const int num_seqs = sh.num_seqs, total_q_tokens = sh.total_q_tokens, max_kv_len = sh.max_kv_len;
    const int num_kv_heads = sh.num_kv_heads, head_dim = sh.head_dim;
    const int G = sh.num_heads / num_kv_heads;
    const int max_q_len = sh.max_q_len > 0 ? sh.max_q_len : total_q_tokens - (num_seqs - 1);
    AttnPlan p{};
    p.tiles_per_seq = attn_cdiv((long)max_q_len * G, 16);
    p.grid_y = (unsigned)num_kv_heads;
    p.grid_z = 1;
    p.nsplit = 1;
    p.waves = 4;
    p.block = 256;
    // prefill-like batches (most sequences bring many rows): LDS-shared K/V form.  The token count bounds the work units.
    const bool flash_off = kn.attn_no_flash;
    const long flash_min_rows = kn.attn_flash_min_rows;          // tests lower it
    // … and only when its workgroups (128 rows × one kv head each) cover the chip: a lone 256-token prompt has 64 of them and
    // is faster KV-split over 512 workgroups (TTFT 6.7 vs 7.1 ms)
    const long flash_min_wgs = kn.attn_flash_min_rows_set ? 1 : 256;
    // short prompts whose whole context fits one LDS image (kv ≤ 256 at head_dim 128): resident-K/V form, two workgroups per
    // (sequence, kv head).  max_kv_len bounds every sequence; needs ≥ 4 row tiles per sequence on average to pay off.
    if (!fused_qkv && varlen && head_dim == 128 && !kn.attn_no_resident && max_kv_len <= 256 && max_q_len >= 32 &&
        (long)total_q_tokens * G >= (long)num_seqs * 64 && (long)num_seqs * 2 * num_kv_heads >= kn.attn_resident_min_wgs) {
        p.kernel = ATTN_KERNEL_RESIDENT;
        p.waves = 8;
        p.block = 512;
        p.grid_x = (unsigned)(num_seqs * 2);
        p.lds_bytes = (size_t)2 * (256 / ATTN_KV_BLOCK) * 16 * 128 * 2;       // K + V images: 128 KiB
        p.form = FORM_ATTN_RESIDENT;
        return p;
    }
    if (!fused_qkv && varlen && !flash_off && (long)max_q_len * G >= flash_min_rows &&
        (long)total_q_tokens * 2 >= (long)num_seqs * max_q_len &&
        ((long)total_q_tokens * G / (head_dim == 256 ? 64 : 128)) * num_kv_heads >= flash_min_wgs) {
        const int mt = head_dim == 256 ? 1 : 2, unit_tiles = 4 * mt;
        const long tiles_bound = ((long)total_q_tokens * G) / 16 + num_seqs;
        const long units = attn_cdiv(tiles_bound, (long)unit_tiles) + num_seqs;
        const size_t lds = (size_t)2 * 4 * 16 * head_dim * 2;      // two stages × four tiles
        p.kernel = head_dim == 128 ? ATTN_KERNEL_FLASH64 : ATTN_KERNEL_FLASH32;
        p.mt = mt;
        p.grid_x = (unsigned)units;
        p.lds_bytes = head_dim == 128 ? 2 * lds : lds;             // 64 keys per step: two pairs per stage
        p.form = FORM_ATTN_FLASH;
        return p;
    }
    const int tiles = num_seqs * p.tiles_per_seq;
    int nsplit = choose_splits(tiles, num_kv_heads, max_kv_len);
    if (kn.attn_splits > 0) nsplit = kn.attn_splits;             // tuning override (development)
    p.workspace_need = (size_t)tiles * num_kv_heads * nsplit * 16 * (head_dim + 2) * sizeof(float);
    if (nsplit > 1 && p.workspace_need > workspace_bytes) nsplit = 1;
    p.nsplit = nsplit;
    p.grid_x = (unsigned)tiles;
    p.grid_z = (unsigned)nsplit;
    // prefill (≥ 4 row tiles per sequence, no KV split): the waves of a workgroup take consecutive row tiles
    // (only when that still leaves ≥ 2 workgroups per CU: a single 256-token prompt is faster KV-split, 7.5 vs 7.85 ms TTFT)
    const long rs_min_wgs = kn.attn_rs_min_wgs;                  // tests lower it
    const bool rs = !fused_qkv && nsplit == 1 && p.tiles_per_seq >= 4 &&
                    (long)num_seqs * attn_cdiv(p.tiles_per_seq, 4) * num_kv_heads >= rs_min_wgs && !kn.attn_no_rs;
    if (rs) p.grid_x = (unsigned)(num_seqs * attn_cdiv(p.tiles_per_seq, 4));
    // ragged batch without a KV split: enumerate only the real work units (upper bound from the token count)
    if (varlen && nsplit == 1 && p.tiles_per_seq > 1) {
        const long tiles_bound = ((long)total_q_tokens * G) / 16 + num_seqs;
        const long units = rs ? attn_cdiv(tiles_bound, 4) + num_seqs : tiles_bound;
        if (units < (long)p.grid_x) {
            p.compact = 1;
            p.grid_x = (unsigned)units;
        }
    }
    // decode with ≥ 8 block pairs per split: 8 waves per workgroup (more loads in flight per CU)
    const bool wide = max_q_len == 1 && attn_cdiv(attn_cdiv(max_kv_len, ATTN_KV_BLOCK), 2) / nsplit >= 8 && !kn.attn_narrow;
    // (the fused-qkv form is never row-split; row-split goes before wide, which it can only meet at a GQA group of ≥ 49 heads)
    p.kernel = rs ? ATTN_KERNEL_ROW_SPLIT : ATTN_KERNEL_KV_SPLIT;
    if (wide && !rs) {
        p.waves = 8;
        p.block = 512;
    }
    p.reduce = nsplit > 1;
    if (p.reduce) {
        p.reduce_grid_x = (unsigned)tiles;
        p.reduce_grid_y = (unsigned)num_kv_heads;
        p.reduce_block = 16 * head_dim / 8;
    }
    p.form = fused_qkv ? (wide ? FORM_ATTN_FUSED_QKV_WIDE : FORM_ATTN_FUSED_QKV_NARROW)
                       : rs ? FORM_ATTN_ROW_SPLIT : (wide ? FORM_ATTN_KV_WIDE : FORM_ATTN_KV_NARROW);
    return p;
}

}  // namespace fh
