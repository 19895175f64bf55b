// Development knobs and kernel-form accounting (knobs.cc; host-only, no HIP header).
//
// Knobs: every FERRUM_HIP_* tuning variable a launcher consults is read ONCE (library load) into this struct —
// no getenv on a launch path.  Tests that steer a kernel form set the variable and call
// ferrum_hip_debug_reload_knobs(); product code never does.
//
// Forms: each launcher records which kernel form it chose (one relaxed atomic add at enqueue time), so a test
// that names a form can assert that this form — not a neighbour picked by a drifted heuristic — produced the
// result it checked (ferrum_hip_debug_form_hits).  A hipGraph replay does not re-count its captured launches;
// FORM_GRAPH_REPLAY counts replays.
#pragma once
#include <stdint.h>

namespace fh {

// One row per knob: X(C type, field, environment variable, default, parse kind).  struct Knobs and reload_knobs() are both
// generated from this list.  Parse kinds: INT = atoi of the variable, the default when unset; FLAG = set and non-zero;
// PRESENT = set at all.
#define FH_KNOBS(X)                                                                                                                  \
    /* paged attention (attn_plan.h decides with them) */                                                                            \
    X(bool, attn_no_flash, "FERRUM_HIP_ATTN_NO_FLASH", false, FLAG)                                                                  \
    X(long, attn_flash_min_rows, "FERRUM_HIP_ATTN_FLASH_MIN_ROWS", 512, INT)                                                         \
    X(int, attn_splits, "FERRUM_HIP_ATTN_SPLITS", 0, INT)                       /* > 0: forced KV split count */                     \
    X(long, attn_rs_min_wgs, "FERRUM_HIP_ATTN_RS_MIN_WGS", 512, INT)                                                                 \
    X(bool, attn_no_rs, "FERRUM_HIP_ATTN_NO_RS", false, FLAG)                                                                        \
    X(bool, attn_narrow, "FERRUM_HIP_ATTN_NARROW", false, FLAG)                                                                      \
    X(bool, attn_no_resident, "FERRUM_HIP_ATTN_NO_RESIDENT", false, FLAG)       /* never take the resident-K/V short-prompt prefill form */ \
    X(long, attn_resident_min_wgs, "FERRUM_HIP_ATTN_RESIDENT_MIN_WGS", 128, INT) /* … and only from this many workgroups (tests lower it) */ \
    /* INT4 GEMMs (w4_decode.hip, w4_tiles.hip, w4_skinny.hip) */                                                                    \
    X(int, moe_kw_pairs, "FERRUM_HIP_MOE_KW_PAIRS", 16, INT)                                                                         \
    X(int, decode_chain, "FERRUM_HIP_DECODE_CHAIN", 1, INT)                     /* MoE decode at ≤ 32 rows: tail + q|k|v + attention + o_proj + route as ONE launch (0 = five launches) */ \
    X(int, chain_max_rows, "FERRUM_HIP_CHAIN_MAX_ROWS", 128, INT)               /* decode chain up to this many rows (≤ 128) */      \
    X(int, sandwich_wide, "FERRUM_HIP_SANDWICH_WIDE", 1, INT)                   /* sandwich add + norms of ≤ 64 rows: 1024 threads per row, loads ahead of the reductions (0 = 256 threads) */ \
    X(int, chain_qkv_half, "FERRUM_HIP_CHAIN_QKV_HALF", 1, INT)                 /* decode chain at ≤ 16 rows: q|k|v in 32-column blocks (0 = 64) */ \
    X(int, chain_o_half, "FERRUM_HIP_CHAIN_O_HALF", 1, INT)                     /* … and o_proj */                                   \
    X(int, chain_split_keys, "FERRUM_HIP_CHAIN_SPLIT_KEYS", 256, INT)           /* decode chain attention: target keys per KV range (≤ 16 ranges per (sequence, kv head), see chain_desc in runner_forward.hip); 0 = never split */ \
    X(int, chain_qkv_wide, "FERRUM_HIP_CHAIN_QKV_WIDE", -1, INT)                /* decode chain q|k|v blocks of 128 columns: -1 = where the 64-column blocks + attention exceed chain_slots */ \
    X(int, chain_slots, "FERRUM_HIP_CHAIN_SLOTS", 256, INT)                     /* workgroups of the chain kernel the chip holds at once (one per CU) */ \
    X(int, route_gemm_topk, "FERRUM_HIP_ROUTE_GEMM_TOPK", 1, INT)               /* prefill router GEMM + top-k as one launch (E = 128) */ \
    X(int, chain_attn_splits, "FERRUM_HIP_CHAIN_ATTN_SPLITS", 0, INT)           /* > 0: that many KV ranges whatever the context (experiments) */ \
    X(int, chain_max_keys, "FERRUM_HIP_CHAIN_MAX_KEYS", 4096, INT)              /* decode chain only up to this many keys per attention workgroup (× T·nkv / 128) */ \
    X(int, dense_chain, "FERRUM_HIP_DENSE_CHAIN", 1, INT)                       /* dense models at 17–32 rows: the attention half of the layer as the chain launch too (0 = five launches) */ \
    X(int, moe_em2, "FERRUM_HIP_MOE_EM2", 1, INT)                               /* decode: gate_up → down as one expert-major launch (0 = two launches) */ \
    X(int, moe_deferred_merge, "FERRUM_HIP_MOE_DEFERRED_MERGE", 1, INT)         /* decode chain: the grouped GEMM's prologue merges the router's candidate lists (0 = role B does) */ \
    X(int, moe_pair_rank_lists, "FERRUM_HIP_MOE_PAIR_RANK_LISTS", 1, INT)       /* decode chain + expert pair: the pair's tiles resolve their rows from the candidate lists (0 = role B merges) */ \
    X(int, w4_tile_min_m, "FERRUM_HIP_W4_TILE_MIN_M", 0, INT)                                                                        \
    X(int, w4_tile_wgs, "FERRUM_HIP_W4_TILE_WGS", 256, INT)                                                                          \
    X(int, w4_ldsa, "FERRUM_HIP_W4_LDSA", 1, INT)                                                                                    \
    X(int, w4_ldsa_nw, "FERRUM_HIP_W4_LDSA_NW", 0, INT)                                                                              \
    X(int, w4_ldsa_s, "FERRUM_HIP_W4_LDSA_S", 0, INT)                                                                                \
    X(int, w4_big, "FERRUM_HIP_W4_BIG", 0, INT)                                 /* 0 auto, −1 never, 8 / 16 forces w4_gemm_big_kernel's 128- / 256-row tiles */ \
    X(int, w4_nt, "FERRUM_HIP_W4_NT", 0, INT)                                                                                        \
    X(int, w4_w, "FERRUM_HIP_W4_W", 0, INT)                                                                                          \
    X(int, lds_min_wgs, "FERRUM_HIP_LDS_MIN_WGS", 128, INT)                                                                          \
    X(int, lds_min_groups, "FERRUM_HIP_LDS_MIN_GROUPS", 8, INT)                                                                      \
    /* runner */                                                                                                                     \
    X(bool, no_graph, "FERRUM_HIP_NO_GRAPH", false, PRESENT)                                                                         \
    X(bool, trace_launches, "FERRUM_HIP_TRACE_LAUNCHES", false, PRESENT)        /* … and only together with no_graph */              \
    X(bool, time_same_layer, "FERRUM_HIP_TIME_SAME_LAYER", false, PRESENT)                                                           \
    X(int, tp_fused_norm, "FERRUM_HIP_TP_FUSED_NORM", 1, INT)                   /* tensor parallel, one-shot transport: all-reduce + residual add + norm as one launch (0 = two) */ \
    X(int, tp_oneshot, "FERRUM_HIP_TP_ONESHOT", -1, INT)                        /* -1 auto, 0 never, 1 always (tensor-parallel all-reduce form) */

struct Knobs {
#define FH_KNOB_FIELD(type, field, env, dflt, kind) type field = dflt;
    FH_KNOBS(FH_KNOB_FIELD)
#undef FH_KNOB_FIELD
    bool attn_flash_min_rows_set = false;   // FERRUM_HIP_ATTN_FLASH_MIN_ROWS was given (the runner then takes the value too)
};

const Knobs& knobs();
void reload_knobs();

// One row per kernel form: X(enumerator suffix, name).  enum Form and form_name() are both generated from this list; tests and
// tools index by position and by name, so rows are only ever appended.
#define FH_FORMS(X)                                                                                                                  \
    X(ATTN_FLASH, "attn_flash")                       /* paged_prefill_attn_kernel (LDS-shared K/V, long prompts) */                 \
    X(ATTN_ROW_SPLIT, "attn_row_split")               /* paged_attn_kernel<…, RS> (four row tiles per workgroup) */                  \
    X(ATTN_KV_WIDE, "attn_kv_wide")                   /* paged_attn_kernel 8 waves (decode, ≥ 8 block pairs per split) */            \
    X(ATTN_KV_NARROW, "attn_kv_narrow")               /* paged_attn_kernel 4 waves */                                                \
    X(ATTN_FUSED_QKV_WIDE, "attn_fused_qkv_wide")     /* decode with QK-norm + RoPE + KV write in the prologue, 8 waves */           \
    X(ATTN_FUSED_QKV_NARROW, "attn_fused_qkv_narrow")                                                                                \
    X(ATTN_SPLIT_REDUCE, "attn_split_reduce")         /* KV-split partials + reduce launch */                                        \
    X(W4_WGSPLIT, "w4_wgsplit")                       /* ≤ 16 rows (and small projections): K split over the waves of a workgroup */ \
    X(W4_LDSA, "w4_ldsa")                             /* 17–32 rows: LDS-shared activations */                                       \
    X(W4_TILEP, "w4_tilep")                           /* ≥ 33/64 rows: pipelined 64-row tiles */                                     \
    X(W4_SLABS, "w4_slabs")                           /* fp32 split-K slabs from the skinny kernel */                                \
    X(W4_SLABS_LDS, "w4_slabs_lds")                   /* … from the LDS-shared-activation kernel */                                  \
    X(W4_SLABS_TILE, "w4_slabs_tile")                 /* … from the pipelined tile kernel */                                         \
    X(W4_ROWSUM, "w4_rowsum")                         /* prefill tile kernel with activation row sums taken at LDS staging */        \
    X(MOE_EXPERT_MAJOR, "moe_expert_major")                                                                                          \
    X(MOE_INLINE_ALIGN, "moe_inline_align")                                                                                          \
    X(MOE_BLOCK16, "moe_block16")                                                                                                    \
    X(MOE_TILE64, "moe_tile64")                                                                                                      \
    X(MOE_TILE32, "moe_tile32")                                                                                                      \
    X(MOE_TILE_BIG, "moe_tile_big")                   /* prefill: 96- or 128-pair blocks through w4_gemm_big_kernel */               \
    X(MOE_MERGE_ROUTE, "moe_merge_route")                                                                                            \
    X(ROUTE_SPLIT, "route_split")                     /* add + norm + router split over Q parts per token, merge in the launch */    \
    X(ROUTE_FUSED, "route_fused")                     /* add + norm + router + top-k, one workgroup per token */                     \
    X(ROUTE_GEMM, "route_gemm")                       /* router as a GEMM over all tokens + top-k kernel */                          \
    X(DENSE_SLAB_CHAIN, "dense_slab_chain")           /* dense MLP block: slab GEMMs reduced by their consumers */                   \
    X(GRAPH_CAPTURE, "graph_capture")                                                                                                \
    X(GRAPH_REPLAY, "graph_replay")                                                                                                  \
    X(TP_ALLREDUCE_RCCL, "tp_allreduce_rccl")                                                                                        \
    X(TP_ALLREDUCE_LOOPBACK, "tp_allreduce_loopback")                                                                                \
    X(TP_ALLREDUCE_ONESHOT, "tp_allreduce_oneshot")                                                                                  \
    X(F16_DENSE_LINEAR, "f16_dense_linear")           /* unquantised projection (DenseLinear) */                                     \
    X(W4_FUSED_TAIL, "w4_fused_tail")                 /* ≤ 4-row q|k|v GEMM with the previous layer's combine + add + norm as its prologue */ \
    X(ATTN_RESIDENT, "attn_resident")                 /* short-prompt prefill: the sequence's K/V resident in LDS */                 \
    X(W4_BIG, "w4_big")                               /* prefill: 128- / 256-row tiles, scale folded into the fp16 B operand */      \
    X(GATHER_COLUMNS, "gather_columns")               /* act-order input gather as a launch of its own (no producer wrote the permuted row) */ \
    X(PERM_PRODUCER, "perm_producer")                 /* act-order: the producing kernel (norm, gated activation via gate_up's column order, decode attention) wrote the permuted row */ \
    X(MOE_EXPERT_MAJOR_PAIR, "moe_expert_major_pair") /* gate_up → down in one expert-major launch (in-launch hand-off per expert) */ \
    X(DECODE_CHAIN, "decode_chain")                   /* the attention half of a MoE decode layer as one launch (chain.hip) */       \
    X(MOE_DEFERRED_MERGE, "moe_deferred_merge")       /* the merged grouped GEMM took the routing as per-part candidate lists and merged them itself */ \
    X(DENSE_CHAIN, "dense_chain")                     /* dense model: tail + q|k|v + attention + o_proj + add/norm as the one chain launch (chain.hip) */ \
    X(TP_ALLREDUCE_NORM_FUSED, "tp_allreduce_norm_fused") /* tensor parallel: one-shot all-reduce + residual add + norm as one launch */ \
    X(CHAIN_ATTN_KV_SPLITS, "chain_attn_kv_splits")   /* decode chain with several KV ranges per (sequence, kv head) in its attention role (ticket merge) */ \
    X(CHAIN_QKV_WIDE, "chain_qkv_wide")               /* decode chain with 128-column q|k|v blocks (the narrow ones + attention exceed the resident workgroups) */ \
    X(ROUTE_GEMM_TOPK, "route_gemm_topk")             /* prefill router: logits (MFMA) + softmax + top-k in one launch (moe_route_gemm_topk_kernel) */ \
    X(MOE_PAIR_RANK_LISTS, "moe_pair_rank_lists")     /* the expert pair took the routing as per-part candidate lists: each tile ranks its own expert's candidates */ \
    X(CHAIN_QKV_HALF, "chain_qkv_half")               /* decode chain with 32-column q|k|v blocks (≤ 16 rows; neither this nor chain_qkv_wide: 64 columns) */ \
    X(CHAIN_O_HALF, "chain_o_half")                   /* decode chain with 32-column o_proj blocks (≤ 16 rows, ≤ 2048 columns; otherwise 64) */

enum Form : int {
#define FH_FORM_ENUM(id, name) FORM_##id,
    FH_FORMS(FH_FORM_ENUM)
#undef FH_FORM_ENUM
    FORM_COUNT
};

void form_hit(Form f);
const char* form_name(int f);
void form_hits_snapshot(uint64_t* hits);   // FORM_COUNT counters
void form_hits_reset();

}  // namespace fh
