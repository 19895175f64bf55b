// Paged-KV attention for gfx950: the three entry points and the head-major single-sequence prefill over them.  They check the arguments, fill the kernel argument block, ask
// attn_plan.h which form the shape takes and hand the plan to the launch function of the kernel family: attention_decode.hip
// (KV-split, row-split, fused-qkv decode and the split reduce) or attention_prefill.hip (the LDS-staged prefill forms).
//
// Reference ops: `paged_varlen_attention` / `paged_batched_decode_attention` /
// `paged_decode_attention` (ferrum-kernels/src/backend/traits.rs:1813,1885,1719; CUDA launch sites
// backend/cuda/paged.rs:942,1309,1160).  Maths = causal GQA softmax(QKᵀ/√hd)·V with optional sliding
// window (CPU forms: backend/cpu.rs:2179-2259, ferrum-kv/src/attention.rs:30-114).
#include "attn_common.h"
#include "kernels.h"
#include "kv_layout.h"

// index words of the head-major single-sequence prefill below (C linkage: the symbol name it has always had)
extern "C" __global__ void single_seq_index_kernel(const uint32_t* __restrict__ context_lens, uint32_t* __restrict__ cu, uint32_t* __restrict__ pos, int q_len) {
    if (threadIdx.x == 0) { cu[0] = 0; cu[1] = (uint32_t)q_len; pos[0] = context_lens[0] - (uint32_t)q_len; }
}

namespace fh {

static_assert(ATTN_KV_BLOCK == KV_BLOCK, "attn_plan.h restates the block size of kv_layout.h");

size_t paged_attention_workspace_bytes(int total_q_tokens, int num_heads, int head_dim, int max_kv_len) {
    return attn_workspace_bytes(total_q_tokens, num_heads, head_dim);
}

struct FusedQkv {
    const __half* qkv; const __half* q_norm_w; const __half* k_norm_w; const float* cos_t; const float* sin_t;
    __half* k_pool_w; __half* v_pool_w; float eps; int qk_mode;
};

static int paged_attention_launch(const __half* q, const __half* k_pool, const __half* v_pool, __half* out,
                               const uint32_t* cu_seqlens_q, const uint32_t* pos_offsets, const uint32_t* kv_lens,
                               const int32_t* block_tables, int num_seqs, int total_q_tokens, int max_q_len,
                               int max_kv_len, int num_heads, int num_kv_heads, int head_dim,
                               int sliding_window, int block_size, int max_blocks_per_seq, float* workspace,
                               size_t workspace_bytes, hipStream_t s, const FusedQkv* fq = nullptr,
                               const int32_t* out_scatter = nullptr) {
    if (num_seqs <= 0 || total_q_tokens <= 0) return 0;
    FH_REQUIRE(!out_scatter || (!cu_seqlens_q && max_q_len == 1), "paged attention: scattered output is a decode-form feature");
    FH_REQUIRE(block_size == KV_BLOCK, "paged attention: block_size=%d unsupported (native layout uses 16)", block_size);
    FH_REQUIRE(num_kv_heads > 0 && num_heads % num_kv_heads == 0, "paged attention: nq=%d not a multiple of nkv=%d",
               num_heads, num_kv_heads);
    FH_REQUIRE(head_dim == 128 || head_dim == 64 || head_dim == 256, "paged attention: head_dim=%d unsupported", head_dim);
    // the knobs are read once at library load (knobs.h), never per launch
    const AttnPlan plan = attn_plan({num_seqs, total_q_tokens, max_q_len, max_kv_len, num_heads, num_kv_heads, head_dim}, knobs(),
                                    cu_seqlens_q != nullptr, fq != nullptr, workspace ? workspace_bytes : 0);
    AttnArgs a{};
    a.q = q; a.k_pool = k_pool; a.v_pool = v_pool; a.out = out;
    a.cu_seqlens_q = cu_seqlens_q; a.pos_offsets = pos_offsets; a.kv_lens = kv_lens; a.block_tables = block_tables;
    a.num_seqs = num_seqs; a.nq = num_heads; a.nkv = num_kv_heads;
    a.tiles_per_seq = plan.tiles_per_seq;
    a.max_blocks = max_blocks_per_seq; a.sliding_window = sliding_window;
    a.scale = 1.0f / sqrtf((float)head_dim);
    a.out_scatter = out_scatter;
    a.nsplit = plan.nsplit;
    a.compact = plan.compact;
    a.partial = workspace;
    if (fq) {
        a.qkv = fq->qkv; a.q_norm_w = fq->q_norm_w; a.k_norm_w = fq->k_norm_w; a.cos_t = fq->cos_t; a.sin_t = fq->sin_t;
        a.k_pool_w = fq->k_pool_w; a.v_pool_w = fq->v_pool_w; a.eps = fq->eps; a.qk_mode = fq->qk_mode;
    }
    const bool decode_family = plan.kernel == ATTN_KERNEL_KV_SPLIT || plan.kernel == ATTN_KERNEL_ROW_SPLIT;
    if (int rc = decode_family ? paged_attn_decode_launch(plan, a, head_dim, fq != nullptr, s)
                               : paged_attn_prefill_launch(plan, a, head_dim, s)) return rc;
    form_hit(plan.form);
    if (plan.reduce) form_hit(FORM_ATTN_SPLIT_REDUCE);
    return 0;
}

int paged_varlen_attention_f16(const __half* q, const __half* k_pool, const __half* v_pool, __half* out,
                               const uint32_t* cu_seqlens_q, const uint32_t* pos_offsets,
                               const int32_t* block_tables, int num_seqs, int total_q_tokens, int max_q_len,
                               int max_kv_len, int num_heads, int num_kv_heads, int head_dim,
                               int sliding_window, int block_size, int max_blocks_per_seq, float* workspace,
                               size_t workspace_bytes, hipStream_t s) {
    return paged_attention_launch(q, k_pool, v_pool, out, cu_seqlens_q, pos_offsets, nullptr, block_tables, num_seqs,
                                  total_q_tokens, max_q_len, max_kv_len, num_heads, num_kv_heads, head_dim,
                                  sliding_window, block_size, max_blocks_per_seq, workspace, workspace_bytes, s);
}

// paged_batched_decode_attention (traits.rs:1885): q_len = 1 per sequence, kv length given directly.
int paged_batched_decode_attention_f16(const __half* q, const __half* k_pool, const __half* v_pool, __half* out,
                                       const int32_t* block_tables, const uint32_t* valid_kv_lens, int num_seqs,
                                       int max_kv_len, int num_heads, int num_kv_heads, int head_dim, int block_size,
                                       int max_blocks_per_seq, float* workspace, size_t workspace_bytes,
                                       hipStream_t s, const int32_t* out_scatter) {
    return paged_attention_launch(q, k_pool, v_pool, out, nullptr, nullptr, valid_kv_lens, block_tables, num_seqs,
                                  num_seqs, 1, max_kv_len, num_heads, num_kv_heads, head_dim, 0, block_size,
                                  max_blocks_per_seq, workspace, workspace_bytes, s, nullptr, out_scatter);
}

// Decode step of one layer in ONE launch: split_qkv_norm_rope_into_paged_cache_varlen (q_len = 1 per sequence,
// position = valid_kv_lens[seq] − 1) + paged_batched_decode_attention.  Same results as the two-op chain.
int paged_decode_attention_fused_qkv_f16(const __half* qkv, const __half* q_norm_w, const __half* k_norm_w,
                                         const float* cos_t, const float* sin_t, float eps, int qk_mode, __half* k_pool,
                                         __half* v_pool, __half* out, const int32_t* block_tables,
                                         const uint32_t* valid_kv_lens, int num_seqs, int max_kv_len, int num_heads,
                                         int num_kv_heads, int head_dim, int sliding_window, int block_size,
                                         int max_blocks_per_seq, float* workspace, size_t workspace_bytes, hipStream_t s,
                                         const int32_t* out_scatter) {
    FH_REQUIRE(num_kv_heads > 0 && num_heads % num_kv_heads == 0 && num_heads / num_kv_heads <= 14,
               "fused decode attention: GQA group %d/%d must be <= 14", num_heads, num_kv_heads);
    FH_REQUIRE(qk_mode >= 0 && qk_mode <= 3, "fused decode attention: qk_mode=%d out of range", qk_mode);
    FusedQkv fq{qkv, q_norm_w, k_norm_w, cos_t, sin_t, k_pool, v_pool, eps, qk_mode};
    return paged_attention_launch(nullptr, k_pool, v_pool, out, nullptr, nullptr, valid_kv_lens, block_tables, num_seqs,
                                  num_seqs, 1, max_kv_len, num_heads, num_kv_heads, head_dim, sliding_window, block_size,
                                  max_blocks_per_seq, workspace, workspace_bytes, s, &fq, out_scatter);
}

// The q_len > 1 form of BackendPagedKv::paged_decode_attention (traits.rs:1719-1738): ONE sequence in causal prefill, q / out
// [num_heads, q_len, head_dim] head-major; context_lens[0] is the FINAL kv length (token i sees positions
// [0, context_len − q_len + 1 + i)).  The workspace holds the two token-major copies, the index words and the attention scratch.
int paged_single_seq_prefill_attention_f16(const __half* q, const __half* k_pool, const __half* v_pool, __half* out,
                                           const int32_t* block_tables, const uint32_t* context_lens, int q_len, int num_heads,
                                           int num_kv_heads, int head_dim, int block_size, int max_num_blocks_per_seq,
                                           float* workspace, size_t workspace_bytes, hipStream_t s) {
    const int kv_bound = max_num_blocks_per_seq * block_size;            // the kv lengths live on the device: the table width bounds them
    const size_t elems = (size_t)q_len * num_heads * head_dim;
    const size_t need = 2 * elems * 2 + 256;
    FH_REQUIRE(workspace && workspace_bytes >= need + (1 << 20), "paged_decode_attention: workspace of %zu bytes needed for the head-major transposes", need + (1 << 20));
    __half* q_tm = reinterpret_cast<__half*>(workspace);
    __half* o_tm = q_tm + elems;
    uint32_t* idx = reinterpret_cast<uint32_t*>(o_tm + elems);
    float* attn_ws = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(workspace) + (need + 255) / 256 * 256);
    const size_t attn_ws_bytes = workspace_bytes - (need + 255) / 256 * 256;
    hipLaunchKernelGGL(single_seq_index_kernel, dim3(1), dim3(64), 0, s, context_lens, idx, idx + 2, q_len);
    FH_CHECK_LAUNCH();
    if (int rc = transpose_head_to_token_f16(q, q_tm, q_len, num_heads, head_dim, s)) return rc;
    if (int rc = paged_varlen_attention_f16(q_tm, k_pool, v_pool, o_tm, idx, idx + 2, block_tables, 1, q_len, q_len, kv_bound,
                                            num_heads, num_kv_heads, head_dim, 0, block_size, max_num_blocks_per_seq, attn_ws,
                                            attn_ws_bytes, s)) return rc;
    return transpose_token_to_head_f16(o_tm, out, q_len, num_heads, head_dim, s);
}

}  // namespace fh
