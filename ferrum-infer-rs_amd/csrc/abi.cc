// C-ABI layer (include/ferrum_hip.h) over the gfx950 kernels: the error text, device / stream / memory / event / workspace /
// graph calls, the thin op wrappers (argument validation, then the fh:: launcher), the block allocator and the
// native-operator descriptor.  Host-only code; compiled with hipcc.  The GPTQ / expert-stack handle is abi_gptq.cc.
#include <stdarg.h>

#include "../../include/ferrum_hip.h"
#include "abi_private.h"
#include "block_allocator.h"
#include "common.h"
#include "kernels.h"
#include "knobs.h"

namespace fh {
static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char* last_error() { return g_err; }
}  // namespace fh

using namespace fh;

struct FerrumHipGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

extern "C" {

// ── native operator artifact ────────────────────────────────────────────────
static const FerrumNativeOperatorDescriptor g_desc = {1u, "ferrum_hip_decode", "1"};
int ferrum_native_op_init(void) { return 0; }
const FerrumNativeOperatorDescriptor* ferrum_native_op_descriptor(void) { return &g_desc; }

const char* ferrum_hip_last_error(void) { return fh::last_error(); }

// ── debug: which kernel forms ran, and re-reading the development knobs ─────
int ferrum_hip_debug_form_count(void) { return fh::FORM_COUNT; }
const char* ferrum_hip_debug_form_name(int form) { return fh::form_name(form); }
int ferrum_hip_debug_form_hits(uint64_t* hits, int capacity) {
    FH_REQUIRE(hits && capacity >= fh::FORM_COUNT, "debug_form_hits: need room for %d counters", (int)fh::FORM_COUNT);
    fh::form_hits_snapshot(hits);
    return 0;
}
int ferrum_hip_debug_form_reset(void) { fh::form_hits_reset(); return 0; }
int ferrum_hip_debug_reload_knobs(void) { fh::reload_knobs(); return 0; }

int ferrum_hip_device_count(int* count) {
    FH_REQUIRE(count, "device_count: null output");
    hipError_t e = hipGetDeviceCount(count);
    if (e != hipSuccess) { *count = 0; fh::set_error("hipGetDeviceCount: %s", hipGetErrorString(e)); return 1; }
    return 0;
}
int ferrum_hip_set_device(int ordinal) { FH_CHECK_HIP(hipSetDevice(ordinal)); return 0; }
int ferrum_hip_stream_create(void** stream) {
    FH_REQUIRE(stream, "stream_create: null output");
    hipStream_t s;
    FH_CHECK_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = s;
    return 0;
}
int ferrum_hip_stream_destroy(void* stream) { FH_CHECK_HIP(hipStreamDestroy(ST(stream))); return 0; }
int ferrum_hip_stream_synchronize(void* stream) { FH_CHECK_HIP(hipStreamSynchronize(ST(stream))); return 0; }
int ferrum_hip_alloc(void** dev_ptr, size_t bytes) {
    FH_REQUIRE(dev_ptr, "alloc: null output");
    *dev_ptr = nullptr;
    if (bytes == 0) return 0;
    FH_CHECK_HIP(hipMalloc(dev_ptr, bytes));
    FH_CHECK_HIP(hipMemset(*dev_ptr, 0, bytes));
    return 0;
}
int ferrum_hip_free(void* dev_ptr) { if (dev_ptr) FH_CHECK_HIP(hipFree(dev_ptr)); return 0; }
int ferrum_hip_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream) {
    if (bytes == 0) return 0;
    FH_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ST(stream)));
    FH_CHECK_HIP(hipStreamSynchronize(ST(stream)));
    return 0;
}
int ferrum_hip_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream) {
    if (bytes == 0) return 0;
    FH_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ST(stream)));
    FH_CHECK_HIP(hipStreamSynchronize(ST(stream)));
    return 0;
}
int ferrum_hip_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream) {
    if (bytes == 0) return 0;
    FH_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ST(stream)));
    return 0;
}
int ferrum_hip_memset_zero(void* p, size_t bytes, void* stream) {
    if (bytes == 0) return 0;
    FH_CHECK_HIP(hipMemsetAsync(p, 0, bytes, ST(stream)));
    return 0;
}

int ferrum_hip_workspace_create(FerrumHipWorkspace** ws, size_t bytes) {
    FH_REQUIRE(ws, "workspace_create: null output");
    auto* w = new FerrumHipWorkspace();
    if (bytes) {
        hipError_t e = hipMalloc((void**)&w->ptr, bytes);
        if (e != hipSuccess) { delete w; fh::set_error("workspace hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); return 1; }
    }
    w->bytes = bytes;
    *ws = w;
    return 0;
}
int ferrum_hip_workspace_destroy(FerrumHipWorkspace* ws) {
    if (!ws) return 0;
    if (ws->ptr) (void)hipFree(ws->ptr);
    delete ws;
    return 0;
}

// ── norms / elementwise ─────────────────────────────────────────────────────
int ferrum_hip_rms_norm_f16(const void* x, const void* w, float eps, void* out, int tokens, int dim, void* stream) {
    FH_REQUIRE(tokens == 0 || (x && w && out), "rms_norm: null buffer");
    return rms_norm_f16(CH(x), CH(w), eps, H(out), tokens, dim, ST(stream));
}
int ferrum_hip_fused_add_rms_norm_f16(void* residual, const void* x, const void* w, float eps, void* out,
                                      int tokens, int dim, void* stream) {
    FH_REQUIRE(tokens == 0 || (residual && x && w && out), "fused_add_rms_norm: null buffer");
    return fused_add_rms_norm_f16(H(residual), CH(x), CH(w), eps, H(out), tokens, dim, ST(stream));
}
int ferrum_hip_embedding_lookup_f16(const void* table, const uint32_t* ids, void* out, int n_ids, int dim, void* stream) {
    FH_REQUIRE(n_ids == 0 || (table && ids && out), "embedding_lookup: null buffer");
    return embedding_lookup_f16(CH(table), ids, H(out), n_ids, dim, ST(stream));
}
int ferrum_hip_fused_silu_mul_split_f16(const void* gate_up, void* out, int tokens, int im, void* stream) {
    FH_REQUIRE(tokens == 0 || (gate_up && out), "fused_silu_mul_split: null buffer");
    return fused_silu_mul_split_f16(CH(gate_up), H(out), tokens, im, ST(stream));
}
int ferrum_hip_fused_gelu_tanh_mul_split_f16(const void* gate_up, void* out, int tokens, int im, void* stream) {
    FH_REQUIRE(tokens == 0 || (gate_up && out), "fused_gelu_tanh_mul_split: null buffer");
    return fused_gelu_tanh_mul_split_f16(CH(gate_up), H(out), tokens, im, ST(stream));
}
int ferrum_hip_scale_inplace_f16(void* buf, float scale, size_t len, void* stream) {
    FH_REQUIRE(len == 0 || buf, "scale_inplace: null buffer");
    return scale_inplace_f16(H(buf), scale, (long)len, ST(stream));
}
int ferrum_hip_add_inplace_f16(void* residual, const void* x, size_t len, void* stream) {
    FH_REQUIRE(len == 0 || (residual && x), "add_inplace: null buffer");
    return add_inplace_f16(H(residual), CH(x), (long)len, ST(stream));
}
int ferrum_hip_add_bias_f16(void* data, const void* bias, int rows, int cols, void* stream) {
    FH_REQUIRE(rows == 0 || cols == 0 || (data && bias), "add_bias: null buffer");
    return add_bias_f16(H(data), CH(bias), rows, cols, ST(stream));
}

// ── head / tail of a forward, slab-input and gathered-store forms (the runner's own launches, exported op by op) ──
int ferrum_hip_fused_add_rms_norm_perm_f16(void* residual, const void* x, const void* w, float eps, void* out, int tokens, int dim,
                                           const int32_t* out_perm, void* stream) {
    FH_REQUIRE(tokens == 0 || (residual && x && w && out), "fused_add_rms_norm_perm: null buffer");
    return fused_add_rms_norm_f16(H(residual), CH(x), CH(w), eps, H(out), tokens, dim, ST(stream), out_perm);
}
int ferrum_hip_embed_rms_norm_f16(const void* table, const uint32_t* token_ids, float embed_scale, void* residual, float* residual_f32,
                                  const void* w, float eps, void* norm_out, int tokens, int dim, unsigned* zero_words, int n_zero,
                                  const int32_t* out_perm, void* stream) {
    FH_REQUIRE(tokens == 0 || (table && token_ids && w && norm_out), "embed_rms_norm: null buffer");
    FH_REQUIRE(n_zero >= 0 && (n_zero == 0 || zero_words), "embed_rms_norm: n_zero=%d without zero_words", n_zero);
    return embed_rms_norm_f16(CH(table), token_ids, embed_scale, H(residual), residual_f32, CH(w), eps, H(norm_out), tokens, dim,
                              zero_words, n_zero, ST(stream), out_perm);
}
int ferrum_hip_gather_rms_norm_f16(const void* x, const int32_t* row_idx, const void* w, float eps, void* out, int rows, int dim,
                                   void* stream) {
    FH_REQUIRE(rows == 0 || (x && row_idx && w && out), "gather_rms_norm: null buffer");
    return gather_rms_norm_f16(CH(x), row_idx, CH(w), eps, H(out), rows, dim, ST(stream));
}
int ferrum_hip_fused_gated_act_slabs_f16(const float* slabs, int num_slabs, size_t slab_stride, int ld, void* out, int tokens, int im,
                                         int gelu, void* stream) {
    FH_REQUIRE(tokens == 0 || (slabs && out), "fused_gated_act_slabs: null buffer");
    return fused_gated_act_slabs_f16(slabs, num_slabs, (long)slab_stride, ld, H(out), tokens, im, gelu, ST(stream));
}
int ferrum_hip_gather_columns_f16(const void* in, const int32_t* perm, void* out, int rows, int cols, void* stream) {
    FH_REQUIRE(rows == 0 || cols == 0 || (in && perm && out), "gather_columns: null buffer");
    FH_REQUIRE(in != out || rows == 0, "gather_columns: in place");
    return gather_columns_f16(CH(in), perm, H(out), rows, cols, ST(stream));
}

// ── the scoring head (score_head.hip) ──
int ferrum_hip_logprob_rows_f32(const float* logits, int ld, int m, int n, const int32_t* pair_rows, const uint32_t* pair_tokens,
                                int num_pairs, float* pair_logprob, float* row_lse, uint32_t* row_top, FerrumHipWorkspace* ws, void* stream) {
    FH_REQUIRE(m <= 0 || logits, "logprob_rows: null logits");
    FH_REQUIRE(num_pairs <= 0 || (pair_rows && pair_tokens && pair_logprob), "logprob_rows: null pair buffer");
    return logprob_rows_f32(logits, ld, m, n, pair_rows, pair_tokens, num_pairs, pair_logprob, row_lse, row_top, nullptr, ws ? ws->ptr : nullptr,
                            ws ? ws->bytes : 0, ST(stream));
}

// ── the embedding tail (embed_pool.hip), exported for the element-wise tests ──
static int embed_pool_export(const void* hidden, bool f32, const int32_t* seq_rows, const void* norm_w, float eps, int pooling, int normalize,
                             int dims, float* out, int num_seqs, int dim, FerrumHipWorkspace* ws, void* stream) {
    FH_REQUIRE(num_seqs <= 0 || (hidden && seq_rows && out), "embed_pool: null buffer");
    return embed_pool(hidden, f32, seq_rows, CH(norm_w), eps, pooling, normalize, dims, out, num_seqs, dim, 0, ws ? ws->ptr : nullptr,
                      ws ? ws->bytes : 0, ST(stream));
}
int ferrum_hip_embed_pool_f16(const void* hidden, const int32_t* seq_rows, const void* norm_w, float eps, int pooling, int normalize,
                              int dims, float* out, int num_seqs, int dim, FerrumHipWorkspace* ws, void* stream) {
    return embed_pool_export(hidden, false, seq_rows, norm_w, eps, pooling, normalize, dims, out, num_seqs, dim, ws, stream);
}
int ferrum_hip_embed_pool_f32(const float* hidden, const int32_t* seq_rows, const void* norm_w, float eps, int pooling, int normalize,
                              int dims, float* out, int num_seqs, int dim, FerrumHipWorkspace* ws, void* stream) {
    return embed_pool_export(hidden, true, seq_rows, norm_w, eps, pooling, normalize, dims, out, num_seqs, dim, ws, stream);
}

int ferrum_hip_layer_norm_f16(const void* x, const void* gamma, const void* beta, float eps, void* out, int tokens, int dim, void* stream) {
    FH_REQUIRE(tokens == 0 || (x && gamma && beta && out), "layer_norm: null buffer");
    return layer_norm_f16(CH(x), CH(gamma), CH(beta), eps, H(out), tokens, dim, ST(stream));
}
int ferrum_hip_gelu_f16(const void* x, void* out, size_t len, void* stream) {
    FH_REQUIRE(len == 0 || (x && out), "gelu: null buffer");
    return gelu_f16(CH(x), H(out), (long)len, ST(stream));
}

// ── device timer (Backend::Timer, backend/timer.rs:88-109: record on the context's stream, elapsed after both fired) ──
int ferrum_hip_event_create(void** event) {
    FH_REQUIRE(event, "event_create: null");
    hipEvent_t e;
    FH_CHECK_HIP(hipEventCreate(&e));
    *event = (void*)e;
    return 0;
}
int ferrum_hip_event_destroy(void* event) {
    if (event) (void)hipEventDestroy((hipEvent_t)event);
    return 0;
}
int ferrum_hip_event_record(void* event, void* stream) {
    FH_REQUIRE(event, "event_record: null");
    FH_CHECK_HIP(hipEventRecord((hipEvent_t)event, ST(stream)));
    return 0;
}
int ferrum_hip_event_elapsed_ms(void* start, void* end, float* ms) {
    FH_REQUIRE(start && end && ms, "event_elapsed_ms: null");
    FH_CHECK_HIP(hipEventSynchronize((hipEvent_t)end));
    FH_CHECK_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)end));
    return 0;
}

// ── dense GEMM ──────────────────────────────────────────────────────────────
int ferrum_hip_gemm_f16(const void* a, const void* b, void* out, int m, int n, int k, FerrumHipWorkspace* ws, void* stream) {
    FH_REQUIRE(m == 0 || (a && b && out), "gemm: null buffer");
    return f16_gemm(CH(a), CH(b), H(out), m, n, k, ws ? ws->ptr : nullptr, ws ? ws->bytes : 0, ST(stream));
}
int ferrum_hip_gemm_f16_f32out(const void* a, const void* b, float* out, int m, int n, int k, FerrumHipWorkspace* ws,
                               void* stream) {
    FH_REQUIRE(m == 0 || (a && b && out), "gemm: null buffer");
    return f16_gemm_f32out(CH(a), CH(b), out, m, n, k, ws ? ws->ptr : nullptr, ws ? ws->bytes : 0, ST(stream));
}

size_t ferrum_hip_dense_f16t_bytes(int n, int k) { return f16t_elems(n, k) * 2; }
int ferrum_hip_dense_repack_f16t(const void* w, void* out, int n, int k, void* stream) {
    FH_REQUIRE(w && out, "dense_repack_f16t: null buffer");
    return f16t_repack(CH(w), H(out), n, k, ST(stream));
}
int ferrum_hip_gemm_f16t(const void* a, const void* b, void* out, int m, int n, int k, FerrumHipWorkspace* ws, void* stream) {
    FH_REQUIRE(m == 0 || (a && b && out), "gemm_f16t: null buffer");
    return f16t_gemm(CH(a), CH(b), H(out), m, n, k, ws ? ws->ptr : nullptr, ws ? ws->bytes : 0, ST(stream));
}
int ferrum_hip_gemm_f16t_f32out(const void* a, const void* b, float* out, int m, int n, int k, FerrumHipWorkspace* ws,
                                void* stream) {
    FH_REQUIRE(m == 0 || (a && b && out), "gemm_f16t: null buffer");
    return f16t_gemm_f32out(CH(a), CH(b), out, m, n, k, ws ? ws->ptr : nullptr, ws ? ws->bytes : 0, ST(stream));
}

int ferrum_hip_sandwich_add_rms_norm_f32(const void* branch_f16, const void* w_branch, float* residual_f32, const void* w_next,
                                         float eps, void* norm_out_f16, int tokens, int dim, void* stream) {
    FH_REQUIRE(tokens == 0 || (branch_f16 && w_branch && residual_f32 && (!w_next || norm_out_f16)), "sandwich_add_rms_norm_f32: null buffer");
    return sandwich_add_rms_norm_f32(CH(branch_f16), CH(w_branch), residual_f32, CH(w_next), eps, H(norm_out_f16), tokens, dim,
                                     ST(stream));
}
int ferrum_hip_sandwich_add_rms_norm_f32_perm(const void* branch_f16, const void* w_branch, float* residual_f32, const void* w_next,
                                              float eps, void* norm_out_f16, int tokens, int dim, const int32_t* out_perm, void* stream) {
    FH_REQUIRE(tokens == 0 || (branch_f16 && w_branch && residual_f32 && (!w_next || norm_out_f16)), "sandwich_add_rms_norm_f32_perm: null buffer");
    return sandwich_add_rms_norm_f32(CH(branch_f16), CH(w_branch), residual_f32, CH(w_next), eps, H(norm_out_f16), tokens, dim,
                                     ST(stream), out_perm);
}
int ferrum_hip_sandwich_add_rms_norm_f32_slabs(const float* slabs, int num_slabs, size_t slab_stride, int ld_slab, const void* w_branch,
                                               float* residual_f32, const void* w_next, float eps, void* norm_out_f16, int tokens,
                                               int dim, const int32_t* out_perm, void* stream) {
    FH_REQUIRE(tokens == 0 || (slabs && w_branch && residual_f32 && (!w_next || norm_out_f16)), "sandwich_add_rms_norm_f32_slabs: null buffer");
    FH_REQUIRE(ld_slab >= dim, "sandwich_add_rms_norm_f32_slabs: ld_slab=%d < dim=%d", ld_slab, dim);
    return sandwich_add_rms_norm_f32_slabs(slabs, num_slabs, (long)slab_stride, ld_slab, CH(w_branch), residual_f32, CH(w_next), eps,
                                           H(norm_out_f16), tokens, dim, ST(stream), out_perm);
}
int ferrum_hip_rms_norm_f32_to_f16(const float* x_f32, const int32_t* row_idx, const void* w, float eps, void* out_f16, int n_rows,
                                   int dim, void* stream) {
    FH_REQUIRE(n_rows == 0 || (x_f32 && w && out_f16), "rms_norm_f32_to_f16: null buffer");
    return rms_norm_f32_to_f16(x_f32, row_idx, CH(w), eps, H(out_f16), n_rows, dim, ST(stream));
}

// ── contiguous-KV lane of the core trait ─────────────────────────────────────
int ferrum_hip_split_qkv_f16(const void* qkv, void* q, void* k, void* v, int tokens, int q_dim, int kv_dim, void* stream) {
    FH_REQUIRE(tokens == 0 || (qkv && q && k && v), "split_qkv: null buffer");
    return split_qkv_f16(CH(qkv), H(q), H(k), H(v), tokens, q_dim, kv_dim, ST(stream));
}
int ferrum_hip_qk_norm_rope_f16(const void* input, const void* norm_w, const float* cos_tab, const float* sin_tab, void* output,
                                int tokens, int heads, int head_dim, int pos_offset, float eps, int mode, void* stream) {
    FH_REQUIRE(tokens == 0 || (input && output), "qk_norm_rope: null buffer");
    FH_REQUIRE(mode == 0 || (cos_tab && sin_tab), "qk_norm_rope: rope tables missing");
    FH_REQUIRE(mode != 1 || norm_w, "qk_norm_rope: norm weights missing for mode 1");
    return qk_norm_rope_f16(CH(input), CH(norm_w), cos_tab, sin_tab, H(output), tokens, heads, head_dim, pos_offset, eps, mode,
                            ST(stream));
}
int ferrum_hip_kv_cache_append_head_major_f16(void* cache_k, void* cache_v, int cache_len, int cache_capacity, const void* new_k,
                                              const void* new_v, int new_tokens, int nkv, int head_dim, void* stream) {
    FH_REQUIRE(new_tokens == 0 || (cache_k && cache_v && new_k && new_v), "kv_cache_append_head_major: null buffer");
    return kv_cache_append_head_major_f16(H(cache_k), H(cache_v), cache_len, cache_capacity, CH(new_k), CH(new_v), new_tokens, nkv,
                                          head_dim, ST(stream));
}
int ferrum_hip_transpose_head_to_token_f16(const void* src, void* dst, int tokens, int heads, int dim, void* stream) {
    FH_REQUIRE(tokens == 0 || (src && dst), "transpose_head_to_token: null buffer");
    return transpose_head_to_token_f16(CH(src), H(dst), tokens, heads, dim, ST(stream));
}
int ferrum_hip_transpose_token_to_head_f16(const void* src, void* dst, int tokens, int heads, int dim, void* stream) {
    FH_REQUIRE(tokens == 0 || (src && dst), "transpose_token_to_head: null buffer");
    return transpose_token_to_head_f16(CH(src), H(dst), tokens, heads, dim, ST(stream));
}
int ferrum_hip_copy_slice_f16(const void* src, size_t src_offset, void* dst, size_t dst_offset, size_t len, void* stream) {
    FH_REQUIRE(len == 0 || (src && dst), "copy_slice: null buffer");
    return copy_slice_f16(CH(src), (long)src_offset, H(dst), (long)dst_offset, (long)len, ST(stream));
}
int ferrum_hip_scaled_add_inplace_f16(void* dst, const void* src, float scale, size_t len, void* stream) {
    FH_REQUIRE(len == 0 || (src && dst), "scaled_add_inplace: null buffer");
    return scaled_add_inplace_f16(H(dst), CH(src), scale, (long)len, ST(stream));
}
int ferrum_hip_flash_attention_f16(const void* q, const void* k, const void* v, void* out, int batch, int q_len, int kv_len,
                                   int pos_offset, int num_heads, int num_kv_heads, int head_dim, int causal, float scale,
                                   int kv_seq_stride, int sliding_window, void* stream) {
    FH_REQUIRE(q && k && v && out, "flash_attention: null buffer");
    if (batch != 1) { fh::set_error("flash_attention: batch=%d (the reference's CPU and decode paths use batch 1)", batch); return FERRUM_HIP_UNSUPPORTED; }
    return flash_attention_contig_f16(CH(q), CH(k), CH(v), H(out), q_len, kv_len, causal, pos_offset, num_heads, num_kv_heads, head_dim,
                                      scale, kv_seq_stride, sliding_window, ST(stream));
}

// ── paged KV ────────────────────────────────────────────────────────────────
size_t ferrum_hip_paged_pool_bytes(int num_blocks, int kv_heads, int head_dim) {
    return (size_t)num_blocks * kv_heads * 16 * head_dim * 2;
}

int ferrum_hip_split_qkv_norm_rope_into_paged_cache_varlen_f16(
    const void* qkv, const void* q_norm_w, const void* k_norm_w, const float* cos_tab, const float* sin_tab,
    void* q_out, void* cache_k, void* cache_v, const uint32_t* cu_seqlens_q, const uint32_t* pos_offsets,
    const int32_t* block_tables, int num_seqs, int m_total, int q_heads, int kv_heads, int head_dim, float eps,
    int qk_mode, int block_size, int max_blocks_per_seq, void* stream) {
    FH_REQUIRE(m_total == 0 || (qkv && q_out && cache_k && cache_v && cu_seqlens_q && pos_offsets && block_tables),
               "split_qkv_norm_rope_into_paged_cache_varlen: null buffer");
    FH_REQUIRE(qk_mode == 0 || (cos_tab && sin_tab), "split_qkv_norm_rope: rope tables missing");
    FH_REQUIRE(qk_mode != 1 || (q_norm_w && k_norm_w), "split_qkv_norm_rope: norm weights missing for qk_mode 1");
    return split_qkv_norm_rope_into_paged_cache_varlen_f16(CH(qkv), CH(q_norm_w), CH(k_norm_w), cos_tab, sin_tab,
                                                           H(q_out), H(cache_k), H(cache_v), cu_seqlens_q, pos_offsets,
                                                           block_tables, num_seqs, m_total, q_heads, kv_heads, head_dim,
                                                           eps, qk_mode, block_size, max_blocks_per_seq, ST(stream));
}

int ferrum_hip_paged_varlen_attention_f16(const void* q, const void* k_pool, const void* v_pool, void* out,
                                          const uint32_t* cu_seqlens_q, const uint32_t* pos_offsets,
                                          const int32_t* block_tables, int num_seqs, int total_q_tokens, int max_kv_len,
                                          int num_heads, int num_kv_heads, int head_dim, int sliding_window,
                                          int block_size, int max_num_blocks_per_seq, int max_q_len,
                                          FerrumHipWorkspace* ws, void* stream) {
    FH_REQUIRE(total_q_tokens == 0 || (q && k_pool && v_pool && out && cu_seqlens_q && pos_offsets && block_tables),
               "paged_varlen_attention: null buffer");
    return paged_varlen_attention_f16(CH(q), CH(k_pool), CH(v_pool), H(out), cu_seqlens_q, pos_offsets, block_tables,
                                      num_seqs, total_q_tokens, max_q_len, max_kv_len, num_heads, num_kv_heads, head_dim,
                                      sliding_window, block_size, max_num_blocks_per_seq, ws ? ws->ptr : nullptr,
                                      ws ? ws->bytes : 0, ST(stream));
}

int ferrum_hip_paged_batched_decode_attention_f16(const void* q, const void* k_pool, const void* v_pool, void* out,
                                                  const int32_t* block_tables, const uint32_t* valid_kv_lens,
                                                  int num_seqs, int max_kv_len, int num_heads, int num_kv_heads,
                                                  int head_dim, int block_size, int max_num_blocks_per_seq,
                                                  FerrumHipWorkspace* ws, void* stream) {
    FH_REQUIRE(num_seqs == 0 || (q && k_pool && v_pool && out && block_tables && valid_kv_lens),
               "paged_batched_decode_attention: null buffer");
    return paged_batched_decode_attention_f16(CH(q), CH(k_pool), CH(v_pool), H(out), block_tables, valid_kv_lens,
                                              num_seqs, max_kv_len, num_heads, num_kv_heads, head_dim, block_size,
                                              max_num_blocks_per_seq, ws ? ws->ptr : nullptr, ws ? ws->bytes : 0,
                                              ST(stream));
}

// BackendPagedKv::paged_decode_attention (traits.rs:1719-1738).  q_len == 1: q / out [num_seqs, num_heads, head_dim]
// token-major, one query token per sequence.  q_len > 1: ONE sequence in causal prefill, q / out [num_heads, q_len, head_dim]
// head-major; context_lens[0] is the FINAL kv length (token i sees positions [0, context_len − q_len + 1 + i)).
int ferrum_hip_paged_decode_attention_f16(const void* q, const void* k_pool, const void* v_pool, void* out,
                                          const int32_t* block_tables, const uint32_t* context_lens, int num_seqs, int num_heads,
                                          int num_kv_heads, int head_dim, int block_size, int max_num_blocks_per_seq, int q_len,
                                          FerrumHipWorkspace* ws, void* stream) {
    FH_REQUIRE(num_seqs == 0 || (q && k_pool && v_pool && out && block_tables && context_lens), "paged_decode_attention: null buffer");
    FH_REQUIRE(q_len >= 1, "paged_decode_attention: q_len=%d", q_len);
    if (num_seqs <= 0) return 0;
    const int kv_bound = max_num_blocks_per_seq * block_size;            // the kv lengths live on the device: the table width bounds them
    if (q_len == 1)
        return paged_batched_decode_attention_f16(CH(q), CH(k_pool), CH(v_pool), H(out), block_tables, context_lens, num_seqs, kv_bound,
                                                  num_heads, num_kv_heads, head_dim, block_size, max_num_blocks_per_seq,
                                                  ws ? ws->ptr : nullptr, ws ? ws->bytes : 0, ST(stream));
    if (num_seqs != 1) { fh::set_error("paged_decode_attention: q_len=%d > 1 is the single-sequence prefill form (num_seqs=%d)", q_len, num_seqs); return FERRUM_HIP_UNSUPPORTED; }
    return paged_single_seq_prefill_attention_f16(CH(q), CH(k_pool), CH(v_pool), H(out), block_tables, context_lens, q_len, num_heads,
                                                  num_kv_heads, head_dim, block_size, max_num_blocks_per_seq, ws ? ws->ptr : nullptr,
                                                  ws ? ws->bytes : 0, ST(stream));
}

// BackendGraph (capabilities.rs:35-70): begin / end stream capture, replay, drop.  The key → graph map of the trait
// (`end_graph_capture(key)`, `replay_graph(key)`) is a HashMap in the binding; this side owns the graph objects.
int ferrum_hip_graph_begin_capture(void* stream) {
    FH_CHECK_HIP(hipStreamBeginCapture(ST(stream), hipStreamCaptureModeThreadLocal));
    return 0;
}
int ferrum_hip_graph_end_capture(void* stream, FerrumHipGraph** graph) {
    FH_REQUIRE(graph, "graph_end_capture: null output");
    auto* g = new FerrumHipGraph();
    hipError_t e = hipStreamEndCapture(ST(stream), &g->graph);
    if (e == hipSuccess) e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        if (g->graph) (void)hipGraphDestroy(g->graph);
        delete g;
        fh::set_error("graph_end_capture: %s", hipGetErrorString(e));
        return 1;
    }
    *graph = g;
    return 0;
}
int ferrum_hip_graph_replay(FerrumHipGraph* graph, void* stream) {
    FH_REQUIRE(graph && graph->exec, "graph_replay: null graph");
    FH_CHECK_HIP(hipGraphLaunch(graph->exec, ST(stream)));
    return 0;
}
int ferrum_hip_graph_destroy(FerrumHipGraph* graph) {
    if (!graph) return 0;
    if (graph->exec) (void)hipGraphExecDestroy(graph->exec);
    if (graph->graph) (void)hipGraphDestroy(graph->graph);
    delete graph;
    return 0;
}

int ferrum_hip_paged_decode_attention_fused_qkv_f16(const void* qkv, const void* q_norm_w, const void* k_norm_w,
                                                    const float* cos_tab, const float* sin_tab, float eps, int qk_mode,
                                                    void* k_pool, void* v_pool, void* out, const int32_t* block_tables,
                                                    const uint32_t* valid_kv_lens, int num_seqs, int max_kv_len,
                                                    int num_heads, int num_kv_heads, int head_dim, int sliding_window,
                                                    int block_size, int max_num_blocks_per_seq, FerrumHipWorkspace* ws,
                                                    void* stream) {
    FH_REQUIRE(num_seqs == 0 || (qkv && k_pool && v_pool && out && block_tables && valid_kv_lens),
               "paged_decode_attention_fused_qkv: null buffer");
    FH_REQUIRE(qk_mode == 0 || (cos_tab && sin_tab), "paged_decode_attention_fused_qkv: rope tables missing");
    FH_REQUIRE(qk_mode != 1 || (q_norm_w && k_norm_w), "paged_decode_attention_fused_qkv: norm weights missing for qk_mode 1");
    return paged_decode_attention_fused_qkv_f16(CH(qkv), CH(q_norm_w), CH(k_norm_w), cos_tab, sin_tab, eps, qk_mode,
                                                H(k_pool), H(v_pool), H(out), block_tables, valid_kv_lens, num_seqs,
                                                max_kv_len, num_heads, num_kv_heads, head_dim, sliding_window, block_size,
                                                max_num_blocks_per_seq, ws ? ws->ptr : nullptr, ws ? ws->bytes : 0,
                                                ST(stream));
}

int ferrum_hip_paged_kv_read_f16(const void* cache_k, const void* cache_v, const int32_t* block_table, int kv_len,
                                 int kv_heads, int head_dim, int block_size, void* k_out, void* v_out, void* stream) {
    return paged_kv_read_f16(CH(cache_k), CH(cache_v), block_table, kv_len, kv_heads, head_dim, block_size, H(k_out),
                             H(v_out), ST(stream));
}

int ferrum_hip_kv_move_blocks(const void* const* pools_dev, int num_pools, const uint32_t* pairs_dev, int num_pairs, void* staging_dev,
                              size_t chunk_bytes, int num_blocks, int mode, void* stream) {
    FH_REQUIRE(((uintptr_t)staging_dev & 15) == 0, "kv_move_blocks: staging buffer is not 16-byte aligned");
    return kv_move_blocks(const_cast<void* const*>(pools_dev), num_pools, pairs_dev, num_pairs, staging_dev, chunk_bytes, num_blocks, mode,
                          ST(stream));
}

// ── MoE routing ─────────────────────────────────────────────────────────────
int ferrum_hip_moe_route_topk_softmax_f16(const void* logits, int32_t* ids, float* w, int tokens, int num_experts,
                                          int top_k, int norm, void* stream) {
    return moe_route_topk_softmax_f16(CH(logits), ids, w, tokens, num_experts, top_k, norm, ST(stream));
}
int ferrum_hip_moe_route_topk_softmax_f32(const float* logits, int32_t* ids, float* w, int tokens, int num_experts,
                                          int top_k, int norm, void* stream) {
    return moe_route_topk_softmax_f32(logits, ids, w, tokens, num_experts, top_k, norm, ST(stream));
}
int ferrum_hip_moe_align_block_size(const int32_t* expert_ids, int32_t* sorted_token_ids, int32_t* block_ids,
                                    int32_t* total_post_pad, int batch_x_topk, int num_experts, int block_size,
                                    int sorted_max, void* stream) {
    FH_REQUIRE((expert_ids || batch_x_topk == 0) && sorted_token_ids && block_ids && total_post_pad, "moe_align_block_size: null buffer");
    return moe_align_block_size(expert_ids, sorted_token_ids, block_ids, total_post_pad, batch_x_topk, num_experts,
                                block_size, sorted_max, ST(stream));
}
int ferrum_hip_moe_combine_f16(const void* down, const float* weights, void* out, int tokens, int top_k, int hidden,
                               int accumulate, void* stream) {
    return moe_combine_f16(CH(down), weights, H(out), tokens, top_k, hidden, accumulate, ST(stream));
}

int ferrum_hip_moe_align_block_size_packed_rows(const int32_t* expert_ids, int32_t* sorted_token_ids, int32_t* block_ids,
                                                int32_t* total_post_pad, int batch_x_topk, int num_experts, int block_size,
                                                int sorted_max, void* stream) {
    FH_REQUIRE(batch_x_topk == 0 || (expert_ids && sorted_token_ids && block_ids && total_post_pad), "moe_align_block_size: null buffer");
    return moe_align_block_size_packed_rows(expert_ids, sorted_token_ids, block_ids, total_post_pad, batch_x_topk, num_experts,
                                            block_size, sorted_max, ST(stream));
}
int ferrum_hip_moe_build_pairs_by_token(const int32_t* expert_ids, int32_t* pairs_by_token, int32_t* packed_token_idx,
                                        int32_t* expert_offsets, int batch_x_topk, int num_experts, int top_k, void* stream) {
    FH_REQUIRE(expert_offsets && (batch_x_topk == 0 || (expert_ids && pairs_by_token && packed_token_idx)), "moe_build_pairs_by_token: null buffer");
    return moe_build_pairs_by_token(expert_ids, pairs_by_token, packed_token_idx, expert_offsets, batch_x_topk, num_experts, top_k,
                                    ST(stream));
}
int ferrum_hip_moe_combine_pairs_f16(const void* packed_down, const int32_t* pairs_by_token, const float* pair_weights, void* out,
                                     int batch, int hidden, int top_k, int total_pairs, void* stream) {
    FH_REQUIRE(batch == 0 || (packed_down && pairs_by_token && pair_weights && out), "moe_combine: null buffer");
    return moe_combine_pairs_f16(CH(packed_down), pairs_by_token, pair_weights, H(out), batch, hidden, top_k, total_pairs, ST(stream));
}
// weighted_sum_batched / weighted_sum_batched_offset (capabilities.rs:560-600): out[b, h] = Σ_k weights[b, k]·slots[b, k, h];
// offsets in ELEMENTS into `weights` (start of [batch, top_k]) and `out` (start of [batch, hidden]).
int ferrum_hip_weighted_sum_batched_f16(const void* slots, const float* weights, size_t weights_offset, void* out, size_t out_offset,
                                        int batch, int top_k, int hidden, void* stream) {
    FH_REQUIRE(batch == 0 || (slots && weights && out), "weighted_sum_batched: null buffer");
    FH_REQUIRE(out_offset % 8 == 0, "weighted_sum_batched: out_offset=%zu must be a multiple of 8 elements", out_offset);
    return moe_combine_f16(CH(slots), weights + weights_offset, H(out) + out_offset, batch, top_k, hidden, 0, ST(stream));
}

int ferrum_hip_fused_add_rms_norm_route_f16(void* residual, const void* x, const void* w, float eps, void* norm_out,
                                            const void* router_w, int num_experts, int top_k, int norm_topk_prob,
                                            int32_t* expert_ids, float* expert_weights, float* logits_out, int tokens,
                                            int hidden, void* stream) {
    FH_REQUIRE(tokens == 0 || (residual && x && w && norm_out), "fused_add_rms_norm_route: null buffer");
    FH_REQUIRE(num_experts == 0 || (router_w && expert_ids && expert_weights), "fused_add_rms_norm_route: null router buffers");
    return fused_add_rms_norm_route_f16(H(residual), CH(x), CH(w), eps, H(norm_out), CH(router_w), num_experts, top_k,
                                        norm_topk_prob, expert_ids, expert_weights, logits_out, tokens, hidden, ST(stream));
}
int ferrum_hip_moe_combine_add_rms_norm_f16(const void* down, const float* weights, void* residual,
                                            const void* next_norm_w, float eps, void* norm_out, int tokens, int top_k,
                                            int hidden, void* stream) {
    FH_REQUIRE(tokens == 0 || (down && weights && residual && (!next_norm_w || norm_out)), "moe_combine_add_rms_norm: null buffer");
    return moe_combine_add_rms_norm_f16(CH(down), weights, CH(residual), H(residual), CH(next_norm_w), eps, H(norm_out),
                                        tokens, top_k, hidden, ST(stream));
}

int ferrum_hip_fused_add_rms_norm_route_parts_f16(const void* residual_in, void* residual_out, const void* x_f16,
                                                  const float* x_slabs, int num_slabs, long slab_stride, int ld_slab,
                                                  const void* w, float eps, void* norm_out, const void* router_w_tiled,
                                                  int num_experts, int top_k, int num_parts, void* cand, float* stats,
                                                  float* logits_out, int tokens, int hidden, void* stream) {
    FH_REQUIRE(tokens == 0 || (residual_in && residual_out && w && norm_out && (x_f16 || x_slabs)), "route_parts: null buffer");
    FH_REQUIRE(num_experts == 0 || (router_w_tiled && cand && stats), "route_parts: null router buffers");
    return fused_add_rms_norm_route_parts_f16(CH(residual_in), H(residual_out), CH(x_f16), x_slabs, num_slabs, slab_stride,
                                              ld_slab, CH(w), eps, H(norm_out), CH(router_w_tiled), num_experts, top_k,
                                              num_parts, reinterpret_cast<RouteCand*>(cand), stats, logits_out, tokens, hidden,
                                              ST(stream));
}
int ferrum_hip_fused_add_rms_norm_route_split_f16(const void* residual_in, void* residual_out, const void* x_f16,
                                                  const float* x_slabs, int num_slabs, long slab_stride, int ld_slab,
                                                  const void* w, float eps, void* norm_out, const void* router_w_tiled,
                                                  int num_experts, int top_k, int norm_topk_prob, int num_parts,
                                                  void* cand, float* stats, uint32_t* arrive, int32_t* expert_ids,
                                                  float* expert_weights, float* logits_out, int tokens, int hidden,
                                                  void* stream) {
    FH_REQUIRE(tokens == 0 || (residual_in && residual_out && w && norm_out && (x_f16 || x_slabs)), "route_split: null buffer");
    FH_REQUIRE(num_experts == 0 || (router_w_tiled && cand && stats && arrive && expert_ids && expert_weights),
               "route_split: null router buffers");
    return fused_add_rms_norm_route_split_f16(CH(residual_in), H(residual_out), CH(x_f16), x_slabs, num_slabs, slab_stride,
                                              ld_slab, CH(w), eps, H(norm_out), CH(router_w_tiled), num_experts, top_k,
                                              num_parts, reinterpret_cast<RouteCand*>(cand), stats, arrive, norm_topk_prob,
                                              expert_ids, expert_weights, logits_out, tokens, hidden, ST(stream));
}

// ── sampling ────────────────────────────────────────────────────────────────
int ferrum_hip_argmax_rows_f16(const void* logits, uint32_t* out, const uint8_t* mask, int mask_len, int m, int n, void* stream) {
    return argmax_rows_f16(CH(logits), out, mask, mask_len, m, n, ST(stream));
}
int ferrum_hip_argmax_rows_f32(const float* logits, uint32_t* out, const uint8_t* mask, int mask_len, int m, int n, void* stream) {
    return argmax_rows_f32(logits, out, mask, mask_len, m, n, ST(stream));
}
int ferrum_hip_argmax_rows_f16_ws(const void* logits, uint32_t* out, const uint8_t* mask, int mask_len, int m, int n,
                                  FerrumHipWorkspace* ws, void* stream) {
    return argmax_rows_f16_ws(CH(logits), out, mask, mask_len, m, n, ws ? ws->ptr : nullptr, ws ? ws->bytes : 0, ST(stream));
}
int ferrum_hip_argmax_rows_f32_ws(const float* logits, uint32_t* out, const uint8_t* mask, int mask_len, int m, int n,
                                  FerrumHipWorkspace* ws, void* stream) {
    return argmax_rows_f32_ws(logits, out, mask, mask_len, m, n, ws ? ws->ptr : nullptr, ws ? ws->bytes : 0, ST(stream));
}
int ferrum_hip_apply_repetition_penalties_sparse_f16(void* logits, const uint32_t* row_offsets, const uint32_t* token_ids,
                                                     const float* penalties, int m, int n, void* stream) {
    return apply_repetition_penalties_sparse_f16(H(logits), row_offsets, token_ids, penalties, m, n, ST(stream));
}
int ferrum_hip_apply_repetition_penalties_sparse_f32(float* logits, const uint32_t* row_offsets, const uint32_t* token_ids,
                                                     const float* penalties, int m, int n, void* stream) {
    return apply_repetition_penalties_sparse_f32(logits, row_offsets, token_ids, penalties, m, n, ST(stream));
}

// ── BlockAllocator ──────────────────────────────────────────────────────────
struct FerrumHipBlockAllocator { fh::BlockAllocator impl; explicit FerrumHipBlockAllocator(uint32_t n) : impl(n) {} };

int ferrum_hip_block_allocator_create(FerrumHipBlockAllocator** a, uint32_t num_blocks) {
    FH_REQUIRE(a, "block_allocator_create: null output");
    *a = new FerrumHipBlockAllocator(num_blocks);
    return 0;
}
int ferrum_hip_block_allocator_destroy(FerrumHipBlockAllocator* a) { delete a; return 0; }
int ferrum_hip_block_allocator_allocate(FerrumHipBlockAllocator* a, uint32_t* block) {
    FH_REQUIRE(a && block, "block_allocator_allocate: null argument");
    if (!a->impl.allocate(block)) {
        fh::set_error("paged KV pool exhausted (capacity=%u blocks, all in use)", a->impl.capacity());
        return FERRUM_HIP_INVALID;
    }
    return 0;
}
int ferrum_hip_block_allocator_allocate_n(FerrumHipBlockAllocator* a, uint32_t n, uint32_t* blocks) {
    FH_REQUIRE(a && (n == 0 || blocks), "block_allocator_allocate_n: null argument");
    if (!a->impl.allocate_n(n, blocks)) {
        fh::set_error("paged KV pool exhausted: need %u blocks but only %u free", n, a->impl.free_count());
        return FERRUM_HIP_INVALID;
    }
    return 0;
}
int ferrum_hip_block_allocator_free(FerrumHipBlockAllocator* a, const uint32_t* blocks, uint32_t n) {
    FH_REQUIRE(a && (n == 0 || blocks), "block_allocator_free: null argument");
    // the reference indexes its ref-count vector (a bad id panics, paged_pool.rs:333-345): a bad id from the FFI side must
    // fail here, before anything is freed, instead of writing outside the vectors
    for (uint32_t i = 0; i < n; i++)
        FH_REQUIRE(blocks[i] < a->impl.capacity(), "block_allocator_free: block %u >= capacity %u", blocks[i], a->impl.capacity());
    a->impl.free(blocks, n);
    return 0;
}
int ferrum_hip_block_allocator_acquire(FerrumHipBlockAllocator* a, uint32_t block) {
    FH_REQUIRE(a, "block_allocator_acquire: null");
    FH_REQUIRE(block < a->impl.capacity(), "block_allocator_acquire: block %u >= capacity %u", block, a->impl.capacity());
    // paged_pool.rs acquire: checked_add on the ref count (panics on overflow) — here: an error, the count is left alone
    FH_REQUIRE(a->impl.ref_count(block) < 0xFFFFu, "block_allocator_acquire: ref count of block %u would overflow", block);
    a->impl.acquire(block);
    return 0;
}
int ferrum_hip_block_allocator_register_hash(FerrumHipBlockAllocator* a, uint32_t block, uint64_t hash) {
    FH_REQUIRE(a, "block_allocator_register_hash: null");
    FH_REQUIRE(block < a->impl.capacity(), "block_allocator_register_hash: block %u >= capacity %u", block, a->impl.capacity());
    a->impl.register_block_hash(block, hash);
    return 0;
}
int ferrum_hip_block_allocator_try_acquire_by_hash(FerrumHipBlockAllocator* a, uint64_t hash, int64_t* block) {
    FH_REQUIRE(a && block, "block_allocator_try_acquire_by_hash: null");
    *block = a->impl.try_acquire_by_hash(hash);
    return 0;
}
uint32_t ferrum_hip_block_allocator_free_count(const FerrumHipBlockAllocator* a) { return a->impl.free_count(); }
uint32_t ferrum_hip_block_allocator_ref_count(const FerrumHipBlockAllocator* a, uint32_t b) { return b < a->impl.capacity() ? a->impl.ref_count(b) : 0; }
uint32_t ferrum_hip_block_allocator_peak_in_use(const FerrumHipBlockAllocator* a) { return a->impl.peak_in_use(); }
uint32_t ferrum_hip_block_allocator_hash_table_size(const FerrumHipBlockAllocator* a) { return a->impl.hash_table_size(); }

}  // extern "C"
