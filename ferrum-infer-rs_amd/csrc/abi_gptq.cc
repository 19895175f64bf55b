// The GPTQ / expert-stack handle of the C ABI (include/ferrum_hip.h): loaders, the dense INT4 linear entries and every
// ferrum_hip_moe_gemm_phase_* entry.  Host-only code; compiled with hipcc.  The rest of the ABI is abi.cc.
#include "../../include/ferrum_hip.h"
#include "abi_private.h"
#include "common.h"
#include "kernels.h"
#include "moe_dispatch_plan.h"
#include "w4_upload.h"

using namespace fh;

struct FerrumHipGptq {
    W4Device dev;
    bool symmetric = true;
    __half* gather_scratch = nullptr;   // act-order input gather buffer [m_cap, K]
    int gather_rows = 0;
    std::vector<void*> retired_scratch;  // outgrown gather buffers: a graph captured earlier may still hold them → freed with the handle
    // gemm_phase_batched: rotating (pinned host, device, event) slots for the per-call dispatch arrays
    struct DispatchSlot { int32_t* host = nullptr; int32_t* dev = nullptr; size_t cap = 0; hipEvent_t done = nullptr; };
    DispatchSlot slots[4];
    int next_slot = 0;
    // expert_major_pair: [2][E] arrival counters + the give-up word of the merged gate_up → down launch
    unsigned* pair_arrive = nullptr;
    int pair_experts = 0;
    bool shape_only = false;            // ferrum_hip_gptq_shape_only: k / n / G and nothing on the device
};

namespace fh {
const W4Device* gptq_device(const FerrumHipGptq* h) { return &h->dev; }
bool gptq_is_shape_only(const FerrumHipGptq* h) { return h->shape_only; }
}

// Every entry that computes passes its handle(s) through this, behind its null check: a handle made by
// ferrum_hip_gptq_shape_only (or one whose upload never happened) has nothing a kernel could read.
#define FH_REQUIRE_WEIGHTS(h, what) \
    FH_REQUIRE(!(h)->shape_only && ((h)->dev.qw || (h)->dev.f16t), what ": the handle carries no weights (shape-only)")

extern "C" {

// ── GPTQ ────────────────────────────────────────────────────────────────────
static int check_gptq_args(int bits, int group_size, int k, int n) {
    if (bits != 4) { fh::set_error("gptq: only bits=4 supported (got %d)", bits); return FERRUM_HIP_UNSUPPORTED; }
    if (k <= 0 || n <= 0 || k % 128 != 0 || n % 8 != 0) {
        fh::set_error("gptq: unsupported shape K=%d N=%d (K %% 128, N %% 8 required)", k, n);
        return FERRUM_HIP_UNSUPPORTED;
    }
    if (group_size <= 0 || group_size % 128 != 0 || k % group_size != 0) {
        fh::set_error("gptq: unsupported group_size=%d for K=%d (multiple of 128 required)", group_size, k);
        return FERRUM_HIP_UNSUPPORTED;
    }
    return 0;
}

static int upload_bias(const float* bias, int n, __half** dev) {
    std::vector<uint16_t> bh(n);
    for (int i = 0; i < n; i++) { _Float16 h = (_Float16)bias[i]; memcpy(&bh[i], &h, 2); }
    FH_CHECK_HIP(hipMalloc((void**)dev, bh.size() * 2));
    FH_CHECK_HIP(hipMemcpy(*dev, bh.data(), bh.size() * 2, hipMemcpyHostToDevice));
    return 0;
}

int ferrum_hip_gptq_load(FerrumHipGptq** handle, const int32_t* qweight, const float* scales, const int32_t* qzeros,
                         const int32_t* g_idx, const float* bias, int bits, int group_size, int k, int n) {
    FH_REQUIRE(handle && qweight && scales && qzeros, "gptq_load: null argument");
    if (int rc = check_gptq_args(bits, group_size, k, n)) return rc;
    W4HostPacked hp;
    if (int rc = w4_repack_host(qweight, scales, qzeros, g_idx, nullptr, group_size, k, n, &hp)) return rc;
    auto* g = new FerrumHipGptq();
    g->symmetric = hp.symmetric;
    int rc = w4_upload(hp, &g->dev);
    if (!rc && bias) rc = upload_bias(bias, n, &g->dev.bias);
    if (rc) { ferrum_hip_gptq_free(g); return rc; }
    *handle = g;
    return 0;
}

int ferrum_hip_gptq_load_stacked(FerrumHipGptq** handle, const int32_t* const* qweights, const float* const* scales,
                                 const int32_t* const* qzeros, const int32_t* g_idx, int bits, int group_size, int k,
                                 int n_per_expert, int num_experts, int fuse_gate_up) {
    FH_REQUIRE(handle && qweights && scales && qzeros && num_experts > 0, "gptq_load_stacked: null argument");
    if (int rc = check_gptq_args(bits, group_size, k, n_per_expert)) return rc;
    const int n = n_per_expert;
    std::vector<int32_t> col_perm;
    if (fuse_gate_up) {
        if (n % 64 != 0) { fh::set_error("gptq_load_stacked: fused gate_up needs N %% 64 == 0 (N=%d)", n); return FERRUM_HIP_UNSUPPORTED; }
        col_perm = gate_up_col_perm(n);
    }
    auto* g = new FerrumHipGptq();
    int rc = w4_stack_reserve(&g->dev, k, n, num_experts, fuse_gate_up != 0);
    for (int e = 0; e < num_experts && !rc; e++) {
        // one g_idx for the whole stack (capabilities.rs:180-189; cuda/quant.rs:862 ff. samples expert 0's): act-order rows
        // are packed in sorted-group order and the phase entry points gather the input columns to match
        W4HostPacked hp;
        rc = w4_repack_host(qweights[e], scales[e], qzeros[e], g_idx, fuse_gate_up ? col_perm.data() : nullptr, group_size, k, n, &hp);
        if (!rc && e == 0 && !hp.perm.empty()) rc = w4_upload_perm(hp.perm, &g->dev);
        if (!rc) rc = w4_stack_put(&g->dev, e, hp);
    }
    if (rc) { ferrum_hip_gptq_free(g); return rc; }
    g->symmetric = g->dev.zp == nullptr;
    *handle = g;
    return 0;
}

// A handle that carries a projection's dims and no weights (no device call): what the shape predicates
// (ferrum_hip_decode_chain_supports) are asked with before weights exist.  num_experts is 0 and the weight pointer null; every
// entry that computes refuses it by name (FH_REQUIRE_WEIGHTS), the stack entries included.
int ferrum_hip_gptq_shape_only(FerrumHipGptq** handle, int group_size, int k, int n) {
    FH_REQUIRE(handle, "gptq_shape_only: null argument");
    if (int rc = check_gptq_args(4, group_size, k, n)) return rc;
    auto* g = new FerrumHipGptq();
    g->dev.k = k; g->dev.n = n; g->dev.n64 = (n + 63) / 64; g->dev.G = k / 128;
    g->dev.num_experts = 0;
    g->shape_only = true;
    *handle = g;
    return 0;
}

// Act-order weights: the entry points read gathered input rows x'[r][j] = x[r][perm[j]] (`rows` input rows of K columns;
// cuda/quant.rs:434).  The scratch grows outside of graph capture only (first call with more rows); an outgrown buffer stays
// alive with the handle, because a graph captured at the smaller size holds its address.
static int gathered_input(const FerrumHipGptq* handle, const void* input, int rows, hipStream_t s, const __half** x) {
    *x = CH(input);
    if (!handle->dev.perm || rows <= 0) return 0;
    auto* g = const_cast<FerrumHipGptq*>(handle);
    if (g->gather_rows < rows) {
        if (g->gather_scratch) g->retired_scratch.push_back(g->gather_scratch);
        g->gather_scratch = nullptr;
        FH_CHECK_HIP(hipMalloc((void**)&g->gather_scratch, (size_t)rows * g->dev.k * 2));
        g->gather_rows = rows;
    }
    if (int rc = gather_columns_f16(CH(input), g->dev.perm, g->gather_scratch, rows, g->dev.k, s)) return rc;
    *x = g->gather_scratch;
    return 0;
}
static inline int input_rows(int prob_m, int top_k) { return (prob_m + top_k - 1) / top_k; }      // pair p reads row p / top_k

int ferrum_hip_gptq_free(FerrumHipGptq* g) {
    if (!g) return 0;
    w4_free(g->dev);
    if (g->gather_scratch) (void)hipFree(g->gather_scratch);
    for (void* p : g->retired_scratch) (void)hipFree(p);
    if (g->pair_arrive) (void)hipFree(g->pair_arrive);
    for (auto& sl : g->slots) {
        if (sl.done) { (void)hipEventSynchronize(sl.done); (void)hipEventDestroy(sl.done); }
        if (sl.host) (void)hipHostFree(sl.host);
        if (sl.dev) (void)hipFree(sl.dev);
    }
    delete g;
    return 0;
}

int ferrum_hip_gptq_info(const FerrumHipGptq* g, int* k, int* n, int* num_experts, int* symmetric) {
    FH_REQUIRE(g, "gptq_info: null handle");
    if (k) *k = g->dev.k;
    if (n) *n = g->dev.n;
    if (num_experts) *num_experts = g->dev.num_experts;
    if (symmetric) *symmetric = g->symmetric ? 1 : 0;
    return 0;
}

int ferrum_hip_gptq_linear_forward_f16(const FerrumHipGptq* handle, const void* in, void* out, int m,
                                       FerrumHipWorkspace* ws, void* stream) {
    FH_REQUIRE(handle && (m == 0 || (in && out)), "gptq_linear_forward: null argument");
    FH_REQUIRE_WEIGHTS(handle, "gptq_linear_forward");
    FH_REQUIRE(handle->dev.num_experts == 1, "gptq_linear_forward: handle is an expert stack");
    const __half* x = nullptr;
    if (int rc = gathered_input(handle, in, m, ST(stream), &x)) return rc;
    // the bias (if any) is added in the GEMM epilogue / split-K reduce (W4Device::bias)
    return w4_gemm_dense(handle->dev, x, H(out), m, ws ? ws->ptr : nullptr, ws ? ws->bytes : 0, ST(stream));
}

// op-level entries of the forms only the runner reaches: the fp32 slab producers and the fused combine + add + norm prologue
int ferrum_hip_gptq_linear_slabs_f16(const FerrumHipGptq* handle, const void* x, float* slabs, size_t slab_bytes, int m, int form,
                                     int* S_inout, int* rows_pad_out, int* n_pad_out, void* stream) {
    FH_REQUIRE(handle && S_inout && rows_pad_out && n_pad_out && (m == 0 || (x && slabs)), "gptq_linear_slabs: null argument");
    FH_REQUIRE(form >= 0 && form <= 2, "gptq_linear_slabs: unknown form %d (0 skinny, 1 LDS-shared activations, 2 64-row tiles)", form);
    FH_REQUIRE_WEIGHTS(handle, "gptq_linear_slabs");
    const W4Device& w = handle->dev;
    FH_REQUIRE(w.num_experts == 1 && w.qw && !w.f16t, "gptq_linear_slabs: handle is not a single INT4 projection");
    FH_REQUIRE(!w.perm, "gptq_linear_slabs: act-order weights (the runner's producers write the gathered rows themselves)");
    if (form == 0) {
        const int S = std::max(1, std::min(*S_inout, w.G));       // the clamp w4_gemm_dense_slabs applies
        if (int rc = w4_gemm_dense_slabs(w, CH(x), slabs, slab_bytes, m, S, rows_pad_out, n_pad_out, ST(stream))) return rc;
        *S_inout = S;
        return 0;
    }
    if (form == 1) return w4_gemm_dense_slabs_lds(w, CH(x), slabs, slab_bytes, m, S_inout, rows_pad_out, n_pad_out, ST(stream));
    return w4_gemm_dense_slabs_tile(w, CH(x), slabs, slab_bytes, m, S_inout, rows_pad_out, n_pad_out, ST(stream));
}

int ferrum_hip_gptq_linear_forward_fused_tail_f16(const FerrumHipGptq* handle, const void* down, const float* weights,
                                                  const void* residual_in, void* residual_out, const void* ln_w, float eps, int top_k,
                                                  void* out, int m, FerrumHipWorkspace* ws, void* stream) {
    FH_REQUIRE(handle && (m == 0 || (down && weights && residual_in && residual_out && ln_w && out)), "gptq_linear_forward_fused_tail: null argument");
    FH_REQUIRE(m == 0 || residual_in != residual_out, "gptq_linear_forward_fused_tail: residual_in == residual_out (every workgroup reads, one writes)");
    FH_REQUIRE_WEIGHTS(handle, "gptq_linear_forward_fused_tail");
    FH_REQUIRE(handle->dev.num_experts == 1, "gptq_linear_forward_fused_tail: handle is an expert stack");
    const FusedCombineNorm fa{CH(down), weights, CH(residual_in), H(residual_out), CH(ln_w), eps, top_k};
    return w4_gemm_dense(handle->dev, nullptr, H(out), m, ws ? ws->ptr : nullptr, ws ? ws->bytes : 0, ST(stream), &fa);
}

int ferrum_hip_gptq_linear_can_fuse_tail(const FerrumHipGptq* handle, int m) {
    return handle && !handle->shape_only && handle->dev.num_experts == 1 && w4_gemm_dense_can_fuse_combine_norm(handle->dev, m) ? 1 : 0;
}

int ferrum_hip_moe_gemm_phase_f16(const FerrumHipGptq* stack, const void* input, const int32_t* sorted_token_ids,
                                  const int32_t* expert_ids, const int32_t* num_tokens_past_padded, void* output,
                                  int prob_m, int moe_block_size, int top_k, int max_blocks, int fused_silu_mul,
                                  void* stream) {
    FH_REQUIRE(stack && input && sorted_token_ids && expert_ids && num_tokens_past_padded && output,
               "moe_gemm_phase: null argument");
    FH_REQUIRE_WEIGHTS(stack, "moe_gemm_phase");
    if (moe_block_size != 16 && moe_block_size != 32 && moe_block_size != 64 && moe_block_size != 96 && moe_block_size != 128) {
        fh::set_error("moe_gemm_phase: moe_block_size=%d unsupported (16, 32, 64, 96 or 128)", moe_block_size);
        return FERRUM_HIP_UNSUPPORTED;
    }
    if (moe_block_size >= 96 && stack->dev.G % 2 != 0) {
        fh::set_error("moe_gemm_phase: 96- / 128-row blocks need an even number of 128-wide quant groups (K=%d)", stack->dev.k);
        return FERRUM_HIP_UNSUPPORTED;
    }
    FH_REQUIRE(top_k >= 1, "moe_gemm_phase: top_k=%d", top_k);
    FH_REQUIRE(!fused_silu_mul || stack->dev.fused_gate_up, "moe_gemm_phase: fused epilogue needs a stack loaded with fuse_gate_up");
    FH_REQUIRE(fused_silu_mul || !stack->dev.fused_gate_up, "moe_gemm_phase: stack was loaded with fuse_gate_up; plain output is column-permuted");
    const __half* x = nullptr;
    if (int rc = gathered_input(stack, input, input_rows(prob_m, top_k), ST(stream), &x)) return rc;
    if (moe_block_size >= 32)   // prefill-sized batches: 128-, 64- or 32-row LDS tiles
        return w4_gemm_moe_tile(stack->dev, x, H(output), sorted_token_ids, expert_ids, num_tokens_past_padded, prob_m,
                                max_blocks, moe_block_size, top_k, fused_silu_mul, ST(stream));
    return w4_gemm_moe(stack->dev, x, H(output), sorted_token_ids, expert_ids, num_tokens_past_padded, prob_m,
                       max_blocks, top_k, fused_silu_mul, ST(stream));
}

int ferrum_hip_moe_gemm_phase_inline_align_f16(const FerrumHipGptq* stack, const void* input,
                                               const int32_t* expert_ids_per_pair, void* output, int prob_m,
                                               int num_experts, int top_k, int max_blocks, int fused_silu_mul,
                                               void* stream) {
    FH_REQUIRE(stack && input && expert_ids_per_pair && output, "moe_gemm_phase_inline_align: null argument");
    FH_REQUIRE_WEIGHTS(stack, "moe_gemm_phase_inline_align");
    FH_REQUIRE(top_k >= 1, "moe_gemm_phase_inline_align: top_k=%d", top_k);
    FH_REQUIRE(!fused_silu_mul || stack->dev.fused_gate_up, "moe_gemm_phase_inline_align: fused epilogue needs a stack loaded with fuse_gate_up");
    FH_REQUIRE(fused_silu_mul || !stack->dev.fused_gate_up, "moe_gemm_phase_inline_align: stack was loaded with fuse_gate_up; plain output is column-permuted");
    if (prob_m > 1024) { fh::set_error("moe_gemm_phase_inline_align: prob_m=%d > 1024 (use moe_align_block_size + moe_gemm_phase)", prob_m); return FERRUM_HIP_UNSUPPORTED; }
    const __half* x = nullptr;
    if (int rc = gathered_input(stack, input, input_rows(prob_m, top_k), ST(stream), &x)) return rc;
    return w4_gemm_moe_inline_align(stack->dev, x, H(output), expert_ids_per_pair, num_experts, prob_m, max_blocks,
                                    top_k, fused_silu_mul, nullptr, nullptr, nullptr, ST(stream));
}

int ferrum_hip_moe_gemm_phase_expert_major_f16(const FerrumHipGptq* stack, const void* input,
                                               const int32_t* expert_ids_per_pair, void* output, int prob_m,
                                               int num_experts, int top_k, int fused_silu_mul, void* stream) {
    FH_REQUIRE(stack && input && expert_ids_per_pair && output, "moe_gemm_phase_expert_major: null argument");
    FH_REQUIRE_WEIGHTS(stack, "moe_gemm_phase_expert_major");
    FH_REQUIRE(top_k >= 1 && num_experts >= 1, "moe_gemm_phase_expert_major: top_k=%d num_experts=%d", top_k, num_experts);
    FH_REQUIRE(!fused_silu_mul || stack->dev.fused_gate_up, "moe_gemm_phase_expert_major: fused epilogue needs a stack loaded with fuse_gate_up");
    FH_REQUIRE(fused_silu_mul || !stack->dev.fused_gate_up, "moe_gemm_phase_expert_major: stack was loaded with fuse_gate_up; plain output is column-permuted");
    if (prob_m > 1024) { fh::set_error("moe_gemm_phase_expert_major: prob_m=%d > 1024 (use moe_align_block_size + moe_gemm_phase)", prob_m); return FERRUM_HIP_UNSUPPORTED; }
    const __half* x = nullptr;
    if (int rc = gathered_input(stack, input, input_rows(prob_m, top_k), ST(stream), &x)) return rc;
    return w4_gemm_moe_expert_major(stack->dev, x, H(output), expert_ids_per_pair, num_experts, prob_m, top_k,
                                    fused_silu_mul, ST(stream));
}

int ferrum_hip_moe_gemm_phase_expert_major_pair_f16(FerrumHipGptq* gate_up_stack, const FerrumHipGptq* down_stack, const void* input,
                                                    const int32_t* expert_ids_per_pair, void* act_out, void* output, int prob_m,
                                                    int num_experts, int top_k, void* stream) {
    FH_REQUIRE(gate_up_stack && down_stack && input && expert_ids_per_pair && act_out && output, "moe_gemm_phase_expert_major_pair: null argument");
    FH_REQUIRE_WEIGHTS(gate_up_stack, "moe_gemm_phase_expert_major_pair");
    FH_REQUIRE_WEIGHTS(down_stack, "moe_gemm_phase_expert_major_pair");
    FH_REQUIRE(top_k >= 1 && num_experts >= 1, "moe_gemm_phase_expert_major_pair: top_k=%d num_experts=%d", top_k, num_experts);
    FH_REQUIRE(gate_up_stack->dev.fused_gate_up && !down_stack->dev.fused_gate_up,
               "moe_gemm_phase_expert_major_pair: gate_up stack must be loaded with fuse_gate_up, the down stack without");
    if (prob_m > 1024) { fh::set_error("moe_gemm_phase_expert_major_pair: prob_m=%d > 1024", prob_m); return FERRUM_HIP_UNSUPPORTED; }
    if (down_stack->dev.perm) {       // the gated activations would need a gather between the two GEMMs of the launch
        fh::set_error("moe_gemm_phase_expert_major_pair: act-order down stack (run the two phases separately)");
        return FERRUM_HIP_UNSUPPORTED;
    }
    const __half* x_in = nullptr;
    if (int rc = gathered_input(gate_up_stack, input, input_rows(prob_m, top_k), ST(stream), &x_in)) return rc;
    FerrumHipGptq* g = gate_up_stack;
    if (g->pair_experts < num_experts) {
        // (a captured graph may still hold the old counters: retired with the handle, like outgrown gather buffers)
        if (g->pair_arrive) g->retired_scratch.push_back(g->pair_arrive);
        g->pair_arrive = nullptr;
        const size_t words = (size_t)2 * num_experts * MOE_PAIR_COUNTER_STRIDE + 4;
        FH_CHECK_HIP(hipMalloc((void**)&g->pair_arrive, words * sizeof(unsigned)));
        FH_CHECK_HIP(hipMemset(g->pair_arrive, 0, words * sizeof(unsigned)));
        g->pair_experts = num_experts;
    }
    // op level: the counters are zeroed by a memset node in front of every launch (a captured call replays with the same
    // pointers, so the runner's alternating halves do not apply); the give-up word is checked by ferrum_hip_moe_pair_status
    unsigned* arrive = g->pair_arrive;
    const size_t half = (size_t)g->pair_experts * MOE_PAIR_COUNTER_STRIDE;
    FH_CHECK_HIP(hipMemsetAsync(arrive, 0, half * sizeof(unsigned), ST(stream)));
    int took = 0;
    if (int rc = w4_gemm_moe_expert_major_pair(g->dev, down_stack->dev, x_in, H(act_out), H(output), expert_ids_per_pair, num_experts,
                                               prob_m, top_k, arrive, arrive + half, arrive + 2 * half, &took, ST(stream)))
        return rc;
    if (!took) { fh::set_error("moe_gemm_phase_expert_major_pair: shapes not taken by the merged form"); return FERRUM_HIP_UNSUPPORTED; }
    return 0;
}

/* number of in-launch waits of the stack's merged launches that gave up so far (0 = every hand-off completed) */
int ferrum_hip_moe_pair_status(const FerrumHipGptq* gate_up_stack, unsigned* timeouts) {
    FH_REQUIRE(gate_up_stack && timeouts, "moe_pair_status: null argument");
    *timeouts = 0;
    if (!gate_up_stack->pair_arrive) return 0;
    FH_CHECK_HIP(hipMemcpy(timeouts, gate_up_stack->pair_arrive + 2 * (size_t)gate_up_stack->pair_experts * MOE_PAIR_COUNTER_STRIDE, sizeof(unsigned), hipMemcpyDeviceToHost));
    return 0;
}

int ferrum_hip_moe_gemm_phase_merge_route_f16(const FerrumHipGptq* stack, const void* input, const void* cand,
                                              const float* stats, void* output, int tokens, int num_parts, int top_k,
                                              int norm_topk_prob, int num_experts, int max_blocks, int fused_silu_mul,
                                              int32_t* expert_ids_out, float* expert_weights_out,
                                              int32_t* sorted_token_ids_out, int32_t* block_ids_out,
                                              int32_t* total_post_pad_out, void* stream) {
    FH_REQUIRE(stack && input && cand && stats && output && expert_ids_out && expert_weights_out, "merge_route: null argument");
    FH_REQUIRE_WEIGHTS(stack, "merge_route");
    FH_REQUIRE(!fused_silu_mul || stack->dev.fused_gate_up, "merge_route: fused epilogue needs a stack loaded with fuse_gate_up");
    FH_REQUIRE(fused_silu_mul || !stack->dev.fused_gate_up, "merge_route: stack was loaded with fuse_gate_up; plain output is column-permuted");
    const __half* x_in = nullptr;
    if (int rc = gathered_input(stack, input, tokens, ST(stream), &x_in)) return rc;
    return w4_gemm_moe_merge_route(stack->dev, x_in, H(output), reinterpret_cast<const RouteCand*>(cand), stats, tokens,
                                   num_parts, top_k, norm_topk_prob, num_experts, max_blocks, fused_silu_mul, expert_ids_out,
                                   expert_weights_out, sorted_token_ids_out, block_ids_out, total_post_pad_out, ST(stream));
}

// MarlinExpertStack::gemm_phase_batched (marlin_expert_stack.rs:63-74): dispatches[i] = (expert, in_row_offset,
// out_row_offset, m); rows [in_off, in_off + m) of `input` × tile[expert] → rows [out_off, out_off + m) of `output`.
// One grouped launch per planned group (moe_dispatch_plan.h); the routing arrays travel through rotating pinned slots.
int ferrum_hip_moe_gemm_phase_batched_f16(FerrumHipGptq* stack, const void* input, const int32_t* dispatches, int num_dispatches,
                                          void* output, int k, int fused_silu_mul, void* stream) {
    FH_REQUIRE(stack && (num_dispatches == 0 || (input && dispatches && output)), "gemm_phase_batched: null argument");
    FH_REQUIRE_WEIGHTS(stack, "gemm_phase_batched");
    FH_REQUIRE(k == stack->dev.k, "gemm_phase_batched: k=%d but the stack was packed with K=%d", k, stack->dev.k);
    FH_REQUIRE(!fused_silu_mul || stack->dev.fused_gate_up, "gemm_phase_batched: fused epilogue needs a stack loaded with fuse_gate_up");
    FH_REQUIRE(fused_silu_mul || !stack->dev.fused_gate_up, "gemm_phase_batched: stack was loaded with fuse_gate_up; plain output is column-permuted");
    if (num_dispatches <= 0) return 0;
    BatchedDispatchPlan plan;
    if (int rc = plan_batched_dispatch(dispatches, num_dispatches, stack->dev.num_experts, &plan)) return rc;
    if (plan.rows == 0) return 0;
    const int br = plan.br;
    const long max_row = plan.max_row;
    const int ldo = fused_silu_mul ? stack->dev.n / 2 : stack->dev.n;
    const __half* x_in = nullptr;
    if (int rc = gathered_input(stack, input, (int)max_row, ST(stream), &x_in)) return rc;
    for (const BatchedDispatchPlan::Group& grp : plan.groups) {
        const std::vector<int32_t>& sorted = grp.sorted;
        const std::vector<int32_t>& blocks = grp.blocks;
        const long dl = grp.delta;
        const size_t nb = blocks.size(), need = sorted.size() + nb + 4;
        FerrumHipGptq::DispatchSlot& sl = stack->slots[stack->next_slot];
        stack->next_slot = (stack->next_slot + 1) % 4;
        if (sl.done) FH_CHECK_HIP(hipEventSynchronize(sl.done));      // the launch that last used this slot has consumed it
        else FH_CHECK_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
        if (sl.cap < need) {
            if (sl.host) (void)hipHostFree(sl.host);
            if (sl.dev) (void)hipFree(sl.dev);
            sl.host = nullptr; sl.dev = nullptr; sl.cap = 0;
            FH_CHECK_HIP(hipHostMalloc((void**)&sl.host, need * 2 * 4, hipHostMallocDefault));
            FH_CHECK_HIP(hipMalloc((void**)&sl.dev, need * 2 * 4));
            sl.cap = need * 2;
        }
        memcpy(sl.host, sorted.data(), sorted.size() * 4);
        memcpy(sl.host + sorted.size(), blocks.data(), nb * 4);
        sl.host[sorted.size() + nb] = (int32_t)sorted.size();           // total_tokens_post_pad
        FH_CHECK_HIP(hipMemcpyAsync(sl.dev, sl.host, need * 4, hipMemcpyHostToDevice, ST(stream)));
        const int32_t* d_sorted = sl.dev;
        const int32_t* d_blocks = sl.dev + sorted.size();
        const int32_t* d_total = sl.dev + sorted.size() + nb;
        __half* out_shift = H(output) + dl * ldo;                        // row (in_off + r) of the shifted view = out_off + r
        int rc = br == 64 ? w4_gemm_moe_tile(stack->dev, x_in, out_shift, d_sorted, d_blocks, d_total, (int)max_row, (int)nb, 64, 1,
                                             fused_silu_mul, ST(stream))
                          : w4_gemm_moe(stack->dev, x_in, out_shift, d_sorted, d_blocks, d_total, (int)max_row, (int)nb, 1,
                                        fused_silu_mul, ST(stream));
        if (rc) return rc;
        FH_CHECK_HIP(hipEventRecord(sl.done, ST(stream)));
    }
    return 0;
}

}  // extern "C"
