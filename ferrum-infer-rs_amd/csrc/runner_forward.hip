// Decoder runner, the forward itself: one unified prefill + decode forward enqueued on the model's stream.
//
// Op order per layer follows the reference's unified forward
//   LlamaFamilyModel::unified_forward_layer (ferrum-models/src/models/llama_family_forward_batched.rs:2625-3090)
//   Qwen3MoeModel::unified_forward_layer    (models/qwen3_moe_forward_unified_layer.rs:46-455)
//   moe_forward_bucketed                    (moe/dispatch.rs:1558-2192)
// and the drivers unified_forward_internal (models/qwen3_moe_forward_unified.rs:174-445):
//   embed → L × { rms_norm → qkv → split/qk-norm/rope/paged-write → paged attention → o_proj →
//   fused_add_rms_norm → [gate_up → act·mul → down | router → top-k → align → grouped gate_up(+silu·mul)
//   → grouped down → combine] → residual add } → final rms_norm (sampled rows) → lm_head → argmax.
#include "runner.h"
#include "knobs.h"

using namespace fh;

#define FH_TRY(call) do { if (int rc_ = (call)) return rc_; } while (0)

// Dense projection of the runner: act-order (desc_act) weights were repacked with their rows sorted by group, so the
// input columns are gathered with the same permutation first (like the op-level ferrum_hip_gptq_linear_forward_f16).
// gate_up (+silu·mul) and down grouped GEMMs of a decode-sized batch (P ≤ 1024 pairs) straight from expert_ids:
// expert-major when most experts are routed to (no align at all), else block-major with the align computed inside gate_up.
// Under expert parallelism the kernels see the rank's own experts only: local ids (−1 = another rank's expert, ignored by
// every form) and the local expert count.
const int32_t* fh::moe_ids(const FerrumHipModel* m) { return m->cfg.expert_parallel ? m->expert_ids_local : m->expert_ids; }

// Σ_e ceil(cnt_e/16) ≤ P/16 + min(P, E): the grid of 16-row blocks covers every block that can exist
int fh::moe_max_blocks(int P, int E) { return std::min((P + E * 16) / 16, P / 16 + std::min(P, E)); }
// the expert-major threshold compares pairs per expert: P pairs over num_experts, whatever share of them is local
bool fh::moe_expert_major(const FerrumHipModel* m, int P) {
    return m->moe_em_min_pairs_x8 > 0 && 8L * P >= (long)m->moe_em_min_pairs_x8 * m->cfg.num_experts;
}
// one half of the double-buffered arrival counters of the merged launches (layout: model_finalize)
unsigned* fh::arrive_half(const FerrumHipModel* m, int parity) { return m->em2_arrive + (size_t)parity * m->arrive_half_words; }

// Inputs of the two grouped GEMMs.  Act-order (desc_act) expert stacks read x'[j] = x[perm[j]] (the packed rows are in sorted-g_idx
// order): the normalised rows / the gated activations are gathered by a launch in front of the GEMM (one per act-order stack and
// layer: kernels/gather_columns.cu:15 in the reference sits in front of every Marlin call).  Natural-order stacks: no launch.
static int moe_gate_up_input(FerrumHipModel* m, LayerWeights& L, int T, hipStream_t s, const __half** x) {
    *x = m->norm_out;
    if (!L.exp_gate_up.perm) return 0;
    FH_REQUIRE(m->moe_gather_x, "MoE act-order gate_up stack without gather scratch");
    if (int rc = gather_columns_f16(m->norm_out, L.exp_gate_up.perm, m->moe_gather_x, T, L.exp_gate_up.k, s)) return rc;
    *x = m->moe_gather_x;
    return 0;
}
static int moe_down_input(FerrumHipModel* m, LayerWeights& L, int P, hipStream_t s, const __half** h) {
    *h = m->moe_act;
    if (!L.exp_down.perm) return 0;
    FH_REQUIRE(m->moe_gather_h, "MoE act-order down stack without gather scratch");
    if (int rc = gather_columns_f16(m->moe_act, L.exp_down.perm, m->moe_gather_h, P, L.exp_down.k, s)) return rc;
    *h = m->moe_gather_h;
    return 0;
}

// `route` (decode chain with a deferred merge): the routing arrives as per-part candidate lists; only forms that merge them in
// their own prologue may run (moe_deferred_merge_ok decides that BEFORE the chain launch).
static bool moe_pair_form(const FerrumHipModel* m, const LayerWeights& L, int P) {
    return moe_expert_major(m, P) && knobs().moe_em2 && m->em2_arrive && !m->em2_failed && !L.exp_down.perm;
}
static bool moe_deferred_merge_ok(const FerrumHipModel* m, const LayerWeights& L, int T, int Q) {
    if (!knobs().moe_deferred_merge || m->cfg.expert_parallel || Q < 2 || Q > 4 || m->cfg.top_k > 8) return false;
    if ((long)T * Q > MOE_ROUTE_LIST_CAPACITY) return false;
    const int P = T * m->cfg.top_k;
    // few pairs (block-major grid): every workgroup runs the full merge + align on a few hundred bytes of lists
    // (only where the gate_up launch is the K-split form — ≤ 16 pairs, c ≤ 2: c = 1 1.99 → 1.88 ms per step, c = 2 2.16 → 2.03.
    // In the one-wave-per-tile form every one of the ≈ 770 workgroups at c = 4 pays the merge: its launch 13.5 → 17.3 µs against
    // 2.9 µs saved in the chain; at c = 8 2.89 → 3.03 ms per step)
    return P <= std::min(knobs().moe_kw_pairs, 64) && T <= 4 && !moe_pair_form(m, L, P);
}

// router parts per token (the chain's role B, the split route kernel)
int fh::chain_route_parts(const FerrumHipModel* m) {
    if (m->cfg.num_experts <= 0) return 1;
    int Q = m->route_parts;
    const int tiles = (m->cfg.num_experts + 15) / 16;
    while (Q > 1 && (tiles % Q != 0 || Q > 8)) Q >>= 1;
    return Q;
}
// the router's candidate lists of T tokens in Q parts, as the runner's buffers hold them
MoeRouteLists fh::route_lists(const FerrumHipModel* m, int T, int Q) {
    MoeRouteLists l;
    l.cand = m->route_cand; l.stats = m->route_stats; l.T = T; l.Q = Q; l.norm_topk = m->cfg.norm_topk_prob;
    l.pub_expert_ids = m->expert_ids; l.pub_expert_w = m->expert_w;
    return l;
}
// The expert pair resolves its rows from the lists itself (w4_gemm_moe_em2_kernel<…, LISTS>): wherever the pair is the batch's
// form, the lists have the geometry its lookup takes and the list buffers hold them.  Decided BEFORE the chain launch, like
// the deferred merge: role B then stops at the lists and the ≈ 3.7 µs in-launch merge leaves the layer.
bool fh::moe_pair_rank_lists_ok(const FerrumHipModel* m, const LayerWeights& L, int T, int Q) {
    if (!knobs().moe_pair_rank_lists || m->cfg.expert_parallel || !m->route_cand || !m->route_stats) return false;
    if ((long)T * Q > MOE_ROUTE_LIST_CAPACITY) return false;
    const int P = T * m->cfg.top_k;
    return moe_pair_form(m, L, P) && w4_gemm_moe_expert_major_pair_supports(L.exp_gate_up, L.exp_down, m->ep_E, P) &&
           w4_gemm_moe_expert_major_pair_takes_lists(route_lists(m, T, Q), m->ep_E, P, m->cfg.top_k);
}

static int moe_decode_gemms(FerrumHipModel* m, LayerWeights& L, int P, int max_blocks, hipStream_t s, const MoeRouteLists* route = nullptr) {
    const FerrumHipModelConfig& c = m->cfg;
    const int E = m->ep_E, K = c.top_k;
    const int32_t* ids = moe_ids(m);
    const __half *gx = nullptr, *hx = nullptr;
    if (int rc = moe_gate_up_input(m, L, P / K, s, &gx)) return rc;
    if (moe_expert_major(m, P)) {
        if (moe_pair_form(m, L, P)) {
            // one launch: down tiles wait for their expert's gate_up tiles inside it (w4_gemm_moe_em2_kernel)
            int took = 0;
            if (int rc = w4_gemm_moe_expert_major_pair(L.exp_gate_up, L.exp_down, gx, m->moe_act, m->moe_down, ids, E, P, K, arrive_half(m, m->em2_parity),
                                                       arrive_half(m, m->em2_parity ^ 1), m->inlaunch_timeouts, &took, s, route)) return rc;
            if (took) { m->em2_parity ^= 1; return 0; }
        }
        FH_REQUIRE(!route, "MoE decode: the routing was left as candidate lists but the batch takes the expert-major form");
        if (int rc = w4_gemm_moe_expert_major(L.exp_gate_up, gx, m->moe_act, ids, E, P, K, 1, s)) return rc;
        if (int rc = moe_down_input(m, L, P, s, &hx)) return rc;
        return w4_gemm_moe_expert_major(L.exp_down, hx, m->moe_down, ids, E, P, 1, 0, s);
    }
    if (route) {
        // gate_up merges the lists, aligns, and publishes ids / weights / align arrays; down reads the align arrays
        if (int rc = w4_gemm_moe_merge_route(L.exp_gate_up, gx, m->moe_act, route->cand, route->stats, route->T, route->Q, K, route->norm_topk,
                                             E, max_blocks, 1, route->pub_expert_ids, route->pub_expert_w, m->sorted_ids, m->block_ids,
                                             m->total_post_pad, s)) return rc;
        form_hit(FORM_MOE_DEFERRED_MERGE);
        if (int rc = moe_down_input(m, L, P, s, &hx)) return rc;
        return w4_gemm_moe(L.exp_down, hx, m->moe_down, m->sorted_ids, m->block_ids, m->total_post_pad, P, max_blocks, 1, 0, s);
    }
    // (the router picks K distinct experts per token: with ≤ 16 tokens no expert holds more than 16 pairs — the ballot align)
    if (int rc = w4_gemm_moe_inline_align(L.exp_gate_up, gx, m->moe_act, ids, E, P, max_blocks, K, 1,
                                          m->sorted_ids, m->block_ids, m->total_post_pad, s, P / K <= 16 && !c.expert_parallel)) return rc;
    if (int rc = moe_down_input(m, L, P, s, &hx)) return rc;
    return w4_gemm_moe(L.exp_down, hx, m->moe_down, m->sorted_ids, m->block_ids, m->total_post_pad, P, max_blocks, 1, 0, s);
}

// gate_up (+silu·mul) and down grouped GEMMs for any batch size, straight from expert_ids: decode-sized batches (≤ 1024
// pairs) without a separate align launch, else align + the block shape that fits the pairs per expert.
static int moe_batch_gemms(FerrumHipModel* m, LayerWeights& L, int P, int sorted_max, int max_blocks, hipStream_t s) {
    const FerrumHipModelConfig& c = m->cfg;
    const int E = m->ep_E, K = c.top_k, Eg = c.num_experts;     // block shapes are chosen by pairs per expert over ALL experts
    const int32_t* ids = moe_ids(m);
    const __half *gx = nullptr, *hx = nullptr;
    if (P <= 1024) return moe_decode_gemms(m, L, P, max_blocks, s);
    FH_TRY(moe_gate_up_input(m, L, P / K, s, &gx));
    const bool even_groups = L.exp_gate_up.G % 2 == 0 && L.exp_down.G % 2 == 0;
    int bs = 16;                     // align block size
    if (P >= (long)m->moe_tile96_min_pairs_per_expert * Eg && even_groups) {
        // long prefill: 96-row blocks through w4_gemm_big_kernel<6> (two workgroups per CU; group scale folded into the fp16 B operand)
        bs = 96;
    } else if (P >= (long)m->moe_tile128_min_pairs_per_expert * Eg && even_groups) {
        // long prefill: 128-row blocks through w4_gemm_big_kernel (group scale folded into the fp16 B operand: the matrix pipe, not
        // vector issue, bounds it; twice the padding of 64-row blocks, hence only from a few hundred pairs per expert)
        bs = 128;
    } else if (P >= m->moe_tile_min_pairs_per_expert * Eg) {
        // prefill: ≥ 32 pairs per expert on average → 64-row blocks through the LDS-tiled kernel
        bs = 64;
    } else if (P >= m->moe_tile32_min_pairs_per_expert * Eg) {
        // a few hundred tokens (a fresh prompt riding along with the decode batch, a lone short prefill: 8–31 pairs
        // per expert): 32-row blocks through the LDS-tiled kernel — every expert's weights about once instead of
        // once per 16 pairs
        bs = 32;
    }
    if (bs == 16) {
        FH_TRY(moe_align_block_size(ids, m->sorted_ids, m->block_ids, m->total_post_pad, P, E, 16, sorted_max, s));
        FH_TRY(w4_gemm_moe(L.exp_gate_up, gx, m->moe_act, m->sorted_ids, m->block_ids, m->total_post_pad, P, max_blocks, K, 1, s));
        FH_TRY(moe_down_input(m, L, P, s, &hx));
        return w4_gemm_moe(L.exp_down, hx, m->moe_down, m->sorted_ids, m->block_ids, m->total_post_pad, P, max_blocks, 1, 0, s);
    }
    const int sorted_max_bs = P + E * bs, max_blocks_bs = std::min(sorted_max_bs / bs, P / bs + std::min(P, E));
    FH_TRY(moe_align_block_size(ids, m->sorted_ids, m->block_ids, m->total_post_pad, P, E, bs, sorted_max_bs, s));
    FH_TRY(w4_gemm_moe_tile(L.exp_gate_up, gx, m->moe_act, m->sorted_ids, m->block_ids, m->total_post_pad, P, max_blocks_bs, bs, K, 1, s));
    FH_TRY(moe_down_input(m, L, P, s, &hx));
    return w4_gemm_moe_tile(L.exp_down, hx, m->moe_down, m->sorted_ids, m->block_ids, m->total_post_pad, P, max_blocks_bs, bs, 1, 0, s);
}

static int dense_linear(FerrumHipModel* m, const W4Device& w, const __half* x, __half* out, int T, hipStream_t s, bool x_permuted = false) {
    if (w.perm && (x_permuted || w.perm_folded)) form_hit(FORM_PERM_PRODUCER);
    else if (w.perm) {
        FH_REQUIRE(m->gather_scratch, "dense_linear: act-order weights but no gather scratch");
        if (int rc = gather_columns_f16(x, w.perm, m->gather_scratch, T, w.k, s)) return rc;
        x = m->gather_scratch;
    }
    return w4_gemm_dense(w, x, out, T, m->workspace, m->workspace_bytes, s);
}

namespace {

// per-layer attention schedule (llama_layer_attention_schedule, llama_family.rs:1028-1045)
struct AttnSchedule { int window; const float *cos_t, *sin_t; };
static AttnSchedule attn_schedule(const FerrumHipModel* m, int li) {
    const int pattern = m->cfg.sliding_window_pattern;
    const bool is_global = pattern == 0 || (li + 1) % pattern == 0;
    return {pattern == 0 ? m->cfg.sliding_window : (is_global ? 0 : m->cfg.sliding_window),
            (!is_global && m->cos_local) ? m->cos_local : m->cos_t, (!is_global && m->sin_local) ? m->sin_local : m->sin_t};
}
// QK-norm weight argument of the attention kernels: models without QK-norm hand over a valid pointer that is never read
static const __half* norm_w_or_input_ln(const LayerWeights& L, const __half* w) { return w ? w : L.input_ln; }

// fp32 split-K slabs [S][rows_pad][n_pad] of a dense projection in the workspace: summed by the kernel that consumes them
struct Slabs {
    const float* base = nullptr; int S = 0, rows_pad = 0, n_pad = 0;
    long stride() const { return (long)rows_pad * n_pad; }
};

// what plan_chain decides for a layer: whether one of the one-launch attention halves (chain.hip) is its form, and the launch
enum ChainKind { CHAIN_NONE, CHAIN_DENSE, CHAIN_MOE };
struct ChainPlan { ChainKind kind = CHAIN_NONE; DecodeChainDesc d; };

// FERRUM_HIP_TRACE_LAUNCHES=1 (with FERRUM_HIP_NO_GRAPH=1: a stream cannot be synchronised inside a capture): every step of
// the forward is named on stderr and waited for, so a faulting kernel is the last line printed
#define RUN(x)                                                                       \
    do {                                                                             \
        if (trace) fprintf(stderr, "[ferrum_hip] T=%d %.70s\n", T, #x);              \
        FH_TRY(x);                                                                   \
        if (trace) FH_CHECK_HIP(hipStreamSynchronize(s));                            \
    } while (0)

// One forward, enqueued on m->stream (the index tensors are already on the device): the stages that enqueue_forward below drives,
// and what one layer hands to the next — a tail left for the next layer's first launch, the order its rows were written in.
struct ForwardPass {
    FerrumHipModel* const m; const StepShape& sh; const FerrumHipModelConfig& c; const hipStream_t s;
    const int T, H, nq, nkv, hd, qk_mode;
    const bool sandwich, trace;
    const IndexBlock ix;                 // device index block
    // ── carried from layer to layer ──
    bool qkv_in_perm = false;            // norm_out holds the row in the next q|k|v's packed order
    // decode at ≤ 4 rows (MoE models): the tail of layer l — combine + residual add + next input norm — runs as the prologue of
    // layer l+1's q|k|v GEMM instead of as a launch of its own (every dependent launch costs ≈ 4 µs there)
    bool pending_tail = false;
    FusedCombineNorm tail{};
    bool pending_chain_tail = false;     // MoE chain: combine + add + next input norm is the first role of the next layer's launch
    bool pending_dense_tail = false;     // dense chain: MLP output (its down slabs, or mlp_out) + residual + next input norm likewise
    Slabs dense_tail_slabs;
    // ── the layer in flight ──
    int li = 0; LayerWeights* Lp = nullptr;
    const __half* next_ln = nullptr;            // the next layer's input norm (null behind the last layer) …
    const int32_t* next_qkv_perm = nullptr;     // … and the act-order permutation of its q|k|v, if any

    ForwardPass(FerrumHipModel* m_, const StepShape& sh_)
        : m(m_), sh(sh_), c(m_->cfg), s(m_->stream), T(sh_.m_total), H(c.hidden), nq(c.num_heads), nkv(c.num_kv_heads), hd(c.head_dim),
          qk_mode(c.has_qk_norm ? 1 : 2), sandwich(c.sandwich_norms != 0), trace(knobs().trace_launches), ix(index_block(m_, m_->idx_dev)) {
        dense_tail_slabs.base = m->workspace;
    }
    void begin_layer(int l) {
        li = l; Lp = &m->layers[l];
        const bool last = l + 1 >= c.num_layers;
        next_ln = last ? nullptr : m->layers[l + 1].input_ln;
        next_qkv_perm = last ? nullptr : m->layers[l + 1].qkv.perm;
    }
    // (an act-order q|k|v of the next layer gets its rows permuted by the kernel that writes the next input norm)
    bool next_in_perm() const { return next_ln && next_qkv_perm != nullptr; }

    // head, one launch: embedding_lookup (+ the Gemma embedding scale, llama_family.rs:3656) → residual stream (fp16; for
    // sandwich-norm models also the fp32 shadow, llama_family.rs:3664-3674) → layer 0's input norm.  Later layers get their
    // input norm fused into the previous layer's tail.
    // act-order (desc_act) projections read x'[j] = x[perm[j]]: the kernel that PRODUCES the row writes it permuted wherever one
    // workgroup owns the row (every norm of the dense layer) or the rows are few (decode attention scatters); the gated
    // activation is permuted by gate_up's column order (pack_gate_up).  Only the prefill o_proj keeps a gather launch.
    // The arrival counters of the split route kernel are re-armed by the kernel itself, but zeroed per forward as well (here) so
    // that an aborted launch can never poison the next one.
    int head() {
        const LayerWeights& L0 = m->layers[0];
        RUN(embed_rms_norm_f16(m->embed, ix.tokens, c.embed_scale, m->residual, sandwich ? m->residual_f32 : nullptr, L0.input_ln,
                               c.rms_eps, m->norm_out, T, H, m->route_arrive, m->route_arrive ? 64 + (int)m->arrive_half_words : 0, s, L0.qkv.perm));
        m->em2_parity = 0;          // the head kernel zeroed half 0 of the merged launches' counters; every such launch zeroes the other half
        m->chain_parity = 0;
        qkv_in_perm = L0.qkv.perm != nullptr;
        return 0;
    }

    // ── the one-launch attention half of a decode layer (chain.hip) ──
    DecodeChainDesc chain_desc(int l) const {
        LayerWeights& L = m->layers[l];
        DecodeChainDesc d;
        d.T = T; d.H = H; d.nq = nq; d.nkv = nkv; d.head_dim = hd;
        d.top_k = c.top_k; d.down = m->moe_down; d.comb_w = m->expert_w; d.res_in = m->residual2; d.ln_in = L.input_ln; d.eps = c.rms_eps;
        d.res_a = m->residual; d.norm1 = m->norm_out;
        d.qkv = &L.qkv; d.qkv_out = m->qkv_out;
        d.k_pool = L.k_pool; d.v_pool = L.v_pool; d.block_tables = ix.bt; d.kv_lens = ix.kvl;
        d.q_norm_w = norm_w_or_input_ln(L, L.q_norm); d.k_norm_w = norm_w_or_input_ln(L, L.k_norm);
        const AttnSchedule as = attn_schedule(m, l);
        d.sliding_window = as.window; d.cos_t = as.cos_t; d.sin_t = as.sin_t;
        d.qk_mode = qk_mode; d.max_blocks = m->max_blocks_per_seq;
        d.attn_out = m->attn_out; d.o = &L.o; d.o_out = m->o_out; d.o_part = m->chain_o_part;
        d.res_b_out = m->residual2; d.post_ln = L.post_ln; d.norm2 = m->norm_out; d.router_w = L.router;
        d.E = c.num_experts; d.r_top_k = c.top_k; d.norm_topk = c.norm_topk_prob;
        d.Q = chain_route_parts(m);
        d.cand = m->route_cand; d.stats = m->route_stats; d.route_arrive = m->route_arrive; d.ids = m->expert_ids; d.weights = m->expert_w;
        d.timeout = m->inlaunch_timeouts;
        // KV ranges per (sequence, kv head) in the attention role: ≈ chain_split_keys (256) keys each while the role stays within
        // W workgroups — W = 32 … 256 growing with the (sequence, kv head) count: the chain holds one workgroup per CU, and ranges
        // beyond that push the o_proj / router roles (which prefetch their weights while they wait) out of residence — but never
        // more than ≈ 1024 keys per range while 256 workgroups allow (profiles/r03_chain_kv_splits.txt: c × context × ranges)
        const long keys = chain_keys(d);
        const long units = (long)T * nkv, sk = std::max(1, knobs().chain_split_keys);
        const long cap_w = std::min<long>(256, std::max<long>(4 * units, std::min<long>(8 * units, 64)));
        long ns_l = std::min<long>({16, std::max<long>(1, cap_w / units), (keys + sk - 1) / sk});
        ns_l = std::max<long>(ns_l, std::min<long>({16, std::max<long>(1, 256 / units), (keys + 4 * sk - 1) / (4 * sk)}));
        int ns = keys <= 2 * sk ? 1 : (int)std::max<long>(1, ns_l);        // (≤ 512 keys: one range — c=4 at 256+: 2.31 vs 2.36 ms split in two)
        if (knobs().chain_attn_splits > 0) ns = std::min(16, knobs().chain_attn_splits);
        while (ns > 1 && units * ns > CHAIN_MAX_ATTN_WGS) ns--;
        if (!m->chain_attn_partial || units > 4096 || knobs().chain_split_keys <= 0) ns = 1;
        d.attn_splits = ns; d.attn_partial = m->chain_attn_partial; d.attn_tickets = m->chain_attn_tickets;
        return d;
    }
    // the most keys one sequence's attention streams in this layer
    long chain_keys(const DecodeChainDesc& d) const {
        return d.sliding_window > 0 ? std::min<long>(sh.max_kv_len, d.sliding_window) : sh.max_kv_len;
    }
    // The chain stays the layer's form while one attention workgroup has ≤ chain_max_keys (4096) keys to stream (more where T·nkv
    // workgroups already cover the chip twice); with its KV ranges it beat the stand-alone split-KV launches at every point measured
    // (c=1 at 32 k keys: 3.06 vs 3.52 ms per step; c=4 at 16 k: 3.62 vs 3.96; c=32 at 8 k: 7.85 vs 8.24) — beyond that is unmeasured
    bool chain_kv_ok(const DecodeChainDesc& d) const {
        return chain_keys(d) <= (long)knobs().chain_max_keys * d.attn_splits * std::max<long>(1, (long)T * nkv / 128);
    }
    // MoE decode at ≤ 32 rows: [the previous layer's tail] + q|k|v + attention + o_proj + add/norm/route as ONE launch
    // (chain.hip), then the merged gate_up → down launch: two launches per layer instead of seven
    bool moe_chain_ok(const DecodeChainDesc& d) const {
        if (c.num_experts <= 0 || !knobs().decode_chain || m->em2_failed || !m->em2_arrive || !m->inlaunch_timeouts) return false;
        if (!sh.all_single_token || !m->fuse_rope_attn || T > knobs().chain_max_rows || m->taps_enabled || sandwich) return false;
        if (c.tp_world > 1 && c.expert_parallel != 2) return false;             // (tensor-parallel attention: an all-reduce sits behind o_proj)
        if (T * c.top_k > 1024 || c.top_k > 8 || T > 128 || !chain_kv_ok(d)) return false;
        return decode_chain_supports(d);
    }
    // dense models at 17–32 rows: the same launch for the attention half (tail of the previous layer's MLP — its down slabs +
    // residual + norm — q|k|v, attention, o_proj, add + norm), then gate_up slabs → gated activation → down slabs
    bool dense_chain_ok(const LayerWeights& L, const DecodeChainDesc& d) const {
        if (c.num_experts > 0 || !knobs().decode_chain || !knobs().dense_chain || m->em2_failed || !m->em2_arrive || !m->inlaunch_timeouts || !m->residual2) return false;
        if (!sh.all_single_token || !m->fuse_rope_attn || T > std::min(64, knobs().chain_max_rows) || m->taps_enabled || sandwich || c.tp_world > 1) return false;      // (beyond 64 rows the 64-row GEMM tiles win: Llama-3.1-8B c=96 5.56 vs 5.61 ms)
        if (!L.o.qw || !L.gate_up.qw || !L.down.qw || L.gate_up.perm || L.down.perm || L.qkv.perm || L.o.perm) return false;
        if (L.qkv.bias || L.o.bias || !chain_kv_ok(d)) return false;
        return decode_chain_supports(d);
    }
    // (the dense chain is tested first; the description leaves here without a tail role — the layer body adds it)
    ChainPlan plan_chain(int l) const {
        ChainPlan p;
        p.d = chain_desc(l);
        p.kind = dense_chain_ok(m->layers[l], p.d) ? CHAIN_DENSE : moe_chain_ok(p.d) ? CHAIN_MOE : CHAIN_NONE;
        return p;
    }

    int dense_chain_layer(DecodeChainDesc d, bool next_chained) {
        LayerWeights& L = *Lp;
        const Slabs& a = dense_tail_slabs;
        d.has_a = pending_dense_tail;
        d.a_slabs = a.base; d.a_S = a.S; d.a_slab_stride = a.stride(); d.a_ld = a.n_pad;
        d.a_x = a.S == 0 ? m->mlp_out : nullptr;
        d.cnt = arrive_half(m, m->chain_parity);
        d.cnt_next = arrive_half(m, m->chain_parity ^ 1);
        RUN(decode_chain_f16(d, s));
        m->chain_parity ^= 1;
        pending_dense_tail = false;
        form_hit(FORM_DENSE_CHAIN);
        Slabs down{m->workspace};
        const bool slabs = m->dense_slabs && T > 16 && T <= 32;      // 17–32 rows: split-K slabs summed by their consumers
        if (slabs) {
            RUN(gate_up_act(true));
            RUN(w4_gemm_dense_slabs_lds(L.down, m->act_out, m->workspace, m->workspace_bytes, T, &down.S, &down.rows_pad, &down.n_pad, s));
        } else {
            RUN(dense_mlp_ops());
        }
        if (next_chained) {
            pending_dense_tail = true;          // MLP output + residual + next input norm: the first role of the next layer's launch
            dense_tail_slabs = down;
            return 0;
        }
        // (the residual of this layer sits in the ping-pong buffer: the stand-alone tail works on it in place, then it moves back)
        if (slabs) RUN(slab_tail(down, m->residual2, L.post_ffn_ln, next_ln, next_qkv_perm));
        else RUN(dense_tail(m->mlp_out, m->residual2, L.post_ffn_ln, next_ln, next_qkv_perm));
        FH_CHECK_HIP(hipMemcpyAsync(m->residual, m->residual2, (size_t)T * H * sizeof(__half), hipMemcpyDeviceToDevice, s));
        qkv_in_perm = next_in_perm();
        return 0;
    }

    int moe_chain_layer(DecodeChainDesc d, bool next_chained) {
        LayerWeights& L = *Lp;
        const int P = T * c.top_k;
        const size_t behind_pair = (size_t)c.num_experts * MOE_PAIR_COUNTER_STRIDE;      // the chain's counters follow the pair's in each half
        d.has_a = pending_chain_tail;
        d.cnt = arrive_half(m, m->chain_parity) + behind_pair;
        d.cnt_next = arrive_half(m, m->chain_parity ^ 1) + behind_pair;
        // the Q candidate lists of a token are merged by the grouped GEMM's prologue (under its first weight loads) where that
        // form runs, instead of by role B's first part at the end of the chain (≈ 3.7 µs of every layer)
        // … or, where the layer's grouped GEMMs are the expert pair, looked up by each of its tiles for its own expert
        d.defer_merge = d.Q > 1 && (moe_deferred_merge_ok(m, L, T, d.Q) || moe_pair_rank_lists_ok(m, L, T, d.Q));
        const MoeRouteLists lists = route_lists(m, T, d.Q);
        RUN(decode_chain_f16(d, s));
        m->chain_parity ^= 1;
        pending_chain_tail = false;
        form_hit(d.Q > 1 ? FORM_ROUTE_SPLIT : FORM_ROUTE_FUSED);
        RUN(after_route(P));
        RUN(moe_decode_gemms(m, L, P, moe_max_blocks(P, c.num_experts), s, d.defer_merge ? &lists : nullptr));
        if (!c.expert_parallel && next_chained) pending_chain_tail = true;
        else RUN(moe_tail(m->residual2, m->residual));
        return 0;
    }

    // ── the multi-launch layer ──
    // q|k|v GEMM, then QK-norm + RoPE + KV write + attention.  *attn_perm: attn_out holds the row in L.o's packed order
    int qkv_attention(bool* attn_perm) {
        LayerWeights& L = *Lp;
        if (pending_tail) {
            RUN(w4_gemm_dense(L.qkv, nullptr, m->qkv_out, T, m->workspace, m->workspace_bytes, s, &tail));
            pending_tail = false;
        } else {
            RUN(dense_linear(m, L.qkv, m->norm_out, m->qkv_out, T, s, qkv_in_perm));
        }
        qkv_in_perm = false;
        *attn_perm = false;
        const AttnSchedule as = attn_schedule(m, li);
        const __half *q_norm = norm_w_or_input_ln(L, L.q_norm), *k_norm = norm_w_or_input_ln(L, L.k_norm);
        const int mb = m->max_blocks_per_seq;
        if (sh.all_single_token && m->fuse_rope_attn && nq / nkv <= 14) {
            // decode: QK-norm + RoPE + KV write happen in the attention kernel's prologue (one launch fewer)
            RUN(paged_decode_attention_fused_qkv_f16(m->qkv_out, q_norm, k_norm, as.cos_t, as.sin_t, c.rms_eps, qk_mode, L.k_pool, L.v_pool,
                                                     m->attn_out, ix.bt, ix.kvl, sh.num_seqs, sh.max_kv_len, nq, nkv, hd, as.window, KV_BLOCK,
                                                     mb, m->workspace, m->workspace_bytes, s, L.o.inv_perm));
            *attn_perm = L.o.perm != nullptr;
            return 0;
        }
        RUN(split_qkv_norm_rope_into_paged_cache_varlen_f16(m->qkv_out, q_norm, k_norm, as.cos_t, as.sin_t, m->q_out, L.k_pool, L.v_pool,
                                                            ix.cu, ix.pos, ix.bt, sh.num_seqs, T, nq, nkv, hd, c.rms_eps, qk_mode, KV_BLOCK, mb, s));
        if (sh.pure_decode && as.window == 0) {
            RUN(paged_batched_decode_attention_f16(m->q_out, L.k_pool, L.v_pool, m->attn_out, ix.bt, ix.kvl, sh.num_seqs, sh.max_kv_len, nq, nkv, hd,
                                                   KV_BLOCK, mb, m->workspace, m->workspace_bytes, s, L.o.inv_perm));
            *attn_perm = L.o.perm != nullptr;
        } else if (sh.single_prefix > 0 && sh.single_prefix < sh.num_seqs && (long)sh.rest_min_q * (nq / nkv) >= 16L * m->attn_flash_min_rows) {
            // decode rows first, LONG prompts after them (≥ 1024 tokens at a GQA group of 8; for a 256-token prompt the
            // second launch costs more than the form saves: 9.7 → 10.2 ms per iteration): two launches, so that the
            // prompts take the LDS-shared K/V form and the decode rows the KV-split form (q/out are indexed by the
            // absolute token offsets in cu_seqlens_q, so sub-ranges of the sequence arrays are enough)
            const int n1 = sh.single_prefix;
            RUN(varlen_attention(as.window, 0, n1, n1, 1));
            RUN(varlen_attention(as.window, n1, sh.num_seqs - n1, T - n1, sh.max_q_len));
        } else {
            RUN(varlen_attention(as.window, 0, sh.num_seqs, T, sh.max_q_len));
        }
        return 0;
    }
    // paged attention over the sequences [first, first + n_seqs) of the batch, which bring `tokens` query rows
    int varlen_attention(int window, int first, int n_seqs, int tokens, int max_q_len) {
        const int mb = m->max_blocks_per_seq;
        return paged_varlen_attention_f16(m->q_out, Lp->k_pool, Lp->v_pool, m->attn_out, ix.cu + first, ix.pos + first, ix.bt + (size_t)first * mb,
                                          n_seqs, tokens, max_q_len, sh.max_kv_len, nq, nkv, hd, window, KV_BLOCK, mb, m->workspace,
                                          m->workspace_bytes, s);
    }

    // expert parallel: after routing, the pair ids become local ids (−1 = another rank's expert)
    int after_route(int P) {
        return c.expert_parallel ? moe_remap_expert_ids(m->expert_ids, m->expert_ids_local, P, m->ep_e0, m->ep_E, s) : 0;
    }
    // the MoE layer tail: residual_out = residual_in + Σ_k w_k·down_k, then the next input norm.  Expert parallel: the sum over
    // the rank's own experts is a partial [T, H] that meets the other ranks' in the all-reduce a dense MLP uses, and the
    // reduced row then enters the residual like a single expert row of weight 1 (the same kernel, top_k = 1)
    int moe_tail(const __half* res_in, __half* res_out) {
        const __half* rows = m->moe_down;
        const float* w = m->expert_w;
        int K = c.top_k;
        if (c.expert_parallel) {
            RUN(moe_combine_local_f16(rows, w, m->expert_ids_local, m->mlp_out, T, K, H, s));
            RUN(tp_all_reduce(m, m->mlp_out, (size_t)T * H));
            rows = m->mlp_out; w = m->ones; K = 1;
        }
        RUN(moe_combine_add_rms_norm_f16(rows, w, res_in, res_out, next_ln, c.rms_eps, m->norm_out, T, K, H, s, next_qkv_perm));
        qkv_in_perm = next_in_perm();
        return 0;
    }

    // o_proj → add/norm/route → grouped GEMMs → tail
    int moe_mlp(bool attn_perm) {
        const LayerWeights& L = *Lp;
        const int E = c.num_experts, K = c.top_k, P = T * K, tiles = (E + 15) / 16, Q = chain_route_parts(m);
        // attention heads sharded, o_proj row-parallel: all-reduce before the add + norm + route kernel (expert_parallel 2 keeps
        // attention replicated: full heads on every rank, nothing to reduce there)
        const bool tp = c.tp_world > 1 && c.expert_parallel != 2;
        const bool o_quant = L.o.qw != nullptr;           // the slab forms are INT4 kernels; an unquantised o_proj takes the direct GEMM
        if (T <= 64 && P <= 1024 && K <= 8 && Q >= 1 && tiles / Q <= 8 && (!L.o.perm || attn_perm)) return moe_mlp_decode_fast(attn_perm, tp, Q);
        // short prefill / a prompt riding along with the decode batch: o_proj as fp32 split-K slabs straight into the
        // add + norm + route kernel (no reduce launch)
        const bool o_slabs = T >= 64 && T < m->route_gemm_min_tokens && !tp && o_quant && !L.o.perm && !L.o.bias && m->o_slabs > 0;
        return moe_mlp_batch(attn_perm, tp, o_slabs);
    }
    // decode-fast o_proj: fp32 split-K slabs, reduced inside the next kernel (no reduce launch), where a slab form applies
    int o_proj_decode_fast(bool attn_perm, bool tp, Slabs* o) {
        LayerWeights& L = *Lp;
        o->S = m->o_slabs;
        if (tp || !L.o.qw) {
            RUN(dense_linear(m, L.o, m->attn_out, m->o_out, T, s, attn_perm));
            if (tp) RUN(tp_all_reduce(m, m->o_out, (size_t)T * H));
            o->S = 0;
        } else if (o->S > 0 && T > 16 && T <= 32 && !L.o.bias) {
            if (L.o.perm) form_hit(FORM_PERM_PRODUCER);          // (attn_perm: the decode attention wrote the permuted rows)
            // 17–32 rows: activations staged once per workgroup in LDS (a wave fetching its own fragments pulls 2× the
            // weight bytes from L2); decode c=32 4.60 → 4.57 ms per step
            RUN(w4_gemm_dense_slabs_lds(L.o, m->attn_out, m->workspace, m->workspace_bytes, T, &o->S, &o->rows_pad, &o->n_pad, s));
            o->base = m->workspace;
        } else if (o->S > 0) {
            if (L.o.perm) form_hit(FORM_PERM_PRODUCER);
            RUN(w4_gemm_dense_slabs(L.o, m->attn_out, m->workspace, m->workspace_bytes, T, o->S, &o->rows_pad, &o->n_pad, s));
            o->base = m->workspace;
            o->S = std::min(o->S, L.o.G);
        } else {
            RUN(dense_linear(m, L.o, m->attn_out, m->o_out, T, s, attn_perm));
        }
        return 0;
    }
    int moe_mlp_decode_fast(bool attn_perm, bool tp, int Q) {
        LayerWeights& L = *Lp;
        const int E = c.num_experts, K = c.top_k, P = T * K;
        Slabs o;
        RUN(o_proj_decode_fast(attn_perm, tp, &o));
        form_hit(Q > 1 ? FORM_ROUTE_SPLIT : FORM_ROUTE_FUSED);
        if (Q > 1) {
            // B over Q expert parts per token (one CU pulls the 512-KB router at ≈70 GB/s; Q CUs share it):
            // residual → residual2 (ping-pong), norm_out; each token's last-arriving part merges the Q
            // candidate lists inside the launch and writes expert_ids / expert_w.
            RUN(fused_add_rms_norm_route_split_f16(m->residual, m->residual2, m->o_out, o.base, o.S, o.stride(), o.n_pad, L.post_ln, c.rms_eps,
                                                   m->norm_out, L.router, E, K, Q, m->route_cand, m->route_stats, m->route_arrive,
                                                   c.norm_topk_prob, m->expert_ids, m->expert_w, nullptr, T, H, s));
        } else {
            RUN(fused_add_rms_norm_route_slabs_f16(m->residual, m->o_out, o.base, o.S, o.stride(), o.n_pad, L.post_ln, c.rms_eps, m->norm_out,
                                                   L.router, E, K, c.norm_topk_prob, m->expert_ids, m->expert_w, nullptr, T, H, s));
        }
        RUN(after_route(P));
        RUN(moe_decode_gemms(m, L, P, moe_max_blocks(P, E), s));
        if (Q > 1 && T <= m->fuse_tail_max_rows && next_ln && !m->taps_enabled && !c.expert_parallel &&
            w4_gemm_dense_can_fuse_combine_norm(m->layers[li + 1].qkv, T)) {
            tail = FusedCombineNorm{m->moe_down, m->expert_w, m->residual2, m->residual, next_ln, c.rms_eps, K};
            pending_tail = true;
        } else {
            RUN(moe_tail(Q > 1 ? m->residual2 : m->residual, m->residual));
        }
        return 0;
    }
    int moe_mlp_batch(bool attn_perm, bool tp, bool o_slabs) {
        LayerWeights& L = *Lp;
        const int E = c.num_experts, K = c.top_k, P = T * K;
        if (o_slabs) {
            Slabs o{m->workspace, 1};
            RUN(w4_gemm_dense_slabs_tile(L.o, m->attn_out, m->workspace, m->workspace_bytes, T, &o.S, &o.rows_pad, &o.n_pad, s));
            RUN(fused_add_rms_norm_route_slabs_f16(m->residual, m->o_out, o.base, o.S, o.stride(), o.n_pad, L.post_ln, c.rms_eps, m->norm_out,
                                                   L.router, E, K, c.norm_topk_prob, m->expert_ids, m->expert_w, nullptr, T, H, s));
        } else {
            RUN(dense_linear(m, L.o, m->attn_out, m->o_out, T, s, attn_perm));
            if (tp) RUN(tp_all_reduce(m, m->o_out, (size_t)T * H));
            form_hit(T >= m->route_gemm_min_tokens ? FORM_ROUTE_GEMM : FORM_ROUTE_FUSED);
            if (T < m->route_gemm_min_tokens) {
                // residual += o; post-attention norm; router logits; top-k — one launch (fused.hip B)
                RUN(fused_add_rms_norm_route_f16(m->residual, m->o_out, L.post_ln, c.rms_eps, m->norm_out, L.router, E, K,
                                                 c.norm_topk_prob, m->expert_ids, m->expert_w, nullptr, T, H, s));
            } else {
                // prefill: one workgroup per token would pull the whole router (E·H·2 B) from L2 per token (2048 tokens:
                // 1 GB, 95 µs) — run the router as a GEMM over all tokens instead, then the top-k kernel
                RUN(fused_add_rms_norm_f16(m->residual, m->o_out, L.post_ln, c.rms_eps, m->norm_out, T, H, s));
                if (knobs().route_gemm_topk && !m->taps_enabled && moe_route_gemm_topk_supports(E, H, K)) {
                    // … and the top-k in the same workgroups: the logits stay on the CU (8192 tokens: 27 + 7 + 16 µs → one launch)
                    form_hit(FORM_ROUTE_GEMM_TOPK);
                    RUN(moe_route_gemm_topk_f16(m->norm_out, L.router, m->expert_ids, m->expert_w, T, E, H, K, c.norm_topk_prob, s));
                } else {
                    RUN(f16t_gemm_f32out(m->norm_out, L.router, m->router_logits, T, E, H, m->workspace, m->workspace_bytes, s));
                    RUN(moe_route_topk_softmax_f32(m->router_logits, m->expert_ids, m->expert_w, T, E, K, c.norm_topk_prob, s));
                }
            }
        }
        RUN(after_route(P));
        RUN(moe_batch_gemms(m, L, P, P + E * 16, moe_max_blocks(P, E), s));
        RUN(moe_tail(m->residual, m->residual));
        return 0;
    }

    // ── dense MLP block ──
    // gate_up → gated activation: as split-K slabs that the activation sums, or GEMM + activation (gate_up's input arrives
    // permuted from its producer where it is act-order)
    int gate_up_act(bool slabs) {
        const int I = c.intermediate;
        Slabs g{m->workspace};
        if (slabs) {
            RUN(w4_gemm_dense_slabs_lds(Lp->gate_up, m->norm_out, m->workspace, m->workspace_bytes, T, &g.S, &g.rows_pad, &g.n_pad, s));
            RUN(fused_gated_act_slabs_f16(g.base, g.S, g.stride(), g.n_pad, m->act_out, T, I, c.activation == 1, s));
            return 0;
        }
        RUN(dense_linear(m, Lp->gate_up, m->norm_out, m->gate_up_out, T, s, true));
        if (c.activation == 1) RUN(fused_gelu_tanh_mul_split_f16(m->gate_up_out, m->act_out, T, I, s));
        else RUN(fused_silu_mul_split_f16(m->gate_up_out, m->act_out, T, I, s));
        return 0;
    }
    // the MLP as an op chain: gate_up → gated activation → down
    int dense_mlp_ops() {
        RUN(gate_up_act(false));
        RUN(dense_linear(m, Lp->down, m->act_out, m->mlp_out, T, s));
        return 0;
    }
    // A branch output x (o_proj or down: row-parallel partials under tensor parallelism) is all-reduced and enters the residual, and
    // the norm that follows rides along.  Sandwich norms (Gemma 3, llama_family.rs:3357-3421): residual_f32 += norm(x, post_norm).
    // Behind the last layer a plain add (the final norm runs on the sampled rows).  `perm`: act-order permutation of norm_out's reader
    int dense_tail(__half* x, __half* residual, const __half* post_norm, const __half* next_norm, const int32_t* perm) {
        if (sandwich) {
            RUN(tp_all_reduce(m, x, (size_t)T * H));
            RUN(sandwich_add_rms_norm_f32(x, post_norm, m->residual_f32, next_norm, c.rms_eps, m->norm_out, T, H, s, perm));
        } else if (next_norm) {
            RUN(tp_all_reduce_add_rms_norm(m, x, residual, next_norm, c.rms_eps, m->norm_out, T, H, s, perm));
        } else {
            RUN(tp_all_reduce(m, x, (size_t)T * H));
            RUN(add_inplace_f16(residual, x, (long)T * H, s));
        }
        return 0;
    }
    // the same for a branch output that arrives as split-K slabs (one GPU): the add + norm kernel sums them.  Behind the last
    // layer the norm output is unused (any valid weight will do)
    int slab_tail(const Slabs& x, __half* residual, const __half* post_norm, const __half* next_norm, const int32_t* perm) {
        if (sandwich) {
            RUN(sandwich_add_rms_norm_f32_slabs(x.base, x.S, x.stride(), x.n_pad, post_norm, m->residual_f32, next_norm, c.rms_eps, m->norm_out,
                                                T, H, s, perm));
        } else {
            RUN(fused_add_rms_norm_route_slabs_f16(residual, nullptr, x.base, x.S, x.stride(), x.n_pad, next_norm ? next_norm : Lp->input_ln,
                                                   c.rms_eps, m->norm_out, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, T, H, s, perm));
        }
        return 0;
    }
    int dense_mlp(bool attn_perm) {
        LayerWeights& L = *Lp;
        const int32_t* gu_perm = L.gate_up.perm;
        // 17–32 rows, one GPU: every projection of the MLP block writes fp32 split-K slabs (LDS-shared activations) and
        // the consumer that exists anyway — add+norm, gated activation — sums them: no reduce launches.
        // Tensor parallel (o / down row-parallel): the partial sums of the ranks meet in an all-reduce, so those two
        // projections produce fp16 partials (GEMM + reduce), all-reduce, then add + norm; the column-parallel gate_up keeps
        // its slabs → gated-activation form.  Everything stays stream-ordered device work, so the step is still one graph.
        const bool tp = c.tp_world > 1;
        // (act-order projections: every input of the chain arrives permuted from its producer — decode attention, the norms
        // below, gate_up's column order)
        const bool slab_chain = m->dense_slabs && T > 16 && T <= 32 && (!L.o.perm || attn_perm) && (!L.down.perm || L.down.perm_folded) &&
                                L.o.qw && L.gate_up.qw && L.down.qw;   // INT4 slab kernels; unquantised projections take the op chain
        const bool slabs = slab_chain && !tp;         // … o_proj and down hand their consumer slabs
        if (slab_chain) form_hit(FORM_DENSE_SLAB_CHAIN);
        if (slabs) {
            Slabs o{m->workspace};
            if (L.o.perm) form_hit(FORM_PERM_PRODUCER);
            RUN(w4_gemm_dense_slabs_lds(L.o, m->attn_out, m->workspace, m->workspace_bytes, T, &o.S, &o.rows_pad, &o.n_pad, s));
            RUN(slab_tail(o, m->residual, L.post_attn_ln, L.post_ln, gu_perm));
        } else {
            RUN(dense_linear(m, L.o, m->attn_out, m->o_out, T, s, attn_perm));
            RUN(dense_tail(m->o_out, m->residual, L.post_attn_ln, L.post_ln, gu_perm));
        }
        if (slab_chain && gu_perm) form_hit(FORM_PERM_PRODUCER);
        if (slab_chain && L.down.perm) form_hit(FORM_PERM_PRODUCER);
        RUN(gate_up_act(slab_chain));
        if (slabs) {
            Slabs down{m->workspace};
            RUN(w4_gemm_dense_slabs_lds(L.down, m->act_out, m->workspace, m->workspace_bytes, T, &down.S, &down.rows_pad, &down.n_pad, s));
            RUN(slab_tail(down, m->residual, L.post_ffn_ln, next_ln, next_qkv_perm));
        } else {
            RUN(dense_linear(m, L.down, m->act_out, m->mlp_out, T, s));
            RUN(dense_tail(m->mlp_out, m->residual, L.post_ffn_ln, next_ln, next_qkv_perm));
        }
        qkv_in_perm = next_in_perm();
        return 0;
    }

    // the residual stream behind this layer, for ferrum_hip_model_read_taps
    int tap() {
        if (!m->taps_enabled || !m->taps) return 0;
        float* dst = m->taps + (size_t)li * c.max_tokens * H;
        if (sandwich) FH_CHECK_HIP(hipMemcpyAsync(dst, m->residual_f32, (size_t)T * H * 4, hipMemcpyDeviceToDevice, s));
        else f16_to_f32(m->residual, dst, (long)T * H, s);
        return 0;
    }

    // final norm + lm_head on the sampled rows only (same rows the reference packs, qwen3_moe_forward_unified.rs:365-392), then
    // the greedy argmax on the device
    int sample_head(bool greedy, const GreedyDeviceOpts* gopts, const DecodeAdvance* advance, int* advance_fused) {
        const int n = sh.num_sampled;
        if (n <= 0) return 0;
        if (sandwich) RUN(rms_norm_f32_to_f16(m->residual_f32, ix.sampled_idx, m->final_norm, c.rms_eps, m->sampled_hidden, n, H, s));
        else RUN(gather_rms_norm_f16(m->residual, ix.sampled_idx, m->final_norm, c.rms_eps, m->sampled_hidden, n, H, s));
        const int Vn = m->vp_n, v0 = m->vp_v0;                  // this rank's vocabulary rows (all of them unless vocabulary parallel)
        RUN(f16t_gemm_f32out(m->sampled_hidden, m->lm_head_t, m->logits, n, Vn, H, m->workspace, m->workspace_bytes, s));
        if (!greedy) return 0;
        const bool penalties = gopts && gopts->row_offsets;
        if (!c.vocab_parallel) {
            // LogitsReturnPolicy::GreedyArgmax { token_mask, repetition_penalty } (model_executor.rs:109-150): the sparse
            // penalty rewrites the listed logits in place, then raw or masked argmax (traits.rs:1571-1591)
            if (penalties) RUN(apply_repetition_penalties_sparse_f32(m->logits, gopts->row_offsets, gopts->token_ids, gopts->penalties, n, c.vocab, s));
            RUN(argmax_rows_f32_ws_advance(m->logits, m->out_tokens, gopts ? gopts->mask : nullptr, gopts ? gopts->mask_len : 0, n, c.vocab,
                                           m->workspace, m->workspace_bytes, advance, advance_fused, s));
            return 0;
        }
        // vocabulary parallel: penalty and mask act on the rank's slice (ids / mask bytes shifted by v0), the local first
        // maximum becomes a (logit, global id) pair, the pairs of all ranks are gathered and the first maximum in rank
        // order wins — the lowest id among equal logits, as on one GPU.  The merge also advances the decode state.
        if (penalties)
            RUN(apply_repetition_penalties_sparse_f32_shard(m->logits, gopts->row_offsets, gopts->token_ids, gopts->penalties, n, Vn, v0, s));
        const uint8_t* mask = gopts && gopts->mask ? gopts->mask + std::min(v0, gopts->mask_len) : nullptr;
        const int mask_len = gopts && gopts->mask ? std::max(0, gopts->mask_len - v0) : 0;
        RUN(argmax_rows_f32_ws(m->logits, m->out_tokens, mask, mask_len, n, Vn, m->workspace, m->workspace_bytes, s));
        RUN(argmax_pairs_f32(m->logits, m->out_tokens, m->vp_pairs, n, Vn, v0, mask, mask_len, s));
        RUN(tp_all_gather(m, m->vp_pairs, m->vp_gathered, (size_t)n * 8));
        RUN(argmax_merge_ranks(m->vp_gathered, m->out_tokens, n, c.tp_world, advance, s));
        if (advance && advance_fused) *advance_fused = 1;
        return 0;
    }
    // the embedding tail instead: final norm (fp32, never rounded) → pool over each final-chunk item's rows → cut → L2.  The
    // residual stream is complete here in every form: behind the last layer no chain launch follows, so its tail has run.
    int embed_head(const EmbedHead& eh) {
        if (sh.num_sampled <= 0) return 0;
        const void* rows = sandwich ? (const void*)m->residual_f32 : (const void*)m->residual;
        return embed_pool(rows, sandwich, ix.embed_spans, eh.final_norm ? m->final_norm : nullptr, c.rms_eps, eh.pooling, eh.normalize, eh.dims,
                          eh.out, sh.num_sampled, H, eh.max_span_rows, m->workspace, m->workspace_bytes, s);
    }
    // the scoring head instead: the rows the targets name, a pass at a time, through what sample_head runs on its rows (final
    // norm, lm_head) and then the log-sum-exp / first maximum / gather of score_head.hip on the pass's logits
    int score_head(const ScoreHead& h) {
        for (int q = 0; q < h.num_passes; q++) {
            const int r0 = h.pass_row_begin[q], n = h.pass_row_begin[q + 1] - r0;
            const int p0 = h.pass_pair_begin[q], pairs = h.pass_pair_begin[q + 1] - p0;
            if (sandwich) RUN(rms_norm_f32_to_f16(m->residual_f32, h.rows + r0, m->final_norm, c.rms_eps, m->score_hidden, n, H, s));
            else RUN(gather_rms_norm_f16(m->residual, h.rows + r0, m->final_norm, c.rms_eps, m->score_hidden, n, H, s));
            RUN(f16t_gemm_f32out(m->score_hidden, m->lm_head_t, m->score_logits, n, c.vocab, H, m->workspace, m->workspace_bytes, s));
            RUN(logprob_rows_f32(m->score_logits, c.vocab, n, c.vocab, h.pair_rows + p0, h.pair_tokens + p0, pairs, h.pair_logprob + p0, nullptr,
                                 h.row_top + r0, h.row_top_logprob + r0, m->workspace, m->workspace_bytes, s));
        }
        return 0;
    }
};
#undef RUN

}  // namespace

// Enqueue one forward: head, the layers — each as one of the chain forms (decided per layer, the next layer's decision known, so
// that a tail can be left to its launch) or as q|k|v + attention and the MLP block — then the sampling head, or (`embed`) the
// embedding tail, or (`score`) the scoring head in its place.
int fh::enqueue_forward(FerrumHipModel* m, const StepShape& sh, bool greedy, const GreedyDeviceOpts* gopts, const DecodeAdvance* advance,
                        int* advance_fused, const EmbedHead* embed, const ScoreHead* score) {
    if (advance_fused) *advance_fused = 0;
    const int n_layers = m->cfg.num_layers;
    ForwardPass f(m, sh);
    FH_TRY(f.head());
    ChainPlan plan = f.plan_chain(0);
    for (int li = 0; li < n_layers; li++) {
        const ChainPlan next = li + 1 < n_layers ? f.plan_chain(li + 1) : ChainPlan();
        f.begin_layer(li);
        if (plan.kind == CHAIN_DENSE) {
            FH_TRY(f.dense_chain_layer(plan.d, next.kind == CHAIN_DENSE));
        } else if (plan.kind == CHAIN_MOE) {
            FH_TRY(f.moe_chain_layer(plan.d, next.kind == CHAIN_MOE));
        } else {
            bool attn_perm = false;
            FH_TRY(f.qkv_attention(&attn_perm));
            FH_TRY(m->cfg.num_experts > 0 ? f.moe_mlp(attn_perm) : f.dense_mlp(attn_perm));
            FH_TRY(f.tap());           // (the chain forms are never taken with taps on)
        }
        plan = next;
    }
    m->taps_tokens = sh.m_total;
    if (embed) return f.embed_head(*embed);
    if (score) return f.score_head(*score);
    return f.sample_head(greedy, gopts, advance, advance_fused);
}
#undef FH_TRY
