// Op-level entry of the one-launch decode chain (chain.hip) over the C ABI (include/ferrum_hip.h): a test and diagnosis
// entry.  It fills a DecodeChainDesc from the public struct and calls decode_chain_f16 — the runner's launcher, unchanged: the
// same kernel instantiations, knobs and form counters.  What it adds is in front of the launch: every buffer comes with its
// capacity in bytes and is held against what the launch touches (chain_extents below restates the roles' index ranges), and
// the two device arrays that steer addresses — kv_lens and the block tables — are read back and range-checked.  Anything short,
// null or out of range is an error return, never a launch.  Host-only code; compiled with hipcc.
#include "../../include/ferrum_hip.h"
#include "abi_private.h"
#include "common.h"
#include "kernels.h"
#include "kv_layout.h"

#include <vector>

using namespace fh;

namespace {

struct Extent { const char* name; const void* ptr; size_t have, need; unsigned align = 16; };      // align: of the widest access the kernel makes

// What one launch reads or writes of every buffer, in bytes (need == 0: the form does not touch it).
std::vector<Extent> chain_extents(const FerrumHipDecodeChainDesc& d, int counter_words) {
    const size_t T = (size_t)d.T, H = (size_t)d.H, hd = 128;
    const size_t n_qkv = (size_t)(d.nq + 2 * d.nkv) * hd, row = T * H * 2;
    const bool moe = d.E > 0, a_moe = d.has_a && moe, a_rows = d.has_a && !moe && d.a_x, a_slabs = d.has_a && !moe && !d.a_x;
    const size_t tiles = moe ? (size_t)(d.E + 15) / 16 : 0;
    const int splits = d.attn_splits > 1 ? d.attn_splits : 1;
    return {
        // role A: down [T·top_k, H] fp16, comb_w [T·top_k] f32 | S slabs of [rows][a_ld] f32 | fp16 rows [T, H]
        {"down", d.down, d.down_bytes, a_moe ? T * (size_t)d.top_k * H * 2 : 0},
        {"comb_w", d.comb_w, d.comb_w_bytes, a_moe ? T * (size_t)d.top_k * 4 : 0, 4},
        {"a_slabs", d.a_slabs, d.a_slabs_bytes, a_slabs ? ((size_t)(d.a_S - 1) * (size_t)d.a_slab_stride + (T - 1) * (size_t)d.a_ld + H) * 4 : 0},
        {"a_x", d.a_x, d.a_x_bytes, a_rows ? row : 0},
        {"res_in", d.res_in, d.res_in_bytes, d.has_a ? row : 0},
        {"ln_in", d.ln_in, d.ln_in_bytes, d.has_a ? H * 2 : 0},
        {"res_a", d.res_a, d.res_a_bytes, row},                            // written by role A (or the caller), read by role B
        {"norm1", d.norm1, d.norm1_bytes, row},
        {"qkv_out", d.qkv_out, d.qkv_out_bytes, T * n_qkv * 2},
        // attention: norm weights with qk_mode 1, RoPE rows with qk_mode != 0 (their row count follows kv_lens: checked on the device values)
        {"q_norm_w", d.q_norm_w, d.q_norm_w_bytes, d.qk_mode == 1 ? hd * 2 : 0},
        {"k_norm_w", d.k_norm_w, d.k_norm_w_bytes, d.qk_mode == 1 ? hd * 2 : 0},
        {"cos_t", d.cos_t, d.cos_t_bytes, d.qk_mode != 0 ? hd / 2 * 4 : 0},
        {"sin_t", d.sin_t, d.sin_t_bytes, d.qk_mode != 0 ? hd / 2 * 4 : 0},
        {"k_pool", d.k_pool, d.k_pool_bytes, (size_t)d.nkv * KV_BLOCK * hd * 2},      // at least one block; the table's ids are checked below
        {"v_pool", d.v_pool, d.v_pool_bytes, (size_t)d.nkv * KV_BLOCK * hd * 2},
        {"block_tables", d.block_tables, d.block_tables_bytes, T * (size_t)d.max_blocks * 4, 4},
        {"kv_lens", d.kv_lens, d.kv_lens_bytes, T * 4, 4},
        {"attn_out", d.attn_out, d.attn_out_bytes, T * (size_t)d.nq * hd * 2},
        {"attn_partial", d.attn_partial, d.attn_partial_bytes, splits > 1 ? T * (size_t)d.nkv * splits * 16 * (hd + 4) * 4 : 0},
        {"attn_tickets", d.attn_tickets, d.attn_tickets_bytes, splits > 1 ? T * (size_t)d.nkv * 4 : 0, 4},
        {"o_part", d.o_part, d.o_part_bytes, 2 * T * H * 4},
        // role B
        {"res_b_out", d.res_b_out, d.res_b_out_bytes, row},
        {"post_ln", d.post_ln, d.post_ln_bytes, H * 2},
        {"norm2", d.norm2, d.norm2_bytes, row},
        {"router_w", d.router_w, d.router_w_bytes, tiles * 16 * H * 2},     // whole 16-expert tiles, [tile][H/32][64 lanes][8]
        {"cand", d.cand, d.cand_bytes, moe && d.defer_merge ? T * (size_t)d.Q * 8 * 8 : 0, 8},
        {"stats", d.stats, d.stats_bytes, moe && d.defer_merge ? T * (size_t)d.Q * 8 : 0, 8},
        {"ids", d.ids, d.ids_bytes, moe && !d.defer_merge ? T * (size_t)d.r_top_k * 4 : 0, 4},
        {"weights", d.weights, d.weights_bytes, moe && !d.defer_merge ? T * (size_t)d.r_top_k * 4 : 0, 4},
        {"cnt", d.cnt, d.cnt_bytes, (size_t)counter_words * 4},
        {"cnt_next", d.cnt_next, d.cnt_next_bytes, (size_t)counter_words * 4},
        {"timeout", d.timeout, d.timeout_bytes, 4, 4},
    };
}

// The internal descriptor of the public one.  The two W4Device copies live in `w` (a weightless handle — ferrum_hip_gptq_shape_only —
// answers the shape predicate as a loaded one of its shape would: `probe` stands in for its weight pointer there, never at a launch).
struct Lowered { W4Device w[2]; DecodeChainDesc d; };

int lower(const FerrumHipDecodeChainDesc& p, Lowered* out) {
    FH_REQUIRE(p.qkv && p.o, "decode_chain: null weight handle");
    static uint32_t probe;
    const FerrumHipGptq* hs[2] = {p.qkv, p.o};
    for (int i = 0; i < 2; i++) {
        out->w[i] = *gptq_device(hs[i]);
        if (gptq_is_shape_only(hs[i])) out->w[i].qw = &probe;
        else FH_REQUIRE(out->w[i].num_experts == 1, "decode_chain: handle is an expert stack");
    }
    DecodeChainDesc& d = out->d;
    d.T = p.T; d.H = p.H; d.nq = p.nq; d.nkv = p.nkv; d.head_dim = p.head_dim;
    d.has_a = p.has_a != 0; d.top_k = p.top_k;
    d.down = CH(p.down); d.comb_w = p.comb_w; d.res_in = CH(p.res_in); d.ln_in = CH(p.ln_in);
    d.a_slabs = p.a_slabs; d.a_S = p.a_S; d.a_slab_stride = (long)p.a_slab_stride; d.a_ld = p.a_ld; d.a_x = CH(p.a_x);
    d.eps = p.eps; d.res_a = H(p.res_a); d.norm1 = H(p.norm1);
    d.qkv = &out->w[0]; d.qkv_out = H(p.qkv_out);
    d.k_pool = H(p.k_pool); d.v_pool = H(p.v_pool); d.block_tables = p.block_tables; d.kv_lens = p.kv_lens;
    d.q_norm_w = CH(p.q_norm_w); d.k_norm_w = CH(p.k_norm_w); d.cos_t = p.cos_t; d.sin_t = p.sin_t;
    d.qk_mode = p.qk_mode; d.max_blocks = p.max_blocks; d.sliding_window = p.sliding_window;
    d.attn_out = H(p.attn_out);
    d.o = &out->w[1]; d.o_out = nullptr;
    d.res_b_out = H(p.res_b_out); d.post_ln = CH(p.post_ln); d.norm2 = H(p.norm2); d.router_w = CH(p.router_w);
    d.E = p.E; d.r_top_k = p.r_top_k; d.Q = p.Q; d.norm_topk = p.norm_topk; d.defer_merge = p.defer_merge != 0;
    d.cand = reinterpret_cast<RouteCand*>(p.cand); d.stats = p.stats; d.route_arrive = nullptr; d.ids = p.ids; d.weights = p.weights;
    d.o_part = p.o_part;
    d.attn_splits = p.attn_splits; d.attn_partial = p.attn_partial; d.attn_tickets = p.attn_tickets;
    d.cnt = p.cnt; d.cnt_next = p.cnt_next; d.timeout = p.timeout;
    return 0;
}

}  // namespace

extern "C" {

int ferrum_hip_decode_chain_counter_words(void) { return decode_chain_counter_words(); }

int ferrum_hip_decode_chain_supports(const FerrumHipDecodeChainDesc* desc) {
    Lowered l;
    if (!desc || lower(*desc, &l)) return 0;
    return decode_chain_supports(l.d) ? 1 : 0;
}

int ferrum_hip_decode_chain_f16(const FerrumHipDecodeChainDesc* desc, void* stream) {
    FH_REQUIRE(desc, "decode_chain: null descriptor");
    const FerrumHipDecodeChainDesc& p = *desc;
    Lowered l;
    if (int rc = lower(p, &l)) return rc;
    if (!decode_chain_supports(l.d)) { fh::set_error("decode_chain: shapes not taken by the merged form"); return FERRUM_HIP_UNSUPPORTED; }
    FH_REQUIRE(p.qk_mode >= 0 && p.qk_mode <= 3 && p.max_blocks >= 1 && p.sliding_window >= 0 && p.attn_splits >= 0,
               "decode_chain: qk_mode=%d max_blocks=%d sliding_window=%d attn_splits=%d", p.qk_mode, p.max_blocks, p.sliding_window, p.attn_splits);
    // (role A sums at most eight slabs: reduce_slabs8)
    FH_REQUIRE(!p.has_a || p.E > 0 || p.a_x || (p.a_slab_stride >= 0 && p.a_S >= 1 && p.a_S <= 8), "decode_chain: a_S=%d (1 … 8) a_slab_stride=%lld",
               p.a_S, (long long)p.a_slab_stride);
    for (const Extent& e : chain_extents(p, decode_chain_counter_words())) {
        if (e.need == 0) continue;
        FH_REQUIRE(e.ptr, "decode_chain: null %s (this form touches %zu bytes of it)", e.name, e.need);
        FH_REQUIRE(e.have >= e.need, "decode_chain: %s holds %zu bytes, the launch touches %zu", e.name, e.have, e.need);
        FH_REQUIRE(((uintptr_t)e.ptr & (e.align - 1)) == 0, "decode_chain: %s is not %u-byte aligned", e.name, e.align);
    }
    FH_REQUIRE(p.cnt != p.cnt_next, "decode_chain: cnt == cnt_next (the launch zeroes the other half while it counts in this one)");
    FH_REQUIRE(!gptq_is_shape_only(p.qkv) && !gptq_is_shape_only(p.o), "decode_chain: a shape-only handle carries no weights");
    // the device values that become addresses: 1 ≤ kv_len ≤ 16·max_blocks, a RoPE row per position, every block id the context
    // names inside both pools (a synchronous read-back: this entry is for tests and diagnosis, not for a captured step)
    std::vector<uint32_t> lens(p.T);
    std::vector<int32_t> bt((size_t)p.T * p.max_blocks);
    FH_CHECK_HIP(hipStreamSynchronize(ST(stream)));
    FH_CHECK_HIP(hipMemcpy(lens.data(), p.kv_lens, lens.size() * 4, hipMemcpyDeviceToHost));
    FH_CHECK_HIP(hipMemcpy(bt.data(), p.block_tables, bt.size() * 4, hipMemcpyDeviceToHost));
    const size_t block_bytes = (size_t)p.nkv * kv_tile_elems(128) * 2;
    const long pool_blocks = (long)(std::min(p.k_pool_bytes, p.v_pool_bytes) / block_bytes);
    for (int t = 0; t < p.T; t++) {
        const long n = lens[t];
        FH_REQUIRE(n >= 1 && n <= (long)p.max_blocks * KV_BLOCK, "decode_chain: kv_lens[%d] = %ld outside [1, %ld]", t, n, (long)p.max_blocks * KV_BLOCK);
        FH_REQUIRE(p.qk_mode == 0 || std::min(p.cos_t_bytes, p.sin_t_bytes) >= (size_t)n * 64 * 4,
                   "decode_chain: the RoPE tables hold fewer than kv_lens[%d] = %ld rows", t, n);
        for (long b = 0; b < (n + KV_BLOCK - 1) / KV_BLOCK; b++) {
            const long id = bt[(size_t)t * p.max_blocks + b];
            FH_REQUIRE(id >= 0 && id < pool_blocks, "decode_chain: block_tables[%d][%ld] = %ld outside the pools' %ld blocks", t, b, id, pool_blocks);
        }
    }
    return decode_chain_f16(l.d, ST(stream));
}

}  // extern "C"
