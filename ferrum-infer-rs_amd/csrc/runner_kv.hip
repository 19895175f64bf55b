// Decoder runner, sequences and their KV: the `ferrum_hip_model_*` admission, prefix-cache, truncate / fork / swap calls as
// argument checks over fh::SeqTable (seq_table.h: all of the bookkeeping, host-only) plus the device work they need — whole-block
// moves (kv_move.hip), the swap staging buffer and header — and the read-back calls of the tests (KV, taps, routing).
#include "runner.h"

using namespace fh;

static __global__ void f16_to_f32_kernel(const __half* __restrict__ src, float* __restrict__ dst, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = __half2float(src[i]);
}
void fh::f16_to_f32(const __half* src, float* dst, long n, hipStream_t s) {
    hipLaunchKernelGGL(f16_to_f32_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, src, dst, n);
}

static FerrumHipKvSlotReservation to_abi(const KvCapacity& c) { return {c.block_size, c.total_blocks, c.free_blocks_before, c.free_blocks_after}; }

extern "C" {

int ferrum_hip_model_kv_capacity_snapshot(const FerrumHipModel* m, FerrumHipKvSlotReservation* out) {
    FH_REQUIRE(m && out, "kv_capacity_snapshot: null");
    *out = to_abi(m->seqs->capacity_snapshot());
    return 0;
}

int ferrum_hip_model_reserve_kv_slots(FerrumHipModel* m, const FerrumHipKvSlotRequest* reqs, int n,
                                      FerrumHipKvSlotReservation* out) {
    FH_REQUIRE(m && (n == 0 || reqs), "reserve_kv_slots: null");
    KvCapacity cap{};
    if (int rc = m->seqs->reserve(reqs, n, &cap)) return rc;
    if (out) *out = to_abi(cap);
    return 0;
}

int ferrum_hip_model_release(FerrumHipModel* m, uint64_t seq_id) {
    FH_REQUIRE(m, "model_release: null");
    m->seqs->release(seq_id);
    return 0;
}

// ── block-level prefix cache (ferrum-models/src/models/qwen3_moe/prefix_cache.rs:66-235, prefill_decode.rs:10-70) ──
int ferrum_hip_block_hash_chain(const uint32_t* tokens, int n, int block_size, uint64_t* out, int capacity, int* count) {
    FH_REQUIRE((tokens || n == 0) && block_size > 0 && count, "block_hash_chain: bad argument");
    std::vector<uint64_t> h = fh::block_hash_chain(tokens, n, block_size);
    *count = (int)h.size();
    for (int i = 0; i < (int)h.size() && i < capacity; i++) out[i] = h[i];
    return 0;
}
uint64_t ferrum_hip_siphash(int c_rounds, int d_rounds, uint64_t k0, uint64_t k1, const uint8_t* data, size_t len) {
    return fh::siphash(c_rounds, d_rounds, k0, k1, data, len);
}

int ferrum_hip_model_prefix_cache_acquire(FerrumHipModel* m, uint64_t seq_id, const uint32_t* tokens, int n, int* cached_tokens) {
    FH_REQUIRE(m && tokens && n > 0 && cached_tokens, "prefix_cache_acquire: bad argument");
    return m->seqs->prefix_acquire(seq_id, tokens, n, cached_tokens);
}

int ferrum_hip_model_prefix_cache_register(FerrumHipModel* m, uint64_t seq_id, const uint32_t* all_tokens, int n,
                                           int prior_cached_tokens) {
    FH_REQUIRE(m && all_tokens && n >= 0 && prior_cached_tokens >= 0, "prefix_cache_register: bad argument");
    return m->seqs->prefix_register(seq_id, all_tokens, n, prior_cached_tokens);
}

int ferrum_hip_model_prefix_cache_stats(const FerrumHipModel* m, uint64_t* hits, uint64_t* misses, uint64_t* saved_prefill_tokens,
                                        uint64_t* entries) {
    FH_REQUIRE(m, "prefix_cache_stats: null");
    m->seqs->prefix_stats(hits, misses, saved_prefill_tokens, entries);
    return 0;
}

int ferrum_hip_model_block_table(const FerrumHipModel* m, uint64_t seq_id, uint32_t* blocks, int capacity,
                                 int* num_blocks, int* kv_len) {
    FH_REQUIRE(m, "model_block_table: null");
    const SeqState* st = m->seqs->find(seq_id);
    FH_REQUIRE(st, "model_block_table: unknown sequence %llu", (unsigned long long)seq_id);
    int nb = (int)st->blocks.size();
    if (num_blocks) *num_blocks = nb;
    if (kv_len) *kv_len = st->len;
    for (int i = 0; i < nb && i < capacity; i++) blocks[i] = st->blocks[i];
    return 0;
}

int ferrum_hip_model_read_kv_f32(FerrumHipModel* m, uint64_t seq_id, int layer, int is_v, float* out_host) {
    FH_REQUIRE(m && m->finalized && out_host && layer >= 0 && layer < m->cfg.num_layers, "model_read_kv: bad argument");
    const SeqState* stp = m->seqs->find(seq_id);
    FH_REQUIRE(stp, "model_read_kv: unknown sequence");
    const SeqState& st = *stp;
    if (st.len == 0) return 0;
    const FerrumHipModelConfig& c = m->cfg;
    size_t n = (size_t)st.len * c.num_kv_heads * c.head_dim;
    __half *kd = nullptr, *vd = nullptr;
    float* fd = nullptr;
    int32_t* bt = nullptr;
    FH_CHECK_HIP(hipMalloc((void**)&kd, n * 2));
    FH_CHECK_HIP(hipMalloc((void**)&vd, n * 2));
    FH_CHECK_HIP(hipMalloc((void**)&fd, n * 4));
    FH_CHECK_HIP(hipMalloc((void**)&bt, st.blocks.size() * 4));
    FH_CHECK_HIP(hipMemcpy(bt, st.blocks.data(), st.blocks.size() * 4, hipMemcpyHostToDevice));
    int rc = paged_kv_read_f16(m->layers[layer].k_pool, m->layers[layer].v_pool, bt, st.len, c.num_kv_heads, c.head_dim,
                               KV_BLOCK, kd, vd, m->stream);
    if (!rc) {
        f16_to_f32(is_v ? vd : kd, fd, (long)n, m->stream);
        (void)hipMemcpyAsync(out_host, fd, n * 4, hipMemcpyDeviceToHost, m->stream);
        (void)hipStreamSynchronize(m->stream);
    }
    (void)hipFree(kd); (void)hipFree(vd); (void)hipFree(fd); (void)hipFree(bt);
    return rc;
}

// ── sequence KV lifecycle: truncate, copy-on-write fork, host swap (include/ferrum_hip.h) ──────────────────────────────
// All of it is whole-block copying (kv_move.hip) plus allocator bookkeeping.  Every call validates and allocates first, moves,
// waits for the stream, and only then commits the host state: a failure returns with the model as it was.
static size_t kv_chunk_bytes(const FerrumHipModelConfig& c) { return (size_t)c.num_kv_heads * kv_tile_elems(c.head_dim) * sizeof(__half); }
static size_t kv_block_bytes(const FerrumHipModelConfig& c) { return kv_chunk_bytes(c) * 2 * (size_t)c.num_layers; }   // every layer, K and V
constexpr size_t KV_STAGING_CAP_BYTES = (size_t)64 << 20;   // a longer sequence swaps in block ranges of this size
constexpr size_t KV_SWAP_HEADER_BYTES = 32;
constexpr uint32_t KV_SWAP_MAGIC = 0x564B4846u, KV_SWAP_VERSION = 1u;   // "FHKV"

// pairs: (src, dst) u32 pairs of one move, uploaded through the growable device list.  The caller waits for the stream before
// `pairs` goes away.
static int kv_move(FerrumHipModel* m, const std::vector<uint32_t>& pairs, int mode) {
    const size_t n = pairs.size() / 2;
    if (!n) return 0;
    if (int rc = grow_device((void**)&m->kv_pairs_dev, &m->kv_pairs_bytes, std::max<size_t>(n, 256) * 8, m->stream)) return rc;
    FH_CHECK_HIP(hipMemcpyAsync(m->kv_pairs_dev, pairs.data(), n * 8, hipMemcpyHostToDevice, m->stream));
    return kv_move_blocks(m->kv_pools_dev, 2 * m->cfg.num_layers, m->kv_pairs_dev, (int)n, m->kv_staging, kv_chunk_bytes(m->cfg),
                          m->cfg.kv_num_blocks, mode, m->stream);
}

// pool → pool copy of one block of every layer, finished when this returns
static int kv_copy_block(FerrumHipModel* m, uint32_t src, uint32_t dst) {
    const std::vector<uint32_t> pair = {src, dst};
    if (int rc = kv_move(m, pair, KV_MOVE_POOL)) return rc;
    FH_CHECK_HIP(hipStreamSynchronize(m->stream));
    return 0;
}

// blocks one staging pass of a swap carries (≥ 1), and the staging buffer grown to hold min(num_blocks, that many)
static int kv_staging_for(FerrumHipModel* m, int num_blocks, int* per_pass) {
    const size_t bb = kv_block_bytes(m->cfg);
    *per_pass = (int)std::max<size_t>(1, KV_STAGING_CAP_BYTES / bb);
    const size_t want = bb * (size_t)std::min(num_blocks, *per_pass);
    return grow_device((void**)&m->kv_staging, &m->kv_staging_bytes, want, m->stream);
}

int ferrum_hip_model_truncate_kv(FerrumHipModel* m, uint64_t seq_id, int new_len) {
    FH_REQUIRE(m && m->finalized, "model_truncate_kv: model null or not finalized");
    FH_REQUIRE(new_len >= 0, "model_truncate_kv: new_len=%d", new_len);
    return m->seqs->truncate(seq_id, new_len, [m](uint32_t src, uint32_t dst) { return kv_copy_block(m, src, dst); });
}

int ferrum_hip_model_fork(FerrumHipModel* m, uint64_t src_seq_id, uint64_t dst_seq_id) {
    FH_REQUIRE(m && m->finalized, "model_fork: model null or not finalized");
    return m->seqs->fork(src_seq_id, dst_seq_id, [m](uint32_t src, uint32_t dst) { return kv_copy_block(m, src, dst); });
}

int ferrum_hip_model_block_info(const FerrumHipModel* m, uint32_t block, uint32_t* ref_count, int* hashed) {
    FH_REQUIRE(m && m->seqs, "model_block_info: null model");
    return m->seqs->block_info(block, ref_count, hashed);
}

int ferrum_hip_model_kv_swap_bytes(const FerrumHipModel* m, uint64_t seq_id, size_t* bytes) {
    FH_REQUIRE(m && m->finalized && bytes, "model_kv_swap_bytes: null argument or model not finalized");
    const SeqState* st = m->seqs->find(seq_id);
    FH_REQUIRE(st, "model_kv_swap_bytes: unknown sequence %llu", (unsigned long long)seq_id);
    *bytes = KV_SWAP_HEADER_BYTES + (size_t)m->seqs->blocks_for(st->len) * kv_block_bytes(m->cfg);
    return 0;
}

int ferrum_hip_model_kv_swap_out(FerrumHipModel* m, uint64_t seq_id, void* host_buf, size_t capacity, size_t* written) {
    FH_REQUIRE(m && m->finalized && host_buf && written, "model_kv_swap_out: null argument or model not finalized");
    const SeqState* stp = m->seqs->find(seq_id);
    FH_REQUIRE(stp, "model_kv_swap_out: unknown sequence %llu", (unsigned long long)seq_id);
    const FerrumHipModelConfig& c = m->cfg;
    const SeqState& st = *stp;
    const std::vector<uint32_t> blocks = m->seqs->swap_out_blocks(st);
    const int nb = (int)blocks.size();
    const size_t bb = kv_block_bytes(c), need = KV_SWAP_HEADER_BYTES + (size_t)nb * bb;
    FH_REQUIRE(capacity >= need, "model_kv_swap_out: sequence %llu needs %zu bytes, the buffer holds %zu", (unsigned long long)seq_id, need, capacity);
    int per = 1;
    if (int rc = kv_staging_for(m, nb, &per)) return rc;
    const uint32_t header[8] = {KV_SWAP_MAGIC, KV_SWAP_VERSION, (uint32_t)c.num_layers, (uint32_t)c.num_kv_heads, (uint32_t)c.head_dim,
                                (uint32_t)KV_BLOCK, (uint32_t)st.len, (uint32_t)nb};
    static_assert(sizeof(header) == KV_SWAP_HEADER_BYTES, "swap header is 32 bytes");
    memcpy(host_buf, header, sizeof(header));
    uint8_t* payload = static_cast<uint8_t*>(host_buf) + KV_SWAP_HEADER_BYTES;
    std::vector<uint32_t> pairs;
    for (int b0 = 0; b0 < nb; b0 += per) {
        const int n = std::min(per, nb - b0);
        pairs.clear();
        for (int i = 0; i < n; i++) { pairs.push_back(blocks[b0 + i]); pairs.push_back(0); }
        if (int rc = kv_move(m, pairs, KV_MOVE_GATHER)) return rc;
        FH_CHECK_HIP(hipMemcpyAsync(payload + (size_t)b0 * bb, m->kv_staging, (size_t)n * bb, hipMemcpyDeviceToHost, m->stream));
        FH_CHECK_HIP(hipStreamSynchronize(m->stream));     // the staging buffer is reused by the next range
    }
    *written = need;
    m->seqs->release(seq_id);
    return 0;
}

int ferrum_hip_model_kv_swap_in(FerrumHipModel* m, uint64_t seq_id, const void* host_buf, size_t bytes) {
    FH_REQUIRE(m && m->finalized && host_buf, "model_kv_swap_in: null argument or model not finalized");
    FH_REQUIRE(bytes >= KV_SWAP_HEADER_BYTES, "model_kv_swap_in: %zu bytes hold no header", bytes);
    const FerrumHipModelConfig& c = m->cfg;
    uint32_t h[8];
    memcpy(h, host_buf, sizeof(h));
    FH_REQUIRE(h[0] == KV_SWAP_MAGIC && h[1] == KV_SWAP_VERSION, "model_kv_swap_in: not a KV swap buffer (magic %08x, version %u)", h[0], h[1]);
    FH_REQUIRE(h[2] == (uint32_t)c.num_layers && h[3] == (uint32_t)c.num_kv_heads && h[4] == (uint32_t)c.head_dim && h[5] == (uint32_t)KV_BLOCK,
               "model_kv_swap_in: buffer is of a model with %u layers, %u kv heads, head_dim %u, block %u; this one has %d, %d, %d, %d",
               h[2], h[3], h[4], h[5], c.num_layers, c.num_kv_heads, c.head_dim, KV_BLOCK);
    FH_REQUIRE(h[6] <= (uint32_t)c.max_seq_len && h[7] == (uint32_t)cdiv(h[6], KV_BLOCK) && (int)h[7] <= m->max_blocks_per_seq,
               "model_kv_swap_in: kv length %u in %u blocks does not fit this model (max_seq_len %d)", h[6], h[7], c.max_seq_len);
    const int len = (int)h[6], nb = (int)h[7];
    const size_t bb = kv_block_bytes(c);
    FH_REQUIRE(bytes == KV_SWAP_HEADER_BYTES + (size_t)nb * bb, "model_kv_swap_in: %zu bytes given, the header describes %zu", bytes,
               KV_SWAP_HEADER_BYTES + (size_t)nb * bb);
    std::vector<uint32_t> blocks;
    if (int rc = m->seqs->swap_in_allocate(seq_id, nb, &blocks)) return rc;
    int per = 1;
    if (int rc = kv_staging_for(m, nb, &per)) { m->seqs->give_back(blocks); return rc; }
    const uint8_t* payload = static_cast<const uint8_t*>(host_buf) + KV_SWAP_HEADER_BYTES;
    auto scatter = [&]() -> int {
        std::vector<uint32_t> pairs;
        for (int b0 = 0; b0 < nb; b0 += per) {
            const int n = std::min(per, nb - b0);
            pairs.clear();
            for (int i = 0; i < n; i++) { pairs.push_back(0); pairs.push_back(blocks[b0 + i]); }
            FH_CHECK_HIP(hipMemcpyAsync(m->kv_staging, payload + (size_t)b0 * bb, (size_t)n * bb, hipMemcpyHostToDevice, m->stream));
            if (int rc = kv_move(m, pairs, KV_MOVE_SCATTER)) return rc;
            FH_CHECK_HIP(hipStreamSynchronize(m->stream));
        }
        return 0;
    };
    if (int rc = scatter()) { m->seqs->give_back(blocks); return rc; }
    m->seqs->commit(seq_id, std::move(blocks), len);
    return 0;
}

int ferrum_hip_model_enable_taps(FerrumHipModel* m, int enable) {
    FH_REQUIRE(m && m->finalized, "model_enable_taps: bad state");
    m->taps_enabled = enable != 0;
    if (m->taps_enabled && !m->taps)
        return dev_alloc(&m->taps, (size_t)m->cfg.num_layers * m->cfg.max_tokens * m->cfg.hidden);
    return 0;
}
int ferrum_hip_model_read_taps(FerrumHipModel* m, float* out_host, int max_tokens) {
    FH_REQUIRE(m && m->taps && out_host, "model_read_taps: taps not enabled");
    const int T = std::min(max_tokens, m->taps_tokens);
    for (int li = 0; li < m->cfg.num_layers; li++)
        FH_CHECK_HIP(hipMemcpy(out_host + (size_t)li * max_tokens * m->cfg.hidden,
                               m->taps + (size_t)li * m->cfg.max_tokens * m->cfg.hidden,
                               (size_t)T * m->cfg.hidden * 4, hipMemcpyDeviceToHost));
    return 0;
}
int ferrum_hip_model_read_routing(FerrumHipModel* m, int32_t* ids_host, float* weights_host, int pairs) {
    FH_REQUIRE(m && m->finalized && ids_host && weights_host, "model_read_routing: bad state");
    FH_REQUIRE(m->expert_ids && m->expert_w && pairs >= 1 && pairs <= m->cfg.max_tokens * std::max(m->cfg.top_k, 1),
               "model_read_routing: not a MoE model, or pairs=%d out of range", pairs);
    FH_CHECK_HIP(hipStreamSynchronize(m->stream));
    FH_CHECK_HIP(hipMemcpy(ids_host, m->expert_ids, (size_t)pairs * 4, hipMemcpyDeviceToHost));
    FH_CHECK_HIP(hipMemcpy(weights_host, m->expert_w, (size_t)pairs * 4, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
