// Host-side sequence / KV bookkeeping of the runner: which physical blocks each sequence holds and how many tokens they
// carry, over BlockAllocator.  reserve_paged_kv_slots (llama_family.rs:2255) + PagedSeqState::ensure_capacity
// (paged_pool.rs:416-442), the block-level prefix cache (qwen3_moe/prefix_cache.rs:66-235, prefill_decode.rs:10-70), and the
// bookkeeping half of truncate / copy-on-write fork / host swap (include/ferrum_hip.h).
// Pure host code, no HIP: device work is the caller's.  Every operation validates and allocates first, lets the caller move
// the data (the injected block copy; the swap's gather / scatter), and only then commits: a failure returns the error code
// with the table as it was.
#pragma once
#include <algorithm>
#include <unordered_map>
#include <utility>
#include <vector>

#include "block_allocator.h"
#include "error.h"

namespace fh {

struct SeqState {
    std::vector<uint32_t> blocks;
    int len = 0;
};

// KvSlotReservation (model_executor.rs:24-64)
struct KvCapacity { int block_size, total_blocks, free_blocks_before, free_blocks_after; };

class SeqTable {
public:
    SeqTable(uint32_t num_blocks, int block_size, int max_blocks_per_seq)
        : alloc_(num_blocks), bs_(block_size), max_blocks_per_seq_(max_blocks_per_seq) {}

    KvCapacity capacity_snapshot() const {
        const int free = (int)alloc_.free_count();
        return {bs_, (int)alloc_.capacity(), free, free};
    }

    // All-or-nothing over the n requests (anything with .seq_id and .target_len): nothing is allocated unless all of them fit.
    template <typename Req>
    int reserve(const Req* reqs, int n, KvCapacity* out) {
        const int before = (int)alloc_.free_count();
        long need = 0;
        for (int i = 0; i < n; i++) {
            const int blocks = blocks_for(reqs[i].target_len);
            FH_REQUIRE(blocks <= max_blocks_per_seq_, "paged KV: target_len=%d would need %d blocks, exceeds max_blocks_per_seq=%d",
                       reqs[i].target_len, blocks, max_blocks_per_seq_);
            const SeqState* st = find(reqs[i].seq_id);
            const int have = st ? (int)st->blocks.size() : 0;
            if (blocks > have) need += blocks - have;
        }
        FH_REQUIRE(need <= before, "paged KV pool exhausted: need %ld blocks but only %d free", need, before);
        for (int i = 0; i < n; i++) {
            SeqState& st = seqs_[reqs[i].seq_id];
            const int blocks = blocks_for(reqs[i].target_len);
            while ((int)st.blocks.size() < blocks) {
                uint32_t b;
                alloc_.allocate(&b);
                st.blocks.push_back(b);
            }
        }
        if (out) *out = {bs_, (int)alloc_.capacity(), before, (int)alloc_.free_count()};
        return 0;
    }

    void release(uint64_t seq_id) {
        auto it = seqs_.find(seq_id);
        if (it == seqs_.end()) return;
        alloc_.free(it->second.blocks.data(), (uint32_t)it->second.blocks.size());
        seqs_.erase(it);
    }

    // null for an unknown sequence
    const SeqState* find(uint64_t seq_id) const {
        auto it = seqs_.find(seq_id);
        return it == seqs_.end() ? nullptr : &it->second;
    }
    int len(uint64_t seq_id) const {
        const SeqState* st = find(seq_id);
        return st ? st->len : 0;
    }
    // a forward wrote n more tokens of the sequence
    void advance(uint64_t seq_id, int n) {
        if (SeqState* st = find_mut(seq_id)) st->len += n;
    }
    int blocks_for(int len) const { return (len + bs_ - 1) / bs_; }

    // ── block-level prefix cache ──
    int prefix_acquire(uint64_t seq_id, const uint32_t* tokens, int n, int* cached_tokens) {
        *cached_tokens = 0;
        SeqState* stp = find_mut(seq_id);
        FH_REQUIRE(stp, "prefix_cache_acquire: reserve KV slots for sequence %llu first", (unsigned long long)seq_id);
        SeqState& st = *stp;
        FH_REQUIRE(st.len == 0, "prefix_cache_acquire: sequence %llu already holds %d tokens", (unsigned long long)seq_id, st.len);
        const std::vector<uint64_t> hashes = block_hash_chain(tokens, n, bs_);
        // longest contiguous prefix: stop at the first miss
        std::vector<uint32_t> matched;
        for (uint64_t h : hashes) {
            if (matched.size() >= st.blocks.size()) break;
            int64_t b = alloc_.try_acquire_by_hash(h);
            if (b < 0) break;
            matched.push_back((uint32_t)b);
        }
        if (matched.empty()) {
            prefix_misses_++;
            return 0;
        }
        // the freshly reserved blocks in the matched slots go back to the pool; the cached ids take their place
        alloc_.free(st.blocks.data(), (uint32_t)matched.size());
        for (size_t i = 0; i < matched.size(); i++) st.blocks[i] = matched[i];
        int cached = (int)matched.size() * bs_;
        // a full hit keeps one block's worth to re-run so the forward still yields final logits (prefill_decode.rs:34-48);
        // the suffix then rewrites the shared block with identical content
        if (cached >= n) cached = std::min(std::max(cached - bs_, 0), n - 1);
        st.len = cached;
        if (cached > 0) { prefix_hits_++; prefix_saved_tokens_ += (uint64_t)cached; } else { prefix_misses_++; }
        *cached_tokens = cached;
        return 0;
    }

    int prefix_register(uint64_t seq_id, const uint32_t* all_tokens, int n, int prior_cached_tokens) {
        const SeqState* st = find(seq_id);
        FH_REQUIRE(st, "prefix_cache_register: unknown sequence %llu", (unsigned long long)seq_id);
        const std::vector<uint64_t> hashes = block_hash_chain(all_tokens, n, bs_);
        // only blocks whose slots were all written: (i + 1)·block ≤ kv length
        for (size_t i = (size_t)prior_cached_tokens / bs_; i < hashes.size() && i < st->blocks.size(); i++) {
            if ((int)(i + 1) * bs_ > st->len) break;
            alloc_.register_block_hash(st->blocks[i], hashes[i]);
        }
        return 0;
    }

    void prefix_stats(uint64_t* hits, uint64_t* misses, uint64_t* saved_prefill_tokens, uint64_t* entries) const {
        if (hits) *hits = prefix_hits_;
        if (misses) *misses = prefix_misses_;
        if (saved_prefill_tokens) *saved_prefill_tokens = prefix_saved_tokens_;
        if (entries) *entries = alloc_.hash_table_size();
    }

    // ── truncate, copy-on-write fork ──
    // copy_block(src, dst) → int: a FINISHED pool → pool copy of one block (every layer); non-zero = failed, and is what the call returns
    template <typename Copy>
    int truncate(uint64_t seq_id, int new_len, Copy&& copy_block) {
        SeqState* stp = find_mut(seq_id);
        FH_REQUIRE(stp, "model_truncate_kv: unknown sequence %llu", (unsigned long long)seq_id);
        SeqState& st = *stp;
        if (new_len >= st.len) return 0;
        const size_t keep = (size_t)blocks_for(new_len);
        if (new_len % bs_) {
            // the block that becomes partial is the one the next forward writes into: another sequence's (fork, prefix hit) or the
            // prefix cache's view of it must not change, so the sequence takes a private copy first
            const size_t idx = (size_t)new_len / bs_;
            const uint32_t old = st.blocks[idx];
            if (alloc_.ref_count(old) > 1 || alloc_.has_hash(old)) {
                uint32_t fresh;
                FH_REQUIRE(alloc_.allocate(&fresh), "model_truncate_kv: sequence %llu shares block %u, which the cut at %d makes partial, and no "
                           "block is free for a private copy", (unsigned long long)seq_id, old, new_len);
                if (int rc = copy_block(old, fresh)) { alloc_.free(&fresh, 1); return rc; }
                st.blocks[idx] = fresh;
                alloc_.free(&old, 1);      // a hashed block stays a (soft-free) cache entry
            }
        }
        if (st.blocks.size() > keep) {
            alloc_.free(st.blocks.data() + keep, (uint32_t)(st.blocks.size() - keep));
            st.blocks.resize(keep);
        }
        st.len = new_len;
        return 0;
    }

    template <typename Copy>
    int fork(uint64_t src_seq_id, uint64_t dst_seq_id, Copy&& copy_block) {
        const SeqState* src = find(src_seq_id);
        FH_REQUIRE(src && src->len > 0, "model_fork: source sequence %llu is unknown or empty", (unsigned long long)src_seq_id);
        FH_REQUIRE(!find(dst_seq_id), "model_fork: destination sequence %llu exists", (unsigned long long)dst_seq_id);
        const int len = src->len;
        const size_t full = (size_t)len / bs_;
        // full blocks are shared; blocks the source reserved beyond its length are not inherited
        std::vector<uint32_t> blocks(src->blocks.begin(), src->blocks.begin() + blocks_for(len));
        for (size_t i = 0; i < full; i++)
            FH_REQUIRE(alloc_.ref_count(blocks[i]) < 0xFFFF, "model_fork: block %u is already shared 65535 times", blocks[i]);
        if (len % bs_) {       // the partial tail is where both sequences write next: the fork gets its own copy now
            uint32_t fresh;
            FH_REQUIRE(alloc_.allocate(&fresh), "model_fork: no free block for the copy of the partial last block (kv length %d)", len);
            if (int rc = copy_block(blocks[full], fresh)) { alloc_.free(&fresh, 1); return rc; }
            blocks[full] = fresh;
        }
        for (size_t i = 0; i < full; i++) alloc_.acquire(blocks[i]);
        commit(dst_seq_id, std::move(blocks), len);
        return 0;
    }

    int block_info(uint32_t block, uint32_t* ref_count, int* hashed) const {
        FH_REQUIRE(block < alloc_.capacity(), "model_block_info: block %u outside the pool of %u", block, alloc_.capacity());
        if (ref_count) *ref_count = alloc_.ref_count(block);
        if (hashed) *hashed = alloc_.has_hash(block) ? 1 : 0;
        return 0;
    }

    // ── host swap ──
    // out: the blocks that hold the sequence's tokens, in order (reserved-but-unused ones carry nothing); the caller gathers
    // them and then releases the sequence
    std::vector<uint32_t> swap_out_blocks(const SeqState& st) const {
        return std::vector<uint32_t>(st.blocks.begin(), st.blocks.begin() + blocks_for(st.len));
    }
    // in: nb fresh blocks for a sequence that must not exist yet; after the scatter the caller commits them, or gives them back
    int swap_in_allocate(uint64_t seq_id, int nb, std::vector<uint32_t>* blocks) {
        FH_REQUIRE(!find(seq_id), "model_kv_swap_in: sequence %llu exists", (unsigned long long)seq_id);
        FH_REQUIRE((int)alloc_.free_count() >= nb, "paged KV pool exhausted: swap-in needs %d blocks but only %u free", nb, alloc_.free_count());
        blocks->resize((size_t)nb);
        if (nb) alloc_.allocate_n((uint32_t)nb, blocks->data());
        return 0;
    }
    void commit(uint64_t seq_id, std::vector<uint32_t>&& blocks, int len) {
        SeqState& st = seqs_[seq_id];
        st.blocks = std::move(blocks);
        st.len = len;
    }
    void give_back(const std::vector<uint32_t>& blocks) { alloc_.free(blocks.data(), (uint32_t)blocks.size()); }

private:
    SeqState* find_mut(uint64_t seq_id) {
        auto it = seqs_.find(seq_id);
        return it == seqs_.end() ? nullptr : &it->second;
    }

    BlockAllocator alloc_;
    const int bs_, max_blocks_per_seq_;
    std::unordered_map<uint64_t, SeqState> seqs_;
    uint64_t prefix_hits_ = 0, prefix_misses_ = 0, prefix_saved_tokens_ = 0;   // block-level prefix cache probes
};

}  // namespace fh
