// Stand-alone check of fh::SeqTable (csrc/seq_table.h), the runner's host-only sequence / KV bookkeeping: built and run by
// tests/test_seq_table.py with plain g++ (under AddressSanitizer + UBSan where the toolchain links them), no GPU, no library.
// The block copy that truncate and fork need is injected: here it records (src, dst) and can be told to fail — the failure
// paths a real card cannot be made to take.
// Shapes: block size 16, a pool of 8 blocks, max_blocks_per_seq 4, lengths 0 / 15 / 16 / 17 / 33.
//   usage: seq_table_check <reserve|prefix|fork|truncate|swap|advance>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "seq_table.h"

static std::string g_err;
namespace fh {
void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}
}  // namespace fh

using fh::SeqTable;
using Blocks = std::vector<uint32_t>;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        g_checked++;                                                                     \
        if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s   (last error: %s)\n", __FILE__, __LINE__, #cond, g_err.c_str()); } \
    } while (0)
// the call fails with code 2 and the error text names `word`
#define CHECK_REFUSED(call, word)                                \
    do {                                                         \
        g_err.clear();                                           \
        CHECK((call) == 2);                                      \
        CHECK(g_err.find(word) != std::string::npos);            \
    } while (0)

struct Req { uint64_t seq_id; int target_len; };
struct Copier {
    std::vector<std::pair<uint32_t, uint32_t>> calls;
    int fail_rc = 0;
    int operator()(uint32_t src, uint32_t dst) { calls.push_back({src, dst}); return fail_rc; }
};

static int free_count(const SeqTable& t) { return t.capacity_snapshot().free_blocks_after; }
static uint32_t refs(const SeqTable& t, uint32_t b) { uint32_t r = 99; t.block_info(b, &r, nullptr); return r; }
static bool hashed(const SeqTable& t, uint32_t b) { int h = -1; t.block_info(b, nullptr, &h); return h == 1; }
static Blocks blocks(const SeqTable& t, uint64_t seq) { return t.find(seq) ? t.find(seq)->blocks : Blocks{0xdead}; }
static int reserve1(SeqTable& t, uint64_t seq, int len) { Req r{seq, len}; return t.reserve(&r, 1, nullptr); }
static Blocks tokens(int n, uint32_t base) { Blocks v(n); for (int i = 0; i < n; i++) v[i] = base + 7u * i; return v; }

static void check_reserve() {
    SeqTable t(8, 16, 4);
    fh::KvCapacity cap = t.capacity_snapshot();
    CHECK(cap.block_size == 16 && cap.total_blocks == 8 && cap.free_blocks_before == 8 && cap.free_blocks_after == 8);
    // ids come out 0, 1, 2, …; ceil(len / 16) blocks: 0 → 0, 15 → 1, 16 → 1, 17 → 2, 33 → 3
    Req r1{1, 33};
    CHECK(t.reserve(&r1, 1, &cap) == 0);
    CHECK(cap.block_size == 16 && cap.total_blocks == 8 && cap.free_blocks_before == 8 && cap.free_blocks_after == 5);
    CHECK((blocks(t, 1) == Blocks{0, 1, 2}) && t.len(1) == 0);
    CHECK(reserve1(t, 9, 0) == 0 && t.find(9) && blocks(t, 9).empty() && free_count(t) == 5);
    CHECK(reserve1(t, 2, 15) == 0 && blocks(t, 2) == Blocks{3});
    CHECK(reserve1(t, 2, 16) == 0 && blocks(t, 2) == Blocks{3} && free_count(t) == 4);
    CHECK(reserve1(t, 2, 17) == 0 && (blocks(t, 2) == Blocks{3, 4}) && free_count(t) == 3);
    CHECK(reserve1(t, 2, 1) == 0 && (blocks(t, 2) == Blocks{3, 4}));          // a reservation never shrinks
    CHECK(t.reserve((const Req*)nullptr, 0, nullptr) == 0 && free_count(t) == 3);
    // … and come back LIFO after a release
    t.release(2);
    t.release(77);                                                            // unknown: nothing happens
    CHECK(!t.find(2) && free_count(t) == 5);
    CHECK(reserve1(t, 3, 17) == 0 && (blocks(t, 3) == Blocks{4, 3}));
    // a target over max_blocks_per_seq (65 tokens = 5 blocks > 4) is rejected before anything is allocated, also as the last request
    CHECK_REFUSED(reserve1(t, 5, 65), "max_blocks_per_seq");
    Req over[2] = {{6, 16}, {5, 65}};
    CHECK_REFUSED(t.reserve(over, 2, nullptr), "max_blocks_per_seq");
    CHECK(!t.find(5) && !t.find(6) && free_count(t) == 3);
    SeqTable u(8, 16, 4);
    CHECK(reserve1(u, 5, 64) == 0 && blocks(u, 5).size() == 4);               // exactly the maximum fits
    // all-or-nothing: sequence 1 holds 3 blocks, 3 holds 2, two are free; 1 → 4 and 3 → 4 blocks need three
    CHECK(reserve1(t, 4, 16) == 0 && free_count(t) == 2);
    Req both[2] = {{1, 64}, {3, 64}};
    cap = {-1, -1, -1, -1};
    CHECK_REFUSED(t.reserve(both, 2, &cap), "exhausted");
    CHECK(free_count(t) == 2 && (blocks(t, 1) == Blocks{0, 1, 2}) && (blocks(t, 3) == Blocks{4, 3}) && cap.free_blocks_after == -1);
    Req new_one[2] = {{1, 64}, {8, 33}};                                      // the same with a sequence the table has not seen
    CHECK_REFUSED(t.reserve(new_one, 2, nullptr), "exhausted");
    CHECK(free_count(t) == 2 && !t.find(8) && blocks(t, 1).size() == 3);
    both[1].target_len = 48;                                                  // one block each: fits exactly
    CHECK(t.reserve(both, 2, &cap) == 0 && cap.free_blocks_before == 2 && cap.free_blocks_after == 0);
    CHECK(blocks(t, 1).size() == 4 && blocks(t, 3).size() == 3 && free_count(t) == 0);
}

static void check_prefix() {
    SeqTable t(8, 16, 4);
    const Blocks p = tokens(33, 100);
    uint64_t hits = 9, misses = 9, saved = 9, entries = 9;
    int cached = -1;
    // register hashes only fully written blocks, (i + 1)·16 ≤ len — whatever the token list holds
    CHECK(reserve1(t, 1, 33) == 0);
    t.advance(1, 17);
    CHECK(t.prefix_register(1, p.data(), 33, 0) == 0);
    CHECK(hashed(t, 0) && !hashed(t, 1) && !hashed(t, 2));
    t.advance(1, 16);                                                          // len 33: block 1 is full now, block 2 holds one token
    CHECK(t.prefix_register(1, p.data(), 33, 16) == 0);
    CHECK(hashed(t, 0) && hashed(t, 1) && !hashed(t, 2));
    t.prefix_stats(&hits, &misses, &saved, &entries);
    CHECK(hits == 0 && misses == 0 && saved == 0 && entries == 2);
    CHECK_REFUSED(t.prefix_register(42, p.data(), 33, 0), "unknown sequence");
    // a hit on both full blocks: the cached ids replace the reserved ones, which go back to the pool
    CHECK(reserve1(t, 2, 33) == 0 && (blocks(t, 2) == Blocks{3, 4, 5}) && free_count(t) == 2);
    CHECK(t.prefix_acquire(2, p.data(), 33, &cached) == 0 && cached == 32 && t.len(2) == 32);
    CHECK((blocks(t, 2) == Blocks{0, 1, 5}) && free_count(t) == 4 && refs(t, 0) == 2 && refs(t, 1) == 2 && refs(t, 3) == 0 && refs(t, 4) == 0);
    // acquire stops at the first miss: same first block, another second block
    Blocks q = p;
    for (int i = 16; i < 33; i++) q[i] += 1;
    CHECK(reserve1(t, 3, 33) == 0 && free_count(t) == 1);
    const Blocks reserved3 = blocks(t, 3);
    CHECK(t.prefix_acquire(3, q.data(), 33, &cached) == 0 && cached == 16 && t.len(3) == 16);
    CHECK(blocks(t, 3)[0] == 0 && blocks(t, 3)[1] == reserved3[1] && blocks(t, 3)[2] == reserved3[2]);
    CHECK(free_count(t) == 2 && refs(t, 0) == 3 && refs(t, 1) == 2 && refs(t, reserved3[0]) == 0);
    t.prefix_stats(&hits, &misses, &saved, nullptr);
    CHECK(hits == 2 && misses == 0 && saved == 48);
    // a full hit of n = 32 keeps one block's worth to run: min(max(32 − 16, 0), 31) = 16
    t.release(3);
    CHECK(reserve1(t, 4, 32) == 0);
    CHECK(t.prefix_acquire(4, p.data(), 32, &cached) == 0 && cached == 16 && t.len(4) == 16 && (blocks(t, 4) == Blocks{0, 1}));
    // … and of n = 16 nothing: min(max(16 − 16, 0), 15) = 0 counts as a miss (the shared block is still taken)
    CHECK(reserve1(t, 5, 16) == 0);
    CHECK(t.prefix_acquire(5, p.data(), 16, &cached) == 0 && cached == 0 && t.len(5) == 0 && blocks(t, 5) == Blocks{0});
    // a prompt the cache has not seen, and one shorter than a block
    const Blocks other = tokens(33, 5000);
    CHECK(reserve1(t, 6, 17) == 0);
    const Blocks reserved6 = blocks(t, 6);
    CHECK(t.prefix_acquire(6, other.data(), 17, &cached) == 0 && cached == 0 && blocks(t, 6) == reserved6);
    t.release(6);
    CHECK(reserve1(t, 6, 15) == 0 && t.prefix_acquire(6, p.data(), 15, &cached) == 0 && cached == 0);
    t.prefix_stats(&hits, &misses, &saved, &entries);
    CHECK(hits == 3 && misses == 3 && saved == 64 && entries == 2);
    CHECK_REFUSED(t.prefix_acquire(42, p.data(), 33, &cached), "reserve KV slots");
    CHECK_REFUSED(t.prefix_acquire(2, p.data(), 33, &cached), "already holds");
}

static void check_fork() {
    SeqTable t(8, 16, 4);
    Copier cp;
    CHECK(reserve1(t, 1, 48) == 0);                                            // three blocks reserved …
    CHECK_REFUSED(t.fork(1, 2, cp), "unknown or empty");                       // … but nothing written yet
    CHECK_REFUSED(t.fork(42, 2, cp), "unknown or empty");
    t.advance(1, 16);
    // at len 16: the full block is shared, no copy, the source's reserved-but-unused blocks are not inherited
    CHECK(t.fork(1, 2, cp) == 0 && cp.calls.empty());
    CHECK(blocks(t, 2) == Blocks{0} && t.len(2) == 16 && refs(t, 0) == 2 && refs(t, 1) == 1 && free_count(t) == 5);
    CHECK_REFUSED(t.fork(1, 2, cp), "exists");
    // at len 17: exactly one copy (old tail → fresh), the tail is private
    t.advance(1, 1);
    CHECK(t.fork(1, 3, cp) == 0);
    CHECK(cp.calls.size() == 1 && cp.calls[0] == std::make_pair(1u, 3u));
    CHECK((blocks(t, 3) == Blocks{0, 3}) && t.len(3) == 17 && refs(t, 0) == 3 && refs(t, 1) == 1 && refs(t, 3) == 1 && free_count(t) == 4);
    CHECK((blocks(t, 1) == Blocks{0, 1, 2}) && t.len(1) == 17);
    // pool exhausted: refused, nothing copied, the table unchanged
    CHECK(reserve1(t, 8, 64) == 0 && free_count(t) == 0);
    cp.calls.clear();
    CHECK_REFUSED(t.fork(1, 4, cp), "no free block");
    CHECK(cp.calls.empty() && !t.find(4) && refs(t, 0) == 3 && refs(t, 1) == 1 && free_count(t) == 0);
    // failing copy: its code comes back, the fresh block is in the pool again, the destination is absent, ref counts unchanged
    t.release(8);
    cp.fail_rc = 7;
    CHECK(t.fork(1, 4, cp) == 7);
    CHECK(cp.calls.size() == 1 && cp.calls[0].first == 1u && refs(t, cp.calls[0].second) == 0);
    CHECK(!t.find(4) && refs(t, 0) == 3 && refs(t, 1) == 1 && free_count(t) == 4);
    cp.fail_rc = 0;
    CHECK(t.fork(1, 4, cp) == 0 && t.len(4) == 17 && refs(t, 0) == 4 && free_count(t) == 3);     // and the same call succeeds afterwards
}

static void check_truncate() {
    Copier cp;
    {
        SeqTable t(8, 16, 4);
        CHECK_REFUSED(t.truncate(42, 0, cp), "unknown sequence");
        CHECK(reserve1(t, 1, 33) == 0);
        t.advance(1, 33);
        CHECK(t.fork(1, 2, cp) == 0 && (blocks(t, 2) == Blocks{0, 1, 3}) && free_count(t) == 4);
        cp.calls.clear();
        // new_len ≥ len is a no-op
        CHECK(t.truncate(2, 33, cp) == 0 && t.truncate(2, 40, cp) == 0);
        CHECK(t.len(2) == 33 && (blocks(t, 2) == Blocks{0, 1, 3}) && free_count(t) == 4 && cp.calls.empty());
        // to 16 on a shared sequence: a block boundary, no copy; the blocks behind it are released
        CHECK(t.truncate(2, 16, cp) == 0 && cp.calls.empty());
        CHECK(t.len(2) == 16 && blocks(t, 2) == Blocks{0} && refs(t, 0) == 2 && refs(t, 1) == 1 && refs(t, 3) == 0 && free_count(t) == 5);
        // to 17 where the block that becomes partial is shared: one copy, the old block's count drops by one
        CHECK(t.fork(1, 3, cp) == 0 && refs(t, 1) == 2);
        const Blocks before = blocks(t, 3);
        cp.calls.clear();
        // … first with a failing copy: length, blocks, ref counts and the free count stay
        cp.fail_rc = 5;
        const int free_before = free_count(t);
        CHECK(t.truncate(3, 17, cp) == 5 && cp.calls.size() == 1);
        CHECK(t.len(3) == 33 && blocks(t, 3) == before && refs(t, 1) == 2 && refs(t, cp.calls[0].second) == 0 && free_count(t) == free_before);
        cp.fail_rc = 0;
        cp.calls.clear();
        CHECK(t.truncate(3, 17, cp) == 0);
        CHECK(cp.calls.size() == 1 && cp.calls[0].first == 1u);
        const uint32_t fresh = cp.calls[0].second;
        CHECK(fresh != 1 && (blocks(t, 3) == Blocks{0, fresh}) && t.len(3) == 17 && refs(t, 1) == 1 && refs(t, fresh) == 1 && refs(t, before[2]) == 0);
        CHECK(free_count(t) == free_before);                                   // one block taken for the copy, the old tail given back
        // … and where it is a prefix-cache entry: one copy, and the entry stays findable by its hash
        const Blocks p = tokens(33, 100);
        CHECK(t.prefix_register(1, p.data(), 33, 0) == 0 && hashed(t, 1) && refs(t, 1) == 1);
        cp.calls.clear();
        CHECK(t.truncate(1, 17, cp) == 0 && cp.calls.size() == 1 && cp.calls[0].first == 1u);
        CHECK(blocks(t, 1)[1] == cp.calls[0].second && blocks(t, 1).size() == 2 && t.len(1) == 17 && refs(t, 1) == 0 && hashed(t, 1));
        int cached = -1;
        CHECK(reserve1(t, 5, 33) == 0 && t.prefix_acquire(5, p.data(), 33, &cached) == 0 && cached == 32);
        CHECK(blocks(t, 5)[0] == 0 && blocks(t, 5)[1] == 1 && refs(t, 1) == 1);
        // no block free for the private copy: refused, unchanged
        while (free_count(t) > 0) CHECK(reserve1(t, 100 + free_count(t), 16) == 0);
        cp.calls.clear();
        CHECK_REFUSED(t.truncate(5, 17, cp), "no block is free");
        CHECK(cp.calls.empty() && t.len(5) == 32 && blocks(t, 5).size() == 3 && refs(t, 1) == 1);
    }
    {
        // a private, unhashed block: no copy.  Cuts at 17, 15 and 0
        SeqTable t(8, 16, 4);
        cp.calls.clear();
        CHECK(reserve1(t, 1, 33) == 0);
        t.advance(1, 33);
        CHECK(t.truncate(1, 17, cp) == 0 && (blocks(t, 1) == Blocks{0, 1}) && t.len(1) == 17 && free_count(t) == 6);
        CHECK(t.truncate(1, 15, cp) == 0 && blocks(t, 1) == Blocks{0} && t.len(1) == 15 && free_count(t) == 7);
        CHECK(t.truncate(1, 0, cp) == 0 && blocks(t, 1).empty() && t.len(1) == 0 && free_count(t) == 8 && t.find(1));
        CHECK(cp.calls.empty());
    }
}

static void check_swap() {
    SeqTable t(8, 16, 4);
    // out: the gather list is the first ceil(len / 16) blocks; the release returns everything, the reserved tail included
    CHECK(reserve1(t, 1, 64) == 0 && free_count(t) == 4);
    CHECK(t.swap_out_blocks(*t.find(1)).empty());                              // len 0
    const int lens[4] = {15, 16, 17, 33};
    const size_t want[4] = {1, 1, 2, 3};
    for (int i = 0; i < 4; i++) {
        t.advance(1, lens[i] - t.len(1));
        const Blocks g = t.swap_out_blocks(*t.find(1)), all = blocks(t, 1);
        CHECK(all.size() == 4 && g.size() == want[i] && g == Blocks(all.begin(), all.begin() + want[i]));
    }
    t.release(1);
    CHECK(!t.find(1) && free_count(t) == 8);
    // in: allocate nb, then commit …
    Blocks b;
    CHECK(t.swap_in_allocate(2, 3, &b) == 0 && b.size() == 3 && free_count(t) == 5 && !t.find(2));
    const Blocks got = b;
    t.commit(2, std::move(b), 33);
    CHECK(t.len(2) == 33 && blocks(t, 2) == got && refs(t, got[0]) == 1 && free_count(t) == 5);
    CHECK_REFUSED(t.swap_in_allocate(2, 1, &b), "exists");
    CHECK_REFUSED(t.swap_in_allocate(3, 6, &b), "exhausted");
    CHECK(free_count(t) == 5 && !t.find(3));
    // … or give back
    CHECK(t.swap_in_allocate(3, 2, &b) == 0 && b.size() == 2 && free_count(t) == 3);
    t.give_back(b);
    CHECK(free_count(t) == 5 && !t.find(3) && refs(t, b[0]) == 0 && refs(t, b[1]) == 0);
    CHECK(t.swap_in_allocate(3, 0, &b) == 0 && b.empty() && free_count(t) == 5);          // an empty sequence swaps in as no blocks
    t.commit(3, std::move(b), 0);
    CHECK(t.find(3) && t.len(3) == 0);
}

static void check_advance() {
    SeqTable t(8, 16, 4);
    Req r[2] = {{1, 33}, {2, 17}};
    CHECK(t.reserve(r, 2, nullptr) == 0 && t.len(1) == 0 && t.len(2) == 0 && t.len(42) == 0);
    const uint64_t listed[3] = {1, 2, 1};
    const int by[3] = {15, 17, 1};
    for (int i = 0; i < 3; i++) t.advance(listed[i], by[i]);
    CHECK(t.len(1) == 16 && t.len(2) == 17 && t.find(1)->len == 16);
    t.advance(42, 5);                                                          // an unknown id does not become a sequence
    CHECK(!t.find(42) && t.len(42) == 0 && free_count(t) == 3);
    CHECK_REFUSED(t.block_info(8, nullptr, nullptr), "outside the pool");
}

int main(int argc, char** argv) {
    const struct { const char* name; void (*run)(); } cases[] = {{"reserve", check_reserve}, {"prefix", check_prefix},   {"fork", check_fork},
                                                                 {"truncate", check_truncate}, {"swap", check_swap}, {"advance", check_advance}};
    bool ran = false;
    for (const auto& c : cases)
        if (argc == 2 && !strcmp(argv[1], c.name)) { c.run(); ran = true; }
    if (!ran) { printf("usage: %s <reserve|prefix|fork|truncate|swap|advance>\n", argv[0]); return 2; }
    printf("%s: %d checks, %d failed\n", argv[1], g_checked, g_failed);
    return g_failed ? 1 : 0;
}
