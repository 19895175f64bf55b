// Stand-alone check of csrc/knobs.cc — the knob table (defaults, variable names, parse kinds, the three special rules) and the
// form list with its hit counters: built and run by tests/test_knobs.py with plain g++ (under AddressSanitizer + UBSan where
// the toolchain links them), no GPU, no library.  Every literal below is written out by hand, none comes from the tables.
//   usage: knobs_check <defaults|each|special|forms>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <type_traits>
#include <vector>

#include "knobs.h"

extern char** environ;
using fh::Knobs;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        g_checked++;                                                                     \
        if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static_assert(std::is_same<decltype(Knobs::attn_flash_min_rows), long>::value && std::is_same<decltype(Knobs::attn_rs_min_wgs), long>::value &&
              std::is_same<decltype(Knobs::attn_resident_min_wgs), long>::value, "the three long knobs");
static_assert(std::is_same<decltype(Knobs::attn_no_flash), bool>::value && std::is_same<decltype(Knobs::no_graph), bool>::value &&
              std::is_same<decltype(Knobs::attn_flash_min_rows_set), bool>::value && std::is_same<decltype(Knobs::w4_big), int>::value, "bool / int knobs");

// field, its variable, default, a value to set, the field's value after that (every other field keeps its default)
struct Row { const char* field; const char* env; long dflt; const char* set; long after; long (*get)(const Knobs&); };
#define ROW(f, env, dflt, set, after) {#f, "FERRUM_HIP_" env, dflt, set, after, [](const Knobs& k) -> long { return (long)k.f; }}
static const Row ROWS[] = {
    ROW(attn_no_flash, "ATTN_NO_FLASH", 0, "1", 1),
    ROW(attn_flash_min_rows_set, "ATTN_FLASH_MIN_ROWS", 0, "300", 1),
    ROW(attn_flash_min_rows, "ATTN_FLASH_MIN_ROWS", 512, "300", 300),
    ROW(attn_splits, "ATTN_SPLITS", 0, "3", 3),
    ROW(attn_rs_min_wgs, "ATTN_RS_MIN_WGS", 512, "64", 64),
    ROW(attn_no_rs, "ATTN_NO_RS", 0, "1", 1),
    ROW(attn_narrow, "ATTN_NARROW", 0, "1", 1),
    ROW(attn_no_resident, "ATTN_NO_RESIDENT", 0, "1", 1),
    ROW(attn_resident_min_wgs, "ATTN_RESIDENT_MIN_WGS", 128, "2", 2),
    ROW(moe_kw_pairs, "MOE_KW_PAIRS", 16, "4", 4),
    ROW(decode_chain, "DECODE_CHAIN", 1, "0", 0),
    ROW(chain_max_rows, "CHAIN_MAX_ROWS", 128, "77", 77),
    ROW(sandwich_wide, "SANDWICH_WIDE", 1, "0", 0),
    ROW(chain_qkv_half, "CHAIN_QKV_HALF", 1, "0", 0),
    ROW(chain_o_half, "CHAIN_O_HALF", 1, "0", 0),
    ROW(chain_split_keys, "CHAIN_SPLIT_KEYS", 256, "0", 0),
    ROW(chain_qkv_wide, "CHAIN_QKV_WIDE", -1, "1", 1),
    ROW(chain_slots, "CHAIN_SLOTS", 256, "128", 128),
    ROW(route_gemm_topk, "ROUTE_GEMM_TOPK", 1, "0", 0),
    ROW(chain_attn_splits, "CHAIN_ATTN_SPLITS", 0, "4", 4),
    ROW(chain_max_keys, "CHAIN_MAX_KEYS", 4096, "1024", 1024),
    ROW(dense_chain, "DENSE_CHAIN", 1, "0", 0),
    ROW(moe_em2, "MOE_EM2", 1, "0", 0),
    ROW(moe_deferred_merge, "MOE_DEFERRED_MERGE", 1, "0", 0),
    ROW(moe_pair_rank_lists, "MOE_PAIR_RANK_LISTS", 1, "0", 0),
    ROW(w4_tile_min_m, "W4_TILE_MIN_M", 0, "33", 33),
    ROW(w4_tile_wgs, "W4_TILE_WGS", 256, "512", 512),
    ROW(w4_ldsa, "W4_LDSA", 1, "0", 0),
    ROW(w4_ldsa_nw, "W4_LDSA_NW", 0, "8", 8),
    ROW(w4_ldsa_s, "W4_LDSA_S", 0, "2", 2),
    ROW(w4_big, "W4_BIG", 0, "-1", -1),
    ROW(w4_nt, "W4_NT", 0, "2", 2),
    ROW(w4_w, "W4_W", 0, "4", 4),
    ROW(lds_min_wgs, "LDS_MIN_WGS", 128, "1", 1),
    ROW(lds_min_groups, "LDS_MIN_GROUPS", 8, "16", 16),
    ROW(no_graph, "NO_GRAPH", 0, "0", 1),                      // present is enough, whatever the value
    ROW(trace_launches, "TRACE_LAUNCHES", 0, "1", 0),           // … alone: stays off (see special)
    ROW(time_same_layer, "TIME_SAME_LAYER", 0, "", 1),
    ROW(tp_fused_norm, "TP_FUSED_NORM", 1, "0", 0),
    ROW(tp_oneshot, "TP_ONESHOT", -1, "1", 1),
};
static const int NUM_ROWS = (int)(sizeof(ROWS) / sizeof(ROWS[0]));
static const char* const FLAGS[] = {"FERRUM_HIP_ATTN_NO_FLASH", "FERRUM_HIP_ATTN_NO_RS", "FERRUM_HIP_ATTN_NARROW", "FERRUM_HIP_ATTN_NO_RESIDENT"};

static void clear_env() {
    std::vector<std::string> names;
    for (char** e = environ; *e; e++)
        if (!strncmp(*e, "FERRUM_HIP_", 11)) names.push_back(std::string(*e, strchr(*e, '=') - *e));
    for (const std::string& n : names) unsetenv(n.c_str());
}
static const Knobs& reloaded() { fh::reload_knobs(); return fh::knobs(); }
// every field has its default, except those of variable `env` (when given), which have their `after`
static void check_all(const Knobs& k, const char* env) {
    for (const Row& r : ROWS) {
        const long want = env && !strcmp(env, r.env) ? r.after : r.dflt;
        g_checked++;
        if (r.get(k) != want) { g_failed++; printf("FAILED: with %s set, %s = %ld, expected %ld\n", env ? env : "nothing", r.field, r.get(k), want); }
    }
}

static void check_defaults() {
    CHECK(NUM_ROWS == 40);
    check_all(Knobs(), nullptr);          // the member initialisers …
    check_all(fh::knobs(), nullptr);      // … what the load-time initialiser read (the test starts this program without FERRUM_HIP_*) …
    check_all(reloaded(), nullptr);       // … and a reload
}

static void check_each() {
    for (const Row& r : ROWS) {
        CHECK(r.after != r.dflt || !strcmp(r.field, "trace_launches"));
        setenv(r.env, r.set, 1);
        check_all(reloaded(), r.env);
        unsetenv(r.env);
    }
    for (const char* f : FLAGS) {         // a flag set to 0 is off
        setenv(f, "0", 1);
        check_all(reloaded(), nullptr);
        unsetenv(f);
    }
    setenv("FERRUM_HIP_W4_NT", "junk", 1);      // atoi: not a number reads as 0 …
    CHECK(reloaded().w4_nt == 0);
    unsetenv("FERRUM_HIP_W4_NT");
    setenv("FERRUM_HIP_DECODE_CHAIN", "junk", 1);   // … also where the default is not 0
    CHECK(reloaded().decode_chain == 0);
    unsetenv("FERRUM_HIP_DECODE_CHAIN");
    check_all(reloaded(), nullptr);
}

static void check_special() {
    setenv("FERRUM_HIP_CHAIN_MAX_ROWS", "500", 1);
    CHECK(reloaded().chain_max_rows == 128);
    setenv("FERRUM_HIP_CHAIN_MAX_ROWS", "128", 1);
    CHECK(reloaded().chain_max_rows == 128);
    setenv("FERRUM_HIP_CHAIN_MAX_ROWS", "32", 1);
    CHECK(reloaded().chain_max_rows == 32);
    unsetenv("FERRUM_HIP_CHAIN_MAX_ROWS");
    setenv("FERRUM_HIP_TRACE_LAUNCHES", "1", 1);
    CHECK(!reloaded().trace_launches && !fh::knobs().no_graph);
    setenv("FERRUM_HIP_NO_GRAPH", "1", 1);
    CHECK(reloaded().trace_launches && fh::knobs().no_graph);
    unsetenv("FERRUM_HIP_TRACE_LAUNCHES");
    CHECK(!reloaded().trace_launches && fh::knobs().no_graph);
    unsetenv("FERRUM_HIP_NO_GRAPH");
    CHECK(!reloaded().attn_flash_min_rows_set && fh::knobs().attn_flash_min_rows == 512);
    setenv("FERRUM_HIP_ATTN_FLASH_MIN_ROWS", "512", 1);       // given, with the default's value: still marked as given
    CHECK(reloaded().attn_flash_min_rows_set && fh::knobs().attn_flash_min_rows == 512);
    setenv("FERRUM_HIP_ATTN_FLASH_MIN_ROWS", "48", 1);
    CHECK(reloaded().attn_flash_min_rows_set && fh::knobs().attn_flash_min_rows == 48);
    unsetenv("FERRUM_HIP_ATTN_FLASH_MIN_ROWS");
    check_all(reloaded(), nullptr);
}

static void check_forms() {
    static const char* const NAMES[] = {
        "attn_flash", "attn_row_split", "attn_kv_wide", "attn_kv_narrow", "attn_fused_qkv_wide", "attn_fused_qkv_narrow",
        "attn_split_reduce", "w4_wgsplit", "w4_ldsa", "w4_tilep", "w4_slabs", "w4_slabs_lds", "w4_slabs_tile", "w4_rowsum",
        "moe_expert_major", "moe_inline_align", "moe_block16", "moe_tile64", "moe_tile32", "moe_tile_big", "moe_merge_route", "route_split",
        "route_fused", "route_gemm", "dense_slab_chain", "graph_capture", "graph_replay", "tp_allreduce_rccl",
        "tp_allreduce_loopback", "tp_allreduce_oneshot", "f16_dense_linear", "w4_fused_tail", "attn_resident", "w4_big", "gather_columns",
        "perm_producer", "moe_expert_major_pair", "decode_chain", "moe_deferred_merge", "dense_chain", "tp_allreduce_norm_fused", "chain_attn_kv_splits", "chain_qkv_wide", "route_gemm_topk",
        "moe_pair_rank_lists", "chain_qkv_half", "chain_o_half"};
    const int n = (int)(sizeof(NAMES) / sizeof(NAMES[0]));
    CHECK(n == 47 && fh::FORM_COUNT == 47);
    CHECK(fh::form_name(-1) == nullptr && fh::form_name(fh::FORM_COUNT) == nullptr);
    std::set<std::string> seen;
    for (int i = 0; i < fh::FORM_COUNT; i++) {
        const char* name = fh::form_name(i);
        CHECK(name != nullptr);
        if (!name) continue;
        CHECK(i < n && !strcmp(name, NAMES[i]));
        CHECK(seen.insert(name).second);
    }
    // positions that tests and tools rely on
    CHECK(fh::FORM_ATTN_FLASH == 0 && fh::FORM_MOE_BLOCK16 == 16 && fh::FORM_GRAPH_REPLAY == 26 && fh::FORM_MOE_PAIR_RANK_LISTS == 44);
    uint64_t hits[fh::FORM_COUNT];
    fh::form_hits_reset();
    fh::form_hits_snapshot(hits);
    for (uint64_t h : hits) CHECK(h == 0);
    fh::form_hit(fh::FORM_MOE_BLOCK16);
    fh::form_hit(fh::FORM_MOE_BLOCK16);
    fh::form_hit(fh::FORM_MOE_PAIR_RANK_LISTS);
    fh::form_hits_snapshot(hits);
    for (int i = 0; i < fh::FORM_COUNT; i++) CHECK(hits[i] == (i == 16 ? 2u : i == 44 ? 1u : 0u));
    fh::form_hits_reset();
    fh::form_hits_snapshot(hits);
    for (uint64_t h : hits) CHECK(h == 0);
}

int main(int argc, char** argv) {
    const std::string which = argc > 1 ? argv[1] : "";
    if (which == "defaults") check_defaults();
    else {
        clear_env();
        if (which == "each") check_each();
        else if (which == "special") check_special();
        else if (which == "forms") check_forms();
        else { printf("usage: knobs_check <defaults|each|special|forms>\n"); return 2; }
    }
    printf("%s: %d checked, %d failed\n", which.c_str(), g_checked, g_failed);
    return g_failed ? 1 : 0;
}
