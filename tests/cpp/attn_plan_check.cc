// Stand-alone check of fh::attn_plan (csrc/attn_plan.h), the launch decision of paged attention: built and run by
// tests/test_attn_plan.py with plain g++ (under AddressSanitizer + UBSan where the toolchain links them), no GPU, no library.
// Every expected value is a literal worked out by hand from the launcher as it stood before the plan became a header (the
// arithmetic is spelled out next to each case); none is produced by calling the code under test another way.
// Heads unless a case says otherwise: 32 q / 4 kv × 128 (GQA group 8: a token is 8 rows, a 16-row tile is 2 tokens).
//   usage: attn_plan_check <forms|thresholds|splits|heads|knobs|compact>
#include <stdio.h>
#include <string.h>

#include "attn_plan.h"

using namespace fh;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        g_checked++;                                                                     \
        if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static const size_t BIG = (size_t)1 << 32;      // a workspace that is never the limit

static AttnShape shape(int num_seqs, int total_q, int max_q_len, int max_kv_len, int hd = 128) {
    return AttnShape{num_seqs, total_q, max_q_len, max_kv_len, 32, 4, hd};
}
static AttnPlan varlen(const AttnShape& s, const Knobs& kn = Knobs()) { return attn_plan(s, kn, true, false, BIG); }
static AttnPlan decode(int num_seqs, int max_kv_len, size_t ws = BIG, const Knobs& kn = Knobs(), bool fused = false) {
    return attn_plan(shape(num_seqs, num_seqs, 1, max_kv_len), kn, false, fused, ws);
}
static bool launch_is(const AttnPlan& p, AttnKernel k, unsigned gx, unsigned gy, unsigned gz, int block, size_t lds, Form f) {
    const bool ok = p.kernel == k && p.grid_x == gx && p.grid_y == gy && p.grid_z == gz && p.block == block && p.waves * 64 == block &&
                    p.lds_bytes == lds && p.form == f;
    if (!ok) printf("  plan: kernel %d grid (%u, %u, %u) block %d waves %d lds %zu nsplit %d compact %d tiles_per_seq %d form %d\n", (int)p.kernel,
                    p.grid_x, p.grid_y, p.grid_z, p.block, p.waves, p.lds_bytes, p.nsplit, p.compact, p.tiles_per_seq, (int)p.form);
    return ok;
}
static bool kv_narrow(const AttnPlan& p, unsigned gx, int compact) {
    return launch_is(p, ATTN_KERNEL_KV_SPLIT, gx, 4, 1, 256, 0, FORM_ATTN_KV_NARROW) && p.nsplit == 1 && !p.reduce && p.compact == compact;
}
static bool row_split(const AttnPlan& p, unsigned gx, int compact) {
    return launch_is(p, ATTN_KERNEL_ROW_SPLIT, gx, 4, 1, 256, 0, FORM_ATTN_ROW_SPLIT) && p.nsplit == 1 && !p.reduce && p.compact == compact;
}
static bool flash64(const AttnPlan& p, unsigned gx) { return launch_is(p, ATTN_KERNEL_FLASH64, gx, 4, 1, 256, 65536, FORM_ATTN_FLASH) && !p.reduce; }
static bool resident(const AttnPlan& p, unsigned gx) { return launch_is(p, ATTN_KERNEL_RESIDENT, gx, 4, 1, 512, 131072, FORM_ATTN_RESIDENT) && !p.reduce; }

// the five named shapes
static void check_forms() {
    // 32 fresh prompts of 256 tokens: kv 256 ≤ 256, 64 work-groups × 4 kv heads ≥ 128 → resident, two work-groups per (sequence, kv head)
    CHECK(resident(varlen(shape(32, 8192, 256, 256)), 64));
    // one 256-token prompt: resident has 1·2·4 = 8 < 128 work-groups; flash has (256·8 / 128)·4 = 64 < 256; 128 row tiles × 4 kv heads =
    // 512 work-groups ≥ 256 → one split; row-split would be 32·4 = 128 < 512 work-groups; 256·8 / 16 + 1 = 129 units is not below 128
    const AttnPlan lone = varlen(shape(1, 256, 256, 256));
    CHECK(kv_narrow(lone, 128, 0) && lone.tiles_per_seq == 128);
    CHECK(kv_narrow(varlen(shape(1, 256, 0, 256)), 128, 0));          // max_q_len unknown: total − (num_seqs − 1) = 256
    // 4 × 2048: (8192·8 / 128)·4 = 2048 work-groups ≥ 256 → flash, 64-key steps; tiles ≤ 65536 / 16 + 4 = 4100, units ≤ ⌈4100 / 8⌉ + 4 = 517;
    // LDS two stages × two pairs × four 4-KiB tiles
    CHECK(flash64(varlen(shape(4, 8192, 2048, 2048)), 517));
    // decode, 32 sequences at 4096 keys: 32·4 = 128 work-groups < 256 and 128 block pairs / 2 ≥ 16 → 2 splits (256 work-groups: no further);
    // 64 pairs per split ≥ 8 → 8 waves; partials 32·4·2·16·130·4 bytes; the reduce runs one thread per (row, 8 dims)
    const AttnPlan dec = decode(32, 4096);
    CHECK(launch_is(dec, ATTN_KERNEL_KV_SPLIT, 32, 4, 2, 512, 0, FORM_ATTN_KV_WIDE) && dec.nsplit == 2 && dec.compact == 0);
    CHECK(dec.reduce && dec.reduce_grid_x == 32 && dec.reduce_grid_y == 4 && dec.reduce_block == 256 && dec.workspace_need == 2129920);
    CHECK(decode(32, 4096, 2129920).nsplit == 2);                      // exactly enough
    // … without a workspace, or one byte short: one split, still 8 waves (128 pairs per split)
    const size_t short_ws[2] = {0, 2129919};
    for (size_t ws : short_ws) {
        const AttnPlan one = decode(32, 4096, ws);
        CHECK(launch_is(one, ATTN_KERNEL_KV_SPLIT, 32, 4, 1, 512, 0, FORM_ATTN_KV_WIDE) && one.nsplit == 1 && !one.reduce);
    }
    // what the runner reserves: (32·32 + 16·4096) rows × 32 splits × 130 floats
    CHECK(attn_workspace_bytes(32, 32, 128) == (size_t)1107558400);
}

// each side of every threshold of the prefill forms and of row-split / wide
static void check_thresholds() {
    // resident: max_kv_len 256 | 257.  Past it the batch is a flash batch: tiles ≤ 4096 + 32, units ≤ ⌈4128 / 8⌉ + 32 = 548
    CHECK(resident(varlen(shape(32, 8192, 256, 256)), 64));
    CHECK(flash64(varlen(shape(32, 8192, 256, 257)), 548));
    // resident: max_q_len 32 | 31.  32 × 31 tokens: 31·8 = 248 rows < 512 is no flash batch either; 16 row tiles per sequence, 32·4·4 = 512
    // work-groups → row-split on 32·4 of them; units ≤ ⌈(496 + 32) / 4⌉ + 32 = 164 is not below 128
    CHECK(resident(varlen(shape(32, 1024, 32, 32)), 64));
    CHECK(row_split(varlen(shape(32, 992, 31, 31)), 128, 0));
    // resident: 16·2·4 = 128 work-groups | 15·2·4 = 120.  15 × 256 is a flash batch ((3840·8 / 128)·4 = 960): ⌈(1920 + 15) / 8⌉ + 15 = 257
    CHECK(resident(varlen(shape(16, 4096, 256, 256)), 32));
    CHECK(flash64(varlen(shape(15, 3840, 256, 256)), 257));
    // resident: ≥ 4 row tiles (64 rows) per sequence on average, 32 sequences: 256·8 = 2048 rows | 255·8 = 2040.  Below: 16 row tiles for
    // the longest, 32·4·4 = 512 work-groups → row-split; tiles ≤ 2040 / 16 + 32 = 159, units ≤ ⌈159 / 4⌉ + 32 = 72 < 128
    CHECK(resident(varlen(shape(32, 256, 32, 32)), 64));
    CHECK(row_split(varlen(shape(32, 255, 32, 32)), 72, 1));
    // flash: (1024·8 / 128)·4 = 256 work-groups | (1023·8 / 128 = 63)·4 = 252.  One prompt of 1024: ⌈513 / 8⌉ + 1 = 66 units.  Of 1023: 512
    // row tiles, row-split over 128·4 = 512 work-groups; units ≤ ⌈(511 + 1) / 4⌉ + 1 = 129 is not below 128
    CHECK(flash64(varlen(shape(1, 1024, 1024, 1024)), 66));
    CHECK(row_split(varlen(shape(1, 1023, 1023, 1023)), 128, 0));
    // … at one kv head (8 q heads) the count moves in ones: 4096·8 / 128 = 256 | 4095·8 / 128 = 255.  4096: ⌈2049 / 8⌉ + 1 = 258 units;
    // 4095: 2048 row tiles, row-split on 512 work-groups, ⌈2048 / 4⌉ + 1 = 513 units is not below 512
    CHECK(launch_is(attn_plan(AttnShape{1, 4096, 4096, 4096, 8, 1, 128}, Knobs(), true, false, BIG), ATTN_KERNEL_FLASH64, 258, 1, 1, 256, 65536,
                    FORM_ATTN_FLASH));
    CHECK(launch_is(attn_plan(AttnShape{1, 4095, 4095, 4095, 8, 1, 128}, Knobs(), true, false, BIG), ATTN_KERNEL_ROW_SPLIT, 512, 1, 1, 256, 0,
                    FORM_ATTN_ROW_SPLIT));
    // flash_min_rows: 64·8 = 512 rows | 63·8 = 504, 16 sequences continuing a context (kv 1000).  64: ⌈(512 + 16) / 8⌉ + 16 = 82 units.
    // 63: 32 row tiles per sequence, 16·8·4 = 512 work-groups → row-split on 128; ⌈(504 + 16) / 4⌉ + 16 = 146 units is not below 128
    CHECK(flash64(varlen(shape(16, 1024, 64, 1000)), 82));
    CHECK(row_split(varlen(shape(16, 1008, 63, 1000)), 128, 0));
    // flash only when most sequences bring many rows, 2·total ≥ num_seqs·max_q_len: 64 sequences of up to 64 tokens, 2048 | 2047 in all.
    // 2048: ⌈(1024 + 64) / 8⌉ + 64 = 200 units.  2047: row-split on 64·8 work-groups, ⌈(1023 + 64) / 4⌉ + 64 = 336 units < 512
    CHECK(flash64(varlen(shape(64, 2048, 64, 1000)), 200));
    CHECK(row_split(varlen(shape(64, 2047, 64, 1000)), 336, 1));
    // row-split: tiles_per_seq 4 | 3, 128 sequences of 8 | 6 tokens (4·128 = 512 work-groups).  ⌈(512 + 128) / 4⌉ + 128 = 288 units is
    // not below 128; 3 tiles: KV-split on 384 tiles, 384 + 128 = 512 units is not below 384
    CHECK(row_split(varlen(shape(128, 1024, 8, 512)), 128, 0));
    CHECK(kv_narrow(varlen(shape(128, 768, 6, 512)), 384, 0));
    // row-split: 128·1·4 = 512 work-groups | 127·1·4 = 508 (KV-split on 127·4 tiles; 508 + 127 units is not below 508)
    CHECK(kv_narrow(varlen(shape(127, 1016, 8, 512)), 508, 0));
    // wide: 225 keys = 15 blocks = 8 pairs per split | 224 keys = 14 blocks = 7 pairs
    CHECK(launch_is(decode(32, 225), ATTN_KERNEL_KV_SPLIT, 32, 4, 1, 512, 0, FORM_ATTN_KV_WIDE));
    CHECK(kv_narrow(decode(32, 224), 32, 0));
    // … per SPLIT: 4096 keys in 32 splits (forced) is 128 / 32 = 4 pairs each → 4 waves
    Knobs kn;
    kn.attn_splits = 32;
    CHECK(launch_is(decode(32, 4096, BIG, kn), ATTN_KERNEL_KV_SPLIT, 32, 4, 32, 256, 0, FORM_ATTN_KV_NARROW));
    // … and only for one query token per sequence
    CHECK(varlen(shape(32, 64, 2, 4096)).waves == 4);
}

static void check_splits() {
    // doubling while the work-groups are < 256 and the pairs per doubled split ≥ 16: one tile × 4 kv heads
    CHECK(choose_splits(1, 4, 992) == 1);          // 62 blocks = 31 pairs: 31 / 2 = 15
    CHECK(choose_splits(1, 4, 1024) == 2);         // 32 pairs: 32 / 2 = 16, then 32 / 4 = 8
    CHECK(choose_splits(1, 4, 2016) == 2);         // 63 pairs: 63 / 4 = 15
    CHECK(choose_splits(1, 4, 2048) == 4);         // 64 pairs: 64 / 4 = 16, then 64 / 8 = 8
    CHECK(choose_splits(1, 4, 32768) == 32);       // 1024 pairs: 1024 / 64 = 16 …
    CHECK(choose_splits(1, 4, 65536) == 32);       // … and 2048 / 128 = 16 would double again: the cap
    CHECK(choose_splits(1, 4, 16352) == 16);       // 511 pairs: 511 / 32 = 15
    // enough work-groups: 63·4 = 252 < 256 doubles once (504), 64·4 = 256 does not
    CHECK(choose_splits(63, 4, 4096) == 2);
    CHECK(choose_splits(64, 4, 4096) == 1);
    CHECK(choose_splits(8, 4, 4096) == 8);         // 32 work-groups: 64, 128, 256 — and 128 pairs / 16 = 8 stops it there as well
    CHECK(choose_splits(8, 4, 1 << 20) == 8);      // … the work-groups alone
}

static void check_heads() {
    // head_dim 64 and 256 take the 32-key flash form, 2 | 1 row tiles per wave; 4 × 2048
    const AttnPlan h64 = varlen(shape(4, 8192, 2048, 2048, 64));
    CHECK(launch_is(h64, ATTN_KERNEL_FLASH32, 517, 4, 1, 256, 16384, FORM_ATTN_FLASH) && h64.mt == 2);
    // 256: a work-group is 64 rows ((65536 / 64)·4 work-groups), units ≤ ⌈4100 / 4⌉ + 4 = 1029; LDS two stages × four 8-KiB tiles
    const AttnPlan h256 = varlen(shape(4, 8192, 2048, 2048, 256));
    CHECK(launch_is(h256, ATTN_KERNEL_FLASH32, 1029, 4, 1, 256, 65536, FORM_ATTN_FLASH) && h256.mt == 1);
    // … from (512·8 / 64)·4 = 256 work-groups, where head_dim 128 has (512·8 / 128)·4 = 128
    CHECK(varlen(shape(1, 512, 512, 512, 256)).kernel == ATTN_KERNEL_FLASH32);
    CHECK(varlen(shape(1, 512, 512, 512, 64)).kernel == ATTN_KERNEL_KV_SPLIT);
    // the resident form is head_dim 128 only: 32 × 256 at head_dim 64 is a flash batch
    CHECK(varlen(shape(32, 8192, 256, 256, 64)).kernel == ATTN_KERNEL_FLASH32);
    // the reduce launch: 16 rows × head_dim / 8 threads
    CHECK(attn_plan(shape(32, 32, 1, 4096, 64), Knobs(), false, false, BIG).reduce_block == 128);
    CHECK(attn_plan(shape(32, 32, 1, 4096, 256), Knobs(), false, false, BIG).reduce_block == 512);
    CHECK(attn_plan(shape(32, 32, 1, 4096, 256), Knobs(), false, false, BIG).workspace_need == (size_t)32 * 4 * 2 * 16 * 258 * 4);
    // other GQA groups: 8 q / 8 kv heads (a tile is 16 tokens) — one 256-token prompt is 16 tiles, 4·8 = 32 < 512 work-groups
    const AttnPlan g1 = attn_plan(AttnShape{1, 256, 256, 256, 8, 8, 128}, Knobs(), true, false, BIG);
    CHECK(launch_is(g1, ATTN_KERNEL_KV_SPLIT, 16, 8, 1, 256, 0, FORM_ATTN_KV_NARROW) && g1.tiles_per_seq == 16 && g1.compact == 0);
    // the fused-qkv decode form never takes a prefill form, whatever the shape says …
    const AttnPlan fres = attn_plan(shape(32, 8192, 256, 256), Knobs(), true, true, BIG);
    CHECK(launch_is(fres, ATTN_KERNEL_KV_SPLIT, 4096, 4, 1, 256, 0, FORM_ATTN_FUSED_QKV_NARROW));
    CHECK(attn_plan(shape(4, 8192, 2048, 2048), Knobs(), true, true, BIG).kernel == ATTN_KERNEL_KV_SPLIT);
    // … nor row-split (one 1023-token "prompt" above), and counts its own forms
    CHECK(attn_plan(shape(1, 1023, 1023, 1023), Knobs(), true, true, BIG).kernel == ATTN_KERNEL_KV_SPLIT);
    const AttnPlan fdec = decode(32, 4096, BIG, Knobs(), true);
    CHECK(launch_is(fdec, ATTN_KERNEL_KV_SPLIT, 32, 4, 2, 512, 0, FORM_ATTN_FUSED_QKV_WIDE) && fdec.reduce);
    CHECK(launch_is(decode(32, 224, BIG, Knobs(), true), ATTN_KERNEL_KV_SPLIT, 32, 4, 1, 256, 0, FORM_ATTN_FUSED_QKV_NARROW));
}

static void check_knobs() {
    const AttnShape lone = shape(1, 256, 256, 256), four = shape(4, 8192, 2048, 2048), many = shape(32, 8192, 256, 256);
    {   // attn_no_flash: 4 × 2048 goes row-split, 4·256 work-groups × 4 kv heads; ⌈4100 / 4⌉ + 4 = 1029 units is not below 1024
        Knobs kn;
        kn.attn_no_flash = true;
        CHECK(row_split(varlen(four, kn), 1024, 0));
    }
    {   // attn_flash_min_rows(_set): a set value also lifts the 256-work-group minimum — the lone prompt: ⌈129 / 8⌉ + 1 = 18 units
        Knobs kn;
        kn.attn_flash_min_rows_set = true;
        kn.attn_flash_min_rows = 1;
        CHECK(flash64(varlen(lone, kn), 18));
        kn.attn_flash_min_rows = 2049;             // 256·8 = 2048 rows
        CHECK(kv_narrow(varlen(lone, kn), 128, 0));
        kn.attn_flash_min_rows_set = false;        // the value alone: 4 × 2048 has 16384 rows a sequence
        kn.attn_flash_min_rows = 16385;
        CHECK(varlen(four, kn).kernel == ATTN_KERNEL_ROW_SPLIT);
    }
    {   // attn_splits: 4 splits of 32 pairs, partials twice those of 2; without room for them one split again
        Knobs kn;
        kn.attn_splits = 4;
        const AttnPlan p = decode(32, 4096, BIG, kn);
        CHECK(launch_is(p, ATTN_KERNEL_KV_SPLIT, 32, 4, 4, 512, 0, FORM_ATTN_KV_WIDE) && p.nsplit == 4 && p.reduce && p.workspace_need == 4259840);
        CHECK(decode(32, 4096, 4259839, kn).nsplit == 1);
        kn.attn_splits = 1;
        CHECK(decode(32, 4096, BIG, kn).nsplit == 1 && !decode(32, 4096, BIG, kn).reduce);
    }
    {   // attn_rs_min_wgs: the lone prompt row-split on 128 / 4 = 32 work-groups; ⌈129 / 4⌉ + 1 = 34 units is not below 32
        Knobs kn;
        kn.attn_rs_min_wgs = 1;
        CHECK(row_split(varlen(lone, kn), 32, 0));
    }
    {   // attn_no_rs: 128 sequences of 8 tokens stay KV-split on 128·4 tiles (512 + 128 units is not below 512)
        Knobs kn;
        kn.attn_no_rs = true;
        CHECK(kv_narrow(varlen(shape(128, 1024, 8, 512), kn), 512, 0));
    }
    {   // attn_narrow: the split decode on 4 waves
        Knobs kn;
        kn.attn_narrow = true;
        const AttnPlan p = decode(32, 4096, BIG, kn);
        CHECK(launch_is(p, ATTN_KERNEL_KV_SPLIT, 32, 4, 2, 256, 0, FORM_ATTN_KV_NARROW) && p.reduce);
    }
    {   // attn_no_resident: 32 × 256 as a flash batch (548 units, as past 256 keys)
        Knobs kn;
        kn.attn_no_resident = true;
        CHECK(flash64(varlen(many, kn), 548));
    }
    {   // attn_resident_min_wgs: the lone prompt on its two work-groups per kv head | 8 work-groups against 9
        Knobs kn;
        kn.attn_resident_min_wgs = 1;
        CHECK(resident(varlen(lone, kn), 2));
        kn.attn_resident_min_wgs = 8;
        CHECK(resident(varlen(lone, kn), 2));
        kn.attn_resident_min_wgs = 9;
        CHECK(kv_narrow(varlen(lone, kn), 128, 0));
    }
}

// the compact grid of a ragged batch: only the real work units, bounded from the token count
static void check_compact() {
    // 31 decode tokens + one 256-token prompt at up to 4096 keys: 128 tiles per sequence, 32·32·4 work-groups → row-split on 1024;
    // tiles ≤ 287·8 / 16 + 32 = 175, units ≤ ⌈175 / 4⌉ + 32 = 76 < 1024
    const AttnShape mixed = shape(32, 287, 256, 4096);
    CHECK(row_split(varlen(mixed), 76, 1));
    // … KV-split (attn_no_rs): 175 units < 32·128 = 4096 tiles
    Knobs kn;
    kn.attn_no_rs = true;
    CHECK(kv_narrow(varlen(mixed, kn), 175, 1));
    // KV-split on its own heuristic: 31 decode tokens + one of 4 tokens, 2 tiles per sequence; 35·8 / 16 + 32 = 49 units < 64 tiles
    CHECK(kv_narrow(varlen(shape(32, 35, 4, 4096)), 49, 1));
    // the bound must be BELOW the full grid: 32 sequences × 4 tokens have 64 + 32 = 96 units against 64 tiles
    CHECK(kv_narrow(varlen(shape(32, 128, 4, 4096)), 64, 0));
    // … 4 tokens + 1 token at 100 keys: 5·8 / 16 + 2 = 4 units against 2·2 = 4 tiles — equal is not below
    CHECK(kv_narrow(varlen(shape(2, 5, 4, 100)), 4, 0));
    // one prompt of 2048 and three decode tokens: no flash batch (4102 < 8192); row-split, ⌈(1025 + 4) / 4⌉ + 4 = 262 < 4·256 units
    CHECK(row_split(varlen(shape(4, 2051, 2048, 2048)), 262, 1));
    // never with one tile per sequence (varlen decode), never under a KV split, never without cu_seqlens_q
    CHECK(varlen(shape(32, 20, 1, 300)).compact == 0 && varlen(shape(32, 20, 1, 300)).grid_x == 32);
    kn = Knobs();
    kn.attn_splits = 2;
    const AttnPlan split = varlen(shape(32, 35, 4, 4096), kn);
    CHECK(split.compact == 0 && split.grid_x == 64 && split.grid_z == 2 && split.reduce && split.reduce_grid_x == 64);
    CHECK(attn_plan(shape(32, 35, 4, 4096), Knobs(), false, false, BIG).compact == 0);
}

int main(int argc, char** argv) {
    const struct { const char* name; void (*run)(); } cases[] = {{"forms", check_forms}, {"thresholds", check_thresholds}, {"splits", check_splits},
                                                                 {"heads", check_heads}, {"knobs", check_knobs}, {"compact", check_compact}};
    bool ran = false;
    for (const auto& c : cases)
        if (argc == 2 && !strcmp(argv[1], c.name)) { c.run(); ran = true; }
    if (!ran) { printf("usage: %s <forms|thresholds|splits|heads|knobs|compact>\n", argv[0]); return 2; }
    printf("%s: %d checks, %d failed\n", argv[1], g_checked, g_failed);
    return g_failed ? 1 : 0;
}
