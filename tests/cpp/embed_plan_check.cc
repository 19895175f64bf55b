// Stand-alone check of fh::embed_plan and the span functions (csrc/embed_plan.h), the launch decision of the embedding tail:
// built and run by tests/test_embed_plan.py with plain g++ (under AddressSanitizer + UBSan where the toolchain links them), no
// GPU, no library.  Expected values are literals worked out by hand (the arithmetic is next to each case): a span is cut into
// chunks of 16 rows, doubled while it would need more than the slots it owns; a launch owns min(512, ⌈longest span / 16⌉ when
// known, what fits the workspace) chunk slots per span, and ⌈slots / 16⌉ group slots on top where that is more than 32 chunks
// (a span of more than 32 chunks has its partials summed in groups of 16 before the finish); one slot of every span is
// num_seqs · dim · 4 bytes.
//   usage: embed_plan_check <chunks|workspace|independent|invalid>
#include <initializer_list>
#include <stdio.h>
#include <string.h>

#include "embed_plan.h"

using namespace fh;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        g_checked++;                                                                     \
        if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static const size_t BIG = (size_t)1 << 40;      // a workspace that is never the limit
static char g_why[256];

static int plan(EmbedPlan* p, int num_seqs, int dim, int pooling, int dims, int max_span_rows, size_t ws) {
    g_why[0] = 0;
    return embed_plan(EmbedShape{num_seqs, dim, pooling, 1, dims, max_span_rows}, ws, p, g_why, sizeof(g_why));
}
static EmbedPlan ok_plan(int num_seqs, int dim, int pooling, int dims, int max_span_rows, size_t ws) {
    EmbedPlan p{};
    const int rc = plan(&p, num_seqs, dim, pooling, dims, max_span_rows, ws);
    CHECK(rc == 0 && g_why[0] == 0);
    return p;
}

static void check_chunks() {
    // a span's chunks with all 512 slots: 16 rows each up to 8192 rows, then 32
    CHECK(embed_span_chunks(0, 512) == 0 && embed_span_chunks(-3, 512) == 0);
    CHECK(embed_span_chunks(1, 512) == 1 && embed_span_chunks(15, 512) == 1 && embed_span_chunks(16, 512) == 1);
    CHECK(embed_span_chunks(17, 512) == 2 && embed_span_chunks(32, 512) == 2 && embed_span_chunks(33, 512) == 3);
    CHECK(embed_span_chunk_rows(8192, 512) == 16 && embed_span_chunks(8192, 512) == 512);
    CHECK(embed_span_chunk_rows(8193, 512) == 32 && embed_span_chunks(8193, 512) == 257);        // ⌈8193 / 32⌉
    CHECK(embed_span_chunk_rows(16384, 512) == 32 && embed_span_chunk_rows(16385, 512) == 64);
    // mean, longest span unknown: every span owns 512 slots; grid (chunk, span), finish one workgroup per span
    EmbedPlan p = ok_plan(3, 4096, EMBED_POOL_MEAN, 0, 0, BIG);
    CHECK(p.partials && p.max_chunks == 512 && p.partial_grid_x == 512 && p.partial_grid_y == 3 && p.finish_grid_x == 3 && p.block == 256);
    CHECK(p.workspace_want == (size_t)3 * 4096 * 4 * (512 + 32) && p.workspace_used == p.workspace_want && p.out_dim == 4096);
    CHECK(p.reduce && p.max_groups == 32 && p.reduce_grid_x == 32 && p.reduce_grid_y == 3 && p.level2_offset == (size_t)3 * 512 * 4096);
    // groups of a span: none up to 32 chunks, ⌈n / 16⌉ beyond
    CHECK(embed_span_groups(0) == 0 && embed_span_groups(1) == 0 && embed_span_groups(32) == 0);
    CHECK(embed_span_groups(33) == 3 && embed_span_groups(48) == 3 && embed_span_groups(49) == 4 && embed_span_groups(512) == 32);
    // 512 rows known: 32 chunk slots, no group launch; 513: 33 + 3
    EmbedPlan e = ok_plan(3, 4096, EMBED_POOL_MEAN, 0, 512, BIG);
    CHECK(e.max_chunks == 32 && !e.reduce && e.max_groups == 0 && e.reduce_grid_x == 0 && e.reduce_grid_y == 0);
    e = ok_plan(3, 4096, EMBED_POOL_MEAN, 0, 513, BIG);
    CHECK(e.max_chunks == 33 && e.reduce && e.max_groups == 3 && e.workspace_used == (size_t)3 * 4096 * 4 * 36);
    // … known: ⌈rows / 16⌉ slots — 16 → 1, 17 → 2, 256 → 16, 8192 → 512, 8193 → still 512 (the spans double their rows)
    CHECK(ok_plan(3, 4096, EMBED_POOL_MEAN, 0, 1, BIG).max_chunks == 1);
    CHECK(ok_plan(3, 4096, EMBED_POOL_MEAN, 0, 16, BIG).max_chunks == 1);
    CHECK(ok_plan(3, 4096, EMBED_POOL_MEAN, 0, 17, BIG).max_chunks == 2);
    CHECK(ok_plan(3, 4096, EMBED_POOL_MEAN, 0, 256, BIG).max_chunks == 16);
    CHECK(ok_plan(3, 4096, EMBED_POOL_MEAN, 0, 8192, BIG).max_chunks == 512);
    CHECK(ok_plan(3, 4096, EMBED_POOL_MEAN, 0, 8193, BIG).max_chunks == 512);
    CHECK(ok_plan(3, 4096, EMBED_POOL_MEAN, 0, 1 << 30, BIG).max_chunks == 512);
    // last / first: no partial launch, no workspace, whatever the workspace
    for (int pooling : {EMBED_POOL_LAST, EMBED_POOL_FIRST}) {
        p = ok_plan(5, 4096, pooling, 100, 8192, 0);
        CHECK(!p.partials && p.max_chunks == 0 && p.workspace_used == 0 && p.workspace_want == 0 && p.finish_grid_x == 5 && p.out_dim == 100);
    }
    // 16-byte vectors per thread: ⌈dim / 8 / 256⌉ rounded up to 1, 2, 4, 8
    CHECK(ok_plan(1, 8, 0, 0, 0, 0).vec_chunks == 1 && ok_plan(1, 256, 0, 0, 0, 0).vec_chunks == 1 && ok_plan(1, 2048, 0, 0, 0, 0).vec_chunks == 1);
    CHECK(ok_plan(1, 2056, 0, 0, 0, 0).vec_chunks == 2 && ok_plan(1, 4096, 0, 0, 0, 0).vec_chunks == 2);
    CHECK(ok_plan(1, 4104, 0, 0, 0, 0).vec_chunks == 4 && ok_plan(1, 5376, 0, 0, 0, 0).vec_chunks == 4 && ok_plan(1, 8192, 0, 0, 0, 0).vec_chunks == 4);
    CHECK(ok_plan(1, 8200, 0, 0, 0, 0).vec_chunks == 8 && ok_plan(1, 16384, 0, 0, 0, 0).vec_chunks == 8);
}

static void check_workspace() {
    // 4 spans of dim 1024: one slot of every span is 4 · 1024 · 4 = 16384 bytes; 512 chunks + 32 groups wanted = 8.5 MiB
    const size_t slot = 16384;
    EmbedPlan p = ok_plan(4, 1024, EMBED_POOL_MEAN, 0, 0, slot * 544);
    CHECK(p.max_chunks == 512 && p.max_groups == 32 && p.workspace_want == slot * 544 && p.workspace_used == slot * 544);
    // one byte less: 543 slots fit → 511 chunks + 32 groups
    p = ok_plan(4, 1024, EMBED_POOL_MEAN, 0, 0, slot * 544 - 1);
    CHECK(p.max_chunks == 511 && p.partial_grid_x == 511 && p.max_groups == 32 && p.workspace_want == slot * 544 && p.workspace_used == slot * 543);
    // 512 slots: 481 chunks + 31 groups (482 would need 482 + 31 = 513)
    p = ok_plan(4, 1024, EMBED_POOL_MEAN, 0, 0, slot * 512);
    CHECK(p.max_chunks == 481 && p.max_groups == 31 && p.workspace_used == slot * 512 && p.level2_offset == (size_t)4 * 481 * 1024);
    // 36 slots: 33 chunks + 3 groups; 35 or 33 slots: 32 chunks and no second level (33 chunks would need 36)
    p = ok_plan(4, 1024, EMBED_POOL_MEAN, 0, 0, slot * 36);
    CHECK(p.max_chunks == 33 && p.reduce && p.max_groups == 3 && p.workspace_used == slot * 36);
    p = ok_plan(4, 1024, EMBED_POOL_MEAN, 0, 0, slot * 35);
    CHECK(p.max_chunks == 32 && !p.reduce && p.max_groups == 0 && p.workspace_used == slot * 32);
    p = ok_plan(4, 1024, EMBED_POOL_MEAN, 0, 0, slot * 33);
    CHECK(p.max_chunks == 32 && !p.reduce && p.workspace_used == slot * 32);
    p = ok_plan(4, 1024, EMBED_POOL_MEAN, 0, 0, slot * 3 + 100);
    CHECK(p.max_chunks == 3 && p.workspace_used == slot * 3 && p.workspace_used <= slot * 3 + 100);
    p = ok_plan(4, 1024, EMBED_POOL_MEAN, 0, 0, slot);
    CHECK(p.max_chunks == 1 && p.partial_grid_x == 1 && p.workspace_used == slot);
    // a known longest span that wants fewer than fit: the want decides (40 rows → 3 slots)
    p = ok_plan(4, 1024, EMBED_POOL_MEAN, 0, 40, slot * 100);
    CHECK(p.max_chunks == 3 && p.workspace_want == slot * 3 && p.workspace_used == slot * 3);
    // not even one slot per span: refused, nothing planned
    EmbedPlan q{};
    CHECK(plan(&q, 4, 1024, EMBED_POOL_MEAN, 0, 0, slot - 1) == 2 && strstr(g_why, "workspace"));
    CHECK(plan(&q, 4, 1024, EMBED_POOL_MEAN, 0, 0, 0) == 2 && strstr(g_why, "workspace"));
    // with 3 slots a span of 100 rows takes 64-row chunks (16·3 = 48 < 100, 32·3 = 96 < 100, 64·3 ≥ 100): 2 chunks; 96 rows: 32 → 3
    CHECK(embed_span_chunk_rows(100, 3) == 64 && embed_span_chunks(100, 3) == 2);
    CHECK(embed_span_chunk_rows(96, 3) == 32 && embed_span_chunks(96, 3) == 3);
    CHECK(embed_span_chunk_rows(48, 3) == 16 && embed_span_chunks(48, 3) == 3 && embed_span_chunk_rows(49, 3) == 32 && embed_span_chunks(49, 3) == 2);
    CHECK(embed_span_chunks(1 << 30, 1) == 1);
    // never more chunks than slots, and the chunks cover the span exactly
    for (int slots : {1, 2, 3, 7, 511, 512})
        for (long len = 1; len <= 20000; len += (len < 600 ? 1 : 97)) {
            const long r = embed_span_chunk_rows(len, slots);
            const int n = embed_span_chunks(len, slots);
            CHECK(n >= 1 && n <= slots && n * r >= len && (n - 1) * r < len && r % 16 == 0);
        }
}

static void check_independent() {
    // the slots of a launch do not move a span's seams while they suffice: alone, among 9 spans, with the longest span known or not
    const EmbedPlan alone = ok_plan(1, 5376, EMBED_POOL_MEAN, 0, 0, (size_t)256 << 20);
    const EmbedPlan ragged = ok_plan(9, 5376, EMBED_POOL_MEAN, 0, 0, (size_t)256 << 20);
    // 256 MiB / (5376 · 4) = 12483 ≥ 544; / (9 · 5376 · 4) = 1387 ≥ 544
    CHECK(alone.max_chunks == 512 && ragged.max_chunks == 512);
    const EmbedPlan known_short = ok_plan(2, 5376, EMBED_POOL_MEAN, 0, 65, BIG), known_long = ok_plan(2, 5376, EMBED_POOL_MEAN, 0, 4000, BIG);
    CHECK(known_short.max_chunks == 5 && known_long.max_chunks == 250);
    for (long len = 1; len <= 65; len++) {
        CHECK(embed_span_chunk_rows(len, known_short.max_chunks) == 16 && embed_span_chunk_rows(len, known_long.max_chunks) == 16);
        CHECK(embed_span_chunk_rows(len, alone.max_chunks) == 16);
        CHECK(embed_span_chunks(len, known_short.max_chunks) == embed_span_chunks(len, ragged.max_chunks));
    }
    // a small workspace shared by more spans is where it binds: 1 MiB over 9 spans of 5376 → 5 slots, alone → 48 = 45 chunks + 3 groups
    CHECK(ok_plan(9, 5376, EMBED_POOL_MEAN, 0, 0, (size_t)1 << 20).max_chunks == 5);
    CHECK(ok_plan(1, 5376, EMBED_POOL_MEAN, 0, 0, (size_t)1 << 20).max_chunks == 45);
}

static void check_invalid() {
    EmbedPlan p{};
    CHECK(plan(&p, -1, 256, 0, 0, 0, BIG) == 2 && strstr(g_why, "num_seqs"));
    CHECK(plan(&p, 65536, 256, 0, 0, 0, BIG) == 2 && strstr(g_why, "num_seqs"));
    CHECK(plan(&p, 65535, 256, 0, 0, 0, BIG) == 0);
    CHECK(plan(&p, 0, 256, 1, 0, 0, 0) == 0 && !p.partials && p.finish_grid_x == 0);       // nothing to do: no workspace needed
    CHECK(plan(&p, 1, 0, 0, 0, 0, BIG) == 2 && strstr(g_why, "dim"));
    CHECK(plan(&p, 1, -8, 0, 0, 0, BIG) == 2 && strstr(g_why, "dim"));
    CHECK(plan(&p, 1, 12, 0, 0, 0, BIG) == 2 && strstr(g_why, "dim"));
    CHECK(plan(&p, 1, 16392, 0, 0, 0, BIG) == 2 && strstr(g_why, "dim"));
    CHECK(plan(&p, 1, 16384, 0, 0, 0, BIG) == 0 && plan(&p, 1, 8, 0, 0, 0, BIG) == 0);
    CHECK(plan(&p, 1, 256, -1, 0, 0, BIG) == 2 && strstr(g_why, "pooling"));
    CHECK(plan(&p, 1, 256, 3, 0, 0, BIG) == 2 && strstr(g_why, "pooling"));
    CHECK(plan(&p, 1, 256, 2, 0, 0, BIG) == 0 && plan(&p, 1, 256, 1, 0, 0, BIG) == 0);
    CHECK(plan(&p, 1, 256, 0, -1, 0, BIG) == 2 && strstr(g_why, "dims"));
    CHECK(plan(&p, 1, 256, 0, 257, 0, BIG) == 2 && strstr(g_why, "dims"));
    CHECK(plan(&p, 1, 256, 0, 256, 0, BIG) == 0 && p.out_dim == 256);
    CHECK(plan(&p, 1, 256, 0, 1, 0, BIG) == 0 && p.out_dim == 1);
}

int main(int argc, char** argv) {
    const char* which = argc > 1 ? argv[1] : "";
    if (!strcmp(which, "chunks")) check_chunks();
    else if (!strcmp(which, "workspace")) check_workspace();
    else if (!strcmp(which, "independent")) check_independent();
    else if (!strcmp(which, "invalid")) check_invalid();
    else { printf("usage: embed_plan_check <chunks|workspace|independent|invalid>\n"); return 2; }
    printf("%s: %d checked, %d failed\n", which, g_checked, g_failed);
    return g_failed ? 1 : 0;
}
