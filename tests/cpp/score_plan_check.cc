// Stand-alone check of fh::score_plan and fh::score_batch_plan (csrc/score_plan.h), the launch decisions of the scoring head:
// built and run by tests/test_score_plan.py with plain g++ (under AddressSanitizer + UBSan where the toolchain links them), no
// GPU, no library.  Expected values are literals worked out by hand: a row of n logits is cut into ⌈n / 4096⌉ segments, one
// workgroup each; the workspace holds three 4-byte words per (row, segment) and one per row; the model-level call sorts the
// distinct packed rows its targets name and cuts them into passes of C rows.
//   usage: score_plan_check <segments|workspace|passes|roundtrip|invalid>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "score_plan.h"

using namespace fh;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        g_checked++;                                                                     \
        if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static const size_t BIG = (size_t)1 << 40;
static char g_why[256];

static int plan(ScorePlan* p, int m, int n, int ld, int pairs, size_t ws) {
    g_why[0] = 0;
    return score_plan(ScoreShape{m, n, ld, pairs}, ws, p, g_why, sizeof(g_why));
}

static void check_segments() {
    CHECK(SCORE_SEGMENT == 4096 && SCORE_BLOCK == 256);
    CHECK(score_segments(0) == 0 && score_segments(-5) == 0);
    CHECK(score_segments(1) == 1 && score_segments(4095) == 1 && score_segments(4096) == 1 && score_segments(4097) == 2);
    CHECK(score_segments(8192) == 2 && score_segments(8193) == 3);
    CHECK(score_segments(151936) == 38);                          // 37 · 4096 = 151552 < 151936 ≤ 38 · 4096
    CHECK(score_segments(2147483647) == 524288);
    ScorePlan p{};
    for (int n : {1, 4095, 4096}) {
        CHECK(plan(&p, 3, n, n, 5, BIG) == 0 && p.segments == 1 && p.partial_grid_x == 1 && p.partial_grid_y == 3 && p.merge_grid_x == 3);
        CHECK(p.gather_grid_x == 1 && p.block == 256);
    }
    CHECK(plan(&p, 33, 4097, 4100, 257, BIG) == 0 && p.segments == 2 && p.partial_grid_x == 2 && p.partial_grid_y == 33 && p.gather_grid_x == 2);
    CHECK(plan(&p, 256, 151936, 151936, 256, BIG) == 0 && p.segments == 38 && p.partial_grid_x == 38 && p.partial_grid_y == 256);
    CHECK(p.merge_grid_x == 256 && p.gather_grid_x == 1);
    // no pairs: no gather launch; no rows: nothing at all, and no workspace needed
    CHECK(plan(&p, 2, 100, 100, 0, BIG) == 0 && p.gather_grid_x == 0 && p.partial_grid_y == 2);
    CHECK(plan(&p, 0, 100, 100, 0, 0) == 0 && p.partial_grid_y == 0 && p.merge_grid_x == 0 && p.workspace_bytes == 0);
}

static void check_workspace() {
    ScorePlan p{};
    // 256 rows of 151 936: 256 · 38 = 9728 partials of 12 bytes + 256 · 4 = 117 760 bytes
    CHECK(plan(&p, 256, 151936, 151936, 1, BIG) == 0 && p.workspace_bytes == 117760);
    CHECK(p.off_sum == 9728 && p.off_idx == 19456 && p.off_lse == 29184);
    CHECK(plan(&p, 256, 151936, 151936, 1, 117760) == 0);
    CHECK(plan(&p, 256, 151936, 151936, 1, 117759) == 2 && strstr(g_why, "workspace") && strstr(g_why, "117760"));
    CHECK(plan(&p, 256, 151936, 151936, 1, 0) == 2 && strstr(g_why, "workspace"));
    // one row of one element: 12 + 4 bytes
    CHECK(plan(&p, 1, 1, 1, 0, 16) == 0 && p.workspace_bytes == 16 && p.off_sum == 1 && p.off_idx == 2 && p.off_lse == 3);
    CHECK(plan(&p, 1, 1, 1, 0, 15) == 2 && strstr(g_why, "16 bytes"));
    // 5 rows of 4097: 10 partials → 120 + 20
    CHECK(plan(&p, 5, 4097, 4097, 0, 140) == 0 && p.workspace_bytes == 140);
    // the seams do not depend on m or ld
    ScorePlan a{}, b{};
    CHECK(plan(&a, 1, 10000, 10000, 0, BIG) == 0 && plan(&b, 33, 10000, 12345, 0, BIG) == 0 && a.segments == b.segments && a.segments == 3);
}

struct Batch {
    std::vector<int32_t> rows;
    std::vector<ScoreTargetRef> targets;
    ScoreBatchPlan plan;
    int rc;
};
static Batch batch(std::vector<int32_t> item_rows, std::vector<ScoreTargetRef> targets, int C, int vocab = 512, int hidden = 256, int max_tokens = 1024) {
    Batch b{item_rows, targets, {}, 0};
    g_why[0] = 0;
    b.rc = score_batch_plan(ScoreBatchShape{(int)b.rows.size(), b.rows.data(), (int)b.targets.size(), b.targets.data(), vocab, hidden, max_tokens, C},
                            &b.plan, g_why, sizeof(g_why));
    return b;
}
template <typename T>
static bool eq(const std::vector<T>& a, std::initializer_list<T> b) { return a == std::vector<T>(b); }

static void check_passes() {
    // items of 4, 1, 3 and 2 rows start at packed rows 0, 4, 5 and 8.  Targets, unsorted, with a duplicate, with two tokens on one
    // row, and none on item 1:  (2,1)→6  (0,3)→3  (3,0)→8  (0,0)→0  (0,3)→3 again, other token  (2,1)→6 same token  (0,2)→2
    Batch b = batch({4, 1, 3, 2}, {{2, 1, 10}, {0, 3, 11}, {3, 0, 12}, {0, 0, 13}, {0, 3, 14}, {2, 1, 10}, {0, 2, 15}}, 3);
    CHECK(b.rc == 0 && b.plan.pass_rows == 3 && b.plan.num_rows == 5 && b.plan.num_passes == 2);
    CHECK(eq<int32_t>(b.plan.rows, {0, 2, 3, 6, 8}));
    CHECK(eq<int32_t>(b.plan.pass_row_begin, {0, 3, 5}));
    // pairs in (packed row, target) order: t3 (0) | t6 (2) | t1, t4 (3) || t0, t5 (6) | t2 (8)
    CHECK(eq<int32_t>(b.plan.pair_rows, {0, 1, 2, 2, 0, 0, 1}));
    CHECK(eq<uint32_t>(b.plan.pair_tokens, {13, 15, 11, 14, 10, 10, 12}));
    CHECK(eq<int32_t>(b.plan.pass_pair_begin, {0, 4, 7}));
    CHECK(eq<int32_t>(b.plan.target_pair, {4, 2, 6, 0, 3, 5, 1}));
    CHECK(eq<int32_t>(b.plan.target_pass, {1, 0, 1, 0, 0, 1, 0}));
    CHECK(eq<int32_t>(b.plan.target_pass_row, {0, 2, 1, 0, 2, 0, 1}));
    // buffers: the widest pass has 3 rows; hidden 256 fp16, vocab 512 fp32, lists 5 + 2 · 7 words, results 7 + 2 · 5 words,
    // workspace of the op at 3 rows of 512: (3 · 3 · 1 + 3) · 4
    CHECK(b.plan.hidden_bytes == 3 * 256 * 2 && b.plan.logits_bytes == 3 * 512 * 4 && b.plan.lists_bytes == 19 * 4 && b.plan.results_bytes == 17 * 4);
    CHECK(b.plan.workspace_bytes == 48);
    // R = C: one full pass; R = C + 1: a second pass of one row; R = 2C + 1 > 2C: three passes
    std::vector<ScoreTargetRef> all;
    for (int r = 0; r < 7; r++) all.push_back({0, 6 - r, (uint32_t)r});         // descending rows of one item of 7
    b = batch({7}, std::vector<ScoreTargetRef>(all.begin(), all.begin() + 3), 3);
    CHECK(b.rc == 0 && b.plan.num_rows == 3 && b.plan.num_passes == 1 && eq<int32_t>(b.plan.pass_row_begin, {0, 3}) && eq<int32_t>(b.plan.rows, {4, 5, 6}));
    b = batch({7}, std::vector<ScoreTargetRef>(all.begin(), all.begin() + 4), 3);
    CHECK(b.rc == 0 && b.plan.num_rows == 4 && b.plan.num_passes == 2 && eq<int32_t>(b.plan.pass_row_begin, {0, 3, 4}));
    CHECK(eq<int32_t>(b.plan.pass_pair_begin, {0, 3, 4}) && eq<int32_t>(b.plan.target_pass, {1, 0, 0, 0}) && eq<int32_t>(b.plan.target_pass_row, {0, 2, 1, 0}));
    b = batch({7}, all, 3);
    CHECK(b.rc == 0 && b.plan.num_rows == 7 && b.plan.num_passes == 3 && eq<int32_t>(b.plan.pass_row_begin, {0, 3, 6, 7}));
    CHECK(b.plan.hidden_bytes == 3 * 256 * 2);
    // fewer rows than a pass holds: the buffers are sized by the rows, not by C
    b = batch({7}, {{0, 6, 1}, {0, 6, 2}}, 0, 151936, 2048, 8192);
    CHECK(b.rc == 0 && b.plan.pass_rows == 256 && b.plan.num_rows == 1 && b.plan.num_passes == 1);
    CHECK(b.plan.hidden_bytes == 4096 && b.plan.logits_bytes == (size_t)151936 * 4 && b.plan.workspace_bytes == (3 * 38 + 1) * 4);
    // the default pass: min(max_tokens, 256)
    CHECK(batch({7}, all, 0, 512, 256, 100).plan.pass_rows == 100 && batch({7}, all, 0, 512, 256, 256).plan.pass_rows == 256);
    CHECK(batch({7}, all, 0, 512, 256, 257).plan.pass_rows == 256 && batch({7}, all, 1000).plan.pass_rows == 1000);
    // no targets: a KV-fill call, nothing to allocate, no passes
    b = batch({4, 1}, {}, 0);
    CHECK(b.rc == 0 && b.plan.num_rows == 0 && b.plan.num_passes == 0 && b.plan.logits_bytes == 0 && b.plan.hidden_bytes == 0 && b.plan.results_bytes == 0);
    CHECK(eq<int32_t>(b.plan.pass_row_begin, {0}));
}

static void check_roundtrip() {
    // ragged items; every (item, row) with (item + row) % 3 != 1 is a target, twice for even rows, visited in a scrambled order
    const std::vector<int32_t> lens = {19, 1, 7, 12, 3};
    std::vector<int32_t> first(lens.size() + 1, 0);
    for (size_t i = 0; i < lens.size(); i++) first[i + 1] = first[i] + lens[i];
    std::vector<ScoreTargetRef> t;
    for (int i = 0; i < (int)lens.size(); i++)
        for (int r = 0; r < lens[i]; r++)
            if ((i + r) % 3 != 1)
                for (int k = 0; k < (r % 2 == 0 ? 2 : 1); k++) t.push_back({i, r, (uint32_t)(100 * i + r + 50 * k)});
    for (size_t k = 0; k < t.size(); k++) std::swap(t[k], t[(k * 7 + 3) % t.size()]);
    for (int C : {1, 3, 4, 7, 29, 1000}) {
        Batch b = batch(lens, t, C);
        CHECK(b.rc == 0);
        const ScoreBatchPlan& p = b.plan;
        CHECK(p.num_passes == (p.num_rows + C - 1) / C && (int)p.pass_row_begin.size() == p.num_passes + 1);
        for (size_t r = 1; r < p.rows.size(); r++) CHECK(p.rows[r - 1] < p.rows[r]);
        for (int q = 0; q < p.num_passes; q++) {
            CHECK(p.pass_row_begin[q] == q * C && p.pass_row_begin[q + 1] - p.pass_row_begin[q] <= C && p.pass_row_begin[q + 1] > p.pass_row_begin[q]);
            for (int k = p.pass_pair_begin[q]; k < p.pass_pair_begin[q + 1]; k++)
                CHECK(p.pair_rows[k] >= 0 && p.pair_rows[k] < p.pass_row_begin[q + 1] - p.pass_row_begin[q]);
        }
        std::vector<int> seen(t.size(), 0);
        for (size_t j = 0; j < t.size(); j++) {
            const int q = p.target_pass[j], r = p.target_pass_row[j], k = p.target_pair[j];
            CHECK(q >= 0 && q < p.num_passes && r >= 0 && r < C);
            CHECK(p.rows[p.pass_row_begin[q] + r] == first[t[j].item] + t[j].row);       // (pass, row) → packed row → (item, row)
            CHECK(k >= p.pass_pair_begin[q] && k < p.pass_pair_begin[q + 1] && p.pair_rows[k] == r && p.pair_tokens[k] == t[j].token);
            seen[k]++;
        }
        for (int s : seen) CHECK(s == 1);
    }
}

static void check_invalid() {
    ScorePlan p{};
    CHECK(plan(&p, -1, 10, 10, 0, BIG) == 2 && strstr(g_why, "m="));
    CHECK(plan(&p, 65536, 10, 10, 0, BIG) == 2 && strstr(g_why, "m="));
    CHECK(plan(&p, 65535, 10, 10, 0, BIG) == 0);
    CHECK(plan(&p, 1, 0, 10, 0, BIG) == 2 && strstr(g_why, "n="));
    CHECK(plan(&p, 1, -3, 10, 0, BIG) == 2 && strstr(g_why, "n="));
    CHECK(plan(&p, 1, 10, 9, 0, BIG) == 2 && strstr(g_why, "ld="));
    CHECK(plan(&p, 1, 10, 10, -1, BIG) == 2 && strstr(g_why, "num_pairs"));
    CHECK(plan(&p, 0, 10, 10, 1, BIG) == 2 && strstr(g_why, "no rows"));
    // the model-level call: every class, the target named
    CHECK(batch({4, 2}, {{0, 0, 1}, {2, 0, 1}}, 0).rc == 2 && strstr(g_why, "target 1") && strstr(g_why, "item 2"));
    CHECK(batch({4, 2}, {{-1, 0, 1}}, 0).rc == 2 && strstr(g_why, "target 0") && strstr(g_why, "item -1"));
    CHECK(batch({4, 2}, {{0, 0, 1}, {0, 1, 1}, {1, 2, 1}}, 0).rc == 2 && strstr(g_why, "target 2") && strstr(g_why, "row 2"));
    CHECK(batch({4, 2}, {{0, -1, 1}}, 0).rc == 2 && strstr(g_why, "target 0") && strstr(g_why, "row -1"));
    CHECK(batch({4, 2}, {{1, 1, 512}}, 0).rc == 2 && strstr(g_why, "target 0") && strstr(g_why, "token 512"));
    CHECK(batch({4, 2}, {{1, 1, 511}}, 0).rc == 0);
    CHECK(batch({4, 2}, {{1, 1, 5}}, -1).rc == 2 && strstr(g_why, "max_rows_per_pass"));
    CHECK(batch({}, {{0, 0, 5}}, 0).rc == 2 && strstr(g_why, "item 0"));
    ScoreBatchPlan bp;
    const int32_t one = 1;
    const ScoreTargetRef tr{0, 0, 0};
    CHECK(score_batch_plan(ScoreBatchShape{-1, &one, 0, &tr, 512, 256, 64, 0}, &bp, g_why, sizeof(g_why)) == 2 && strstr(g_why, "num_items"));
    CHECK(score_batch_plan(ScoreBatchShape{1, &one, -1, &tr, 512, 256, 64, 0}, &bp, g_why, sizeof(g_why)) == 2 && strstr(g_why, "num_targets"));
    CHECK(score_batch_plan(ScoreBatchShape{1, nullptr, 0, &tr, 512, 256, 64, 0}, &bp, g_why, sizeof(g_why)) == 2 && strstr(g_why, "null items"));
    CHECK(score_batch_plan(ScoreBatchShape{1, &one, 1, nullptr, 512, 256, 64, 0}, &bp, g_why, sizeof(g_why)) == 2 && strstr(g_why, "null targets"));
    CHECK(score_batch_plan(ScoreBatchShape{1, &one, 1, &tr, 0, 256, 64, 0}, &bp, g_why, sizeof(g_why)) == 2 && strstr(g_why, "vocab"));
    CHECK(score_batch_plan(ScoreBatchShape{1, &one, 1, &tr, 512, 256, 64, 0}, &bp, g_why, sizeof(g_why)) == 0 && bp.num_rows == 1);
}

int main(int argc, char** argv) {
    const char* which = argc > 1 ? argv[1] : "";
    if (!strcmp(which, "segments")) check_segments();
    else if (!strcmp(which, "workspace")) check_workspace();
    else if (!strcmp(which, "passes")) check_passes();
    else if (!strcmp(which, "roundtrip")) check_roundtrip();
    else if (!strcmp(which, "invalid")) check_invalid();
    else { printf("usage: score_plan_check <segments|workspace|passes|roundtrip|invalid>\n"); return 2; }
    printf("%s: %d checked, %d failed\n", which, g_checked, g_failed);
    return g_failed ? 1 : 0;
}
