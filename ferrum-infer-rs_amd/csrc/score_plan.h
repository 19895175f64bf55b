// Launch plan of the scoring head (score_head.hip, ferrum_hip_model_score): argument checks, how a row of logits is cut into
// segments, the grids, the workspace the partials take; and, for the model-level call, which rows of the packed batch are scored,
// how they are cut into lm_head passes, where each target's result lands and how large the buffers are.  Host-only (the standard
// library, nothing else) and pure integer arithmetic, so every comparison is checked on the CPU (tests/cpp/score_plan_check.cc);
// the launcher and the runner only execute a plan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

namespace fh {

constexpr int SCORE_SEGMENT = 4096;          // elements of a row one workgroup reduces: 256 threads × 4 loads × 16 bytes.  A compile-time
                                             // constant, so a row's seams sit at multiples of it and depend on nothing but n
constexpr int SCORE_BLOCK = 256;
constexpr int SCORE_MAX_ROWS = 65535;        // grid.y
constexpr int SCORE_DEFAULT_PASS_ROWS = 256; // rows of one lm_head pass of ferrum_hip_model_score (min with max_tokens)

#define FH_SCORE_REJECT(cond, ...)                \
    do {                                          \
        if (cond) {                               \
            snprintf(why, why_cap, __VA_ARGS__);  \
            return 2;                             \
        }                                         \
    } while (0)

inline int score_segments(int n) { return n <= 0 ? 0 : (int)(((long)n + SCORE_SEGMENT - 1) / SCORE_SEGMENT); }

struct ScoreShape {
    int m, n, ld, num_pairs;
};

// The workspace, in 4-byte words from its start: [m][segments] fp32 maxima, then as many fp32 sums, then as many int32 first
// arguments, then [m] fp32 log-sum-exps (what the gather reads, row_lse being optional).  Every word read is written first.
struct ScorePlan {
    int segments;
    unsigned partial_grid_x, partial_grid_y;   // (segment, row)
    unsigned merge_grid_x;                     // one wave per row
    unsigned gather_grid_x;                    // 256 pairs per workgroup; 0: no gather launch
    int block;
    size_t off_sum, off_idx, off_lse;
    size_t workspace_bytes;
};

// 0 and *p filled, or 2 (FERRUM_HIP_INVALID) and a message in `why`
inline int score_plan(const ScoreShape& sh, size_t workspace_bytes, ScorePlan* p, char* why, size_t why_cap) {
    FH_SCORE_REJECT(sh.m < 0 || sh.m > SCORE_MAX_ROWS, "logprob_rows: m=%d must be in [0, %d]", sh.m, SCORE_MAX_ROWS);
    FH_SCORE_REJECT(sh.num_pairs < 0, "logprob_rows: num_pairs=%d must not be negative", sh.num_pairs);
    *p = ScorePlan{};
    p->block = SCORE_BLOCK;
    if (sh.m == 0) {
        FH_SCORE_REJECT(sh.num_pairs > 0, "logprob_rows: num_pairs=%d but there are no rows", sh.num_pairs);
        return 0;
    }
    FH_SCORE_REJECT(sh.n <= 0, "logprob_rows: n=%d must be positive", sh.n);
    FH_SCORE_REJECT(sh.ld < sh.n, "logprob_rows: ld=%d is less than n=%d", sh.ld, sh.n);
    p->segments = score_segments(sh.n);
    p->partial_grid_x = (unsigned)p->segments;
    p->partial_grid_y = (unsigned)sh.m;
    p->merge_grid_x = (unsigned)sh.m;
    p->gather_grid_x = (unsigned)(((long)sh.num_pairs + SCORE_BLOCK - 1) / SCORE_BLOCK);
    const size_t parts = (size_t)sh.m * p->segments;
    p->off_sum = parts;
    p->off_idx = 2 * parts;
    p->off_lse = 3 * parts;
    p->workspace_bytes = (3 * parts + (size_t)sh.m) * 4;
    FH_SCORE_REJECT(workspace_bytes < p->workspace_bytes, "logprob_rows: %d rows of %d need a workspace of %zu bytes, got %zu", sh.m, sh.n,
                    p->workspace_bytes, workspace_bytes);
    return 0;
}

// ── the model-level call ─────────────────────────────────────────────────────
struct ScoreTargetRef {     // FerrumHipScoreTarget without its padding
    int32_t item, row;
    uint32_t token;
};

struct ScoreBatchShape {
    int num_items;
    const int32_t* item_rows;     // [num_items] num_q_tokens of every item
    int num_targets;
    const ScoreTargetRef* targets;
    int vocab, hidden, max_tokens;
    int max_rows_per_pass;        // 0 = min(max_tokens, SCORE_DEFAULT_PASS_ROWS)
};

// Pairs are the targets sorted by (packed row, target index): the pairs of one pass are contiguous, and so are those of one row.
struct ScoreBatchPlan {
    int pass_rows = 0;                       // C
    int num_rows = 0, num_passes = 0;        // R distinct scored rows, ⌈R / C⌉
    std::vector<int32_t> rows;               // [R] packed row (item's first row + target row), ascending
    std::vector<int32_t> pass_row_begin;     // [passes + 1] into rows
    std::vector<int32_t> pass_pair_begin;    // [passes + 1] into the pair lists
    std::vector<int32_t> pair_rows;          // [T] row inside its pass
    std::vector<uint32_t> pair_tokens;       // [T]
    std::vector<int32_t> target_pair;        // [T] target → its pair
    std::vector<int32_t> target_pass, target_pass_row;   // [T] target → (pass, row in pass); its row of `rows` is pass · C + row
    // device buffers, bytes: the normed rows [C, hidden] fp16, the logits [C, vocab] fp32, the lists (rows | pair_rows |
    // pair_tokens, 4-byte words) and the results (pair log-probs [T] | row top log-probs [R] | row top tokens [R], 4-byte words)
    size_t hidden_bytes = 0, logits_bytes = 0, lists_bytes = 0, results_bytes = 0;
    size_t workspace_bytes = 0;              // of the op at C rows
};

inline int score_batch_plan(const ScoreBatchShape& sh, ScoreBatchPlan* p, char* why, size_t why_cap) {
    FH_SCORE_REJECT(sh.num_items < 0, "model_score: num_items=%d must not be negative", sh.num_items);
    FH_SCORE_REJECT(sh.num_targets < 0, "model_score: num_targets=%d must not be negative", sh.num_targets);
    FH_SCORE_REJECT(sh.max_rows_per_pass < 0, "model_score: max_rows_per_pass=%d must not be negative", sh.max_rows_per_pass);
    FH_SCORE_REJECT(sh.num_items > 0 && !sh.item_rows, "model_score: null items");
    FH_SCORE_REJECT(sh.num_targets > 0 && !sh.targets, "model_score: null targets");
    FH_SCORE_REJECT(sh.vocab <= 0 || sh.hidden <= 0 || sh.max_tokens <= 0, "model_score: vocab=%d, hidden=%d, max_tokens=%d must be positive",
                    sh.vocab, sh.hidden, sh.max_tokens);
    *p = ScoreBatchPlan{};
    const int T = sh.num_targets;
    std::vector<int32_t> first(sh.num_items + 1, 0);
    for (int i = 0; i < sh.num_items; i++) first[i + 1] = first[i] + (sh.item_rows[i] > 0 ? sh.item_rows[i] : 0);
    std::vector<int32_t> packed(T), order(T);
    for (int t = 0; t < T; t++) {
        const ScoreTargetRef& g = sh.targets[t];
        FH_SCORE_REJECT(g.item < 0 || g.item >= sh.num_items, "model_score: target %d names item %d of %d", t, g.item, sh.num_items);
        FH_SCORE_REJECT(g.row < 0 || g.row >= sh.item_rows[g.item], "model_score: target %d names row %d of item %d, which has %d", t, g.row,
                        g.item, sh.item_rows[g.item]);
        FH_SCORE_REJECT(g.token >= (uint32_t)sh.vocab, "model_score: target %d names token %u, the vocabulary has %d", t, g.token, sh.vocab);
        packed[t] = first[g.item] + g.row;
        order[t] = t;
    }
    p->pass_rows = sh.max_rows_per_pass ? sh.max_rows_per_pass : std::min(sh.max_tokens, SCORE_DEFAULT_PASS_ROWS);
    if (p->pass_rows > SCORE_MAX_ROWS) p->pass_rows = SCORE_MAX_ROWS;
    const int C = p->pass_rows;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return packed[a] != packed[b] ? packed[a] < packed[b] : a < b; });
    p->pair_rows.resize(T);
    p->pair_tokens.resize(T);
    p->target_pair.resize(T);
    p->target_pass.resize(T);
    p->target_pass_row.resize(T);
    p->pass_row_begin.push_back(0);
    p->pass_pair_begin.push_back(0);
    for (int k = 0; k < T; k++) {
        const int t = order[k];
        if (p->rows.empty() || p->rows.back() != packed[t]) {
            if (!p->rows.empty() && (int)p->rows.size() % C == 0) {       // the pass is full: this row opens the next
                p->pass_row_begin.push_back((int32_t)p->rows.size());
                p->pass_pair_begin.push_back(k);
            }
            p->rows.push_back(packed[t]);
        }
        const int r = (int)p->rows.size() - 1;
        p->pair_rows[k] = r % C;
        p->pair_tokens[k] = sh.targets[t].token;
        p->target_pair[t] = k;
        p->target_pass[t] = r / C;
        p->target_pass_row[t] = r % C;
    }
    p->num_rows = (int)p->rows.size();
    p->num_passes = p->num_rows ? (p->num_rows + C - 1) / C : 0;
    if (p->num_rows) {
        p->pass_row_begin.push_back(p->num_rows);
        p->pass_pair_begin.push_back(T);
    }
    if (T == 0) return 0;
    const size_t widest = (size_t)std::min(C, p->num_rows);     // rows of the largest pass
    p->hidden_bytes = widest * sh.hidden * 2;
    p->logits_bytes = widest * sh.vocab * 4;
    p->lists_bytes = ((size_t)p->num_rows + 2 * (size_t)T) * 4;
    p->results_bytes = ((size_t)T + 2 * (size_t)p->num_rows) * 4;
    p->workspace_bytes = (3 * widest * score_segments(sh.vocab) + widest) * 4;
    return 0;
}

#undef FH_SCORE_REJECT

}  // namespace fh
