// MarlinExpertStack::gemm_phase_batched (marlin_expert_stack.rs:63-74), host side: the dispatch list
// (expert, in_row_offset, out_row_offset, m) becomes the block-major routing arrays of the grouped GEMM — one group per
// distinct output displacement (out_off − in_off; normally one: in_off == out_off, the packed-row convention), 16-row
// blocks, or 64-row LDS tiles when the experts see ≥ 32 rows on average.  Host-only: standard library and error.h.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "error.h"

namespace fh {

struct BatchedDispatchPlan {
    long rows = 0;       // Σ m (0: nothing to launch, no groups)
    long max_row = 0;    // max(in_off + m): the input row count, and the sentinel of the padding rows (= prob_m)
    int br = 16;         // rows per block
    struct Group {
        long delta = 0;                 // out_off − in_off: row (in_off + r) of the shifted output view = out_off + r
        std::vector<int32_t> sorted;    // [blocks.size() · br] input rows, padded with max_row
        std::vector<int32_t> blocks;    // expert id per block
    };
    std::vector<Group> groups;          // first-seen order of the displacements
};

inline int plan_batched_dispatch(const int32_t* dispatches, int num_dispatches, int num_experts, BatchedDispatchPlan* out) {
    *out = BatchedDispatchPlan();
    long rows = 0, max_row = 0;
    for (int i = 0; i < num_dispatches; i++) {
        const int32_t* d = dispatches + 4 * i;
        FH_REQUIRE(d[0] >= 0 && d[0] < num_experts && d[1] >= 0 && d[2] >= 0 && d[3] >= 0,
                   "gemm_phase_batched: dispatch %d = (%d, %d, %d, %d) out of range", i, d[0], d[1], d[2], d[3]);
        rows += d[3];
        max_row = std::max<long>(max_row, (long)d[1] + d[3]);
    }
    out->rows = rows; out->max_row = max_row;
    if (rows == 0) return 0;
    const int br = out->br = rows >= 32L * num_dispatches ? 64 : 16;
    // group by output displacement
    std::vector<long> deltas;
    for (int i = 0; i < num_dispatches; i++) {
        const long dl = (long)dispatches[4 * i + 2] - dispatches[4 * i + 1];
        if (dispatches[4 * i + 3] > 0 && std::find(deltas.begin(), deltas.end(), dl) == deltas.end()) deltas.push_back(dl);
    }
    for (long dl : deltas) {
        out->groups.emplace_back();
        BatchedDispatchPlan::Group& g = out->groups.back();
        g.delta = dl;
        for (int i = 0; i < num_dispatches; i++) {
            const int32_t* d = dispatches + 4 * i;
            if (d[3] == 0 || (long)d[2] - d[1] != dl) continue;
            for (int r0 = 0; r0 < d[3]; r0 += br) {
                g.blocks.push_back(d[0]);
                for (int r = 0; r < br; r++) g.sorted.push_back(r0 + r < d[3] ? d[1] + r0 + r : (int32_t)max_row);   // sentinel = prob_m
            }
        }
    }
    return 0;
}

}  // namespace fh
