// Stand-alone check of fh::plan_batched_dispatch (csrc/moe_dispatch_plan.h), the host half of gemm_phase_batched: built and
// run by tests/test_dispatch_plan.py with plain g++ (under AddressSanitizer + UBSan where the toolchain links them), no GPU,
// no library.  The expected arrays are written out by hand from the rules: 16-row blocks unless Σ m ≥ 32 · dispatches (then
// 64), one group per distinct out_off − in_off in first-seen order, padding rows carry the sentinel max(in_off + m).
//   usage: dispatch_plan_check <groups|tiles|threshold|empty|refused|order>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "moe_dispatch_plan.h"

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

using fh::BatchedDispatchPlan;
using Ints = std::vector<int32_t>;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        g_checked++;                                                                     \
        if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s   (last error: %s)\n", __FILE__, __LINE__, #cond, g_err.c_str()); } \
    } while (0)

static int plan(const Ints& d, int num_experts, BatchedDispatchPlan* p) {
    return fh::plan_batched_dispatch(d.data(), (int)d.size() / 4, num_experts, p);
}
// first, first + 1, …, last
static Ints range(int first, int last) { Ints v; for (int i = first; i <= last; i++) v.push_back(i); return v; }
static Ints operator+(Ints a, const Ints& b) { a.insert(a.end(), b.begin(), b.end()); return a; }
static Ints fill(int n, int32_t v) { return Ints(n, v); }

static void check_groups() {
    // the middle dispatch is empty; the last one writes 5 rows further down than it reads: two groups
    BatchedDispatchPlan p;
    CHECK(plan({2, 0, 0, 3, 0, 3, 3, 0, 1, 3, 8, 20}, 3, &p) == 0);
    CHECK(p.rows == 23 && p.max_row == 23 && p.br == 16);              // 23 < 32 · 3
    CHECK(p.groups.size() == 2);
    if (p.groups.size() != 2) return;
    CHECK(p.groups[0].delta == 0 && p.groups[0].blocks == Ints{2});
    CHECK(p.groups[0].sorted == range(0, 2) + fill(13, 23));
    CHECK(p.groups[1].delta == 5 && (p.groups[1].blocks == Ints{1, 1}));
    CHECK(p.groups[1].sorted == range(3, 18) + range(19, 22) + fill(12, 23));
}

static void check_tiles() {
    BatchedDispatchPlan p;
    CHECK(plan({0, 0, 0, 70}, 1, &p) == 0);
    CHECK(p.rows == 70 && p.max_row == 70 && p.br == 64);              // 70 ≥ 32 · 1
    CHECK(p.groups.size() == 1);
    if (p.groups.size() != 1) return;
    CHECK(p.groups[0].delta == 0 && (p.groups[0].blocks == Ints{0, 0}));
    CHECK(p.groups[0].sorted == range(0, 63) + range(64, 69) + fill(58, 70));
}

static void check_threshold() {
    // two dispatches: 63 rows stay with 16-row blocks, 64 rows take the 64-row tiles
    BatchedDispatchPlan p;
    CHECK(plan({0, 0, 0, 31, 1, 31, 31, 32}, 2, &p) == 0);
    CHECK(p.rows == 63 && p.br == 16 && p.groups.size() == 1);
    if (p.groups.size() == 1) {
        CHECK((p.groups[0].blocks == Ints{0, 0, 1, 1}));
        CHECK(p.groups[0].sorted == range(0, 30) + fill(1, 63) + range(31, 62) && p.groups[0].sorted.size() == 64);
    }
    CHECK(plan({0, 0, 0, 32, 1, 32, 32, 32}, 2, &p) == 0);
    CHECK(p.rows == 64 && p.br == 64 && p.groups.size() == 1);
    if (p.groups.size() == 1) {
        CHECK((p.groups[0].blocks == Ints{0, 1}));
        CHECK(p.groups[0].sorted == range(0, 31) + fill(32, 64) + range(32, 63) + fill(32, 64));
    }
}

static void check_empty() {
    BatchedDispatchPlan p;
    CHECK(plan({0, 0, 0, 0, 1, 5, 9, 0}, 2, &p) == 0);
    CHECK(p.rows == 0 && p.groups.empty());
    CHECK(plan({}, 2, &p) == 0);
    CHECK(p.rows == 0 && p.groups.empty());
}

static void check_refused() {
    BatchedDispatchPlan p;
    g_err.clear();
    CHECK(plan({0, 0, 0, 1, 3, 0, 0, 1}, 3, &p) == 2);                 // expert id == num_experts
    CHECK(g_err == "gemm_phase_batched: dispatch 1 = (3, 0, 0, 1) out of range");
    CHECK(plan({2, 0, 0, 1}, 3, &p) == 0);                             // … the last valid one passes
    g_err.clear();
    CHECK(plan({-1, 0, 0, 1}, 3, &p) == 2);
    CHECK(g_err == "gemm_phase_batched: dispatch 0 = (-1, 0, 0, 1) out of range");
    g_err.clear();
    CHECK(plan({0, -1, 0, 1}, 3, &p) == 2);                            // negative input offset
    CHECK(g_err == "gemm_phase_batched: dispatch 0 = (0, -1, 0, 1) out of range");
    g_err.clear();
    CHECK(plan({0, 0, -4, 1}, 3, &p) == 2);                            // negative output offset
    CHECK(g_err == "gemm_phase_batched: dispatch 0 = (0, 0, -4, 1) out of range");
    g_err.clear();
    CHECK(plan({0, 0, 0, 1, 1, 1, 1, -2}, 3, &p) == 2);                // negative m
    CHECK(g_err == "gemm_phase_batched: dispatch 1 = (1, 1, 1, -2) out of range");
    CHECK(p.groups.empty());
}

static void check_order() {
    // displacements 4, 0, 4 arrive interleaved: groups in first-seen order, each with its dispatches in list order
    BatchedDispatchPlan p;
    CHECK(plan({0, 0, 4, 2, 1, 2, 2, 1, 2, 3, 7, 2}, 3, &p) == 0);
    CHECK(p.rows == 5 && p.max_row == 5 && p.br == 16 && p.groups.size() == 2);
    if (p.groups.size() != 2) return;
    CHECK(p.groups[0].delta == 4 && (p.groups[0].blocks == Ints{0, 2}));
    CHECK(p.groups[0].sorted == range(0, 1) + fill(14, 5) + range(3, 4) + fill(14, 5));
    CHECK(p.groups[1].delta == 0 && p.groups[1].blocks == Ints{1});
    CHECK(p.groups[1].sorted == range(2, 2) + fill(15, 5));
    // a negative displacement (output above the input) is a group like any other
    CHECK(plan({0, 6, 1, 2}, 1, &p) == 0);
    CHECK(p.max_row == 8 && p.groups.size() == 1 && p.groups[0].delta == -5);
}

int main(int argc, char** argv) {
    const std::string which = argc > 1 ? argv[1] : "";
    if (which == "groups") check_groups();
    else if (which == "tiles") check_tiles();
    else if (which == "threshold") check_threshold();
    else if (which == "empty") check_empty();
    else if (which == "refused") check_refused();
    else if (which == "order") check_order();
    else { printf("usage: dispatch_plan_check <groups|tiles|threshold|empty|refused|order>\n"); return 2; }
    printf("%s: %d checked, %d failed\n", which.c_str(), g_checked, g_failed);
    return g_failed ? 1 : 0;
}
