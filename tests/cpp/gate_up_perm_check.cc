// Stand-alone check of fh::gate_up_col_perm (csrc/w4_repack.cc), the column order of a fused gate_up stack: supertile st of the
// packed matrix holds gate columns [32·st, 32·st + 32) followed by up columns [I + 32·st, I + 32·st + 32), I = n / 2.  Built by
// tests/test_knobs.py from this file and w4_repack.cc (host side only) and run as a child process; no GPU is touched.
#include <stdarg.h>
#include <stdio.h>

#include <algorithm>

#include "w4_upload.h"

namespace fh {
void set_error(const char*, ...) {}
}  // namespace fh

static int g_failed = 0, g_checked = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        g_checked++;                                                                     \
        if (!(cond)) { g_failed++; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

int main() {
    std::vector<int32_t> want;
    for (int first : {0, 64, 32, 96})
        for (int c = 0; c < 32; c++) want.push_back(first + c);
    CHECK(fh::gate_up_col_perm(128) == want);
    for (int n : {64, 256}) {
        std::vector<int32_t> p = fh::gate_up_col_perm(n);
        CHECK((int)p.size() == n);
        std::sort(p.begin(), p.end());
        for (int i = 0; i < n && i < (int)p.size(); i++) CHECK(p[i] == i);
    }
    printf("gate_up_perm: %d checked, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
