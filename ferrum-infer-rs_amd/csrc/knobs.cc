// Development knobs (read once, at library load) and kernel-form accounting: the two tables of knobs.h turned into code.
// Host-only: builds with a plain host compiler, no HIP header.
#include "knobs.h"

#include <stdlib.h>

#include <algorithm>
#include <atomic>

namespace fh {

static Knobs g_knobs;
static int knob_INT(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static bool knob_FLAG(const char* name, bool) { const char* e = getenv(name); return e && atoi(e) != 0; }
static bool knob_PRESENT(const char* name, bool) { return getenv(name) != nullptr; }
void reload_knobs() {
    Knobs k;
#define FH_KNOB_READ(type, field, env, dflt, kind) k.field = (type)knob_##kind(env, dflt);
    FH_KNOBS(FH_KNOB_READ)
#undef FH_KNOB_READ
    // the three that are not a plain read
    k.chain_max_rows = std::min(128, k.chain_max_rows);
    k.trace_launches = k.trace_launches && k.no_graph;
    k.attn_flash_min_rows_set = getenv("FERRUM_HIP_ATTN_FLASH_MIN_ROWS") != nullptr;
    g_knobs = k;
}
namespace { struct KnobsInit { KnobsInit() { reload_knobs(); } } g_knobs_init; }
const Knobs& knobs() { return g_knobs; }

static std::atomic<uint64_t> g_form_hits[FORM_COUNT];
void form_hit(Form f) { g_form_hits[f].fetch_add(1, std::memory_order_relaxed); }
void form_hits_snapshot(uint64_t* hits) {
    for (int i = 0; i < FORM_COUNT; i++) hits[i] = g_form_hits[i].load(std::memory_order_relaxed);
}
void form_hits_reset() {
    for (int i = 0; i < FORM_COUNT; i++) g_form_hits[i].store(0, std::memory_order_relaxed);
}
static const char* const g_form_names[FORM_COUNT] = {
#define FH_FORM_NAME(id, name) name,
    FH_FORMS(FH_FORM_NAME)
#undef FH_FORM_NAME
};
const char* form_name(int f) { return f >= 0 && f < FORM_COUNT ? g_form_names[f] : nullptr; }

}  // namespace fh
