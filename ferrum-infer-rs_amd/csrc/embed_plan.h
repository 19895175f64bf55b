// Launch plan of the embedding tail (embed_pool.hip): argument checks, how a span of rows is cut into chunks for mean pooling,
// how much of the workspace the fp32 partials take (two levels for long spans), the grids.  Host-only (the standard library,
// nothing else) and pure integer arithmetic, so every comparison is checked on the CPU (tests/cpp/embed_plan_check.cc); the
// launcher only executes a plan.  The span functions are the ones the kernels call, so host and device cannot disagree about a
// span's chunks.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#if defined(__HIPCC__)
#define FH_EMBED_HD __host__ __device__
#else
#define FH_EMBED_HD
#endif

namespace fh {

enum EmbedPooling : int { EMBED_POOL_LAST = 0, EMBED_POOL_MEAN = 1, EMBED_POOL_FIRST = 2 };

constexpr int EMBED_MAX_DIM = 16384;        // 256 threads × 8 vectors × 8 elements, as embed_rms_norm
constexpr int EMBED_CHUNK_ROWS = 16;        // rows one workgroup sums for a mean (one partial row of `dim` floats each)
constexpr int EMBED_MAX_CHUNKS = 512;       // partial slots per span: 8192 rows at 16 per chunk
constexpr int EMBED_MAX_SEQS = 65535;       // grid.y
constexpr int EMBED_REDUCE_GROUP = 16;      // a span of more than EMBED_REDUCE_ABOVE chunks has its partials summed in groups of this many
constexpr int EMBED_REDUCE_ABOVE = 32;      // (a second level of partials) before the finish, which then adds ≤ 32 rows, not ≤ 512

// Rows per chunk of a span of `len` rows that owns `max_chunks` partial slots: EMBED_CHUNK_ROWS, doubled while the span would
// need more slots than it owns.  A function of the span's own length (and the slot count of the launch, which only binds where
// the workspace is too small for the chunks wanted): what else is in the launch never moves a span's chunk seams.
FH_EMBED_HD inline long embed_span_chunk_rows(long len, int max_chunks) {
    long r = EMBED_CHUNK_ROWS;
    while (r * max_chunks < len) r *= 2;
    return r;
}
FH_EMBED_HD inline int embed_span_chunks(long len, int max_chunks) {
    if (len <= 0) return 0;
    const long r = embed_span_chunk_rows(len, max_chunks);
    return (int)((len + r - 1) / r);
}

// second-level partials of a span of n chunks: 0 = none, the finish adds the n chunk partials themselves
FH_EMBED_HD inline int embed_span_groups(int n) { return n > EMBED_REDUCE_ABOVE ? (n + EMBED_REDUCE_GROUP - 1) / EMBED_REDUCE_GROUP : 0; }

struct EmbedShape {
    int num_seqs, dim, pooling, normalize, dims;
    int max_span_rows;                 // longest span when the host knows it (the runner does), ≤ 0: unknown
};

struct EmbedPlan {
    int out_dim;                       // dims ? dims : dim
    int vec_chunks;                    // 16-byte vectors of a row per thread: 1, 2, 4 or 8
    bool partials;                     // mean: the partial launch runs before the finish launch
    int max_chunks;                    // partial slots per span, [num_seqs][max_chunks][dim] fp32 in the workspace
    unsigned partial_grid_x, partial_grid_y;   // (chunk, span)
    bool reduce;                       // max_chunks > EMBED_REDUCE_ABOVE: the group launch runs between the two
    int max_groups;                    // second-level slots per span, [num_seqs][max_groups][dim] fp32 behind the first level
    unsigned reduce_grid_x, reduce_grid_y;     // (group, span)
    size_t level2_offset;              // floats from the workspace's start to the second level
    unsigned finish_grid_x;            // one workgroup per span
    int block;
    size_t workspace_want;             // bytes the chunks wanted take (before the fallback to fewer)
    size_t workspace_used;             // bytes the chosen slot count takes: ≤ the workspace given
};

// 0 and *p filled, or 2 (FERRUM_HIP_INVALID) and a message in `why`
inline int embed_plan(const EmbedShape& sh, size_t workspace_bytes, EmbedPlan* p, char* why, size_t why_cap) {
#define FH_EMBED_REJECT(cond, ...)                    \
    do {                                              \
        if (cond) {                                   \
            snprintf(why, why_cap, __VA_ARGS__);      \
            return 2;                                 \
        }                                             \
    } while (0)
    FH_EMBED_REJECT(sh.num_seqs < 0 || sh.num_seqs > EMBED_MAX_SEQS, "embed_pool: num_seqs=%d must be in [0, %d]", sh.num_seqs, EMBED_MAX_SEQS);
    FH_EMBED_REJECT(sh.dim <= 0 || sh.dim % 8 != 0 || sh.dim > EMBED_MAX_DIM, "embed_pool: dim=%d must be a multiple of 8 and <= %d", sh.dim,
                    EMBED_MAX_DIM);
    FH_EMBED_REJECT(sh.pooling < EMBED_POOL_LAST || sh.pooling > EMBED_POOL_FIRST, "embed_pool: pooling=%d must be 0 (last), 1 (mean) or 2 (first)",
                    sh.pooling);
    FH_EMBED_REJECT(sh.dims < 0 || sh.dims > sh.dim, "embed_pool: dims=%d must be 0 (all) or in [1, dim=%d]", sh.dims, sh.dim);
    *p = EmbedPlan{};
    p->out_dim = sh.dims ? sh.dims : sh.dim;
    const int per_thread = (sh.dim / 8 + 255) / 256;
    p->vec_chunks = per_thread <= 1 ? 1 : per_thread <= 2 ? 2 : per_thread <= 4 ? 4 : 8;
    p->block = 256;
    p->finish_grid_x = (unsigned)sh.num_seqs;
    if (sh.pooling != EMBED_POOL_MEAN || sh.num_seqs == 0) return 0;
    int want = EMBED_MAX_CHUNKS;
    if (sh.max_span_rows > 0) {
        const long c = ((long)sh.max_span_rows + EMBED_CHUNK_ROWS - 1) / EMBED_CHUNK_ROWS;
        if (c < want) want = (int)c;
    }
    const size_t slot_bytes = (size_t)sh.num_seqs * sh.dim * sizeof(float);       // one partial row of every span
    p->workspace_want = slot_bytes * ((size_t)want + embed_span_groups(want));
    const size_t fit = workspace_bytes / slot_bytes;
    FH_EMBED_REJECT(fit == 0, "embed_pool: mean pooling of %d spans of dim %d needs a workspace of at least %zu bytes, got %zu", sh.num_seqs,
                    sh.dim, slot_bytes, workspace_bytes);
    // the most chunks per span (≤ want) whose two levels of partials fit
    int mc = fit < (size_t)want ? (int)fit : want;
    while ((size_t)mc + embed_span_groups(mc) > fit) mc--;
    p->max_chunks = mc;
    p->partials = true;
    p->partial_grid_x = (unsigned)mc;
    p->partial_grid_y = (unsigned)sh.num_seqs;
    p->max_groups = embed_span_groups(mc);
    p->reduce = p->max_groups > 0;
    p->reduce_grid_x = (unsigned)p->max_groups;
    p->reduce_grid_y = p->reduce ? (unsigned)sh.num_seqs : 0;
    p->level2_offset = (size_t)sh.num_seqs * mc * sh.dim;
    p->workspace_used = slot_bytes * ((size_t)mc + p->max_groups);
#undef FH_EMBED_REJECT
    return 0;
}

}  // namespace fh
