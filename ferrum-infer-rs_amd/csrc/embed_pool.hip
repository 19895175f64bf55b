// The tail of an embedding forward (gfx950): final norm → pool over a span of rows → cut to the leading `dims` components →
// L2-normalise, fp32 throughout (the normed row is never rounded to fp16).  What ferrum_hip_model_embed runs in place of the
// sampling head; reference: ferrum-engine/src/embedding_engine.rs (pool + normalise on the host there).
//
//   partial launch (mean only)  grid (chunk, span): one 256-thread workgroup norms the rows of one chunk of one span, one row at
//                               a time with the next rows' loads in flight, and writes Σ n_t as one fp32 row of the workspace
//                               [span][chunk][dim]
//   group launch (mean, spans   grid (group, span): the partials of 16 consecutive chunks summed in chunk order into a second
//   of more than 32 chunks)     level [span][group][dim], so that the finish adds ≤ 32 rows per span and not 512
//   finish launch               grid (span): mean — the span's partials (its groups, where it has them) summed in index order,
//                               ÷ L; last / first — that one row read and normed; then the cut, the L2 norm, the store
//
// Determinism: no atomics; a span's chunk seams come from its own length (embed_plan.h); rows inside a chunk and chunks inside
// a span are summed in index order; the reductions of a row are fixed trees.  So a span's vector is the same bit for bit
// whatever else the launch holds, and from run to run.
// A row is loaded once (16-byte loads, 8 elements per lane and vector) and kept in registers between its sum of squares and
// its scaling, as in norm.hip.
#include "common.h"
#include "embed_plan.h"
#include "kernels.h"

namespace fh {
namespace {

// eight consecutive elements of a row as they were loaded (fp16: one 16-byte load, fp32: two)
template <typename T> struct Raw8;
template <> struct Raw8<__half> {
    half8 v;
    __device__ __forceinline__ void load(const __half* p) { v = *reinterpret_cast<const half8*>(p); }
    __device__ __forceinline__ void zero() { for (int j = 0; j < 8; j++) v[j] = (_Float16)0; }
    __device__ __forceinline__ float get(int j) const { return (float)v[j]; }
};
template <> struct Raw8<float> {
    float4v lo, hi;
    __device__ __forceinline__ void load(const float* p) {
        lo = reinterpret_cast<const float4v*>(p)[0];
        hi = reinterpret_cast<const float4v*>(p)[1];
    }
    __device__ __forceinline__ void zero() { for (int j = 0; j < 4; j++) lo[j] = hi[j] = 0.f; }
    __device__ __forceinline__ float get(int j) const { return j < 4 ? lo[j] : hi[j - 4]; }
};

// Σ over the 256 threads, every thread gets it; `slot` [4] must not be rewritten before every thread has read it (the callers
// alternate two slots, or use each once)
__device__ __forceinline__ float block_sum_256(float v, float* slot) {
    v = wave_reduce_sum(v);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    return slot[0] + slot[1] + slot[2] + slot[3];
}

template <typename T, int CHUNKS, bool NORM>
__global__ __launch_bounds__(256) void embed_pool_partial_kernel(const T* __restrict__ hidden, const int32_t* __restrict__ seq_rows,
                                                                 const __half* __restrict__ w, float eps, float* __restrict__ partial,
                                                                 int dim, int max_chunks) {
    __shared__ float red[2][4];
    const int seq = blockIdx.y, chunk = blockIdx.x;
    const long b = seq_rows[2 * seq], e = seq_rows[2 * seq + 1], len = e - b;
    if (len <= 0) return;
    const long rows = embed_span_chunk_rows(len, max_chunks);
    const long r0 = b + chunk * rows;
    if (r0 >= e) return;                                   // (the grid holds max_chunks chunks for every span)
    const long r1 = r0 + rows < e ? r0 + rows : e;
    const int nvec = dim >> 3;
    constexpr int DEPTH = CHUNKS <= 2 ? 4 : 2;             // rows in registers: the one being summed and DEPTH − 1 on their way
    float acc[CHUNKS][8];
    half8 wv[CHUNKS];
    Raw8<T> ring[DEPTH][CHUNKS];
#pragma unroll
    for (int c = 0; c < CHUNKS; c++) {
        const int i = threadIdx.x + c * 256;
#pragma unroll
        for (int j = 0; j < 8; j++) acc[c][j] = 0.f;
        if (NORM) {
#pragma unroll
            for (int j = 0; j < 8; j++) wv[c][j] = (_Float16)0;
            if (i < nvec) wv[c] = *reinterpret_cast<const half8*>(w + i * 8);
        }
#pragma unroll
        for (int s = 0; s < DEPTH; s++) {
            ring[s][c].zero();
            if (i < nvec && r0 + s < r1) ring[s][c].load(hidden + (r0 + s) * dim + i * 8);
        }
    }
    int par = 0;
    for (long base = r0; base < r1; base += DEPTH) {
#pragma unroll
        for (int s = 0; s < DEPTH; s++) {
            const long r = base + s;
            if (r >= r1) break;                            // (uniform)
            float inv = 1.f;
            if (NORM) {
                float ss = 0.f;
#pragma unroll
                for (int c = 0; c < CHUNKS; c++)
#pragma unroll
                    for (int j = 0; j < 8; j++) ss += ring[s][c].get(j) * ring[s][c].get(j);
                const float total = block_sum_256(ss, red[par]);      // (slot `par` is next written two rows on, behind the next barrier)
                par ^= 1;
                inv = 1.0f / sqrtf(total / (float)dim + eps);
            }
#pragma unroll
            for (int c = 0; c < CHUNKS; c++) {
#pragma unroll
                for (int j = 0; j < 8; j++) acc[c][j] += NORM ? ring[s][c].get(j) * inv * (float)wv[c][j] : ring[s][c].get(j);
                const int i = threadIdx.x + c * 256;
                if (i < nvec && r + DEPTH < r1) ring[s][c].load(hidden + (r + DEPTH) * dim + i * 8);     // the slot's next row
            }
        }
    }
    float* dst = partial + ((long)seq * max_chunks + chunk) * dim;
#pragma unroll
    for (int c = 0; c < CHUNKS; c++) {
        const int i = threadIdx.x + c * 256;
        if (i < nvec) {
            float4v lo, hi;
#pragma unroll
            for (int j = 0; j < 4; j++) { lo[j] = acc[c][j]; hi[j] = acc[c][4 + j]; }
            reinterpret_cast<float4v*>(dst + i * 8)[0] = lo;
            reinterpret_cast<float4v*>(dst + i * 8)[1] = hi;
        }
    }
}

// second level of a long span's partials: group g = Σ of its chunks [16 g, 16 g + 16) in chunk order
template <int CHUNKS>
__global__ __launch_bounds__(256) void embed_pool_group_kernel(const int32_t* __restrict__ seq_rows, const float* __restrict__ partial,
                                                               float* __restrict__ level2, int dim, int max_chunks, int max_groups) {
    const int seq = blockIdx.y, g = blockIdx.x;
    const long len = (long)seq_rows[2 * seq + 1] - seq_rows[2 * seq];
    const int n = embed_span_chunks(len, max_chunks);
    if (g >= embed_span_groups(n)) return;                 // (short spans have no second level)
    const int k0 = g * EMBED_REDUCE_GROUP, k1 = k0 + EMBED_REDUCE_GROUP < n ? k0 + EMBED_REDUCE_GROUP : n;
    const int nvec = dim >> 3;
    const float* src = partial + (long)seq * max_chunks * dim;
    float* dst = level2 + ((long)seq * max_groups + g) * dim;
#pragma unroll
    for (int c = 0; c < CHUNKS; c++) {
        const int i = threadIdx.x + c * 256;
        if (i >= nvec) continue;
        float4v lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int k = k0; k < k1; k++) {
            lo += reinterpret_cast<const float4v*>(src + (long)k * dim + i * 8)[0];
            hi += reinterpret_cast<const float4v*>(src + (long)k * dim + i * 8)[1];
        }
        reinterpret_cast<float4v*>(dst + i * 8)[0] = lo;
        reinterpret_cast<float4v*>(dst + i * 8)[1] = hi;
    }
}

template <typename T, int CHUNKS>
__global__ __launch_bounds__(256) void embed_pool_finish_kernel(const T* __restrict__ hidden, const int32_t* __restrict__ seq_rows,
                                                                const __half* __restrict__ w, float eps, const float* __restrict__ partial,
                                                                const float* __restrict__ level2, int max_chunks, int max_groups, int pooling,
                                                                int normalize, int d, float* __restrict__ out, int dim) {
    __shared__ float red[2][4];
    const int seq = blockIdx.x;
    const long b = seq_rows[2 * seq], e = seq_rows[2 * seq + 1], len = e - b;
    const int nvec = dim >> 3;
    float v[CHUNKS][8];
#pragma unroll
    for (int c = 0; c < CHUNKS; c++)
#pragma unroll
        for (int j = 0; j < 8; j++) v[c][j] = 0.f;
    if (len > 0 && pooling == EMBED_POOL_MEAN) {
        const int chunks = embed_span_chunks(len, max_chunks), groups = embed_span_groups(chunks);
        const int n = groups ? groups : chunks;
        const float* src = groups ? level2 + (long)seq * max_groups * dim : partial + (long)seq * max_chunks * dim;
#pragma unroll 4
        for (int k = 0; k < n; k++) {
#pragma unroll
            for (int c = 0; c < CHUNKS; c++) {
                const int i = threadIdx.x + c * 256;
                if (i < nvec) {
                    const float4v lo = reinterpret_cast<const float4v*>(src + (long)k * dim + i * 8)[0];
                    const float4v hi = reinterpret_cast<const float4v*>(src + (long)k * dim + i * 8)[1];
#pragma unroll
                    for (int j = 0; j < 4; j++) { v[c][j] += lo[j]; v[c][4 + j] += hi[j]; }
                }
            }
        }
        const float L = (float)len;
#pragma unroll
        for (int c = 0; c < CHUNKS; c++)
#pragma unroll
            for (int j = 0; j < 8; j++) v[c][j] = v[c][j] / L;
    } else if (len > 0) {
        const long row = pooling == EMBED_POOL_LAST ? e - 1 : b;
        Raw8<T> x[CHUNKS];
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < CHUNKS; c++) {
            const int i = threadIdx.x + c * 256;
            x[c].zero();
            if (i < nvec) x[c].load(hidden + row * dim + i * 8);
#pragma unroll
            for (int j = 0; j < 8; j++) ss += x[c].get(j) * x[c].get(j);
        }
        if (w) {                                            // (uniform)
            const float total = block_sum_256(ss, red[0]);
            const float inv = 1.0f / sqrtf(total / (float)dim + eps);
#pragma unroll
            for (int c = 0; c < CHUNKS; c++) {
                const int i = threadIdx.x + c * 256;
                if (i < nvec) {
                    const half8 wv = *reinterpret_cast<const half8*>(w + i * 8);
#pragma unroll
                    for (int j = 0; j < 8; j++) v[c][j] = x[c].get(j) * inv * (float)wv[j];
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < CHUNKS; c++)
#pragma unroll
                for (int j = 0; j < 8; j++) v[c][j] = x[c].get(j);
        }
    }
    // the cut comes first, the L2 norm is taken over what is kept
    if (normalize) {
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < CHUNKS; c++) {
            const int i = threadIdx.x + c * 256;
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (i * 8 + j < d) ss += v[c][j] * v[c][j];
        }
        const float r = fmaxf(sqrtf(block_sum_256(ss, red[1])), 1e-12f);
#pragma unroll
        for (int c = 0; c < CHUNKS; c++)
#pragma unroll
            for (int j = 0; j < 8; j++) v[c][j] = v[c][j] / r;
    }
    float* dst = out + (long)seq * d;
    const bool vec4 = (d & 3) == 0;                        // rows of the output then start 16-byte aligned
#pragma unroll
    for (int c = 0; c < CHUNKS; c++) {
        const int i = threadIdx.x + c * 256;
        if (vec4) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                if (i * 8 + h * 4 < d) {
                    float4v o;
#pragma unroll
                    for (int j = 0; j < 4; j++) o[j] = v[c][h * 4 + j];
                    *reinterpret_cast<float4v*>(dst + i * 8 + h * 4) = o;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (i * 8 + j < d) dst[i * 8 + j] = v[c][j];
        }
    }
}

template <typename T>
int launch_embed_pool(const EmbedPlan& p, const T* hidden, const int32_t* seq_rows, const __half* w, float eps, int pooling, int normalize,
                      float* out, int dim, float* workspace, hipStream_t s) {
    const dim3 block(p.block);
    if (p.partials) {
        const dim3 grid(p.partial_grid_x, p.partial_grid_y);
#define FH_EP(C)                                                                                                                     \
    do {                                                                                                                             \
        if (w) hipLaunchKernelGGL((embed_pool_partial_kernel<T, C, true>), grid, block, 0, s, hidden, seq_rows, w, eps, workspace, dim, p.max_chunks); \
        else hipLaunchKernelGGL((embed_pool_partial_kernel<T, C, false>), grid, block, 0, s, hidden, seq_rows, w, eps, workspace, dim, p.max_chunks); \
    } while (0)
        if (p.vec_chunks == 1) FH_EP(1); else if (p.vec_chunks == 2) FH_EP(2); else if (p.vec_chunks == 4) FH_EP(4); else FH_EP(8);
#undef FH_EP
        FH_CHECK_LAUNCH();
    }
    float* level2 = workspace ? workspace + p.level2_offset : nullptr;
    if (p.reduce) {
        const dim3 grid(p.reduce_grid_x, p.reduce_grid_y);
#define FH_EG(C) hipLaunchKernelGGL((embed_pool_group_kernel<C>), grid, block, 0, s, seq_rows, workspace, level2, dim, p.max_chunks, p.max_groups)
        if (p.vec_chunks == 1) FH_EG(1); else if (p.vec_chunks == 2) FH_EG(2); else if (p.vec_chunks == 4) FH_EG(4); else FH_EG(8);
#undef FH_EG
        FH_CHECK_LAUNCH();
    }
    const dim3 grid(p.finish_grid_x);
#define FH_EF(C) hipLaunchKernelGGL((embed_pool_finish_kernel<T, C>), grid, block, 0, s, hidden, seq_rows, w, eps, workspace, level2, p.max_chunks, p.max_groups, pooling, normalize, p.out_dim, out, dim)
    if (p.vec_chunks == 1) FH_EF(1); else if (p.vec_chunks == 2) FH_EF(2); else if (p.vec_chunks == 4) FH_EF(4); else FH_EF(8);
#undef FH_EF
    FH_CHECK_LAUNCH();
    return 0;
}

}  // namespace

int embed_pool(const void* hidden, bool hidden_f32, const int32_t* seq_rows, const __half* norm_w, float eps, int pooling, int normalize,
               int dims, float* out, int num_seqs, int dim, int max_span_rows, float* workspace, size_t workspace_bytes, hipStream_t s) {
    EmbedPlan p;
    char why[256];
    if (embed_plan(EmbedShape{num_seqs, dim, pooling, normalize, dims, max_span_rows}, workspace ? workspace_bytes : 0, &p, why, sizeof(why))) {
        fh::set_error("%s", why);
        return 2;
    }
    if (num_seqs == 0) return 0;
    FH_REQUIRE(hidden && seq_rows && out, "embed_pool: null buffer");
    if (hidden_f32) return launch_embed_pool(p, static_cast<const float*>(hidden), seq_rows, norm_w, eps, pooling, normalize, out, dim, workspace, s);
    return launch_embed_pool(p, static_cast<const __half*>(hidden), seq_rows, norm_w, eps, pooling, normalize, out, dim, workspace, s);
}

}  // namespace fh
