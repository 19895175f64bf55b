// The scoring head (gfx950): log-probabilities of given tokens from rows of fp32 logits — what ferrum_hip_model_score runs
// behind the lm_head GEMM in place of the sampling head; the OpenAI `logprobs` fields of the reference
// (ferrum-server/src/openai.rs) and an evaluation harness's loglikelihood are built on it.
//
//   partial launch  grid (segment, row): one 256-thread workgroup reads one segment of SCORE_SEGMENT = 4096 columns of one row
//                   into registers (16 values per lane: four 16-byte loads, issued together), takes the segment's maximum m and
//                   first argument (wave reduction by DPP, the four waves through LDS), then s = Σ exp(x − m) over what it
//                   holds, and writes (m, s, first argument) to the workspace.  The row is read once; one exp per element.
//   merge launch    one wave per row: M = max m_p, first maximum under "larger value, then smaller index",
//                   S = Σ_p s_p · exp(m_p − M) — lane l adds segments l, l + 64, … in that order, then the fixed wave tree —
//                   lse = M + log S
//   gather launch   one thread per pair: x[row][token] − lse[row]
//
// Determinism: no atomics; lane l of a workgroup holds columns seg·4096 + (k·256 + l)·4 + j whatever the row's address, so
// which values a lane adds, in which order, depends on n and the column alone; the reductions are fixed trees.  A row's lse,
// top and log-probs are the same bit for bit from run to run, whatever m is and whichever other rows the launch holds.
// Loads are 16 bytes wide at 4-byte alignment (a row starts wherever row·ld puts it; global memory needs no more for a
// four-dword load); only the four columns that straddle n are read one by one.
// Special values: −inf contributes 0; a row with nothing above −inf has lse = −inf, top = 0 and NaN log-probs; a NaN anywhere
// in a row reaches its lse through the sum (the maximum, taken with `>`, never sees it), so lse and every log-prob of the row
// are NaN.  expf / logf, not the fast forms: the tests' error bound rests on their accuracy.
#include "common.h"
#include "kernels.h"
#include "score_plan.h"

namespace fh {
namespace {

typedef float float4u __attribute__((ext_vector_type(4), aligned(4)));

// (value, index) under the total order "larger value, then smaller index": exact whatever the pairing
__device__ __forceinline__ void first_max(float& best, int& idx, float ov, int oi) {
    if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
}
template <int CTRL>
__device__ __forceinline__ void first_max_dpp(float& best, int& idx) {
    const float ov = dpp_move<CTRL>(best);
    const int oi = __builtin_amdgcn_update_dpp(0, idx, CTRL, 0xF, 0xF, true);
    first_max(best, idx, ov, oi);
}
__device__ __forceinline__ void first_max_swap(float& best, int& idx, bool half) {
    const unsigned b = __float_as_uint(best), i = (unsigned)idx;
    const auto rv = half ? __builtin_amdgcn_permlane32_swap(b, b, false, false) : __builtin_amdgcn_permlane16_swap(b, b, false, false);
    const auto ri = half ? __builtin_amdgcn_permlane32_swap(i, i, false, false) : __builtin_amdgcn_permlane16_swap(i, i, false, false);
    best = __uint_as_float(rv[0]);
    idx = (int)ri[0];
    first_max(best, idx, __uint_as_float(rv[1]), (int)ri[1]);
}
// every lane gets the wave's (maximum, first argument)
__device__ __forceinline__ void wave_first_max(float& best, int& idx) {
    first_max_dpp<0xB1>(best, idx);
    first_max_dpp<0x4E>(best, idx);
    first_max_dpp<0x141>(best, idx);
    first_max_dpp<0x140>(best, idx);
    first_max_swap(best, idx, false);
    first_max_swap(best, idx, true);
}

constexpr int NO_INDEX = 0x7fffffff;
constexpr int SCORE_VECS = SCORE_SEGMENT / (SCORE_BLOCK * 4);       // 16-byte loads per lane

__global__ __launch_bounds__(SCORE_BLOCK) void score_partial_kernel(const float* __restrict__ logits, long ld, int n,
                                                                    float* __restrict__ pmax, float* __restrict__ psum,
                                                                    int* __restrict__ pidx) {
    __shared__ float s_max[4], s_sum[4];
    __shared__ int s_idx[4];
    const int seg = blockIdx.x, segments = gridDim.x;
    const long row = blockIdx.y;
    const float* p = logits + row * ld;
    float v[SCORE_VECS][4];
#pragma unroll
    for (int k = 0; k < SCORE_VECS; k++) {
        const long c0 = (long)seg * SCORE_SEGMENT + (k * SCORE_BLOCK + threadIdx.x) * 4;
        if (c0 + 4 <= n) {
            const float4u x = *reinterpret_cast<const float4u*>(p + c0);
#pragma unroll
            for (int j = 0; j < 4; j++) v[k][j] = x[j];
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) v[k][j] = c0 + j < n ? p[c0 + j] : -INFINITY;       // past n: contributes nothing
        }
    }
    float best = -INFINITY;
    int idx = NO_INDEX;
#pragma unroll
    for (int k = 0; k < SCORE_VECS; k++)
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (v[k][j] > best) { best = v[k][j]; idx = seg * SCORE_SEGMENT + (k * SCORE_BLOCK + threadIdx.x) * 4 + j; }     // ascending: the first stays
    wave_first_max(best, idx);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { s_max[wave] = best; s_idx[wave] = idx; }
    __syncthreads();
    best = s_max[0];
    idx = s_idx[0];
#pragma unroll
    for (int w = 1; w < 4; w++) first_max(best, idx, s_max[w], s_idx[w]);
    // x == −inf is tested, not left to exp: with a segment maximum of −inf the difference would be NaN.  A NaN x stays one.
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < SCORE_VECS; k++)
#pragma unroll
        for (int j = 0; j < 4; j++) sum += v[k][j] == -INFINITY ? 0.f : expf(v[k][j] - best);
    sum = wave_reduce_sum(sum);
    if (lane == 0) s_sum[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const long slot = row * segments + seg;
        pmax[slot] = best;
        psum[slot] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        pidx[slot] = idx;
    }
}

__global__ __launch_bounds__(64) void score_merge_kernel(const float* __restrict__ pmax, const float* __restrict__ psum,
                                                         const int* __restrict__ pidx, int segments, float* __restrict__ lse_ws,
                                                         float* __restrict__ row_lse, uint32_t* __restrict__ row_top,
                                                         float* __restrict__ row_top_logprob) {
    const long row = blockIdx.x;
    const float* rm = pmax + row * segments;
    const float* rs = psum + row * segments;
    const int* ri = pidx + row * segments;
    float best = -INFINITY;
    int idx = NO_INDEX;
    for (int c = threadIdx.x; c < segments; c += 64) first_max(best, idx, rm[c], ri[c]);
    wave_first_max(best, idx);
    float sum = 0.f;
    for (int c = threadIdx.x; c < segments; c += 64) {
        const float mp = rm[c], sp = rs[c];
        sum += mp == -INFINITY ? sp : sp * expf(mp - best);      // (an all −inf segment holds 0, or the NaN it met)
    }
    sum = wave_reduce_sum(sum);
    if (threadIdx.x == 0) {
        const float lse = best + logf(sum);                      // nothing above −inf: −inf + log 0 = −inf
        lse_ws[row] = lse;
        if (row_lse) row_lse[row] = lse;
        if (row_top) row_top[row] = idx == NO_INDEX ? 0u : (uint32_t)idx;
        if (row_top_logprob) row_top_logprob[row] = best - lse;
    }
}

__global__ __launch_bounds__(SCORE_BLOCK) void score_gather_kernel(const float* __restrict__ logits, long ld, int n,
                                                                   const int32_t* __restrict__ pair_rows,
                                                                   const uint32_t* __restrict__ pair_tokens, int num_pairs,
                                                                   const float* __restrict__ lse_ws, float* __restrict__ out) {
    const int p = blockIdx.x * SCORE_BLOCK + threadIdx.x;
    if (p >= num_pairs) return;
    const long row = pair_rows[p];
    const uint32_t tok = pair_tokens[p];
    out[p] = tok < (uint32_t)n ? logits[row * ld + tok] - lse_ws[row] : -INFINITY;
}

}  // namespace

int logprob_rows_f32(const float* logits, int ld, int m, int n, const int32_t* pair_rows, const uint32_t* pair_tokens, int num_pairs,
                     float* pair_logprob, float* row_lse, uint32_t* row_top, float* row_top_logprob, float* workspace,
                     size_t workspace_bytes, hipStream_t s) {
    ScorePlan p;
    char why[256];
    if (score_plan(ScoreShape{m, n, ld, num_pairs}, workspace ? workspace_bytes : 0, &p, why, sizeof(why))) {
        fh::set_error("%s", why);
        return 2;
    }
    if (m == 0) return 0;
    FH_REQUIRE(logits, "logprob_rows: null logits");
    FH_REQUIRE(num_pairs == 0 || (pair_rows && pair_tokens && pair_logprob), "logprob_rows: null pair buffer");
    float* pmax = workspace;
    float* psum = workspace + p.off_sum;
    int* pidx = reinterpret_cast<int*>(workspace + p.off_idx);
    float* lse_ws = workspace + p.off_lse;
    hipLaunchKernelGGL(score_partial_kernel, dim3(p.partial_grid_x, p.partial_grid_y), dim3(p.block), 0, s, logits, (long)ld, n, pmax, psum, pidx);
    FH_CHECK_LAUNCH();
    hipLaunchKernelGGL(score_merge_kernel, dim3(p.merge_grid_x), dim3(64), 0, s, pmax, psum, pidx, p.segments, lse_ws, row_lse, row_top,
                       row_top_logprob);
    FH_CHECK_LAUNCH();
    if (p.gather_grid_x) {
        hipLaunchKernelGGL(score_gather_kernel, dim3(p.gather_grid_x), dim3(p.block), 0, s, logits, (long)ld, n, pair_rows, pair_tokens, num_pairs,
                           lse_ws, pair_logprob);
        FH_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace fh
