// GPTQ-INT4 dequant-GEMM for gfx950: what the INT4 kernel translation units share — w4_skinny.hip (16-row supertile kernel
// and the in-launch routing prologues), w4_moe_em.hip (expert-major grouped GEMMs), w4_decode.hip (dense decode kernels
// and the dense dispatcher), w4_tiles.hip (64- to 256-row tiles).  Private to them: the runner (runner_*.hip) and the C-ABI layer (abi.cc, abi_gptq.cc) see kernels.h.
//
// Replaces, on the reference side: `GptqLinear::forward` → `B::load_gptq` + Marlin
// (ferrum-quantization/src/gptq.rs:42-112, ferrum-kernels/src/backend/cuda/marlin.rs:488-633)
// and `MarlinExpertStack::gemm_phase_vllm` (ferrum-kernels/src/marlin_expert_stack.rs:86).
// Arithmetic contract (cpu.rs:2283-2315): W[n,k] = (q − (z+1))·s[k/g, n].
//
// Design (HBM-bound at T ≤ 64):
//  * load-time repack GPTQ [K/8,N] → "w4t" tiles (w4_repack.cc): one wave-instruction (64 lanes × 16 B = 1 KiB,
//    fully coalesced) fetches a 16-column × 128-row (= one quant group) tile whose per-lane dwords
//    ARE the B-operand fragments of four v_mfma_f32_16x16x32_f16 k-steps.
//  * weights go HBM → VGPR directly (no LDS round trip: each weight byte is used once);
//    nibbles are expanded to exact fp16 integers with the 0x6400 magic-number trick at 5 VALU per
//    8 weights (the kernel is VALU-issue-bound, not HBM-bound, above that); the 1024/zero-point
//    offsets are removed by four extra MFMAs per group instead of per-weight subtracts, and the group
//    scale is applied to the fp32 MFMA chain result, so the only rounding is fp32 accumulation.
//  * activations are the A operand (rows = tokens, padded to 16); a wave owns a 64-column
//    "supertile" so every A fragment feeds four MFMAs.
//  * split-K writes fp32 slabs that a small epilogue kernel sums in fixed order (deterministic).
#pragma once
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "knobs.h"
#include "w4_device.h"
#include "w4_upload.h"

namespace fh {

struct W4Args {
    const uint32_t* qw;   // repacked weights (expert 0)
    const __half* sc;
    const __half* zp;     // null when symmetric
    long expert_stride_qw;   // dwords between experts (MoE), 0 for dense
    long expert_stride_sc;   // halves between experts
    const __half* x;      // activations [rows, K]
    __half* out;          // fp16 output [rows, ldo] (non-split, or fused-act)
    float* partial;       // fp32 slabs [S][rows_pad][n_pad] when split-K
    const __half* bias;   // optional [N] (wgsplit kernel)
    int M;                // rows (dense) / number of valid pair ids (MoE: T·k)
    int K, N, G, n64;
    int ldo;              // output row stride (elements)
    int S;                // K splits
    // MoE routing (null for dense)
    const int32_t* sorted_token_ids;
    const int32_t* block_ids;
    const int32_t* total_post_pad;
    int top_k;            // input row = id / top_k
    int few_pairs_per_expert;   // the caller's promise that no expert holds more than 16 of the pairs (≤ 16 tokens, distinct experts per token)
    int rows_pad;         // slab row count
    int n_pad;            // slab column count (= n64·64)
    // inline align (decode-sized batches): raw per-pair expert ids instead of the three arrays above
    const int32_t* pair_expert_ids;
    int num_experts;
    // when set, the inline align publishes its result so the NEXT grouped GEMM (down) can read it
    int32_t* pub_sorted_token_ids;
    int32_t* pub_block_ids;
    int32_t* pub_total_post_pad;
    // route merge (decode): Q sorted candidate lists per token from add_rmsnorm_route_part_kernel
    const RouteCand* cand;
    const float* stats;
    int route_T, route_Q, route_K, norm_topk;
    int32_t* pub_expert_ids;   // [T·K] merged ids  (published by one workgroup)
    float* pub_expert_w;       // [T·K] combine weights
    // fused prologue of the ≤ 4-row skinny GEMM (w4_gemm_wgsplit_kernel<…, FUSE_A>): the input rows are not read from `x` but
    // computed — MoE combine + residual add + RMSNorm of the PREVIOUS layer's tail (fused.hip kernel A)
    const __half* fa_down;     // [M·top_k, K] expert outputs
    const float* fa_weights;   // [M·top_k] combine weights
    const __half* fa_res_in;   // [M, K] residual before the add
    __half* fa_res_out;        // [M, K] residual after the add (≠ fa_res_in: every workgroup reads, one writes)
    const __half* fa_ln;       // [K] norm weights
    float fa_eps;
    int fa_top_k;
#ifdef FERRUM_HIP_EXPERIMENTS
    unsigned long long* tl;    // development: per-wave wall-clock stamps of the LDS-shared-activation kernel (tools/exp_timeline.py)
#endif
};
#ifdef FERRUM_HIP_EXPERIMENTS
// set by ferrum_hip_debug_set_timeline{,_mode} (w4_decode.hip)
extern unsigned long long* g_timeline;
extern int g_timeline_mode;          // expert-major grouped GEMM: 0 every launch, 1 down, 2 gate_up
#define FH_TL(i)                                                                                                        \
    do {                                                                                                                \
        if (p.tl && lane == 0)                                                                                          \
            p.tl[((((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 4 + (i)] = wall_clock64(); \
    } while (0)
#else
#define FH_TL(i) do {} while (0)
#endif

// sched_barrier(0) pins "issue next group" ABOVE "consume this group": without it hipcc sinks the
// loads below the MFMAs (to shorten live ranges) and every group pays its full HBM latency.
#define FH_PIN() __builtin_amdgcn_sched_barrier(0)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ───────────────────── launcher facts, each derived once (host) ─────────────────────

// distance between the experts of a stack: dwords of qw, halves of sc (and of zp)
inline long expert_stride_qw(const W4Device& w) { return (long)w4_qw_words(w.n64, w.G); }
inline long expert_stride_sc(const W4Device& w) { return (long)w4_sc_elems(w.n64, w.G); }

// 16-row tiles per wave of the skinny kernels
inline int skinny_row_tiles(int m) { return m <= 16 ? 1 : (m <= 32 ? 2 : 4); }

// dense y[M,N] = x[M,K]·Wᵀ: everything but the output (fp16 `out` + bias, or fp32 slabs) and the K split
inline W4Args dense_args(const W4Device& w, const __half* x, int m) {
    W4Args a{};
    a.qw = w.qw; a.sc = w.sc; a.zp = w.zp;
    a.x = x; a.M = m; a.K = w.k; a.N = w.n; a.G = w.G; a.n64 = w.n64; a.ldo = w.n; a.S = 1;
    return a;
}

// grouped GEMM over an expert stack (out row = pair id, in row = pair id / top_k): everything but the routing
inline W4Args moe_args(const W4Device& w, const __half* x, __half* out, int num_valid_pairs, int top_k, int fused_silu) {
    W4Args a{};
    a.qw = w.qw; a.sc = w.sc; a.zp = w.zp;
    a.expert_stride_qw = expert_stride_qw(w);
    a.expert_stride_sc = expert_stride_sc(w);
    a.x = x; a.out = out; a.M = num_valid_pairs; a.K = w.k; a.N = w.n; a.G = w.G; a.n64 = w.n64;
    a.ldo = fused_silu ? w.n / 2 : w.n;
    a.S = 1;
    a.top_k = top_k;
    return a;
}

// fp32 slab output [S][rows_pad][n64·64] of the w4_gemm_dense_slabs* entry points (their consumer kernels sum the slabs in order)
inline int slab_output(W4Args& a, int S, int rows_pad, float* slabs, size_t slab_bytes, const char* who, int* rows_pad_out, int* n_pad_out) {
    a.S = S; a.partial = slabs; a.rows_pad = rows_pad; a.n_pad = a.n64 * 64;
    FH_REQUIRE((size_t)S * a.rows_pad * a.n_pad * sizeof(float) <= slab_bytes, "%s: workspace too small", who);
    *rows_pad_out = a.rows_pad; *n_pad_out = a.n_pad;
    return 0;
}

// The HAS_ZP template argument of a launch from the weights' runtime flag: f(std::true_type) or f(std::false_type).
template <typename F>
inline void with_zp(bool has_zp, F&& f) {
    if (has_zp) f(std::true_type{});
    else f(std::false_type{});
}

// launchers that w4_gemm_dense (w4_decode.hip) reaches in w4_tiles.hip; the template switch stays with the kernels
int launch_big(const W4Args& a, int mt, int mode, bool has_zp, dim3 grid, hipStream_t stream);   // mt 6 / 8 / 16 (mode 0), 6 / 8 (modes 1, 2)
int launch_tilep(const W4Args& a, bool has_zp, dim3 grid, hipStream_t stream);

}  // namespace fh
