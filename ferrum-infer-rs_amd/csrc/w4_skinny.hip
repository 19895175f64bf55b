// INT4 GEMM, 16-row supertile kernel (w4_gemm_kernel): the block-major MoE grouped GEMM with its in-launch routing prologues
// (candidate merge, align) and the dense fp32-slab form.  Layout and arithmetic: w4_gemm.h.
#include "w4_gemm.h"
#include "route_merge.h"

namespace fh {

// Merge the Q per-part candidate lists of every token (each sorted by logit desc, id asc) into the token's
// top-K, in the same order route_into picks them (ferrum-models/src/moe/router.rs:159-178: descending
// probability, ties → lower expert id), and derive the combine weights (softmax over all experts from the
// parts' (max, Σexp) statistics, optional renormalisation over the K picked — router.rs:141-157,180-193).
// One wave; lane t ↔ token t (T ≤ 64).  Results: s_ids[t·K+k] in LDS; one workgroup also publishes them.
__device__ __forceinline__ void merge_route_candidates(const RouteCand* __restrict__ cand, const float* __restrict__ stats,
                                                       int T, int Q, int K, int norm_topk, RouteCand* s_cand, int* s_ids,
                                                       bool publish, int32_t* pub_ids, float* pub_w) {
    const int lane = threadIdx.x & 63;
    const int n = T * Q * 8;
    for (int i = lane; i < n; i += 64) s_cand[i] = cand[i];
    __syncthreads();
    if (lane < T) {
        const int t = lane;
        float M = -INFINITY;
        for (int q = 0; q < Q; q++) M = fmaxf(M, stats[(t * Q + q) * 2]);
        float S = 0.f;
        for (int q = 0; q < Q; q++) S += stats[(t * Q + q) * 2 + 1] * expf(stats[(t * Q + q) * 2] - M);
        const float inv_sum = 1.0f / S;
        uint32_t heads = 0;                         // 4 bits per part: next unread candidate
        float pk[8];
        int idk[8];
        float sel_sum = 0.f;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            pk[k] = 0.f;
            idk[k] = 0;
            if (k < K) {
                float best_l = -INFINITY;
                int best_id = 0x7fffffff, best_q = 0;
                for (int q = 0; q < Q; q++) {
                    const int h = (heads >> (4 * q)) & 15;
                    if (h < 8) {
                        const RouteCand c = s_cand[(t * Q + q) * 8 + h];
                        if (c.logit > best_l || (c.logit == best_l && c.id < best_id)) { best_l = c.logit; best_id = c.id; best_q = q; }
                    }
                }
                heads += 1u << (4 * best_q);
                if (best_id == 0x7fffffff) best_id = 0;
                const float p = expf(best_l - M) * inv_sum;
                pk[k] = p;
                idk[k] = best_id;
                sel_sum += p;
                s_ids[t * K + k] = best_id;
            }
        }
        if (publish) {
            const float scale = norm_topk ? (sel_sum > 0.f ? 1.0f / sel_sum : 0.f) : 1.0f;
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (k < K) {
                    pub_ids[t * K + k] = idk[k];
                    pub_w[t * K + k] = (norm_topk && !(sel_sum > 0.f)) ? 1.0f / (float)K : pk[k] * scale;
                }
        }
    }
    __syncthreads();
}

// The same merge for a handful of tokens (T ≤ 8: decode at c ≤ 8), lane-parallel and without LDS staging: the lists of all
// tokens are requested at once (one 8-byte load per lane and token pair), every pair of tokens then takes route_merge_pair's
// 4-probe searches — short enough to sit in the prologue of every workgroup of the gate_up launch (role B of the decode chain
// then stops at the lists: chain.hip, defer_merge).  Only the publishing workgroup derives the combine weights.  One wave;
// results in s_ids[t·K + k].  Q ∈ {1, 2, 4}.
__device__ __forceinline__ void merge_route_lists_fast(const RouteCand* __restrict__ cand, const float* __restrict__ stats, int T,
                                                       int Q, int K, int norm_topk, int* s_ids, bool publish, int32_t* pub_ids,
                                                       float* pub_w) {
    const int lane = threadIdx.x & 63;
    const int half = lane >> 5, li = lane & 31, ncand = Q * 8;
    const unsigned long long* cg = reinterpret_cast<const unsigned long long*>(cand);
    const unsigned long long none = (0x7fffffffull << 32) | 0xff800000ull;
    unsigned long long c[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int t = 2 * r + half;
        c[r] = (t < T && li < ncand) ? cg[t * ncand + li] : none;           // RouteCand {logit, id}: low word logit, high word id
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (2 * r < T) {
            const int t = 2 * r + half;
            const bool valid = t < T && li < ncand;
            int id;
            const int rank = route_merge_pair(c[r], Q, &id);
            if (id == 0x7fffffff) id = 0;                                     // (fewer than K experts in all: as merge_route_candidates)
            const bool keep = valid && rank < K;
            if (keep) s_ids[t * K + rank] = id;
            if (publish) {
                const float ww = route_merge_pair_weight(c[r], rank, valid, stats + (long)(t < T ? t : 0) * Q * 2, Q, K, norm_topk);
                if (keep) { pub_ids[t * K + rank] = id; pub_w[t * K + rank] = ww; }
            }
        }
    }
    __syncthreads();
}

// Align-block-size computed INSIDE the grouped GEMM (P ≤ 1024 pairs) from the per-pair expert ids staged in
// LDS: LDS histogram, wave scan of the padded counts, ballot compaction — identical result to
// moe_align_block_size (ascending pair id inside an expert) without the separate ≈8 µs launch.
// One wave per workgroup.
__device__ __forceinline__ bool inline_align_block(const int* s_ids, int P, int E, int rb, int* s_cnt, int* s_rows,
                                                   int* expert_out, int* total_blocks_out) {
    const int lane = threadIdx.x & 63;
    for (int i = lane; i < E; i += 64) s_cnt[i] = 0;
    if (lane < 16) s_rows[lane] = P;      // sentinel
    __syncthreads();
    for (int p = lane; p < P; p += 64) {
        int e = s_ids[p];
        if (e >= 0 && e < E) atomicAdd(&s_cnt[e], 1);
    }
    __syncthreads();
    // lane owns experts [8·lane, 8·lane+8): blocks per expert, then an exclusive wave scan
    int nb[8], local = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        int e = lane * 8 + i;
        nb[i] = e < E ? (s_cnt[e] + 15) >> 4 : 0;
        local += nb[i];
    }
    int incl = local;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        int t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    const int total = __shfl(incl, 63, 64);
    *total_blocks_out = total;
    if (rb >= total) return false;
    const int excl = incl - local;
    int found = -1;          // (expert << 16) | block-within-expert, on the owning lane
    if (rb >= excl && rb < incl) {
        int base = excl;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (rb >= base && rb < base + nb[i]) found = ((lane * 8 + i) << 16) | (rb - base);
            base += nb[i];
        }
    }
    const unsigned long long owner = __ballot(found >= 0);
    found = __shfl(found, __ffsll((long long)owner) - 1, 64);
    const int e_star = found >> 16, j = found & 0xffff;
    int base = 0;
    for (int p0 = 0; p0 < P; p0 += 64) {
        int p = p0 + lane;
        bool mine = p < P && s_ids[p] == e_star;
        unsigned long long bal = __ballot(mine);
        int r = base + __popcll(bal & ((1ull << lane) - 1ull));
        if (mine && (r >> 4) == j) s_rows[r & 15] = p;
        base += __popcll(bal);
    }
    __syncthreads();
    *expert_out = e_star;
    return true;
}

// The align for a few tokens (P ≤ 128 pairs, E ≤ 128 experts, every expert at most once per token and T ≤ 16 tokens — so one
// 16-row block per active expert): no histogram, no scan.  The active experts are two 64-bit words of presence bits; block rb
// is the rb-th set bit; its rows are the pairs holding that expert, compacted in ascending pair order — the arrays
// moe_align_block_size would produce.  One wave, two pairs per lane; ≈ 0.3 µs instead of inline_align_block's ≈ 1.5.
__device__ __forceinline__ bool align_block_few_pairs(const int* s_ids, int P, int rb, unsigned* s_bits, int* s_rows, int* expert_out,
                                                      int* total_blocks_out) {
    const int lane = threadIdx.x & 63;
    if (lane < 4) s_bits[lane] = 0u;
    if (lane < 16) s_rows[lane] = P;      // sentinel
    __syncthreads();
    const int e0 = lane < P ? s_ids[lane] : -1, e1 = 64 + lane < P ? s_ids[64 + lane] : -1;
    if (e0 >= 0 && e0 < 128) atomicOr(&s_bits[e0 >> 5], 1u << (e0 & 31));
    if (e1 >= 0 && e1 < 128) atomicOr(&s_bits[e1 >> 5], 1u << (e1 & 31));
    __syncthreads();
    const unsigned long long lo = ((unsigned long long)s_bits[1] << 32) | s_bits[0], hi = ((unsigned long long)s_bits[3] << 32) | s_bits[2];
    const int n_lo = __popcll(lo), total = n_lo + __popcll(hi);
    *total_blocks_out = total;
    if (rb >= total) return false;
    // lane l ↔ bit l of the word that holds the rb-th set bit
    const unsigned long long w = rb < n_lo ? lo : hi;
    const int want = rb < n_lo ? rb : rb - n_lo;
    const bool hit = ((w >> lane) & 1ull) && __popcll(w & ((1ull << lane) - 1ull)) == want;
    const int e_star = (__ffsll((long long)__ballot(hit)) - 1) + (rb < n_lo ? 0 : 64);
    const bool m0 = e0 == e_star, m1 = e1 == e_star;
    const unsigned long long b0 = __ballot(m0), b1 = __ballot(m1);
    if (m0) s_rows[__popcll(b0 & ((1ull << lane) - 1ull)) & 15] = lane;
    if (m1) s_rows[(__popcll(b0) + __popcll(b1 & ((1ull << lane) - 1ull))) & 15] = 64 + lane;
    __syncthreads();
    *expert_out = e_star;
    return true;
}

// MODE: 0 dense, 1 MoE (plain output), 2 MoE gate_up with fused silu·mul epilogue
// KW (MoE only): waves per workgroup that split K.  Small batches (≤ 64 pairs) launch too few one-wave workgroups to
// cover the chip and each streams its 64 KiB at one group per memory round trip; with KW = 4 every wave takes a quarter
// of K (all its groups in flight) and the partial sums meet in LDS — c=1 gate_up 11.8 → ≈6 µs.  Each wave runs the
// (cheap) routing prologue on its own LDS slice, so no cross-wave protocol is needed before the reduce.
// RT (MoE only): the routing prologue (candidate merge / align) runs inside the launch and owns ≈ 12 KiB of LDS per
// workgroup; with explicit align arrays (RT = false) no LDS is allocated, so 25 one-wave workgroups per CU stay resident
// instead of 13 (prefill-side batches of a few hundred tokens launch ≈ 6500 of them).
template <int MT, bool HAS_ZP, int MODE, int KW = 1, bool RT = true>
__global__ __launch_bounds__(MODE == 0 ? 256 : 64 * KW) void w4_gemm_kernel(W4Args p) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int a = lane >> 4, b = lane & 15;
    // dense: 4 waves per workgroup, one 64-column supertile each.  MoE: ONE wave per workgroup — the
    // grouped GEMM is bound by the per-CU fetch rate (≈10 B/clk/CU), so its time is the byte count of the
    // most loaded CU; wave-granular workgroups balance 64-KiB streams over the 256 CUs to ±1.
    const int st = MODE == 0 ? blockIdx.x * 4 + wave : blockIdx.x;
    if (st >= p.n64) return;
    const int rb = blockIdx.y;                     // row block (16·MT rows)
    const int z = blockIdx.z;                      // K split

    const uint32_t* qw = p.qw;
    const __half* sc = p.sc;
    const __half* zp = p.zp;
    int row_in[MT], row_out[MT];
    bool row_ok[MT];
    if (MODE == 0) {
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            int r = rb * 16 * MT + mt * 16 + b;
            row_ok[mt] = r < p.M;
            row_in[mt] = row_ok[mt] ? r : p.M - 1;
            row_out[mt] = r;
        }
    } else {
        // MoE: one 16-row block of sorted pair ids, all of one expert.
        // LDS: raw[0..8K) holds the route candidates during the merge, then (first 2 KB) the histogram
        int e, id;
        if constexpr (RT) {
            __shared__ __attribute__((aligned(16))) unsigned char s_raw_all[KW][KW == 1 ? 8192 : 2048];
            __shared__ int s_ids_all[KW][KW == 1 ? 1024 : 64], s_rows_all[KW][16];
            unsigned char* s_raw = s_raw_all[KW == 1 ? 0 : wave];
            int* s_ids = s_ids_all[KW == 1 ? 0 : wave];
            int* s_rows = s_rows_all[KW == 1 ? 0 : wave];
            int* s_cnt = reinterpret_cast<int*>(s_raw);
            const bool publisher = blockIdx.x == 0 && rb == 0 && wave == 0;
            if (p.cand && p.route_T <= 8 && (p.route_Q == 1 || p.route_Q == 2 || p.route_Q == 4)) {
                merge_route_lists_fast(p.cand, p.stats, p.route_T, p.route_Q, p.route_K, p.norm_topk, s_ids, publisher,
                                       p.pub_expert_ids, p.pub_expert_w);
            } else if (p.cand) {      // (KW = 4: every wave merges on its own slice — ≤ 256 candidates, ≤ 64 pairs; launch_w4 checks)
                merge_route_candidates(p.cand, p.stats, p.route_T, p.route_Q, p.route_K, p.norm_topk,
                                       reinterpret_cast<RouteCand*>(s_raw), s_ids, publisher, p.pub_expert_ids, p.pub_expert_w);
            } else {
                for (int i = lane; i < p.M; i += 64) s_ids[i] = p.pair_expert_ids[i];
                __syncthreads();
            }
            int total_blocks;
            if (((p.cand && p.route_T <= 8) || p.few_pairs_per_expert) && p.M <= (KW == 1 ? 128 : 64) && p.num_experts <= 128) {
                if (!align_block_few_pairs(s_ids, p.M, rb, reinterpret_cast<unsigned*>(s_cnt), s_rows, &e, &total_blocks)) return;
            } else if (!inline_align_block(s_ids, p.M, p.num_experts, rb, s_cnt, s_rows, &e, &total_blocks)) return;
            id = s_rows[b];
            if (p.pub_sorted_token_ids && blockIdx.x == 0 && wave == 0) {
                if (threadIdx.x < 16) p.pub_sorted_token_ids[rb * 16 + threadIdx.x] = s_rows[threadIdx.x];
                if (threadIdx.x == 0) {
                    p.pub_block_ids[rb] = e;
                    if (rb == 0) *p.pub_total_post_pad = total_blocks * 16;
                }
            }
        } else {
            const int total = *p.total_post_pad;
            if (rb * 16 >= total) return;
            e = p.block_ids[rb];
            id = p.sorted_token_ids[rb * 16 + b];
        }
        qw += (long)e * p.expert_stride_qw;
        sc += (long)e * p.expert_stride_sc;
        if (HAS_ZP) zp += (long)e * p.expert_stride_sc;
        row_ok[0] = id < p.M;
        row_out[0] = id;
        row_in[0] = row_ok[0] ? id / p.top_k : 0;
    }

    int g0 = (int)((long)p.G * z / p.S), g1 = (int)((long)p.G * (z + 1) / p.S);
    if (MODE != 0 && KW > 1) {   // this wave's quarter of K
        const int span = g1 - g0, base = g0;
        g0 = base + span * wave / KW;
        g1 = base + span * (wave + 1) / KW;
    }
    // per-lane bases
    const u32x4* qw_lane = reinterpret_cast<const u32x4*>(qw) + ((long)st * p.G * 4) * 64 + lane;
    const uint2* sc_lane = reinterpret_cast<const uint2*>(sc) + ((long)st * p.G) * 16 + b;
    const uint2* zp_lane = HAS_ZP ? reinterpret_cast<const uint2*>(zp) + ((long)st * p.G) * 16 + b : nullptr;
    const __half* xrow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) xrow[mt] = p.x + (long)row_in[mt] * p.K + 8 * a;

    float4v acc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < 4; nt++) acc[mt][nt] = (float4v){0.f, 0.f, 0.f, 0.f};

    // register double buffer: group g+1 is in flight while group g is consumed
    u32x4 wq[2][4];
    uint2 scv[2], zpv[2];
    half8 af[2][MT][4];
    auto issue = [&](int buf, int g) {
#pragma unroll
        for (int nt = 0; nt < 4; nt++) wq[buf][nt] = __builtin_nontemporal_load(qw_lane + ((long)g * 4 + nt) * 64);
        scv[buf] = sc_lane[(long)g * 16];
        if (HAS_ZP) zpv[buf] = zp_lane[(long)g * 16];
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int s = 0; s < 4; s++)
                af[buf][mt][s] = *reinterpret_cast<const half8*>(xrow[mt] + g * 128 + 32 * s);
    };
    auto consume = [&](int buf) {
        const unsigned long long sb = ((unsigned long long)scv[buf].y << 32) | scv[buf].x;
        const unsigned long long zb = HAS_ZP ? (((unsigned long long)zpv[buf].y << 32) | zpv[buf].x) : 0ull;
        w4_consume_group<MT, 4, HAS_ZP>(wq[buf], sb, zb, 0, af[buf], acc);
    };

    if (g0 < g1) {
        issue(0, g0);
        FH_PIN();
        int g = g0;
        for (; g + 2 <= g1 - 1; g += 2) {   // two groups per trip keeps buffer indices static
            issue(1, g + 1);
            FH_PIN();
            consume(0);
            FH_PIN();
            issue(0, g + 2);
            FH_PIN();
            consume(1);
            FH_PIN();
        }
        if (g + 1 < g1) {
            issue(1, g + 1);
            FH_PIN();
            consume(0);
            consume(1);
        } else {
            consume(0);
        }
    }
    if (MODE != 0 && KW > 1) {
        // partial sums of the KW K-quarters meet in LDS; wave 0 adds them in wave order and owns the epilogue
        __shared__ float kred[KW][16][64];
#pragma unroll
        for (int nt = 0; nt < 4; nt++)
#pragma unroll
            for (int r = 0; r < 4; r++) kred[wave][nt * 4 + r][lane] = acc[0][nt][r];
        __syncthreads();
        if (wave != 0) return;
#pragma unroll
        for (int nt = 0; nt < 4; nt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float s = kred[0][nt * 4 + r][lane];
#pragma unroll
                for (int k = 1; k < KW; k++) s += kred[k][nt * 4 + r][lane];
                acc[0][nt][r] = s;
            }
    }

    // accumulator map (v_mfma_f32_16x16x32): column = lane&15 → n, row = 4·(lane>>4)+r → token.
    // Lanes exchange nothing: every lane owns token rows 4a..4a+3 of column b.  The A operand
    // was loaded with lane b ↔ token b, so token t = 4a'+r lives in lanes with (lane>>4)==a'.
    // (D row index is the A row index, i.e. the token slot 0..15 of this block.)
    int out_rows[MT][4];
    bool out_ok[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            // the token slot 4a+r's routing lives in lane (·, b=4a+r): fetch it by shuffle
            int src_lane = 4 * a + r;
            out_rows[mt][r] = __shfl(row_out[mt], src_lane, 64);
            out_ok[mt][r] = __shfl((int)row_ok[mt], src_lane, 64) != 0;
        }

    if (MODE == 2) {
        // supertile = [16 gate | 16 gate | 16 up | 16 up] (column-permuted at repack):
        // act[row][st·32 + j·16 + b] = silu(gate)·up   (cpu.rs:1666-1680)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (!out_ok[0][r]) continue;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                float gt = acc[0][j][r], up = acc[0][2 + j][r];
                float v = (gt / (1.0f + __expf(-gt))) * up;
                int col = st * 32 + j * 16 + b;
                if (col < p.ldo) p.out[(long)out_rows[0][r] * p.ldo + col] = __float2half(v);
            }
        }
        return;
    }
    if (p.S > 1 || (MODE == 0 && p.partial)) {
        float* slab = p.partial + (long)z * p.rows_pad * p.n_pad;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                int row = MODE == 0 ? rb * 16 * MT + mt * 16 + 4 * a + r : rb * 16 + 4 * a + r;
#pragma unroll
                for (int nt = 0; nt < 4; nt++)
                    slab[(long)row * p.n_pad + st * 64 + nt * 16 + b] = acc[mt][nt][r];
            }
        return;
    }
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (!out_ok[mt][r]) continue;
#pragma unroll
            for (int nt = 0; nt < 4; nt++) {
                int col = st * 64 + nt * 16 + b;
                if (col < p.N) p.out[(long)out_rows[mt][r] * p.ldo + col] = __float2half(acc[mt][nt][r]);
            }
        }
}

// ─────────────────────────────── host launchers ────────────────────────────

template <int MODE>
static int launch_w4(const W4Args& a, int mt, bool has_zp, dim3 grid, hipStream_t stream) {
#define FH_W4_CASE(MTV) hipLaunchKernelGGL((w4_gemm_kernel<MTV, ZP, MODE>), grid, dim3(256), 0, stream, a)
    if constexpr (MODE != 0) {
        // few pairs (decode at c ≤ 8): 4 waves per workgroup split K (see KW)
        // default 16 pairs, measured on Qwen3-30B-A3B: c=1 + 10 %, c=2 + 5.5 % (756 → 798 tok/s), c=3 ±0, c=4 − 2.7 %, c=8 − 6.5 %.
        // Never beyond 64 pairs: the K-split form keeps its per-wave pair list in 64 LDS slots.
        const int kw_pairs = std::min(knobs().moe_kw_pairs, 64);
        const bool rt = a.cand != nullptr || a.pair_expert_ids != nullptr;      // routing prologue inside the launch (owns LDS)
        const bool kw4 = a.M <= kw_pairs && (a.cand == nullptr || a.route_T * a.route_Q * 8 <= 256) && a.G >= 4;
#define FH_W4_MOE(KWV, RTV) hipLaunchKernelGGL((w4_gemm_kernel<1, ZP, MODE, KWV, RTV>), grid, dim3(64 * KWV), 0, stream, a)
        with_zp(has_zp, [&](auto zp) {
            constexpr bool ZP = decltype(zp)::value;
            if (kw4) { if (rt) FH_W4_MOE(4, true); else FH_W4_MOE(4, false); }
            else { if (rt) FH_W4_MOE(1, true); else FH_W4_MOE(1, false); }
        });
#undef FH_W4_MOE
    } else {
        with_zp(has_zp, [&](auto zp) {
            constexpr bool ZP = decltype(zp)::value;
            if (mt == 1) FH_W4_CASE(1);
            else if (mt == 2) FH_W4_CASE(2);
            else FH_W4_CASE(4);
        });
    }
#undef FH_W4_CASE
    FH_CHECK_LAUNCH();
    return 0;
}

// MoE grouped GEMM over align-block routing arrays (block size 16).
// out row = pair id, in row = pair id / top_k (vLLM marlin_moe convention, ops.cu:942).
int w4_gemm_moe_inline_align(const W4Device& w, const __half* x, __half* out, const int32_t* pair_expert_ids,
                             int num_experts, int num_valid_pairs, int max_blocks, int top_k, int fused_silu,
                             int32_t* pub_sorted, int32_t* pub_block_ids, int32_t* pub_total, hipStream_t stream,
                             bool few_pairs_per_expert) {
    if (num_valid_pairs <= 0 || max_blocks <= 0) return 0;
    FH_REQUIRE(num_valid_pairs <= 1024 && num_experts <= 512, "inline align: pairs=%d experts=%d out of range", num_valid_pairs, num_experts);
    W4Args a = moe_args(w, x, out, num_valid_pairs, top_k, fused_silu);
    a.pair_expert_ids = pair_expert_ids; a.num_experts = num_experts;
    a.pub_sorted_token_ids = pub_sorted; a.pub_block_ids = pub_block_ids; a.pub_total_post_pad = pub_total;
    a.few_pairs_per_expert = few_pairs_per_expert ? 1 : 0;
    dim3 grid(w.n64, max_blocks, 1);
    form_hit(FORM_MOE_INLINE_ALIGN);
    if (fused_silu) return launch_w4<2>(a, 1, w.zp != nullptr, grid, stream);
    return launch_w4<1>(a, 1, w.zp != nullptr, grid, stream);
}

// gate_up phase of a decode step: routing is taken from the Q candidate lists written by
// fused_add_rms_norm_route_parts_f16; the merged ids / weights and the align arrays are published.
int w4_gemm_moe_merge_route(const W4Device& w, const __half* x, __half* out, const RouteCand* cand, const float* stats,
                            int tokens, int Q, int top_k, int norm_topk, int num_experts, int max_blocks, int fused_silu,
                            int32_t* pub_expert_ids, float* pub_expert_w, int32_t* pub_sorted, int32_t* pub_block_ids,
                            int32_t* pub_total, hipStream_t stream) {
    if (tokens <= 0 || max_blocks <= 0) return 0;
    FH_REQUIRE(tokens <= 64 && tokens * Q <= 128 && tokens * top_k <= 1024 && top_k <= 8 && num_experts <= 512,
               "merge_route: tokens=%d Q=%d top_k=%d experts=%d out of range", tokens, Q, top_k, num_experts);
    W4Args a = moe_args(w, x, out, tokens * top_k, top_k, fused_silu);
    a.num_experts = num_experts;
    a.cand = cand; a.stats = stats; a.route_T = tokens; a.route_Q = Q; a.route_K = top_k; a.norm_topk = norm_topk;
    a.pub_expert_ids = pub_expert_ids; a.pub_expert_w = pub_expert_w;
    a.pub_sorted_token_ids = pub_sorted; a.pub_block_ids = pub_block_ids; a.pub_total_post_pad = pub_total;
    dim3 grid(w.n64, max_blocks, 1);
    form_hit(FORM_MOE_MERGE_ROUTE);
    if (fused_silu) return launch_w4<2>(a, 1, w.zp != nullptr, grid, stream);
    return launch_w4<1>(a, 1, w.zp != nullptr, grid, stream);
}

// Dense projection as S fp32 split-K slabs [S][rows_pad][n_pad] (no reduction here: the consumer kernel sums
// them in slab order).  Used where the consumer is a fused kernel anyway (o_proj → add+norm+route).
int w4_gemm_dense_slabs(const W4Device& w, const __half* x, float* slabs, size_t slab_bytes, int m, int S,
                        int* rows_pad_out, int* n_pad_out, hipStream_t stream) {
    if (m <= 0) return 0;
    // (act-order weights: the caller hands over rows its producer already wrote in the packed-row order, like w4_gemm_dense)
    FH_REQUIRE(w.bias == nullptr, "w4_gemm_dense_slabs: bias weights use the direct path");
    W4Args a = dense_args(w, x, m);
    const int mt = skinny_row_tiles(m);
    const int row_blocks = cdiv(m, 16 * mt);
    S = std::max(1, std::min(S, w.G));
    if (int rc = slab_output(a, S, row_blocks * 16 * mt, slabs, slab_bytes, "w4_gemm_dense_slabs", rows_pad_out, n_pad_out)) return rc;
    // S == 1 still writes a slab (the MODE-0 kernel writes fp16 `out` only when S == 1 → force the slab path)
    form_hit(FORM_W4_SLABS);
    return launch_w4<0>(a, mt, w.zp != nullptr, dim3(cdiv(w.n64, 4), row_blocks, S), stream);
}

int w4_gemm_moe(const W4Device& w, const __half* x, __half* out, const int32_t* sorted_token_ids,
                const int32_t* block_ids, const int32_t* total_post_pad, int num_valid_pairs, int max_blocks,
                int top_k, int fused_silu, hipStream_t stream) {
    if (num_valid_pairs <= 0 || max_blocks <= 0) return 0;
    W4Args a = moe_args(w, x, out, num_valid_pairs, top_k, fused_silu);
    a.sorted_token_ids = sorted_token_ids; a.block_ids = block_ids; a.total_post_pad = total_post_pad;
    dim3 grid(w.n64, max_blocks, 1);
    form_hit(FORM_MOE_BLOCK16);
    if (fused_silu) return launch_w4<2>(a, 1, w.zp != nullptr, grid, stream);
    return launch_w4<1>(a, 1, w.zp != nullptr, grid, stream);
}

}  // namespace fh
