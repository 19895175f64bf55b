// INT4 dense GEMMs of the decode regime (≤ 64 rows): K split across the waves of a workgroup (w4_gemm_wgsplit_kernel),
// activations shared through LDS (w4_gemm_ldsa_kernel), the split-K reduce — and w4_gemm_dense, the dispatcher over every
// dense form (the tile kernels are in w4_tiles.hip).  Layout and arithmetic: w4_gemm.h.
#include "w4_gemm.h"

namespace fh {

__global__ void splitk_reduce_bias_kernel(const float* __restrict__ partial, __half* __restrict__ out,
                                          const __half* __restrict__ bias, int S, int M, int N, int rows_pad, int n_pad,
                                          int ldo) {
    int col = blockIdx.x * blockDim.x + threadIdx.x;
    int row = blockIdx.y;
    if (col >= N || row >= M) return;
    float s = 0.f;
    for (int z = 0; z < S; z++) s += partial[((long)z * rows_pad + row) * n_pad + col];
    if (bias) s += __half2float(bias[col]);
    out[(long)row * ldo + col] = __float2half(s);
}

// ── dense skinny GEMM, K split ACROSS THE WAVES of one workgroup ─────────────────────────────────
// The small projections of the decode layer (qkv, o) are latency-bound: a slab split-K needs a second
// launch (≈5 µs) to reduce.  Here the W waves of a workgroup take K-slices of the same NT column
// tiles and reduce their fp32 accumulators through LDS, so the GEMM is ONE launch with fp16 output.
// FUSE_A (MT = 1, ≤ 4 rows — decode at c ≤ 4, where every dependent launch costs ≈ 4 µs whatever it does): the activation rows
// are produced by the workgroup itself — residual' = residual + Σ_k w_k·down_k (k ascending, fp32, one fp16 rounding: the
// arithmetic of moe_combine_add_rmsnorm_kernel), x = rms_norm(residual')·ln — into LDS, after the first weight group has been
// requested; workgroup 0 also stores residual'.  Every workgroup repeats the ≈ 36 KB per row of L2 reads: cheap at ≤ 4 rows,
// prohibitive at 32, which is why only the small batches fuse.
template <int MT, int NT, bool HAS_ZP, bool FUSE_A = false>
__global__ __launch_bounds__(MT == 1 ? 1024 : (MT == 2 ? (NT == 1 ? 1024 : 512) : 256)) void w4_gemm_wgsplit_kernel(W4Args p) {
    static_assert(!FUSE_A || MT == 1, "the fused prologue serves one 16-row tile");
    extern __shared__ __attribute__((aligned(16))) float red[];
    const int W = blockDim.x >> 6;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int a = lane >> 4, b = lane & 15;
    const int tile0 = blockIdx.x * NT;            // first 16-column tile of this workgroup
    const int st = tile0 >> 2, nt0 = tile0 & 3;   // NT divides 4 → all tiles in one supertile
    const int rb = blockIdx.y;
    constexpr int V = MT * NT * 4;

    const __half* xrow[MT];
    const int KP = p.K + 8;                                   // LDS row pitch of the fused rows (16 B of padding: rows on different banks)
    __half* xs = reinterpret_cast<__half*>(red + (size_t)W * V * 64);
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        int r = rb * 16 * MT + mt * 16 + b;
        if (FUSE_A) xrow[mt] = xs + (long)(r < p.M ? r : p.M - 1) * KP + 8 * a;
        else xrow[mt] = p.x + (long)(r < p.M ? r : p.M - 1) * p.K + 8 * a;
    }
    const u32x4* qw_lane = reinterpret_cast<const u32x4*>(p.qw) + ((long)st * p.G * 4 + nt0) * 64 + lane;
    const uint2* sc_lane = reinterpret_cast<const uint2*>(p.sc) + ((long)st * p.G) * 16 + b;
    const uint2* zp_lane = HAS_ZP ? reinterpret_cast<const uint2*>(p.zp) + ((long)st * p.G) * 16 + b : nullptr;

    float4v acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) acc[mt][nt] = (float4v){0.f, 0.f, 0.f, 0.f};

    const int g0 = (int)((long)p.G * wave / W), g1 = (int)((long)p.G * (wave + 1) / W);
    u32x4 wq[2][NT];
    uint2 scv[2], zpv[2];
    half8 af[2][MT][4];
    auto issue_w = [&](int buf, int g) __attribute__((always_inline)) {
#pragma unroll
        for (int nt = 0; nt < NT; nt++) wq[buf][nt] = __builtin_nontemporal_load(qw_lane + ((long)g * 4 + nt) * 64);
        scv[buf] = sc_lane[(long)g * 16];
        if (HAS_ZP) zpv[buf] = zp_lane[(long)g * 16];
    };
    auto issue_a = [&](int buf, int g) __attribute__((always_inline)) {
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int s = 0; s < 4; s++) af[buf][mt][s] = *reinterpret_cast<const half8*>(xrow[mt] + g * 128 + 32 * s);
    };
    auto issue = [&](int buf, int g) __attribute__((always_inline)) { issue_w(buf, g); issue_a(buf, g); };
    auto consume = [&](int buf) {
        const unsigned long long sb = ((unsigned long long)scv[buf].y << 32) | scv[buf].x;
        const unsigned long long zb = HAS_ZP ? (((unsigned long long)zpv[buf].y << 32) | zpv[buf].x) : 0ull;
        w4_consume_group<MT, NT, HAS_ZP, false>(wq[buf], sb, zb, nt0, af[buf], acc);
    };
    if (FUSE_A) {
        if (g0 < g1) issue_w(0, g0);                          // the first weight group travels while the rows are made
        FH_PIN();
        float* wred = reinterpret_cast<float*>(xs + (size_t)p.M * KP);     // [W] partial sums of squares
        const int nvec = p.K >> 3, tk = p.fa_top_k;
        const bool writer = blockIdx.x == 0 && blockIdx.y == 0;
        for (int t = 0; t < p.M; t++) {
            float ss = 0.f;
            for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
                float accv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                float wk8[8];
                half8 d8[8];
#pragma unroll
                for (int k = 0; k < 8; k++) {                  // the first 8 expert rows are requested together
                    const int kc = k < tk ? k : tk - 1;
                    wk8[k] = p.fa_weights[t * tk + kc];
                    d8[k] = *reinterpret_cast<const half8*>(p.fa_down + ((long)t * tk + kc) * p.K + i * 8);
                }
                half8 rv = *reinterpret_cast<const half8*>(p.fa_res_in + (long)t * p.K + i * 8);
#pragma unroll
                for (int k = 0; k < 8; k++)
                    if (k < tk) {
#pragma unroll
                        for (int j = 0; j < 8; j++) accv[j] += wk8[k] * (float)d8[k][j];
                    }
                for (int k = 8; k < tk; k++) {
                    const float wk = p.fa_weights[t * tk + k];
                    const half8 d = *reinterpret_cast<const half8*>(p.fa_down + ((long)t * tk + k) * p.K + i * 8);
#pragma unroll
                    for (int j = 0; j < 8; j++) accv[j] += wk * (float)d[j];
                }
#pragma unroll
                for (int j = 0; j < 8; j++) rv[j] = (_Float16)((float)rv[j] + accv[j]);
                if (writer) *reinterpret_cast<half8*>(p.fa_res_out + (long)t * p.K + i * 8) = rv;
                *reinterpret_cast<half8*>(xs + (long)t * KP + i * 8) = rv;           // un-normalised for now
#pragma unroll
                for (int j = 0; j < 8; j++) ss += (float)rv[j] * (float)rv[j];
            }
            ss = wave_reduce_sum(ss);
            if (lane == 0) wred[wave] = ss;
            __syncthreads();
            float total = 0.f;
            for (int w = 0; w < W; w++) total += wred[w];
            const float inv = 1.0f / sqrtf(total / (float)p.K + p.fa_eps);
            for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
                half8 rv = *reinterpret_cast<const half8*>(xs + (long)t * KP + i * 8);       // this thread's own store
                const half8 wv = *reinterpret_cast<const half8*>(p.fa_ln + i * 8);
#pragma unroll
                for (int j = 0; j < 8; j++) rv[j] = (_Float16)((float)rv[j] * inv * (float)wv[j]);
                *reinterpret_cast<half8*>(xs + (long)t * KP + i * 8) = rv;
            }
            __syncthreads();
        }
        if (g0 < g1) issue_a(0, g0);
        FH_PIN();
    }
    if (g0 < g1) {
        if (!FUSE_A) issue(0, g0);
        FH_PIN();
        int g = g0;
        for (; g + 2 <= g1 - 1; g += 2) {
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
    // cross-wave reduction through LDS: red[wave][v][lane]
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++)
#pragma unroll
            for (int r = 0; r < 4; r++) red[((wave * V) + (mt * NT + nt) * 4 + r) * 64 + lane] = acc[mt][nt][r];
    __syncthreads();
    for (int v = wave; v < V; v += W) {
        float sum = 0.f;
        for (int w = 0; w < W; w++) sum += red[(w * V + v) * 64 + lane];
        const int r = v & 3, nt = (v >> 2) % NT, mt = (v >> 2) / NT;
        const int row = rb * 16 * MT + mt * 16 + 4 * a + r;
        const int col = (tile0 + nt) * 16 + b;
        if (row < p.M && col < p.N) {
            if (p.bias) sum += __half2float(p.bias[col]);
            p.out[(long)row * p.ldo + col] = __float2half(sum);
        }
    }
}

// ── dense GEMM for 17–64 rows: activations staged ONCE per workgroup in LDS ───────────────────────
// With MT ≥ 2 row tiles a wave that fetches its own A fragments pulls 2–4× more activation bytes (from L2)
// than weight bytes (from HBM) and the kernel runs at the activation rate (gate_up 4096→28672: 12.6 µs at
// m = 1, 25.7 µs at m = 32).  Here the NW waves of a workgroup own NW neighbouring 64-column supertiles over
// the SAME K range: each 128-k group's activations (MT·4 KiB, fragment-major) are loaded cooperatively into
// a double-buffered LDS tile and every wave reads its MFMA A fragments with conflict-free ds_read_b128.
// One barrier per group.  K may be split over grid.z into fp32 slabs (reduced by the consumer kernel).
template <int MT, int NW, bool HAS_ZP>
__global__ __launch_bounds__(NW * 64) void w4_gemm_ldsa_kernel(W4Args p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    half8* lds_a = reinterpret_cast<half8*>(lds_raw);          // [2][MT·4][64] half8
    constexpr int FR = MT * 256;                                // 16-byte fragments per group
    constexpr int NT_ = NW * 64;
    constexpr int ALD = (FR + NT_ - 1) / NT_;                   // fragment loads per thread per group
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int a = lane >> 4, b = lane & 15;
    const int st_raw = blockIdx.x * NW + wave;
    const bool st_ok = st_raw < p.n64;
    const int st = st_ok ? st_raw : p.n64 - 1;
    const int rb = blockIdx.y, z = blockIdx.z;
    const int g0 = (int)((long)p.G * z / p.S), g1 = (int)((long)p.G * (z + 1) / p.S);
    FH_TL(0);

    // cooperative A loads: fragment idx ↔ (mt, k-step s, lane l): row mt·16 + (l & 15), k = 32 s + 8 (l >> 4)
    const __half* asrc[ALD];
#pragma unroll
    for (int i = 0; i < ALD; i++) {
        const int idx = min(threadIdx.x + i * NT_, FR - 1);
        const int mt = idx >> 8, s = (idx >> 6) & 3, l = idx & 63;
        const int r = rb * 16 * MT + mt * 16 + (l & 15);
        asrc[i] = p.x + (long)(r < p.M ? r : p.M - 1) * p.K + 32 * s + 8 * (l >> 4);
    }
    const u32x4* qw_lane = reinterpret_cast<const u32x4*>(p.qw) + ((long)st * p.G * 4) * 64 + lane;
    const uint2* sc_lane = reinterpret_cast<const uint2*>(p.sc) + ((long)st * p.G) * 16 + b;
    const uint2* zp_lane = HAS_ZP ? reinterpret_cast<const uint2*>(p.zp) + ((long)st * p.G) * 16 + b : nullptr;

    float4v acc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < 4; nt++) acc[mt][nt] = (float4v){0.f, 0.f, 0.f, 0.f};

    // Rings of depth 4 (static slots through a 4× unrolled loop): weights of group g+3 and activations of
    // group g+3 are requested while group g is consumed, so one workgroup alone keeps ≈3 groups × NW × 4 KiB
    // in flight (a CU needs ≈48 KB in flight to hold its share of HBM at ≈2 µs latency).
    constexpr int D = 4;
    u32x4 wq[D][4];
    uint2 scv[D], zpv[D];
    half8 areg[D][ALD];
    auto issue_w = [&](int slot, int g) {
#pragma unroll
        for (int nt = 0; nt < 4; nt++) wq[slot][nt] = __builtin_nontemporal_load(qw_lane + ((long)g * 4 + nt) * 64);
        scv[slot] = sc_lane[(long)g * 16];
        if (HAS_ZP) zpv[slot] = zp_lane[(long)g * 16];
    };
    auto issue_a = [&](int slot, int g) {
#pragma unroll
        for (int i = 0; i < ALD; i++) areg[slot][i] = *reinterpret_cast<const half8*>(asrc[i] + (long)g * 128);
    };
    auto store_a = [&](int slot, int buf) {
#pragma unroll
        for (int i = 0; i < ALD; i++) {
            const int idx = threadIdx.x + i * NT_;
            if (idx < FR) lds_a[buf * FR + idx] = areg[slot][i];
        }
    };
    auto consume = [&](int slot, int abuf) {
        half8 af[MT][4];
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int s = 0; s < 4; s++) af[mt][s] = lds_a[abuf * FR + (mt * 4 + s) * 64 + lane];
        const unsigned long long sb = ((unsigned long long)scv[slot].y << 32) | scv[slot].x;
        const unsigned long long zb = HAS_ZP ? (((unsigned long long)zpv[slot].y << 32) | zpv[slot].x) : 0ull;
        w4_consume_group<MT, 4, HAS_ZP>(wq[slot], sb, zb, 0, af, acc);
    };
    // No load sits under a runtime condition in the steady loop (a conditional load makes hipcc wait vmcnt(0) at
    // the join and every group then pays the full memory latency): prefetch indices are CLAMPED to the last group
    // instead — the few repeated requests at the tail hit L2.
    if (g0 < g1) {
        const int gl = g1 - 1;
#pragma unroll
        for (int d = 0; d < D - 1; d++) { issue_w(d, min(g0 + d, gl)); issue_a(d, min(g0 + d, gl)); }
        FH_PIN();
        store_a(0, 0);                                  // A(g0) → LDS buffer 0
        __syncthreads();
        FH_TL(1);
        int gb = g0;
        for (; gb + D <= g1; gb += D) {
#pragma unroll
            for (int d = 0; d < D; d++) {
                const int g = gb + d;
                issue_w((d + D - 1) % D, min(g + D - 1, gl));
                issue_a((d + D - 1) % D, min(g + D - 1, gl));
                store_a((d + 1) % D, (d + 1) & 1);      // A(g+1), requested two groups ago
                FH_PIN();
                consume(d, d & 1);
                FH_PIN();
                __syncthreads();
            }
        }
        // tail: ≤ 3 groups, already requested (slots 0..2 relative to gb)
#pragma unroll
        for (int d = 0; d < D - 1; d++) {
            if (gb + d < g1) {
                if (d + 1 < D - 1) store_a(d + 1, (d + 1) & 1);
                consume(d, d & 1);
                __syncthreads();
            }
        }
    }
    FH_TL(2);
    if (!st_ok) return;
    if (p.partial) {
        float* slab = p.partial + (long)z * p.rows_pad * p.n_pad;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = rb * 16 * MT + mt * 16 + 4 * a + r;
#pragma unroll
                for (int nt = 0; nt < 4; nt++) slab[(long)row * p.n_pad + st * 64 + nt * 16 + b] = acc[mt][nt][r];
            }
#ifdef FERRUM_HIP_EXPERIMENTS
        if (p.tl) { __builtin_amdgcn_s_waitcnt(0); FH_TL(3); }
#endif
        return;
    }
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = rb * 16 * MT + mt * 16 + 4 * a + r;
            if (row >= p.M) continue;
#pragma unroll
            for (int nt = 0; nt < 4; nt++) {
                const int col = st * 64 + nt * 16 + b;
                if (col < p.N) {
                    float v = acc[mt][nt][r];
                    if (p.bias) v += __half2float(p.bias[col]);
                    p.out[(long)row * p.ldo + col] = __float2half(v);
                }
            }
        }
}

#ifdef FERRUM_HIP_EXPERIMENTS
unsigned long long* g_timeline = nullptr;
int g_timeline_mode = 0;
extern "C" __attribute__((visibility("default"))) void ferrum_hip_debug_set_timeline(void* p) { g_timeline = (unsigned long long*)p; }
extern "C" __attribute__((visibility("default"))) void ferrum_hip_debug_set_timeline_mode(int m) { g_timeline_mode = m; }
#endif

template <int MT, int NW>
static int launch_ldsa(const W4Args& a_in, bool has_zp, dim3 grid, hipStream_t stream) {
    const size_t lds = (size_t)2 * MT * 256 * 16;
#ifdef FERRUM_HIP_EXPERIMENTS
    W4Args a = a_in;
    a.tl = g_timeline;
#else
    const W4Args& a = a_in;
#endif
    with_zp(has_zp, [&](auto zp) { hipLaunchKernelGGL((w4_gemm_ldsa_kernel<MT, NW, decltype(zp)::value>), grid, dim3(NW * 64), lds, stream, a); });
    FH_CHECK_LAUNCH();
    return 0;
}

// LDS of a wgsplit launch: the cross-wave reduction [W][MT·NT·4][64] fp32 — and, with the fused prologue, the m rows (pitch
// K + 8 halves) and the [W] partial sums of squares (64 floats reserved)
static size_t wgsplit_lds_bytes(int W, int mt, int nt, bool fused, int m, int k) {
    size_t lds = (size_t)W * mt * nt * 4 * 64 * sizeof(float);
    if (fused) lds += (size_t)m * (k + 8) * sizeof(__half) + 64 * sizeof(float);
    return lds;
}

template <int MT, int NT>
static int launch_wgsplit(const W4Args& a, bool has_zp, dim3 grid, int W, hipStream_t stream) {
    const size_t lds = wgsplit_lds_bytes(W, MT, NT, MT == 1 && a.fa_down != nullptr, a.M, a.K);
    if constexpr (MT == 1) {
        if (a.fa_down) {                                       // fused combine + add + norm prologue (≤ 4 rows)
            FH_REQUIRE(lds <= 64 * 1024, "w4_gemm_dense: fused prologue needs %zu bytes of LDS", lds);
            form_hit(FORM_W4_FUSED_TAIL);
        }
    }
    with_zp(has_zp, [&](auto zp) {
        constexpr bool ZP = decltype(zp)::value;
        if constexpr (MT == 1) {
            if (a.fa_down) {
                hipLaunchKernelGGL((w4_gemm_wgsplit_kernel<1, NT, ZP, true>), grid, dim3(W * 64), lds, stream, a);
                return;
            }
        }
        hipLaunchKernelGGL((w4_gemm_wgsplit_kernel<MT, NT, ZP>), grid, dim3(W * 64), lds, stream, a);
    });
    FH_CHECK_LAUNCH();
    return 0;
}

// The split-K tail of w4_gemm_dense's tile and LDS branches: S (the branch's own heuristic) falls back to 1 when the fp32
// slabs [S][rows_pad][n64·64] do not fit the workspace; `launch(S)` runs the GEMM over grid.z = S; S > 1 adds the reduce.
template <typename Launch>
static int launch_splitk(W4Args& a, const W4Device& w, int S, int rows_pad, float* workspace, size_t workspace_bytes, Form form,
                         hipStream_t stream, Launch&& launch) {
    const int n_pad = w.n64 * 64;
    if (S > 1 && (workspace == nullptr || (size_t)S * rows_pad * n_pad * sizeof(float) > workspace_bytes)) S = 1;
    a.S = S;
    a.rows_pad = rows_pad; a.n_pad = n_pad;
    a.partial = S > 1 ? workspace : nullptr;
    if (int rc = launch(S)) return rc;
    form_hit(form);
    if (S == 1) return 0;
    hipLaunchKernelGGL(splitk_reduce_bias_kernel, dim3(cdiv(w.n, 256), a.M), dim3(256), 0, stream, workspace, a.out, w.bias, S, a.M,
                       w.n, rows_pad, n_pad, w.n);
    FH_CHECK_LAUNCH();
    return 0;
}

// Shape of the intra-workgroup split launch for m rows: NT column tiles per workgroup and W waves (= K slices).  One rule
// for the dispatcher and for the fused-prologue predicate, which has to know the LDS the launch will ask for.
struct WgsplitShape { int nt, W; };
static WgsplitShape wgsplit_shape(const W4Device& w, int m) {
    const int mt = skinny_row_tiles(m);
    const int row_blocks = cdiv(m, 16 * mt);
    const int n16 = w.n64 * 4;
    // column tiles per workgroup: as wide as possible (A-fragment reuse) while ≥ ~384 workgroups exist
    int nt = 4;
    while (nt > 1 && (long)cdiv(n16, nt) * row_blocks < 384) nt >>= 1;
    // with ≥ 2 row tiles the activation fragments dominate the load traffic: share each across two
    // column tiles as long as ≥ 128 workgroups remain (measured: qkv 2048→5120 at T=32 10.4 → 7.2 µs)
    if (mt >= 2 && nt == 1 && (long)cdiv(n16, 2) * row_blocks >= 128) nt = 2;
    // waves per workgroup (= K slices): enough waves to cover the chip, ≥ 1 group each, LDS ≤ 128 KiB
    const long wgs = (long)cdiv(n16, nt) * row_blocks;
    const int w_cap = mt == 1 ? 16 : (mt == 2 ? (nt == 1 ? 16 : 8) : 4);    // matches the kernel's __launch_bounds__
    int W = 4;
    while (wgs * W < 2048 && W * 2 <= std::min(w_cap, w.G) && W * 2 * mt * nt * 4 <= 512) W <<= 1;
    while (W > w.G && W > 1) W >>= 1;
    const Knobs& kn = knobs();
    if (kn.w4_nt) nt = kn.w4_nt;        // tuning overrides (development)
    if (kn.w4_w) W = kn.w4_w;
    return {nt, W};
}

// Dense y[M,N] = x[M,K]·Wᵀ (+bias).  One launch: K is split across the waves of each workgroup.
// The fused prologue keeps its m rows in LDS beside the reduction buffer of the launch w4_gemm_dense would make, so the answer
// depends on that launch's NT and W: at K = 8192 three rows fit only with W·NT ≤ 15 and four rows never do.
bool w4_gemm_dense_can_fuse_combine_norm(const W4Device& w, int m) {
    if (!(m >= 1 && m <= 4 && w.qw != nullptr && w.f16t == nullptr && w.perm == nullptr && w.k % 8 == 0 && w.k <= 8192)) return false;
    const WgsplitShape sh = wgsplit_shape(w, m);
    return wgsplit_lds_bytes(sh.W, 1, sh.nt, true, m, w.k) <= 64 * 1024;
}

int w4_gemm_dense(const W4Device& w, const __half* x, __half* out, int m, float* workspace,
                  size_t workspace_bytes, hipStream_t stream, const FusedCombineNorm* fa) {
    if (m <= 0) return 0;
    // (act-order weights: the packed rows are in sorted-g_idx order and every caller hands over activations whose columns were
    // gathered with the same permutation — dense_linear, ferrum_hip_gptq_linear_forward_f16 — so every kernel form applies)
    FH_REQUIRE(!fa || (w4_gemm_dense_can_fuse_combine_norm(w, m) && fa->residual_in != fa->residual_out && fa->top_k >= 1),
               "w4_gemm_dense: the fused combine + norm prologue needs <= 4 rows of a plain INT4 projection and ping-pong residual buffers");
    if (w.f16t) {                                     // DenseLinear: B::gemm on fp16 weights (linear.rs:109-129)
        form_hit(FORM_F16_DENSE_LINEAR);
        if (int rc = f16t_gemm(x, w.f16t, out, m, w.n, w.k, workspace, workspace_bytes, stream)) return rc;
        return w.bias ? add_bias_f16(out, w.bias, m, w.n, stream) : 0;
    }
    W4Args a = dense_args(w, x, m);
    a.out = out; a.bias = w.bias;
    if (fa) {
        a.fa_down = fa->down; a.fa_weights = fa->weights; a.fa_res_in = fa->residual_in; a.fa_res_out = fa->residual_out;
        a.fa_ln = fa->ln_w; a.fa_eps = fa->eps; a.fa_top_k = fa->top_k;
    }
    const int mt = skinny_row_tiles(m);
    const int row_blocks = cdiv(m, 16 * mt);
    const bool zp = w.zp != nullptr;
    // LDS-shared activations (w4_gemm_ldsa_kernel) + fp32 split-K slabs + one reduce launch.  Measured at m = 32 against
    // the one-launch intra-workgroup split below (tools/exp_dense.py): down 14336→4096 31.3 → 18.4 µs (S = 8),
    // gate_up 4096→28672 25.7 → 23.2 µs (S = 2); the small projections (qkv, o) tie, so they keep the single launch.
    // 64-row pipelined tiles (w4_gemm_tilep_kernel) for prefill — and for 33–63 rows on the larger projections, where the
    // skinny kernels' four row tiles re-fetch every activation fragment per 16–64 columns (c=48 decode, Llama-3.1-8B 5.18 →
    // 4.02 ms per step, Gemma-3-27B 15.1 → 11.5; the 2048→5120 / 4096→2048 projections of Qwen3-30B-A3B are faster skinny)
    const Knobs& kn = knobs();
    // ≥ 96 rows: 96- / 128- / 256-row tiles with the group scale folded into the fp16 B operand (w4_gemm_big_kernel) when they
    // fill the chip.  Deep K (≥ 24 groups): the tallest tile whose last round of 256 workgroups is ≥ 70 % full — 4096→28672 at
    // M = 8192: 64-row tiles 905, 96-row 1204, 128-row 1171, 256-row 1277 TFLOP/s (tools/exp_prefill_gemm.py, a throttled
    // back-to-back loop; one prefill of Llama-3.1-8B: 133 → 101 ms).  Shallow K: the 96-row form, two workgroups per CU, whose
    // prologues and epilogues overlap (2048→5120 at M = 8192: 852 / 924 TFLOP/s for 128 / 256 rows, 962 for 96).
    if (kn.w4_big >= 0 && m >= 96 && w.G % 2 == 0) {
        const int cols = cdiv(w.n64, 4);
        const long wgs6 = (long)cols * cdiv(m, 96), wgs8 = (long)cols * cdiv(m, 128), wgs16 = (long)cols * cdiv(m, 256);
        auto fill = [](long wgs) { return (double)wgs / (double)(cdiv(wgs, 256) * 256); };
        int MTv = 0;
        if (kn.w4_big == 6 || kn.w4_big == 8 || kn.w4_big == 16) MTv = m >= 16 * kn.w4_big ? kn.w4_big : 0;       // development: forced
        else if (w.G >= 24 && m >= 256 && wgs16 >= 192 && fill(wgs16) >= 0.7) MTv = 16;
        else if (w.G >= 24 && m >= 128 && wgs8 >= 192 && fill(wgs8) >= 0.7) MTv = 8;
        else if (wgs6 >= 128) MTv = 6;
        if (MTv) {
            a.S = 1; a.partial = nullptr;
            form_hit(FORM_W4_BIG);
            return launch_big(a, MTv, 0, zp, dim3(cols, cdiv(m, 16 * MTv), 1), stream);
        }
    }
    const int tile_min_env = kn.w4_tile_min_m;
    const int tile_min_m = tile_min_env > 0 ? tile_min_env : ((long)w.k * w.n >= (12L << 20) ? 33 : 64);
    if (m >= tile_min_m) {
        // too few tiles to cover the chip (narrow N or few rows): split K over grid.z into fp32 slabs + one reduce launch,
        // keeping ≥ 8 quant groups per split
        const int tile_wgs = kn.w4_tile_wgs;
        const int cols = cdiv(w.n64, 4), rts = cdiv(m, 64);
        int S = 1;
        while ((long)cols * rts * S < tile_wgs && w.G / (S * 2) >= 8) S *= 2;
        return launch_splitk(a, w, S, rts * 64, workspace, workspace_bytes, FORM_W4_TILEP, stream,
                             [&](int s) { return launch_tilep(a, zp, dim3(cols, rts, s), stream); });
    }
    const int lds_mode = kn.w4_ldsa;
    const bool lds_shape = (w.G >= 64 && w.n64 >= 32) || w.n64 >= 256;
    if (mt >= 2 && (lds_mode == 2 || (lds_mode == 1 && lds_shape && mt == 2))) {
        int nw = 4;
        if (kn.w4_ldsa_nw) nw = kn.w4_ldsa_nw == 8 && mt == 2 ? 8 : 4;
        const int cols = cdiv(w.n64, nw);
        int S = 1;
        while ((long)cols * row_blocks * S < 128 && w.G / (S * 2) >= 8) S *= 2;
        while (w.n64 <= 128 && (long)cols * row_blocks * S < 256 && w.G / (S * 2) >= 16) S *= 2;
        if (kn.w4_ldsa_s) S = std::max(1, std::min(kn.w4_ldsa_s, w.G));
        return launch_splitk(a, w, S, row_blocks * 16 * mt, workspace, workspace_bytes, FORM_W4_LDSA, stream, [&](int s) {
            const dim3 grid(cols, row_blocks, s);
            if (mt == 2) return nw == 8 ? launch_ldsa<2, 8>(a, zp, grid, stream) : launch_ldsa<2, 4>(a, zp, grid, stream);
            return launch_ldsa<4, 4>(a, zp, grid, stream);      // MT = 4 with 8 waves would exceed 256 VGPRs per lane
        });
    }
    const int n16 = w.n64 * 4;
    const WgsplitShape sh = wgsplit_shape(w, m);
    const int nt = sh.nt, W = sh.W;
    dim3 grid(cdiv(n16, nt), row_blocks, 1);
    form_hit(FORM_W4_WGSPLIT);
#define FH_WG(MTV, NTV) return launch_wgsplit<MTV, NTV>(a, zp, grid, W, stream)
    if (mt == 1) { if (nt == 4) FH_WG(1, 4); if (nt == 2) FH_WG(1, 2); FH_WG(1, 1); }
    if (mt == 2) { if (nt == 4) FH_WG(2, 4); if (nt == 2) FH_WG(2, 2); FH_WG(2, 1); }
    if (nt == 4) FH_WG(4, 4);
    if (nt == 2) FH_WG(4, 2);
    FH_WG(4, 1);
#undef FH_WG
}

// Split count the LDS-shared-activation kernel wants for this shape (tools/exp_dense.py sweeps): enough workgroups to
// cover the chip (≥ 128–256 of 4 waves) while every split keeps ≥ 8 quant groups.
int w4_gemm_dense_lds_splits(const W4Device& w, int m) {
    const int mt = skinny_row_tiles(m);
    const int row_blocks = cdiv(m, 16 * mt), cols = cdiv(w.n64, 4);
    int S = 1;
    const int min_wgs = knobs().lds_min_wgs, min_groups = knobs().lds_min_groups;
    while ((long)cols * row_blocks * S < min_wgs && w.G / (S * 2) >= min_groups) S *= 2;
    // deep K (≥ 16 groups per split left): go on to one workgroup per CU — Llama-70B down 28672→8192 ran on 128 of 256 CUs
    // (narrow N only: for wide N the extra fp32 slabs cost more than the idle CUs — Gemma-3 gate_up 5376→43008 got slower)
    while (w.n64 <= 128 && (long)cols * row_blocks * S < 2 * min_wgs && w.G / (S * 2) >= 2 * min_groups) S *= 2;
    return S;
}

// Dense projection for 17–32 rows as S fp32 slabs through w4_gemm_ldsa_kernel (activations staged once per workgroup in
// LDS); the consumer kernel sums the slabs in order.  S ≤ 0 → w4_gemm_dense_lds_splits.
int w4_gemm_dense_slabs_lds(const W4Device& w, const __half* x, float* slabs, size_t slab_bytes, int m, int* S_inout,
                            int* rows_pad_out, int* n_pad_out, hipStream_t stream) {
    if (m <= 0) return 0;
    FH_REQUIRE(w.bias == nullptr, "w4_gemm_dense_slabs_lds: bias weights use the direct path");
    FH_REQUIRE(m > 16 && m <= 32, "w4_gemm_dense_slabs_lds: m=%d (17..32 rows)", m);
    int S = *S_inout > 0 ? *S_inout : w4_gemm_dense_lds_splits(w, m);
    S = std::max(1, std::min(S, w.G));
    W4Args a = dense_args(w, x, m);
    if (int rc = slab_output(a, S, 32, slabs, slab_bytes, "w4_gemm_dense_slabs_lds", rows_pad_out, n_pad_out)) return rc;
    *S_inout = S;
    form_hit(FORM_W4_SLABS_LDS);
    return launch_ldsa<2, 4>(a, w.zp != nullptr, dim3(cdiv(w.n64, 4), 1, S), stream);
}

}  // namespace fh
