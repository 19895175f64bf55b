// fp16 GEMMs for weights that stay unquantised (router, lm_head, DenseLinear projections): row-major and f16t-tiled.
#include "common.h"
#include "kernels.h"

namespace fh {

// Sum S fp32 slabs in fixed order → fp16 [M, N] (optionally gathering padded MoE rows).
template <typename OutT>
__global__ void splitk_reduce_kernel(const float* __restrict__ partial, OutT* __restrict__ out, int S,
                                     int M, int N, int rows_pad, int n_pad, int ldo) {
    int col = blockIdx.x * blockDim.x + threadIdx.x;
    int row = blockIdx.y;
    if (col >= N || row >= M) return;
    float s = 0.f;
    for (int z = 0; z < S; z++) s += partial[((long)z * rows_pad + row) * n_pad + col];
    out[(long)row * ldo + col] = (OutT)s;
}

// ───────────────────────── fp16 skinny GEMM (router, lm_head) ───────────────
// out[M,N] = x[M,K]·Wᵀ with W [N,K] fp16 row-major (B::gemm, traits.rs:190; cuBLAS hgemm on the
// reference's CUDA lane).  Same operand roles as the INT4 kernel: W rows are B-operand columns.
template <int MT, typename OutT>
__global__ __launch_bounds__(256) void f16_gemm_kernel(const __half* __restrict__ x, const __half* __restrict__ w,
                                                       OutT* __restrict__ out, float* __restrict__ partial,
                                                       int M, int N, int K, int S, int rows_pad, int n_pad) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int a = lane >> 4, b = lane & 15;
    const int ntile2 = blockIdx.x * 4 + wave;       // pair of 16-column tiles
    const int n0 = ntile2 * 32;
    if (n0 >= N) return;
    const int rb = blockIdx.y, z = blockIdx.z;
    const int ksteps = K / 32;
    const int s0 = (int)((long)ksteps * z / S), s1 = (int)((long)ksteps * (z + 1) / S);
    const __half* xrow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        int r = rb * 16 * MT + mt * 16 + b;
        xrow[mt] = x + (long)(r < M ? r : M - 1) * K + 8 * a;
    }
    const __half* wrow[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        int n = n0 + j * 16 + b;
        wrow[j] = w + (long)(n < N ? n : N - 1) * K + 8 * a;
    }
    float4v acc[MT][2];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[mt][j] = (float4v){0.f, 0.f, 0.f, 0.f};

    constexpr int U = 4;   // k-steps in flight per trip
    int s = s0;
    for (; s + U <= s1; s += U) {
        half8 bw[U][2], ax[U][MT];
#pragma unroll
        for (int u = 0; u < U; u++) {
#pragma unroll
            for (int j = 0; j < 2; j++)
                bw[u][j] = __builtin_nontemporal_load(reinterpret_cast<const half8*>(wrow[j] + (s + u) * 32));
#pragma unroll
            for (int mt = 0; mt < MT; mt++) ax[u][mt] = *reinterpret_cast<const half8*>(xrow[mt] + (s + u) * 32);
        }
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
                    acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ax[u][mt], bw[u][j], acc[mt][j], 0, 0, 0);
    }
    for (; s < s1; s++) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            half8 bwv = *reinterpret_cast<const half8*>(wrow[j] + s * 32);
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                half8 axv = *reinterpret_cast<const half8*>(xrow[mt] + s * 32);
                acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(axv, bwv, acc[mt][j], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            int row = rb * 16 * MT + mt * 16 + 4 * a + r;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                int col = n0 + j * 16 + b;
                if (S > 1) {
                    partial[((long)z * rows_pad + row) * n_pad + col] = acc[mt][j][r];
                } else if (row < M && col < N) {
                    out[(long)row * N + col] = (OutT)acc[mt][j][r];
                }
            }
        }
}

// ───────────── fp16 weights in MFMA-fragment-major tiles ("f16t") ─────────────
// Dense fp16 weights that are streamed once per step (lm_head, MoE router) are re-laid at load from
// row-major [N,K] to [N/16 tiles][K/32 k-steps][64 lanes][8 halves]: lane (a,b) of k-step s holds
// W[16·tile + b][32s + 8a .. +8], i.e. exactly its B-operand fragment, so every wave load is one
// contiguous 1-KiB line burst (the row-major form makes each lane of a load touch a different 4-KiB-
// strided row — 64 separate 16-byte segments per instruction).
__global__ void f16t_repack_kernel(const __half* __restrict__ w, __half* __restrict__ out, int N, int K) {
    const long chunk = (long)blockIdx.x * blockDim.x + threadIdx.x;      // one 16-byte chunk per thread
    const int ksteps = K >> 5;
    const long total = (long)((N + 15) >> 4) * ksteps * 64;
    if (chunk >= total) return;
    const int lane = (int)(chunk & 63);
    const long ts = chunk >> 6;
    const int s = (int)(ts % ksteps);
    const long tile = ts / ksteps;
    const int a = lane >> 4, b = lane & 15;
    const long n = tile * 16 + b;
    half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (n < N) v = *reinterpret_cast<const half8*>(w + n * K + 32 * s + 8 * a);
    *reinterpret_cast<half8*>(out + chunk * 8) = v;
}

int f16t_repack(const __half* w_rowmajor, __half* out_tiled, int n, int k, hipStream_t stream) {
    FH_REQUIRE(k % 32 == 0, "f16t repack: K=%d must be a multiple of 32", k);
    long total = (long)cdiv(n, 16) * (k / 32) * 64;
    hipLaunchKernelGGL(f16t_repack_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, w_rowmajor, out_tiled, n, k);
    FH_CHECK_LAUNCH();
    return 0;
}
size_t f16t_elems(int n, int k) { return (size_t)cdiv(n, 16) * 16 * k; }

// J = 16-column tiles per wave: 2, or 4 for two row tiles against a wide N (the lm_head at 17–32 rows: with 2 the activation
// fragments a wave re-reads from L2 are as many bytes as the weights it streams from HBM)
template <int MT, typename OutT, int J = 2>
__global__ __launch_bounds__(256) void f16t_gemm_kernel(const __half* __restrict__ x, const __half* __restrict__ wt,
                                                        OutT* __restrict__ out, float* __restrict__ partial, int M, int N,
                                                        int K, int S, int rows_pad, int n_pad) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int a = lane >> 4, b = lane & 15;
    const int ntile2 = blockIdx.x * 4 + wave;       // group of J 16-column tiles
    const int n0 = ntile2 * 16 * J;
    if (n0 >= N) return;
    const int rb = blockIdx.y, z = blockIdx.z;
    const int ksteps = K >> 5;
    const int tiles = (N + 15) >> 4;
    const int s0 = (int)((long)ksteps * z / S), s1 = (int)((long)ksteps * (z + 1) / S);
    const __half* xrow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        int r = rb * 16 * MT + mt * 16 + b;
        xrow[mt] = x + (long)(r < M ? r : M - 1) * K + 8 * a;
    }
    const __half* wtile[J];
#pragma unroll
    for (int j = 0; j < J; j++) {
        int t = ntile2 * J + j;
        wtile[j] = wt + ((long)(t < tiles ? t : tiles - 1) * ksteps * 64 + lane) * 8;
    }
    float4v acc[MT][J];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int j = 0; j < J; j++) acc[mt][j] = (float4v){0.f, 0.f, 0.f, 0.f};
    constexpr int U = 4;
    int s = s0;
    for (; s + U <= s1; s += U) {
        half8 bw[U][J], ax[U][MT];
#pragma unroll
        for (int u = 0; u < U; u++) {
#pragma unroll
            for (int j = 0; j < J; j++)
                bw[u][j] = __builtin_nontemporal_load(reinterpret_cast<const half8*>(wtile[j] + (long)(s + u) * 512));
#pragma unroll
            for (int mt = 0; mt < MT; mt++) ax[u][mt] = *reinterpret_cast<const half8*>(xrow[mt] + (s + u) * 32);
        }
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int j = 0; j < J; j++)
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
                    acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ax[u][mt], bw[u][j], acc[mt][j], 0, 0, 0);
    }
    for (; s < s1; s++) {
#pragma unroll
        for (int j = 0; j < J; j++) {
            half8 bwv = *reinterpret_cast<const half8*>(wtile[j] + (long)s * 512);
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                half8 axv = *reinterpret_cast<const half8*>(xrow[mt] + s * 32);
                acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(axv, bwv, acc[mt][j], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            int row = rb * 16 * MT + mt * 16 + 4 * a + r;
#pragma unroll
            for (int j = 0; j < J; j++) {
                int col = n0 + j * 16 + b;
                if (S > 1) {
                    partial[((long)z * rows_pad + row) * n_pad + col] = acc[mt][j][r];
                } else if (row < M && col < N) {
                    out[(long)row * N + col] = (OutT)acc[mt][j][r];
                }
            }
        }
}

// One launcher for both layouts — TILED: f16t tiles (f16t_gemm_kernel), else row-major [N,K] (f16_gemm_kernel).
template <typename OutT, bool TILED>
static int f16_gemm_impl(const __half* x, const __half* w, OutT* out, int m, int n, int k, float* workspace,
                         size_t workspace_bytes, hipStream_t stream) {
    if (m <= 0) return 0;
    FH_REQUIRE(k % 32 == 0, "%s: K=%d must be a multiple of 32", TILED ? "f16t_gemm" : "f16_gemm", k);
    int mt = m <= 16 ? 1 : (m <= 32 ? 2 : 4);
    int row_blocks = cdiv(m, 16 * mt);
    int ntile2 = cdiv(n, 32);
    int ksteps = k / 32;
    long tasks = (long)ntile2 * row_blocks;
    int S = 1;
    while (tasks * S < 2048 && S * 2 <= ksteps / 8) S *= 2;
    int rows_pad = row_blocks * 16 * mt, n_pad = ntile2 * 32;
    if (S > 1 && (size_t)S * rows_pad * n_pad * sizeof(float) > workspace_bytes) S = 1;
    if constexpr (TILED) {
        if (mt == 2 && S == 1 && n >= 32768 && n % 64 == 0) {       // wide N at 17–32 rows (the lm_head): 64 columns per wave
            hipLaunchKernelGGL((f16t_gemm_kernel<2, OutT, 4>), dim3(cdiv(cdiv(n, 64), 4), row_blocks, 1), dim3(256), 0, stream, x, w, out, workspace, m,
                               n, k, 1, rows_pad, n_pad);
            FH_CHECK_LAUNCH();
            return 0;
        }
    }
    dim3 grid(cdiv(ntile2, 4), row_blocks, S);
#define FH_F16(MTV)                                                                                                                                      \
    if constexpr (TILED) hipLaunchKernelGGL((f16t_gemm_kernel<MTV, OutT>), grid, dim3(256), 0, stream, x, w, out, workspace, m, n, k, S, rows_pad, n_pad); \
    else hipLaunchKernelGGL((f16_gemm_kernel<MTV, OutT>), grid, dim3(256), 0, stream, x, w, out, workspace, m, n, k, S, rows_pad, n_pad)
    if (mt == 1) { FH_F16(1); } else if (mt == 2) { FH_F16(2); } else { FH_F16(4); }
#undef FH_F16
    FH_CHECK_LAUNCH();
    if (S > 1) {
        hipLaunchKernelGGL(splitk_reduce_kernel<OutT>, dim3(cdiv(n, 256), m), dim3(256), 0, stream, workspace, out, S, m, n,
                           rows_pad, n_pad, n);
        FH_CHECK_LAUNCH();
    }
    return 0;
}

int f16_gemm(const __half* x, const __half* w, __half* out, int m, int n, int k, float* workspace,
             size_t workspace_bytes, hipStream_t stream) {
    return f16_gemm_impl<__half, false>(x, w, out, m, n, k, workspace, workspace_bytes, stream);
}
int f16_gemm_f32out(const __half* x, const __half* w, float* out, int m, int n, int k, float* workspace,
                    size_t workspace_bytes, hipStream_t stream) {
    return f16_gemm_impl<float, false>(x, w, out, m, n, k, workspace, workspace_bytes, stream);
}
int f16t_gemm(const __half* x, const __half* wt, __half* out, int m, int n, int k, float* workspace,
              size_t workspace_bytes, hipStream_t stream) {
    return f16_gemm_impl<__half, true>(x, wt, out, m, n, k, workspace, workspace_bytes, stream);
}
int f16t_gemm_f32out(const __half* x, const __half* wt, float* out, int m, int n, int k, float* workspace,
                     size_t workspace_bytes, hipStream_t stream) {
    return f16_gemm_impl<float, true>(x, wt, out, m, n, k, workspace, workspace_bytes, stream);
}

}  // namespace fh
