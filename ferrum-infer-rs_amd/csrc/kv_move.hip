// Whole-block moves of the paged KV cache: the one kernel behind sequence fork, truncate (privatising a shared block), and
// host swap-out / swap-in (runner.hip).  Off the forward path: nothing here is captured into the decode graph.
//
// One KV block of one pool (a layer's K or V, kv_layout.h) is ONE contiguous chunk of kv_heads · 16 · head_dim fp16 — 2 KiB at
// nkv 1 / hd 64, 16 KiB at nkv 4 / hd 128 — so "move N blocks of a sequence" is N · 2L chunk copies, whatever the tile layout
// inside the chunk is.  The grid is (pair, pool); a workgroup copies one chunk with 16-byte loads and stores per lane, four
// loads of a lane in flight before its first store while whole passes remain.  A chunk need not fill a 256-lane pass (2 KiB =
// 128 lanes): what is left after the whole passes moves under a guard by the chunk's own length.  Slots of a block beyond the sequence's length travel too (don't-care content).
//
//   KV_MOVE_POOL    : pools[p][pair.dst] = pools[p][pair.src]
//   KV_MOVE_GATHER  : staging[pair index][p] = pools[p][pair.src]      staging is [pair][layer][K, V][chunk], contiguous
//   KV_MOVE_SCATTER : pools[p][pair.dst] = staging[pair index][p]
#include "kernels.h"

namespace fh {

namespace {

constexpr int KV_MOVE_THREADS = 256;
constexpr int KV_MOVE_PASS = 4 * KV_MOVE_THREADS;     // 16-byte vectors one workgroup moves per full pass: four per lane

// 16 bytes in the global address space: a pool base read from the pointer array is a generic pointer to the compiler, which
// would address it with flat instructions
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) u32x4 g_u32x4;

__global__ __launch_bounds__(KV_MOVE_THREADS) void kv_move_kernel(void* const* __restrict__ pools, const uint2* __restrict__ pairs,
                                                                  void* staging, int chunk_vecs, unsigned num_blocks, int mode) {
    const int pair = blockIdx.x, pool = blockIdx.y;
    const uint2 p = pairs[pair];
    // ids come from the host allocator; an id outside the pool moves nothing rather than touch memory that is not the pool's
    if ((mode != KV_MOVE_SCATTER && p.x >= num_blocks) || (mode != KV_MOVE_GATHER && p.y >= num_blocks)) return;
    if (mode == KV_MOVE_POOL && p.x == p.y) return;
    g_u32x4* base = (g_u32x4*)pools[pool];
    g_u32x4* stage = (g_u32x4*)staging + ((long)pair * gridDim.y + pool) * chunk_vecs;
    const g_u32x4* src = mode == KV_MOVE_SCATTER ? stage : base + (long)p.x * chunk_vecs;
    g_u32x4* dst = mode == KV_MOVE_GATHER ? stage : base + (long)p.y * chunk_vecs;
    // full passes: four loads of a lane in flight before its first store (source and destination chunks never overlap)
    int i = threadIdx.x;
    for (; i + 3 * KV_MOVE_THREADS < chunk_vecs; i += KV_MOVE_PASS) {
        const u32x4 v0 = src[i], v1 = src[i + KV_MOVE_THREADS], v2 = src[i + 2 * KV_MOVE_THREADS], v3 = src[i + 3 * KV_MOVE_THREADS];
        dst[i] = v0;
        dst[i + KV_MOVE_THREADS] = v1;
        dst[i + 2 * KV_MOVE_THREADS] = v2;
        dst[i + 3 * KV_MOVE_THREADS] = v3;
    }
    // the tail: whatever is left of the chunk, one guarded vector per lane and step (a 2 KiB chunk is all tail: 128 lanes, once)
    for (; i < chunk_vecs; i += KV_MOVE_THREADS) dst[i] = src[i];
}

}  // namespace

int kv_move_blocks(void* const* pools_dev, int num_pools, const uint32_t* pairs_dev, int num_pairs, void* staging, size_t chunk_bytes,
                   int num_blocks, int mode, hipStream_t s) {
    if (num_pairs <= 0) return 0;
    FH_REQUIRE(pools_dev && pairs_dev, "kv_move: null pool or pair array");
    FH_REQUIRE(mode == KV_MOVE_POOL || mode == KV_MOVE_GATHER || mode == KV_MOVE_SCATTER, "kv_move: mode=%d", mode);
    FH_REQUIRE(mode == KV_MOVE_POOL || staging, "kv_move: gather / scatter without a staging buffer");
    FH_REQUIRE(num_pools >= 1 && num_pools <= 65535, "kv_move: %d pools (1 … 65535)", num_pools);
    FH_REQUIRE(num_blocks >= 1, "kv_move: num_blocks=%d", num_blocks);
    FH_REQUIRE(chunk_bytes >= 16 && chunk_bytes % 16 == 0 && chunk_bytes / 16 <= (size_t)1 << 24,
               "kv_move: chunk of %zu bytes (a multiple of 16, at most 256 MiB)", chunk_bytes);
    hipLaunchKernelGGL(kv_move_kernel, dim3(num_pairs, num_pools), dim3(KV_MOVE_THREADS), 0, s, pools_dev,
                       reinterpret_cast<const uint2*>(pairs_dev), staging, (int)(chunk_bytes / 16),
                       (unsigned)num_blocks, mode);
    FH_CHECK_LAUNCH();
    return 0;
}

}  // namespace fh
