#!/usr/bin/env python3
"""The whole-block KV move (csrc/kv_move.hip) in its gather mode at Qwen3-30B-A3B dimensions — 48 layers, 4 kv heads × 128,
1.5 MiB per 16-token block over 96 pools — against ONE hipMemcpyAsync device-to-device of the same byte count (the runtime's
yardstick: a contiguous copy, which a swap of scattered blocks cannot be).  1, 24 and 256 blocks per launch; µs per launch
by device events, GB/s of bytes moved (read + written counts once, as for a copy), and the ratio.

Sources rotate over a 1024-block pool (1.5 GiB, six times the Infinity Cache) so that no launch re-reads what the last one
left on the die; the two forms alternate window by window, five windows each, median reported with the spread.
Usage: exp_kv_move.py [out.txt]      (prints the table; writes it to out.txt too when one is named)"""
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge

LAYERS, NKV, HD, POOL_BLOCKS, WINDOWS = 48, 4, 128, 1024, 5
CHUNK = NKV * 16 * HD * 2
BLOCK_BYTES = 2 * LAYERS * CHUNK


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    assert torch.cuda.is_available(), "needs a GPU: a timing from anywhere else says nothing"
    lib = ge.load_package().load_library()
    pools = [torch.empty(POOL_BLOCKS * CHUNK, dtype=torch.uint8, device="cuda").random_(0, 256) for _ in range(2 * LAYERS)]
    ptrs = torch.tensor([p.data_ptr() for p in pools], dtype=torch.int64).cuda()
    flat = torch.empty(POOL_BLOCKS * BLOCK_BYTES // 2, dtype=torch.uint8, device="cuda").random_(0, 256)   # memcpy source, 768 MiB
    rng = np.random.default_rng(0)
    lines = [f"kv_move gather vs one hipMemcpyAsync D2D — {LAYERS} layers, nkv {NKV}, hd {HD}: {CHUNK} B per chunk, "
             f"{BLOCK_BYTES / 2**20:.2f} MiB per block, {2 * LAYERS} pools of {POOL_BLOCKS} blocks; {torch.cuda.get_device_name(0)}"]
    for nb in (1, 24, 256):
        nbytes = nb * BLOCK_BYTES
        stage = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        sets = max(2, min(POOL_BLOCKS // nb, 64))                  # distinct source block sets a window cycles through
        perm = rng.permutation(POOL_BLOCKS)[:sets * nb].astype(np.int32).reshape(sets, nb)
        pairs = torch.from_numpy(np.stack([perm, np.zeros_like(perm)], axis=-1).copy()).cuda()            # [sets][nb][src, dst]
        launches = int(min(5000, max(40, (16 << 30) // nbytes)))   # ≥ 40 launches, up to 16 GiB per window
        pair_ptrs = [C.c_void_p(pairs[s_].data_ptr()) for s_ in range(sets)]
        pools_p, stage_p = C.c_void_p(ptrs.data_ptr()), C.c_void_p(stage.data_ptr())

        def gather(i):
            rc = lib.ferrum_hip_kv_move_blocks(pools_p, 2 * LAYERS, pair_ptrs[i % sets], nb, stage_p, C.c_size_t(CHUNK), POOL_BLOCKS, 1, None)
            assert rc == 0, lib.ferrum_hip_last_error().decode()

        def memcpy(i):
            off = (i * nbytes) % (flat.numel() - nbytes + 1) // 256 * 256
            rc = lib.ferrum_hip_memcpy_d2d(stage_p, C.c_void_p(flat.data_ptr() + off), C.c_size_t(nbytes), None)
            assert rc == 0, lib.ferrum_hip_last_error().decode()

        def window(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(launches):
                fn(i)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / launches

        for fn in (gather, memcpy):                                # warm-up: code object, both paths, every source set once
            for i in range(min(launches, sets + 3)):
                fn(i)
        torch.cuda.synchronize()
        # what was gathered is what the pools hold
        gather(0)
        torch.cuda.synchronize()
        got = stage.view(nb, 2 * LAYERS, CHUNK)
        for j in (0, nb - 1):
            b = int(perm[0, j])
            assert all(torch.equal(got[j, p], pools[p][b * CHUNK:(b + 1) * CHUNK]) for p in (0, 1, 2 * LAYERS - 1)), (nb, j)
        us = {"kernel": [], "memcpy": []}
        for _ in range(WINDOWS):
            us["kernel"].append(window(gather))
            us["memcpy"].append(window(memcpy))
        k, m = statistics.median(us["kernel"]), statistics.median(us["memcpy"])
        lines.append(f"blocks {nb:4d}  {nbytes / 2**20:8.2f} MiB  launches/window {launches:5d}  "
                     f"kernel {k:9.2f} us [{min(us['kernel']):.2f} … {max(us['kernel']):.2f}] {nbytes / k / 1e3:8.1f} GB/s   "
                     f"memcpy {m:9.2f} us [{min(us['memcpy']):.2f} … {max(us['memcpy']):.2f}] {nbytes / m / 1e3:8.1f} GB/s   "
                     f"kernel/memcpy time {k / m:.3f}")
        print(lines[-1], flush=True)
        del stage, pairs
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("wrote", out_path)


if __name__ == "__main__":
    main()
