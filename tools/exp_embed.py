#!/usr/bin/env python3
"""The embedding path at Qwen3-Embedding-8B dimensions (hidden 4096, 36 layers, 32 / 8 heads × 128, intermediate 12288,
vocabulary 151 665; synthetic GPTQ-INT4 weights), one GPU:

 (a) `embed` (last-token, and mean pooling) against `unified_forward(want_logits=True)` of the same 32 × 256-token batch in the
     same build: host clock around a call that ends in a device synchronise, median of 10 after 3 warm-ups, the three forms
     alternating round by round.  What the embedding call saves is the sampling head: the lm_head GEMM over the vocabulary and
     its logits copy.
 (b) the mean-pool launches alone (ferrum_hip_embed_pool_f16: partial, group where a span has more than 32 chunks, finish)
     over 32 × 256 and 1 × 8192 rows of 4096: µs per call by device events, and bytes ÷ time (rows read once + norm weight + output; the fp32 partials are written and read
     on top and not counted) against the achievable HBM rate of MI355X_MICROARCH.md (≈ 6.3 TB/s).  The row buffers rotate over
     more than the 256 MiB Infinity Cache so that no call re-reads what the last one left on the die.

Usage: exp_embed.py [out.txt] [layers]      (prints the report; writes it to out.txt too when one is named)"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge

DIMS = dict(hidden=4096, num_layers=36, num_heads=32, num_kv_heads=8, head_dim=128, intermediate=12288, vocab=151665,
            has_qk_norm=1, rope_theta=1e6, rms_eps=1e-6)
SEQS, PLEN, WARMUP, REPS = 32, 256, 3, 10
HBM_ACHIEVABLE_GBS = 6300.0


def model_part(pkg, layers, lines):
    d = dict(DIMS, num_layers=layers)
    tokens = SEQS * PLEN
    m = pkg.HipModel(group_size=128, kv_num_blocks=(SEQS + 2) * (PLEN // 16 + 1), max_seqs=SEQS, max_tokens=tokens, max_seq_len=PLEN + 16, **d)
    m.init_synthetic(9271)
    m.finalize()
    rng = np.random.default_rng(1)
    prompts = [rng.integers(256, d["vocab"], size=PLEN).astype(np.uint32) for _ in range(SEQS)]
    items = [(i, p, 0, True) for i, p in enumerate(prompts)]

    def logits():
        m.unified_forward(items, greedy=False, want_logits=True)
        for i in range(SEQS):
            m.release(i)

    forms = {"unified_forward(want_logits)": logits,
             "embed(last)": lambda: m.embed(items, pooling="last", release=True),
             "embed(mean)": lambda: m.embed(items, pooling="mean", release=True)}
    times = {k: [] for k in forms}
    for r in range(WARMUP + REPS):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                                  # (each call ends in a stream synchronise of its own)
            dt = (time.perf_counter() - t0) * 1e3
            if r >= WARMUP:
                times[name].append(dt)
    base = statistics.median(times["unified_forward(want_logits)"])
    lines.append(f"(a) {SEQS} x {PLEN}-token prompts, {layers} layers, one forward per call; ms per call, median of {REPS} after {WARMUP} warm-ups "
                 f"(min .. max), forms alternating")
    for name, ts in times.items():
        med = statistics.median(ts)
        lines.append(f"    {name:30s} {med:9.2f} ms  ({min(ts):.2f} .. {max(ts):.2f})   {med - base:+8.2f} ms against the logits call  ({med / base:.4f} x)")
    del m


def pool_part(pkg, lines):
    H = DIMS["hidden"]
    ctx = pkg.HipBackend.new_context(256 << 20)
    w = (1.0 + 0.1 * torch.randn(H, device="cuda")).half()
    lines.append(f"(b) mean pool alone (final norm, partial / group / finish launches, L2 on), hidden {H}, fp16 rows; µs per call by device events, "
                 f"median of {REPS} windows after {WARMUP}; GB/s = (rows + weight + output bytes) / time; achievable HBM {HBM_ACHIEVABLE_GBS / 1e3:.1f} TB/s")
    for seqs, rows in ((32, 256), (1, 8192)):
        total = seqs * rows
        nbuf = max(2, (768 << 20) // (total * H * 2))             # 768 MiB of rows: three times the Infinity Cache
        bufs = [torch.randn(total, H, device="cuda").half() for _ in range(nbuf)]
        spans = torch.tensor([[i * rows, (i + 1) * rows] for i in range(seqs)], dtype=torch.int32, device="cuda")
        out = torch.empty(seqs, H, dtype=torch.float32, device="cuda")
        calls = 4 * nbuf
        bytes_ = total * H * 2 + H * 2 + seqs * H * 4
        ts = []
        for r in range(WARMUP + REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(calls):
                pkg.HipBackend.embed_pool(ctx, bufs[i % nbuf], spans, w, 1e-6, 1, 1, 0, out, seqs, H)
            e1.record()
            e1.synchronize()
            if r >= WARMUP:
                ts.append(e0.elapsed_time(e1) * 1e3 / calls)
        med = statistics.median(ts)
        gbs = bytes_ / med / 1e3
        lines.append(f"    {seqs:3d} x {rows:5d} rows  {med:8.2f} us  ({min(ts):.2f} .. {max(ts):.2f})   {bytes_ / 2**20:7.1f} MiB  {gbs:8.1f} GB/s  "
                     f"= {gbs / HBM_ACHIEVABLE_GBS:.2f} of achievable HBM")
        del bufs
    ctx.sync()


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    layers = int(sys.argv[2]) if len(sys.argv) > 2 else DIMS["num_layers"]
    assert torch.cuda.is_available(), "needs a GPU: a timing from anywhere else says nothing"
    pkg = ge.load_package()
    pkg.load_library()
    lines = [f"tools/exp_embed.py — Qwen3-Embedding-8B dimensions, synthetic GPTQ-INT4 weights; {torch.cuda.get_device_name(0)}"]
    pool_part(pkg, lines)
    model_part(pkg, layers, lines)
    text = "\n".join(lines)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
