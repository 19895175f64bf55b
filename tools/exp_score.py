#!/usr/bin/env python3
"""The scoring path at Qwen3-30B-A3B dimensions (hidden 2048, 48 layers, 32 / 4 heads × 128, 128 experts top-8 of 768,
vocabulary 151 936; synthetic GPTQ-INT4 weights), one GPU:

 (a) the op alone (ferrum_hip_logprob_rows_f32: partial, merge and gather launches) over m = 1 / 32 / 256 rows of 151 936 fp32
     logits with one pair per row: µs per call by device events, and bytes ÷ time (the logits read once; the partials, 12 bytes
     per 4096 logits, are not counted) against the achievable HBM rate of MI355X_MICROARCH.md (≈ 6.3 TB/s).  The logits buffers
     rotate over more than the 256 MiB Infinity Cache so that no call re-reads what the last one left on the die.
 (b) `score` of the last row of each of 32 × 256-token items against `unified_forward(want_logits=True)` of the same batch in
     the same build — the gap is the logits copy-back the scoring call saves — and `score` of every row (8192 rows, the default
     256 rows per lm_head pass) against the same forward with no targets — the gap is the cost of the head, 32 lm_head passes.
     Host clock around a call that ends in a device synchronise, median of 10 after 3 warm-ups, the forms alternating round by
     round.

Usage: exp_score.py [out.txt] [layers]      (prints the report; writes it to out.txt too when one is named)"""
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

DIMS = dict(num_layers=48, hidden=2048, num_heads=32, num_kv_heads=4, head_dim=128, intermediate=0, vocab=151936, has_qk_norm=1,
            activation=0, num_experts=128, top_k=8, expert_inter=768, norm_topk_prob=1, rms_eps=1e-6, rope_theta=1e6)
SEQS, PLEN, WARMUP, REPS = 32, 256, 3, 10
HBM_ACHIEVABLE_GBS = 6300.0


def op_part(pkg, lines):
    V = DIMS["vocab"]
    ctx = pkg.HipBackend.new_context(8 << 20)
    lines.append(f"(a) the op alone (partial / merge / gather launches), n = {V} fp32 logits, one pair per row; µs per call by device events, "
                 f"median of {REPS} windows after {WARMUP} (min .. max); GB/s = logits bytes / time; achievable HBM {HBM_ACHIEVABLE_GBS / 1e3:.1f} TB/s")
    for m in (1, 32, 256):
        nbuf = max(2, (768 << 20) // (m * V * 4))                 # 768 MiB of logits: three times the Infinity Cache
        bufs = [torch.randn(m, V, device="cuda") for _ in range(nbuf)]
        rows = torch.arange(m, dtype=torch.int32, device="cuda")
        toks = torch.randint(0, V, (m,), dtype=torch.int32, device="cuda")
        out = torch.empty(m, dtype=torch.float32, device="cuda")
        lse = torch.empty(m, dtype=torch.float32, device="cuda")
        top = torch.empty(m, dtype=torch.int32, device="cuda")
        calls = max(4 * nbuf, 64)
        ts = []
        for r in range(WARMUP + REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(calls):
                pkg.HipBackend.logprob_rows(ctx, bufs[i % nbuf], rows, toks, out, lse, top)
            e1.record()
            e1.synchronize()
            if r >= WARMUP:
                ts.append(e0.elapsed_time(e1) * 1e3 / calls)
        med = statistics.median(ts)
        gbs = m * V * 4 / med / 1e3
        print(f"op m={m} done", flush=True)
        lines.append(f"    m = {m:3d}  {med:8.2f} us  ({min(ts):.2f} .. {max(ts):.2f})   {m * V * 4 / 2**20:7.1f} MiB  {gbs:8.1f} GB/s  "
                     f"= {gbs / HBM_ACHIEVABLE_GBS:.2f} of achievable HBM   ({nbuf} buffers in rotation)")
        del bufs
    ctx.sync()


def model_part(pkg, layers, lines):
    d = dict(DIMS, num_layers=layers)
    tokens = SEQS * PLEN
    m = pkg.HipModel(group_size=128, kv_num_blocks=(SEQS + 2) * (PLEN // 16 + 1), max_seqs=SEQS, max_tokens=tokens, max_seq_len=PLEN + 16, **d)
    m.init_synthetic(9271)
    m.finalize()
    print("model ready", flush=True)
    rng = np.random.default_rng(1)
    prompts = [rng.integers(256, d["vocab"], size=PLEN).astype(np.uint32) for _ in range(SEQS)]
    items = [(i, p, 0, True) for i, p in enumerate(prompts)]
    last = [(i, PLEN - 1, int(p[0])) for i, p in enumerate(prompts)]
    every = [(i, r, int(p[(r + 1) % PLEN])) for i, p in enumerate(prompts) for r in range(PLEN)]

    def logits():
        m.unified_forward(items, greedy=False, want_logits=True)
        for i in range(SEQS):
            m.release(i)

    def scorer(targets):
        """The C arrays built once: the clock holds the call, not the marshalling of 8192 targets in Python."""
        from ferrum_infer_rs_amd.executor import BatchItem, ScoreOptions, ScoreTarget, TokenScore
        arr = (BatchItem * SEQS)(*[BatchItem(i, p.ctypes.data_as(C.POINTER(C.c_uint32)), PLEN, 0, 1, 0) for i, p in enumerate(prompts)])
        tg = (ScoreTarget * max(len(targets), 1))(*[ScoreTarget(*t, 0) for t in targets])
        out, opts = (TokenScore * max(len(targets), 1))(), ScoreOptions(0, 1)

        def run():
            rc = m.lib.ferrum_hip_model_score(m.h, arr, SEQS, tg, len(targets), C.byref(opts), out)
            assert rc == 0, m.lib.ferrum_hip_last_error()
        return run

    forms = {"unified_forward(want_logits)": logits,
             "score(last row of each item)": scorer(last),
             "score(no targets)": scorer([]),
             "score(every row)": scorer(every)}
    times = {k: [] for k in forms}
    for r in range(WARMUP + REPS):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                                  # (each call ends in a stream synchronise of its own)
            dt = (time.perf_counter() - t0) * 1e3
            if r >= WARMUP:
                times[name].append(dt)
        print(f"round {r} done", flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    lines.append(f"(b) {SEQS} x {PLEN}-token items, {layers} layers, one forward per call; ms per call, median of {REPS} after {WARMUP} warm-ups "
                 f"(min .. max), forms alternating")
    for name, ts in times.items():
        lines.append(f"    {name:30s} {med[name]:9.2f} ms  ({min(ts):.2f} .. {max(ts):.2f})")
    lines.append(f"    last rows against the logits call: {med['score(last row of each item)'] - med['unified_forward(want_logits)']:+.2f} ms; "
                 f"every row against no targets: {med['score(every row)'] - med['score(no targets)']:+.2f} ms for {tokens} rows in "
                 f"{tokens // 256} passes of 256")
    del m


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    layers = int(sys.argv[2]) if len(sys.argv) > 2 else DIMS["num_layers"]
    assert torch.cuda.is_available(), "needs a GPU: a timing from anywhere else says nothing"
    pkg = ge.load_package()
    pkg.load_library()
    lines = [f"tools/exp_score.py — Qwen3-30B-A3B dimensions, synthetic GPTQ-INT4 weights; {torch.cuda.get_device_name(0)}"]
    op_part(pkg, lines)
    model_part(pkg, layers, lines)
    text = "\n".join(lines)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
