#!/usr/bin/env python3
"""bench.py — decode throughput of the MI355X-native ferrum hot path.

Workload (BASELINE.json metric): Qwen3-30B-A3B GPTQ-INT4 architecture (48 layers, H 2048, 32/4 heads × 128,
128 experts top-8, expert-I 768, V 151936), synthetic GPTQ weights generated on the device (no checkpoints
offline), 256-token random prompts, greedy decode at concurrency c (default 32), KV block 16, fp16 KV.
A "step" = one decode step of the whole batch (c new tokens) through the C++ runner in libferrum_hip.so
(hipGraph replay); `value` = output tokens/s summed over all GPUs.  Per SURVEY.md §8(e) the reference does
not shard this MoE config, so N GPUs run N independent replicas ("scaling": "weak").

A plain run sets up, warms up, times the `--steps` steps and prints the line.  `--full` also measures everything else: the
whole 128-step workload window (`e2e_tok_s`, `vs_baseline`), per-kernel and roofline figures, the c sweep and TTFT, the
closed-loop serve driver, the CPU baseline and the tensor-parallel extras below.  `--dump-outputs DIR` writes the sampled
token ids of the last timed step to DIR (inputs are seeded: two builds can be compared output for output).

Tensor parallel (the dense BASELINE configs): with N > 1 ranks a `--full` launch ALSO times
Llama-3 70B GPTQ-INT4 (configs[4]) as ONE tensor-parallel group of N ranks — per-rank shards (heads, kv heads
and intermediate ÷ N), RCCL all-reduce after o_proj and down_proj captured inside the per-rank decode hipGraph —
and reports it under `tp_scaling` (N = 2 adds Gemma-3 27B, configs[3]); N = 1 reports the same models unsharded,
the base of the scaling curve.  `--model llama3-70b --tp N` makes that TP run the headline line instead
("scaling": "strong").

Launch: `python bench.py --gpus 1` or
`python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

QWEN3_30B_A3B = dict(num_layers=48, hidden=2048, num_heads=32, num_kv_heads=4, head_dim=128, intermediate=0,
                     vocab=151936, has_qk_norm=1, activation=0, num_experts=128, top_k=8, expert_inter=768,
                     norm_topk_prob=1, rms_eps=1e-6, rope_theta=1e6)
LLAMA31_8B = dict(num_layers=32, hidden=4096, num_heads=32, num_kv_heads=8, head_dim=128, intermediate=14336,
                  vocab=128256, has_qk_norm=0, activation=0, num_experts=0, top_k=0, expert_inter=0, norm_topk_prob=0,
                  rms_eps=1e-5, rope_theta=5e5)
# BASELINE configs[3]/[4] are TP=2 / TP=8 on the reference's 24 GB cards; one 288 GB MI355X holds them whole, so they are
# benchable here at TP=1 (extra workloads, not the metric).
GEMMA3_27B = dict(num_layers=62, hidden=5376, num_heads=32, num_kv_heads=16, head_dim=128, intermediate=21504, vocab=262208,
                  has_qk_norm=1, activation=1, num_experts=0, top_k=0, expert_inter=0, norm_topk_prob=0, rms_eps=1e-6,
                  rope_theta=1e6, rope_scaling_kind=1, rope_p0=8.0, sliding_window=1024, sliding_window_pattern=6,
                  sandwich_norms=1, embed_scale=73.5, rope_local_theta=10000.0,
                  desc_act=1)    # the GPTQ pack BASELINE names is act-order: every dense projection gets a row permutation
LLAMA3_70B = dict(num_layers=80, hidden=8192, num_heads=64, num_kv_heads=8, head_dim=128, intermediate=28672, vocab=128256,
                  has_qk_norm=0, activation=0, num_experts=0, top_k=0, expert_inter=0, norm_topk_prob=0, rms_eps=1e-5,
                  rope_theta=5e5)
MODELS = {"qwen3-30b-a3b": QWEN3_30B_A3B, "llama31-8b": LLAMA31_8B, "gemma3-27b": GEMMA3_27B, "llama3-70b": LLAMA3_70B}
BASELINE_CFG_INDEX = {"qwen3-30b-a3b": 2, "llama31-8b": 1, "gemma3-27b": 3, "llama3-70b": 4}
MFMA_PEAK_TFLOPS = 2500.0     # dense fp16 MFMA peak (MI355X_MICROARCH.md)
HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
TP_EXTRA_DEADLINE_S = 420   # multi-GPU runs: the tensor- / expert-parallel extras may take this long before the line goes out without them


def shard_cfg(cfg, world, rank):
    """Per-rank config of a tensor-parallel group (tensor_parallel.rs:209-262): query heads, kv heads and the MLP
    intermediate are divided by the world size; hidden, vocabulary and norms are replicated."""
    d = dict(cfg)
    if world > 1 and d["num_experts"] > 0:
        # MoE (beyond the reference, which does not shard this config): experts split over the ranks; attention tensor-parallel
        # when the kv heads divide (expert_parallel 1), else replicated on every rank (2)
        assert d["num_experts"] % world == 0, f"num_experts={d['num_experts']} not divisible by {world}"
        mode = 1 if d["num_kv_heads"] % world == 0 else 2
        if mode == 1:
            d["num_heads"] //= world
            d["num_kv_heads"] //= world
        d.update(tp_rank=rank, tp_world=world, expert_parallel=mode, vocab_parallel=1)
    elif world > 1:
        for k in ("num_heads", "num_kv_heads", "intermediate"):
            assert d[k] % world == 0, f"{k}={d[k]} not divisible by tp={world}"
            d[k] //= world
        assert (d["intermediate"] % 128) == 0 and (d["num_heads"] * d["head_dim"]) % 128 == 0, "row-parallel shards must cut on quant groups"
        d.update(tp_rank=rank, tp_world=world, vocab_parallel=1)     # lm_head rows sharded too: per-rank argmax pairs are gathered
    return d


def build_model(pkg, cfg, c, max_seq_len, prefill_tokens, seed, layers=None):
    d = dict(cfg)
    if layers:
        d["num_layers"] = layers
    # act-order (desc_act) pack: random row permutations on the synthetic projections (read by init_synthetic; single GPU only —
    # a real desc_act pack cannot be row-sharded without requantising, so the tensor-parallel runs keep natural-order packs)
    desc_act = bool(d.pop("desc_act", 0)) and d.get("tp_world", 1) <= 1
    blocks = (c + 2) * ((max_seq_len + 15) // 16)
    m = pkg.HipModel(group_size=128, kv_num_blocks=blocks, max_seqs=max(c, 1), max_tokens=max(prefill_tokens, c),
                     max_seq_len=max_seq_len, **d)
    prev = os.environ.get("FERRUM_HIP_SYNTH_DESC_ACT")
    if desc_act:
        os.environ["FERRUM_HIP_SYNTH_DESC_ACT"] = "1"
    try:
        m.init_synthetic(seed)
    finally:
        if desc_act and prev is None:
            del os.environ["FERRUM_HIP_SYNTH_DESC_ACT"]
    m.finalize()
    return m


def prefill(model, prompts, first_id, chunk_tokens, ttft_ms=None):
    """Whole-prompt prefill in batches of ≤ chunk_tokens query tokens; returns the first sampled tokens.
    ttft_ms (list) receives, per prompt, the time from the start of the call to its first token (all prompts are
    submitted together, like a closed-loop client at concurrency len(prompts))."""
    out = []
    per = max(1, chunk_tokens // len(prompts[0]))
    t0 = time.perf_counter()
    if len(prompts[0]) > chunk_tokens:                                  # long prompts: one sequence at a time, chunk_tokens per forward
        for i, p in enumerate(prompts):
            for o in range(0, len(p), chunk_tokens):
                last = o + chunk_tokens >= len(p)
                toks, _ = model.unified_forward([(first_id + i, p[o:o + chunk_tokens], o, last)], greedy=True)
            out.append(int(toks[0]))
            if ttft_ms is not None: ttft_ms.append((time.perf_counter() - t0) * 1e3)
        return np.array(out, np.uint32)
    for i in range(0, len(prompts), per):
        items = [(first_id + i + j, p, 0, True) for j, p in enumerate(prompts[i:i + per])]
        toks, _ = model.unified_forward(items, greedy=True)        # returns after the tokens are on the host
        out.extend(int(t) for t in toks)
        if ttft_ms is not None:
            ttft_ms.extend([(time.perf_counter() - t0) * 1e3] * len(items))
    return np.array(out, np.uint32)


def attention_long_ctx(pkg, cfg, c, kv_len):
    """Decode paged attention alone (paged_batched_decode_attention through the C ABI) on c sequences of kv_len keys with the
    model's head geometry: HIP-event time per launch and achieved K+V GB/s.  The pool is rotated over three copies so the
    256 MiB Infinity Cache cannot serve it."""
    import torch
    B = pkg.HipBackend
    ctx = B.new_context()
    nq, nkv, hd = cfg["num_heads"], cfg["num_kv_heads"], cfg["head_dim"]
    nb = (kv_len + 15) // 16
    pools = [(torch.randn(c * nb * nkv * 16 * hd, device="cuda").half(), torch.randn(c * nb * nkv * 16 * hd, device="cuda").half())
             for _ in range(3)]
    tables = torch.from_numpy(np.random.default_rng(0).permutation(c * nb).astype(np.int32).reshape(c, nb)).cuda()
    lens = torch.full((c,), kv_len, dtype=torch.int32, device="cuda")
    q = torch.randn(c, nq, hd, device="cuda").half()
    out = torch.empty_like(q)

    def run(i):
        k, v = pools[i % 3]
        B.paged_batched_decode_attention(ctx, q, k, v, out, tables, lens, c, kv_len, nq, nkv, hd, 16, nb)
    for i in range(3):
        run(i)
    ctx.sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)   # the context launches on torch's current stream
    n = 30
    e0.record()
    for i in range(n):
        run(i)
    e1.record()
    e1.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / n
    byts = c * kv_len * nkv * hd * 2 * 2
    return {"c": c, "kv_len": kv_len, "avg_us": round(us, 2), "bytes": byts, "gbs": round(byts / us / 1e3, 1),
            "peak": HBM_PEAK_GBS, "frac": round(byts / us / 1e3 / HBM_PEAK_GBS, 4)}


def attention_prefill_long_prompt(pkg, cfg, q_len):
    """Prefill paged attention alone (paged_varlen_attention through the C ABI) on one fresh q_len-token prompt with the
    model's head geometry: HIP-event time per launch and achieved TFLOP/s (4·nq·hd flops per causal query-key pair)."""
    import torch
    B = pkg.HipBackend
    ctx = B.new_context()
    nq, nkv, hd = cfg["num_heads"], cfg["num_kv_heads"], cfg["head_dim"]
    nb = (q_len + 15) // 16
    k = torch.randn(nb * nkv * 16 * hd, device="cuda").half()
    v = torch.randn(nb * nkv * 16 * hd, device="cuda").half()
    tables = torch.arange(nb, dtype=torch.int32, device="cuda").reshape(1, nb)
    cu = torch.tensor([0, q_len], dtype=torch.int32, device="cuda")
    po = torch.zeros(1, dtype=torch.int32, device="cuda")
    q = torch.randn(q_len, nq, hd, device="cuda").half()
    out = torch.empty_like(q)

    def run():
        B.paged_varlen_attention(ctx, q, k, v, out, cu, po, tables, 1, q_len, q_len, nq, nkv, hd, 0, 16, nb, q_len)
    for _ in range(2):
        run()
    ctx.sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 10
    e0.record()
    for _ in range(n):
        run()
    e1.record()
    e1.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / n
    fl = 4.0 * nq * hd * q_len * (q_len + 1) / 2
    return {"prompt_len": q_len, "avg_us": round(us, 1), "tflops": round(fl / us / 1e6, 1), "peak_tflops": MFMA_PEAK_TFLOPS,
            "frac": round(fl / us / 1e6 / MFMA_PEAK_TFLOPS, 4)}


def moe_gemm_bytes(cfg, blocks, tokens, which):
    """Algorithmic HBM bytes of one MoE grouped-GEMM launch: every routed expert's INT4
    weights + fp16 group scales once, plus the fp16 activations in and out."""
    H, I, K = cfg["hidden"], cfg["expert_inter"], cfg["top_k"]
    P = tokens * K
    if which == "moe_gate_up":
        w = H * 2 * I // 2 + (H // 128) * 2 * I * 2
        act = tokens * H * 2 + P * I * 2
    else:
        w = I * H // 2 + (I // 128) * H * 2
        act = P * I * 2 + P * H * 2
    return blocks * w + act


def usable_cores():
    """CPUs this process may actually run on: the affinity mask, cut to the cgroup's cpu.max quota when there is one."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(seed=1, prompt=24, n_dec=16):
    """the reference's CPU path (restated in C under oracle/: f64-accumulating GEMM, ONE thread like
    cpu.rs:483-491) at BASELINE configs[0]'s shape — Qwen3-0.6B dims, all 28 layers, V 151936, tied lm_head, synthetic
    weights — greedy decode at c=1.  §8(d) names a 256-token prompt + 128 decode tokens; that is ≈ 200 s of one core, so the
    timed sample is BOUNDED: a `prompt`-token prefill, then `n_dec` decode tokens (≈ 15-25 s); the rate is per decode token
    at kv ≈ prompt + n_dec/2 (attention is < 1 % of a CPU token at these lengths; the GEMMs do not depend on kv)."""
    from oracle import oracle as O
    O.set_threads(1)
    t_build = time.time()
    L, H, nq, nkv, hd, I, V = 28, 1024, 16, 8, 128, 3072, 151936
    rng = np.random.default_rng(seed)
    om = O.OracleModel(num_layers=L, hidden=H, num_heads=nq, num_kv_heads=nkv, head_dim=hd, intermediate=I, vocab=V,
                       max_seq_len=400, has_qk_norm=1, num_experts=0, top_k=0, expert_inter=0, norm_topk_prob=0, rms_eps=1e-6,
                       rope_theta=1e6)
    om.set_global("embed", (rng.standard_normal((V, H)) * 0.02).astype(np.float32))
    om.set_global("final_norm", np.ones(H, np.float32))      # lm_head tied to embed (llama_family.rs:969-1001)

    def gptq(k, n, s):
        qw, sc, qz = O.make_synthetic_gptq(k, n, 128, s, symmetric=True)
        return qw, sc / np.float32(0.28 * np.sqrt(k)), qz
    qd, kvd = nq * hd, nkv * hd
    ws = {"qkv": (H, qd + 2 * kvd, gptq(H, qd + 2 * kvd, 11)), "o": (qd, H, gptq(qd, H, 12)),
          "gate_up": (H, 2 * I, gptq(H, 2 * I, 13)), "down": (I, H, gptq(I, H, 14))}    # same tensors in every layer: timing only
    for li in range(L):
        for name in ("input_ln", "post_ln"):
            om.set_layer_dense(li, name, np.ones(H, np.float32))
        om.set_layer_dense(li, "q_norm", np.ones(hd, np.float32))
        om.set_layer_dense(li, "k_norm", np.ones(hd, np.float32))
        for name, (k, n, t) in ws.items():
            om.set_gptq(li, name, *t, 128, k, n)
    build_s = time.time() - t_build
    toks = rng.integers(256, V, size=prompt).astype(np.uint32)
    t0 = time.perf_counter()
    om.forward(0, toks, 0)
    t_prefill = time.perf_counter() - t0
    t0 = time.perf_counter()
    for i in range(n_dec):
        om.forward(0, np.array([toks[i % prompt]], np.uint32), prompt + i)
    t_tok = (time.perf_counter() - t0) / n_dec
    # the same model and loop with the oracle's OpenMP row loops on every core this process may use (the reference's CPU lane
    # is one thread; this is the "what if its GEMV were threaded" figure — same arithmetic, bit-identical logits)
    cores = usable_cores()
    O.set_threads(cores)
    om.forward(0, np.array([toks[0]], np.uint32), prompt + n_dec)              # thread-pool start-up outside the timed loop
    # with every core the whole protocol of SURVEY.md 8(d) fits the budget: a 256-token prompt, then 128 decode tokens (cache 1)
    P2, D2 = (256, 128) if cores >= 4 else (prompt, 2 * n_dec)
    toks2 = rng.integers(256, V, size=P2).astype(np.uint32)
    t0 = time.perf_counter()
    om.forward(1, toks2, 0)
    t_pre2 = time.perf_counter() - t0
    t0 = time.perf_counter()
    for i in range(D2):
        om.forward(1, np.array([toks2[i % P2]], np.uint32), P2 + i)
    t_par = (time.perf_counter() - t0) / D2
    O.set_threads(1)
    all_cores = {"value": round(1.0 / t_par, 4), "unit": "tok/s", "cores": cores, "kind": "port",
                 "e2e_tok_s": round(D2 / (t_pre2 + D2 * t_par), 4),
                 "sample": f"same model, OpenMP over the GEMM / GEMV output rows on {cores} threads, the protocol of SURVEY 8(d): "
                           f"{P2}-token prefill ({t_pre2:.1f} s) then {D2} decode tokens timed ({t_par * 1e3:.0f} ms/token)"}
    return {"value": round(1.0 / t_tok, 4), "unit": "tok/s", "cores": 1, "kind": "port", "all_cores": all_cores,
            "sample": f"oracle C restatement of the reference CPU path, BASELINE configs[0] shape (Qwen3-0.6B dims: 28 layers, H 1024, "
                      f"16/8 heads x 128, I 3072, V 151936, tied lm_head; synthetic weights), c=1, 1 thread: {prompt}-token prefill "
                      f"({t_prefill:.1f} s) then {n_dec} decode tokens timed ({t_tok * 1e3:.0f} ms/token) - a bounded sample of SURVEY 8(d)'s "
                      f"256-prompt + 128-decode run (≈ {t_tok * 384:.0f} s at this rate); setup {build_s:.0f} s",
            "host_cpus": os.cpu_count()}


def _dist_dev(dist):
    """Device of the tensors handed to torch.distributed: the GPU under nccl (= RCCL), the host under gloo (the one-GPU
    rehearsal, where every rank shares device 0 and RCCL would refuse the second rank)."""
    return "cuda" if dist.get_backend() == "nccl" else "cpu"


def tp_decode_case(pkg, torch, dist, model_name, world, rank, c, PL, steps, warm, chunk, try_oneshot=True, transport="rccl", layers=None,
                   last_tokens=None):
    """One tensor-parallel group of `world` ranks (this process = rank `rank`) decoding `c` sequences of a dense model:
    per-rank shards, a communicator per rank (RCCL shared through a broadcast unique id; or, transport "oneshot", only the
    hand-written peer reduce over hipIpc buffers), prefill, `warm` + `steps` decode steps through the per-rank hipGraph
    (all-reduces captured).  Returns the whole-group rate (the slowest rank's time); `last_tokens` (a list), when given,
    receives the ids the last timed step sampled."""
    cfg = shard_cfg(MODELS[model_name], world, rank)
    max_seq_len = ((PL + 2 * (warm + steps) + 8 + 15) // 16) * 16
    t0 = time.perf_counter()
    model = build_model(pkg, cfg, c, max_seq_len, min(chunk, c * PL), 9271, layers=layers)   # same seed on every rank: replicated tensors agree
    comm = None
    if world > 1 and transport == "oneshot":
        # decode AND prefill all-reduces go through the peer buffers: they must hold the largest prefill message
        need = min(chunk, c * PL) * cfg["hidden"] * 2
        assert need <= (64 << 20), f"one-shot buffer of {need} bytes: lower --prefill-chunk"
        comm = pkg.Comm.bare(world, rank)
        hs = [None] * world
        dist.all_gather_object(hs, comm.oneshot_export(max(need, 1 << 20)))
        comm.oneshot_attach(hs)
        model.set_comm(comm)
    elif world > 1:
        uid = torch.zeros(128, dtype=torch.uint8, device=_dist_dev(dist))
        if rank == 0:
            uid.copy_(torch.frombuffer(bytearray(pkg.Comm.unique_id()), dtype=torch.uint8))
        dist.broadcast(uid, 0)
        comm = pkg.Comm.rccl(world, rank, bytes(uid.cpu().numpy().tobytes()))
        model.set_comm(comm)
    build_s = time.perf_counter() - t0

    def barrier():
        torch.cuda.synchronize()
        if dist is not None and world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    rng = np.random.default_rng(9271)                          # identical prompts on every rank of the group
    prompts = [rng.integers(256, cfg["vocab"], size=PL).astype(np.uint32) for _ in range(c)]

    def run(first_id):
        torch.cuda.synchronize()
        tp0 = time.perf_counter()
        first = prefill(model, prompts, first_id, chunk)
        t_prefill = time.perf_counter() - tp0
        ids = list(range(first_id, first_id + c))
        nxt = model.decode_steps(ids, first, warm)[-1] if warm > 0 else first
        barrier()
        t0 = time.perf_counter()
        out = model.decode_steps(ids, nxt, steps)
        torch.cuda.synchronize()
        t_local = time.perf_counter() - t0
        barrier()
        t = torch.tensor([t_local, t_prefill], dtype=torch.float64, device=_dist_dev(dist) if (dist is not None and world > 1) else "cpu")
        if dist is not None and world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        for sid in ids:
            model.release(sid)
        return float(t[0].item()), float(t[1].item()), out

    t_dec, t_pre, out = run(0)
    if last_tokens is not None:
        last_tokens.append(out[-1].copy())
    res = {"model": model_name, "tp": world, "concurrency": c, "steps": steps, "warmup": warm, "tok_s": round(c * steps / t_dec, 1),
           "ms_per_step": round(t_dec / steps * 1e3, 4), "prefill_ms": round(t_pre * 1e3, 2), "build_s": round(build_s, 1),
           "allreduce": ("none (TP=1)" if world == 1 else
                         "one-shot peer reduce over hipIpc buffers (rank-ordered fp32 sum), captured in the per-rank decode hipGraph" if transport == "oneshot"
                         else "RCCL ncclAllReduce fp16, in place, captured in the per-rank decode hipGraph"),
           "per_rank_shapes": {"num_heads": cfg["num_heads"], "num_kv_heads": cfg["num_kv_heads"], "intermediate": cfg["intermediate"],
                               **({"experts": cfg["num_experts"] // world, "expert_parallel": cfg.get("expert_parallel", 0)} if cfg["num_experts"] else {})}}
    if world > 1:
        # every rank must have sampled the same ids (identical all-reduced activations, replicated lm_head)
        chk = torch.tensor([int(np.asarray(out, np.int64).sum() % (1 << 31))], dtype=torch.int64, device=_dist_dev(dist))
        lo, hi = chk.clone(), chk.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        res["ranks_agree_on_ids"] = bool(lo.item() == hi.item())
    if world > 1 and transport == "oneshot":
        st = comm.oneshot_status()
        tmo = torch.tensor([st["timeouts"]], dtype=torch.int64, device=_dist_dev(dist))
        dist.all_reduce(tmo, op=dist.ReduceOp.MAX)
        res["oneshot_timeouts"] = int(tmo.item())
        res["oneshot_epochs"] = st["epoch"]
    if world > 1 and try_oneshot and transport == "rccl":
        # the hand-written one-shot peer all-reduce over hipIpc-imported buffers (opt-in: every spin is bounded, a rank that
        # cannot see its peers counts a timeout and the attempt is reported as failed instead of hanging)
        try:
            handle = comm.oneshot_export(4 << 20)
            hs = [None] * world
            dist.all_gather_object(hs, handle)
            comm.oneshot_attach(hs)
            os.environ["FERRUM_HIP_TP_ONESHOT"] = "1"
            pkg.load_library().ferrum_hip_debug_reload_knobs()
            model.set_comm(comm)                               # drops the captured graph: the next capture takes the one-shot kernel
            t_dec1, _, out1 = run(10000)
            st = comm.oneshot_status()
            tmo = torch.tensor([st["timeouts"]], dtype=torch.int64, device=_dist_dev(dist))
            dist.all_reduce(tmo, op=dist.ReduceOp.MAX)
            res["oneshot"] = {"tok_s": round(c * steps / t_dec1, 1), "ms_per_step": round(t_dec1 / steps * 1e3, 4),
                              "timeouts": int(tmo.item()), "ids_equal_to_rccl_run": bool(np.array_equal(out, out1)),
                              "transport": "one-shot peer reduce over hipIpc buffers (rank-ordered fp32 sum), in the decode hipGraph"}
        except Exception as e:                                  # reported, never fatal: RCCL is the measured default
            res["oneshot"] = {"error": str(e)[:300]}
        finally:
            os.environ.pop("FERRUM_HIP_TP_ONESHOT", None)
            pkg.load_library().ferrum_hip_debug_reload_knobs()
    del model
    if comm is not None:
        comm.destroy()
    return res


def dump_outputs(dirname, rank, tokens):
    """--dump-outputs: what the timed path hands its caller in its last step — the sampled id of every sequence — as float64
    (ids are exact).  One file per rank: replicas decode prompts of their own."""
    os.makedirs(dirname, exist_ok=True)
    name = "decode_tokens" if rank == 0 else f"decode_tokens_rank{rank}"
    np.save(os.path.join(dirname, name + ".npy"), np.asarray(tokens, np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--concurrency", type=int, default=32)
    ap.add_argument("--prompt-len", type=int, default=256)
    ap.add_argument("--prefill-chunk", type=int, default=8192, help="query tokens per prefill forward (MoE padding and tile tails shrink with larger chunks: 2048 → 8192 tokens is 100 → 77 ms for 32 × 256-token prompts)")
    ap.add_argument("--layers", type=int, default=0, help="debug: fewer layers (result is then NOT the metric)")
    ap.add_argument("--model", default="qwen3-30b-a3b", choices=sorted(MODELS),
                    help="default = BASELINE.json's metric config; llama31-8b = configs[1] (dense), reported as an extra workload")
    ap.add_argument("--tp", type=int, default=0, help="with a dense --model: run it as ONE tensor-parallel group of this many ranks "
                    "(= --gpus) and make that the headline line (\"scaling\": \"strong\")")
    ap.add_argument("--tp-oneshot", action="store_true", help="after the RCCL run, also try the hand-written one-shot peer all-reduce "
                    "over hipIpc buffers (opt-in: unmeasured on multi-GPU hardware so far)")
    ap.add_argument("--tp-transport", default="rccl", choices=("rccl", "oneshot"), help="all-reduce of the tensor-parallel runs: RCCL over xGMI "
                    "(default) or only the hand-written one-shot peer reduce over hipIpc buffers")
    ap.add_argument("--no-tp-scaling", action="store_true", help="skip the dense tensor-parallel extra (tp_scaling)")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--full", action="store_true", help="also measure what the headline does not need: the whole 128-step window, "
                    "per-kernel / roofline / north-star kernel figures, the c sweep and TTFT, the serve loop, the CPU baseline and the "
                    "tensor-parallel extras (the --no-* options above trim this set)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write the ids the last timed step sampled to "
                    "DIR/decode_tokens.npy (float64, one per sequence; rank r > 0: decode_tokens_rank<r>.npy)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    import torch
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1 or "RANK" in os.environ:               # launched by torch.distributed.run (any world size)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    import __graft_entry__ as ge
    pkg = ge.load_package()
    pkg.load_library()
    cfg = dict(MODELS[args.model])
    moe = cfg["num_experts"] > 0
    c, K, W, PL = args.concurrency, args.steps, args.warmup, args.prompt_len
    OUT_LEN = 128                                              # BASELINE workload: 256 in / 128 out
    max_seq_len = ((max(PL + W + K, PL + OUT_LEN) + 8 + 15) // 16) * 16
    chunk = args.prefill_chunk
    if args.tp:
        assert args.tp == world and not moe, "--tp N needs --gpus N ranks and a dense --model (SURVEY.md 8e: the MoE config is replicas only)"

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    prefill_ms = {}
    ttft_by_c = {}

    def run_case(model, conc, steps, warm, first_id):
        rng = np.random.default_rng(9271 + rank)               # seed of the reference's bench-serve command
        prompts = [rng.integers(256, cfg["vocab"], size=PL).astype(np.uint32) for _ in range(conc)]
        torch.cuda.synchronize()
        tp0 = time.perf_counter()
        tt = []
        first = prefill(model, prompts, first_id, chunk, tt)
        prefill_ms[conc] = (time.perf_counter() - tp0) * 1e3   # all `conc` prompts prefilled (≤ chunk tokens per forward)
        ttft_by_c[conc] = float(np.median(tt))
        ids = list(range(first_id, first_id + conc))
        warm_toks = model.decode_steps(ids, first, warm) if warm > 0 else None
        nxt = warm_toks[-1] if warm > 0 else first
        barrier()
        t0 = time.perf_counter()
        toks = model.decode_steps(ids, nxt, steps)
        torch.cuda.synchronize()
        t_local = time.perf_counter() - t0
        barrier()
        return t_local, PL + warm + steps, toks[-1]

    _last_stage = ["start"]

    def stage(name):                                            # FERRUM_BENCH_STAGES=1: progress on stderr (fault triage)
        _last_stage[0] = name
        if os.environ.get("FERRUM_BENCH_STAGES"):
            torch.cuda.synchronize()
            print(f"[bench] {name}", file=sys.stderr, flush=True)

    if args.tp:
        # a dense BASELINE config as ONE tensor-parallel group: the headline line of this invocation
        last = []
        res = tp_decode_case(pkg, torch, dist, args.model, world, rank, c, PL, K, W, min(chunk, 2048), try_oneshot=args.tp_oneshot,
                             transport=args.tp_transport, layers=args.layers or None, last_tokens=last)
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, rank, last[0])
        if rank == 0:
            mname = {"llama31-8b": "Llama-3.1-8B", "gemma3-27b": "Gemma-3-27B", "llama3-70b": "Llama-3-70B"}[args.model]
            print(json.dumps({
                "metric": f"output tok/s at c={c}, {mname} GPTQ-INT4, tensor parallel x{world}, {PL}-token prompts, decode steps timed at kv {PL + W}->{PL + W + K}",
                "value": res["tok_s"], "unit": "tok/s", "n_gpus": world, "steps": K, "warmup": W, "ms_per_step": res["ms_per_step"],
                "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
                "dtype": "int4-weights/f16-activations/f32-accumulate", "data": "synthetic",
                "config": {"workload": f"{mname} GPTQ-INT4 (BASELINE configs[{BASELINE_CFG_INDEX[args.model]}]), one TP group of {world} ranks",
                           "concurrency": c, "prompt_len": PL, "kv_block": 16, "parallelism": f"tp{world}"},
                "tp": res, "rccl_ranks": world if world > 1 else 0}))
        if dist is not None:
            dist.destroy_process_group()
        return

    model = build_model(pkg, cfg, c, max_seq_len, chunk, 9271 + rank, layers=args.layers or None)
    stage("model built")
    t_local, kv_end, last = run_case(model, c, K, W, 0)
    stage("timed decode done")
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, rank, last)
    t = torch.tensor([t_local], dtype=torch.float64, device="cuda")
    if dist is not None:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    t_max = float(t.item())
    value = world * c * K / t_max

    extra = {}
    # the BASELINE workload's whole decode window, whatever --steps says: 128 steps from kv 256 to 384 on fresh sequences
    # (no warm-up steps inside the window; the graph is already captured for this batch size or re-captured at the bucket edge)
    full = None
    if args.full and not args.tp and c * (PL + OUT_LEN) <= 10 ** 7:
        for sid in range(c):
            model.release(sid)
        t_full, _, _ = run_case(model, c, OUT_LEN, 0, 50000)
        tf = torch.tensor([t_full, prefill_ms[c] / 1e3], dtype=torch.float64, device="cuda")
        if dist is not None:
            dist.all_reduce(tf, op=dist.ReduceOp.MAX)
        full = {"steps": OUT_LEN, "kv_len_range": [PL, PL + OUT_LEN], "ms_per_step": round(float(tf[0]) / OUT_LEN * 1e3, 4),
                "decode_tok_s": round(world * c * OUT_LEN / float(tf[0]), 1), "prefill_ms_all_prompts": round(float(tf[1]) * 1e3, 2),
                "e2e_tok_s": round(world * c * OUT_LEN / (float(tf[0]) + float(tf[1])), 1)}
        extra["full_window_256_in_128_out"] = full
        kv_end = PL + OUT_LEN                                  # the index state the per-kernel timings below replay
        for sid in range(50000, 50000 + c):
            model.release(sid)
        stage("full 128-step window done")
    if rank == 0 and args.full:
        # dominant kernel: MoE gate_up grouped INT4 GEMM — live HIP-event timing on the runner's stream
        kernels = {}
        mlp_names = ("moe_gate_up", "moe_down") if moe else ("gate_up", "down")
        for name in mlp_names + ("attention", "qkv", "o", "lm_head"):
            stage(f"time_kernel {name}")
            us, blocks = model.time_kernel(name, c, kv_end, reps=3)
            entry = {"avg_us": round(us, 2)}
            if name.startswith("moe"):
                b = moe_gemm_bytes(cfg, blocks, c, name)
                entry.update(expert_blocks=blocks, bytes=b, gbs=round(b / us / 1e3, 1))
            elif name == "attention":
                mean_kv = kv_end - 0.5
                b = int(c * mean_kv * cfg["num_kv_heads"] * cfg["head_dim"] * 2 * 2 + 2 * c * cfg["num_heads"] * cfg["head_dim"] * 2)
                entry.update(bytes=b, gbs=round(b / us / 1e3, 1))
            elif name in ("qkv", "o", "gate_up", "down"):
                kk, nn = {"qkv": (cfg["hidden"], (cfg["num_heads"] + 2 * cfg["num_kv_heads"]) * cfg["head_dim"]),
                          "o": (cfg["num_heads"] * cfg["head_dim"], cfg["hidden"]),
                          "gate_up": (cfg["hidden"], 2 * cfg["intermediate"]),
                          "down": (cfg["intermediate"], cfg["hidden"])}[name]
                b = kk * nn // 2 + (kk // 128) * nn * 2 + c * (kk + nn) * 2
                entry.update(bytes=b, gbs=round(b / us / 1e3, 1))
            else:
                b = cfg["vocab"] * cfg["hidden"] * 2 + c * cfg["vocab"] * 4
                entry.update(bytes=b, gbs=round(b / us / 1e3, 1))
            kernels[name] = entry
        dom, dom_name = kernels[mlp_names[0]], ("w4_gemm_moe_em_kernel<false,2> (MoE gate_up INT4 grouped GEMM + silu*mul, expert-major)" if moe
                                                else "w4_gemm dense gate_up INT4 GEMM")
        traffic_file = "pmc_traffic_gate_up.json"
        if moe:
            # what the decode step launches since round 3: gate_up (+ silu·mul) AND down as one expert-major launch — the
            # dominant kernel of the step (≈ 55 % of it); its algorithmic bytes are the two GEMMs' (the gated activations are
            # written and read through memory inside the launch, counted on both sides)
            try:
                stage("time_kernel moe_pair")
                us, blocks = model.time_kernel("moe_pair", c, kv_end, reps=3)
                b = moe_gemm_bytes(cfg, blocks, c, "moe_gate_up") + moe_gemm_bytes(cfg, blocks, c, "moe_down")
                kernels["moe_pair"] = {"avg_us": round(us, 2), "expert_blocks": blocks, "bytes": b, "gbs": round(b / us / 1e3, 1)}
                dom, dom_name = kernels["moe_pair"], "w4_gemm_moe_em2_kernel<false, false> (MoE gate_up + silu*mul -> down INT4 grouped GEMMs, one expert-major launch)"
                traffic_file = "pmc_traffic_moe_pair.json"
            except Exception as e:       # batches that do not take the merged form (c < 32): the two-launch kernels above stand
                kernels["moe_pair"] = {"unavailable": str(e)[:120]}
        traffic, traffic_src = None, None                       # HBM bytes per launch from the committed PMC passes
        tp = os.path.join(ROOT, "profiles", traffic_file)
        if moe and c == 32 and os.path.exists(tp):
            traffic = json.load(open(tp)).get("traffic_bytes_per_launch")
            traffic_src = f"committed profile profiles/{traffic_file} (separate --pmc FETCH_SIZE / WRITE_SIZE passes of this command)"
        extra["roofline"] = {"bound": "hbm", "kernel": dom_name,
                             "achieved": dom["gbs"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": round(dom["gbs"] / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_src,
                             "bytes_per_launch": dom["bytes"], "avg_launch_us": dom["avg_us"]}
        extra["kernels"] = kernels
        # whole-step roofline: weights touched + KV + lm_head per step
        L = model.cfg.num_layers
        step_bytes = L * (kernels[mlp_names[0]]["bytes"] + kernels[mlp_names[1]]["bytes"] + kernels["attention"]["bytes"] +
                          kernels["qkv"]["bytes"] + kernels["o"]["bytes"]) + kernels["lm_head"]["bytes"]
        extra["step_roofline"] = {"bytes_per_step": int(step_bytes), "achieved_gbs": round(step_bytes / (t_max / K) / 1e9, 1),
                                  "frac": round(step_bytes / (t_max / K) / 1e9 / HBM_PEAK_GBS, 4)}
        # BASELINE.json's two stated kernel targets, measured live (HIP events) where the workload makes them meaningful:
        #  * INT4 GEMM on MFMA — the prefill form of the qkv projection at `chunk` rows (decode GEMMs are HBM-bound, above);
        #    the matrix-pipe busy fraction of the same launch comes from the committed PMC pass (profiles/)
        #  * paged-attention decode against the HBM roofline at a context long enough to leave the latency floor
        #    (c sequences × 4096 keys; the 256-in/128-out workload itself holds 22 MB of KV per layer)
        ns = {}
        if chunk <= model.cfg.max_tokens and chunk >= 1024:
            us, _ = model.time_kernel("qkv", chunk, kv_end, reps=2)
            kk, nn = cfg["hidden"], (cfg["num_heads"] + 2 * cfg["num_kv_heads"]) * cfg["head_dim"]
            tf = 2.0 * chunk * kk * nn / us / 1e6
            ns["int4_gemm_prefill"] = {"kernel": f"w4_gemm_big_kernel (96/128/256-row tiles, scale folded into the fp16 B operand) qkv {kk}->{nn}, M={chunk}",
                                       "avg_us": round(us, 2),
                                       "tflops": round(tf, 1), "peak_tflops": MFMA_PEAK_TFLOPS, "frac": round(tf / MFMA_PEAK_TFLOPS, 4)}
            if not cfg.get("num_experts"):            # dense model: the widest projection too (Llama-3.1-8B: 4096 -> 28672)
                us2, _ = model.time_kernel("gate_up", chunk, kv_end, reps=2)
                k2, n2 = cfg["hidden"], 2 * cfg["intermediate"]
                tf2 = 2.0 * chunk * k2 * n2 / us2 / 1e6
                ns["int4_gemm_prefill_gate_up"] = {"kernel": f"w4_gemm_big_kernel gate_up {k2}->{n2}, M={chunk}", "avg_us": round(us2, 2),
                                                   "tflops": round(tf2, 1), "peak_tflops": MFMA_PEAK_TFLOPS, "frac": round(tf2 / MFMA_PEAK_TFLOPS, 4)}
            mp = os.path.join(ROOT, "profiles", "pmc_mfma_busy.json")
            if os.path.exists(mp):
                ns["int4_gemm_prefill"]["mfma_busy_pmc"] = dict(json.load(open(mp)), source_kind="committed profile (profiles/pmc_mfma_busy.json), not measured by this run")
        stage("north-star: attention decode at long context")
        ns["attention_decode_long_ctx"] = attention_long_ctx(pkg, cfg, c, 4096)
        stage("north-star: attention prefill, long prompt")
        ns["attention_prefill_long_prompt"] = attention_prefill_long_prompt(pkg, cfg, 4096)
        stage("north-star kernels done")
        extra["north_star_kernels"] = ns
        for sid in range(c):
            model.release(sid)
        if not args.no_sweep and world == 1:
            sweep = {str(c): round(value, 1)}
            ttft = []
            for conc in (1, 4, 16):
                tl, _, _ = run_case(model, conc, min(K, 32), 4, 1000 * conc)
                sweep[str(conc)] = round(conc * min(K, 32) / tl, 1)
                for s in range(1000 * conc, 1000 * conc + conc):
                    model.release(s)
            rng = np.random.default_rng(1)
            for i in range(5):                                 # TTFT: 256-token prompt, idle engine (c=1)
                p = rng.integers(256, cfg["vocab"], size=PL).astype(np.uint32)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.unified_forward([(5000 + i, p, 0, True)], greedy=True)
                ttft.append((time.perf_counter() - t0) * 1e3)
                model.release(5000 + i)
            extra["sweep_tok_s"] = sweep
            extra["ttft_ms_p50_c1"] = round(float(np.median(ttft)), 2)
            extra["prefill_ms_all_prompts"] = {str(k): round(v, 2) for k, v in sorted(prefill_ms.items())}
            # p50 time-to-first-token when all c prompts arrive together (BASELINE.md quotes the reference's per-c TTFT)
            extra["ttft_ms_p50_by_c"] = {str(k): round(v, 2) for k, v in sorted(ttft_by_c.items())}
        if not args.no_sweep and world == 1 and args.model in ("qwen3-30b-a3b", "llama31-8b") and not args.layers:
            # the reference's own measurement shape (`ferrum bench-serve`: closed loop, 96 requests, 256-in/128-out, c in
            # flight) driven by the C++ continuous-batching loop over the C ABI (csrc/serve_loop.cc) in its own process
            exe = os.path.join(ROOT, "ferrum-infer-rs_amd", "bin", "ferrum_hip_serve")
            import subprocess
            # the child is not to be profiled when this process runs under rocprofv3 (its preloaded tool crashed in the
            # child at exit): drop the profiler's environment
            env = {k: v for k, v in os.environ.items()
                   if not (k.startswith(("ROCP", "ROCPROF")) or (k in ("LD_PRELOAD", "HSA_TOOLS_LIB") and "rocprof" in v.lower()))}

            def serve(budget):
                cmd = [exe, "--requests", "96", "--concurrency", str(c), "--prompt-len", str(PL), "--out-len", "128",
                       "--max-batched-tokens", str(budget)] + (["--dense"] if args.model == "llama31-8b" else [])
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
                if p.returncode != 0:
                    raise RuntimeError(f"ferrum_hip_serve failed: {p.stderr[-500:]}")
                return json.loads(p.stdout.strip().splitlines()[0])
            # two token budgets per engine iteration: the reference's own default (DEFAULT_MAX_BATCHED_TOKENS = 2048,
            # ferrum-cli/src/gpu_mem_autosize.rs:25: prompts are admitted 8 at a time, so the median request gets its first
            # token early) and one forward for all 32 prompts (highest throughput, every request waits for the whole prefill)
            extra["serve_closed_loop"] = serve(2048)
            extra["serve_closed_loop_one_prefill_forward"] = serve(chunk)
        if not args.no_cpu_baseline and world == 1:
            stage("cpu baseline")
            extra["cpu_baseline"] = cpu_baseline()

    num_layers_run = model.cfg.num_layers

    def make_line():
        # BASELINE.md's published c=32 number for this model (RTX 4090, ferrum 0.7.7 gate, `ferrum bench-serve`: output
        # tokens over the whole 256-in/128-out run, i.e. prefill included).  `value` is the decode-loop rate BASELINE.md
        # line 52 defines; `e2e_tok_s` is the serve-like form (prefill of all prompts + 128 decode steps) for a like-for-like ratio.
        ref_c32 = 706.0 if moe else 745.6          # the reference publishes c=32 numbers for configs[2] and configs[1] only
        e2e = None
        if full is not None:
            # like-for-like with the reference's bench-serve number (prefill included): all c prompts prefilled, then the whole
            # 128-step window
            e2e = full["e2e_tok_s"]
            extra["e2e_tok_s"] = e2e
            if args.model in ("qwen3-30b-a3b", "llama31-8b"):
                extra["e2e_vs_baseline"] = round(e2e / ref_c32, 2)
                extra["decode_only_vs_baseline"] = round(value / ref_c32, 2)
        if moe:
            extra["baseline"] = {"value": ref_c32, "unit": "tok/s", "hardware": "1x RTX 4090 (reference CUDA lane)",
                                 "source": "BASELINE.md table row 'Qwen3-30B-A3B-GPTQ-Int4 output tok/s (0.7.7 gate)', c=32"}
        is_metric = args.model == "qwen3-30b-a3b" and c == 32 and num_layers_run == cfg["num_layers"] and not args.tp
        mname = {"qwen3-30b-a3b": "Qwen3-30B-A3B", "llama31-8b": "Llama-3.1-8B", "gemma3-27b": "Gemma-3-27B",
                 "llama3-70b": "Llama-3-70B"}[args.model]
        if args.model == "llama31-8b":
            extra["baseline"] = {"value": 745.6, "unit": "tok/s", "hardware": "1x RTX 4090 (reference CUDA lane)",
                                 "source": "BASELINE.md row 'Llama-3.1-8B-Instruct-GPTQ-INT4 output tok/s', c=32"}
        # `value` = the K timed decode steps (kv window below); `vs_baseline` compares like with like: the reference's 706 tok/s
        # is a bench-serve number with prefill inside, so the ratio uses e2e_tok_s (prefill of all prompts + the whole
        # 128-step window), not the decode-only rate.  RTX 4090 vs MI355X: context, not a same-hardware comparison.
        line = {"metric": f"output tok/s at c={c}, {mname} GPTQ-INT4, {PL}-token prompts, decode steps timed at kv {PL + W}->{PL + W + K}",
                "value": round(value, 1),
                "unit": "tok/s", "n_gpus": world, "steps": K, "warmup": W, "ms_per_step": round(t_max / K * 1e3, 4),
                "higher_is_better": True, "scaling": "weak",
                "vs_baseline": round(e2e / ref_c32, 2) if (is_metric and e2e) else None,
                "dtype": "int4-weights/f16-activations/f32-accumulate",
                "data": "synthetic",
                "config": {"workload": f"{mname} GPTQ-INT4 (BASELINE configs[{BASELINE_CFG_INDEX[args.model]}]), TP=1 per GPU, replicas across GPUs",
                           "concurrency": c, "prompt_len": PL, "kv_len_range": [PL + W, PL + W + K], "kv_block": 16,
                           "layers": num_layers_run, "parallelism": f"replica x{world}",
                           **({"desc_act": True} if cfg.get("desc_act") else {})}}
        line.update(extra)
        return line

    emitted = []                                                # the one JSON line, whichever path prints it

    def emit():
        if rank == 0 and not emitted:
            emitted.append(1)
            print(json.dumps(make_line()), flush=True)

    # ── tensor-parallel / expert-parallel extras (collective: every rank takes part) ─────────────
    # They run AFTER everything the headline needs has been measured, under a watchdog: a multi-GPU collective that never
    # completes (these paths have not run on a multi-GPU node yet) must cost the extras, not the line — past the deadline rank 0
    # prints the line without them and every rank leaves.
    if args.full and not args.no_tp_scaling and not args.layers and args.model == "qwen3-30b-a3b" and world in (1, 2, 4, 8):
        import threading

        def bail_out():
            # the line still goes out (the headline was measured before the extras), but the process leaves with a non-zero
            # code: a hung collective must show in the run record, not only as a string inside the JSON
            extra.setdefault("tp_scaling", {"error": f"the tensor-parallel extra did not finish within {TP_EXTRA_DEADLINE_S} s",
                                            "stage": _last_stage[0]})
            emit()
            os._exit(3)
        watchdog = threading.Timer(TP_EXTRA_DEADLINE_S, bail_out) if world > 1 else None
        if watchdog:
            watchdog.daemon = True
            watchdog.start()
        for sid in range(50000, 50000 + c):
            model.release(sid)
        del model
        model = None
        torch.cuda.empty_cache()
        try:
            tps = []
            for name in ["llama3-70b"] + (["gemma3-27b"] if world == 2 else []):
                stage(f"tp_scaling {name} tp={world}")
                tps.append(tp_decode_case(pkg, torch, dist, name, world, rank, c, PL, min(K, 32), min(W, 4) if W else 2, 2048,
                                          try_oneshot=args.tp_oneshot, transport=args.tp_transport))
            extra["tp_scaling"] = tps
            extra["rccl_ranks"] = world if world > 1 else 0
            if world > 1:
                # beyond the reference: the headline model as ONE expert-parallel group of all ranks — experts
                # sharded, partial MoE outputs all-reduced — next to the replica headline above
                stage(f"ep_scaling qwen3-30b-a3b x{world}")
                extra["ep_scaling"] = tp_decode_case(pkg, torch, dist, "qwen3-30b-a3b", world, rank, c, PL, min(K, 32), min(W, 4) if W else 2, 2048,
                                                     try_oneshot=False, transport=args.tp_transport)
        except Exception as e:                                  # reported in the line, never fatal to it
            extra.setdefault("tp_scaling", {"error": str(e)[:400]})
            extra["tp_extra_error"] = str(e)[:400]
        if watchdog:
            watchdog.cancel()

    emit()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
