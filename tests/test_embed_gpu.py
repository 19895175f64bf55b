"""Embeddings on the GPU: the tail kernel element by element against the float64 restatement and bound of
tests/embed_bounds.py, its batch invariance bit for bit, and ferrum_hip_model_embed against the logits path, the CPU model,
chunked prefill, the prefix cache and the KV life cycle.

The op-level inputs share one layout per hidden size: spans of 1, 15, 16, 17, 65 and 3 rows, one span that is a single all-zero
row and one mean span of three chunks (length from csrc/embed_plan.h), laid out in another order than the span list with a gap
of 1e4-filled rows between them — a kernel that reads a row outside its span, or pools spans in row order, lands far outside
the bound.  Every output is NaN before the call and is followed by a guard row that must stay NaN."""
import functools
import os
import re

import numpy as np
import pytest

from tests import embed_bounds as eb
from tests import parity_bounds as pb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-6
SPAN_LENS = [1, 15, 16, 17, 65, 3]
GAP = 2
WORST = {}


def _chunk_rows():
    src = open(os.path.join(ROOT, "ferrum-infer-rs_amd", "csrc", "embed_plan.h")).read()
    return int(re.search(r"EMBED_CHUNK_ROWS\s*=\s*(\d+)", src).group(1))


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as ge
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    pkg = ge.load_package()
    pkg.load_library()          # raises if the HIP extension is missing — no fallback
    ctx = pkg.HipBackend.new_context(64 << 20)
    yield pkg, ctx, torch
    ctx.sync()
    print("\nembed_pool, largest err/tol: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


@functools.lru_cache(maxsize=None)
def _inputs(H):
    """(x16 [rows, H] fp16-valued, x32 [rows, H] fp32-valued, w [H], spans [(begin, end)], index of the zero span, of the long one)."""
    rng = np.random.default_rng(1000 + H)
    lens = SPAN_LENS + [1, 2 * _chunk_rows() + 1]                # … the all-zero row, the smallest span of three chunks
    zero_span, long_span = len(SPAN_LENS), len(SPAN_LENS) + 1
    order = [4, 7, 0, 6, 2, 5, 1, 3]                            # where each span lies in memory: not the span order
    assert sorted(order) == list(range(len(lens)))
    spans, at = [None] * len(lens), GAP
    for i in order:
        spans[i] = (at, at + lens[i])
        at += lens[i] + GAP
    x = np.full((at, H), 1e4)
    body, kinds = pb.norm_rows(rng, sum(lens), H, start=3)
    assert set(kinds) == set(pb.ROW_KINDS)
    used = 0
    for b, e in spans:
        x[b:e] = body[used:used + e - b]
        used += e - b
    x[spans[zero_span][0]] = 0.0
    x16 = pb.f16r(x)
    x32 = np.asarray(x16 * (1.0 + 2.0 ** -13), np.float32)      # values fp16 cannot hold
    return x16, x32, pb.mixed_sign_weight(rng, H), spans, zero_span, long_span


def _run(env, x, w, spans, pooling, normalize, dims):
    """The op on device copies of x [rows, H] (float16 or float32 array) → fp32 [len(spans), d]; checks the NaN guard row."""
    pkg, ctx, torch = env
    H = x.shape[1]
    d = dims or H
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    wd = None if w is None else torch.from_numpy(np.asarray(w, np.float16)).cuda()
    sd = torch.from_numpy(np.asarray(spans, np.int32).reshape(-1, 2)).cuda()
    out = torch.full((len(spans) + 1, d), float("nan"), dtype=torch.float32, device="cuda")
    pkg.HipBackend.embed_pool(ctx, xd, sd, wd, EPS, pooling, normalize, dims, out, len(spans), H)
    ctx.sync()
    got = out.cpu().numpy()
    assert np.isnan(got[-1]).all(), "the guard row behind the output was written"
    return got[:-1]


@pytest.mark.parametrize("with_w", [True, False], ids=["w", "now"])
@pytest.mark.parametrize("dims", [0, 32, 100])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("pooling", [0, 1, 2])
@pytest.mark.parametrize("dtype", ["f16", "f32"])
@pytest.mark.parametrize("H", [256, 5376, 8192])
def test_embed_pool_elementwise(env, H, dtype, pooling, normalize, dims, with_w):
    x16, x32, w, spans, zero_span, _ = _inputs(H)
    x = x16.astype(np.float16) if dtype == "f16" else x32
    got = _run(env, x, w if with_w else None, spans, pooling, normalize, dims)
    ref, tol = eb.ref_tol(x, w if with_w else None, EPS, spans, pooling, normalize, dims)
    what = f"embed_pool H={H} {dtype} pooling={pooling} normalize={normalize} dims={dims} w={with_w}"
    worst = pb.assert_within(ref, tol, got, what)
    WORST[dtype + (" mean" if pooling == 1 else " row")] = max(WORST.get(dtype + (" mean" if pooling == 1 else " row"), 0.0), worst)
    assert (got[zero_span] == 0).all(), what


def test_embed_pool_is_batch_invariant_and_repeatable(env):
    H = 5376
    x16, _, w, spans, _, long_span = _inputs(H)
    x = x16.astype(np.float16)
    for pooling, normalize in ((1, 1), (1, 0), (0, 1), (2, 1)):
        ragged = _run(env, x, w, spans, pooling, normalize, 0)
        again = _run(env, x, w, spans, pooling, normalize, 0)
        assert ragged.tobytes() == again.tobytes(), f"pooling {pooling}: a second launch gave other bits"
        for i, span in enumerate(spans):
            alone = _run(env, x, w, [span], pooling, normalize, 0)
            assert alone[0].tobytes() == ragged[i].tobytes(), f"pooling {pooling}: span {i} {span} differs alone and in the ragged launch"
    assert spans[long_span][1] - spans[long_span][0] > 2 * _chunk_rows()


def _plan_constant(name):
    src = open(os.path.join(ROOT, "ferrum-infer-rs_amd", "csrc", "embed_plan.h")).read()
    return int(re.search(name + r"\s*=\s*(\d+)", src).group(1))


@pytest.mark.parametrize("dtype", ["f16", "f32"])
@pytest.mark.parametrize("H", [256, 5376])
def test_embed_pool_long_spans_take_the_second_level(env, H, dtype):
    """Spans either side of the chunk count from which a span's partials are summed in groups first (csrc/embed_plan.h): the
    element-wise bound, and each span alone bit-identical to itself in the launch."""
    rows, above, group = _chunk_rows(), _plan_constant("EMBED_REDUCE_ABOVE"), _plan_constant("EMBED_REDUCE_GROUP")
    lens = [rows * above, rows * above + 1, rows * (above + group) + 5, 7]       # 32 chunks: one level; 33 and 49: two; a short one
    rng = np.random.default_rng(2000 + H)
    spans, at = [], 1
    for n in lens:
        spans.append((at, at + n))
        at += n + 1
    x, _ = pb.norm_rows(rng, at, H, start=1)
    w = pb.mixed_sign_weight(rng, H)
    x = x.astype(np.float16) if dtype == "f16" else np.asarray(x * (1.0 + 2.0 ** -13), np.float32)
    for normalize in (0, 1):
        got = _run(env, x, w, spans, 1, normalize, 0)
        ref, tol = eb.ref_tol(x, w, EPS, spans, 1, normalize, 0)
        worst = pb.assert_within(ref, tol, got, f"embed_pool long spans H={H} {dtype} normalize={normalize}")
        WORST[dtype + " mean, two levels"] = max(WORST.get(dtype + " mean, two levels", 0.0), worst)
        for i, span in enumerate(spans):
            alone = _run(env, x, w, [span], 1, normalize, 0)
            assert alone[0].tobytes() == got[i].tobytes(), f"span {i} {span} differs alone and in the launch"


# ── the model call ──────────────────────────────────────────────────────────
@pytest.fixture(scope="module")
def pkg(env):
    return env[0]


def _cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((a * b).sum() / (np.sqrt((a * a).sum() * (b * b).sum()) + 1e-300))


def _assert_close(got, ref, what):
    """The project's model-level bar (modelgen.Parity defaults): cosine > 0.999 per vector, max |got − ref| ≤ 2e-2·max |ref|."""
    from tests import modelgen
    bar = modelgen.Parity(what)
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    for j in range(len(ref)):
        c = _cos(got[j], ref[j])
        err = float(np.max(np.abs(got[j] - ref[j])))
        assert c > bar.cos_min, f"{what} vector {j}: cosine {c}"
        assert err <= bar.rel_max * float(np.max(np.abs(ref[j]))), f"{what} vector {j}: max err {err} against max |ref| {np.max(np.abs(ref[j]))}"


def test_model_embed_last_token_agrees_with_the_logits_path(pkg):
    from tests import modelgen
    tm = modelgen.TinyModel(False, layers=2, seed=11)
    hm = tm.hip_model(pkg)
    H, V = tm.cfg["hidden"], tm.cfg["vocab"]
    assert hm.embedding_dim() == H
    rng = np.random.default_rng(12)
    prompts = [rng.integers(0, V, size=n).astype(np.uint32) for n in (19, 33)]
    free0 = hm.kv_slot_capacity_snapshot()["free_blocks"]
    _, Lg = hm.unified_forward([(1 + i, p, 0, True) for i, p in enumerate(prompts)], greedy=False, want_logits=True)
    for i in range(2):
        hm.release(1 + i)
    e = hm.embed([(11 + i, p, 0, True) for i, p in enumerate(prompts)], pooling="last", normalize=False, release=True)
    assert e.shape == (2, H) and e.dtype == np.float32
    # both heads norm the same residual rows (prefill is bit-repeatable); the logits path rounds its normed row to fp16 (2^-11
    # per element, with the norm's own allowance on either side) before an fp32-out GEMM of H terms
    ref, absdot = pb.gemm_refs(e, tm.glob["lm_head"])
    tol = 2.0 ** -24 * np.abs(ref) + (H * 2.0 ** -23 + 2.0 ** -11 + 2 * pb.norm_scale_allowance(H)) * absdot + 2.0 ** -149
    print("logits against embedding · lm_head, max err/tol:", pb.assert_within(ref, tol, Lg, "logits path against the embedding"))
    e64 = e.astype(np.float64)
    n = hm.embed([(21 + i, p, 0, True) for i, p in enumerate(prompts)], pooling="last", normalize=True, release=True)
    cut = hm.embed([(31 + i, p, 0, True) for i, p in enumerate(prompts)], pooling="last", normalize=True, dims=64, release=True)
    assert cut.shape == (2, 64)
    for j in range(2):
        pb.assert_within(*eb.l2_ref_tol(e64[j], np.zeros(H)), n[j], f"normalised embedding {j}")
        pb.assert_within(*eb.l2_ref_tol(e64[j, :64], np.zeros(64)), cut[j], f"dims=64 embedding {j}")
    assert hm.kv_slot_capacity_snapshot()["free_blocks"] == free0


def _cpu_embeddings(tm, om, prompts, pooling):
    """Last layer's residual rows from the CPU model's taps; final norm, pooling and L2 in float64."""
    w = np.asarray(tm.glob["final_norm"], np.float64)
    out = []
    for i, p in enumerate(prompts):
        om.forward(i, p, 0)
        rows = np.asarray(om.taps(len(p))[-1], np.float64)
        n = pb.rms_norm_ref64(rows, w, tm.cfg["rms_eps"])[0]
        v = {"last": n[-1], "first": n[0], "mean": n.mean(0)}[pooling]
        out.append(v / max(np.sqrt((v * v).sum()), 1e-12))
        om.release(i)
    return np.stack(out)


# the last two are the smallest models whose one-token batches take the one-launch decode chain (chain.hip) — there the last
# layer's tail must have run inside that layer when the pool reads the residual stream
_CHAIN = dict(hidden=2048, nq=32, nkv=4, hd=128, vocab=2048, max_seq_len=64)
MODEL_CASES = {
    "dense-qk-norm": dict(moe=False, kw=dict(qk_norm=True)),
    "moe": dict(moe=True, kw={}),
    "sandwich-f32-residual": dict(moe=False, kw=dict(sandwich=True, activation=1, embed_scale=4.0, mlp_down_first=True)),
    "dense-chain": dict(moe=False, kw=dict(inter=2048, qk_norm=False, rope_theta=500000.0, **_CHAIN), chain=("decode_chain", "dense_chain")),
    "moe-chain": dict(moe=True, kw=dict(experts=32, top_k=4, expert_inter=256, **_CHAIN), chain=("decode_chain",)),
}


@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_model_embed_follows_the_cpu_model(pkg, case, forms):
    from tests import modelgen
    spec = MODEL_CASES[case]
    tm = modelgen.TinyModel(spec["moe"], layers=2, seed=21, **spec["kw"])
    hm, om = tm.hip_model(pkg), tm.oracle_model()
    om.enable_taps(64)
    V = tm.cfg["vocab"]
    free0 = hm.kv_slot_capacity_snapshot()["free_blocks"]
    rng = np.random.default_rng(22)
    ragged = [rng.integers(0, V, size=n).astype(np.uint32) for n in (7, 19, 33)]
    ones = [rng.integers(0, V, size=1).astype(np.uint32) for _ in range(4)]           # the decode-shaped batch
    sid = 1
    for name, prompts in (("ragged", ragged), ("one-token", ones)):
        if name == "ragged" and "chain" in spec:
            continue                                                                   # (the chain cases are about the one-token batch)
        for pooling in ("last", "mean", "first"):
            forms.reset()
            got = hm.embed([(sid + i, p, 0, True) for i, p in enumerate(prompts)], pooling=pooling, release=True)
            if name == "one-token":
                forms.require(*spec.get("chain", ()))
            sid += len(prompts)
            _assert_close(got, _cpu_embeddings(tm, om, prompts, pooling), f"{case} {name} {pooling}")
    assert hm.kv_slot_capacity_snapshot()["free_blocks"] == free0


def test_model_embed_chunks_prefix_cache_release_and_errors(pkg):
    from tests import modelgen
    tm = modelgen.TinyModel(False, layers=2, seed=31)
    hm = tm.hip_model(pkg)
    H, V = tm.cfg["hidden"], tm.cfg["vocab"]
    rng = np.random.default_rng(32)
    p = rng.integers(0, V, size=40).astype(np.uint32)
    free0 = hm.kv_slot_capacity_snapshot()["free_blocks"]
    whole = hm.embed([(1, p, 0, True)], pooling="last", release=True)
    assert hm.kv_slot_capacity_snapshot()["free_blocks"] == free0      # release=1 gave the blocks back …
    with pytest.raises(RuntimeError):
        hm.block_table(1)                                              # … and the sequence is unknown
    # chunks 16 + 24: the first only fills the cache
    assert hm.embed([(2, p[:16], 0, False)], pooling="last").shape == (0, H)
    # mean / first over a chunked sequence: refused before anything is reserved
    free1 = hm.kv_slot_capacity_snapshot()["free_blocks"]
    for pooling in ("mean", "first"):
        with pytest.raises(RuntimeError, match="item 0"):
            hm.embed([(2, p[16:], 16, True)], pooling=pooling)
        assert hm.kv_slot_capacity_snapshot()["free_blocks"] == free1 and hm.block_table(2)[1] == 16
    with pytest.raises(RuntimeError, match="dims"):
        hm.embed([(2, p[16:], 16, True)], pooling="last", dims=H + 1)
    assert hm.kv_slot_capacity_snapshot()["free_blocks"] == free1 and hm.block_table(2)[1] == 16
    chunked = hm.embed([(2, p[16:], 16, True)], pooling="last")       # release=0 …
    _assert_close(chunked, whole, "chunks 16 + 24 against the single item")
    assert hm.block_table(2)[1] == 40
    toks = hm.decode_steps([2], [int(p[0])], 2)                       # … leaves a sequence the decode loop continues
    assert toks.shape == (2, 1) and hm.block_table(2)[1] == 42
    hm.release(2)
    # prefix cache: the second request of the same prompt finds two full blocks and embeds the rest
    def run(seq_id):
        hm.reserve_kv_slots([(seq_id, len(p))])
        cached = hm.prefix_cache_acquire(seq_id, p)
        got = hm.embed([(seq_id, p[cached:], cached, True)], pooling="last")
        hm.prefix_cache_register(seq_id, p, cached)
        hm.release(seq_id)
        return cached, got
    c0, first = run(3)
    c1, second = run(4)
    assert (c0, c1) == (0, 32)
    _assert_close(first, whole, "prefix-cache miss against the single item")
    _assert_close(second, whole, "prefix-cache hit against the single item")
