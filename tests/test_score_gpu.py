"""Scoring on the GPU: the op (csrc/score_head.hip) element by element against the float64 restatement and the derived bound of
tests/score_bounds.py, its batch independence bit for bit, and ferrum_hip_model_score against the device's own logits, the CPU
model, chunked prefill, several lm_head passes and the KV life cycle.

The op-level rows cycle through six kinds (ROW_KINDS): normal; the row maximum planted twice, on the last element of a segment
and the first of the next (on the middle and the last element where the row is one segment) — the first must win; spread over
±80, so most exponentials underflow; all equal (top = 0, lse = x + log n); a third of the entries −inf; all −inf.  The padding
between n and ld holds 1e30: a kernel that reads it lands at infinity.  Outputs hold a sentinel before the call and are
followed by a guard element; the workspace holds 0xFF bytes (NaN patterns)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from tests import score_bounds as sb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_KINDS = ("normal", "seam", "spread", "equal", "third_inf", "all_inf")
SENTINEL = 12345.0
WORST = {}

# (m, n, ld).  4095 / 4096 / 4097 / 8195 are segment − 1 / segment / segment + 1 / 2·segment + 3 of SCORE_SEGMENT = 4096
# (csrc/score_plan.h; test_segment_constant checks it).  (4, 4097, ld = n): an odd ld puts every second row off 16-byte alignment.
OP_SHAPES = [(1, 1, 1), (3, 7, 7), (5, 1000, 1003), (33, 4095, 4095), (33, 4096, 4096), (33, 4097, 4100), (33, 8195, 8195),
             (2, 151936, 151936), (4, 4097, 4097)]


def test_segment_constant():
    src = open(os.path.join(ROOT, "ferrum-infer-rs_amd", "csrc", "score_plan.h")).read()
    assert int(re.search(r"SCORE_SEGMENT\s*=\s*(\d+)", src).group(1)) == sb.SEGMENT == 4096


def seam_columns(n):
    """Where the "seam" rows hold their two equal maxima."""
    if n > sb.SEGMENT:
        return sb.SEGMENT - 1, sb.SEGMENT
    return (n // 2, n - 1) if n >= 2 else (0, 0)


@functools.lru_cache(maxsize=None)
def op_inputs(m, n):
    """(x [m, n] float32, kinds [m], pair_rows, pair_tokens): computed once per shape and never written to."""
    rng = np.random.default_rng(7000 + 31 * m + n)
    x = np.empty((m, n), np.float32)
    kinds = [ROW_KINDS[r % len(ROW_KINDS)] for r in range(m)]
    for r, kind in enumerate(kinds):
        if kind in ("normal", "seam", "third_inf"):
            x[r] = (3.0 * rng.standard_normal(n)).astype(np.float32)
        if kind == "seam":
            a, b = seam_columns(n)
            x[r, a] = x[r, b] = np.float32(np.max(x[r]) + 8.0)
        elif kind == "third_inf":
            x[r, rng.random(n) < 1.0 / 3.0] = -np.inf
            if n >= 2:
                x[r, n - 1] = np.float32(0.5)                       # (something stays)
        elif kind == "spread":
            x[r] = rng.uniform(-80.0, 80.0, n).astype(np.float32)
        elif kind == "equal":
            x[r] = np.float32(1.25)
        elif kind == "all_inf":
            x[r] = -np.inf
    # pairs: one to three tokens on six rows of seven (7 is coprime with the six kinds, so every kind has rows with pairs and,
    # from 42 rows on, rows without), both seam columns on the seam rows, a duplicate, a token ≥ n; shuffled
    rows, toks = [], []
    for r, kind in enumerate(kinds):
        if r % 7 != 6:
            for _ in range(1 + int(rng.integers(0, 3))):
                rows.append(r)
                toks.append(int(rng.integers(0, n)))
        if kind == "seam":
            rows += [r, r]
            toks += list(seam_columns(n))
    rows += [rows[0], 0]
    toks += [toks[0], n]
    order = rng.permutation(len(rows))
    x.setflags(write=False)
    return x, kinds, np.asarray(rows, np.int32)[order], np.asarray(toks, np.int64)[order]


@functools.lru_cache(maxsize=None)
def op_reference(m, n):
    x, _, pr, pt = op_inputs(m, n)
    lse, tol_lse, top = sb.row_ref_tol(x)
    ref, tol = sb.pair_ref_tol(x, lse, tol_lse, pr, pt)
    return lse, tol_lse, top, ref, tol


class _Workspace(C.Structure):                                   # FerrumHipWorkspace (csrc/abi_private.h)
    _fields_ = [("ptr", C.c_void_p), ("bytes", C.c_size_t)]


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as ge
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    pkg = ge.load_package()
    pkg.load_library()          # raises if the HIP extension is missing — no fallback
    ctx = pkg.HipBackend.new_context(8 << 20)
    yield pkg, ctx, torch
    ctx.sync()
    print("\nlogprob_rows, largest err/tol: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def _dirty_workspace(ctx):
    ws = _Workspace.from_address(ctx.ws.value)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    assert hip.hipMemset(ws.ptr, 0xFF, ws.bytes) == 0
    assert hip.hipDeviceSynchronize() == 0


def run_op(env, x, ld, pair_rows, pair_tokens, want_rows=True, dirty=True):
    """The op on a device copy of x laid out with row stride ld → (logprob [pairs], lse [m], top [m]); checks the guards."""
    pkg, ctx, torch = env
    m, n = x.shape
    buf = np.full((m, ld), 1e30, np.float32)
    buf[:, :n] = x
    xd = torch.from_numpy(buf).cuda()
    prd = torch.from_numpy(np.ascontiguousarray(pair_rows, np.int32)).cuda()
    ptd = torch.from_numpy(np.asarray(pair_tokens, np.int64).astype(np.uint32).view(np.int32)).cuda()
    out = torch.full((len(pair_rows) + 1,), SENTINEL, dtype=torch.float32, device="cuda")
    lse = torch.full((m + 1,), SENTINEL, dtype=torch.float32, device="cuda")
    top = torch.full((m + 1,), -7, dtype=torch.int32, device="cuda")
    if dirty:
        _dirty_workspace(ctx)
    pkg.HipBackend.logprob_rows(ctx, xd, prd, ptd, out, lse if want_rows else None, top if want_rows else None, m=m, n=n, ld=ld)
    ctx.sync()
    out, lse, top = out.cpu().numpy(), lse.cpu().numpy(), top.cpu().numpy()
    assert out[-1] == SENTINEL and lse[-1] == SENTINEL and top[-1] == -7, "a guard element behind an output was written"
    if not want_rows:
        assert (lse == SENTINEL).all() and (top == -7).all()
    return out[:-1], lse[:-1], top[:-1].view(np.uint32)


@pytest.mark.parametrize("m,n,ld", OP_SHAPES, ids=[f"{m}x{n}ld{ld}" for m, n, ld in OP_SHAPES])
def test_logprob_rows_elementwise(env, m, n, ld):
    x, kinds, pr, pt = op_inputs(m, n)
    lse_ref, tol_lse, top_ref, ref, tol = op_reference(m, n)
    got, lse, top = run_op(env, x, ld, pr, pt)
    what = f"logprob_rows m={m} n={n} ld={ld}"
    WORST["lse"] = max(WORST.get("lse", 0.0), sb.assert_within(lse_ref, tol_lse, lse, what + " lse"))
    WORST["logprob"] = max(WORST.get("logprob", 0.0), sb.assert_within(ref, tol, got, what + " logprob"))
    assert (top == top_ref).all(), f"{what}: top {top} is not the first maximum {top_ref}"
    assert (got[pt >= n] == -np.inf).all() and (pt >= n).sum() == 1
    for r, kind in enumerate(kinds):
        if kind == "seam":
            assert top[r] == seam_columns(n)[0]
        if kind == "equal":
            assert top[r] == 0 and abs(float(lse[r]) - (1.25 + np.log(n))) <= tol_lse[r]
        if kind == "all_inf":
            in_row = (pr == r) & (pt < n)
            assert in_row.any(), f"{what}: the all -inf row {r} has no pair"
            assert top[r] == 0 and lse[r] == -np.inf and np.isnan(got[in_row]).all()
    # every kind the shape holds has a log-prob under the bound, and (from 7 rows on) some row has no pair at all
    assert {kinds[r] for r, t in zip(pr, pt) if t < n} == set(kinds)
    assert m < 7 or set(range(m)) - set(int(r) for r in pr)
    # without the optional row outputs the pairs are the same bits
    again, _, _ = run_op(env, x, ld, pr, pt, want_rows=False)
    assert again.tobytes() == got.tobytes()


def test_logprob_rows_nan_at_a_seam_stays_in_its_row(env):
    m, n = 5, 8195
    x, _, pr, pt = op_inputs(m, n)
    clean, lse0, top0 = run_op(env, x, n, pr, pt)
    for col in (sb.SEGMENT - 1, sb.SEGMENT, n - 1):
        y = np.array(x)
        y[1, col] = np.nan
        got, lse, top = run_op(env, y, n, pr, pt)
        in_row = (pr == 1) & (pt < n)
        assert in_row.any() and np.isnan(lse[1]) and np.isnan(got[in_row]).all(), f"NaN at column {col} was dropped"
        others = np.arange(m) != 1
        assert lse[others].tobytes() == lse0[others].tobytes() and (top[others] == top0[others]).all()
        assert got[~in_row].tobytes() == clean[~in_row].tobytes()


@pytest.mark.parametrize("n,ld", [(8195, 8195), (4097, 4097), (151936, 151936)])
def test_logprob_rows_is_batch_independent_and_repeatable(env, n, ld):
    """The same rows alone (m = 1), among 3 and among 33, at other positions — with an odd ld at other alignments too — give the
    same bits; so does a second launch."""
    rng = np.random.default_rng(n)
    probe = (3.0 * rng.standard_normal((2, n))).astype(np.float32)
    probe[1, seam_columns(n)[0]] = probe[1, seam_columns(n)[1]] = 20.0
    toks = np.array([0, sb.SEGMENT - 1, sb.SEGMENT, n - 1, 17], np.int64)
    seen = {}
    for m, places in ((1, (0,)), (3, (0, 1, 2)), (33, (0, 7, 32))):
        if n > 100000 and m == 33:
            m, places = 5, (0, 3, 4)                              # (the wide row: five rows hold the same three facts)
        for k in range(2):
            for at in places:
                x = (3.0 * rng.standard_normal((m, n))).astype(np.float32)
                x[at] = probe[k]
                got, lse, top = run_op(env, x, ld, np.full(len(toks), at, np.int32), toks, dirty=False)
                bits = (got.tobytes(), lse[at].tobytes(), int(top[at]))
                assert seen.setdefault(k, bits) == bits, f"row {k} at position {at} of {m} rows differs from its first launch"
    x = (3.0 * rng.standard_normal((3, n))).astype(np.float32)
    a = run_op(env, x, ld, np.array([0, 1, 2], np.int32), toks[:3])
    b = run_op(env, x, ld, np.array([0, 1, 2], np.int32), toks[:3])
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


def test_logprob_rows_refuses_a_short_workspace(env):
    pkg, _, torch = env
    small = pkg.HipBackend.new_context(1024)                      # 33 rows of 8195 need (3 · 33 · 3 + 33) · 4 = 1320 bytes
    x = torch.zeros((33, 8195), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="1320"):
        pkg.HipBackend.logprob_rows(small, x, None, None, None)
    pkg.HipBackend.logprob_rows(small, x[:25], None, None, None)  # 25 rows: 1000 bytes
    small.sync()


# ── the model call ──────────────────────────────────────────────────────────
@pytest.fixture(scope="module")
def pkg(env):
    return env[0]


def _log_softmax64(logits):
    z = np.asarray(logits, np.float64)
    z = z - z.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


@pytest.mark.parametrize("moe", [False, True], ids=["dense", "moe"])
def test_model_score_last_rows_agree_with_the_device_logits(pkg, moe):
    """The sharp one: the same rows in the same order and number as the logits call, so the lm_head GEMM has the same shape and
    the scores must be the float64 log-softmax of the returned logits under the op's derived bound."""
    from tests import modelgen
    tm = modelgen.TinyModel(moe, layers=2, seed=41)
    hm = tm.hip_model(pkg)
    V = tm.cfg["vocab"]
    rng = np.random.default_rng(42)
    prompts = [rng.integers(0, V, size=n).astype(np.uint32) for n in (7, 19, 33)]
    free0 = hm.kv_slot_capacity_snapshot()["free_blocks"]
    _, Lg = hm.unified_forward([(1 + i, p, 0, True) for i, p in enumerate(prompts)], greedy=False, want_logits=True)
    for i in range(3):
        hm.release(1 + i)
    targets = []
    for i, p in enumerate(prompts):
        targets += [(i, len(p) - 1, int(t)) for t in [np.argmax(Lg[i]), np.argmin(Lg[i]), *rng.integers(0, V, size=i)]]
    order = rng.permutation(len(targets))
    targets = [targets[k] for k in order]
    scores = hm.score([(11 + i, p, 0, True) for i, p in enumerate(prompts)], targets, release=True)
    assert hm.kv_slot_capacity_snapshot()["free_blocks"] == free0
    lse, tol_lse, top = sb.row_ref_tol(Lg)
    ref, tol = sb.pair_ref_tol(Lg, lse, tol_lse, [t[0] for t in targets], [t[2] for t in targets])
    worst = sb.assert_within(ref, tol, [s[0] for s in scores], "score against the logits call")
    tref, ttol = sb.pair_ref_tol(Lg, lse, tol_lse, [t[0] for t in targets], [top[t[0]] for t in targets])
    worst = max(worst, sb.assert_within(tref, ttol, [s[1] for s in scores], "top log-prob against the logits call"))
    assert [s[2] for s in scores] == [int(top[t[0]]) for t in targets]
    print("score against the device's own logits, largest err/tol:", worst)


# Every row against the CPU model.  Log-sum-exp is 1-Lipschitz in the max-norm, so |Δ logprob_t| ≤ |Δ x_t| + |Δ lse| ≤
# 2·max_v |Δ logit_v|; the project's model-level bar (modelgen.Parity) allows max_v |Δ logit_v| ≤ 2e-2·max|logit| per row, so the
# tolerance of a row is 2 · 2e-2 · max |o_row|.  top_token is compared exactly and every mismatch counted the Parity way, none
# allowed: the seeds were picked on the CPU so that the CPU model's own smallest top-2 margin over the scored rows is at least
# 1e-2·max|logit| of its row (the value found is recorded per case and asserted), which puts zero within reach of the reference.
MODEL_CASES = {          # seed: of the model; prompts: of the prompt tokens; margin_rel: the smallest top-2 margin the CPU model has there
    "dense": dict(moe=False, kw={}, seed=41, prompts=108, lens=(7, 19, 33), margin_rel=0.01765),
    "moe": dict(moe=True, kw={}, seed=42, prompts=153, lens=(7, 19, 33), margin_rel=0.02229),
    "sandwich-f32-residual": dict(moe=False, kw=dict(sandwich=True, activation=1, embed_scale=4.0, mlp_down_first=True), seed=41, prompts=225,
                                  lens=(7, 19, 33), margin_rel=0.01213),
    "ragged-19-1-7": dict(moe=False, kw={}, seed=41, prompts=110, lens=(19, 1, 7), margin_rel=0.02148),
}
MARGIN_FLOOR = 1e-2


def _against_the_cpu_model(tm, hm, om, what, prompts, chunks=None, max_rows_per_pass=0, rng=None, margin_rel=None):
    """Score every row of every prompt (fed as the given chunks) and compare with the CPU model's all-row logits."""
    from tests import modelgen
    bar = modelgen.Parity(what)
    refs, margins = [], []
    for i, p in enumerate(prompts):
        _, al = om.forward(i, p, 0, all_logits=True)
        om.release(i)
        refs.append(np.asarray(al, np.float64))
        margins += [modelgen.margin(row) / float(np.max(np.abs(row))) for row in al]
    found = min(margins)
    print(f"{what}: the CPU model's smallest top-2 margin over {len(margins)} rows is {found:.4f} of its row's max |logit|")
    assert found >= MARGIN_FLOOR, found
    if margin_rel is not None:
        assert abs(found - margin_rel) <= 5e-2 * margin_rel, (found, margin_rel)      # (the recorded value, up to the CPU build's own rounding)
    got = {}
    for lo, hi in chunks or [(0.0, 1.0)]:
        items, targets, keys = [], [], []
        for i, p in enumerate(prompts):
            a, b = int(round(lo * len(p))), int(round(hi * len(p)))
            if b <= a:
                continue
            items.append((100 + i, p[a:b], a, b == len(p)))
            for r in range(a, b):
                extra = [int(p[r + 1])] if r + 1 < len(p) else []           # the next prompt token: what a perplexity asks for
                for tok in [int(np.argmax(refs[i][r]))] + extra:
                    targets.append((len(items) - 1, r - a, tok))
                    keys.append((i, r, tok))
        if rng is not None:
            order = rng.permutation(len(targets))
            targets, keys = [targets[k] for k in order], [keys[k] for k in order]
        for key, s in zip(keys, hm.score(items, targets, max_rows_per_pass=max_rows_per_pass)):
            got.setdefault(key, s)
            assert got[key] == s, f"{what}: two targets of one (row, token) disagree"
    for i in range(len(prompts)):
        hm.release(100 + i)
    mismatches, worst = [], 0.0
    for (i, r, tok), (lp, top_lp, top) in got.items():
        o = refs[i][r]
        ls = _log_softmax64(o)
        tol = 2 * bar.rel_max * float(np.max(np.abs(o)))
        oi = int(np.argmax(o))
        if top != oi:
            mismatches.append((i, r, oi, top, modelgen.margin(o)))
        assert abs(lp - ls[tok]) <= tol and np.isfinite(lp), f"{what} item {i} row {r} token {tok}: {lp} against {ls[tok]}, tolerance {tol}"
        assert abs(top_lp - ls[oi]) <= tol, f"{what} item {i} row {r}: top log-prob {top_lp} against {ls[oi]}, tolerance {tol}"
        worst = max(worst, abs(lp - ls[tok]) / tol, abs(top_lp - ls[oi]) / tol)
    print(f"{what}: {len(got)} (row, token) pairs, largest err/tol {worst:.3f}, top-token mismatches {mismatches}")
    assert len({(i, r) for i, r, _ in got}) == sum(len(p) for p in prompts)
    assert not mismatches, mismatches


def _case(pkg, case):
    from tests import modelgen
    spec = MODEL_CASES[case]
    tm = modelgen.TinyModel(spec["moe"], layers=2, seed=spec["seed"], **spec["kw"])
    rng = np.random.default_rng(spec["prompts"])
    prompts = [rng.integers(0, tm.cfg["vocab"], size=n).astype(np.uint32) for n in spec["lens"]]
    return tm, tm.hip_model(pkg), tm.oracle_model(), prompts, spec["margin_rel"]


@pytest.mark.parametrize("case", ["dense", "moe", "sandwich-f32-residual"])
def test_model_score_every_row_follows_the_cpu_model(pkg, case):
    tm, hm, om, prompts, margin_rel = _case(pkg, case)
    _against_the_cpu_model(tm, hm, om, case, prompts, margin_rel=margin_rel)


def test_model_score_over_two_chunks(pkg):
    """The sequences fed as two chunks (the second with pos_offset > 0), targets in both."""
    tm, hm, om, prompts, margin_rel = _case(pkg, "dense")
    _against_the_cpu_model(tm, hm, om, "two chunks", prompts, chunks=[(0.0, 0.4), (0.4, 1.0)], margin_rel=margin_rel)


def test_model_score_in_passes_of_three_rows(pkg):
    """max_rows_per_pass = 3 over the 27 distinct rows of items of 19, 1 and 7 tokens, the targets shuffled."""
    tm, hm, om, prompts, margin_rel = _case(pkg, "ragged-19-1-7")
    _against_the_cpu_model(tm, hm, om, "passes of 3", prompts, max_rows_per_pass=3, rng=np.random.default_rng(44), margin_rel=margin_rel)


def test_model_score_life_cycle_and_errors(pkg):
    from tests import modelgen
    from ferrum_infer_rs_amd.backend import Unsupported
    from ferrum_infer_rs_amd.executor import BatchItem, ScoreOptions, ScoreTarget, TokenScore
    tm = modelgen.TinyModel(False, layers=2, seed=51)
    hm = tm.hip_model(pkg)
    V = tm.cfg["vocab"]
    rng = np.random.default_rng(52)
    p = rng.integers(0, V, size=21).astype(np.uint32)
    free0 = hm.kv_slot_capacity_snapshot()["free_blocks"]
    # score(release=False) leaves a sequence the decode loop continues exactly like its twin behind unified_forward
    tok, _ = hm.unified_forward([(1, p, 0, True)], greedy=True)
    (lp, top_lp, top), = hm.score([(2, p, 0, True)], [(0, len(p) - 1, int(tok[0]))])
    assert top == int(tok[0]) and lp == top_lp and hm.block_table(2)[1] == len(p)
    a, b = hm.decode_steps([1], [int(tok[0])], 4), hm.decode_steps([2], [top], 4)
    assert a.tolist() == b.tolist()
    hm.release(1)
    hm.release(2)
    assert hm.kv_slot_capacity_snapshot()["free_blocks"] == free0
    # release=True gives the blocks back; so does a KV-fill call (no targets) with it
    hm.score([(3, p, 0, True), (4, p[:5], 0, False)], [(0, 3, 1), (1, 0, 2)], release=True)
    assert hm.kv_slot_capacity_snapshot()["free_blocks"] == free0
    assert hm.score([(3, p, 0, True)], []) == [] and hm.block_table(3)[1] == len(p)
    hm.release(3)
    assert hm.kv_slot_capacity_snapshot()["free_blocks"] == free0
    # every invalid-argument class: rc 2, the target named, nothing reserved
    items = [(5, p, 0, True), (6, p[:4], 0, True)]
    for targets, word in (([(0, 0, 1), (2, 0, 1)], "target 1"), ([(-1, 0, 1)], "target 0"), ([(1, 4, 1)], "target 0"), ([(1, 0, 1), (0, -1, 1)], "target 1"),
                          ([(0, 0, 1), (0, 1, 2), (1, 3, V)], "target 2")):
        with pytest.raises(RuntimeError, match=word):
            hm.score(items, targets)
    with pytest.raises(RuntimeError, match="max_rows_per_pass"):
        hm.score(items, [(0, 0, 1)], max_rows_per_pass=-1)
    keep = np.ascontiguousarray(p, np.uint32)
    arr = (BatchItem * 1)(BatchItem(7, keep.ctypes.data_as(C.POINTER(C.c_uint32)), len(keep), 0, 1, 0))
    tg, out, opts = (ScoreTarget * 1)(ScoreTarget(0, 0, 1, 0)), (TokenScore * 1)(), ScoreOptions(0, 0)
    lib = hm.lib
    assert lib.ferrum_hip_model_score(hm.h, arr, 1, tg, -1, C.byref(opts), out) == 2 and b"num_targets" in lib.ferrum_hip_last_error()
    assert lib.ferrum_hip_model_score(hm.h, arr, -1, tg, 0, C.byref(opts), out) == 2 and b"num_items" in lib.ferrum_hip_last_error()
    assert lib.ferrum_hip_model_score(hm.h, arr, 1, tg, 1, C.byref(opts), None) == 2 and b"null output" in lib.ferrum_hip_last_error()
    assert lib.ferrum_hip_model_score(hm.h, arr, 1, None, 1, C.byref(opts), out) == 2 and b"null targets" in lib.ferrum_hip_last_error()
    assert lib.ferrum_hip_model_score(hm.h, None, 1, tg, 1, C.byref(opts), out) == 2 and b"null items" in lib.ferrum_hip_last_error()
    assert hm.kv_slot_capacity_snapshot()["free_blocks"] == free0
    for sid in (5, 6, 7):
        with pytest.raises(RuntimeError):
            hm.block_table(sid)                                   # … and no sequence came to be
    # a vocabulary-parallel lm_head is refused as unsupported before anything is reserved
    from tests.test_model_gpu import _tp_rank_models
    rank = _tp_rank_models(pkg, tm, 2, vocab_parallel=1, kv_num_blocks=24, max_seqs=4, max_tokens=128)[0]
    free_r = rank.kv_slot_capacity_snapshot()["free_blocks"]
    with pytest.raises(Unsupported):
        rank.score([(1, p, 0, True)], [(0, 0, 1)])
    assert rank.kv_slot_capacity_snapshot()["free_blocks"] == free_r


def test_loglikelihood_is_the_sum_of_its_scores(pkg):
    from tests import modelgen
    tm = modelgen.TinyModel(False, layers=2, seed=61)
    hm = tm.hip_model(pkg)
    V = tm.cfg["vocab"]
    rng = np.random.default_rng(62)
    ctx_a, ctx_b = [int(t) for t in rng.integers(0, V, size=9)], [int(rng.integers(0, V))]
    cont_b = [int(t) for t in rng.integers(0, V, size=6)]
    free0 = hm.kv_slot_capacity_snapshot()["free_blocks"]
    # request a continues with the one token greedy decoding would produce (learnt from the same batch), request b at random
    items = [(70, ctx_a, 0, True), (71, (ctx_b + cont_b)[:-1], 0, True)]
    (_, _, top_a), = hm.score(items, [(0, len(ctx_a) - 1, 0)], release=True)
    requests = [(ctx_a, [top_a]), (ctx_b, cont_b)]
    ll = hm.loglikelihood(requests)
    assert hm.kv_slot_capacity_snapshot()["free_blocks"] == free0
    targets = [(0, len(ctx_a) - 1, top_a)] + [(1, len(ctx_b) - 1 + k, t) for k, t in enumerate(cont_b)]
    scores = hm.score(items, targets, release=True)                  # the same batch: prefill is bit-repeatable
    for j, (a, b) in enumerate(((0, 1), (1, 1 + len(cont_b)))):
        assert ll[j][0] == float(sum(np.float64(s[0]) for s in scores[a:b]))
        assert ll[j][1] == all(s[2] == t[2] for s, t in zip(scores[a:b], targets[a:b]))
    assert ll[0][1] is True and ll[0][0] < 0 and ll[1][0] < ll[0][0]
    with pytest.raises(ValueError):
        hm.loglikelihood([([], [1])])
    assert hm.kv_slot_capacity_snapshot()["free_blocks"] == free0
