"""The expert pair resolving its rows from the router's per-part candidate lists (form `moe_pair_rank_lists`: role B of the
decode chain stops at the lists, every tile of the merged gate_up → down launch ranks its own expert's candidates) against
the in-chain merge (FERRUM_HIP_MOE_PAIR_RANK_LISTS=0) at Qwen3-30B-A3B's dimensions: the same pairs, the same combine
weights and the same logits BIT FOR BIT — both forms pick by the one order of route_merge.h and the weights come from the
same arithmetic — in single forwards and in the hipGraph loop."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIMS = dict(hidden=2048, nq=32, nkv=4, hd=128, experts=128, top_k=8, expert_inter=768)      # Qwen3-30B-A3B
LAYERS, VOCAB, PLEN, STEPS, GRAPH_STEPS = 3, 2048, 5, 3, 4
# expert counts that are no multiple of 16 · parts: the router splits them by whole 16-expert tiles, so the last part is short
# ([0,16) [16,32) [32,48) [48,60), and [0,16) [16,24)); two quant groups per down projection, the fewest the pair takes
SHORT_LAST_PART = {"e60": dict(experts=60, top_k=4, expert_inter=256), "e24": dict(experts=24, top_k=4, expert_inter=256)}
TIE_GROUPS = 16          # experts g, 32 + g, 64 + g, 96 + g (one per router part) share one router row, g < TIE_GROUPS


@pytest.fixture(scope="module")
def pkg():
    import torch
    import __graft_entry__ as ge
    assert torch.cuda.is_available()
    p = ge.load_package()
    p.load_library()
    return p


_TM = {}


def _model(kind):
    from tests import modelgen
    if kind == "asym":
        if kind not in _TM:
            _TM[kind] = modelgen.TinyModel(True, layers=2, vocab=VOCAB, seed=53, max_seq_len=64, expert_asym=True, **DIMS)
        return _TM[kind]
    if kind in SHORT_LAST_PART:
        if kind not in _TM:
            _TM[kind] = modelgen.TinyModel(True, layers=2, vocab=VOCAB, seed=54, max_seq_len=64, **{**DIMS, **SHORT_LAST_PART[kind]})
        return _TM[kind]
    if "sym" not in _TM:
        _TM["sym"] = modelgen.TinyModel(True, layers=LAYERS, vocab=VOCAB, seed=51, max_seq_len=64, **DIMS)
    if kind == "tied" and kind not in _TM:
        # equal router rows in all four parts: the logits of a group are the same number (the same dot product, part by part),
        # so only the tie rule — lower expert id first — orders them, across the parts' lists
        tm = copy.copy(_TM["sym"])
        tm.layers = [dict(L) for L in tm.layers]
        for L in tm.layers:
            L["dense"] = dict(L["dense"])
            r = L["dense"]["router"].copy()
            for g in range(TIE_GROUPS):
                for part in range(1, 4):
                    r[32 * part + g] = r[g]
            L["dense"]["router"] = r
        _TM[kind] = tm
    return _TM[kind]


def _drive(tm, pkg, knobs, forms, c, on, graph):
    """c sequences: prefill, STEPS single decode forwards (ids, logits, the last layer's routing, the forms that ran), then
    GRAPH_STEPS more steps — in the hipGraph loop or as single forwards."""
    knobs.set(MOE_PAIR_RANK_LISTS=on)
    hm = tm.hip_model(pkg, kv_num_blocks=c * 2 + 4, max_seqs=c, max_tokens=max(c * PLEN, 64))
    rng = np.random.default_rng(52)
    prompts = [rng.integers(0, VOCAB, size=PLEN).astype(np.uint32) for _ in range(c)]
    toks, _ = hm.unified_forward([(i, p, 0, True) for i, p in enumerate(prompts)], greedy=True, want_logits=True)
    cur = np.array(toks, np.uint32)
    forms.reset()
    K = tm.cfg["top_k"]
    out = []
    for s in range(STEPS):
        toks, lg = hm.unified_forward([(i, [int(cur[i])], PLEN + s, True) for i in range(c)], greedy=True, want_logits=True)
        ids, w = hm.read_routing(c * K)
        cur = np.array(toks, np.uint32)
        out.append((cur.copy(), lg.copy(), ids, w))
    hits = forms.hits()
    if graph:
        tail = np.asarray(hm.decode_steps(list(range(c)), cur, GRAPH_STEPS), np.uint32)
    else:
        tail = np.zeros((GRAPH_STEPS, c), np.uint32)
        for s in range(GRAPH_STEPS):
            toks, _ = hm.unified_forward([(i, [int(cur[i])], PLEN + STEPS + s, True) for i in range(c)], greedy=True)
            cur = np.array(toks, np.uint32)
            tail[s] = cur
    del hm
    return out, hits, tail


def _on_equals_off(tm, pkg, knobs, forms, c):
    layers = len(tm.layers)
    on, hits_on, graph_ids = _drive(tm, pkg, knobs, forms, c, 1, True)
    off, hits_off, eager_ids = _drive(tm, pkg, knobs, forms, c, 0, False)
    assert hits_on.get("moe_pair_rank_lists", 0) == layers * STEPS and hits_on.get("moe_expert_major_pair", 0) == layers * STEPS, hits_on
    assert hits_on.get("decode_chain", 0) == layers * STEPS, hits_on
    assert "moe_pair_rank_lists" not in hits_off and hits_off.get("moe_expert_major_pair", 0) == layers * STEPS, hits_off
    K, E = tm.cfg["top_k"], tm.cfg["num_experts"]
    for s, ((t1, l1, i1, w1), (t0, l0, i0, w0)) in enumerate(zip(on, off)):
        assert np.array_equal(i1, i0), (s, np.nonzero(i1 != i0)[0][:8])
        assert np.array_equal(w1.view(np.uint32), w0.view(np.uint32)), (s, np.nonzero(w1.view(np.uint32) != w0.view(np.uint32))[0][:8])
        assert np.array_equal(l1.view(np.uint32), l0.view(np.uint32)), (s, float(np.abs(l1 - l0).max()))
        assert np.array_equal(t1, t0), s
        # a routing, not a leftover: K distinct experts per token, weights that sum to one (norm_topk_prob)
        ids = i1.reshape(c, K)
        assert ids.min() >= 0 and ids.max() < E and all(len(set(r)) == K for r in ids.tolist()), s
        assert np.allclose(w1.reshape(c, K).sum(axis=1), 1.0, atol=1e-5), s
    # graph ≡ eager: the hipGraph loop with the form on samples what single forwards with the in-chain merge sample
    assert np.array_equal(graph_ids, eager_ids), np.nonzero(graph_ids != eager_ids)
    return on


@pytest.mark.parametrize("c", [18, 32, 64, 128])
def test_pair_rank_lists_is_bit_identical_to_the_in_chain_merge(pkg, knobs, forms, c):
    _on_equals_off(_model("sym"), pkg, knobs, forms, c)


def test_pair_rank_lists_tie_rule_across_router_parts(pkg, knobs, forms):
    """Router rows repeated across the four parts: whole groups of experts tie exactly, and where the top-k boundary falls
    inside a group the lower expert ids — candidates of DIFFERENT parts' lists — must be the ones picked, by both forms."""
    c, K = 32, DIMS["top_k"]
    on = _on_equals_off(_model("tied"), pkg, knobs, forms, c)
    split = 0
    for _, _, ids, _ in on:
        for row in ids.reshape(c, K).tolist():
            for g in range(TIE_GROUPS):
                took = [p for p in range(4) if 32 * p + g in row]
                if 0 < len(took) < 4:
                    split += 1
                    assert took == list(range(len(took))), (g, row)            # the lower ids of the group, nothing else
    assert split > 0, "no token had its top-k boundary inside a tied group: the tie rule was not exercised"


@pytest.mark.parametrize("kind,c", [("e60", 32), ("e24", 18)])
def test_pair_rank_lists_with_a_short_last_router_part(pkg, knobs, forms, kind, c):
    """60 experts in four parts, 24 in two: the parts are whole 16-expert tiles, not equal shares, and a tile of the pair must
    look its expert up in the part the router put it in (experts 15, 30, 31, 45–47 of the 60; 12–15 of the 24 are the ones an
    equal-shares split would misplace).  Every expert that the in-chain merge picks must be picked here: bit identity."""
    on = _on_equals_off(_model(kind), pkg, knobs, forms, c)
    E, Q = SHORT_LAST_PART[kind]["experts"], 4 if kind == "e60" else 2
    misplaced = {e for e in range(E) if e // (E // Q) != e // 16}
    assert misplaced & {int(e) for _, _, ids, _ in on for e in ids}, "no token picked an expert whose part differs between the splits"


def test_pair_rank_lists_with_asymmetric_expert_stacks(pkg, knobs, forms):
    """Expert stacks with explicit zero points: the HAS_ZP instantiation of the merged launch."""
    _on_equals_off(_model("asym"), pkg, knobs, forms, 32)


def test_pair_rank_lists_only_where_the_pair_runs(pkg, knobs, forms):
    """Below 1.125 pairs per expert (c ≤ 17) the layer's grouped GEMMs are not the expert pair: role B keeps its merge (or,
    at ≤ 2 rows, the deferred merge of the K-split gate_up form) and the new form must not appear."""
    tm = _model("sym")
    c = 17
    knobs.set(MOE_PAIR_RANK_LISTS=1)
    hm = tm.hip_model(pkg, kv_num_blocks=c * 2 + 4, max_seqs=c, max_tokens=max(c * PLEN, 64))
    rng = np.random.default_rng(52)
    prompts = [rng.integers(0, VOCAB, size=PLEN).astype(np.uint32) for _ in range(c)]
    toks, _ = hm.unified_forward([(i, p, 0, True) for i, p in enumerate(prompts)], greedy=True, want_logits=True)
    cur = np.array(toks, np.uint32)
    for n in (17, 9, 2):
        forms.reset()
        toks, _ = hm.unified_forward([(i, [int(cur[i])], PLEN + (17, 9, 2).index(n), True) for i in range(n)], greedy=True)
        cur[:n] = np.array(toks, np.uint32)
        hits = forms.hits()
        assert hits.get("decode_chain", 0) == LAYERS, (n, hits)
        assert "moe_pair_rank_lists" not in hits and "moe_expert_major_pair" not in hits, (n, hits)
        if n <= 2: assert hits.get("moe_deferred_merge", 0) == LAYERS, (n, hits)
