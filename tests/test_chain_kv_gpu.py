"""What the one-launch decode chain (chain.hip) and the merged MoE pair write into the paged KV cache, vector by vector.

The chain tests in test_model_gpu.py see the chain through final logits only; here every decode-written cache slot of every
followed sequence is held against the oracle on its own — the last layer per (position, kv head) vector, layer 0 against a
threshold measured on the CPU — across a 16-token block boundary, eager and under hipGraph, and every prefill-written slot must
keep its bits.  Attention shape of Qwen3-30B-A3B (the shape the chain takes), two layers, a small expert side."""
import numpy as np
import pytest

from tests import parity_bounds as pb

pytestmark = pytest.mark.gpu

ORACLE_THREADS = 16
STEPS = 5
VOCAB = 512
LAYER0_MARGIN = 4.0        # × the measured emulation-vs-oracle deviation (fp32 summation order, fast-math exp / rsqrt are not emulated)
_TM = {}


@pytest.fixture(scope="module")
def pkg():
    import torch
    import __graft_entry__ as ge
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    p = ge.load_package()
    p.load_library()
    return p


def _model(moe):
    from tests import modelgen
    if moe not in _TM:
        if moe:       # E = 32, top-k 4, I = 256: the smallest expert side the chain, its router role and the merged pair still take
            _TM[moe] = modelgen.TinyModel(True, layers=2, hidden=2048, nq=32, nkv=4, hd=128, vocab=VOCAB, experts=32, top_k=4,
                                          expert_inter=256, seed=61, max_seq_len=64)
        else:
            _TM[moe] = modelgen.TinyModel(False, layers=2, hidden=2048, nq=32, nkv=4, hd=128, inter=2048, vocab=VOCAB, seed=63,
                                          max_seq_len=64, qk_norm=False, rope_theta=500000.0)
    return _TM[moe]


def _prompt_lens(c):
    """Staggered over 12…17.  Row 0 holds 16 tokens: its first decode write is position 16, the first slot of a fresh block;
    row 1 holds 15: its first write is the last slot of a block, its second opens the next.  Rows 2–4 (12, 13, 14) and the last
    row (14) cross 15 → 16 (→ 17) later in the 5 steps; the rows in between alternate 16 / 17 (a fresh block at once / one slot
    into it), so that the oracle can follow every boundary-crossing sequence within seconds."""
    lens = [16, 15, 12, 13, 14, 17][:c] + [16 + (i % 2) for i in range(6, c)]
    if c > 6: lens[-1] = 14
    return lens


def _followed(c, lens):
    rows = set(range(min(c, 6))) | {0, c // 2, c - 1} if c > 9 else set(range(c))
    rows |= {i for i, n in enumerate(lens) if n < 16}            # every sequence that crosses the block boundary while decoding
    return sorted(rows)


def _layer0_emulation_deviation(tm, om_kv, fed_rows, lens, followed):
    """Largest normalised deviation (max |Δ| / vector RMS) of the numpy fp16-storage restatement of layer 0's K / V path from
    the f32 oracle, over all followed rows and decode-written positions → (K figure, V figure)."""
    from oracle import oracle as O
    L, cfg = tm.layers[0], tm.cfg
    k_, n_, qw, sc, qz = L["gptq"]["qkv"]
    w = O.dequant_gptq(qw, sc, qz, 128, k_, n_)
    worst = [0.0, 0.0]
    for i in followed:
        pos = np.arange(lens[i], lens[i] + STEPS)
        emu = pb.emulate_layer0_kv(tm.glob["embed"][fed_rows[i]], L["dense"]["input_ln"], w, L["dense"].get("k_norm"), pos,
                                   cfg["num_heads"], cfg["num_kv_heads"], cfg["head_dim"], cfg["rms_eps"], cfg["rope_theta"],
                                   qk_norm=bool(cfg["has_qk_norm"]))
        for is_v in (0, 1):
            worst[is_v] = max(worst[is_v], float(pb.kv_vector_maxerr(om_kv[(i, 0, is_v)][pos], emu[is_v]).max()))
    return worst


@pytest.mark.parametrize("kind,c", [("moe", 1), ("moe", 9), ("moe", 32), ("dense", 20)])
def test_decode_chain_kv_writes_across_a_block_boundary(pkg, kind, c, forms, knobs):
    """Per followed sequence, K and V: (1) last layer, NMSE of every decode-written (position, kv head) vector < 3e-3 (the fp16
    round-trip bucket, per vector); (2) layer 0, max |Δ| / RMS of every such vector < 4 × the deviation of a CPU emulation with
    the device's fp16 storage points from the oracle — measured 2.1e-3 (K) and 1.3e-3 (V) on the MoE model, 2.3e-3 and 1.1e-3 on
    the dense one, so the limits are ≈ 9e-3 and ≈ 5e-3; the figure is recomputed here for the rows actually fed; (3) every
    prefill-written slot keeps its bits through all decode steps; (4) the seven-launch layer (DECODE_CHAIN=0, MOE_EM2=0) on the
    same fed ids passes (2) on its own; then the hipGraph loop's cache is bit-identical to the eager chain run's."""
    from oracle import oracle as O
    moe = kind == "moe"
    tm = _model(moe)
    L = tm.cfg["num_layers"]
    lens = _prompt_lens(c)
    followed = _followed(c, lens)
    assert lens[0] == 16 and (c < 2 or lens[1] == 15) and len(followed) >= min(c, 8)
    rng = np.random.default_rng(62)
    prompts = [rng.integers(0, VOCAB, size=n).astype(np.uint32) for n in lens]
    O.set_threads(ORACLE_THREADS)
    om = tm.oracle_model()

    def read_all(hm):
        return {(i, l, v): hm.read_kv(i, l, v) for i in range(c) for l in range(L) for v in (0, 1)}

    def drive(chain, fed):
        """Prefill, then STEPS eager single-token forwards.  fed=None: teacher-forced on the oracle's ids for the followed rows
        (the others feed their own); otherwise on the given ids."""
        if moe: knobs.set(DECODE_CHAIN=chain, MOE_EM2=chain)
        else: knobs.set(DENSE_CHAIN=chain)
        hm = tm.hip_model(pkg, kv_num_blocks=c * 3 + 4, max_seqs=c, max_tokens=max(sum(lens), 64))
        toks, _ = hm.unified_forward([(i, p, 0, True) for i, p in enumerate(prompts)], greedy=True)
        cur = np.array(toks, np.uint32)
        if fed is None:
            for oc, i in enumerate(followed):
                cur[i] = int(O.argmax_rows(om.forward(oc, prompts[i], 0)[None])[0])
        else:
            cur = fed[0].copy()
        after_prefill = read_all(hm)
        out_fed = [cur.copy()]
        forms.reset()
        for s in range(STEPS):
            toks, _ = hm.unified_forward([(i, [int(cur[i])], lens[i] + s, True) for i in range(c)], greedy=True)
            nxt = np.array(toks, np.uint32)
            if fed is None:
                for oc, i in enumerate(followed):
                    lg = om.forward(oc, np.array([cur[i]], np.uint32), lens[i] + s)
                    nxt[i] = int(O.argmax_rows(lg[None])[0])
            elif s + 1 < len(fed):
                nxt = fed[s + 1].copy()
            cur = nxt
            out_fed.append(cur.copy())
        return dict(hm=hm, hits=forms.hits(), fed=out_fed[:STEPS], prefill=after_prefill, final=read_all(hm))

    def check_prefill_slots_untouched(run, what):
        for (i, l, v), a in run["prefill"].items():
            b = run["final"][(i, l, v)]
            assert b.shape[0] == lens[i] + STEPS and a.shape[0] == lens[i], (what, i, a.shape, b.shape)
            assert np.array_equal(a, b[:lens[i]]), f"{what}: a decode write touched a prefill-written slot of sequence {i}, layer {l}, {'V' if v else 'K'}"

    def check_layer0(run, limits, what):
        for i in followed:
            pos = np.arange(lens[i], lens[i] + STEPS)
            for v in (0, 1):
                pb.assert_kv_positions(om_kv[(i, 0, v)], run["final"][(i, 0, v)], pos, limits[v], pb.kv_vector_maxerr,
                                       f"{what} c={c} sequence {i} layer 0 {'V' if v else 'K'} (max |err| / rms)")

    # ── eager chain run, teacher-forced on the oracle ──
    a = drive(1, None)
    O.set_threads(1)
    fed = a["fed"]
    om_kv = {(i, l, v): om.read_kv(oc, l, v) for oc, i in enumerate(followed) for l in range(L) for v in (0, 1)}
    hits = a["hits"]
    assert hits.get("decode_chain", 0) == L * STEPS, hits                    # one chain launch per layer and step
    forms.require("decode_chain")
    if moe and 8 * c * tm.cfg["top_k"] >= 9 * tm.cfg["num_experts"]:
        assert hits.get("moe_expert_major_pair", 0) == L * STEPS, hits
        forms.require("moe_expert_major_pair")
    if not moe:
        assert hits.get("dense_chain", 0) == L * STEPS, hits
    fed_rows = {i: np.array([fed[s][i] for s in range(STEPS)]) for i in followed}
    dev_k, dev_v = _layer0_emulation_deviation(tm, om_kv, fed_rows, lens, followed)
    print(f"{kind} c={c}: layer-0 emulation deviation from the oracle K {dev_k:.3g} V {dev_v:.3g} (limit {LAYER0_MARGIN:g}×)")
    assert 1e-4 < dev_v < 5e-3 and 1e-4 < dev_k < 5e-3, (dev_k, dev_v)       # fp16 storage: a few 2^-11 of the largest entry
    limits = (LAYER0_MARGIN * dev_k, LAYER0_MARGIN * dev_v)
    for i in followed:                                                       # (1) last layer, vector by vector
        pos = np.arange(lens[i], lens[i] + STEPS)
        for v in (0, 1):
            pb.assert_kv_positions(om_kv[(i, L - 1, v)], a["final"][(i, L - 1, v)], pos, pb.KV_ROUNDTRIP_NMSE, pb.kv_vector_nmse,
                                   f"chain c={c} sequence {i} last layer {'V' if v else 'K'} (NMSE per vector)")
    check_layer0(a, limits, "chain")                                         # (2)
    check_prefill_slots_untouched(a, "chain")                                # (3)
    final_a = a["final"]
    del a["hm"]

    # ── (4) the seven-launch layer on the same fed ids, against the oracle on its own ──
    b = drive(0, fed)
    assert "decode_chain" not in b["hits"] and "moe_expert_major_pair" not in b["hits"], b["hits"]
    check_layer0(b, limits, "seven-launch layer")
    check_prefill_slots_untouched(b, "seven-launch layer")
    del b

    # ── the same steps through the hipGraph loop: bit-identical cache ──
    if moe: knobs.set(DECODE_CHAIN=1, MOE_EM2=1)
    else: knobs.set(DENSE_CHAIN=1)
    hm = tm.hip_model(pkg, kv_num_blocks=c * 3 + 4, max_seqs=c, max_tokens=max(sum(lens), 64))
    hm.unified_forward([(i, p, 0, True) for i, p in enumerate(prompts)], greedy=True)
    forms.reset()
    ids = hm.decode_steps(list(range(c)), fed[0], STEPS)
    forms.require("decode_chain", "graph_replay")
    graph_fed = [fed[0]] + [ids[s].astype(np.uint32) for s in range(STEPS - 1)]
    final_g = read_all(hm)
    del hm
    if not all(np.array_equal(x, y) for x, y in zip(graph_fed, fed)):
        # the loop feeds its own samples: where one differs from the oracle's id, compare with an eager chain run fed the loop's ids
        final_a = drive(1, graph_fed)["final"]
    for key, g in final_g.items():
        assert np.array_equal(g, final_a[key]), f"hipGraph loop: KV differs from the eager chain run (sequence, layer, is_v) = {key}"


def test_per_position_check_sees_a_shifted_k_row_that_the_sequence_nmse_passes(pkg):
    """Detection, without touching a kernel: in a HOST copy of a 700-token sequence's cache, the K row of one decode-written
    position takes the previous slot's content (a block-table index off by one).  The whole-sequence NMSE < 3e-3 assert the
    suite had passes it (2 / 702 of the power); the per-(position, head) check names the position."""
    from tests import modelgen
    plen, steps = 700, 3
    res = modelgen.run_parity_case(pkg, moe=True, layers=2, prompt_len=plen, decode_steps=steps, seed=9, max_seq_len=1024)
    om, hm = res["oracle"], res["model"]
    ref, got = om.read_kv(0, 1, 0), hm.read_kv(1, 1, 0)
    pos = np.arange(plen, plen + steps)
    assert pb.assert_kv_positions(ref, got, pos, pb.KV_ROUNDTRIP_NMSE, pb.kv_vector_nmse, "clean") < pb.KV_ROUNDTRIP_NMSE
    bad = got.copy()
    bad[plen + 1] = got[plen]
    assert modelgen.nmse(ref, bad) < 3e-3                                    # the old whole-sequence assert
    with pytest.raises(AssertionError, match=f"position {plen + 1}"):
        pb.assert_kv_positions(ref, bad, pos, pb.KV_ROUNDTRIP_NMSE, pb.kv_vector_nmse, "shifted K row")
    with pytest.raises(AssertionError, match=f"position {plen + 1}"):
        pb.assert_kv_positions(ref, bad, pos, 0.05, pb.kv_vector_maxerr, "shifted K row")
