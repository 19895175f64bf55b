"""GPU parity, element by element (tests/parity_bounds.py): every phase of the MoE expert path and the many-row dense INT4
forms against a float64 reference built from that phase's OWN device input, so roundings do not stack and the tolerance is the
derived one.  The whole-tensor NMSE asserts elsewhere in the suite stay; these see the single wrong element, the wrong fragment
and the wrong quant group that an average over 10^5 … 10^7 elements hides."""
import numpy as np
import pytest

from tests import parity_bounds as pb

pytestmark = pytest.mark.gpu

NMSE_FP16_TOL = 1e-6
NAN = float("nan")


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as ge
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    pkg = ge.load_package()
    pkg.load_library()          # raises if the HIP extension is missing — no fallback
    from oracle import oracle as O
    O.build()
    ctx = pkg.HipBackend.new_context()
    return pkg, pkg.HipBackend, ctx, O, torch


def dev16(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda").half().contiguous()


def host(t):
    return t.float().cpu().numpy()


# ── MoE phases ───────────────────────────────────────────────────────────────────────────────────────────────────────────
def _hand_routing():
    """24 tokens × 2 of 8 experts, by hand: experts 1 and 4 get no pair, expert 2 exactly 16 (one full pass of the expert-major
    grid), expert 3 gets 17 (one pair into a second pass), the last expert index (7) is used."""
    rid = [(2, 3)] * 16 + [(3, 7)] + [(0, 5), (6, 7), (0, 6), (5, 7), (0, 7), (5, 6), (0, 5)]
    rid = np.array(rid, np.uint32)
    cnt = np.bincount(rid.ravel(), minlength=8)
    assert cnt[1] == 0 and cnt[4] == 0 and cnt[2] == 16 and cnt[3] == 17 and cnt[7] > 0
    w = np.random.default_rng(11).random(rid.shape).astype(np.float32) + 0.1
    return rid, (w / w.sum(axis=1, keepdims=True)).astype(np.float32)


def _pair_refs(rows, w_stack, eids):
    """float64 (ref, Σ|x||w|) of out[p] = rows[p] · w_stack[eids[p]]ᵀ."""
    ref = np.zeros((len(eids), w_stack.shape[1]))
    absdot = np.zeros_like(ref)
    for e in np.unique(eids):
        sel = np.nonzero(eids == e)[0]
        ref[sel], absdot[sel] = pb.gemm_refs(rows[sel], w_stack[e])
    return ref, absdot


MOE_CASES = {
    # (tokens, E, K, H, I, asymmetric, hand-built routing); I = 256 is the smallest the merged pair takes (down needs ≥ 2 groups)
    "t32-e16-k4": (32, 16, 4, 512, 256, False, False),
    "t64-e8-k2-further-passes": (64, 8, 2, 512, 256, False, False),       # experts hold more than 16 pairs
    "hand-routing": (24, 8, 2, 512, 256, False, True),
    "asymmetric-zero-points": (32, 16, 4, 512, 256, True, False),
}


@pytest.mark.parametrize("case", sorted(MOE_CASES))
def test_moe_phases_element_by_element(env, case, forms):
    """gate_up (unfused), the fused silu·mul output, down and combine of every grouped-GEMM entry point, each against float64
    from the phase's own device input.  None of these forms folds the scale into the B operand (the group scale multiplies
    the fp32 chain result: w4_gemm.h, w4_consume_group), so folded=False throughout."""
    pkg, B, ctx, O, torch = env
    tokens, E, K, H, I, asym, hand = MOE_CASES[case]
    rng = np.random.default_rng(tokens * E + H + asym)
    gu = [O.make_synthetic_gptq(H, 2 * I, 128, 700 + e, symmetric=not asym) for e in range(E)]
    dn = [O.make_synthetic_gptq(I, H, 128, 900 + e, symmetric=not asym) for e in range(E)]
    gu = [(q, pb.f16r(s / (0.28 * np.sqrt(H))), z) for q, s, z in gu]
    dn = [(q, pb.f16r(s / (0.28 * np.sqrt(I))), z) for q, s, z in dn]
    gw = np.stack([O.dequant_gptq(q, s, z, 128, H, 2 * I) for q, s, z in gu])
    dw = np.stack([O.dequant_gptq(q, s, z, 128, I, H) for q, s, z in dn])
    x = pb.f16r(rng.standard_normal((tokens, H)))
    if hand:
        rid, rw = _hand_routing()
    else:
        rid, rw = O.route_topk(rng.standard_normal((tokens, E)).astype(np.float32), E, K, True)
    eids = rid.astype(np.int64).reshape(-1)
    P = tokens * K
    if case == "t64-e8-k2-further-passes": assert np.bincount(eids, minlength=E).max() > 16
    ids_d = torch.from_numpy(eids.astype(np.int32)).cuda()
    wd = torch.from_numpy(rw.reshape(-1).copy()).cuda()
    xd = dev16(torch, x)
    load = lambda t, k, n, fused=False: B.load_gptq_stacked([q for q, _, _ in t], [s for _, s, _ in t], [z for _, _, z in t], None,
                                                            4, 128, k, n, fuse_gate_up=fused)
    plain, fused, down_stack = load(gu, H, 2 * I), load(gu, H, 2 * I, True), load(dn, I, H)

    x_rows = x[np.arange(P) // K]
    gu_ref, gu_abs = _pair_refs(x_rows, gw, eids)

    def check_gate_up(gup, what):
        pb.assert_gemm_elementwise(gu_ref, gu_abs, host(gup), H, False, f"{case} {what} gate_up")

    def check_act(act, what):
        pb.assert_gated_elementwise(gu_ref[:, :I], gu_ref[:, I:], gu_abs[:, :I], gu_abs[:, I:], host(act), H, False, f"{case} {what} silu·mul")

    def check_down_and_combine(act, down, what):
        ref, absdot = _pair_refs(host(act), dw, eids)            # from THIS act: the rounding of act is not charged to down
        pb.assert_gemm_elementwise(ref, absdot, host(down), I, False, f"{case} {what} down")
        out = torch.full((tokens, H), NAN, dtype=torch.float16, device="cuda")
        B.moe_combine(ctx, down, wd, out, tokens, K, H)
        ctx.sync()
        pb.assert_combine_elementwise(host(down), rw, host(out), tokens, K, f"{case} {what} combine")

    def poisoned(cols):
        return torch.full((P, cols), NAN, dtype=torch.float16, device="cuda")

    def run(what, form, gate_up_call, down_call):
        forms.reset()
        gup, act, down = poisoned(2 * I), poisoned(I), poisoned(H)
        gate_up_call(plain, gup, False)
        gate_up_call(fused, act, True)
        down_call(act, down)
        ctx.sync()
        forms.require(form)
        check_gate_up(gup, what)
        check_act(act, what)
        check_down_and_combine(act, down, what)

    run("expert-major", "moe_expert_major",
        lambda st, out, f: st.gemm_phase_expert_major(ctx, xd, ids_d, out, P, E, K, fused_silu_mul=f),
        lambda act, out: down_stack.gemm_phase_expert_major(ctx, act, ids_d, out, P, E, 1))

    # gate_up → down as one launch, on NaN-poisoned outputs
    forms.reset()
    act4, down4 = poisoned(I), poisoned(H)
    fused.gemm_phase_expert_major_pair(ctx, down_stack, xd, ids_d, act4, down4, P, E, K)
    ctx.sync()
    assert fused.pair_timeouts(ctx) == 0
    forms.require("moe_expert_major_pair")
    check_act(act4, "pair")
    check_down_and_combine(act4, down4, "pair")

    for blk in (16, 64):
        sorted_max = P + E * blk
        sd = torch.empty(sorted_max, dtype=torch.int32, device="cuda")
        bd = torch.empty(sorted_max // blk + 1, dtype=torch.int32, device="cuda")
        td = torch.zeros(1, dtype=torch.int32, device="cuda")
        B.moe_align_block_size_pair_ids(ctx, ids_d, sd, bd, td, P, E, blk, sorted_max)
        mb = sorted_max // blk
        run(f"block-{blk}", "moe_block16" if blk == 16 else "moe_tile64",
            lambda st, out, f: st.gemm_phase_vllm(ctx, xd, sd, bd, td, out, P, blk, K, mb, fused_silu_mul=f),
            lambda act, out: down_stack.gemm_phase_vllm(ctx, act, sd, bd, td, out, P, blk, 1, mb))

    mb = P // 16 + E
    run("inline-align", "moe_inline_align",
        lambda st, out, f: st.gemm_phase_inline_align(ctx, xd, ids_d, out, P, E, K, mb, fused_silu_mul=f),
        lambda act, out: down_stack.gemm_phase_inline_align(ctx, act, ids_d, out, P, E, 1, mb))


# ── dense forms with many row tiles: where a whole-tensor NMSE is blind ──────────────────────────────────────────────────
DENSE_CASES = {
    # (k, n, m, symmetric, bias, forced W4_BIG, form, folded)
    # folded — from the kernel source (w4_tiles.hip): w4_gemm_big_kernel finishes each weight as fp16 in registers,
    # (q − zero)·scale rounded once (v_pk_mul_f16), before the MFMA: folded.  w4_gemm_tilep_kernel keeps exact fp16 integers in
    # the B operand and multiplies the fp32 chain result of each k-half by the scale: not folded (nor are the split-K slabs it
    # may write: fp32, summed in fixed order).
    "big-2100-rows": (1024, 4096, 2100, False, False, None, "w4_big", True),
    "tilep-odd-groups-ragged": (640, 320, 1100, True, False, None, "w4_tilep", False),
    "tilep-ragged-tile-partial-columns": (1024, 1000, 1153, True, False, None, "w4_tilep", False),
    "big-forced-n1000-bias": (1024, 1000, 16 * 8 + 37, False, True, 8, "w4_big", True),
}


@pytest.mark.parametrize("case", sorted(DENSE_CASES))
def test_dense_many_row_forms_element_by_element(env, case, forms, knobs):
    pkg, B, ctx, O, torch = env
    k, n, m, sym, with_bias, force_big, form, folded = DENSE_CASES[case]
    qw, sc, qz = O.make_synthetic_gptq(k, n, 128, k * 7 + n, symmetric=sym)
    sc = pb.f16r(sc / (0.28 * np.sqrt(k)))
    bias = pb.f16r(np.random.default_rng(5).standard_normal(n)) if with_bias else None
    lin = pkg.GptqLinear.from_raw(qw, sc, qz, None, bias, 4, 128, k, n)
    w = O.dequant_gptq(qw, sc, qz, 128, k, n)
    if force_big: knobs.set(W4_BIG=force_big)
    x = pb.f16r(np.random.default_rng(m).standard_normal((m, k)))
    out = torch.full((m + 1, n), 7.0, dtype=torch.float16, device="cuda")         # guard row: nothing may write past m rows
    forms.reset()
    lin.forward(ctx, dev16(torch, x), out, m)
    ctx.sync()
    forms.require(form, absent=tuple(f for f in ("w4_wgsplit", "w4_ldsa", "w4_tilep", "w4_big") if f != form))
    ref, absdot = pb.gemm_refs(x, w, bias)                                        # the bias is one more term of the sum
    got = host(out)
    assert np.all(got[m] == 7.0), case
    worst = pb.assert_gemm_elementwise(ref, absdot, got[:m], k, folded, case)
    print(f"{case}: worst err/tol {worst:.3f}")
    if case == "big-2100-rows":
        # detection, without touching the kernel: one element of the DEVICE output zeroed — the whole-tensor NMSE assert the suite
        # had passes it, the element-wise bound names it
        r, c = 1234, 77
        assert abs(ref[r, c]) > 0.05 * ref.std()
        out[r, c] = 0.0
        bad = host(out)[:m]
        assert pb.nmse(ref, bad) < NMSE_FP16_TOL
        with pytest.raises(AssertionError, match=rf"1 of {m * n} elements.*\(row, col\) = \({r}, {c}\)"):
            pb.assert_gemm_elementwise(ref, absdot, bad, k, folded, case)
