"""The one-launch decode chain (csrc/chain.hip) role by role, through its op-level entry ferrum_hip_decode_chain_f16.

Every stage is held against a reference computed from the DEVICE's own input to that stage (the convention of
pb.assert_gemm_elementwise), so no slack is left for a wrong intermediate:

  role A     res_a / norm1 bit for bit what the stand-alone kernel gives on the same inputs (moe_combine_add_rms_norm for the MoE
             tail, fused_add_rms_norm for the dense forms), and inside the combine and row-norm bounds;
  q|k|v      every element of qkv_out from the device's norm1 (unfolded INT4 bound, k = H);
  prologue   the new token's K / V slot and the q rows bit for bit what split_qkv_norm_rope_into_paged_cache_varlen makes of the
             device's qkv_out; every other cache slot keeps its bits, poison included;
  attention  attn_out against the float64 attention over the planted context (pb.decode_attn_ref_tol) with q from the stand-alone
             op and K / V from paged_kv_read after the launch;
  o_proj     each of the two fp32 K parts against the float64 product over its half of K from the device's attn_out;
  role B     res_b_out bit for bit fp16(res_a + fp16(part 0 + part 1)); norm2 inside the row-norm bound from the device's
             res_b_out; the routing without logits (pb.assert_route_selection / _ties / _lists) from the device's norm2.

All outputs and scratch are NaN-poisoned before a launch, with a guard row of 7 behind each that must keep its bits.  After
every launch the give-up word, cnt_next, the tickets and the granule area of cnt must be zero.  Each case is launched on
an unplanted cache first (its qkv_out supplies the query directions for the planting — q does not depend on the cache), then
twice on the planted cache on swapped counter halves: both planted launches must agree in every bit, the last one is checked.
The module prints the largest err/tol per role and case (-s); no tolerance is set from those figures."""
import numpy as np
import pytest

from tests import parity_bounds as pb

pytestmark = pytest.mark.gpu

NAN = float("nan")
EPS = 1e-6
NQ, HD = 32, 128
WORST = {}
GPU_ERROR = []                                # a launch or a synchronisation that failed: nothing more is launched by this module
_SLOT, _DIM = np.meshgrid(np.arange(16), np.arange(HD), indexing="ij")
K_OFF = (((_DIM >> 3) * 16 + _SLOT) * 8 + (_DIM & 7)).ravel()                                           # csrc/kv_layout.h, k_tile_off
V_OFF = ((((((_DIM >> 4) >> 1) * 4 + (_SLOT >> 2)) * 16 + (_DIM & 15)) * 2 + ((_DIM >> 4) & 1)) * 4 + (_SLOT & 3)).ravel()   # v_tile_off


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as ge
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    pkg = ge.load_package()
    pkg.load_library()
    from oracle import oracle as O
    O.build()
    ctx = pkg.HipBackend.new_context(64 << 20)
    yield pkg, pkg.HipBackend, ctx, O, torch
    ctx.sync()
    print("\ndecode chain roles, largest err/tol per role: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


_LIN = {}


def linear(env, k, n):
    """(GptqLinear, dequantised w [n, k]) — symmetric, group 128 — built once per shape for the whole module."""
    if (k, n) not in _LIN:
        pkg, B, ctx, O, torch = env
        qw, sc, qz = O.make_synthetic_gptq(k, n, 128, k * 7 + n, symmetric=True)
        sc = pb.f16r(sc / (0.28 * np.sqrt(k)))
        _LIN[(k, n)] = (pkg.GptqLinear.from_raw(qw, sc, qz, None, None, 4, 128, k, n), O.dequant_gptq(qw, sc, qz, 128, k, n))
    return _LIN[(k, n)]


_ROPE = {}


def rope(env, rows):
    if rows not in _ROPE:
        _ROPE[rows] = env[3].build_rope_cache(1e6, HD, rows)
    return _ROPE[rows]


def _note(role, case, ratio):
    WORST[role] = max(WORST.get(role, 0.0), ratio)
    print(f"{case}: {role} worst err/tol {ratio:.3f}")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


class Out:
    """A NaN-poisoned (integers: −1) output of `rows` rows with a guard row of 7 behind it; the entry is told the rows only."""

    def __init__(self, torch, rows, cols, dtype):
        self.t = torch.empty((rows + 1, cols), dtype=dtype, device="cuda")
        self.rows, self.fill = rows, (-1 if dtype in (torch.int32, torch.int64) else NAN)
        self.poison()

    def poison(self):
        self.t[:self.rows] = self.fill
        self.t[self.rows] = 7

    def arg(self):
        return (self.t.data_ptr(), self.rows * self.t.shape[1] * self.t.element_size())

    def host(self, what):
        a = self.t.float().cpu().numpy() if self.t.element_size() == 2 else self.t.cpu().numpy()
        assert np.all(a[self.rows] == 7), f"{what}: the guard row was written"
        return a[:self.rows]


def dev16(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda").half().contiguous()


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda").contiguous()


def h16(t):
    return t.float().cpu().numpy()


# ── the cases ────────────────────────────────────────────────────────────────────────────────────────────────────────────
SHORT = (1, 2, 15, 16, 17, 33)


def case(T, H=2048, nkv=4, E=128, K=8, Q=4, tail="moe", top_k=8, norm_topk=1, defer=0, qk_mode=1, splits=1, window=0, contexts=SHORT,
         knobs=None, forms=(), norm_rows=False, ties="lead"):
    return dict(T=T, H=H, nkv=nkv, E=E, K=K, Q=Q, tail=tail, top_k=top_k, norm_topk=norm_topk, defer=defer, qk_mode=qk_mode,
                splits=splits, window=window, contexts=contexts, knobs=knobs or {}, forms=forms, norm_rows=norm_rows, ties=ties)


def attn_case(name, T, **kw):
    nkv, splits, window, contexts = pb.ATTN_CASES[name]
    dense = nkv == 8                                        # (the shapes the chain takes: dense H 4096 / nkv 8, MoE H 2048 / nkv 4 or 16)
    return case(T, H=4096 if dense else 2048, nkv=nkv, E=0 if dense else 128, Q=1 if dense else 4, tail="rows" if dense else "moe",
                splits=splits, window=window, contexts=contexts, forms=("chain_attn_kv_splits",) if splits > 1 else (), **kw)


CASES = {
    # q|k|v and o_proj forms: 32-column blocks (T ≤ 16, default knobs), 64-column blocks, CHAIN_QKV_HALF / CHAIN_O_HALF = 0, the
    # 128-column blocks on and off at T = 32, both group counts, the clamped row T − 1 of a ragged last block
    "moe-T1-32col": case(1, norm_rows=True),
    "moe-T15-32col-deferred": case(15, defer=1, norm_rows=True),
    "moe-T16-64col-forced": case(16, knobs=dict(CHAIN_QKV_HALF=0, CHAIN_O_HALF=0), norm_topk=0, ties=None),
    "moe-T17-64col": case(17, defer=1, norm_topk=0, ties=None),
    "moe-T32-wide": case(32, knobs=dict(CHAIN_QKV_WIDE=1), forms=("chain_qkv_wide",), ties="plain"),
    "moe-T32-not-wide": case(32, knobs=dict(CHAIN_QKV_WIDE=0), defer=1, ties="plain"),
    "moe-T33-E60": case(33, E=60, K=4, norm_rows=True, ties=None),
    "moe-T128-E24-Q2-deferred": case(128, E=24, K=4, Q=2, defer=1),
    "moe-T9-E60-deferred-no-tail": case(9, E=60, K=4, defer=1, tail="none", norm_topk=0),
    "moe-T5-E24-Q2-top_k-10-tail": case(5, E=24, K=4, Q=2, top_k=10, norm_rows=True),
    "moe-H4096-T16": case(16, H=4096, nkv=8, norm_rows=True, ties="plain"),
    "moe-H4096-T33-deferred": case(33, H=4096, nkv=8, defer=1),
    "dense-H4096-T1-rows": case(1, H=4096, nkv=8, E=0, Q=1, tail="rows", qk_mode=2, norm_rows=True),
    "dense-H4096-T17-slabs": case(17, H=4096, nkv=8, E=0, Q=1, tail="slabs", qk_mode=2, norm_rows=True),
    "dense-H4096-T33-rows": case(33, H=4096, nkv=8, E=0, Q=1, tail="rows", qk_mode=2),
    "dense-H2048-T16-slabs-mode3": case(16, E=0, Q=1, tail="slabs", qk_mode=3),
    "moe-T4-mode0": case(4, qk_mode=0),
    # attention: every context of pb.ATTN_CASES (the CPU self-test runs the restatement through the same list)
    "attn-g8-unsplit": attn_case("g8-unsplit", 14, ties=None),
    "attn-g8-5-ranges-mode2": attn_case("g8-5-ranges", 14, qk_mode=2),
    "attn-g8-16-ranges": attn_case("g8-16-ranges", 14),
    "attn-g4-5-ranges": attn_case("g4-5-ranges", 14, qk_mode=2),
    "attn-g4-unsplit-mode1": attn_case("g4-unsplit", 14),
    "attn-g2-unsplit": attn_case("g2-unsplit", 14, qk_mode=2, ties="plain"),
    "attn-g2-16-ranges": attn_case("g2-16-ranges", 14),
    "attn-window-1": attn_case("window-1", 4),
    "attn-window-16-5-ranges": attn_case("window-16-5-ranges", 4, qk_mode=2),
    "attn-window-17": attn_case("window-17", 4),
    "attn-window-150-5-ranges": attn_case("window-150-5-ranges", 4),
    "attn-window-150-g4-16-ranges": attn_case("window-150-g4-16-ranges", 4, qk_mode=2),
    "attn-long-unsplit": attn_case("long-unsplit", 3),
    "attn-long-5-ranges": attn_case("long-5-ranges", 3, qk_mode=2),
}


def tie_groups(E, Q, mode):
    """Router rows duplicated across parts, so that experts of different parts carry bit-identical logits.
    "plain": ONE group of Q experts, one in every part (the last included), plain copies of one random row: their logit lies among
    the others', so selection, rank order and combine weights keep their grip (tol_L stays that of an ordinary row) and ties are
    resolved by id wherever the group is chosen.
    "lead": two groups of 12 (E 128), 8 (E 60) or 6 (E 24) experts, each wider than the top-k, rows 8·r and −8·r: for every token
    one of the two leads the ranking (unless its norm2 is nearly orthogonal to r) and the top-k boundary falls inside it."""
    EQ = pb._cdiv(E, 16) // Q * 16
    if mode == "plain":
        return [[q * EQ + 3 for q in range(Q)]]
    per = {128: 3, 60: 2, 24: 3}[E]
    return [sorted(q * EQ + first + 2 * j for q in range(Q) for j in range(per)) for first in (1, 2)]


@pytest.mark.parametrize("name", sorted(CASES))
def test_decode_chain_roles(env, forms, knobs, name):
    pkg, B, ctx, O, torch = env
    from ferrum_infer_rs_amd import backend as be
    c = CASES[name]
    assert not GPU_ERROR, f"an earlier case ended in a GPU error ({GPU_ERROR[0]}): nothing more is launched"
    T, H, nkv, E, Kr, Q = c["T"], c["H"], c["nkv"], c["E"], c["K"], c["Q"]
    G, N = NQ // nkv, (NQ + 2 * nkv) * HD
    rng = np.random.default_rng(sum(map(ord, name)))
    if c["knobs"]:
        knobs.set(**c["knobs"])
    lin_qkv, w_qkv = linear(env, H, N)
    lin_o, w_o = linear(env, NQ * HD, H)
    kv_lens = [c["contexts"][t % len(c["contexts"])] for t in range(T)]
    cols = max(pb._cdiv(n, 16) for n in kv_lens) + 2                       # two spare table columns per sequence
    cos, sin = rope(env, 2080 if max(kv_lens) > 320 else 320)
    qn, kn = pb.mixed_sign_weight(rng, HD), pb.mixed_sign_weight(rng, HD)

    # ── inputs of role A (or, without a tail, norm1 / res_a themselves) ──
    rows = (lambda: pb.norm_rows(rng, T, H, start=T)[0]) if c["norm_rows"] else (lambda: pb.f16r(rng.standard_normal((T, H))))
    ln_in, post_ln = pb.mixed_sign_weight(rng, H), pb.mixed_sign_weight(rng, H)
    a = {}
    if c["tail"] == "moe":
        tk = c["top_k"]
        a["down"] = pb.f16r(0.5 * rng.standard_normal((T * tk, H)))
        cw = rng.random((T, tk)) + 0.05
        a["comb_w"] = (cw / cw.sum(axis=1, keepdims=True)).astype(np.float32)
        a["res_in"] = rows()
    elif c["tail"] == "rows":
        a["a_x"], a["res_in"] = pb.f16r(rng.standard_normal((T, H))), rows()
    elif c["tail"] == "slabs":
        S, ld = 3, H + 64
        target = pb.f16r(rng.standard_normal((T, H)))
        slabs = np.zeros((S, T + 1, ld), np.float32)                          # (a row of padding per slab: the stride is not T·ld)
        slabs[:, :T, :H] = pb.split_into_slabs(rng, target, S)
        a["a_slabs"], a["res_in"] = slabs, rows()
    else:
        a["res_a"] = rows()
        a["norm1"] = pb.f16r(pb.rms_norm_ref64(a["res_a"], ln_in, EPS)[0])
    d_in = {k: (dev(torch, v) if v.dtype == np.float32 and k in ("comb_w", "a_slabs") else dev16(torch, v)) for k, v in a.items()}
    d_ln_in, d_post_ln, d_qn, d_kn = dev16(torch, ln_in), dev16(torch, post_ln), dev16(torch, qn), dev16(torch, kn)
    d_cos, d_sin = dev(torch, cos), dev(torch, sin)

    # ── router ──
    groups = []
    if E > 0:
        rw = pb.f16r(2.0 * rng.standard_normal((E, H)) / np.sqrt(H))
        if c["ties"]:
            groups = tie_groups(E, Q, c["ties"])
            r = rw[groups[0][0]].copy()
            if c["ties"] == "plain":
                rw[groups[0]] = r
            else:
                rw[groups[0]], rw[groups[1]] = pb.f16r(8.0 * r), pb.f16r(-8.0 * r)
        rw_pad = np.zeros((pb._cdiv(E, 16) * 16, H), np.float32)
        rw_pad[:E] = rw
        d_rw = B.dense_repack_f16t(ctx, dev16(torch, rw_pad), rw_pad.shape[0], H)

    # ── cache: T·cols blocks in a permuted pool, every table column names a block of its own ──
    nb = T * cols
    tables = rng.permutation(nb).astype(np.int32).reshape(T, cols)
    pool = [pb.f16r(rng.standard_normal((nb, nkv, 16 * HD))).astype(np.float16) for _ in range(2)]
    d_tables, d_lens = dev(torch, tables), dev(torch, np.array(kv_lens, np.uint32).view(np.int32))

    def put(seq, kvh, Klog, Vlog):
        pool[0][tables[seq][:, None], kvh, K_OFF[None, :]] = Klog.reshape(cols, 16 * HD).astype(np.float16)
        pool[1][tables[seq][:, None], kvh, V_OFF[None, :]] = Vlog.reshape(cols, 16 * HD).astype(np.float16)

    def logical(p, seq, kvh, off):
        return p[tables[seq][:, None], kvh, off[None, :]].reshape(cols * 16, HD).astype(np.float32)

    # ── outputs and scratch ──
    f16, f32, i32 = torch.float16, torch.float32, torch.int32
    o = dict(qkv_out=Out(torch, T, N, f16), attn_out=Out(torch, T, NQ * HD, f16), o_part=Out(torch, 2 * T, H, f32),
             res_b_out=Out(torch, T, H, f16), norm2=Out(torch, T, H, f16))
    if c["tail"] != "none":
        o.update(res_a=Out(torch, T, H, f16), norm1=Out(torch, T, H, f16))
    if E > 0 and c["defer"]:
        o.update(cand=Out(torch, T * Q, 16, f32), stats=Out(torch, T * Q, 2, f32))
    elif E > 0:
        o.update(ids=Out(torch, T, Kr, i32), weights=Out(torch, T, Kr, f32))
    if c["splits"] > 1:
        o.update(attn_partial=Out(torch, T * nkv * c["splits"] * 16, HD + 4, f32))
    words = be.decode_chain_counter_words()
    cnt = torch.zeros((2, words), dtype=i32, device="cuda")
    tickets = torch.zeros(T * nkv, dtype=i32, device="cuda")
    timeout = torch.zeros(1, dtype=i32, device="cuda")

    def launch(half, d_pool):
        for x in o.values():
            x.poison()
        bufs = {k: x.arg() for k, x in o.items()}
        bufs.update({k: v for k, v in d_in.items()})
        if c["tail"] != "none":
            bufs.update(ln_in=d_ln_in)
        if c["qk_mode"] == 1:
            bufs.update(q_norm_w=d_qn, k_norm_w=d_kn)
        if c["qk_mode"] != 0:
            bufs.update(cos_t=d_cos, sin_t=d_sin)
        if E > 0:
            bufs.update(router_w=d_rw)
        if c["splits"] > 1:
            bufs.update(attn_tickets=tickets)
        extra = dict(a_S=3, a_ld=H + 64, a_slab_stride=(T + 1) * (H + 64)) if c["tail"] == "slabs" else {}
        desc = be.decode_chain_desc(lin_qkv, lin_o, T=T, H=H, nq=NQ, nkv=nkv, has_a=int(c["tail"] != "none"), top_k=c["top_k"], eps=EPS,
                                    qk_mode=c["qk_mode"], max_blocks=cols, sliding_window=c["window"], E=E, r_top_k=Kr if E else 0, Q=Q,
                                    norm_topk=c["norm_topk"], defer_merge=c["defer"], attn_splits=c["splits"], k_pool=d_pool[0],
                                    v_pool=d_pool[1], block_tables=d_tables, kv_lens=d_lens, post_ln=d_post_ln, cnt=cnt[half],
                                    cnt_next=cnt[1 - half], timeout=timeout, **extra, **bufs)
        assert be.decode_chain_supports(desc), name
        forms.reset()
        try:
            be.decode_chain(ctx, desc)
            ctx.sync()
        except RuntimeError as e:
            if "decode_chain failed (rc=2)" not in str(e) and not isinstance(e, be.Unsupported):
                GPU_ERROR.append(name)
            raise
        # which block widths ran, by the launcher's stated rule: 32 columns at ≤ 16 rows unless the knob says 0 (o_proj: ≤ 2048
        # columns only), 128 columns where CHAIN_QKV_WIDE forces them (never with 32-column blocks), otherwise 64
        qkv_half = T <= 16 and c["knobs"].get("CHAIN_QKV_HALF", 1) != 0
        o_half = T <= 16 and H <= 2048 and c["knobs"].get("CHAIN_O_HALF", 1) != 0
        want = {"chain_qkv_half": qkv_half, "chain_o_half": o_half, "chain_attn_kv_splits": c["splits"] > 1}
        if qkv_half or "CHAIN_QKV_WIDE" in c["knobs"]:
            want["chain_qkv_wide"] = bool(c["knobs"].get("CHAIN_QKV_WIDE", 0)) and not qkv_half
        assert all(want.get(f, True) for f in c["forms"]), (name, want)
        forms.require("decode_chain", *[f for f, on in want.items() if on], *c["forms"], absent=tuple(f for f, on in want.items() if not on))
        gave_up = int(timeout.cpu().numpy().view(np.uint32)[0])
        assert gave_up == 0, f"{name}: an in-launch wait gave up (word {gave_up:#x})"
        cn = cnt.cpu().numpy()
        assert not cn[1 - half].any(), f"{name}: cnt_next is not all zero after the launch"
        assert not cn[half][words - 128 * 4 * 10 * 2:].any(), f"{name}: the granule area of cnt was not cleared"
        assert not tickets.cpu().numpy().any(), f"{name}: a ticket was left behind"
        got = {k: x.host(f"{name} {k}") for k, x in o.items() if k != "attn_partial"}
        if "attn_partial" in o:
            o["attn_partial"].host(f"{name} attn_partial")                       # (guard row only: its content is scratch)
        got["k_pool"], got["v_pool"] = (p.cpu().numpy().reshape(nb, nkv, 16 * HD) for p in d_pool)
        return got

    def standalone_split(qkv_out_dev):
        """q rows [T, nq, 128] and the new token's K / V slots as the stand-alone op writes them into zeroed pools."""
        q_out = torch.empty(T, NQ, HD, dtype=f16, device="cuda")
        sk, sv = B.alloc_paged_pool(nb, nkv, HD), B.alloc_paged_pool(nb, nkv, HD)
        B.split_qkv_norm_rope_into_paged_cache_varlen(
            ctx, qkv_out_dev, d_qn if c["qk_mode"] == 1 else None, d_kn if c["qk_mode"] == 1 else None, d_cos, d_sin, q_out, sk, sv,
            dev(torch, np.arange(T + 1, dtype=np.int32)), dev(torch, np.array(kv_lens, np.int32) - 1), d_tables, T, T, NQ, nkv, HD, EPS,
            c["qk_mode"], 16, cols)
        ctx.sync()
        return h16(q_out), sk.cpu().numpy().reshape(nb, nkv, 16 * HD), sv.cpu().numpy().reshape(nb, nkv, 16 * HD)

    # ── launch 1: unplanted cache → qkv_out → the query directions and the new token's K / V ──
    first = launch(0, [dev(torch, p.reshape(-1)) for p in pool])
    q_rows, sk, sv = standalone_split(o["qkv_out"].t[:T].contiguous())
    plans = {}
    for t in range(T):
        for kvh in range(nkv):
            k_new = logical(sk, t, kvh, K_OFF)[kv_lens[t] - 1]
            plan = pb.plant_context(rng, q_rows[t, kvh * G:(kvh + 1) * G], k_new, kv_lens[t], c["window"], c["splits"], cols)
            put(t, kvh, plan["K"], plan["V"])
            plans[(t, kvh)] = plan
    # ── launches 2 and 3: the planted cache on swapped counter halves ──
    second = launch(1, [dev(torch, p.reshape(-1)) for p in pool])
    d_pool = [dev(torch, p.reshape(-1)) for p in pool]
    got = launch(0, d_pool)
    for k in got:
        assert np.array_equal(bits(second[k]), bits(got[k])), f"{name}: {k} differs between the two launches on swapped counter halves"
    assert np.array_equal(bits(first["qkv_out"]), bits(got["qkv_out"])), f"{name}: qkv_out depends on the cache"

    # ── role A ──
    if c["tail"] != "none":
        res_a, norm1 = got["res_a"], got["norm1"]
        r2, n2 = d_in["res_in"].clone(), torch.full((T, H), NAN, dtype=f16, device="cuda")
        if c["tail"] == "moe":
            B.moe_combine_add_rms_norm(ctx, d_in["down"], d_in["comb_w"], r2, d_ln_in, EPS, n2, T, c["top_k"], H)
            ref, tol = pb.fused_tail_residual_ref_tol(a["down"], a["comb_w"], a["res_in"], T, c["top_k"])
        else:
            x = a["a_x"] if c["tail"] == "rows" else pb.slabs_to_f16(a["a_slabs"][:, :T, :H])
            B.fused_add_rms_norm(ctx, r2, dev16(torch, x), d_ln_in, EPS, n2, T, H)
            ref = a["res_in"].astype(np.float64) + x.astype(np.float64)
            tol = pb.EPS_F16 * np.abs(ref) + pb.FLOOR_F16                         # fp16 + fp16 is exact in fp32: one fp16 rounding
        ctx.sync()
        assert np.array_equal(bits(h16(r2)), bits(res_a)), f"{name}: res_a is not the stand-alone kernel's bits"
        assert np.array_equal(bits(h16(n2)), bits(norm1)), f"{name}: norm1 is not the stand-alone kernel's bits"
        _note("res_a", name, pb.assert_within(ref, tol, res_a, f"{name} res_a"))
        _note("norm1", name, pb.assert_rms_norm_elementwise(res_a, ln_in, EPS, norm1, f"{name} norm1"))
    else:
        res_a, norm1 = a["res_a"], a["norm1"]

    # ── q|k|v from the device's norm1 ──
    ref, absdot = pb.gemm_refs(norm1, w_qkv)
    _note("qkv_out", name, pb.assert_gemm_elementwise(ref, absdot, got["qkv_out"], H, False, f"{name} qkv_out"))

    # ── prologue: the new token's slot and the q rows, bit for bit; every other slot keeps its bits ──
    for t in range(T):
        blk, slot = tables[t, (kv_lens[t] - 1) // 16], (kv_lens[t] - 1) % 16
        for p_got, p_sa, p_in, off, what in ((got["k_pool"], sk, pool[0], K_OFF, "K"), (got["v_pool"], sv, pool[1], V_OFF, "V")):
            idx = off.reshape(16, HD)[slot]
            assert np.array_equal(bits(p_got[blk][:, idx]), bits(p_sa[blk][:, idx])), f"{name}: the new token's {what} of sequence {t} is not the stand-alone op's bits"
            p_in[blk][:, idx] = p_got[blk][:, idx]                                # (what is left must be untouched)
    assert np.array_equal(bits(got["k_pool"]), bits(pool[0])) and np.array_equal(bits(got["v_pool"]), bits(pool[1])), \
        f"{name}: a cache slot other than the new tokens' changed"

    # ── attention: q from the stand-alone op, K / V read back through paged_kv_read ──
    worst = 0.0
    for t in range(T):
        kk, vv = B.paged_kv_read(ctx, d_pool[0], d_pool[1], d_tables[t].contiguous(), kv_lens[t], nkv, HD)
        ctx.sync()
        kk, vv = h16(kk), h16(vv)
        for kvh in range(nkv):
            plan = plans[(t, kvh)]
            Kl, Vl = plan["K"].copy(), plan["V"].copy()
            n = kv_lens[t]
            assert np.array_equal(kk[:n - 1, kvh], Kl[:n - 1].astype(np.float32)) and np.array_equal(vv[:n - 1, kvh], Vl[:n - 1].astype(np.float32)), \
                f"{name}: the cache read back differs from what was planted (sequence {t}, kv head {kvh})"
            Kl[:n], Vl[:n] = kk[:, kvh], vv[:, kvh]
            ref, tol, w = pb.decode_attn_ref_tol(q_rows[t, kvh * G:(kvh + 1) * G], Kl, Vl, plan["allowed"], n, c["window"], c["splits"])
            for p, h in zip(plan["edges"], plan["heads"]):                      # the planting holds on the device's own q and cache
                assert pb.PLANT_MASS[0] <= w[h, p] <= pb.PLANT_MASS[1], \
                    f"{name}: the key planted at position {p} of sequence {t} (kv_len {n}), kv head {kvh} carries {w[h, p]:.3g} of row {h}'s mass"
            out = got["attn_out"].reshape(T, NQ, HD)[t, kvh * G:(kvh + 1) * G]
            worst = max(worst, pb.assert_within(ref, tol, out, f"{name} attn_out sequence {t} (kv_len {n}) kv head {kvh}"))
    _note("attn_out", name, worst)
    if c["splits"] == 1 and c["window"] == 0:
        ref_out = torch.full((T, NQ * HD), NAN, dtype=f16, device="cuda")
        B.paged_batched_decode_attention(ctx, dev16(torch, q_rows.reshape(T, NQ * HD)), d_pool[0], d_pool[1], ref_out, d_tables, d_lens, T,
                                         max(kv_lens), NQ, nkv, HD, 16, cols)
        ctx.sync()
        diff = np.abs(h16(ref_out) - got["attn_out"])
        print(f"{name}: attn_out against paged_batched_decode_attention on the same q and cache: largest |difference| {float(diff.max()):.3g}, "
              f"{int((diff != 0).sum())} of {diff.size} elements differ")

    # ── o_proj: each K half from the device's attn_out ──
    Kh = NQ * HD // 2
    parts = got["o_part"].reshape(2, T, H)
    for ks in range(2):
        ref, absdot = pb.gemm_refs(got["attn_out"][:, ks * Kh:(ks + 1) * Kh], w_o[:, ks * Kh:(ks + 1) * Kh])
        _note("o_part", name, pb.assert_gemm_elementwise(ref, absdot, parts[ks], Kh, False, f"{name} o_part[{ks}]", out_f32=True))

    # ── role B ──
    with np.errstate(over="ignore"):
        x16 = (parts[0] + parts[1]).astype(np.float16).astype(np.float32)
        want = (res_a.astype(np.float32) + x16).astype(np.float16).astype(np.float32)
    assert np.array_equal(bits(want), bits(got["res_b_out"])), f"{name}: res_b_out is not fp16(res_a + fp16(part 0 + part 1))"
    _note("norm2", name, pb.assert_rms_norm_elementwise(got["res_b_out"], post_ln, EPS, got["norm2"], f"{name} norm2"))
    if E > 0:
        L, tolL = pb.route_logits_ref_tol(got["norm2"], rw)
        if c["defer"]:
            cand = got["cand"].reshape(T, Q, 8, 2)
            cl, ci = cand[..., 0], np.ascontiguousarray(cand[..., 1]).view(np.int32).astype(np.int64)
            pb.assert_route_lists(L, tolL, cl, ci, got["stats"].reshape(T, Q, 2), Q, Kr, f"{name} candidate lists")
            for g in groups:                                                       # duplicated rows: bit-identical logits wherever listed
                for t in range(T):
                    seen = {cl[t].ravel()[i].tobytes() for i in np.nonzero(np.isin(ci[t].ravel(), g))[0]}
                    assert len(seen) <= 1, f"{name}: token {t}: the tied experts {g} carry different logit bits"
        else:
            _note(f"combine weights (ties {c['ties']})", name, pb.assert_route_selection(L, tolL, got["ids"], got["weights"], c["norm_topk"], f"{name} routing"))
            if c["ties"] != "lead" and T * Kr >= 32:
                # logits spread over all experts: every part — the last, short one included — must supply a chosen expert to some token
                EQ = pb._cdiv(E, 16) // Q * 16
                parts_seen = set((got["ids"] // EQ).ravel().tolist())
                assert parts_seen == set(range(Q)), f"{name}: no token chose an expert of parts {sorted(set(range(Q)) - parts_seen)}"
            if groups:
                cut = pb.assert_route_ties(got["ids"], groups, f"{name} routing")
                assert cut >= 1 or T < 4 or c["ties"] != "lead", f"{name}: no token's top-k boundary falls inside the tied group"
                print(f"{name}: the top-k boundary cuts the tied group for {cut} of {T} tokens")
