"""GPU parity, element by element, of the decode-regime dense GEMM forms (tests/parity_bounds.py): the intra-workgroup K split
(`w4_wgsplit`, every <MT, NT> instance and the exits of its two-deep pipeline), the LDS-shared-activation kernel (`w4_ldsa`,
its three instances, forced split counts and both bias paths), `w4_tilep` at 33–63 rows, the three fp32 slab producers
(`w4_slabs`, `w4_slabs_lds`, `w4_slabs_tile`), the fused combine + add + norm prologue (`w4_fused_tail`) and the fp16 GEMMs of
the router and the lm_head — which the rest of the suite holds to a whole-tensor NMSE only, or does not call at op level at all.

Every output is NaN-poisoned with a guard row of 7.0 after row m, every input must come back unchanged, the float64 reference
and Σ|x||w| come from pb.gemm_refs, and the form that ran is required by name.  None of these kernels folds the scale into the
B operand (folded=False).  Shapes are the smallest on which each path exists; the W4_* knobs only ever force launches inside
the kernels' own launch bounds."""
import numpy as np
import pytest

from tests import parity_bounds as pb

pytestmark = pytest.mark.gpu

NAN = float("nan")
DENSE_FORMS = ("w4_wgsplit", "w4_ldsa", "w4_tilep", "w4_big")
WORST = {}                                    # form → largest err/tol seen (printed at module teardown; information only)


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as ge
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    pkg = ge.load_package()
    pkg.load_library()          # raises if the HIP extension is missing — no fallback
    from oracle import oracle as O
    O.build()
    ctx = pkg.HipBackend.new_context(64 << 20)
    yield pkg, pkg.HipBackend, ctx, O, torch
    ctx.sync()
    print("\ndense decode forms, largest err/tol per form: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def _note(form, ratio, what):
    WORST[form] = max(WORST.get(form, 0.0), ratio)
    print(f"{what}: worst err/tol {ratio:.3f}")


def dev16(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda").half().contiguous()


def dev32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda").contiguous()


def host(t):
    return t.float().cpu().numpy()


class Unchanged:
    """Device inputs that must come back bit for bit."""

    def __init__(self, torch, *tensors):
        self.torch = torch
        self.pairs = [(t, t.clone()) for t in tensors]

    def check(self):
        for t, c in self.pairs:
            it = self.torch.int16 if t.element_size() == 2 else self.torch.int32
            assert self.torch.equal(t.view(it), c.view(it)), "an input buffer was modified"


def poisoned(torch, m, n, dtype=None):
    """[m + 1, n] of NaN whose last row is the guard: nothing may write past m rows."""
    out = torch.full((m + 1, n), NAN, dtype=dtype or torch.float16, device="cuda")
    out[m] = 7.0
    return out


def guarded_rows(out, m, what):
    got = host(out)
    assert np.all(got[m] == 7.0), f"{what}: the guard row after row {m} was written"
    return got[:m]


_LINEARS = {}


def linear(env, k, n, sym=True, bias=False, g_idx=False):
    """(GptqLinear, dequantised w [n, k], bias or None), built once per shape and shared by the cases that use it."""
    key = (k, n, sym, bias, g_idx)
    if key not in _LINEARS:
        pkg, B, ctx, O, torch = env
        qw, sc, qz = O.make_synthetic_gptq(k, n, 128, k * 7 + n, symmetric=sym)
        sc = pb.f16r(sc / (0.28 * np.sqrt(k)))
        b = pb.f16r(np.random.default_rng(5).standard_normal(n)) if bias else None
        gi = O.make_desc_act_g_idx(k, 128) if g_idx else None
        _LINEARS[key] = (pkg.GptqLinear.from_raw(qw, sc, qz, gi, b, 4, 128, k, n), O.dequant_gptq(qw, sc, qz, 128, k, n, g_idx=gi), b)
    return _LINEARS[key]


def run_forward(env, forms, form, case, m, k, n, sym=True, bias=False, g_idx=False):
    """lin.forward on m rows: poisoned output, guard row, inputs unchanged, the form required, every element in bound."""
    pkg, B, ctx, O, torch = env
    lin, w, b = linear(env, k, n, sym, bias, g_idx)
    x = pb.f16r(np.random.default_rng(m * 131 + k).standard_normal((m, k)))
    xd = dev16(torch, x)
    ins = Unchanged(torch, xd)
    out = poisoned(torch, m, n)
    forms.reset()
    lin.forward(ctx, xd, out, m)
    ctx.sync()
    forms.require(form, absent=tuple(f for f in DENSE_FORMS if f != form))
    ins.check()
    ref, absdot = pb.gemm_refs(x, w, b)                          # the bias is one more term of the sum
    _note(form, pb.assert_gemm_elementwise(ref, absdot, guarded_rows(out, m, case), k, False, case), case)


# ── w4_gemm_wgsplit_kernel ───────────────────────────────────────────────────────────────────────────────────────────────
WGSPLIT_CASES = {
    # (m, k, n, W4_NT, W4_W, symmetric, bias, act-order).  Launch bounds: W ≤ 16 at MT 1 (≤ 16 rows); ≤ 8 at MT 2 (17–32 rows) with
    # NT ≥ 2, ≤ 16 with NT 1; ≤ 4 at MT 4 (33–63 rows, on k·n < 12 Mi so that the tile kernel stays out); LDS W·MT·NT KiB ≤ 64.
    # W4_W=1 puts the whole K into one wave: 1…5 groups are the exits of the two-deep pipeline loop.
    "m1-k128-one-group": (1, 128, 72, 4, 1, True, False, False),
    "m15-k256-two-groups": (15, 256, 72, 2, 1, True, False, False),
    "m16-k384-three-groups": (16, 384, 72, 1, 1, True, False, False),
    "m16-k512-four-groups": (16, 512, 1000, 4, 1, True, False, False),
    "m16-k640-five-groups": (16, 640, 1000, 2, 1, True, False, False),
    "m16-k384-w4-empty-wave-0": (16, 384, 1000, 4, 4, True, False, False),
    "m16-k640-w4-uneven-slices": (16, 640, 2048, 4, 4, True, False, False),
    "m16-k8192-n256-w16": (16, 8192, 256, 4, 16, True, False, False),
    "m15-k640-bias": (15, 640, 1000, 4, 4, True, True, False),
    "m16-k512-zero-points": (16, 512, 1000, 2, 2, False, False, False),
    "m16-k512-act-order-unforced": (16, 512, 1000, None, None, False, False, True),
    "m1-k2048-unforced": (1, 2048, 2048, None, None, True, False, False),
    "m17-k512-mt2-nt2-w8": (17, 512, 1000, 2, 8, True, False, False),
    "m32-k640-mt2-nt4-w8-zero-points": (32, 640, 2048, 4, 8, False, False, False),
    "m32-k512-mt2-nt1-w16": (32, 512, 72, 1, 16, True, True, False),
    "m33-k640-mt4-nt4-w4": (33, 640, 1000, 4, 4, True, False, False),
    "m63-k512-mt4-nt1-w4-zero-points-bias": (63, 512, 2048, 1, 4, False, True, False),
    "m63-k2048-mt4-nt2-w4": (63, 2048, 320, 2, 4, True, False, False),
}


@pytest.mark.parametrize("case", sorted(WGSPLIT_CASES))
def test_wgsplit_element_by_element(env, case, forms, knobs):
    m, k, n, nt, W, sym, bias, g_idx = WGSPLIT_CASES[case]
    mt = 1 if m <= 16 else (2 if m <= 32 else 4)
    if W is not None:
        assert W <= {1: 16, 2: 16 if nt == 1 else 8, 4: 4}[mt] and W * mt * nt <= 64, "a launch outside the kernel's bounds is not a test"
        knobs.set(W4_NT=nt, W4_W=W)
    if mt == 2:
        knobs.set(W4_LDSA=0)                                     # keeps the LDS kernel out at 17–32 rows
    assert mt < 4 or k * n < (12 << 20)
    run_forward(env, forms, "w4_wgsplit", "wgsplit " + case, m, k, n, sym, bias, g_idx)


# ── w4_gemm_ldsa_kernel (+ splitk_reduce_bias_kernel) ────────────────────────────────────────────────────────────────────
LDSA_CASES = {
    # (m, k, n, W4_LDSA_NW, W4_LDSA_S, symmetric, bias); S = 1 stores fp16 (+ bias) itself, S > 1 goes through the reduce
    "m17-k640-n320-s1-bias": (17, 640, 320, None, 1, True, True),
    "m31-k640-n320-s2-of-5-groups-bias": (31, 640, 320, None, 2, True, True),
    "m32-k640-n320-nw8-idle-waves-sG-zero-points": (32, 640, 320, 8, 5, False, False),
    "m32-k1024-n1000-nw8-s2": (32, 1024, 1000, 8, 2, True, False),
    "m17-k1024-n1000-sG-zero-points": (17, 1024, 1000, None, 8, False, False),
    "m33-k640-n320-mt4-s2": (33, 640, 320, None, 2, True, False),
    "m63-k1024-n1000-mt4-s1-zero-points": (63, 1024, 1000, None, 1, False, False),
    "m63-k640-n320-mt4-sG-bias": (63, 640, 320, None, 5, True, True),
}


@pytest.mark.parametrize("case", sorted(LDSA_CASES))
def test_ldsa_element_by_element(env, case, forms, knobs):
    m, k, n, nw, S, sym, bias = LDSA_CASES[case]
    knobs.set(W4_LDSA=2, W4_LDSA_S=S)
    if nw:
        knobs.set(W4_LDSA_NW=nw)
    run_forward(env, forms, "w4_ldsa", "ldsa " + case, m, k, n, sym, bias)


def test_ldsa_unforced_at_8192_by_2048(env, forms):
    """No knob: 32 rows of 8192 → 2048 (64 groups, 32 supertiles) are what the dispatcher sends to the LDS kernel on its own."""
    run_forward(env, forms, "w4_ldsa", "ldsa unforced 32x8192x2048", 32, 8192, 2048)


@pytest.mark.parametrize("m", [33, 63])
def test_tilep_one_ragged_tile_with_split_k(env, m, forms, knobs):
    """W4_TILE_MIN_M=33 on 2048 → 320: one ragged 64-row tile, 2 column workgroups, so the launcher splits K (S = 2: 16 groups,
    ≥ 8 per split) into slabs and reduces."""
    knobs.set(W4_TILE_MIN_M=33)
    run_forward(env, forms, "w4_tilep", f"tilep m={m} 2048x320", m, 2048, 320)


# ── the fp32 slab producers ──────────────────────────────────────────────────────────────────────────────────────────────
def _pad(v, to):
    return (v + to - 1) // to * to


SLAB_CASES = [(0, m, S) for m in (1, 16, 32) for S in (1, 3, "G")] + [(1, m, S) for m in (17, 32) for S in (0, "G")] + [(2, 64, 0), (2, 100, 0)]
SLAB_FORMS = ("w4_slabs", "w4_slabs_lds", "w4_slabs_tile")
SLAB_TAIL = 4096                              # NaN words after the extent the producer may write


def _produce_slabs(env, forms, form, m, S_req, k, n, sym):
    pkg, B, ctx, O, torch = env
    lin, w, _ = linear(env, k, n, sym)
    G = k // 128
    S_req = G if S_req == "G" else S_req
    rows_pad = {0: _pad(m, 16 if m <= 16 else (32 if m <= 32 else 64)), 1: 32, 2: _pad(m, 64)}[form]      # the documented geometry
    n_pad = _pad(n, 64)
    x = pb.f16r(np.random.default_rng(m * 17 + form).standard_normal((m, k)))
    xd = dev16(torch, x)
    ins = Unchanged(torch, xd)
    S_max = max(S_req, G if form else 1, 1)
    buf = torch.full((S_max * rows_pad * n_pad + SLAB_TAIL,), NAN, dtype=torch.float32, device="cuda")
    forms.reset()
    S, rp, npad = lin.slabs(ctx, xd, buf, m, form, S_req)
    ctx.sync()
    forms.require(SLAB_FORMS[form], absent=tuple(f for f in SLAB_FORMS + DENSE_FORMS if f != SLAB_FORMS[form]))
    ins.check()
    assert (rp, npad) == (rows_pad, n_pad), (rp, npad)
    assert 1 <= S <= G and (S_req <= 0 or S == min(S_req, G))
    raw = buf.cpu().numpy()
    extent = S * rows_pad * n_pad
    assert np.all(np.isnan(raw[extent:])), "words beyond S·rows_pad·n_pad were written"
    return x, w, raw[:extent].reshape(S, rows_pad, n_pad), S, buf


@pytest.mark.parametrize("form,m,S_req", SLAB_CASES)
@pytest.mark.parametrize("sym", [True, False])
def test_slab_producers_element_by_element(env, forms, form, m, S_req, sym):
    """The float64 sum of the S fp32 slabs over [m][n] against the out_f32 bound with the full k."""
    k, n = (640, 1000) if form == 0 else (2048, 320)
    x, w, slabs, S, _ = _produce_slabs(env, forms, form, m, S_req, k, n, sym)
    if form == 1 and S_req == 0:
        assert S == 2                                            # the heuristic at 2048 → 320: 2 workgroups, 16 groups, ≥ 8 per split
    if form == 2:
        assert S == 2                                            # same rule in the tile launcher
    ref, absdot = pb.gemm_refs(x, w)
    got = slabs[:, :m, :n].astype(np.float64).sum(axis=0)
    what = f"{SLAB_FORMS[form]} m={m} S={S} {k}x{n} {'symmetric' if sym else 'zero points'}"
    _note(SLAB_FORMS[form], pb.assert_gemm_elementwise(ref, absdot, got, k, False, what, out_f32=True), what)


def test_lds_slabs_feed_the_sandwich_consumer(env, forms):
    """End to end: w4_gemm_dense_slabs_lds's slabs and geometry go straight to ferrum_hip_sandwich_add_rms_norm_f32_slabs; the
    result is held by the norm-family bounds computed from the device's own slabs."""
    import ctypes as C
    pkg, B, ctx, O, torch = env
    m, k, n, eps = 31, 2048, 320, 1e-6
    x, w, slabs, S, buf = _produce_slabs(env, forms, 1, m, 0, k, n, True)
    rows_pad, n_pad = slabs.shape[1:]
    rng = np.random.default_rng(31)
    wb, wn = pb.mixed_sign_weight(rng, n), pb.mixed_sign_weight(rng, n)
    r0 = (3 * rng.standard_normal((m, n))).astype(np.float32)
    res = torch.full((m + 1, n), NAN, dtype=torch.float32, device="cuda")
    res[:m] = dev32(torch, r0)
    res[m] = 7.0
    out = poisoned(torch, m, n)
    wbd, wnd = dev16(torch, wb), dev16(torch, wn)
    ins = Unchanged(torch, buf, wbd, wnd)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert ctx.lib.ferrum_hip_sandwich_add_rms_norm_f32_slabs(p(buf), S, C.c_size_t(rows_pad * n_pad), n_pad, p(wbd), p(res), p(wnd),
                                                              C.c_float(eps), p(out), m, n, None, ctx.stream) == 0
    ctx.sync()
    ins.check()
    got_res = res.cpu().numpy()
    assert np.all(got_res[m] == 7.0)
    branch = pb.slabs_to_f16(slabs[:, :m, :n])
    _note("slabs → sandwich", pb.assert_sandwich_residual(branch, wb, r0, eps, got_res[:m], "sandwich residual from w4_slabs_lds"), "sandwich residual")
    _note("slabs → sandwich", pb.assert_rms_norm_elementwise(got_res[:m], wn, eps, guarded_rows(out, m, "sandwich norm_out"), "sandwich norm_out"), "sandwich norm_out")


# ── the fused combine + add + norm prologue ──────────────────────────────────────────────────────────────────────────────
def _tail_inputs(torch, m, k, top_k, seed):
    rng = np.random.default_rng(seed)
    down = pb.f16r(rng.standard_normal((m * top_k, k)))
    wts = rng.random((m, top_k)).astype(np.float32) + np.float32(0.1)
    wts = (wts / wts.sum(axis=1, keepdims=True)).astype(np.float32)
    r_in = 2 * rng.standard_normal((m, k))
    r_in[0, -8:] = 30.0 * rng.choice([-1.0, 1.0], 8)            # row 0: most of its energy in the last vector (a wrong row sum shows)
    r_in = pb.f16r(r_in)
    ln = pb.mixed_sign_weight(rng, k)
    return down, wts, r_in, ln


def _run_fused_tail(env, forms, lin, w, m, k, n, top_k, what):
    """One fused forward, held as tests/parity_bounds.py derives it → (device out, tolerance of out)."""
    pkg, B, ctx, O, torch = env
    eps = 1e-6
    down, wts, r_in, ln = _tail_inputs(torch, m, k, top_k, m * 100 + top_k + k)
    dd, wd, rd, ld = dev16(torch, down), dev32(torch, wts.reshape(-1)), dev16(torch, r_in), dev16(torch, ln)
    ins = Unchanged(torch, dd, wd, rd, ld)
    r_out, out = poisoned(torch, m, k), poisoned(torch, m, n)
    forms.reset()
    lin.forward_fused_tail(ctx, dd, wd, rd, r_out, ld, eps, top_k, out, m)
    ctx.sync()
    forms.require("w4_fused_tail", absent=("w4_ldsa", "w4_tilep", "w4_big"))
    ins.check()                                                  # residual_in among them
    res = guarded_rows(r_out, m, what + " residual_out")
    ref_r, tol_r = pb.fused_tail_residual_ref_tol(down, wts, r_in, m, top_k)
    _note("w4_fused_tail residual_out", pb.assert_within(ref_r, tol_r, res, what + " residual_out"), what + " residual_out")
    ref, tol = pb.fused_tail_gemm_ref_tol(res, ln, eps, w)       # from the DEVICE's residual_out
    got = guarded_rows(out, m, what)
    _note("w4_fused_tail out", pb.assert_within(ref, tol, got, what), what)
    return (dd, wd, rd, ld, eps), got, tol


@pytest.mark.parametrize("k,n,sym", [(512, 320, True), (512, 320, False), (2048, 1000, True), (2048, 1000, False)])
def test_fused_tail_element_by_element(env, forms, k, n, sym):
    """m ∈ {1, 3, 4} × top_k ∈ {1, 2, 8, 9} (nine enters the kernel's second expert loop): residual_out and out in bound, and
    the same out against the two-launch chain (moe_combine_add_rms_norm, then forward) under twice the element bound."""
    pkg, B, ctx, O, torch = env
    lin, w, _ = linear(env, k, n, sym)
    for m in (1, 3, 4):
        assert lin.can_fuse_tail(m)
        for top_k in (1, 2, 8, 9):
            what = f"fused tail m={m} top_k={top_k} {k}x{n} {'symmetric' if sym else 'zero points'}"
            (dd, wd, rd, ld, eps), got, tol = _run_fused_tail(env, forms, lin, w, m, k, n, top_k, what)
            res2, norm2, out2 = rd.clone(), poisoned(torch, m, k), poisoned(torch, m, n)
            B.moe_combine_add_rms_norm(ctx, dd, wd, res2, ld, eps, norm2, m, top_k, k)
            lin.forward(ctx, norm2, out2, m)
            ctx.sync()
            pb.assert_within(guarded_rows(out2, m, what + " two-op chain"), 2.0 * tol, got, what + " against the two-op chain")


@pytest.mark.parametrize("k", [4096, 8192])
def test_fused_tail_predicate_and_launcher_agree(env, forms, knobs, k):
    """Wherever can_fuse_tail answers 1 the fused forward returns 0 (and is right); where it answers 0 the forward refuses on
    the host.  The rows live in LDS beside the launch's reduction buffer [W][NT·4][64] fp32, so the answer depends on the
    launch shape: at K = 8192 three rows need W·NT ≤ 15 (NT = 4, W = 4 asks for 65,840 bytes) and four rows never fit."""
    pkg, B, ctx, O, torch = env
    n = 1024
    lin, w, _ = linear(env, k, n, True)
    answers = {}
    for shape in ({}, {"W4_NT": 4, "W4_W": 4}, {"W4_NT": 1, "W4_W": 8}):
        knobs.set(W4_NT=shape.get("W4_NT"), W4_W=shape.get("W4_W"))
        for m in (1, 2, 3, 4):
            what = f"fused tail K={k} m={m} {shape or 'default shape'}"
            answers[(tuple(shape.values()), m)] = ok = lin.can_fuse_tail(m)
            if ok:
                _run_fused_tail(env, forms, lin, w, m, k, n, 2, what)      # rc 0, or _check raises
            else:
                down, wts, r_in, ln = _tail_inputs(torch, m, k, 2, m)
                r_out, out = poisoned(torch, m, k), poisoned(torch, m, n)
                with pytest.raises(RuntimeError, match="rc=2"):
                    lin.forward_fused_tail(ctx, dev16(torch, down), dev32(torch, wts.reshape(-1)), dev16(torch, r_in), r_out,
                                           dev16(torch, ln), 1e-6, 2, out, m)
                ctx.sync()
                assert np.all(np.isnan(host(r_out)[:m])) and np.all(np.isnan(host(out)[:m])), what + ": refused, yet something was written"
    if k == 8192:
        # W·NT·1024 + m·(8192 + 8)·2 + 256 ≤ 65536
        assert answers[((4, 4), 2)] and not answers[((4, 4), 3)] and answers[((1, 8), 3)]
        assert not any(ok for (shape, m), ok in answers.items() if m == 4)
    else:
        assert all(answers.values())                             # 4 rows of 4096: 32,832 + 256 bytes beside ≤ 16 KiB


# ── fp16 GEMMs (router, lm_head, DenseLinear) ────────────────────────────────────────────────────────────────────────────
F16_ROWS = (1, 16, 17, 32, 33, 64, 65)


def _f16_case(env, ms, n, k, what):
    """B.gemm (row-major W) and B.gemm_f16t (tiled W), fp16 and fp32 out, for every m of `ms` on one weight."""
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(n * 31 + k)
    w = pb.f16r(rng.standard_normal((n, k)) / np.sqrt(k))
    wd = dev16(torch, w)
    wt = B.dense_repack_f16t(ctx, wd, n, k)
    ctx.sync()
    for m in ms:
        x = pb.f16r(rng.standard_normal((m, k)))
        xd = dev16(torch, x)
        ins = Unchanged(torch, xd, wd, wt)
        ref, absdot = pb.gemm_refs(x, w)
        for name, fn, wdev in (("f16_gemm", B.gemm, wd), ("f16t_gemm", B.gemm_f16t, wt)):
            for f32 in (False, True):
                out = poisoned(torch, m, n, torch.float32 if f32 else torch.float16)
                fn(ctx, xd, wdev, out, m, n, k)
                ctx.sync()
                case = f"{name}{' f32 out' if f32 else ''} {what} m={m}"
                got = out.cpu().numpy().astype(np.float64)
                assert np.all(got[m] == 7.0), case
                WORST[name + (" f32 out" if f32 else "")] = max(WORST.get(name + (" f32 out" if f32 else ""), 0.0),
                                                               pb.assert_gemm_elementwise(ref, absdot, got[:m], k, False, case, out_f32=f32))
        ins.check()


@pytest.mark.parametrize("k", [256, 1120, 2048])
@pytest.mark.parametrize("n", [96, 104, 1511])
def test_f16_gemms_element_by_element(env, n, k):
    """The launcher's rule (f16_gemm_impl): S doubles while tasks·S < 2048 and 2·S ≤ (K/32)/8, tasks = ⌈N/32⌉·row blocks ≤ 96 here.
    K = 256: 8 k-steps, S = 1, two trips of the 4-unrolled loop.  K = 1120: 35 k-steps, 35/8 = 4 → S = 4, slices of 8, 9, 9, 9
    k-steps: uneven, and three of them end in the remainder loop.  K = 2048: 64 k-steps → S = 8, slices of 8, plus the reduce.
    N = 96 / 104 / 1511: whole 32-column pairs, a partial 16-column tile, a partial pair at an odd width."""
    _f16_case(env, F16_ROWS, n, k, f"{k}x{n}")
    print(f"fp16 GEMMs {k}x{n}: " + ", ".join(f"{f} {v:.3f}" for f, v in sorted(WORST.items()) if f.startswith("f16")))


@pytest.mark.parametrize("n", [32768 + 64, 32768 + 64 + 32])
def test_f16t_wide_form_and_its_neighbour(env, n):
    """17 and 32 rows against N ≥ 32768 with N % 64 == 0 and S = 1 (K = 128: 4 k-steps) take f16t_gemm_kernel<2, ·, 4>, 64 columns
    per wave; N + 32 is no multiple of 64, must not take it and must still be right (the row-major kernel never takes it)."""
    assert (n % 64 == 0) == (n == 32768 + 64)
    _f16_case(env, (17, 32), n, 128, f"128x{n}")
