"""Element-wise parity of the norm family (csrc/norm.hip) through the C ABI: the head and tail of a forward
(embed_rms_norm, gather_rms_norm), the fp32 residual stream's sandwich update in branch and slab form and both thread
shapes, rms_norm_f32_to_f16, the slab-input gated activations, gather_columns, add_bias — and rms_norm,
fused_add_rms_norm, layer_norm, gelu and fused_*_mul_split, which tests/test_ops_gpu.py holds to a whole-tensor NMSE only.

Every element is held against a float64 reference with the bounds of tests/parity_bounds.py ("norm family": derived from
the number formats, self-tested on the CPU by tests/test_parity_bounds.py); stores that involve one rounding of an exact
value are held bit for bit.  Shapes sit on the kernels' seams: the 256-thread chunk boundaries (2048 / 2056, 4104, 8192 / 8200),
the CHUNKS template instances (1, 2, 4 and — for five chunks — 8), 64 / 65 rows, rows narrower than one wave.  Every output
is NaN-poisoned before the call, lies between two guard rows that must keep their bit pattern, and every input must come back
unchanged."""
import ctypes as C

import numpy as np
import pytest

from tests import parity_bounds as pb

pytestmark = pytest.mark.gpu

DIMS = [8, 248, 2048, 2056, 4104, 5376, 8192]
DIMS_WIDE = DIMS + [8200, 16384]              # the fp16 row norms go to 16384; 8200 is five chunks (the 8-chunk instance)
ROWS = [1, 3, 64, 65]
EPS = (1e-6, 1e-5)
PAT16, PAT32 = 0x7E5A, 0x7FC5A5A5             # NaN bit patterns of the poison
WORST = {}                                    # op → largest err/tol seen (printed at module teardown; information only)


@pytest.fixture(scope="module")
def env():
    import torch
    import __graft_entry__ as ge
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    pkg = ge.load_package()
    pkg.load_library()          # raises if the HIP extension is missing — no fallback
    ctx = pkg.HipBackend.new_context(1 << 20)
    yield pkg, ctx, torch
    ctx.sync()
    print("\nnorm family, largest err/tol per op: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def _note(op, ratio):
    WORST[op] = max(WORST.get(op, 0.0), ratio)


def _case_id(dim, rows, dims=DIMS_WIDE):
    return dims.index(dim) * len(ROWS) + ROWS.index(rows)


def _p(t):
    return C.c_void_p(0 if t is None else (t.ptr if isinstance(t, Guarded) else t.data_ptr()))


def _f(v):
    return C.c_float(v)


class Guarded:
    """[rows, dim] device buffer between two guard rows, all of it NaN poison (`init` fills the rows)."""

    def __init__(self, torch, rows, dim, f32=False, init=None):
        self.torch, self.rows_n, self.f32 = torch, rows, f32
        self.idt, self.pat = (torch.int32, PAT32) if f32 else (torch.int16, PAT16)
        self.raw = torch.full((rows + 2, dim), self.pat, dtype=self.idt, device="cuda")
        self.t = self.raw.view(torch.float32 if f32 else torch.float16)
        self.ptr = self.t[1:].data_ptr()
        if init is not None:
            self.t[1:rows + 1].copy_(torch.from_numpy(np.ascontiguousarray(init, np.float32 if f32 else np.float16)))

    def host(self):
        """The rows as float32 numpy, after asserting that both guard rows kept their bits."""
        raw = self.raw.cpu().numpy()
        assert (raw[0] == self.pat).all() and (raw[-1] == self.pat).all(), "a guard row was written"
        return self.t[1:self.rows_n + 1].float().cpu().numpy()

    def bits(self):
        return self.raw[1:self.rows_n + 1].cpu().numpy().copy()

    def untouched(self):
        return bool((self.raw == self.pat).all().item())


def _h16(torch, a):
    with np.errstate(over="ignore"):
        return torch.from_numpy(np.ascontiguousarray(a).astype(np.float16)).cuda()


def _f32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _i32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


class _Inputs:
    """Device inputs that must come back bit for bit."""

    def __init__(self, torch, *tensors):
        self.torch = torch
        self.pairs = [(t, t.clone()) for t in tensors if t is not None]

    def unchanged(self):
        for t, c in self.pairs:
            it = self.torch.int16 if t.element_size() == 2 else self.torch.int32
            assert self.torch.equal(t.view(it), c.view(it)), "an input buffer was modified"


def _f16mul(x, scale):
    """float16(float32(x)·float32(scale)) — the scaled embedding row."""
    return (np.asarray(x, np.float32) * np.float32(scale)).astype(np.float16).astype(np.float32)


def _zero_rows_are_zero(kinds, got):
    for i, k in enumerate(kinds):
        if k == "zero":
            assert np.all(got[i] == 0.0), f"row {i} (all-zero input) is not zero"


# ── rms_norm, fused_add_rms_norm (+ out_perm) ────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dim", DIMS_WIDE)
def test_rms_norm_and_fused_add_elementwise(env, dim, rows):
    pkg, ctx, torch = env
    lib, cid = ctx.lib, _case_id(dim, rows)
    rng = np.random.default_rng(1000 + cid)
    x, kinds = pb.norm_rows(rng, rows, dim, start=cid)
    w = pb.mixed_sign_weight(rng, dim)
    xd, wd = _h16(torch, x), _h16(torch, w)
    ins = _Inputs(torch, xd, wd)
    for eps in EPS:
        out = Guarded(torch, rows, dim)
        assert lib.ferrum_hip_rms_norm_f16(_p(xd), _p(wd), _f(eps), _p(out), rows, dim, ctx.stream) == 0
        got = out.host()
        _note("rms_norm", pb.assert_rms_norm_elementwise(x, w, eps, got, f"rms_norm {rows}x{dim} eps {eps}"))
        _zero_rows_are_zero(kinds, got)
    # fused add: the residual is one fp16 rounding of r + x (bit-exact); the norm is taken from the rounded residual
    eps = EPS[cid % 2]
    r = 0.05 * pb.norm_rows(rng, rows, dim, start=cid)[0]
    for i, k in enumerate(kinds):
        if k in ("normal", "first", "last", "v255", "v256"):
            r[i] += 3.0 * rng.standard_normal(dim)
    r = pb.f16r(r)
    res_ref = pb.f16r(r + x)
    assert np.all(np.isfinite(res_ref))
    res, out = Guarded(torch, rows, dim, init=r), Guarded(torch, rows, dim)
    assert lib.ferrum_hip_fused_add_rms_norm_f16(_p(res), _p(xd), _p(wd), _f(eps), _p(out), rows, dim, ctx.stream) == 0
    got_res, got = res.host(), out.host()
    assert np.array_equal(got_res, res_ref), "fused_add residual is not f16(r + x)"
    _note("fused_add_rms_norm", pb.assert_rms_norm_elementwise(got_res, w, eps, got, f"fused_add_rms_norm {rows}x{dim}"))
    _zero_rows_are_zero(kinds, got)
    # gathered store: exactly the same values, column j from column perm[j]
    perm = rng.permutation(dim).astype(np.int32)
    pd = _i32(torch, perm)
    ins_p = _Inputs(torch, pd)
    res2, out2 = Guarded(torch, rows, dim, init=r), Guarded(torch, rows, dim)
    assert lib.ferrum_hip_fused_add_rms_norm_perm_f16(_p(res2), _p(xd), _p(wd), _f(eps), _p(out2), rows, dim, _p(pd), ctx.stream) == 0
    out2.host(), res2.host()
    assert np.array_equal(res2.bits(), res.bits())
    assert np.array_equal(out2.bits(), out.bits()[:, perm]), "out_perm store differs from out[:, perm]"
    ins.unchanged(), ins_p.unchanged()


# ── embed_rms_norm ───────────────────────────────────────────────────────────────────────────────────────────────────────
SCALES = (0.0, 4.0, float(np.sqrt(5376.0)))


def _embed_table(rng, vocab, dim, start, scale):
    table, kinds = pb.norm_rows(rng, vocab, dim, start=start)
    if scale != 0.0:
        for i, k in enumerate(kinds):
            if k == "big":
                table[i] /= 128.0                     # exact; the scaled row stays a finite fp16
    return table, kinds


def _run_embed(env, rng, dim, rows, scale, copies, n_zero, with_perm, eps, start, what):
    pkg, ctx, torch = env
    vocab = 11
    table, tkinds = _embed_table(rng, vocab, dim, start, scale)
    ids = np.concatenate([[vocab - 1, 0, vocab - 1, 0, 3], rng.integers(0, vocab, max(rows - 5, 0))])[:rows].astype(np.uint32)
    w = pb.mixed_sign_weight(rng, dim)
    td, wd = _h16(torch, table), _h16(torch, w)
    idd = torch.from_numpy(ids.view(np.int32)).cuda()
    perm = rng.permutation(dim).astype(np.int32) if with_perm else None
    pd = _i32(torch, perm) if with_perm else None
    ins = _Inputs(torch, td, wd, idd, pd)
    out = Guarded(torch, rows, dim)
    c16 = Guarded(torch, rows, dim) if copies in ("f16", "both") else None
    c32 = Guarded(torch, rows, dim, f32=True) if copies == "both" else None
    words = torch.arange(1, n_zero + 10, dtype=torch.int32, device="cuda")          # non-zero counters, and words after them
    words_before = words.cpu().numpy().copy()
    rc = ctx.lib.ferrum_hip_embed_rms_norm_f16(_p(td), _p(idd), _f(scale), _p(c16), _p(c32), _p(wd), _f(eps), _p(out), rows, dim,
                                               _p(words) if n_zero else None, n_zero, _p(pd), ctx.stream)
    assert rc == 0
    scaled = table[ids] if scale == 0.0 else _f16mul(table[ids], scale)
    assert np.all(np.isfinite(scaled))
    got = out.host()
    if with_perm:
        inv = np.empty_like(perm)
        inv[perm] = np.arange(dim, dtype=np.int32)
        got = got[:, inv]                              # got_perm[:, j] = y[:, perm[j]]  →  y = got_perm[:, inv]
    _note("embed_rms_norm", pb.assert_rms_norm_elementwise(scaled, w, eps, got, what))
    _zero_rows_are_zero([tkinds[i] for i in ids], got)
    if c16 is not None:
        assert np.array_equal(c16.host(), scaled), f"{what}: fp16 residual copy is not f16(f32(x)·f32(scale))"
    if c32 is not None:
        assert np.array_equal(c32.host(), scaled), f"{what}: fp32 residual copy is not the fp16 value widened"
    after = words.cpu().numpy()
    assert np.all(after[:n_zero] == 0), f"{what}: zero_words not cleared"
    assert np.array_equal(after[n_zero:], words_before[n_zero:]), f"{what}: words past n_zero were written"
    ins.unchanged()


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dim", DIMS_WIDE)
def test_embed_rms_norm_elementwise(env, dim, rows):
    cid = _case_id(dim, rows)
    rng = np.random.default_rng(2000 + cid)
    # 36 cases walk every (scale, copies) pair four times; n_zero and out_perm rotate against them
    _run_embed(env, rng, dim, rows, SCALES[cid % 3], ("f16", "both", "none")[(cid // 3) % 3], (0, 1, 300)[(cid + cid // 3) % 3],
               cid % 2 == 1, EPS[(cid // 2) % 2], cid, f"embed_rms_norm {rows}x{dim}")


@pytest.mark.parametrize("n_zero", [0, 1, 300])
@pytest.mark.parametrize("rows", [1, 5])
def test_embed_rms_norm_rearms_the_counters(env, rows, n_zero):
    """Block 0 clears zero_words in a loop of stride 256: 300 words need its second trip; with 5 rows, four more blocks run
    that must not clear anything."""
    rng = np.random.default_rng(2100 + rows * 7 + n_zero)
    for copies in ("f16", "both", "none"):
        _run_embed(env, rng, 248, rows, SCALES[1], copies, n_zero, False, 1e-6, rows, f"embed_rms_norm re-arm {rows} rows, {n_zero} words")


# ── gather_rms_norm, rms_norm_f32_to_f16 ─────────────────────────────────────────────────────────────────────────────────
def _row_idx(rng, rows, n_src):
    """Non-monotonic, with repeats, includes the last source row."""
    if rows == 1:
        return np.array([n_src - 1], np.int32)
    idx = rng.integers(0, n_src, rows).astype(np.int32)
    idx[0], idx[1], idx[2] = n_src - 1, 2, 2
    return idx


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dim", DIMS_WIDE)
def test_gather_rms_norm_elementwise(env, dim, rows):
    pkg, ctx, torch = env
    cid = _case_id(dim, rows)
    rng = np.random.default_rng(3000 + cid)
    n_src = rows + 5
    src, kinds = pb.norm_rows(rng, n_src, dim, start=cid)
    idx = _row_idx(rng, rows, n_src)
    src[np.setdiff1d(np.arange(n_src), idx)] = np.nan            # rows nobody sampled
    w, eps = pb.mixed_sign_weight(rng, dim), EPS[cid % 2]
    sd, wd, idd = _h16(torch, src), _h16(torch, w), _i32(torch, idx)
    ins = _Inputs(torch, sd, wd, idd)
    out = Guarded(torch, rows, dim)
    assert ctx.lib.ferrum_hip_gather_rms_norm_f16(_p(sd), _p(idd), _p(wd), _f(eps), _p(out), rows, dim, ctx.stream) == 0
    got = out.host()
    _note("gather_rms_norm", pb.assert_rms_norm_elementwise(src[idx], w, eps, got, f"gather_rms_norm {rows}x{dim}"))
    _zero_rows_are_zero([kinds[i] for i in idx], got)
    ins.unchanged()


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dim", DIMS)
def test_rms_norm_f32_to_f16_elementwise(env, dim, rows):
    pkg, ctx, torch = env
    cid = _case_id(dim, rows, DIMS)
    rng = np.random.default_rng(4000 + cid)
    n_src = rows + 5
    base, kinds = pb.norm_rows(rng, n_src, dim, start=cid)
    src = (base * (1.0 + 1e-3 * rng.standard_normal(base.shape))).astype(np.float32)      # fp32-valued: all 24 bits in use
    idx = _row_idx(rng, rows, n_src)
    w, eps = pb.mixed_sign_weight(rng, dim), EPS[cid % 2]
    wd = _h16(torch, w)
    full = _f32(torch, src[:rows])                                # null row_idx: row i from row i
    ins = _Inputs(torch, full, wd)
    out = Guarded(torch, rows, dim)
    assert ctx.lib.ferrum_hip_rms_norm_f32_to_f16(_p(full), None, _p(wd), _f(eps), _p(out), rows, dim, ctx.stream) == 0
    got = out.host()
    _note("rms_norm_f32_to_f16", pb.assert_rms_norm_elementwise(src[:rows], w, eps, got, f"rms_norm_f32_to_f16 {rows}x{dim}"))
    _zero_rows_are_zero(kinds[:rows], got)
    ins.unchanged()
    src[np.setdiff1d(np.arange(n_src), idx)] = np.nan
    sd, idd = _f32(torch, src), _i32(torch, idx)
    ins = _Inputs(torch, sd, idd, wd)
    out = Guarded(torch, rows, dim)
    assert ctx.lib.ferrum_hip_rms_norm_f32_to_f16(_p(sd), _p(idd), _p(wd), _f(eps), _p(out), rows, dim, ctx.stream) == 0
    got = out.host()
    _note("rms_norm_f32_to_f16", pb.assert_rms_norm_elementwise(src[idx], w, eps, got, f"rms_norm_f32_to_f16 row_idx {rows}x{dim}"))
    _zero_rows_are_zero([kinds[i] for i in idx], got)
    ins.unchanged()


# ── sandwich_add_rms_norm_f32: branch and slabs, 256-thread and wide kernels ─────────────────────────────────────────────
SLAB_COUNTS = (1, 3, 8, 9)
SANDWICH_CASES = [(d, r, wide) for d in DIMS for r in ROWS for wide in (1, 0) if not (r == 65 and wide == 0)]
# 65 rows: above the wide kernel's limit, the default knob already runs the 256-thread kernel


def _sandwich_check(ctx, torch, call, branch, wb, wn, r0, eps, rows, dim, perm, what):
    """Runs `call(residual, w_next or None, norm_out, perm or None)` three times from the same residual: with w_next, with
    w_next null, with the gathered store."""
    res, out = Guarded(torch, rows, dim, f32=True, init=r0), Guarded(torch, rows, dim)
    assert call(res, True, out, None) == 0
    got_res, got = res.host(), out.host()
    _note("sandwich residual", pb.assert_sandwich_residual(branch, wb, r0, eps, got_res, what + " residual"))
    # norm_out from the residual the device returned: with the residual bound above, no slack for a wrong intermediate
    _note("sandwich norm_out", pb.assert_rms_norm_elementwise(got_res, wn, eps, got, what + " norm_out"))
    res_n, out_n = Guarded(torch, rows, dim, f32=True, init=r0), Guarded(torch, rows, dim)
    assert call(res_n, False, out_n, None) == 0
    res_n.host(), out_n.host()
    assert np.array_equal(res_n.bits(), res.bits()), what + ": residual differs without w_next"
    assert out_n.untouched(), what + ": norm_out written although w_next is null"
    res_p, out_p = Guarded(torch, rows, dim, f32=True, init=r0), Guarded(torch, rows, dim)
    assert call(res_p, True, out_p, perm) == 0
    res_p.host(), out_p.host()
    assert np.array_equal(res_p.bits(), res.bits()), what + ": residual differs with out_perm"
    assert np.array_equal(out_p.bits(), out.bits()[:, perm]), what + ": out_perm store differs from norm_out[:, perm]"


@pytest.mark.parametrize("dim,rows,wide", SANDWICH_CASES)
def test_sandwich_add_rms_norm_f32_elementwise(env, knobs, dim, rows, wide):
    pkg, ctx, torch = env
    lib = ctx.lib
    if not wide:
        knobs.set(SANDWICH_WIDE=0)
    cid = _case_id(dim, rows, DIMS)
    rng = np.random.default_rng(5000 + cid)
    eps = EPS[cid % 2]
    target, kinds = pb.norm_rows(rng, rows, dim, start=cid)
    wb, wn = pb.mixed_sign_weight(rng, dim), pb.mixed_sign_weight(rng, dim)
    r0 = (3 * rng.standard_normal((rows, dim))).astype(np.float32)
    perm = rng.permutation(dim).astype(np.int32)
    bd, wbd, wnd, pd = _h16(torch, target), _h16(torch, wb), _h16(torch, wn), _i32(torch, perm)
    ins = _Inputs(torch, bd, wbd, wnd, pd)

    def branch_call(res, with_next, out, p):
        if p is None:
            return lib.ferrum_hip_sandwich_add_rms_norm_f32(_p(bd), _p(wbd), _p(res), _p(wnd) if with_next else None, _f(eps), _p(out),
                                                            rows, dim, ctx.stream)
        return lib.ferrum_hip_sandwich_add_rms_norm_f32_perm(_p(bd), _p(wbd), _p(res), _p(wnd) if with_next else None, _f(eps), _p(out),
                                                             rows, dim, _p(pd), ctx.stream)
    _sandwich_check(ctx, torch, branch_call, target, wb, wn, r0, eps, rows, dim, perm, f"sandwich {rows}x{dim} wide={wide}")
    ins.unchanged()
    ld, rows_pad = dim + 8, rows + 2                             # padded columns and padded rows hold NaN
    for S in (SLAB_COUNTS[cid % 4], SLAB_COUNTS[(cid + 2) % 4]):
        slabs = pb.split_into_slabs(rng, target, S)
        branch = pb.slabs_to_f16(slabs)
        assert np.all(np.isfinite(branch))
        padded = np.full((S, rows_pad, ld), np.nan, np.float32)
        padded[:, :rows, :dim] = slabs
        sd = _f32(torch, padded)
        ins_s = _Inputs(torch, sd, wbd, wnd, pd)

        def slab_call(res, with_next, out, p):
            return lib.ferrum_hip_sandwich_add_rms_norm_f32_slabs(_p(sd), S, C.c_size_t(rows_pad * ld), ld, _p(wbd), _p(res),
                                                                  _p(wnd) if with_next else None, _f(eps), _p(out), rows, dim,
                                                                  _p(pd) if p is not None else None, ctx.stream)
        _sandwich_check(ctx, torch, slab_call, branch, wb, wn, r0, eps, rows, dim, perm, f"sandwich slabs S={S} {rows}x{dim} wide={wide}")
        ins_s.unchanged()


@pytest.mark.parametrize("dim", [8200, 12])
def test_sandwich_rejects_dims_it_cannot_hold(env, dim):
    pkg, ctx, torch = env
    lib, rows = ctx.lib, 3
    z16 = _h16(torch, np.ones((rows, dim)))
    wd = _h16(torch, np.ones(dim))
    slabs = _f32(torch, np.ones((2, rows, dim)))
    r0 = np.ones((rows, dim), np.float32)
    res, out = Guarded(torch, rows, dim, f32=True, init=r0), Guarded(torch, rows, dim)
    before = res.bits()
    assert lib.ferrum_hip_sandwich_add_rms_norm_f32(_p(z16), _p(wd), _p(res), _p(wd), _f(1e-6), _p(out), rows, dim, ctx.stream) == 2
    assert lib.ferrum_hip_sandwich_add_rms_norm_f32_perm(_p(z16), _p(wd), _p(res), _p(wd), _f(1e-6), _p(out), rows, dim, None, ctx.stream) == 2
    assert lib.ferrum_hip_sandwich_add_rms_norm_f32_slabs(_p(slabs), 2, C.c_size_t(rows * dim), dim, _p(wd), _p(res), _p(wd), _f(1e-6),
                                                          _p(out), rows, dim, None, ctx.stream) == 2
    assert lib.ferrum_hip_rms_norm_f32_to_f16(_p(res.t[1:]), None, _p(wd), _f(1e-6), _p(out), rows, dim, ctx.stream) == 2
    ctx.sync()
    res.host()
    assert np.array_equal(res.bits(), before) and out.untouched()


# ── gated activations from slabs ─────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("gelu", [0, 1])
@pytest.mark.parametrize("S", [1, 2, 8, 9])
@pytest.mark.parametrize("im", [8, 2048, 2056])
def test_fused_gated_act_slabs_elementwise(env, im, S, gelu):
    pkg, ctx, torch = env
    lib, rows = ctx.lib, 3
    rng = np.random.default_rng(6000 + im + S)
    target = pb.gated_inputs(rng, rows, im)
    slabs = pb.split_into_slabs(rng, target.reshape(-1, 1), S).reshape(S, rows, 2 * im)    # per-element slab magnitudes
    gu = pb.slabs_to_f16(slabs)                                   # the fp16 gate_up the kernel forms, exactly
    assert np.all(np.isfinite(gu)) and np.max(np.abs(gu[:, :im])) >= 65000
    ld, rows_pad = 2 * im + 8, rows + 1
    padded = np.full((S, rows_pad, ld), np.nan, np.float32)
    padded[:, :rows, :2 * im] = slabs
    sd, gud = _f32(torch, padded), _h16(torch, gu)
    ins = _Inputs(torch, sd, gud)
    out, out_split = Guarded(torch, rows, im), Guarded(torch, rows, im)
    assert lib.ferrum_hip_fused_gated_act_slabs_f16(_p(sd), S, C.c_size_t(rows_pad * ld), ld, _p(out), rows, im, gelu, ctx.stream) == 0
    split = lib.ferrum_hip_fused_gelu_tanh_mul_split_f16 if gelu else lib.ferrum_hip_fused_silu_mul_split_f16
    assert split(_p(gud), _p(out_split), rows, im, ctx.stream) == 0
    got = out.host()
    op = "gelu" if gelu else "silu"
    _note(f"gated_act_slabs {op}", pb.assert_gated_act_elementwise(gu, got, bool(gelu), f"gated_act_slabs {op} im={im} S={S}"))
    out_split.host()
    assert np.array_equal(out.bits(), out_split.bits()), "slab form is not bit-identical to reduce → fused_*_mul_split"
    ins.unchanged()


# ── gather_columns ───────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("cols", [8, 100, 5376, 32768, 32776])
def test_gather_columns_is_an_exact_copy(env, forms, cols, rows):
    """100 and 32776 take the scalar kernel (not a multiple of 8; past the LDS form's 32768 columns = 64 KiB of dynamic LDS)."""
    pkg, ctx, torch = env
    rng = np.random.default_rng(7000 + cols + rows)
    a = pb.f16r(rng.standard_normal((rows, cols)) * 100)
    a[:, -1], a[:, 0] = 65504.0, 2.0 ** -24                       # the row's two ends are recognisable
    ad = _h16(torch, a)
    for perm in (rng.permutation(cols).astype(np.int32), np.arange(cols - 1, -1, -1, dtype=np.int32)):
        pd = _i32(torch, perm)
        ins = _Inputs(torch, ad, pd)
        out = Guarded(torch, rows, cols)
        forms.reset()
        assert ctx.lib.ferrum_hip_gather_columns_f16(_p(ad), _p(pd), _p(out), rows, cols, ctx.stream) == 0, \
            ctx.lib.ferrum_hip_last_error()
        ctx.sync()
        forms.require("gather_columns")
        assert np.array_equal(out.host(), a[:, perm])
        ins.unchanged()


# ── add_bias ─────────────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("cols", [1, 257, 5120])
def test_add_bias_is_one_rounding(env, cols, rows):
    pkg, ctx, torch = env
    rng = np.random.default_rng(8000 + cols + rows)
    a = pb.f16r(rng.standard_normal((rows, cols)) * 50)
    b = pb.f16r(rng.standard_normal(cols) * np.where(rng.random(cols) < 0.5, 1e-3, 30.0))
    bd = _h16(torch, b)
    ins = _Inputs(torch, bd)
    data = Guarded(torch, rows, cols, init=a)
    assert ctx.lib.ferrum_hip_add_bias_f16(_p(data), _p(bd), rows, cols, ctx.stream) == 0
    assert np.array_equal(data.host(), pb.f16r(a + b[None, :]))
    ins.unchanged()


# ── the ops test_ops_gpu.py holds to an NMSE: one element-wise case each ─────────────────────────────────────────────────
@pytest.mark.parametrize("dim", [4100, 2056])
def test_layer_norm_and_gelu_elementwise(env, dim):
    pkg, ctx, torch = env
    lib, rows = ctx.lib, 3
    rng = np.random.default_rng(9000 + dim)
    x = pb.f16r(rng.standard_normal((rows, dim)) * 3 + 0.7)
    gam, beta = pb.mixed_sign_weight(rng, dim), pb.f16r(0.1 * rng.standard_normal(dim))
    xd, gd, bd = _h16(torch, x), _h16(torch, gam), _h16(torch, beta)
    ins = _Inputs(torch, xd, gd, bd)
    out = Guarded(torch, rows, dim)
    assert lib.ferrum_hip_layer_norm_f16(_p(xd), _p(gd), _p(bd), _f(1e-5), _p(out), rows, dim, ctx.stream) == 0
    ref, tol = pb.layer_norm_ref_tol(x, gam, beta, 1e-5)
    _note("layer_norm", pb.assert_within(ref, tol, out.host(), f"layer_norm {rows}x{dim}"))
    x[0, :4] = (-4.0, -6.0, 12.0, -12.0)
    xd = _h16(torch, x)
    ins2 = _Inputs(torch, xd)
    out = Guarded(torch, rows, dim)
    assert lib.ferrum_hip_gelu_f16(_p(xd), _p(out), C.c_size_t(rows * dim), ctx.stream) == 0
    gref = pb.gelu_erf_poly_ref64(x)
    _note("gelu", pb.assert_within(gref, pb.gelu_tanh_mul_tolerance(gref, x), out.host(), f"gelu {rows}x{dim}"))
    ins.unchanged(), ins2.unchanged()


@pytest.mark.parametrize("gelu", [0, 1])
def test_fused_mul_split_elementwise(env, gelu):
    pkg, ctx, torch = env
    rows, im = 3, 2056
    gu = pb.gated_inputs(np.random.default_rng(9500 + gelu), rows, im)
    gud = _h16(torch, gu)
    ins = _Inputs(torch, gud)
    out = Guarded(torch, rows, im)
    fn = ctx.lib.ferrum_hip_fused_gelu_tanh_mul_split_f16 if gelu else ctx.lib.ferrum_hip_fused_silu_mul_split_f16
    assert fn(_p(gud), _p(out), rows, im, ctx.stream) == 0
    op = "fused_gelu_tanh_mul_split" if gelu else "fused_silu_mul_split"
    _note(op, pb.assert_gated_act_elementwise(gu, out.host(), bool(gelu), op))
    ins.unchanged()
