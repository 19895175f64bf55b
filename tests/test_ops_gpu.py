"""GPU parity tests: every hot-path op through the C ABI (libferrum_hip.so) vs the CPU oracle on the
same seeded inputs.  Tolerances are the reference's own op_diff buckets
(ferrum-testkit/src/op_diff/mod.rs:46-49: NMSE fp16 1e-6, attention 5e-3, fp16 round-trip 3e-3)
unless a tighter one is written in the test; integer outputs are bit-exact."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NMSE_FP16_TOL = 1e-6
NMSE_ATTN_TOL = 5e-3


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


def f16r(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def nmse(ref, got):
    ref, got = np.asarray(ref, np.float64).ravel(), np.asarray(got, np.float64).ravel()
    return float(((ref - got) ** 2).mean() / max((ref ** 2).mean(), 1e-30))


def dev16(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda").half().contiguous()


def host(t):
    return t.float().cpu().numpy()


# ── norms / elementwise ──────────────────────────────────────────────────────
@pytest.mark.parametrize("tokens,dim", [(1, 768), (7, 1024), (3, 4100), (2, 8192)])
def test_layer_norm_and_gelu_core_ops(env, tokens, dim):
    # Backend::layer_norm / Backend::gelu (required core ops of the trait; CPU cpu.rs:2081-2122) + the event timer
    pkg, B, ctx, O, torch = env
    import ctypes as C
    rng = np.random.default_rng(dim * 3 + tokens)
    x = f16r(rng.standard_normal((tokens, dim)) * 3 + 0.7)
    g, b = f16r(1 + 0.2 * rng.standard_normal(dim)), f16r(0.1 * rng.standard_normal(dim))
    out = torch.empty(tokens, dim, dtype=torch.float16, device="cuda")
    lib = ctx.lib
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert lib.ferrum_hip_event_create(C.byref(e0)) == 0 and lib.ferrum_hip_event_create(C.byref(e1)) == 0
    assert lib.ferrum_hip_event_record(e0, ctx.stream) == 0
    B.layer_norm(ctx, dev16(torch, x), dev16(torch, g), dev16(torch, b), 1e-5, out, tokens, dim)
    assert lib.ferrum_hip_event_record(e1, ctx.stream) == 0
    ms = C.c_float(-1.0)
    assert lib.ferrum_hip_event_elapsed_ms(e0, e1, C.byref(ms)) == 0 and 0.0 <= ms.value < 1000.0
    lib.ferrum_hip_event_destroy(e0); lib.ferrum_hip_event_destroy(e1)
    assert nmse(O.layer_norm(x, g, b, 1e-5), host(out)) < NMSE_FP16_TOL
    B.gelu(ctx, dev16(torch, x), out, tokens * dim)
    assert nmse(O.gelu(x), host(out)) < NMSE_FP16_TOL


@pytest.mark.parametrize("tokens,dim", [(1, 1024), (5, 2048), (32, 4096), (3, 5376), (2, 8192), (7, 128)])
def test_rms_norm_and_fused_add(env, tokens, dim):
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(dim + tokens)
    x = f16r(rng.standard_normal((tokens, dim)) * 2)
    r = f16r(rng.standard_normal((tokens, dim)) * 3)
    w = f16r(1 + 0.2 * rng.standard_normal(dim))
    out = torch.empty(tokens, dim, dtype=torch.float16, device="cuda")
    B.rms_norm(ctx, dev16(torch, x), dev16(torch, w), 1e-6, out, tokens, dim)
    assert nmse(O.rms_norm(x, w, 1e-6), host(out)) < NMSE_FP16_TOL
    rd = dev16(torch, r)
    B.fused_add_rms_norm(ctx, rd, dev16(torch, x), dev16(torch, w), 1e-6, out, tokens, dim)
    r_ref, o_ref = O.fused_add_rms_norm(r, x, w, 1e-6)
    assert nmse(r_ref, host(rd)) < NMSE_FP16_TOL          # residual stored as fp16
    # the fp16 lane norms the ROUNDED residual (fused_add_rms_norm.cu:88-101): compare both ways
    assert nmse(o_ref, host(out)) < 3e-6
    assert nmse(O.rms_norm(host(rd), w, 1e-6), host(out)) < NMSE_FP16_TOL


def test_rms_norm_empty_is_noop(env):
    pkg, B, ctx, O, torch = env
    out = torch.empty(0, 128, dtype=torch.float16, device="cuda")
    B.rms_norm(ctx, out, dev16(torch, np.ones(128)), 1e-6, out, 0, 128)


def test_embedding_silu_gelu_add_scale(env):
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(1)
    table = f16r(rng.standard_normal((300, 256)))
    ids = np.array([0, 299, 17, 17, 4], np.uint32)
    out = torch.empty(5, 256, dtype=torch.float16, device="cuda")
    B.embedding_lookup(ctx, dev16(torch, table), torch.from_numpy(ids.astype(np.int32)).cuda(), out, 256)
    assert np.array_equal(host(out), O.embedding_lookup(table, ids))        # a copy: exact
    gu = f16r(rng.standard_normal((6, 2 * 768)) * 3)
    act = torch.empty(6, 768, dtype=torch.float16, device="cuda")
    B.fused_silu_mul_split(ctx, dev16(torch, gu), act, 6, 768)
    assert nmse(O.fused_silu_mul_split(gu, 768), host(act)) < NMSE_FP16_TOL
    B.fused_gelu_tanh_mul_split(ctx, dev16(torch, gu), act, 6, 768)
    assert nmse(O.fused_gelu_tanh_mul_split(gu, 768), host(act)) < NMSE_FP16_TOL
    a, b = f16r(rng.standard_normal(1000)), f16r(rng.standard_normal(1000))
    ad = dev16(torch, a)
    B.add_inplace(ctx, ad, dev16(torch, b), 1000)
    assert np.array_equal(host(ad), f16r(O.add_inplace(a, b)))              # one rounding, exact after fp16
    sd = dev16(torch, np.array([1.0, -2.0, 0.5]))
    B.scale_inplace(ctx, sd, 33.9375, 3)                                    # llama_family.rs:6076-6086 KAT
    assert list(host(sd)) == [33.9375, -67.875, 16.96875]


# ── GPTQ INT4 linear ─────────────────────────────────────────────────────────
def _gptq_case(env, k, n, m, seed, symmetric, g_idx=False, x_fn=None):
    pkg, B, ctx, O, torch = env
    qw, sc, qz = O.make_synthetic_gptq(k, n, 128, seed, symmetric=symmetric)
    sc = f16r(sc)                                          # scales travel as fp16 on the device
    gi = O.make_desc_act_g_idx(k, 128) if g_idx else None
    lin = pkg.GptqLinear.from_raw(qw, sc, qz, gi, None, 4, 128, k, n)
    if x_fn is None:
        x = f16r(np.random.default_rng(seed).standard_normal((m, k)))
    else:
        x = f16r(x_fn(np.arange(m * k, dtype=np.float32)).reshape(m, k))
    out = torch.empty(m, n, dtype=torch.float16, device="cuda")
    lin.forward(ctx, dev16(torch, x), out, m)
    w = O.dequant_gptq(qw, sc, qz, 128, k, n, g_idx=gi)
    ref = O.gemm(x, w, m, n, k)
    return ref, host(out)


def test_gptq_reference_shapes(env):
    # gptq_parity_test.rs:108-145 (K=256,N=128,m=2, sin(0.001 i)) and :329-405 (K=512,N=256,m=2, symmetric,
    # cos(0.003 i) rounded to f16, rel err < 5 %): we hold the fp16 NMSE bucket instead
    ref, got = _gptq_case(env, 256, 128, 2, 0xDEADBEEF, False, x_fn=lambda i: np.sin(i * np.float32(0.001)))
    assert nmse(ref, got) < NMSE_FP16_TOL
    ref, got = _gptq_case(env, 512, 256, 2, 0xC0FFEE, True, x_fn=lambda i: np.cos(i * np.float32(0.003)))
    assert nmse(ref, got) < NMSE_FP16_TOL
    assert np.max(np.abs(ref - got)) / np.max(np.abs(ref)) < 2e-3


@pytest.mark.parametrize("k,n,m", [(2048, 5120, 1), (2048, 5120, 32), (4096, 2048, 4), (4096, 2048, 16),
                                   (1024, 1536, 33), (768, 2048, 64), (512, 264, 100), (256, 72, 7)])
def test_gptq_model_shapes(env, k, n, m):
    ref, got = _gptq_case(env, k, n, m, 0x1234 + k + n + m, True)
    assert nmse(ref, got) < NMSE_FP16_TOL


@pytest.mark.parametrize("k,n,m", [(512, 256, 3), (2048, 640, 17)])
def test_gptq_asymmetric_and_act_order(env, k, n, m):
    ref, got = _gptq_case(env, k, n, m, 0x51A7E5, False)                 # explicit zero points
    assert nmse(ref, got) < NMSE_FP16_TOL
    ref, got = _gptq_case(env, k, n, m, 0x5A170A7, False, g_idx=True)    # desc_act (gptq_parity_test.rs:271)
    assert nmse(ref, got) < NMSE_FP16_TOL


@pytest.mark.parametrize("k,n,m,form", [(8192, 2048, 32, "w4_ldsa"), (2048, 640, 200, "w4_tilep"), (1024, 4096, 2100, "w4_big"),
                                        (4096, 6144, 40, "w4_tilep")])
def test_gptq_act_order_takes_every_dense_kernel_form(env, k, n, m, form, forms):
    """desc_act weights (BASELINE configs[3]: Gemma-3 GPTQ): the packed rows are in sorted-g_idx order and the activations' columns
    are gathered with the same permutation before the GEMM, so the 17–32-row, 64-row-tile and tall-tile kernels serve them like
    any other weights (round 1 sent every act-order projection of ≥ 17 rows through the per-wave-activation skinny kernel)."""
    forms.reset()
    ref, got = _gptq_case(env, k, n, m, 0xAC70 + m, False, g_idx=True)
    forms.require(form)
    assert nmse(ref, got) < NMSE_FP16_TOL


@pytest.mark.parametrize("k,n,ms,sym", [
    # row-count boundaries of the three dense kernels (≤16 wgsplit, 17–32 LDS-A / wgsplit, ≥64 pipelined tile + split-K, 33–63 wgsplit)
    # on shapes that select each path: deep-K narrow-N (LDS-A with slabs), wide-N, tiny, N not a multiple of 64, asymmetric
    (8192, 2048, (16, 17, 32, 33), True), (1024, 16384, (17, 32, 64, 65), True), (256, 64, (1, 16, 31, 63, 64, 127, 128, 200), True),
    (1536, 1000, (5, 20, 64, 130), True), (2048, 640, (24, 64, 96), False), (14336, 512, (32, 64), True),
    # many row tiles through the pipelined tile kernel — ragged last tile, odd group count (K = 640: 5 groups), split-K
    # (narrow N), columns not a multiple of 256, asymmetric + bias
    (640, 320, (1024, 1100), True), (2048, 512, (1024,), True), (1024, 1000, (1153,), True), (768, 640, (1025,), False),
    # 33–63 rows of the larger projections (K·N ≥ 12 Mi) take the pipelined tile kernel with one ragged 64-row tile
    (4096, 4096, (33, 48, 63), True), (2048, 6144, (40,), False),
    # enough 128- / 256-row tiles to fill the chip: w4_gemm_big_kernel (ragged last tile; asymmetric)
    (2048, 5120, (1664, 3100), True), (1024, 4096, (2100,), False)])
def test_gptq_row_regimes_and_edge_shapes(env, k, n, ms, sym, forms):
    pkg, B, ctx, O, torch = env
    seen = set()
    qw, sc, qz = O.make_synthetic_gptq(k, n, 128, k * 7 + n, symmetric=sym)
    sc = f16r(sc / (0.28 * np.sqrt(k)))
    bias = f16r(np.random.default_rng(n).standard_normal(n)) if n == 640 else None
    lin = pkg.GptqLinear.from_raw(qw, sc, qz, None, bias, 4, 128, k, n)
    w = O.dequant_gptq(qw, sc, qz, 128, k, n)
    for m in ms:
        x = f16r(np.random.default_rng(m).standard_normal((m, k)))
        out = torch.full((m + 1, n), 7.0, dtype=torch.float16, device="cuda")     # guard row: nothing may write past m rows
        forms.reset()
        lin.forward(ctx, dev16(torch, x), out, m)
        ctx.sync()
        # the kernel the row count selects (w4_gemm_dense): ≤ 16 rows K-split skinny; ≥ 64 rows (33 on the larger projections)
        # the pipelined tile kernel; in between the LDS-shared-activation kernel on shapes deep or wide enough for it
        h = forms.hits()
        ran = [f for f in ("w4_wgsplit", "w4_ldsa", "w4_tilep", "w4_big") if h.get(f)]
        assert len(ran) == 1, (k, n, m, h)
        big = k * n >= (12 << 20)
        want = "w4_wgsplit" if m <= 16 else ("w4_tilep" if m >= (33 if big else 64) else None)
        if m >= 1024 and n >= 4096: want = "w4_big"
        assert want is None or ran[0] == want, (k, n, m, h)
        seen.add(ran[0])
        ref = O.gemm(x, w, m, n, k) + (bias[None, :] if bias is not None else 0.0)
        got = host(out)
        assert nmse(ref, got[:m]) < NMSE_FP16_TOL, (k, n, m)
        assert np.all(got[m] == 7.0), (k, n, m)
    if (k, n) in ((8192, 2048), (1024, 16384)):
        assert "w4_ldsa" in seen, seen                     # the 17–32-row cases of these shapes are the LDS-A kernel's


@pytest.mark.parametrize("mt", [6, 8, 16])
@pytest.mark.parametrize("sym", [True, False])
def test_gptq_big_tile_forms(env, mt, sym, knobs, forms):
    """w4_gemm_big_kernel forced on a small projection: 128- and 256-row tiles, ragged last tile, N = 1000 (a partial 256-column
    workgroup and a partial 64-column supertile), bias, symmetric and asymmetric zero points.  Its fp16 weights are
    (q − zero)·scale rounded once — the reference's own dequantisation (`cpu.rs:2283-2315` produces exactly that value in
    f32; Marlin in fp16) — so the oracle comparison holds at the fp16 tolerance."""
    pkg, B, ctx, O, torch = env
    k, n = 1024, 1000
    qw, sc, qz = O.make_synthetic_gptq(k, n, 128, 99 + mt, symmetric=sym)
    sc = f16r(sc / (0.28 * np.sqrt(k)))
    bias = f16r(np.random.default_rng(5).standard_normal(n))
    lin = pkg.GptqLinear.from_raw(qw, sc, qz, None, bias, 4, 128, k, n)
    w = O.dequant_gptq(qw, sc, qz, 128, k, n)
    knobs.set(W4_BIG=mt)
    for m in (16 * mt, 16 * mt + 37, 3 * 16 * mt - 1):
        x = f16r(np.random.default_rng(m).standard_normal((m, k)))
        out = torch.full((m + 1, n), 7.0, dtype=torch.float16, device="cuda")
        forms.reset()
        lin.forward(ctx, dev16(torch, x), out, m)
        ctx.sync()
        forms.require("w4_big", absent=("w4_tilep", "w4_ldsa", "w4_wgsplit"))
        ref = O.gemm(x, w, m, n, k) + bias[None, :]
        got = host(out)
        assert nmse(ref, got[:m]) < NMSE_FP16_TOL, (mt, sym, m)
        assert np.all(got[m] == 7.0), (mt, sym, m)


def test_gptq_linearity(env):
    # size-independent property at a BASELINE shape (Llama-8B o_proj 4096→4096): f(a·x+y) = a·f(x)+f(y)
    pkg, B, ctx, O, torch = env
    k, n, m = 4096, 4096, 8
    qw, sc, qz = O.make_synthetic_gptq(k, n, 128, 99, symmetric=True)
    lin = pkg.GptqLinear.from_raw(qw, f16r(sc), qz, None, None, 4, 128, k, n)
    rng = np.random.default_rng(5)
    x, y = f16r(rng.standard_normal((m, k))), f16r(rng.standard_normal((m, k)))
    z = f16r(2.0 * x + y)                                 # exactly representable inputs are not needed:
    outs = []
    for v in (x, y, z):
        o = torch.empty(m, n, dtype=torch.float16, device="cuda")
        lin.forward(ctx, dev16(torch, v), o, m)
        outs.append(host(o).astype(np.float64))
    lhs = outs[2]
    rhs = None
    # z was rounded to fp16, so compare against f applied to the exact combination in fp64
    w = O.dequant_gptq(qw, f16r(sc), qz, 128, k, n).astype(np.float64)
    rhs = z.astype(np.float64) @ w.T
    assert nmse(rhs, lhs) < NMSE_FP16_TOL
    assert nmse(x.astype(np.float64) @ w.T, outs[0]) < NMSE_FP16_TOL


# ── dense fp16 GEMM (router / lm_head) ───────────────────────────────────────
@pytest.mark.parametrize("m,n,k,f32out", [(1, 128, 2048, True), (32, 128, 2048, True), (5, 1511, 1024, True),
                                          (33, 96, 256, False), (64, 2048, 512, False),
                                          (20, 32768 + 128, 256, True), (32, 32768 + 64, 128, False)])   # the wide-N form of 17–32 rows (lm_head): 64 columns per wave
def test_dense_gemm(env, m, n, k, f32out):
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(m * n + k)
    a, b = f16r(rng.standard_normal((m, k))), f16r(rng.standard_normal((n, k)) * 0.1)
    out = torch.empty(m, n, dtype=torch.float32 if f32out else torch.float16, device="cuda")
    B.gemm(ctx, dev16(torch, a), dev16(torch, b), out, m, n, k)
    ref = O.gemm(a, b, m, n, k)
    assert nmse(ref, host(out)) < (1e-10 if f32out else NMSE_FP16_TOL)
    # same product through the load-time fragment-major layout (lm_head / router path)
    bt = B.dense_repack_f16t(ctx, dev16(torch, b), n, k)
    out2 = torch.zeros_like(out)
    B.gemm_f16t(ctx, dev16(torch, a), bt, out2, m, n, k)
    ctx.sync()
    assert nmse(ref, host(out2)) < (1e-10 if f32out else NMSE_FP16_TOL)


# ── paged KV write / read ────────────────────────────────────────────────────
def _rope(O, hd, max_seq, theta=1e6):
    return O.build_rope_cache(theta, hd, max_seq)


@pytest.mark.parametrize("qk_mode,hd", [(1, 128), (2, 128), (3, 128), (0, 128), (1, 64), (2, 256)])
def test_split_qkv_norm_rope_into_paged_cache_varlen(env, qk_mode, hd):
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(qk_mode * 10 + hd)
    nq, nkv, bs = 8, 2, 16
    q_lens, pos_offs = [5, 1, 19], [3, 40, 0]               # mixed prefill chunks + a decode row
    num_seqs, m_total = len(q_lens), sum(q_lens)
    max_blocks, num_blocks = 8, 32
    cos, sin = _rope(O, hd, 128)
    qkv = f16r(rng.standard_normal((m_total, (nq + 2 * nkv) * hd)))
    qn, kn = f16r(1 + 0.1 * rng.standard_normal(hd)), f16r(1 + 0.1 * rng.standard_normal(hd))
    perm = rng.permutation(num_blocks)
    tables = np.zeros((num_seqs, max_blocks), np.int32)
    used = 0
    for s in range(num_seqs):
        nb = (pos_offs[s] + q_lens[s] + bs - 1) // bs
        tables[s, :nb] = perm[used:used + nb]
        used += nb
    cu = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32)
    ck, cv = B.alloc_paged_pool(num_blocks, nkv, hd), B.alloc_paged_pool(num_blocks, nkv, hd)
    q_out = torch.empty(m_total, nq, hd, dtype=torch.float16, device="cuda")
    B.split_qkv_norm_rope_into_paged_cache_varlen(
        ctx, dev16(torch, qkv), dev16(torch, qn), dev16(torch, kn), torch.from_numpy(cos).cuda(),
        torch.from_numpy(sin).cuda(), q_out, ck, cv, torch.from_numpy(cu).cuda(),
        torch.from_numpy(np.array(pos_offs, np.int32)).cuda(), torch.from_numpy(tables).cuda(), num_seqs, m_total, nq,
        nkv, hd, 1e-6, qk_mode, bs, max_blocks)
    ctx.sync()
    for s in range(num_seqs):
        rows = qkv[cu[s]:cu[s + 1]]
        q, k, v = O.split_qkv(rows, nq * hd, nkv * hd)
        T = q_lens[s]
        q_ref = O.qk_norm_rope(q.reshape(T, nq, hd), qn, cos, sin, T, nq, hd, pos_offs[s], 1e-6, qk_mode).transpose(1, 0, 2)
        k_ref = O.qk_norm_rope(k.reshape(T, nkv, hd), kn, cos, sin, T, nkv, hd, pos_offs[s], 1e-6, qk_mode).transpose(1, 0, 2)
        v_ref = v.reshape(T, nkv, hd)
        assert nmse(q_ref, host(q_out[cu[s]:cu[s + 1]])) < NMSE_FP16_TOL
        kv_len = pos_offs[s] + T
        kk, vv = B.paged_kv_read(ctx, ck, cv, torch.from_numpy(tables[s]).cuda(), kv_len, nkv, hd)
        ctx.sync()
        kk, vv = host(kk), host(vv)
        assert nmse(k_ref, kk[pos_offs[s]:]) < NMSE_FP16_TOL
        assert np.array_equal(vv[pos_offs[s]:], v_ref)                     # V is a copy: exact
        assert not kk[:pos_offs[s]].any() and not vv[:pos_offs[s]].any()   # earlier slots untouched
    # bit-exact KV-block indexing: only the blocks named by the tables were written
    written = set(int(b) for s in range(num_seqs) for b in
                  tables[s, pos_offs[s] // bs:(pos_offs[s] + q_lens[s] + bs - 1) // bs])
    pool = host(ck).reshape(num_blocks, -1)
    for blk in range(num_blocks):
        assert bool(pool[blk].any()) == (blk in written)


def test_ragged_batch_of_many_sequences_including_empty_ones(env):
    """150 sequences (more than two 64-wide passes of the in-kernel sequence lookups), a few of them with no query token at
    all: the split/norm/RoPE/paged-write op and the ragged attention grid must place every token with its own sequence."""
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(2025)
    nq, nkv, hd, bs, S = 4, 2, 64, 16, 150
    q_lens = [int(x) for x in rng.integers(1, 7, size=S)]
    for s in (0, 63, 64, 65, 128, 149):
        q_lens[s] = 0                                           # empty sequences at chunk boundaries and both ends
    q_lens[10], q_lens[100] = 40, 23                            # a few longer chunks
    pos_offs = [int(x) for x in rng.integers(0, 20, size=S)]
    kv_lens = [p + t for p, t in zip(pos_offs, q_lens)]
    max_blocks = (max(kv_lens) + bs - 1) // bs
    num_blocks = sum((n + bs - 1) // bs for n in kv_lens) + 1
    perm = rng.permutation(num_blocks)
    tables = np.zeros((S, max_blocks), np.int32)
    used = 0
    for s, n in enumerate(kv_lens):
        nb = (n + bs - 1) // bs
        tables[s, :nb] = perm[used:used + nb]
        used += nb
    m_total = sum(q_lens)
    cu = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32)
    cos, sin = _rope(O, hd, 128)
    qkv = f16r(rng.standard_normal((m_total, (nq + 2 * nkv) * hd)))
    qn, kn = f16r(1 + 0.1 * rng.standard_normal(hd)), f16r(1 + 0.1 * rng.standard_normal(hd))
    # context already in the cache: fill it through the same op, one "prefill" of pos_offs[s] tokens per sequence
    ctx_lens = pos_offs
    ctx_total = sum(ctx_lens)
    ccu = np.concatenate([[0], np.cumsum(ctx_lens)]).astype(np.int32)
    ctx_qkv = f16r(rng.standard_normal((ctx_total, (nq + 2 * nkv) * hd)))
    ck, cv = B.alloc_paged_pool(num_blocks, nkv, hd), B.alloc_paged_pool(num_blocks, nkv, hd)
    cosd, sind, td = torch.from_numpy(cos).cuda(), torch.from_numpy(sin).cuda(), torch.from_numpy(tables).cuda()
    scratch = torch.empty(max(ctx_total, 1), nq, hd, dtype=torch.float16, device="cuda")
    B.split_qkv_norm_rope_into_paged_cache_varlen(ctx, dev16(torch, ctx_qkv), dev16(torch, qn), dev16(torch, kn), cosd, sind, scratch,
                                                  ck, cv, torch.from_numpy(ccu).cuda(), torch.zeros(S, dtype=torch.int32, device="cuda"),
                                                  td, S, ctx_total, nq, nkv, hd, 1e-6, 1, bs, max_blocks)
    q_out = torch.empty(m_total, nq, hd, dtype=torch.float16, device="cuda")
    B.split_qkv_norm_rope_into_paged_cache_varlen(ctx, dev16(torch, qkv), dev16(torch, qn), dev16(torch, kn), cosd, sind, q_out, ck, cv,
                                                  torch.from_numpy(cu).cuda(), torch.from_numpy(np.array(pos_offs, np.int32)).cuda(),
                                                  td, S, m_total, nq, nkv, hd, 1e-6, 1, bs, max_blocks)
    out = torch.full((m_total + 1, nq, hd), 5.0, dtype=torch.float16, device="cuda")
    B.paged_varlen_attention(ctx, q_out, ck, cv, out, torch.from_numpy(cu).cuda(), torch.from_numpy(np.array(pos_offs, np.int32)).cuda(),
                             td, S, m_total, max(kv_lens), nq, nkv, hd, 0, bs, max_blocks, max(q_lens))
    ctx.sync()
    got_q, got = host(q_out), host(out)
    assert np.all(got[m_total] == 5.0)
    for s in range(S):
        T = q_lens[s]
        if T == 0:
            continue
        q, k, v = O.split_qkv(qkv[cu[s]:cu[s + 1]], nq * hd, nkv * hd)
        q_ref = O.qk_norm_rope(q.reshape(T, nq, hd), qn, cos, sin, T, nq, hd, pos_offs[s], 1e-6, 1).transpose(1, 0, 2)
        assert nmse(q_ref, got_q[cu[s]:cu[s + 1]]) < NMSE_FP16_TOL, s
        kk, vv = B.paged_kv_read(ctx, ck, cv, td[s], kv_lens[s], nkv, hd)
        ctx.sync()
        ref = _ref_attention(O, got_q[cu[s]:cu[s + 1]], host(kk), host(vv), pos_offs[s], nq, nkv, hd, 0)
        assert nmse(ref, got[cu[s]:cu[s + 1]]) < 1e-5, s


# ── contiguous-KV lane of the core trait (kv_layer.rs:370-513) ────────────────
@pytest.mark.parametrize("nq,nkv,hd,mode,window", [(8, 2, 128, 1, 0), (4, 4, 64, 2, 0), (6, 2, 128, 3, 5), (2, 1, 256, 1, 3)])
def test_contiguous_lane_prefill_then_decode(env, nq, nkv, hd, mode, window):
    """split_qkv → qk_norm_rope (→ head-major) → kv_cache_append_head_major → flash_attention → transpose_head_to_token,
    op by op against the CPU restatement (cpu.rs:1645-1783,1993-2060,2179-2259), for a 9-token prefill followed by a decode
    token at position 9; plus copy_slice / scaled_add_inplace / transpose_token_to_head."""
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(nq * 7 + hd + mode)
    cap = 32
    cos, sin = _rope(O, hd, cap)
    cosd, sind = torch.from_numpy(cos).cuda(), torch.from_numpy(sin).cuda()
    qn, kn = f16r(1 + 0.1 * rng.standard_normal(hd)), f16r(1 + 0.1 * rng.standard_normal(hd))
    q_dim, kv_dim = nq * hd, nkv * hd
    ck = torch.zeros(nkv, cap, hd, dtype=torch.float16, device="cuda")
    cv = torch.zeros_like(ck)
    ck_ref, cv_ref = np.zeros((nkv, cap, hd), np.float32), np.zeros((nkv, cap, hd), np.float32)
    cache_len = 0
    for T in (9, 1):
        qkv = f16r(rng.standard_normal((T, q_dim + 2 * kv_dim)))
        qd, kd, vd = (torch.empty(T, n, dtype=torch.float16, device="cuda") for n in (q_dim, kv_dim, kv_dim))
        B.split_qkv(ctx, dev16(torch, qkv), qd, kd, vd, T, q_dim, kv_dim)
        ctx.sync()
        q, k, v = O.split_qkv(qkv, q_dim, kv_dim)
        assert np.array_equal(host(qd), q) and np.array_equal(host(kd), k) and np.array_equal(host(vd), v)
        qh = torch.empty(nq, T, hd, dtype=torch.float16, device="cuda")
        kh = torch.empty(nkv, T, hd, dtype=torch.float16, device="cuda")
        vh = torch.empty(nkv, T, hd, dtype=torch.float16, device="cuda")
        B.qk_norm_rope(ctx, qd, dev16(torch, qn), cosd, sind, qh, T, nq, hd, cache_len, 1e-6, mode)
        B.qk_norm_rope(ctx, kd, dev16(torch, kn), cosd, sind, kh, T, nkv, hd, cache_len, 1e-6, mode)
        B.qk_norm_rope(ctx, vd, dev16(torch, kn), cosd, sind, vh, T, nkv, hd, cache_len, 1e-6, 0)
        ctx.sync()
        q_ref = O.qk_norm_rope(q.reshape(T, nq, hd), qn, cos, sin, T, nq, hd, cache_len, 1e-6, mode)
        k_ref = O.qk_norm_rope(k.reshape(T, nkv, hd), kn, cos, sin, T, nkv, hd, cache_len, 1e-6, mode)
        v_ref = O.qk_norm_rope(v.reshape(T, nkv, hd), kn, cos, sin, T, nkv, hd, cache_len, 1e-6, 0)
        assert nmse(q_ref, host(qh)) < NMSE_FP16_TOL and nmse(k_ref, host(kh)) < NMSE_FP16_TOL
        assert np.array_equal(host(vh), v_ref)                                   # mode 0 = transpose only
        B.kv_cache_append_head_major(ctx, ck, cv, cache_len, cap, kh, vh, T, nkv, hd)
        ck_ref[:, cache_len:cache_len + T] = host(kh)
        cv_ref[:, cache_len:cache_len + T] = host(vh)
        kv_len = cache_len + T
        out = torch.full((nq, T, hd), 3.0, dtype=torch.float16, device="cuda")
        B.flash_attention(ctx, qh, ck, cv, out, 1, T, kv_len, cache_len, nq, nkv, hd, causal=True, kv_seq_stride=cap,
                          sliding_window=window)
        ctx.sync()
        assert np.array_equal(host(ck), ck_ref) and np.array_equal(host(cv), cv_ref)
        a_ref = O.cpu_attention(host(qh), ck_ref, cv_ref, T, kv_len, True, cache_len, nq, nkv, hd, sliding_window=window,
                                kv_seq_stride=cap)
        assert nmse(a_ref, host(out)) < 1e-5
        tm_ = torch.empty(T, nq, hd, dtype=torch.float16, device="cuda")
        B.transpose_head_to_token(ctx, out, tm_, T, nq, hd)
        back = torch.empty_like(out)
        B.transpose_token_to_head(ctx, tm_, back, T, nq, hd)
        ctx.sync()
        assert np.array_equal(host(tm_), host(out).transpose(1, 0, 2)) and torch.equal(back, out)
        cache_len = kv_len
    a = dev16(torch, rng.standard_normal(1000))
    b = dev16(torch, rng.standard_normal(1000))
    ref = host(a).copy()
    ref[100:400] = f16r(ref[100:400] + np.float32(0.37) * host(b)[5:305])
    B.scaled_add_inplace(ctx, a[100:], b[5:], 0.37, 300)
    c = torch.zeros(64, dtype=torch.float16, device="cuda")
    B.copy_slice(ctx, b, 17, c, 3, 40)
    ctx.sync()
    assert np.array_equal(host(a), ref)
    exp = np.zeros(64, np.float32)
    exp[3:43] = host(b)[17:57]
    assert np.array_equal(host(c), exp)


# ── paged attention ──────────────────────────────────────────────────────────
def _fill_pool(env, K, V, tables, kv_lens, nkv, hd, num_blocks):
    """Write per-sequence K/V [len,nkv,hd] into native pools through the product's own writer (mode 0)."""
    pkg, B, ctx, O, torch = env
    ck, cv = B.alloc_paged_pool(num_blocks, nkv, hd), B.alloc_paged_pool(num_blocks, nkv, hd)
    nq = nkv
    for s, n in enumerate(kv_lens):
        qkv = np.concatenate([np.zeros((n, nq * hd), np.float32), K[s].reshape(n, -1), V[s].reshape(n, -1)], axis=1)
        q_out = torch.empty(n, nq, hd, dtype=torch.float16, device="cuda")
        dummy = dev16(torch, np.ones(hd))
        cs = torch.zeros(max(kv_lens) + 1, hd // 2, device="cuda")
        B.split_qkv_norm_rope_into_paged_cache_varlen(
            ctx, dev16(torch, qkv), dummy, dummy, cs, cs, q_out, ck, cv,
            torch.tensor([0, n], dtype=torch.int32, device="cuda"), torch.tensor([0], dtype=torch.int32, device="cuda"),
            torch.from_numpy(tables[s:s + 1].copy()).cuda(), 1, n, nq, nkv, hd, 1e-6, 0, 16, tables.shape[1])
    ctx.sync()
    return ck, cv


def _paged_batch(env, rng, kv_lens, nq, nkv, hd, q_lens=None, spare_blocks=1, spare_columns=0):
    """The paged batch the attention tests run on: block tables over a permuted pool (`spare_blocks` more blocks than the sequences
    hold, `spare_columns` more table columns than the longest needs), per-sequence K / V [len, nkv, hd] written through _fill_pool,
    and for `q_lens` the cu_seqlens and q [Σ q_lens, nq, hd].  Draws from `rng` in this order: the permutation, K then V of each
    sequence, q."""
    S = len(kv_lens)
    b = types.SimpleNamespace(max_blocks=(max(kv_lens) + 15) // 16 + spare_columns,
                              num_blocks=sum((n + 15) // 16 for n in kv_lens) + spare_blocks, K=[], V=[])
    perm = rng.permutation(b.num_blocks)
    b.tables = np.zeros((S, b.max_blocks), np.int32)
    used = 0
    for s, n in enumerate(kv_lens):
        nb = (n + 15) // 16
        b.tables[s, :nb] = perm[used:used + nb]
        used += nb
        b.K.append(f16r(rng.standard_normal((n, nkv, hd))))
        b.V.append(f16r(rng.standard_normal((n, nkv, hd))))
    b.ck, b.cv = _fill_pool(env, b.K, b.V, b.tables, kv_lens, nkv, hd, b.num_blocks)
    if q_lens is not None:
        b.m_total = sum(q_lens)
        b.cu = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32)
        b.q = f16r(rng.standard_normal((b.m_total, nq, hd)))
    return b


def _ref_attention(O, q, K, V, pos_offset, nq, nkv, hd, window=0):
    """q [T,nq,hd] at positions pos_offset.. over K/V [len,nkv,hd] → [T,nq,hd] (cpu.rs:2179-2259)."""
    T, kv_len = q.shape[0], K.shape[0]
    out = O.cpu_attention(q.transpose(1, 0, 2), K.transpose(1, 0, 2), V.transpose(1, 0, 2), T, kv_len, True, pos_offset,
                          nq, nkv, hd, sliding_window=window)
    return out.transpose(1, 0, 2)


def test_paged_decode_uniform_scores_golden(env):
    # ferrum-kv/src/attention.rs:162-195: equal scores → output = mean(V) = 2.0
    pkg, B, ctx, O, torch = env
    nq = nkv = 2
    hd = 64
    K = [np.ones((3, nkv, hd), np.float32)]
    V = [np.stack([np.full((nkv, hd), p + 1, np.float32) for p in range(3)])]
    tables = np.array([[5, 0]], np.int32)
    ck, cv = _fill_pool(env, K, V, tables, [3], nkv, hd, 8)
    out = torch.empty(1, nq, hd, dtype=torch.float16, device="cuda")
    B.paged_batched_decode_attention(ctx, dev16(torch, np.ones((1, nq, hd))), ck, cv, out, torch.from_numpy(tables).cuda(),
                                     torch.tensor([3], dtype=torch.int32, device="cuda"), 1, 3, nq, nkv, hd, 16, 2)
    ctx.sync()
    assert np.all(np.abs(host(out) - 2.0) < 1e-3)


@pytest.mark.parametrize("nq,nkv,hd,kv_lens", [(32, 4, 128, [1, 16, 17, 257, 300, 384, 33, 250]),
                                               (32, 8, 128, [100, 5]), (8, 8, 128, [48]), (16, 1, 128, [700, 31]),
                                               (4, 2, 64, [77]), (8, 2, 256, [40, 130])])
def test_paged_batched_decode_attention(env, nq, nkv, hd, kv_lens):
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(nq + nkv + hd + len(kv_lens))
    S = len(kv_lens)
    b = _paged_batch(env, rng, kv_lens, nq, nkv, hd, q_lens=[1] * S, spare_blocks=3, spare_columns=1)
    tables, K, V, ck, cv, max_blocks = b.tables, b.K, b.V, b.ck, b.cv, b.max_blocks
    q = b.q
    out = torch.empty(S, nq, hd, dtype=torch.float16, device="cuda")
    B.paged_batched_decode_attention(ctx, dev16(torch, q), ck, cv, out, torch.from_numpy(tables).cuda(),
                                     torch.from_numpy(np.array(kv_lens, np.int32)).cuda(), S, max(kv_lens), nq, nkv, hd,
                                     16, max_blocks)
    ctx.sync()
    got = host(out)
    for s, n in enumerate(kv_lens):
        ref = _ref_attention(O, q[s:s + 1], K[s], V[s], n - 1, nq, nkv, hd)
        assert nmse(ref, got[s:s + 1]) < 1e-5, (s, n)          # far inside the 5e-3 attention bucket
        # cross-check with the second reference formulation (ferrum-kv attention.rs three-pass softmax)
    assert NMSE_ATTN_TOL > 1e-5


@pytest.mark.parametrize("window,nq,nkv,hd", [(0, 8, 2, 128), (24, 8, 2, 128), (0, 14, 2, 128), (40, 28, 4, 128), (0, 4, 4, 64),
                                              (17, 6, 6, 64), (0, 4, 1, 256), (33, 32, 16, 128), (1, 8, 2, 128)])
def test_paged_varlen_attention_mixed_batch(env, window, nq, nkv, hd, knobs, forms):
    pkg, B, ctx, O, torch = env
    # half of the cases ask for the row-split (prefill) form; it applies from 4 row tiles per sequence (37 tokens × GQA group / 16)
    want_rs = (window + nq) % 2 == 0 and -(-37 * (nq // nkv) // 16) >= 4
    if (window + nq) % 2 == 0:
        knobs.set(ATTN_RS_MIN_WGS=1)
    rng = np.random.default_rng(11 + window + nq + hd)
    q_lens, pos_offs = [37, 1, 16, 3], [0, 90, 20, 250]       # fresh prefill, decode, chunk, late chunk
    S = len(q_lens)
    kv_lens = [p + t for p, t in zip(pos_offs, q_lens)]
    b = _paged_batch(env, rng, kv_lens, nq, nkv, hd, q_lens=q_lens)
    tables, K, V, ck, cv, max_blocks = b.tables, b.K, b.V, b.ck, b.cv, b.max_blocks
    m_total, cu, q = b.m_total, b.cu, b.q
    out = torch.zeros(m_total, nq, hd, dtype=torch.float16, device="cuda")
    B.paged_varlen_attention(ctx, dev16(torch, q), ck, cv, out, torch.from_numpy(cu).cuda(),
                             torch.from_numpy(np.array(pos_offs, np.int32)).cuda(), torch.from_numpy(tables).cuda(), S,
                             m_total, max(kv_lens), nq, nkv, hd, window, 16, max_blocks, max(q_lens))
    ctx.sync()
    forms.require("attn_row_split" if want_rs else "attn_kv_narrow", absent=("attn_flash",))
    got = host(out)
    for s in range(S):
        ref = _ref_attention(O, q[cu[s]:cu[s + 1]], K[s], V[s], pos_offs[s], nq, nkv, hd, window)
        assert nmse(ref, got[cu[s]:cu[s + 1]]) < 1e-5, s
    if window == 0:
        # the paged reference (attention.rs:30-114) agrees for the fresh-prefill sequence
        pk = np.zeros((b.num_blocks, 16, nkv, hd), np.float32)
        pv = np.zeros_like(pk)
        for p in range(kv_lens[0]):
            pk[tables[0, p // 16], p % 16] = K[0][p]
            pv[tables[0, p // 16], p % 16] = V[0][p]
        ref2 = O.paged_attention(q[:q_lens[0]], q_lens[0], nq, nkv, hd, pk, pv, tables[0], 16, kv_lens[0])
        assert nmse(ref2, got[:q_lens[0]]) < 1e-5


@pytest.mark.parametrize("window", [0, 50])
def test_paged_varlen_attention_many_prefill_tiles_row_split(env, window, knobs, forms):
    """24 prompts × 200 tokens (GQA group 2 ⇒ 25 row tiles each): enough workgroups for the row-split prefill form on its own
    heuristic; every sequence against the CPU restatement."""
    pkg, B, ctx, O, torch = env
    knobs.set(ATTN_NO_FLASH=1, ATTN_NO_RESIDENT=1)                 # the flash and resident-K/V forms have their own tests below
    rng = np.random.default_rng(77 + window)
    nq, nkv, hd, S, T = 8, 4, 128, 24, 200
    q_lens, pos_offs = [T] * S, [0] * (S - 2) + [48, 5]            # two of them continue an existing context
    kv_lens = [p + t for p, t in zip(pos_offs, q_lens)]
    b = _paged_batch(env, rng, kv_lens, nq, nkv, hd, q_lens=q_lens)
    tables, K, V, ck, cv, max_blocks = b.tables, b.K, b.V, b.ck, b.cv, b.max_blocks
    m_total, cu, q = b.m_total, b.cu, b.q
    out = torch.zeros(m_total, nq, hd, dtype=torch.float16, device="cuda")
    B.paged_varlen_attention(ctx, dev16(torch, q), ck, cv, out, torch.from_numpy(cu).cuda(),
                             torch.from_numpy(np.array(pos_offs, np.int32)).cuda(), torch.from_numpy(tables).cuda(), S,
                             m_total, max(kv_lens), nq, nkv, hd, window, 16, max_blocks, max(q_lens))
    ctx.sync()
    forms.require("attn_row_split", absent=("attn_flash", "attn_kv_narrow"))
    got = host(out)
    for s in range(S):
        ref = _ref_attention(O, q[cu[s]:cu[s + 1]], K[s], V[s], pos_offs[s], nq, nkv, hd, window)
        assert nmse(ref, got[cu[s]:cu[s + 1]]) < 1e-5, s


@pytest.mark.parametrize("window,nq,nkv,hd", [(0, 8, 2, 128), (24, 8, 2, 128), (0, 14, 2, 128), (40, 32, 4, 128), (0, 4, 4, 64),
                                              (17, 6, 6, 64), (0, 4, 1, 256), (33, 32, 16, 128), (1, 8, 2, 128)])
def test_paged_prefill_attention_lds_shared_kv(env, window, nq, nkv, hd, knobs, forms):
    """The flash form (K/V of a block pair staged once per workgroup in LDS, 8 row tiles per workgroup): ragged prefill batch —
    fresh prompts, chunks that continue a context, a sequence shorter than one workgroup unit, odd block counts."""
    pkg, B, ctx, O, torch = env
    knobs.set(ATTN_FLASH_MIN_ROWS=1)
    rng = np.random.default_rng(5 + window + nq + hd)
    q_lens, pos_offs = [70, 33, 64, 17, 49], [0, 90, 20, 5, 300]
    S = len(q_lens)
    kv_lens = [p + t for p, t in zip(pos_offs, q_lens)]
    b = _paged_batch(env, rng, kv_lens, nq, nkv, hd, q_lens=q_lens)
    tables, K, V, ck, cv, max_blocks = b.tables, b.K, b.V, b.ck, b.cv, b.max_blocks
    m_total, cu, q = b.m_total, b.cu, b.q
    out = torch.full((m_total + 1, nq, hd), 9.0, dtype=torch.float16, device="cuda")      # guard row
    B.paged_varlen_attention(ctx, dev16(torch, q), ck, cv, out, torch.from_numpy(cu).cuda(),
                             torch.from_numpy(np.array(pos_offs, np.int32)).cuda(), torch.from_numpy(tables).cuda(), S,
                             m_total, max(kv_lens), nq, nkv, hd, window, 16, max_blocks, max(q_lens))
    ctx.sync()
    forms.require("attn_flash", absent=("attn_row_split", "attn_kv_narrow"))
    got = host(out)
    assert np.all(got[m_total] == 9.0)
    for s in range(S):
        ref = _ref_attention(O, q[cu[s]:cu[s + 1]], K[s], V[s], pos_offs[s], nq, nkv, hd, window)
        assert nmse(ref, got[cu[s]:cu[s + 1]]) < 1e-5, s


@pytest.mark.parametrize("window,nq,nkv", [(0, 8, 2), (24, 8, 2), (0, 14, 2), (40, 32, 4), (0, 32, 16), (1, 8, 8)])
def test_paged_prefill_attention_resident_kv(env, window, nq, nkv, knobs, forms):
    """Short prompts whose whole context fits one LDS image (kv ≤ 256, head_dim 128): the resident-K/V form — fresh prompts, chunks
    that continue a context, odd block counts and block counts that are not a multiple of the four-block step, a sequence with
    fewer row tiles than waves, the full 256-key case, GQA groups 1 … 8 (7: rows of a token straddle tiles)."""
    pkg, B, ctx, O, torch = env
    knobs.set(ATTN_RESIDENT_MIN_WGS=1)
    hd = 128
    rng = np.random.default_rng(11 + window + nq)
    q_lens, pos_offs = [200, 33, 64, 256, 49, 100], [0, 90, 20, 0, 200, 70]
    S = len(q_lens)
    kv_lens = [p + t for p, t in zip(pos_offs, q_lens)]
    assert max(kv_lens) <= 256
    b = _paged_batch(env, rng, kv_lens, nq, nkv, hd, q_lens=q_lens)
    tables, K, V, ck, cv, max_blocks = b.tables, b.K, b.V, b.ck, b.cv, b.max_blocks
    m_total, cu, q = b.m_total, b.cu, b.q
    out = torch.full((m_total + 1, nq, hd), 9.0, dtype=torch.float16, device="cuda")      # guard row
    B.paged_varlen_attention(ctx, dev16(torch, q), ck, cv, out, torch.from_numpy(cu).cuda(),
                             torch.from_numpy(np.array(pos_offs, np.int32)).cuda(), torch.from_numpy(tables).cuda(), S,
                             m_total, max(kv_lens), nq, nkv, hd, window, 16, max_blocks, max(q_lens))
    ctx.sync()
    forms.require("attn_resident", absent=("attn_flash", "attn_row_split", "attn_kv_narrow"))
    got = host(out)
    assert np.all(got[m_total] == 9.0)
    for s_ in range(S):
        ref = _ref_attention(O, q[cu[s_]:cu[s_ + 1]], K[s_], V[s_], pos_offs[s_], nq, nkv, hd, window)
        assert nmse(ref, got[cu[s_]:cu[s_ + 1]]) < 1e-5, s_


def test_paged_prefill_attention_lds_shared_kv_many_sequences(env, knobs, forms):
    """The flash form over 70 sequences (two passes of its in-kernel sequence lookup), two of them empty."""
    pkg, B, ctx, O, torch = env
    knobs.set(ATTN_FLASH_MIN_ROWS=1)
    rng = np.random.default_rng(404)
    nq, nkv, hd, S = 4, 2, 128, 70
    q_lens = [int(x) for x in rng.integers(15, 26, size=S)]
    q_lens[0], q_lens[64] = 0, 0
    pos_offs = [int(x) for x in rng.integers(0, 40, size=S)]
    kv_lens = [p + t for p, t in zip(pos_offs, q_lens)]
    b = _paged_batch(env, rng, kv_lens, nq, nkv, hd, q_lens=q_lens)
    tables, K, V, ck, cv, max_blocks = b.tables, b.K, b.V, b.ck, b.cv, b.max_blocks
    m_total, cu, q = b.m_total, b.cu, b.q
    out = torch.zeros(m_total, nq, hd, dtype=torch.float16, device="cuda")
    B.paged_varlen_attention(ctx, dev16(torch, q), ck, cv, out, torch.from_numpy(cu).cuda(),
                             torch.from_numpy(np.array(pos_offs, np.int32)).cuda(), torch.from_numpy(tables).cuda(), S,
                             m_total, max(kv_lens), nq, nkv, hd, 0, 16, max_blocks, max(q_lens))
    ctx.sync()
    forms.require("attn_flash", absent=("attn_row_split", "attn_kv_narrow"))
    got = host(out)
    for s in range(S):
        if q_lens[s] == 0:
            continue
        ref = _ref_attention(O, q[cu[s]:cu[s + 1]], K[s], V[s], pos_offs[s], nq, nkv, hd, 0)
        assert nmse(ref, got[cu[s]:cu[s + 1]]) < 1e-5, s


@pytest.mark.parametrize("no_rs", [False, True])
def test_paged_varlen_attention_compact_grid_many_sequences(env, no_rs, knobs, forms):
    """The compact grid of the row-split and the KV-split form over 70 sequences (two passes of the in-kernel sequence lookup):
    69 decode-like sequences of 1 … 3 tokens, one of them empty, and at index 66 — found in the second pass — a 200-token prompt.
    328 tokens × GQA group 2: 25 row tiles for the longest sequence and 70·7·2 = 980 work-groups, so row-split on its own heuristic,
    ⌈111 / 4⌉ + 70 = 98 units against a grid of 490; KV-split (ATTN_NO_RS) with 111 units against 1750 tiles."""
    pkg, B, ctx, O, torch = env
    if no_rs:
        knobs.set(ATTN_NO_RS=1)
    rng = np.random.default_rng(7066)
    nq, nkv, hd, S = 4, 2, 128, 70
    q_lens = [int(x) for x in rng.integers(1, 4, size=S)]
    q_lens[9], q_lens[66] = 0, 200
    pos_offs = [int(x) for x in rng.integers(0, 41, size=S)]
    pos_offs[9] = 5
    kv_lens = [p + t for p, t in zip(pos_offs, q_lens)]
    b = _paged_batch(env, rng, kv_lens, nq, nkv, hd, q_lens=q_lens)
    out = torch.full((b.m_total + 1, nq, hd), 9.0, dtype=torch.float16, device="cuda")      # guard row
    B.paged_varlen_attention(ctx, dev16(torch, b.q), b.ck, b.cv, out, torch.from_numpy(b.cu).cuda(),
                             torch.from_numpy(np.array(pos_offs, np.int32)).cuda(), torch.from_numpy(b.tables).cuda(), S,
                             b.m_total, max(kv_lens), nq, nkv, hd, 0, 16, b.max_blocks, max(q_lens))
    ctx.sync()
    if no_rs:
        forms.require("attn_kv_narrow", absent=("attn_row_split", "attn_flash", "attn_resident", "attn_split_reduce"))
    else:
        forms.require("attn_row_split", absent=("attn_kv_narrow", "attn_flash", "attn_resident", "attn_split_reduce"))
    got = host(out)
    assert np.all(got[b.m_total] == 9.0)
    for s in range(S):
        if q_lens[s] == 0:
            continue
        ref = _ref_attention(O, b.q[b.cu[s]:b.cu[s + 1]], b.K[s], b.V[s], pos_offs[s], nq, nkv, hd, 0)
        assert nmse(ref, got[b.cu[s]:b.cu[s + 1]]) < 1e-5, s


def test_paged_decode_long_context_split_kv(env, forms):
    # exercises the grid.z flash-decode split + reduce at a BASELINE-like head config (Qwen3-30B: 32/4 heads)
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(3)
    nq, nkv, hd, kv_lens = 32, 4, 128, [4096, 1500]
    S = 2
    b = _paged_batch(env, rng, kv_lens, nq, nkv, hd, q_lens=[1] * S, spare_blocks=0)
    tables, K, V, ck, cv, max_blocks = b.tables, b.K, b.V, b.ck, b.cv, b.max_blocks
    q = b.q
    q[0, 3] *= 6.0                                          # a peaked row: forces large online-softmax rescales
    out = torch.empty(S, nq, hd, dtype=torch.float16, device="cuda")
    B.paged_batched_decode_attention(ctx, dev16(torch, q), ck, cv, out, torch.from_numpy(tables).cuda(),
                                     torch.from_numpy(np.array(kv_lens, np.int32)).cuda(), S, max(kv_lens), nq, nkv, hd,
                                     16, max_blocks)
    ctx.sync()
    forms.require("attn_kv_wide", "attn_split_reduce")
    got = host(out)
    for s, n in enumerate(kv_lens):
        ref = _ref_attention(O, q[s:s + 1], K[s], V[s], n - 1, nq, nkv, hd)
        assert nmse(ref, got[s:s + 1]) < 1e-5


@pytest.mark.parametrize("nq,nkv,hd,kv_lens,qk_mode,window", [
    (32, 4, 128, [1, 16, 17, 257, 300, 384, 33, 250], 1, 0), (32, 8, 128, [100, 5], 2, 0), (8, 8, 128, [48], 3, 0),
    (16, 2, 128, [700, 31], 0, 0), (4, 2, 64, [77, 64, 65], 1, 0), (8, 2, 256, [40, 130], 1, 0), (32, 4, 128, [4096, 1500], 1, 0),
    (32, 16, 128, [300, 7, 1024, 1025, 40], 1, 64), (8, 2, 128, [90, 33], 2, 17)])
def test_paged_decode_attention_fused_qkv_equals_two_op_chain(env, nq, nkv, hd, kv_lens, qk_mode, window):
    """One-launch decode (QK-norm + RoPE + KV write in the attention prologue) is bit-identical — attention output
    AND both cache pools — to split_qkv_norm_rope_into_paged_cache_varlen + paged_batched_decode_attention."""
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(nq * 3 + nkv + hd + len(kv_lens) + qk_mode)
    S = len(kv_lens)
    b = _paged_batch(env, rng, kv_lens, nq, nkv, hd, spare_blocks=3, spare_columns=1)    # (the last slot of each sequence holds stale values the step overwrites)
    tables, ck, cv, max_blocks = b.tables, b.ck, b.cv, b.max_blocks
    ck2, cv2 = ck.clone(), cv.clone()
    cos, sin = _rope(O, hd, max(kv_lens) + 1)
    cosd, sind = torch.from_numpy(cos).cuda(), torch.from_numpy(sin).cuda()
    qkv = dev16(torch, rng.standard_normal((S, (nq + 2 * nkv) * hd)))
    qn, kn = dev16(torch, 1 + 0.1 * rng.standard_normal(hd)), dev16(torch, 1 + 0.1 * rng.standard_normal(hd))
    td = torch.from_numpy(tables).cuda()
    lens = torch.from_numpy(np.array(kv_lens, np.int32)).cuda()
    q_out = torch.empty(S, nq, hd, dtype=torch.float16, device="cuda")
    out1 = torch.empty(S, nq, hd, dtype=torch.float16, device="cuda")
    out2 = torch.zeros_like(out1)
    B.split_qkv_norm_rope_into_paged_cache_varlen(ctx, qkv, qn, kn, cosd, sind, q_out, ck, cv,
                                                  torch.arange(S + 1, dtype=torch.int32, device="cuda"), lens - 1, td, S, S,
                                                  nq, nkv, hd, 1e-6, qk_mode, 16, max_blocks)
    if window:      # sliding window: the varlen op is the two-op reference (decode form: one query token per sequence)
        B.paged_varlen_attention(ctx, q_out, ck, cv, out1, torch.arange(S + 1, dtype=torch.int32, device="cuda"), lens - 1, td, S, S,
                                 max(kv_lens), nq, nkv, hd, window, 16, max_blocks, max_q_len=1)
    else:
        B.paged_batched_decode_attention(ctx, q_out, ck, cv, out1, td, lens, S, max(kv_lens), nq, nkv, hd, 16, max_blocks)
    B.paged_decode_attention_fused_qkv(ctx, qkv, qn, kn, cosd, sind, 1e-6, qk_mode, ck2, cv2, out2, td, lens, S, max(kv_lens),
                                       nq, nkv, hd, 16, max_blocks, sliding_window=window)
    ctx.sync()
    assert torch.equal(ck, ck2) and torch.equal(cv, cv2)
    assert torch.equal(out1, out2)
    assert torch.isfinite(out2.float()).all()


# ── MoE ──────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("batch,ne,k,norm,seed", [(32, 128, 8, True, 0xDEADBEEF), (1, 128, 8, True, 0x1234),
                                                  (64, 128, 8, True, 0x5678), (8, 64, 4, False, 0xC0FFEE),
                                                  (4, 16, 1, True, 0x42), (3, 256, 8, True, 7)])
def test_route_topk_softmax(env, batch, ne, k, norm, seed):
    # router.rs:203-244 shapes; ids bit-exact, weights within the renorm-divide ulps (1e-6, :219-222)
    pkg, B, ctx, O, torch = env
    logits = O.Lcg(seed).array_f32(batch * ne, -3.0, 3.0).reshape(batch, ne)
    ids = torch.empty(batch, k, dtype=torch.int32, device="cuda")
    w = torch.empty(batch, k, dtype=torch.float32, device="cuda")
    B.route_topk_softmax(ctx, torch.from_numpy(logits).cuda(), ids, w, batch, ne, k, norm)
    ctx.sync()
    rid, rw = O.route_topk(logits, ne, k, norm)
    assert np.array_equal(ids.cpu().numpy().astype(np.uint32), rid)
    assert np.max(np.abs(w.cpu().numpy() - rw)) < 1e-6
    # fp16-logit entry point (moe_router.cu:32 form)
    l16 = f16r(logits)
    B.route_topk_softmax(ctx, dev16(torch, l16), ids, w, batch, ne, k, norm)
    ctx.sync()
    rid, rw = O.route_topk(l16, ne, k, norm)
    assert np.array_equal(ids.cpu().numpy().astype(np.uint32), rid)


def test_route_ties_lowest_index(env):
    pkg, B, ctx, O, torch = env
    logits = np.full((2, 128), 0.5, np.float32)
    ids = torch.empty(2, 8, dtype=torch.int32, device="cuda")
    w = torch.empty(2, 8, dtype=torch.float32, device="cuda")
    B.route_topk_softmax(ctx, torch.from_numpy(logits).cuda(), ids, w, 2, 128, 8, True)
    ctx.sync()
    assert np.array_equal(ids.cpu().numpy(), np.tile(np.arange(8), (2, 1)))
    assert np.all(np.abs(w.cpu().numpy() - 0.125) < 1e-7)


@pytest.mark.parametrize("tokens,ne,k", [(1, 128, 8), (32, 128, 8), (700, 128, 8), (5, 8, 2), (0, 16, 2)])
def test_moe_align_block_size_bit_exact(env, tokens, ne, k):
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(tokens + ne)
    ids = np.stack([rng.choice(ne, size=k, replace=False) for _ in range(tokens)]).astype(np.int32) if tokens else \
        np.zeros((0, k), np.int32)
    n = tokens * k
    sorted_max = n + ne * 16
    sd = torch.full((sorted_max,), -7, dtype=torch.int32, device="cuda")
    bd = torch.full((sorted_max // 16 + 1,), -7, dtype=torch.int32, device="cuda")
    td = torch.zeros(1, dtype=torch.int32, device="cuda")
    B.moe_align_block_size_pair_ids(ctx, torch.from_numpy(ids.reshape(-1).copy()).cuda(), sd, bd, td, n, ne, 16, sorted_max)
    ctx.sync()
    rs, rb, rt = O.moe_align_block_size(ids, ne, 16)
    assert int(td.item()) == rt
    assert np.array_equal(sd.cpu().numpy(), rs)
    assert np.array_equal(bd.cpu().numpy()[:len(rb)], rb)


@pytest.mark.parametrize("tokens,E,K,H,I", [(1, 8, 2, 256, 128), (9, 8, 2, 256, 128), (32, 16, 4, 512, 256), (64, 8, 2, 256, 128),
                                            (32, 128, 8, 2048, 768), (96, 128, 8, 2048, 768),    # Qwen3-30B-A3B expert dims
                                            (1, 128, 8, 2048, 768), (7, 128, 8, 2048, 768)])
def test_moe_grouped_gemm_and_combine(env, tokens, E, K, H, I, forms):
    # whole expert MLP path vs moe_forward_cpu (dispatch.rs:2208-2288), plain and fused-silu stacks
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(tokens * E + H)
    gu = [O.make_synthetic_gptq(H, 2 * I, 128, 100 + e, symmetric=True) for e in range(E)]
    dn = [O.make_synthetic_gptq(I, H, 128, 200 + e, symmetric=True) for e in range(E)]
    gu = [(q, f16r(s / (0.28 * np.sqrt(H))), z) for q, s, z in gu]
    dn = [(q, f16r(s / (0.28 * np.sqrt(I))), z) for q, s, z in dn]
    x = f16r(rng.standard_normal((tokens, H)))
    logits = rng.standard_normal((tokens, E)).astype(np.float32)
    rid, rw = O.route_topk(logits, E, K, True)
    gw = np.stack([O.dequant_gptq(q, s, z, 128, H, 2 * I) for q, s, z in gu])
    dw = np.stack([O.dequant_gptq(q, s, z, 128, I, H) for q, s, z in dn])
    ref = O.moe_forward_cpu(x, H, I, K, rid, rw, gw, dw)
    P = tokens * K
    sorted_max = P + E * 16
    ids_d = torch.from_numpy(rid.astype(np.int32).reshape(-1).copy()).cuda()
    sd = torch.empty(sorted_max, dtype=torch.int32, device="cuda")
    bd = torch.empty(sorted_max // 16 + 1, dtype=torch.int32, device="cuda")
    td = torch.zeros(1, dtype=torch.int32, device="cuda")
    B.moe_align_block_size_pair_ids(ctx, ids_d, sd, bd, td, P, E, 16, sorted_max)
    max_blocks = sorted_max // 16
    xd = dev16(torch, x)
    wd = torch.from_numpy(rw.reshape(-1).copy()).cuda()
    down_stack = B.load_gptq_stacked([q for q, _, _ in dn], [s for _, s, _ in dn], [z for _, _, z in dn], None, 4, 128, I, H)
    for fused in (False, True):
        stack = B.load_gptq_stacked([q for q, _, _ in gu], [s for _, s, _ in gu], [z for _, _, z in gu], None, 4, 128, H,
                                    2 * I, fuse_gate_up=fused)
        act = torch.zeros(P, I, dtype=torch.float16, device="cuda")
        forms.reset()
        if fused:
            stack.gemm_phase_vllm(ctx, xd, sd, bd, td, act, P, 16, K, max_blocks, fused_silu_mul=True)
        else:
            gup = torch.zeros(P, 2 * I, dtype=torch.float16, device="cuda")
            stack.gemm_phase_vllm(ctx, xd, sd, bd, td, gup, P, 16, K, max_blocks)
            B.fused_silu_mul_split(ctx, gup, act, P, I)
        down = torch.zeros(P, H, dtype=torch.float16, device="cuda")
        down_stack.gemm_phase_vllm(ctx, act, sd, bd, td, down, P, 16, 1, max_blocks)
        forms.require("moe_block16")
        out = torch.zeros(tokens, H, dtype=torch.float16, device="cuda")
        B.moe_combine(ctx, down, wd, out, tokens, K, H)
        ctx.sync()
        assert nmse(ref, host(out)) < 3e-6, fused            # three fp16 roundings (act, down, out)
        for blk in ((64, 32) + ((128, 96) if I % 256 == 0 and H % 256 == 0 else ()) if fused and P >= 64 else ()):
            # 64- and 32-row blocks through the prefill tile kernel: same maths, different block shape; 128-row blocks through
            # w4_gemm_big_kernel: the group scale folded into fp16 weights (one more rounding per weight, like the reference's own
            # fp16 dequantisation), so equal within the tolerance, not bit for bit
            sdb = torch.empty(P + E * blk, dtype=torch.int32, device="cuda")
            bdb = torch.empty((P + E * blk) // blk + 1, dtype=torch.int32, device="cuda")
            tdb = torch.zeros(1, dtype=torch.int32, device="cuda")
            B.moe_align_block_size_pair_ids(ctx, ids_d, sdb, bdb, tdb, P, E, blk, P + E * blk)
            mbb = (P + E * blk) // blk
            actb = torch.zeros(P, I, dtype=torch.float16, device="cuda")
            downb = torch.zeros(P, H, dtype=torch.float16, device="cuda")
            forms.reset()
            stack.gemm_phase_vllm(ctx, xd, sdb, bdb, tdb, actb, P, blk, K, mbb, fused_silu_mul=True)
            down_stack.gemm_phase_vllm(ctx, actb, sdb, bdb, tdb, downb, P, blk, 1, mbb)
            forms.require({64: "moe_tile64", 32: "moe_tile32"}.get(blk, "moe_tile_big"), absent=("moe_block16",))
            outb = torch.zeros(tokens, H, dtype=torch.float16, device="cuda")
            B.moe_combine(ctx, downb, wd, outb, tokens, K, H)
            ctx.sync()
            if blk < 96: assert torch.equal(actb, act), blk      # per-row sums are independent of the block shape
            else: assert nmse(host(act), host(actb)) < 1e-6, blk
            assert nmse(ref, host(outb)) < 3e-6, blk
        # expert-major grid straight from the raw expert ids (no align arrays): bit-identical outputs; experts with more
        # than 16 pairs (the 64-token / 8-expert case) take further passes, experts without pairs leave early
        # (≤ 16 pairs of a K ≥ 512 stack: the block-major launches above split K over four waves — another fp32 summation order)
        same = (lambda x_, y_: torch.equal(x_, y_)) if P > 16 else (lambda x_, y_: nmse(host(x_), host(y_)) < 1e-6)
        down3 = torch.zeros(P, H, dtype=torch.float16, device="cuda")
        forms.reset()
        if fused:
            act3 = torch.zeros(P, I, dtype=torch.float16, device="cuda")
            stack.gemm_phase_expert_major(ctx, xd, ids_d, act3, P, E, K, fused_silu_mul=True)
            ctx.sync()
            assert same(act, act3)
        else:
            gup3 = torch.zeros(P, 2 * I, dtype=torch.float16, device="cuda")
            stack.gemm_phase_expert_major(ctx, xd, ids_d, gup3, P, E, K)
            ctx.sync()
            assert same(gup, gup3)
        down_stack.gemm_phase_expert_major(ctx, act3 if fused else act, ids_d, down3, P, E, 1)
        forms.require("moe_expert_major")
        ctx.sync()
        assert same(down, down3)
        if fused and P <= 1024 and I >= 256:
            # gate_up → down as ONE launch (down tiles wait in the launch for their expert's gate_up tiles): the same bits, on
            # poisoned output buffers, three times over (the counters are re-armed per call)
            forms.reset()
            for rep in range(3):
                act4 = torch.full((P, I), float("nan"), dtype=torch.float16, device="cuda")
                down4 = torch.full((P, H), float("nan"), dtype=torch.float16, device="cuda")
                stack.gemm_phase_expert_major_pair(ctx, down_stack, xd, ids_d, act4, down4, P, E, K)
                ctx.sync()
                assert stack.pair_timeouts(ctx) == 0
                assert torch.equal(act3, act4) and torch.equal(down3, down4), rep      # the bits of the two expert-major launches
            forms.require("moe_expert_major_pair")
        if fused:
            # align computed inside the GEMM from the raw expert ids: bit-identical outputs
            act2 = torch.zeros(P, I, dtype=torch.float16, device="cuda")
            down2 = torch.zeros(P, H, dtype=torch.float16, device="cuda")
            forms.reset()
            stack.gemm_phase_inline_align(ctx, xd, ids_d, act2, P, E, K, max_blocks, fused_silu_mul=True)
            down_stack.gemm_phase_inline_align(ctx, act2, ids_d, down2, P, E, 1, max_blocks)
            forms.require("moe_inline_align")
            ctx.sync()
            assert torch.equal(act, act2) and torch.equal(down, down2)


@pytest.mark.parametrize("tokens,E,K,H,I", [(9, 8, 2, 256, 128), (32, 128, 8, 2048, 768), (80, 128, 8, 2048, 768)])
@pytest.mark.parametrize("asym,desc_act", [(True, False), (False, True), (True, True)])
def test_moe_asymmetric_and_act_order_expert_stacks(env, tokens, E, K, H, I, asym, desc_act, forms):
    """Expert stacks with non-8 zero points (the reference's vLLM-Marlin branch, cuda/quant.rs:795-839) and with an act-order
    g_idx shared by the stack (cuda/quant.rs:862 ff., capabilities.rs:180-189) against moe_forward_cpu on weights dequantised
    WITH g_idx (cpu.rs:2283-2315): every phase entry point, at Qwen3-30B-A3B expert dims."""
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(tokens * E + H + 2 * asym + desc_act)
    gu = [O.make_synthetic_gptq(H, 2 * I, 128, 300 + e, symmetric=not asym) for e in range(E)]
    dn = [O.make_synthetic_gptq(I, H, 128, 500 + e, symmetric=not asym) for e in range(E)]
    gu = [(q, f16r(s / (0.28 * np.sqrt(H))), z) for q, s, z in gu]
    dn = [(q, f16r(s / (0.28 * np.sqrt(I))), z) for q, s, z in dn]
    gi_gu = O.make_desc_act_g_idx(H, 128) if desc_act else None
    gi_dn = O.make_desc_act_g_idx(I, 128) if desc_act else None
    x = f16r(rng.standard_normal((tokens, H)))
    rid, rw = O.route_topk(rng.standard_normal((tokens, E)).astype(np.float32), E, K, True)
    gw = np.stack([O.dequant_gptq(q, s, z, 128, H, 2 * I, g_idx=gi_gu) for q, s, z in gu])
    dw = np.stack([O.dequant_gptq(q, s, z, 128, I, H, g_idx=gi_dn) for q, s, z in dn])
    ref = O.moe_forward_cpu(x, H, I, K, rid, rw, gw, dw)
    P = tokens * K
    ids_d = torch.from_numpy(rid.astype(np.int32).reshape(-1).copy()).cuda()
    xd, x_keep = dev16(torch, x), dev16(torch, x)
    wd = torch.from_numpy(rw.reshape(-1).copy()).cuda()
    stack = B.load_gptq_stacked([q for q, _, _ in gu], [s for _, s, _ in gu], [z for _, _, z in gu], gi_gu, 4, 128, H, 2 * I,
                                fuse_gate_up=True)
    down_stack = B.load_gptq_stacked([q for q, _, _ in dn], [s for _, s, _ in dn], [z for _, _, z in dn], gi_dn, 4, 128, I, H)

    def combine(down):
        out = torch.zeros(tokens, H, dtype=torch.float16, device="cuda")
        B.moe_combine(ctx, down, wd, out, tokens, K, H)
        ctx.sync()
        return host(out)

    base = None
    for blk in (16, 64):
        sd = torch.empty(P + E * blk, dtype=torch.int32, device="cuda")
        bd = torch.empty((P + E * blk) // blk + 1, dtype=torch.int32, device="cuda")
        td = torch.zeros(1, dtype=torch.int32, device="cuda")
        B.moe_align_block_size_pair_ids(ctx, ids_d, sd, bd, td, P, E, blk, P + E * blk)
        mb = (P + E * blk) // blk
        act = torch.full((P, I), float("nan"), dtype=torch.float16, device="cuda")
        down = torch.full((P, H), float("nan"), dtype=torch.float16, device="cuda")
        stack.gemm_phase_vllm(ctx, xd, sd, bd, td, act, P, blk, K, mb, fused_silu_mul=True)
        down_stack.gemm_phase_vllm(ctx, act, sd, bd, td, down, P, blk, 1, mb)
        assert nmse(ref, combine(down)) < 3e-6, blk
        if base is None: base = (act, down)
        else: assert torch.equal(act, base[0]) and torch.equal(down, base[1])      # block shape does not change a row's sum
    act, down = base
    act3 = torch.full((P, I), float("nan"), dtype=torch.float16, device="cuda")
    down3 = torch.full((P, H), float("nan"), dtype=torch.float16, device="cuda")
    stack.gemm_phase_expert_major(ctx, xd, ids_d, act3, P, E, K, fused_silu_mul=True)
    down_stack.gemm_phase_expert_major(ctx, act3, ids_d, down3, P, E, 1)
    ctx.sync()
    assert torch.equal(act, act3) and torch.equal(down, down3)
    act2 = torch.full((P, I), float("nan"), dtype=torch.float16, device="cuda")
    down2 = torch.full((P, H), float("nan"), dtype=torch.float16, device="cuda")
    stack.gemm_phase_inline_align(ctx, xd, ids_d, act2, P, E, K, P // 16 + E, fused_silu_mul=True)
    down_stack.gemm_phase_inline_align(ctx, act2, ids_d, down2, P, E, 1, P // 16 + E)
    ctx.sync()
    assert torch.equal(act, act2) and torch.equal(down, down2)
    if I >= 256:
        act4 = torch.full((P, I), float("nan"), dtype=torch.float16, device="cuda")
        down4 = torch.full((P, H), float("nan"), dtype=torch.float16, device="cuda")
        if desc_act:        # the down stack's input gather cannot sit inside the one launch: refused, callers run two phases
            with pytest.raises(pkg.backend.Unsupported, match="act-order down stack"):
                stack.gemm_phase_expert_major_pair(ctx, down_stack, xd, ids_d, act4, down4, P, E, K)
        else:
            forms.reset()
            stack.gemm_phase_expert_major_pair(ctx, down_stack, xd, ids_d, act4, down4, P, E, K)
            ctx.sync()
            assert stack.pair_timeouts(ctx) == 0
            assert torch.equal(act, act4) and torch.equal(down, down4)
            forms.require("moe_expert_major_pair")
    assert torch.equal(xd, x_keep)                                         # the gather works on a scratch copy


def mixed_stack_case(O, asym_experts, tokens=5, E=3, K=2, H=256, I=128):
    """Inputs and the dequantised CPU reference of test_moe_mixed_symmetric_and_asymmetric_expert_stack (no GPU involved)."""
    rng = np.random.default_rng(1000 + 7 * sum(1 << e for e in asym_experts))
    gu = [O.make_synthetic_gptq(H, 2 * I, 128, 700 + e, symmetric=e not in asym_experts) for e in range(E)]
    dn = [O.make_synthetic_gptq(I, H, 128, 900 + e, symmetric=e not in asym_experts) for e in range(E)]
    gu = [(q, f16r(s / (0.28 * np.sqrt(H))), z) for q, s, z in gu]
    dn = [(q, f16r(s / (0.28 * np.sqrt(I))), z) for q, s, z in dn]
    x = f16r(rng.standard_normal((tokens, H)))
    rid, rw = O.route_topk(rng.standard_normal((tokens, E)).astype(np.float32), E, K, True)
    gw = np.stack([O.dequant_gptq(q, s, z, 128, H, 2 * I) for q, s, z in gu])
    dw = np.stack([O.dequant_gptq(q, s, z, 128, I, H) for q, s, z in dn])
    return gu, dn, x, rid, rw, O.moe_forward_cpu(x, H, I, K, rid, rw, gw, dw)


@pytest.mark.parametrize("asym_experts", [(1,), (0,)], ids=["sym-asym-sym", "asym-sym-sym"])
def test_moe_mixed_symmetric_and_asymmetric_expert_stack(env, asym_experts, forms):
    """A stack that mixes symmetric and asymmetric experts: the zero-point array arrives with the first asymmetric expert,
    after (sym, asym, sym) or before (asym, sym, sym) symmetric experts have been written, and those carry the explicit zero
    point 8.0.  Two quant groups, fused gate_up, 16-row blocks; bound of test_moe_asymmetric_and_act_order_expert_stacks."""
    pkg, B, ctx, O, torch = env
    tokens, E, K, H, I = 5, 3, 2, 256, 128
    gu, dn, x, rid, rw, ref = mixed_stack_case(O, asym_experts)
    assert np.isfinite(ref).all() and set(rid.reshape(-1).tolist()) == set(range(E))      # every expert holds a pair
    P = tokens * K
    ids_d = torch.from_numpy(rid.astype(np.int32).reshape(-1).copy()).cuda()
    xd, wd = dev16(torch, x), torch.from_numpy(rw.reshape(-1).copy()).cuda()
    stack = B.load_gptq_stacked([q for q, _, _ in gu], [s for _, s, _ in gu], [z for _, _, z in gu], None, 4, 128, H, 2 * I,
                                fuse_gate_up=True)
    down_stack = B.load_gptq_stacked([q for q, _, _ in dn], [s for _, s, _ in dn], [z for _, _, z in dn], None, 4, 128, I, H)
    sd = torch.empty(P + E * 16, dtype=torch.int32, device="cuda")
    bd = torch.empty((P + E * 16) // 16 + 1, dtype=torch.int32, device="cuda")
    td = torch.zeros(1, dtype=torch.int32, device="cuda")
    B.moe_align_block_size_pair_ids(ctx, ids_d, sd, bd, td, P, E, 16, P + E * 16)
    mb = (P + E * 16) // 16
    act = torch.full((P, I), float("nan"), dtype=torch.float16, device="cuda")
    down = torch.full((P, H), float("nan"), dtype=torch.float16, device="cuda")
    forms.reset()
    stack.gemm_phase_vllm(ctx, xd, sd, bd, td, act, P, 16, K, mb, fused_silu_mul=True)
    down_stack.gemm_phase_vllm(ctx, act, sd, bd, td, down, P, 16, 1, mb)
    forms.require("moe_block16")
    out = torch.zeros(tokens, H, dtype=torch.float16, device="cuda")
    B.moe_combine(ctx, down, wd, out, tokens, K, H)
    ctx.sync()
    err = nmse(ref, host(out))
    print("mixed stack", asym_experts, "nmse", err)
    assert err < 3e-6


@pytest.mark.parametrize("tokens,H,E,K", [(1, 2048, 128, 8), (32, 2048, 128, 8), (5, 1024, 64, 4), (3, 4096, 16, 2)])
def test_fused_add_rms_norm_route_equals_op_chain(env, tokens, H, E, K):
    # fused.hip B ≡ fused_add_rms_norm → gemm(router) → route_topk_softmax, each as the oracle defines it
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(tokens + H + E)
    r, x = f16r(rng.standard_normal((tokens, H)) * 2), f16r(rng.standard_normal((tokens, H)))
    w = f16r(1 + 0.1 * rng.standard_normal(H))
    rw = f16r(rng.standard_normal((E, H)) * 0.05)
    rd, nd = dev16(torch, r), torch.empty(tokens, H, dtype=torch.float16, device="cuda")
    ids = torch.empty(tokens, K, dtype=torch.int32, device="cuda")
    wt = torch.empty(tokens, K, dtype=torch.float32, device="cuda")
    lg = torch.empty(tokens, E, dtype=torch.float32, device="cuda")
    B.fused_add_rms_norm_route(ctx, rd, dev16(torch, x), dev16(torch, w), 1e-6, nd,
                               B.dense_repack_f16t(ctx, dev16(torch, rw), E, H), E, K, True, ids, wt, lg, tokens, H)
    ctx.sync()
    r_ref, _ = O.fused_add_rms_norm(r, x, w, 1e-6)
    assert nmse(r_ref, host(rd)) < NMSE_FP16_TOL
    n_ref = O.rms_norm(host(rd), w, 1e-6)                                  # norm of the fp16-rounded residual
    assert nmse(n_ref, host(nd)) < NMSE_FP16_TOL
    logits_ref = O.gemm(host(nd), rw, tokens, E, H)                        # router sees the fp16 norm_out
    assert nmse(logits_ref, lg.cpu().numpy()) < 1e-10
    rid, rwt = O.route_topk(lg.cpu().numpy(), E, K, True)                  # routing of the device logits: bit-exact ids
    assert np.array_equal(ids.cpu().numpy().astype(np.uint32), rid)
    assert np.max(np.abs(wt.cpu().numpy() - rwt)) < 1e-6


@pytest.mark.parametrize("tokens,H,E,K,Q,slabs", [(32, 2048, 128, 8, 4, 0), (1, 2048, 128, 8, 4, 3), (9, 1024, 64, 4, 2, 2),
                                                     (5, 512, 16, 2, 1, 0), (16, 2048, 128, 8, 8, 0)])
def test_route_parts_and_merge_equal_single_kernel_route(env, tokens, H, E, K, Q, slabs):
    """Decode path: router split over Q parts + candidate merge in the gate_up GEMM ≡ route_topk_softmax on the
    same logits (ids bit-exact, weights 1e-6), residual/norm as the op chain, align arrays as moe_align_block_size."""
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(tokens + H + E + Q)
    r = f16r(rng.standard_normal((tokens, H)) * 2)
    w = f16r(1 + 0.1 * rng.standard_normal(H))
    rw = f16r(rng.standard_normal((E, H)) * 0.05)
    if slabs:
        parts = [rng.standard_normal((tokens, H)).astype(np.float32) * 0.5 for _ in range(slabs)]
        xs = torch.from_numpy(np.stack(parts)).cuda()                      # [S, T, H] fp32
        x = f16r(sum(parts[1:], parts[0].copy()))                          # slab-order fp32 sum, rounded like the fp16 o_proj
        xd = None
    else:
        x = f16r(rng.standard_normal((tokens, H)))
        xs, xd = None, dev16(torch, x)
    rd, r2 = dev16(torch, r), torch.zeros(tokens, H, dtype=torch.float16, device="cuda")
    nd = torch.empty(tokens, H, dtype=torch.float16, device="cuda")
    cand = torch.zeros(tokens * Q * 8 * 2, dtype=torch.int32, device="cuda")
    stats = torch.zeros(tokens * Q * 2, dtype=torch.float32, device="cuda")
    lg = torch.empty(tokens, E, dtype=torch.float32, device="cuda")
    B.fused_add_rms_norm_route_parts(ctx, rd, r2, xd, xs, slabs, tokens * H, H, dev16(torch, w), 1e-6, nd,
                                     B.dense_repack_f16t(ctx, dev16(torch, rw), E, H), E, K, Q, cand, stats, lg, tokens, H)
    ctx.sync()
    assert np.array_equal(host(rd), r)                                     # input residual untouched (ping-pong)
    r_ref, _ = O.fused_add_rms_norm(r, x, w, 1e-6)
    assert nmse(r_ref, host(r2)) < NMSE_FP16_TOL
    assert nmse(O.rms_norm(host(r2), w, 1e-6), host(nd)) < NMSE_FP16_TOL
    logits = lg.cpu().numpy()
    assert nmse(O.gemm(host(nd), rw, tokens, E, H), logits) < 1e-10
    # merge inside a grouped GEMM (tiny expert stack; only the routing outputs are checked here)
    Hs, I = 128, 64
    gu = [O.make_synthetic_gptq(Hs, 2 * I, 128, 300 + e, symmetric=True) for e in range(E)]
    stack = B.load_gptq_stacked([q for q, _, _ in gu], [f16r(s) for _, s, _ in gu], [z for _, _, z in gu], None, 4, 128, Hs, 2 * I)
    P = tokens * K
    sorted_max = P + E * 16
    xin = dev16(torch, rng.standard_normal((tokens, Hs)))
    out = torch.zeros(P, 2 * I, dtype=torch.float16, device="cuda")
    ids = torch.full((P,), -1, dtype=torch.int32, device="cuda")
    wts = torch.zeros(P, dtype=torch.float32, device="cuda")
    sd = torch.full((sorted_max,), P, dtype=torch.int32, device="cuda")
    bd = torch.zeros(sorted_max // 16 + 1, dtype=torch.int32, device="cuda")
    td = torch.zeros(1, dtype=torch.int32, device="cuda")
    stack.gemm_phase_merge_route(ctx, xin, cand, stats, out, tokens, Q, K, True, E, sorted_max // 16, ids, wts, sd, bd, td)
    ctx.sync()
    rid, rwt = O.route_topk(logits, E, K, True)
    assert np.array_equal(ids.cpu().numpy().reshape(tokens, K).astype(np.uint32), rid)
    assert np.max(np.abs(wts.cpu().numpy().reshape(tokens, K) - rwt)) < 1e-6
    rs, rb, rt = O.moe_align_block_size(rid.astype(np.int32), E, 16)
    assert int(td.item()) == rt
    assert np.array_equal(sd.cpu().numpy()[:rt], rs[:rt]) and np.array_equal(bd.cpu().numpy()[:len(rb)], rb)
    out2 = torch.zeros_like(out)
    stack.gemm_phase_inline_align(ctx, xin, ids, out2, P, E, K, sorted_max // 16)
    ctx.sync()
    assert torch.equal(out, out2)


@pytest.mark.parametrize("tokens,H,E,K,Q,slabs", [(32, 2048, 128, 8, 4, 8), (64, 2048, 128, 8, 8, 0), (1, 2048, 128, 8, 2, 3),
                                                     (9, 1024, 64, 4, 2, 2), (5, 512, 16, 2, 1, 0), (33, 2048, 128, 8, 4, 0)])
def test_route_split_in_launch_merge_equals_route_topk(env, tokens, H, E, K, Q, slabs):
    """Split router with the merge done by each token's last-arriving part: ids bit-exact and weights 1e-6 against
    route_topk_softmax on the emitted logits; repeated launches reuse cand/stats/arrive (counter re-arm, stale lines)."""
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(7 * tokens + H + E + Q)
    w = f16r(1 + 0.1 * rng.standard_normal(H))
    rw = f16r(rng.standard_normal((E, H)) * 0.05)
    rwt = B.dense_repack_f16t(ctx, dev16(torch, rw), E, H)
    cand = torch.zeros(tokens * Q * 8 * 2, dtype=torch.int32, device="cuda")
    stats = torch.zeros(tokens * Q * 2, dtype=torch.float32, device="cuda")
    arrive = torch.zeros(tokens, dtype=torch.int32, device="cuda")
    wd = dev16(torch, w)
    for rep in range(4):
        r = f16r(rng.standard_normal((tokens, H)) * 2)
        if slabs:
            parts = [rng.standard_normal((tokens, H)).astype(np.float32) * 0.5 for _ in range(slabs)]
            xs = torch.from_numpy(np.stack(parts)).cuda()
            x = f16r(sum(parts[1:], parts[0].copy()))
            xd = None
        else:
            x = f16r(rng.standard_normal((tokens, H)))
            xs, xd = None, dev16(torch, x)
        rd, r2 = dev16(torch, r), torch.zeros(tokens, H, dtype=torch.float16, device="cuda")
        nd = torch.empty(tokens, H, dtype=torch.float16, device="cuda")
        lg = torch.empty(tokens, E, dtype=torch.float32, device="cuda")
        ids = torch.full((tokens, K), -1, dtype=torch.int32, device="cuda")
        wts = torch.zeros(tokens, K, dtype=torch.float32, device="cuda")
        B.fused_add_rms_norm_route_split(ctx, rd, r2, xd, xs, slabs, tokens * H, H, wd, 1e-6, nd, rwt, E, K, rep % 2, Q, cand,
                                         stats, arrive, ids, wts, lg, tokens, H)
        ctx.sync()
        assert int(arrive.abs().sum().item()) == 0                         # counters re-armed
        r_ref, _ = O.fused_add_rms_norm(r, x, w, 1e-6)
        assert nmse(r_ref, host(r2)) < NMSE_FP16_TOL
        assert nmse(O.rms_norm(host(r2), w, 1e-6), host(nd)) < NMSE_FP16_TOL
        logits = lg.cpu().numpy()
        assert nmse(O.gemm(host(nd), rw, tokens, E, H), logits) < 1e-10
        rid, rwt_ref = O.route_topk(logits, E, K, bool(rep % 2))
        assert np.array_equal(ids.cpu().numpy().astype(np.uint32), rid), f"rep {rep}"
        assert np.max(np.abs(wts.cpu().numpy() - rwt_ref)) < 1e-6


@pytest.mark.parametrize("tokens,H,K,with_norm", [(1, 2048, 8, True), (32, 2048, 8, True), (7, 1024, 2, False)])
def test_moe_combine_add_rms_norm_equals_op_chain(env, tokens, H, K, with_norm):
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(tokens * H + K)
    down = f16r(rng.standard_normal((tokens * K, H)))
    wts = rng.random((tokens, K)).astype(np.float32)
    wts /= wts.sum(axis=1, keepdims=True)
    r = f16r(rng.standard_normal((tokens, H)))
    nw = f16r(1 + 0.1 * rng.standard_normal(H))
    rd, nd = dev16(torch, r), torch.zeros(tokens, H, dtype=torch.float16, device="cuda")
    B.moe_combine_add_rms_norm(ctx, dev16(torch, down), torch.from_numpy(wts).cuda(), rd,
                               dev16(torch, nw) if with_norm else None, 1e-6, nd, tokens, K, H)
    ctx.sync()
    comb = np.zeros((tokens, H), np.float32)
    for b in range(tokens):
        for k in range(K):
            comb[b] += wts[b, k] * down[b * K + k]                         # moe_forward_cpu order (dispatch.rs:2277-2283)
    assert nmse(r + comb, host(rd)) < NMSE_FP16_TOL
    if with_norm:
        assert nmse(O.rms_norm(host(rd), nw, 1e-6), host(nd)) < NMSE_FP16_TOL
    else:
        assert not host(nd).any()


# ── sampling ─────────────────────────────────────────────────────────────────
def test_argmax_rows_first_max_and_mask(env):
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(9)
    m, n = 5, 151936
    logits = rng.standard_normal((m, n)).astype(np.float32)
    logits[0, 777] = logits[0, 120000] = 9.0               # tie → first index (traits.rs:1547)
    logits[1, n - 1] = 50.0
    logits[2, 0] = 50.0
    ld = torch.from_numpy(logits).cuda()
    assert np.array_equal(B.argmax_rows_f16(ctx, ld, m, n), O.argmax_rows(logits))
    l16 = f16r(logits)
    assert np.array_equal(B.argmax_rows_f16(ctx, dev16(torch, l16), m, n), O.argmax_rows(l16))
    mask = np.ones(n, np.uint8)
    mask[777] = 0
    mask_len = n - 1                                        # ids ≥ mask_len are invalid
    got = B.argmax_rows_f16_masked(ctx, ld, torch.from_numpy(mask).cuda(), mask_len, m, n)
    masked = logits.copy()
    masked[:, 777] = -np.inf
    masked[:, mask_len:] = -np.inf
    assert np.array_equal(got, O.argmax_rows(masked))
    # single-launch entry point (no workspace) and an all -inf row (→ id 0 on both paths)
    logits[3, :] = -np.inf
    ld = torch.from_numpy(logits).cuda()
    out = torch.empty(m, dtype=torch.int32, device="cuda")
    import ctypes
    assert ctx.lib.ferrum_hip_argmax_rows_f32(ctypes.c_void_p(ld.data_ptr()), ctypes.c_void_p(out.data_ptr()), None, 0, m, n,
                                              ctx.stream) == 0
    ctx.sync()
    ref = O.argmax_rows(logits)
    assert ref[3] == 0
    assert np.array_equal(out.cpu().numpy().astype(np.uint32), ref)
    assert np.array_equal(B.argmax_rows_f16(ctx, ld, m, n), ref)


@pytest.mark.parametrize("n", [4096, 5003, 40000, 40004])
def test_argmax_rows_widths_and_mask_tails(env, n):
    """Row widths on both sides of the vector form's conditions (n % 8, ≥ 4096) with a mask shorter than the row."""
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(n)
    m = 7
    logits = rng.standard_normal((m, n)).astype(np.float32)
    logits[0, n - 1] = 30.0
    logits[1, n - 3] = logits[1, 5] = 30.0
    logits[2, :] = 1.0                                      # all equal → id 0, or the first valid id under the mask
    ld = torch.from_numpy(logits).cuda()
    assert np.array_equal(B.argmax_rows_f16(ctx, ld, m, n), O.argmax_rows(logits))
    l16 = f16r(logits)
    assert np.array_equal(B.argmax_rows_f16(ctx, dev16(torch, l16), m, n), O.argmax_rows(l16))
    mask = (rng.random(n) < 0.7).astype(np.uint8)
    mask[:3] = 0
    mask_len = n - 5
    got = B.argmax_rows_f16_masked(ctx, ld, torch.from_numpy(mask).cuda(), mask_len, m, n)
    masked = logits.copy()
    masked[:, mask == 0] = -np.inf
    masked[:, mask_len:] = -np.inf
    assert np.array_equal(got, O.argmax_rows(masked))


def test_sparse_repetition_penalty_then_argmax(env):
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(10)
    m, n = 3, 4096
    logits = rng.standard_normal((m, n)).astype(np.float32)
    prev = [np.unique(rng.integers(0, n, size=50)).astype(np.uint32) for _ in range(m)]
    for r in range(m):
        logits[r, prev[r][0]] = 20.0                        # the penalised id was the winner
    offs = np.concatenate([[0], np.cumsum([len(p) for p in prev])]).astype(np.int32)
    pens = np.array([1.1, 1.0, 3.0], np.float32)
    ld = torch.from_numpy(logits.copy()).cuda()
    got = B.argmax_rows_f16_sparse_repetition_penalty(
        ctx, ld, None, torch.from_numpy(offs).cuda(), torch.from_numpy(np.concatenate(prev).astype(np.int32)).cuda(),
        torch.from_numpy(pens).cuda(), int(offs[-1]), m, n)
    ref_logits = np.stack([O.repetition_penalty(logits[r], prev[r], float(pens[r])) for r in range(m)])
    assert np.allclose(ld.cpu().numpy(), ref_logits, rtol=1e-6, atol=0)
    assert np.array_equal(got, O.argmax_rows(ref_logits))


# ── trait-surface entry points of the bucketed MoE path and the single-sequence paged attention ─────────────────
@pytest.mark.parametrize("tokens,ne,k,block", [(1, 128, 8, 16), (32, 128, 8, 16), (700, 128, 8, 64), (5, 8, 2, 16), (257, 60, 4, 32)])
def test_moe_build_pairs_by_token_and_packed_row_align_bit_exact(env, tokens, ne, k, block):
    """moe_build_pairs_by_token (capabilities.rs:410) and the packed-row moe_align_block_size (capabilities.rs:429): the
    device plan must equal MoeBucketPlan::rebuild_into (moe/dispatch.rs:1408-1461, restated in the oracle) bit for bit —
    a STABLE counting sort, where the reference's CUDA kernels leave the order inside an expert to atomicAdd."""
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(tokens * 131 + ne)
    ids = np.stack([rng.choice(ne, size=k, replace=False) for _ in range(tokens)]).astype(np.uint32)
    P = tokens * k
    off_ref, packed_ref, pairs_ref = O.bucket_plan(ids, tokens, ne, k)
    ids_d = torch.from_numpy(ids.astype(np.int32).reshape(-1).copy()).cuda()
    pairs = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    packed = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    offs = torch.full((ne + 1,), -7, dtype=torch.int32, device="cuda")
    B.moe_build_pairs_by_token(ctx, ids_d, pairs, packed, offs, P, ne, k)
    ctx.sync()
    assert np.array_equal(offs.cpu().numpy(), np.asarray(off_ref, np.int32))
    assert np.array_equal(packed.cpu().numpy(), np.asarray(packed_ref, np.int32))
    assert np.array_equal(pairs.cpu().numpy(), np.asarray(pairs_ref, np.int32))
    # packed-row align: expert e's padded region holds expert_offsets[e] + 0, 1, …; padding and the unused tail hold P
    sorted_max = P + ne * block
    sd = torch.full((sorted_max,), -7, dtype=torch.int32, device="cuda")
    bd = torch.full((sorted_max // block + 1,), -7, dtype=torch.int32, device="cuda")
    td = torch.zeros(1, dtype=torch.int32, device="cuda")
    B.moe_align_block_size(ctx, ids_d, sd, bd, td, P, ne, block, sorted_max)
    ctx.sync()
    exp_sorted, exp_blocks = [], []
    for e in range(ne):
        cnt = int(off_ref[e + 1] - off_ref[e])
        pad = -(-cnt // block) * block
        exp_sorted += [int(off_ref[e]) + i for i in range(cnt)] + [P] * (pad - cnt)
        exp_blocks += [e] * (pad // block)
    assert int(td.item()) == len(exp_sorted)
    got = sd.cpu().numpy()
    assert np.array_equal(got[:len(exp_sorted)], np.asarray(exp_sorted, np.int32)) and np.all(got[len(exp_sorted):] == P)
    assert np.array_equal(bd.cpu().numpy()[:len(exp_blocks)], np.asarray(exp_blocks, np.int32))
    # ids outside [0, E) are skipped: pairs_by_token = −1 (kernels/moe_build_pairs.cu:84-87), the rest unchanged in order
    bad = ids.astype(np.int32).reshape(-1).copy()
    bad[::3] = np.where(np.arange(len(bad[::3])) % 2 == 0, -1, ne + 5)
    pairs.fill_(-7)
    B.moe_build_pairs_by_token(ctx, torch.from_numpy(bad).cuda(), pairs, packed, offs, P, ne, k)
    ctx.sync()
    pr, of = pairs.cpu().numpy(), offs.cpu().numpy()
    valid = (bad >= 0) & (bad < ne)
    assert np.all(pr[~valid] == -1) and of[ne] == valid.sum()
    for e in range(ne):
        rows = pr[valid & (bad == e)]
        assert np.array_equal(rows, np.arange(of[e], of[e + 1]))       # ascending pair id inside an expert


@pytest.mark.parametrize("tokens,K,H", [(1, 8, 2048), (32, 8, 2048), (7, 2, 1024)])
def test_moe_combine_by_pairs_and_weighted_sum_batched(env, tokens, K, H):
    """moe_combine with pairs_by_token (capabilities.rs:684-724: out[b] = Σ_k w[b,k]·packed_down[pairs[b,k]], −1 skipped)
    and weighted_sum_batched[_offset] (capabilities.rs:560-600), against the trait's own default loop in f32."""
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(tokens + K + H)
    P = tokens * K
    down = f16r(rng.standard_normal((P, H)))
    w = rng.random((tokens, K)).astype(np.float32)
    pairs = rng.permutation(P).astype(np.int32).reshape(tokens, K)
    if tokens > 1:
        pairs[1, 0] = -1
    ref = np.zeros((tokens, H), np.float32)
    for b in range(tokens):
        for k in range(K):
            if pairs[b, k] >= 0:
                ref[b] += w[b, k] * down[pairs[b, k]]
    out = torch.full((tokens, H), 3.0, dtype=torch.float16, device="cuda")
    B.moe_combine_pairs(ctx, dev16(torch, down), torch.from_numpy(pairs.reshape(-1).copy()).cuda(), torch.from_numpy(w.reshape(-1).copy()).cuda(),
                        out, tokens, H, K, P)
    ctx.sync()
    assert nmse(ref, host(out)) < NMSE_FP16_TOL
    # weighted_sum_batched: slots [b, k, h]; the offset form reads weights / writes out at element offsets
    ref2 = np.einsum("bk,bkh->bh", w, down.reshape(tokens, K, H)).astype(np.float32)
    out2 = torch.zeros(tokens, H, dtype=torch.float16, device="cuda")
    B.weighted_sum_batched(ctx, dev16(torch, down), torch.from_numpy(w.reshape(-1).copy()).cuda(), out2, tokens, K, H)
    wbig = torch.zeros(16 + P, dtype=torch.float32, device="cuda")
    wbig[16:] = torch.from_numpy(w.reshape(-1).copy()).cuda()
    obig = torch.full((2 * H + tokens * H,), 5.0, dtype=torch.float16, device="cuda")
    B.weighted_sum_batched_offset(ctx, dev16(torch, down), wbig, 16, obig, 2 * H, tokens, K, H)
    ctx.sync()
    assert nmse(ref2, host(out2)) < NMSE_FP16_TOL
    assert torch.equal(obig[2 * H:].reshape(tokens, H), out2) and bool(torch.all(obig[:2 * H] == 5.0))


@pytest.mark.parametrize("tokens,E,K,H,I", [(9, 8, 2, 256, 128), (40, 16, 4, 512, 256), (300, 8, 2, 256, 128)])
def test_gemm_phase_batched_bucketed_dispatch(env, tokens, E, K, H, I):
    """MarlinExpertStack::gemm_phase_batched (marlin_expert_stack.rs:63): per-expert (m × K)·tile[e] over the expert-bucketed
    packed rows of the host plan — the reference's bucketed MoE path (moe/dispatch.rs:1558-2192): gather → gemm1 → silu·mul →
    gemm3 → moe_combine through pairs_by_token — against moe_forward_cpu."""
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(tokens + E + H)
    gu = [O.make_synthetic_gptq(H, 2 * I, 128, 300 + e, symmetric=True) for e in range(E)]
    dn = [O.make_synthetic_gptq(I, H, 128, 400 + e, symmetric=True) for e in range(E)]
    gu = [(q, f16r(s / (0.28 * np.sqrt(H))), z) for q, s, z in gu]
    dn = [(q, f16r(s / (0.28 * np.sqrt(I))), z) for q, s, z in dn]
    x = f16r(rng.standard_normal((tokens, H)))
    rid, rw = O.route_topk(rng.standard_normal((tokens, E)).astype(np.float32), E, K, True)
    gw = np.stack([O.dequant_gptq(q, s, z, 128, H, 2 * I) for q, s, z in gu])
    dw = np.stack([O.dequant_gptq(q, s, z, 128, I, H) for q, s, z in dn])
    ref = O.moe_forward_cpu(x, H, I, K, rid, rw, gw, dw)
    P = tokens * K
    off, packed_idx, pairs = O.bucket_plan(rid, tokens, E, K)
    xp = dev16(torch, x[np.asarray(packed_idx)])                 # the gather step (embedding_lookup of x into x_packed)
    disp = [(e, int(off[e]), int(off[e]), int(off[e + 1] - off[e])) for e in range(E)]
    g_stack = B.load_gptq_stacked([q for q, _, _ in gu], [s for _, s, _ in gu], [z for _, _, z in gu], None, 4, 128, H, 2 * I,
                                  fuse_gate_up=True)
    d_stack = B.load_gptq_stacked([q for q, _, _ in dn], [s for _, s, _ in dn], [z for _, _, z in dn], None, 4, 128, I, H)
    act = torch.zeros(P, I, dtype=torch.float16, device="cuda")
    g_stack.gemm_phase_batched(ctx, xp, disp, act, H, fused_silu_mul=True)
    # the down phase writes each expert's rows 3 rows further down (out_row_offset ≠ in_row_offset)
    down = torch.zeros(P + 3, H, dtype=torch.float16, device="cuda")
    d_stack.gemm_phase_batched(ctx, act, [(e, i, o + 3, m) for e, i, o, m in disp], down, I)
    out = torch.zeros(tokens, H, dtype=torch.float16, device="cuda")
    B.moe_combine_pairs(ctx, down[3:], torch.from_numpy(np.asarray(pairs, np.int32)).cuda(), torch.from_numpy(rw.reshape(-1).copy()).cuda(),
                        out, tokens, H, K, P)
    ctx.sync()
    assert bool(torch.all(down[:3] == 0))
    assert nmse(ref, host(out)) < 3e-6


@pytest.mark.parametrize("nq,nkv,hd,q_len,ctx_len", [(8, 2, 128, 1, 300), (8, 2, 128, 37, 37), (32, 4, 128, 70, 200), (4, 4, 64, 20, 33)])
def test_paged_decode_attention_trait_form(env, nq, nkv, hd, q_len, ctx_len):
    """BackendPagedKv::paged_decode_attention (traits.rs:1719-1738): q_len == 1 over several sequences (token-major), and the
    single-sequence causal prefill whose q / out are HEAD-major [nq, q_len, hd] with context_lens[0] the final kv length."""
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(nq + q_len + ctx_len)
    S = 3 if q_len == 1 else 1
    kv_lens = [ctx_len, 17, 130][:S]
    b = _paged_batch(env, rng, kv_lens, nq, nkv, hd, q_lens=[1] * S if q_len == 1 else [q_len], spare_blocks=2, spare_columns=1)
    tables, K, V, ck, cv, max_blocks = b.tables, b.K, b.V, b.ck, b.cv, b.max_blocks
    lens_d = torch.from_numpy(np.array(kv_lens, np.int32)).cuda()
    if q_len == 1:
        q = b.q
        out = torch.zeros(S, nq, hd, dtype=torch.float16, device="cuda")
        B.paged_decode_attention(ctx, dev16(torch, q), ck, cv, out, torch.from_numpy(tables).cuda(), lens_d, S, nq, nkv, hd, 16, max_blocks, 1)
        ctx.sync()
        got = host(out)
        for s, n in enumerate(kv_lens):
            assert nmse(_ref_attention(O, q[s:s + 1], K[s], V[s], n - 1, nq, nkv, hd), got[s:s + 1]) < 1e-5, s
    else:
        q_tm = b.q                                               # token-major for the reference …
        q_hm = np.ascontiguousarray(q_tm.transpose(1, 0, 2))     # … head-major for the call
        out = torch.zeros(nq, q_len, hd, dtype=torch.float16, device="cuda")
        B.paged_decode_attention(ctx, dev16(torch, q_hm), ck, cv, out, torch.from_numpy(tables).cuda(), lens_d, 1, nq, nkv, hd, 16, max_blocks, q_len)
        ctx.sync()
        ref = _ref_attention(O, q_tm, K[0], V[0], ctx_len - q_len, nq, nkv, hd)
        assert nmse(ref, host(out).transpose(1, 0, 2)) < 1e-5


def test_backend_graph_capture_and_replay(env):
    """BackendGraph (capabilities.rs:35-70): ops enqueued between begin / end capture are recorded, not run; every replay
    runs them on the current buffer contents."""
    pkg, B, ctx, O, torch = env
    rng = np.random.default_rng(9)
    x = f16r(rng.standard_normal((5, 1024)))
    w = f16r(1 + 0.1 * rng.standard_normal(1024))
    xd, wd = dev16(torch, x), dev16(torch, w)
    out = torch.zeros(5, 1024, dtype=torch.float16, device="cuda")
    ctx.sync()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c2 = B.new_context()                                       # capture needs a non-default stream
        B.begin_graph_capture(c2)
        B.rms_norm(c2, xd, wd, 1e-6, out, 5, 1024)
        g = B.end_graph_capture(c2)
        c2.sync()
        assert float(out.abs().max()) == 0.0                       # recorded, not executed
        B.replay_graph(c2, g)
        c2.sync()
        assert nmse(O.rms_norm(x, w, 1e-6), host(out)) < NMSE_FP16_TOL
        x2 = f16r(rng.standard_normal((5, 1024)))
        xd.copy_(dev16(torch, x2))
        c2.sync()
        B.replay_graph(c2, g)
        c2.sync()
        assert nmse(O.rms_norm(x2, w, 1e-6), host(out)) < NMSE_FP16_TOL
        B.reset_graph(c2, g)
