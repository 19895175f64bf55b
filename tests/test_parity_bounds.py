"""CPU self-test of tests/parity_bounds.py: a clean fp16 GEMM emulation (fp16 inputs, float32 matmul, fp16 store) passes the
element-wise bound, four single faults a kernel can make are flagged — and on the many-row shape two of them stay below the
whole-tensor NMSE bucket (1e-6) the suite used alone, which is why the element-wise bound exists.  The second half does the
same for the norm family's bounds (row norm, sandwich update, slab inputs, gated activations, layer_norm)."""
import numpy as np
import pytest

from tests import parity_bounds as pb

NMSE_FP16_TOL = 1e-6
GROUP = 128


def _case(oracle, k, n, m):
    qw, sc, qz = oracle.make_synthetic_gptq(k, n, GROUP, k * 7 + n, symmetric=False)
    sc = pb.f16r(sc / (0.28 * np.sqrt(k)))                      # scales travel as fp16, as in the GPU tests
    w = oracle.dequant_gptq(qw, sc, qz, GROUP, k, n)            # (q − zero)·scale: exact in f32
    x = pb.f16r(np.random.default_rng(m).standard_normal((m, k)))
    return x, w, sc.reshape(k // GROUP, n)


def _emulate(x, w, folded):
    wd = pb.f16r(w) if folded else w                            # folded forms round each weight to fp16 once
    return (x.astype(np.float32) @ wd.astype(np.float32).T).astype(np.float16).astype(np.float32)


def _scale_step_columns(sc):
    """(the column whose last two groups' scales differ most, the column with the largest last-group scale, the first column
    whose last two scales differ by only 5–15 %).  The third is the subtle version of 'took the neighbour's scale'.  The bound is
    a worst case: at k = 8192 its term k·2^-23 = 2^-10 of Σ|x||w| is wider than a 10 % step in one of 64 groups, so every shape
    is checked with the columns where the fault is largest and the many-row shape with the subtle column as well."""
    step = np.abs(sc[-2] - sc[-1])
    rel = step / sc[-1]
    subtle = np.nonzero((rel > 0.05) & (rel < 0.15))[0]
    assert subtle.size, "no column with a 5-15 % scale step between its last two groups"
    return int(np.argmax(step)), int(np.argmax(sc[-1])), int(subtle[0])


@pytest.mark.parametrize("folded", [False, True])
@pytest.mark.parametrize("k,n,m", [(2048, 640, 200), (8192, 2048, 32), (1024, 4096, 2100)])
def test_elementwise_bound_passes_clean_emulation_and_flags_single_faults(oracle, k, n, m, folded):
    x, w, sc = _case(oracle, k, n, m)
    ref, absdot = pb.gemm_refs(x, w)
    clean = _emulate(x, w, folded)
    worst = pb.assert_gemm_elementwise(ref, absdot, clean, k, folded, "clean emulation")
    assert worst < 0.5, worst                                   # worst-case bound against random-walk error: far inside
    assert pb.nmse(ref, clean) < NMSE_FP16_TOL
    last = slice(k - GROUP, k)
    col, col_drop, subtle = _scale_step_columns(sc)

    def column_fault(c, w_col):
        out = clean.copy()
        out[:, c] = _emulate(x, w_col[None, :], folded)[:, 0]
        return out

    def neighbours_scale(c):                                     # last group dequantised with the previous group's scale
        w_col = w[c].copy()
        w_col[last] = (w[c, last].astype(np.float64) * (float(sc[-2, c]) / float(sc[-1, c]))).astype(np.float32)
        return column_fault(c, w_col)

    zeroed = clean.copy()
    zeroed[m // 3, n // 5] = 0.0
    frag = clean.copy()                                          # one 16-column fragment of the last row from its neighbour
    frag[m - 1, 32:48] = clean[m - 1, 48:64]
    w_drop = w[col_drop].copy()
    w_drop[last] = 0.0
    faults = {"element zeroed": zeroed, "fragment from neighbour": frag, "neighbouring group's scale": neighbours_scale(col),
              "last group dropped": column_fault(col_drop, w_drop)}
    if (k, n, m) == (1024, 4096, 2100):
        faults["neighbouring group's scale, 5-15 % apart"] = neighbours_scale(subtle)
    for name, out in faults.items():
        with pytest.raises(AssertionError, match="outside the element-wise bound"):
            pb.assert_gemm_elementwise(ref, absdot, out, k, folded, name)
    if (k, n, m) == (1024, 4096, 2100):
        # the reason for the helper: the whole-tensor NMSE assert passes these two
        assert pb.nmse(ref, faults["element zeroed"]) < NMSE_FP16_TOL
        assert pb.nmse(ref, faults["neighbouring group's scale, 5-15 % apart"]) < NMSE_FP16_TOL


def test_elementwise_bound_reports_count_worst_position_and_ratio():
    ref = np.ones((3, 4))
    got = ref.copy()
    got[2, 1] = 1.5
    got[0, 0] = float("nan")
    with pytest.raises(AssertionError) as e:
        pb.assert_gemm_elementwise(ref, np.ones((3, 4)), got, 128, False, "demo")
    msg = str(e.value)
    assert "2 of 12 elements" in msg and "(row, col) = (0, 0)" in msg and "err/tol" in msg      # NaN is the worst
    got[0, 0] = 1.0
    with pytest.raises(AssertionError, match=r"1 of 12 elements.*\(row, col\) = \(2, 1\)"):
        pb.assert_gemm_elementwise(ref, np.ones((3, 4)), got, 128, False, "demo")


def test_gated_and_combine_bounds_pass_clean_emulation_and_flag_one_element(oracle):
    k, inter, m, top_k = 512, 256, 24, 4
    x, w, _ = _case(oracle, k, 2 * inter, m)
    g, ag = pb.gemm_refs(x, w[:inter])
    u, au = pb.gemm_refs(x, w[inter:])
    g32, u32 = x @ w[:inter].T, x @ w[inter:].T                 # fp32 sums, never stored as fp16
    act = pb.f16r(g32 / (1.0 + np.exp(-g32)) * u32)
    assert pb.assert_gated_elementwise(g, u, ag, au, act, k, False) < 0.5
    bad = act.copy()
    bad[5, 7] = act[5, 8]
    with pytest.raises(AssertionError, match=r"\(row, col\) = \(5, 7\)"):
        pb.assert_gated_elementwise(g, u, ag, au, bad, k, False)
    down = pb.f16r(np.random.default_rng(1).standard_normal((m, inter)))
    wts = np.random.default_rng(2).random((m // top_k, top_k)).astype(np.float32)
    out = pb.f16r((down.reshape(-1, top_k, inter) * wts[:, :, None]).sum(axis=1, dtype=np.float32))
    assert pb.assert_combine_elementwise(down, wts, out, m // top_k, top_k) <= 1.0
    out[1, 3] = 0.0
    with pytest.raises(AssertionError, match=r"\(row, col\) = \(1, 3\)"):
        pb.assert_combine_elementwise(down, wts, out, m // top_k, top_k)


def test_per_vector_kv_checks_see_a_shifted_row_that_the_sequence_nmse_hides():
    rng = np.random.default_rng(3)
    ref = rng.standard_normal((400, 4, 128)).astype(np.float32)
    got = pb.f16r(ref)
    pos = np.arange(400)
    assert pb.assert_kv_positions(ref, got, pos, pb.KV_ROUNDTRIP_NMSE, pb.kv_vector_nmse, "clean") < 1e-6
    got2 = got.copy()
    got2[399, 2] = got2[398, 2]                                  # one kv head of one position
    assert pb.nmse(ref, got2) < pb.KV_ROUNDTRIP_NMSE             # passes the whole-sequence assert
    with pytest.raises(AssertionError, match="position 399, head 2"):
        pb.assert_kv_positions(ref, got2, pos, pb.KV_ROUNDTRIP_NMSE, pb.kv_vector_nmse, "shifted")
    with pytest.raises(AssertionError, match="position 399, head 2"):
        pb.assert_kv_positions(ref, got2, pos, 0.05, pb.kv_vector_maxerr, "shifted")


# ── norm family ──────────────────────────────────────────────────────────────────────────────────────────────────────────
def _row_ss32(x):
    """Per-vector fp32 sums of squares [rows, nvec] and their total taken from the last vector to the first (float64
    sums pairwise from the front: a different order)."""
    x32 = np.asarray(x, np.float32)
    ssv = (x32 * x32).reshape(x32.shape[0], -1, 8).sum(axis=-1, dtype=np.float32)
    total = np.zeros(x32.shape[0], np.float32)
    for v in range(ssv.shape[1] - 1, -1, -1):
        total = total + ssv[:, v]
    return ssv, total


def _emu_rms(x, w, eps, total=None, store16=True):
    """numpy float32 restatement of the row norm; `total` replaces the row sums (fault injection)."""
    x32, w32 = np.asarray(x, np.float32), np.asarray(w, np.float32)
    if total is None:
        total = _row_ss32(x)[1]
    inv = (np.float32(1.0) / np.sqrt(total / np.float32(x32.shape[1]) + np.float32(eps))).astype(np.float32)
    y = x32 * inv[:, None] * w32
    return y.astype(np.float16).astype(np.float32) if store16 else y


def _flagged(fn):
    with pytest.raises(AssertionError, match="outside the element-wise bound"):
        fn()


def _two_ulps(out, r, c):
    bad = out.copy()
    h = bad[r, c].astype(np.float16)
    bad[r, c] = np.float32(np.nextafter(np.nextafter(h, np.float16(np.inf)), np.float16(np.inf)))
    return bad


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("dim", [248, 2056, 4104, 8184, 8192, 16384])
def test_row_norm_bound_passes_clean_emulation_and_flags_each_fault(dim, eps):
    """Rows of every kind (tests/parity_bounds.norm_rows) at 65 rows; 8192 carries the widest any-order allowance a
    sandwich kernel can meet, 8184 is the widest row of the 1024-thread form that still has an inactive lane."""
    rng = np.random.default_rng(dim)
    rows, nvec = 65, dim // 8
    x, kinds = pb.norm_rows(rng, rows, dim)
    w = pb.mixed_sign_weight(rng, dim)
    clean = _emu_rms(x, w, eps)
    assert pb.assert_rms_norm_elementwise(x, w, eps, clean, "clean emulation") <= 1.0
    assert np.all(clean[kinds.index("zero")] == 0.0)
    ref, _ = pb.rms_norm_ref64(x, w, eps)
    assert pb.nmse(ref, clean) < NMSE_FP16_TOL
    ssv, total = _row_ss32(x)
    faults = {}
    r, c = kinds.index("normal"), int(np.argmax(np.abs(clean[0]) > 0.5))
    faults["one element off by two fp16 ulps"] = _two_ulps(clean, r, c)
    sub = kinds.index("subnormal")                               # the eps-dominated row: a vector an earlier clear left at 0
    stale = clean.copy()
    stale[sub, -8:] = 0.0
    faults["stale last vector"] = stale
    nb = clean.copy()
    nb[9] = clean[8]
    faults["neighbouring row gathered"] = nb
    faults["last vector left out of the row sum"] = _emu_rms(x, w, eps, total - ssv[:, -1])
    if nvec > 256:
        faults["chunk-seam vector counted twice"] = _emu_rms(x, w, eps, total + ssv[:, 256])
    if nvec < 1024:
        faults["inactive lanes add vector 0"] = _emu_rms(x, w, eps, total + np.float32(1024 - nvec) * ssv[:, 0])
    for name, out in faults.items():
        _flagged(lambda: pb.assert_rms_norm_elementwise(x, w, eps, out, name))
    # the whole-tensor average passes the first two on this very data (the second once a row has a few hundred vectors)
    assert pb.nmse(ref, faults["one element off by two fp16 ulps"]) < NMSE_FP16_TOL
    if dim >= 2056:
        assert pb.nmse(ref, faults["stale last vector"]) < NMSE_FP16_TOL
    # fused-add residual and the scaled embedding copies are held bit-exact: one fp16 rounding of an exact fp32 value
    r16 = pb.f16r(3 * rng.standard_normal((rows, dim)))
    assert np.array_equal(pb.f16r(r16.astype(np.float64) + x.astype(np.float64)), pb.f16r(r16 + x))


@pytest.mark.parametrize("S", [0, 3, 9])
@pytest.mark.parametrize("dim", [248, 4104, 8192])
def test_sandwich_bounds_pass_clean_emulation_and_flag_each_fault(dim, S):
    """residual += rms_norm(branch)·w_branch in fp32, norm_out = fp16(rms_norm(residual)·w_next); S > 0: the branch
    arrives as S fp32 slabs and is fp16(Σ slabs) by sequential float32 adds."""
    rng = np.random.default_rng(dim + S)
    rows, eps, nvec = 65, 1e-6, dim // 8
    target, kinds = pb.norm_rows(rng, rows, dim, start=1)
    if S:
        slabs = pb.split_into_slabs(rng, target, S)
        branch = pb.slabs_to_f16(slabs)
        assert np.all(np.isfinite(branch)) and np.all(branch[kinds.index("zero")] == 0.0)
        assert np.max(np.abs(branch - target)) <= 2.0 ** -10 * np.max(np.abs(target))
    else:
        branch = target
    wb, wn = pb.mixed_sign_weight(rng, dim), pb.mixed_sign_weight(rng, dim)
    r0 = (3 * rng.standard_normal((rows, dim))).astype(np.float32)

    def emu(total=None, w_first=wb):
        res = (r0 + _emu_rms(branch, w_first, eps, total, store16=False)).astype(np.float32)
        return res, _emu_rms(res, wn, eps)

    res, out = emu()
    assert pb.assert_sandwich_residual(branch, wb, r0, eps, res, "clean residual") <= 1.0
    assert pb.assert_rms_norm_elementwise(res, wn, eps, out, "clean norm_out") <= 1.0
    ssv, total = _row_ss32(branch)
    faulty = {"w_next where w_branch belongs": emu(w_first=wn)[0],
              "last vector left out of the row sum": emu(total - ssv[:, -1])[0]}
    if nvec > 256:
        faulty["chunk-seam vector counted twice"] = emu(total + ssv[:, 256])[0]
    if nvec < 1024:
        faulty["inactive lanes add vector 0"] = emu(total + np.float32(1024 - nvec) * ssv[:, 0])[0]
    nb = res.copy()
    nb[5] = res[4]
    faulty["neighbouring row"] = nb
    for name, bad in faulty.items():
        _flagged(lambda: pb.assert_sandwich_residual(branch, wb, r0, eps, bad, name))
    # norm_out is judged from the residual the device returned: a wrong second row sum or a stale vector shows there
    ssv2, total2 = _row_ss32(res)
    big2 = int(np.argmax(ssv2.max(axis=1) / total2))             # the row whose energy is most concentrated
    _flagged(lambda: pb.assert_rms_norm_elementwise(res, wn, eps, _emu_rms(res, wn, eps, total2 - ssv2[:, int(np.argmax(ssv2[big2]))]), "second sum"))
    _flagged(lambda: pb.assert_rms_norm_elementwise(res, wn, eps, _two_ulps(out, 0, int(np.argmax(np.abs(out[0]) > 0.5))), "two ulps"))
    if S:                                                        # a slab left out, or summed twice, is a different fp16 branch
        assert not np.array_equal(pb.slabs_to_f16(slabs[:-1]), branch)


@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("rows,im", [(3, 8), (3, 2056), (2, 4100)])
def test_gated_activation_bounds_pass_plain_float32_and_flag_faults(rows, im, gelu):
    gu = pb.gated_inputs(np.random.default_rng(im), rows, im)
    g, u = gu[:, :im].astype(np.float32), gu[:, im:].astype(np.float32)
    for v in pb.GATE_PLANTS:
        assert (g == v).any()
    with np.errstate(over="ignore"):
        if gelu:
            a = np.float32(0.5) * g * (np.float32(1.0) + np.tanh(np.float32(0.79788456) * (g + np.float32(0.044715) * g * g * g)))
        else:
            a = g / (np.float32(1.0) + np.exp(-g))
        with np.errstate(under="ignore"):
            clean = (a * u).astype(np.float16).astype(np.float32)
    assert clean.dtype == np.float32 and a.dtype == np.float32
    assert pb.assert_gated_act_elementwise(gu, clean, gelu) <= 1.0
    ref = (pb.gelu_tanh_mul_ref64 if gelu else pb.silu_mul_ref64)(g, u)
    r, c = np.unravel_index(int(np.argmax(np.abs(clean) > 0.5)), clean.shape)
    _flagged(lambda: pb.assert_gated_act_elementwise(gu, _two_ulps(clean, r, c), gelu))
    stale = clean.copy()
    stale[-1, -8:] = clean[0, -8:]
    _flagged(lambda: pb.assert_gated_act_elementwise(gu, stale, gelu))
    nb = clean.copy()
    nb[1] = clean[0]
    _flagged(lambda: pb.assert_gated_act_elementwise(gu, nb, gelu))
    if gelu:
        # the absolute term: at g = −4 an absolute 2^-24 in the bracket is about three fp16 ulps of the result, yet the
        # bound stays within a few ulps there (a term that swallowed the result would hide a wrong element)
        g4, u4 = np.float64(-4.0), np.float64(3.0)
        r4 = pb.gelu_tanh_mul_ref64(g4, u4)
        t4 = pb.gelu_tanh_mul_tolerance(r4, g4, u4)
        assert 0.5 * 4 * 3 * 2.0 ** -24 > 2 * 2.0 ** -11 * abs(r4) and t4 < 0.02 * abs(r4)
    assert ref.shape == clean.shape


def test_layer_norm_and_gelu_bounds_pass_float32_emulation_and_flag_faults():
    rng = np.random.default_rng(4100)
    rows, dim = 3, 4100
    x = pb.f16r(rng.standard_normal((rows, dim)) * 3 + 0.7)
    gam, beta = pb.mixed_sign_weight(rng, dim), pb.f16r(0.1 * rng.standard_normal(dim))
    x32 = x.astype(np.float32)
    mean = (x32[:, ::-1].sum(axis=1, dtype=np.float32) / np.float32(dim))[:, None]
    d = x32 - mean
    inv = np.float32(1.0) / np.sqrt((d * d).sum(axis=1, dtype=np.float32)[:, None] / np.float32(dim) + np.float32(1e-5))
    clean = pb.f16r(d * inv * gam + beta)
    ref, tol = pb.layer_norm_ref_tol(x, gam, beta, 1e-5)
    assert pb.assert_within(ref, tol, clean, "clean layer_norm") <= 1.0
    stale = clean.copy()
    stale[2, -8:] = clean[1, -8:]
    _flagged(lambda: pb.assert_within(ref, tol, stale, "stale"))
    nb = clean.copy()
    nb[1] = clean[0]
    _flagged(lambda: pb.assert_within(ref, tol, nb, "row"))
    shifted = pb.f16r((d + np.float32(0.01)) * inv * gam + beta)             # a mean that is off by 0.3 % of the spread
    _flagged(lambda: pb.assert_within(ref, tol, shifted, "mean"))
    with pytest.raises(AssertionError, match="offset exceeds"):
        pb.layer_norm_ref_tol(x + 100.0, gam, beta, 1e-5)
    # erf-form gelu through the GELU bound with u = 1
    xs = pb.f16r(np.concatenate([3 * rng.standard_normal(4096), [-4.0, -6.0, 12.0, -12.0]]))
    z = xs / np.float32(np.sqrt(2.0))
    t = np.float32(1.0) / (np.float32(1.0) + np.float32(0.3275911) * np.abs(z))
    y = np.float32(1.0) - (((((np.float32(1.0614054) * t - np.float32(1.4531521)) * t) + np.float32(1.4214138)) * t - np.float32(0.28449672)) * t + np.float32(0.2548296)) * t * np.exp(-z * z)
    got = pb.f16r(np.float32(0.5) * xs * (np.float32(1.0) + np.where(z < 0, np.float32(-1.0), np.float32(1.0)) * y))
    gref = pb.gelu_erf_poly_ref64(xs)
    gtol = pb.gelu_tanh_mul_tolerance(gref, xs)
    assert pb.assert_within(gref, gtol, got, "clean gelu") <= 1.0
    _flagged(lambda: pb.assert_within(gref, gtol, _two_ulps(got[None], 0, int(np.argmax(got > 0.5)))[0], "two ulps"))


# ── decode-regime dense forms: the unfolded INT4 chain, fp32 slabs, the fused tail, the fp16 GEMMs ───────────────────────
DECODE_KS = (128, 256, 384, 512, 640, 1024, 2048, 8192)          # every K of tests/test_dense_decode_gpu.py's INT4 cases


def _q_case(oracle, k, n, m, symmetric):
    """_case with the integer operands the kernel sees: (x, w, q [n, k], scales [G, n], zero [G, n])."""
    qw, sc, qz = oracle.make_synthetic_gptq(k, n, GROUP, k * 7 + n, symmetric=symmetric)
    sc = pb.f16r(sc / (0.28 * np.sqrt(k)))
    w = oracle.dequant_gptq(qw, sc, qz, GROUP, k, n)
    q, zero = pb.unpack_gptq(qw, qz, k, n)
    scg = sc.reshape(k // GROUP, n)
    assert np.array_equal(((q - np.repeat(zero, GROUP, axis=0).T) * np.repeat(scg, GROUP, axis=0).T).astype(np.float32), w)
    if symmetric:
        assert np.all(zero == 8)
    x = pb.f16r(np.random.default_rng(m + k).standard_normal((m, k)))
    return x, w, q, scg, zero


def _flagged_at(fn, rows, cols):
    """The bound flags the fault and the element it names lies in the faulted footprint."""
    import re
    with pytest.raises(AssertionError, match="outside the element-wise bound") as e:
        fn()
    r, c = (int(v) for v in re.search(r"\(row, col\) = \((\d+), (\d+)\)", str(e.value)).groups())
    assert r in rows and c in cols, (r, c, str(e.value))


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("k", DECODE_KS)
def test_unfolded_chain_emulations_against_the_bound(oracle, k, symmetric):
    """The MFMA-shaped restatement of w4_consume_group (one fp32 rounding per 32-term k-step, offset chain first, per-wave
    slices summed in wave order) passes the existing bound at every K the GPU cases use — fp16 store and fp32 slabs alike.
    The fully sequential restatement (one rounding per term) is the stated worst-case model: its max err/tol is printed and
    recorded in DESIGN.md, not asserted below 1."""
    m, n, G = 16, 64, k // GROUP
    x, w, q, sc, zero = _q_case(oracle, k, n, m, symmetric)
    ref, absdot = pb.gemm_refs(x, w)
    W = min(4, G)
    parts = pb.w4_chain_parts(x, q, sc, zero, pb.even_slices(G, W), not symmetric)
    mfma = pb.assert_gemm_elementwise(ref, absdot, pb.sum_parts(parts), k, False, f"MFMA-shaped chain, K={k}")
    slabs = pb.assert_gemm_elementwise(ref, absdot, parts.astype(np.float64).sum(axis=0), k, False, f"slab sum, K={k}", out_f32=True)
    seq = pb.w4_chain_parts(x, q, sc, zero, [(0, G)], not symmetric, sequential=True)
    ratio = float(np.max(np.abs(pb.sum_parts(seq) - ref) / pb.gemm_tolerance(ref, absdot, k, False)))
    ratio32 = float(np.max(np.abs(seq[0].astype(np.float64) - ref) / pb.gemm_tolerance(ref, absdot, k, False, out_f32=True)))
    print(f"K={k} {'symmetric' if symmetric else 'zero points'}: max err/tol, fp16 store | fp32 kept: MFMA-shaped {mfma:.3f} | {slabs:.3f}, "
          f"fully sequential {ratio:.3f} | {ratio32:.3f}")
    assert np.isfinite(ratio) and ratio > 0.0 and np.isfinite(ratio32)


def test_decode_form_faults_are_flagged_and_two_hide_from_the_whole_tensor_average(oracle):
    """Eight single faults of the decode-regime kernels, injected into the clean MFMA-shaped restatement with the footprint
    the kernel would give them (one workgroup's rows × one 16-column tile or one column): each is flagged and the element
    named lies in the footprint.  Two of them — the neighbouring group's scale and the neighbouring column's zero point, 16
    rows of one column of a 63 × 4096 output — stay under the whole-tensor NMSE of 1e-6 on the same data."""
    k, n, m = 1024, 4096, 63
    G = k // GROUP
    x, w, q, sc, zero = _q_case(oracle, k, n, m, symmetric=False)
    bias = pb.f16r(np.random.default_rng(5).standard_normal(n))
    ref, absdot = pb.gemm_refs(x, w)
    ref_b, absdot_b = pb.gemm_refs(x, w, bias)
    slices = pb.even_slices(G, 8)
    parts = pb.w4_chain_parts(x, q, sc, zero, slices, True)
    clean = pb.sum_parts(parts)
    assert pb.assert_gemm_elementwise(ref, absdot, clean, k, False, "clean") <= 1.0
    assert pb.assert_gemm_elementwise(ref_b, absdot_b, pb.sum_parts(parts, bias), k, False, "clean + bias") <= 1.0
    slab_sum = lambda ps: np.asarray(ps, np.float64).sum(axis=0)
    assert pb.assert_gemm_elementwise(ref, absdot, slab_sum(parts), k, False, "clean slabs", out_f32=True) <= 1.0
    rows, cols = range(16, 32), range(48, 64)                    # row block 1 of a 16-row launch, one 16-column tile
    rs, cs = slice(16, 32), slice(48, 64)
    every_row, every_col = range(m), range(n)

    def patched(values, r=rs, c=cs):
        out = clean.copy()
        out[r, c] = values[r, c]
        return out

    check = lambda got, name: pb.assert_gemm_elementwise(ref, absdot, got, k, False, name)
    _flagged_at(lambda: check(patched(pb.sum_parts(np.delete(parts, 3, axis=0))), "wave 3's K slice missing"), rows, cols)
    _flagged_at(lambda: pb.assert_gemm_elementwise(ref, absdot, slab_sum(parts[:-1]), k, False, "slab dropped", out_f32=True), every_row, every_col)
    _flagged_at(lambda: pb.assert_gemm_elementwise(ref, absdot, slab_sum(list(parts) + [parts[2]]), k, False, "slab twice", out_f32=True),
                every_row, every_col)
    _flagged_at(lambda: pb.assert_gemm_elementwise(ref_b, absdot_b, pb.sum_parts(parts, bias, 2), k, False, "bias twice"), every_row, every_col)
    clamped = clean.copy()
    clamped[m - 2, cs] = clean[m - 1, cs]
    _flagged_at(lambda: check(clamped, "row M-2 computed from the clamped row M-1"), [m - 2], cols)

    def column(c, sc_c, zero_c):                                 # rows 16..31 of column c recomputed with the given scales / zeros
        out = clean.copy()
        out[rs, c] = pb.sum_parts(pb.w4_chain_parts(x[rs], q[c:c + 1], sc_c[:, None], zero_c[:, None], slices, True))[:, 0]
        return out

    _, _, subtle = _scale_step_columns(sc)
    sc_bad = sc[:, subtle].copy()
    sc_bad[-1] = sc[-2, subtle]
    scale_fault = column(subtle, sc_bad, zero[:, subtle])
    _flagged_at(lambda: check(scale_fault, "neighbouring group's scale"), rows, [subtle])
    zc = int(np.argmax(zero[3, :-1] != zero[3, 1:]))
    zero_bad = zero[:, zc].copy()
    zero_bad[3] = zero[3, zc + 1]
    assert zero_bad[3] != zero[3, zc]
    zero_fault = column(zc, sc[:, zc], zero_bad)
    _flagged_at(lambda: check(zero_fault, "neighbouring column's zero point"), rows, [zc])
    # what the whole-tensor assert the suite had makes of the last two
    assert pb.nmse(ref, scale_fault) < NMSE_FP16_TOL and pb.nmse(ref, zero_fault) < NMSE_FP16_TOL
    assert pb.nmse(ref, clean) < NMSE_FP16_TOL

    # fp16 GEMM, K = 1120: 35 k-steps in S = 4 slices of 8, 9, 9, 9 — three slices end in the remainder loop
    rng = np.random.default_rng(1120)
    xf, wf = pb.f16r(rng.standard_normal((17, 1120))), pb.f16r(rng.standard_normal((96, 1120)) / np.sqrt(1120))
    rf, af = pb.gemm_refs(xf, wf)
    for f32 in (False, True):
        good = pb.sum_parts(pb.f16_gemm_parts(xf, wf, 4), store16=not f32)
        assert pb.assert_gemm_elementwise(rf, af, good, 1120, False, "fp16 GEMM", out_f32=f32) <= 1.0
        bad = pb.sum_parts(pb.f16_gemm_parts(xf, wf, 4, skip_remainder=True), store16=not f32)
        _flagged_at(lambda: pb.assert_gemm_elementwise(rf, af, bad, 1120, False, "remainder k-steps skipped", out_f32=f32), range(17), range(96))
    # the f32-out bound is the tighter one: an fp32 result that is off by one fp16 ulp (2^-10 relative) fails it
    ulp = good.copy()
    r0, c0 = np.unravel_index(int(np.argmax(np.abs(rf))), rf.shape)
    ulp[r0, c0] *= 1.0 + 2.0 ** -10
    _flagged_at(lambda: pb.assert_gemm_elementwise(rf, af, ulp, 1120, False, "fp32 result off by 2^-10", out_f32=True), [r0], [c0])


@pytest.mark.parametrize("top_k", [1, 2, 8, 9])
@pytest.mark.parametrize("k,symmetric", [(512, True), (2048, False)])
def test_fused_tail_bounds_pass_float32_emulation_and_flag_faults(oracle, k, symmetric, top_k):
    """The fused combine + add + norm prologue in float32 as the kernel computes it (Σ_j w_j·down_j in j order, fp16(r + c),
    the row sum of squares, x̂ = fp16(r'·inv·ln)), then the MFMA-shaped chain on x̂."""
    m, n, eps, G = 4, 64, 1e-6, k // GROUP
    _, w, q, sc, zero = _q_case(oracle, k, n, m, symmetric)
    rng = np.random.default_rng(k + top_k)
    down = pb.f16r(rng.standard_normal((m * top_k, k)))
    wts = rng.random((m, top_k)).astype(np.float32) + np.float32(0.1)
    wts = (wts / wts.sum(axis=1, keepdims=True)).astype(np.float32)
    r_in = 2 * rng.standard_normal((m, k))
    r_in[0, -8:] = 30.0 * rng.choice([-1.0, 1.0], 8)            # row 0: most of the energy in the last vector (pb.norm_rows, "last")
    r_in = pb.f16r(r_in)
    ln = pb.mixed_sign_weight(rng, k)
    c32 = np.zeros((m, k), np.float32)
    for j in range(top_k):
        c32 = c32 + wts[:, j:j + 1] * down.reshape(m, top_k, k)[:, j].astype(np.float32)
    res = pb.f16r(r_in.astype(np.float32) + c32)
    ref_r, tol_r = pb.fused_tail_residual_ref_tol(down, wts, r_in, m, top_k)
    assert pb.assert_within(ref_r, tol_r, res, "clean residual_out") <= 1.0
    _flagged(lambda: pb.assert_within(ref_r, tol_r, _two_ulps(res, 1, int(np.argmax(np.abs(res[1]) > 0.5))), "two ulps"))
    if top_k > 1:                                                # the last expert row left out
        short = pb.f16r(r_in.astype(np.float32) + c32 - wts[:, -1:] * down.reshape(m, top_k, k)[:, -1].astype(np.float32))
        _flagged(lambda: pb.assert_within(ref_r, tol_r, short, "last expert row missing"))

    def gemm(total=None, rows=res):
        xh = _emu_rms(rows, ln, eps, total)                      # fp16(r'·inv·ln) in float32
        return pb.sum_parts(pb.w4_chain_parts(xh, q, sc, zero, pb.even_slices(G, 4), not symmetric))

    ref, tol = pb.fused_tail_gemm_ref_tol(res, ln, eps, w)
    assert pb.assert_within(ref, tol, gemm(), "clean fused-tail GEMM") <= 1.0
    ssv, total = _row_ss32(res)
    _flagged(lambda: pb.assert_within(ref, tol, gemm(total - ssv[:, -1]), "last vector left out of the row sum"))
    _flagged(lambda: pb.assert_within(ref, tol, gemm(np.roll(total, 1)), "the previous row's sum of squares"))
    _flagged(lambda: pb.assert_within(ref, tol, gemm(rows=r_in), "GEMM on residual_in"))


# ── decode attention of the chain: bound, restatement, planted contexts, injected faults ─────────────────────────────────
def _attn_case(kv_len, window, splits, G, seed=0, spare=3):
    rng = np.random.default_rng(seed * 100003 + kv_len * 31 + window * 7 + splits)
    q = pb.f16r(1.5 * rng.standard_normal((G, 128)))
    k_new, v_new = pb.f16r(rng.standard_normal(128)), pb.f16r(rng.standard_normal(128))
    ctx = pb.plant_context(rng, q, k_new, kv_len, window, splits, pb._cdiv(kv_len, 16) + spare)
    K, V = pb.effective_kv(ctx, k_new, v_new, kv_len)
    ref, tol, w = pb.decode_attn_ref_tol(q, K, V, ctx["allowed"], kv_len, window, splits)
    return dict(q=q, k_new=k_new, v_new=v_new, ctx=ctx, K=K, V=V, ref=ref, tol=tol, w=w, kv_len=kv_len, window=window, splits=splits)


def _emulate_attn(c, fault=None, fault_range=0):
    return pb.chain_attn_emulate(c["q"], c["ctx"]["K"], c["ctx"]["V"], c["k_new"], c["v_new"], c["kv_len"], c["window"], c["splits"],
                                 fault=fault, fault_range=fault_range)


def _attn_flagged(c, out):
    with np.errstate(invalid="ignore"):
        return bool((~(np.abs(out.astype(np.float64) - c["ref"]) <= c["tol"])).any())


@pytest.mark.parametrize("name", sorted(pb.ATTN_CASES))
def test_attention_restatement_is_inside_the_bound_and_planted_keys_weigh_2_to_20_percent(name):
    """At every context of the GPU module's cases: the float32 / fp16 restatement of chain_role_attn lies inside the bound; on
    the float64 reference alone every planted key carries 2–20 % of the mass of the row it was planted for, and every poisoned
    position would carry more than 50 % of every row if it were counted."""
    nkv, splits, window, contexts = pb.ATTN_CASES[name]
    G = 32 // nkv
    worst, planted = 0.0, 0
    for kv_len in contexts:
        c = _attn_case(kv_len, window, splits, G)
        ctx = c["ctx"]
        for p, h in zip(ctx["edges"], ctx["heads"]):
            assert pb.PLANT_MASS[0] <= c["w"][h, p] <= pb.PLANT_MASS[1], (name, kv_len, p, h, c["w"][h, p])
            planted += 1
        assert not set(ctx["edges"]) & set(ctx["poison"]) and not c["w"][:, [p for p in ctx["poison"] if p != kv_len - 1]].any()
        s_all = pb.ATTN_SCALE * (c["q"].astype(np.float64) @ c["K"][ctx["allowed"]].T)
        logZ = np.logaddexp.reduce(s_all, axis=1)
        for p in ctx["poison"]:
            s_p = pb.ATTN_SCALE * (c["q"].astype(np.float64) @ ctx["K"][p])
            assert np.all(s_p > logZ), (name, kv_len, p)                    # e^s_p / (Z + e^s_p) > 1/2 on every row
            assert np.all(np.abs(ctx["V"][p]) == pb.POISON_V)
        out = _emulate_attn(c)
        ratio = float((np.abs(out.astype(np.float64) - c["ref"]) / c["tol"]).max())
        assert ratio < 1.0, (name, kv_len, ratio)
        worst = max(worst, ratio)
    assert planted or window == 1                             # (a window of one key holds the new token alone: nothing to plant)
    print(f"attention restatement {name}: largest err/tol {worst:.3f}")


ATTN_FAULT_CASES = [
    # (fault, kv_len, window, splits, G, ranges the fault is applied to)
    ("drop_last_key_of_range", 300, 0, 5, 8, (0, 1, 2, 3)),
    ("drop_last_key_of_range", 2064, 0, 5, 8, (0, 3)),
    ("drop_last_key_of_range", 257, 150, 16, 2, (2, 5)),           # six pairs over 16 ranges: ranges 2, 5, 7, 10, 13, 15 hold one each
    ("first_key_of_next_range_twice", 300, 0, 5, 8, (0, 1, 2, 3)),
    ("first_key_of_next_range_twice", 2064, 0, 16, 4, (0, 14)),
    ("win_lo_one_low", 257, 150, 1, 8, (0,)),
    ("win_lo_one_low", 18, 17, 1, 8, (0,)),
    ("win_lo_one_low", 2, 1, 1, 8, (0,)),
    ("win_lo_one_low", 300, 150, 5, 4, (0,)),
    ("win_lo_one_high", 257, 150, 1, 8, (0,)),
    ("win_lo_one_high", 17, 16, 5, 8, (0,)),
    ("win_lo_one_high", 300, 150, 16, 2, (0,)),
    ("slot_past_kv_len", 250, 0, 1, 8, (0,)),
    ("slot_past_kv_len", 17, 0, 5, 4, (0,)),
    ("slot_past_kv_len", 1, 0, 1, 8, (0,)),
    ("slot_past_kv_len", 2064, 0, 5, 8, (0,)),
    ("absent_second_block", 33, 0, 1, 8, (0,)),
    ("absent_second_block", 257, 0, 5, 8, (0,)),
    ("absent_second_block", 2064, 0, 1, 2, (0,)),
    ("absent_second_block", 1, 0, 1, 8, (0,)),
    ("new_token_from_pool", 1, 0, 1, 8, (0,)),
    ("new_token_from_pool", 16, 0, 1, 8, (0,)),
    ("new_token_from_pool", 300, 0, 5, 4, (0,)),
    ("new_token_from_pool", 1040, 0, 1, 8, (0,)),
    ("range_left_out", 300, 0, 5, 8, (0, 1, 2, 3, 4)),
    ("range_left_out", 2064, 0, 16, 2, (0, 9, 15)),
    ("range_left_out", 33, 0, 5, 8, (4,)),                    # two pairs over five ranges: only ranges 2 and 4 hold one
    ("stale_m", 300, 0, 5, 8, (1, 2, 3, 4)),
    ("stale_m", 2064, 0, 5, 4, (1, 4)),
    ("neighbour_q", 300, 0, 1, 8, (0,)),
    ("neighbour_q", 16, 0, 5, 4, (0,)),
    ("neighbour_q", 129, 0, 16, 2, (0,)),
    ("window_not_reloaded", 1040, 0, 1, 8, (0,)),
    ("window_not_reloaded", 2064, 0, 1, 8, (0,)),
]


@pytest.mark.parametrize("fault,kv_len,window,splits,G,ranges", ATTN_FAULT_CASES, ids=[f"{c[0]}-{c[1]}-w{c[2]}-s{c[3]}-g{c[4]}" for c in ATTN_FAULT_CASES])
def test_attention_bound_flags_every_injected_fault(fault, kv_len, window, splits, G, ranges):
    """Each fault, applied to the clean restatement with the footprint the kernel would give it, leaves an element of the
    affected rows (the G rows of the kv head) outside the bound.  No fault may go unflagged."""
    c = _attn_case(kv_len, window, splits, G, seed=1)
    assert not _attn_flagged(c, _emulate_attn(c))
    for r in ranges:
        assert _attn_flagged(c, _emulate_attn(c, fault, r)), (fault, kv_len, window, splits, G, r)


def test_every_attention_fault_has_a_case():
    assert {c[0] for c in ATTN_FAULT_CASES} == set(pb.ATTN_FAULTS)


# ── routing without logits ───────────────────────────────────────────────────────────────────────────────────────────────
def _routing(E=60, Q=4, K=4, T=6, H=256, seed=3):
    rng = np.random.default_rng(seed)
    x, w = pb.f16r(rng.standard_normal((T, H))), pb.f16r(rng.standard_normal((E, H)) / np.sqrt(H))
    w[17], w[33] = w[2], w[2]                                                  # a tied group across parts
    L, tol = pb.route_logits_ref_tol(x, w)
    l32 = (x.astype(np.float32) @ w.astype(np.float32).T)
    l32[:, 17], l32[:, 33] = l32[:, 2], l32[:, 2]
    order = np.lexsort((np.arange(E)[None, :].repeat(T, 0), -l32), axis=1)
    ids = order[:, :K]
    p = np.exp(l32.astype(np.float64) - l32.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    wts = np.take_along_axis(p, ids, 1)
    EQ = pb._cdiv(E, 16) // Q * 16
    cl, ci, st = np.full((T, Q, 8), -np.inf, np.float32), np.full((T, Q, 8), 0x7fffffff, np.int64), np.zeros((T, Q, 2), np.float32)
    for t in range(T):
        for q in range(Q):
            own = np.arange(q * EQ, min(E, (q + 1) * EQ))
            o = own[np.lexsort((own, -l32[t, own]))][:K]
            ci[t, q, :len(o)], cl[t, q, :len(o)] = o, l32[t, o]
            st[t, q] = l32[t, own].max(), np.exp(l32[t, own] - l32[t, own].max()).sum()
    return dict(L=L, tol=tol, ids=ids, wts=wts / wts.sum(axis=1, keepdims=True), cl=cl, ci=ci, st=st, Q=Q, K=K, l32=l32)


def test_routing_checks_pass_a_clean_router_and_flag_its_faults():
    r = _routing()
    pb.assert_route_selection(r["L"], r["tol"], r["ids"], r["wts"], True)
    pb.assert_route_ties(r["ids"], [[2, 17, 33]])
    pb.assert_route_lists(r["L"], r["tol"], r["cl"], r["ci"], r["st"], r["Q"], r["K"])
    T, E = r["L"].shape
    worst = np.argsort(r["l32"][0])[0]

    def bad(fn, **kw):
        with pytest.raises(AssertionError):
            fn(**kw)
    ids = r["ids"].copy(); ids[0, -1] = worst                                  # a far-worse expert chosen
    bad(lambda: pb.assert_route_selection(r["L"], r["tol"], ids, r["wts"], True))
    ids = r["ids"].copy(); ids[0, [0, -1]] = ids[0, [-1, 0]]                   # ranks swapped
    bad(lambda: pb.assert_route_selection(r["L"], r["tol"], ids, r["wts"][:, ::-1] if False else r["wts"], True))
    w = r["wts"].copy(); w[1, 0] *= 1.001                                      # one combine weight off by 0.1 %
    bad(lambda: pb.assert_route_selection(r["L"], r["tol"], r["ids"], w, True))
    bad(lambda: pb.assert_route_selection(r["L"], r["tol"], r["ids"], r["wts"], False))      # renormalised where it should not be
    bad(lambda: pb.assert_route_ties(np.array([[17, 2, 5, 6]]), [[2, 17, 33]]))             # higher id first
    bad(lambda: pb.assert_route_ties(np.array([[2, 33, 5, 6]]), [[2, 17, 33]]))             # a lower id skipped
    assert pb.assert_route_ties(np.array([[5, 2, 17, 6]]), [[2, 17, 33]]) == 1              # the boundary cuts the group: counted
    for name, mutate in {
        "order": lambda cl, ci, st: (cl.__setitem__((0, 0, [0, 1]), cl[0, 0, [1, 0]]), ci.__setitem__((0, 0, [0, 1]), ci[0, 0, [1, 0]])),
        "value": lambda cl, ci, st: cl.__setitem__((0, 1, 2), cl[0, 1, 2] * np.float32(1.01)),
        "coverage": lambda cl, ci, st: (ci.__setitem__((0, 0, 3), np.argsort(r["l32"][0, :16])[0]), cl.__setitem__((0, 0, 3), np.sort(r["l32"][0, :16])[0])),
        "unused": lambda cl, ci, st: ci.__setitem__((0, 0, 5), 3),
        "max": lambda cl, ci, st: st.__setitem__((0, 2, 0), np.nextafter(st[0, 2, 0], np.float32(9))),
        "sumexp": lambda cl, ci, st: st.__setitem__((0, 3, 1), st[0, 3, 1] * np.float32(1.001)),
    }.items():
        cl, ci, st = r["cl"].copy(), r["ci"].copy(), r["st"].copy()
        mutate(cl, ci, st)
        with pytest.raises(AssertionError):
            pb.assert_route_lists(r["L"], r["tol"], cl, ci, st, r["Q"], r["K"])
            pytest.fail(name)
