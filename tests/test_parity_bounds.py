"""CPU self-test of tests/parity_bounds.py: a clean fp16 GEMM emulation (fp16 inputs, float32 matmul, fp16 store) passes the
element-wise bound, four single faults a kernel can make are flagged — and on the many-row shape two of them stay below the
whole-tensor NMSE bucket (1e-6) the suite used alone, which is why the element-wise bound exists."""
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
