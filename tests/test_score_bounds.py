"""tests/score_bounds.py on the CPU: an fp32 numpy emulation of the scoring head with the sum taken sequentially, segment by
segment and merged, and as a pairwise tree stays inside the derived bound on the very inputs of tests/test_score_gpu.py, and
each planted error — a dropped segment, a seam element counted twice, a target read from the neighbouring row, a target one
column off — is far outside it."""
import numpy as np
import pytest

from tests import score_bounds as sb
from tests import test_score_gpu as tg

F = np.float32


def _tree32(a):
    a = np.asarray(a, F)
    while len(a) > 1:
        if len(a) % 2:
            a = np.concatenate([a, np.zeros(1, F)])
        a = a[0::2] + a[1::2]
    return a[0] if len(a) else F(0)


def _seq32(a):
    a = np.asarray(a, F)
    return np.cumsum(a, dtype=F)[-1] if len(a) else F(0)


def _exp32(d):
    """exp of fp32 differences, −inf − (−inf) taken as "contributes 0" like the kernel's test for −inf."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.isneginf(d) | np.isnan(d), F(0), np.exp(d.astype(F), dtype=F)).astype(F)


def emulate_lse(row, order, drop_segment=None, twice=None):
    """fp32 log-sum-exp of one row.  order: "sequential", "tree" (one maximum, one sum) or "segments" (per-segment maximum and
    sum, merged in segment order).  drop_segment / twice plant the errors."""
    row = np.asarray(row, F)
    if order in ("sequential", "tree"):
        M = row.max()
        if M == -np.inf:
            return F(-np.inf)
        e = _exp32(row - M)
        S = _seq32(e) if order == "sequential" else _tree32(e)
        with np.errstate(divide="ignore"):
            return F(M + np.log(S, dtype=F))
    parts = []
    for p, lo in enumerate(range(0, len(row), sb.SEGMENT)):
        if p == drop_segment:
            continue
        seg = row[lo:lo + sb.SEGMENT]
        m = seg.max()
        e = _exp32(seg - m) if m > -np.inf else np.zeros(len(seg), F)
        s = _tree32(e)
        if twice is not None and lo <= twice < lo + sb.SEGMENT:
            s = F(s + e[twice - lo])
        parts.append((m, s))
    M = max(m for m, _ in parts)
    if M == -np.inf:
        return F(-np.inf)
    S = F(0)
    for m, s in parts:
        S = F(S + (F(s * np.exp(F(m - M), dtype=F)) if m > -np.inf else s))
    return F(M + np.log(S, dtype=F))


def _emulated_pairs(x, lse, pr, pt, row_shift=0, col_shift=0):
    m, n = x.shape
    out = np.empty(len(pr), F)
    for p, (r, t) in enumerate(zip(pr, pt)):
        with np.errstate(invalid="ignore"):
            out[p] = F(-np.inf) if t >= n else F(x[(r + row_shift) % m, (t + col_shift) % n] - lse[r])
    return out


SHAPES = [(m, n) for m, n, _ in tg.OP_SHAPES]


def test_fp32_emulation_is_inside_the_bound():
    worst_lse = worst_lp = 0.0
    for m, n in sorted(set(SHAPES)):
        x, kinds, pr, pt = tg.op_inputs(m, n)
        lse_ref, tol_lse, top, ref, tol = tg.op_reference(m, n)
        for order in ("sequential", "segments", "tree"):
            lse = np.array([emulate_lse(x[r], order) for r in range(m)], F)
            worst_lse = max(worst_lse, sb.assert_within(lse_ref, tol_lse, lse, f"emulated lse {m}x{n} {order}"))
            worst_lp = max(worst_lp, sb.assert_within(ref, tol, _emulated_pairs(x, lse, pr, pt), f"emulated log-probs {m}x{n} {order}"))
        for r, kind in enumerate(kinds):
            if kind == "seam":
                assert top[r] == tg.seam_columns(n)[0]
    print(f"largest honest err/tol: lse {worst_lse:.3f}, log-probs {worst_lp:.3f}")
    assert worst_lse < 1.0 and worst_lp < 1.0


def test_the_bound_sees_every_planted_error():
    m, n = 33, 2 * sb.SEGMENT + 3
    x, kinds, pr, pt = tg.op_inputs(m, n)
    lse_ref, tol_lse, _, ref, tol = tg.op_reference(m, n)
    honest = np.array([emulate_lse(x[r], "segments") for r in range(m)], F)
    # a dropped segment, on the rows whose mass is spread over the segments
    normal = [r for r, k in enumerate(kinds) if k in ("normal", "third_inf", "equal")]
    dropped = min(abs(float(emulate_lse(x[r], "segments", drop_segment=p)) - lse_ref[r]) / tol_lse[r] for r in normal for p in (0, 1))
    # a seam element counted twice, on the rows that hold their maximum on the seam
    seam = [r for r, k in enumerate(kinds) if k == "seam"]
    twice = min(abs(float(emulate_lse(x[r], "segments", twice=c)) - lse_ref[r]) / tol_lse[r] for r in seam for c in tg.seam_columns(n))
    # a target read from the neighbouring row / the neighbouring column: every pair whose wrong logit differs from the right one
    # (the all-equal rows, two −inf entries and the twin seam maxima coincide: reading the wrong one of those changes nothing)
    # must be outside the bound, and all but a tenth of them far outside
    def planted(**kw):
        wrong = _emulated_pairs(x, honest, pr, pt, **kw)
        right = _emulated_pairs(x, honest, pr, pt)
        differ = np.isfinite(ref) & np.isfinite(wrong) & (wrong != right)
        assert differ.sum() >= 20
        ratio = np.abs(wrong[differ].astype(np.float64) - ref[differ]) / tol[differ]
        return float(ratio.min()), float(np.quantile(ratio, 0.1))
    row_min, row = planted(row_shift=1)
    col_min, col = planted(col_shift=1)
    print(f"planted err/tol: dropped segment {dropped:.3g}, seam element twice {twice:.3g}, neighbouring row {row:.3g} (smallest {row_min:.3g}), "
          f"neighbouring column {col:.3g} (smallest {col_min:.3g})")
    assert min(dropped, twice, row, col) > 100.0 and min(row_min, col_min) > 1.0
    for kw in (dict(row_shift=1), dict(col_shift=1)):
        with pytest.raises(AssertionError):
            sb.assert_within(ref, tol, _emulated_pairs(x, honest, pr, pt, **kw), "planted")
    bad = honest.copy()
    bad[normal[0]] = emulate_lse(x[normal[0]], "segments", drop_segment=1)
    with pytest.raises(AssertionError):
        sb.assert_within(lse_ref, tol_lse, bad, "planted")
    # a NaN that a maximum dropped must not pass as a number
    bad = honest.copy().astype(np.float64)
    ref_nan = lse_ref.copy()
    ref_nan[0] = np.nan
    with pytest.raises(AssertionError):
        sb.assert_within(ref_nan, tol_lse, bad, "dropped NaN")
