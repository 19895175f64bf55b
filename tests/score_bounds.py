"""The element-wise bound of the scoring head (csrc/score_head.hip), derived from the arithmetic, not measured.

The op restated in float64 for one row x of n fp32 logits: M = max x, d_i = M − x_i, e_i = exp(−d_i), S = Σ e_i,
lse = M + log S, logprob_t = x_t − lse.  The kernel cuts the row into P = ⌈n / 4096⌉ segments, takes m_p and
s_p = Σ exp(x_i − m_p) per segment in fp32 and merges S = Σ_p s_p·exp(m_p − M).  With u = 2^-24:

  one term      x_i − m_p is one fp32 subtraction (relative u, so absolute (m_p − x_i)·u in the exponent, which the exponential
                turns into a relative error of the term), expf adds U_exp; the merge factor exp(m_p − M) the same with
                (M − m_p)·u — together d_i·u + U_exp, first term below — and one more U_exp + 2u for the factor's own expf and
                the product, which is absent where the row is one segment (m_p = M: the factor is exp(0) = 1 exactly);
  the sums      the formula allows (n + P + 2)·u relative to S, the worst case of adding n terms and P partials one after the
                other.  The kernel adds at most 16 terms per lane, then a 6-level wave tree, 3 waves, and the merge ⌈P / 64⌉
                terms per lane and 6 levels: ≤ 32 roundings whatever n.  For n > 4096 the difference, (n − 30)·u, is far more
                than the U_exp + 2u left over above, so the formula covers the two-level form;
  the logarithm logf: U_log relative to |log S|; the relative error of S enters log S one to one (first order);
  the last add  M + log S rounds to fp32: u·|lse|; x_t − lse likewise: u·|x_t − lse|.

  tol_lse     = Σ e_i·(d_i·u + U_exp)/S + (n + P + 2)·u + U_log·|log S| + u·|lse|
  tol_logprob = tol_lse + u·|x_t − lse|

ASSUMPTION: U_exp = U_log = 4 ulp = 4·2^-23.  The HIP math API documents expf and logf at 1 ulp; that could not be confirmed
where this was written, so 4 ulp is a stated cap — the bound only has to discriminate, and a wrong row, token or segment is
orders of magnitude outside it.

Special rows: −inf entries have e = 0; a row with nothing above −inf has lse = −inf and NaN log-probs; a row with a NaN has
NaN lse and log-probs; a token ≥ n gives −inf.  The references carry these as they are, with a tolerance of 0, and
assert_within asks for the same NaN or infinity there.

Checked on the CPU (tests/test_score_bounds.py) with an fp32 numpy emulation in sequential, segment-then-merge and pairwise-
tree order on the inputs of tests/test_score_gpu.py: largest honest err/tol 0.40 (lse), 0.48 (log-probs); planted errors on
the 33 × 8195 input: a dropped segment ≥ 880, a seam element counted twice ≥ 824; a target read from the neighbouring row:
smallest 353, 4.2e3 at the lowest tenth of the pairs; from the neighbouring column: smallest 7.8, 1.3e3 at the lowest tenth
(over the pairs whose wrong logit differs from the right one at all)."""
import numpy as np

U = 2.0 ** -24
U_EXP = 4 * 2.0 ** -23
U_LOG = 4 * 2.0 ** -23
SEGMENT = 4096            # SCORE_SEGMENT of csrc/score_plan.h (tests/test_score_gpu.py checks the two agree)


def row_ref_tol(x):
    """x [m, n] fp32-valued → (lse64 [m], tol_lse [m], top [m]).  top is the first maximum (0 for a row with none)."""
    x = np.asarray(x, np.float64)
    m, n = x.shape
    P = -(-n // SEGMENT)
    lse, tol, top = np.empty(m), np.zeros(m), np.zeros(m, np.int64)
    for r in range(m):
        row = x[r]
        if np.isnan(row).any():
            lse[r] = np.nan
            continue
        M = row.max()
        if M == -np.inf:
            lse[r] = -np.inf
            continue
        top[r] = int(np.argmax(row))          # (numpy's argmax is the first maximum)
        d = M - row
        e = np.exp(-d)
        S = e.sum()
        lse[r] = M + np.log(S)
        terms = np.where(e > 0, e * (np.where(e > 0, d, 0.0) * U + U_EXP), 0.0).sum() / S
        tol[r] = terms + (n + P + 2) * U + U_LOG * abs(np.log(S)) + U * abs(lse[r])
    return lse, tol, top


def pair_ref_tol(x, lse, tol_lse, pair_rows, pair_tokens):
    """(ref64 [pairs], tol [pairs]) of the gathered log-probs."""
    x = np.asarray(x, np.float64)
    n = x.shape[1]
    ref, tol = np.empty(len(pair_rows)), np.zeros(len(pair_rows))
    for p, (r, t) in enumerate(zip(pair_rows, pair_tokens)):
        if t >= n:
            ref[p] = -np.inf
            continue
        with np.errstate(invalid="ignore"):
            ref[p] = x[r, t] - lse[r]                 # −inf − (−inf) = NaN: the row has no distribution
        if np.isfinite(ref[p]):
            tol[p] = tol_lse[r] + U * abs(ref[p])
    return ref, tol


def assert_within(ref, tol, got, what):
    """Finite references within the bound; NaN where the reference is NaN, the same infinity where it is infinite.  Returns the
    largest err/tol over the finite ones."""
    ref, tol, got = np.asarray(ref, np.float64), np.asarray(tol, np.float64), np.asarray(got, np.float64)
    assert ref.shape == got.shape, (what, ref.shape, got.shape)
    fin = np.isfinite(ref)
    assert (np.isnan(got) == np.isnan(ref)).all(), f"{what}: NaN where the reference has none, or none where it has one: {np.flatnonzero(np.isnan(got) != np.isnan(ref))[:8]}"
    inf = np.isinf(ref)
    assert (got[inf] == ref[inf]).all(), f"{what}: an infinite reference is not matched"
    err = np.abs(got[fin] - ref[fin])
    bad = ~(err <= tol[fin])
    if bad.any():
        k = int(np.argmax(np.where(np.isfinite(err), err / tol[fin], np.inf)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} outside the bound; worst is finite element {k}: got {got[fin][k]!r}, "
                             f"reference {ref[fin][k]!r}, err/tol = {err[k] / tol[fin][k]:.3g}")
    return float(np.max(err / tol[fin])) if err.size else 0.0
