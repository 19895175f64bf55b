"""The element-wise bound of the embedding tail (csrc/embed_pool.hip), derived from the arithmetic, not measured.

The op restated in float64: final norm of every row → pool over a span → cut to the leading d components → L2.  With
A(k) = parity_bounds.norm_scale_allowance(k), the relative error of x·inv·w held in fp32 (any summation order):

  normed row     |δn_t| ≤ A(H)·|n_t| — kept in fp32, no fp16 store; A = 0 without a norm weight (n_t = x_t exactly);
  pooled v       last / first: tol_v = A(H)·|v|;
                 mean of L rows: tol_v = (A(H) + L·2^-23 + 2^-24)·S with S = (1/L)·Σ_t |n_t| — an fp32 sum of L terms in any
                 order ((L − 1)·2^-24 relative to Σ|n_t|, doubled for the rounding of the partials' own sums) plus the divide;
  without L2     tol = tol_v + 2^-149;
  with L2        r = ‖v[:d]‖₂, q = ‖tol_v[:d]‖₂ / r, out = v / r.  The computed norm is within r·(q + A(d)) of r to first
                 order (the vector moves by at most ‖tol_v‖; the sum of d squares, the square root and the divide are
                 A(d)), so tol = tol_v/r·(1 + q) + |out|·(q + q² + A(d)) + 2^-149.  The first-order step needs q small: the
                 helper asserts q ≤ 2^-6.  r == 0: the reference is exact zeros (v / max(r, 1e-12)), tolerance 2^-149.

Checked on the CPU with an fp32 numpy emulation in sequential and in tree order on the inputs of
test_embed_gpu.test_embed_pool_elementwise: max err/tol 0.056, largest q 1.4e-3; one dropped token of a 65-token mean gives
err/tol ≈ 350."""
import numpy as np

from tests import parity_bounds as pb


def l2_ref_tol(v, tv):
    """L2 step alone: v float64 [d] with element-wise tolerance tv → (out, tol)."""
    d = v.shape[0]
    r = np.sqrt((v * v).sum())
    if r == 0:
        return v * 0, np.full(d, 2.0 ** -149)
    q = np.sqrt((tv * tv).sum()) / r
    assert q <= 2.0 ** -6, q
    out = v / max(r, 1e-12)
    return out, tv / r * (1 + q) + np.abs(out) * (q + q * q + pb.norm_scale_allowance(d)) + 2.0 ** -149


def ref_tol(x, w, eps, spans, pooling, normalize, dims):
    """x [rows, H] (fp16- or fp32-valued), w [H] or None, spans [(begin, end)] → (ref64, tol64), each [len(spans), dims or H]."""
    H = x.shape[1]
    d = dims or H
    n = pb.rms_norm_ref64(x, w, eps)[0] if w is not None else np.asarray(x, np.float64)
    A = pb.norm_scale_allowance(H) if w is not None else 0.0
    refs, tols = [], []
    for b, e in spans:
        rows = n[b:e]
        L = len(rows)
        if pooling == 0:
            v, S, extra = rows[-1], np.abs(rows[-1]), 0.0
        elif pooling == 2:
            v, S, extra = rows[0], np.abs(rows[0]), 0.0
        else:
            v, S, extra = rows.mean(0), np.abs(rows).mean(0), L * 2.0 ** -23 + 2.0 ** -24
        v, tv = v[:d], ((A + extra) * S)[:d]
        if not normalize:
            refs.append(v)
            tols.append(tv + 2.0 ** -149)
            continue
        out, tol = l2_ref_tol(v, tv)
        refs.append(out)
        tols.append(tol)
    return np.stack(refs), np.stack(tols)
