"""Element-wise parity bounds shared by the GPU parity tests (imported like tests/modelgen.py).

A whole-tensor NMSE is an average: on an output of millions of elements one wrong element, one wrong column or one wrong
cache slot disappears in it.  The checks here hold EVERY element (every cache vector) against a float64 reference with a
tolerance that is derived from the number formats, not measured on the code under test:

    |got − ref| ≤ 2^-11·|ref| + (k·2^-23 + [folded]·2^-11)·Σ|x||w| + 2^-24

  * 2^-11·|ref|       one fp16 rounding of the result (round to nearest: half an ulp of an 11-bit significand);
  * k·2^-23·Σ|x||w|   fp32 accumulation of k products in ANY order: each of the ≤ k − 1 additions (and, in forms that scale a
                      group's chain result, one multiply per group) rounds by ≤ 2^-24 of a partial sum that is itself
                      ≤ Σ|x||w|, so (k − 1 + groups)·2^-24 ≤ k·2^-23 to first order.  fp16 × fp16 products are exact in fp32;
  * 2^-11·Σ|x||w|     forms that finish the weight as fp16 before the MFMA ("folded": (q − zero)·scale rounded once per
                      weight) carry one fp16 rounding per weight;
  * 2^-24             the smallest fp16 subnormal: the floor below which the format cannot resolve.

A bias is one more term of the sum (x = 1, w = bias): callers add it to `ref64` and |bias| to `absdot64`.
"""
import numpy as np

EPS_F16 = 2.0 ** -11          # unit roundoff of fp16
EPS_F32_SUM = 2.0 ** -23      # per-term allowance of a worst-case fp32 sum (two roundings of 2^-24 per term)
FLOOR_F16 = 2.0 ** -24        # smallest fp16 subnormal
KV_ROUNDTRIP_NMSE = 3e-3      # the project's fp16 round-trip bucket (op_diff), applied per cache vector
SILU_SLOPE_MAX = 1.1          # max |silu'(g)| (≈ 1.0998 at g ≈ 2.4)


def nmse(ref, got):
    ref, got = np.asarray(ref, np.float64).ravel(), np.asarray(got, np.float64).ravel()
    return float(((ref - got) ** 2).mean() / max((ref ** 2).mean(), 1e-30))


def gemm_refs(x, w, bias=None):
    """float64 reference and magnitude sum of y = x·wᵀ (+ bias): x [m, k], w [n, k] → (ref64, absdot64), each [m, n]."""
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    ref, absdot = x64 @ w64.T, np.abs(x64) @ np.abs(w64).T
    if bias is not None:
        ref, absdot = ref + np.asarray(bias, np.float64)[None, :], absdot + np.abs(np.asarray(bias, np.float64))[None, :]
    return ref, absdot


def sum_tolerance(ref64, absdot64, k, folded):
    """The accumulation part of the bound (everything except the result's own fp16 rounding and the floor)."""
    return (k * EPS_F32_SUM + (EPS_F16 if folded else 0.0)) * np.asarray(absdot64, np.float64)


def gemm_tolerance(ref64, absdot64, k, folded):
    return EPS_F16 * np.abs(np.asarray(ref64, np.float64)) + sum_tolerance(ref64, absdot64, k, folded) + FLOOR_F16


def assert_within(ref64, tol64, got, what=""):
    """Every element of `got` within `tol64` of `ref64` (NaN fails).  The failure names how many elements are outside, the
    worst one's (row, col) and its err/tol."""
    ref64, tol64 = np.asarray(ref64, np.float64), np.asarray(tol64, np.float64)
    got64 = np.asarray(got, np.float64)
    assert got64.shape == ref64.shape, f"{what}: shape {got64.shape} against reference {ref64.shape}"
    err = np.abs(got64 - ref64)
    bad = ~(err <= tol64)                                   # NaN compares false: counted
    if bad.any():
        ratio = np.where(np.isfinite(err), err / tol64, np.inf)
        worst = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the element-wise bound; worst at "
                             f"(row, col) = {tuple(int(i) for i in worst)}: got {got64[worst]!r}, reference {ref64[worst]!r}, "
                             f"err/tol = {float(ratio[worst]):.3g}")
    return float(np.max(err / tol64)) if err.size else 0.0


def assert_gemm_elementwise(ref64, absdot64, got, k, folded, what="gemm"):
    """|got − ref64| ≤ 2^-11·|ref64| + (k·2^-23 + (2^-11 if folded else 0))·absdot64 + 2^-24 for every element (module
    docstring).  ref64 = x @ w.T and absdot64 = |x| @ |w|.T in float64; k the length of the sum.  Returns max err/tol."""
    return assert_within(ref64, gemm_tolerance(ref64, absdot64, k, folded), got, what)


def silu64(g):
    g = np.asarray(g, np.float64)
    return g / (1.0 + np.exp(-g))


def assert_gated_elementwise(g64, u64, absdot_g64, absdot_u64, got, k, folded, what="silu·mul"):
    """act = silu(g)·u computed from fp32 sums g, u that were never stored: for every element

        |got − silu(g)·u| ≤ |silu'(g)|·|u|·tol_g + |silu(g)|·tol_u + 2^-11·|silu(g)·u| + 2^-24

    Derivation: the kernel holds ĝ = g + δg, û = u + δu with |δg| ≤ tol_g, |δu| ≤ tol_u, the accumulation parts of the GEMM
    bound (no fp16 rounding: g and u stay in fp32 registers).  First order, silu(ĝ)·û − silu(g)·u = silu'(g)·u·δg + silu(g)·δu,
    and |silu'| ≤ 1.1 everywhere, so |silu'(g)|·|u|·tol_g ≤ 1.1·|u|·tol_g is used (no need to trust the slope at a perturbed
    point).  The activation itself (exp, divide, multiply in fp32, fast-math exp accurate to a few 2^-23) adds a relative
    error two orders below the 2^-11 rounding of the fp16 store, which is the third term; 2^-24 is the fp16 floor."""
    g64, u64 = np.asarray(g64, np.float64), np.asarray(u64, np.float64)
    ref = silu64(g64) * u64
    tol_g, tol_u = sum_tolerance(g64, absdot_g64, k, folded), sum_tolerance(u64, absdot_u64, k, folded)
    tol = SILU_SLOPE_MAX * np.abs(u64) * tol_g + np.abs(silu64(g64)) * tol_u + EPS_F16 * np.abs(ref) + FLOOR_F16
    return assert_within(ref, tol, got, what)


def assert_combine_elementwise(down, weights, got, tokens, top_k, what="combine"):
    """out[t] = Σ_j weights[t, j]·down[t·top_k + j] from fp16 `down` and fp32 weights: a top_k-term fp32 sum (each product
    rounds once, each addition once: ≤ 2·top_k roundings of 2^-24 of partial sums ≤ Σ|w||down|) and one fp16 rounding:

        |got − ref| ≤ 2^-11·|ref| + top_k·2^-23·Σ_j|w_j||down_j| + 2^-24"""
    d = np.asarray(down, np.float64).reshape(tokens, top_k, -1)
    w = np.asarray(weights, np.float64).reshape(tokens, top_k, 1)
    ref, absdot = (d * w).sum(axis=1), (np.abs(d) * np.abs(w)).sum(axis=1)
    return assert_within(ref, gemm_tolerance(ref, absdot, top_k, False), got, what)


# ── paged KV cache, vector by vector ─────────────────────────────────────────────────────────────────────────────────────
def kv_vector_nmse(ref, got):
    """NMSE of each (position, kv head) vector: [positions, heads, head_dim] → [positions, heads]."""
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    return ((ref - got) ** 2).mean(axis=-1) / np.maximum((ref ** 2).mean(axis=-1), 1e-30)


def kv_vector_maxerr(ref, got):
    """Largest absolute error of each (position, kv head) vector divided by that reference vector's RMS."""
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    return np.abs(ref - got).max(axis=-1) / np.maximum(np.sqrt((ref ** 2).mean(axis=-1)), 1e-30)


def assert_kv_positions(ref, got, positions, limit, metric, what):
    """metric(ref, got) < limit at every listed position and every kv head separately; names the worst (position, head)."""
    m = metric(np.asarray(ref)[positions], np.asarray(got)[positions])
    bad = ~(m < limit)
    if bad.any():
        p, h = np.unravel_index(int(np.argmax(np.where(np.isfinite(m), m, np.inf))), m.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} (position, kv head) vectors outside {limit:g}; worst at "
                             f"position {int(np.asarray(positions)[p])}, head {int(h)}: {float(m[p, h]):.3g}")
    return float(m.max()) if m.size else 0.0


def f16r(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def emulate_layer0_kv(embed_rows, input_ln, w_qkv, k_norm, positions, nq, nkv, hd, eps, theta, qk_norm=True):
    """numpy restatement of layer 0's K/V path of a decode row — input norm → q|k|v product → k-norm → rope — that rounds to
    fp16 exactly where the device stores fp16: the norm output, the q|k|v output, the cache.  embed_rows [T, H] (fp16-valued),
    w_qkv [(nq + 2·nkv)·hd, H] dequantised, positions [T] → (K, V) each [T, nkv, hd].  Sums run in float64 (the device's fp32
    summation order and fast-math exp / rsqrt are NOT modelled: the caller's margin covers them)."""
    x = np.asarray(embed_rows, np.float64)
    inv = 1.0 / np.sqrt((x * x).mean(axis=1, keepdims=True) + eps)
    normed = f16r(x * inv * np.asarray(input_ln, np.float64)[None, :]).astype(np.float64)             # fp16: norm output
    qkv = f16r(normed @ np.asarray(w_qkv, np.float64).T).astype(np.float64)                            # fp16: q|k|v output
    T = x.shape[0]
    k = qkv[:, nq * hd:(nq + nkv) * hd].reshape(T, nkv, hd)
    v = qkv[:, (nq + nkv) * hd:].reshape(T, nkv, hd)
    if qk_norm:
        k = k / np.sqrt((k * k).mean(axis=-1, keepdims=True) + eps) * np.asarray(k_norm, np.float64)[None, None, :]
    half = hd // 2
    freq = 1.0 / np.power(float(theta), 2.0 * np.arange(half) / hd)
    ang = np.asarray(positions, np.float64)[:, None] * freq[None, :]
    c, s = np.cos(ang).astype(np.float32).astype(np.float64)[:, None, :], np.sin(ang).astype(np.float32).astype(np.float64)[:, None, :]
    k0, k1 = k[..., :half], k[..., half:]
    kr = np.concatenate([k0 * c - k1 * s, k1 * c + k0 * s], axis=-1)
    return f16r(kr), f16r(v)                                                                           # fp16: the cache
