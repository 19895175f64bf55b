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

The row norms, the fp32 residual stream's sandwich update, the gated activations and layer_norm have bounds of their own
further down ("norm family"), derived the same way; each function's docstring carries its derivation.
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


def gemm_tolerance(ref64, absdot64, k, folded, out_f32=False):
    """out_f32: the result is kept as fp32 (split-K slabs, f32-out GEMMs) — its own rounding is 2^-24·|ref| and there is no
    fp16 floor (2^-149, the fp32 subnormal, stands in so that an all-zero row has a tolerance).  The float64 sum of S slabs
    is held by the same bound with the FULL k: slab s carries k_s·2^-23·Σ_s|x||w| of its own part and Σ_s k_s·Σ_s ≤ k·Σ."""
    if out_f32:
        return 2.0 ** -24 * np.abs(np.asarray(ref64, np.float64)) + sum_tolerance(ref64, absdot64, k, folded) + 2.0 ** -149
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


def assert_gemm_elementwise(ref64, absdot64, got, k, folded, what="gemm", out_f32=False):
    """|got − ref64| ≤ 2^-11·|ref64| + (k·2^-23 + (2^-11 if folded else 0))·absdot64 + 2^-24 for every element (module
    docstring; out_f32: gemm_tolerance).  ref64 = x @ w.T and absdot64 = |x| @ |w|.T in float64; k the length of the sum.
    Returns max err/tol."""
    return assert_within(ref64, gemm_tolerance(ref64, absdot64, k, folded, out_f32), got, what)


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


def fused_tail_residual_ref_tol(down, weights, residual_in, tokens, top_k):
    """residual_out = fp16(residual_in + Σ_j w_j·down_j) of the fused combine + add + norm prologue → (ref64, tol64):

        tol = [2^-11·|c| + top_k·2^-23·Σ_j|w_j||down_j| + 2^-24] + 2^-11·|r + c|,   c = Σ_j w_j·down_j

    the combine bound (assert_combine_elementwise) plus one fp16 rounding of the add.  The kernel keeps c in fp32 and rounds
    r + c once to fp32 and once to fp16; the combine bound's own 2^-11·|c| (a rounding this kernel does not make) covers the
    fp32 add's 2^-24·|r + c| wherever |c| ≥ 2^-13·|r + c|, and the 2^-24 floor below that."""
    d = np.asarray(down, np.float64).reshape(tokens, top_k, -1)
    w = np.asarray(weights, np.float64).reshape(tokens, top_k, 1)
    c, absdot = (d * w).sum(axis=1), (np.abs(d) * np.abs(w)).sum(axis=1)
    ref = np.asarray(residual_in, np.float64) + c
    return ref, gemm_tolerance(c, absdot, top_k, False) + EPS_F16 * np.abs(ref)


def fused_tail_gemm_ref_tol(residual_out, ln_w, eps, w, bias=None):
    """out = fp16(x·Wᵀ) of the fused prologue's GEMM, whose input row x is never stored → (ref64, tol64).  The reference is
    built from the DEVICE's residual_out: x = res·rsqrt(mean(res²) + eps)·ln in float64, ref = x·Wᵀ, and

        tol = 2^-11·|ref| + k·2^-23·Σ|x||w| + 2^-24  +  (2^-11 + k·2^-25 + 8·2^-24)·Σ|x||w|

    The first three terms are the unfolded GEMM bound on the exact x.  The kernel's x̂ differs from x element by element by
    its fp32 norm arithmetic — a relative k·2^-25 + 8·2^-24 (norm_scale_allowance: the row sum of k squares in any order,
    /k, +eps, sqrt, divide, two multiplies) — and by the one fp16 rounding of the LDS store, 2^-11: |x̂_i − x_i| ≤
    (2^-11 + k·2^-25 + 8·2^-24)·|x_i| to first order, so the product moves by at most that times Σ|x||w|."""
    res = np.asarray(residual_out, np.float64)
    k = res.shape[-1]
    x, _ = rms_norm_ref64(res, ln_w, eps)
    ref, absdot = gemm_refs(x, w, bias)
    return ref, gemm_tolerance(ref, absdot, k, False) + (EPS_F16 + norm_scale_allowance(k)) * absdot


# ── the unfolded INT4 chain (csrc/w4_device.h, w4_consume_group) and the fp16 GEMMs, restated in float32 ─────────────────
# The bound's accumulation term k·2^-23·Σ|x||w| is derived from "every partial sum ≤ Σ|x||w|".  That does not hold for the
# unfolded INT4 kernels: a group's chain starts at −1032·S_lo − 72·S_hi (−1024 / −64 with zero points) and adds (1024 + q)·x
# and (64 + q)·x, so its partial sums are of order 1039·Σ|x| — two orders above Σ|(q − z)·x| — and only the group's END value
# is small.  The restatements below measure what that costs: `w4_chain_emulate(..., sequential=False)` rounds where the
# kernel's instruction sequence rounds IF one v_mfma_f32_16x16x32_f16 adds its 32 exact products to the accumulator with a
# single fp32 rounding (an assumption about the hardware nobody here has measured); sequential=True rounds after every
# single term, the stated worst-case model.  tests/test_parity_bounds.py runs both at every K the GPU cases use.
GROUP = 128


def unpack_gptq(qweight, qzeros, k, n, group=GROUP):
    """AutoGPTQ packing → (q [n, k] in 0..15, zero [k/group, n] in 1..16): W[n, k] = (q − zero[k // group, n])·scale."""
    qw = np.asarray(qweight, np.int64) & 0xFFFFFFFF
    q = np.stack([(qw >> (4 * j)) & 15 for j in range(8)], axis=1).reshape(k, n)                 # row 8·i + j
    qz = np.asarray(qzeros, np.int64) & 0xFFFFFFFF
    z = np.stack([(qz >> (4 * j)) & 15 for j in range(8)], axis=2).reshape(k // group, n)        # column 8·i + j
    return np.ascontiguousarray(q.T), z + 1


def _fl32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def w4_chain_parts(x, q, sc, zero, slices, has_zp, sequential=False):
    """fp32 accumulators of each K slice: x [m, k] fp16-valued, q [n, k], sc / zero [G, n], slices = [(g0, g1), …] in
    groups → [len(slices), m, n] float32.  Per group (w4_consume_group): t = the offset chain over the four 32-term k-steps
    (B = −1032 | −72 | −1032 | −72 without zero points, −1024 | −64 | … with), then (1024 + q)·x on k-steps 0 and 2 and
    (64 + q)·x on 1 and 3, each k-step's exact sum added with ONE fp32 rounding (sequential: one per term); with zero points
    Σx is a chain of its own and v = fma(−zero, Σx, t); acc = fma(scale, v, acc).  float64 holds every exact intermediate
    (24-bit × 24-bit products, 32-term sums of 22-bit products)."""
    x, q = np.asarray(x, np.float64), np.asarray(q, np.float64)
    sc, zero = np.asarray(sc, np.float64), np.asarray(zero, np.float64)
    m, n = x.shape[0], q.shape[0]
    lo_off, hi_off = (-1024.0, -64.0) if has_zp else (-1032.0, -72.0)

    def chain(t, xs, bs):
        """t ← fl32(t + Σ xs·bs) per k-step (bs [n, 32] or a scalar), or per term."""
        if np.isscalar(bs):
            if not sequential:
                return _fl32(t + (xs.sum(axis=1) * bs)[:, None])
            for i in range(xs.shape[1]):
                t = _fl32(t + (xs[:, i] * bs)[:, None])
            return t
        if not sequential:
            return _fl32(t + xs @ bs.T)
        for i in range(xs.shape[1]):
            t = _fl32(t + np.outer(xs[:, i], bs[:, i]))
        return t

    parts = np.zeros((len(slices), m, n))
    for p, (g0, g1) in enumerate(slices):
        acc = np.zeros((m, n))
        for g in range(g0, g1):
            steps = [slice(g * GROUP + 32 * s, g * GROUP + 32 * s + 32) for s in range(4)]
            t = np.zeros((m, 1))
            for s in range(4):
                t = chain(t, x[:, steps[s]], lo_off if s % 2 == 0 else hi_off)
            t = np.broadcast_to(t, (m, n)).copy()
            if has_zp:
                u = np.zeros((m, 1))
                for s in range(4):
                    u = chain(u, x[:, steps[s]], 1.0)
            # the kernel runs k-steps 0, 1 of every tile, then 2, 3: per accumulator the order is 0, 1, 2, 3
            for s in range(4):
                t = chain(t, x[:, steps[s]], q[:, steps[s]] + (1024.0 if s % 2 == 0 else 64.0))
            v = _fl32(-zero[g][None, :] * u + t) if has_zp else t
            acc = _fl32(sc[g][None, :] * v + acc)
        parts[p] = acc
    return parts.astype(np.float32)


def even_slices(G, W):
    """The K slices [G·w/W, G·(w + 1)/W) of the W waves of a workgroup (or of the S slabs of a split-K grid)."""
    return [(G * w // W, G * (w + 1) // W) for w in range(W)]


def sum_parts(parts, bias=None, bias_times=1, store16=True):
    """Σ parts in order from 0 in float32 (+ bias, `bias_times` times: fault injection), then the fp16 store."""
    acc = np.zeros(np.asarray(parts).shape[1:], np.float32)
    for p in parts:
        acc = acc + np.asarray(p, np.float32)
    for _ in range(bias_times if bias is not None else 0):
        acc = acc + np.asarray(bias, np.float32)[None, :]
    return acc.astype(np.float16).astype(np.float32) if store16 else acc


def f16_gemm_parts(x, w, S, skip_remainder=False):
    """The fp16 GEMM kernels' split-K: k-steps of 32 in S slices [ks·z/S, ks·(z + 1)/S), each k-step's exact sum added with one
    fp32 rounding → [S, m, n] float32.  skip_remainder: the k-steps a slice has beyond a multiple of 4 (the kernels' remainder
    loop after the 4-unrolled main loop) are left out — the fault."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    ks = x.shape[1] // 32
    parts = np.zeros((S, x.shape[0], w.shape[0]))
    for z in range(S):
        s0, s1 = ks * z // S, ks * (z + 1) // S
        if skip_remainder:
            s1 = s0 + (s1 - s0) // 4 * 4
        for s in range(s0, s1):
            parts[z] = _fl32(parts[z] + x[:, 32 * s:32 * s + 32] @ w[:, 32 * s:32 * s + 32].T)
    return parts.astype(np.float32)


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


# ── norm family (csrc/norm.hip): row norms, sandwich update, gated activations, layer_norm ──────────────────────────────
EPS_F32 = 2.0 ** -24          # unit roundoff of fp32
FLOOR_F32 = 2.0 ** -149       # smallest fp32 subnormal
ROW_KINDS = ("normal", "first", "last", "big", "subnormal", "zero", "v255", "v256")


def mixed_sign_weight(rng, dim):
    """fp16 norm weight 1 + 0.3·N(0, 1) with a quarter of the signs flipped."""
    return f16r((1.0 + 0.3 * rng.standard_normal(dim)) * np.where(rng.random(dim) < 0.25, -1.0, 1.0))


def norm_rows(rng, rows, dim, start=0):
    """fp16-valued [rows, dim] test rows, kind of row i = ROW_KINDS[(start + i) % 8]:
      normal     N(0, 1);
      first / last / v255 / v256
                 N(0, 1) with ONE 8-element vector at ±30·(1 ± 5 %): about half of the row's energy at dim 8192, nearly
                 all of it at small dims.  A row sum that drops, repeats or adds such a vector moves the norm scale by
                 tens of per cent, where the same fault on a normal row (8 of dim terms) hides inside the any-order
                 allowance.  Vector 0, the last one, and the two vectors either side of the first 256-thread chunk seam
                 (v255 / v256 fall back to the last vector where dim has no such vector);
      big        |x| in [5e4, 6e4]: squares of 3.6e9, the fp16 range's end;
      subnormal  fp16 subnormals k·2^-24, k in [1, 1023]: eps decides the scale;
      zero       all zero: the output is 0 (eps > 0), never NaN.
    Returns (x, kinds)."""
    nvec = dim // 8
    x = rng.standard_normal((rows, dim))
    kinds = [ROW_KINDS[(start + i) % len(ROW_KINDS)] for i in range(rows)]
    for i, kind in enumerate(kinds):
        if kind in ("first", "last", "v255", "v256"):
            v = {"first": 0, "last": nvec - 1, "v255": 255, "v256": 256}[kind]
            v = v if v < nvec else nvec - 1
            x[i, v * 8:v * 8 + 8] = 30.0 * (1.0 + 0.05 * rng.standard_normal(8)) * rng.choice([-1.0, 1.0], 8)
        elif kind == "big":
            x[i] = rng.uniform(5e4, 6e4, dim) * rng.choice([-1.0, 1.0], dim)
        elif kind == "subnormal":
            x[i] = rng.integers(1, 1024, dim) * 2.0 ** -24 * rng.choice([-1.0, 1.0], dim)
        elif kind == "zero":
            x[i] = 0.0
    return f16r(x), kinds


def rms_norm_ref64(x, w, eps):
    """(x·inv·w, inv) in float64, inv = 1/sqrt(mean(x²) + eps) per row; eps is the float32 the kernel receives."""
    x64 = np.asarray(x, np.float64)
    inv = 1.0 / np.sqrt((x64 * x64).mean(axis=-1, keepdims=True) + float(np.float32(eps)))
    return x64 * inv * np.asarray(w, np.float64), inv


def norm_scale_allowance(dim):
    """Relative error of x·inv·w held in fp32, before any store: dim·2^-25 + 8·2^-24.

    The row sum: each square rounds once when x is fp32 (exact for fp16 x), and a sum of dim non-negative terms in ANY
    order is within (dim − 1)·2^-24 relative — dim·2^-24 with the squares' own rounding.  /dim and +eps round once each
    (both terms non-negative, so relative errors do not grow): (dim + 2)·2^-24 on the argument of the square root, which
    halves it: dim·2^-25 + 2^-24 on inv, plus a correctly rounded sqrt and divide (2^-24 each; 2.5 ulp covers a fast
    divide) and the two multiplies x·inv and ·w (2^-24 each): dim·2^-25 + (1 + 1 + 2.5 + 2)·2^-24 ≤ dim·2^-25 + 8·2^-24.
    The kernel's tree order is not modelled: any order is allowed."""
    return dim * 2.0 ** -25 + 8 * EPS_F32


def rms_norm_tolerance(ref64, dim):
    """|got − ref| ≤ |ref|·(2^-11 + dim·2^-25 + 8·2^-24) + 2^-24: one fp16 rounding of the stored result on top of
    norm_scale_allowance, and the fp16 floor (a subnormal result rounds by at most 2^-25)."""
    return np.abs(np.asarray(ref64, np.float64)) * (EPS_F16 + norm_scale_allowance(dim)) + FLOOR_F16


def assert_rms_norm_elementwise(x, w, eps, got, what="rms_norm"):
    """Every element of got = fp16(x·inv·w) against float64 from the rows `x` (fp16- or fp32-valued) the kernel normed."""
    ref, _ = rms_norm_ref64(x, w, eps)
    return assert_within(ref, rms_norm_tolerance(ref, np.asarray(x).shape[-1]), got, what)


def assert_sandwich_residual(branch, w_branch, residual_in, eps, got, what="sandwich residual"):
    """residual_out = residual_in + b in fp32, b = rms_norm(branch)·w_branch never stored:

        |got − (r + b)| ≤ 2^-24·|r + b| + |b|·(dim·2^-25 + 8·2^-24) + 2^-149

    b carries norm_scale_allowance; the add rounds once (2^-24 of the result; 2^-149 where the result is subnormal)."""
    b, _ = rms_norm_ref64(branch, w_branch, eps)
    ref = np.asarray(residual_in, np.float64) + b
    tol = EPS_F32 * np.abs(ref) + np.abs(b) * norm_scale_allowance(np.asarray(branch).shape[-1]) + FLOOR_F32
    return assert_within(ref, tol, got, what)


def slabs_to_f16(slabs):
    """fp16(Σ_s slab_s) exactly as the device forms it: float32 adds in slab order from 0, one fp16 rounding.  [S, …] → […]."""
    slabs = np.asarray(slabs, np.float32)
    acc = np.zeros(slabs.shape[1:], np.float32)
    for s in range(slabs.shape[0]):
        acc = acc + slabs[s]
    with np.errstate(over="ignore"):
        return acc.astype(np.float16).astype(np.float32)


def split_into_slabs(rng, target, S):
    """S float32 slabs whose slab-order sum is `target` up to fp32 rounding (an all-zero row stays exactly zero): S − 1
    random slabs of half the row's largest magnitude and the remainder."""
    t = np.asarray(target, np.float32)
    scale = (0.5 * np.abs(t).max(axis=-1, keepdims=True)).astype(np.float32)
    out = np.empty((S,) + t.shape, np.float32)
    acc = np.zeros_like(t)
    for s in range(S - 1):
        out[s] = rng.standard_normal(t.shape).astype(np.float32) * scale
        acc = acc + out[s]
    out[S - 1] = t - acc
    return out


GATE_PLANTS = (12.0, -12.0, 30.0, -30.0, 65504.0, -65504.0)


def gated_inputs(rng, rows, im):
    """fp16-valued gate_up [rows, 2·im] (gate columns, then up columns): 3·N(0, 1), with the six gates of GATE_PLANTS
    planted evenly through the tensor.  Under a ±65504 gate the up value is divided by 16 and clipped to ±0.9, so that the
    product stays a finite fp16."""
    gu = 3.0 * rng.standard_normal((rows, 2 * im))
    g, u = gu[:, :im], gu[:, im:]
    pos = np.linspace(0, rows * im - 1, len(GATE_PLANTS)).astype(int)
    for p, v in zip(pos, GATE_PLANTS):
        r, c = divmod(int(p), im)
        g[r, c] = v
        if abs(v) > 1e4:
            u[r, c] = np.clip(u[r, c] / 16.0, -0.9, 0.9)
    return f16r(gu)


def silu_mul_ref64(g, u):
    g, u = np.asarray(g, np.float64), np.asarray(u, np.float64)
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g)) * u


GELU_C0, GELU_C1 = float(np.float32(0.79788456)), float(np.float32(0.044715))     # the constants of the op, as fp32 holds them


def gelu_tanh_mul_ref64(g, u):
    g, u = np.asarray(g, np.float64), np.asarray(u, np.float64)
    return 0.5 * g * (1.0 + np.tanh(GELU_C0 * (g + GELU_C1 * g * g * g))) * u


def silu_mul_tolerance(ref64):
    """out = fp16(g/(1 + exp(−g))·u) from fp16 g, u in fp32:  |got − ref| ≤ |ref|·(2^-11 + 2^-17) + 2^-24.

    fp32 part: the fast exp scales its argument by log2(e) before exp2 and so loses |g|·2^-24 relative besides its own
    ~2 ulp; 1 + e, the divide (≤ 2.5 ulp) and ·u round once each: (|g| + 6.5)·2^-24 ≤ 2^-17 for |g| ≤ 120.  Past |g| ≈ 32
    nothing of it is visible: for g < −32, |silu(g)·u| < 32·e^-32·65504 < 2^-24, under the floor; for g > 32, e^-g < 2^-46
    and silu(g) = g to fp32 precision whatever exp returns (0 and inf included: g/(1 + 0) = g, g/inf = 0)."""
    return np.abs(np.asarray(ref64, np.float64)) * (EPS_F16 + 2.0 ** -17) + FLOOR_F16


def gelu_tanh_mul_tolerance(ref64, g, u=1.0):
    """out = fp16(0.5·g·(1 + tanh(inner))·u), inner = c0·(g + c1·g³), in fp32:

        |got − ref| ≤ |ref|·(2^-11 + 2^-17) + |g|·|u|·2^-22 + 2^-24

    The bracket 1 + t cancels for negative g (t → −1), so its error is absolute, not relative: tanhf is good to ~2 ulp of
    |t| ≤ 1 (2·2^-24); inner carries 4 roundings, which move t by 4·2^-24·|inner|·(1 − t²) ≤ 4·2^-24·0.45 (x·sech²x ≤ 0.448);
    the sum 1 + t rounds by 2^-24·(1 + t) ≤ 2·2^-24: under 6·2^-24 in all, allowed 8·2^-24 = 2^-21.  Times 0.5·|g|·|u|, that is
    |g|·|u|·2^-22.  At g = −4 (1 + t = 3.5e-5 ≈ 2^-15) an absolute 2^-24 alone is 2^-9 of the result: about three fp16
    ulps, which a purely relative bound would reject.  The remaining multiplies are relative (2^-17 covers them).
    With u = 1 the same bound serves the erf-form `gelu` op, whose bracket 1 − (1 − p·exp(−z²)) cancels the same way."""
    g, u = np.asarray(g, np.float64), np.asarray(u, np.float64)
    return np.abs(np.asarray(ref64, np.float64)) * (EPS_F16 + 2.0 ** -17) + np.abs(g) * np.abs(u) * 2.0 ** -22 + FLOOR_F16


def assert_gated_act_elementwise(gate_up, got, gelu, what=None):
    """fused_{silu,gelu_tanh}_mul_split of an fp16-valued gate_up [rows, 2·im] against float64, every element."""
    gate_up = np.asarray(gate_up, np.float64)
    im = gate_up.shape[1] // 2
    g, u = gate_up[:, :im], gate_up[:, im:]
    if gelu:
        ref = gelu_tanh_mul_ref64(g, u)
        return assert_within(ref, gelu_tanh_mul_tolerance(ref, g, u), got, what or "gelu_tanh·mul")
    ref = silu_mul_ref64(g, u)
    return assert_within(ref, silu_mul_tolerance(ref), got, what or "silu·mul")


def gelu_erf_poly_ref64(x):
    """The `gelu` op's own function in float64: 0.5·x·(1 + erf(x/√2)) with the Abramowitz–Stegun 7.1.26 polynomial (fp32
    coefficients) that the op defines as its erf."""
    x = np.asarray(x, np.float64)
    z = x / np.sqrt(2.0)
    az = np.abs(z)
    c = [float(np.float32(v)) for v in (0.3275911, 1.0614054, 1.4531521, 1.4214138, 0.28449672, 0.2548296)]
    t = 1.0 / (1.0 + c[0] * az)
    y = 1.0 - (((((c[1] * t - c[2]) * t) + c[3]) * t - c[4]) * t + c[5]) * t * np.exp(-az * az)
    return 0.5 * x * (1.0 + np.where(z < 0, -1.0, 1.0) * y)


def layer_norm_ref_tol(x, gamma, beta, eps):
    """out = fp16((x − mean)·inv·γ + β), inv = 1/sqrt(mean((x − mean)²) + eps), two passes in fp32 → (ref64, tol64):

        tol = 2^-11·|ref| + |n|·(dim·2^-25 + 8·2^-24) + M·inv·|γ| + 2^-24·|ref| + 2^-24,   n = (x − mean)·inv·γ,
        M   = dim·2^-24·max|x − mean|   (the cancellation term: the absolute error of the fp32 mean)

    The mean is an fp32 sum of dim signed terms in any order: |δmean| ≤ dim·2^-24·mean|x|.  The term is stated with
    max|x − mean| of the row, which is no smaller on rows whose spread exceeds their offset — asserted here, so the
    bound is only used where it is derived.  Every d = x − mean carries that SAME shift δmean (plus its own 2^-24), so
    n is off by M·inv·|γ| absolutely — the cancellation — while the variance does not see the shift to first order
    (Σd = 0: Σ(d + δ)² = Σd² + dim·δ²) and inv carries the row norm's allowance.  The β add rounds once (2^-24·|ref|),
    then the fp16 store."""
    x64 = np.asarray(x, np.float64)
    dim = x64.shape[-1]
    mean = x64.mean(axis=-1, keepdims=True)
    d = x64 - mean
    assert np.all(np.abs(x64).mean(axis=-1) <= np.abs(d).max(axis=-1)), "row offset exceeds its spread: M understates the mean's error"
    inv = 1.0 / np.sqrt((d * d).mean(axis=-1, keepdims=True) + float(np.float32(eps)))
    gam = np.asarray(gamma, np.float64)
    n = d * inv * gam
    ref = n + np.asarray(beta, np.float64)
    M = dim * EPS_F32 * np.abs(d).max(axis=-1, keepdims=True)
    tol = (EPS_F16 + EPS_F32) * np.abs(ref) + np.abs(n) * norm_scale_allowance(dim) + M * inv * np.abs(gam) + FLOOR_F16
    return ref, tol


# ── decode attention of the one-launch chain (csrc/chain.hip, chain_role_attn) ───────────────────────────────────────────
# A context is given in LOGICAL positions: K / V [columns·16, 128] are what the block table's columns name, in table order
# (spare columns beyond the context included), fp16-valued.  The new token's K / V travel apart (the kernel patches them into
# its fragments from LDS and must not read their pool slot).
ATTN_SCALE = float(np.float32(1.0) / np.sqrt(np.float32(128.0)))      # the launcher's 1.0f / sqrtf(128)
ATTN_CONTEXTS = (1, 2, 15, 16, 17, 31, 32, 33, 48, 129, 250, 256, 257, 300)
ATTN_LONG_CONTEXTS = (1025, 1040, 2064)                               # beyond one 64-entry block-table window
POISON_V = 6e4
PLANT_MASS = (0.02, 0.20)


def _cdiv(a, b):
    return -(-a // b)


def chain_attn_ranges(kv_len, window, splits):
    """(win_lo, [(my_lo, my_hi)] per range) in block pairs, by the kernel's own split rule: the pairs [all_lo, all_hi) of the
    masked context, range s = all_lo + n·s/NS … all_lo + n·(s + 1)/NS."""
    pos0 = kv_len - 1
    win_lo = max(0, pos0 + 1 - window) if window > 0 else 0
    all_lo, all_hi = (win_lo // 16) // 2, (_cdiv(kv_len, 16) + 1) // 2
    n = max(0, all_hi - all_lo)
    return win_lo, [(all_lo + n * s // splits, all_lo + n * (s + 1) // splits) for s in range(splits)]


def decode_attn_ref_tol(q, K, V, allowed, kv_len, window, splits=1, scale=ATTN_SCALE):
    """float64 decode attention of R query rows over the `allowed` logical positions, and the element-wise bound of
    chain_role_attn → (ref [R, 128], tol [R, 128], w [R, positions] the softmax masses, 0 outside `allowed`).

        o = Σ_j w_j·v_j,  w = softmax(scale·q·k_j),      tol_d = 2^-11·|o_d| + ε·(Σ_j w_j|v_jd| + |o_d|) + S_d + 2^-24

    q, K, V are the fp16 values the device used (K / V with the new token's row already in place).  ε is the sum of the relative
    errors one probability w_j = p_j / l can carry, numerator and denominator counted separately, each term against the line
    of chain_role_attn it covers (n keys allowed, it = ceil(pairs / 8) iterations of a wave at most, NS ranges):

      2^-11                 `pf[j] = (_Float16)pv`: P is rounded to fp16 for the PV MFMA while `psum += pv` sums the unrounded
                            fp32 values — numerator only;
      2·δs                  `s0 = mfma(kf0[s], qf[s], s0)` ×4 and `sc[r] = s0[r] * p.scale`: 128 exact fp16 products accumulated in
                            fp32 in the worst case one by one, δs_j = 128·2^-23·scale·Σ_i|q_i||k_ji| + 2^-24·|s_j| (the multiply),
                            maximised over the row's keys; exp(s + δ) = exp(s)·(1 + δ): once in p_j, once (at most) in l;
      2·(it + 3)·e_exp      `__expf` — on gfx950 v_mul_f32 by log2(e), then v_exp_f32 (1 ulp: 2^-23).  The product rounds once
                            and log2(e) is itself an fp32 constant: 2·2^-24·|x| on the result; the argument `sc[j] - m_safe` rounds
                            once more (2^-24·|x|): e_exp = 2^-23 + 3·2^-24·D with D the row's largest |s − m|.  A value meets its own
                            exp, then one `alpha = __expf(m_run - m_safe)` per later iteration of its wave, `fw[w]` of the wave
                            merge and `f` of the range merge (their arguments are differences of maxima of the same row: ≤ D) —
                            at most it + 3 factors, in the numerator and in l alike;
      2^-24·(2·(n + it + 2·8 + 2·NS) + 2)
                            one 2^-24 per fp32 operation a value passes through, numerator and l each: the accumulation of PV
                            (`o_acc = mfma(vfrag, pf, o_acc)`) and of `psum` / `l_run` over n terms in ANY order, `o_acc *= alpha`
                            and `l_run * alpha` per iteration, multiply and add per wave of the LDS merge (`acc += lds_o·fw[w]`),
                            multiply and add per range of the range merge; then `1.0f / Lm` and `ov[i] * inv`.

    S_d = Σ_j min(w_j, 2^-14·w_max)·|v_jd| is absolute: p_j = exp(s_j − m_run) ≥ w_j / w_max whenever it is formed (m_run ≤ the
    row's final maximum), so a p_j below the fp16 normal range 2^-14 — flushed by v_exp_f32 or coarsened to a subnormal by the
    cast, in the numerator only — belongs to a key with w_j < 2^-14·w_max and is worth at most all of w_j.
    2^-11·|o_d| is the fp16 store of the result, 2^-24 the fp16 floor.  One v_mfma_f32_16x16x32_f16 may add its 32 products with
    a single rounding (an assumption nobody here has measured); the bound does not use it: n terms one by one cover both."""
    q, K, V = np.asarray(q, np.float64), np.asarray(K, np.float64), np.asarray(V, np.float64)
    allowed = np.asarray(allowed, bool)
    idx = np.nonzero(allowed)[0]
    Ka, Va = K[idx], V[idx]
    s = scale * (q @ Ka.T)                                               # [R, n]
    m = s.max(axis=1, keepdims=True)
    e = np.exp(s - m)
    wa = e / e.sum(axis=1, keepdims=True)
    ref = wa @ Va
    absw = wa @ np.abs(Va)
    n = idx.size
    _, ranges = chain_attn_ranges(kv_len, window, 1)
    it = _cdiv(max(1, ranges[0][1] - ranges[0][0]), 8)
    d_s = (128 * EPS_F32_SUM * scale * (np.abs(q) @ np.abs(Ka).T) + EPS_F32 * np.abs(s)).max(axis=1, keepdims=True)
    e_exp = 2.0 ** -23 + 3 * EPS_F32 * (m - s.min(axis=1, keepdims=True))
    eps = EPS_F16 + 2 * d_s + 2 * (it + 3) * e_exp + EPS_F32 * (2 * (n + it + 16 + 2 * splits) + 2)
    small = np.minimum(wa, 2.0 ** -14 * wa.max(axis=1, keepdims=True)) @ np.abs(Va)
    tol = EPS_F16 * np.abs(ref) + eps * (absw + np.abs(ref)) + small + FLOOR_F16
    w = np.zeros((q.shape[0], K.shape[0]))
    w[:, idx] = wa
    return ref, tol, w


def _exp32(x):
    with np.errstate(under="ignore"):
        return np.exp(np.asarray(x, np.float64)).astype(np.float32)


ATTN_FAULTS = ("drop_last_key_of_range", "first_key_of_next_range_twice", "win_lo_one_low", "win_lo_one_high", "slot_past_kv_len",
               "absent_second_block", "new_token_from_pool", "range_left_out", "stale_m", "neighbour_q", "window_not_reloaded")


def chain_attn_emulate(q, K, V, k_new, v_new, kv_len, window, splits=1, scale=ATTN_SCALE, fault=None, fault_range=0):
    """chain_role_attn restated in float32 / fp16, in the kernel's order: block pairs (32 keys) strided over 8 waves, per pair
    four 32-term k-steps of QKᵀ (each k-step's exact sum added with one fp32 rounding — the single-rounding assumption of the
    MFMA), `·scale`, mask, online softmax with fp32 `l` and fp16 P, one PV MFMA per pair; the 8 wave states merged in wave order;
    the `splits` range states (m, l, o) merged in range order; reciprocal, multiply, fp16 store.  exp is float64 rounded to
    fp32.  q [R, 128] the rows of ONE kv head, K / V logical positions (see above), k_new / v_new the new token's rows.

    `fault` (ATTN_FAULTS) changes what the kernel would change: which logical positions are read and counted, which state
    enters a merge.  fault_range picks the range for the faults that name one."""
    assert fault is None or fault in ATTN_FAULTS
    q32 = np.asarray(q, np.float32)
    if fault == "neighbour_q":
        q32 = np.roll(q32, 1, axis=0)
    q64 = q32.astype(np.float64)
    K, V = np.asarray(K, np.float64), np.asarray(V, np.float64)
    R, NW = q32.shape[0], 8
    pos0, nblocks = kv_len - 1, _cdiv(kv_len, 16)
    win_lo, ranges = chain_attn_ranges(kv_len, window, splits)
    win_eff = win_lo + {"win_lo_one_low": -1, "win_lo_one_high": 1}.get(fault, 0)
    mult = np.ones(K.shape[0])
    if fault == "drop_last_key_of_range":
        mult[ranges[fault_range][1] * 32 - 1] = 0
    if fault == "first_key_of_next_range_twice":
        mult[ranges[fault_range + 1][0] * 32] = 2
    ninf = np.float32(-np.inf)
    states = []
    for (my_lo, my_hi) in ranges:
        bt_lo = 2 * my_lo
        wm, wl, wo = np.full((NW, R), ninf), np.zeros((NW, R), np.float32), np.zeros((NW, R, 128), np.float32)
        for wave in range(NW):
            m_run, l_run, o = np.full(R, ninf), np.zeros(R, np.float32), np.zeros((R, 128), np.float32)
            for pr in range(my_lo + wave, my_hi, NW):
                pos = pr * 32 + np.arange(32)
                blk = pos // 16
                has = blk < nblocks
                if fault == "absent_second_block":
                    has = blk < K.shape[0] // 16
                src_blk = np.where(has, blk, 2 * pr)                         # phys1 = phys0 where the pair has no second block
                if fault == "window_not_reloaded":
                    src_blk = bt_lo + (src_blk - bt_lo) % 64
                src = src_blk * 16 + pos % 16
                Kp, Vp = K[src].copy(), V[src].copy()
                if fault != "new_token_from_pool" and pos[0] <= pos0 <= pos[-1]:
                    Kp[pos0 - pos[0]], Vp[pos0 - pos[0]] = k_new, v_new
                s = np.zeros((R, 32))
                for ks in range(4):
                    s = _fl32(s + q64[:, 32 * ks:32 * ks + 32] @ Kp[:, 32 * ks:32 * ks + 32].T)
                ok = (pos <= pos0 + (1 if fault == "slot_past_kv_len" else 0)) & (pos >= win_eff)
                if fault == "absent_second_block":
                    ok = ok | ((blk >= nblocks) & has & (blk == 2 * pr + 1))
                ok = ok & (mult[pos] > 0)
                sc = np.where(ok[None, :], (s.astype(np.float32) * np.float32(scale)), ninf).astype(np.float32)
                m_new = np.maximum(m_run, sc.max(axis=1))
                m_safe = np.where(np.isneginf(m_new), np.float32(0), m_new)
                with np.errstate(invalid="ignore"):
                    alpha = np.where(np.isneginf(m_run), np.float32(0), _exp32(m_run - m_safe))
                p = _exp32(sc - m_safe[:, None]) * mult[pos][None, :].astype(np.float32)
                l_run = l_run * alpha + p.sum(axis=1, dtype=np.float32)
                pf = p.astype(np.float16).astype(np.float64)
                o = _fl32((o * alpha[:, None]).astype(np.float64) + pf @ Vp).astype(np.float32)
                m_run = m_new
            wm[wave], wl[wave], wo[wave] = m_run, l_run, o
        M = wm.max(axis=0)
        Ms = np.where(np.isneginf(M), np.float32(0), M)
        L, acc = np.zeros(R, np.float32), np.zeros((R, 128), np.float32)
        for w in range(NW):
            fw = _exp32(wm[w] - Ms)
            L = L + wl[w] * fw
            acc = acc + wo[w] * fw[:, None]
        states.append((M, L, acc))
    if splits == 1:
        M, L, acc = states[0]
    else:
        ms = np.stack([st[0] for st in states])
        merged = [i for i in range(splits) if not (fault == "range_left_out" and i == fault_range)]
        M = ms[merged].max(axis=0)
        Ms = np.where(np.isneginf(M), np.float32(0), M)
        L, acc = np.zeros(R, np.float32), np.zeros((R, 128), np.float32)
        for i in merged:
            m_i = ms[i - 1] if (fault == "stale_m" and i == fault_range) else ms[i]
            f = _exp32(m_i - Ms)
            L = L + states[i][1] * f
            acc = acc + states[i][2] * f[:, None]
    with np.errstate(divide="ignore"):
        inv = np.where(L > 0, np.float32(1) / L, np.float32(0)).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return (acc * inv[:, None]).astype(np.float16).astype(np.float32)


def attn_edge_positions(kv_len, window, splits):
    """The positions inside the mask (the new token apart) that a fault would lose or wrongly gain: position 0, win_lo, the
    first and last key of every KV range (my_lo·32, my_hi·32 − 1), both sides of the last two 16-key block seams, pos0 − 1."""
    pos0 = kv_len - 1
    win_lo, ranges = chain_attn_ranges(kv_len, window, splits)
    want = [0, win_lo, pos0 - 1]
    for lo, hi in ranges:
        if hi > lo:
            want += [lo * 32, hi * 32 - 1]
    for seam in ((pos0 // 16) * 16, (pos0 // 16 - 1) * 16):
        want += [seam - 1, seam]
    return sorted({p for p in want if win_lo <= p < pos0})


def attn_poison_positions(kv_len, window, columns):
    """Logical positions outside the mask that must not be counted: win_lo − 1, every slot ≥ kv_len of the last block, the
    whole second block of an odd pair and every table column beyond the context, and the new token's own pool slot."""
    pos0, nblocks = kv_len - 1, _cdiv(kv_len, 16)
    win_lo, _ = chain_attn_ranges(kv_len, window, 1)
    out = set(range(kv_len, columns * 16)) | {pos0}
    if win_lo > 0:
        out.add(win_lo - 1)
    return sorted(out)


def plant_context(rng, q, k_new, kv_len, window, splits, columns, scale=ATTN_SCALE):
    """Logical K / V [columns·16, 128] (fp16-valued) of one (sequence, kv head) whose G query rows are q [G, 128] → dict(K, V,
    edges, heads, poison).  Background N(0, 1).  Edge position i (attn_edge_positions) holds K = f16(β_h·q̂_h), h = i mod G, with
    β_h solved so that each of the m_h keys planted for row h carries t_h = min(8 %, 60 % / m_h) of that row's softmax mass
    against everything else the row sees (the other rows' planted keys and the new token included; four fixed-point rounds),
    and V = ±2 in a sign pattern of its own.  Poison (attn_poison_positions): K = f16(γ·u), u the unit vector with the same product on every q̂ (pinv(q̂)·1) and γ such
    that on EVERY row the key alone would outweigh the whole allowed context by e (> 50 % of the mass if counted), V = ±6e4."""
    q = np.asarray(q, np.float64)
    G, P = q.shape[0], columns * 16
    pos0 = kv_len - 1
    win_lo, _ = chain_attn_ranges(kv_len, window, 1)
    K, V = f16r(rng.standard_normal((P, 128))).astype(np.float64), f16r(rng.standard_normal((P, 128))).astype(np.float64)
    qn = np.linalg.norm(q, axis=1)
    qhat = q / qn[:, None]
    edges = attn_edge_positions(kv_len, window, splits)
    heads = [i % G for i in range(len(edges))]
    for p in edges:
        V[p] = 2.0 * np.random.default_rng(7000 + p).choice([-1.0, 1.0], 128)
    allowed = np.zeros(P, bool)
    allowed[win_lo:kv_len] = True
    Keff = K.copy()
    Keff[pos0] = k_new
    beta = np.zeros(G)
    for _ in range(4):
        for p, h in zip(edges, heads):
            Keff[p] = f16r(beta[h] * qhat[h])
        s = scale * (q @ Keff[allowed].T)                                # [G, n]
        apos = np.nonzero(allowed)[0]
        for h in range(G):
            mine = np.isin(apos, [p for p, hh in zip(edges, heads) if hh == h])
            m_h = int(mine.sum())
            if m_h == 0:
                continue
            t = min(0.08, 0.6 / m_h)
            logZ = np.logaddexp.reduce(s[h, ~mine]) if (~mine).any() else 0.0
            beta[h] = (np.log(t / (1.0 - m_h * t)) + logZ) / (scale * qn[h])
    for p, h in zip(edges, heads):
        K[p] = f16r(beta[h] * qhat[h])
    Keff[edges] = K[edges]
    u = np.linalg.pinv(qhat) @ np.ones(G)                                 # q̂_h·u = 1 for every row (G ≤ 14 independent rows of 128)
    u /= np.linalg.norm(u)
    assert np.all(q @ u > 0), "a query row points away from the poison direction"
    logZ = np.logaddexp.reduce(scale * (q @ Keff[allowed].T), axis=1)
    gamma = float(((logZ + 1.0) / (scale * (q @ u))).max())
    poison = attn_poison_positions(kv_len, window, columns)
    for p in poison:
        K[p] = f16r(gamma * u)
        V[p] = POISON_V * np.where((np.arange(128) + p) % 2 == 0, 1.0, -1.0)
    assert np.isfinite(K).all() and np.abs(K).max() < 6e4
    return dict(K=K, V=V, edges=edges, heads=heads, poison=poison, allowed=allowed)


def effective_kv(ctx, k_new, v_new, kv_len):
    """K / V as the kernel sees them: the planted context with the new token's rows in place."""
    K, V = ctx["K"].copy(), ctx["V"].copy()
    K[kv_len - 1], V[kv_len - 1] = k_new, v_new
    return K, V


# ── routing without logits (role B of the chain never stores them) ────────────────────────────────────────────────────────
def route_logits_ref_tol(norm2, router_w):
    """float64 router logits L = norm2·Wᵀ from the DEVICE's norm2 rows and the fp16 router rows, and the fp32 GEMM bound
    gemm_tolerance(…, k = H, folded = False, out_f32 = True) → (L [T, E], tol_L [T, E])."""
    ref, absdot = gemm_refs(norm2, router_w)
    return ref, gemm_tolerance(ref, absdot, np.asarray(norm2).shape[1], False, out_f32=True)


def assert_route_selection(L, tol, ids, weights, norm_topk, what="routing"):
    """ids / weights [T, K] of the merged routing against float64 logits L ± tol.

      selection   no unchosen expert u may have L_u − tol_u > L_c + tol_c for a chosen c;
      rank order  consecutive chosen experts a (rank r), b (rank r + 1): not L_b − tol_b > L_a + tol_a;
      exact ties  experts whose router rows are duplicates give bit-identical logits: callers pass them through `tie_groups`
                  to assert_route_ties;
      weights     against softmax(L) over all E, renormalised over the device's chosen set when norm_topk:
                  |w − ref| ≤ ref·(2·max tol_L + (E + 8)·2^-24) — every exponent moves by ≤ tol_L (numerator) and the sum by ≤ max
                  tol_L (denominator); the fp32 sum of E exps in any order, the exp, the reciprocal and the products: (E + 8)·2^-24.
    Returns the largest weight err/tol."""
    L, tol = np.asarray(L, np.float64), np.asarray(tol, np.float64)
    ids, weights = np.asarray(ids), np.asarray(weights, np.float64)
    T, E = L.shape
    K = ids.shape[1]
    worst = 0.0
    for t in range(T):
        c = ids[t]
        assert len(set(c.tolist())) == K and c.min() >= 0 and c.max() < E, f"{what}: token {t} ids {c.tolist()}"
        un = np.setdiff1d(np.arange(E), c)
        if un.size:
            u = un[np.argmax(L[t, un] - tol[t, un])]
            lo = c[np.argmin(L[t, c] + tol[t, c])]
            assert not (L[t, u] - tol[t, u] > L[t, lo] + tol[t, lo]), \
                f"{what}: token {t}: unchosen expert {u} (L {L[t, u]!r}) beats chosen {lo} (L {L[t, lo]!r}) beyond both tolerances"
        for r in range(K - 1):
            a, b = c[r], c[r + 1]
            assert not (L[t, b] - tol[t, b] > L[t, a] + tol[t, a]), f"{what}: token {t}: rank {r + 1} (expert {b}) above rank {r} (expert {a})"
        p = np.exp(L[t] - L[t].max())
        p /= p.sum()
        ref = p[c] / p[c].sum() if norm_topk else p[c]
        wtol = ref * (2 * tol[t].max() + (E + 8) * EPS_F32)
        err = np.abs(weights[t] - ref)
        assert np.all(err <= wtol), f"{what}: token {t} combine weights {weights[t].tolist()} against {ref.tolist()} (err/tol {float((err / wtol).max()):.3g})"
        worst = max(worst, float((err / wtol).max()))
    return worst


def assert_route_ties(ids, tie_groups, what="routing"):
    """tie_groups: lists of expert ids with bit-identical logits (duplicated router rows).  Of a tied group the chosen members
    must be its LOWEST ids, in id order, at consecutive ranks.  Returns the number of tokens whose top-k boundary cuts a group."""
    cut = 0
    for t, c in enumerate(np.asarray(ids).tolist()):
        for g in tie_groups:
            g = sorted(g)
            chosen = [e for e in c if e in g]
            assert chosen == g[:len(chosen)], f"{what}: token {t}: tied group {g} chose {chosen}"
            if chosen:
                r = [c.index(e) for e in chosen]
                assert r == list(range(r[0], r[0] + len(r))), f"{what}: token {t}: tied experts {chosen} at ranks {r}"
            cut += 0 < len(chosen) < len(g)
    return cut


def route_beats(lj, ij, l, i):
    return lj > l or (lj == l and ij < i)


def assert_route_lists(L, tol, cand_logit, cand_id, stats, Q, top_k, what="candidate lists"):
    """The per-part candidate lists of defer_merge: cand_logit / cand_id [T, Q, 8], stats [T, Q, 2] (max, Σexp); part q owns
    experts [q, q + 1)·EQ cut at E, EQ = ceil(E / 16) / Q · 16, and lists its best keep = min(top_k, EQ).

      order     each list is sorted by route_beats on its own logit bits;
      values    every listed logit within tol_L of float64;
      coverage  no unlisted expert u of the part with L_u − tol_u > L_last + tol_last;
      unused    slots ≥ keep hold (0x7fffffff, −inf);
      stats     max equals the first listed logit bit for bit; Σexp = Σ_e exp(l_e − max) within
                Σexp·((EQ + 8)·2^-24 + 2·max tol_L): every exponent and the maximum move by ≤ tol_L; EQ exps summed in fp32 in any
                order, the exp and the subtraction: (EQ + 8)·2^-24."""
    L, tol = np.asarray(L, np.float64), np.asarray(tol, np.float64)
    T, E = L.shape
    EQ = _cdiv(E, 16) // Q * 16
    keep = min(top_k, EQ)
    cl, ci, st = np.asarray(cand_logit, np.float32), np.asarray(cand_id), np.asarray(stats, np.float32)
    for t in range(T):
        for qq in range(Q):
            own = np.arange(qq * EQ, min(E, (qq + 1) * EQ))
            n_l = min(keep, own.size)
            ids, lg = ci[t, qq], cl[t, qq]
            assert np.all(ids[n_l:] == 0x7fffffff) and np.all(np.isneginf(lg[n_l:])), f"{what}: token {t} part {qq}: unused slots {ids.tolist()} {lg.tolist()}"
            listed = ids[:n_l]
            assert len(set(listed.tolist())) == n_l and np.all(np.isin(listed, own)), f"{what}: token {t} part {qq}: ids {listed.tolist()}"
            for r in range(n_l - 1):
                assert route_beats(lg[r], int(ids[r]), lg[r + 1], int(ids[r + 1])), f"{what}: token {t} part {qq}: slots {r}, {r + 1} out of order"
            assert np.all(np.abs(lg[:n_l].astype(np.float64) - L[t, listed]) <= tol[t, listed]), f"{what}: token {t} part {qq}: a listed logit outside tol_L"
            un = np.setdiff1d(own, listed)
            if un.size and n_l:
                u, last = un[np.argmax(L[t, un] - tol[t, un])], listed[-1]
                assert not (L[t, u] - tol[t, u] > L[t, last] + tol[t, last]), f"{what}: token {t} part {qq}: unlisted expert {u} beats the last listed {last}"
            assert st[t, qq, 0].tobytes() == lg[0].tobytes(), f"{what}: token {t} part {qq}: stats.max {st[t, qq, 0]!r} is not the first listed logit {lg[0]!r}"
            ref = np.exp(L[t, own] - L[t, own].max()).sum()
            stol = ref * ((EQ + 8) * EPS_F32 + 2 * tol[t, own].max())
            assert abs(float(st[t, qq, 1]) - ref) <= stol, f"{what}: token {t} part {qq}: Σexp {st[t, qq, 1]!r} against {ref!r} (tol {stol:.3g})"


# The attention cases of tests/test_chain_roles_gpu.py (the CPU self-test runs the restatement through the same list):
# name → (nkv, attn_splits, sliding_window, contexts — row t of the launch holds contexts[t % len]).
def _window_contexts(w):
    return tuple(n for n in (w - 1, w, w + 1) if n >= 1) + (300,)


ATTN_CASES = {
    "g8-unsplit": (4, 1, 0, ATTN_CONTEXTS),
    "g8-5-ranges": (4, 5, 0, ATTN_CONTEXTS),
    "g8-16-ranges": (4, 16, 0, ATTN_CONTEXTS),
    "g4-5-ranges": (8, 5, 0, ATTN_CONTEXTS),
    "g4-unsplit": (8, 1, 0, ATTN_CONTEXTS),
    "g2-unsplit": (16, 1, 0, ATTN_CONTEXTS),
    "g2-16-ranges": (16, 16, 0, ATTN_CONTEXTS),
    "window-1": (4, 1, 1, _window_contexts(1)),
    "window-16-5-ranges": (4, 5, 16, _window_contexts(16)),
    "window-17": (4, 1, 17, _window_contexts(17)),
    "window-150-5-ranges": (4, 5, 150, _window_contexts(150)),
    "window-150-g4-16-ranges": (8, 16, 150, _window_contexts(150)),
    "long-unsplit": (4, 1, 0, ATTN_LONG_CONTEXTS),
    "long-5-ranges": (4, 5, 0, ATTN_LONG_CONTEXTS),
}
