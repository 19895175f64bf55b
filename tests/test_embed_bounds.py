"""tests/embed_bounds.py on the CPU: an fp32 emulation of the embedding tail (row norm, pool, cut, L2; sums in sequential and
in pairwise-tree order) stays inside the bound on the inputs the GPU test uses, and a mean that drops one token of a 65-token
span, an L2 norm taken before the cut, and a NaN do not."""
import numpy as np
import pytest

from tests import embed_bounds as eb
from tests import parity_bounds as pb

EPS = 1e-6


def _sum32(a, tree):
    """fp32 sum over axis 0 of a [n, ...] array, sequentially or as a pairwise tree."""
    a = np.asarray(a, np.float32)
    if not tree:
        acc = np.zeros(a.shape[1:], np.float32)
        for r in a:
            acc = acc + r
        return acc
    while len(a) > 1:
        if len(a) % 2:
            a = np.concatenate([a, np.zeros((1,) + a.shape[1:], np.float32)])
        a = a[0::2] + a[1::2]
    return a[0]


def _emulate(x, w, spans, pooling, normalize, dims, tree, drop=None, cut_last=False):
    H = x.shape[1]
    xf = np.asarray(x, np.float32)
    if w is not None:
        ss = _sum32((xf * xf).T, tree)
        inv = (np.float32(1) / np.sqrt(ss / np.float32(H) + np.float32(EPS))).astype(np.float32)
        n = (xf * inv[:, None]).astype(np.float32) * np.asarray(w, np.float32)
    else:
        n = xf
    out = []
    for i, (b, e) in enumerate(spans):
        if pooling == 0:
            v = n[e - 1]
        elif pooling == 2:
            v = n[b]
        else:
            rows = n[b:e - 1] if drop == i else n[b:e]
            v = _sum32(rows, tree) / np.float32(e - b)
        d = dims or H
        if normalize and cut_last:
            v = (v / max(np.sqrt(_sum32(v * v, tree)), np.float32(1e-12)))[:d]
        else:
            v = v[:d]
            if normalize:
                v = v / max(np.sqrt(_sum32(v * v, tree)), np.float32(1e-12))
        out.append(v)
    return np.stack(out)


def _inputs(H):
    from tests import test_embed_gpu
    x16, x32, w, spans, zero_span, _ = test_embed_gpu._inputs(H)
    return x16, x32, w, spans, zero_span


@pytest.mark.parametrize("H", [256, 5376])
def test_fp32_emulation_is_inside_the_bound(H):
    x16, x32, w, spans, zero_span = _inputs(H)
    worst = 0.0
    for x in (x16, x32):
        for wv in (w, None):
            for pooling in (0, 1, 2):
                for normalize in (0, 1):
                    for dims in (0, 32, 100):
                        ref, tol = eb.ref_tol(x, wv, EPS, spans, pooling, normalize, dims)
                        assert (ref[zero_span] == 0).all()
                        for tree in (False, True):
                            worst = max(worst, pb.assert_within(ref, tol, _emulate(x, wv, spans, pooling, normalize, dims, tree), "emulation"))
    print("largest err/tol of the fp32 emulation:", worst)
    assert worst < 1.0


def test_the_bound_sees_a_dropped_token_a_late_cut_and_nan():
    x16, _, w, spans, _ = _inputs(256)
    long65 = [i for i, (b, e) in enumerate(spans) if e - b == 65][0]
    ref, tol = eb.ref_tol(x16, w, EPS, spans, 1, 1, 0)
    with pytest.raises(AssertionError):
        pb.assert_within(ref, tol, _emulate(x16, w, spans, 1, 1, 0, False, drop=long65), "dropped token")
    ref, tol = eb.ref_tol(x16, w, EPS, spans, 0, 1, 32)
    with pytest.raises(AssertionError):
        pb.assert_within(ref, tol, _emulate(x16, w, spans, 0, 1, 32, False, cut_last=True), "L2 before the cut")
    got = _emulate(x16, w, spans, 0, 1, 32, False)
    got[0, 0] = np.nan
    with pytest.raises(AssertionError):
        pb.assert_within(ref, tol, got, "NaN")
