"""The scoring surface without a GPU: both symbols are exported, the op-level entry refuses bad arguments on the host (return
code 2 and a message, before anything is launched), the ctypes mirrors of the three structs follow the header's field order,
and the Python and Rust layers carry the entry points over names the library really exports."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ferrum_hip_model_score", "ferrum_hip_logprob_rows_f32")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


def _exported(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    return set(line.split()[-1] for line in out.splitlines() if " T " in line)


def test_score_symbols_are_exported(pkg):
    exported = _exported(pkg)
    assert not [s for s in SYMBOLS if s not in exported]


def test_logprob_rows_rejects_bad_arguments_on_the_host(pkg):
    """logits, ld, m, n, pair_rows, pair_tokens, num_pairs, pair_logprob, row_lse, row_top, ws, stream: nothing below reaches a
    device — every call fails a check first, so the pointers are never dereferenced."""
    lib = pkg.load_library()
    call = lib.ferrum_hip_logprob_rows_f32
    one = C.c_void_p(16)
    cases = {
        "null logits": (lambda: call(None, 8, 1, 8, one, one, 1, one, None, None, None, None), b"null logits"),
        "null pair_rows": (lambda: call(one, 8, 1, 8, None, one, 1, one, None, None, None, None), b"null pair"),
        "null pair_tokens": (lambda: call(one, 8, 1, 8, one, None, 1, one, None, None, None, None), b"null pair"),
        "null pair_logprob": (lambda: call(one, 8, 1, 8, one, one, 1, None, None, None, None, None), b"null pair"),
        "m < 0": (lambda: call(one, 8, -1, 8, one, one, 1, one, None, None, None, None), b"m="),
        "m > 65535": (lambda: call(one, 8, 65536, 8, one, one, 1, one, None, None, None, None), b"m="),
        "n = 0": (lambda: call(one, 8, 1, 0, one, one, 1, one, None, None, None, None), b"n="),
        "n < 0": (lambda: call(one, 8, 1, -4, one, one, 1, one, None, None, None, None), b"n="),
        "ld < n": (lambda: call(one, 7, 1, 8, one, one, 1, one, None, None, None, None), b"ld="),
        "num_pairs < 0": (lambda: call(one, 8, 1, 8, one, one, -1, one, None, None, None, None), b"num_pairs"),
        "pairs without rows": (lambda: call(None, 8, 0, 8, one, one, 1, one, None, None, None, None), b"no rows"),
        "no workspace": (lambda: call(one, 8, 1, 8, one, one, 1, one, None, None, None, None), b"workspace of 16 bytes"),
    }
    for name, (run, word) in cases.items():
        assert run() == 2, name
        assert word in lib.ferrum_hip_last_error(), (name, lib.ferrum_hip_last_error())
    assert call(None, 0, 0, 0, None, None, 0, None, None, None, None, None) == 0            # no rows: a no-op


def test_model_score_refuses_a_null_model(pkg):
    lib = pkg.load_library()
    assert lib.ferrum_hip_model_score(None, None, 0, None, 0, None, None) == 2
    assert b"model_score" in lib.ferrum_hip_last_error()


def _header_struct(name):
    src = open(os.path.join(ROOT, "include", "ferrum_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(t, n) for t, n in re.findall(r"(\w+)\s+(\w+)\s*;", body)]


def test_struct_mirrors_follow_the_header(pkg):
    from ferrum_infer_rs_amd.executor import ScoreOptions, ScoreTarget, TokenScore
    ctype = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float}
    for mirror, name, size in ((ScoreTarget, "FerrumHipScoreTarget", 16), (TokenScore, "FerrumHipTokenScore", 16), (ScoreOptions, "FerrumHipScoreOptions", 8)):
        fields = _header_struct(name)
        assert fields and [(ctype[t], n) for t, n in fields] == [(t, n) for n, t in mirror._fields_], name
        assert C.sizeof(mirror) == size


def test_python_layers_carry_the_entry_points(pkg):
    from ferrum_infer_rs_amd.backend import HipBackend
    from ferrum_infer_rs_amd.executor import HipModel
    assert callable(HipModel.score) and callable(HipModel.loglikelihood) and callable(HipBackend.logprob_rows)


def test_rust_crate_scores_over_exported_names(pkg):
    src = open(os.path.join(ROOT, "crates", "ferrum-hip", "src", "executor.rs")).read()
    ffi = open(os.path.join(ROOT, "crates", "ferrum-hip", "src", "ffi.rs")).read()
    exported = _exported(pkg)
    m = re.search(r"pub fn score_tokens\b.*?\n    }\n", src, flags=re.S)
    assert m, "crates/ferrum-hip/src/executor.rs has no fn score_tokens"
    used = set(re.findall(r"ffi::(\w+)", m.group(0)))
    fns = {u for u in used if u.startswith("ferrum_hip_")}
    assert "ferrum_hip_model_score" in fns and not [u for u in fns if u not in exported]
    for u in used - fns:                                         # structs and constants: declared in the generated ffi.rs
        assert re.search(r"pub (struct|const) %s\b" % u, ffi), u
