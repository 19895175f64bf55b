"""The embedding surface without a GPU: the two op-level exports refuse bad arguments on the host (return code 2 and a message,
before anything is launched), the four new symbols are exported, and the Python and Rust layers carry the entry points over
names the library really exports."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ferrum_hip_model_embed", "ferrum_hip_model_embedding_dim", "ferrum_hip_embed_pool_f16", "ferrum_hip_embed_pool_f32")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


def _exported(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    return set(line.split()[-1] for line in out.splitlines() if " T " in line)


def test_embed_symbols_are_exported(pkg):
    exported = _exported(pkg)
    assert not [s for s in SYMBOLS if s not in exported]


@pytest.mark.parametrize("fn", ["ferrum_hip_embed_pool_f16", "ferrum_hip_embed_pool_f32"])
def test_embed_pool_exports_reject_bad_arguments_on_the_host(pkg, fn):
    """hidden, seq_rows, norm_w, eps, pooling, normalize, dims, out, num_seqs, dim, ws, stream: nothing below reaches a device —
    every call fails a check first, so the pointers are never dereferenced."""
    lib = pkg.load_library()
    call = getattr(lib, fn)
    f, one = C.c_float(1e-6), C.c_void_p(16)
    cases = {
        "null hidden": (lambda: call(None, one, one, f, 0, 1, 0, one, 1, 256, None, None), b"null"),
        "null seq_rows": (lambda: call(one, None, one, f, 0, 1, 0, one, 1, 256, None, None), b"null"),
        "null out": (lambda: call(one, one, one, f, 0, 1, 0, None, 1, 256, None, None), b"null"),
        "pooling = 3": (lambda: call(one, one, one, f, 3, 1, 0, one, 1, 256, None, None), b"pooling"),
        "pooling = -1": (lambda: call(one, one, one, f, -1, 1, 0, one, 1, 256, None, None), b"pooling"),
        "dims > dim": (lambda: call(one, one, one, f, 0, 1, 257, one, 1, 256, None, None), b"dims"),
        "dims < 0": (lambda: call(one, one, one, f, 0, 1, -1, one, 1, 256, None, None), b"dims"),
        "dim % 8": (lambda: call(one, one, one, f, 0, 1, 0, one, 1, 260, None, None), b"dim"),
        "dim > 16384": (lambda: call(one, one, one, f, 0, 1, 0, one, 1, 16392, None, None), b"dim"),
        "num_seqs < 0": (lambda: call(one, one, one, f, 0, 1, 0, one, -1, 256, None, None), b"num_seqs"),
        "mean without a workspace": (lambda: call(one, one, one, f, 1, 1, 0, one, 1, 256, None, None), b"workspace"),
    }
    for name, (run, word) in cases.items():
        assert run() == 2, name
        assert word in lib.ferrum_hip_last_error(), (name, lib.ferrum_hip_last_error())
    assert call(None, None, None, f, 0, 1, 0, None, 0, 256, None, None) == 0           # no spans: a no-op


def test_python_layers_carry_the_entry_points(pkg):
    from ferrum_infer_rs_amd.backend import HipBackend
    from ferrum_infer_rs_amd.executor import EmbedOptions, HipModel
    assert callable(HipModel.embed) and callable(HipModel.embedding_dim) and callable(HipBackend.embed_pool)
    assert [n for n, _ in EmbedOptions._fields_] == ["pooling", "normalize", "dims", "skip_final_norm", "release", "_pad"]
    assert C.sizeof(EmbedOptions) == 24


def test_model_embed_refuses_a_null_model(pkg):
    lib = pkg.load_library()
    h = C.c_int(-1)
    assert lib.ferrum_hip_model_embed(None, None, 0, None, None) == 2
    assert lib.ferrum_hip_model_embedding_dim(None, C.byref(h)) == 2 and h.value == -1


def test_rust_crate_embeds_over_exported_names(pkg):
    src = open(os.path.join(ROOT, "crates", "ferrum-hip", "src", "executor.rs")).read()
    ffi = open(os.path.join(ROOT, "crates", "ferrum-hip", "src", "ffi.rs")).read()
    exported = _exported(pkg)
    used = set()
    for name in ("embed_tokens", "embedding_dim"):
        m = re.search(r"pub fn %s\b.*?\n    }\n" % name, src, flags=re.S)
        assert m, f"crates/ferrum-hip/src/executor.rs has no fn {name}"
        used |= set(re.findall(r"ffi::(\w+)", m.group(0)))
    fns = {u for u in used if u.startswith("ferrum_hip_")}
    assert {"ferrum_hip_model_embed", "ferrum_hip_model_embedding_dim"} <= fns
    assert not [u for u in fns if u not in exported]
    for u in used - fns:                                         # structs and constants: declared in the generated ffi.rs
        assert re.search(r"pub (struct|const) %s\b" % u, ffi), u
