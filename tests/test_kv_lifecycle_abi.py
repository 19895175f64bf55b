"""Sequence KV lifecycle over the C ABI (no GPU): truncate_kv, fork and the host swap trio are declared in
include/ferrum_hip.h, exported by the library, refuse a null model with an error text, and the Rust view of the header is current."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIFECYCLE = ("ferrum_hip_model_truncate_kv", "ferrum_hip_model_fork", "ferrum_hip_model_kv_swap_bytes",
             "ferrum_hip_model_kv_swap_out", "ferrum_hip_model_kv_swap_in")
SUPPORT = ("ferrum_hip_kv_move_blocks", "ferrum_hip_model_block_info")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


def test_lifecycle_entry_points_are_declared_and_exported(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ferrum_hip.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    for name in LIFECYCLE + SUPPORT:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), f"{name} is not declared in ferrum_hip.h"
        assert name in exported, f"{name} is not exported by the library"


def test_lifecycle_calls_refuse_a_null_model_with_a_message(pkg):
    lib = pkg.load_library()
    buf = (C.c_uint8 * 64)()
    n = C.c_size_t()
    calls = {
        "ferrum_hip_model_truncate_kv": lambda f: f(None, C.c_uint64(1), 0),
        "ferrum_hip_model_fork": lambda f: f(None, C.c_uint64(1), C.c_uint64(2)),
        "ferrum_hip_model_kv_swap_bytes": lambda f: f(None, C.c_uint64(1), C.byref(n)),
        "ferrum_hip_model_kv_swap_out": lambda f: f(None, C.c_uint64(1), buf, C.c_size_t(64), C.byref(n)),
        "ferrum_hip_model_kv_swap_in": lambda f: f(None, C.c_uint64(1), buf, C.c_size_t(64)),
        "ferrum_hip_model_block_info": lambda f: f(None, C.c_uint32(0), None, None),
    }
    assert set(LIFECYCLE) <= set(calls)
    for name, call in calls.items():
        rc = call(getattr(lib, name))
        msg = lib.ferrum_hip_last_error().decode()
        assert rc != 0, name
        assert name.replace("ferrum_hip_", "") in msg, (name, msg)  # the text is this call's own


def test_kv_move_launcher_validates_before_it_launches(pkg):
    """Argument errors of the op-level move come back before any device work (this runs without a GPU)."""
    lib = pkg.load_library()
    f = lib.ferrum_hip_kv_move_blocks
    one = C.c_void_p(16)                                             # non-null, aligned, never dereferenced on these paths
    assert f(one, 2, one, 0, None, C.c_size_t(2048), 4, 0, None) == 0            # nothing to move
    for args in ((None, 2, one, 1, None, C.c_size_t(2048), 4, 0, None),          # no pools
                 (one, 2, None, 1, None, C.c_size_t(2048), 4, 0, None),          # no pairs
                 (one, 2, one, 1, None, C.c_size_t(2048), 4, 3, None),           # unknown mode
                 (one, 2, one, 1, None, C.c_size_t(2048), 4, 1, None),           # gather without staging
                 (one, 2, one, 1, C.c_void_p(24), C.c_size_t(2048), 4, 2, None), # misaligned staging
                 (one, 0, one, 1, None, C.c_size_t(2048), 4, 0, None),           # no pool count
                 (one, 70000, one, 1, None, C.c_size_t(2048), 4, 0, None),       # beyond the grid's second dimension
                 (one, 2, one, 1, None, C.c_size_t(2040), 4, 0, None),           # chunk not in 16-byte vectors
                 (one, 2, one, 1, None, C.c_size_t(2048), 0, 0, None)):          # empty pool
        assert f(*args) == 2, args
        assert "kv_move" in lib.ferrum_hip_last_error().decode()


def test_rust_ffi_view_is_current_and_binds_the_lifecycle(pkg):
    gen = os.path.join(ROOT, "tools", "gen_ffi_rs.py")
    assert subprocess.run(["python", gen, "--check"]).returncode == 0, "ffi.rs is stale: run python tools/gen_ffi_rs.py"
    crate = os.path.join(ROOT, "crates", "ferrum-hip", "src")
    ffi = open(os.path.join(crate, "ffi.rs")).read()
    for name in LIFECYCLE + SUPPORT:
        assert re.search(r"pub fn %s\(" % name, ffi), name
    ex = open(os.path.join(crate, "executor.rs")).read()
    assert "ffi::ferrum_hip_model_truncate_kv" in ex
    # the trait's default forward_verify starts at position 0 (common/llm.rs:207-216): the model must bring its own
    assert re.search(r"fn forward_verify\(&mut self, cache_id: &str, tokens: &\[u32\]\) -> Vec<f32>", ex)
    assert re.search(r"fn truncate_kv\(&mut self, cache_id: &str, new_len: usize\)", ex)
