"""C-ABI surface (no GPU needed): the library loads, exports every symbol include/ferrum_hip.h
declares, carries the native-operator descriptor, and the host-only pieces (BlockAllocator,
argument validation) behave like the reference's."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    return ge.build()


def _declared():
    text = open(os.path.join(ROOT, "include", "ferrum_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ferrum_(?:hip|native)_\w+)\s*\(", text)))


def test_every_declared_symbol_is_exported(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    declared = _declared()
    assert len(declared) > 60
    missing = [s for s in declared if s not in exported]
    assert not missing, f"declared in ferrum_hip.h but not exported: {missing}"
    # nothing CUDA-flavoured or oracle-flavoured leaks into the product
    assert not [s for s in exported if s.startswith("fo_")]


def test_native_operator_descriptor(pkg):
    # ferrum-native-ops/src/abi.rs:3-13 + resolver.rs:478-481 fixture contract
    lib = pkg.load_library()
    assert lib.ferrum_native_op_init() == 0

    class Desc(C.Structure):
        _fields_ = [("abi_version", C.c_uint32), ("operator_name", C.c_char_p), ("operator_abi_version", C.c_char_p)]
    d = C.cast(lib.ferrum_native_op_descriptor(), C.POINTER(Desc)).contents
    assert d.abi_version == 1 and d.operator_name == b"ferrum_hip_decode" and d.operator_abi_version == b"1"


def test_product_does_not_link_the_oracle(pkg):
    out = subprocess.check_output(["ldd", pkg.LIB_PATH], text=True)
    assert "oracle" not in out
    src = os.path.join(ROOT, "ferrum-infer-rs_amd")
    for dirpath, _, files in os.walk(src):
        for f in files:
            if f.endswith((".py", ".hip", ".cc", ".h")):
                assert "oracle" not in open(os.path.join(dirpath, f)).read().replace("no CPU fallback", ""), f


def test_block_allocator_rejects_out_of_range_ids_and_ref_count_overflow(pkg):
    """The reference indexes its vectors and uses checked_add (a bad id or a wrapped count panics, paged_pool.rs:333-365);
    over the C ABI the same mistakes must come back as errors and leave the allocator untouched."""
    from ferrum_infer_rs_amd.backend import BlockAllocator
    a = BlockAllocator(4)
    b0 = a.allocate()
    for bad in (4, 5, 2 ** 31):
        with pytest.raises(RuntimeError):
            a.free([b0, bad])                                    # nothing of the call is applied
        with pytest.raises(RuntimeError):
            a.acquire(bad)
        with pytest.raises(RuntimeError):
            a.register_block_hash(bad, 7)
        assert a.ref_count(bad) == 0
    assert a.ref_count(b0) == 1 and a.free_count() == 3
    for _ in range(0xFFFF - 1):
        a.acquire(b0)
    assert a.ref_count(b0) == 0xFFFF
    with pytest.raises(RuntimeError):
        a.acquire(b0)                                            # u16 count would wrap
    assert a.ref_count(b0) == 0xFFFF


def test_block_allocator_matches_reference_sequences(pkg, oracle):
    # paged_pool.rs:465-481 + randomised differential test against the oracle restatement
    from ferrum_infer_rs_amd.backend import BlockAllocator
    a = BlockAllocator(4)
    assert [a.allocate() for _ in range(4)] == [0, 1, 2, 3]
    with pytest.raises(RuntimeError):
        a.allocate()
    a.free([1, 3])
    assert a.allocate() == 3 and a.allocate() == 1
    rng = np.random.default_rng(0)
    prod, ref = BlockAllocator(64), oracle.BlockAllocator(64)
    live, hashed = [], {}
    for step in range(3000):
        op = rng.integers(0, 6)
        if op <= 1 and prod.free_count() > 0:
            x, y = prod.allocate(), ref.allocate()
            assert x == y
            live.append(x)
        elif op == 2 and live:
            k = int(rng.integers(1, min(4, len(live)) + 1))
            idx = sorted(rng.choice(len(live), size=k, replace=False), reverse=True)
            blocks = [live.pop(i) for i in idx]
            prod.free(blocks); ref.free(blocks)
        elif op == 3 and live:
            b = live[int(rng.integers(len(live)))]
            h = int(rng.integers(1, 40))
            prod.register_block_hash(b, h); ref.register_block_hash(b, h)
            hashed[h] = b
        elif op == 4:
            h = int(rng.integers(1, 40))
            x, y = prod.try_acquire_by_hash(h), ref.try_acquire_by_hash(h)
            assert x == y
            if x is not None:
                live.append(x)
        elif op == 5:
            n = int(rng.integers(0, 5))
            if n <= prod.free_count():
                x, y = prod.allocate_n(n), ref.allocate_n(n)
                assert x == y
                live.extend(x)
            else:
                with pytest.raises(RuntimeError):
                    prod.allocate_n(n)
        assert prod.free_count() == ref.free_count()
        assert prod.hash_table_size() == ref.hash_table_size()
    assert prod.peak_in_use() == ref.peak_in_use()


def test_gptq_load_rejects_unsupported_shapes(pkg):
    # capability ops signal `unsupported` (capabilities.rs:147) — checked before any device work
    from ferrum_infer_rs_amd.backend import HipBackend, Unsupported
    qw = np.zeros((8, 16), np.int32); sc = np.ones((1, 16), np.float32); qz = np.zeros((1, 2), np.int32)
    with pytest.raises(Unsupported):
        HipBackend.load_gptq(qw, sc, qz, None, None, 8, 128, 128, 16)     # bits != 4
    with pytest.raises(Unsupported):
        HipBackend.load_gptq(qw, sc, qz, None, None, 4, 64, 64, 16)       # K % 128
    with pytest.raises(Unsupported):
        HipBackend.load_gptq(qw, sc, qz, None, None, 4, 32, 128, 16)      # group 32


def test_model_create_validates_config(pkg):
    from ferrum_infer_rs_amd import HipModel
    with pytest.raises(RuntimeError):
        HipModel(num_layers=1, hidden=100, num_heads=2, num_kv_heads=1, head_dim=128, intermediate=128, vocab=64)
    with pytest.raises(RuntimeError):
        HipModel(num_layers=1, hidden=128, num_heads=3, num_kv_heads=2, head_dim=128, intermediate=128, vocab=64)


def test_block_hash_chain_matches_restatement_and_published_siphash(pkg, oracle):
    """paged_pool.rs:60-98 through the product's C ABI: same chain as the independent restatement on random prompts,
    SipHash-2-4 paper vectors through the product's own routine."""
    import struct
    lib = pkg.load_library()
    lib.ferrum_hip_siphash.restype = C.c_uint64
    lib.ferrum_hip_siphash.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_char_p, C.c_size_t]
    k0, k1 = struct.unpack("<QQ", bytes(range(16)))
    assert lib.ferrum_hip_siphash(2, 4, k0, k1, b"", 0) == 0x726FDB47DD0E0E31
    assert lib.ferrum_hip_siphash(2, 4, k0, k1, bytes(range(15)), 15) == 0xA129CA6149BE45E5
    rng = np.random.default_rng(5)
    for n in (0, 15, 16, 17, 100, 256, 1000):
        toks = rng.integers(0, 2**32 - 1, size=n, dtype=np.uint64).astype(np.uint32)
        out = np.zeros(n // 16 + 1, np.uint64)
        cnt = C.c_int()
        assert lib.ferrum_hip_block_hash_chain(toks.ctypes.data_as(C.POINTER(C.c_uint32)), n, 16,
                                               out.ctypes.data_as(C.POINTER(C.c_uint64)), len(out), C.byref(cnt)) == 0
        ref = oracle.block_hash_chain(toks, 16)
        assert cnt.value == n // 16 == len(ref) and np.array_equal(out[:cnt.value], ref)


def test_native_operator_manifest_matches_the_binary(pkg, tmp_path):
    """tools/make_manifest.py emits the reference's manifest schema (native_operator.rs:39-58); the resolver's fail-closed
    checks (resolver.rs:136-318) are reproduced here: sha256 of the file, every declared export visible to nm."""
    import hashlib
    import json
    subprocess.check_call(["python", os.path.join(ROOT, "tools", "make_manifest.py")])
    m = json.load(open(os.path.join(os.path.dirname(pkg.LIB_PATH), "native_operator_manifest.json")))
    assert m["schema_version"] == 1 and m["ferrum_native_abi_version"] == "1" and m["linkage"] == "dynamic"
    assert m["binary_sha256"] == hashlib.sha256(open(pkg.LIB_PATH, "rb").read()).hexdigest()
    assert len(m["inputs_sha256"]) == 64 and m["compute_capabilities"] == ["gfx950"]
    out = subprocess.check_output(["nm", "-g", "--defined-only", pkg.LIB_PATH], text=True)
    visible = set(line.split()[-1] for line in out.splitlines())
    assert "ferrum_native_op_init" in m["exports"] and "ferrum_native_op_descriptor" in m["exports"]
    assert all(e in visible for e in m["exports"])


def test_host_sampler_chain_matches_restatement(pkg, oracle):
    """sampler.rs:186-467 through the product's C ABI vs the independent restatement, bit for bit, on random logits with
    ties, -inf entries, repeated previous tokens and the edge parameters (k ≥ n, p outside (0,1), penalty 1, T ≤ 0)."""
    lib = pkg.load_library()
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)

    class Params(C.Structure):
        _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("repetition_penalty", C.c_float),
                    ("previous_tokens", up), ("num_previous_tokens", C.c_int32), ("greedy", C.c_int32),
                    ("random_u32", C.c_uint32), ("_pad", C.c_uint32)]
    rng = np.random.default_rng(17)
    for trial in range(60):
        n = int(rng.choice([5, 64, 1000, 4096]))
        logits = (rng.standard_normal(n) * 3).astype(np.float32)
        logits[rng.integers(0, n, size=max(1, n // 10))] = np.float32(1.5)        # ties
        if trial % 4 == 0:
            logits[rng.integers(0, n, size=n // 3)] = -np.inf
        prev = rng.integers(0, n + 3, size=int(rng.integers(0, 40))).astype(np.uint32)   # duplicates and out-of-range ids
        temp = float(rng.choice([0.0, 1.0, 0.7, 1.3]))
        k = int(rng.choice([0, 1, 5, n // 2, n, n + 7]))
        p = float(rng.choice([0.0, 0.3, 0.9, 1.0, 1.5]))
        pen = float(rng.choice([1.0, 1.2, 0.8]))
        u = int(rng.integers(0, 2**32 - 1))
        # reference order: penalty, top-k, top-p, temperature (lowest priority), then the sampler
        ref = oracle.repetition_penalty(logits, prev, pen)
        ref = oracle.top_k(ref, k) if k > 0 else ref
        ref = oracle.top_p(ref, p)
        ref = oracle.temperature(ref, temp)
        for greedy in (1, 0):
            work = logits.copy()
            prm = Params(temp, k, p, pen, prev.ctypes.data_as(up), len(prev), greedy, u, 0)
            tok = C.c_uint32()
            rc = lib.ferrum_hip_sampler_sample(work.ctypes.data_as(fp), n, C.byref(prm), C.byref(tok))
            assert np.array_equal(work, ref, equal_nan=True), trial
            if greedy:
                assert rc == 0 and tok.value == oracle.greedy_sample(ref)
            elif np.isfinite(ref).any():
                assert rc == 0 and tok.value == oracle.multinomial(ref, u), trial
            else:
                assert rc != 0                                                   # "No valid tokens for sampling"
    # greedy = last maximum, device-style argmax = first (both reference behaviours)
    tie = np.array([1.0, 7.0, 7.0, 3.0], np.float32)
    tok = C.c_uint32()
    assert lib.ferrum_hip_sampler_greedy(tie.ctypes.data_as(fp), 4, C.byref(tok)) == 0 and tok.value == 2
    assert int(oracle.argmax_rows(tie[None])[0]) == 1


def test_rust_ffi_crate_matches_the_library(pkg):
    """crates/ferrum-hip (cannot be compiled here — no Rust toolchain): src/ffi.rs is generated from
    include/ferrum_hip.h and must (a) be current, (b) declare exactly the library's exported entry points, one to one,
    and (c) every entry point the hand-written trait impls and TRAIT_MAP name must exist in the library."""
    gen = os.path.join(ROOT, "tools", "gen_ffi_rs.py")
    assert subprocess.run(["python", gen, "--check"]).returncode == 0, "ffi.rs is stale: run python tools/gen_ffi_rs.py"
    crate = os.path.join(ROOT, "crates", "ferrum-hip", "src")
    ffi = open(os.path.join(crate, "ffi.rs")).read()
    declared = re.findall(r"pub fn (ferrum_\w+)\(", ffi)
    assert len(declared) == len(set(declared))
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    exported = sorted(line.split()[-1] for line in out.splitlines() if " T " in line and line.split()[-1].startswith("ferrum_"))
    assert sorted(declared) == exported, (sorted(set(exported) - set(declared)), sorted(set(declared) - set(exported)))
    used = set()
    for f in os.listdir(crate):
        if f.endswith(".rs") and f != "ffi.rs":
            src = open(os.path.join(crate, f)).read()
            used |= set(re.findall(r"ffi::(ferrum_\w+)", src)) | set(re.findall(r'"(ferrum_hip_\w+)"', src))
    assert len(used) > 40
    assert not (used - set(exported)), sorted(used - set(exported))
    # the #[repr(C)] structs carry every field of the C structs, in order
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ferrum_hip.h")).read(), flags=re.S)
    for m in re.finditer(r"typedef struct\s*\{(.*?)\}\s*(\w+);", hdr, flags=re.S):
        names = []
        for decl in m.group(1).split(";"):
            decl = re.sub(r"\s+", " ", decl.strip())
            if decl:                                             # "int32_t a, b, c" / "const char* name": the last word of each declarator
                first, *rest = decl.split(",")
                names += [first.split()[-1].lstrip("*")] + [r.strip().lstrip("*") for r in rest]
        body = re.search(r"pub struct %s \{(.*?)\n\}" % m.group(2), ffi, flags=re.S).group(1)
        assert re.findall(r"pub (\w+):", body) == names, m.group(2)


# ── the trait impls of crates/ferrum-hip against the reference's trait signatures ───────────────────────────────────────
# tests/golden/reference_trait_methods.json: per trait, [name, number of parameters, has a default body] of every fn of
# the reference's `pub trait <trait>`, parsed out of the reference's own sources (the file each trait lives in is named).
TRAITS = os.path.join(ROOT, "tests", "golden", "reference_trait_methods.json")


def _count_params(params):
    params = re.sub(r"//[^\n]*", "", params)
    depth, n, cur = 0, 0, ""
    for ch in params:
        if ch in "([<{":
            depth += 1
        elif ch in ")]>}":
            depth -= 1
        if ch == "," and depth == 0:
            n += bool(cur.strip())
            cur = ""
        else:
            cur += ch
    return n + bool(cur.strip())


def _crate_fns():
    """name → set of parameter counts of every `fn` in crates/ferrum-hip/src (ffi.rs excluded)."""
    crate = os.path.join(ROOT, "crates", "ferrum-hip", "src")
    fns = {}
    for f in os.listdir(crate):
        if not f.endswith(".rs") or f == "ffi.rs":
            continue
        src = open(os.path.join(crate, f)).read()
        for m in re.finditer(r"\bfn (\w+)\s*(?:<[^>]*>)?\s*\(", src):
            p, depth = m.end(), 1
            while depth:
                depth += {"(": 1, ")": -1}.get(src[p], 0)
                p += 1
            fns.setdefault(m.group(1), set()).add(_count_params(src[m.end():p - 1]))
    return fns


def test_rust_crate_implements_every_required_trait_method():
    """crates/ferrum-hip cannot be compiled here (no Rust toolchain), so the next best check runs instead: the REQUIRED methods
    (no default body) of the reference's `Backend`, `BackendTimer`, `DecoderOnlyLLM` and `ModelExecutor` traits — as stored in
    tests/golden/reference_trait_methods.json — must each have an `fn` of the same name and the same number of parameters in the crate, and
    so must the defaulted methods the drop-in needs to override (paged KV, graph capture, unified forward, admission)."""
    fns = _crate_fns()
    need = {
        ("ferrum-kernels/src/backend/traits.rs", "Backend"): (),
        ("ferrum-kernels/src/backend/timer.rs", "BackendTimer"): (),
        ("ferrum-models/src/common/llm.rs", "DecoderOnlyLLM"): ("reserve_kv_slots", "kv_slot_capacity_snapshot", "unified_forward",
                                                                "unified_forward_with_logits_policy", "decode_batch"),
        ("ferrum-interfaces/src/model_executor.rs", "ModelExecutor"): ("unified_decode", "reserve_kv_slots", "kv_slot_capacity_snapshot",
                                                                       "release_cache", "supports_native_unified_decode"),
        ("ferrum-kernels/src/backend/traits.rs", "BackendPagedKv"): ("split_qkv_norm_rope_into_paged_cache_varlen", "paged_varlen_attention",
                                                                      "paged_batched_decode_attention", "paged_decode_attention"),
        ("ferrum-kernels/src/backend/capabilities.rs", "BackendGraph"): ("begin_graph_capture", "end_graph_capture", "replay_graph", "reset_graph"),
    }
    traits = json.load(open(TRAITS))
    checked = 0
    for (rel, trait), also in need.items():
        assert traits[trait]["source"] == rel, (trait, traits[trait]["source"])
        methods = [tuple(m) for m in traits[trait]["methods"]]
        required = [(n, c) for n, c, d in methods if not d]
        if trait == "Backend":
            assert len(required) == 24, (len(required), [n for n, _ in required])          # the count VERDICT r2 quotes
        wanted = required + [(n, c) for n, c, d in methods if d and n in also]
        assert set(also) <= {n for n, _, _ in methods}, (trait, set(also) - {n for n, _, _ in methods})
        for name, count in wanted:
            assert name in fns, f"{trait}::{name} has no fn in crates/ferrum-hip/src"
            assert count in fns[name], f"{trait}::{name}: the reference takes {count} parameters, the crate's fn takes {sorted(fns[name])}"
            checked += 1
    assert checked >= 45, checked


def test_elementwise_and_norm_exports_reject_null_buffers_on_the_host(pkg):
    """Return code 2 before any launch (nothing here touches a device): the five elementwise exports that used to hand a
    null pointer straight to their kernel, and the norm-family exports; a count of zero stays a no-op."""
    lib = pkg.load_library()
    f, z = C.c_float(1e-6), C.c_size_t
    one = C.c_void_p(16)                                         # never dereferenced: every call below fails its null check first
    calls = {
        "fused_silu_mul_split": lambda: lib.ferrum_hip_fused_silu_mul_split_f16(None, one, 1, 8, None),
        "fused_silu_mul_split out": lambda: lib.ferrum_hip_fused_silu_mul_split_f16(one, None, 1, 8, None),
        "fused_gelu_tanh_mul_split": lambda: lib.ferrum_hip_fused_gelu_tanh_mul_split_f16(None, one, 1, 8, None),
        "fused_gelu_tanh_mul_split out": lambda: lib.ferrum_hip_fused_gelu_tanh_mul_split_f16(one, None, 1, 8, None),
        "scale_inplace": lambda: lib.ferrum_hip_scale_inplace_f16(None, C.c_float(2.0), z(8), None),
        "add_inplace": lambda: lib.ferrum_hip_add_inplace_f16(None, one, z(8), None),
        "add_inplace x": lambda: lib.ferrum_hip_add_inplace_f16(one, None, z(8), None),
        "add_bias": lambda: lib.ferrum_hip_add_bias_f16(None, one, 1, 8, None),
        "add_bias bias": lambda: lib.ferrum_hip_add_bias_f16(one, None, 1, 8, None),
        "fused_add_rms_norm_perm": lambda: lib.ferrum_hip_fused_add_rms_norm_perm_f16(None, one, one, f, one, 1, 8, None, None),
        "embed_rms_norm": lambda: lib.ferrum_hip_embed_rms_norm_f16(one, None, C.c_float(0.0), None, None, one, f, one, 1, 8, None, 0, None, None),
        "embed_rms_norm n_zero": lambda: lib.ferrum_hip_embed_rms_norm_f16(one, one, C.c_float(0.0), None, None, one, f, one, 1, 8, None, 4, None, None),
        "gather_rms_norm": lambda: lib.ferrum_hip_gather_rms_norm_f16(one, None, one, f, one, 1, 8, None),
        "sandwich_perm": lambda: lib.ferrum_hip_sandwich_add_rms_norm_f32_perm(one, one, None, None, f, None, 1, 8, None, None),
        "sandwich_slabs": lambda: lib.ferrum_hip_sandwich_add_rms_norm_f32_slabs(None, 1, z(8), 8, one, one, None, f, None, 1, 8, None, None),
        "sandwich_slabs norm_out": lambda: lib.ferrum_hip_sandwich_add_rms_norm_f32_slabs(one, 1, z(8), 8, one, one, one, f, None, 1, 8, None, None),
        "fused_gated_act_slabs": lambda: lib.ferrum_hip_fused_gated_act_slabs_f16(None, 1, z(16), 16, one, 1, 8, 0, None),
        "gather_columns": lambda: lib.ferrum_hip_gather_columns_f16(one, None, one, 1, 8, None),
    }
    for name, call in calls.items():
        assert call() == 2, name
        assert b"null" in lib.ferrum_hip_last_error() or b"n_zero" in lib.ferrum_hip_last_error(), name
    assert lib.ferrum_hip_fused_silu_mul_split_f16(None, None, 0, 8, None) == 0
    assert lib.ferrum_hip_fused_gelu_tanh_mul_split_f16(None, None, 0, 8, None) == 0
    assert lib.ferrum_hip_scale_inplace_f16(None, C.c_float(2.0), z(0), None) == 0
    assert lib.ferrum_hip_add_inplace_f16(None, None, z(0), None) == 0
    assert lib.ferrum_hip_add_bias_f16(None, None, 0, 8, None) == 0


def test_dense_decode_exports_reject_bad_arguments_on_the_host(pkg):
    """ferrum_hip_gptq_linear_slabs_f16 / _forward_fused_tail_f16 / _can_fuse_tail: null buffers, an unknown form and
    residual_in == residual_out come back as 2 before the handle is read or anything is launched."""
    lib = pkg.load_library()
    one, two = C.c_void_p(16), C.c_void_p(32)                    # never dereferenced: every call below fails a check first
    s, rp, npad = C.c_int(1), C.c_int(0), C.c_int(0)
    geo = (C.byref(s), C.byref(rp), C.byref(npad))
    z, f = C.c_size_t(1 << 20), C.c_float(1e-6)
    slabs = lambda h, x, sl, form, g=geo: lib.ferrum_hip_gptq_linear_slabs_f16(h, x, sl, z, 1, form, *g, None)
    tail = lambda h, d, w, ri, ro, ln, out: lib.ferrum_hip_gptq_linear_forward_fused_tail_f16(h, d, w, ri, ro, ln, f, 2, out, 1, None, None)
    calls = {
        "slabs handle": (lambda: slabs(None, one, one, 0), b"null"),
        "slabs x": (lambda: slabs(one, None, one, 0), b"null"),
        "slabs buffer": (lambda: slabs(one, one, None, 1), b"null"),
        "slabs S": (lambda: slabs(one, one, one, 0, (None, C.byref(rp), C.byref(npad))), b"null"),
        "slabs rows_pad": (lambda: slabs(one, one, one, 2, (C.byref(s), None, C.byref(npad))), b"null"),
        "slabs form 3": (lambda: slabs(one, one, one, 3), b"unknown form"),
        "slabs form -1": (lambda: slabs(one, one, one, -1), b"unknown form"),
        "tail handle": (lambda: tail(None, one, one, one, two, one, one), b"null"),
        "tail down": (lambda: tail(one, None, one, one, two, one, one), b"null"),
        "tail weights": (lambda: tail(one, one, None, one, two, one, one), b"null"),
        "tail residual_in": (lambda: tail(one, one, one, None, two, one, one), b"null"),
        "tail residual_out": (lambda: tail(one, one, one, one, None, one, one), b"null"),
        "tail ln_w": (lambda: tail(one, one, one, one, two, None, one), b"null"),
        "tail out": (lambda: tail(one, one, one, one, two, one, None), b"null"),
        "tail in-place residual": (lambda: tail(one, one, one, one, one, one, one), b"residual_in == residual_out"),
    }
    for name, (call, word) in calls.items():
        assert call() == 2, name
        assert word in lib.ferrum_hip_last_error(), (name, lib.ferrum_hip_last_error())
    assert lib.ferrum_hip_gptq_linear_can_fuse_tail(None, 1) == 0


# ── the op-level decode-chain entry: symbols, the shape predicate and the capacity checks, all on the host ─────────────────
def _chain_shape(be, H=2048, nq=32, nkv=4, T=4, E=128, Q=4, r_top_k=8, attn_splits=1, group=128, **kw):
    """A descriptor over weightless handles with every buffer the form touches at a fake, aligned, never-dereferenced address and
    exactly the capacity the launch needs (restated here from the roles' index ranges, not read from the library)."""
    qkv = be.gptq_shape_only(group, H, (nq + 2 * nkv) * 128)
    o = be.gptq_shape_only(group, nq * 128, H)
    f = dict(T=T, H=H, nq=nq, nkv=nkv, E=E, Q=Q, r_top_k=r_top_k, attn_splits=attn_splits, has_a=1, top_k=8, eps=1e-6, qk_mode=1,
             max_blocks=5, sliding_window=0, norm_topk=1, defer_merge=0, a_S=0, a_ld=0, a_slab_stride=0)
    dense_form = kw.pop("dense_form", "rows")
    f.update(kw)
    T, H, E, Q = f["T"], f["H"], f["E"], f["Q"]
    words = be.decode_chain_counter_words()
    row = T * H * 2
    need = dict(res_in=row, ln_in=H * 2, res_a=row, norm1=row, qkv_out=T * (nq + 2 * nkv) * 128 * 2, q_norm_w=256, k_norm_w=256,
                cos_t=256, sin_t=256, k_pool=nkv * 4096, v_pool=nkv * 4096, block_tables=T * f["max_blocks"] * 4, kv_lens=T * 4,
                attn_out=T * nq * 256, o_part=2 * T * H * 4, res_b_out=row, post_ln=H * 2, norm2=row, cnt=words * 4, cnt_next=words * 4,
                timeout=4)
    if E > 0:
        need.update(down=T * f["top_k"] * H * 2, comb_w=T * f["top_k"] * 4, router_w=(E + 15) // 16 * 16 * H * 2)
        need.update(dict(cand=T * Q * 64, stats=T * Q * 8) if f["defer_merge"] else dict(ids=T * f["r_top_k"] * 4, weights=T * f["r_top_k"] * 4))
    elif dense_form == "rows":
        need.update(a_x=row)
    else:
        f.update(a_S=3, a_ld=H + 64, a_slab_stride=T * (H + 64) + 32)
        need.update(a_slabs=(2 * f["a_slab_stride"] + (T - 1) * f["a_ld"] + H) * 4)
    if f["attn_splits"] > 1:
        need.update(attn_partial=T * nkv * f["attn_splits"] * 16 * 132 * 4, attn_tickets=T * nkv * 4)
    bufs = {n: (0x10000 * (i + 1), b) for i, (n, b) in enumerate(sorted(need.items()))}
    return (qkv, o), f, bufs


def test_decode_chain_entry_symbols_and_struct_order(pkg):
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.LIB_PATH], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert {"ferrum_hip_decode_chain_f16", "ferrum_hip_decode_chain_supports", "ferrum_hip_decode_chain_counter_words"} <= exported
    from ferrum_infer_rs_amd import backend as be
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ferrum_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct\s*\{([^}]*)\}\s*FerrumHipDecodeChainDesc;", hdr).group(1)
    names = []
    for decl in body.split(";"):
        decl = re.sub(r"\s+", " ", decl.strip())
        if decl:
            first, *rest = decl.split(",")
            names += [first.split()[-1]] + [r.strip() for r in rest]
    assert [n for n, _ in be.DecodeChainDesc._fields_] == names                # the ctypes mirror follows the header
    # 56 line slots of 64 words + 16 kv heads × 4 replicas, and the route granules of 128 tokens × 4 parts × 10 × 2 words
    assert be.decode_chain_counter_words() == (56 + 4 * 16) * 64 + 128 * 4 * 10 * 2


def test_decode_chain_supports_answers_by_shape(pkg):
    """ferrum_hip_decode_chain_supports over weightless handles (nothing touches a device): the table of the shapes the chain
    takes and refuses, as decode_chain_supports (csrc/chain.hip) states them."""
    from ferrum_infer_rs_amd import backend as be
    table = {
        "H 2048 MoE": (dict(), True),
        "H 4096 MoE": (dict(H=4096), True),
        "H 4096 dense": (dict(H=4096, nkv=8, E=0, Q=1), True),
        "H 2048 nkv 16": (dict(nkv=16), True),
        "T 128": (dict(T=128), True),
        "T 129": (dict(T=129), False),
        "H 1024": (dict(H=1024), False),
        "H 8192": (dict(H=8192), False),
        "nq 16": (dict(nq=16), False),
        "nq 64": (dict(nq=64, nkv=8), False),
        "GQA group 16": (dict(nkv=2), False),
        "head_dim 64": (dict(head_dim=64), False),
        "E 60 Q 4": (dict(E=60, Q=4, r_top_k=4), True),
        "E 24 Q 2": (dict(E=24, Q=2, r_top_k=4), True),
        "E 128 Q 3 (8 tiles)": (dict(E=128, Q=3), False),
        "E 48 Q 2 (3 tiles)": (dict(E=48, Q=2), False),
        "E 128 Q 5": (dict(E=128, Q=5), False),
        "r_top_k 9": (dict(r_top_k=9), False),
        "dense Q 2": (dict(E=0, Q=2), False),
        "attn_splits 16": (dict(attn_splits=16), True),
        "attn_splits 17": (dict(attn_splits=17), False),
        "group 256": (dict(group=256), True),                   # (the packed layout is in 128-wide groups whatever the checkpoint's)
    }
    for name, (kw, want) in table.items():
        hs, f, bufs = _chain_shape(be, **kw)
        assert be.decode_chain_supports(be.decode_chain_desc(*hs, **f, **bufs)) == want, name
    hs, f, bufs = _chain_shape(be, attn_splits=5)
    assert be.decode_chain_supports(be.decode_chain_desc(*hs, **f, **bufs))
    for missing in ("attn_partial", "attn_tickets", "o_part"):
        assert not be.decode_chain_supports(be.decode_chain_desc(*hs, **f, **{k: v for k, v in bufs.items() if k != missing})), missing
    d = be.decode_chain_desc(*hs, **f, **bufs)
    d.qkv = None
    assert not be.decode_chain_supports(d)
    hs2, _, _ = _chain_shape(be, H=4096)
    assert not be.decode_chain_supports(be.decode_chain_desc(hs2[0], hs[1], **f, **bufs))      # q|k|v of another hidden size


def test_decode_chain_entry_refuses_short_buffers_before_any_launch(pkg):
    """Per form, every buffer the launch touches: one byte short, null, or misaligned → FERRUM_HIP_INVALID naming the buffer.
    With exactly the needed capacities every check passes and the call stops at the weightless handles — the pointers here are
    fake, so reaching a launch (or the device read-back of kv_lens) is not survivable: the order of the checks is under test."""
    from ferrum_infer_rs_amd import backend as be
    lib = pkg.load_library()
    forms = {
        "moe merged": dict(),
        "moe deferred, 5 ranges": dict(defer_merge=1, attn_splits=5, T=3),
        "moe H 4096 top_k 10": dict(H=4096, top_k=10, T=17),
        "moe no tail, no rope": dict(has_a=0, qk_mode=0),
        "dense rows": dict(H=4096, nkv=8, E=0, Q=1, qk_mode=2),
        "dense slabs": dict(H=4096, nkv=8, E=0, Q=1, dense_form="slabs", T=33),
    }
    call = lambda d: lib.ferrum_hip_decode_chain_f16(C.byref(d), None)
    checked = 0
    for form, kw in forms.items():
        hs, f, bufs = _chain_shape(be, **kw)
        if not f["has_a"]:
            bufs = {k: v for k, v in bufs.items() if k not in ("down", "comb_w", "res_in", "ln_in")}
        if f["qk_mode"] != 1:
            bufs = {k: v for k, v in bufs.items() if k not in ("q_norm_w", "k_norm_w")}
        if f["qk_mode"] == 0:
            bufs = {k: v for k, v in bufs.items() if k not in ("cos_t", "sin_t")}
        assert call(be.decode_chain_desc(*hs, **f, **bufs)) == 2, form
        assert b"shape-only handle" in lib.ferrum_hip_last_error(), (form, lib.ferrum_hip_last_error())
        for name, (ptr, nbytes) in bufs.items():
            for what, bad in (("holds", (ptr, nbytes - 1)), ("null", (0, nbytes)), ("aligned", (ptr + 2, nbytes))):
                if name in ("o_part", "attn_partial", "attn_tickets", "a_x", "a_slabs") and what == "null":
                    continue                                  # (nulls the shape predicate itself refuses — rc 3; a null a_x selects the slab form)
                assert call(be.decode_chain_desc(*hs, **f, **{**bufs, name: bad})) == 2, (form, name, what)
                err = lib.ferrum_hip_last_error()
                assert name.encode() in err and what.encode() in err, (form, name, what, err)
                checked += 1
    assert checked > 300
    hs, f, bufs = _chain_shape(be)
    assert call(be.decode_chain_desc(*hs, **f, **{**bufs, "cnt_next": bufs["cnt"]})) == 2 and b"cnt == cnt_next" in lib.ferrum_hip_last_error()
    assert call(be.decode_chain_desc(*hs, **{**f, "H": 1024}, **bufs)) == 3
    assert call(be.decode_chain_desc(*hs, **{**f, "qk_mode": 4}, **bufs)) == 2
    assert lib.ferrum_hip_decode_chain_f16(None, None) == 2


def test_weightless_handle_is_refused_by_every_computing_entry(pkg):
    """A ferrum_hip_gptq_shape_only handle carries dims and no weights: every GPTQ entry that would launch — the single-projection
    ones and every expert-stack phase — returns FERRUM_HIP_INVALID naming the reason, before anything else is read (the other
    pointers here are fake and never dereferenced); can_fuse_tail answers 0, info answers the dims."""
    from ferrum_infer_rs_amd import backend as be
    lib = pkg.load_library()
    lin, lin2 = be.gptq_shape_only(128, 2048, 512), be.gptq_shape_only(128, 256, 2048)      # (they free their handles when they go)
    h, h2 = lin.handle, lin2.handle
    one, two = C.c_void_p(4096), C.c_void_p(8192)
    s, rp, npad = C.c_int(1), C.c_int(0), C.c_int(0)
    f = C.c_float(1e-6)
    calls = {
        "gptq_linear_forward": lambda: lib.ferrum_hip_gptq_linear_forward_f16(h, one, one, 1, None, None),
        "gptq_linear_slabs": lambda: lib.ferrum_hip_gptq_linear_slabs_f16(h, one, one, C.c_size_t(1 << 20), 1, 0, C.byref(s), C.byref(rp), C.byref(npad), None),
        "gptq_linear_forward_fused_tail": lambda: lib.ferrum_hip_gptq_linear_forward_fused_tail_f16(h, one, one, one, two, one, f, 2, one, 1, None, None),
        "moe_gemm_phase": lambda: lib.ferrum_hip_moe_gemm_phase_f16(h, one, one, one, one, one, 8, 16, 2, 4, 0, None),
        "moe_gemm_phase_inline_align": lambda: lib.ferrum_hip_moe_gemm_phase_inline_align_f16(h, one, one, one, 8, 4, 2, 4, 0, None),
        "moe_gemm_phase_expert_major": lambda: lib.ferrum_hip_moe_gemm_phase_expert_major_f16(h, one, one, one, 8, 4, 2, 0, None),
        "moe_gemm_phase_expert_major_pair": lambda: lib.ferrum_hip_moe_gemm_phase_expert_major_pair_f16(h, h2, one, one, one, one, 8, 4, 2, None),
        "merge_route": lambda: lib.ferrum_hip_moe_gemm_phase_merge_route_f16(h, one, one, one, one, 4, 2, 2, 1, 32, 4, 0, one, one, one, one, one, None),
        "gemm_phase_batched": lambda: lib.ferrum_hip_moe_gemm_phase_batched_f16(h, one, one, 1, one, 2048, 0, None),
    }
    for name, call in calls.items():
        assert call() == 2, name
        err = lib.ferrum_hip_last_error()
        assert name.encode() in err and b"carries no weights" in err, (name, err)
    assert lib.ferrum_hip_gptq_linear_can_fuse_tail(h, 1) == 0
    k, n, e = C.c_int(), C.c_int(), C.c_int()
    assert lib.ferrum_hip_gptq_info(h, C.byref(k), C.byref(n), C.byref(e), None) == 0 and (k.value, n.value, e.value) == (2048, 512, 0)
