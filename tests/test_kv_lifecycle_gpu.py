"""Sequence KV lifecycle on the device: host swap round trip, copy-on-write fork, truncate_kv and the privatising copy that keeps
a truncate from corrupting sharers — plus the move kernel (kv_move.hip) on its own, chunk by chunk.

Everything the lifecycle calls do is copying, so every check of what they moved is bit-exact (`np.array_equal` on `read_kv`);
what a forward computes afterwards is held against an uninterrupted oracle sequence with `Parity` at its default bounds.
Tiny dense model (2 layers, hidden 256, vocab 512, 64 KV blocks); the copy-sensitive tests run at (nkv 1, hd 64) — a 2 KiB
chunk, half of one 256-lane × 16-byte pass, the case the kernel's tail guard exists for — and at (nkv 2, hd 128)."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VOCAB, LAYERS, KV_BLOCKS = 512, 2, 64
DIMS = [(1, 64), (2, 128)]
_TM, _OM = {}, {}


@pytest.fixture(scope="module")
def pkg():
    import torch
    import __graft_entry__ as ge
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    p = ge.load_package()
    p.load_library()
    return p


@pytest.fixture(scope="module", autouse=True)
def _drop_oracle_models():
    """The cached oracle models go before the interpreter starts tearing modules down."""
    yield
    _OM.clear()


def _tiny(nkv, hd):
    from tests import modelgen
    if (nkv, hd) not in _TM:
        _TM[(nkv, hd)] = modelgen.TinyModel(False, layers=LAYERS, hidden=256, nq=4, nkv=nkv, hd=hd, vocab=VOCAB, seed=31 + hd)
    return _TM[(nkv, hd)]


def _oracle_model(nkv, hd):
    """One oracle model per shape for the whole module; every test releases the cache ids it used."""
    if (nkv, hd) not in _OM:
        _OM[(nkv, hd)] = _tiny(nkv, hd).oracle_model()
    return _OM[(nkv, hd)]


def _hip(pkg, nkv, hd):
    return _tiny(nkv, hd).hip_model(pkg, kv_num_blocks=KV_BLOCKS)


def _prompt(n, seed):
    return np.random.default_rng(seed).integers(0, VOCAB, size=n).astype(np.uint32)


def _kv(hm, sid):
    return [hm.read_kv(sid, l, v) for l in range(LAYERS) for v in (0, 1)]


def _same_kv(a, b, upto=None):
    return all(np.array_equal(x[:upto], y[:upto]) for x, y in zip(a, b))


def _free(hm):
    return hm.kv_slot_capacity_snapshot()["free_blocks"]


def _exhaust(hm, leave=0):
    """Reserve all but `leave` free blocks under throw-away sequence ids; returns them (release to give the blocks back)."""
    sids, sid = [], 10_000
    while _free(hm) > leave:
        hm.reserve_kv_slots([(sid, min(_free(hm) - leave, 16) * 16)])
        sids.append(sid)
        sid += 1
    return sids


def _parity(case):
    from tests import modelgen
    return modelgen.Parity(case)


def _check_row(par, tag, o_logits, g_logits, g_tok):
    assert np.isfinite(g_logits).all(), f"{par.case} {tag}: non-finite logits"
    par.check(tag, o_logits, g_logits, g_tok)


# ── 1. swap round trip ────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("nkv,hd", DIMS)
@pytest.mark.parametrize("final_len", [15, 16, 17, 37])
def test_swap_round_trip_is_bit_exact_and_decoding_continues(pkg, oracle, nkv, hd, final_len):
    A, B = 1, 2
    prompt = _prompt(final_len - 3, 100 + final_len)
    om = _oracle_model(nkv, hd)

    def start(hm):
        toks, _ = hm.unified_forward([(A, prompt, 0, True)], greedy=True)
        ids = hm.decode_steps([A], [toks[0]], 3)
        return [int(toks[0])] + [int(t) for t in ids[:, 0]]          # fed: [0], [1], [2]; [3] is the next input

    hm = _hip(pkg, nkv, hd)
    free0 = _free(hm)
    chain = start(hm)
    old_table, kv_len = hm.block_table(A)
    assert kv_len == final_len
    snap = _kv(hm, A)
    need = hm.swap_bytes(A)
    chunk = nkv * 16 * hd * 2
    assert need == 32 + -(-final_len // 16) * LAYERS * 2 * chunk
    buf = hm.swap_out(A)
    assert len(buf) == need
    assert struct.unpack("<8I", buf[:32])[2:] == (LAYERS, nkv, hd, 16, final_len, -(-final_len // 16))
    with pytest.raises(RuntimeError):
        hm.block_table(A)                                             # A is unknown now …
    assert _free(hm) == free0                                         # … and every block it held or had reserved is back
    # B takes A's old ids (the free list is LIFO) and overwrites them
    hm.unified_forward([(B, _prompt(final_len, 7), 0, True)], greedy=True)
    assert set(hm.block_table(B)[0]) & set(old_table)
    hm.swap_in(A, buf)
    new_table, new_len = hm.block_table(A)
    assert new_len == final_len and len(new_table) == -(-final_len // 16) and new_table != old_table[:len(new_table)]
    assert not set(new_table) & set(hm.block_table(B)[0])
    assert all(hm.block_info(b) == (1, False) for b in new_table)     # private, unhashed
    assert _same_kv(_kv(hm, A), snap)
    # 4 more steps: logits against an oracle sequence that never left, ids against a model that was never swapped
    o_last = om.forward(0, prompt, 0)
    for i, t in enumerate(chain[:3]):
        o_last = om.forward(0, np.array([t], np.uint32), len(prompt) + i)
    par = _parity(f"swap-nkv{nkv}-hd{hd}-len{final_len}")
    tok, got = chain[3], []
    for s in range(4):
        o_last = om.forward(0, np.array([tok], np.uint32), final_len + s)
        g_tok, g_logits = hm.unified_forward([(A, [tok], final_len + s, True)], greedy=True, want_logits=True)
        _check_row(par, f"step{s}", o_last, g_logits[0], g_tok[0])
        tok = int(g_tok[0])
        got.append(tok)
    om.release(0)
    par.finish()
    control = _hip(pkg, nkv, hd)
    assert start(control) == chain
    assert [int(t) for t in control.decode_steps([A], [chain[3]], 4)[:, 0]] == got


def test_swap_refusals_leave_the_model_untouched(pkg):
    nkv, hd = DIMS[0]
    A, B = 1, 2
    hm = _hip(pkg, nkv, hd)
    hm.unified_forward([(A, _prompt(37, 1), 0, True)], greedy=True)
    hm.unified_forward([(B, _prompt(17, 2), 0, True)], greedy=True)

    def state():
        return _free(hm), hm.block_table(A), hm.block_table(B), [hm.block_info(b) for b in range(KV_BLOCKS)]

    before, snap = state(), _kv(hm, A)
    with pytest.raises(RuntimeError, match="needs"):
        hm.swap_out(A, capacity=hm.swap_bytes(A) - 1)                 # short capacity: fails before anything moves
    with pytest.raises(RuntimeError):
        hm.swap_bytes(99)                                             # unknown sequence
    assert state() == before and _same_kv(_kv(hm, A), snap)
    other = _hip(pkg, *DIMS[1])                                       # a buffer written by a model with another head_dim
    other.unified_forward([(A, _prompt(5, 3), 0, True)], greedy=True)
    foreign = other.swap_out(A)
    with pytest.raises(RuntimeError, match="head_dim"):
        hm.swap_in(7, foreign)
    buf = hm.swap_out(A)
    after_out = (_free(hm), hm.block_table(B))
    with pytest.raises(RuntimeError, match="exists"):
        hm.swap_in(B, buf)                                            # the id is taken
    with pytest.raises(RuntimeError):
        hm.swap_in(A, buf[:-16])                                      # byte count does not match the header
    with pytest.raises(RuntimeError):
        hm.swap_in(A, b"\0" * 32)                                     # no magic
    filler = _exhaust(hm, leave=2)                                    # 2 blocks free, A needs 3
    assert _free(hm) == 2
    with pytest.raises(RuntimeError, match="exhausted"):
        hm.swap_in(A, buf)
    assert _free(hm) == 2
    for s in filler:
        hm.release(s)
    assert (_free(hm), hm.block_table(B)) == after_out
    hm.swap_in(A, buf)
    assert _same_kv(_kv(hm, A), snap)


# ── 2. fork ───────────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("nkv,hd", DIMS)
def test_fork_shares_full_blocks_and_isolates_the_tail(pkg, oracle, nkv, hd):
    A, B, n = 1, 2, 37
    prompt = _prompt(n, 11)
    om = _oracle_model(nkv, hd)
    hm = _hip(pkg, nkv, hd)
    toks, _ = hm.unified_forward([(A, prompt, 0, True)], greedy=True)
    free1 = _free(hm)
    hm.fork(A, B)
    ta, tb = hm.block_table(A), hm.block_table(B)
    assert ta[1] == tb[1] == n and len(tb[0]) == 3
    assert ta[0][:2] == tb[0][:2] and ta[0][2] != tb[0][2]
    assert [hm.block_info(b)[0] for b in tb[0]] == [2, 2, 1] and hm.block_info(ta[0][2])[0] == 1
    assert _free(hm) == free1 - 1
    assert _same_kv(_kv(hm, A), _kv(hm, B))
    # the same token through A alone and through B alone: the same bits
    t0 = int(toks[0])
    ga = hm.unified_forward([(A, [t0], n, True)], greedy=True, want_logits=True)
    gb = hm.unified_forward([(B, [t0], n, True)], greedy=True, want_logits=True)
    assert np.isfinite(ga[1]).all() and np.array_equal(ga[1], gb[1]) and ga[0][0] == gb[0][0]
    snap = _kv(hm, A)
    # then they part: different tokens, one batch, each against its own oracle sequence (the oracle replays the prefix)
    for c in (0, 1):
        om.forward(c, prompt, 0)
        om.forward(c, np.array([t0], np.uint32), n)
    pa, pb_ = _parity(f"fork-A-nkv{nkv}-hd{hd}"), _parity(f"fork-B-nkv{nkv}-hd{hd}")
    tok_a, tok_b = int(ga[0][0]), (int(ga[0][0]) + 101) % VOCAB
    for s in range(3):
        pos = n + 1 + s
        oa = om.forward(0, np.array([tok_a], np.uint32), pos)
        ob = om.forward(1, np.array([tok_b], np.uint32), pos)
        g_tok, g_logits = hm.unified_forward([(A, [tok_a], pos, True), (B, [tok_b], pos, True)], greedy=True, want_logits=True)
        _check_row(pa, f"step{s}", oa, g_logits[0], g_tok[0])
        _check_row(pb_, f"step{s}", ob, g_logits[1], g_tok[1])
        tok_a, tok_b = int(g_tok[0]), (int(g_tok[1]) + 101) % VOCAB
    om.release(0)
    om.release(1)
    pa.finish()
    pb_.finish()
    kva, kvb = _kv(hm, A), _kv(hm, B)
    assert _same_kv(kva, snap, upto=n + 1), "B's writes (or A's own) changed A's prefix"
    assert _same_kv(kvb, snap, upto=n + 1)
    assert not _same_kv(kva, kvb)                                      # the tails did diverge
    # releasing A keeps B whole
    hm.release(A)
    assert [hm.block_info(b)[0] for b in hm.block_table(B)[0]] == [1, 1, 1]
    assert _same_kv(_kv(hm, B), kvb)
    g_tok, g_logits = hm.unified_forward([(B, [tok_b], n + 4, True)], greedy=True, want_logits=True)
    assert np.isfinite(g_logits).all()


def test_fork_block_accounting_at_the_edges(pkg):
    nkv, hd = DIMS[0]
    A, B, C_, D = 1, 2, 3, 4
    hm = _hip(pkg, nkv, hd)
    hm.unified_forward([(A, _prompt(32, 5), 0, True)], greedy=True)
    hm.reserve_kv_slots([(A, 70)])                                    # reserved, unwritten blocks are not inherited
    free1 = _free(hm)
    hm.fork(A, B)
    assert _free(hm) == free1                                         # len % 16 == 0: nothing allocated, nothing copied
    assert hm.block_table(B) == (hm.block_table(A)[0][:2], 32) and len(hm.block_table(A)[0]) == 5
    assert [hm.block_info(b)[0] for b in hm.block_table(A)[0]] == [2, 2, 1, 1, 1]
    with pytest.raises(RuntimeError, match="exists"):
        hm.fork(A, B)
    with pytest.raises(RuntimeError):
        hm.fork(77, 78)                                               # unknown source
    hm.reserve_kv_slots([(D, 16)])
    with pytest.raises(RuntimeError):
        hm.fork(D, 78)                                                # empty source
    # an empty pool: a fork that needs a block for the partial tail fails and changes no count
    hm.unified_forward([(C_, _prompt(21, 6), 0, True)], greedy=True)
    filler = _exhaust(hm)
    counts = [hm.block_info(b) for b in range(KV_BLOCKS)]
    with pytest.raises(RuntimeError, match="no free block"):
        hm.fork(C_, 78)
    assert [hm.block_info(b) for b in range(KV_BLOCKS)] == counts and _free(hm) == 0
    with pytest.raises(RuntimeError):
        hm.block_table(78)
    hm.fork(A, 79)                                                    # whole blocks only: still possible
    assert [hm.block_info(b)[0] for b in hm.block_table(79)[0]] == [3, 3]
    for s in filler:
        hm.release(s)


# ── 3. truncate ───────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("nkv,hd", DIMS)
def test_truncate_rolls_back_and_the_next_forward_continues_there(pkg, oracle, nkv, hd):
    A, n = 1, 37
    prompt = _prompt(n, 21)
    new = _prompt(5, 22)
    om = _oracle_model(nkv, hd)
    hm = _hip(pkg, nkv, hd)
    free0 = _free(hm)
    hm.unified_forward([(A, prompt, 0, True)], greedy=True)
    snap = _kv(hm, A)
    state = (hm.block_table(A), _free(hm))
    for keep in (n, n + 5):                                           # new_len ≥ len changes nothing
        hm.truncate_kv(A, keep)
        assert (hm.block_table(A), _free(hm)) == state
    with pytest.raises(RuntimeError):
        hm.truncate_kv(55, 3)                                         # unknown sequence
    with pytest.raises(RuntimeError):
        hm.truncate_kv(A, -1)
    assert (hm.block_table(A), _free(hm)) == state
    par = _parity(f"truncate-nkv{nkv}-hd{hd}")
    # 37 → 21: the third block goes back; five other tokens at pos_offset 21
    hm.truncate_kv(A, 21)
    assert hm.block_table(A) == (state[0][0][:2], 21) and _free(hm) == state[1] + 1
    assert _same_kv(_kv(hm, A), snap, upto=21)
    g_tok, g_logits = hm.unified_forward([(A, new, 21, True)], greedy=True, want_logits=True)
    _check_row(par, "21+5", om.forward(0, np.concatenate([prompt[:21], new]), 0), g_logits[0], g_tok[0])
    om.release(0)
    assert _same_kv(_kv(hm, A), snap, upto=21)
    # 37 → 32: a cut on a block edge; one token at 32
    hm.truncate_kv(A, 0)
    assert hm.block_table(A) == ([], 0) and _free(hm) == free0
    hm.unified_forward([(A, prompt, 0, True)], greedy=True)
    hm.truncate_kv(A, 32)
    assert hm.block_table(A)[1] == 32 and len(hm.block_table(A)[0]) == 2 and _free(hm) == free0 - 2
    g_tok, g_logits = hm.unified_forward([(A, new[:1], 32, True)], greedy=True, want_logits=True)
    _check_row(par, "32+1", om.forward(0, np.concatenate([prompt[:32], new[:1]]), 0), g_logits[0], g_tok[0])
    om.release(0)
    # → 0, then the whole prompt again from position 0
    hm.truncate_kv(A, 0)
    assert hm.block_table(A) == ([], 0) and _free(hm) == free0
    g_tok, g_logits = hm.unified_forward([(A, prompt, 0, True)], greedy=True, want_logits=True)
    _check_row(par, "0+37", om.forward(0, prompt, 0), g_logits[0], g_tok[0])
    om.release(0)
    par.finish()
    # blocks reserved ahead of the length go back too
    hm.reserve_kv_slots([(A, 80)])
    assert len(hm.block_table(A)[0]) == 5 and _free(hm) == free0 - 5
    hm.truncate_kv(A, 36)
    assert hm.block_table(A)[1] == 36 and len(hm.block_table(A)[0]) == 3 and _free(hm) == free0 - 3


# ── 4. truncate must not corrupt sharers ──────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("nkv,hd", DIMS)
def test_truncate_inside_a_forked_block_leaves_the_fork_alone(pkg, oracle, nkv, hd):
    A, B, n = 1, 2, 37
    prompt, new = _prompt(n, 31), _prompt(6, 32)
    om = _oracle_model(nkv, hd)
    hm = _hip(pkg, nkv, hd)
    hm.unified_forward([(A, prompt, 0, True)], greedy=True)
    hm.fork(A, B)
    snap_b, table_b = _kv(hm, B), hm.block_table(B)
    free1 = _free(hm)
    hm.truncate_kv(A, 20)                                             # inside shared block 1
    ta = hm.block_table(A)
    assert ta[1] == 20 and len(ta[0]) == 2
    assert ta[0][0] == table_b[0][0] and ta[0][1] != table_b[0][1], "A must own a private copy of the block it will write"
    assert [hm.block_info(b)[0] for b in table_b[0]] == [2, 1, 1] and hm.block_info(ta[0][1]) == (1, False)
    assert _free(hm) == free1                                         # one block taken for the copy, A's old tail given back
    g_tok, g_logits = hm.unified_forward([(A, new, 20, True)], greedy=True, want_logits=True)
    assert hm.block_table(B) == table_b
    assert _same_kv(_kv(hm, B), snap_b), "A's writes after its truncate reached B"
    par = _parity(f"truncate-fork-nkv{nkv}-hd{hd}")
    _check_row(par, "A 20+6", om.forward(0, np.concatenate([prompt[:20], new]), 0), g_logits[0], g_tok[0])
    om.release(0)
    g_tok, g_logits = hm.unified_forward([(B, new[:1], n, True)], greedy=True, want_logits=True)
    _check_row(par, "B 37+1", om.forward(0, np.concatenate([prompt, new[:1]]), 0), g_logits[0], g_tok[0])
    om.release(0)
    par.finish()


@pytest.mark.parametrize("nkv,hd", DIMS)
def test_truncate_inside_a_prefix_cache_block_keeps_the_cache_entry(pkg, oracle, nkv, hd):
    A, C_ = 1, 3
    prompt, new = _prompt(48, 41), _prompt(10, 42)
    om = _oracle_model(nkv, hd)
    hm = _hip(pkg, nkv, hd)
    hm.reserve_kv_slots([(A, 48)])
    assert hm.prefix_cache_acquire(A, prompt) == 0
    hm.unified_forward([(A, prompt, 0, True)], greedy=True)
    hm.prefix_cache_register(A, prompt, 0)
    old = hm.block_table(A)[0]
    assert [hm.block_info(b) for b in old] == [(1, True)] * 3
    hm.truncate_kv(A, 20)
    ta = hm.block_table(A)[0]
    assert ta[0] == old[0] and ta[1] != old[1] and hm.block_info(ta[1]) == (1, False)
    assert [hm.block_info(b) for b in old] == [(1, True), (0, True), (0, True)]      # soft-free cache entries
    hm.unified_forward([(A, new, 20, True)], greedy=True)              # rewrites positions 20 … 29 of A's own block
    hits = hm.prefix_cache_stats()["hits"]
    hm.reserve_kv_slots([(C_, 48)])
    cached = hm.prefix_cache_acquire(C_, prompt)
    assert cached == 32 and hm.prefix_cache_stats()["hits"] == hits + 1              # a full hit, rolled back by one block
    assert hm.block_table(C_)[0] == old
    g_tok, g_logits = hm.unified_forward([(C_, prompt[cached:], cached, True)], greedy=True, want_logits=True)
    par = _parity(f"truncate-prefix-nkv{nkv}-hd{hd}")
    _check_row(par, "C", om.forward(0, prompt, 0), g_logits[0], g_tok[0])
    om.release(0)
    par.finish()


# ── the move kernel on its own ────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("chunk_bytes", [48, 2048, 4112, 16384, 65568])
def test_kv_move_kernel_moves_whole_chunks_and_nothing_else(pkg, chunk_bytes):
    """Pool → pool, gather and scatter of the op-level move over 3 pools of 9 blocks: every byte that should move does, every
    other byte of the pools and of the staging buffer keeps its fill.  48 B and 2 KiB are less than one 256-lane pass, 4112 B
    ends inside a pass, 16 KiB is the four-loads-per-lane pass exactly, 65568 B needs a second trip round the loop with a tail."""
    import ctypes as C
    import torch
    lib = pkg.load_library()
    nb, npools = 9, 3
    g = torch.Generator().manual_seed(chunk_bytes)
    host = [torch.randint(0, 256, (nb + 1, chunk_bytes), dtype=torch.uint8, generator=g) for _ in range(npools)]   # + 1 spare block
    pools = [h.cuda() for h in host]
    ptrs = torch.tensor([p.data_ptr() for p in pools], dtype=torch.int64).cuda()
    pairs_h = [(0, 5), (7, 1), (3, 3), (8, 2), (nb, 6), (4, nb)]                     # a self-pair and two ids outside the pool
    pairs = torch.tensor(pairs_h, dtype=torch.int32).cuda()
    stage = torch.full((len(pairs_h) + 1, npools, chunk_bytes), 0xA5, dtype=torch.uint8).cuda()

    def move(mode):
        torch.cuda.synchronize()
        rc = lib.ferrum_hip_kv_move_blocks(C.c_void_p(ptrs.data_ptr()), npools, C.c_void_p(pairs.data_ptr()), len(pairs_h),
                                           C.c_void_p(stage.data_ptr()), C.c_size_t(chunk_bytes), nb, mode, None)
        assert rc == 0, lib.ferrum_hip_last_error().decode()
        torch.cuda.synchronize()

    move(1)                                                                          # gather
    got = stage.cpu()
    for i, (s, _) in enumerate(pairs_h):
        for p in range(npools):
            want = host[p][s] if s < nb else torch.full((chunk_bytes,), 0xA5, dtype=torch.uint8)
            assert torch.equal(got[i, p], want), ("gather", i, p)
    assert (got[len(pairs_h)] == 0xA5).all()
    assert all(torch.equal(pools[p].cpu(), host[p]) for p in range(npools))
    move(0)                                                                          # pool → pool
    exp = [h.clone() for h in host]
    for s, d in pairs_h:
        if s < nb and d < nb:
            for p in range(npools):
                exp[p][d] = host[p][s]
    assert all(torch.equal(pools[p].cpu(), exp[p]) for p in range(npools)), "pool → pool"
    stage.copy_(torch.randint(0, 256, tuple(stage.shape), dtype=torch.uint8, generator=g))
    src = stage.cpu()
    move(2)                                                                          # scatter
    for i, (_, d) in enumerate(pairs_h):
        if d < nb:
            for p in range(npools):
                exp[p][d] = src[i, p]
    assert all(torch.equal(pools[p].cpu(), exp[p]) for p in range(npools)), "scatter"
    assert torch.equal(stage.cpu(), src)
