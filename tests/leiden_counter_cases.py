"""TEST INFRASTRUCTURE shared by tests/test_gpu_leiden_counters.py (the product library on the GPU),
tests/test_emu_leiden_counters_cpu.py (the same kernels on the emulator) and tools/leiden_counters_fixtures.py (which recorded
tests/golden/leiden_counters/): the graphs of the whole-run checks of the list and totals kernels of csrc/leiden.hip
("hot words").  Those kernels bound the workgroups that touch one counter word by COUNT_GRID
(SCAMD_LEIDEN_COUNT_GRID); every quantity they produce is an integer sum, minimum or count, or a list whose order nobody
observes, so a run computes bit for bit the same whatever the knob says.  Nothing here touches a device."""
from __future__ import annotations

from pathlib import Path

import numpy as np
from scipy import sparse

GOLDEN = Path(__file__).resolve().parent / "golden" / "leiden_counters"
COUNT_GRID_KNOB = "SCAMD_LEIDEN_COUNT_GRID"
N_WHOLE = 20000
WHOLE_RUNS = ("planted", "weak", "clique_ring_hubs")
# rows of the hubs of `clique_ring_hubs`: at 16 lanes per vertex (rows of ~20 entries) beyond the main tier (96), the wave
# tier (384) and the block tier (1536), two of each and in different 1024-vertex chunks
HUB_ROWS = (130, 200, 500, 900, 1700, 2600)


def _symmetric(n, rows, cols, rng, lo=0.1, hi=1.0):
    """symmetric float32 CSR over the undirected pairs (rows, cols): duplicates and loops dropped, one weight per pair"""
    a, b = np.minimum(rows, cols), np.maximum(rows, cols)
    keep = a != b
    pairs = np.unique(a[keep].astype(np.int64) * n + b[keep])
    a, b = pairs // n, pairs % n
    w = (rng.random(pairs.size) * (hi - lo) + lo).astype(np.float32)
    m = sparse.coo_matrix((w, (a, b)), shape=(n, n)).tocsr()
    m = (m + m.T).tocsr().astype(np.float32)
    m.sort_indices()
    return m


def blocks_knn_like(n, n_blocks, k_in, k_out, seed):
    """every vertex draws k_in neighbours inside its block (v % n_blocks) and k_out anywhere: rows of about 2 (k_in + k_out)"""
    rng = np.random.default_rng(seed)
    v = np.arange(n)
    per = n // n_blocks
    src_in = np.repeat(v, k_in)
    dst_in = (rng.integers(0, per, n * k_in) * n_blocks + src_in % n_blocks) % n
    src_out = np.repeat(v, k_out)
    dst_out = rng.integers(0, n, n * k_out)
    return _symmetric(n, np.concatenate([src_in, src_out]), np.concatenate([dst_in, dst_out]), rng)


def clique_ring_hubs(n, clique, seed):
    """cliques of `clique` vertices on a ring, neighbouring cliques joined by one edge, and len(HUB_ROWS) hubs whose rows
    have about HUB_ROWS entries (random other vertices)"""
    rng = np.random.default_rng(seed)
    n_cl = n // clique
    i, j = np.triu_indices(clique, k=1)
    base = (np.arange(n_cl) * clique)[:, None]
    rows = [(base + i[None, :]).ravel(), base.ravel() + clique - 1]
    cols = [(base + j[None, :]).ravel(), ((base + clique) % (n_cl * clique)).ravel()]
    hubs = 777 + 3011 * np.arange(len(HUB_ROWS))
    for h, r in zip(hubs, HUB_ROWS):
        rows.append(np.full(r, h))
        cols.append(rng.choice(n, r, replace=False))
    return _symmetric(n, np.concatenate(rows), np.concatenate(cols), rng)


_BUILDERS = {
    "planted": lambda: blocks_knn_like(N_WHOLE, 40, 10, 1, 1),
    "weak": lambda: blocks_knn_like(N_WHOLE, 40, 6, 5, 2),
    "clique_ring_hubs": lambda: clique_ring_hubs(N_WHOLE, 16, 3),
}
_graphs = {}


def whole_graph(name: str):
    """computed once, never written"""
    if name not in _graphs:
        m = _BUILDERS[name]()
        for arr in (m.data, m.indices, m.indptr):
            arr.setflags(write=False)
        _graphs[name] = m
    return _graphs[name]


def recorded(name: str):
    """(labels int32 [n], Q as float.hex, communities) of the build BEFORE the counter words were bounded"""
    import json

    meta = json.loads((GOLDEN / "recorded.json").read_text())[name]
    return np.load(GOLDEN / f"{name}_labels.npy"), meta["q_hex"], meta["communities"]


def check_whole_run(run, name: str, monkeypatch, count_grid):
    """run.leiden(adj, **kw) -> (labels numpy, Q, communities).  count_grid: value of the knob, None = the default"""
    if count_grid is None:
        monkeypatch.delenv(COUNT_GRID_KNOB, raising=False)
    else:
        monkeypatch.setenv(COUNT_GRID_KNOB, str(count_grid))
    labels, q_hex, nc = recorded(name)
    memb, q, got_nc = run.leiden(whole_graph(name), seed=0, n_iterations=-1)
    print(f"{name} COUNT_GRID={count_grid}: Q={q!r} communities={got_nc} (recorded {float.fromhex(q_hex)!r}, {nc})")
    assert got_nc == nc
    assert float(q).hex() == q_hex
    assert np.array_equal(np.asarray(memb, dtype=np.int32), labels)


# ---- the counters of one sweep: the test entry scamd_leiden_debug_counters_f32 ------------------------------------------------
# A runner hands in  counters(adj, membership, decision, flags, n_cls, salt) -> dict of numpy arrays / integers (the keys of
# scanpy_amd._kernels.leiden_debug_counters)  and  bounds(lanes) -> (main_max, wave_max, block_max).  Every expected value below
# is recomputed from the inputs in numpy.
KNOBS = ("1", "2", None)           # SCAMD_LEIDEN_COUNT_GRID: one span, two spans, the default (a span per 1024 vertices here)
SIZES = (1, 63, 1024, 1025, 2049, 4097)
COUNTS_WORDS = 32 + 16 * 32


def hash32(x):  # csrc/leiden.hip hash32, on uint64 arrays holding 32-bit values
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def lm_class(v, salt, n_cls):
    """csrc/leiden.hip lm_class"""
    v = np.asarray(v, dtype=np.uint64)
    return ((hash32((v * 0x9E3779B1 + salt) & 0xFFFFFFFF) >> 9) & (n_cls - 1)).astype(np.int64)


def quantise(w):
    """ld_level0_setup_kernel: llrint(w * 2^32) (ties to even, as np.rint), 0 for w <= 0"""
    w = np.asarray(w, dtype=np.float32).astype(np.float64)
    return np.where(w > 0.0, np.rint(w * 4294967296.0), 0.0).astype(np.int64)


def ring_with_long_rows(n, long_rows, seed):
    """a ring (every row two entries; n = 1: none, n = 2: one) plus, for every (vertex, length) of `long_rows`, further
    neighbours among the ordinary vertices until that vertex's row has exactly `length` entries"""
    rng = np.random.default_rng(seed)
    v = np.arange(n)
    rows, cols = [v], [(v + 1) % n]
    special = np.array([h for h, _ in long_rows], dtype=np.int64)
    ordinary = np.setdiff1d(v, np.concatenate([special, (special + 1) % n, (special - 1) % n])) if long_rows else v
    for h, length in long_rows:
        t = rng.choice(ordinary, length - 2, replace=False)
        rows.append(np.full(t.size, h))
        cols.append(t)
    m = _symmetric(n, np.concatenate(rows), np.concatenate(cols), rng) if n > 1 else sparse.csr_matrix((1, 1), dtype=np.float32)
    deg = np.diff(m.indptr)
    assert all(deg[h] == length for h, length in long_rows)
    return m


def _long_rows_for(n, bounds16):
    """the first row of the wave, block and giant tier and the last row below each, where the graph has room for them: three of
    each `first` length in the first 1024 vertices (two) and in the last chunk, one of each `last` length"""
    main_max, wave_max, block_max = bounds16
    out, at = [], 5
    for length in (main_max + 1, wave_max + 1, block_max + 1):
        if length + 40 < n:
            for h in (at, at + 600, n - 7 - at):
                out.append((h, length))
            out.append((at + 300, length - 1))
            at += 11
    return out


def _partition(kind, n, rng):
    if kind == "one":
        return np.full(n, n // 2, dtype=np.int32)
    if kind == "singletons":
        return rng.permutation(n).astype(np.int32)
    if kind == "interleaved2049":  # more keys than the 2048-slot table of a workgroup holds
        return (np.arange(n) % 2049).astype(np.int32)
    ids = rng.choice(n, min(64, n), replace=False)  # "random64"
    return ids[rng.integers(0, ids.size, n)].astype(np.int32)


def _flags(kind, n, rng):
    if kind is None:
        return None
    f = np.zeros(n, dtype=np.int32)
    if kind == "ones":
        f[:] = 1
    elif kind == "one":
        f[n // 3] = 1
    elif kind == "every1024":
        f[::1024] = 7  # (any non-zero word is a flag)
    elif kind == "half":
        f[rng.random(n) < 0.5] = 1
    else:
        assert kind == "none"
    return f


def _empty_class_salt(n, n_cls):
    for salt in range(1, 100000):
        if np.bincount(lm_class(np.arange(n), salt, n_cls), minlength=n_cls).min() == 0:
            return salt
    raise AssertionError("no salt leaves a class empty")


# name -> (n, long rows?, partition, flags, n_cls, salt)
def _unit_cases():
    t = {}
    for n in SIZES:
        t[f"n{n}_base"] = (n, False, "random64", None, 8, 0x1234)
        for fl in ("ones", "none", "one", "every1024"):
            t[f"n{n}_flags_{fl}"] = (n, False, "random64", fl, 8, 77)
        t[f"n{n}_cls1"] = (n, False, "random64", None, 1, 5)
        if n <= 4096:
            t[f"n{n}_cls32"] = (n, False, "random64", "half", 32, 6)
        for part in ("one", "singletons"):
            t[f"n{n}_part_{part}"] = (n, False, part, None, 8, 9)
    t["n63_empty_class"] = (63, False, "random64", None, 8, "empty")
    t["n4097_interleaved2049"] = (4097, False, "interleaved2049", None, 8, 3)
    for n in (1025, 2049, 4097):
        t[f"n{n}_long_rows"] = (n, True, "random64", None, 8, 11)
        t[f"n{n}_long_rows_half"] = (n, True, "random64", "half", 4, 12)
    return t


UNIT_CASES = _unit_cases()
_units = {}


def unit_case(name, bounds16):
    """(graph, membership, decision, flags, n_cls, salt): computed once, never written"""
    if name not in _units:
        n, long_rows, part, fl, n_cls, salt = UNIT_CASES[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        m = ring_with_long_rows(n, _long_rows_for(n, bounds16) if long_rows else [], 21)
        memb = _partition(part, n, rng)
        u = rng.random(n)
        decision = np.where(u < 0.4, memb[rng.integers(0, n, n)], np.where(u < 0.5, -2, -1)).astype(np.int32)
        flags = _flags(fl, n, rng)
        if salt == "empty":
            salt = _empty_class_salt(n, n_cls)
        for arr in (m.data, m.indices, m.indptr, memb, decision) + (() if flags is None else (flags,)):
            arr.setflags(write=False)
        _units[name] = (m, memb, decision, flags, n_cls, salt)
    return _units[name]


def check_counters(out, m, memb, decision, flags, n_cls, salt, bounds):
    """every property of one call's outputs; returns the class of every vertex (-1: not listed)"""
    n = m.shape[0]
    deg = np.diff(m.indptr)
    k = np.zeros(n, dtype=np.int64)
    np.add.at(k, np.repeat(np.arange(n), deg), quantise(m.data))
    listed = np.ones(n, dtype=bool) if flags is None else flags != 0
    want_cls = np.where(listed, lm_class(np.arange(n), salt, n_cls), -1)
    # every flagged vertex in exactly one list, exactly once, and in the list of its class
    lists = np.asarray(out["lists"]).reshape(n_cls, n)
    got_cls = np.full(n, -1, dtype=np.int64)
    seen = np.zeros(n, dtype=np.int64)
    for c in range(n_cls):
        ln = int(out["list_len"][c])
        assert 0 <= ln <= n
        vs = lists[c, :ln]
        assert vs.size == 0 or (vs.min() >= 0 and vs.max() < n)
        np.add.at(seen, vs, 1)
        got_cls[vs] = c
    assert np.array_equal(seen, listed.astype(np.int64)), "a flagged vertex is missing, listed twice, or an unflagged one listed"
    assert np.array_equal(got_cls, want_cls)
    # the tier lists hold exactly the positions whose degree falls in the bounds
    main_max, wave_max, block_max = bounds
    tiers = np.asarray(out["tier_lists"]).reshape(n_cls, n)
    giant = np.asarray(out["giant_lists"]).reshape(n_cls, -1)
    assert giant.shape[1] == int(m.nnz) // (block_max + 1) + 1 == out["giant_stride"]
    for c in range(n_cls):
        ln = int(out["list_len"][c])
        d = deg[lists[c, :ln]]
        n_w, n_b, n_g = (int(x) for x in out["tier_len"][c])
        for what, got, lo, hi in (("wave", tiers[c, :n_w], main_max, wave_max), ("block", tiers[c, n - n_b:][::-1] if n_b else tiers[c, :0], wave_max, block_max),
                                  ("giant", giant[c, :n_g], block_max, 1 << 40)):
            want = np.flatnonzero((d > lo) & (d <= hi))
            assert np.array_equal(np.sort(got), want), f"class {c}: {what} tier positions {np.sort(got)} != {want}"
    # totals: int64 sums
    Kb = np.zeros(n, dtype=np.int64)
    np.add.at(Kb, memb, k)
    assert np.array_equal(np.asarray(out["Ktot_before"]).astype(np.int64), Kb)
    assert np.array_equal(np.asarray(out["csize_before"]), np.bincount(memb, minlength=n))
    # moved / blocked and the state after: a sequential application
    mv = listed & (decision >= 0)
    bl = listed & (decision == -2)
    assert (out["moved"], out["blocked"]) == (int(mv.sum()), int(bl.sum()))
    comm, Ka, cs = memb.astype(np.int64).copy(), Kb.copy(), np.bincount(memb, minlength=n).astype(np.int64)
    for v in np.flatnonzero(mv):
        a, d = comm[v], int(decision[v])
        Ka[a] -= k[v]
        Ka[d] += k[v]
        cs[a] -= 1
        cs[d] += 1
        comm[v] = d
    assert np.array_equal(np.asarray(out["comm_after"]), comm)
    assert np.array_equal(np.asarray(out["Ktot_after"]).astype(np.int64), Ka)
    assert np.array_equal(np.asarray(out["csize_after"]), cs)
    assert np.array_equal(np.asarray(out["flags_after"]) != 0, bl)
    return got_cls


def run_unit_case(run, name, knob, monkeypatch):
    if knob is None:
        monkeypatch.delenv(COUNT_GRID_KNOB, raising=False)
    else:
        monkeypatch.setenv(COUNT_GRID_KNOB, knob)
    monkeypatch.delenv("SCAMD_LEIDEN_QUAD", raising=False)
    bounds16 = run.bounds(16)
    m, memb, decision, flags, n_cls, salt = unit_case(name, bounds16)
    out = run.counters(m, memb, decision, flags, n_cls, salt)
    assert out["lanes"] == 16, "the ring graphs are 16-lane levels"
    cls = check_counters(out, m, memb, decision, flags, n_cls, salt, bounds16)
    if UNIT_CASES[name][5] == "empty":
        assert min(out["list_len"][:n_cls]) == 0, "the salt was chosen to leave a class empty"
    if UNIT_CASES[name][1]:
        assert sum(int(x) for row in out["tier_len"] for x in row) > 0 or flags is not None
    again = run.counters(m, memb, decision, flags, n_cls, salt)
    assert np.array_equal(cls, check_counters(again, m, memb, decision, flags, n_cls, salt, bounds16)), "class differs between two calls"


def host_counters(lib, m, memb, decision, flags, n_cls, salt, block_max):
    """scamd_leiden_debug_counters_f32 of a library that takes HOST pointers (the emulator build) -> the runner's dict"""
    import ctypes as C

    n, nnz = m.shape[0], int(m.nnz)
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)  # noqa: E731
    indptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(m.indices, dtype=np.int32) if nnz else np.zeros(1, dtype=np.int32)
    w = np.ascontiguousarray(m.data, dtype=np.float32) if nnz else np.zeros(1, dtype=np.float32)
    memb = np.ascontiguousarray(memb, dtype=np.int32)
    decision = np.ascontiguousarray(decision, dtype=np.int32)
    fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.int32)
    stride = nnz // (block_max + 1) + 1
    i32 = lambda k: np.full(max(k, 1), -7, dtype=np.int32)  # noqa: E731
    i64 = lambda k: np.full(max(k, 1), -7, dtype=np.int64)  # noqa: E731
    out = dict(lists=i32(n_cls * n), tier_lists=i32(n_cls * n), giant_lists=i32(n_cls * stride), Ktot_before=i64(n), csize_before=i32(n),
               comm_after=i32(n), Ktot_after=i64(n), csize_after=i32(n), flags_after=i32(n))
    ws = np.full(max(int(lib.scamd_leiden_workspace_bytes(n, nnz)), 1), 0xAB, dtype=np.uint8)
    counts = (C.c_int32 * COUNTS_WORDS)()
    info = (C.c_int64 * 4)()
    rc = lib.scamd_leiden_debug_counters_f32(p(indptr), p(indices), p(w), n, nnz, p(memb), p(fl), n_cls, salt, p(decision),
                                             *(p(out[key]) for key in out), counts, info, p(ws), ws.size, None)
    assert rc == 0, lib.scamd_last_error().decode()
    out["list_len"] = [int(x) for x in counts[:n_cls]]
    out["tier_len"] = [[int(counts[32 + 16 * c + 8 + t]) for t in range(3)] for c in range(n_cls)]
    out.update(moved=int(info[0]), blocked=int(info[1]), giant_stride=int(info[2]), lanes=int(info[3]))
    return out
