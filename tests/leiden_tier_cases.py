"""TEST INFRASTRUCTURE shared by tests/test_gpu_leiden_tiers.py (the product library on the GPU) and
tests/test_emu_leiden_tiers_cpu.py (the same host code and kernels on the emulator, through tests/emu/harness.py): the smallest
graphs at which every tier of a Leiden decide step (csrc/leiden.hip `decide_tiers`) is reached, ONE
checker, and the recorded result of every case.  Nothing here touches a device: a test hands in a `Runner`.

The tiers of a row of `deg` entries in a launch with `lanes` lanes per vertex, with the bounds
`scamd_leiden_tier_bounds(lanes)` reports:  deg <= main_max: the main tier;  <= wave_max: the wave-per-row tier;
<= block_max: the 256-thread workgroup-per-row tier;  longer: the 1024-thread ("giant") tier.

EXPECTED below was recorded with `python tests/leiden_tier_cases.py <emulator library>` on the emulator build of the commit
BEFORE the tiers were fused into one launch (three launches per decide step, lists appended by the decide kernels), with
the bounds that build had written out by hand (96 / 192 / 384, and 1536 for the graphs' sake only).  The fused build has to
reproduce every figure on the emulator and on the device: every decision is the same rule on the same snapshot, in integers.
"""
from __future__ import annotations

import hashlib

import numpy as np
from scipy import sparse

QUADS = ("0", "1", "2")                  # SCAMD_LEIDEN_QUAD: 64 / 16 / 32 lanes per vertex on every level
LANES = {"0": 64, "1": 16, "2": 32}
RECORDED_BOUNDS = {16: (96, 384, 1536), 32: (192, 384, 1536), 64: (384, 384, 1536)}  # lanes -> main_max, wave_max, block_max


def _symmetric_weights(adj_bool, rng):
    """float32 weights in [0.1, 1) on the upper triangle of a symmetric 0/1 matrix, mirrored"""
    up = sparse.triu(sparse.csr_matrix(adj_bool), k=1).tocoo()
    w = (rng.random(up.nnz) * 0.9 + 0.1).astype(np.float32)
    m = sparse.coo_matrix((w, (up.row, up.col)), shape=adj_bool.shape).tocsr()
    return (m + m.T).tocsr().astype(np.float32)


def _hash32(x):  # csrc/leiden.hip hash32
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def lm_class(v, sweep, n_cls=8, seed=0):
    """class of vertex v in local-moving sweep `sweep` of the first iteration (csrc/leiden.hip lm_class and the sweep's salt)"""
    salt = _hash32(seed + 0x85EBCA77 * (sweep + 1))
    return (_hash32(v * 0x9E3779B1 + salt) >> 9) & (n_cls - 1)


def boundary_graph(bounds):
    """3000 vertices with eight random neighbours each (symmetrised), then two vertices for every length in `bounds` and
    `bounds` + 1 whose rows have EXACTLY that many entries (filled up with ordinary vertices, which no other special row
    may touch afterwards).  The classes are drawn afresh in every sweep; the two vertices of a length sit in different
    classes in at least two of the first three sweeps of level 0, so more than one class holds such a row"""
    rng = np.random.default_rng(11)
    n, deg = 3000, 8
    a = np.zeros((n, n), dtype=bool)
    a[np.repeat(np.arange(n), deg), rng.integers(0, n, n * deg)] = True
    a |= a.T
    np.fill_diagonal(a, False)
    lengths = sorted({b + d for b in bounds for d in (0, 1)})
    special = np.arange(2 * len(lengths)) * 37 + 5  # spread over the classes; two per length
    a[np.ix_(special, special)] = False
    for i in range(len(lengths)):
        assert sum(lm_class(int(special[2 * i]), sw) != lm_class(int(special[2 * i + 1]), sw) for sw in range(3)) >= 2
    ordinary = np.setdiff1d(np.arange(n), special)
    want = {}
    for i, length in enumerate(lengths):
        for v in special[2 * i:2 * i + 2]:
            free = ordinary[~a[v, ordinary]]
            t = rng.choice(free, length - int(a[v].sum()), replace=False)
            a[v, t] = True
            a[t, v] = True
            want[int(v)] = length
    m = _symmetric_weights(a, rng)
    got = np.diff(m.indptr)
    assert all(got[v] == length for v, length in want.items())
    return m


def blocks_graph(n, n_blocks, p_in, p_out, seed):
    """dense planted blocks: every row has about n (p_in / n_blocks + p_out (1 - 1 / n_blocks)) entries, heavy inside a block"""
    rng = np.random.default_rng(seed)
    blk = np.arange(n) % n_blocks
    same = blk[:, None] == blk[None, :]
    a = np.triu(rng.random((n, n)) < np.where(same, p_in, p_out), k=1)
    w = np.where(same, rng.random((n, n)) * 0.5 + 0.5, rng.random((n, n)) * 0.1 + 0.05) * a
    return sparse.csr_matrix((w + w.T).astype(np.float32))


def _long_rows():
    from helpers import long_rows_graph

    return long_rows_graph()


def _cpm_weights(n):
    return (np.arange(n) % 4 + 2) / 4.0  # 0.5 .. 1.25 in quarters: exact in the kernel's fixed point


# name -> (graph(bounds), leiden arguments, tiers every lane setting must reach beyond the main one)
CASES = {
    "long_rows_two_iterations": (lambda b: _long_rows(), dict(n_iterations=2), ("wave", "block", "giant")),
    "long_rows_with_polish": (lambda b: _long_rows(), dict(n_iterations=-1), ("wave", "block", "giant")),
    "boundary_rows": (lambda b: boundary_graph(sorted({x for t in b.values() for x in t})), dict(n_iterations=2),
                      ("wave", "block", "giant")),
    # every row of the level-0 graph is a block-tier row: the main range of the grid is empty there
    "all_block_rows": (lambda b: blocks_graph(600, 6, 0.95, 0.70, 3), dict(n_iterations=-1), ("block",)),
    # ... a giant-tier row (the emulator runs the full graph too: ~1700 x 1600 entries)
    "all_giant_rows": (lambda b: blocks_graph(1700, 4, 0.97, 0.94, 4), dict(n_iterations=2), ("giant",)),
    "long_rows_cpm_node_weights": (lambda b: _long_rows(), dict(n_iterations=2, objective=1, resolution=0.02, node_weights="cpm"),
                                   ("wave", "block", "giant")),
}

# name -> labels sha256, Q (float.hex), communities, iterations, lm_sweeps, hub_pass_vertices, overflow_pass_vertices by QUAD
EXPECTED = {
    "long_rows_two_iterations": ('c07fed456dbcf2f22d4f10cb1ff593bac5091597829319dbf594773c741de839',
        '0x1.e4f3a9e3d18fep-3', 20, 2, 48, 88, {'0': 0, '1': 1314, '2': 150}),
    "long_rows_with_polish": ('7bba07426dd5ebb7bcbdf85d9c0f42c1281080a004118db15b0dc0344e022336',
        '0x1.f35b0b9f3f592p-3', 19, 22, 244, 463, {'0': 0, '1': 7952, '2': 712}),
    "boundary_rows": ('e70758d1d9c81d153254195c0ded0b1401899edf806df9998fd4f540935fa73d',
        '0x1.b1d969eb914cfp-3', 14, 2, 46, 202, {'0': 0, '1': 841, '2': 321}),
    "all_block_rows": ('a02c68d21a8171a9ebe108d6e7c1a514a441654a1f1ec20ca9a911c67f390447',
        '0x1.013a8ea2a055bp-1', 6, 2, 8, 3000, {'0': 0, '1': 3000, '2': 2400}),
    "all_giant_rows": ('8461bf4d32fee8d8c1171119c1e49eb254c5d0a9010428fa5faba5b9486c4af8',
        '0x1.e17cf2895bb6ap-2', 4, 2, 8, 8500, {'0': 0, '1': 8500, '2': 6800}),
    "long_rows_cpm_node_weights": ('c9a36ff8643444f15f9ca550a8071653ef718d46ff029e5a97cf56d7bc23b934',
        '0x1.94ca4c46ea75cp-3', 179, 2, 38, 75, {'0': 0, '1': 2976, '2': 112}),
}

_graphs = {}


def case_graph(name: str):
    """computed once, never written"""
    if name not in _graphs:
        m = CASES[name][0](RECORDED_BOUNDS).tocsr()
        m.sort_indices()
        for arr in (m.data, m.indices, m.indptr):
            arr.setflags(write=False)
        _graphs[name] = m
    return _graphs[name]


def _rows_in(deg, lo, hi):
    return int(((deg > lo) & (deg <= hi)).sum())


def run_case(run, name: str, monkeypatch, label: str = "", expected=EXPECTED):
    """run: .leiden(adj, **kw) -> (labels [n] numpy, Q, communities), .stats() -> dict of the last call, .bounds(lanes) ->
    (main_max, wave_max, block_max).  Returns the figures of the case in the form of an EXPECTED entry."""
    from oracle import leiden as ol

    m = case_graph(name)
    _, kw, tiers = CASES[name]
    kw = dict(kw)
    if kw.get("node_weights") == "cpm":
        kw["node_weights"] = _cpm_weights(m.shape[0])
    deg = np.diff(m.indptr)
    monkeypatch.setenv("SCAMD_LEIDEN_SMALL", "0")
    out, overflow = {}, {}
    for quad in QUADS:
        monkeypatch.setenv("SCAMD_LEIDEN_QUAD", quad)
        main_max, wave_max, block_max = run.bounds(LANES[quad])
        assert (main_max, wave_max, block_max) == RECORDED_BOUNDS[LANES[quad]], "the graphs were built for other bounds"
        memb, q, nc = run.leiden(m, seed=0, **kw)
        st = run.stats()
        print(f"{label} {name} QUAD={quad}: Q={q!r} communities={nc} iterations={st['iterations']} lm_sweeps={st['lm_sweeps']} "
              f"overflow pass={st['overflow_pass_vertices']} hub pass={st['hub_pass_vertices']} launches={st['launches']}")
        assert abs(q - ol.modularity(m, memb)) < 1e-8 and nc == int(memb.max()) + 1
        # the tiers were reached: the first sweep of level 0 visits every vertex, so each statistic counts at least the
        # level-0 rows of its tier (block and giant tier share `hub_pass_vertices`: the graph's row lengths tell them apart)
        n_wave, n_block, n_giant = _rows_in(deg, main_max, wave_max), _rows_in(deg, wave_max, block_max), _rows_in(deg, block_max, 1 << 30)
        for tier, rows in (("wave", n_wave if LANES[quad] < 64 else None), ("block", n_block), ("giant", n_giant)):
            if tier in tiers and rows is not None:
                assert rows > 0, f"{name}: no level-0 row for the {tier} tier at {LANES[quad]} lanes"
        # (`overflow_pass_vertices` counts every row beyond the main tier of a 16- / 32-lane launch, whichever tier decides it)
        assert st["overflow_pass_vertices"] >= (n_wave + n_block + n_giant if LANES[quad] < 64 else 0)
        assert st["hub_pass_vertices"] >= n_block + n_giant
        if LANES[quad] == 64:
            assert st["overflow_pass_vertices"] == 0
        if tiers == ("block",):
            assert deg.min() > wave_max and deg.max() <= block_max
        if tiers == ("giant",):
            assert deg.min() > block_max
        out[quad] = (memb, q, nc, st["iterations"], st["lm_sweeps"], st["hub_pass_vertices"])
        overflow[quad] = st["overflow_pass_vertices"]
    for quad in QUADS[1:]:
        assert np.array_equal(out[quad][0], out["0"][0]) and out[quad][1:] == out["0"][1:], f"{name}: QUAD={quad} differs from QUAD=0"
    memb, q, nc, iters, sweeps, hub = out["0"]
    got = (hashlib.sha256(np.ascontiguousarray(memb, dtype=np.int32).tobytes()).hexdigest(), float(q).hex(), nc, iters, sweeps, hub,
           overflow)
    if expected is not None:
        assert got == expected[name], f"{name}: {got} != recorded {expected[name]}"
    return got


if __name__ == "__main__":  # python tests/leiden_tier_cases.py <emulator library>: prints the EXPECTED table of that build
    import sys
    import time
    from pathlib import Path

    import pytest

    root = Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(root), str(root / "tests"), str(root / "tests" / "emu")]
    import ctypes as C

    import harness

    lib = C.CDLL(sys.argv[1])
    for fn_name in ("scamd_leiden_workspace_bytes", "scamd_leiden_csr_nw_f32", "scamd_leiden_last_stats", "scamd_leiden_stat_name",
                    "scamd_last_error"):
        fn = getattr(lib, fn_name)
        fn.restype, fn.argtypes = harness.SIGNATURES[fn_name]

    class Recorded:
        leiden = staticmethod(lambda adj, **kw: harness.leiden(lib, adj, **kw))
        stats = staticmethod(lambda: harness.leiden_stats(lib))
        bounds = staticmethod(lambda lanes: RECORDED_BOUNDS[lanes])

    mp = pytest.MonkeyPatch()
    for case in sys.argv[2:] or CASES:
        t0 = time.time()
        print(f'    "{case}": {run_case(Recorded, case, mp, expected=None)!r},  # {time.time() - t0:.1f} s', flush=True)
    mp.undo()
