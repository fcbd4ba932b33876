"""Leiden's reuse of the stored hierarchy (csrc/leiden.hip `reuse_level`) on the HOST-emulated kernels
(tests/emu/README.md).  An iteration after the first whose local moving moves nothing at the levels below takes the coarse
graph and the vertex map of the hierarchy that produced the best partition instead of refining and aggregating again;
`SCAMD_LEIDEN_REUSE=0` is the behaviour without it.  `SCAMD_LEIDEN_SMALL=0` throughout: graphs of this size would otherwise
leave the separate-kernel levels after one level.

`levels_reused` / `quiet_reuse_iterations` of the statistics: levels reused / iterations that ran on the stored hierarchy to
its end without a move."""
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy import sparse
from scipy.sparse.csgraph import connected_components

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT))
from oracle import connectivities as oconn  # noqa: E402
from oracle import knn as oknn  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build as emu_build
    import harness

    if not Path(emu_build.CLANG).exists():
        pytest.skip("no clang++ to build the host emulation of the kernels")
    return harness, harness.load()


def _blob_graph(n, seed, spread):
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((12, 10)) * spread
    x = (cent[rng.integers(0, 12, n)] + rng.standard_normal((n, 10))).astype(np.float32)
    idx, dist = oknn.knn_exact_f64(x, np.arange(n), 15)
    conn, _, _ = oconn.fuzzy_simplicial_set(idx, dist, n, 15)
    return conn


def _with_and_without(H, lib, monkeypatch, conn, **kw):
    monkeypatch.delenv("SCAMD_LEIDEN_REUSE", raising=False)
    new = H.leiden(lib, conn, **kw)
    st_new = H.leiden_stats(lib)
    monkeypatch.setenv("SCAMD_LEIDEN_REUSE", "0")
    old = H.leiden(lib, conn, **kw)
    st_old = H.leiden_stats(lib)
    monkeypatch.delenv("SCAMD_LEIDEN_REUSE")
    print(f"reuse: {st_new}  Q {new[1]!r} nc {new[2]}\nhook : {st_old}  Q {old[1]!r} nc {old[2]}")
    return new, st_new, old, st_old


def _connected_communities(conn, memb):
    conn = conn.tocsr()
    same = memb[np.repeat(np.arange(conn.shape[0]), np.diff(conn.indptr))] == memb[conn.indices]
    inner = sparse.csr_matrix((same.astype(np.int8), conn.indices.copy(), conn.indptr.copy()), shape=conn.shape)
    inner.eliminate_zeros()
    return connected_components(inner, directed=False)[0]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_separated_graph_is_bit_identical_to_the_run_without_reuse(emu, monkeypatch, seed):
    """12 well separated blobs, 6000 vertices: the second iteration only verifies the first one's partition.  With reuse it
    runs on the stored levels; labels, Q, community count and iteration count are those of the run that refines and
    aggregates every level again"""
    H, lib = emu
    monkeypatch.setenv("SCAMD_LEIDEN_SMALL", "0")
    conn = _blob_graph(6000, seed, 4.0)
    new, st_new, old, st_old = _with_and_without(H, lib, monkeypatch, conn, seed=seed)
    assert np.array_equal(new[0], old[0]) and new[1] == old[1] and new[2] == old[2]
    assert st_new["iterations"] == st_old["iterations"]
    assert st_new["levels_reused"] > 0 and st_old["levels_reused"] == 0
    assert st_new["quiet_reuse_iterations"] == 1 and st_old["quiet_reuse_iterations"] == 0
    assert st_new["launches"] < st_old["launches"]


def test_overlapping_graph_keeps_the_guarantees(emu, monkeypatch):
    """12 overlapping blobs (separation 0.8): a dozen iterations that all move vertices at level 0 -- nothing to reuse there --
    and a last one that moves nothing.  Reproducible; the reported Q is the labels' modularity; no vertex move and no merge
    improves the partition (oracle/leiden_guarantees.py); every community is connected; Q not below the oracle's own run"""
    from oracle import leiden as ol
    from oracle import leiden_guarantees as lg

    H, lib = emu
    monkeypatch.setenv("SCAMD_LEIDEN_SMALL", "0")
    monkeypatch.delenv("SCAMD_LEIDEN_REUSE", raising=False)
    conn = _blob_graph(6000, 0, 0.8)
    memb, q, nc = H.leiden(lib, conn, seed=0)
    st = H.leiden_stats(lib)
    memb2, q2, nc2 = H.leiden(lib, conn, seed=0)
    print(f"overlapping: Q {q!r}, {nc} communities, {st}")
    assert np.array_equal(memb, memb2) and q == q2 and nc == nc2 and H.leiden_stats(lib) == st
    assert abs(q - ol.modularity(conn, memb)) < 1e-8 and nc == int(memb.max()) + 1
    assert lg.improving_moves(conn, memb)["count"] == 0 and lg.mergeable_pairs(conn, memb)["count"] == 0
    assert _connected_communities(conn, memb) == nc
    q_oracle = ol.leiden(conn, seed=0)[1]
    print(f"oracle Q {q_oracle!r}")
    assert q > q_oracle - 2e-3


def test_iteration_after_the_polish_reuses_nothing(emu, monkeypatch):
    """the polish changes the best partition in place: the stored hierarchy is no longer that partition's own, and the
    verifying iteration that follows (level-0 local moving finds nothing to move: exactly the case the rule looks for) must
    refine and aggregate every level.  SCAMD_LEIDEN_MAX_ITERS=1: the polish meets the unfinished result of ONE iteration"""
    from oracle import leiden as ol
    from oracle import leiden_guarantees as lg

    H, lib = emu
    monkeypatch.setenv("SCAMD_LEIDEN_SMALL", "0")
    monkeypatch.delenv("SCAMD_LEIDEN_REUSE", raising=False)
    monkeypatch.setenv("SCAMD_LEIDEN_MAX_ITERS", "1")
    n = 2500
    x = np.random.default_rng(5).standard_normal((n, 10)).astype(np.float32)
    idx, dist = oknn.knn_exact_f64(x, np.arange(n), 15)
    conn, _, _ = oconn.fuzzy_simplicial_set(idx, dist, n, 15)
    memb, q, nc = H.leiden(lib, conn, seed=0)
    st = H.leiden_stats(lib)
    print(f"polish path: Q {q!r}, {nc} communities, {st}")
    assert st["polish_moves"] > 0 and st["iterations"] >= 2, st  # (the polish moved vertices, an iteration followed it)
    assert st["levels_reused"] == 0 and st["quiet_reuse_iterations"] == 0, st
    assert abs(q - ol.modularity(conn, memb)) < 1e-8 and nc == int(memb.max()) + 1
    assert lg.improving_moves(conn, memb)["count"] == 0 and lg.mergeable_pairs(conn, memb)["count"] == 0
    assert _connected_communities(conn, memb) == nc


def test_cpm_objective_is_bit_identical_to_the_run_without_reuse(emu, monkeypatch):
    """the CPM objective stores its vertex weights (sizes) with the levels: same equality against the hook"""
    H, lib = emu
    monkeypatch.setenv("SCAMD_LEIDEN_SMALL", "0")
    rng = np.random.default_rng(0)
    n = 1500
    cent = rng.standard_normal((12, 10)) * 4
    x = (cent[rng.integers(0, 12, n)] + rng.standard_normal((n, 10))).astype(np.float32)
    idx, dist = oknn.knn_exact_f64(x, np.arange(n), 15)
    conn, _, _ = oconn.fuzzy_simplicial_set(idx, dist, n, 15)
    new, st_new, old, st_old = _with_and_without(H, lib, monkeypatch, conn, seed=0, resolution=0.01, objective=1)
    assert np.array_equal(new[0], old[0]) and new[1] == old[1] and new[2] == old[2]
    assert st_new["iterations"] == st_old["iterations"]
    assert st_new["levels_reused"] > 0 and st_old["levels_reused"] == 0
