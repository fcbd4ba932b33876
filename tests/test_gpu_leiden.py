"""GPU Leiden vs the CPU oracle (oracle/leiden.c).  Label parity is UNPINNED in the reference (no golden
labels; tests/test_clustering.py pins determinism, seed sensitivity, NMI > 0.9 between flavors), so the
checks are: identical modularity arithmetic, quality at least the oracle's, ARI on planted partitions."""
from __future__ import annotations

import numpy as np
import pytest
from scipy import sparse
from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score

from oracle import connectivities as oc
from oracle import knn as oknn
from oracle import leiden as ol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from scanpy_amd import _kernels

    return _kernels


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _graph_dev(adj):
    adj = sparse.csr_matrix(adj)
    adj.sort_indices()
    return _dev(adj.indptr.astype(np.int64)), _dev(adj.indices.astype(np.int32)), _dev(adj.data.astype(np.float32)), adj.shape[0]


def _blob_graph(n, n_types, seed, spread=1.0, k=15):
    from scanpy_amd.datasets import blobs_embedding

    x, lab = blobs_embedding(n, 50, n_types=n_types, spread=spread, seed=seed)
    idx, dist, _ = oknn.knn_sklearn(x, k, n_jobs=-1)
    c, _, _ = oc.fuzzy_simplicial_set(idx, dist, n, k)
    return c, lab


def test_modularity_matches_oracle(K, pbmc68k):
    adj = pbmc68k["connectivities"].astype(np.float32)
    ip, ix, w, n = _graph_dev(adj)
    for memb in (pbmc68k["louvain_codes"].astype(np.int32), np.arange(n, dtype=np.int32), np.zeros(n, dtype=np.int32)):
        for res in (1.0, 0.5, 2.0):
            q = K.modularity(ip, ix, w, n, _dev(memb), resolution=res)
            assert abs(q - ol.modularity(adj, memb, resolution=res)) < 1e-8


def test_leiden_fixture_quality_and_determinism(K, pbmc68k):
    adj = pbmc68k["connectivities"].astype(np.float32)
    ip, ix, w, n = _graph_dev(adj)
    m0, q0, nc0 = K.leiden(ip, ix, w, n, seed=0)
    m0 = m0.cpu().numpy()
    _, q_oracle = ol.leiden(adj, seed=0)
    print("gpu Q", q0, "n_comm", nc0, "oracle Q", q_oracle)
    assert abs(q0 - ol.modularity(adj, m0)) < 1e-8, "reported modularity must be that of the labels"
    assert q0 > q_oracle - 0.01
    assert m0.min() == 0 and m0.max() == nc0 - 1
    sizes = np.bincount(m0)
    assert (np.diff(sizes) <= 0).all(), "ids ordered by decreasing size"
    m1, q1, _ = K.leiden(ip, ix, w, n, seed=0)
    np.testing.assert_array_equal(m0, m1.cpu().numpy())
    assert q0 == q1
    mo, _ = ol.leiden(adj, seed=0)
    nmi = normalized_mutual_info_score(mo, m0)
    print("NMI vs oracle", nmi, "ARI", adjusted_rand_score(mo, m0))
    assert nmi > 0.9  # the reference's own cross-implementation bar (tests/test_clustering.py:130-163)


def test_leiden_seed_changes_labels(K, pbmc68k):
    adj = pbmc68k["connectivities"].astype(np.float32)
    ip, ix, w, n = _graph_dev(adj)
    labels = [K.leiden(ip, ix, w, n, seed=s)[0].cpu().numpy() for s in (0, 1, 2, 3)]
    assert any((labels[0] != l).any() for l in labels[1:])


@pytest.mark.parametrize(("n", "n_types"), [(5000, 8), (20000, 32), (60000, 64)])
def test_leiden_planted(K, n, n_types):
    adj, truth = _blob_graph(n, n_types, seed=n)
    ip, ix, w, _ = _graph_dev(adj)
    m, q, nc = K.leiden(ip, ix, w, n)
    m = m.cpu().numpy()
    mo, qo = ol.leiden(adj)
    ari_truth, ari_oracle = adjusted_rand_score(truth, m), adjusted_rand_score(mo, m)
    print(f"n={n}: gpu Q={q:.6f} nc={nc}; oracle Q={qo:.6f} nc={mo.max() + 1}; ARI truth={ari_truth:.4f} oracle={ari_oracle:.4f}")
    assert ari_oracle >= 0.99
    assert ari_truth >= 0.99
    assert q >= qo - 1e-6


def test_leiden_resolution_and_iterations(K):
    adj, _ = _blob_graph(8000, 16, seed=3)
    ip, ix, w, n = _graph_dev(adj)
    for res in (0.3, 1.0, 3.0):
        m, q, nc = K.leiden(ip, ix, w, n, resolution=res)
        mo, qo = ol.leiden(adj, resolution=res)
        print(f"res={res}: gpu Q={q:.5f} nc={nc} oracle Q={qo:.5f} nc={mo.max() + 1}")
        assert abs(q - ol.modularity(adj, m.cpu().numpy(), resolution=res)) < 1e-8
        assert q >= qo - 0.01
    m2, q2, _ = K.leiden(ip, ix, w, n, n_iterations=2)
    assert q2 > 0.5


def test_leiden_disconnected_and_isolated(K):
    # two cliques + three isolated vertices
    a = np.zeros((11, 11), dtype=np.float32)
    a[:4, :4] = 1
    a[4:8, 4:8] = 1
    np.fill_diagonal(a, 0)
    adj = sparse.csr_matrix(a)
    ip, ix, w, n = _graph_dev(adj)
    m, q, nc = K.leiden(ip, ix, w, n)
    m = m.cpu().numpy()
    assert nc == 5 and len(set(m[:4])) == 1 and len(set(m[4:8])) == 1 and m[0] != m[4]
    assert len(set(m[8:])) == 3


@pytest.mark.parametrize(
    "env",
    [
        {"SCAMD_LEIDEN_AGG_WAVE_MAX": "0"},  # every coarse row through the workgroup tier
        {"SCAMD_LEIDEN_AGG_WAVE_MAX": "0", "SCAMD_LEIDEN_AGG_MID_MAX": "0"},  # ... through the 8192-slot tier
        {"SCAMD_LEIDEN_AGG_WAVE_MAX": "0", "SCAMD_LEIDEN_AGG_MID_MAX": "0", "SCAMD_LEIDEN_AGG_PASS_KEYS": "16"},
        # (round 5: a multi-pass row first tries one optimistic pass with bounded probing; 0 = straight to the class passes,
        #  1 = a trial that fails on the first collision and falls back)
        {"SCAMD_LEIDEN_AGG_WAVE_MAX": "0", "SCAMD_LEIDEN_AGG_MID_MAX": "0", "SCAMD_LEIDEN_AGG_PASS_KEYS": "16",
         "SCAMD_LEIDEN_HUB_TRY_PROBES": "0"},
        {"SCAMD_LEIDEN_AGG_WAVE_MAX": "0", "SCAMD_LEIDEN_AGG_MID_MAX": "0", "SCAMD_LEIDEN_AGG_PASS_KEYS": "16",
         "SCAMD_LEIDEN_HUB_TRY_PROBES": "1"},
        {"SCAMD_LEIDEN_AGG_WAVE_WORK": "64", "SCAMD_LEIDEN_AGG_MID_WORK": "512"},  # tiers by work: rows leave the wave tier early
        # coarse rows cut into parts of 64 / 1024 member entries, built as pseudo rows by several workgroups and merged
        {"SCAMD_LEIDEN_AGG_WAVE_WORK": "32", "SCAMD_LEIDEN_AGG_SPLIT_CHUNK": "64", "SCAMD_LEIDEN_AGG_SPLIT_WORK": "64"},
        {"SCAMD_LEIDEN_AGG_SPLIT_CHUNK": "1024", "SCAMD_LEIDEN_AGG_SPLIT_WORK": "4096"},
    ],
    ids=["mid", "big", "big-multipass", "big-classpasses", "big-failed-trial", "work-tiers", "split-64", "split-1024"],
)
def test_leiden_coarse_row_tiers_agree(K, monkeypatch, env):
    """the wave / workgroup / multi-pass builders of the coarse graph produce the same graph, so the partition
    (deterministic given the seed) is the same through each of them"""
    adj, _ = _blob_graph(6000, 12, seed=3)
    ip, ix, w, n = _graph_dev(adj.astype(np.float32))
    m0, q0, nc0 = K.leiden(ip, ix, w, n, seed=5)
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    m1, q1, nc1 = K.leiden(ip, ix, w, n, seed=5)
    assert nc0 == nc1 and q0 == q1
    assert np.array_equal(m0.cpu().numpy(), m1.cpu().numpy())


def test_leiden_long_hub_rows_single_pass_equals_class_passes(K, monkeypatch):
    """vertices with 6500 / 7000 neighbours (beyond the 6000-entry single-pass bound of the hub kernels): the optimistic
    single pass (default), a trial that fails at once (2 probes) and the class passes alone (0) must give the same
    partition -- the decision of a row does not depend on how its table was filled"""
    rng = np.random.default_rng(2)
    n, deg = 8000, 6
    m = sparse.coo_matrix((rng.random(n * deg).astype(np.float32) * 0.9 + 0.1,
                           (np.repeat(np.arange(n), deg), rng.integers(0, n, n * deg))), shape=(n, n)).tocsr()
    for h, dh in ((0, 7000), (1, 6500)):
        t = rng.choice(n, dh, replace=False)
        m = m + sparse.coo_matrix((rng.random(dh).astype(np.float32) * 0.5 + 0.1, (np.full(dh, h), t)), shape=(n, n)).tocsr()
    m.setdiag(0)
    m.eliminate_zeros()
    m = m.maximum(m.T).tocsr().astype(np.float32)
    assert np.diff(m.indptr).max() >= 7000
    ip, ix, w, n = _graph_dev(m)
    out = {}
    for probes in ("64", "0", "2"):
        monkeypatch.setenv("SCAMD_LEIDEN_HUB_TRY_PROBES", probes)
        memb, q, nc = K.leiden(ip, ix, w, n, seed=0)
        out[probes] = (memb.cpu().numpy(), q, nc)
    assert abs(out["0"][1] - ol.modularity(m, out["0"][0])) < 1e-8
    for probes in ("64", "2"):
        assert out[probes][1] == out["0"][1] and np.array_equal(out[probes][0], out["0"][0])


def test_leiden_small_levels_in_one_workgroup_vs_separate_kernels(K, monkeypatch, pbmc68k):
    """levels of <= 1024 nodes run in ONE workgroup (ld_small_levels_kernel: 8 nodes at a time) -- a different schedule
    from the class sub-rounds of the separate kernels, so the partitions need not be equal; both must reach the oracle's
    modularity on the fixture (which is such a level from the start) and both must be reproducible"""
    adj = pbmc68k["connectivities"].astype(np.float32)
    ip, ix, w, n = _graph_dev(adj)
    _, q_oracle = ol.leiden(adj, seed=0)
    out = {}
    for small in ("1", "0"):
        monkeypatch.setenv("SCAMD_LEIDEN_SMALL", small)
        m0, q0, nc0 = K.leiden(ip, ix, w, n, seed=0)
        m1, q1, _ = K.leiden(ip, ix, w, n, seed=0)
        assert q0 == q1 and np.array_equal(m0.cpu().numpy(), m1.cpu().numpy())
        assert abs(q0 - ol.modularity(adj, m0.cpu().numpy())) < 1e-8
        out[small] = (q0, nc0)
    print("one workgroup:", out["1"], "separate kernels:", out["0"], "oracle Q", q_oracle)
    assert min(out["1"][0], out["0"][0]) > q_oracle - 3e-3


def _tiny_graphs():
    from scipy import sparse

    rng = np.random.default_rng(1)
    out = [sparse.csr_matrix(np.array([[0, 1], [1, 0]], dtype=np.float32)),                       # one edge
           sparse.csr_matrix(np.array([[0, 1, 0], [1, 0, 0], [0, 0, 0]], dtype=np.float32))]      # an edge and a loner
    while len(out) < 40:
        n = int(rng.integers(3, 24))
        a = (rng.random((n, n)) < rng.choice([0.1, 0.3, 0.6, 1.0])).astype(np.float32) * rng.random((n, n)).astype(np.float32)
        a = np.triu(a, 1)
        if a.sum() > 0:
            out.append(sparse.csr_matrix(a + a.T))
    return out


def test_leiden_tiny_graphs(K):
    """Levels of <= 16 vertices move one vertex at a time (ld_small_levels_kernel, SMALL_SEQ_N): with eight vertices deciding
    at once on such graphs neighbours swapped communities for ever -- a single edge ended as two singletons (Q = -0.5).
    Found on the host emulation of the kernels (tests/emu), which also showed the rule costs larger levels nothing."""
    worst = 0.0
    for adj in _tiny_graphs():
        ip, ix, w, n = _graph_dev(adj)
        q_oracle = min(ol.leiden(adj, seed=s)[1] for s in range(5))  # the oracle's worst of five seeds
        for seed in (0, 1):
            m, q, _ = K.leiden(ip, ix, w, n, seed=seed)
            assert abs(q - ol.modularity(adj, m.cpu().numpy())) < 1e-9
            assert q > -1e-12, (n, adj.nnz, q)  # (the one-community partition has Q = 0: nothing may end below it)
            worst = min(worst, q - q_oracle)
    print("largest shortfall against the oracle's worst seed", worst)
    assert worst > -0.05  # (a 13-vertex graph ends in a local optimum 0.036 below the oracle for two seeds: visiting order)


def test_leiden_quarter_wave_kernels_agree(K, monkeypatch):
    """four-vertices-per-wave and wave-per-vertex decision kernels implement the same rule: same partition"""
    adj, _ = _blob_graph(6000, 12, seed=4)
    ip, ix, w, n = _graph_dev(adj.astype(np.float32))
    monkeypatch.setenv("SCAMD_LEIDEN_QUAD", "0")
    m0, q0, nc0 = K.leiden(ip, ix, w, n, seed=7)
    for forced in ("1", "2"):  # 16 and 32 lanes per vertex
        monkeypatch.setenv("SCAMD_LEIDEN_QUAD", forced)
        m1, q1, nc1 = K.leiden(ip, ix, w, n, seed=7)
        assert nc0 == nc1 and q0 == q1
        assert np.array_equal(m0.cpu().numpy(), m1.cpu().numpy())


def test_leiden_long_row_tiers_agree(K, monkeypatch):
    """the decide step of a row is the same rule in every tier: with 64, 16 and 32 lanes per vertex (SCAMD_LEIDEN_QUAD = 0 /
    1 / 2) the rows of 150 .. 2500 entries are decided by the main launch, the 64-lane overflow pass or the hub pass, and the
    partition must not depend on which.  `overflow_pass_vertices` / `hub_pass_vertices` of the statistics (vertices taken over by
    the overflow pass / handed to the hub pass) show that the tiers were reached: with 64 lanes there is no overflow tier."""
    from helpers import long_rows_graph

    m = long_rows_graph()
    ip, ix, w, n = _graph_dev(m)
    monkeypatch.setenv("SCAMD_LEIDEN_SMALL", "0")
    out = {}
    for quad in ("0", "1", "2"):
        monkeypatch.setenv("SCAMD_LEIDEN_QUAD", quad)
        memb, q, nc = K.leiden(ip, ix, w, n, seed=0)
        st = K.leiden_last_stats()
        print(f"QUAD={quad}: Q={q!r} communities={nc} overflow pass={st['overflow_pass_vertices']} hub pass={st['hub_pass_vertices']}")
        out[quad] = (memb.cpu().numpy(), q, nc)
        assert abs(q - ol.modularity(m, out[quad][0])) < 1e-8
        assert st["hub_pass_vertices"] > 0
        assert (st["overflow_pass_vertices"] == 0) if quad == "0" else (st["overflow_pass_vertices"] > 0)
    for quad in ("1", "2"):
        assert out[quad][1] == out["0"][1] and out[quad][2] == out["0"][2] and np.array_equal(out[quad][0], out["0"][0])


def test_leiden_entry_points_are_one_run(K, pbmc68k):
    """scamd_leiden_csr_f32 / _init_f32 / _ex_f32 / _nw_f32 on the 700-cell fixture graph (helpers.check_leiden_entry_points)"""
    import torch
    from helpers import check_leiden_entry_points

    from scanpy_amd import _lib
    from scanpy_amd._device import ptr, stream_ptr

    lib = _lib.load()
    ip, ix, w, n = _graph_dev(pbmc68k["connectivities"].astype(np.float32))
    ws = torch.full((int(lib.scamd_leiden_workspace_bytes(n, w.numel())),), 0xAB, dtype=torch.uint8, device="cuda")
    check_leiden_entry_points(lib, ptr, (ip, ix, w, n, w.numel()), lambda m: torch.empty(m, dtype=torch.int32, device="cuda"),
                              lambda t: t.cpu().numpy(), torch.arange(n, dtype=torch.int32, device="cuda"),
                              torch.ones(n, dtype=torch.float32, device="cuda"), ws, stream_ptr())


def test_leiden_stat_keys(K):
    """the statistics dict is built from the library's own slot -> key table: the keys are the documented ones"""
    from helpers import check_leiden_stat_keys

    from scanpy_amd import _lib

    check_leiden_stat_keys(_lib.load(), K.leiden_last_stats())
