"""Leiden's reuse of the stored hierarchy (csrc/leiden.hip `reuse_level`) on the GPU, on the path's own
fuzzy graphs of 200k cells (built as tests/leiden_det_worker.py builds them).

planted: the second iteration only verifies the first one's partition -- with reuse it runs on the stored levels, and labels,
Q, community count and iteration count are those of a run that refines and aggregates every level again
(`SCAMD_LEIDEN_REUSE=0`).  weak: a run of many iterations, most of which move vertices at level 0 (nothing to reuse) -- the
paper's guarantees hold for what it returns.

`levels_reused` / `quiet_reuse_iterations` of the statistics: levels reused / iterations that ran on the stored hierarchy to
its end without a move."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest
from scipy import sparse
from scipy.sparse.csgraph import connected_components

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

N = 200_000


def _graph(structure):
    import bench
    from scanpy_amd._pipeline import run_path
    from scanpy_amd.preprocessing._pca_solver import GpuBackend

    x, _ = bench.make_matrix(N, 2000, 0, structure)
    backend = GpuBackend()
    res = run_path(backend.upload(x), N, backend=backend)
    return res.conn_indptr, res.conn_indices, res.conn_data


def _run(ip, ix, w, seed):
    import torch

    from scanpy_amd import _kernels as K

    labels, q, nc = K.leiden(ip, ix, w, N, seed=seed)
    torch.cuda.synchronize()
    return labels.cpu().numpy(), q, nc, K.leiden_last_stats()


@pytest.fixture(scope="module")
def planted_graph():
    return _graph("planted")


@pytest.mark.parametrize("seed", [0, 1])
def test_planted_graph_is_bit_identical_to_the_run_without_reuse(planted_graph, monkeypatch, seed):
    ip, ix, w = planted_graph
    monkeypatch.delenv("SCAMD_LEIDEN_REUSE", raising=False)
    lab, q, nc, st = _run(ip, ix, w, seed)
    monkeypatch.setenv("SCAMD_LEIDEN_REUSE", "0")
    lab0, q0, nc0, st0 = _run(ip, ix, w, seed)
    print(f"seed {seed}: reuse {st} Q {q!r} nc {nc}\n          hook  {st0} Q {q0!r} nc {nc0}")
    # (three separate-kernel levels at least: the rule is exercised above level 0 as well)
    assert st["levels_first_iteration"] >= 3, st
    assert np.array_equal(lab, lab0) and q == q0 and nc == nc0
    assert st["iterations"] == st0["iterations"]
    assert st["levels_reused"] >= 3 and st0["levels_reused"] == 0, (st, st0)
    assert st["quiet_reuse_iterations"] == 1 and st0["quiet_reuse_iterations"] == 0, (st, st0)
    assert st["launches"] < st0["launches"]


def test_weak_graph_keeps_the_guarantees():
    from oracle import leiden_guarantees as lg
    from scanpy_amd import _kernels as K

    ip, ix, w = _graph("weak")
    lab, q, nc, st = _run(ip, ix, w, 0)
    lab2, q2, nc2, st2 = _run(ip, ix, w, 0)
    print(f"weak: Q {q!r}, {nc} communities, {st}")
    assert np.array_equal(lab, lab2) and q == q2 and nc == nc2 and st == st2  # reproducible
    import torch

    assert abs(K.modularity(ip, ix, w, N, torch.from_numpy(lab).to(ip.device)) - q) < 1e-8
    conn = sparse.csr_matrix((w.cpu().numpy(), ix.cpu().numpy(), ip.cpu().numpy()), shape=(N, N))
    im = lg.improving_moves(conn, lab)
    mp = lg.mergeable_pairs(conn, lab)
    same = lab[np.repeat(np.arange(N), np.diff(conn.indptr))] == lab[conn.indices]
    inner = sparse.csr_matrix((same.astype(np.int8), conn.indices.copy(), conn.indptr.copy()), shape=conn.shape)
    inner.eliminate_zeros()
    n_comp, _ = connected_components(inner, directed=False)
    print(f"weak: improving moves {im['count']} (max gain {im['max_gain']:.3e}), mergeable pairs {mp['count']}, "
          f"{n_comp} components of {nc} communities")
    assert nc > 1 and nc == int(lab.max()) + 1 and n_comp == nc
    assert im["count"] == 0, im
    assert mp["count"] == 0, mp
