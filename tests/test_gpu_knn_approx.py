"""The approximate IVF search (`scamd_knn_l2_ivf_f32`; BASELINE configs[4], the reference's own default above 8192 cells is
approximate: src/scanpy/neighbors/__init__.py:734-739, 769-781) against the exact engine on the same embedding.

What the mode promises: a list is the true nearest neighbours AMONG THE PROBED ROWS, or better (a query whose certificate
fails is scanned over every cell within its bound and gets its exact list).  That promise itself -- every list against the rows
the cell tables say its query could see -- is checked by tests/test_gpu_knn_cells.py.  Asserted here is what follows from it
without the tables: self first, exact float64 distances, ascending, recall rises with nprobe and reaches the exact lists once
every cell is probed; and the front-ends (`pp.neighbors(transformer='ivf')`, `MI355XKNNTransformer(nprobe=)`) reach it.  Recall figures at the
bench's size are measured by bench.py (`knn_approx`)."""
from __future__ import annotations

import sys
from pathlib import Path

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
# (SCAMD_TESTS_ON_EMULATOR=1, tests/emu/README.md: the same tests at sizes a lane-by-lane executor finishes)
SMALL = os.environ.get("SCAMD_TESTS_ON_EMULATOR") == "1"
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _overlapping(n, d, n_c, seed, spread=1.0):
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((n_c, d)) * spread
    return (cent[rng.integers(0, n_c, n)] + rng.standard_normal((n, d))).astype(np.float32)


def _recall(idx, exact):
    import torch

    hit = 0
    for s0 in range(0, idx.shape[0], 32768):
        a, b = idx[s0:s0 + 32768, 1:], exact[s0:s0 + 32768, 1:]
        hit += int((a[:, :, None] == b[:, None, :]).any(2).sum())
    return hit / float(idx.shape[0] * (idx.shape[1] - 1))


@pytest.mark.parametrize(("n", "d", "k"), [(150_000, 50, 15), (70_000, 20, 10), (20_000, 50, 15)] if not SMALL else [(4500, 50, 15)])
def test_recall_rises_with_nprobe_and_reaches_the_exact_lists(n, d, k, monkeypatch):
    import torch

    from scanpy_amd import _kernels as K
    from scanpy_amd import _lib

    lib = _lib.load()
    if SMALL:
        monkeypatch.setenv("SCAMD_KNN_CELL_ROWS", "256")
    x = torch.from_numpy(_overlapping(n, d, 24, n + d)).cuda()
    ei, ed, _ = K.knn(x, k)
    xd = x.double()
    last, n_cells = 0.0, 1024
    for nprobe in (1, 4, 16, 2048):
        idx, dist, _ = K.knn(x, k, nprobe=nprobe)
        assert bool((idx[:, 0] == torch.arange(n, device=idx.device)).all()) and not bool(dist[:, 0].any())
        assert bool((dist[:, 1:] >= dist[:, :-1]).all()) and int(idx.min()) >= 0
        rows = torch.randint(0, n, (2048,), device=idx.device)
        dd = torch.linalg.norm(xd[idx[rows].long()] - xd[rows][:, None, :], dim=2)
        assert float((dd - dist[rows]).abs().max()) < 1e-9
        r = _recall(idx, ei)
        frac = float(lib.scamd_knn_last_select_pairs()) / float(n) ** 2
        print(f"n={n} d={d} k={k} nprobe={nprobe}: recall {r:.4f}, pairs evaluated {frac:.3f} of n^2")
        assert r >= last - 1e-9
        last = r
        if nprobe == 2048:  # every cell: the exact lists (ties may come in either order)
            from oracle import compare as cmp

            assert cmp.knn_rows_differing_beyond_ties(idx.cpu().numpy(), dist.cpu().numpy(), ei.cpu().numpy(), ed.cpu().numpy())[0] == 0
        elif nprobe == 1:
            assert frac < 0.2 and 0.1 < r < 1.0
    assert last == 1.0


def test_front_ends_reach_the_approximate_search():
    import scanpy_amd as sc
    from scanpy_amd import MI355XKNNTransformer
    from scanpy_amd._settings import settings

    n, k = (30_000, 15) if not SMALL else (4500, 15)
    x = _overlapping(n, 50, 24, 3)
    exact = sc.AnnData(x[:, :1])
    exact.obsm["X_pca"] = x
    sc.pp.neighbors(exact, n_neighbors=k, use_rep="X_pca")
    e = exact.obsp["distances"].indices.reshape(n, k - 1)
    old = settings.knn_nprobe
    try:
        settings.knn_nprobe = 2
        a = sc.AnnData(x[:, :1])
        a.obsm["X_pca"] = x
        sc.pp.neighbors(a, n_neighbors=k, use_rep="X_pca", transformer="ivf")
    finally:
        settings.knn_nprobe = old
    g = a.obsp["distances"].indices.reshape(n, k - 1)
    r_ivf = float(np.mean([(np.isin(g[i], e[i])).mean() for i in range(0, n, 7)]))
    assert 0.2 < r_ivf < 1.0 and a.obsp["connectivities"].shape == (n, n) and a.uns["neighbors"]["params"]["n_neighbors"] == k
    t = MI355XKNNTransformer(n_neighbors=k, nprobe=2)
    assert t.get_params()["nprobe"] == 2
    m = t.fit_transform(x)
    assert np.array_equal(m.indices.reshape(n, k - 1), g)  # same engine, same probes: same lists
    full = MI355XKNNTransformer(n_neighbors=k, nprobe=10_000).fit_transform(x)
    assert np.array_equal(np.sort(full.indices.reshape(n, k - 1), axis=1), np.sort(e, axis=1))
    with pytest.raises(ValueError):
        MI355XKNNTransformer(n_neighbors=k, nprobe=-1)
