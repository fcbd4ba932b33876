"""Shared comparison helpers for parity tests."""
from __future__ import annotations

import numpy as np


def knn_sets_equal_mod_ties(idx_a, dist_a, idx_b, dist_b, *, rtol=1e-6, atol=1e-9):
    """Compare two kNN results (rows sorted by distance).  Returns the number of rows whose index
    SETS differ for a reason other than a tie at the k-th distance."""
    idx_a, idx_b = np.asarray(idx_a), np.asarray(idx_b)
    dist_a, dist_b = np.asarray(dist_a, dtype=np.float64), np.asarray(dist_b, dtype=np.float64)
    assert idx_a.shape == idx_b.shape
    bad = 0
    sa, sb = np.sort(idx_a, axis=1), np.sort(idx_b, axis=1)
    differ = np.flatnonzero((sa != sb).any(axis=1))
    for r in differ:
        only_a = np.setdiff1d(idx_a[r], idx_b[r])
        only_b = np.setdiff1d(idx_b[r], idx_a[r])
        da = dist_a[r][np.isin(idx_a[r], only_a)]
        db = dist_b[r][np.isin(idx_b[r], only_b)]
        kth = max(dist_a[r].max(), dist_b[r].max())
        # all symmetric-difference members must sit at the k-th distance (a genuine tie)
        tol = atol + rtol * kth
        if not (np.all(np.abs(da - kth) <= tol) and np.all(np.abs(db - kth) <= tol)):
            bad += 1
    return bad, len(differ)


def csr_from_parts(indptr, indices, data, n):
    from scipy import sparse

    return sparse.csr_matrix((np.asarray(data), np.asarray(indices), np.asarray(indptr)), shape=(n, n))


def long_rows_graph():
    """3000 vertices with eight random neighbours each, five of them given 150, 250, 500, 1200 and 2500 more; symmetrised,
    float32.  The smallest rows in every bucket of the Leiden decide kernels: 97-192 entries overflow from the 16-lane table
    only, 193-384 from the 16- and the 32-lane tables, longer ones are hub rows (2500: still one pass of the hub table)."""
    from scipy import sparse

    rng = np.random.default_rng(2)
    n, deg = 3000, 8
    m = sparse.coo_matrix((rng.random(n * deg).astype(np.float32) * 0.9 + 0.1, (np.repeat(np.arange(n), deg), rng.integers(0, n, n * deg))),
                          shape=(n, n)).tocsr()
    for h, dh in ((0, 150), (1, 250), (2, 500), (3, 1200), (4, 2500)):
        t = rng.choice(n, dh, replace=False)
        m = m + sparse.coo_matrix((rng.random(dh).astype(np.float32) * 0.5 + 0.1, (np.full(dh, h), t)), shape=(n, n)).tocsr()
    m.setdiag(0)
    m.eliminate_zeros()
    return m.maximum(m.T).tocsr().astype(np.float32)
