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


# keys of the Leiden statistics by slot (scamd_leiden_last_stats / scamd_leiden_stat_name); slot 14 is unused
LEIDEN_STAT_KEYS = ("iterations", "launches", "host_round_trips", "polish_full_sweeps", "polish_rounds", "polish_moves",
                    "polish_skipped_proven", "levels_first_iteration", "lm_sweeps", "lm_sweep_algorithmic_MB", "polish_splits",
                    "ended_by_iteration_cap", "polish_ended_by_round_cap", "iteration_cap", None, "device_fills",
                    "levels_reused", "quiet_reuse_iterations", "overflow_pass_vertices", "hub_pass_vertices")


def check_leiden_stat_keys(lib, stats: dict):
    """the dict a Python layer builds from the library's table has exactly the keys written out above, in slot order, and
    scamd_leiden_stat_name knows no slot outside them"""
    assert tuple(stats) == tuple(k for k in LEIDEN_STAT_KEYS if k is not None)
    for slot, key in enumerate(LEIDEN_STAT_KEYS):
        got = lib.scamd_leiden_stat_name(slot)
        assert (got is None) if key is None else (got.decode() == key), (slot, got)
    for slot in (-1, 14, 20):
        assert lib.scamd_leiden_stat_name(slot) is None


def check_leiden_entry_points(lib, P, graph, empty_i32, to_numpy, singletons, node_weights, ws, stream):
    """The four scamd_leiden_csr_* entries are one run behind four argument lists: two iterations from seed 0 give the same
    membership, Q and community count through each (singleton start, objective 0 where the entry has the argument), and each
    entry still refuses what it alone checks.  P: array -> pointer the library takes; graph = (indptr, indices, weights, n, nnz)
    and `singletons` (arange(n), int32), `node_weights` (float32 [n]), `ws` (uint8 workspace) where the library reads them."""
    import ctypes as C

    ip, ix, w, n, nnz = graph
    head = (P(ip), P(ix), P(w), n, nnz, 1.0, 2, 0.01, 0)

    def call(fn, *mid):
        memb, q, nc = empty_i32(n), C.c_double(-1.0), C.c_int32(-1)
        rc = fn(*head, *mid, P(memb), C.byref(q), C.byref(nc), P(ws), ws.nbytes if hasattr(ws, "nbytes") else ws.numel(), stream)
        return rc, to_numpy(memb), q.value, nc.value

    null = C.c_void_p(0)
    runs = {"csr": call(lib.scamd_leiden_csr_f32), "init": call(lib.scamd_leiden_csr_init_f32, P(singletons)),
            "ex": call(lib.scamd_leiden_csr_ex_f32, 0, null), "nw": call(lib.scamd_leiden_csr_nw_f32, 0, null, null)}
    rc0, memb0, q0, nc0 = runs["csr"]
    assert rc0 == 0 and nc0 == int(memb0.max()) + 1 and 1 < nc0 < n and q0 > 0.0
    for name, (rc, memb, q, nc) in runs.items():
        assert rc == 0 and q == q0 and nc == nc0 and np.array_equal(memb, memb0), name
    EINVAL, EUNSUPPORTED = -1, -4
    assert call(lib.scamd_leiden_csr_init_f32, null)[0] == EINVAL
    assert call(lib.scamd_leiden_csr_ex_f32, 2, null)[0] == EINVAL
    assert call(lib.scamd_leiden_csr_nw_f32, 2, null, null)[0] == EINVAL
    assert call(lib.scamd_leiden_csr_nw_f32, 0, P(node_weights), null)[0] == EUNSUPPORTED
