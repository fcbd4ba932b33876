"""`sc.pp.scrublet` on the GPU.  Kernel level: the pair and score case tables of tests/scrublet_cases.py through the product library
(the same cases and checkers tests/test_emu_scrublet_cpu.py runs on the host emulator).  Pipeline level, on the generator's
counts with planted doublets: the device's neighbour counts against an exact float64 search on the device's own manifold
(check A) and against the float64 restatement after an orthogonal Procrustes rotation (check B), then the public function end
to end.

Check B's exemption: a point error e moves a distance by at most 2 e, so a row of the restatement whose k_adj-th and
(k_adj + 1)-th neighbours are of different kinds and at most 4 e apart may count one neighbour differently; at most 5 % of the
rows may be such rows (in the restatement, rows with a mixed boundary and a relative gap below 1e-4 are 0.9 % and 1.4 %)."""
from __future__ import annotations

import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
from scipy import sparse
from scipy.linalg import orthogonal_procrustes

sys.path.insert(0, str(Path(__file__).resolve().parent / "emu"))

import scrublet_cases as S  # noqa: E402

import scanpy_amd as sc  # noqa: E402

pytestmark = pytest.mark.gpu

E2E = (2000, 500, 6, 3)          # n, g, programmes, seed of the generator
SHAPES = ((2000, 500, 6, 3), (600, 300, 4, 3))


@pytest.fixture(scope="module")
def abi():
    from scanpy_amd import _lib

    return S.ScrubletAbi(_lib.load(), S.DeviceMem())


@pytest.mark.parametrize("name", S.PAIR_CASES)
def test_row_pair_sums_on_every_case(abi, name):
    """bitwise against scipy's sum made canonical and against tot[a] + tot[b]; the 6000-pair case twice with equal bytes"""
    S.run_pair_case(abi, name, label="gpu")


@pytest.mark.parametrize("name", S.SCORE_CASE_NAMES)
def test_scores_on_every_case(abi, name):
    """counts exact; scores and errors equal numpy's bit for bit"""
    S.run_score_case(abi, name, label="gpu")


def test_bad_pairs_and_a_foreign_indptr_raise_their_flags(abi):
    S.run_pair_flag_cases(abi)


def test_argument_checks(abi):
    S.run_pair_argument_checks(abi)


# ---- the manifold and the neighbour counts -----------------------------------------------------------------------------
N_SELF = 5


@lru_cache(maxsize=None)
def _manifold_run(shape, n_self=0):
    """the `adata_sim=` route on all genes -> (what the private hook saw, the restatement on the same counts).  n_self: the
    first simulated doublets are made (i, i) instead (no restatement then: such a doublet ties with its cell everywhere)"""
    n, g, t, seed = shape
    x, _ = S.make_counts(n, g, t, seed)
    pairs = S.sample_pairs(n, 2 * n, 7)
    pairs[:n_self] = np.arange(n_self)[:, None]
    sim_counts = S.expected_pairs(x, pairs.astype(np.int32))
    ref = None if n_self else S.ref_call(S.ref_normalize(x), S.ref_normalize(sim_counts))
    a = sc.AnnData(x.copy())
    sim = sc.AnnData(sim_counts.astype(np.float32))
    sim.obsm["doublet_parents"] = pairs
    sc.pp.normalize_total(a, target_sum=1e6)
    sc.pp.normalize_total(sim, target_sum=1e6)
    seen = {}
    sc.pp.scrublet(a, adata_sim=sim, threshold=0.2, verbose=False, _hook=seen.update)
    seen["pairs"] = pairs
    return seen, ref


def _exact_counts(manifold, n_obs, k_adj):
    """float64 brute force on the given points: candidates by the Gram form, then their distances again by differences (exact
    differences of float32 values) -> (n_sim_neigh, rows whose k_adj-th and (k_adj + 1)-th distances tie across kinds, the two
    points at that boundary)"""
    m = manifold.astype(np.float64)
    sq = (m * m).sum(axis=1)
    counts = np.empty(len(m), dtype=np.int64)
    tied = np.zeros(len(m), dtype=bool)
    boundary = np.empty((len(m), 2), dtype=np.int64)
    for lo in range(0, len(m), 1000):
        blk = m[lo: lo + 1000]
        d2 = sq[lo: lo + 1000, None] + sq[None, :] - 2.0 * (blk @ m.T)
        cand = np.argpartition(d2, k_adj + 4, axis=1)[:, : k_adj + 5]
        diff = m[cand] - blk[:, None, :]
        exact = (diff * diff).sum(axis=2)
        order = np.lexsort((cand, exact), axis=1)
        cand, exact = np.take_along_axis(cand, order, axis=1), np.take_along_axis(exact, order, axis=1)
        kinds = cand >= n_obs
        counts[lo: lo + 1000] = kinds[:, :k_adj].sum(axis=1)
        tied[lo: lo + 1000] = (exact[:, k_adj - 1] == exact[:, k_adj]) & (kinds[:, k_adj - 1] != kinds[:, k_adj])
        boundary[lo: lo + 1000] = cand[:, k_adj - 1: k_adj + 1]
    return counts, tied, boundary


@pytest.mark.parametrize("shape", SHAPES)
def test_counts_against_the_devices_own_manifold(shape):
    """check A, and the scores as the formulas of the device's counts.

    The only exemption is a row whose k_adj-th and (k_adj + 1)-th distances are exactly equal and of different kinds.  These
    inputs are NOT free of such rows: `default_rng(7).choice` draws the parents (i, i) four times at n = 600 ((347, 347),
    (376, 376), (266, 266), (571, 571)) and once at n = 2000 ((1622, 1622)), such a doublet sits exactly on its cell (a separate
    test), and every other point is then equally far from both.  So instead of "no such row" this asserts what explains each
    one: the two points at a tied boundary are a cell and its own (i, i) doublet; a tied row may differ by one."""
    seen, ref = _manifold_run(shape)
    n_obs, k_adj, man, pairs = seen["n_obs"], seen["k_adj"], seen["manifold"], seen["pairs"]
    assert k_adj == ref["k_adj"] and man.dtype == np.float32 and man.shape == (3 * n_obs, 30)
    want, tied, boundary = _exact_counts(man, n_obs, k_adj)
    twins = {(int(pairs[r, 0]), n_obs + int(r)) for r in np.flatnonzero(pairs[:, 0] == pairs[:, 1])}
    print(f"scrublet check A {shape}: {int(tied.sum())} rows tie across kinds at the boundary; (i, i) doublets: {sorted(twins)}")
    for row in np.flatnonzero(tied):
        assert tuple(sorted(int(v) for v in boundary[row])) in twins, (row, boundary[row])
    got = seen["n_sim_neigh"].astype(np.int64)
    assert np.array_equal(got[~tied], want[~tied]), np.flatnonzero((got != want) & ~tied)[:10]
    assert (np.abs(got[tied] - want[tied]) <= 1).all()
    ld, se = S.ref_scores(seen["n_sim_neigh"], k_adj, 0.05, 2.0, 0.02)
    assert seen["score"].tobytes() == ld.tobytes() and seen["score_err"].tobytes() == se.tobytes()


def test_a_doublet_of_a_cell_with_itself_sits_exactly_on_the_cell():
    seen, _ = _manifold_run(SHAPES[1], N_SELF)
    n_obs, man = seen["n_obs"], seen["manifold"].astype(np.float64)
    for i in range(N_SELF):
        assert ((man[n_obs + i] - man[i]) ** 2).sum() == 0.0, i      # distance exactly 0


@pytest.mark.parametrize("shape", SHAPES)
def test_counts_against_the_restatement(shape):
    """check B"""
    seen, ref = _manifold_run(shape)
    k_adj = ref["k_adj"]
    dev = seen["manifold"].astype(np.float64)
    rot, _ = orthogonal_procrustes(dev, ref["manifold"])
    e = float(np.sqrt((((dev @ rot) - ref["manifold"]) ** 2).sum(axis=1)).max())
    print(f"scrublet check B {shape}: largest row error after the Procrustes rotation e = {e:.3e} "
          f"(manifold scale {float(np.abs(ref['manifold']).max()):.3e})")
    kinds = ref["neighbors"] >= ref["n_obs"]
    assert ref["dist"].shape[1] == k_adj + 1
    last, nxt = ref["dist"][:, k_adj - 1], ref["dist"][:, k_adj]
    mixed = kinds[:, k_adj - 1] != (ref["neighbors_next"] >= ref["n_obs"])
    exempt = mixed & (nxt - last <= 4 * e)
    differ = seen["n_sim_neigh"].astype(np.int64) - kinds.sum(axis=1)
    print(f"scrublet check B {shape}: exempt rows {exempt.mean():.4%}, rows that differ {np.count_nonzero(differ)}")
    assert (differ[~exempt] == 0).all(), np.flatnonzero((differ != 0) & ~exempt)[:10]
    assert (np.abs(differ[exempt]) <= 1).all()
    assert exempt.mean() <= 0.05


# ---- end to end ------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _e2e():
    x, planted = S.make_counts(*E2E)
    a = sc.AnnData(x.copy())
    sc.pp.scrublet(a, rng=7, verbose=False)
    return a, planted


def test_end_to_end_finds_the_planted_doublets():
    a, planted = _e2e()
    assert "threshold" in a.uns["scrublet"] and a.obs["predicted_doublet"].dtype == bool
    called = a.obs["predicted_doublet"].to_numpy()
    print(f"scrublet end to end: threshold {a.uns['scrublet']['threshold']:.5f}, called {called.sum()}, of them planted "
          f"{(called & planted).sum()}, planted {planted.sum()}")
    assert called.sum() > 0 and (called & planted).sum() >= 0.9 * called.sum()
    assert (called & planted).sum() >= 0.5 * planted.sum()


def test_two_runs_are_bit_identical():
    a, _ = _e2e()
    b = sc.AnnData(S.make_counts(*E2E)[0].copy())
    sc.pp.scrublet(b, rng=7, verbose=False)
    assert a.obs["doublet_score"].to_numpy().tobytes() == b.obs["doublet_score"].to_numpy().tobytes()
    assert a.uns["scrublet"]["doublet_scores_sim"].tobytes() == b.uns["scrublet"]["doublet_scores_sim"].tobytes()
    assert np.array_equal(a.obs["predicted_doublet"], b.obs["predicted_doublet"])


def test_equals_the_manual_composition_of_the_public_pieces():
    a, _ = _e2e()
    m = sc.AnnData(S.make_counts(*E2E)[0].copy())
    sc.pp.filter_genes(m, min_cells=3)
    sc.pp.filter_cells(m, min_genes=3)
    m.layers["raw"] = m.X.copy()
    sc.pp.normalize_total(m)
    logged = m.copy()
    sc.pp.log1p(logged)
    sc.pp.highly_variable_genes(logged)
    m = m[:, logged.var["highly_variable"].to_numpy()].copy()
    sim = sc.pp.scrublet_simulate_doublets(m, layer="raw", rng=7)
    sc.pp.normalize_total(m, target_sum=1e6)
    sc.pp.normalize_total(sim, target_sum=1e6)
    sc.pp.scrublet(m, adata_sim=sim, rng=7, verbose=False)
    assert np.array_equal(m.uns["scrublet"]["doublet_parents"], a.uns["scrublet"]["doublet_parents"])
    assert m.obs["doublet_score"].to_numpy().tobytes() == a.obs["doublet_score"].to_numpy().tobytes()
    assert m.uns["scrublet"]["doublet_scores_sim"].tobytes() == a.uns["scrublet"]["doublet_scores_sim"].tobytes()
    assert m.uns["scrublet"]["threshold"] == a.uns["scrublet"]["threshold"]


def test_batch_key_writes_both_entries():
    a = sc.AnnData(S.make_counts(*E2E)[0].copy())
    a.obs["sample"] = np.repeat(["s1", "s2"], E2E[0] // 2)
    sc.pp.scrublet(a, batch_key="sample", rng=7, verbose=False)
    u = a.uns["scrublet"]
    assert u["batched_by"] == "sample" and set(u["batches"]) == {"s1", "s2"}
    assert a.obs["doublet_score"].notna().all() and len(u["batches"]["s1"]["doublet_scores_sim"]) == E2E[0]


def test_the_k_limit():
    big = sc.AnnData(sparse.random(30000, 8, density=0.5, format="csr", dtype=np.float32, random_state=0))
    with pytest.raises(NotImplementedError, match="k_adj"):
        sc.pp.scrublet(big)
    a = sc.AnnData(S.make_counts(3000, 300, 4, 5)[0].copy())
    sc.pp.scrublet(a, n_neighbors=85, rng=1, threshold=0.2, verbose=False)          # k_adj = 255
    assert a.obs["doublet_score"].notna().all() and a.uns["scrublet"]["parameters"]["n_neighbors"] == 85
