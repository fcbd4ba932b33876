"""Host logic of scanpy_amd.pp.scrublet / pp.scrublet_simulate_doublets with the device stage replaced by the float64 restatement
(tests/scrublet_cases.CpuStubScrubletBackend: scipy sums, sklearn PCA / TruncatedSVD, brute-force neighbours, numpy formulas):
every error, warning and refusal, the parents against numpy's generator, the properties the reference's own tests
(tests/test_scrublet.py there) check that need no download, and the restated `threshold_minimum`.  The same front end runs on
the HIP kernels in tests/test_gpu_scrublet.py."""
from __future__ import annotations

import logging
import sys
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
from scipy import sparse

sys.path.insert(0, str(Path(__file__).resolve().parent / "emu"))

import scrublet_cases as S  # noqa: E402

import scanpy_amd as sc  # noqa: E402
from scanpy_amd.preprocessing import _csr_device, _scrublet  # noqa: E402

N, G, T, SEED = 600, 300, 4, 3


@pytest.fixture(autouse=True)
def _stub(monkeypatch):
    monkeypatch.setattr(_csr_device, "default_backend", lambda: S.CpuStubScrubletBackend())


def _adata(n=N, g=G, t=T, seed=SEED, dtype=np.float32):
    x, _ = S.make_counts(n, g, t, seed)
    return sc.AnnData(x.astype(dtype))


@pytest.fixture(scope="module")
def base():
    be = S.CpuStubScrubletBackend()
    old = _csr_device.default_backend
    _csr_device.default_backend = lambda: be
    try:
        a = _adata()
        sc.pp.scrublet(a, rng=7)
    finally:
        _csr_device.default_backend = old
    return a


def test_exported():
    assert {"scrublet", "scrublet_simulate_doublets"} <= set(sc.pp.__all__)
    assert sc.pp.scrublet is _scrublet.scrublet and sc.pp.scrublet_simulate_doublets is _scrublet.scrublet_simulate_doublets


class _Backed:
    is_backed, dtype, shape = True, np.dtype(np.float32), (50, 20)


@pytest.mark.parametrize(("kwargs", "exc", "match"), [
    (dict(rng=1, random_state=2), TypeError, "at most one of `rng` and `random_state`"),
    (dict(batch_key="nope"), ValueError, "`batch_key` must be a column of .obs"),
    (dict(use_approx_neighbors=True), NotImplementedError, "outside the MI355X hot path"),
    (dict(knn_dist_metric="manhattan"), NotImplementedError, "the MI355X kNN kernel offers"),
    (dict(knn_dist_metric=lambda a, b: 0.0), NotImplementedError, "the MI355X kNN kernel offers"),
    (dict(synthetic_doublet_umi_subsampling=0.8), NotImplementedError, "binomial sampler"),
])
def test_refusals(kwargs, exc, match):
    with pytest.raises(exc, match=match):
        sc.pp.scrublet(_adata(), **kwargs)


def test_more_refusals():
    with pytest.raises(NotImplementedError, match="binomial sampler"):
        sc.pp.scrublet_simulate_doublets(_adata(), synthetic_doublet_umi_subsampling=0.5)
    with pytest.raises(TypeError, match="at most one"):
        sc.pp.scrublet_simulate_doublets(_adata(), rng=1, random_state=1)
    with pytest.raises(NotImplementedError, match="float32"):
        sc.pp.scrublet(_adata(dtype=np.float64))
    with pytest.raises(NotImplementedError, match="float32"):
        sc.pp.scrublet_simulate_doublets(_adata(dtype=np.float64))
    a = _adata()
    a.X = _Backed()
    with pytest.raises(NotImplementedError, match="in memory"):
        sc.pp.scrublet(a)
    with pytest.raises(NotImplementedError, match="in memory"):
        sc.pp.scrublet_simulate_doublets(a)
    a = _adata()
    sim = sc.pp.scrublet_simulate_doublets(a, rng=1)
    with pytest.raises(ValueError, match="same genes"):
        sc.pp.scrublet(a[:, np.arange(G) < 100].copy(), adata_sim=sim)
    del sim.obsm["doublet_parents"]
    with pytest.raises(ValueError, match="doublet_parents"):
        sc.pp.scrublet(a, adata_sim=sim)


def test_k_limit_is_checked_before_anything_runs(monkeypatch):
    def no_backend():
        raise AssertionError("the k limit must be checked before the device is touched")

    monkeypatch.setattr(_csr_device, "default_backend", no_backend)
    big = sc.AnnData(sparse.random(30000, 8, density=0.5, format="csr", dtype=np.float32, random_state=0))
    with pytest.raises(NotImplementedError, match=r"k_adj.*at most 256.*29 000 cells.*`batch_key`.*`n_neighbors`"):
        sc.pp.scrublet(big)
    big.obs["batch"] = np.repeat(["a", "b"], 15000)
    with pytest.raises(AssertionError, match="before the device"):     # two batches of 15 000 pass the check
        sc.pp.scrublet(big, batch_key="batch")
    assert _scrublet._k_adjusted(29000, 58000, None) == (85, 255) and _scrublet._k_adjusted(30000, 60000, None)[1] > 256
    with pytest.raises(NotImplementedError, match="k_adj"):
        sc.pp.scrublet(_adata(), n_neighbors=86)                        # 86 * 3 = 258


def test_parents_are_numpys_choice_unravelled(base):
    want = np.vstack(np.unravel_index(np.random.default_rng(7).choice(N * N, 2 * N, replace=False), (N, N))).T
    got = base.uns["scrublet"]["doublet_parents"]
    assert got.shape == (2 * N, 2) and np.array_equal(got, want)
    assert base.uns["scrublet"]["parameters"] == {"expected_doublet_rate": 0.05, "sim_doublet_ratio": 2.0, "n_neighbors": 12}
    assert base.uns["scrublet"]["doublet_scores_sim"].shape == (2 * N,) and base.uns["scrublet"]["doublet_scores_sim"].dtype == np.float64
    assert base.obs["doublet_score"].dtype == np.float64 and base.obs["predicted_doublet"].dtype == bool
    assert 0 < base.obs["predicted_doublet"].sum() < 0.2 * N and "threshold" in base.uns["scrublet"]


def test_legacy_random_state_is_recorded_and_draws_as_sklearn():
    from sklearn.random_projection import sample_without_replacement

    a = _adata()
    sim = sc.pp.scrublet_simulate_doublets(a, sim_doublet_ratio=0.05)    # default: random_state=0
    want = np.vstack(np.unravel_index(sample_without_replacement(N * N, 30, random_state=0), (N, N))).T
    assert np.array_equal(sim.obsm["doublet_parents"], want)
    b = sc.pp.scrublet(a, adata_sim=sc.pp.scrublet_simulate_doublets(a, random_state=3), random_state=3, threshold=0.2, copy=True)
    assert b.uns["scrublet"]["parameters"]["random_state"] == 3
    assert "doublet_score" not in a.obs and "doublet_score" in b.obs      # copy=True leaves the input alone


def test_simulate_doublets_parents_counts_and_matrix():
    a = _adata()
    a.layers["raw"] = a.X.copy()
    sim = sc.pp.scrublet_simulate_doublets(a, layer="raw", sim_doublet_ratio=0.5, rng=11)
    pairs = S.sample_pairs(N, 300, 11)
    assert np.array_equal(sim.obsm["doublet_parents"], pairs)
    want = (a.X[pairs[:, 0]] + a.X[pairs[:, 1]]).tocsr()
    assert sim.X.dtype == np.float32 and (sim.X != want).nnz == 0
    tot = np.asarray(a.X.sum(axis=1)).ravel()
    assert sim.obs["n_counts"].dtype == np.float32 and np.array_equal(sim.obs["n_counts"].to_numpy(), tot[pairs[:, 0]] + tot[pairs[:, 1]])
    assert sim.uns["scrublet"] == {"parameters": {"sim_doublet_ratio": 0.5}}
    sim_i = sc.pp.scrublet_simulate_doublets(_adata(dtype=np.int32), sim_doublet_ratio=0.5, rng=11)
    assert sim_i.obs["n_counts"].dtype == np.int64 and np.array_equal(sim_i.obs["n_counts"].to_numpy(), sim.obs["n_counts"].to_numpy())
    with pytest.raises(ValueError, match="2\\^24"):
        sc.pp.scrublet_simulate_doublets(sc.AnnData(sparse.csr_matrix(np.full((4, 3), 2.0 ** 24, dtype=np.float32))), rng=0)


@pytest.mark.parametrize(("param", "value", "changes"), [
    ("expected_doublet_rate", 0.1, True), ("synthetic_doublet_umi_subsampling", 1.0, False), ("normalize_variance", False, True),
    ("log_transform", True, True), ("mean_center", False, True), ("n_prin_comps", 10, True), ("n_neighbors", 2, True),
    ("threshold", 0.1, True), ("knn_dist_metric", "cosine", True), ("knn_dist_metric", "sqeuclidean", False),
])
def test_parameters_change_or_keep_the_result(base, param, value, changes):
    cur = sc.pp.scrublet(_adata(), rng=7, copy=True, **{param: value})
    same = (np.array_equal(cur.obs["doublet_score"], base.obs["doublet_score"])
            and np.array_equal(cur.obs["predicted_doublet"], base.obs["predicted_doublet"])
            and cur.uns["scrublet"].get("threshold") == base.uns["scrublet"].get("threshold"))
    assert same != changes


def test_main_route_equals_the_manual_composition(base):
    a = _adata()
    sc.pp.filter_genes(a, min_cells=3)
    sc.pp.filter_cells(a, min_genes=3)
    a.layers["raw"] = a.X.copy()
    sc.pp.normalize_total(a)
    logged = a.copy()
    sc.pp.log1p(logged)
    sc.pp.highly_variable_genes(logged)
    a = a[:, logged.var["highly_variable"].to_numpy()].copy()
    sim = sc.pp.scrublet_simulate_doublets(a, layer="raw", rng=7)
    sc.pp.normalize_total(a, target_sum=1e6)
    sc.pp.normalize_total(sim, target_sum=1e6)
    sc.pp.scrublet(a, adata_sim=sim, rng=7)
    np.testing.assert_allclose(a.obs["doublet_score"], base.obs["doublet_score"], rtol=1e-12, atol=0)   # (float64 stand-in)
    assert np.array_equal(a.uns["scrublet"]["doublet_parents"], base.uns["scrublet"]["doublet_parents"])
    assert a.uns["scrublet"]["parameters"]["sim_doublet_ratio"] == 2.0


@pytest.mark.parametrize("batch_key", [None, "batch"])
def test_duplicate_obs_names(batch_key):
    a = _adata()
    a.obs["batch"] = N // 2 * ["a"] + N // 2 * ["b"]
    names = [f"c{i}" for i in range(N // 2)] * 2
    a.obs.index = pd.Index(names)
    sc.pp.scrublet(a, batch_key=batch_key, rng=1)
    assert list(a.obs_names) == names
    assert a.obs["doublet_score"].notna().all() and a.obs["predicted_doublet"].dtype == bool
    if batch_key:
        b = _adata()
        sc.pp.filter_genes(b, min_cells=3)
        want = np.concatenate([sc.pp.filter_cells(_half(h), min_genes=3, inplace=False)[1] for h in (0, 1)])
        assert np.array_equal(a.obs["n_genes"].to_numpy(), want)


def _half(h):
    a = _adata()
    a = a[np.arange(N) // (N // 2) == h].copy()
    sc.pp.filter_genes(a, min_cells=3)
    return a


@pytest.mark.parametrize("batch_key", [None, "batch"])
def test_filtered_cells_come_back_missing(batch_key):
    a = _adata()
    a.obs["batch"] = N // 2 * ["a"] + N // 2 * ["b"]
    dropped = [5, N // 2 + 5]
    x = a.X.tolil()
    x[dropped, :] = 0
    a.X = x.tocsr()
    sc.pp.scrublet(a, batch_key=batch_key, rng=1)
    assert np.flatnonzero(a.obs["doublet_score"].isna()).tolist() == dropped
    assert a.obs["predicted_doublet"].isna().sum() == 2


def test_batched_keys_and_dtypes():
    a = _adata()
    a.obs["batch"] = pd.Categorical(N // 2 * ["a"] + N // 2 * ["b"])
    a.obs["depth"] = np.arange(N, dtype=np.int32)
    sc.pp.scrublet(a, batch_key="batch", rng=2)
    u = a.uns["scrublet"]
    assert set(u) == {"batches", "batched_by"} and u["batched_by"] == "batch" and set(u["batches"]) == {"a", "b"}
    assert a.obs["batch"].dtype == "category" and a.obs["depth"].dtype == np.int32 and a.obs["predicted_doublet"].dtype == bool
    for b in "ab":
        assert u["batches"][b]["doublet_parents"].shape == (N, 2) and u["batches"][b]["doublet_parents"].max() < N // 2
    assert not np.array_equal(u["batches"]["a"]["doublet_parents"], u["batches"]["b"]["doublet_parents"])   # rng.spawn


def test_failed_threshold_follows_the_reference(monkeypatch, caplog):
    def fail(scores):
        raise RuntimeError("Unable to find two maxima in histogram")

    monkeypatch.setattr(_scrublet, "_threshold_minimum", fail)
    a = _adata()
    with caplog.at_level(logging.WARNING, logger="scanpy_amd"):
        sc.pp.scrublet(a, rng=7)
    assert "Failed to automatically identify doublet score threshold" in caplog.text
    assert "threshold" not in a.uns["scrublet"] and not a.obs["predicted_doublet"].any() and a.obs["doublet_score"].notna().all()


def test_verbose_prints_the_three_rates(caplog):
    with caplog.at_level(logging.INFO, logger="scanpy_amd"):
        sc.pp.scrublet(_adata(), rng=7, threshold=0.2)
    for line in ("Running Scrublet", "Embedding transcriptomes using PCA...", "Detected doublet rate = ",
                 "Estimated detectable doublet fraction = ", "Overall doublet rate:", "Scrublet finished"):
        assert line in caplog.text
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="scanpy_amd"):
        sc.pp.scrublet(_adata(), rng=7, threshold=0.2, verbose=False, mean_center=False)
    assert "Detected doublet rate" not in caplog.text and "Truncated SVD" in caplog.text


def test_neighbor_parents_and_zero_variance():
    a = _adata()
    sim = sc.pp.scrublet_simulate_doublets(a, rng=4)
    b = sc.pp.scrublet(a, adata_sim=sim, threshold=0.2, get_doublet_neighbor_parents=True, copy=True)
    lists = b.uns["scrublet"]["doublet_neighbor_parents"]
    assert len(lists) == N and all(np.array_equal(v, np.unique(v)) and (v < N).all() for v in lists) and any(len(v) for v in lists)
    x = a.X.tolil()
    x[:, 0] = 0
    a.X = x.tocsr()
    with pytest.raises(ValueError, match="zero variance"):
        sc.pp.scrublet(a, adata_sim=sim, threshold=0.2)
    sc.pp.scrublet(a, adata_sim=sim, threshold=0.2, normalize_variance=False)     # no scaling: no refusal


# ---- the restated threshold_minimum ----------------------------------------------------------------------------------
def test_threshold_two_clean_modes_one_mode_and_a_plateau():
    rng = np.random.default_rng(0)
    two = np.concatenate([rng.normal(0.1, 0.02, 4000), rng.normal(0.6, 0.05, 1000)])
    th, passes = _scrublet._threshold_minimum(two)
    # between the two maxima by construction; the modes are 5 and 4 standard deviations clear of [0.2, 0.4], so a threshold
    # anywhere in the empty stretch splits the sample 4000 : 1000
    assert 0.1 < th < 0.6 and 1 <= passes < 10000 and (two < th).sum() == 4000
    # one mode, no noise: bin i holds 200 - |i - 128| scores (the two end points fix the range to [0, 1])
    centre = (np.arange(256) + 0.5) / 256
    one = np.concatenate([np.repeat(centre, 200 - np.abs(np.arange(256) - 128)), [0.0, 1.0]])
    with pytest.raises(RuntimeError, match="two maxima"):
        _scrublet._threshold_minimum(one)
    with pytest.raises(RuntimeError):
        _scrublet._threshold_minimum(np.array([]))
    # two flat-topped modes: bins 10 and 11 hold 100 scores each, bins 200 and 201 hold 60 each; a plateau is ONE maximum
    scores = np.concatenate([np.repeat(centre[[10, 11]], 100), np.repeat(centre[[200, 201]], 60), [0.0, 1.0]])
    th, passes = _scrublet._threshold_minimum(scores)
    assert centre[12] < th < centre[199]


@pytest.mark.parametrize(("shape", "threshold", "passes", "called", "planted"), [
    ((600, 300, 4, 3, 7), 0.11795, 856, 32, 48), ((2000, 500, 6, 3, 7), 0.11926, 431, 133, 160)])
def test_threshold_on_the_restatements_scores(shape, threshold, passes, called, planted):
    r = S.ref_generator_run(*shape)
    n = r["n_obs"]
    th, n_pass = _scrublet._threshold_minimum(r["score"][n:])
    assert abs(th - threshold) < 5e-6 and n_pass == passes
    call = r["score"][:n] > th
    assert call.sum() == called and r["planted"].sum() == planted and (call & ~r["planted"]).sum() == 0
