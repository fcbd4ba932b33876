"""`sc.pp.harmony_integrate`, the public call, on the GPU: shapes, dtypes and determinism on the 700 cells of the pbmc68k fixture;
on a planted input (3000 cells, 3 types x 2 batches) the product against the CPU truth of tests/harmony_cases.py driven with
the product's own centroids and permutations, against the truth run the reference's way by the reference's own acceptance
measure, batch mixing and type separation; `pp.pca -> harmony_integrate -> neighbors -> leiden` end to end."""
from __future__ import annotations

import numpy as np
import pandas as pd
import pytest

import harmony_cases as H
import scanpy_amd as sc
from scanpy_amd.preprocessing import _harmony

pytestmark = pytest.mark.gpu


def _pbmc(pbmc68k):
    adata = sc.AnnData(pbmc68k["X"].copy())
    adata.obsm["X_pca"] = pbmc68k["X_pca"]
    adata.obs["batch"] = pd.Categorical(pbmc68k["bulk_labels_codes"])
    return adata


@pytest.mark.parametrize("flavor", ["harmony2", "harmony1"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_shape_dtype_determinism(pbmc68k, flavor, dtype):
    out = []
    for rng in (0, 0, 1):
        adata = _pbmc(pbmc68k)
        assert sc.pp.harmony_integrate(adata, "batch", flavor=flavor, dtype=dtype, rng=rng, max_iter_harmony=3, max_iter_clustering=20) is None
        z = adata.obsm["X_pca_harmony"]
        assert z.shape == adata.obsm["X_pca"].shape and z.dtype == dtype and np.isfinite(z).all()
        out.append(z)
    assert out[0].tobytes() == out[1].tobytes(), "two runs with one rng differ"
    assert not np.array_equal(out[0], out[2]), "another rng gives the same result"
    assert not np.allclose(out[0], adata.obsm["X_pca"])


def test_max_iter_harmony_1_runs_one_correction(pbmc68k, monkeypatch):
    from scanpy_amd import _kernels

    calls = []
    real = _kernels.harmony_correct
    monkeypatch.setattr(_kernels, "harmony_correct", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    adata = _pbmc(pbmc68k)
    sc.pp.harmony_integrate(adata, "batch", max_iter_harmony=1, max_iter_clustering=5, adjusted_basis="X_h", rng=0)
    assert len(calls) == 1 and adata.obsm["X_h"].shape == (700, adata.obsm["X_pca"].shape[1])


def test_several_keys_are_refused(pbmc68k):
    adata = _pbmc(pbmc68k)
    adata.obs["run"] = pd.Categorical(np.arange(700) % 2)
    with pytest.raises(NotImplementedError, match="general-design ridge solve"):
        sc.pp.harmony_integrate(adata, ["batch", "run"])


# caps small enough for a quick test and large enough for the window test of the clustering (from its fourth iteration on) and the
# outer test to be taken; that none of these decisions sits on a knife edge is asserted on the truth before anything is compared
PLANTED = dict(max_iter_harmony=4, max_iter_clustering=8, tol_harmony=1e-4, tol_clustering=1e-5)


@pytest.fixture(scope="module")
def planted_runs():
    """the product on the planted input, the truth driven with the product's centroids and permutations, and the truth run the
    reference's way; computed once"""
    x, types, codes = H.pipeline_input()
    n, n_levels = x.shape[0], 2
    run = _harmony.HarmonyRun(**PLANTED)
    z_dev = run.fit(x.copy(), codes, n_levels, np.full(n_levels, 2.0), np.random.default_rng(3))
    truth = {}
    for tag, t in (("f64", np.float64), ("ld", np.longdouble)):
        truth[tag] = H.harmony_truth(x.astype(t), codes, n_levels, run.centroids_.astype(t),
                                     lambda rnd: H.device_permutation(n, run.seed_, rnd), **PLANTED)
    cen, perms = H.reference_way_draws(H.unit_rows(x), run.n_clusters_, 11)
    ref_way = H.harmony_truth(x, codes, n_levels, cen, perms, **PLANTED)
    return dict(x=x, types=types, codes=codes, z_dev=z_dev, run=run, truth=truth, ref_way=ref_way)


def test_planted_equals_the_truth_driven_with_its_own_draws(planted_runs):
    p = planted_runs
    z64, i64 = p["truth"]["f64"]
    zld, ild = p["truth"]["ld"]
    print(f"rounds: product {p['run'].rounds_}, truth {i64['rounds']}; closest decision {i64['decision_margin']:.2e} of the objective")
    # precondition: every convergence decision of the truth is at least 1e-9 of the objective from flipping, in both precisions
    assert min(i64["decision_margin"], ild["decision_margin"]) > 1e-9
    assert any(r > 3 for r in i64["rounds"]), "no convergence decision was taken"
    assert p["run"].rounds_ == i64["rounds"] == ild["rounds"]
    assert len(p["run"].objectives_) == len(i64["objectives"])
    H.check_close("gpu", "planted pipeline", "objectives", np.array(p["run"].objectives_), np.array(i64["objectives"], np.float64),
                  np.array(ild["objectives"]))
    H.check_close("gpu", "planted pipeline", "z_hat", p["z_dev"], z64, zld)


def test_planted_public_call_is_the_same_run(planted_runs):
    p = planted_runs
    adata = sc.AnnData(np.zeros((3000, 1), np.float32))
    adata.obsm["X_pca"] = p["x"].copy()
    adata.obs["batch"] = pd.Categorical(p["codes"])
    sc.pp.harmony_integrate(adata, "batch", rng=3, **PLANTED)
    assert adata.obsm["X_pca_harmony"].tobytes() == p["z_dev"].tobytes()


def test_planted_agrees_with_the_reference_way(planted_runs):
    p = planted_runs
    r, l2 = H.acceptance(p["z_dev"], p["ref_way"][0])
    print(f"product vs reference-way truth: min column Pearson r {r:.4f}, relative L2 {l2:.4f}")
    assert r > 0.95 and l2 < 0.1


def test_planted_mixes_batches_and_keeps_types(planted_runs):
    p = planted_runs
    before = H.other_batch_share(p["x"], p["codes"])
    truth_gain = H.other_batch_share(p["ref_way"][0], p["codes"]) - before
    gain = H.other_batch_share(p["z_dev"], p["codes"]) - before
    print(f"share of other-batch neighbours: input {before:.3f}, truth +{truth_gain:.3f}, product +{gain:.3f}")
    assert truth_gain > 0 and gain >= 0.5 * truth_gain
    ari, ari_truth = H.type_ari(p["z_dev"], p["types"]), H.type_ari(p["ref_way"][0], p["types"])
    print(f"ARI of 3-means against the types: product {ari:.4f}, truth {ari_truth:.4f}")
    assert ari >= ari_truth


def test_pca_harmony_neighbors_leiden():
    x, types, codes = H.pipeline_input()
    adata = sc.AnnData(x.astype(np.float32))
    adata.obs["batch"] = pd.Categorical(codes)
    sc.pp.pca(adata, n_comps=10)
    sc.pp.harmony_integrate(adata, "batch", rng=0, max_iter_harmony=2, max_iter_clustering=10)
    sc.pp.neighbors(adata, n_neighbors=15, use_rep="X_pca_harmony")
    sc.tl.leiden(adata, flavor="igraph")
    assert adata.obsm["X_pca_harmony"].shape == (3000, 10) and adata.obs["leiden"].nunique() >= 3
