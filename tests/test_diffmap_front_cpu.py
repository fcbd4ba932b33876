"""The front ends `tl.diffmap` / `tl.dpt` and the diffusion-map slice of `Neighbors` on a machine WITHOUT a GPU: the argument
errors and their messages (raised before anything touches the library), `n_dcs` beyond what is stored, the `key_added` slots
and `copy=True`.  Where a test needs eigenpairs the three kernel wrappers are replaced by the CPU truth of
tests/diffmap_cases.py; the kernels themselves are tested by tests/test_emu_diffmap_cpu.py and tests/test_gpu_diffmap.py."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import diffmap_cases as D
import scanpy_amd as sc
from scanpy_amd._anndata import AnnData
from scanpy_amd.neighbors import Neighbors


def _adata(name="pbmc"):
    a = D.graph_input(name)["a"]
    n = a.shape[0]
    x = np.random.default_rng(0).standard_normal((n, 6)).astype(np.float32)
    return AnnData(x, obsp={"connectivities": a.copy(), "distances": a.copy()},
                   uns={"neighbors": {"connectivities_key": "connectivities", "distances_key": "distances",
                                      "params": {"n_neighbors": 10, "method": "umap"}}})


@pytest.fixture
def no_library(monkeypatch):
    """every way into the kernel library fails the test"""
    from scanpy_amd import _device, _lib

    def boom(*a, **k):
        raise AssertionError("the call reached the kernel library")

    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_device, "require_gpu", boom)


@pytest.fixture
def cpu_kernels(monkeypatch):
    """the three wrappers of scanpy_amd/_kernels.py as their CPU truth, on torch CPU tensors; counts the calls"""
    from scipy import sparse

    from scanpy_amd import _device, _kernels

    calls = {"transitions_sym": 0, "diffmap": 0, "dpt_pseudotime": 0}
    monkeypatch.setattr(_device, "require_gpu", lambda: torch.device("cpu"))

    def transitions_sym(indptr, indices, weights, n, *, density_normalize=True):
        calls["transitions_sym"] += 1
        a = sparse.csr_matrix((weights.numpy(), indices.numpy(), indptr.numpy()), shape=(n, n))
        t, z = D.transitions_truth(a, density_normalize)
        return torch.from_numpy(t.data.astype(np.float32)), torch.from_numpy(z)

    def diffmap(indptr, indices, t_sym, n, n_comps, *, seed=0, **kw):
        calls["diffmap"] += 1
        t = sparse.csr_matrix((t_sym.numpy(), indices.numpy(), indptr.numpy()), shape=(n, n))
        lam, vec = D.eigen_truth(t, n_comps)
        return torch.from_numpy(lam.copy()), torch.from_numpy(vec.copy()), {"converged": True}

    def dpt_pseudotime(evals, basis, iroot, labels=None, *, scale=True):
        calls["dpt_pseudotime"] += 1
        return torch.from_numpy(D.dpt_truth(evals.numpy(), basis.numpy(), iroot, None if labels is None else labels.numpy(), scale))

    monkeypatch.setattr(_kernels, "transitions_sym", transitions_sym)
    monkeypatch.setattr(_kernels, "diffmap", diffmap)
    monkeypatch.setattr(_kernels, "dpt_pseudotime", dpt_pseudotime)
    return calls


# ---- argument errors: before anything touches the library -------------------------------------------------------------
def test_diffmap_argument_errors(no_library):
    adata = _adata()
    with pytest.raises(ValueError, match="You need to run `pp.neighbors` first to compute a neighborhood graph."):
        sc.tl.diffmap(AnnData(adata.X))
    with pytest.raises(ValueError, match="You need to run `pp.neighbors` first"):
        sc.tl.diffmap(adata, neighbors_key="other")
    for n_comps in (0, 1, 2):
        with pytest.raises(ValueError, match="Provide any value greater than 2 for `n_comps`"):
            sc.tl.diffmap(adata, n_comps)
    with pytest.raises(NotImplementedError, match="n_comps=27.*at most 26 components"):
        sc.tl.diffmap(adata, 27)
    with pytest.raises(TypeError, match="at most one of `rng` and `random_state`"):
        sc.tl.diffmap(adata, rng=1, random_state=2)
    assert not adata.obsm and set(adata.uns) == {"neighbors"}


def test_compute_eigen_argument_errors(no_library):
    nb = Neighbors(_adata())
    with pytest.raises(ValueError, match="Run `.compute_transitions` first."):
        nb.compute_eigen()
    nb._transitions_sym = D.graph_input("pbmc")["t32"]
    with pytest.raises(NotImplementedError, match="sort='increase'"):
        nb.compute_eigen(sort="increase")
    with pytest.raises(NotImplementedError, match="n_comps=0"):
        nb.compute_eigen(n_comps=0)
    with pytest.raises(NotImplementedError, match="at most 26 components"):
        nb.compute_eigen(n_comps=27)


def test_empty_rows_are_a_value_error(no_library):
    adata = _adata()
    holed = adata.obsp["connectivities"].tolil()
    holed[5, :] = 0
    holed = holed.tocsr()
    holed.eliminate_zeros()
    adata.obsp["connectivities"] = holed
    with pytest.raises(ValueError, match="empty row"):
        Neighbors(adata).compute_transitions()
    nb = Neighbors(adata)
    nb._transitions_sym = holed
    with pytest.raises(ValueError, match="empty row"):
        nb.compute_eigen(n_comps=3)


def test_dpt_argument_errors(no_library):
    adata = _adata()
    with pytest.raises(ValueError, match="You need to run `pp.neighbors` and `tl.diffmap` first."):
        sc.tl.dpt(AnnData(adata.X))
    with pytest.raises(NotImplementedError, match="n_branchings=1: the branching search walks .* separate piece of work"):
        sc.tl.dpt(adata, n_branchings=1)


def test_n_dcs_beyond_what_is_stored(no_library):
    adata = _adata()
    g = D.graph_input("pbmc")
    adata.obsm["X_diffmap"] = g["vec"][:, :5].astype(np.float32)
    adata.uns["diffmap_evals"] = g["lam"][:5].astype(np.float32)
    with pytest.raises(ValueError, match="Cannot instantiate using `n_dcs`=6. Compute diffmap/spectrum with more components first."):
        Neighbors(adata, n_dcs=6)
    adata.uns["iroot"] = 3
    with pytest.raises(ValueError, match="Cannot instantiate using `n_dcs`=10"):
        sc.tl.dpt(adata)  # the default n_dcs=10
    nb = Neighbors(adata, n_dcs=4)
    assert nb.n_dcs == 4 and nb.eigen_values.shape == (4,) and nb.eigen_basis.shape == (700, 4) and nb.iroot == 3


# ---- slots, copy, root cells (kernels replaced by the CPU truth) ------------------------------------------------------
def test_key_added_slots(cpu_kernels):
    from scanpy_amd._settings import settings

    adata = _adata()
    assert sc.tl.diffmap(adata, 4) is None
    assert adata.obsm["X_diffmap"].shape == (700, 4) and adata.obsm["X_diffmap"].dtype == np.float32
    assert adata.uns["diffmap_evals"].shape == (4,) and adata.uns["diffmap_evals"].dtype == np.float32
    np.testing.assert_allclose(adata.uns["diffmap_evals"], D.graph_input("pbmc")["lam"][:4], atol=1e-6)
    adata = _adata()
    sc.tl.diffmap(adata, 4, key_added="dm")
    assert set(adata.obsm) == {"dm"} and set(adata.uns["dm"]) == {"evals"} and adata.uns["dm"]["evals"].shape == (4,)
    # the stored map is found again under its key, and under the V2 preset's key without one
    assert Neighbors(adata, diffmap_key="dm").n_dcs == 4
    adata = _adata()
    old = settings.preset
    try:
        settings.preset = "ScanpyV2Preview"
        sc.tl.diffmap(adata, 4)
    finally:
        settings.preset = old
    assert set(adata.obsm) == {"diffmap"} and adata.uns["diffmap"]["evals"].shape == (4,)
    assert Neighbors(adata).n_dcs == 4
    adata = _adata()
    sc.tl.diffmap(adata, 4, key_added=None)
    assert set(adata.obsm) == {"X_diffmap"}


def test_copy_returns_a_new_object(cpu_kernels):
    adata = _adata()
    adata.uns["iroot"] = 7
    out = sc.tl.diffmap(adata, 5, copy=True)
    assert out is not adata and "X_diffmap" in out.obsm and not adata.obsm and "diffmap_evals" not in adata.uns
    out2 = sc.tl.dpt(out, n_dcs=5, copy=True)
    assert out2 is not out and "dpt_pseudotime" in out2.obs and "dpt_pseudotime" not in out.obs
    pt = np.asarray(out2.obs["dpt_pseudotime"])
    assert pt.dtype == np.float32 and pt[7] == 0 and pt.max() == 1 and out2.uns["iroot"] == 7


def test_transitions_properties(cpu_kernels):
    nb = Neighbors(_adata("toy"))
    nb.compute_transitions()
    f = np.load(D.GOLDEN / "neighbors_toy.npz")
    assert nb.transitions_sym.dtype == np.float32 and nb.transitions_sym.format == "csr"
    np.testing.assert_allclose(nb.transitions_sym.toarray(), f["transitions_sym_umap"], rtol=1e-5)
    np.testing.assert_allclose(nb.transitions.toarray(), f["transitions_umap"], rtol=1e-5)
    np.testing.assert_allclose(nb.Z.diagonal(), 1.0 / D.graph_input("toy")["z"], rtol=1e-12)


def test_dpt_root_cells_and_fallback(cpu_kernels):
    adata = _adata()
    with pytest.warns(UserWarning) as rec:
        sc.tl.dpt(adata)
    texts = [str(w.message) for w in rec]
    assert any(t.startswith("No root cell found.") for t in texts)
    assert any(t.startswith("Trying to run `tl.dpt` without prior call of `tl.diffmap`.") for t in texts)
    assert adata.obsm["X_diffmap"].shape == (700, 15) and "dpt_pseudotime" not in adata.obs and "iroot" not in adata.uns
    # an index out of range is ignored, with a warning
    adata.uns["iroot"] = 700
    with pytest.warns(UserWarning, match="Root cell index 700 does not exist for 700 samples"):
        sc.tl.dpt(adata)
    assert "dpt_pseudotime" not in adata.obs
    # var['xroot']: the nearest cell in X
    del adata.uns["iroot"]
    adata.var["xroot"] = adata.X[123] + 1e-3
    sc.tl.dpt(adata)
    assert adata.uns["iroot"] == 123 and adata.obs["dpt_pseudotime"].iloc[123] == 0
    want = D.dpt_truth(adata.uns["diffmap_evals"][:10], adata.obsm["X_diffmap"][:, :10], 123)
    assert np.array_equal(np.asarray(adata.obs["dpt_pseudotime"]), want)
    assert cpu_kernels["dpt_pseudotime"] == 1


def test_exports():
    assert sc.tl.diffmap.__module__ == "scanpy_amd.tools._diffmap" and sc.tl.dpt.__module__ == "scanpy_amd.tools._dpt"
    assert {"diffmap", "dpt"} <= set(sc.tl.__all__)
