"""`pp.neighbors -> tl.diffmap -> tl.dpt` end to end on the 700 cells of the pbmc68k fixture: slots, dtypes, shapes, the fall-back
of `tl.dpt` to `tl.diffmap`, and the guard of the width templating of the panel kernels -- `tl.umap(init_pos='spectral')`, which
runs their narrow instantiation, gives the bytes it gave before the diffusion map widened them."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest

import diffmap_cases as D
import scanpy_amd as sc

pytestmark = pytest.mark.gpu

# sha256 of the float64 spectral initialisation and of the float32 layout of `tl.umap` on the fixture graph, recorded on an
# MI355X with the library of the commit BEFORE tl.diffmap (the kernels are bitwise reproducible: tests/test_gpu_umap.py)
SPECTRAL_INIT_SHA256 = "5e94384d591899234fded786cbc746864e8180bf788160eb10080fa3cde11bb8"
UMAP_LAYOUT_SHA256 = "7894a87643cd8822b53ba652f4751f55ab739647cd0934811eb7f59842523e3d"


def _neighbors_adata(pbmc68k):
    adata = sc.AnnData(pbmc68k["X"].copy())
    adata.obsm["X_pca"] = pbmc68k["X_pca"]
    sc.pp.neighbors(adata, n_neighbors=10, use_rep="X_pca")
    return adata


def test_neighbors_diffmap_dpt(pbmc68k):
    adata = _neighbors_adata(pbmc68k)
    adata.uns["iroot"] = 42
    assert sc.tl.diffmap(adata) is None
    basis, evals = adata.obsm["X_diffmap"], adata.uns["diffmap_evals"]
    assert basis.shape == (700, 15) and basis.dtype == np.float32 and evals.shape == (15,) and evals.dtype == np.float32
    assert np.all(np.diff(evals) <= 0) and abs(evals[0] - 1) < 1e-6
    # against scipy on the transition matrix of the same graph
    nb = sc.Neighbors(adata)
    nb.compute_transitions()
    assert nb.transitions_sym.dtype == np.float32 and nb.transitions_sym.shape == (700, 700)
    lam, _ = D.eigen_truth(nb.transitions_sym, 15)
    np.testing.assert_allclose(evals, lam, atol=D.TOL_EVALS + 2.0 ** -24)  # (one float32 rounding of a value <= 1)
    assert sc.tl.dpt(adata) is None
    pt = np.asarray(adata.obs["dpt_pseudotime"])
    assert pt.shape == (700,) and pt.dtype == np.float32 and pt[42] == 0 and pt.max() == 1 and np.isfinite(pt).all()
    assert adata.uns["iroot"] == 42
    want = D.dpt_truth(evals[:10], basis[:, :10], 42)
    assert np.abs(pt.astype(np.float64) - want).max() < D.TOL_PSEUDOTIME
    row = sc.Neighbors(adata, n_dcs=10).distances_dpt[42]  # the DPT distances themselves, not divided by their maximum
    assert row.dtype == np.float32 and row.max() != 1 and np.abs(row / row.max() - pt).max() < 4 * 2.0 ** -24  # (three float32 roundings of values <= 1)
    # key_added, copy
    out = sc.tl.diffmap(adata, 5, key_added="dm", copy=True)
    assert out is not adata and out.obsm["dm"].shape == (700, 5) and out.uns["dm"]["evals"].shape == (5,) and "dm" not in adata.obsm
    np.testing.assert_allclose(out.uns["dm"]["evals"], evals[:5], atol=4 * D.TOL_EVALS)


def test_dpt_without_diffmap_warns_and_falls_back(pbmc68k):
    adata = _neighbors_adata(pbmc68k)
    adata.uns["iroot"] = 0
    with pytest.warns(UserWarning, match="Trying to run `tl.dpt` without prior call of `tl.diffmap`"):
        sc.tl.dpt(adata)
    assert adata.obsm["X_diffmap"].shape == (700, 15) and adata.obs["dpt_pseudotime"].iloc[0] == 0


def test_spectral_umap_bytes_are_those_of_the_narrow_kernels(pbmc68k):
    import torch

    from scanpy_amd.tools import _umap

    adata = sc.AnnData(pbmc68k["X"].copy())
    adata.obsm["X_pca"] = pbmc68k["X_pca"]
    conn = pbmc68k["connectivities"].astype(np.float32).tocsr()
    conn.sort_indices()
    adata.obsp["connectivities"] = conn
    adata.obsp["distances"] = pbmc68k["distances"]
    adata.uns["neighbors"] = dict(connectivities_key="connectivities", distances_key="distances",
                                  params=dict(n_neighbors=10, method="umap"))
    dev = torch.device("cuda")
    ini = _umap._spectral_init(torch.from_numpy(conn.indptr.astype(np.int64)).to(dev), torch.from_numpy(conn.indices.astype(np.int32)).to(dev),
                               torch.from_numpy(conn.data).to(dev), 700, 2, 0)
    sc.tl.umap(adata, init_pos="spectral")
    got = (hashlib.sha256(np.ascontiguousarray(ini).tobytes()).hexdigest(),
           hashlib.sha256(np.ascontiguousarray(adata.obsm["X_umap"]).tobytes()).hexdigest())
    print("spectral init / umap layout sha256:", got)
    assert got == (SPECTRAL_INIT_SHA256, UMAP_LAYOUT_SHA256)
