"""`sc.pp.calculate_qc_metrics` on the GPU.  Kernel level: the case table of tests/qc_cases.py through the product library (the
same cases and checkers tests/test_emu_qc_cpu.py runs on the host emulator); what only the hardware can say: the float64 LDS and
global atomics of the per-gene table, the ordering of subnormals, the grid-stride trips beyond the grid caps.  Front end: the
committed 10x and pbmc68k count matrices against the numpy restatement of the rule and of the column formulas, `filter_cells` on
the new column, and a backed matrix against the in-memory call."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest
from scipy import sparse

sys.path.insert(0, str(Path(__file__).resolve().parent / "emu"))

import qc_cases as Q  # noqa: E402

import scanpy_amd as sc  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def qabi():
    from scanpy_amd import _lib

    return Q.QcAbi(_lib.load(), Q.DeviceMem())


@pytest.mark.parametrize("name", Q.TOP_CASE_NAMES)
def test_sweep_and_top_n_on_every_case(qabi, name):
    """row lengths 0, 1, both sides of every position, of 64, of the workgroup, of every power of two the sort pads to and of the
    staging capacity, rows of all g genes; both per-gene tables; integer-valued data exactly equal to the restatement and
    bit-identical on a second run, other data within L * 2^-52 * sum|x|"""
    Q.run_top_case(qabi, name, label="gpu")


@pytest.mark.parametrize("g", Q.COL_TABLE_G)
def test_per_gene_table_at_its_boundaries(qabi, g):
    Q.run_col_table_case(qabi, g, label="gpu")


@pytest.mark.parametrize("part", Q.GRID_CAP_PARTS)
def test_beyond_the_grid_caps(qabi, part):
    Q.run_grid_cap_case(qabi, part, label="gpu grid cap")


def test_argument_checks(qabi):
    Q.run_argument_checks(qabi)


def _check_against_restatement(adata, qc_vars, percent_top):
    obs, var = sc.pp.calculate_qc_metrics(adata, qc_vars=qc_vars, percent_top=percent_top)
    masks = np.stack([adata.var[v].to_numpy() for v in qc_vars]) if qc_vars else np.zeros((0, adata.n_vars), bool)
    prim = Q.ref_primitives(adata.X, masks, percent_top)
    assert Q.integer_valued(sparse.csr_matrix(adata.X)) and prim["row_total"].max() < 2 ** 24  # counts: every column is exact
    want_obs, want_var = Q.ref_columns(prim, adata.X.dtype, adata.n_obs, qc_vars=qc_vars, percent_top=percent_top)
    Q.assert_frames_equal_columns(obs, want_obs, "obs")
    Q.assert_frames_equal_columns(var, want_var, "var")
    assert obs.index.equals(adata.obs_names) and var.index.equals(adata.var_names)
    return obs, var


def test_10x_fixture_equals_the_restatement_and_feeds_filter_cells():
    adata = sc.read_10x_h5(GOLDEN / "10x_data" / "3.0.0" / "filtered_feature_bc_matrix.h5")
    adata.var["ap"] = adata.var_names.str.startswith("AP")
    adata.var["none"] = False
    assert 0 < adata.var["ap"].sum() < adata.n_vars
    obs, _ = _check_against_restatement(adata, ["ap", "none"], (50, 100, 200, 500))
    assert (obs["total_counts_none"] == 0).all() and obs["pct_counts_in_top_500_genes"].max() <= 100.0
    stored = adata.X.copy()
    sc.pp.calculate_qc_metrics(adata, qc_vars="ap", inplace=True)
    assert (adata.X != stored).nnz == 0 and np.array_equal(adata.obs["n_genes_by_counts"].to_numpy(), obs["n_genes_by_counts"].to_numpy())
    n_genes = adata.obs["n_genes_by_counts"].to_numpy()
    cut = int(np.median(n_genes))
    names = adata.obs_names[n_genes >= cut]
    sc.pp.filter_cells(adata, min_genes=cut)
    assert 0 < adata.n_obs < len(n_genes) and adata.obs_names.equals(names)
    assert np.array_equal(adata.obs["n_genes"].to_numpy(), adata.obs["n_genes_by_counts"].to_numpy())


def test_pbmc68k_counts_equal_the_restatement(pbmc68k):
    adata = sc.AnnData(pbmc68k["counts"].astype(np.float32))
    adata.var["first"] = np.arange(adata.n_vars) < 40
    adata.var["none"] = False
    _check_against_restatement(adata, ["first", "none"], (50, 100, 200, 500))
    as_int = sc.AnnData(pbmc68k["counts"].astype(np.int32))
    as_int.var["first"] = adata.var["first"].to_numpy()
    obs, var = _check_against_restatement(as_int, ["first"], (1, 20))
    assert obs["total_counts"].dtype == np.int64 and var["total_counts"].dtype == np.int64


def test_backed_matrix_equals_the_in_memory_call(tmp_path, monkeypatch):
    from scanpy_amd.preprocessing import _qc

    rng = np.random.default_rng(5)
    x = sparse.random(700, 260, density=0.15, format="csr", dtype=np.float32, random_state=5)
    x.data = np.ceil(x.data * 40).astype(np.float32)
    a = sc.AnnData(x)
    a.var["mt"] = rng.random(260) < 0.1
    sc.write_h5ad(tmp_path / "a.h5ad", a)
    b = sc.read_h5ad(tmp_path / "a.h5ad", backed="r")
    assert b.X.is_backed
    orig = _qc._StreamedQc.__init__
    monkeypatch.setattr(_qc._StreamedQc, "__init__", lambda self, be, x, step=97: orig(self, be, x, step))
    kw = dict(qc_vars=["mt"], percent_top=(1, 10, 100))
    obs_a, var_a = sc.pp.calculate_qc_metrics(a, **kw)
    obs_b, var_b = sc.pp.calculate_qc_metrics(b, **kw)
    assert b.X.is_backed
    for got, want in ((obs_b, obs_a), (var_b, var_a)):
        assert list(got.columns) == list(want.columns)
        for col in want.columns:
            assert got[col].dtype == want[col].dtype and got[col].to_numpy().tobytes() == want[col].to_numpy().tobytes(), col
