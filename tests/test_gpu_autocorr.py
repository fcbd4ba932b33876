"""`sc.metrics.morans_i` / `sc.metrics.gearys_c` on the GPU.  Kernel level: the case table of tests/autocorr_cases.py through the
product library (the same cases and the same checker tests/test_emu_autocorr_cpu.py runs on the host emulator); what only the
hardware can say: the wave-wide gathers with four rows in flight, a hub row shared by parts that run at the same time, two runs
giving the same bits.  Front end: the pbmc68k checks of tests/test_autocorr_front_cpu.py end to end on the device."""
from __future__ import annotations

import sys
import warnings
from pathlib import Path

import numpy as np
import pytest
from scipy import sparse

sys.path.insert(0, str(Path(__file__).resolve().parent / "emu"))

import autocorr_cases as A  # noqa: E402

import scanpy_amd as sc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abi():
    from scanpy_amd import _lib

    return A.AutocorrAbi(_lib.load(), A.DeviceMem())


@pytest.fixture(params=[sc.metrics.morans_i, sc.metrics.gearys_c], ids=["morans_i", "gearys_c"])
def metric(request):
    return request.param


def test_hand_cases(abi):
    """two cells: I == -1.0 and C == 1.0; the reference's block graphs: C == 0.0 exactly, |I - 1| <= 1e-14"""
    A.run_hand_cases(abi, label="gpu")


@pytest.mark.parametrize("name", [n for n in A.CASE_NAMES if n not in A.DETERMINISM_CASES])
def test_every_case(abi, name):
    """min / max exactly, the mean and W_sum to 1e-12, constant columns exactly those with min == max, I and C within atol 1e-11 /
    rtol 1e-9 of the float64 restatement, nothing written beyond ncols"""
    A.run_case(abi, name, label="gpu")


@pytest.mark.parametrize("name", A.DETERMINISM_CASES)
def test_hub_graph_twice(abi, name):
    """n = 5000, one row and one other column of 4 000 entries: the hub row spans at least 3 parts; two runs give the same bits,
    and so do the columns in reverse order (a result does not depend on its lane)"""
    indptr, _, _ = A.case_graph(name)
    pe = abi.lib.scamd_graph_autocorr_part_entries(int(indptr[-1]))
    assert (int(indptr[A.HUB_ROW + 1]) - 1) // pe - int(indptr[A.HUB_ROW]) // pe + 1 >= 3, pe
    A.run_case(abi, name, label="gpu", rerun=True)


def test_nonfinite_values_stay_in_their_lane(abi):
    A.run_nan_case(abi, label="gpu")


def test_argument_checks(abi):
    A.run_argument_checks(abi)


def test_front_consistency(metric, pbmc68k):
    A.front_consistency(metric, pbmc68k)


def test_front_raw_matrix_inputs_agree_bit_for_bit(metric, pbmc68k):
    A.front_raw_matrix(metric, pbmc68k)


def test_front_hand_cases_and_graph_from_neighbors(metric):
    (indptr, indices, w), x = A.two_cells()
    g = sparse.csr_matrix((w, indices, indptr), shape=(2, 2))
    assert sc.metrics.morans_i(g, x) == -1.0 and sc.metrics.gearys_c(g, x) == 1.0
    g, x = A.block_graph(30)
    assert sc.metrics.gearys_c(g, x) == 0.0 and sc.metrics.gearys_c(g, sparse.csr_matrix(x))[0] == 0.0
    g, x = A.block_graph(50)
    assert abs(sc.metrics.morans_i(g, x) - 1.0) <= 1e-14
    # `test_metrics_graph_params`: the graph `pp.neighbors` writes (float32 weights), under its own key and under the default
    rng = np.random.default_rng(0)
    adata = sc.AnnData(rng.normal(size=(300, 20)).astype(np.float32))
    sc.pp.neighbors(adata, key_added="bar")
    by_key = metric(adata, neighbors_key="bar")
    assert adata.obsp["bar_connectivities"].dtype == np.float32 and by_key.shape == (20,) and np.isfinite(by_key).all()
    assert by_key.tobytes() == metric(sc.AnnData(adata.X, obsp=adata.obsp), use_graph="bar_connectivities").tobytes()
    A.assert_close(by_key, A.restate_metric(metric, adata.obsp["bar_connectivities"], adata.X.astype(np.float64)))
    with pytest.raises(KeyError, match=r"neighbors.*uns"):
        metric(adata)


def test_front_constant_and_nonfinite_features(metric, pbmc68k):
    g = pbmc68k["connectivities"]
    dense = pbmc68k["raw_X"].T.tocsr()[:130].toarray()
    full = metric(g, dense)
    const = np.array([0, 63, 64, 129])
    other = ~np.isin(np.arange(130), const)
    zero, fortytwo = dense.copy(), dense.copy()
    zero[const], fortytwo[const] = 0.0, 42.0
    for vals in (zero, sparse.csr_matrix(zero), fortytwo, sparse.csc_matrix(fortytwo)):
        with pytest.warns(UserWarning, match=r"4 variables were constant, will return nan for these") as rec:
            out = metric(g, vals)
        assert len(rec) == 1 and np.isnan(out[const]).all() and out[other].tobytes() == full[other].tobytes()
    dirty = dense.astype(np.float64)
    dirty[5, 100] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = metric(g, dirty)
        assert np.isnan(metric(g, np.full(700, 42.0)))
    assert np.isnan(out[5]) and np.isfinite(np.delete(out, 5)).all()
    A.assert_close(np.delete(out, 5), np.delete(full, 5))
    assert np.isnan(metric(sparse.csr_matrix((700, 700)), dense[:3])).all()   # W_sum == 0: IEEE, no exception
