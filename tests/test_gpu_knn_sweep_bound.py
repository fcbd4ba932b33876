"""The sweep tables of the exact pruned kNN search (csrc/knn.hip: max of the ball bound and the projection bound between cells)
on the GPU against numpy float64: the cases and checkers of tests/knn_sweep_bound_cases.py through the product library
(tests/test_emu_knn_sweep_bound_cpu.py runs them on the host emulator).  Beyond the 16-cell geometries: 32768 rows / 128 cells,
where a short list outgrows the 32 directions a block of the reach kernel takes per pass, overlapping data on which no cell
gets a list, and cells of 1024 rows, which span several blocks of that kernel."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import knn_cell_cases as K  # noqa: E402
import knn_sweep_bound_cases as B  # noqa: E402


@pytest.fixture(scope="module")
def abi():
    import harness
    from graph_kernel_cases import DeviceMem
    from scanpy_amd import _lib

    return harness.Abi(_lib.load(), DeviceMem())


@pytest.mark.parametrize("case", B.GEOMETRY_CASES + (K.OFFSET_CASE, B.DUP_CASE, B.TWIN_CASE), ids=lambda c: c.name)
def test_sweep_tables(abi, monkeypatch, case):
    B.run_case(abi, monkeypatch.setenv, case, "gpu")


@pytest.mark.parametrize("case", (B.SIGMA_CASE, B.SIGMA_F32_CASE), ids=lambda c: c.name)
def test_projection_bound_prunes_where_the_ball_bound_cannot(abi, monkeypatch, case):
    B.run_case(abi, monkeypatch.setenv, case, "gpu", strict_pairs=True, min_strict=B.SIGMA_MIN_SHARE)


@pytest.mark.parametrize("case", B.BIG_CASES, ids=lambda c: c.name)
def test_128_cells(abi, monkeypatch, case):
    sigma = case.data == "sigma"
    fig, T, W = B.run_case(abi, monkeypatch.setenv, case, "gpu", min_strict=B.SIGMA_MIN_SHARE if sigma else None)
    if case.data == "overlap32":  # no structure at the scale of the cells: no lists, the sweep rows are the ball rows
        assert fig["list_max"] == 0 and fig["strict_share"] == 0.0 and fig["cells"] > B.REACH_MAX_LIST
    if case.name == "big-d20":  # lists beyond the 32 directions of a pass of the reach kernel
        assert fig["list_max"] > B.REACH_DIRS["gpu"]
    if "SCAMD_KNN_CELL_ROWS" in case.env:  # cells of several blocks of the reach kernel
        assert fig["tiles_max"] > B.REACH_TILES["gpu"]


def test_folded_and_empty_cells(abi, monkeypatch):
    fig, T, W = B.run_case(abi, monkeypatch.setenv, K.FOLD_CASE, "gpu", min_asymmetric=1)
    assert (T["cell_map"] != range(T["nc"])).sum() >= 2 and (W["list_len"][T["ntiles"] == 0] == 0).all()


def test_query_shard_off_the_block_grid(abi, monkeypatch):
    B.run_case(abi, monkeypatch.setenv, B.SIGMA_CASE, "gpu shard", shard=B.SHARD, strict_pairs=True)


@pytest.mark.parametrize("case", (B.SIGMA_CASE, B.BIG_CASES[0]), ids=lambda c: c.name)
def test_tables_are_deterministic(abi, monkeypatch, case):
    B.run_determinism_case(abi, monkeypatch.setenv, case, "gpu")


def test_approximate_mode_keeps_the_ball_rows(abi, monkeypatch):
    B.run_approximate_mode(abi, monkeypatch.setenv, K.BY_NAME["d20"], 3, "gpu")
