"""The cell tables of the pruned and of the approximate kNN search (csrc/knn.hip) on the GPU against numpy float64, and the
approximate lists against the rows those tables name: the cases and checkers of tests/knn_cell_cases.py through the product
library (tests/test_emu_knn_cells_cpu.py runs them on the host emulator).  Here the sweep's cell table holds 64 entries, so the
refill is crossed at 128 cells (n = 32768) by nprobe 64 | 65; the 16-cell geometries run every nprobe of the table."""
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


@pytest.fixture(scope="module")
def abi():
    import harness
    from graph_kernel_cases import DeviceMem
    from scanpy_amd import _lib

    return harness.Abi(_lib.load(), DeviceMem())


def test_every_cell_path_has_a_case():
    assert K.assert_every_cell_path_has_a_case() == [8, 16, 25, 32]


@pytest.mark.parametrize("case", K.GEOMETRY_CASES + (K.OFFSET_CASE,) + K.BIG_CASES, ids=lambda c: c.name)
def test_exact_pruned_tables(abi, monkeypatch, case):
    K.run_exact_case(abi, monkeypatch.setenv, case, "gpu")


@pytest.mark.parametrize(("case", "nprobe"), [(c, p) for c in K.GEOMETRY_CASES for p in K.NPROBE_16],
                         ids=lambda v: v.name if isinstance(v, K.Case) else str(v))
def test_approximate_tables_and_promise(abi, monkeypatch, case, nprobe):
    fig, _ = K.run_approx_case(abi, monkeypatch.setenv, case, nprobe, "gpu", min_share=K.min_share(case, nprobe), max_fallback=0.05)
    if nprobe >= 16:  # every cell probed, still through the approximate plan: the exact lists
        assert fig["R_ne_E"] == 0.0


@pytest.mark.parametrize(("case", "nprobe"), [(c, p) for c in K.BIG_CASES for p in K.NPROBE_128],
                         ids=lambda v: v.name if isinstance(v, K.Case) else str(v))
def test_refill_of_the_64_entry_cell_table(abi, monkeypatch, case, nprobe):
    K.run_approx_case(abi, monkeypatch.setenv, case, nprobe, "gpu", sample=K.BIG_SAMPLE, max_fallback=0.05)


def test_folded_and_empty_cells(abi, monkeypatch):
    K.run_fold_case(abi, monkeypatch.setenv, (1, 5), "gpu")


def test_offset_data_approximate(abi, monkeypatch):
    K.run_approx_case(abi, monkeypatch.setenv, K.OFFSET_CASE, 3, "gpu", max_fallback=0.05)


@pytest.mark.parametrize("case", K.SCAN_CASES, ids=lambda c: c.name)
def test_after_the_sweep(abi, monkeypatch, case):
    K.run_scan_case(abi, monkeypatch.setenv, case, "gpu")


def test_query_shard(abi, monkeypatch):
    K.run_shard_case(abi, monkeypatch.setenv, "gpu")


@pytest.mark.parametrize("nprobe", [0, 3])
def test_tables_are_deterministic(abi, monkeypatch, nprobe):
    K.run_determinism_case(abi, monkeypatch.setenv, K.BY_NAME["d50"], nprobe, "gpu")


def test_shape_answered_exactly_has_no_tables(abi, monkeypatch):
    K.run_exactly_answered_shape(abi, monkeypatch.setenv, "gpu")


def test_debug_entry_argument_checks(abi, monkeypatch):
    K.run_argument_checks(abi, monkeypatch.setenv, None, "gpu")
