"""The cell tables of the pruned and of the approximate kNN search (csrc/knn.hip) on the HOST emulator (tests/emu/README.md)
against numpy float64, and the approximate lists against the rows those tables name: the cases and checkers of
tests/knn_cell_cases.py, which tests/test_gpu_knn_cells.py runs on the GPU.  No GPU.  The emulator build's sweep keeps 4 cells in
its LDS table (the GPU's 64), so at 16 cells nprobe 4 | 5 and 8 | 9 straddle a refill; where a case is not about the queries
it asks for a shard of them, the tables cover every row either way."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import knn_cell_cases as K  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build as emu_build
    import harness

    if not Path(emu_build.CLANG).exists():
        pytest.skip("no clang++ to build the host emulation of the kernels")
    lib = harness.load()
    return lib, harness.Abi(lib, harness.HostMem())


def test_every_cell_path_has_a_case():
    assert K.assert_every_cell_path_has_a_case() == [8, 16, 25, 32]


@pytest.mark.parametrize("case", K.GEOMETRY_CASES + (K.OFFSET_CASE,), ids=lambda c: c.name)
def test_exact_pruned_tables(emu, monkeypatch, case):
    K.run_exact_case(emu[1], monkeypatch.setenv, case, "emulator", shard=K.EMU_SHARD)


@pytest.mark.parametrize(("case", "nprobe"), [(c, p) for c in K.GEOMETRY_CASES for p in K.emu_nprobe(c)],
                         ids=lambda v: v.name if isinstance(v, K.Case) else str(v))
def test_approximate_tables_and_promise(emu, monkeypatch, case, nprobe):
    K.run_approx_case(emu[1], monkeypatch.setenv, case, nprobe, "emulator", shard=K.EMU_SHARD, min_share=K.min_share(case, nprobe),
                      max_fallback=0.05)


def test_all_queries_at_nprobe_3(emu, monkeypatch):
    K.run_approx_case(emu[1], monkeypatch.setenv, K.BY_NAME["d20"], 3, "emulator all queries", min_share=0.1, max_fallback=0.05)


def test_folded_and_empty_cells(emu, monkeypatch):
    K.run_fold_case(emu[1], monkeypatch.setenv, (1, 5), "emulator", shard=K.EMU_FOLD_SHARD)


def test_offset_data_approximate(emu, monkeypatch):
    K.run_approx_case(emu[1], monkeypatch.setenv, K.OFFSET_CASE, 3, "emulator", shard=K.EMU_SHARD, max_fallback=0.05)


@pytest.mark.parametrize("case", K.SCAN_CASES, ids=lambda c: c.name)
def test_after_the_sweep(emu, monkeypatch, case):
    K.run_scan_case(emu[1], monkeypatch.setenv, case, "emulator", shard=K.EMU_SMALL_SHARD)


def test_query_shard(emu, monkeypatch):
    K.run_shard_case(emu[1], monkeypatch.setenv, "emulator")


@pytest.mark.parametrize("nprobe", [0, 3])
def test_tables_are_deterministic(emu, monkeypatch, nprobe):
    K.run_determinism_case(emu[1], monkeypatch.setenv, K.BY_NAME["d50"], nprobe, "emulator", shard=K.EMU_SMALL_SHARD)


def test_shape_answered_exactly_has_no_tables(emu, monkeypatch):
    K.run_exactly_answered_shape(emu[1], monkeypatch.setenv, "emulator", shard=K.EMU_SMALL_SHARD)


def test_debug_entry_argument_checks(emu, monkeypatch):
    lib, abi = emu
    K.run_argument_checks(abi, monkeypatch.setenv, lib.emu_launches, "emulator", shard=K.EMU_SMALL_SHARD)
