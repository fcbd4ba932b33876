"""The sweep tables of the exact pruned kNN search (csrc/knn.hip: max of the ball bound and the projection bound between cells)
on the HOST emulator (tests/emu/README.md) against numpy float64: the cases and checkers of tests/knn_sweep_bound_cases.py,
which tests/test_gpu_knn_sweep_bound.py runs on the GPU.  No GPU.  16 cells of ~256 rows; the emulator build of the reach
kernel takes 4 directions per pass and 2 tiles per block, so every short list (8 cells at least) goes through several passes
and every cell through several blocks, and its sweep keeps 4 cells in its LDS table, so every list is longer than that table."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import knn_cell_cases as K  # noqa: E402
import knn_sweep_bound_cases as B  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build as emu_build
    import harness

    if not Path(emu_build.CLANG).exists():
        pytest.skip("no clang++ to build the host emulation of the kernels")
    lib = harness.load()
    return lib, harness.Abi(lib, harness.HostMem())


@pytest.mark.parametrize("case", B.GEOMETRY_CASES + (K.OFFSET_CASE, B.DUP_CASE, B.TWIN_CASE), ids=lambda c: c.name)
def test_sweep_tables(emu, monkeypatch, case):
    fig, T, W = B.run_case(emu[1], monkeypatch.setenv, case, "emulator", shard=K.EMU_SHARD)
    assert fig["list_max"] > K.META_CELLS["emulator"] and fig["list_max"] > B.REACH_DIRS["emulator"]
    assert fig["tiles_max"] > B.REACH_TILES["emulator"]  # a cell of several blocks of the reach kernel


@pytest.mark.parametrize("case", (B.SIGMA_CASE, B.SIGMA_F32_CASE), ids=lambda c: c.name)
def test_projection_bound_prunes_where_the_ball_bound_cannot(emu, monkeypatch, case):
    B.run_case(emu[1], monkeypatch.setenv, case, "emulator", shard=K.EMU_SHARD, strict_pairs=True, min_strict=B.SIGMA_MIN_SHARE)


def test_folded_and_empty_cells(emu, monkeypatch):
    fig, T, W = B.run_case(emu[1], monkeypatch.setenv, K.FOLD_CASE, "emulator", shard=K.EMU_FOLD_SHARD, min_asymmetric=1)
    assert (T["cell_map"] != range(T["nc"])).sum() >= 2 and (W["list_len"][T["ntiles"] == 0] == 0).all()


def test_query_shard_off_the_block_grid(emu, monkeypatch):
    assert B.SHARD[0] % 128 and B.SHARD[1] % 128
    B.run_case(emu[1], monkeypatch.setenv, B.SIGMA_CASE, "emulator shard", shard=B.SHARD, strict_pairs=True)


def test_tables_are_deterministic(emu, monkeypatch):
    B.run_determinism_case(emu[1], monkeypatch.setenv, B.SIGMA_CASE, "emulator", shard=K.EMU_SMALL_SHARD)


def test_approximate_mode_keeps_the_ball_rows(emu, monkeypatch):
    B.run_approximate_mode(emu[1], monkeypatch.setenv, K.BY_NAME["d20"], 3, "emulator", shard=K.EMU_SMALL_SHARD)
