"""The shape tables of tests/graph_kernel_cases.py on the HOST emulator (tests/emu/README.md): the connectivity kernels of
csrc/fuzzy.hip and the sparse half of PCA of csrc/pca.hip, the same cases and checkers as tests/test_gpu_connectivity_shapes.py
and tests/test_gpu_sparse_pca_shapes.py.  The emulator says nothing about the hardware's ballots, DPP rotations, v_exp_f32 or
LDS limits; it does say whether every instantiation and branch indexes, pads and merges correctly, and it counts cross-lane
operations executed by partial waves.  Also here, needing neither GPU nor emulator: the accounting test -- every instantiation
and branch the restated dispatch rules name has a case, and the rules' constants still stand in the .hip sources."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT))

import graph_kernel_cases as G  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build as emu_build
    import harness

    if not Path(emu_build.CLANG).exists():
        pytest.skip("no clang++ to build the host emulation of the kernels")
    lib = harness.load()
    return harness, lib, harness.abi(lib)


def _no_partial_wave_collectives(H, lib):
    st = H.stats(lib)
    assert st["partial_collectives"] == st["mixed_collectives"] == st["reads_of_inactive_lanes"] == 0, st


def test_tables_cover_every_instantiation_and_branch():
    """no GPU, no emulator"""
    ks = G.assert_every_connectivity_path_has_a_case()
    assert ks == sorted(G.CONN_K)
    assert G.assert_every_sparse_pca_path_has_a_case() == ["quad", "rows<1>", "rows<2>", "rows<3>", "rows<4>"]
    assert G.fill_branches(2, 301) == {"in_wave"} and G.fill_branches(3, 301) == {"in_wave", "prev_wave"}
    assert G.fill_branches(65, 137) == {"in_wave", "prev_wave", "prev_wave_back64"}
    assert G.fill_branches(66, 301) == {"in_wave", "prev_wave", "prev_wave_back64"} and G.fill_branches(67, 301) == set(G.FILL_BRANCHES)
    assert (G.transpose_rows_per_chunk(170000, G.TRANSPOSE_MAX_G), G.transpose_rows_per_chunk(300, G.TRANSPOSE_MAX_G)) == (512, 256)


def test_dispatch_constants_still_stand_in_the_sources():
    G.assert_sources_still_say_so()


# ---- connectivity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("n", "k", "kind"), G.CONN_CASES)
def test_connectivity_case(emu, n, k, kind):
    H, lib, abi = emu
    lib.emu_reset_stats()
    G.run_connectivity_case(abi, n, k, kind, label="emulator")
    _no_partial_wave_collectives(H, lib)


@pytest.mark.parametrize("extra_in_edge", [False, True])
def test_sortrows_lds_block_at_and_over_its_cap(emu, extra_in_edge):
    H, lib, abi = emu
    lib.emu_reset_stats()
    G.run_sortrows_boundary(abi, extra_in_edge, label="emulator")
    _no_partial_wave_collectives(H, lib)


def test_sigma_on_extreme_rows(emu):
    H, lib, abi = emu
    lib.emu_reset_stats()
    G.run_extreme_rows(abi, label="emulator")
    _no_partial_wave_collectives(H, lib)


@pytest.mark.parametrize(("n", "k", "cuts"), G.SHARD_CASES)
def test_sharded_pair_is_bitwise_the_single_call(emu, n, k, cuts):
    H, lib, abi = emu
    lib.emu_reset_stats()
    G.run_sharded_case(abi, n, k, cuts, label="emulator")
    _no_partial_wave_collectives(H, lib)


def test_connectivity_argument_checks_start_no_kernel(emu):
    H, lib, abi = emu
    G.run_connectivity_argument_checks(abi, launches=lib.emu_launches)


# ---- sparse PCA ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", G.SPMM_L)
def test_spmm_case(emu, l):
    H, lib, abi = emu
    lib.emu_reset_stats()
    G.run_spmm_case(abi, l, second_trip=False, label="emulator")
    _no_partial_wave_collectives(H, lib)


@pytest.mark.parametrize("l", G.SPMM_SECOND_TRIP_L)
def test_spmm_second_grid_stride_trip(emu, l):
    H, lib, abi = emu
    G.run_spmm_case(abi, l, second_trip=True, label="emulator")


@pytest.mark.parametrize("l", G.F64ACC_L)
def test_spmm_f64acc_case(emu, l):
    H, lib, abi = emu
    lib.emu_reset_stats()
    G.run_f64acc_case(abi, l, label="emulator")
    _no_partial_wave_collectives(H, lib)


@pytest.mark.parametrize("l", G.COLSUM_L)
def test_colsum_cases(emu, l):
    H, lib, abi = emu
    worst = max(G.run_colsum_case(abi, n, l, label="emulator") for n in G.COLSUM_N)
    print(f"emulator colsum l={l}: worst error / bound = {worst:.3f}")


def test_row_stats_case(emu):
    H, lib, abi = emu
    G.run_row_stats_case(abi, label="emulator")


@pytest.mark.parametrize(("n", "g", "per_row"), G.TRANSPOSE_CASES)
def test_transpose_case(emu, n, g, per_row):
    H, lib, abi = emu
    G.run_transpose_case(abi, n, g, per_row, label="emulator")


def test_sparse_pca_argument_checks_start_no_kernel(emu):
    H, lib, abi = emu
    G.run_spmm_argument_checks(abi, launches=lib.emu_launches)
