"""The shape tables of tests/pp_umap_kernel_cases.py on the HOST emulator (tests/emu/README.md): the kernels of
csrc/preprocess.hip and csrc/umap.hip, the same cases and checkers as tests/test_gpu_preprocess_shapes.py and
tests/test_gpu_umap_shapes.py, less the cases beyond a grid cap (millions of fibres each).  The emulator says nothing about the
hardware's LDS limit, its float64 LDS atomics or v_exp_f32 / v_log_f32; it does say whether every instantiation indexes, strides
and reduces correctly.  Also here, needing neither GPU nor emulator: the accounting tests -- every (kernel, lanes per row), both
column tables, both output dtypes, every UMAP (lanes per vertex, DIM instantiation) and every number of negative batches has a
case, and the rules' constants still stand in the .hip sources.

What is asserted of the emulator's counters: `reads_of_inactive_lanes == 0` after every case.  `partial_collectives` is
REPORTED, not asserted to be zero: a wave holds 64 / G lane groups, each walks its own row (vertex) and leaves the grid-stride
loop when its rows run out, so the xor-shuffles of the groups that still have a row may be executed by a partial wave -- by design.
A shuffle with an offset below G stays inside the group, whose lanes leave the loop together, so no lane ever reads a lane that
is not there; that is what the first counter proves."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT))

import pp_umap_kernel_cases as P  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build as emu_build
    import harness

    if not Path(emu_build.CLANG).exists():
        pytest.skip("no clang++ to build the host emulation of the kernels")
    lib = harness.load()
    return harness, lib, harness.abi(lib)


def _lanes_read_only_live_lanes(H, lib, what):
    st = H.stats(lib)
    print(f"emulator {what}: {st['launches']} launches, {st['partial_collectives']} collectives by partial waves")
    assert st["reads_of_inactive_lanes"] == 0 and st["mixed_collectives"] == 0, st


def test_tables_cover_every_instantiation_and_branch():
    """no GPU, no emulator"""
    assert P.assert_every_preprocess_path_has_a_case() == {(k, G) for k in P.PP_ROW_KERNELS for G in (8, 16, 32, 64)}
    assert P.assert_every_umap_path_has_a_case() == {(G, d) for G in (4, 8, 16, 32) for d in (2, 3, 0)}
    assert [P.pp_lanes(a * 100, 100) for a in (0, 32, 33, 160, 161, 512, 513)] == [8, 8, 16, 16, 32, 32, 64]
    assert [P.umap_lanes(a * 100, 100) for a in (12, 13, 24, 25, 96, 97)] == [4, 8, 8, 16, 16, 32]
    assert (P.col_table(4096), P.col_table(4097)) == ("lds", "global")


def test_dispatch_constants_still_stand_in_the_sources():
    P.assert_sources_still_say_so()


def test_one_epoch_cannot_move_anything():
    """the schedule alone (no kernel): at epoch 0 no sample fires, whatever the weights"""
    for n_epochs, fires in ((1, False), (2, True)):
        _, _, eps, _ = P.umap_inputs(503, 25, 2, n_epochs)
        assert (P.umap_schedule_stats(eps, n_epochs, 5)[1] > 0) == fires


# ---- preprocess ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("n", "avg"), P.PP_ROW_CASES)
def test_row_wise_kernels_at_every_lane_count(emu, n, avg):
    H, lib, abi = emu
    lib.emu_reset_stats()
    P.run_pp_row_case(abi, n, avg, label="emulator")
    _lanes_read_only_live_lanes(H, lib, f"row case n={n} nnz/n={avg}")


@pytest.mark.parametrize("g", P.PP_COL_TABLE_G)
def test_column_table_at_its_boundaries(emu, g):
    H, lib, abi = emu
    lib.emu_reset_stats()
    P.run_pp_col_table_case(abi, g, label="emulator")
    _lanes_read_only_live_lanes(H, lib, f"column table g={g}")
    # which table the launches used: the LDS one asks for 20 g + 16 bytes of dynamic LDS, the global one for none
    assert lib.emu_max_dyn_lds() == (P.col_table_lds_bytes(g) if P.col_table(g) == "lds" else 0)


@pytest.mark.parametrize("offset", P.PP_LOG1P_OFFSETS)
def test_log1p_head_body_tail(emu, offset):
    H, lib, abi = emu
    P.run_pp_log1p_cases(abi, offset, label="emulator")


def test_log1p_and_dense_fill_beyond_their_grid_caps(emu):
    """(the two grid caps the emulator passes in a few seconds; the row-wise ones take 2 M fibres per launch: GPU only)"""
    H, lib, abi = emu
    P.check_log1p(abi, P.PP_LOG1P_GRID_CAP_COUNT, 1, 2.0, label="emulator grid cap")
    P.run_pp_dense_cap_case(abi, label="emulator 1100x4000")


def test_preprocess_argument_checks_start_no_kernel(emu):
    H, lib, abi = emu
    P.run_pp_argument_checks(abi, launches=lib.emu_launches)


# ---- UMAP ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.UMAP_CASES, ids=lambda c: "n{}-deg{}-dim{}-rate{}-ep{}-alpha{:g}".format(*c))
def test_umap_case(emu, case):
    H, lib, abi = emu
    lib.emu_reset_stats()
    P.run_umap_case(abi, case, label="emulator")
    _lanes_read_only_live_lanes(H, lib, "umap case")


def test_umap_return_codes_and_fixed_points(emu):
    H, lib, abi = emu
    P.run_umap_edges(abi, launches=lib.emu_launches, label="emulator")
