"""The case table of tests/qc_cases.py on the HOST emulator (tests/emu/README.md): the kernels of csrc/qc.hip
(`scamd_pp_qc_sweep_f32`, `scamd_pp_qc_top_f32`), the same cases and checkers as tests/test_gpu_qc.py.  The emulator says nothing
about the hardware's float64 atomics or its handling of subnormals; it does say whether every instantiation indexes, stages, sorts,
selects and reduces correctly.  Also here, needing neither GPU nor emulator: every (lanes per row, masked totals per lane, per-gene
table) of the sweep and both thread counts of the top-n kernel have a case, and the rules' constants still stand in the source.

The loops of both kernels are uniform over the workgroup, so -- unlike the older row-wise kernels -- every cross-lane operation is
executed by a full wave: `partial_collectives`, `mixed_collectives` and `reads_of_inactive_lanes` all stay 0."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT))

import qc_cases as Q  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build as emu_build
    import harness

    if not Path(emu_build.CLANG).exists():
        pytest.skip("no clang++ to build the host emulation of the kernels")
    lib = harness.load()
    return harness, lib, Q.QcAbi(lib, harness.HostMem())


def _only_full_waves(H, lib, what):
    st = H.stats(lib)
    assert st["partial_collectives"] == st["mixed_collectives"] == st["reads_of_inactive_lanes"] == 0, (what, st)


def test_table_covers_every_instantiation_and_branch():
    """no GPU, no emulator"""
    sweep, tops = Q.assert_every_qc_path_has_a_case()
    assert tops == {64, 256} and {(G, mk) for G, mk, _ in sweep} >= {(8, 0), (16, 32), (32, 4), (64, 0)}
    assert [Q.sweep_lanes(a * 100, 100) for a in (0, 32, 33, 160, 161, 512, 513)] == [8, 8, 16, 16, 32, 32, 64]
    assert [Q.top_threads(a * 100, 100, 500) for a in (0, 256, 257)] == [64, 64, 256]
    assert [Q.top_threads(100, 100, p) for p in (2048, 2049, 4096)] == [64, 256, 256]
    assert (Q.top_capacity(64), Q.top_capacity(256)) == (2048, 8192)
    assert (Q.col_table(4096), Q.col_table(4097)) == ("lds", "global")
    assert [Q.sweep_mk(k) for k in (0, 1, 4, 5, 32)] == [0, 4, 4, 32, 32]


def test_sources_still_say_what_the_table_assumes():
    Q.assert_sources_still_say_so()


def test_restatement_on_a_row_worked_by_hand():
    """the rule itself: values 5 3 3 -2 (and a stored 0), positions 1 2 3 6 -> n_max = 6: two zeros of padding rank before -2"""
    import numpy as np
    from scipy import sparse

    x = sparse.csr_matrix(np.array([[3, 0, 5, -2, 3, 0, 0, 0]], dtype=np.float32))
    x.data[1] = 0.0  # (a stored zero: the 5 goes; 3 -2 3 stay)
    top, _ = Q.ref_top(x, (1, 2, 3))        # n_max = 3 = the non-zeros left: no padding
    assert top.tolist() == [[3.0, 6.0, 4.0]]
    top, _ = Q.ref_top(x, (1, 2, 3, 4))     # one zero of padding ranks before the -2
    assert top.tolist() == [[3.0, 6.0, 6.0, 4.0]]
    x = sparse.csr_matrix(np.array([[3, 0, 5, -2, 3, 0, 0, 0]], dtype=np.float32))
    top, _ = Q.ref_top(x, (1, 2, 3, 6))
    assert top.tolist() == [[5.0, 8.0, 11.0, 9.0]]
    top, _ = Q.ref_top(x, (1, 2, 3, 4))     # n_max = 4 = the stored non-zeros: no padding, the -2 is the fourth largest
    assert top.tolist() == [[5.0, 8.0, 11.0, 9.0]]
    top, _ = Q.ref_top(x, (5,))             # one zero of padding
    assert top.tolist() == [[9.0]]


@pytest.mark.parametrize("name", Q.TOP_CASE_NAMES)
def test_sweep_and_top_n_on_every_case(emu, name):
    """per case: row lengths 0, 1, both sides of every position, of 64, of the workgroup, of every power of two the sort pads to
    and of the staging capacity, rows of all g genes, empty rows at both ends and in the middle; the sweep with the LDS and the
    global per-gene table; integer-valued data exactly equal to the restatement and bit-identical on a second run, other data within
    L * 2^-52 * sum|x|"""
    H, lib, qabi = emu
    lib.emu_reset_stats()
    Q.run_top_case(qabi, name, label="emulator")
    _only_full_waves(H, lib, name)


@pytest.mark.parametrize("g", Q.COL_TABLE_G)
def test_per_gene_table_at_its_boundaries(emu, g):
    """g = 1, both sides of the LDS / global split; one column that every row hits, columns nothing hits stay exactly 0"""
    H, lib, qabi = emu
    lib.emu_reset_stats()
    Q.run_col_table_case(qabi, g, label="emulator")
    _only_full_waves(H, lib, f"g={g}")
    assert lib.emu_max_dyn_lds() == (12 * g + 16 if Q.col_table(g) == "lds" else 0)


@pytest.mark.parametrize("part", Q.GRID_CAP_PARTS)
def test_beyond_the_grid_caps(emu, part):
    """one block more than each launch takes, mostly empty rows: the grid-stride trips of both kernels"""
    H, lib, qabi = emu
    lib.emu_reset_stats()
    Q.run_grid_cap_case(qabi, part, label="emulator grid cap")
    _only_full_waves(H, lib, "grid cap")


def test_argument_checks_start_no_kernel(emu):
    H, lib, qabi = emu
    Q.run_argument_checks(qabi, launches=lib.emu_launches)
