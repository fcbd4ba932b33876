"""The case table of tests/pearson_cases.py on the HOST emulator (tests/emu/README.md): the kernels of csrc/pearson.hip
(`scamd_pp_pearson_gene_var_f32`, `scamd_pp_pearson_residuals_f32`), the same cases and the same checker as
tests/test_gpu_pearson.py.  The emulator says nothing about rates; it does say whether a workgroup finds its gene and its chunk,
whether the chunks of one gene add up, whether the tail of the totals is swept, whether a wave finds the first entry of its
column window, and whether every cell of the matrix is written once and nothing beyond it.  The kernels use no cross-lane
operation: `partial_collectives`, `mixed_collectives` and `reads_of_inactive_lanes` stay 0."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT))

import pearson_cases as P  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build as emu_build
    import harness

    if not Path(emu_build.CLANG).exists():
        pytest.skip("no clang++ to build the host emulation of the kernels")
    lib = harness.load()
    return harness, lib, P.PearsonAbi(lib, harness.HostMem())


def test_table_covers_the_issue_and_sources_still_say_so():
    """no GPU, no emulator"""
    P.assert_table_covers_the_issue()
    P.assert_sources_still_say_so()


def test_restatement_on_values_worked_by_hand():
    """no GPU, no emulator.  x = [[1, 0], [1, 2]]: s = (2, 2), t = (1, 3), T = 4, mu = [[.5, .5], [1.5, 1.5]]; Poisson, no clip:
    r = (x - mu) / sqrt(mu)"""
    x = np.array([[1.0, 0.0], [1.0, 2.0]])
    r = P.restate_residuals(x, np.inf, np.inf)
    want = np.array([[0.5 / np.sqrt(0.5), -0.5 / np.sqrt(0.5)], [-0.5 / np.sqrt(1.5), 0.5 / np.sqrt(1.5)]])
    assert np.allclose(r, want, rtol=1e-15, atol=0)
    assert np.allclose(P.restate_gene_var(x, np.inf, np.inf), np.var(want, axis=0), rtol=1e-15, atol=0)
    assert (P.restate_residuals(x, np.inf, 0.0) == 0).all() and np.abs(P.restate_residuals(x, 100.0, 0.5)).max() == 0.5
    codes = np.array([0, 1])
    assert (P.restate_gene_var(x, 100.0, 3.0, codes, 0) == 0).all()   # one cell: no variance; gene 1 absent: 0, not NaN


def test_library_states_the_same_constants(emu):
    H, lib, abi = emu
    P.assert_library_agrees(lib)


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_every_case(emu, name):
    """the gene variance of every batch within the derived bound (collapsed totals and the plain sweep), NaN and 0 where the
    reference has them, the residual matrix within its tolerance in both output types between untouched guard words; the
    determinism cases bit-identical on a second run and, for the variance, with the rows permuted"""
    H, lib, abi = emu
    lib.emu_reset_stats()
    P.run_case(abi, name, label="emulator")
    st = H.stats(lib)
    assert st["partial_collectives"] == st["mixed_collectives"] == st["reads_of_inactive_lanes"] == 0, (name, st)


def test_argument_checks_start_no_kernel(emu):
    H, lib, abi = emu
    P.run_argument_checks(abi, launches=lib.emu_launches)


def test_worst_observed_ratios_stay_below_one(emu):
    """(runs after the table: prints what DESIGN.md 3.15 records)"""
    print("worst observed error / bound on the emulator:", P.worst)
    assert P.worst["var"] <= 1.0 and P.worst["resid64"] <= 1.0
