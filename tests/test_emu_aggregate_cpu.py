"""The case table of tests/aggregate_cases.py on the HOST emulator (tests/emu/README.md): the kernels of csrc/aggregate.hip
(`scamd_aggregate_moments_f32`, `scamd_aggregate_median_f32`), the same cases and the same checker as tests/test_gpu_aggregate.py.
The emulator says nothing about rates; it does say whether a part finds its first slot and its group, whether a run is flushed
once and into the right cells, whether the three median tiers pick the right ranks, and whether an exact-size workspace is
enough.  Also here, needing neither GPU nor emulator: every instantiation and both sides of every sizing rule have a case, and
the rules' constants still stand in the source.

The cross-lane operations of these kernels are the shuffles of the in-wave median, reached by all 64 lanes of a wave (a wave
without a pair leaves whole, before them): `partial_collectives`, `mixed_collectives` and `reads_of_inactive_lanes` stay 0."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT))

import aggregate_cases as A  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build as emu_build
    import harness

    if not Path(emu_build.CLANG).exists():
        pytest.skip("no clang++ to build the host emulation of the kernels")
    lib = harness.load()
    return harness, lib, A.AggregateAbi(lib, harness.HostMem())


def _only_full_waves(H, lib, what):
    st = H.stats(lib)
    assert st["partial_collectives"] == st["mixed_collectives"] == st["reads_of_inactive_lanes"] == 0, (what, st)


def test_table_covers_every_instantiation_and_rule():
    """no GPU, no emulator"""
    lanes, seg = A.assert_table_covers_every_path()
    assert len(lanes) == 4


def test_sources_still_say_what_the_table_assumes():
    A.assert_sources_still_say_so()


def test_restatement_on_values_worked_by_hand():
    """no GPU, no emulator: {-3, 0, 0, 5} and {2}: sums 2 and 2, m2 = 2 * 0.25 + 12.25 + 20.25 = 33 and 0, medians 0 and 2"""
    vals = np.array([[-3.0], [0.0], [2.0], [0.0], [5.0], [9.0]], np.float32)
    r = A.restate(vals, np.array([0, 0, 1, 0, 0, -1], np.int32), 3, True)
    assert r["sum"][:, 0].tolist() == [2.0, 2.0, 0.0] and r["m2"][:, 0].tolist() == [33.0, 0.0, 0.0]
    assert r["count_nonzero"][:, 0].tolist() == [2, 1, 0] and r["count_negative"][:, 0].tolist() == [1, 0, 0]
    assert r["median"][0, 0] == 0.0 and r["median"][1, 0] == 2.0 and np.isnan(r["median"][2, 0])
    assert A.middle(1.0, 1.0 + 2.0 ** -23, False, True) != A.middle(1.0, 1.0 + 2.0 ** -23, False, False)
    assert A.middle(2.0 ** 24 - 1, 2.0 ** 24, False, False) == 2.0 ** 24 - 0.5
    assert not np.signbit(A.middle(-0.0, -0.0, True, True))


def test_library_states_the_same_rules(emu):
    H, lib, abi = emu
    A.assert_library_agrees(lib)


@pytest.mark.parametrize("name", A.CASE_NAMES)
def test_every_case(emu, name):
    """per case: the two counts and the median (mid_in_f32 on and off) exactly, sum and m2 within the bounds the header states,
    nothing written beyond [n_groups x g]; the determinism cases bit-identical on a second run and with the rows permuted"""
    H, lib, abi = emu
    lib.emu_reset_stats()
    cs, got, out = A.run_case(abi, name, label="emulator")
    A.check_case_specifics(name, cs, got, out)
    _only_full_waves(H, lib, name)


def test_nonfinite_values_are_flagged_and_stay_in_their_pair(emu):
    H, lib, abi = emu
    A.run_nan_case(abi, label="emulator")


def test_argument_checks_start_no_kernel(emu):
    H, lib, abi = emu
    A.run_argument_checks(abi, launches=lib.emu_launches)
