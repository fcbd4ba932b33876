"""The case tables of tests/scrublet_cases.py on the HOST emulator (tests/emu/README.md): the kernels of csrc/scrublet.hip
(`scamd_pp_scrublet_pair_count`, `scamd_pp_scrublet_pair_fill_f32`, `scamd_scrublet_scores_f64`), the same cases and checkers as
tests/test_gpu_scrublet.py.  Also here, needing neither GPU nor emulator: every lane-group size of the three kernels has a case
and the rules' constants still stand in the source.

The merge uses ballots inside its chunk loop, but NOT partial groups: the trip count of that loop is the maximum over the groups
of the wave (a shuffle reduction before the loop), the row loop is uniform over the workgroup, and the score kernel's loop runs
over k, which every row shares.  So every collective is one of a full wave and `partial_collectives`, `mixed_collectives` and
`reads_of_inactive_lanes` all stay 0.

The scores are compared with numpy bit for bit: the emulator's division and square root are the host's IEEE ones, no ulp of
slack is needed here."""
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy import sparse

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT))

import scrublet_cases as S  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build as emu_build
    import harness

    if not Path(emu_build.CLANG).exists():
        pytest.skip("no clang++ to build the host emulation of the kernels")
    lib = harness.load()
    return harness, lib, S.ScrubletAbi(lib, harness.HostMem())


def _only_full_waves(H, lib, what):
    st = H.stats(lib)
    assert st["partial_collectives"] == st["mixed_collectives"] == st["reads_of_inactive_lanes"] == 0, (what, st)


def test_tables_cover_every_lane_group():
    """no GPU, no emulator"""
    assert S.assert_every_pair_path_has_a_case() == {8, 16, 32, 64}
    assert {S.score_lanes(c[2]) for c in S.SCORE_CASES} == {8, 16, 32, 64}
    assert {c[2] for c in S.SCORE_CASES} >= {1, 66, 256}
    assert [S.pair_lanes(a * 100, 100) for a in (0, 32, 33, 160, 161, 512, 513)] == [8, 8, 16, 16, 32, 32, 64]
    assert [S.score_lanes(k) for k in (1, 8, 9, 16, 17, 32, 33, 256)] == [8, 8, 16, 16, 32, 32, 64, 64]


def test_sources_still_say_what_the_tables_assume():
    S.assert_sources_still_say_so()


def test_five_cells_worked_by_hand(emu):
    """5 cells x 6 genes; the unions, sums and totals written out by hand, then the scores of a hand-made neighbour table"""
    H, lib, abi = emu
    dense = np.array([[1, 0, 2, 0, 0, 3],
                      [0, 4, 2, 0, 0, 0],
                      [0, 0, 0, 0, 0, 0],
                      [5, 0, 0, 0, 0, 1],
                      [0, 0, 0, 6, 0, 0]], dtype=np.float32)
    x = sparse.csr_matrix(dense)
    x = sparse.csr_matrix((x.data, x.indices.astype(np.int32), x.indptr.astype(np.int64)), shape=x.shape)
    pairs = np.array([[0, 1], [3, 0], [2, 4], [1, 1], [2, 2]], dtype=np.int32)
    tot = dense.sum(axis=1).astype(np.float64)          # 6, 6, 0, 6, 6
    lib.emu_reset_stats()
    got, total, flags, _ = abi.pairs(x, pairs, tot)
    _only_full_waves(H, lib, "five cells")
    assert flags == 0
    assert got.indptr.tolist() == [0, 4, 7, 8, 10, 10]
    assert got.indices.tolist() == [0, 1, 2, 5, 0, 2, 5, 3, 1, 2]
    assert got.data.tolist() == [1, 4, 4, 3, 6, 2, 4, 6, 8, 4]
    assert total.tolist() == [12, 12, 6, 12, 0]
    # 2 observed + 1 simulated row, k = 3: counts 1, 0, 2.  rho = 0.25, r = 0.5, se_rho = 0.05:
    idx = np.array([[0, 2, 1], [1, 0, 0], [2, 2, 1]], dtype=np.int32)
    rc, cnt, score, err = abi.scores(idx, 2, 0.25, 0.5, 0.05)
    assert rc == 0 and cnt.tolist() == [1, 0, 2]
    # q = (nd + 1) / 5; 1 - rho - rho / r = 0.25; score = q * 0.5 / (0.75 - 0.25 q)
    assert np.allclose(score, [0.4 * 0.5 / 0.65, 0.2 * 0.5 / 0.7, 0.6 * 0.5 / 0.6], rtol=1e-15)
    q = 0.4
    se_q = np.sqrt(q * 0.6 / 6)
    assert np.isclose(err[0], q * 0.5 / 0.65 ** 2 * np.sqrt((se_q / q * 0.75) ** 2 + (0.05 / 0.25 * 0.6) ** 2), rtol=1e-14)


@pytest.mark.parametrize("name", S.PAIR_CASES)
def test_row_pair_sums_on_every_case(emu, name):
    """bitwise against scipy's sum made canonical and against tot[a] + tot[b]; the 6000-pair case twice with equal bytes"""
    H, lib, abi = emu
    lib.emu_reset_stats()
    S.run_pair_case(abi, name, label="emulator")
    _only_full_waves(H, lib, name)


@pytest.mark.parametrize("name", S.SCORE_CASE_NAMES)
def test_scores_on_every_case(emu, name):
    H, lib, abi = emu
    lib.emu_reset_stats()
    S.run_score_case(abi, name, label="emulator")
    _only_full_waves(H, lib, name)


def test_bad_pairs_and_a_foreign_indptr_raise_their_flags(emu):
    H, lib, abi = emu
    S.run_pair_flag_cases(abi)


def test_argument_checks_start_no_kernel(emu):
    H, lib, abi = emu
    S.run_pair_argument_checks(abi, launches=lib.emu_launches)
