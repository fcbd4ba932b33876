"""The two raw entry points of csrc/rank_genes.hip on the HOST emulator (tests/emu/README.md) against the dense integer
oracle of tests/rank_genes_cases.py, exactly; no GPU.  The matrix is the shape table's with ONE chunk boundary crossed (about
chunk + 100 rows: columns of 0, 1, 2, 63, 64, 65, chunk - 1, chunk, chunk + 1 entries, a dense column of two chunks, one
giant tie, negatives, stored 0.0 / -0.0, heavy ties); the GPU suite runs the same table across three chunks.  The emulator
says nothing about LDS limits or timing; it does say whether the sort network, the searches across chunks and the closed
form of the zero block index and count correctly, and it counts cross-lane operations executed by partial waves."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import rank_genes_cases as R  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build as emu_build
    import harness

    if not Path(emu_build.CLANG).exists():
        pytest.skip("no clang++ to build the host emulation of the kernels")
    lib = harness.load()
    return harness, lib, R.RankGenesAbi(lib, harness.HostMem())


@pytest.fixture(scope="module")
def matrices(emu):
    lib = emu[1]
    return {c: R.kernel_matrix(c, chunks=1) for c in {lib.scamd_rank_genes_chunk_entries(k) for k in (2, 17, R.MAX_GROUPS)}}


def _no_partial_wave_collectives(H, lib):
    st = H.stats(lib)
    assert st["partial_collectives"] == st["mixed_collectives"] == st["reads_of_inactive_lanes"] == 0, st


def test_chunk_entries_shrink_with_the_group_count(emu):
    lib = emu[1]
    small, big = lib.scamd_rank_genes_chunk_entries(2), lib.scamd_rank_genes_chunk_entries(R.MAX_GROUPS)
    assert small >= big > 0 and small & (small - 1) == 0 and big & (big - 1) == 0
    assert 8 * (16 + 3 * R.MAX_GROUPS + big) <= 64 * 1024  # the LDS tables of the largest group count


# the emulator runs the small group counts, the reference first and last, and the maximum once each way
@pytest.mark.parametrize(("n_groups", "reference"), [(2, -1), (2, 1), (17, -1), (17, 0), (17, 16), (R.MAX_GROUPS, R.MAX_GROUPS - 1)])
def test_wilcoxon_case(emu, matrices, n_groups, reference):
    H, lib, abi = emu
    lib.emu_reset_stats()
    R.run_wilcoxon_case(abi, matrices[lib.scamd_rank_genes_chunk_entries(n_groups)], n_groups, reference, label="emulator")
    _no_partial_wave_collectives(H, lib)


@pytest.mark.parametrize("n_groups", [2, 17])
def test_group_stats_case(emu, matrices, n_groups):
    H, lib, abi = emu
    lib.emu_reset_stats()
    xt = matrices[lib.scamd_rank_genes_chunk_entries(n_groups)]
    worst = R.run_stats_case(abi, xt, n_groups, label="emulator")
    print(f"emulator group_stats n_groups={n_groups}: worst error / bound = {worst:.3f}")
    R.run_stats_transform_case(abi, xt[:, :12], n_groups, 0.7, label="emulator")
    _no_partial_wave_collectives(H, lib)


def test_argument_checks_start_no_kernel(emu):
    H, lib, abi = emu
    R.run_argument_checks(abi, launches=lib.emu_launches)
