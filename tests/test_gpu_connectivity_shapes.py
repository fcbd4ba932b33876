"""Every shape of the connectivity kernels (csrc/fuzzy.hip: scamd_fuzzy_simplicial_set_f32, scamd_gauss_connectivities_f32,
scamd_jaccard_connectivities_f32, and the row-sharded pair scamd_fuzzy_weights_f32 / scamd_fuzzy_merge_rows_f32) on the GPU,
at kernel level: the tables, input builders and checkers of tests/graph_kernel_cases.py, which
tests/test_emu_graph_shapes_cpu.py runs on the host emulator.  The neighbour lists are built on the host (float64 brute force,
the row itself in column 0), so nothing here depends on the kNN kernel.  What only the hardware can say: the wave ballots of
fss_fill_kernel, the DPP rotations and the xor-16 shuffle of fss_recip_rec_kernel, and v_exp_f32 in the first phase of the
bisection for sigma -- sigma is demanded bit-equal to the oracle's float64 bisection."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "emu"))

import graph_kernel_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def abi():
    import harness

    from scanpy_amd import _lib

    return harness.Abi(_lib.load(), G.DeviceMem())


@pytest.mark.parametrize(("n", "k", "kind"), G.CONN_CASES)
def test_connectivity_case(abi, n, k, kind):
    """umap, gauss and jaccard on one (n, k, data kind) of the table: pattern, ascending columns, exact symmetry, rho and
    sigma bit-equal, values within the method's bound"""
    G.run_connectivity_case(abi, n, k, kind, label="gpu")


@pytest.mark.parametrize("extra_in_edge", [False, True])
def test_sortrows_lds_block_at_and_over_its_cap(abi, extra_in_edge):
    """every block of 32 rows holds exactly SR_CAP = 2048 entries (the LDS path at its cap); with one in-only entry more, one
    block holds 2049 and takes the wave-per-row path"""
    G.run_sortrows_boundary(abi, extra_in_edge, label="gpu")


def test_sigma_on_extreme_rows(abi):
    """zero, constant, 40-decade, near-denormal, subnormal, 1e30 and one-ulp-apart distance rows: sigma and rho bit-equal to
    both forms of the oracle"""
    G.run_extreme_rows(abi, label="gpu")


@pytest.mark.parametrize(("n", "k", "cuts"), G.SHARD_CASES)
def test_sharded_pair_is_bitwise_the_single_call(abi, n, k, cuts):
    """no processes: weights shard by shard (an empty and a one-row shard among them), in-edges routed with numpy, merged
    rows concatenated -- bitwise the single call's indptr, indices and data"""
    G.run_sharded_case(abi, n, k, cuts, label="gpu")


def test_connectivity_argument_checks(abi):
    """k = 1, k = 257, a capacity one entry short, a workspace one byte short: the documented codes"""
    G.run_connectivity_argument_checks(abi)
