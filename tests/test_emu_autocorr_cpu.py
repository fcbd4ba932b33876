"""The case table of tests/autocorr_cases.py on the HOST emulator (tests/emu/README.md): the kernels of csrc/graph_autocorr.hip
(`scamd_graph_autocorr_slab_{f32,f64}`, `scamd_graph_weight_sum_f64`, `scamd_csr_dense_slab_f32`, `scamd_transpose_slab_{f32,f64}`),
the same cases and the same checker as tests/test_gpu_autocorr.py.  The emulator says nothing about the gather rate; it does say
whether every instantiation finds its first row, steps over empty rows, shares a hub row between parts, masks the lanes beyond
ncols and adds its partial sums in the order it promises.  Also here, needing neither GPU nor emulator: every instantiation and
both reachable sides of every sizing rule have a case, and the rules' constants still stand in the source.

The only cross-lane operation of these kernels is the `readfirstlane` of the wave index at the top of the edge sweep, reached by
all 64 lanes of every wave (the waves that pad the last workgroup leave after it, whole): `partial_collectives`,
`mixed_collectives` and `reads_of_inactive_lanes` all stay 0; no masked tail takes part in a collective."""
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy import sparse

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT))

import autocorr_cases as A  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import build as emu_build
    import harness

    if not Path(emu_build.CLANG).exists():
        pytest.skip("no clang++ to build the host emulation of the kernels")
    lib = harness.load()
    return harness, lib, A.AutocorrAbi(lib, harness.HostMem())


def _only_full_waves(H, lib, what):
    st = H.stats(lib)
    assert st["partial_collectives"] == st["mixed_collectives"] == st["reads_of_inactive_lanes"] == 0, (what, st)


def test_table_covers_every_instantiation_and_rule():
    """no GPU, no emulator"""
    sweeps, builders = A.assert_table_covers_every_path()
    assert len(sweeps) == 4 and len(builders) >= 5


def test_sources_still_say_what_the_table_assumes():
    A.assert_sources_still_say_so()


def test_restatement_on_graphs_worked_by_hand():
    """no GPU, no emulator: two cells (I = -1, C = 1), the block graphs (C = 0 exactly, I = 1 exactly), a permutation of the
    cells moves nothing but rounding"""
    graph, x = A.two_cells()
    assert A.restate(*graph, x) == (-1.0, 1.0)
    g, x = A.block_graph(30)
    assert A.restate(g.indptr, g.indices, g.data, x)[1] == 0.0
    g, x = A.block_graph(50)
    assert A.restate(g.indptr, g.indices, g.data, x)[0] == 1.0
    indptr, indices, w = A.case_graph("n1000-m1")
    v = A.case_values("n1000-m1")[:, 0].astype(np.float64)
    g = sparse.csr_matrix((w, indices, indptr), shape=(1000, 1000))
    perm = np.random.default_rng(0).permutation(1000)
    gp = g[perm][:, perm].tocsr()
    np.testing.assert_allclose(A.restate(gp.indptr, gp.indices, gp.data, v[perm]), A.restate(indptr, indices, w, v), rtol=1e-12)


def test_hand_cases(emu):
    """two cells: I == -1.0 and C == 1.0; the reference's block graphs: C == 0.0 exactly, |I - 1| <= 1e-14"""
    H, lib, abi = emu
    lib.emu_reset_stats()
    A.run_hand_cases(abi, label="emulator")
    _only_full_waves(H, lib, "hand cases")


@pytest.mark.parametrize("name", A.CASE_NAMES)
def test_every_case(emu, name):
    """per case: min / max exactly, the mean and W_sum to 1e-12, constant columns exactly those with min == max, I and C within
    atol 1e-11 / rtol 1e-9 of the float64 restatement, nothing written beyond ncols; the hub cases bit-identical on a second
    run and with the columns reversed"""
    H, lib, abi = emu
    lib.emu_reset_stats()
    A.run_case(abi, name, label="emulator")
    _only_full_waves(H, lib, name)


def test_hub_row_is_shared_by_parts(emu):
    H, lib, abi = emu
    indptr, _, _ = A.case_graph("hub")
    pe = lib.scamd_graph_autocorr_part_entries(int(indptr[-1]))
    first, last = int(indptr[A.HUB_ROW]) // pe, (int(indptr[A.HUB_ROW + 1]) - 1) // pe
    assert last - first + 1 >= 3, (pe, first, last)


def test_rows_in_flight_change_no_bit(emu, monkeypatch):
    """SCAMD_AUTOCORR_UNROLL = 4 / 8 (both instantiations of the sweep): the entries are added in the same order"""
    H, lib, abi = emu
    runs = []
    for unroll in ("8", "4"):
        monkeypatch.setenv("SCAMD_AUTOCORR_UNROLL", unroll)
        lib.emu_reset_stats()
        runs.append([A.case_stats(abi, name)[0] for name in ("hub", "messy", "n1000-m129")])
        _only_full_waves(H, lib, unroll)
    for a, b in zip(*runs):
        for k in A.OUT_KEYS:
            assert a[k].tobytes() == b[k].tobytes(), k


def test_nonfinite_values_stay_in_their_lane(emu):
    H, lib, abi = emu
    A.run_nan_case(abi, label="emulator")


def test_argument_checks_start_no_kernel(emu):
    H, lib, abi = emu
    A.run_argument_checks(abi, launches=lib.emu_launches)
