"""One level of a Leiden iteration -- the refinement and the coarse graph (csrc/leiden.hip `refinement`, `aggregate`) -- on the
HOST-emulated kernels (tests/emu/README.md), through the test entry scamd_leiden_debug_level_f32: the cases and checkers of
tests/leiden_level_cases.py, exact against int64 sums.  The same table runs on the device in tests/test_gpu_leiden_level.py;
the cases at the default split bounds (3 10^5 member entries through 1024-thread workgroups) run there only, their code here
through the cases with the split bounds lowered."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))
import leiden_level_cases as cases  # noqa: E402


@pytest.fixture(scope="module")
def run():
    import ctypes as C

    import build as emu_build
    import harness

    if not Path(emu_build.CLANG).exists():
        pytest.skip("no clang++ to build the host emulation of the kernels")
    lib = harness.load()

    class Emulator:
        @staticmethod
        def level(adj, membership, **kw):
            return harness.leiden_level(lib, adj, membership, **kw)

        @staticmethod
        def leiden(adj, **kw):
            return harness.leiden(lib, adj, **kw)

        @staticmethod
        def stats():
            return harness.leiden_stats(lib)

        @staticmethod
        def bounds(lanes):
            a, b, c = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
            assert lib.scamd_leiden_tier_bounds(lanes, C.byref(a), C.byref(b), C.byref(c)) == 0
            return a.value, b.value, c.value

    Emulator.lib = lib
    return Emulator


@pytest.mark.parametrize("name", cases.agg_case_names("emu"))
def test_coarse_graph_case(run, monkeypatch, name):
    """the coarse graph under a given refined partition is P^T Wq P entry for entry, built by the builders the case names"""
    cases.run_agg_case(run, name, monkeypatch)


@pytest.mark.parametrize("name", sorted(cases.FORCED))
def test_coarse_graph_forced_builder(run, monkeypatch, name):
    """every forced builder gives P^T Wq P itself (not merely what another builder gives)"""
    cases.run_forced_case(run, name, monkeypatch)


@pytest.mark.parametrize("seed", cases.SEEDS)
@pytest.mark.parametrize("beta", cases.BETAS)
@pytest.mark.parametrize("name", sorted(cases.REFINE_CASES))
def test_refinement_case(run, monkeypatch, name, beta, seed):
    """nested, connected groups of well-connected vertices whose Kref / Eref / refsize equal a recomputation; the same with 64, 16
    and 32 lanes per vertex and when repeated"""
    cases.run_refine_case(run, name, beta, seed, monkeypatch)


def test_level_entry_refuses_bad_partitions(run):
    """ids outside [0, n), a group not named by a member, a group across two communities"""
    import numpy as np

    m, membership, refined = cases._once("one_group", cases.AGG_CASES["one_group"][0])
    for memb, ref in ((np.full(200, 200), refined), (membership, np.full(200, -1)), (membership, np.where(np.arange(200) < 5, 17, 3)),
                      (np.arange(200) % 2, refined)):
        with pytest.raises(RuntimeError, match="leiden level"):
            run.level(m, memb, refined_in=ref)


def test_renumbering_orders_equal_sizes_by_smallest_member(run):
    cases.check_renumbering(run)


@pytest.mark.parametrize("name", sorted(cases.SMALL_ENTRY_CASES))
def test_one_workgroup_path_at_its_entry_bounds(run, name):
    """n = 17, n = 1024 with 65536 entries (the one-workgroup kernel), with 65538 and n = 1025 (separate kernels)"""
    cases.check_small_entry_case(run, name)
