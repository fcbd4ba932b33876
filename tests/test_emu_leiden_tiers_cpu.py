"""The tiers of a Leiden decide step (csrc/leiden.hip `decide_tiers`: main, wave-per-row and block tier in ONE launch, the giant
tier in a launch of its own; tier lists written by the list builders) on the HOST-emulated kernels (tests/emu/README.md):
the case table of tests/leiden_tier_cases.py, whose recorded figures are those of the build that ran the tiers one launch
behind the other.  The emulator runs every case at its full size, the dense ones too (three lane settings each: `all_block_rows` about
half a minute, `all_giant_rows` one to one and a half, `long_rows_with_polish` with its 22 iterations about two)."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))
import leiden_tier_cases as cases  # noqa: E402


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


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_tier_case(run, monkeypatch, name):
    """same partition with 64, 16 and 32 lanes per vertex, Q is the labels' modularity, every tier the case is for was
    reached, and labels, Q, sweeps, iterations and the tier statistics are the recorded ones"""
    cases.run_case(run, name, monkeypatch, "emu")


def test_tier_bounds_accessor(run):
    """the bounds the graphs were built for; another lane count is refused"""
    for lanes, want in cases.RECORDED_BOUNDS.items():
        assert run.bounds(lanes) == want
    assert run.lib.scamd_leiden_tier_bounds(48, None, None, None) == -1
    assert run.lib.scamd_leiden_tier_bounds(64, None, None, None) == 0

