"""An iteration's quality from its last level, the starting quality from the level-0 set-up pass (csrc/leiden.hip
`iteration_quality`, `ld_level0_setup_kernel`) on the HOST-emulated kernels (tests/emu/README.md): the case table of
tests/leiden_quality_cases.py, recorded from the emulator build that walked the level-0 graph for every quality.  Labels, Q
(bit for bit), iteration and level counts, round trips and the polish figures are the recorded ones; the level-0 graph is
walked for a quality only where a polish pass, a given start partition or the CPM report needs it."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))
import leiden_quality_cases as cases  # noqa: E402


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
        def raw_stats():
            out = (C.c_int32 * 20)()
            lib.scamd_leiden_last_stats(out, 20)
            return list(out)

    return Emulator


@pytest.mark.parametrize("case", cases.CASES)
def test_quality_case(run, monkeypatch, case):
    cases.run_case(run, case, monkeypatch, "emu")
