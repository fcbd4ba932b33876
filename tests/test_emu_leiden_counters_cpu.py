"""The list builders, the apply step and the community totals of csrc/leiden.hip -- the kernels whose workgroups share a few
counter words, bounded by SCAMD_LEIDEN_COUNT_GRID -- on the HOST-emulated kernels (tests/emu/README.md),
through the test entry scamd_leiden_debug_counters_f32: the case table and checkers of tests/leiden_counter_cases.py, every expected
value recomputed in numpy.  The same table runs on the device in tests/test_gpu_leiden_counters.py, which also runs whole
clusterings against results recorded before the change."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "emu"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))
import leiden_counter_cases as cases  # noqa: E402
import leiden_tier_cases as tier_cases  # noqa: E402


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
        def bounds(lanes):
            a, b, c = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
            assert lib.scamd_leiden_tier_bounds(lanes, C.byref(a), C.byref(b), C.byref(c)) == 0
            return a.value, b.value, c.value

        @staticmethod
        def counters(m, memb, decision, flags, n_cls, salt):
            before = harness.stats(lib)
            out = cases.host_counters(lib, m, memb, decision, flags, n_cls, salt, Emulator.bounds(64)[2])
            after = harness.stats(lib)
            for key in ("partial_collectives", "mixed_collectives", "reads_of_inactive_lanes"):
                assert after[key] == before[key], f"{key}: a ballot or shuffle without its whole wave"
            return out

        @staticmethod
        def leiden(adj, **kw):
            return harness.leiden(lib, adj, **kw)

    Emulator.lib = lib
    return Emulator


@pytest.mark.parametrize("knob", cases.KNOBS, ids=lambda k: f"grid{k or 'default'}")
@pytest.mark.parametrize("name", sorted(cases.UNIT_CASES))
def test_counter_case(run, monkeypatch, name, knob):
    """every flagged vertex once and in the list of its class, the tier lists by row length, totals, moved / blocked and the
    state after the apply step equal to a recomputation; the classes the same in two calls"""
    cases.run_unit_case(run, name, knob, monkeypatch)


def test_entry_refuses_bad_arguments(run):
    import numpy as np

    m, memb, decision, flags, n_cls, salt = cases.unit_case("n4097_base", run.bounds(16))
    block_max = run.bounds(64)[2]
    for bad_memb, bad_cls in ((np.full(4097, 4097, dtype=np.int32), 8), (memb, 3), (memb, 32), (memb, 0)):
        with pytest.raises(AssertionError, match="leiden counters"):
            cases.host_counters(run.lib, m, bad_memb, decision, flags, bad_cls, salt, block_max)


@pytest.mark.parametrize("knob", ("1", "2"))
def test_whole_run_is_the_same_at_every_grid(run, monkeypatch, knob):
    """a whole clustering with long rows in every tier (tests/leiden_tier_cases.py: `boundary_rows`, recorded before the change):
    the recorded labels and modularity with one and with two workgroups per counter word"""
    import hashlib

    import numpy as np

    monkeypatch.setenv(cases.COUNT_GRID_KNOB, knob)
    monkeypatch.setenv("SCAMD_LEIDEN_SMALL", "0")
    monkeypatch.setenv("SCAMD_LEIDEN_QUAD", "1")
    memb, q, nc = run.leiden(tier_cases.case_graph("boundary_rows"), seed=0, n_iterations=2)
    sha, q_hex, want_nc = tier_cases.EXPECTED["boundary_rows"][:3]
    assert (hashlib.sha256(np.ascontiguousarray(memb, dtype=np.int32).tobytes()).hexdigest(), float(q).hex(), nc) == (sha, q_hex, want_nc)
