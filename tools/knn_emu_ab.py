"""A/B of two BUILDS of the host-emulated library (tests/emu) on the kNN search, for a change that must compute the same:
every `harness.knn` call of the kNN tests of tests/test_emu_cpu.py, one line per call with the hashes of its lists and its
counters.

  python tools/knn_emu_ab.py run <libscanpy_amd_emu.so> <out.txt>     one process per build (the parent's library is built from a
                                                                      checkout of the parent: python tests/emu/build.py there)
  python tools/knn_emu_ab.py table <parent.txt> <new.txt>             the merged table; exit status 1 if any line differs
"""
from __future__ import annotations

import hashlib
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def run(lib_path: str, out_path: str) -> int:
    import pytest

    sys.path.insert(0, str(ROOT / "tests" / "emu"))
    import harness

    lib = harness.load(path=lib_path)
    knn, lines, calls = harness.knn, [], {}

    def recorded(lib_, x, k, **kw):
        idx, dist, n_scan = knn(lib_, x, k, **kw)
        test = os.environ.get("PYTEST_CURRENT_TEST", "?").split("::")[-1].split(" ")[0]
        calls[test] = calls.get(test, 0) + 1
        sha = lambda a: hashlib.sha256(a.tobytes()).hexdigest()[:16]  # noqa: E731
        lines.append(f"{test} #{calls[test]} x={x.shape} k={k} idx={sha(idx)} dist={sha(dist)} n_fallback={n_scan} "
                     f"second_tier={lib_.scamd_knn_last_second_tier_queries()} pairs={lib_.scamd_knn_last_select_pairs():.0f} "
                     f"user_counters={harness.user_counters(lib_, 6)}")
        return idx, dist, n_scan

    harness.knn, harness.load = recorded, lambda *a, **kw: lib  # what the `emu` fixture of the tests hands out
    rc = pytest.main([str(ROOT / "tests" / "test_emu_cpu.py"), "-k", "knn", "-q", "-p", "no:cacheprovider"])
    Path(out_path).write_text("\n".join(lines) + "\n")
    return int(rc)


def table(a_path: str, b_path: str) -> int:
    a, b = Path(a_path).read_text().splitlines(), Path(b_path).read_text().splitlines()
    differ = abs(len(a) - len(b))
    for la, lb in zip(a, b):
        differ += la != lb
        print(la + "  same" if la == lb else f"DIFFER\n  parent: {la}\n  new:    {lb}")
    print(f"{len(a)} / {len(b)} calls, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit({"run": run, "table": table}[sys.argv[1]](*sys.argv[2:4]))
