"""Every `file.py:line[-line]` citation of the reference in the boundary documents points at an existing file and an
existing line range (guards against stale citations).  The reference's files and their line counts are recorded in
tests/golden/reference_line_counts.json (tests/golden/make_golden.py), so the check needs nothing outside the repository."""
from __future__ import annotations

import json
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
LINE_COUNTS = json.loads((ROOT / "tests" / "golden" / "reference_line_counts.json").read_text())
DOCS = ["include/scanpy_amd.h", "INTEGRATION.md", "DESIGN.md"]
CITE = re.compile(r"(?<![\w/.])((?:src/scanpy|tests)/[\w/]+\.py):(\d+)(?:-(\d+))?")


@pytest.mark.parametrize("doc", DOCS)
def test_full_path_citations_resolve(doc):
    text = (ROOT / doc).read_text()
    cites = CITE.findall(text)
    assert cites, f"{doc}: no reference citations found"
    bad = []
    for path, lo, hi in cites:
        if path not in LINE_COUNTS:
            bad.append(f"{path}: no such file")
            continue
        n = LINE_COUNTS[path]
        lo_i, hi_i = int(lo), int(hi or lo)
        if not (1 <= lo_i <= hi_i <= n):
            bad.append(f"{path}:{lo}-{hi or lo} outside 1..{n}")
    assert not bad, "\n".join(bad)
