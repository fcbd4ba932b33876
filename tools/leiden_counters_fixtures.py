"""Writes tests/golden/leiden_counters/: labels, modularity and community count of K.leiden (n_iterations=-1, seed 0) on the
three 20k-vertex graphs of tests/leiden_counter_cases.py.

The committed fixtures were recorded with the library built from commit 40751a5434285e714a5e318a1e27406c95c6d502 -- the parent
of the change that bounds the workgroups per counter word in the list and totals kernels of csrc/leiden.hip -- on an MI355X:
    python tools/leiden_counters_fixtures.py [output directory]
A later build must reproduce them bit for bit (tests/test_gpu_leiden_counters.py); record them again only from a build that is
known to compute what that parent computed."""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def main():
    import torch

    import leiden_counter_cases as cases
    from scanpy_amd import _kernels as K

    out = Path(sys.argv[1]) if len(sys.argv) > 1 else cases.GOLDEN
    out.mkdir(parents=True, exist_ok=True)
    meta = {}
    for name in cases.WHOLE_RUNS:
        m = cases.whole_graph(name)
        dev = [torch.from_numpy(np.array(a, dtype=t)).cuda() for a, t in ((m.indptr, np.int64), (m.indices, np.int32), (m.data, np.float32))]
        memb, q, nc = K.leiden(*dev, m.shape[0], n_iterations=-1, seed=0)
        again, q2, nc2 = K.leiden(*dev, m.shape[0], n_iterations=-1, seed=0)
        assert torch.equal(memb, again) and q == q2 and nc == nc2, f"{name}: two runs differ"
        np.save(out / f"{name}_labels.npy", memb.cpu().numpy().astype(np.int32))
        st = K.leiden_last_stats()
        meta[name] = dict(q_hex=float(q).hex(), communities=int(nc), iterations=st["iterations"], lm_sweeps=st["lm_sweeps"])
        print(f"{name}: Q={q!r} communities={nc} {st}", flush=True)
    (out / "recorded.json").write_text(json.dumps(meta, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
