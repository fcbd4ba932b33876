"""`tl.rank_genes_groups` alone on the bench's planted matrix after normalize_total + log1p, with the 64 planted labels,
device-resident and warm; per-kernel split by device events.
    python tools/rank_genes_only.py 1000000 planted wilcoxon [--reps 3] [--tie] [--out profiles/rank_genes_1M.json]
Without a GPU it times the float64 numpy / scipy restatement (tests/rank_genes_cases.py) at 100 000 cells on the first
`--cpu-genes` genes: a CPU figure for orientation, NOT the 1M figure and not the same work."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def _event_ms(fn, reps):
    import torch

    out = None
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return out, ts


def gpu(args, x, truth):
    import pandas as pd
    import torch

    import scanpy_amd as sc
    from scanpy_amd import _kernels as K
    from scanpy_amd import _lib
    from scanpy_amd.tools import _rank_genes_groups as M

    be = M.default_backend()
    n, g = x.shape
    m = be.upload(x)
    sums = be.pp.row_sums(m)  # normalize_total (target: the median of the totals) + log1p, on the device
    be.pp.row_divide_(m, sums / np.median(sums[sums > 0]))
    be.pp.log1p_(m)
    k = int(truth.max()) + 1
    n_table = k + 1
    codes = torch.from_numpy(truth.astype(np.int32)).to(m.data.device)
    sizes = torch.from_numpy(np.bincount(truth, minlength=n_table).astype(np.int64)).to(m.data.device)
    chunk = _lib.load().scamd_rank_genes_chunk_entries(n_table)

    csc, t_transpose = _event_ms(lambda: be.transpose(m), args.reps + 1)
    col_len = np.diff(csc.t_indptr.cpu().numpy())
    _, t_stats = _event_ms(lambda: K.rank_genes_group_stats(csc.t_indptr, csc.t_indices, csc.t_data, n, g, codes, n_table), args.reps + 1)
    out = {"n": n, "g": g, "nnz": int(col_len.sum()), "structure": args.structure, "method": args.method, "groups": k,
           "chunk_entries": int(chunk), "columns_multi_chunk": int((col_len > chunk).sum()), "column_entries_max": int(col_len.max()),
           "chunks_per_column_mean": float(np.ceil(col_len / chunk).mean()), "reps": args.reps,
           "kernel_ms": {"csr_transpose": min(t_transpose[1:]), "group_stats": min(t_stats[1:])}}
    if "wilcoxon" in args.method:
        _, t_w = _event_ms(lambda: K.rank_genes_wilcoxon(csc.t_indptr, csc.t_indices, csc.t_data, n, g, codes, n_table, sizes, -1,
                                                         tie_term=args.tie), args.reps + 1)
        out["kernel_ms"]["wilcoxon" + ("_tie" if args.tie else "")] = min(t_w[1:])
    # the public call on the resident matrix: upload is replaced by a hand-over of the device copy
    ad = sc.AnnData(x)
    ad.obs["planted"] = pd.Categorical(truth.astype(str), categories=[str(i) for i in range(k)])
    be.upload = lambda _x: m
    be.nonnegative_integers = lambda _m: False
    M_default = M.default_backend
    M.default_backend = lambda: be
    try:
        walls = []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            sc.tl.rank_genes_groups(ad, "planted", method=args.method, tie_correct=args.tie)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
    finally:
        M.default_backend = M_default
    out["call_wall_ms_resident"] = {"best": min(walls[1:]), "all": walls[1:],
                                    "note": "sc.tl.rank_genes_groups with the matrix already on the device: transpose, kernels, "
                                            "read-back of the K x g tables and the host finishing (tests, correction, sort)"}
    top = ad.uns["rank_genes_groups"]["names"]["0"][:3].tolist()
    out["top_genes_of_group_0"] = top
    return out


def cpu(args):
    import bench
    import rank_genes_cases as R

    n = 100_000
    x, truth = bench.make_matrix(n, 2000, 0, args.structure)
    dense = x[:, :args.cpu_genes].toarray()
    names = list(range(int(truth.max()) + 1))
    t0 = time.perf_counter()
    R.restate(dense, truth, names[:args.cpu_groups], method=args.method, tie_correct=args.tie)
    dt = time.perf_counter() - t0
    return {"n": n, "genes_timed": args.cpu_genes, "groups_timed": args.cpu_groups, "method": args.method, "cpu_restatement_s": dt,
            "note": "float64 numpy / scipy restatement on the CPU at 100k cells, a subset of genes and groups: NOT the 1M figure, "
                    "no GPU was present"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, nargs="?", default=1_000_000)
    ap.add_argument("structure", nargs="?", default="planted")
    ap.add_argument("method", nargs="?", default="wilcoxon")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tie", action="store_true")
    ap.add_argument("--cpu-genes", type=int, default=20)
    ap.add_argument("--cpu-groups", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if torch.cuda.is_available():
        import bench

        x, truth = bench.make_matrix(args.n, 2000, 0, args.structure)
        out = gpu(args, x, truth)
    else:
        out = cpu(args)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
