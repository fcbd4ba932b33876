#!/usr/bin/env python3
"""bench.py -- cells/sec through pca + neighbors + leiden on MI355X (BASELINE.json metric).

    python bench.py --gpus 1 --steps 3 --warmup 1
    python bench.py --gpus 1 --steps 3 --warmup 1 --full
    python bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" is one full pass of the hot path (PCA 50 comps -> exact kNN k=15 -> umap connectivities ->
Leiden res 1.0) over the synthetic planted-cluster log-normal CSR (1M cells x 2k genes, ~5 % nnz: BASELINE
configs[2], the 1x MI355X roofline configuration; the 1M cells are row-sharded over the N ranks for N > 1,
i.e. strong scaling of configs[3]).  The CSR shard is resident in HBM before the timed region starts; the
timed region ends with the labels on the device.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times `--steps` steps and prints the line: `value`, `ms_per_step`, `stage_ms_per_step`,
`roofline` (from the counters of the timed steps themselves), `leiden` and `result`.  `--dump-outputs DIR` writes what
the last timed step returned as DIR/<name>.npy (`dump_outputs`).  Everything that takes runs of its own -- the side
measurements, the CPU baseline, the parity and property gates -- runs only under `--full` (rank 0 of a 1-GPU run):

Extra objects in the line:
  roofline      knn_select_reg_kernel, 3 x bf16 engine (v_mfma_f32_32x32x16_bf16 on the hi / lo split of the float32
                coordinates, result certified in float64): achieved = 3 * 2 * 64 flop per evaluated (query, candidate)
                pair -- the three split products over the 64-slot row are the arithmetic this engine's algorithm asks for
                (scamd_knn_last_select_pairs: the pairs of the swept cells, WITHOUT the threshold pre-pass that re-scores
                every block's own cell; the exact cell-pruned search skips provably empty cells) / its HIP-event
                duration (scamd_knn_last_select_ms), peak = 2500 TFLOP/s dense bf16 (MI355X_MICROARCH.md).  Beside it
                `f32_equivalent_tflops` = 2 * 50 flop per pair (what the float32 engine of rounds 1-2 was priced on;
                its peak was the 157.3 TFLOP/s of the f32-input MFMA).  SCAMD_KNN_B3=0 runs the float32 engine.
  value_h2h (= value_host_to_host; also config.value_h2h_cells_per_s / config.h2h_ms_per_pass, which the driver's record keeps)
                the BASELINE metric at the drop-in boundary: AnnData with a host CSR in -> sc.pp.pca /
                sc.pp.neighbors / sc.tl.leiden -> slots written on the host (H2D, kernels, D2H, scipy / pandas slot
                construction), warm process, best of `--h2h-reps`; `value` is the device-resident figure.
  structure_none       the same path on the pure-noise variant of the matrix: nothing can be pruned, the
                kNN sweep evaluates every pair -- the regime the roofline of the brute-force sweep is quoted on.
  structure_weak       ... and on the overlapping-programme variant (what real scRNA data looks like: the exact cell bound
                prunes nothing either, and the communities are ambiguous).  Both variants carry the Leiden guarantees of
                their result (node optimality, separation, connectivity: gated) and the recall / time of the approximate
                IVF search (`knn_approx`).  `--structure none|weak|planted` makes any of the three the timed workload.
  leiden        the Leiden stage of the timed steps: iterations, launches, blocking host round trips, local-moving
                sweeps and SURVEY 8(d)'s figure for them -- bytes of the rows the sweeps visit / stage time vs 8 TB/s --
                and what the final polish did.
  knn_approx    `scamd_knn_l2_ivf_f32` (pp.neighbors(transformer='ivf')) on the same embedding: recall@k against the exact
                lists of the timed step, stage and select-kernel time, fraction of the pairs evaluated, per nprobe.
  cpu_baseline  the reference's CPU call chain (sklearn PCA arpack + sklearn brute kNN = reference calls; oracle
                fuzzy set + oracle Leiden) on the first n cells of the same matrix for n in `--cpu-sizes`, on this box's
                host cores.  The default sizes END WITH THE FULL 1M CELLS (round 6): `value` is then the measured run
                (`measured_at_full_size`, ~170 s on the GPU box's 256 cores), `extrapolated_seconds_at_full_size` what
                the two small samples predicted (kNN fitted with the n^2 law, the other stages linearly; BASELINE.md
                section 3); a box on which the full size does not fit `--cpu-budget-s` reports the fit and says so.
  parity        (`--verify`, default at N=1 under `--full`) the GPU path against that CPU chain on the largest CPU sample, stage by
                stage (every stage fed the CPU chain's previous output, so a gate isolates one stage) and end to end;
                the process exits non-zero when a north_star gate breaks.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--full", action="store_true",
                    help="also run what takes runs of its own (N=1): side measurements, structure variants, host-to-host, "
                         "full-size properties, CPU baseline and parity; a plain run measures the timed steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float32 / float64; a fixed row sample "
                         "of the per-cell arrays)")
    ap.add_argument("--n-obs", type=int, default=1_000_000)
    ap.add_argument("--n-vars", type=int, default=2000)
    ap.add_argument("--n-comps", type=int, default=50)
    ap.add_argument("--n-neighbors", type=int, default=15)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--scaling", choices=("strong", "weak"), default="strong",
                    help="N > 1: strong = --n-obs cells split over the ranks (BASELINE configs[3]); weak = --n-obs cells PER "
                         "rank (e.g. --n-obs 1250000 --n-vars 4000 --gpus 8 is the configs[4] shape, 10M x 4k)")
    ap.add_argument("--cpu-sizes", type=str, default="100000,250000,1000000",
                    help="cell counts of the CPU-baseline samples (n^2 fit of the brute kNN); '' or 0 = skip")
    ap.add_argument("--cpu-sample", type=int, default=None, help="(old flag) one CPU-baseline sample size; 0 = skip")
    ap.add_argument("--cpu-budget-s", type=float, default=270.0,
                    help="stop adding CPU samples once the next one is predicted to exceed this many seconds in total")
    ap.add_argument("--structure", choices=("planted", "weak", "none"), default="planted",
                    help="planted: 64 separated cell types (BASELINE.md section 3); weak: overlapping types; "
                         "none: pure noise (throughput / roofline only, loadings and labels are ill-conditioned)")
    ap.add_argument("--verify", dest="verify", action="store_true", default=None,
                    help="compare the GPU path with the CPU chain on the largest CPU sample (default at N=1)")
    ap.add_argument("--no-verify", dest="verify", action="store_false")
    ap.add_argument("--h2h-reps", type=int, default=3, help="repetitions of the host-to-host drop-in measurement (0 = skip)")
    ap.add_argument("--no-noise-variant", action="store_true", help="skip the `structure_none` / `structure_weak` side measurements")
    ap.add_argument("--no-side", action="store_true", help="skip upstream_chain / umap_layout side measurements")
    ap.add_argument("--no-properties", action="store_true", help="skip `full_size_properties` (CPU checks of the last timed result)")
    ap.add_argument("--knn-nprobe", type=int, default=0,
                    help="> 0: the timed path uses the APPROXIMATE IVF search (pp.neighbors(transformer='ivf'), BASELINE configs[4]) "
                         "probing this many cells; the line then reports the sampled recall instead of gating exactness, and the "
                         "CPU-chain parity (an exact chain) is skipped")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if a.cpu_sample is not None:
        a.cpu_sizes = str(a.cpu_sample)
    a.cpu_sizes = [int(v) for v in a.cpu_sizes.split(",") if v.strip() and int(v) > 0]
    return a


# p_programme of `synthetic_planted`: the probability that a cell expresses its type's gene in a stratum
STRUCTURE = {"planted": 0.7, "weak": 0.12, "none": 0.0}


def make_matrix(n, g, seed, structure, row_range=None):
    from scanpy_amd.datasets import synthetic_planted

    return synthetic_planted(n, g, seed=seed, p_programme=STRUCTURE[structure], row_range=row_range)


def cpu_chain(x, n_comps: int, k: int) -> dict:
    """The reference's CPU call chain on one matrix: stage seconds + every stage's output (kept for `parity`)."""
    import numpy as np

    from oracle import connectivities as oc
    from oracle import knn as oknn
    from oracle import leiden as ol
    from oracle import pca as opca

    n = x.shape[0]
    t0 = time.perf_counter()
    ref = opca.pca_reference(x, n_comps)
    t1 = time.perf_counter()
    x_pca = np.ascontiguousarray(ref["X_pca"], dtype=np.float32)
    idx, dist, _ = oknn.knn_sklearn(x_pca, k, n_jobs=-1)
    t2 = time.perf_counter()
    conn, _, _ = oc.fuzzy_simplicial_set(idx, dist, n, k)
    t3 = time.perf_counter()
    labels, q = ol.leiden(conn, resolution=1.0, n_iterations=-1, seed=0)
    t4 = time.perf_counter()
    return {"n": n, "seconds": {"pca": t1 - t0, "knn": t2 - t1, "connectivities": t3 - t2, "leiden": t4 - t3},
            "components": ref["components"], "x_pca": x_pca, "idx": idx, "dist": dist, "conn": conn, "labels": labels,
            "modularity": q}


def cpu_baseline(x_full, truth, sizes, n_full: int, n_comps: int, k: int, budget_s: float):
    """Reference CPU chain on the first n cells of the same synthetic matrix for each n in `sizes` (rank 0, N=1 only).
    -> (the `cpu_baseline` object, the chain outputs of the largest sample that ran)."""
    import numpy as np

    from oracle import leiden as ol

    ol.build()
    runs, last, spent = [], None, 0.0
    for n_s in sorted(min(v, x_full.shape[0]) for v in sizes):
        if runs:  # predicted cost of this sample from the previous one: kNN ~ n^2, the rest ~ n
            p = runs[-1]
            r = n_s / p["n"]
            pred = p["knn"] * r * r + (p["pca"] + p["connectivities"] + p["leiden"]) * r
            if spent + pred > budget_s:
                break
        c = cpu_chain(x_full[:n_s], n_comps, k)
        sec = c["seconds"]
        runs.append({"n": n_s, **sec, "total": sum(sec.values())})
        spent += runs[-1]["total"]
        last = c
    # fits through the origin over the samples BELOW the full size: kNN = a n^2 (least squares), every other stage = b n
    big = runs[-1]
    full = big if big["n"] == n_full else None  # the whole workload was RUN (round 6: the default sizes end with it)
    fit_runs = [r for r in runs if r["n"] < n_full] or runs
    ns = np.array([r["n"] for r in fit_runs], dtype=np.float64)
    a_knn = float((np.array([r["knn"] for r in fit_runs]) * ns ** 2).sum() / (ns ** 4).sum())
    lin = {st: float((np.array([r[st] for r in fit_runs]) * ns).sum() / (ns ** 2).sum()) for st in ("pca", "connectivities", "leiden")}
    est = {"knn": a_knn * n_full ** 2, **{st: b * n_full for st, b in lin.items()}}
    est_total = sum(est.values())
    obj = {
        "value": n_full / (full["total"] if full else est_total),
        "unit": "cells/s",
        "cores": os.cpu_count(),
        "kind": "port",
        "measured_at_full_size": full is not None,
        "sample": (f"first n cells x {x_full.shape[1]} genes of the same synthetic CSR for n in {[r['n'] for r in runs]}: "
                   "sklearn PCA(arpack) + sklearn brute kNN(n_jobs=-1) (the reference's own calls) + oracle "
                   "fuzzy_simplicial_set + oracle Leiden (igraph / umap-learn absent); "
                   + (f"`value` = {n_full} cells / the seconds MEASURED on all {n_full} cells (the last entry of `measured`); "
                      "`extrapolated_seconds_at_full_size` = what the smaller samples predicted for it "
                      if full else
                      f"`value` = the full {n_full} cells / the seconds EXTRAPOLATED from these samples (the full size did not fit "
                      "`--cpu-budget-s` on this box) ")
                   + "(fit: brute kNN = a*n^2 least squares, the other stages linear in n; BASELINE.md section 3)"),
        "measured": runs,
        "extrapolated_seconds_at_full_size": {**est, "total": est_total, "fitted_on": [r["n"] for r in fit_runs]},
        "largest_sample_cells_per_s": big["n"] / big["total"],
        "seconds": spent,
    }
    if full:
        obj["measured_seconds_at_full_size"] = {k_: full[k_] for k_ in ("pca", "knn", "connectivities", "leiden", "total")}
        obj["fit_over_measured"] = est_total / full["total"]
    return obj, last


def parity_block(x_full, truth, chain: dict, n_comps: int, k: int) -> dict:
    """GPU path vs the CPU chain on the chain's sample (the first chain['n'] cells), through the drop-in calls.
    Stage-wise: each GPU stage is fed the CPU chain's output of the previous stage, so each gate isolates one stage;
    end to end: all three stages on the GPU from the matrix."""
    import numpy as np

    import scanpy_amd as sc
    from oracle import compare as cmp
    from oracle import leiden as ol

    n_s = chain["n"]
    x = x_full[:n_s]
    out = {"sample_cells": n_s, "gates": dict(cmp.GATES)}
    # end to end on the GPU
    a = sc.AnnData(x)
    sc.pp.pca(a, n_comps=n_comps)
    sc.pp.neighbors(a, n_neighbors=k)
    sc.tl.leiden(a, flavor="igraph", n_iterations=-1)
    gpu_labels = a.obs["leiden"].cat.codes.to_numpy()
    out["pca_loading_err"] = cmp.pca_loading_err(a.varm["PCs"].T, chain["components"])
    out["leiden_ari_vs_cpu_chain"] = cmp.ari(gpu_labels, chain["labels"])
    out["n_clusters"] = {"gpu": int(gpu_labels.max()) + 1, "cpu_chain": int(chain["labels"].max()) + 1}
    out["modularity"] = {"gpu": float(a.uns["leiden"]["modularity"]), "cpu_chain": chain["modularity"]}
    if truth is not None:
        out["ari_vs_truth"] = {"gpu": cmp.ari(gpu_labels, truth[:n_s]), "cpu_chain": cmp.ari(chain["labels"], truth[:n_s])}
    e2e = a.obsp["distances"]
    got = np.sort(e2e.indices.reshape(n_s, k - 1), axis=1)
    out["knn_rows_equal_end_to_end"] = float((got == np.sort(chain["idx"][:, 1:], axis=1)).all(axis=1).mean())
    # stage-wise: neighbors on the CPU chain's embedding
    b = sc.AnnData(x)
    b.obsm["X_pca"] = chain["x_pca"]
    sc.pp.neighbors(b, n_neighbors=k, use_rep="X_pca")
    d = b.obsp["distances"]
    gi = np.hstack([np.arange(n_s, dtype=np.int64)[:, None], d.indices.reshape(n_s, k - 1)])
    gd = np.hstack([np.zeros((n_s, 1)), d.data.reshape(n_s, k - 1)])
    bad, differ = cmp.knn_rows_differing_beyond_ties(gi, gd, chain["idx"], chain["dist"])
    out["knn_rows_differing_beyond_ties"] = bad
    out["knn_rows_differing_at_ties"] = differ - bad
    out["knn_max_rel_distance_err"] = float(np.max(np.abs(np.sort(gd, axis=1) - np.sort(chain["dist"], axis=1))
                                                   / np.maximum(np.sort(chain["dist"], axis=1), 1e-30)))
    # (the GPU search returns the float64 distance rounded once to float32, sklearn's differ from that in the last bit;
    # umap's bisection stops when |sum - log2 k| < 1e-5, so a one-ulp input change moves a few sigmas by ~1e-5:
    # informational, the reference's own bar for recomputed distances is rtol 1e-5, tests/test_neighbors.py:275-296)
    cerr_g, same_g = cmp.conn_max_abs(b.obsp["connectivities"], chain["conn"])
    out["conn_max_abs_from_gpu_distances"] = cerr_g
    # end to end (connectivities from the GPU's own distances against the CPU chain's): sklearn computes the distances
    # of float32 points with a float32 GEMM (relative error ~1e-7, `knn_max_rel_distance_err`), the GPU search returns the
    # exact float64 distance rounded once -- so ~90 % of the rows hold at least one distance that differs in its last
    # float32 bit (`conn_e2e_rows_distance_ulp_fraction`, informational), and umap's bisection, which stops at
    # |sum - log2 k| < 1e-5, turns such an input change into a change of ~1e-5 of the row's weights.  Gates: (a) every
    # entry whose two end points have float32 neighbour lists bit-identical to the CPU chain's meets the reference's own
    # bar for connectivities recomputed from GIVEN distances, rtol 1e-5 (tests/test_neighbors.py:275-296); (b) all entries:
    # identical sparsity pattern and |difference| <= 1e-4 = ten bisection tolerances (measured 1.4e-5 .. 2.5e-5).
    og, oc_ = np.argsort(gi, axis=1), np.argsort(chain["idx"], axis=1)
    gi_s, ci_s = np.take_along_axis(gi, og, 1), np.take_along_axis(chain["idx"], oc_, 1)
    gd_s = np.take_along_axis(gd, og, 1).astype(np.float32)
    cd_s = np.take_along_axis(chain["dist"], oc_, 1).astype(np.float32)
    row_ok = (gi_s == ci_s).all(axis=1) & (gd_s == cd_s).all(axis=1)
    out["conn_e2e_rows_distance_ulp_fraction"] = float(1.0 - row_ok.mean())
    out["conn_e2e_max_rel"], out["conn_e2e_entries_compared"] = cmp.conn_max_rel(b.obsp["connectivities"], chain["conn"], row_ok)
    # stage-wise: the fuzzy set from the CPU chain's OWN distances (`pp.neighbors(distances=...)`)
    from oracle import knn as oknn

    f = sc.AnnData(x[:, :1])
    sc.pp.neighbors(f, n_neighbors=k, distances=oknn.sparse_from_indices_distances(chain["idx"], chain["dist"], keep_self=False))
    cerr, same = cmp.conn_max_abs(f.obsp["connectivities"], chain["conn"])
    out["conn_max_abs"] = cerr
    out["conn_max_rel"], _ = cmp.conn_max_rel(f.obsp["connectivities"], chain["conn"])
    out["conn_same_pattern"] = bool(same and same_g)
    # stage-wise: Leiden on the CPU chain's graph; the oracle's own seed-to-seed agreement is the noise floor
    c = sc.AnnData(x[:, :1])
    sc.tl.leiden(c, adjacency=chain["conn"], flavor="igraph", n_iterations=-1)
    out["leiden_ari_stagewise"] = cmp.ari(c.obs["leiden"].cat.codes.to_numpy(), chain["labels"])
    out["leiden_modularity_stagewise"] = {"gpu": float(c.uns["leiden"]["modularity"]), "cpu_chain": chain["modularity"]}
    other, q_other = ol.leiden(chain["conn"], resolution=1.0, n_iterations=-1, seed=1)
    out["cpu_chain_seed0_vs_seed1_ari"] = cmp.ari(other, chain["labels"])
    fails = []
    if out["pca_loading_err"] > cmp.GATES["pca_loading_err"]:
        fails.append("pca_loading_err")
    if out["knn_rows_differing_beyond_ties"] > 0:
        fails.append("knn_rows_differing_beyond_ties")
    if out["conn_max_abs"] > cmp.GATES["conn_max_abs"] or not same:
        fails.append("conn_max_abs")
    if out["conn_max_rel"] > cmp.GATES["conn_max_rel"]:
        fails.append("conn_max_rel")
    if out["conn_e2e_max_rel"] > cmp.GATES["conn_e2e_max_rel"] or not same_g:
        fails.append("conn_e2e_max_rel")
    if out["conn_max_abs_from_gpu_distances"] > cmp.GATES["conn_max_abs_from_gpu_distances"]:
        fails.append("conn_max_abs_from_gpu_distances")
    out["relaxed_gates"] = {
        "conn_max_abs_from_gpu_distances": "end to end the bar is 1e-4 absolute (ten times the tolerance at which umap's bisection "
        "stops), not the 1e-5 of the stage-wise gates: the CPU chain's distances carry the float32 rounding of sklearn's GEMM, "
        "the GPU's do not; entries whose inputs are bit-identical are gated at the reference's rtol 1e-5 (conn_e2e_max_rel), "
        "the stage-wise comparison from the CPU chain's own distances at 1e-5 absolute AND rtol 1e-5"}
    floor = min(cmp.GATES["leiden_ari_vs_cpu_chain"], out["cpu_chain_seed0_vs_seed1_ari"])
    if min(out["leiden_ari_vs_cpu_chain"], out["leiden_ari_stagewise"]) < floor:
        fails.append("leiden_ari_vs_cpu_chain")
    out["leiden_ari_bar"] = floor
    out["failed_gates"] = fails
    return out


def parity_weak(args, n_s: int = 100_000, n_seeds: int = 5) -> dict:
    """`parity.weak`: Leiden where the answer is NOT unambiguous -- a `weak` sample (overlapping gene programmes, the
    CPU oracle's own seeds agree only partly).  On the CPU chain's graph the oracle's seeds 0 .. n_seeds-1 and the GPU's
    seeds 0 .. n_seeds-1 are two samples of partitions; reported for BOTH: modularity, ARI against the planted truth,
    pairwise ARI.  Gates (reference bar: cross-implementation agreement,
    tests/test_clustering.py:130-163): GPU modularity not below the oracle's worst seed; median GPU ARI-vs-truth >= the
    oracle's median - 0.05; median GPU-vs-oracle ARI (all seed pairs) >= the oracle's median PAIRWISE ARI - 0.02."""
    import itertools

    import numpy as np

    import scanpy_amd as sc
    from oracle import compare as cmp
    from oracle import leiden as ol

    x, truth = make_matrix(n_s, args.n_vars, args.seed, "weak")
    chain = cpu_chain(x, args.n_comps, args.n_neighbors)
    seeds = [(chain["labels"], chain["modularity"])] + [ol.leiden(chain["conn"], resolution=1.0, n_iterations=-1, seed=s)
                                                        for s in range(1, n_seeds)]
    q_or = np.array([q for _, q in seeds])
    o_pair = [cmp.ari(a[0], b[0]) for a, b in itertools.combinations(seeds, 2)]
    o_truth = [cmp.ari(m, truth) for m, _ in seeds]
    gpu = []
    for s_ in range(n_seeds):
        c = sc.AnnData(x[:, :1])
        sc.tl.leiden(c, adjacency=chain["conn"], flavor="igraph", n_iterations=-1, random_state=s_)
        gpu.append((c.obs["leiden"].cat.codes.to_numpy(), float(c.uns["leiden"]["modularity"])))
    q_gpu = np.array([q for _, q in gpu])
    g_truth = [cmp.ari(m, truth) for m, _ in gpu]
    g_cross = [cmp.ari(m, o[0]) for m, _ in gpu for o in seeds]
    g_pair = [cmp.ari(a[0], b[0]) for a, b in itertools.combinations(gpu, 2)]
    a = sc.AnnData(x)
    sc.pp.pca(a, n_comps=args.n_comps)
    sc.pp.neighbors(a, n_neighbors=args.n_neighbors)
    sc.tl.leiden(a, flavor="igraph", n_iterations=-1)
    e_lab = a.obs["leiden"].cat.codes.to_numpy()
    out = {"sample_cells": n_s, "structure": "weak", "seeds": n_seeds,
           "modularity": {"oracle": [float(v) for v in q_or], "gpu": [float(v) for v in q_gpu]},
           "oracle_modularity_range": [float(q_or.min()), float(q_or.max())], "gpu_modularity_same_graph": float(q_gpu[0]),
           "ari_vs_truth": {"oracle": [float(v) for v in o_truth], "gpu": [float(v) for v in g_truth],
                            "oracle_median": float(np.median(o_truth)), "gpu_median": float(np.median(g_truth))},
           "pairwise_ari": {"oracle_median": float(np.median(o_pair)), "oracle_min": float(min(o_pair)),
                            "gpu_vs_oracle_median": float(np.median(g_cross)), "gpu_vs_oracle_min": float(min(g_cross)),
                            "gpu_median": float(np.median(g_pair))},
           "gpu_vs_oracle_seed0_ari": cmp.ari(gpu[0][0], seeds[0][0]),
           "gpu_end_to_end_vs_oracle_seed0_ari": cmp.ari(e_lab, seeds[0][0]),
           "gpu_end_to_end_ari_vs_truth": cmp.ari(e_lab, truth),
           "n_clusters": {"gpu": [int(m.max()) + 1 for m, _ in gpu], "oracle": [int(m.max()) + 1 for m, _ in seeds]},
           "gates": {"modularity": "every gpu seed >= oracle minimum - 1e-4",
                     "ari_vs_truth": "gpu median >= oracle median - 0.05",
                     "ari_vs_oracle": "median over all (gpu seed, oracle seed) pairs >= oracle median pairwise ARI - 0.02"}}
    fails = []
    if q_gpu.min() < q_or.min() - 1e-4:
        fails.append("weak_modularity_below_oracle_range")
    if np.median(g_truth) < np.median(o_truth) - 0.05:
        fails.append("weak_ari_vs_truth_below_oracle_median")
    if np.median(g_cross) < np.median(o_pair) - 0.02:
        fails.append("weak_ari_vs_oracle_below_oracle_pairwise_median")
    out["failed_gates"] = fails
    return out


PROPERTY_GATES = {"knn_rows_differing_beyond_ties": 0, "knn_max_rel_distance_err": 1e-6, "conn_asymmetry": 0.0,
                  "conn_sample_max_abs": 1e-5, "modularity_abs_err": 1e-7, "disconnected_communities": 0,
                  "pca_orthonormality_err": 1e-5, "pca_scores_sample_rel_err": 1e-4,
                  # the Leiden paper's guarantees for a stable partition (oracle/leiden_guarantees.py): no merge of two
                  # communities improves the quality, no single vertex move does -- both exact (round 5: the optimiser ends
                  # an n_iterations = -1 run with a monotone polish; round 4 left 9 / 186 of 300k vertices improvable on the
                  # weak / structure-less graphs and this gate allowed 2e-3 of them)
                  "leiden_mergeable_pairs": 0, "leiden_improving_moves": 0}


def full_size_properties(res, x_host, n: int, k: int, *, n_sample: int = 512, seed: int = 123, approximate: bool = False) -> dict:
    """Properties of ONE result of the timed path that can be checked at ANY size, the bench's full size included (the
    CPU chain of `parity_block` stops at 500k cells and is out of reach at 10M x 4k): kNN rows of a row sample against a
    float64 brute force over ALL cells of the same embedding; structure of every kNN row; exact symmetry, range and row
    order of the connectivities, a row sample of them against the oracle's fuzzy set (which needs the sigma / rho of the
    sampled rows' neighbours only); the reported modularity recomputed from the graph and the labels; every community
    connected, no two communities mergeable with a gain, no vertex movable with a gain (the guarantees of Traag et al.
    2019 for a stable partition: oracle/leiden_guarantees.py); loadings orthonormal and a row sample of the
    scores recomputed in float64 from the host matrix.  CPU work on rank 0 of a 1-GPU run, after the timed region;
    `res` = PathResult (device tensors) or anything with the same fields on the host (tests/test_bench_properties_cpu.py)."""
    import numpy as np
    from scipy import sparse
    from scipy.sparse.csgraph import connected_components

    from oracle import compare as cmp
    from oracle import connectivities as oconn
    from oracle import knn as oknn
    from oracle import leiden as ol
    from oracle import leiden_guarantees as lg

    def host(t):
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    t_start = time.perf_counter()
    out = {"gates": dict(PROPERTY_GATES), "n_obs": n}
    fails = []
    rng = np.random.default_rng(seed)
    rows = np.sort(rng.choice(n, size=min(n_sample, n), replace=False))
    emb = host(res.x_pca)
    idx = host(res.knn_indices).astype(np.int64)
    dist = host(res.knn_distances).astype(np.float64)

    # ---- kNN: every row's structure, a sample's content
    ar = np.arange(n, dtype=np.int64)
    srt = np.sort(idx, axis=1)
    knn = {
        "self_first_rows": float((idx[:, 0] == ar).mean()),
        "rows_sorted_by_distance": bool((np.diff(dist, axis=1) >= 0).all()),
        "indices_in_range": bool(idx.min() >= 0 and idx.max() < n),
        "rows_with_duplicates": int(((np.diff(srt, axis=1) == 0).any(axis=1)).sum()),
    }
    ei, ed = oknn.knn_exact_f64_sample(emb, rows, k)
    bad, differ = cmp.knn_rows_differing_beyond_ties(idx[rows], dist[rows], ei, ed)
    knn["sample_rows"] = int(rows.size)
    if approximate:  # (--knn-nprobe: the lists are exact among the probed rows only; what is reported is the recall)
        knn["approximate"] = True
        knn["sample_recall"] = float(np.mean([np.isin(idx[r, 1:], e[1:]).mean() for r, e in zip(rows, ei)]))
        bad = 0
    knn["rows_differing_beyond_ties"] = int(bad)
    knn["rows_differing_at_ties"] = int(differ - bad)
    # (the reported distance of every reported pair, recomputed: `knn_rows_differing_beyond_ties` takes a row's own
    # distances at their word when it decides what is a tie)
    pair = np.sqrt(((emb[rows].astype(np.float64)[:, None, :] - emb[idx[rows]].astype(np.float64)) ** 2).sum(-1))
    knn["max_rel_distance_err"] = float(max(0.0 if approximate else np.max(np.abs(dist[rows] - ed) / np.maximum(ed, 1e-30)),
                                            np.max(np.abs(dist[rows] - pair) / np.maximum(pair, 1e-30))))
    out["knn"] = knn
    if bad > PROPERTY_GATES["knn_rows_differing_beyond_ties"] or knn["rows_with_duplicates"] or not (
            knn["rows_sorted_by_distance"] and knn["indices_in_range"]):
        fails.append("knn_rows_differing_beyond_ties")
    if knn["max_rel_distance_err"] > PROPERTY_GATES["knn_max_rel_distance_err"]:
        fails.append("knn_max_rel_distance_err")

    # ---- connectivities: whole-matrix structure, a row sample against the oracle
    indptr, cols, vals = host(res.conn_indptr).astype(np.int64), host(res.conn_indices), host(res.conn_data)
    conn = sparse.csr_matrix((vals, cols, indptr), shape=(n, n))
    cs = {"nnz": int(conn.nnz)}
    asym = abs(conn - conn.T)
    cs["asymmetry_max_abs"] = float(asym.max()) if asym.nnz else 0.0
    lens = np.diff(indptr)
    inner = np.ones(conn.nnz, dtype=bool)
    inner[indptr[:-1][lens > 0]] = False  # first entry of each row: no predecessor in its row
    cs["rows_ascending_unique"] = bool((np.diff(cols.astype(np.int64), prepend=-1)[inner] > 0).all())
    cs["values_in_0_1"] = bool(vals.min() > 0.0 and vals.max() <= 1.0) if conn.nnz else True
    cs["diagonal_entries"] = int((cols == np.repeat(ar, lens)).sum())
    d32 = dist.astype(np.float32)
    sub = rows[: max(1, rows.size // 2)]
    want = [sub, idx[sub].ravel(), cols[np.concatenate([np.arange(indptr[i], indptr[i + 1]) for i in sub])].astype(np.int64)]
    need = np.unique(np.concatenate(want))
    need = need[need >= 0]
    loc = -np.ones(n, dtype=np.int64)
    loc[need] = np.arange(need.size)
    sig, rho = oconn.smooth_knn_dist_vec(d32[need], float(k), mean_all=float(d32.mean(dtype=np.float64)))
    # (compute_membership_strengths recognises the self entry by `index == row number` and the rows here are a subset:
    # the self entries are renamed to the local row number, every other id to a negative number that is neither -1 nor a row)
    idx_need = idx[need]
    renamed = np.where(idx_need == need[:, None], np.arange(need.size)[:, None], -2 - idx_need)
    r_, _, v_ = oconn.compute_membership_strengths(renamed, d32[need], sig, rho)
    w_need = sparse.csr_matrix((v_, (r_, idx_need.ravel())), shape=(need.size, n))
    worst, missing, checked = 0.0, 0, 0
    for i in sub:
        cc = cols[indptr[i]:indptr[i + 1]].astype(np.int64)
        w_ic = np.asarray(w_need[loc[i], cc].todense()).ravel().astype(np.float32)
        w_ci = np.asarray(w_need[loc[cc], i].todense()).ravel().astype(np.float32)
        expect = (w_ic + w_ci).astype(np.float32) - (w_ic * w_ci).astype(np.float32)
        worst = max(worst, float(np.abs(expect.astype(np.float64) - vals[indptr[i]:indptr[i + 1]]).max(initial=0.0)))
        own = w_need[loc[i]].tocoo()
        missing += int(np.setdiff1d(own.col[own.data > 0], cc).size)
        checked += cc.size
    cs["sample_rows"] = int(sub.size)
    cs["sample_entries"] = int(checked)
    cs["sample_max_abs"] = worst
    cs["sample_missing_entries"] = missing
    out["connectivities"] = cs
    if cs["asymmetry_max_abs"] > PROPERTY_GATES["conn_asymmetry"] or not (cs["rows_ascending_unique"] and cs["values_in_0_1"]) \
            or cs["diagonal_entries"]:
        fails.append("conn_asymmetry")
    if worst > PROPERTY_GATES["conn_sample_max_abs"] or missing:
        fails.append("conn_sample_max_abs")

    # ---- Leiden: modularity of the labels on the graph, recomputed; every community connected
    labels = host(res.labels).astype(np.int64)
    q_cpu = ol.modularity(conn, labels.astype(np.int32))
    same = labels[np.repeat(ar, lens)] == labels[cols]
    intra = sparse.csr_matrix((np.ones(int(same.sum()), dtype=np.int8), (np.repeat(ar, lens)[same], cols[same])), shape=(n, n))
    n_comp, _ = connected_components(intra, directed=False)
    n_lab = int(np.unique(labels).size)
    ld = {"modularity_reported": float(res.modularity), "modularity_recomputed": float(q_cpu),
          "modularity_abs_err": abs(float(res.modularity) - float(q_cpu)), "n_communities": n_lab,
          "labels_contiguous": bool(labels.min() == 0 and labels.max() + 1 == n_lab == int(res.n_communities)),
          "disconnected_communities": int(n_comp - n_lab)}
    im, mp = lg.improving_moves(conn, labels), lg.mergeable_pairs(conn, labels)
    ld.update({"improving_moves": im["count"], "improving_moves_fraction": im["fraction"], "improving_move_max_gain": im["max_gain"],
               "mergeable_pairs": mp["count"], "merge_max_gain": mp["max_gain"]})
    out["leiden"] = ld
    if ld["modularity_abs_err"] > PROPERTY_GATES["modularity_abs_err"] or not ld["labels_contiguous"]:
        fails.append("modularity_abs_err")
    if ld["disconnected_communities"] != PROPERTY_GATES["disconnected_communities"]:
        fails.append("disconnected_communities")
    if ld["mergeable_pairs"] > PROPERTY_GATES["leiden_mergeable_pairs"]:
        fails.append("leiden_mergeable_pairs")
    if ld["improving_moves"] > PROPERTY_GATES["leiden_improving_moves"]:
        fails.append("leiden_improving_moves")

    # ---- PCA: orthonormal loadings, sampled scores from the host matrix in float64
    comp = np.asarray(res.components, dtype=np.float64)
    var = np.asarray(res.variance, dtype=np.float64)
    pc = {"orthonormality_err": float(np.abs(comp @ comp.T - np.eye(comp.shape[0])).max()),
          "variance_descending_positive": bool((np.diff(var) <= 0).all() and var[-1] > 0)}
    if x_host is not None:
        g = x_host.shape[1]
        mean = np.bincount(x_host.indices, weights=x_host.data.astype(np.float64), minlength=g) / n
        xs = np.asarray(x_host[rows].todense(), dtype=np.float64) - mean
        sc_ref = xs @ comp.T
        pc["scores_sample_rel_err"] = float(np.abs(sc_ref - emb[rows]).max() / np.abs(sc_ref).max())
        # (sign: the scores and the loadings of one result share it)
        if pc["scores_sample_rel_err"] > PROPERTY_GATES["pca_scores_sample_rel_err"]:
            fails.append("pca_scores_sample_rel_err")
    out["pca"] = pc
    if pc["orthonormality_err"] > PROPERTY_GATES["pca_orthonormality_err"] or not pc["variance_descending_positive"]:
        fails.append("pca_orthonormality_err")
    out["failed_gates"] = fails
    out["seconds"] = time.perf_counter() - t_start
    return out


def host_to_host(x, n_comps: int, k: int, reps: int) -> dict:
    """The BASELINE metric at the drop-in boundary (SURVEY 8(d) bullet 1): a host AnnData in, the slots on the host
    out, through sc.pp.pca / sc.pp.neighbors / sc.tl.leiden."""
    import scanpy_amd as sc

    best, runs = None, []
    for _ in range(reps):
        a = sc.AnnData(x)
        t0 = time.perf_counter()
        sc.pp.pca(a, n_comps=n_comps)
        t1 = time.perf_counter()
        sc.pp.neighbors(a, n_neighbors=k)
        t2 = time.perf_counter()
        sc.tl.leiden(a, flavor="igraph", n_iterations=-1)
        t3 = time.perf_counter()
        r = {"pca_ms": (t1 - t0) * 1e3, "neighbors_ms": (t2 - t1) * 1e3, "leiden_ms": (t3 - t2) * 1e3, "total_ms": (t3 - t0) * 1e3}
        runs.append(r)
        if best is None or r["total_ms"] < best["total_ms"]:
            best = r
    return {"value": x.shape[0] / (best["total_ms"] * 1e-3), "unit": "cells/s", "best": best, "first": runs[0], "reps": reps,
            "n_clusters": int(a.obs["leiden"].nunique()),
            "note": "host AnnData (CSR f32) in -> obsm/varm/uns/obsp/obs slots on the host out; includes H2D of X, D2H of "
                    "the results and the scipy / pandas slot construction; warm process"}


def _sha(t) -> str:
    """sha1 (first 16 hex digits) of a device tensor's bytes: lets two runs / boxes be compared bit for bit"""
    import hashlib

    return hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def leiden_block(stats: dict, leiden_ms: float) -> dict:
    """The Leiden stage in SURVEY 8(d)'s currency: local-moving sweeps x bytes of the rows they visit / stage time."""
    gb = stats.get("lm_sweep_algorithmic_MB", 0) / 1e3
    gbps = gb / (leiden_ms * 1e-3) if leiden_ms and leiden_ms > 0 else None
    return {"ms": leiden_ms, "bound": "hbm (gather latency)", "lm_sweeps": stats.get("lm_sweeps"), "lm_sweep_algorithmic_GB": gb,
            "achieved_GBps": gbps, "peak_GBps": 8000.0, "frac": gbps / 8000.0 if gbps else None,
            "note": "bytes = active rows x (12 B per entry + 16 B per vertex) summed over the local-moving sweeps of the levels "
                    "that run as separate kernels; the stage time also holds refinement, aggregation, the one-workgroup small "
                    "levels and the polish",
            **{k: stats.get(k) for k in ("iterations", "launches", "host_round_trips", "levels_first_iteration", "polish_full_sweeps",
                                         "polish_rounds", "polish_moves", "polish_skipped_proven")}}


def leiden_guarantees(res, n: int) -> dict:
    """connected / g-separated / node-optimal (oracle/leiden_guarantees.py) of a result's labels on its own graph"""
    import numpy as np
    from scipy import sparse
    from scipy.sparse.csgraph import connected_components

    from oracle import leiden_guarantees as lg

    ip, ix, w = (t.detach().cpu().numpy() for t in (res.conn_indptr, res.conn_indices, res.conn_data))
    conn = sparse.csr_matrix((w, ix, ip), shape=(n, n))
    lab = res.labels.detach().cpu().numpy()
    im, mp = lg.improving_moves(conn, lab), lg.mergeable_pairs(conn, lab)
    same = lab[np.repeat(np.arange(n), np.diff(ip))] == lab[ix]
    inner = sparse.csr_matrix((same.astype(np.int8), ix.copy(), ip.copy()), shape=(n, n))
    inner.eliminate_zeros()
    n_comp, _ = connected_components(inner, directed=False)
    out = {"improving_moves": im["count"], "improving_move_max_gain": im["max_gain"], "mergeable_pairs": mp["count"],
           "merge_max_gain": mp["max_gain"], "disconnected_communities": int(n_comp - np.unique(lab).size)}
    out["failed_gates"] = [g for g, bad in (("leiden_improving_moves", im["count"] > 0), ("leiden_mergeable_pairs", mp["count"] > 0),
                                            ("disconnected_communities", out["disconnected_communities"] != 0)) if bad]
    return out


def approx_knn_curve(emb, exact_idx, k: int, probes) -> dict:
    """`knn_approx`: scamd_knn_l2_ivf_f32 on the embedding of a timed step, per nprobe: recall@(k-1) against the exact
    lists (self excluded), wall of the call (events), select-kernel time, pairs evaluated / n^2."""
    import torch

    from scanpy_amd import _kernels as K
    from scanpy_amd import _lib

    lib = _lib.load()
    n = emb.shape[0]
    out = {"note": "every query block sweeps the nprobe cells nearest (centroid distance) to its own cell of the exact search's "
                   "k-means quantiser (~2048 rows per cell); exact inside the probed cells; 1 warm-up + 1 timed call per nprobe",
           "k": k, "runs": []}
    ex = exact_idx[:, 1:]
    for p in probes:
        K.knn(emb, k, nprobe=p)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        idx, _, n_fb = K.knn(emb, k, nprobe=p)
        e1.record()
        torch.cuda.synchronize()
        hit = 0
        for s0 in range(0, n, 65536):
            a, b = idx[s0:s0 + 65536, 1:], ex[s0:s0 + 65536]
            hit += int((a[:, :, None] == b[:, None, :]).any(2).sum())
        out["runs"].append({"nprobe": p, "recall": hit / float(n * (k - 1)), "ms": e0.elapsed_time(e1),
                            "select_ms": float(lib.scamd_knn_last_select_ms()),
                            "pairs_evaluated_fraction": float(lib.scamd_knn_last_select_pairs()) / float(n) ** 2,
                            "float64_scan_queries": int(n_fb)})
    return out


def structure_variant(args, backend, kw, structure: str, probes=(8, 32, 128)) -> dict:
    """`structure_none` / `structure_weak`: the path on another variant of the matrix of the same shape (rank 0, N=1)."""
    import torch

    from scanpy_amd import _lib
    from scanpy_amd._pipeline import run_path

    lib = _lib.load()
    x, _ = make_matrix(args.n_obs, args.n_vars, args.seed, structure)
    h = backend.upload(x)
    del x
    run_path(h, args.n_obs, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = run_path(h, args.n_obs, timing=True, **kw)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    sel, pairs = float(lib.scamd_knn_last_select_ms()), float(lib.scamd_knn_last_select_pairs())
    pre = float(lib.scamd_knn_last_select_prepass_pairs())
    brute = float(args.n_obs) ** 2
    tf = 2.0 * pairs * args.n_comps / (sel * 1e-3) / 1e12 if sel > 0 else None
    eng = int(lib.scamd_knn_last_select_engine())
    tf_exec = (3.0 * 2.0 * 64.0 if eng == 1 else 2.0 * args.n_comps) * pairs / (sel * 1e-3) / 1e12 if sel > 0 else None
    notes = {"none": "same shape, p_programme = 0 (i.i.d. genes): PCA spectrum without a gap, kNN without prunable cells",
             "weak": "same shape, p_programme = 0.12 (overlapping gene programmes): the ball bound of the exact search prunes "
                     "nothing, the communities are ambiguous"}
    out = {"note": notes.get(structure, structure) + "; 1 warm-up + 1 timed step, outside `value`",
           "knn_engine": "bf16x3" if eng == 1 else "f32", "knn_select_engine_tflops": tf_exec,
           "knn_select_frac_of_engine_peak": tf_exec / (2500.0 if eng == 1 else 157.3) if tf_exec else None,
           "ms_per_step": ms, "cells_per_s": args.n_obs / (ms * 1e-3), "stage_ms": res.stage_ms,
           "pairs_evaluated_fraction": pairs / brute, "prepass_pairs_fraction_of_useful": pre / pairs if pairs else None,
           "knn_select_ms": sel, "knn_select_tflops": tf,
           "knn_select_frac_of_157.3": tf / 157.3 if tf else None, "n_communities": res.n_communities,
           "modularity": res.modularity, "labels_sha": _sha(res.labels),
           "graph_sha": {"indptr": _sha(res.conn_indptr), "indices": _sha(res.conn_indices), "data": _sha(res.conn_data)},
           "pca_info": {k: v for k, v in res.info.items() if k not in ("knn_fallback_queries", "leiden_stats")},
           "leiden": leiden_block(res.info.get("leiden_stats", {}), res.stage_ms.get("leiden"))}
    out["leiden_guarantees"] = leiden_guarantees(res, args.n_obs)
    # the same graph under the setting the reference recommends for its igraph flavor and announces as its future default
    # (`n_iterations=2`, src/scanpy/tools/_leiden.py:247-256 warning text): what the stage costs when it is not run to stability
    from scanpy_amd import _kernels as K

    K.leiden(res.conn_indptr, res.conn_indices, res.conn_data, args.n_obs, n_iterations=2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, q2, nc2 = K.leiden(res.conn_indptr, res.conn_indices, res.conn_data, args.n_obs, n_iterations=2)
    torch.cuda.synchronize()
    out["leiden_n_iterations_2"] = {"ms": (time.perf_counter() - t0) * 1e3, "modularity": q2, "n_communities": nc2,
                                    "note": "tl.leiden(flavor='igraph', n_iterations=2) on the same graph; `stage_ms.leiden` is n_iterations=-1"}
    if probes:
        out["knn_approx"] = approx_knn_curve(res.x_pca, res.knn_indices, args.n_neighbors, probes)
    return out


def _profiled_traffic(mode: str, engine: str):
    """HBM-side bytes per launch of the roofline kernel from the committed PMC passes (rocprofv3 --pmc FETCH_SIZE /
    WRITE_SIZE are separate profiling runs, they cannot be taken inside this process); None if the committed passes
    are of a different sweep mode or scoring engine than the one that ran (or absent)."""
    f = ROOT / "profiles" / "knn_select_traffic.json"
    try:
        d = json.loads(f.read_text())
        return d["bytes_per_launch"] if d.get("mode") == mode and d.get("engine", "f32") == engine else None
    except (OSError, KeyError, ValueError):
        return None


def _baseline_config(n: int, g: int, world: int) -> str:
    """which BASELINE.json `configs` entry the run corresponds to (the label is informational)"""
    if (n, g) == (1_000_000, 2000):
        return "BASELINE configs[2]" if world == 1 else f"BASELINE configs[3] over {world} GPUs"
    if (n, g) == (100_000, 2000):
        return "BASELINE configs[1]"
    if (n, g) == (10_000_000, 4000):
        return "BASELINE configs[4] sizes, exact kNN, single resolution"
    return "custom size"


def upstream_chain(handle, reps: int = 3) -> dict:
    """SURVEY 8(f).2 rows, measured beside the path (NOT part of `value`): the device passes of
    normalize_total(1e4) -> log1p -> highly_variable_genes('seurat') statistics -> scale(zero_center=False) on the
    resident CSR, each against the HBM roofline with its algorithmic bytes (csrc/preprocess.hip header)."""
    import torch

    from scanpy_amd import _kernels as K

    ip, ix, dt, n, g = handle[:5]
    nnz = dt.numel()
    passes = [
        ("row_sums", 4 * nnz + 8 * (n + 1) + 4 * n),
        ("row_divide", 8 * nnz + 8 * (n + 1) + 4 * n),
        ("log1p", 8 * nnz),
        ("col_stats_expm1", 8 * nnz + 8 * (n + 1) + 24 * g),
        ("scale_csr", 12 * nnz + 8 * (n + 1) + 8 * g),
    ]
    best = [float("inf")] * len(passes)
    for _ in range(reps):
        d = dt.clone()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(passes) + 1)]
        ev[0].record()
        sums = K.pp_row_sums(ip, ix, d, n)
        ev[1].record()
        K.pp_row_divide_(ip, d, n, sums / 1e4)
        ev[2].record()
        K.pp_log1p_(d)
        ev[3].record()
        s, sq, _ = K.pp_col_stats(ip, ix, d, n, g, expm1_scale=1.0, count_positive=False)
        ev[4].record()
        K.pp_scale_csr_(ip, ix, d, n, torch.ones(g, dtype=torch.float64, device=d.device), max_value=10.0)
        ev[5].record()
        torch.cuda.synchronize()
        for i in range(len(passes)):
            best[i] = min(best[i], ev[i].elapsed_time(ev[i + 1]))
    out = {"note": "device passes of pp.normalize_total / log1p / highly_variable_genes / scale on the same CSR; "
                   "best of %d; outside `value`" % reps, "peak_GBps": 8000.0, "passes": {}}
    for (name, nbytes), ms in zip(passes, best):
        gbps = nbytes / (ms * 1e-3) / 1e9
        out["passes"][name] = {"ms": ms, "algorithmic_bytes": nbytes, "GBps": gbps, "frac": gbps / 8000.0}
    out["total_ms"] = sum(best)
    return out


def umap_layout(res, n: int, n_epochs: int = 200) -> dict:
    """SURVEY 8(f).1 row, measured beside the path (NOT part of `value`): the UMAP layout kernel on the fuzzy graph the
    timed path just produced (resident), random start, `n_epochs` synchronous epochs."""
    import torch

    from scanpy_amd import _kernels as K
    from scanpy_amd.tools._umap import find_ab_params, prune_and_schedule_device

    ip, ix, w, eps = prune_and_schedule_device(res.conn_indptr, res.conn_indices, res.conn_data, n, n_epochs)
    a, b = find_ab_params(1.0, 0.5)
    gen = torch.Generator(device="cpu").manual_seed(0)
    y = (torch.rand((n, 2), generator=gen) * 10.0).to(w.device).contiguous()
    fired = float(torch.floor(float(n_epochs - 1) / eps[eps > 0].to(torch.float64)).sum())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    K.umap_optimize_(ip, ix, eps, n, y, n_epochs=n_epochs, a=a, b=b, seed=0)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    nnz = int(ix.numel())
    # per epoch: 16 B of index + schedule per stored sample; a fired sample gathers one neighbour and ~5 negatives (8 B
    # each at n_components = 2) and rewrites 8 B of schedule; plus the embedding in and out
    bytes_total = n_epochs * (16.0 * nnz + 16.0 * n) + fired * (8.0 + 6 * 8.0)
    return {"note": "scamd_umap_optimize_f32 on the path's own fuzzy graph, random start; outside `value`",
            "n_epochs": n_epochs, "stored_samples": nnz, "fired_samples": fired, "ms": ms, "ms_per_epoch": ms / n_epochs,
            "gathers_per_s": fired * 6.0 / (ms * 1e-3), "algorithmic_GBps": bytes_total / (ms * 1e-3) / 1e9,
            "frac_of_8TBps": bytes_total / (ms * 1e-3) / 1e9 / 8000.0, "finite": bool(torch.isfinite(y).all())}


DUMP_SEED, DUMP_MAX_ROWS, DUMP_BUDGET_BYTES = 0, 32768, 48e6


def dump_outputs(res, n: int, lo: int, out_dir) -> dict:
    """`--dump-outputs DIR`: what the last timed step handed back (PathResult), as DIR/<name>.npy in float32 / float64, so
    that two builds can be compared output for output on identical inputs.  Per-cell arrays are cut to a fixed row sample
    (seed DUMP_SEED, the same for every run of the same size: `sample_rows`) so that the files stay far below 64 MB;
    integer arrays are stored as float64 (exact).  `lo` = first global row of this rank's shard."""
    import numpy as np
    import torch

    def host(t, ix=None):
        if hasattr(t, "detach"):
            t = t.detach()
            a = (t if ix is None else t[torch.as_tensor(ix, dtype=torch.int64, device=t.device)]).cpu().numpy()
        else:
            a = np.asarray(t) if ix is None else np.asarray(t)[ix]
        return a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)

    k = res.knn_indices.shape[1]
    per_row = 4 * res.x_pca.shape[1] + 16 * k + 12 * 2 * k + 16  # scores, kNN lists, ~2k graph entries, label, row id
    m = int(min(n, DUMP_MAX_ROWS, DUMP_BUDGET_BYTES // per_row))
    rows = np.sort(np.random.default_rng(DUMP_SEED).choice(n, size=m, replace=False))
    n_local = res.x_pca.shape[0]
    loc = rows[(rows >= lo) & (rows < lo + n_local)] - lo
    arrays = {"sample_rows": rows.astype(np.float64),
              "components": host(res.components), "variance": host(res.variance), "variance_ratio": host(res.variance_ratio),
              "x_pca_sample": host(res.x_pca, loc), "knn_indices_sample": host(res.knn_indices, loc),
              "knn_distances_sample": host(res.knn_distances, loc),
              "labels_sample": host(res.labels, rows),
              "modularity": np.array([res.modularity], dtype=np.float64),
              "n_communities": np.array([res.n_communities], dtype=np.float64)}
    if res.conn_indptr is not None:  # the graph's rows of the sample: their lengths, column ids and weights
        ip = res.conn_indptr.detach().cpu().numpy().astype(np.int64)
        start, lens = ip[rows], ip[rows + 1] - ip[rows]
        sel = np.repeat(start - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()))
        arrays["conn_row_nnz_sample"] = lens.astype(np.float64)
        arrays["conn_indices_sample"] = host(res.conn_indices, sel)
        arrays["conn_data_sample"] = host(res.conn_data, sel)
    total = sum(a.nbytes for a in arrays.values())
    if total > 64e6:
        raise SystemExit(f"--dump-outputs: {total / 1e6:.1f} MB of outputs, the limit is 64 MB")
    out_dir = Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    for name, a in arrays.items():
        np.save(out_dir / f"{name}.npy", np.ascontiguousarray(a))
    return {"dir": str(out_dir), "arrays": sorted(arrays), "sample_rows": m, "bytes": int(total)}


def main() -> None:
    args = parse_args()
    import torch

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run --nproc-per-node N for --gpus N > 1")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    # SCAMD_BENCH_ONE_DEVICE=1: validation mode, all ranks share cuda:0 and the collectives go through gloo (RCCL refuses
    # two ranks on one device); the numbers of such a run are meaningless, the code path is the multi-rank one
    one_device = os.environ.get("SCAMD_BENCH_ONE_DEVICE") == "1"
    if one_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    import torch.distributed as dist

    from scanpy_amd import _lib
    from scanpy_amd._pipeline import run_path, shard_bounds
    from scanpy_amd.preprocessing._pca_solver import GpuBackend, NoComm, TorchDistComm

    comm = NoComm()
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if one_device:
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=dev)
        comm = TorchDistComm()

    n = args.n_obs * (world if args.scaling == "weak" else 1)
    lo, hi = shard_bounds(n, world, rank)
    t_gen = time.perf_counter()
    x, truth = make_matrix(n, args.n_vars, args.seed, args.structure, row_range=(lo, hi))
    t_gen = time.perf_counter() - t_gen
    backend = GpuBackend()
    t_h2d = time.perf_counter()
    handle = backend.upload(x)
    torch.cuda.synchronize()
    t_h2d = time.perf_counter() - t_h2d
    nnz_local = x.nnz
    # the side measurements and the CPU legs (`--full`) need the host matrix: rank 0 of a single-GPU run only
    side = world == 1 and args.full
    if not side:
        del x

    def sync_all():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    kw = dict(comm=comm, backend=backend, n_comps=args.n_comps, n_neighbors=args.n_neighbors, resolution=1.0,
              n_iterations=-1, seed=0, nprobe=args.knn_nprobe if args.knn_nprobe > 0 else None)
    if args.knn_nprobe > 0:
        args.verify = False
    for _ in range(args.warmup):
        run_path(handle, n, **kw)
    lib = _lib.load()
    select_ms, select_pairs, prepass_pairs, stage_acc, res = [], [], [], {}, None
    sync_all()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = run_path(handle, n, timing=True, **kw)
        select_ms.append(float(lib.scamd_knn_last_select_ms()))
        select_pairs.append(float(lib.scamd_knn_last_select_pairs()))
        prepass_pairs.append(float(lib.scamd_knn_last_select_prepass_pairs()))
        for kname, v in res.stage_ms.items():
            stage_acc[kname] = stage_acc.get(kname, 0.0) + v
    sync_all()
    elapsed = time.perf_counter() - t0
    t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    if world > 1:
        if one_device:
            t = t.cpu()
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    ms_per_step = elapsed / max(args.steps, 1) * 1e3
    value = n * args.steps / elapsed
    # N > 1: every rank's stage times side by side (the first scaling run diagnoses itself: which stage stops scaling, how
    # much of the step is the rank-0-only Leiden), gathered with one small collective outside the timed region
    stage_names = ("pca", "knn", "connectivities", "leiden", "broadcast")
    per_rank = None
    if world > 1:
        mine = torch.tensor([stage_acc.get(k_, 0.0) / max(args.steps, 1) for k_ in stage_names], dtype=torch.float64,
                            device="cpu" if one_device else dev)
        allr = torch.empty(world * len(stage_names), dtype=torch.float64, device=mine.device)  # (flat: gloo insists)
        dist.all_gather_into_tensor(allr, mine)
        per_rank = [{k_: float(v) for k_, v in zip(stage_names, row)} for row in allr.view(world, len(stage_names)).cpu().tolist()]

    if rank == 0:
        dumped = dump_outputs(res, n, lo, args.dump_outputs) if args.dump_outputs else None
        sel = sum(select_ms) / max(len(select_ms), 1)
        n_query = hi - lo
        pairs = sum(select_pairs) / max(len(select_pairs), 1)  # (query, candidate) pairs the kernel evaluated
        brute_pairs = float(n_query) * float(n)
        # algorithmic flop of the launch = 2 * d flop per EVALUATED pair: the exact cell-pruned search skips the
        # cells that provably hold no neighbour, what it does evaluate runs on the FP32 MFMA pipe
        engine = int(lib.scamd_knn_last_select_engine())  # 1 = 3 x bf16 split products, 0 = float32 MFMA
        flop_per_pair = 3.0 * 2.0 * 64.0 if engine == 1 else 2.0 * args.n_comps
        flops = flop_per_pair * pairs
        achieved = flops / (sel * 1e-3) / 1e12 if sel > 0 else None
        peak = 2500.0 if engine == 1 else 157.3
        out = {
            "metric": "cells/sec through pca+neighbors+leiden, 1M x 2k CSR" if (n, args.n_vars) == (1_000_000, 2000) else f"cells/sec through pca+neighbors+leiden, {n} x {args.n_vars} CSR",
            "value": value,
            "unit": "cells/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "bf16x3" if int(lib.scamd_knn_last_select_engine()) == 1 else "f32",
            "data": "synthetic",
            "config": {
                "workload": (f"synthetic {args.structure}-structure log-normal CSR {n} cells x {args.n_vars} genes (~5% nnz), PCA {args.n_comps} "
                             f"(exact Gram + dense eigensolve, arpack accuracy) + "
                             + (f"APPROXIMATE IVF kNN k={args.n_neighbors}, nprobe={args.knn_nprobe} cells of the k-means quantiser (exact inside them)"
                                if args.knn_nprobe > 0 else f"exact kNN k={args.n_neighbors} (cell-pruned brute force)") + " + umap "
                             "connectivities + Leiden res=1.0 n_iterations=-1 (" + _baseline_config(n, args.n_vars, world) + "); `value` is the "
                             "device-resident rate: the CSR is in HBM when the timed region starts and the results stay there "
                             "(no H2D / D2H inside it); host AnnData in -> slots written on the host = value_host_to_host"),
                "n_obs": n,
                "n_vars": args.n_vars,
                "nnz_per_rank": int(nnz_local),
                "parallelism": (f"cells row-sharded x{world}: int64 Gram all-reduce, embedding all-gather, fuzzy-set rows per "
                                "rank with an all-to-all of the directed edges; leiden on rank 0"),
            },
            "roofline": {
                "kernel": ("knn_select_reg_kernel<25,64,3,IVF,B3> (v_mfma_f32_32x32x16_bf16 x 12 per 32x32 sub-tile: hi.hi + hi.lo + "
                           "lo.hi of the bf16 split), exact cell-pruned sweep" if engine == 1 else
                           "knn_select_reg_kernel<25,64,3> (v_mfma_f32_32x32x2_f32), exact cell-pruned sweep"),
                "engine": "bf16x3" if engine == 1 else "f32",
                "bound": "mfma",
                "achieved": achieved,
                "peak": peak,
                "unit": "TFLOP/s",
                "frac": (achieved / peak) if achieved else None,
                # the committed PMC passes (profiles/knn_select_traffic.json, separate FETCH_SIZE / WRITE_SIZE passes restricted
                # to this kernel) are of the single-GPU 1M x 1M launch of the planted matrix: not quoted for any other shape
                "traffic": (_profiled_traffic("ivf" if 0 < pairs < brute_pairs else "brute", "bf16x3" if engine == 1 else "f32")
                            if (n, args.n_comps, world, args.structure) == (1_000_000, 50, 1, "planted") else None),
                # algorithmic bytes of the launch: the image once (272 B per row, bf16 engine; 240 B float32) + the candidate
                # lists out (32 ids + threshold per query)
                "algorithmic_bytes_per_launch": float(n) * (272.0 if engine == 1 else 240.0) + float(n_query) * (32 * 4 + 4),
                "launch_ms": sel,
                # (`launch_ms` is the MEAN over the timed steps, as the contract asks; on a shared box one disturbed step
                # moves it -- the spread of the same launches beside it)
                "launch_ms_min_median_max": ([min(select_ms), sorted(select_ms)[len(select_ms) // 2], max(select_ms)]
                                             if select_ms else None),
                "algorithmic_flop_per_launch": flops,
                "flop_per_pair": flop_per_pair,
                # the same launch priced as rounds 1-2 priced the float32 engine: 2 * d flop per pair
                "f32_equivalent_tflops": 2.0 * pairs * args.n_comps / (sel * 1e-3) / 1e12 if sel > 0 else None,
                "f32_equivalent_frac_of_157.3": 2.0 * pairs * args.n_comps / (sel * 1e-3) / 1e12 / 157.3 if sel > 0 else None,
                "pairs_evaluated_fraction": pairs / brute_pairs if brute_pairs > 0 else None,
                # executed but not useful: the threshold pre-pass re-scores every block's own cell; NOT in `achieved`
                "prepass_pairs_fraction_of_useful": (sum(prepass_pairs) / max(len(prepass_pairs), 1)) / pairs if pairs > 0 else None,
                "executed_tflops_incl_prepass": (flop_per_pair * (pairs + sum(prepass_pairs) / max(len(prepass_pairs), 1))
                                                 / (sel * 1e-3) / 1e12) if sel > 0 else None,
                "brute_force_equivalent_tflops": 2.0 * brute_pairs * args.n_comps / (sel * 1e-3) / 1e12 if sel > 0 else None,
            },
            "stage_ms_per_step": {kname: v / max(args.steps, 1) for kname, v in stage_acc.items()},
            **({} if per_rank is None else {"multi_gpu": {
                "per_rank_stage_ms": per_rank,
                # bytes every rank contributes to / receives from each collective of one step
                "collective_bytes": {
                    "gram_all_reduce_int64": 8.0 * (((args.n_vars + 127) // 128 * 128) ** 2 + args.n_vars),
                    "embedding_all_gather_f32": 4.0 * n * args.n_comps,
                    "directed_edges_all_to_all": 12.0 * (hi - lo) * (args.n_neighbors - 1) * (world - 1) / world,
                    "graph_rows_to_rank0": 8.0 * 2 * (hi - lo) * (args.n_neighbors - 1) + 4.0 * (hi - lo),
                    "labels_broadcast_i32": 4.0 * n},
                "rank0_only_ms": stage_acc.get("leiden", 0.0) / max(args.steps, 1),
                "rank0_only_share_of_step": stage_acc.get("leiden", 0.0) / max(args.steps, 1) / ms_per_step if ms_per_step > 0 else None,
                "note": "Leiden runs on rank 0 (global community totals, order-dependent moves: SURVEY 8(e)); the other ranks "
                        "wait in the label broadcast -- Amdahl: speed-up <= 1 / (share + (1 - share) / N) of the 1-GPU step"}}),
            "leiden": leiden_block(res.info.get("leiden_stats", {}), stage_acc.get("leiden", 0.0) / max(args.steps, 1)),
            "result": {"n_communities": res.n_communities, "modularity": res.modularity, "labels_sha": _sha(res.labels),
                       "knn_second_tier_queries": int(lib.scamd_knn_last_second_tier_queries()),
                       **{k_: v_ for k_, v_ in res.info.items() if k_ != "leiden_stats"}},
            "setup_s": {"generate": t_gen, "h2d": t_h2d},
        }
        out["config"]["structure"] = args.structure
        if dumped:
            out["dump_outputs"] = dumped
        rc = 0
        if side:
            if not args.no_side:
                out["upstream_chain"] = upstream_chain(handle)
                out["umap_layout"] = umap_layout(res, n)
            if not args.no_properties:
                # the result of the LAST timed step, at the full size of the run; its gates are part of the exit code
                # (round 4; a checker error propagates like any other error)
                out["full_size_properties"] = full_size_properties(res, x, n, args.n_neighbors, approximate=args.knn_nprobe > 0)
                out["full_size_properties"]["enforced"] = True
                if out["full_size_properties"]["failed_gates"]:
                    rc = 1
            if not args.no_side and args.knn_nprobe == 0:  # (the curve is measured against the EXACT lists of the timed step)
                out["knn_approx"] = approx_knn_curve(res.x_pca, res.knn_indices, args.n_neighbors, (2, 8, 32))
            del handle, res
            if args.h2h_reps > 0:
                h2h = host_to_host(x, args.n_comps, args.n_neighbors, args.h2h_reps)
                out["value_host_to_host"] = h2h["value"]
                out["value_h2h"] = h2h["value"]  # (same number under the short name; also inside `config`, which the driver's record keeps whole)
                out["config"]["value_h2h_cells_per_s"] = h2h["value"]
                out["config"]["h2h_ms_per_pass"] = h2h["best"]["total_ms"] if isinstance(h2h.get("best"), dict) and "total_ms" in h2h["best"] else None
                out["host_to_host"] = h2h
            variant_fails = []
            for st in ("none", "weak"):
                if not args.no_noise_variant and args.structure != st:
                    out["structure_" + st] = structure_variant(args, backend, kw, st, probes=() if args.no_side else (8, 32, 128))
                    variant_fails += [f"structure_{st}:{g}" for g in out["structure_" + st]["leiden_guarantees"]["failed_gates"]]
            if variant_fails:
                out["variant_failed_gates"] = variant_fails
                rc = 1
            if args.cpu_sizes:
                out["cpu_baseline"], chain = cpu_baseline(x, truth, args.cpu_sizes, n, args.n_comps, args.n_neighbors,
                                                          args.cpu_budget_s)
                if args.verify is not False:
                    par = parity_block(x, truth if args.structure != "none" else None, chain, args.n_comps, args.n_neighbors)
                    if args.structure == "none":
                        # i.i.d. genes: no spectral gap (loadings are arbitrary within the bulk) and no communities
                        # -> only the kNN and connectivity gates are meaningful
                        par["failed_gates"] = [f for f in par["failed_gates"] if f in ("knn_rows_differing_beyond_ties", "conn_max_abs")]
                        par["note"] = "structure none: loadings / label gates not asserted"
                    if args.structure == "planted":
                        par["weak"] = parity_weak(args)
                        par["failed_gates"] = par["failed_gates"] + par["weak"]["failed_gates"]
                    out["parity"] = par
                    rc = 1 if par["failed_gates"] else rc
        print(json.dumps(out), flush=True)
        if rc:
            print(f"GATES FAILED: parity {out.get('parity', {}).get('failed_gates')}, full-size properties "
                  f"{out.get('full_size_properties', {}).get('failed_gates')}, variants {out.get('variant_failed_gates')}",
                  file=sys.stderr, flush=True)
            if world > 1:
                dist.destroy_process_group()
            raise SystemExit(2)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
