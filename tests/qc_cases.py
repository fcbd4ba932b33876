"""TEST INFRASTRUCTURE shared by tests/test_gpu_qc.py (the product library on the GPU), tests/test_emu_qc_cpu.py (the same
kernels on the host emulator) and tests/test_qc_front_cpu.py (the front end on a CPU stand-in): the case table of the
quality-control kernels (csrc/qc.hip: `scamd_pp_qc_sweep_f32`, `scamd_pp_qc_top_f32`), restatements of the rules by which the
host code picks an instantiation and a grid, a numpy restatement of the top-n rule and of the obs / var column formulas, input
builders, ONE checker per primitive and a CPU stand-in for `GpuPPBackend.qc_sweep`.  Nothing here touches a device; the callers
hand in `QcAbi` over host memory (tests/emu/harness.py:HostMem) or device memory (graph_kernel_cases.DeviceMem).

The top-n rule (include/scanpy_amd.h): for one row, the stored non-zero values padded with zeros up to n_max = max(positions)
elements; top(n) = the sum of the n largest elements of that multiset."""
from __future__ import annotations

import ctypes as C
import math
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
import pandas as pd
from scipy import sparse

from graph_kernel_cases import EINVAL, EUNSUPPORTED, DeviceMem  # noqa: F401  (DeviceMem: for the GPU tests)
from stub_backend import CpuStubPPBackend

CSRC = Path(__file__).resolve().parent.parent / "scanpy_amd" / "csrc"

# ---------------------------------------------------------------------------------------------------------------------
# The dispatch rules restated; `assert_sources_still_say_so` ties them to the text of csrc/qc.hip.
# ---------------------------------------------------------------------------------------------------------------------
QC_BLOCK = 256
QC_LDS_GENES = 4096          # per-gene tables up to this many genes live in LDS
QC_GRID_CAP = 256 * 32       # workgroups of a row-wise launch
QC_LDS_GRID_CAP = 512        # workgroups of the sweep with the LDS table
QC_LDS_ROWS = 16             # ... which takes 16 rows per lane group and launch
QC_MAX_MASKS = 32
QC_MAX_POSITIONS = 16
QC_MAX_TOP = 4096
QC_TOP_KEYS = 8192           # staged keys per workgroup
QC_G = (8, 16, 32, 64)       # lanes per row of the sweep
QC_MK = (0, 4, 32)           # masked totals kept per lane
QC_T = (64, 256)             # threads per row of the top-n kernel
QC_TOP_AVG = 256             # ... a wave per row up to this mean row length
U = 2.0 ** -52               # the unit of the float64 bounds


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def sweep_lanes(nnz: int, n: int) -> int:
    avg = nnz // n if n > 0 else 0
    return 8 if avg <= 32 else (16 if avg <= 160 else (32 if avg <= 512 else 64))


def sweep_mk(n_masks: int) -> int:
    return 0 if n_masks == 0 else (4 if n_masks <= 4 else 32)


def col_table(g: int) -> str:
    return "lds" if g <= QC_LDS_GENES else "global"


def sweep_grid(n: int, G: int, table: str, capped: bool = True) -> int:
    if table == "lds":
        blocks = max(_cdiv(n, (QC_BLOCK // G) * QC_LDS_ROWS), 1)
        return min(blocks, QC_LDS_GRID_CAP) if capped else blocks
    blocks = max(_cdiv(n, QC_BLOCK // G), 1)
    return min(blocks, QC_GRID_CAP) if capped else blocks


def top_threads(nnz: int, n: int, nmax: int) -> int:
    avg = nnz // n if n > 0 else 0
    return 64 if avg <= QC_TOP_AVG and nmax <= QC_TOP_KEYS // 4 else 256


def top_capacity(T: int) -> int:
    """staged keys per row: a longer row runs the selection first"""
    return QC_TOP_KEYS // (QC_BLOCK // T)


def top_grid(n: int, T: int, capped: bool = True) -> int:
    blocks = max(_cdiv(n, QC_BLOCK // T), 1)
    return min(blocks, QC_GRID_CAP) if capped else blocks


def assert_sources_still_say_so():
    """the constants and thresholds above, read out of the text of csrc/qc.hip"""
    qc = (CSRC / "qc.hip").read_text()

    def has(pattern, what):
        assert re.search(pattern, qc), f"{what}: /{pattern}/ no longer in csrc/qc.hip -- restate the rule and its cases"

    has(rf"constexpr int QC_BLOCK = {QC_BLOCK};", "QC_BLOCK")
    has(rf"constexpr int QC_LDS_GENES = {QC_LDS_GENES};", "QC_LDS_GENES")
    assert QC_GRID_CAP == 256 * 32
    has(r"constexpr int QC_GRID_CAP = 256 \* 32;", "QC_GRID_CAP")
    has(rf"constexpr int QC_LDS_GRID_CAP = {QC_LDS_GRID_CAP};", "QC_LDS_GRID_CAP")
    has(rf"constexpr int QC_MAX_MASKS = {QC_MAX_MASKS};", "QC_MAX_MASKS")
    has(rf"constexpr int QC_MAX_POSITIONS = {QC_MAX_POSITIONS};", "QC_MAX_POSITIONS")
    has(rf"constexpr int QC_MAX_TOP = {QC_MAX_TOP};", "QC_MAX_TOP")
    has(rf"constexpr int QC_TOP_KEYS = {QC_TOP_KEYS};", "QC_TOP_KEYS")
    has(r"return avg <= 32 \? 8 : \(avg <= 160 \? 16 : \(avg <= 512 \? 32 : 64\)\);", "qc_lanes_per_row")
    has(rf"return \(avg <= {QC_TOP_AVG} && nmax <= QC_TOP_KEYS / 4\) \? 64 : 256;", "qc_top_threads")
    has(r"constexpr int R = QC_BLOCK / T, CAP = QC_TOP_KEYS / R, WPR = T / 64;", "rows and staged keys per workgroup")
    has(r"const bool lng = m > CAP;", "the selection starts beyond the staging capacity")
    has(r"const int cols = !want_cols \? 0 : \(g <= QC_LDS_GENES \? 1 : 2\);", "per-gene table split")
    has(r"const int mk = n_masks == 0 \? 0 : \(n_masks <= 4 \? 4 : QC_MAX_MASKS\);", "masked totals per lane")
    has(r"const size_t lds = \(size_t\)g \* \(8 \+ 4\) \+ 16;", "per-gene table LDS bytes")
    has(rf"ceil_div\(n, RPB \* {QC_LDS_ROWS}\), 1\), QC_LDS_GRID_CAP\)", "sweep grid, LDS table")
    has(r"std::max<int64_t>\(ceil_div\(n, RPB\), 1\), QC_GRID_CAP\)", "sweep grid")
    has(r"ceil_div\(n, QC_BLOCK / 64\), 1\), QC_GRID_CAP\)", "top-n grid, T = 64")
    has(r"std::min<int64_t>\(n, QC_GRID_CAP\)", "top-n grid, T = 256")
    has(r"while \(psz < m\) psz <<= 1;", "the sort pads to the next power of two")
    for G in QC_G[:-1]:
        has(rf"case {G}: return qc_launch_sweep_masks<{G}>\(", f"sweep G = {G}")
    has(r"default: return qc_launch_sweep_masks<64>\(", "sweep G = 64")
    has(r"case 0: return qc_launch_sweep<G, 0>\(", "MK = 0")
    has(r"case 4: return qc_launch_sweep<G, 4>\(", "MK = 4")
    has(r"default: return qc_launch_sweep<G, QC_MAX_MASKS>\(", "MK = 32")


# ---------------------------------------------------------------------------------------------------------------------
# Case table.  One matrix per case: the row lengths that matter for its positions, thread count and staging capacity, filled
# up with ordinary rows to the mean row length that selects the instantiation.  `avg` = nnz // n of the matrix.
# ---------------------------------------------------------------------------------------------------------------------
SIXTEEN = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 500, 610, 700)
#            name            g     positions              avg  values       masks
TOP_CASES = (
    ("default-wave",      700, (50, 100, 200, 500),       256, "counts",    1),
    ("default-block",     700, (50, 100, 200, 500),       257, "counts0",   3),
    ("one",               300, (1,),                       32, "two",       0),
    ("small",             300, (1, 2, 3, 10),              33, "ones",      32),
    ("p64",               300, (64,),                     160, "lognormal", 3),
    ("sixteen",           700, SIXTEEN,                   161, "negative",  32),
    ("p4096",            4200, (4096,),                   513, "counts",    0),
    ("cap-wave",         2100, (50, 100, 200, 500),       200, "two",       1),
    ("cap-block",        8200, (50, 500, 4096),           512, "counts0",   0),
    ("cap-block-neg",    8200, (4096,),                   600, "negative",  0),
    ("extreme",           300, (1, 2, 3, 10),              20, "extreme",   1),
)
TOP_CASE_NAMES = tuple(c[0] for c in TOP_CASES)
COL_TABLE_G = (1, QC_LDS_GENES - 1, QC_LDS_GENES, QC_LDS_GENES + 1)
GLOBAL_G_EXTRA = 104           # the matrices of the table also run the global per-gene table, by passing g = QC_LDS_GENES + this
HOT_COLUMN = 0
GRID_CAP_ROWS = QC_GRID_CAP * 32 + 32   # G = 8: one block more than QC_GRID_CAP, and one more than the LDS launch takes
GRID_CAP_TOP_ROWS = QC_GRID_CAP * 4 + 4  # T = 64: one block more than QC_GRID_CAP
GRID_CAP_G = 64


def _case(name):
    return next(c for c in TOP_CASES if c[0] == name)


def special_lengths(g: int, positions, T: int):
    """0 and 1, both sides of every position, of a wave, of the workgroup, of the threads per row, of every power of two the
    sort pads to, of the staging capacity; g itself (twice)"""
    cap = top_capacity(T)
    s = {0, 1, 63, 64, 65, QC_BLOCK - 1, QC_BLOCK, QC_BLOCK + 1, T - 1, T, T + 1, cap - 1, cap, cap + 1}
    for p in positions:
        s |= {p - 1, p, p + 1}
    k = 2
    while k <= min(g, cap):
        s |= {k - 1, k, k + 1}
        k *= 2
    return sorted(v for v in s if 0 <= v <= g) + [g, g]


@lru_cache(maxsize=None)
def case_lengths(name: str):
    """-> lengths [n] with sum // n == avg; rows 0, n // 2 and n - 1 are empty"""
    _, g, positions, avg, _, _ = _case(name)
    T = 64 if avg <= QC_TOP_AVG and max(positions) <= QC_TOP_KEYS // 4 else 256
    special = special_lengths(g, positions, T)
    n = max(sum(special) // avg + 8, len(special) + 24)
    rng = np.random.default_rng(sum(map(ord, name)))
    m = n - len(special) - 3
    total = avg * n + n // 2
    rem = total - sum(special)
    assert m > 2 and 0 <= rem <= m * g, (name, m, rem)
    fill = np.full(m, rem // m, dtype=np.int64)
    fill[: rem % m] += 1
    d = rng.integers(0, min(rem // m, g - rem // m - 1) // 2 + 1, m // 2)
    fill[0:2 * (m // 2):2] += d
    fill[1:2 * (m // 2):2] -= d
    body = rng.permutation(np.concatenate([special, fill]))
    lengths = np.zeros(n, dtype=np.int64)
    lengths[np.setdiff1d(np.arange(n), (0, n // 2, n - 1))] = body
    assert lengths.sum() == total and total // n == avg and lengths.min() >= 0 and lengths.max() <= g
    assert set(special) <= set(lengths.tolist()) and top_threads(total, n, max(positions)) == T
    return lengths


def _values(kind: str, lengths, positions, rng):
    nnz = int(lengths.sum())
    if kind in ("counts", "counts0"):
        v = np.floor(2.0 ** rng.uniform(0, 20, nnz))          # integers spread over 1 .. 2^20
        if kind == "counts0":
            v[rng.random(nnz) < 0.1] = 0.0                     # stored explicit zeros
    elif kind == "ones":
        v = np.ones(nnz)
    elif kind == "two":                                        # two values, the tie straddling each position
        v = np.full(nnz, 3.0)
        off = 0
        choices = sorted({0} | {q for p in positions for q in (p - 1, p, p + 1)})
        for ln in lengths:
            hi = min(int(rng.choice(choices + [ln])), ln)
            v[off + rng.permutation(ln)[:hi]] = 7.0
            off += ln
    elif kind == "negative":
        v = rng.integers(-50, 51, nnz).astype(np.float64)     # zeros among them
        v[rng.random(nnz) < 0.3] *= -1
    elif kind == "lognormal":
        v = rng.lognormal(0.5, 1.5, nnz)
    elif kind == "extreme":
        v = np.floor(2.0 ** rng.uniform(0, 10, nnz))
        v[rng.random(nnz) < 0.1] = 0.0
    else:
        raise ValueError(kind)
    return v.astype(np.float32)


EXTREME_ROWS = (
    # subnormals, +-1.0 and values near 3e38 in one row: a selection on bit patterns must order signs and exponents
    np.array([1e-45, 3e38, -1e-41, 1.0, 1e-40, -1.0, 2.9e38, 0.0, -3e38, 1.1754944e-38, 5e-39, -0.0, 2.0], dtype=np.float32),
    # no large value: the subnormals decide
    np.array([1e-45, 3e-45, 1e-40, 1.1754944e-38, 1e-38, -1e-45, 1e-30, -1e-30, 0.0, 7e-42, 6e-39, 2e-38], dtype=np.float32),
)


@lru_cache(maxsize=None)
def case_matrix(name: str) -> sparse.csr_matrix:
    """unique ascending columns; cached and read-only: one input per case for every test"""
    _, g, positions, _, kind, _ = _case(name)
    lengths = case_lengths(name)
    rng = np.random.default_rng(17 + sum(map(ord, name)))
    cols = [np.sort(rng.choice(g, size=ln, replace=False)) if ln < g else np.arange(g) for ln in lengths]
    indices = np.concatenate(cols).astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    data = _values(kind, lengths, positions, rng)
    if kind in ("counts0", "extreme"):   # one row whose stored values are all zero
        r = int(np.flatnonzero(lengths == 65)[0])
        data[indptr[r]: indptr[r + 1]] = 0.0
    if kind == "extreme":
        for row, src in zip(np.flatnonzero(lengths >= 13)[:2], EXTREME_ROWS):
            data[indptr[row]: indptr[row + 1]] = 0.0   # (the rest of the row: stored zeros)
            data[indptr[row]: indptr[row] + len(src)] = src
    x = sparse.csr_matrix((data, indices, indptr), shape=(len(lengths), g))
    assert x.has_sorted_indices and x.nnz == lengths.sum()
    for a in (x.data, x.indices, x.indptr):
        a.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def case_masks(name: str) -> np.ndarray:
    """bool [k, g]: for k = 3 and 32 one mask selects no gene and one all genes"""
    _, g, _, _, _, k = _case(name)
    return make_masks(k, g, seed=sum(map(ord, name)))


def make_masks(k: int, g: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(900 + seed)
    masks = rng.random((k, g)) < rng.uniform(0.02, 0.6, (k, 1))
    if k >= 3:
        masks[1] = False
        masks[k - 1] = True
    return masks


@lru_cache(maxsize=None)
def col_table_matrix(g: int) -> sparse.csr_matrix:
    """311 rows of about 20 counts; HOT_COLUMN in every non-empty row, columns g // 3 and g - 1 in none (g > 3)"""
    n = 311
    rng = np.random.default_rng(g)
    ln = rng.integers(0, 40, n) if g > 1 else rng.integers(0, 2, n)
    ln[[0, n // 2, n - 1]] = 0
    allowed = np.setdiff1d(np.arange(g), [HOT_COLUMN, g // 3, g - 1])
    cols = [np.sort(np.concatenate([[HOT_COLUMN], rng.choice(allowed, size=v - 1, replace=False)])) for v in ln if v]
    indices = np.concatenate(cols).astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    data = np.floor(2.0 ** rng.uniform(0, 20, len(indices))).astype(np.float32)
    data[rng.random(len(data)) < 0.05] = 0.0
    x = sparse.csr_matrix((data, indices, indptr), shape=(n, g))
    for a in (x.data, x.indices, x.indptr):
        a.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def grid_cap_matrix() -> sparse.csr_matrix:
    """GRID_CAP_ROWS rows of 0 or 2..6 counts over 64 columns (columns 61..63 receive nothing): G = 8"""
    n, g = GRID_CAP_ROWS, GRID_CAP_G
    rng = np.random.default_rng(8192)
    ln = rng.integers(1, 7, n)
    ln[ln == 1] = 0
    ln[[0, n // 2, n - 1]] = 0
    used = g - 3
    start, stride = rng.integers(0, used, n), rng.integers(1, used, n)
    c = (start[:, None] + np.arange(6)[None, :] * stride[:, None]) % used
    keep = np.arange(6)[None, :] < ln[:, None]
    c = np.sort(np.where(keep, c, g + 1), axis=1)
    indices = c[c < g].astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    data = rng.integers(0, 60, len(indices)).astype(np.float32)  # (stored zeros among them)
    x = sparse.csr_matrix((data, indices, indptr), shape=(n, g))
    assert sweep_lanes(x.nnz, n) == 8
    for a in (x.data, x.indices, x.indptr):
        a.setflags(write=False)
    return x


def assert_every_qc_path_has_a_case():
    """-> (the (G, MK, table) the sweep reaches, the T the top-n kernel reaches)"""
    sweep, tops = set(), set()
    for name, g, positions, avg, _, k in TOP_CASES:
        lengths = case_lengths(name)
        n, nnz = len(lengths), int(lengths.sum())
        assert nnz // n == avg
        T = top_threads(nnz, n, max(positions))
        tops.add(T)
        cap = top_capacity(T)
        have = set(lengths.tolist())
        want = {0, 1, 63, 64, 65, QC_BLOCK - 1, QC_BLOCK, QC_BLOCK + 1, g} | {q for p in positions for q in (p - 1, p, p + 1)}
        assert {v for v in want if v <= g} <= have, (name, sorted(want - have))
        assert (lengths == g).sum() >= 2 and (lengths[[0, n // 2, n - 1]] == 0).all()
        if g > cap:
            assert {cap - 1, cap, cap + 1, g} <= have, name
        for tbl_g in (g, QC_LDS_GENES + GLOBAL_G_EXTRA):
            sweep.add((sweep_lanes(nnz, n), sweep_mk(k), col_table(max(tbl_g, g))))
        assert sweep_grid(n, 8, "global") < QC_GRID_CAP and top_grid(n, 64) < QC_GRID_CAP  # (the table stays below the caps)
    assert tops == set(QC_T)
    avgs = {c[3] for c in TOP_CASES}
    assert {32, 33, 160, 161, 512, 513, QC_TOP_AVG, QC_TOP_AVG + 1} <= avgs
    assert {G for G, _, _ in sweep} == set(QC_G) and {mk for _, mk, _ in sweep} == set(QC_MK)
    assert {t for _, _, t in sweep} == {"lds", "global"}
    assert {len(c[2]) for c in TOP_CASES} >= {1, 4, QC_MAX_POSITIONS} and {c[5] for c in TOP_CASES} >= {0, 1, QC_MAX_MASKS}
    # rows beyond the staging capacity at both thread counts, and n_max = QC_MAX_TOP with such rows
    long_cases = {top_threads(int(case_lengths(c[0]).sum()), len(case_lengths(c[0])), max(c[2])) for c in TOP_CASES
                  if c[1] > top_capacity(top_threads(int(case_lengths(c[0]).sum()), len(case_lengths(c[0])), max(c[2])))}
    assert long_cases == set(QC_T)
    assert any(max(c[2]) == QC_MAX_TOP and c[1] > QC_TOP_KEYS for c in TOP_CASES)
    assert any(c[2] == (QC_MAX_TOP,) and c[1] == 4200 for c in TOP_CASES)
    assert {col_table(g) for g in COL_TABLE_G} == {"lds", "global"} and {1, QC_LDS_GENES, QC_LDS_GENES + 1} <= set(COL_TABLE_G)
    n = GRID_CAP_ROWS
    assert sweep_grid(n, 8, "global", capped=False) == QC_GRID_CAP + 1 > sweep_grid(n, 8, "global")
    assert sweep_grid(n, 8, "lds", capped=False) == QC_LDS_GRID_CAP + 1 > sweep_grid(n, 8, "lds")
    assert top_grid(GRID_CAP_TOP_ROWS, 64, capped=False) == QC_GRID_CAP + 1 > top_grid(GRID_CAP_TOP_ROWS, 64)
    return sweep, tops


# ---------------------------------------------------------------------------------------------------------------------
# The restatement: the rule, in numpy.  Integer-valued data in int64 (exact), other data in float64 with exactly rounded
# sums (math.fsum), so that the whole bound belongs to the code under test.
# ---------------------------------------------------------------------------------------------------------------------
def integer_valued(x) -> bool:
    d = np.asarray(x.data, dtype=np.float64)
    return bool(np.all(d == np.rint(d)) and np.all(np.abs(d) <= 2.0 ** 24))


def _rows(x):
    return np.repeat(np.arange(x.shape[0]), np.diff(x.indptr))


def ref_sweep(x, masks, g_pass=None) -> dict:
    """x: scipy CSR float32; masks bool [k, g] -> the primitives and, per primitive, the sum of |values| and the number of
    entries behind each element (for the bounds)"""
    n, g = x.shape
    g_out = g if g_pass is None else g_pass
    exact = integer_valued(x)
    d = np.asarray(x.data, dtype=np.float64)
    nz = d != 0
    rows, cols = _rows(x)[nz], np.asarray(x.indices)[nz]
    d = d[nz]
    k = len(masks)

    def sums(idx, vals, size):
        if exact:
            return np.bincount(idx, weights=vals, minlength=size)  # integers below 2^53: every order is exact
        out = np.zeros(size)
        order = np.argsort(idx, kind="stable")
        bounds = np.searchsorted(idx[order], np.arange(size + 1))
        for i in range(size):
            if bounds[i + 1] > bounds[i]:
                out[i] = math.fsum(vals[order[bounds[i]:bounds[i + 1]]])
        return out

    res = {"row_nnz": np.bincount(rows, minlength=n).astype(np.int64), "row_total": sums(rows, d, n),
           "row_abs": np.bincount(rows, weights=np.abs(d), minlength=n),
           "col_nnz": np.bincount(cols, minlength=g_out).astype(np.int64), "col_sum": sums(cols, d, g_out),
           "col_abs": np.bincount(cols, weights=np.abs(d), minlength=g_out), "negative": bool((d < 0).any()),
           "row_masked": np.zeros((k, n)), "masked_abs": np.zeros((k, n)), "masked_nnz": np.zeros((k, n), dtype=np.int64)}
    for j in range(k):
        sel = np.asarray(masks[j], dtype=bool)[cols]
        res["row_masked"][j] = sums(rows[sel], d[sel], n)
        res["masked_abs"][j] = np.bincount(rows[sel], weights=np.abs(d[sel]), minlength=n)
        res["masked_nnz"][j] = np.bincount(rows[sel], minlength=n)
    return res


def ref_top(x, positions):
    """-> (top [n, len(positions)] float64, sum of |values| of the elements behind each): sort each row descending, pad,
    cumulative sum"""
    n = x.shape[0]
    nmax = max(positions)
    exact = integer_valued(x)
    top, sabs = np.zeros((n, len(positions))), np.zeros((n, len(positions)))
    for r in range(n):
        v = np.asarray(x.data[x.indptr[r]: x.indptr[r + 1]], dtype=np.float64)
        v = v[v != 0]
        v = np.sort(np.concatenate([v, np.zeros(max(nmax - len(v), 0))]))[::-1]
        for j, p in enumerate(positions):
            if exact:
                top[r, j] = float(int(v[:p].astype(np.int64).sum()))
            else:
                top[r, j] = math.fsum(v[:p])
            sabs[r, j] = np.abs(v[:p]).sum()
    return top, sabs


def ref_columns(prim: dict, dtype, n_obs: int, *, expr_type="counts", var_type="genes", qc_vars=(), percent_top=(), log1p=True):
    """The obs / var column formulas of the reference (`describe_obs`, `describe_var`) on the primitives, in the reference's
    dtypes under numpy's conventions: non-zero counts int64, totals float32 for float32 input and int64 for integer input,
    `mean_*` float64, the derived columns whatever numpy makes of the formula.  prim: row_nnz, row_total, row_masked [k, n],
    top [n, len(sorted unique percent_top)], col_nnz, col_sum (float64 / int64 as the device returns them)."""
    dtype = np.dtype(dtype)

    def total(v):
        return np.rint(v).astype(np.int64) if dtype.kind == "i" else np.asarray(v).astype(dtype)

    obs, var = {}, {}
    with np.errstate(invalid="ignore", divide="ignore"):
        nnz = np.asarray(prim["row_nnz"], dtype=np.int64)
        obs[f"n_{var_type}_by_{expr_type}"] = nnz
        if log1p:
            obs[f"log1p_n_{var_type}_by_{expr_type}"] = np.log1p(nnz)
        tot = total(prim["row_total"])
        obs[f"total_{expr_type}"] = tot
        if log1p:
            obs[f"log1p_total_{expr_type}"] = np.log1p(tot)
        ns = sorted(percent_top or ())
        uniq = sorted(set(ns))
        for p in ns:
            obs[f"pct_{expr_type}_in_top_{p}_{var_type}"] = (prim["top"][:, uniq.index(p)] / tot.astype(np.float64)) * 100
        for k, name in enumerate(qc_vars):
            part = total(prim["row_masked"][k])
            obs[f"total_{expr_type}_{name}"] = part
            if log1p:
                obs[f"log1p_total_{expr_type}_{name}"] = np.log1p(part)
            obs[f"pct_{expr_type}_{name}"] = part / tot * 100
        n_cells = np.asarray(prim["col_nnz"], dtype=np.int64)
        mean = np.asarray(prim["col_sum"], dtype=np.float64) / np.float64(n_obs)
        var[f"n_cells_by_{expr_type}"] = n_cells
        var[f"mean_{expr_type}"] = mean
        if log1p:
            var[f"log1p_mean_{expr_type}"] = np.log1p(mean)
        var[f"pct_dropout_by_{expr_type}"] = (1 - n_cells / n_obs) * 100
        ctot = total(prim["col_sum"])
        var[f"total_{expr_type}"] = ctot
        if log1p:
            var[f"log1p_total_{expr_type}"] = np.log1p(ctot)
    return obs, var


def ref_primitives(x, masks, positions) -> dict:
    """the restated primitives of a host matrix (CSR / CSC / dense), as `GpuPPBackend.qc_sweep` returns them"""
    m = sparse.csr_matrix(x).astype(np.float32)
    m.sum_duplicates()
    r = ref_sweep(m, masks)
    uniq = sorted(set(positions or ()))
    r["top"] = ref_top(m, uniq)[0] if uniq else None
    return r


def assert_frames_equal_columns(frame: pd.DataFrame, cols: dict, what=""):
    """same columns, same order, same dtypes, same bits (NaN where the reference divides 0 by 0)"""
    assert list(frame.columns) == list(cols), (what, list(frame.columns), list(cols))
    for name, want in cols.items():
        got = frame[name].to_numpy()
        assert got.dtype == want.dtype, (what, name, got.dtype, want.dtype)
        assert np.array_equal(got, want, equal_nan=want.dtype.kind == "f"), (what, name)


# ---------------------------------------------------------------------------------------------------------------------
# Callers of the two entry points through the raw C ABI: numpy in, numpy out, the return code handed back, outputs prefilled
# (NaN / -1) so that an element nobody wrote shows.  `mem`: tests/emu/harness.py:HostMem or graph_kernel_cases.DeviceMem.
# ---------------------------------------------------------------------------------------------------------------------
def pack_masks(masks) -> np.ndarray:
    masks = np.asarray(masks, dtype=bool)
    if masks.shape[0] == 0:
        return np.zeros(masks.shape[1], dtype=np.uint32)
    return (masks.astype(np.uint32) << np.arange(masks.shape[0], dtype=np.uint32)[:, None]).sum(axis=0, dtype=np.uint32)


class QcAbi:
    def __init__(self, lib, mem):
        self.lib, self.mem = lib, mem

    def _in(self, x, null):
        m = self.mem
        bufs = (m.put(x.indptr, np.int64), m.put(x.indices, np.int32), m.put(x.data, np.float32))
        z = C.c_void_p(0)
        return bufs, [z if name in null else m.ptr(b) for name, b in zip(("indptr", "indices", "data"), bufs)]

    def sweep(self, x, masks=None, *, n=None, g=None, nnz=None, n_masks=None, null=(), per_gene=True):
        """masks: bool [k, columns of x] or None; n / g / nnz / n_masks: the values PASSED where they are to differ; null:
        names of pointers passed as NULL.  -> (rc, dict of outputs); the per-gene outputs are sized by the g passed (at most
        2^16 elements), row_masked by the masks given"""
        m = self.mem
        keep, (ip, ix, dv) = self._in(x, null)
        nr, gx = x.shape
        g = gx if g is None else g
        k = 0 if masks is None else len(masks)
        ga = max(min(g, 1 << 16), gx, 1)
        bits = np.zeros(ga, dtype=np.uint32)
        if k:
            bits[:gx] = pack_masks(masks)
        d_bits = m.put(bits.view(np.int32), np.int32)
        out = {"row_nnz": m.full(max(nr, 1), np.int32, -1), "row_total": m.full(max(nr, 1), np.float64, np.nan),
               "row_masked": m.full((max(k, 1), max(nr, 1)), np.float64, np.nan), "col_nnz": m.full(ga, np.int64, -1),
               "col_sum": m.full(ga, np.float64, np.nan), "flags": m.full(1, np.int32, -1)}
        z = C.c_void_p(0)

        def p(name, on=True):
            return z if name in null or not on else m.ptr(out[name])

        rc = self.lib.scamd_pp_qc_sweep_f32(ip, ix, dv, nr if n is None else n, g, x.nnz if nnz is None else nnz,
                                            z if k == 0 or "gene_mask" in null else m.ptr(d_bits),
                                            k if n_masks is None else n_masks, p("row_nnz"), p("row_total"), p("row_masked", k > 0),
                                            p("col_nnz", per_gene), p("col_sum", per_gene), p("flags"), m.stream)
        m.sync()
        res = {name: m.get(a) for name, a in out.items()}
        res["row_nnz"], res["row_total"] = res["row_nnz"][:nr], res["row_total"][:nr]
        res["row_masked"] = res["row_masked"][:k, :nr]
        return rc, res

    def top(self, x, positions, *, n=None, nnz=None, n_positions=None, null=()):
        """-> (rc, top float64 [rows of x, len(positions)], prefilled with NaN)"""
        m = self.mem
        keep, (ip, _, dv) = self._in(x, null)
        nr = x.shape[0]
        pos = (C.c_int32 * max(len(positions), 1))(*(int(v) for v in positions))
        out = m.full((max(nr, 1), max(len(positions), 1)), np.float64, np.nan)
        z = C.c_void_p(0)
        rc = self.lib.scamd_pp_qc_top_f32(ip, dv, nr if n is None else n, x.nnz if nnz is None else nnz,
                                          z if "positions" in null else C.cast(pos, C.c_void_p),
                                          len(positions) if n_positions is None else n_positions,
                                          z if "top" in null else m.ptr(out), m.stream)
        m.sync()
        return rc, m.get(out)[:nr]


# ---------------------------------------------------------------------------------------------------------------------
# Checkers.  Integer-valued data: every primitive equals the restatement exactly.  Other data: each float64 sum lies within
# L * 2^-52 * sum|x| of the (exactly rounded) restatement, L and the sum taken over the entries involved -- the bound of
# recursive summation, L * 2^-53 * sum|x|, doubled; derived, not measured.
# ---------------------------------------------------------------------------------------------------------------------
def _close(got, want, count, sabs, exact, what):
    if exact:
        assert np.array_equal(got, want), (what, np.flatnonzero(np.ravel(got != want))[:8])
    else:
        err, tol = np.abs(got - want), count * U * sabs
        assert np.all(err <= tol), (what, float((err - tol).max()))


def check_sweep(qabi, x, masks, g_pass=None, label="", rerun=True, rows_only=True):
    ref = ref_sweep(x, masks, g_pass)
    exact = integer_valued(x)
    rc, out = qabi.sweep(x, masks, g=g_pass)
    assert rc == 0, (label, rc)
    g_out = x.shape[1] if g_pass is None else g_pass
    assert np.array_equal(out["row_nnz"], ref["row_nnz"]), label
    _close(out["row_total"], ref["row_total"], ref["row_nnz"], ref["row_abs"], exact, f"{label} row_total")
    _close(out["row_masked"], ref["row_masked"], ref["masked_nnz"], ref["masked_abs"], exact, f"{label} row_masked")
    assert np.array_equal(out["col_nnz"][:g_out], ref["col_nnz"]), label
    _close(out["col_sum"][:g_out], ref["col_sum"], ref["col_nnz"], ref["col_abs"], exact, f"{label} col_sum")
    assert int(out["flags"][0]) == int(ref["negative"]), (label, out["flags"])
    # a mask that selects no gene: exactly 0; one that selects all: the row total, bit for bit (the same lane order)
    for j in range(len(masks)):
        if not masks[j].any():
            assert np.all(out["row_masked"][j] == 0) and not np.signbit(out["row_masked"][j]).any(), label
        if masks[j].all():
            assert np.array_equal(out["row_masked"][j], out["row_total"]), label
    # columns nothing hits stay exactly 0, beyond the matrix too
    assert np.all(out["col_sum"][:g_out][ref["col_nnz"] == 0] == 0) and np.all(out["col_nnz"][:g_out][ref["col_nnz"] == 0] == 0)
    if rerun:
        rc2, again = qabi.sweep(x, masks, g=g_pass)
        assert rc2 == 0
        names = out if exact else ("row_nnz", "row_total", "row_masked", "col_nnz", "flags")  # (float64 atomics elsewhere)
        for name in names:
            assert out[name].tobytes() == again[name].tobytes(), (label, name)
    # the row primitives without the per-gene outputs and without `indices` (no mask): the third variant of the kernel
    if rows_only:
        rc3, rows = qabi.sweep(x, None, per_gene=False, null=("indices",))
        assert rc3 == 0 and rows["row_total"].tobytes() == out["row_total"].tobytes(), label
        assert np.array_equal(rows["row_nnz"], out["row_nnz"]) and np.isnan(rows["col_sum"]).all(), label
    return out


def check_top(qabi, x, positions, label="", kind=None, rerun=True):
    want, sabs = ref_top(x, positions)
    exact = integer_valued(x)
    rc, got = qabi.top(x, positions)
    assert rc == 0, (label, rc)
    assert not np.isnan(got).any(), (label, "rows not written", np.flatnonzero(np.isnan(got).any(axis=1))[:8])
    _close(got, want, np.asarray(positions, dtype=np.float64)[None, :], sabs, exact, f"{label} top")
    if kind == "ones":   # top(n) / total = n / len
        ln = np.diff(x.indptr)
        assert np.array_equal(got, np.minimum(np.asarray(positions)[None, :], ln[:, None]).astype(np.float64)), label
    if rerun:
        rc2, again = qabi.top(x, positions)
        assert rc2 == 0 and got.tobytes() == again.tobytes(), (label, "two runs differ")
    return got


def run_top_case(qabi, name: str, label=""):
    """the sweep (LDS and global per-gene table) and the top-n pass on the matrix of one case"""
    _, g, positions, _, kind, _ = _case(name)
    x, masks = case_matrix(name), case_masks(name)
    check_sweep(qabi, x, masks, None, f"{label} {name}")
    if col_table(g) == "lds":
        check_sweep(qabi, x, masks, QC_LDS_GENES + GLOBAL_G_EXTRA, f"{label} {name} global table", rerun=False)
    got = check_top(qabi, x, positions, f"{label} {name}", kind)
    if kind == "extreme":
        rows = np.flatnonzero(np.diff(x.indptr) >= 13)[:2]
        # the largest value first, whatever the signs and exponents of the others
        assert got[rows[0], 0] == np.float64(np.float32(3e38)) and got[rows[1], 0] == np.float64(np.float32(1e-30)), label
    return got


def run_col_table_case(qabi, g: int, label=""):
    x = col_table_matrix(g)
    out = check_sweep(qabi, x, make_masks(1, g, seed=g), None, f"{label} g={g}")
    hit = np.diff(x.indptr) > 0
    stored = np.bincount(x.indices, minlength=g)
    assert stored[HOT_COLUMN] == hit.sum() and out["col_nnz"][HOT_COLUMN] <= hit.sum()
    if g > 3:
        assert out["col_sum"][g // 3] == 0 and out["col_sum"][g - 1] == 0 and out["col_nnz"][g - 1] == 0


GRID_CAP_PARTS = ("lds", "global", "top")


def run_grid_cap_case(qabi, part: str, label=""):
    """one launch per part: the sweep with the LDS table, with the global table, the top-n pass"""
    x = grid_cap_matrix()
    if part == "lds":
        check_sweep(qabi, x, make_masks(1, GRID_CAP_G, seed=1), None, f"{label} lds", rerun=False, rows_only=False)
    elif part == "global":
        check_sweep(qabi, x, make_masks(1, GRID_CAP_G, seed=1), QC_LDS_GENES + GLOBAL_G_EXTRA, f"{label} global", rerun=False,
                    rows_only=False)
    else:
        head = x[:GRID_CAP_TOP_ROWS]
        assert top_threads(head.nnz, head.shape[0], 3) == 64
        check_top(qabi, head, (1, 3), f"{label} top", rerun=False)


def run_argument_checks(qabi, launches=None):
    """the documented codes; a rejected call starts no kernel and writes no output"""
    x = sparse.random(20, 64, density=0.2, format="csr", dtype=np.float32, random_state=3)
    x.data = np.ceil(10 * x.data).astype(np.float32)
    masks = make_masks(3, 64)
    before = launches() if launches else 0

    def untouched(out):
        for name, a in out.items():
            assert np.isnan(a).all() if a.dtype.kind == "f" else (a == -1).all(), name

    for kw, code in ((dict(null=("indptr",)), EINVAL), (dict(n=-1), EINVAL), (dict(g=-1), EINVAL), (dict(nnz=-1), EINVAL),
                     (dict(g=1 << 31), EINVAL), (dict(null=("data",)), EINVAL), (dict(null=("row_nnz",)), EINVAL),
                     (dict(null=("row_total",)), EINVAL), (dict(null=("flags",)), EINVAL), (dict(null=("col_sum",)), EINVAL),
                     (dict(null=("col_nnz",)), EINVAL), (dict(null=("indices",)), EINVAL), (dict(null=("gene_mask",)), EINVAL),
                     (dict(null=("row_masked",)), EINVAL), (dict(n_masks=-1), EINVAL), (dict(n_masks=33), EUNSUPPORTED)):
        rc, out = qabi.sweep(x, masks, **kw)
        assert rc == code, (kw, rc)
        untouched(out)
    for positions, kw, code in (((5, 3), {}, EINVAL), ((3, 3), {}, EINVAL), ((0, 3), {}, EINVAL), ((-2,), {}, EINVAL),
                                ((1, 2), dict(null=("indptr",)), EINVAL), ((1, 2), dict(null=("data",)), EINVAL),
                                ((1, 2), dict(null=("positions",)), EINVAL), ((1, 2), dict(null=("top",)), EINVAL),
                                ((1, 2), dict(n=-1), EINVAL), ((1, 2), dict(nnz=-1), EINVAL), ((1, 2), dict(n_positions=0), EINVAL),
                                (tuple(range(1, 18)), {}, EUNSUPPORTED), ((QC_MAX_TOP + 1,), {}, EUNSUPPORTED)):
        rc, top = qabi.top(x, positions, **kw)
        assert rc == code, (positions, kw, rc)
        assert np.isnan(top).all(), (positions, kw)
    if launches:
        assert launches() == before, "an argument check let a kernel start"
    # n = 0: OK; the per-gene outputs and the flag word are zeroed, nothing else is written.  g = 0 (an empty pattern): OK
    rc, out = qabi.sweep(x, masks, n=0)
    assert rc == 0 and (out["row_nnz"] == -1).all() and np.isnan(out["row_total"]).all() and np.isnan(out["row_masked"]).all()
    assert (out["col_nnz"] == 0).all() and (out["col_sum"] == 0).all() and out["flags"][0] == 0
    rc, out = qabi.sweep(x, masks, n=0, g=0)
    assert rc == 0 and (out["col_nnz"] == -1).all()
    rc, top = qabi.top(x, (1, 2), n=0)
    assert rc == 0 and np.isnan(top).all()
    empty = sparse.csr_matrix((7, 0), dtype=np.float32)
    rc, out = qabi.sweep(empty, None, g=0)
    assert rc == 0 and (out["row_nnz"] == 0).all() and (out["row_total"] == 0).all() and out["flags"][0] == 0
    rc, top = qabi.top(empty, (1, 2))
    assert rc == 0 and (top == 0).all()
    if launches:
        assert launches() == before + 2, "n = 0 must not start a kernel; the empty pattern starts one per entry point"


# ---------------------------------------------------------------------------------------------------------------------
# CPU stand-in for GpuPPBackend.qc_sweep (the front-end tests): the restated primitives
# ---------------------------------------------------------------------------------------------------------------------
class CpuStubQcBackend(CpuStubPPBackend):
    def qc_sweep(self, m, *, gene_masks=None, positions=(), per_gene=True):
        x = sparse.csr_matrix((m.data, m.indices, m.indptr), shape=m.shape)
        masks = np.zeros((0, m.shape[1]), dtype=bool) if gene_masks is None else np.asarray(gene_masks, dtype=bool)
        r = ref_sweep(x, masks)
        return {"row_nnz": r["row_nnz"], "row_total": r["row_total"], "row_masked": r["row_masked"],
                "col_nnz": r["col_nnz"] if per_gene else None, "col_sum": r["col_sum"] if per_gene else None,
                "negative": r["negative"], "top": ref_top(x, list(positions))[0] if len(positions) else None}
