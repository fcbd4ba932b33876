"""TEST INFRASTRUCTURE shared by tests/test_gpu_preprocess_shapes.py and tests/test_gpu_umap_shapes.py (the product library on
the GPU) and tests/test_emu_pp_umap_shapes_cpu.py (the same kernels on the host emulator): the shape tables of the normalisation
chain (csrc/preprocess.hip: row sums, positive counts, highly-expressed counts, row divide, log1p, column statistics with and
without clipping, CSR and dense scaling) and of the UMAP layout optimiser (csrc/umap.hip), restatements of the rules by which
the host code picks a kernel instantiation and a grid, input builders, and ONE checker per operation against a float64
reference.  Nothing here touches a device; the callers are tests/emu/harness.py:Abi over host or device memory."""
from __future__ import annotations

import re
from functools import lru_cache
from pathlib import Path

import numpy as np
from scipy import sparse

from graph_kernel_cases import EINVAL, EUNSUPPORTED, EWORKSPACE, DeviceMem  # noqa: F401  (DeviceMem: for the GPU tests)
from oracle import preprocess as op
from oracle import umap as ou

CSRC = Path(__file__).resolve().parent.parent / "scanpy_amd" / "csrc"

# ---------------------------------------------------------------------------------------------------------------------
# The dispatch rules restated (the library has no getter of what it launched); `assert_sources_still_say_so` ties them to
# the text of the two .hip files.
# ---------------------------------------------------------------------------------------------------------------------
PP_BLOCK = 256
PP_LDS_GENES = 4096            # column tables up to this many genes live in LDS
PP_G = (8, 16, 32, 64)         # lanes per row
PP_GROUP_GRID_CAP = 256 * 32   # group_grid: blocks of a row-wise kernel
PP_COLSTATS_LDS_BLOCKS = 512   # launch_col_stats, LDS variant: 16 rows per lane group and launch, at most this many blocks
PP_COLSTATS_LDS_ROWS = 16
PP_LOG1P_GRID_CAP = 256 * 32
PP_DENSE_FILL_GRID_CAP = 256 * 64
PP_ROW_KERNELS = ("row_sums", "row_npos", "count_high", "row_divide", "col_stats", "col_stats_clip", "scale_csr", "scale_dense_scatter")
UM_BLOCK, UM_MAXD, UM_NB = 256, 8, 6
UM_G = (4, 8, 16, 32)
UM_GRID_CAP = 256 * 32
UM_DIM_INST = (2, 3, 0)        # umap_epoch_kernel<G, DIM>: 2 and 3 at compile time, 0 = the run-time dimension


def pp_lanes(nnz: int, n: int) -> int:
    """lanes_per_row: G from the mean row length (integer division)"""
    avg = nnz // n if n > 0 else 0
    return 8 if avg <= 32 else (16 if avg <= 160 else (32 if avg <= 512 else 64))


def col_table(g: int) -> str:
    """launch_col_stats: where the per-gene table lives"""
    return "lds" if g <= PP_LDS_GENES else "global"


def col_table_lds_bytes(g: int) -> int:
    return g * (8 + 8 + 4) + 16


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def group_grid(n: int, G: int, capped: bool = True) -> int:
    blocks = max(_cdiv(n, PP_BLOCK // G), 1)
    return min(blocks, PP_GROUP_GRID_CAP) if capped else blocks


def col_stats_lds_grid(n: int, G: int, capped: bool = True) -> int:
    blocks = max(_cdiv(n, (PP_BLOCK // G) * PP_COLSTATS_LDS_ROWS), 1)
    return min(blocks, PP_COLSTATS_LDS_BLOCKS) if capped else blocks


def log1p_grid(count: int, capped: bool = True) -> int:
    blocks = max(_cdiv(count // 4 + 8, PP_BLOCK), 1)
    return min(blocks, PP_LOG1P_GRID_CAP) if capped else blocks


def dense_fill_grid(n: int, g: int, capped: bool = True) -> int:
    blocks = _cdiv(n * g, PP_BLOCK)
    return min(blocks, PP_DENSE_FILL_GRID_CAP) if capped else blocks


def umap_lanes(nnz: int, n: int) -> int:
    avg = nnz // n
    return 4 if avg <= 12 else (8 if avg <= 24 else (16 if avg <= 96 else 32))


def umap_dim_inst(dim: int) -> int:
    return dim if dim in (2, 3) else 0


def umap_grid(n: int, G: int, capped: bool = True) -> int:
    blocks = max(_cdiv(n, UM_BLOCK // G), 1)
    return min(blocks, UM_GRID_CAP) if capped else blocks


def assert_sources_still_say_so():
    """the constants and thresholds above, read out of the text of csrc/preprocess.hip and csrc/umap.hip"""
    pp, um = (CSRC / "preprocess.hip").read_text(), (CSRC / "umap.hip").read_text()

    def has(text, pattern, what):
        assert re.search(pattern, text), f"{what}: /{pattern}/ no longer in the source -- restate the rule and its cases"

    has(pp, rf"constexpr int PP_BLOCK = {PP_BLOCK};", "PP_BLOCK")
    has(pp, rf"constexpr int PP_LDS_GENES = {PP_LDS_GENES};", "PP_LDS_GENES")
    has(pp, r"return avg <= 32 \? 8 : \(avg <= 160 \? 16 : \(avg <= 512 \? 32 : 64\)\);", "lanes_per_row")
    has(pp, r"const int64_t avg = n > 0 \? nnz_hint / n : 0;", "lanes_per_row: mean row length")
    assert PP_GROUP_GRID_CAP == 256 * 32 == PP_LOG1P_GRID_CAP and PP_DENSE_FILL_GRID_CAP == 256 * 64
    has(pp, r"std::max<int64_t>\(ceil_div\(n, PP_BLOCK / G\), 1\), 256 \* 32\)", "group_grid")
    has(pp, r"if \(g <= PP_LDS_GENES\) \{", "column-table split")
    has(pp, r"const size_t lds = \(size_t\)g \* \(8 \+ 8 \+ 4\) \+ 16;", "column-table LDS bytes")
    has(pp, rf"ceil_div\(n, \(PP_BLOCK / G\) \* {PP_COLSTATS_LDS_ROWS}\), 1\), {PP_COLSTATS_LDS_BLOCKS}\)", "col_stats LDS grid")
    has(pp, r"ceil_div\(count / 4 \+ 8, PP_BLOCK\), 1\), 256 \* 32\)", "log1p grid")
    has(pp, r"std::min<int64_t>\(ceil_div\(n \* \(int64_t\)g, PP_BLOCK\), 256 \* 64\)", "dense fill grid")
    has(pp, r"for \(int o = G / 2; o > 0; o >>= 1\) v \+= __shfl_xor\(v, o\);", "group_sum")
    assert len(re.findall(r"#pragma unroll 4\n", pp)) == 5, "the rows of 4 G - 1, 4 G, 4 G + 1 entries are there for `unroll 4`"
    for G in PP_G[:-1]:
        has(pp, rf"case {G}: hipLaunchKernelGGL\(\(KERNEL<{G}>\)", f"PP_DISPATCH_G {G}")
    has(pp, r"default: hipLaunchKernelGGL\(\(KERNEL<64>\)", "PP_DISPATCH_G 64")
    has(pp, r"\(16 - \(reinterpret_cast<uintptr_t>\(data\) & 15\)\) & 15\) / 4", "log1p head")
    has(um, rf"constexpr int UM_BLOCK = {UM_BLOCK};", "UM_BLOCK")
    has(um, rf"constexpr int UM_MAXD = {UM_MAXD};", "UM_MAXD")
    has(um, rf"constexpr int NB = {UM_NB};", "negative batch")
    has(um, r"const int G = avg <= 12 \? 4 : \(avg <= 24 \? 8 : \(avg <= 96 \? 16 : 32\)\);", "umap lanes per vertex")
    has(um, r"std::max<int64_t>\(ceil_div\(n, UM_BLOCK / G\), 1\), 256 \* 32\)", "umap grid")
    has(um, r"if \(dim == 2\)\s+hipLaunchKernelGGL\(\(umap_epoch_kernel<G, 2>\)", "umap DIM = 2")
    has(um, r"else if \(dim == 3\)\s+hipLaunchKernelGGL\(\(umap_epoch_kernel<G, 3>\)", "umap DIM = 3")
    has(um, r"else\s+hipLaunchKernelGGL\(\(umap_epoch_kernel<G, 0>\)", "umap run-time DIM")
    has(um, r"dim >= 1 && dim <= UM_MAXD, SCAMD_EUNSUPPORTED", "umap dim range")


# ---------------------------------------------------------------------------------------------------------------------
# preprocess tables
# ---------------------------------------------------------------------------------------------------------------------
PP_ROW_G = 2100                 # columns of the row-wise cases (the LDS column table); the same matrices run the global table
PP_GLOBAL_G = PP_LDS_GENES + 104  # ... by passing this g: the columns beyond the matrix receive nothing
# (rows, stored entries per row as nnz // n): both sides of 32 | 33, 160 | 161, 512 | 513
PP_ROW_CASES = ((307, 32), (307, 33), (309, 160), (309, 161), (311, 512), (601, 513))
PP_COL_TABLE_G = (3276, 3277, 4095, 4096, 4097)
PP_COL_TABLE_ROWS, PP_COL_TABLE_AVG = 403, 40
PP_GRID_CAP_ROWS, PP_GRID_CAP_G = PP_GROUP_GRID_CAP * 32 + 40, 64   # G = 8: 32 rows per block
PP_LOG1P_COUNTS = tuple(range(10)) + tuple(range(255, 261)) + tuple(1024 + i for i in range(4))
PP_LOG1P_OFFSETS = (0, 1, 2, 3)
PP_LOG1P_BASES = (None, 2.0, 10.0)
PP_LOG1P_GRID_CAP_COUNT = PP_LOG1P_GRID_CAP * PP_BLOCK * 4 + 5
PP_DENSE_CAP_SHAPE = (1100, 4000)  # n g just past the fill kernel's 256 * 64 blocks of 256 elements
PP_DENSE_OUT_F64 = (True, False)  # scamd_pp_scale_dense_f32's out_is_f64: what a sparse and a dense float32 adata.X take
HOT_COLUMN = 7                   # in every non-empty row: every lane group of a block adds to the same table entry


def special_row_lengths(G: int, avg: int):
    """0 (the empty rows), the ends of a lane group's strides and of the `unroll 4` body, one row several times the mean"""
    return [1, G - 1, G, G + 1, 4 * G - 1, 4 * G, 4 * G + 1, 3 * avg]


@lru_cache(maxsize=None)
def pp_row_lengths(n: int, avg: int, seed: int = 0):
    """-> (lengths [n] with sum // n == avg, index of the row whose stored values are all zero).  Rows 0, n // 2 and n - 1
    are empty."""
    rng = np.random.default_rng(1000 * avg + n + seed)
    G = pp_lanes(avg * n, n)
    special = special_row_lengths(G, avg) + [avg]  # (the last one: the all-zero row)
    empties = (0, n // 2, n - 1)
    total = avg * n + n // 2
    m = n - len(special) - len(empties)
    rem = total - sum(special)
    assert m > 2 and rem > 0
    fill = np.full(m, rem // m, dtype=np.int64)
    fill[: rem % m] += 1
    d = rng.integers(0, rem // m // 2 + 1, m // 2)
    fill[0:2 * (m // 2):2] += d
    fill[1:2 * (m // 2):2] -= d
    body = np.concatenate([special, fill])
    perm = rng.permutation(len(body))
    body = body[perm]
    zero_pos = int(np.flatnonzero(perm == len(special) - 1)[0])
    lengths = np.zeros(n, dtype=np.int64)
    slots = np.setdiff1d(np.arange(n), empties)
    lengths[slots] = body
    assert lengths.sum() == total and total // n == avg and (lengths >= 0).all() and (lengths[list(empties)] == 0).all()
    assert set(special_row_lengths(G, avg)) | {0} <= set(lengths.tolist())
    return lengths, int(slots[zero_pos])


@lru_cache(maxsize=None)
def pp_matrix(n: int, g: int, avg: int) -> sparse.csr_matrix:
    """integer-valued float32 counts (5 % of them stored zeros), unique ascending columns, HOT_COLUMN in every non-empty row,
    columns 0, g // 3 and g - 1 in none; cached and read-only: one input per case for every test"""
    lengths, zero_row = pp_row_lengths(n, avg)
    rng = np.random.default_rng(7 * n + g + avg)
    allowed = np.setdiff1d(np.arange(g), [0, g // 3, g - 1, HOT_COLUMN])
    assert lengths.max() - 1 <= len(allowed)
    cols = [np.sort(np.concatenate([[HOT_COLUMN], rng.choice(allowed, size=ln - 1, replace=False)])) for ln in lengths if ln]
    indices = np.concatenate(cols).astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    data = np.minimum(np.ceil(rng.lognormal(0.5, 1.0, size=len(indices))), 60.0).astype(np.float32)
    data[rng.random(len(data)) < 0.05] = 0.0
    data[indptr[zero_row]: indptr[zero_row + 1]] = 0.0
    x = sparse.csr_matrix((data, indices, indptr), shape=(n, g))
    assert x.has_sorted_indices and x.nnz == lengths.sum()
    for a in (x.data, x.indices, x.indptr):
        a.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def pp_grid_cap_matrix() -> sparse.csr_matrix:
    """PP_GRID_CAP_ROWS rows of 0 or 2..6 entries over 64 columns: G = 8, one block more than group_grid allows, and one more
    than the LDS column-statistics launch allows"""
    n, g = PP_GRID_CAP_ROWS, PP_GRID_CAP_G
    rng = np.random.default_rng(8192)
    ln = rng.integers(1, 7, n)
    ln[ln == 1] = 0  # 0 or 2..6 entries
    ln[[0, n // 2, n - 1]] = 0
    used = g - 3  # 61, a prime: start + j * stride are distinct columns mod 61; columns 61..63 receive nothing
    start, stride = rng.integers(0, used, n), rng.integers(1, used, n)
    c = (start[:, None] + np.arange(6)[None, :] * stride[:, None]) % used
    keep = np.arange(6)[None, :] < ln[:, None]
    c = np.sort(np.where(keep, c, g + 1), axis=1)
    indices = c[c < g].astype(np.int32)
    indptr = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    # columns 0..7 hold large counts, the others 1..3: at max_fraction = 0.8 only the former are ever highly expressed
    data = np.where(indices < 8, rng.integers(40, 61, len(indices)), rng.integers(1, 4, len(indices))).astype(np.float32)
    x = sparse.csr_matrix((data, indices, indptr), shape=(n, g))
    assert x.nnz < 1_000_000 and pp_lanes(x.nnz, n) == 8
    for a in (x.data, x.indices, x.indptr):
        a.setflags(write=False)
    return x


def assert_every_preprocess_path_has_a_case():
    """-> the set of (kernel, G) the row-wise table reaches"""
    reached = set()
    for n, avg in PP_ROW_CASES:
        lengths, _ = pp_row_lengths(n, avg)
        G = pp_lanes(int(lengths.sum()), n)
        assert G == pp_lanes(avg * n, n) == pp_lanes(avg * n + n - 1, n)
        reached |= {(k, G) for k in PP_ROW_KERNELS}
        # both column-table variants and both output dtypes run on every one of these matrices (run_pp_row_case)
        assert col_table(PP_ROW_G) == "lds" and col_table(PP_GLOBAL_G) == "global" and set(PP_DENSE_OUT_F64) == {True, False}
        assert lengths.max() >= 3 * avg and (lengths == 0).sum() >= 3
    assert reached == {(k, G) for k in PP_ROW_KERNELS for G in PP_G}, reached
    avgs = {avg for _, avg in PP_ROW_CASES}
    assert {32, 33, 160, 161, 512, 513} <= avgs
    assert [pp_lanes(a * 300, 300) for a in (32, 33, 160, 161, 512, 513)] == [8, 16, 16, 32, 32, 64]
    n64 = [n for n, avg in PP_ROW_CASES if pp_lanes(avg * n, n) == 64]
    assert n64 and max(n64) <= 610
    # column table: both sides of the split, both sides of 64 KB of LDS
    assert {col_table(g) for g in PP_COL_TABLE_G} == {"lds", "global"} and {PP_LDS_GENES, PP_LDS_GENES + 1} <= set(PP_COL_TABLE_G)
    lds = [col_table_lds_bytes(g) for g in PP_COL_TABLE_G if col_table(g) == "lds"]
    assert min(lds) <= 64 * 1024 < sorted(lds)[1] and max(lds) == 81936
    assert col_table_lds_bytes(3276) == 65536 and col_table_lds_bytes(3277) == 65556
    # grid caps: one block beyond each
    n = PP_GRID_CAP_ROWS
    assert group_grid(n, 8, capped=False) == PP_GROUP_GRID_CAP + 2 > group_grid(n, 8)
    assert col_stats_lds_grid(n, 8, capped=False) == PP_COLSTATS_LDS_BLOCKS + 1 > col_stats_lds_grid(n, 8)
    assert log1p_grid(PP_LOG1P_GRID_CAP_COUNT, capped=False) == PP_LOG1P_GRID_CAP + 1
    assert dense_fill_grid(*PP_DENSE_CAP_SHAPE, capped=False) > PP_DENSE_FILL_GRID_CAP
    assert group_grid(max(n for n, _ in PP_ROW_CASES), 64) < PP_GROUP_GRID_CAP  # (the emulator's cases stay below the caps)
    assert set(range(10)) <= set(PP_LOG1P_COUNTS) and set(PP_LOG1P_OFFSETS) == {0, 1, 2, 3}
    return reached


# ---------------------------------------------------------------------------------------------------------------------
# preprocess checkers
# ---------------------------------------------------------------------------------------------------------------------
DIVIDE_RTOL = 2.0 ** -24 * (1 + 2.0 ** -20)  # one correctly rounded float32 division of the float64 quotient
SCALE_CSR_RTOL, SCALE_DENSE_TOL = 1e-6, 1e-12  # tests/test_gpu_preprocess.py
COLSTAT_RTOL, COLSTAT_ATOL, COLSTAT_CLIP_ATOL = 1e-12, 1e-12, 1e-9
EXPM1_SUM_RTOL, EXPM1_SQ_RTOL = 5e-6, 1e-5
LOG1P_RTOL, LOG1P_ATOL = 2e-6, 1e-7
MAX_FRACTION = 0.05


def _rows(x):
    return np.repeat(np.arange(x.shape[0]), np.diff(x.indptr))


def _row_mask(n: int) -> np.ndarray:
    return (np.arange(n) % 3 != 0).astype(np.uint8)


def check_row_sums_chain(abi, x, label="", max_fraction=MAX_FRACTION):
    """row sums, the highly-expressed counts from them, and the row sums that skip the columns so found: all exact"""
    n, g = x.shape
    rows, d64 = _rows(x), x.data.astype(np.float64)
    rc, sums = abi.pp_row_sums(x)
    assert rc == 0, (label, rc)
    ref = np.bincount(rows, weights=d64, minlength=n).astype(np.float32)
    assert np.array_equal(sums, ref), f"{label}: row sums differ in rows {np.flatnonzero(sums != ref)[:8].tolist()}"
    rc, hi = abi.pp_count_high(x, sums, max_fraction)
    assert rc == 0, (label, rc)
    ref_hi = np.bincount(x.indices[x.data > np.float32(max_fraction) * sums[rows]], minlength=g)
    assert np.array_equal(hi, ref_hi), f"{label}: count_high differs in columns {np.flatnonzero(hi != ref_hi)[:8].tolist()}"
    assert hi.any() and (hi == 0).any()
    rc, sums2 = abi.pp_row_sums(x, col_skip=hi)
    assert rc == 0, (label, rc)
    keep = hi[x.indices] == 0
    ref2 = np.bincount(rows[keep], weights=d64[keep], minlength=n).astype(np.float32)
    assert np.array_equal(sums2, ref2), f"{label}: row sums with col_skip differ in rows {np.flatnonzero(sums2 != ref2)[:8].tolist()}"
    assert not np.array_equal(ref, ref2)
    return sums


def check_row_count_positive(abi, x, label=""):
    d = x.data.copy()
    d[::7] = -d[::7]  # `> 0`, not `!= 0`
    x2 = sparse.csr_matrix((d, x.indices, x.indptr), shape=x.shape)
    rc, cnt = abi.pp_row_count_positive(x2)
    assert rc == 0, (label, rc)
    ref = np.bincount(_rows(x)[d > 0], minlength=x.shape[0])
    assert np.array_equal(cnt, ref), f"{label}: positive counts differ in rows {np.flatnonzero(cnt != ref)[:8].tolist()}"


def check_row_divide(abi, x, sums, label=""):
    factor = (sums / np.float32(100.0)).astype(np.float32)
    assert (factor == 0).any()  # empty rows and the all-zero row: divided by 1
    rc, got = abi.pp_row_divide(x, factor)
    assert rc == 0, (label, rc)
    f = np.where(factor == 0, np.float32(1), factor).astype(np.float64)
    q = x.data.astype(np.float64) / f[_rows(x)]
    err = np.abs(got.astype(np.float64) - q)
    assert (err <= DIVIDE_RTOL * np.abs(q)).all(), f"{label}: row divide beyond one float32 rounding at {np.flatnonzero(err > DIVIDE_RTOL * np.abs(q))[:8].tolist()}"


def _log_values(x):
    y = sparse.csr_matrix((np.log1p(x.data).astype(np.float32), x.indices, x.indptr), shape=x.shape)
    return y


def check_col_stats(abi, x, g_pass, mask, transform, label=""):
    """x: integer counts; transform = 1 runs on log1p(x) with tscale = 0.75"""
    tscale = 0.75 if transform else 1.0
    xx = _log_values(x) if transform else x
    rc, s, q, cnt = abi.pp_col_stats(xx, mask, transform, tscale, g=g_pass)
    tag = f"{label} col_stats g={g_pass} ({col_table(g_pass)}) mask={'yes' if mask is not None else 'NULL'} transform={transform}"
    assert rc == 0, (tag, rc, abi.lib.scamd_last_error())
    sel = np.ones(x.nnz, dtype=bool) if mask is None else mask[_rows(x)].astype(bool)
    v32 = xx.data * np.float32(tscale) if transform else xx.data
    v = np.expm1(v32.astype(np.float64)) if transform else v32.astype(np.float64)
    idx = xx.indices[sel]
    ref_s = np.bincount(idx, weights=v[sel], minlength=g_pass)
    ref_q = np.bincount(idx, weights=v[sel] ** 2, minlength=g_pass)
    ref_c = np.bincount(idx[v32[sel] > 0], minlength=g_pass)
    s, q, cnt = s[:g_pass], q[:g_pass], cnt[:g_pass]
    untouched = np.bincount(idx, minlength=g_pass) == 0
    assert untouched.sum() >= 3 and (s[untouched] == 0).all() and (q[untouched] == 0).all() and (cnt[untouched] == 0).all(), f"{tag}: a column without entries is not exactly 0"
    if transform:
        np.testing.assert_allclose(s, ref_s, rtol=EXPM1_SUM_RTOL, err_msg=tag)
        np.testing.assert_allclose(q, ref_q, rtol=EXPM1_SQ_RTOL, err_msg=tag)
    else:
        np.testing.assert_allclose(s, ref_s, rtol=COLSTAT_RTOL, atol=COLSTAT_ATOL, err_msg=tag)
        np.testing.assert_allclose(q, ref_q, rtol=COLSTAT_RTOL, atol=COLSTAT_ATOL, err_msg=tag)
    assert np.array_equal(cnt, ref_c), f"{tag}: npos differs in columns {np.flatnonzero(cnt != ref_c)[:8].tolist()}"


def check_col_stats_clip(abi, x, g_pass, mask, label=""):
    clip = np.random.default_rng(g_pass).uniform(2.0, 30.0, size=g_pass)
    rc, s, q = abi.pp_col_stats_clip(x, clip, mask, g=g_pass)
    tag = f"{label} col_stats_clip g={g_pass} ({col_table(g_pass)}) mask={'yes' if mask is not None else 'NULL'}"
    assert rc == 0, (tag, rc, abi.lib.scamd_last_error())
    sel = np.ones(x.nnz, dtype=bool) if mask is None else mask[_rows(x)].astype(bool)
    idx = x.indices[sel]
    v = np.minimum(x.data.astype(np.float64)[sel], clip[idx])
    s, q = s[:g_pass], q[:g_pass]
    untouched = np.bincount(idx, minlength=g_pass) == 0
    assert (s[untouched] == 0).all() and (q[untouched] == 0).all(), f"{tag}: a column without entries is not exactly 0"
    np.testing.assert_allclose(s, np.bincount(idx, weights=v, minlength=g_pass), rtol=COLSTAT_RTOL, atol=COLSTAT_CLIP_ATOL, err_msg=tag)
    np.testing.assert_allclose(q, np.bincount(idx, weights=v * v, minlength=g_pass), rtol=COLSTAT_RTOL, atol=COLSTAT_CLIP_ATOL, err_msg=tag)


def _mean_std(x, mask):
    sub = x if mask is None else x[mask.astype(bool)]
    mean, var = op.mean_var(sub)
    std = np.sqrt(var)
    std[std == 0] = 1
    return mean, std


def check_scale_csr(abi, x, label=""):
    for mask, max_value in ((None, None), (_row_mask(x.shape[0]), 1.5)):
        mean, std = _mean_std(x, mask)
        rc, got = abi.pp_scale_csr(x, std, max_value, mask)
        assert rc == 0, (label, rc)
        ref, _, _ = op.scale(x, zero_center=False, max_value=max_value, mask_obs=None if mask is None else mask.astype(bool))
        np.testing.assert_allclose(got, ref.data, rtol=SCALE_CSR_RTOL, err_msg=f"{label} scale_csr mask={'yes' if mask is not None else 'NULL'}")
        if max_value is not None:
            assert got.max() > max_value and (got[mask[_rows(x)].astype(bool)] <= max_value).all()  # a row outside the mask keeps a larger value


def dense_reference_f32(x, mean, std, max_value, mask):
    """numpy's in-place arithmetic on a float32 array: the subtraction is rounded to float32, then the division"""
    d = x.toarray().astype(np.float64)
    z = (d - mean[None, :]).astype(np.float32).astype(np.float64) / std[None, :]
    if max_value is not None:
        z = np.clip(z, -max_value, max_value)
    ref = z.astype(np.float32)
    if mask is not None:
        off = ~mask.astype(bool)
        ref[off] = x.toarray()[off]
    return ref


def check_scale_dense(abi, x, label="", dtypes=PP_DENSE_OUT_F64):
    for out_f64 in dtypes:
        for mask, max_value in ((_row_mask(x.shape[0]), 4.0), (None, None)):
            mean, std = _mean_std(x, mask)
            rc, got = abi.pp_scale_dense(x, mean, std, max_value, mask, out_f64)
            tag = f"{label} scale_dense {'float64' if out_f64 else 'float32'} mask={'yes' if mask is not None else 'NULL'}"
            assert rc == 0, (tag, rc)
            assert got.dtype == (np.float64 if out_f64 else np.float32) and np.isfinite(got).all(), f"{tag}: an element was not written"
            if out_f64:
                ref, _, _ = op.scale(x, zero_center=True, max_value=max_value, mask_obs=None if mask is None else mask.astype(bool))
                np.testing.assert_allclose(got, ref, rtol=SCALE_DENSE_TOL, atol=SCALE_DENSE_TOL, err_msg=tag)
            else:
                np.testing.assert_allclose(got, dense_reference_f32(x, mean, std, max_value, mask), rtol=SCALE_CSR_RTOL, atol=0, err_msg=tag)
            if mask is not None:
                off = ~mask.astype(bool)
                assert np.array_equal(got[off], x.toarray()[off].astype(got.dtype)), f"{tag}: a row outside the mask keeps its stored values, 0 elsewhere"
                assert np.abs(got[~off]).max() == max_value


def run_pp_row_case(abi, n: int, avg: int, label=""):
    """the eight row-wise kernels at one G, on one matrix"""
    x = pp_matrix(n, PP_ROW_G, avg)
    tag = f"{label} n={n} nnz/n={avg} G={pp_lanes(x.nnz, n)}"
    sums = check_row_sums_chain(abi, x, tag)
    check_row_count_positive(abi, x, tag)
    check_row_divide(abi, x, sums, tag)
    mask = _row_mask(n)
    for g_pass in (PP_ROW_G, PP_GLOBAL_G):
        check_col_stats(abi, x, g_pass, mask, 0, tag)
        check_col_stats(abi, x, g_pass, None, 1, tag)
        check_col_stats_clip(abi, x, g_pass, mask, tag)
    check_scale_csr(abi, x, tag)
    check_scale_dense(abi, x, tag)


def run_pp_col_table_case(abi, g: int, label=""):
    x = pp_matrix(PP_COL_TABLE_ROWS, g, PP_COL_TABLE_AVG)
    assert np.bincount(x.indices, minlength=g)[HOT_COLUMN] == (np.diff(x.indptr) > 0).sum()  # one column receives every row
    mask = _row_mask(x.shape[0])
    for m in (None, mask):
        for transform in (0, 1):
            check_col_stats(abi, x, g, m, transform, label)
        check_col_stats_clip(abi, x, g, m, label)


def run_pp_grid_cap_case(abi, label=""):
    """every row-wise kernel family takes a second grid-stride trip; the LDS column statistics go past their 512 blocks"""
    x = pp_grid_cap_matrix()
    n = x.shape[0]
    sums = check_row_sums_chain(abi, x, label, max_fraction=0.8)
    check_row_count_positive(abi, x, label)
    check_row_divide(abi, x, sums, label)
    mask = _row_mask(n)
    for g_pass in (PP_GRID_CAP_G, PP_LDS_GENES + 1):
        check_col_stats(abi, x, g_pass, mask, 0, label)
        check_col_stats_clip(abi, x, g_pass, None, label)
    check_scale_csr(abi, x, label)
    check_scale_dense(abi, x, label, dtypes=(False,))


def run_pp_dense_cap_case(abi, label=""):
    n, g = PP_DENSE_CAP_SHAPE
    x = pp_matrix(n, g, 20)
    check_scale_dense(abi, x, label)


def check_log1p(abi, count: int, offset: int, base, label="", pad=7):
    fill = -7.0
    rng = np.random.default_rng(count * 4 + offset)
    v = np.minimum(np.ceil(rng.lognormal(0.5, 1.5, size=count)), 5000.0).astype(np.float32)
    v[::5] = 0.0
    v[1::5] *= np.float32(0.37)
    rc, buf = abi.pp_log1p(v, offset, 0.0 if base is None else base, pad=pad, fill=fill)
    tag = f"{label} log1p count={count} offset={offset} base={base}"
    assert rc == 0, (tag, rc)
    assert (buf[:offset] == fill).all() and (buf[offset + count:] == fill).all() and len(buf) == offset + count + pad, f"{tag}: elements outside the range were touched"
    ref = np.log1p(v.astype(np.float64))
    if base is not None:
        ref = ref / np.log(base)
    np.testing.assert_allclose(buf[offset: offset + count], ref, rtol=LOG1P_RTOL, atol=LOG1P_ATOL, err_msg=tag)


def run_pp_log1p_cases(abi, offset: int, label=""):
    for count in PP_LOG1P_COUNTS:
        for base in PP_LOG1P_BASES:
            check_log1p(abi, count, offset, base, label)


def run_pp_argument_checks(abi, launches=None):
    """the documented codes; none of these calls may start a kernel or write an output"""
    x = sparse.random(20, 64, density=0.2, format="csr", dtype=np.float32, random_state=3)
    x.data = np.ceil(10 * x.data).astype(np.float32)
    n, g = x.shape
    ones_n, ones_g = np.ones(n, np.float32), np.ones(g, np.float64)
    before = launches() if launches else 0
    calls = {
        "row_sums": lambda **kw: abi.pp_row_sums(x, **kw),
        "row_count_positive": lambda **kw: abi.pp_row_count_positive(x, **kw),
        "count_high": lambda **kw: abi.pp_count_high(x, ones_n, 0.05, **kw),
        "row_divide": lambda **kw: abi.pp_row_divide(x, ones_n, **kw),
        "col_stats": lambda **kw: abi.pp_col_stats(x, **kw),
        "col_stats_clip": lambda **kw: abi.pp_col_stats_clip(x, ones_g, **kw),
        "scale_csr": lambda **kw: abi.pp_scale_csr(x, ones_g, **kw),
        "scale_dense": lambda **kw: abi.pp_scale_dense(x, ones_g, ones_g, **kw),
    }
    with_g = ("count_high", "col_stats", "col_stats_clip", "scale_dense")
    for name, call in calls.items():
        assert call(null=("indptr",))[0] == EINVAL, name
        assert call(n=-1)[0] == EINVAL, name
        assert call(nnz=-1)[0] == EINVAL, name
        if name in with_g:
            assert call(g=-1)[0] == EINVAL, name
        if name in ("col_stats", "col_stats_clip", "scale_dense"):
            assert call(g=1 << 31)[0] == EINVAL, name
        # n = 0 (and g = 0): OK, and every output keeps its prefill
        out = call(n=0, g=0) if name in with_g else call(n=0)
        assert out[0] == 0, (name, out[0])
        for a in out[1:]:
            if a is None:
                continue
            if name in ("row_divide", "scale_csr"):
                assert np.array_equal(a, x.data), name
            elif a.dtype.kind == "f":
                assert np.isnan(a).all(), name
            else:
                assert (a == -1).all(), name
    for name in ("col_stats", "scale_dense"):  # g = 0 alone
        out = calls[name](g=0)
        assert out[0] == 0 and np.isnan(out[1]).all(), name
    assert abi.pp_col_stats_clip(x, ones_g, null=("clip",))[0] == EINVAL
    assert abi.pp_col_stats(x, transform=2)[0] == EINVAL
    v = np.arange(8, dtype=np.float32)
    for base in (1.0, -2.0):
        rc, buf = abi.pp_log1p(v, 0, base)
        assert rc == EINVAL and np.array_equal(buf[:8], v), base
    assert abi.pp_log1p(v, 0, count=-1)[0] == EINVAL
    assert abi.pp_log1p(v, 0, null=("data",))[0] == EINVAL
    rc, buf = abi.pp_log1p(v, 1, count=0)
    assert rc == 0 and np.array_equal(buf[1:9], v)
    if launches:
        assert launches() == before, "an argument check let a kernel start"


# ---------------------------------------------------------------------------------------------------------------------
# UMAP tables
# ---------------------------------------------------------------------------------------------------------------------
UMAP_A, UMAP_B = 0.583, 1.334  # find_ab_params(spread=1, min_dist=0.5), scanpy's defaults, to three digits
SMALL_ALPHA = 1e-3
# (n, nnz // n, dim, negative_sample_rate, n_epochs, initial_alpha); nnz // n on both sides of 12 | 13, 24 | 25, 96 | 97
UMAP_CASES = (
    (701, 12, 2, 5, 12, SMALL_ALPHA), (701, 12, 3, 6, 11, SMALL_ALPHA), (701, 12, 1, 7, 12, SMALL_ALPHA),
    (1999, 13, 2, 13, 11, SMALL_ALPHA), (703, 13, 4, 5, 12, SMALL_ALPHA),
    (501, 24, 3, 7, 11, SMALL_ALPHA), (501, 24, 8, 6, 12, SMALL_ALPHA),
    (503, 25, 2, 6, 11, SMALL_ALPHA), (503, 25, 8, 13, 12, SMALL_ALPHA),
    (307, 96, 3, 5, 11, SMALL_ALPHA), (307, 96, 1, 13, 12, SMALL_ALPHA),
    (301, 97, 2, 7, 11, SMALL_ALPHA), (301, 97, 3, 13, 12, SMALL_ALPHA), (301, 97, 4, 6, 11, SMALL_ALPHA),
    # alpha = 1: ulp-level after the one epoch in which a sample can fire.  Epoch 0 never moves anything -- a sample's first
    # firing is at epoch >= epochs_per_sample >= 1 -- so "one epoch of forces" takes n_epochs = 2
    (503, 25, 2, 5, 2, 1.0),
)
UMAP_ONE_EPOCH_CASE = (503, 25, 2, 5, 1, 1.0)   # n_epochs = 1: nothing can fire; y comes back bit-identical through the memcpy
UMAP_GRID_CAP_CASE = (UM_GRID_CAP * 8 + 50, 100, 2, 5, 2, 1.0)  # G = 32: 8 vertices per block
UMAP_BOUND_FACTOR = 4.0  # ~2 ulp of exp2(b log2 x) against powf, and the other summation order (tree over the lanes)


@lru_cache(maxsize=None)
def umap_graph(n: int, avg: int):
    """random symmetric graph, no self loops: vertices 0, n // 2 and n - 1 without edges, vertex 1 of degree 3 G + 1; 30 % of
    the weights are the maximum 1 (epochs_per_sample = 1: fire at every epoch from 1 on), 2 % are stored zeros
    (epochs_per_sample = -1: never fire).  -> (indptr int64, indices int32, weights float64), nnz // n == avg"""
    rng = np.random.default_rng(100 * n + avg)
    G = umap_lanes(avg * n, n)
    total = avg * n + n // 2
    total += total % 2
    m = total // 2
    hub, empties = 1, (0, n // 2, n - 1)
    free = np.setdiff1d(np.arange(n), (hub,) + empties)
    hub_deg = 3 * G + 1
    assert hub_deg < len(free)
    hub_nb = rng.choice(free, size=hub_deg, replace=False)
    need = m - hub_deg
    draws = 3 * need if n < 5000 else need + need // 10  # (few of the n^2 / 2 pairs come twice when n is large)
    u, v = free[rng.integers(0, len(free), draws)], free[rng.integers(0, len(free), draws)]
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    key = (lo.astype(np.int64) * n + hi)[lo != hi]
    key = np.unique(key)
    assert len(key) >= need, "not enough distinct pairs drawn"
    key = key[rng.choice(len(key), size=need, replace=False)]
    lo = np.concatenate([key // n, np.full(hub_deg, hub)])
    hi = np.concatenate([key % n, hub_nb])
    w = np.where(rng.random(m) < 0.3, 1.0, rng.uniform(0.05, 1.0, m)).astype(np.float32).astype(np.float64)
    w[rng.random(m) < 0.02] = 0.0
    rows, cols, ww = np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([w, w])
    order = np.argsort(rows.astype(np.int64) * n + cols)  # (no pair comes twice: no ties)
    rows, cols, ww = rows[order], cols[order], ww[order]
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(np.bincount(rows, minlength=n))
    assert indptr[-1] == total and total // n == avg and umap_lanes(total, n) == G
    assert indptr[hub + 1] - indptr[hub] == hub_deg and all(indptr[e + 1] == indptr[e] for e in empties) and (ww == 0).any()
    indices = cols.astype(np.int32)
    for a in (indptr, indices, ww):
        a.setflags(write=False)
    return indptr, indices, ww


@lru_cache(maxsize=None)
def umap_inputs(n, avg, dim, n_epochs):
    indptr, indices, w = umap_graph(n, avg)
    eps = ou.make_epochs_per_sample(w, max(n_epochs, 1)).astype(np.float32)
    assert (eps[w == 0] == -1).all() and (eps[w > 0] >= 1).all()
    y0 = np.random.default_rng(n + dim).uniform(0, 10, size=(n, dim)).astype(np.float32)
    eps.setflags(write=False)
    y0.setflags(write=False)
    return indptr, indices, eps, y0


def umap_schedule_stats(eps, n_epochs: int, rate: float):
    """the kernel's sample schedule, which does not depend on the embedding, in the same float32 arithmetic
    -> (set of n_neg over all firings, number of firings)"""
    f32 = np.float32
    eps = eps.astype(f32)
    live = eps > 0
    nxt, eps_neg = eps.copy(), eps / f32(rate)
    nneg_next = eps_neg.copy()
    seen, fired = set(), 0
    with np.errstate(invalid="ignore", divide="ignore"):
        for ep in range(n_epochs):
            fire = live & ~(nxt > f32(ep))
            k = ((f32(ep) - nneg_next[fire]) / eps_neg[fire]).astype(np.int32)
            seen |= set(np.unique(k).tolist())
            fired += int(fire.sum())
            nxt[fire] = nxt[fire] + eps[fire]
            nneg_next[fire] = nneg_next[fire] + k.astype(f32) * eps_neg[fire]
    return seen, fired


def last_alpha(n_epochs: int, initial_alpha: float) -> float:
    return float(np.float32(initial_alpha * (1.0 - (n_epochs - 2 if n_epochs > 1 else 0) / n_epochs)))


def error_unit(case, ref64, sabs):
    """per coordinate: alpha 2^-23 sum|term| of the last epoch -- one float32 ulp of every force term that went into the
    coordinate -- plus 2^-24 |y|, the one rounding of the stored float32 coordinate itself, which the float64 reference does
    not make and which is all that is left for a coordinate no sample moved in the last epoch"""
    n, avg, dim, rate, n_epochs, alpha = case
    return last_alpha(n_epochs, alpha) * 2.0 ** -23 * sabs + 2.0 ** -24 * np.abs(ref64)


@lru_cache(maxsize=None)
def umap_reference(case, seed=11):
    """-> (float64 reference, error unit per coordinate, M = the distance of the float32 oracle from the float64 one in that
    unit, worst coordinate).  Computed once per case; both are CPU code of oracle/umap.c, neither is the code under test."""
    n, avg, dim, rate, n_epochs, alpha = case
    indptr, indices, eps, y0 = umap_inputs(n, avg, dim, n_epochs)
    kw = dict(n_epochs=n_epochs, a=UMAP_A, b=UMAP_B, gamma=1.0, initial_alpha=alpha, negative_sample_rate=float(rate), seed=seed)
    ref64, sabs = ou.synchronous_csr_f64(indptr, indices, eps, y0, **kw)
    ref32 = ou.synchronous_csr(indptr, indices, eps, y0, **kw)
    unit = error_unit(case, ref64, sabs)
    assert (unit > 0).all()
    multiple = float((np.abs(ref32.astype(np.float64) - ref64) / unit).max())
    ref64.setflags(write=False)
    unit.setflags(write=False)
    return ref64, unit, multiple


def assert_every_umap_path_has_a_case():
    """-> {(G, DIM instantiation)} of UMAP_CASES; also: every number of negative batches, both parities of n_epochs"""
    reached, batches, nneg = set(), set(), set()
    for n, avg, dim, rate, n_epochs, alpha in UMAP_CASES:
        indptr, indices, eps, _ = umap_inputs(n, avg, dim, n_epochs)
        G = umap_lanes(int(indptr[-1]), n)
        assert 300 <= n <= 2000 and np.diff(indptr).max() >= 3 * G + 1
        reached.add((G, umap_dim_inst(dim)))
        seen, fired = umap_schedule_stats(eps, n_epochs, rate)
        assert fired > n, "a case in which hardly anything fires checks nothing"
        assert min(seen) >= 0
        nneg |= seen
        batches |= {_cdiv(k, UM_NB) for k in seen}
    assert reached == {(G, d) for G in UM_G for d in UM_DIM_INST}, reached
    assert {1, 2, 3} <= batches and {UM_NB, UM_NB + 1} <= nneg, (batches, nneg)  # 6: one full batch; 7: p0 = 6 and five padded slots
    assert {c[1] for c in UMAP_CASES} >= {12, 13, 24, 25, 96, 97}
    assert {c[2] for c in UMAP_CASES} == {1, 2, 3, 4, UM_MAXD} and {c[3] for c in UMAP_CASES} == {5, 6, 7, 13}
    assert {c[4] % 2 for c in UMAP_CASES} == {0, 1}  # odd: the result is copied back from the second buffer
    assert any(c[5] == 1.0 for c in UMAP_CASES) and any(c[5] == SMALL_ALPHA and c[4] == 12 for c in UMAP_CASES)
    n = UMAP_GRID_CAP_CASE[0]
    assert umap_grid(n, 32, capped=False) > UM_GRID_CAP and umap_lanes(UMAP_GRID_CAP_CASE[1] * n, n) == 32
    return reached


def run_umap_case(abi, case, label="", determinism=True):
    """-> (M of the two references, worst error / bound of the kernel)"""
    n, avg, dim, rate, n_epochs, alpha = case
    indptr, indices, eps, y0 = umap_inputs(n, avg, dim, n_epochs)
    ref64, unit, multiple = umap_reference(case)
    kw = dict(n_epochs=n_epochs, a=UMAP_A, b=UMAP_B, gamma=1.0, initial_alpha=alpha, negative_sample_rate=float(rate))
    rc, got = abi.umap_optimize(indptr, indices, eps, y0, seed=11, **kw)
    tag = f"{label} umap n={n} nnz/n={avg} G={umap_lanes(int(indptr[-1]), n)} dim={dim} rate={rate} epochs={n_epochs} alpha={alpha:g}"
    assert rc == 0, (tag, rc)
    assert np.isfinite(got).all(), tag
    moved = float(np.abs(got - y0).max())
    assert moved > (0.5 if alpha == 1.0 else alpha), f"{tag}: it did not move ({moved})"
    lens = np.diff(indptr)
    assert np.array_equal(got[lens == 0], y0[lens == 0]), f"{tag}: a vertex without edges moved"
    bound = UMAP_BOUND_FACTOR * multiple * unit
    err = np.abs(got.astype(np.float64) - ref64)
    ratio = float((err / bound).max())
    print(f"{tag}: float32 oracle = {multiple:.3f} units from the float64 one; kernel: worst error / bound = {ratio:.3f} "
          f"(worst |error| {err.max():.3g}, moved {moved:.3g})")
    assert ratio <= 1.0, f"{tag}: {int((err > bound).sum())} coordinates beyond the bound, first at {np.argwhere(err > bound)[:4].tolist()}"
    if determinism:
        rc2, again = abi.umap_optimize(indptr, indices, eps, y0, seed=11, **kw)
        assert rc2 == 0 and np.array_equal(got.view(np.int32), again.view(np.int32)), f"{tag}: two runs differ"
        rc3, other = abi.umap_optimize(indptr, indices, eps, y0, seed=12, **kw)
        assert rc3 == 0 and not np.array_equal(got, other), f"{tag}: another seed gave the same layout"
    return multiple, ratio


def run_umap_edges(abi, launches=None, label=""):
    """return codes and the inputs at which nothing may move"""
    n, avg, dim, rate, n_epochs, alpha = UMAP_ONE_EPOCH_CASE
    indptr, indices, eps, y0 = umap_inputs(n, avg, dim, n_epochs)
    kw = dict(a=UMAP_A, b=UMAP_B, initial_alpha=1.0, negative_sample_rate=5.0, seed=3)
    bits = y0.view(np.int32)
    before = launches() if launches else 0
    for bad_dim in (0, UM_MAXD + 1):
        assert abi.umap_workspace_bytes(n, len(indices), bad_dim) == 0
        rc, y = abi.umap_optimize(indptr, indices, eps, y0, n_epochs=3, dim=bad_dim, **kw)
        assert rc == EUNSUPPORTED and np.array_equal(y.view(np.int32), bits), bad_dim
    assert abi.umap_workspace_bytes(0, 0, 2) == 0 and abi.umap_workspace_bytes(n, -1, 2) == 0
    assert abi.umap_optimize(indptr, indices, eps, y0, n_epochs=3, null=("indptr",), **kw)[0] == EINVAL
    assert abi.umap_optimize(indptr, indices, eps, y0, n_epochs=3, null=("y",), **kw)[0] == EINVAL
    assert abi.umap_optimize(indptr, indices, eps, y0, n_epochs=-1, **kw)[0] == EINVAL
    assert abi.umap_optimize(indptr, indices, eps, y0, n_epochs=3, **{**kw, "negative_sample_rate": 0.0})[0] == EINVAL
    # the workspace ends on its last buffer, n * dim floats: a size that is a multiple of the 256-byte granule is tight
    n64 = 64
    ip64 = np.minimum(indptr[: n64 + 1], indptr[n64]).astype(np.int64)
    ix64 = (indices[: ip64[-1]] % n64).astype(np.int32)
    assert (n64 * 2 * 4) % 256 == 0
    rc, y = abi.umap_optimize(ip64, ix64, eps[: ip64[-1]], y0[:n64], n_epochs=3, ws_short=1, **kw)
    assert rc == EWORKSPACE and np.array_equal(y.view(np.int32), bits[:n64])
    rc, y = abi.umap_optimize(indptr, indices, eps, y0, n_epochs=0, **kw)
    assert rc == 0 and np.array_equal(y.view(np.int32), bits), "n_epochs = 0 must leave y as it is"
    if launches:
        assert launches() == before, "an argument check, or n_epochs = 0, let a kernel start"
    assert abi.umap_optimize(ip64, ix64, eps[: ip64[-1]], y0[:n64], n_epochs=3, **kw)[0] == 0  # (to its last byte: accepted)
    empty = np.zeros(n + 1, dtype=np.int64)
    rc, y = abi.umap_optimize(empty, np.zeros(0, np.int32), np.zeros(0, np.float32), y0, n_epochs=5, **kw)
    assert rc == 0 and np.array_equal(y.view(np.int32), bits), "nnz = 0 must leave y as it is"
    # one epoch: no sample can fire at epoch 0; the kernel runs, writes the second buffer, and the result is copied back
    rc, y = abi.umap_optimize(indptr, indices, eps, y0, n_epochs=1, **kw)
    assert rc == 0 and np.array_equal(y.view(np.int32), bits), "a sample fired at epoch 0"
    # n = 1: without an entry, and with a self loop (distance 0: no force; its negative samples are the vertex itself)
    one = y0[:1]
    rc, y = abi.umap_optimize(np.zeros(2, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), one, n_epochs=4, **kw)
    assert rc == 0 and np.array_equal(y, one)
    rc, y = abi.umap_optimize(np.array([0, 1], np.int64), np.zeros(1, np.int32), np.ones(1, np.float32), one, n_epochs=4, **kw)
    assert rc == 0 and np.array_equal(y, one)
