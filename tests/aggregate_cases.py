"""TEST INFRASTRUCTURE shared by tests/test_gpu_aggregate.py (the product library on the GPU), tests/test_emu_aggregate_cpu.py (the
same kernels on the host emulator) and tests/test_aggregate_front_cpu.py (the front end on a CPU stand-in): the case table of
the aggregation kernels (csrc/aggregate.hip), restatements of the rules by which the host code sizes its work, an exact numpy
restatement of the five statistics, ONE checker, and a CPU stand-in for `scanpy_amd._get_aggregate.GpuAggregateBackend`.
Nothing here touches a device; the callers hand in `AggregateAbi` over host memory (tests/emu/harness.py:HostMem) or device
memory (graph_kernel_cases.DeviceMem).

The restatement works on the dense float32 array of a case: sums and centred squares in numpy's extended precision (its own
error, n 2^-64 relative, is far below the bounds checked), counts and medians exactly.

Bounds, evaluated here from the inputs and never read from the code under test (include/scanpy_amd.h states them):
    |sum - exact| <= (size 2^-61 + 2^-53) size amax
    |m2 - exact|  <= size^2 D^2 2^-60 + 2^-50 m2 + size ((size 2^-61 + 2^-52) amax)^2
with size the rows of the group, amax the largest |x| of the gene over the rows that take part and D the largest |x - mean| over
the stored non-zero values of the pair.  count_nonzero, count_negative and the median are exact."""
from __future__ import annotations

import ctypes as C
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
from scipy import sparse

from graph_kernel_cases import EINVAL, EUNSUPPORTED, EWORKSPACE, DeviceMem  # noqa: F401  (DeviceMem: for the GPU tests)

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "scanpy_amd" / "csrc"

# ---------------------------------------------------------------------------------------------------------------------
# The sizing rules restated; `assert_sources_still_say_so` ties them to the text of csrc/aggregate.hip and
# `assert_library_agrees` to the library's own answers (scamd_aggregate_part_entries / _lanes_per_row / _tier_bounds).
# ---------------------------------------------------------------------------------------------------------------------
AG_WINDOW, AG_LDS_MIN_RUN, AG_MED_WAVE_MAX, AG_MED_CHUNK = 4096, 512, 64, 4096
AG_PART_MIN, AG_PART_MAX, AG_PART_TARGET = 2048, 32768, 8192
FLAG_NONFINITE, FLAG_CODE, FLAG_ORDER = 1, 2, 4


def part_entries(nnz: int) -> int:
    return min(max(-(-nnz // AG_PART_TARGET), AG_PART_MIN), AG_PART_MAX)


def lanes_per_row(n: int, nnz: int) -> int:
    avg = nnz // n if n > 0 else 0
    return 8 if avg <= 32 else (16 if avg <= 160 else (32 if avg <= 512 else 64))


def assert_sources_still_say_so():
    src = (CSRC / "aggregate.hip").read_text()

    def has(pattern, what):
        assert re.search(pattern, src), f"{what}: /{pattern}/ no longer in csrc/aggregate.hip -- restate the rule and its cases"

    has(r"constexpr int AG_BLOCK = 256;", "AG_BLOCK")
    has(rf"constexpr int AG_WINDOW = {AG_WINDOW};", "AG_WINDOW")
    has(rf"constexpr int AG_PART_MIN = {AG_PART_MIN};", "AG_PART_MIN")
    has(rf"constexpr int AG_PART_MAX = {AG_PART_MAX};", "AG_PART_MAX")
    has(rf"constexpr int AG_PART_TARGET = {AG_PART_TARGET};", "AG_PART_TARGET")
    has(rf"constexpr int AG_LDS_MIN_RUN = {AG_LDS_MIN_RUN};", "AG_LDS_MIN_RUN")
    has(rf"constexpr int AG_MED_WAVE_MAX = {AG_MED_WAVE_MAX};", "AG_MED_WAVE_MAX")
    has(rf"constexpr int AG_MED_CHUNK = {AG_MED_CHUNK};", "AG_MED_CHUNK")
    has(r"const int64_t per = \(nnz \+ AG_PART_TARGET - 1\) / AG_PART_TARGET;", "part rule")
    has(r"std::min<int64_t>\(std::max<int64_t>\(per, AG_PART_MIN\), AG_PART_MAX\)", "part clamp")
    has(r"return avg <= 32 \? 8 : \(avg <= 160 \? 16 : \(avg <= 512 \? 32 : 64\)\);", "lanes per row")
    has(r"const bool lds = run >= AG_LDS_MIN_RUN;", "LDS table or global adds")
    has(r"else if \(pr\.len <= AG_MED_WAVE_MAX\)", "in-wave median tier")
    has(r"const bool staged = pr\.len <= AG_MED_CHUNK;", "staged median tier")
    for mode in (0, 1, 2):
        has(rf"ag_launch_sweep<{mode}>\(", f"sweep mode {mode}")
    # no float atomics, no printf / assert / inline assembly in the kernels
    for m in re.finditer(r"\batomic\w+\(([^;]*);", src):
        assert not re.search(r"\b(float|double)\b", m.group(1)), m.group(0)
    assert not re.search(r"\bprintf\(|\bassert\(|\basm\b", src)


def assert_library_agrees(lib):
    vals = [C.c_int(-1) for _ in range(4)]
    assert lib.scamd_aggregate_tier_bounds(*(C.byref(v) for v in vals)) == 0
    assert [v.value for v in vals] == [AG_WINDOW, AG_LDS_MIN_RUN, AG_MED_WAVE_MAX, AG_MED_CHUNK]
    assert lib.scamd_aggregate_tier_bounds(None, None, None, None) == EINVAL
    for nnz in (0, 1, 6400, AG_PART_MIN * AG_PART_TARGET, AG_PART_MIN * AG_PART_TARGET + 1, AG_PART_MAX * AG_PART_TARGET, 10 ** 11):
        assert lib.scamd_aggregate_part_entries(nnz) == part_entries(nnz), nnz
    for n, nnz in ((0, 0), (10, 320), (10, 330), (10, 1609), (10, 1610), (10, 5129), (10, 5130), (1, 10 ** 6)):
        assert lib.scamd_aggregate_lanes_per_row(n, nnz) == lanes_per_row(n, nnz), (n, nnz)
    assert lib.scamd_aggregate_part_entries(-1) == 0 and lib.scamd_aggregate_lanes_per_row(-1, 0) == 0
    assert lib.scamd_aggregate_workspace_bytes(-1, 1, 1, 0) == 0 and lib.scamd_aggregate_workspace_bytes(3, 1, 1, 4) == 0
    assert lib.scamd_aggregate_workspace_bytes(0, 0, 0, 0) > 0


# ---------------------------------------------------------------------------------------------------------------------
# Case table.  A case is a dense float32 array `vals` [n, g], a pattern `stored` [n, g] (an entry of the CSR where True: a
# stored +-0.0 where vals is 0 there) and codes int32 [n].  Sizes that straddle a rule are derived from the rules above.
# ---------------------------------------------------------------------------------------------------------------------
def _random(rng, n, g, density, scale=3.0):
    vals = (rng.normal(size=(n, g)) * scale).astype(np.float32)
    stored = rng.random((n, g)) < density
    vals[~stored] = 0.0
    return vals, stored


def _codes(rng, n, n_groups, empty=(), single=()):
    """random codes over the groups that are neither `empty` nor `single`; each of `single` gets exactly one row"""
    free = [k for k in range(n_groups) if k not in empty and k not in single]
    codes = rng.choice(free, n).astype(np.int32)
    codes[: len(free)] = free   # every free group is used
    for q, k in enumerate(single):
        codes[len(free) + q] = k
    return rng.permutation(codes).astype(np.int32)


def _build_one_group(rng):
    vals, stored = _random(rng, 300, 7, 0.3)
    return vals, stored, np.zeros(300, np.int32), 1


def _build_identity(rng):
    vals, stored = _random(rng, 200, 13, 0.4)
    return vals, stored, rng.permutation(200).astype(np.int32), 200


def _build_mixed(rng):
    """a group of size 0 (2), of size 1 (4), rows without a group at the start, the end and in runs; empty rows and columns,
    stored +0.0 and -0.0, negatives; column 5 is constant and fully stored within group 3 (a column stored in every row: the
    cases "dense" and "boundary-*")"""
    n, g, n_groups = 1000, 33, 6
    vals, stored = _random(rng, n, g, 0.25, scale=1.0)
    codes = _codes(rng, n, n_groups, empty=(2,), single=(4,))
    codes[:10] = -1
    codes[-7:] = -1
    codes[400:430] = -1
    codes[700:702] = -1
    codes[np.flatnonzero(codes == 4)[1:]] = 0
    if not (codes == 4).any():
        codes[500] = 4
    stored[:, 9] = True                       # stored in every row that stores anything
    vals[:, 9] = rng.normal(size=n).astype(np.float32)
    zero_at = rng.random((n, g)) < 0.05       # stored zeros of both signs
    stored |= zero_at & (np.arange(g)[None, :] != 3) & (np.arange(g)[None, :] != 20)
    vals[zero_at] = np.where(rng.random(zero_at.sum()) < 0.5, np.float32(0.0), np.float32(-0.0))
    in3 = codes == 3
    stored[in3, 5] = True
    vals[in3, 5] = np.float32(2.5)
    stored[(np.arange(n) % 7 == 0) & ~in3] = False   # empty rows
    stored[:, [3, 20]] = False                       # empty columns
    vals[~stored] = 0.0
    return vals, stored, codes, n_groups


def _build_big_group(rng):
    """group 1 holds 60 % of the rows: its entries span at least three parts"""
    n, g = 3000, 8
    vals, stored = _random(rng, n, g, 0.9)
    codes = rng.choice(3, n, p=(0.2, 0.6, 0.2)).astype(np.int32)
    return vals, stored, codes, 3


def _build_many_groups(rng):
    """500 groups of 4 rows and about 10 entries: many groups inside one part, every run below the LDS bound"""
    n, g = 2000, 5
    vals, stored = _random(rng, n, g, 0.5)
    return vals, stored, rng.permutation(np.repeat(np.arange(500), 4)).astype(np.int32), 500


def _build_boundary(rng, extra):
    """every row stores the first 16 columns; group 0 holds part / 16 rows: with extra = 0 its last entry is the last of part
    0, with extra = 1 (row 0 also stores column 16) one entry of it lies beyond.  Group 1: AG_LDS_MIN_RUN entries exactly (the
    LDS table), group 2: one row less (global adds)."""
    n, g, row = 400, 17, 16
    part = part_entries(n * row + extra)
    assert part % row == 0 and AG_LDS_MIN_RUN % row == 0
    sizes = [part // row, AG_LDS_MIN_RUN // row, AG_LDS_MIN_RUN // row - 1]
    sizes.append(n - sum(sizes))
    vals = (rng.normal(size=(n, g)) * 3).astype(np.float32)
    stored = np.zeros((n, g), dtype=bool)
    stored[:, :row] = True
    codes = np.repeat(np.arange(4), sizes).astype(np.int32)
    if extra:
        stored[0, row] = True
    vals[~stored] = 0.0
    return vals, stored, codes, 4


def _build_window(rng, g, density, n):
    """g around the LDS window; the columns at the window's edge are stored in every group"""
    vals, stored = _random(rng, n, g, density)
    for c in (0, AG_WINDOW - 2, AG_WINDOW - 1, AG_WINDOW, g - 1):
        if c < g:
            stored[::2, c] = True
            vals[::2, c] = rng.normal(size=len(vals[::2])).astype(np.float32)
    return vals, stored, (np.arange(n) % 3).astype(np.int32), 3


def _build_dense(rng):
    vals = rng.normal(size=(257, 50)).astype(np.float32)
    return vals, np.ones(vals.shape, dtype=bool), _codes(rng, 257, 4), 4


def _build_g1(rng):
    vals, stored = _random(rng, 500, 1, 0.6)
    return vals, stored, _codes(rng, 500, 3), 3


def _build_cancellation(rng):
    """the reference's test_var_no_catastrophic_cancellation for values exact in float32: two groups of 1000 cells, 4 dense
    genes, values 2^23 + {0, 1, 2, 3}"""
    vals = (2.0 ** 23 + rng.integers(0, 4, size=(2000, 4))).astype(np.float32)
    return vals, np.ones(vals.shape, dtype=bool), np.repeat(np.arange(2), 1000).astype(np.int32), 2


def _fill(rng, vals, stored, rows, col, n_neg, n_pos, mode="random", n_stored_zero=0):
    """column `col` of the group's `rows`: n_neg negative and n_pos positive stored values, n_stored_zero stored zeros"""
    pick = rng.permutation(rows)
    neg, pos, zer = pick[:n_neg], pick[n_neg:n_neg + n_pos], pick[n_neg + n_pos:n_neg + n_pos + n_stored_zero]
    draw = {"random": lambda m: rng.uniform(0.5, 100.0, m), "ties": lambda m: rng.integers(1, 4, m).astype(np.float64),
            "equal": lambda m: np.full(m, 7.25)}[mode]
    vals[neg, col], vals[pos, col] = (-draw(len(neg))).astype(np.float32), draw(len(pos)).astype(np.float32)
    vals[zer, col] = np.where(np.arange(len(zer)) % 2 == 0, np.float32(0.0), np.float32(-0.0))
    stored[np.concatenate([neg, pos, zer]).astype(np.int64), col] = True


def _build_med_tiers(rng):
    """segment lengths 1, 2, each tier bound and that bound + 1 (the last: longer than one LDS chunk): every group is barely
    larger than its segments, so the middle ranks fall among the stored values.  Columns: 0 all negative, 1 all positive,
    2 heavy ties, 3 all equal, 4 the longer neighbour (length + 1)."""
    w, ch = AG_MED_WAVE_MAX, AG_MED_CHUNK
    lengths = [1, 2, w, ch]
    sizes = [2, 3, w + 4, ch + 5]
    n, g = sum(sizes), 5
    vals, stored = np.zeros((n, g), np.float32), np.zeros((n, g), dtype=bool)
    codes = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)
    for k, length in enumerate(lengths):
        rows = np.flatnonzero(codes == k)
        _fill(rng, vals, stored, rows, 0, length, 0)
        _fill(rng, vals, stored, rows, 1, 0, length)
        _fill(rng, vals, stored, rows, 2, 0, length, "ties")
        _fill(rng, vals, stored, rows, 3, length, 0, "equal")
        _fill(rng, vals, stored, rows, 4, 0, length + 1)
    return vals, stored, codes, len(sizes)


# (n_neg, n_pos) for a group of 10 / 11 cells: the middle pair both negative, straddling negative / zero, both in the zero
# block, straddling zero / positive, both positive; the sixth column repeats "straddling zero / positive" with stored zeros
MIDDLE_POSITIONS = {10: ((6, 1), (5, 2), (2, 3), (1, 5), (0, 8), (1, 5)), 11: ((6, 1), (5, 5), (2, 3), (4, 6), (0, 8), (2, 6))}


def _build_med_positions(rng):
    sizes = [10, 11, 10, 11]
    n, g = sum(sizes), 6
    vals, stored = np.zeros((n, g), np.float32), np.zeros((n, g), dtype=bool)
    codes = rng.permutation(np.repeat(np.arange(4), sizes)).astype(np.int32)
    for k, size in enumerate(sizes):
        rows = np.flatnonzero(codes == k)
        for col, (n_neg, n_pos) in enumerate(MIDDLE_POSITIONS[size]):
            _fill(rng, vals, stored, rows, col, n_neg, n_pos, "ties" if k >= 2 else "random", n_stored_zero=2 if col == 5 else 0)
    return vals, stored, codes, 4


def _build_med_rounding(rng):
    """group 0: {1, 1 + 2^-23}, whose float32 sum rounds; group 1: {2^24 - 1, 2^24}, integers whose sum exceeds 2^24; group 2:
    the same pairs with two zeros around them (even size 4, the pair straddles nothing)"""
    vals = np.zeros((8, 2), np.float32)
    vals[0:2, 0] = [1.0, 1.0 + 2.0 ** -23]
    vals[0:2, 1] = [-1.0, -(1.0 + 2.0 ** -23)]
    vals[2:4, 0] = [2.0 ** 24 - 1, 2.0 ** 24]
    vals[2:4, 1] = [-(2.0 ** 24 - 1), -(2.0 ** 24)]
    vals[4:8, 0] = [2.0 ** 24 - 1, 2.0 ** 24, 2.0 ** 24, 3.0]
    vals[4:8, 1] = [1.0, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -22, 0.5]
    return vals, vals != 0, np.array([0, 0, 1, 1, 2, 2, 2, 2], np.int32), 3


#        name              builder
CASES = {
    "one-group":        _build_one_group,
    "identity":         _build_identity,
    "mixed":            _build_mixed,
    "big-group":        _build_big_group,
    "many-groups":      _build_many_groups,
    "boundary-exact":   lambda rng: _build_boundary(rng, 0),
    "boundary-plus1":   lambda rng: _build_boundary(rng, 1),
    "window-1":         lambda rng: _build_window(rng, AG_WINDOW - 1, 0.02, 60),
    "window":           lambda rng: _build_window(rng, AG_WINDOW, 0.05, 60),
    "window+1":         lambda rng: _build_window(rng, AG_WINDOW + 1, 0.15, 40),
    "dense":            _build_dense,
    "g1":               _build_g1,
    "cancellation":     _build_cancellation,
    "med-tiers":        _build_med_tiers,
    "med-positions":    _build_med_positions,
    "med-rounding":     _build_med_rounding,
}
CASE_NAMES = tuple(CASES)
DETERMINISM_CASES = ("mixed", "big-group", "boundary-plus1", "window+1", "med-tiers")


class Case:
    def __init__(self, name, vals, stored, codes, n_groups):
        self.name, self.vals, self.stored, self.codes, self.n_groups = name, vals, stored, codes, n_groups
        self.n, self.g = vals.shape
        assert vals.dtype == np.float32 and stored.shape == vals.shape and codes.dtype == np.int32 and not vals[~stored].any()
        self.indptr = np.concatenate([[0], np.cumsum(stored.sum(axis=1))]).astype(np.int64)
        self.indices = np.nonzero(stored)[1].astype(np.int32)
        self.data = vals[stored]
        self.nnz = int(self.indptr[-1])
        for a in (vals, stored, codes, self.indptr, self.indices, self.data):
            a.setflags(write=False)

    @property
    def order(self):
        return grouping(self.codes, self.n_groups)[0]

    @property
    def sizes(self):
        return grouping(self.codes, self.n_groups)[1]

    def permuted(self, seed=1):
        perm = np.random.default_rng(seed).permutation(self.n)
        return Case(self.name, np.ascontiguousarray(self.vals[perm]), np.ascontiguousarray(self.stored[perm]), self.codes[perm].copy(),
                    self.n_groups)


def grouping(codes, n_groups):
    """-> (order int32: the rows with a group, sorted by group, stable; group_sizes int64 [n_groups])"""
    keep = np.flatnonzero((codes >= 0) & (codes < n_groups))
    order = keep[np.argsort(codes[keep], kind="stable")].astype(np.int32)
    return order, np.bincount(codes[keep], minlength=n_groups).astype(np.int64)


@lru_cache(maxsize=None)
def case(name: str) -> Case:
    seed = 7000 + sum(map(ord, name))
    return Case(name, *CASES[name](np.random.default_rng(seed)))


# ---------------------------------------------------------------------------------------------------------------------
# The restatement.
# ---------------------------------------------------------------------------------------------------------------------
def middle(lo, hi, odd: bool, mid_in_f32: bool) -> np.float64:
    lo, hi = np.float32(lo), np.float32(hi)
    if odd:
        m = np.float64(lo)
    elif mid_in_f32:
        with np.errstate(over="ignore"):
            m = np.float64(np.float32(lo + hi) / np.float32(2))
    else:
        m = (np.float64(lo) + np.float64(hi)) / 2
    return np.float64(0.0) if m == 0 else m


def restate(vals, codes, n_groups, mid_in_f32: bool, want_median=True):
    """-> dict: sum, m2 (extended precision), count_nonzero, count_negative (int64), median (float64), amax [g], dev [n_groups, g],
    sizes"""
    n, g = vals.shape
    wide = vals.astype(np.longdouble)
    keep = (codes >= 0) & (codes < n_groups)
    out = {"sum": np.zeros((n_groups, g), np.longdouble), "m2": np.zeros((n_groups, g), np.longdouble),
           "count_nonzero": np.zeros((n_groups, g), np.int64), "count_negative": np.zeros((n_groups, g), np.int64),
           "median": np.full((n_groups, g), np.nan), "dev": np.zeros((n_groups, g), np.longdouble),
           "amax": np.abs(wide[keep]).max(axis=0) if keep.any() else np.zeros(g, np.longdouble),
           "sizes": np.bincount(codes[keep], minlength=n_groups).astype(np.int64)}
    order = np.flatnonzero(keep)[np.argsort(codes[keep], kind="stable")]
    bounds = np.concatenate([[0], np.cumsum(out["sizes"])])
    for k in range(n_groups):
        rows = order[bounds[k]:bounds[k + 1]]
        size = len(rows)
        if size == 0:
            continue
        x = wide[rows]
        out["sum"][k] = x.sum(axis=0)
        mean = out["sum"][k] / size
        out["m2"][k] = ((x - mean) ** 2).sum(axis=0)
        out["dev"][k] = np.where(x != 0, np.abs(x - mean), 0).max(axis=0)
        out["count_nonzero"][k] = (x != 0).sum(axis=0)
        out["count_negative"][k] = (x < 0).sum(axis=0)
        if want_median:
            s = np.sort(vals[rows], axis=0)
            for j in range(g):
                out["median"][k, j] = middle(s[(size - 1) // 2, j], s[size // 2, j], size % 2 == 1, mid_in_f32)
    return out


def sum_bound(sizes, amax):
    size = sizes.astype(np.longdouble)[:, None]
    return (size * np.longdouble(2) ** -61 + np.longdouble(2) ** -53) * size * amax[None, :]


def m2_bound(sizes, amax, dev, m2):
    size = sizes.astype(np.longdouble)[:, None]
    mean_err = (size * np.longdouble(2) ** -61 + np.longdouble(2) ** -52) * amax[None, :]
    return size ** 2 * dev ** 2 * np.longdouble(2) ** -60 + np.longdouble(2) ** -50 * m2 + size * mean_err ** 2


# ---------------------------------------------------------------------------------------------------------------------
# Callers of the entry points through the raw C ABI: numpy in, numpy out, the return code handed back.  Every output has PAD
# extra elements behind [n_groups x g] and is prefilled, so that an element nobody wrote, or one written beyond the end, shows.
# ---------------------------------------------------------------------------------------------------------------------
PAD = 8
FILL_F, FILL_I = -777.0, -777
MOMENT_KEYS = ("sum", "count_nonzero", "count_negative", "m2")


class AggregateAbi:
    def __init__(self, lib, mem):
        self.lib, self.mem = lib, mem

    def _ws(self, n, g, nnz, n_groups, short=0):
        nbytes = int(self.lib.scamd_aggregate_workspace_bytes(max(n, 0), max(g, 0), max(nnz, 0), min(max(n_groups, 0), max(n, 0))))
        return self.mem.full(max(nbytes - short, 1), np.uint8, 0xAB), max(nbytes - short, 0)

    def _inputs(self, cs, order, sizes):
        m = self.mem
        return dict(indptr=m.put(cs.indptr, np.int64), indices=m.put(cs.indices, np.int32), data=m.put(cs.data, np.float32),
                    codes=m.put(cs.codes, np.int32), order=m.put(order, np.int32), sizes=m.put(sizes, np.int64))

    def moments(self, cs, *, want_m2=True, order=None, sizes=None, null=(), ws_short=0, **over):
        """-> (rc, flags, dict of MOMENT_KEYS -> [n_groups x g + PAD] flat arrays); over: n, g, nnz, n_order, n_groups as PASSED"""
        m, z = self.mem, C.c_void_p(0)
        order = cs.order if order is None else order
        sizes = cs.sizes if sizes is None else sizes
        d = self._inputs(cs, order, sizes)
        cells = cs.n_groups * cs.g
        outs = {"sum": m.full(cells + PAD, np.float64, FILL_F), "count_nonzero": m.full(cells + PAD, np.int64, FILL_I),
                "count_negative": m.full(cells + PAD, np.int64, FILL_I), "m2": m.full(cells + PAD, np.float64, FILL_F)}
        flags = m.full(1, np.uint32, 0xAAAA)
        ws, wsz = self._ws(cs.n, cs.g, cs.nnz, cs.n_groups, ws_short)

        def p(name, buf):
            return z if name in null else m.ptr(buf)

        rc = self.lib.scamd_aggregate_moments_f32(
            p("indptr", d["indptr"]), p("indices", d["indices"]), p("data", d["data"]), over.get("n", cs.n), over.get("g", cs.g),
            over.get("nnz", cs.nnz), p("codes", d["codes"]), p("order", d["order"]), over.get("n_order", len(order)), p("sizes", d["sizes"]),
            over.get("n_groups", cs.n_groups), p("sum", outs["sum"]), p("count_nonzero", outs["count_nonzero"]),
            p("count_negative", outs["count_negative"]), m.ptr(outs["m2"]) if want_m2 and "m2" not in null else z, p("flags", flags),
            p("workspace", ws), wsz, m.stream)
        m.sync()
        return rc, int(m.get(flags)[0]), {k: m.get(v) for k, v in outs.items()}

    def median(self, cs, count_nonzero, count_negative, mid_in_f32, *, null=(), ws_short=0, **over):
        """-> (rc, median [n_groups x g + PAD] flat, info [3])"""
        m, z = self.mem, C.c_void_p(0)
        d = self._inputs(cs, cs.order, cs.sizes)
        cells = cs.n_groups * cs.g
        nz, ng = m.put(count_nonzero[:cells], np.int64), m.put(count_negative[:cells], np.int64)
        out = m.full(cells + PAD, np.float64, FILL_F)
        info = (C.c_int64 * 3)(-1, -1, -1)
        ws, wsz = self._ws(cs.n, cs.g, cs.nnz, cs.n_groups, ws_short)

        def p(name, buf):
            return z if name in null else m.ptr(buf)

        rc = self.lib.scamd_aggregate_median_f32(
            p("indptr", d["indptr"]), p("indices", d["indices"]), p("data", d["data"]), over.get("n", cs.n), over.get("g", cs.g),
            over.get("nnz", cs.nnz), p("order", d["order"]), over.get("n_order", len(cs.order)), p("sizes", d["sizes"]),
            over.get("n_groups", cs.n_groups), p("count_nonzero", nz), p("count_negative", ng), int(mid_in_f32), p("median", out), info,
            p("workspace", ws), wsz, m.stream)
        m.sync()
        return rc, m.get(out), [int(v) for v in info]


# ---------------------------------------------------------------------------------------------------------------------
# The checker.
# ---------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.tobytes() == b.tobytes()


def run_all(abi, cs):
    """both entry points, the median with mid_in_f32 on and off -> dict of flat arrays"""
    rc, flags, out = abi.moments(cs)
    assert rc == 0 and flags == 0, (cs.name, rc, flags)
    for f32 in (1, 0):
        rc, med, info = abi.median(cs, out["count_nonzero"], out["count_negative"], f32)
        assert rc == 0 and sum(info) == cs.n_groups * cs.g and min(info) >= 0, (cs.name, rc, info)
        out[f"median{f32}"], out[f"info{f32}"] = med, info
    return out


def run_case(abi, name, label="", rerun=None):
    cs = case(name)
    what = f"{label} {name}"
    cells, shape = cs.n_groups * cs.g, (cs.n_groups, cs.g)
    out = run_all(abi, cs)
    want = restate(cs.vals, cs.codes, cs.n_groups, True)
    want0 = restate(cs.vals, cs.codes, cs.n_groups, False)
    # nothing is written beyond [n_groups x g]
    for k in ("sum", "m2", "median1", "median0"):
        assert (out[k][cells:] == FILL_F).all(), (what, k, "written beyond the end")
    for k in ("count_nonzero", "count_negative"):
        assert (out[k][cells:] == FILL_I).all(), (what, k, "written beyond the end")
    got = {k: v[:cells].reshape(shape) for k, v in out.items() if not k.startswith("info")}
    assert np.array_equal(got["count_nonzero"], want["count_nonzero"]), (what, "count_nonzero")
    assert np.array_equal(got["count_negative"], want["count_negative"]), (what, "count_negative")
    err = np.abs(got["sum"].astype(np.longdouble) - want["sum"])
    assert (err <= sum_bound(want["sizes"], want["amax"])).all(), (what, "sum", float(err.max()))
    err = np.abs(got["m2"].astype(np.longdouble) - want["m2"])
    bound = m2_bound(want["sizes"], want["amax"], want["dev"], want["m2"])
    assert (err <= bound).all(), (what, "m2", float(err.max()), float(bound[err > bound].min()))
    for key, ref in (("median1", want["median"]), ("median0", want0["median"])):
        assert np.array_equal(got[key], ref, equal_nan=True), (what, key, np.argwhere(~((got[key] == ref) | np.isnan(ref)))[:5])
        assert not np.signbit(got[key][got[key] == 0]).any(), (what, key, "a zero result is +0.0")
        assert np.isnan(got[key][want["sizes"] == 0]).all(), (what, key, "an empty group gives NaN")
    # an empty group: sum 0, counts 0, m2 0
    empty = want["sizes"] == 0
    assert not got["sum"][empty].any() and not got["m2"][empty].any() and not got["count_nonzero"][empty].any(), (what, "empty group")
    if rerun if rerun is not None else name in DETERMINISM_CASES:
        again = run_all(abi, cs)
        shuffled = run_all(abi, cs.permuted())
        for k in ("sum", "count_nonzero", "count_negative", "m2", "median1", "median0"):
            assert same_bits(out[k], again[k]), (what, k, "two runs differ")
            assert same_bits(out[k], shuffled[k]), (what, k, "a permutation of the rows changes the result")
    return cs, got, out


def check_case_specifics(name, cs, got, out):
    """what a case was built to show, beyond the general checks"""
    sizes = cs.sizes
    if name == "identity":
        assert np.array_equal(got["sum"][cs.codes], cs.vals.astype(np.float64)), "n_groups = n: the sum layer is the matrix"
    if name == "mixed":
        assert sizes[2] == 0 and sizes[4] == 1 and cs.codes[0] == -1 and cs.codes[-1] == -1
        assert got["m2"][3, 5] == 0.0 and got["sum"][3, 5] == 2.5 * sizes[3], "a constant, fully stored column: m2 == 0.0 exactly"
    if name == "cancellation":
        x = cs.vals.astype(np.float64)
        for k in range(2):
            xs = x[cs.codes == k]
            true = np.var(xs, axis=0)
            textbook = (xs ** 2).sum(axis=0) / 1000 - (xs.sum(axis=0) / 1000) ** 2
            assert (np.abs(textbook - true) > 1e-4 * true).any(), "the textbook formula was expected to fail on this data"
            np.testing.assert_allclose(got["m2"][k] / 1000, true, rtol=1e-4)
    if name == "dense":
        assert out["info1"][0] == 0, "a dense matrix: no pair is decided from the counts"
    if name == "med-tiers":
        assert out["info1"][1] > 0 and out["info1"][2] > 0
    if name in ("mixed", "many-groups", "big-group"):
        assert out["info1"][0] > 0


def assert_table_covers_every_path():
    """no GPU, no emulator: every kernel instantiation and both sides of every sizing rule have a case"""
    lanes, runs, seg = set(), set(), set()
    spans, groups_in_part, windows = 0, 0, set()
    for name in CASE_NAMES:
        cs = case(name)
        order, sizes = cs.order, cs.sizes
        lanes.add(lanes_per_row(cs.n, cs.nnz))
        windows.add(-(-cs.g // AG_WINDOW))
        part = part_entries(cs.nnz)
        lens = np.diff(cs.indptr)[order]
        pos = np.concatenate([[0], np.cumsum(lens)])
        goff = np.concatenate([[0], np.cumsum(sizes)])
        first, last = pos[goff[:-1]], pos[goff[1:]]          # the entries of every group in the stream
        for k in np.flatnonzero(last > first):
            p_first, p_last = first[k] // part, (last[k] - 1) // part
            spans = max(spans, p_last - p_first + 1)
            for p in range(p_first, p_last + 1):
                runs.add(min(last[k], (p + 1) * part) - max(first[k], p * part) >= AG_LDS_MIN_RUN)
        per_part = np.bincount((first[last > first] // part).astype(np.int64))
        groups_in_part = max(groups_in_part, per_part.max() if len(per_part) else 0)
        if name.startswith("boundary"):
            extra = int(name.endswith("plus1"))
            assert last[0] == part + extra and last[1] - first[1] == AG_LDS_MIN_RUN and last[2] - first[2] == AG_LDS_MIN_RUN - 16
        stored_nz = cs.stored & (cs.vals != 0)
        for k in range(cs.n_groups):
            seg.update(cs.stored[cs.codes == k].sum(axis=0).tolist())
        assert name != "dense" or cs.stored.all()
        assert name != "mixed" or ((stored_nz != cs.stored).any() and (cs.vals < 0).any() and (np.diff(cs.indptr) == 0).any()
                                   and np.signbit(cs.data[cs.data == 0]).any() and not np.signbit(cs.data[cs.data == 0]).all())
    assert lanes == {8, 16, 32, 64}, lanes
    assert runs == {True, False}
    assert spans >= 3 and groups_in_part >= 100
    assert windows == {1, 2} and {case(n).g for n in CASE_NAMES} >= {1, AG_WINDOW - 1, AG_WINDOW, AG_WINDOW + 1}
    w, ch = AG_MED_WAVE_MAX, AG_MED_CHUNK
    assert seg >= {0, 1, 2, 3, w, w + 1, ch, ch + 1}, "segment lengths around the median tiers"
    cs = case("med-positions")
    assert sorted(set(cs.sizes.tolist())) == [10, 11]
    r = case("med-rounding")
    assert np.float32(r.vals[0, 0] + r.vals[1, 0]) != np.float64(r.vals[0, 0]) + np.float64(r.vals[1, 0])
    assert np.float64(r.vals[2, 0]) + np.float64(r.vals[3, 0]) > 2 ** 24
    assert case("identity").n_groups == case("identity").n and case("one-group").n_groups == 1
    return lanes, seg


def run_nan_case(abi, label=""):
    """a NaN and an infinity in two pairs: flag bit 0, the values take part in nothing, every other pair keeps its bits"""
    cs = case("mixed")
    _, _, clean = abi.moments(cs)
    vals = cs.vals.copy()
    rows = np.flatnonzero((cs.codes == 1) & cs.stored[:, 9])
    hit = [(rows[0], 9), (rows[1], 9)]
    vals[hit[0]], vals[hit[1]] = np.nan, -np.inf
    rc, flags, dirty = abi.moments(Case("mixed-nan", vals, cs.stored.copy(), cs.codes.copy(), cs.n_groups))
    assert rc == 0 and flags == FLAG_NONFINITE, (label, rc, flags)
    cells, pair = cs.n_groups * cs.g, 1 * cs.g + 9
    keep = np.ones(cells + PAD, dtype=bool)
    keep[pair] = False
    for k in MOMENT_KEYS:
        assert same_bits(clean[k][keep], dirty[k][keep]), (label, k)
    without = vals.copy()
    without[hit[0]], without[hit[1]] = 0.0, 0.0
    want = restate(without, cs.codes, cs.n_groups, True, want_median=False)
    assert dirty["count_nonzero"][pair] == want["count_nonzero"][1, 9]
    assert abs(np.longdouble(dirty["sum"][pair]) - want["sum"][1, 9]) <= sum_bound(want["sizes"], want["amax"])[1, 9]


def run_argument_checks(abi, launches=None):
    """the documented codes; a rejected call starts no kernel and writes no output"""
    cs = case("one-group")
    _, _, m = abi.moments(cs)   # (the counts the median calls below are handed)
    before = launches() if launches else 0

    def untouched(out):
        return all((out[k] == (FILL_I if k.startswith("count") else FILL_F)).all() for k in MOMENT_KEYS)

    for kw, code in ((dict(null=("indptr",)), EINVAL), (dict(null=("indices",)), EINVAL), (dict(null=("data",)), EINVAL),
                     (dict(null=("codes",)), EINVAL), (dict(null=("order",)), EINVAL), (dict(null=("sizes",)), EINVAL),
                     (dict(null=("sum",)), EINVAL), (dict(null=("count_nonzero",)), EINVAL), (dict(null=("count_negative",)), EINVAL),
                     (dict(null=("flags",)), EINVAL), (dict(n=-1), EINVAL), (dict(g=-1), EINVAL), (dict(nnz=-1), EINVAL),
                     (dict(n_order=-1), EINVAL), (dict(n_groups=-1), EINVAL), (dict(n_groups=cs.n + 1), EINVAL),
                     (dict(n_order=cs.n + 1), EINVAL), (dict(n=1 << 31), EUNSUPPORTED), (dict(g=1 << 31), EUNSUPPORTED),
                     (dict(null=("workspace",)), EWORKSPACE), (dict(ws_short=256), EWORKSPACE)):
        rc, flags, out = abi.moments(cs, **kw)
        assert rc == code and untouched(out) and ("flags" in kw.get("null", ()) or flags == 0xAAAA), (kw, rc, flags)
    for kw, code in ((dict(null=("indptr",)), EINVAL), (dict(null=("order",)), EINVAL), (dict(null=("sizes",)), EINVAL),
                     (dict(null=("median",)), EINVAL), (dict(null=("count_nonzero",)), EINVAL), (dict(null=("count_negative",)), EINVAL),
                     (dict(n=-1), EINVAL), (dict(n_groups=cs.n + 1), EINVAL), (dict(g=40945), EUNSUPPORTED),
                     (dict(null=("workspace",)), EWORKSPACE), (dict(ws_short=256), EWORKSPACE)):
        rc, med, info = abi.median(cs, m["count_nonzero"], m["count_negative"], 1, **kw)
        assert rc == code and (med == FILL_F).all(), (kw, rc)
    if launches:
        assert launches() == before, "an argument check let a kernel start"
    # a code outside [-1, n_groups) is flagged (bit 1) and its row takes part in nothing
    codes = cs.codes.copy()
    r1, r2 = np.flatnonzero(cs.stored.any(axis=1))[:2]
    codes[r1], codes[r2] = 1, -2
    bad = Case("bad-code", cs.vals.copy(), cs.stored.copy(), codes, 1)
    rc, flags, out = abi.moments(bad)
    good = Case("good-code", cs.vals.copy(), cs.stored.copy(), np.where(codes == 0, 0, -1).astype(np.int32), 1)
    rc2, flags2, want = abi.moments(good)
    assert rc == 0 and flags == FLAG_CODE and rc2 == 0 and flags2 == 0
    assert all(same_bits(out[k], want[k]) for k in MOMENT_KEYS)
    # an order that contradicts the codes is flagged (bit 2); nothing is written out of bounds
    wrong = np.arange(cs.n, dtype=np.int32)
    rc, flags, out = abi.moments(bad, order=wrong, sizes=np.array([len(wrong)], np.int64))
    assert rc == 0 and flags & FLAG_ORDER and (out["sum"][cs.g:] == FILL_F).all()
    # n = 0, g = 0, n_groups = 0, n_order = 0 are legal
    for n, g, n_groups in ((0, 5, 0), (7, 0, 2), (7, 5, 0)):
        vals = np.zeros((n, g), np.float32)
        e = Case("empty", vals, np.zeros((n, g), dtype=bool), np.zeros(n, np.int32) if n_groups else np.full(n, -1, np.int32), n_groups)
        rc, flags, out = abi.moments(e)
        assert rc == 0 and flags == 0 and untouched(out), (n, g, n_groups)
        rc, med, info = abi.median(e, out["count_nonzero"], out["count_negative"], 1)
        assert rc == 0 and (med == FILL_F).all() and info == [0, 0, 0]
    nobody = Case("nobody", cs.vals.copy(), cs.stored.copy(), np.full(cs.n, -1, np.int32), 2)
    rc, flags, out = abi.moments(nobody)
    assert rc == 0 and flags == 0 and not out["sum"][: 2 * cs.g].any() and not out["count_nonzero"][: 2 * cs.g].any()
    rc, med, info = abi.median(nobody, out["count_nonzero"], out["count_negative"], 1)
    assert rc == 0 and np.isnan(med[: 2 * cs.g]).all()


# ---------------------------------------------------------------------------------------------------------------------
# CPU stand-in for scanpy_amd._get_aggregate.GpuAggregateBackend (the front-end tests): float64 numpy behind the same
# interface.
# ---------------------------------------------------------------------------------------------------------------------
class CpuStubAggregateBackend:
    def __init__(self):
        self.calls = []

    def csr(self, indptr, indices, data, n, g):
        assert data.dtype == np.float32 and indptr.dtype == np.int64 and indices.dtype == np.int32
        x = sparse.csr_matrix((data, indices, indptr), shape=(n, g))
        assert x.has_canonical_format
        self.calls.append(("csr", n, g))
        return x

    def csr_from_transpose(self, indptr, indices, data, n, g):
        """the arrays are the CSR of the g x n transpose"""
        assert data.dtype == np.float32
        t = sparse.csr_matrix((data, indices, indptr), shape=(g, n))
        assert t.has_canonical_format
        self.calls.append(("csr_from_transpose", n, g))
        x = t.T.tocsr()
        x.sort_indices()
        return x

    def aggregate(self, x, codes, order, group_sizes, *, want_m2, want_median, mid_in_f32):
        assert codes.dtype == np.int32 and order.dtype == np.int32 and group_sizes.dtype == np.int64
        n_groups = len(group_sizes)
        ref = grouping(codes, n_groups)
        assert np.array_equal(ref[0], order) and np.array_equal(ref[1], group_sizes)
        self.calls.append(("aggregate", want_m2, want_median, bool(mid_in_f32)))
        dense = np.asarray(x.toarray(), dtype=np.float32)
        finite = np.isfinite(dense[codes >= 0]).all()
        with np.errstate(invalid="ignore", over="ignore"):
            r = restate(np.where(np.isfinite(dense), dense, np.float32(0)), codes, n_groups, bool(mid_in_f32), want_median=want_median)
        out = {"sum": r["sum"].astype(np.float64), "count_nonzero": r["count_nonzero"], "flags": 0 if finite else FLAG_NONFINITE}
        if want_m2:
            out["m2"] = r["m2"].astype(np.float64)
        if want_median:
            out["median"] = r["median"]
        return out


# ---------------------------------------------------------------------------------------------------------------------
# Front-end check shared by tests/test_aggregate_front_cpu.py (on the stand-in above) and tests/test_gpu_aggregate.py (on the
# device): the reference's test_aggregate_vs_pandas (tests/test_aggregated.py:78-146 of the reference) restated on the committed
# pbmc68k fixture, by louvain x bulk_labels.  The frames are compared with the reference's own check and tolerance,
# `pd.testing.assert_frame_equal(..., check_dtype=False, atol=1e-5)`.  A combination whose cells are all masked stays in the
# result (the categories are formed before the mask, as in the reference) with n_obs_aggregated 0, sum 0, count 0 and NaN
# elsewhere; pandas, which only sees the kept cells, is reindexed to say the same.
# ---------------------------------------------------------------------------------------------------------------------
FRONT_FUNCS = ("sum", "mean", "var", "count_nonzero", "median")


def front_vs_pandas(pbmc68k, source, use_mask, with_na):
    import warnings

    import pandas as pd

    import scanpy_amd as sc

    raw = pbmc68k["raw_X"]
    x = {"raw_csr": raw, "raw_csc": raw.tocsc(), "dense_X": pbmc68k["X"]}[source]
    n, g = x.shape
    assert (n, g) == (700, 765) and x.dtype == np.float32
    lou = pbmc68k["louvain_codes"].astype(np.int64).copy()
    if with_na:
        lou[::5] = -1
    obs = pd.DataFrame({"louvain": pd.Categorical.from_codes(lou, [f"L{c:02d}" for c in range(int(lou.max()) + 1)]),
                        "bulk_labels": pd.Categorical.from_codes(pbmc68k["bulk_labels_codes"].astype(np.int64),
                                                                 [f"B{c}" for c in range(int(pbmc68k["bulk_labels_codes"].max()) + 1)])},
                       index=[f"cell{i}" for i in range(n)])
    var = pd.DataFrame(index=[f"gene{j}" for j in range(g)])
    kwargs = {}
    mask = np.ones(n, dtype=bool)
    if use_mask:
        mask[::4] = False
        kwargs["mask"] = mask
    adata = sc.AnnData(x, obs=obs, var=var)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # (groups of one cell: var is NaN, as in pandas)
        result = sc.get.aggregate(adata, ["louvain", "bulk_labels"], FRONT_FUNCS, **kwargs)
    dense = pd.DataFrame((x.toarray() if sparse.issparse(x) else x).astype(np.float64), index=obs.index, columns=var.index)
    keys = obs[mask]
    groups = dense[mask].join(keys).groupby(["louvain", "bulk_labels"], observed=True)
    sizes = keys.groupby(["louvain", "bulk_labels"], observed=True).size()
    label = sizes.index.to_frame().astype("string").agg("_".join, axis=1).tolist()
    got_index = result.obs.index.tolist()
    assert [i for i in got_index if i in set(label)] == label, "the kept groups, in the order of pandas"
    assert result.obs["n_obs_aggregated"].tolist() == pd.Series(sizes.to_numpy(), index=label).reindex(got_index, fill_value=0).tolist()
    assert result.var is var and list(result.layers) == ["sum", "count_nonzero", "var", "mean", "median"]
    for metric in FRONT_FUNCS:
        if metric == "count_nonzero":
            expected = (dense[mask] != 0).astype(np.float64).join(keys).groupby(["louvain", "bulk_labels"], observed=True).agg("sum")
        else:
            expected = groups.agg(metric)
        expected.index = label
        expected = expected.reindex(got_index, fill_value=0.0 if metric in ("sum", "count_nonzero") else np.nan)
        expected.columns.name = None
        got = pd.DataFrame(result.layers[metric], index=got_index, columns=var.index)
        pd.testing.assert_frame_equal(got, expected, check_dtype=False, atol=1e-5)
    return result
