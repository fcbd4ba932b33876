"""TEST INFRASTRUCTURE: numpy-level callers of the C ABI of the HOST-EMULATED kernel library
(tests/emu/_build/*/libscanpy_amd_emu.so).  The emulated library takes host pointers where the product takes device
pointers; prototypes come from scanpy_amd._lib.SIGNATURES (the same table the product binds with)."""
from __future__ import annotations

import ctypes as C
import os
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
from scanpy_amd._lib import SIGNATURES, leiden_stat_names  # noqa: E402


@lru_cache(maxsize=2)
def load(asan: bool = False, path: str | None = None) -> C.CDLL:
    """path: an emulator library built elsewhere (an A/B of two builds), instead of this tree's"""
    sys.path.insert(0, str(HERE))
    import build as emu_build

    lib = C.CDLL(str(path or emu_build.build(asan=asan)))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    for name in ("emu_launches", "emu_partial_collectives", "emu_mixed_collectives", "emu_reads_of_inactive_lanes", "emu_max_dyn_lds"):
        getattr(lib, name).restype = C.c_longlong
    lib.emu_user_counter.restype, lib.emu_user_counter.argtypes = C.c_longlong, (C.c_int,)
    lib.emu_set_dma_late.restype, lib.emu_set_dma_late.argtypes = None, (C.c_int,)
    return lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def _check(lib, rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: rc={rc}: {lib.scamd_last_error().decode()}")


def _ws(nbytes: int):
    # exact size, its own allocation: an over-run past the workspace is an over-run of a heap block
    return np.full(max(int(nbytes), 1), 0xAB, dtype=np.uint8)


def stats(lib) -> dict:
    return {"launches": lib.emu_launches(), "partial_collectives": lib.emu_partial_collectives(),
            "mixed_collectives": lib.emu_mixed_collectives(), "reads_of_inactive_lanes": lib.emu_reads_of_inactive_lanes()}


def user_counters(lib, n: int = 16) -> list:
    """the event counters the kernels bump under SCAMD_EMU (emu_runtime.cpp: emu_user_counters)"""
    return [int(lib.emu_user_counter(i)) for i in range(n)]


def fuzzy_simplicial_set(lib, idx, dist):
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    n, k = idx.shape
    cap = 2 * n * (k - 1)
    indptr = np.empty(n + 1, dtype=np.int64)
    indices = np.empty(cap, dtype=np.int32)
    data = np.empty(cap, dtype=np.float32)
    sigma = np.empty(n, dtype=np.float32)
    rho = np.empty(n, dtype=np.float32)
    ws = _ws(lib.scamd_fuzzy_workspace_bytes(n, k))
    nnz = C.c_int64(0)
    rc = lib.scamd_fuzzy_simplicial_set_f32(_p(idx), _p(dist), n, k, _p(indptr), _p(indices), _p(data), cap, _p(sigma), _p(rho),
                                            C.byref(nnz), _p(ws), ws.size, None)
    _check(lib, rc, "fuzzy")
    m = int(nnz.value)
    return indptr, indices[:m].copy(), data[:m].copy(), sigma, rho


def leiden(lib, adj, *, resolution=1.0, n_iterations=-1, beta=0.01, seed=0, initial_membership=None, objective=0, node_weights=None):
    adj = adj.tocsr()
    adj.sort_indices()
    n = adj.shape[0]
    indptr = np.ascontiguousarray(adj.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(adj.indices, dtype=np.int32)
    w = np.ascontiguousarray(adj.data, dtype=np.float32)
    memb = np.empty(n, dtype=np.int32)
    q = C.c_double(0)
    nc = C.c_int32(0)
    ws = _ws(lib.scamd_leiden_workspace_bytes(n, adj.nnz))
    init = None if initial_membership is None else np.ascontiguousarray(initial_membership, dtype=np.int32)
    nw = None if node_weights is None else np.ascontiguousarray(node_weights, dtype=np.float32)
    rc = lib.scamd_leiden_csr_nw_f32(_p(indptr), _p(indices), _p(w), n, adj.nnz, float(resolution), int(n_iterations), float(beta),
                                     int(seed), int(objective), _p(nw), _p(init), _p(memb), C.byref(q), C.byref(nc), _p(ws), ws.size, None)
    _check(lib, rc, "leiden")
    return memb, float(q.value), int(nc.value)


def knn(lib, x, k, *, q_begin=0, n_query=None, cert_scale=1.0, nprobe=0, d=None):
    """d: the first d columns of the [n, ld_x] buffer x are the data, the rest is padding the library must not read"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, ld = x.shape
    d = ld if d is None else d
    nq = n if n_query is None else n_query
    idx = np.empty((nq, k), dtype=np.int32)
    dist = np.empty((nq, k), dtype=np.float64)
    ws = _ws(lib.scamd_knn_workspace_bytes(n, d, nq, k))
    nfb = C.c_int64(0)
    if nprobe:
        rc = lib.scamd_knn_l2_ivf_f32(_p(x), n, d, ld, q_begin, nq, k, int(nprobe), _p(idx), _p(dist), C.byref(nfb), _p(ws), ws.size, None)
    else:
        rc = lib.scamd_knn_l2_f32(_p(x), n, d, ld, q_begin, nq, k, _p(idx), _p(dist), float(cert_scale), C.byref(nfb), _p(ws), ws.size, None)
    _check(lib, rc, "knn")
    return idx, dist, int(nfb.value)


def leiden_split(lib, adj, membership):
    """scamd_leiden_debug_split_f32 -> (membership after the split, components - communities)"""
    adj = adj.tocsr()
    adj.sort_indices()
    n = adj.shape[0]
    indptr = np.ascontiguousarray(adj.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(adj.indices, dtype=np.int32)
    w = np.ascontiguousarray(adj.data, dtype=np.float32)
    memb = np.ascontiguousarray(membership, dtype=np.int32).copy()
    ns = C.c_int32(0)
    ws = _ws(lib.scamd_leiden_workspace_bytes(n, adj.nnz))
    rc = lib.scamd_leiden_debug_split_f32(_p(indptr), _p(indices), _p(w), n, adj.nnz, _p(memb), C.byref(ns), _p(ws), ws.size, None)
    _check(lib, rc, "leiden split")
    return memb, int(ns.value)


LEVEL_INFO_KEYS = ("merges", "n_coarse", "coarse_nnz", "n_mid", "n_big", "n_split", "skipped")


def leiden_level(lib, adj, membership, *, refined_in=None, resolution=1.0, beta=0.01, seed=0) -> dict:
    """scamd_leiden_debug_level_f32 -> dict: refined, Kref, Eref, refsize [n], the integers of LEVEL_INFO_KEYS and, unless
    `skipped`, cid [n] and the coarse indptr, indices, wq, k, comm cut to their lengths.  `adj` goes in as it is stored (no
    sorting, no merging of its entries)."""
    n = adj.shape[0]
    indptr = np.ascontiguousarray(adj.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(adj.indices, dtype=np.int32)
    w = np.ascontiguousarray(adj.data, dtype=np.float32)
    nnz = int(indptr[-1])
    memb = np.ascontiguousarray(membership, dtype=np.int32)
    given = None if refined_in is None else np.ascontiguousarray(refined_in, dtype=np.int32)
    assert memb.size == n and (given is None or given.size == n)
    i32 = lambda m: np.full(max(m, 1), -7, dtype=np.int32)  # noqa: E731
    i64 = lambda m: np.full(max(m, 1), -7, dtype=np.int64)  # noqa: E731
    out = dict(refined=i32(n), Kref=i64(n), Eref=i64(n), refsize=i32(n), cid=i32(n), indptr=i64(n + 1), indices=i32(nnz), wq=i64(nnz),
               k=i64(n), comm=i32(n))
    info = (C.c_int64 * 8)()
    ws = _ws(lib.scamd_leiden_workspace_bytes(n, nnz))
    rc = lib.scamd_leiden_debug_level_f32(_p(indptr), _p(indices), _p(w), n, nnz, _p(memb), _p(given), float(resolution), float(beta),
                                          int(seed), *(_p(out[key]) for key in out), info, _p(ws), ws.size, None)
    _check(lib, rc, "leiden level")
    res = dict(zip(LEVEL_INFO_KEYS, (int(v) for v in info)))
    nn, ne = res["n_coarse"], res["coarse_nnz"]
    cut = dict(refined=n, Kref=n, Eref=n, refsize=n, cid=n, indptr=nn + 1, indices=ne, wq=ne, k=nn, comm=nn)
    for key, m in cut.items():
        if not res["skipped"] or key in ("refined", "Kref", "Eref", "refsize"):
            res[key] = out[key][:m]
    return res


def leiden_stats(lib) -> dict:
    keys = leiden_stat_names(lib)
    out = (C.c_int32 * len(keys))()
    lib.scamd_leiden_last_stats(out, len(keys))
    return {k: int(v) for k, v in zip(keys, out) if k is not None}


def pca_csr(lib, x, n_comps, *, zero_center=True, seed=0, tol=2e-8):
    """scamd_pca_csr_f32 on a scipy CSR float32 matrix -> dict(scores, components, variance, variance_ratio, mean, info)"""
    x = x.tocsr()
    x.sort_indices()
    n, g = x.shape
    indptr = np.ascontiguousarray(x.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(x.indices, dtype=np.int32)
    data = np.ascontiguousarray(x.data, dtype=np.float32)
    scores = np.empty((n, n_comps), dtype=np.float32)
    comps = np.empty((n_comps, g), dtype=np.float64)
    var = np.empty(n_comps, dtype=np.float64)
    ratio = np.empty(n_comps, dtype=np.float64)
    mean = np.empty(g, dtype=np.float64)
    info = np.zeros(8, dtype=np.int32)
    ws = _ws(lib.scamd_pca_csr_workspace_bytes(n, g, n_comps))
    rc = lib.scamd_pca_csr_f32(_p(indptr), _p(indices), _p(data), n, g, x.nnz, n_comps, int(zero_center), int(seed), float(tol),
                               _p(scores), _p(comps), _p(var), _p(ratio), _p(mean), _p(info), _p(ws), ws.size, None)
    _check(lib, rc, "pca_csr")
    return dict(scores=scores, components=comps, variance=var, variance_ratio=ratio, mean=mean, info=info)


def dense_info(info):
    return {"n_outer": int(info[0]), "n_gemm": int(info[1]), "block_size": int(info[2]), "chol_retries": int(info[3]),
            "residual": float(info[4:6].view(np.float64)[0])}


def eigh_topk(lib, a, k, *, seed=0, tol=2e-8):
    """scamd_eigh_topk_f64 -> (lam [k], v [g, k], info dict as scanpy_amd._kernels.eigh_topk, raw info words)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    g = a.shape[0]
    lam = np.full(k, np.nan)
    v = np.full((g, k), np.nan)
    info = np.zeros(12, dtype=np.int32)
    ws = _ws(lib.scamd_eigh_topk_workspace_bytes(g, k))
    rc = lib.scamd_eigh_topk_f64(_p(a), g, g, k, int(seed), float(tol), _p(lam), _p(v), _p(info), _p(ws), ws.size, None)
    _check(lib, rc, "eigh_topk")
    return lam, v, dense_info(info), info


def spectral_embedding(lib, a, dim, *, seed=0, tol=2e-6, max_outer=60, max_degree=64):
    """scamd_spectral_embedding_f32 on a scipy CSR graph -> (v [n, dim], info dict as scanpy_amd._kernels.spectral_embedding,
    raw info doubles)"""
    a = a.tocsr()
    a.sort_indices()
    n = a.shape[0]
    indptr = np.ascontiguousarray(a.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(a.indices, dtype=np.int32)
    w = np.ascontiguousarray(a.data, dtype=np.float32)
    out = np.full((n, dim), np.nan)
    info = np.zeros(8, dtype=np.float64)
    ws = _ws(lib.scamd_spectral_embedding_workspace_bytes(n, a.nnz, dim))
    rc = lib.scamd_spectral_embedding_f32(_p(indptr), _p(indices), _p(w), n, a.nnz, dim, int(seed), float(tol), int(max_outer),
                                          int(max_degree), _p(out), info.ctypes.data_as(C.POINTER(C.c_double)), _p(ws), ws.size, None)
    _check(lib, rc, "spectral_embedding")
    return out, {"outer_iterations": int(info[0]), "operator_applications": int(info[1]), "residual": float(info[2]),
                 "converged": bool(info[3] > 0.5), "ritz_values": [float(info[4 + j]) for j in range(min(dim, 4))]}, info


def csr_gram(lib, x, scale_bits=None):
    x = x.tocsr()
    x.sort_indices()
    n, g = x.shape
    indptr = np.ascontiguousarray(x.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(x.indices, dtype=np.int32)
    data = np.ascontiguousarray(x.data, dtype=np.float32)
    ws = _ws(lib.scamd_csr_gram_workspace_bytes(n, g))
    absmax = C.c_float(0)
    rc = lib.scamd_csr_gram_f32(_p(indptr), _p(indices), _p(data), n, g, x.nnz, 0, None, 0, None, C.byref(absmax), _p(ws), ws.size, None)
    _check(lib, rc, "gram absmax")
    if scale_bits is None:
        scale_bits = int(np.floor(62 - np.log2(n * float(absmax.value) ** 2))) - 1
    g_pad = (g + 127) // 128 * 128
    gram = np.zeros((g_pad, g_pad), dtype=np.int64)
    colsum = np.zeros(g_pad, dtype=np.int64)
    rc = lib.scamd_csr_gram_f32(_p(indptr), _p(indices), _p(data), n, g, x.nnz, scale_bits, _p(gram), g_pad, _p(colsum), None, _p(ws), ws.size, None)
    _check(lib, rc, "gram")
    return gram, colsum, scale_bits, float(absmax.value)


def modularity(lib, adj, membership, resolution=1.0):
    adj = adj.tocsr()
    n = adj.shape[0]
    indptr = np.ascontiguousarray(adj.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(adj.indices, dtype=np.int32)
    w = np.ascontiguousarray(adj.data, dtype=np.float32)
    memb = np.ascontiguousarray(membership, dtype=np.int32)
    q = C.c_double(0)
    ws = _ws(lib.scamd_leiden_workspace_bytes(n, adj.nnz))
    rc = lib.scamd_modularity_csr_f32(_p(indptr), _p(indices), _p(w), n, adj.nnz, _p(memb), float(resolution), C.byref(q), _p(ws), ws.size, None)
    _check(lib, rc, "modularity")
    return float(q.value)


# ---------------------------------------------------------------------------------------------------------------------
# The connectivity kernels (csrc/fuzzy.hip) and the sparse half of PCA (csrc/pca.hip) through the raw C ABI: numpy in, numpy
# out, the return code handed back instead of raised (the argument checks are part of what is tested), outputs prefilled so
# that an element nobody wrote shows.  `Abi` does not care where the buffers live: `HostMem` (below) for the emulated
# library, tests/graph_kernel_cases.py:DeviceMem for the product library on a GPU -- one set of callers for both suites.
# ---------------------------------------------------------------------------------------------------------------------
class HostMem:
    stream = None

    def put(self, a, dtype):
        return np.array(a, dtype=dtype, order="C", copy=True)

    def full(self, shape, dtype, fill):
        return np.full(shape, fill, dtype=dtype)

    def ptr(self, a):
        # an empty buffer travels as NULL, as an empty torch tensor does on the product's side
        return C.c_void_p(a.ctypes.data) if a is not None and a.size else C.c_void_p(0)

    def get(self, a):
        return a

    def sync(self):
        pass


class Abi:
    def __init__(self, lib, mem):
        self.lib, self.mem = lib, mem

    def _ws(self, nbytes, short=0):
        # exact size (less `short` bytes), filled with 0xAB: an entry point initialises what it reads
        ws = self.mem.full(max(int(nbytes) - short, 1), np.uint8, 0xAB)
        return ws, max(int(nbytes) - short, 0)

    def connectivity(self, method, idx, dist, *, cap=None, ws_short=0):
        """method: 'umap' | 'gauss' | 'jaccard' -> (rc, indptr, indices, data, sigma, rho); sigma / rho None but for umap"""
        m, lib = self.mem, self.lib
        n, k = idx.shape
        cap = 2 * n * (k - 1) if cap is None else cap
        d_idx, d_dist = m.put(idx, np.int32), m.put(dist, np.float32)
        indptr = m.full(n + 1, np.int64, -1)
        indices = m.full(max(cap, 1), np.int32, -1)
        data = m.full(max(cap, 1), np.float32, np.nan)
        sigma, rho = m.full(n, np.float32, np.nan), m.full(n, np.float32, np.nan)
        ws, wsz = self._ws(lib.scamd_fuzzy_workspace_bytes(n, k), ws_short)
        nnz = C.c_int64(-1)
        p = m.ptr
        if method == "umap":
            rc = lib.scamd_fuzzy_simplicial_set_f32(p(d_idx), p(d_dist), n, k, p(indptr), p(indices), p(data), cap, p(sigma), p(rho),
                                                    C.byref(nnz), p(ws), wsz, m.stream)
        elif method == "gauss":
            rc = lib.scamd_gauss_connectivities_f32(p(d_idx), p(d_dist), n, k, p(indptr), p(indices), p(data), cap, C.byref(nnz), p(ws), wsz, m.stream)
        else:
            rc = lib.scamd_jaccard_connectivities_f32(p(d_idx), n, k, p(indptr), p(indices), p(data), cap, C.byref(nnz), p(ws), wsz, m.stream)
        m.sync()
        if rc != 0:
            return rc, None, None, None, None, None
        z = int(nnz.value)
        um = method == "umap"
        return rc, m.get(indptr), m.get(indices)[:z].copy(), m.get(data)[:z].copy(), m.get(sigma) if um else None, m.get(rho) if um else None

    def fuzzy_weights(self, idx, dist, row_begin, n_total, sum_all):
        """-> (rc, w [n_local, k], sigma, rho, count)"""
        m = self.mem
        n, k = idx.shape
        d_idx, d_dist, d_sum = m.put(idx, np.int32), m.put(dist, np.float32), m.put([sum_all], np.float64)
        w = m.full((n, k), np.float32, np.nan)
        sigma, rho, cnt = m.full(n, np.float32, np.nan), m.full(n, np.float32, np.nan), m.full(max(n, 1), np.int32, -1)
        p = m.ptr
        rc = self.lib.scamd_fuzzy_weights_f32(p(d_idx), p(d_dist), n, k, int(row_begin), int(n_total), p(d_sum), p(w), p(sigma), p(rho),
                                              p(cnt), m.stream)
        m.sync()
        return rc, m.get(w), m.get(sigma), m.get(rho), m.get(cnt)[:n]

    def fuzzy_merge_rows(self, idx, w, in_indptr, in_src, in_w):
        """-> (rc, indptr [n_local + 1], indices, data)"""
        m, lib = self.mem, self.lib
        n, k = idx.shape
        cap = n * (k - 1) + int(len(in_src))
        bufs = [m.put(idx, np.int32), m.put(w, np.float32), m.put(in_indptr, np.int64), m.put(in_src, np.int32), m.put(in_w, np.float32)]
        indptr = m.full(n + 1, np.int64, -1)
        indices, data = m.full(max(cap, 1), np.int32, -1), m.full(max(cap, 1), np.float32, np.nan)
        ws, wsz = self._ws(lib.scamd_fuzzy_merge_workspace_bytes(n, cap))
        nnz = C.c_int64(-1)
        p = m.ptr
        rc = lib.scamd_fuzzy_merge_rows_f32(*(p(b) for b in bufs[:2]), n, k, *(p(b) for b in bufs[2:]), p(indptr), p(indices), p(data), cap,
                                            C.byref(nnz), p(ws), wsz, m.stream)
        m.sync()
        z = max(int(nnz.value), 0)
        return rc, m.get(indptr), m.get(indices)[:z].copy(), m.get(data)[:z].copy()

    # ---- the kNN search with the cell tables it used (csrc/knn.hip: scamd_knn_debug_cell_tables; tests/knn_cell_cases.py) ----
    def knn_cell_sizes(self, n, d, n_query, k, nprobe):
        """-> (rc, cell count, upper bound of the image rows): host only"""
        nc, img = C.c_int(-1), C.c_int64(-1)
        rc = self.lib.scamd_knn_debug_cell_tables_sizes(n, d, n_query, k, int(nprobe), C.byref(nc), C.byref(img))
        return rc, int(nc.value), int(img.value)

    def knn_with_cells(self, x, k, *, nprobe=0, d=None, q_begin=0, n_query=None, ws_short=0, null_ws=False):
        """x [n, ld] float32, of which the first d columns are the data.  One search (the approximate entry when nprobe > 0), then
        the debug entry on the workspace the search left.  -> (idx, dist, n_fallback, rc of the debug entry, tables or None);
        tables: dict of numpy arrays labels, row_cell [n], cell_map, radius, tile0, ntiles [nc], cent [nc, d], order, lb2 [nc, nc],
        perm [image rows], and nc.  ws_short / null_ws: the workspace the DEBUG entry is told about (its argument checks)."""
        m, lib, p = self.mem, self.lib, self.mem.ptr
        x = np.ascontiguousarray(x, dtype=np.float32)
        n, ld = x.shape
        d = ld if d is None else d
        nq = n if n_query is None else n_query
        dx = m.put(x, np.float32)
        idx, dist = m.full((nq, k), np.int32, -7), m.full((nq, k), np.float64, np.nan)
        ws, wsz = self._ws(lib.scamd_knn_workspace_bytes(n, d, nq, k))
        nfb = C.c_int64(-1)
        if nprobe:
            rc = lib.scamd_knn_l2_ivf_f32(p(dx), n, d, ld, q_begin, nq, k, int(nprobe), p(idx), p(dist), C.byref(nfb), p(ws), wsz, m.stream)
        else:
            rc = lib.scamd_knn_l2_f32(p(dx), n, d, ld, q_begin, nq, k, p(idx), p(dist), 1.0, C.byref(nfb), p(ws), wsz, m.stream)
        m.sync()
        _check(lib, rc, "knn")
        rc, nc, img = self.knn_cell_sizes(n, d, nq, k, nprobe)
        nc_a, img_a = max(nc, 1), max(img, 1)  # (a plan without cells: the entry must refuse before it touches these)
        i32 = lambda shape: m.full(shape, np.int32, -7)  # noqa: E731
        f32 = lambda shape: m.full(shape, np.float32, np.nan)  # noqa: E731
        out = dict(labels=i32(n), row_cell=i32(n), cell_map=i32(nc_a), cent=f32((nc_a, d)), radius=f32(nc_a), tile0=i32(nc_a),
                   ntiles=i32(nc_a), order=i32((nc_a, nc_a)), lb2=f32((nc_a, nc_a)), perm=i32(img_a))
        rows = C.c_int64(-1)
        rc = lib.scamd_knn_debug_cell_tables(n, d, nq, k, int(nprobe), C.c_void_p(0) if null_ws else p(ws), max(wsz - ws_short, 0),
                                             *(p(out[key]) for key in out), C.byref(rows), m.stream)
        m.sync()
        idx, dist = m.get(idx), m.get(dist)
        if rc != 0:
            return idx, dist, int(nfb.value), rc, None
        tables = {key: m.get(a) for key, a in out.items()}
        tables["perm"] = tables["perm"][: int(rows.value)]
        tables["nc"] = nc
        return idx, dist, int(nfb.value), rc, tables

    def _csr(self, x):
        m = self.mem
        return m.put(x.indptr, np.int64), m.put(x.indices, np.int32), m.put(x.data, np.float32)

    def spmm(self, x, b, shift=None, *, l=None):
        """x: scipy CSR with sorted unique columns -> (rc, y [n, l] float32, prefilled with NaN)"""
        m = self.mem
        n, g = x.shape
        l = b.shape[1] if l is None else l
        ip, ix, dv = self._csr(x)
        d_b = m.put(b, np.float32)
        d_s = None if shift is None else m.put(shift, np.float32)
        y = m.full((n, max(l, 1)), np.float32, np.nan)
        p = m.ptr
        rc = self.lib.scamd_spmm_csr_f32(p(ip), p(ix), p(dv), n, g, p(d_b), l, p(d_s) if d_s is not None else C.c_void_p(0), p(y), m.stream)
        m.sync()
        return rc, m.get(y)

    def spmm_f64acc(self, x, b, scale=None, colsum=None, *, l=None):
        """-> (rc, w [n_rows, l] float64, prefilled with NaN)"""
        m, lib = self.mem, self.lib
        n = x.shape[0]
        l = b.shape[1] if l is None else l
        ip, ix, dv = self._csr(x)
        d_b = m.put(b, np.float32)
        d_sc = None if scale is None else m.put(scale, np.float64)
        d_cs = None if colsum is None else m.put(colsum, np.float64)
        w = m.full((n, l), np.float64, np.nan)
        ws, wsz = self._ws(lib.scamd_spmm_f64acc_workspace_bytes(n, x.nnz, l))
        p = m.ptr
        null = C.c_void_p(0)
        rc = lib.scamd_spmm_csr_f32_f64acc(p(ip), p(ix), p(dv), n, x.nnz, p(d_b), l, p(d_sc) if d_sc is not None else null,
                                           p(d_cs) if d_cs is not None else null, p(w), p(ws), wsz, m.stream)
        m.sync()
        return rc, m.get(w)

    def colsum(self, y):
        m, lib = self.mem, self.lib
        n, l = y.shape
        d_y = m.put(y, np.float32)
        out = m.full(l, np.float64, np.nan)
        ws, wsz = self._ws(lib.scamd_colsum_workspace_bytes(l))
        rc = lib.scamd_colsum_f32_f64(m.ptr(d_y), n, l, m.ptr(out), m.ptr(ws), wsz, m.stream)
        m.sync()
        return rc, m.get(out)

    def csr_transpose(self, x, *, g=None):
        """-> (rc, t_indptr [g + 1], t_indices, t_data)"""
        m, lib = self.mem, self.lib
        n = x.shape[0]
        g = x.shape[1] if g is None else g
        ip, ix, dv = self._csr(x)
        t_ip = m.full(g + 1, np.int64, -1)
        t_ix, t_dv = m.full(max(x.nnz, 1), np.int32, -1), m.full(max(x.nnz, 1), np.float32, np.nan)
        ws, wsz = self._ws(lib.scamd_csr_transpose_workspace_bytes(n, g, x.nnz))
        p = m.ptr
        rc = lib.scamd_csr_transpose_f32(p(ip), p(ix), p(dv), n, g, x.nnz, p(t_ip), p(t_ix), p(t_dv), p(ws), wsz, m.stream)
        m.sync()
        return rc, m.get(t_ip), m.get(t_ix)[: x.nnz], m.get(t_dv)[: x.nnz]

    def csr_row_stats(self, x):
        """-> (rc, row sums, row sums of squares), float64"""
        m = self.mem
        n = x.shape[0]
        ip, _, dv = self._csr(x)
        s, q = m.full(n, np.float64, np.nan), m.full(n, np.float64, np.nan)
        rc = self.lib.scamd_csr_row_stats_f32(m.ptr(ip), m.ptr(dv), n, m.ptr(s), m.ptr(q), m.stream)
        m.sync()
        return rc, m.get(s), m.get(q)

    # ---- csrc/preprocess.hip and csrc/umap.hip (tables: tests/pp_umap_kernel_cases.py) --------------------------------
    # x: scipy CSR float32.  n / g / nnz: the sizes PASSED, where they are to differ from x's (the argument checks);
    # null: names of pointer arguments passed as NULL.  Outputs are sized by x and prefilled, whatever sizes are passed.
    def _pp_in(self, x, n, nnz, null):
        self._alive = []  # the optional inputs of this call (`_opt`): referenced until the next call
        ip, ix, dv = self._csr(x)
        z, p = C.c_void_p(0), self.mem.ptr
        ptrs = [z if name in null else p(b) for name, b in (("indptr", ip), ("indices", ix), ("data", dv))]
        return (ip, ix, dv), ptrs, x.shape[0] if n is None else n, x.nnz if nnz is None else nnz

    def _opt(self, a, dtype, name="", null=()):
        """-> (buffer kept alive, pointer): NULL for None"""
        if a is None or name in null:
            return None, C.c_void_p(0)
        b = self.mem.put(a, dtype)
        self._alive.append(b)
        return b, self.mem.ptr(b)

    def pp_row_sums(self, x, col_skip=None, *, n=None, nnz=None, null=()):
        """-> (rc, out float32 [rows of x], prefilled with NaN)"""
        m = self.mem
        keep, (ip, ix, dv), n, nnz = self._pp_in(x, n, nnz, null)
        _, skip = self._opt(col_skip, np.int32)
        out = m.full(max(x.shape[0], 1), np.float32, np.nan)
        rc = self.lib.scamd_pp_row_sums_f32(ip, ix, dv, n, nnz, skip, m.ptr(out), m.stream)
        m.sync()
        return rc, m.get(out)[: x.shape[0]]

    def pp_row_count_positive(self, x, *, n=None, nnz=None, null=()):
        """-> (rc, out int32 [rows of x], prefilled with -1)"""
        m = self.mem
        keep, (ip, ix, dv), n, nnz = self._pp_in(x, n, nnz, null)
        out = m.full(max(x.shape[0], 1), np.int32, -1)
        rc = self.lib.scamd_pp_row_count_positive_f32(ip, dv, n, nnz, m.ptr(out), m.stream)
        m.sync()
        return rc, m.get(out)[: x.shape[0]]

    def pp_count_high(self, x, row_total, max_fraction, *, n=None, g=None, nnz=None, null=()):
        """-> (rc, col_counts int32 [columns of x], prefilled with -1)"""
        m = self.mem
        keep, (ip, ix, dv), n, nnz = self._pp_in(x, n, nnz, null)
        _, tot = self._opt(row_total, np.float32)
        out = m.full(max(x.shape[1], 1), np.int32, -1)
        rc = self.lib.scamd_pp_count_high_f32(ip, ix, dv, n, x.shape[1] if g is None else g, nnz, tot, float(max_fraction), m.ptr(out), m.stream)
        m.sync()
        return rc, m.get(out)[: x.shape[1]]

    def pp_row_divide(self, x, factor, *, n=None, nnz=None, null=()):
        """-> (rc, the stored values after the call)"""
        m = self.mem
        keep, (ip, ix, dv), n, nnz = self._pp_in(x, n, nnz, null)
        data = keep[2]
        _, fac = self._opt(factor, np.float32)
        rc = self.lib.scamd_pp_row_divide_f32(ip, dv, n, nnz, fac, m.stream)
        m.sync()
        return rc, m.get(data)

    def pp_log1p(self, values, offset=0, base=0.0, *, count=None, null=(), pad=7, fill=-7.0):
        """the values sit `offset` float32 elements into a 16-byte aligned buffer of `fill`, `pad` more elements of it after
        them: offset 1..3 hands the kernel a pointer that is NOT 16-byte aligned.  -> (rc, the whole buffer)"""
        m = self.mem
        values = np.asarray(values, dtype=np.float32)
        host = np.full(offset + len(values) + pad, fill, dtype=np.float32)
        host[offset: offset + len(values)] = values
        buf = m.put(host, np.float32)
        addr = m.ptr(buf).value
        assert addr % 16 == 0, "the allocator was expected to hand out 16-byte aligned buffers"
        ptr = C.c_void_p(0) if "data" in null else C.c_void_p(addr + 4 * offset)
        rc = self.lib.scamd_pp_log1p_f32(ptr, len(values) if count is None else count, float(base), m.stream)
        m.sync()
        return rc, m.get(buf)

    def pp_col_stats(self, x, row_mask=None, transform=0, tscale=1.0, *, n=None, g=None, nnz=None, null=(), want_npos=True):
        """-> (rc, sum float64 [g], sumsq float64 [g], npos [g] read as int64, or None), prefilled with NaN / -1"""
        m = self.mem
        keep, (ip, ix, dv), n, nnz = self._pp_in(x, n, nnz, null)
        g = x.shape[1] if g is None else g
        ga = max(min(g, 1 << 16), 1)
        _, mask = self._opt(row_mask, np.uint8)
        s, q = m.full(ga, np.float64, np.nan), m.full(ga, np.float64, np.nan)
        cnt = m.full(ga, np.int64, -1) if want_npos else None
        z = C.c_void_p(0)
        rc = self.lib.scamd_pp_col_stats_f32(ip, ix, dv, n, g, nnz, mask, int(transform), float(tscale), z if "sum" in null else m.ptr(s),
                                             m.ptr(q), m.ptr(cnt) if want_npos else z, m.stream)
        m.sync()
        return rc, m.get(s), m.get(q), m.get(cnt) if want_npos else None

    def pp_col_stats_clip(self, x, clip, row_mask=None, *, n=None, g=None, nnz=None, null=()):
        """-> (rc, sum float64 [g], sumsq float64 [g]), prefilled with NaN"""
        m = self.mem
        keep, (ip, ix, dv), n, nnz = self._pp_in(x, n, nnz, null)
        g = x.shape[1] if g is None else g
        ga = max(min(g, 1 << 16), 1)
        _, mask = self._opt(row_mask, np.uint8)
        _, cl = self._opt(clip, np.float64, "clip", null)
        s, q = m.full(ga, np.float64, np.nan), m.full(ga, np.float64, np.nan)
        rc = self.lib.scamd_pp_col_stats_clip_f32(ip, ix, dv, n, g, nnz, mask, cl, m.ptr(s), m.ptr(q), m.stream)
        m.sync()
        return rc, m.get(s), m.get(q)

    def pp_scale_csr(self, x, std, max_value=None, row_mask=None, *, n=None, nnz=None, null=()):
        """-> (rc, the stored values after the call)"""
        m = self.mem
        keep, (ip, ix, dv), n, nnz = self._pp_in(x, n, nnz, null)
        data = keep[2]
        _, sd = self._opt(std, np.float64)
        _, mask = self._opt(row_mask, np.uint8)
        rc = self.lib.scamd_pp_scale_csr_f32(ip, ix, dv, n, nnz, sd, float(max_value or 0.0), int(max_value is not None), mask, m.stream)
        m.sync()
        return rc, m.get(data)

    def pp_scale_dense(self, x, mean, std, max_value=None, row_mask=None, out_f64=True, *, n=None, g=None, nnz=None, null=()):
        """-> (rc, out [rows of x, columns of x] float64 | float32, prefilled with NaN)"""
        m = self.mem
        keep, (ip, ix, dv), n, nnz = self._pp_in(x, n, nnz, null)
        _, mu = self._opt(mean, np.float64)
        _, sd = self._opt(std, np.float64)
        _, mask = self._opt(row_mask, np.uint8)
        out = m.full((max(x.shape[0], 1), max(x.shape[1], 1)), np.float64 if out_f64 else np.float32, np.nan)
        rc = self.lib.scamd_pp_scale_dense_f32(ip, ix, dv, n, x.shape[1] if g is None else g, nnz, mu, sd, float(max_value or 0.0),
                                               int(max_value is not None), mask, m.ptr(out), int(out_f64), m.stream)
        m.sync()
        return rc, m.get(out)

    def umap_workspace_bytes(self, n, nnz, dim):
        return int(self.lib.scamd_umap_workspace_bytes(int(n), int(nnz), int(dim)))

    def umap_optimize(self, indptr, indices, eps, y0, *, n_epochs, a, b, gamma=1.0, initial_alpha=1.0, negative_sample_rate=5.0,
                      seed=0, dim=None, ws_short=0, null=()):
        """y0 float32 [n, dim] (`dim`: the value PASSED, where it is to differ) -> (rc, y after the call)"""
        m, lib = self.mem, self.lib
        n, d = y0.shape
        nnz = int(len(indices))
        dim = d if dim is None else dim
        ip = m.put(indptr, np.int64)
        ix, ep = m.put(indices, np.int32), m.put(eps, np.float32)
        y = m.put(y0, np.float32)
        ws, wsz = self._ws(lib.scamd_umap_workspace_bytes(n, nnz, dim), ws_short)
        z, p = C.c_void_p(0), m.ptr
        rc = lib.scamd_umap_optimize_f32(z if "indptr" in null else p(ip), p(ix), p(ep), n, nnz, dim, int(n_epochs), float(a), float(b),
                                         float(gamma), float(initial_alpha), float(negative_sample_rate), int(seed) & (2**64 - 1),
                                         z if "y" in null else p(y), p(ws), wsz, m.stream)
        m.sync()
        return rc, m.get(y)


def abi(lib) -> Abi:
    return Abi(lib, HostMem())


def _ok(lib, what, out):
    _check(lib, out[0], what)
    return out[1:] if len(out) > 2 else out[1]


def gauss_connectivities(lib, idx, dist):
    return _ok(lib, "gauss", abi(lib).connectivity("gauss", idx, dist))[:3]


def jaccard_connectivities(lib, idx):
    return _ok(lib, "jaccard", abi(lib).connectivity("jaccard", idx, np.zeros(idx.shape, np.float32)))[:3]


def fuzzy_weights(lib, idx, dist, row_begin, n_total, sum_all):
    return _ok(lib, "fuzzy_weights", abi(lib).fuzzy_weights(idx, dist, row_begin, n_total, sum_all))


def fuzzy_merge_rows(lib, idx, w, in_indptr, in_src, in_w):
    return _ok(lib, "fuzzy_merge_rows", abi(lib).fuzzy_merge_rows(idx, w, in_indptr, in_src, in_w))


def spmm(lib, x, b, shift=None):
    return _ok(lib, "spmm", abi(lib).spmm(x, b, shift))


def spmm_f64acc(lib, x, b, scale=None, colsum=None):
    return _ok(lib, "spmm_f64acc", abi(lib).spmm_f64acc(x, b, scale, colsum))


def colsum(lib, y):
    return _ok(lib, "colsum", abi(lib).colsum(y))


def csr_transpose(lib, x):
    return _ok(lib, "csr_transpose", abi(lib).csr_transpose(x))


def csr_row_stats(lib, x):
    return _ok(lib, "csr_row_stats", abi(lib).csr_row_stats(x))
