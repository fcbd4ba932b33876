"""Thin torch-tensor wrappers over the C ABI (include/scanpy_amd.h).  No arithmetic happens here."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._device import ptr, require_gpu, stream_ptr, workspace_pool

import os as _os

# SCAMD_POISON_WORKSPACE=1: the shared scratch buffer is filled with 0xAB bytes before every C call, so that a kernel
# which reads scratch it did not write fails the same way on every box (round 3: such a read showed up as a device
# fault on some boxes only)
_POISON = _os.environ.get("SCAMD_POISON_WORKSPACE") == "1"
# SCAMD_GUARD=1 (debug; round 4's hunt for the unreproduced device faults): every output tensor and every workspace handed
# to a C entry point sits between two 4 KiB guards filled with a canary byte; after the call (and a stream sync) the guards
# are read back -- a kernel that WRITES past either end of a buffer it was given raises here, naming the entry point.
_GUARD = _os.environ.get("SCAMD_GUARD") == "1"
_GUARD_BYTES = 4096
_CANARY = 0xC5
_guards: list = []  # (label, raw uint8 buffer, payload bytes) of the call in progress


def _guarded(nbytes: int, dev: torch.device, label: str) -> torch.Tensor:
    pay = (int(nbytes) + 255) // 256 * 256
    raw = torch.empty(pay + 2 * _GUARD_BYTES, dtype=torch.uint8, device=dev)
    raw[:_GUARD_BYTES] = _CANARY
    raw[_GUARD_BYTES + int(nbytes):] = _CANARY  # (the slack up to the 256-byte boundary belongs to the guard)
    _guards.append((label, raw, int(nbytes)))
    return raw[_GUARD_BYTES:_GUARD_BYTES + int(nbytes)]


def _empty(shape, *, dtype, device):
    if not _GUARD:
        return torch.empty(shape, dtype=dtype, device=device)
    shape = (int(shape),) if not isinstance(shape, (tuple, list, torch.Size)) else tuple(int(v) for v in shape)
    numel = 1
    for v in shape:
        numel *= v
    item = torch.empty((), dtype=dtype).element_size()
    return _guarded(numel * item, device, f"{dtype} {shape}").view(dtype).view(shape)


def _zeros(shape, *, dtype, device):
    t = _empty(shape, dtype=dtype, device=device)
    if _GUARD:
        t.zero_()
        return t
    return torch.zeros(shape, dtype=dtype, device=device)


def _check(rc: int, what: str = "") -> None:
    # the guard list is taken and cleared FIRST: when the C entry point reports an error the guarded buffers must not
    # stay referenced (device memory held) nor be attributed to the next, unrelated call
    pending = list(_guards)
    _guards.clear()
    _lib.check(rc, what)
    if _GUARD and pending:
        torch.cuda.synchronize()
        bad = []
        for label, raw, nbytes in pending:
            lo_ok = bool((raw[:_GUARD_BYTES] == _CANARY).all())
            hi_ok = bool((raw[_GUARD_BYTES + nbytes:] == _CANARY).all())
            if not (lo_ok and hi_ok):
                bad.append(f"{label} ({nbytes} B): {'below' if not lo_ok else ''}{' above' if not hi_ok else ''}")
        if bad:
            raise _lib.ScamdError(f"SCAMD_GUARD: {what} wrote outside " + "; ".join(bad))


def _ws(nbytes: int, dev: torch.device):
    if _GUARD:
        buf = _guarded(max(int(nbytes), 1), dev, "workspace")
        if _POISON:
            buf.fill_(0xAB)
        return buf, C.c_size_t(buf.numel())
    buf = workspace_pool.get(nbytes, dev)
    if _POISON:  # debug: every entry point must initialise what it reads (a dirty workspace is the normal case)
        buf.fill_(0xAB)
    return buf, C.c_size_t(buf.numel())


def mfma_selftest() -> None:
    require_gpu()
    _check(_lib.load().scamd_selftest_mfma_layout(stream_ptr()), "mfma selftest")


def knn(x: torch.Tensor, k: int, *, q_begin: int = 0, n_query: int | None = None, cert_scale: float = 1.0,
        nprobe: int | None = None):
    """x [n, d] float32 (device).  -> (idx int32 [nq, k], dist float64 [nq, k], n_fallback).

    nprobe: None / 0 = the exact search (scamd_knn_l2_f32); > 0 = the approximate IVF mode (scamd_knn_l2_ivf_f32): every
    query sees the rows of the `nprobe` cells nearest to its own cell only."""
    dev = require_gpu()
    lib = _lib.load()
    assert x.dtype == torch.float32 and x.dim() == 2 and x.is_cuda
    x = x.contiguous()
    n, d = x.shape
    nq = n - q_begin if n_query is None else n_query
    idx = _empty((nq, k), dtype=torch.int32, device=dev)
    dist = _empty((nq, k), dtype=torch.float64, device=dev)
    need = lib.scamd_knn_workspace_bytes(n, d, nq, k)
    if need == 0 and nq > 0:
        raise _lib.ScamdError(f"knn: unsupported shape d={d} (max 256) / k={k} (max 256)")
    ws, wsz = _ws(need, dev)
    nfb = C.c_int64(0)
    if nprobe:
        if cert_scale != 1.0:
            raise ValueError("knn: cert_scale is a test knob of the exact entry point")
        rc = lib.scamd_knn_l2_ivf_f32(ptr(x), n, d, x.stride(0), q_begin, nq, k, int(nprobe), ptr(idx), ptr(dist),
                                      C.byref(nfb), ptr(ws), wsz, stream_ptr())
        _check(rc, "scamd_knn_l2_ivf_f32")
        if lib.scamd_knn_last_nprobe() == 0:
            import warnings

            warnings.warn(f"knn: the approximate mode (nprobe={int(nprobe)}) does not take this shape (n={n}, d={d}, k={k}: it "
                          "needs n >= 4096, d <= 64, k <= 24); the search was answered EXACTLY.", UserWarning, stacklevel=3)
    else:
        rc = lib.scamd_knn_l2_f32(ptr(x), n, d, x.stride(0), q_begin, nq, k, ptr(idx), ptr(dist),
                                  float(cert_scale), C.byref(nfb), ptr(ws), wsz, stream_ptr())
        _check(rc, "scamd_knn_l2_f32")
    return idx, dist, int(nfb.value)


def knn_cert_factors(engine: int = 1):
    """the certificate's error-bound factors (cert_k, cert_k2, key_slack) of an engine, in units of u = 2^-24"""
    a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
    _lib.load().scamd_knn_cert_factors(int(engine), C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def knn_debug_b3_scores(x: torch.Tensor, q0: int, nq: int, c0: int, nc: int):
    """TEST entry: raw scores ||c||^2 - 2 q.c (centred frame) of the bf16 engine for queries [q0, q0 + nq) x candidates
    [c0, c0 + nc) (multiples of 32), through the select kernel's own packing and MFMA chain.
    -> (scores float32 [nq, nc], mu float32 [d], cmax float)"""
    dev = require_gpu()
    lib = _lib.load()
    assert x.dtype == torch.float32 and x.dim() == 2 and x.is_cuda
    x = x.contiguous()
    n, d = x.shape
    out = _empty((nq, nc), dtype=torch.float32, device=dev)
    mu = _empty(128, dtype=torch.float32, device=dev)
    cmax = _empty(1, dtype=torch.float32, device=dev)
    ws, wsz = _ws(lib.scamd_knn_debug_b3_scores_workspace_bytes(n), dev)
    rc = lib.scamd_knn_debug_b3_scores_f32(ptr(x), n, d, x.stride(0), q0, nq, c0, nc, ptr(out), ptr(mu), ptr(cmax),
                                           ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_knn_debug_b3_scores_f32")
    return out, mu[:d], float(cmax.item())


def fuzzy_simplicial_set(knn_idx: torch.Tensor, knn_dist: torch.Tensor):
    """-> (indptr int64 [n+1], indices int32 [nnz], data float32 [nnz], sigma [n], rho [n])."""
    dev = require_gpu()
    lib = _lib.load()
    n, k = knn_idx.shape
    knn_idx = knn_idx.to(torch.int32).contiguous()
    knn_dist = knn_dist.to(torch.float32).contiguous()
    cap = 2 * n * (k - 1)
    indptr = _empty(n + 1, dtype=torch.int64, device=dev)
    indices = _empty(cap, dtype=torch.int32, device=dev)
    data = _empty(cap, dtype=torch.float32, device=dev)
    sigma = _empty(n, dtype=torch.float32, device=dev)
    rho = _empty(n, dtype=torch.float32, device=dev)
    ws, wsz = _ws(lib.scamd_fuzzy_workspace_bytes(n, k), dev)
    nnz = C.c_int64(0)
    rc = lib.scamd_fuzzy_simplicial_set_f32(ptr(knn_idx), ptr(knn_dist), n, k, ptr(indptr), ptr(indices), ptr(data),
                                            cap, ptr(sigma), ptr(rho), C.byref(nnz), ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_fuzzy_simplicial_set_f32")
    m = int(nnz.value)
    return indptr, indices[:m], data[:m], sigma, rho


def fuzzy_weights(knn_idx: torch.Tensor, knn_dist: torch.Tensor, row_begin: int, n_total: int, sum_all: torch.Tensor):
    """membership strengths of a rank's own rows (row-sharded fuzzy set, step 1).  knn_idx holds global row ids;
    sum_all = device float64 [1], the sum of all n_total * k distances.  -> w float32 [n_local, k] (0 = absent)"""
    dev = require_gpu()
    n, k = knn_idx.shape
    knn_idx = knn_idx.to(torch.int32).contiguous()
    knn_dist = knn_dist.to(torch.float32).contiguous()
    sum_all = sum_all.to(torch.float64).contiguous()
    w = _empty((n, k), dtype=torch.float32, device=dev)
    cnt = _empty(max(n, 1), dtype=torch.int32, device=dev)
    _check(_lib.load().scamd_fuzzy_weights_f32(ptr(knn_idx), ptr(knn_dist), n, k, int(row_begin), int(n_total),
                                                   ptr(sum_all), ptr(w), None, None, ptr(cnt), stream_ptr()),
               "scamd_fuzzy_weights_f32")
    return w


def fuzzy_merge_rows(knn_idx: torch.Tensor, w: torch.Tensor, in_indptr: torch.Tensor, in_src: torch.Tensor,
                     in_w: torch.Tensor):
    """symmetrised rows of a rank (row-sharded fuzzy set, step 3) from its out-edges (knn_idx, w) and the in-edges the
    other ranks sent, sorted by (row, source).  -> (indptr int64 [n_local + 1], indices int32 (global), data float32)"""
    dev = require_gpu()
    lib = _lib.load()
    n, k = knn_idx.shape
    knn_idx = knn_idx.to(torch.int32).contiguous()
    w = w.to(torch.float32).contiguous()
    in_indptr = in_indptr.to(torch.int64).contiguous()
    in_src = in_src.to(torch.int32).contiguous()
    in_w = in_w.to(torch.float32).contiguous()
    cap = n * (k - 1) + int(in_src.numel())
    indptr = _empty(n + 1, dtype=torch.int64, device=dev)
    indices = _empty(max(cap, 1), dtype=torch.int32, device=dev)
    data = _empty(max(cap, 1), dtype=torch.float32, device=dev)
    ws, wsz = _ws(lib.scamd_fuzzy_merge_workspace_bytes(n, cap), dev)
    nnz = C.c_int64(0)
    rc = lib.scamd_fuzzy_merge_rows_f32(ptr(knn_idx), ptr(w), n, k, ptr(in_indptr), ptr(in_src), ptr(in_w), ptr(indptr),
                                        ptr(indices), ptr(data), cap, C.byref(nnz), ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_fuzzy_merge_rows_f32")
    return indptr, indices[: nnz.value], data[: nnz.value]


def _knn_graph(entry: str, knn_idx: torch.Tensor, knn_dist: torch.Tensor | None):
    """shared driver of the gauss / jaccard connectivity kernels -> (indptr int64, indices int32, data float32)"""
    dev = require_gpu()
    lib = _lib.load()
    n, k = knn_idx.shape
    knn_idx = knn_idx.to(torch.int32).contiguous()
    cap = 2 * n * (k - 1)
    indptr = _empty(n + 1, dtype=torch.int64, device=dev)
    indices = _empty(cap, dtype=torch.int32, device=dev)
    data = _empty(cap, dtype=torch.float32, device=dev)
    ws, wsz = _ws(lib.scamd_fuzzy_workspace_bytes(n, k), dev)
    nnz = C.c_int64(0)
    if entry == "gauss":
        knn_dist = knn_dist.to(torch.float32).contiguous()
        rc = lib.scamd_gauss_connectivities_f32(ptr(knn_idx), ptr(knn_dist), n, k, ptr(indptr), ptr(indices), ptr(data), cap,
                                                C.byref(nnz), ptr(ws), wsz, stream_ptr())
    else:
        rc = lib.scamd_jaccard_connectivities_f32(ptr(knn_idx), n, k, ptr(indptr), ptr(indices), ptr(data), cap,
                                                  C.byref(nnz), ptr(ws), wsz, stream_ptr())
    _check(rc, f"scamd_{entry}_connectivities_f32")
    m = int(nnz.value)
    return indptr, indices[:m], data[:m]


def gauss_connectivities(knn_idx: torch.Tensor, knn_dist: torch.Tensor):
    return _knn_graph("gauss", knn_idx, knn_dist)


def jaccard_connectivities(knn_idx: torch.Tensor):
    return _knn_graph("jaccard", knn_idx, None)


def csr_transpose(indptr: torch.Tensor, indices: torch.Tensor, data: torch.Tensor, n: int, g: int):
    dev = require_gpu()
    lib = _lib.load()
    nnz = data.numel()
    t_indptr = _empty(g + 1, dtype=torch.int64, device=dev)
    t_indices = _empty(nnz, dtype=torch.int32, device=dev)
    t_data = _empty(nnz, dtype=torch.float32, device=dev)
    ws, wsz = _ws(lib.scamd_csr_transpose_workspace_bytes(n, g, nnz), dev)
    rc = lib.scamd_csr_transpose_f32(ptr(indptr), ptr(indices), ptr(data), n, g, nnz, ptr(t_indptr), ptr(t_indices),
                                     ptr(t_data), ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_csr_transpose_f32")
    return t_indptr, t_indices, t_data


def csr_row_stats(indptr: torch.Tensor, data: torch.Tensor, n_rows: int):
    dev = require_gpu()
    s = _empty(n_rows, dtype=torch.float64, device=dev)
    q = _empty(n_rows, dtype=torch.float64, device=dev)
    _check(_lib.load().scamd_csr_row_stats_f32(ptr(indptr), ptr(data), n_rows, ptr(s), ptr(q), stream_ptr()),
               "scamd_csr_row_stats_f32")
    return s, q


def csr_absmax(indptr, indices, data, n: int, g: int) -> float:
    """max |x| over the stored entries (phase 1 of the Gram computation)."""
    dev = require_gpu()
    lib = _lib.load()
    ws, wsz = _ws(lib.scamd_csr_gram_workspace_bytes(n, g), dev)
    mx = C.c_float(0.0)
    rc = lib.scamd_csr_gram_f32(ptr(indptr), ptr(indices), ptr(data), n, g, data.numel(), 0, None, 0, None,
                                C.byref(mx), ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_csr_gram_f32 (absmax)")
    return float(mx.value)


def csr_gram(indptr, indices, data, n: int, g: int, scale_bits: int):
    """-> (gram int64 [g_pad, g_pad], colsum int64 [g_pad]) in fixed point (x 2^scale_bits), g_pad = ceil128(g)."""
    dev = require_gpu()
    lib = _lib.load()
    gp = (g + 127) // 128 * 128
    gram = _empty((gp, gp), dtype=torch.int64, device=dev)
    colsum = _empty(gp, dtype=torch.int64, device=dev)
    ws, wsz = _ws(lib.scamd_csr_gram_workspace_bytes(n, g), dev)
    rc = lib.scamd_csr_gram_f32(ptr(indptr), ptr(indices), ptr(data), n, g, data.numel(), int(scale_bits), ptr(gram),
                                gp, ptr(colsum), None, ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_csr_gram_f32")
    return gram, colsum


def spmm(indptr, indices, data, n: int, g: int, b: torch.Tensor, shift: torch.Tensor | None = None) -> torch.Tensor:
    """Y[n, l] = A B - 1 shift^T, float32."""
    dev = require_gpu()
    b = b.to(torch.float32).contiguous()
    assert b.shape[0] == g
    l = b.shape[1]
    y = _empty((n, l), dtype=torch.float32, device=dev)
    if shift is not None:
        shift = shift.to(torch.float32).contiguous()
    _check(_lib.load().scamd_spmm_csr_f32(ptr(indptr), ptr(indices), ptr(data), n, g, ptr(b), l, ptr(shift),
                                              ptr(y), stream_ptr()), "scamd_spmm_csr_f32")
    return y


def spmm_f64acc(indptr, indices, data, n_rows: int, b: torch.Tensor, scale: torch.Tensor | None = None,
                colsum: torch.Tensor | None = None) -> torch.Tensor:
    """W[n_rows, l] float64 = A B (float64 accumulation) - scale colsum^T."""
    dev = require_gpu()
    lib = _lib.load()
    assert b.dtype == torch.float32 and b.is_contiguous()
    l = b.shape[1]
    nnz = data.numel()
    w = _empty((n_rows, l), dtype=torch.float64, device=dev)
    ws, wsz = _ws(lib.scamd_spmm_f64acc_workspace_bytes(n_rows, nnz, l), dev)
    rc = lib.scamd_spmm_csr_f32_f64acc(ptr(indptr), ptr(indices), ptr(data), n_rows, nnz, ptr(b), l, ptr(scale),
                                       ptr(colsum), ptr(w), ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_spmm_csr_f32_f64acc")
    return w


def dense_debug(op: int, in0: torch.Tensor, in1: torch.Tensor | None = None):
    """building blocks of the dense eigensolver on caller buffers (csrc/dense.hip; tests).  op 1: in0^T in1;
    op 2: CholeskyQR factor of a Gram matrix -> (S, pivot_failed); op 3: Jacobi eigh -> (theta, Y, sweeps);
    op 4: the panel product in0 [m, b] @ in1 [b, n] (b, n <= 128); op 5: two panels stacked in in0 [2 m, b] by the same in1 in one
    launch -> (out0, out1); op 6: op 3 on the symmetrised in0, (in0 + in0^T) / 2 formed by the kernel's load."""
    dev = require_gpu()
    lib = _lib.load()
    in0 = in0.to(torch.float64).contiguous()
    flag = C.c_int(0)
    if op == 1:
        in1 = in1.to(torch.float64).contiguous()
        kdim, m = in0.shape
        n = in1.shape[1]
        out = _empty((m, n), dtype=torch.float64, device=dev)
        rc = lib.scamd_dense_debug_f64(1, ptr(in0), ptr(in1), m, n, kdim, ptr(out), None, C.byref(flag), stream_ptr())
        _check(rc, "scamd_dense_debug_f64")
        return out
    if op == 4:
        in1 = in1.to(torch.float64).contiguous()
        m, kdim = in0.shape
        n = in1.shape[1]
        out = _empty((m, n), dtype=torch.float64, device=dev)
        rc = lib.scamd_dense_debug_f64(4, ptr(in0), ptr(in1), m, n, kdim, ptr(out), None, C.byref(flag), stream_ptr())
        _check(rc, "scamd_dense_debug_f64")
        return out
    if op == 5:
        in1 = in1.to(torch.float64).contiguous()
        m, kdim = in0.shape[0] // 2, in0.shape[1]
        n = in1.shape[1]
        out0, out1 = (_empty((m, n), dtype=torch.float64, device=dev) for _ in range(2))
        rc = lib.scamd_dense_debug_f64(5, ptr(in0), ptr(in1), m, n, kdim, ptr(out0), ptr(out1), C.byref(flag), stream_ptr())
        _check(rc, "scamd_dense_debug_f64")
        return out0, out1
    m = in0.shape[0]
    out0 = _empty((m, m) if op == 2 else (m,), dtype=torch.float64, device=dev)
    out1 = _empty((m, m), dtype=torch.float64, device=dev)
    rc = lib.scamd_dense_debug_f64(op, ptr(in0), None, m, m, m, ptr(out0), ptr(out1), C.byref(flag), stream_ptr())
    _check(rc, "scamd_dense_debug_f64")
    return (out0, int(flag.value)) if op == 2 else (out0, out1, int(flag.value))


def eigh_topk(a: torch.Tensor, k: int, *, seed: int = 0, tol: float = 2e-8):
    """Top-k eigenpairs of the symmetric PSD float64 matrix a [g, g] -> (lam [k] descending, v [g, k], info dict).
    Raises ScamdError (SCAMD_EUNSUPPORTED) outside the device solver's range or when it does not converge."""
    dev = require_gpu()
    lib = _lib.load()
    assert a.dtype == torch.float64 and a.dim() == 2 and a.shape[0] == a.shape[1] and a.is_cuda
    a = a.contiguous()
    g = a.shape[0]
    lam = _empty(k, dtype=torch.float64, device=dev)
    v = _empty((g, k), dtype=torch.float64, device=dev)
    info = (C.c_int32 * 12)()
    need = lib.scamd_eigh_topk_workspace_bytes(g, k)
    ws, wsz = _ws(need, dev)
    rc = lib.scamd_eigh_topk_f64(ptr(a), g, a.stride(0), k, int(seed) & (2**64 - 1), float(tol), ptr(lam), ptr(v), info,
                                 ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_eigh_topk_f64")
    resid = C.cast(C.byref(info, 16), C.POINTER(C.c_double))[0]
    return lam, v, {"n_outer": info[0], "n_gemm": info[1], "block_size": info[2], "chol_retries": info[3], "residual": resid}


def pca_csr(indptr, indices, data, n: int, g: int, n_comps: int, *, zero_center: bool = True, seed: int = 0,
            tol: float = 2e-8):
    """`scamd_pca_csr_f32`: the whole Gram-route PCA of a resident CSR matrix in one C call.
    -> (scores f32 [n, k], components f64 [k, g], variance [k], variance_ratio [k], mean [g], info dict)"""
    dev = require_gpu()
    lib = _lib.load()
    k = int(n_comps)
    scores = _empty((n, k), dtype=torch.float32, device=dev)
    comps = _empty((k, g), dtype=torch.float64, device=dev)
    var = _empty(k, dtype=torch.float64, device=dev)
    ratio = _empty(k, dtype=torch.float64, device=dev)
    mean = _empty(g, dtype=torch.float64, device=dev)
    info = (C.c_int32 * 12)()
    need = lib.scamd_pca_csr_workspace_bytes(n, g, k)
    ws, wsz = _ws(need, dev)
    rc = lib.scamd_pca_csr_f32(ptr(indptr), ptr(indices), ptr(data), n, g, data.numel(), k, 1 if zero_center else 0,
                               int(seed) & (2**64 - 1), float(tol), ptr(scores), ptr(comps), ptr(var), ptr(ratio), ptr(mean),
                               info, ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_pca_csr_f32")
    resid = C.cast(C.byref(info, 16), C.POINTER(C.c_double))[0]
    return scores, comps, var, ratio, mean, {"n_outer": info[0], "n_gemm": info[1], "block_size": info[2],
                                             "chol_retries": info[3], "residual": resid, "scale_bits": info[6]}


def pca_solve_gram(gram_q: torch.Tensor, colsum_q: torch.Tensor, n_total: int, g: int, scale_bits: int, n_comps: int, *,
                   zero_center: bool = True, seed: int = 0, tol: float = 2e-8):
    """`scamd_pca_solve_gram_f64`: the dense half of the Gram route in one C call (no torch arithmetic): int64 Gram matrix
    [gp, gp] + column sums -> (components f64 [k, g], loadings f32 [g, k], shift f32 [k], variance [k], ratio [k],
    mean f64 [g], eigenvalues f64 [k], info)."""
    dev = require_gpu()
    lib = _lib.load()
    k = int(n_comps)
    assert gram_q.dtype == torch.int64 and gram_q.is_contiguous() and colsum_q.dtype == torch.int64
    comps = _empty((k, g), dtype=torch.float64, device=dev)
    v32 = _empty((g, k), dtype=torch.float32, device=dev)
    shift = _empty(k, dtype=torch.float32, device=dev)
    var = _empty(k, dtype=torch.float64, device=dev)
    ratio = _empty(k, dtype=torch.float64, device=dev)
    mean = _empty(g, dtype=torch.float64, device=dev)
    lam = _empty(k, dtype=torch.float64, device=dev)
    info = (C.c_int32 * 12)()
    ws, wsz = _ws(lib.scamd_pca_solve_gram_workspace_bytes(g, k), dev)
    rc = lib.scamd_pca_solve_gram_f64(ptr(gram_q), gram_q.shape[1], ptr(colsum_q), int(n_total), g, int(scale_bits), k,
                                      1 if zero_center else 0, int(seed) & (2**64 - 1), float(tol), ptr(comps), ptr(v32),
                                      ptr(shift), ptr(var), ptr(ratio), ptr(mean), ptr(lam), info, ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_pca_solve_gram_f64")
    resid = C.cast(C.byref(info, 16), C.POINTER(C.c_double))[0]
    return comps, v32, shift, var, ratio, mean, lam, {"n_outer": info[0], "n_gemm": info[1], "block_size": info[2],
                                                       "chol_retries": info[3], "residual": resid}


def spectral_embedding(indptr: torch.Tensor, indices: torch.Tensor, weights: torch.Tensor, n: int, dim: int, *, seed: int = 0,
                       tol: float = 2e-6, max_outer: int = 60, max_degree: int = 64):
    """`scamd_spectral_embedding_f32`: the `dim` eigenvectors of D^-1/2 A D^-1/2 below the trivial one, float64 [n, dim] on the
    device, + info (outer_iterations, operator_applications, residual, converged, ritz_values)."""
    dev = require_gpu()
    lib = _lib.load()
    indptr = indptr.to(torch.int64).contiguous()
    indices = indices.to(torch.int32).contiguous()
    weights = weights.to(torch.float32).contiguous()
    nnz = weights.numel()
    out = _empty((n, dim), dtype=torch.float64, device=dev)
    need = lib.scamd_spectral_embedding_workspace_bytes(n, nnz, int(dim))
    if need == 0:
        raise _lib.ScamdError(f"spectral_embedding: unsupported shape n={n} dim={dim} (at most 10 components)")
    ws, wsz = _ws(need, dev)
    info = (C.c_double * 8)()
    rc = lib.scamd_spectral_embedding_f32(ptr(indptr), ptr(indices), ptr(weights), n, nnz, int(dim), int(seed) & (2**64 - 1),
                                          float(tol), int(max_outer), int(max_degree), ptr(out), info, ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_spectral_embedding_f32")
    return out, {"outer_iterations": int(info[0]), "operator_applications": int(info[1]), "residual": float(info[2]),
                 "converged": bool(info[3] > 0.5), "ritz_values": [float(info[4 + j]) for j in range(min(dim, 4))]}


def transitions_sym(indptr: torch.Tensor, indices: torch.Tensor, weights: torch.Tensor, n: int, *, density_normalize: bool = True):
    """`scamd_transitions_sym_f32`: T_sym on the pattern of the symmetric graph (float32 [nnz]) and z (float64 [n]), on the device."""
    dev = require_gpu()
    lib = _lib.load()
    indptr = indptr.to(torch.int64).contiguous()
    indices = indices.to(torch.int32).contiguous()
    weights = weights.to(torch.float32).contiguous()
    nnz = weights.numel()
    t_sym = _empty(nnz, dtype=torch.float32, device=dev)
    z = _empty(n, dtype=torch.float64, device=dev)
    ws, wsz = _ws(lib.scamd_transitions_sym_workspace_bytes(n, nnz), dev)
    rc = lib.scamd_transitions_sym_f32(ptr(indptr), ptr(indices), ptr(weights), n, nnz, 1 if density_normalize else 0, ptr(t_sym),
                                       ptr(z), ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_transitions_sym_f32")
    return t_sym, z


def diffmap(indptr: torch.Tensor, indices: torch.Tensor, t_sym: torch.Tensor, n: int, n_comps: int, *, seed: int = 0,
            tol: float = 2e-6, max_outer: int = 60, max_degree: int = 64):
    """`scamd_diffmap_f32`: the `n_comps` leading eigenpairs of T_sym -> (evals float64 [n_comps], evecs float64 [n, n_comps]) on
    the device + info (`_lib.diffmap_info`).  NotImplementedError when the largest-magnitude guard refuses the graph."""
    dev = require_gpu()
    lib = _lib.load()
    indptr = indptr.to(torch.int64).contiguous()
    indices = indices.to(torch.int32).contiguous()
    t_sym = t_sym.to(torch.float32).contiguous()
    nnz = t_sym.numel()
    need = lib.scamd_diffmap_workspace_bytes(n, nnz, int(n_comps))
    if need == 0:
        raise _lib.ScamdError(f"diffmap: unsupported shape n={n} n_comps={n_comps} (1 to 26 components)")
    evals = _empty(int(n_comps), dtype=torch.float64, device=dev)
    evecs = _empty((n, int(n_comps)), dtype=torch.float64, device=dev)
    ws, wsz = _ws(need, dev)
    info = (C.c_double * _lib.DIFFMAP_INFO_WORDS)()
    rc = lib.scamd_diffmap_f32(ptr(indptr), ptr(indices), ptr(t_sym), n, nnz, int(n_comps), int(seed) & (2**64 - 1), float(tol),
                               int(max_outer), int(max_degree), ptr(evals), ptr(evecs), info, ptr(ws), wsz, stream_ptr())
    refused = _lib.diffmap_guard_error(rc, info, int(n_comps))
    if refused is not None:
        _guards.clear()
        raise refused
    _check(rc, "scamd_diffmap_f32")
    return evals, evecs, _lib.diffmap_info(info)


def dpt_pseudotime(evals: torch.Tensor, basis: torch.Tensor, iroot: int, labels: torch.Tensor | None = None, *,
                   scale: bool = True) -> torch.Tensor:
    """`scamd_dpt_pseudotime_f32`: evals float32 [n_dcs], basis float32 [n, ld >= n_dcs], labels int32 [n] or None -> float32 [n]:
    the DPT distances from `iroot`, divided by their largest finite value when `scale` (the pseudotime)."""
    dev = require_gpu()
    lib = _lib.load()
    assert evals.dtype == torch.float32 and basis.dtype == torch.float32 and basis.dim() == 2
    evals, basis = evals.contiguous(), basis.contiguous()
    n, ld = basis.shape
    if labels is not None:
        labels = labels.to(torch.int32).contiguous()
    out = _empty(n, dtype=torch.float32, device=dev)
    ws, wsz = _ws(lib.scamd_dpt_pseudotime_workspace_bytes(n), dev)
    rc = lib.scamd_dpt_pseudotime_f32(ptr(evals), ptr(basis), n, evals.numel(), ld, int(iroot), ptr(labels), 1 if scale else 0,
                                      ptr(out), ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_dpt_pseudotime_f32")
    return out


def colsum(y: torch.Tensor) -> torch.Tensor:
    dev = require_gpu()
    lib = _lib.load()
    assert y.dtype == torch.float32 and y.is_contiguous()
    n, l = y.shape
    out = _empty(l, dtype=torch.float64, device=dev)
    ws, wsz = _ws(lib.scamd_colsum_workspace_bytes(l), dev)
    _check(lib.scamd_colsum_f32_f64(ptr(y), n, l, ptr(out), ptr(ws), wsz, stream_ptr()), "scamd_colsum_f32_f64")
    return out


def leiden(indptr: torch.Tensor, indices: torch.Tensor, weights: torch.Tensor, n: int, *, resolution: float = 1.0,
           n_iterations: int = -1, beta: float = 0.01, seed: int = 0, initial_membership: torch.Tensor | None = None,
           objective: str = "modularity", node_weights: torch.Tensor | None = None):
    """Symmetric CSR graph on device -> (membership int32 [n] on device, modularity, n_communities).
    `initial_membership` (int32 [n] on the device, ids in [0, n)): start from that partition instead of singletons.
    `objective`: 'modularity' (resolution normalised by 2m, vertex weight = strength) or 'cpm' (igraph's CPM: vertex weight
    1, resolution as given; the returned float is then the resolution-1 modularity of the partition).
    `node_weights` (float32 [n] in [0, 1e6], CPM only): igraph's `node_weights` -- a community pays resolution x (sum of its
    members' weights)^2."""
    dev = require_gpu()
    lib = _lib.load()
    indptr = indptr.to(torch.int64).contiguous()
    indices = indices.to(torch.int32).contiguous()
    weights = weights.to(torch.float32).contiguous()
    nnz = weights.numel()
    memb = _empty(n, dtype=torch.int32, device=dev)
    ws, wsz = _ws(lib.scamd_leiden_workspace_bytes(n, nnz), dev)
    q = C.c_double(0.0)
    nc = C.c_int32(0)
    init = None
    if initial_membership is not None:
        init = initial_membership.to(device=dev, dtype=torch.int32).contiguous()
        if init.numel() != n:
            raise ValueError(f"initial_membership has {init.numel()} entries for {n} vertices")
    if objective.lower() not in ("modularity", "cpm"):
        raise ValueError(f"objective={objective!r}: 'modularity' or 'cpm'")
    nw = None
    if node_weights is not None:
        if objective.lower() != "cpm":
            raise NotImplementedError("node_weights with the modularity objective (its vertex weights are the strengths)")
        nw = node_weights.to(device=dev, dtype=torch.float32).contiguous()
        if nw.numel() != n:
            raise ValueError(f"node_weights has {nw.numel()} entries for {n} vertices")
    # (the entry that takes everything: NULL node weights / initial membership are the other three)
    rc = lib.scamd_leiden_csr_nw_f32(ptr(indptr), ptr(indices), ptr(weights), n, nnz, float(resolution),
                                     int(n_iterations), float(beta), int(seed) & (2**64 - 1), int(objective.lower() == "cpm"),
                                     ptr(nw), ptr(init), ptr(memb), C.byref(q), C.byref(nc), ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_leiden_csr_nw_f32")
    return memb, float(q.value), int(nc.value)


def leiden_last_stats() -> dict:
    """Diagnostics of this thread's last `leiden` call (scamd_leiden_last_stats)."""
    lib = _lib.load()
    keys = _lib.leiden_stat_names(lib)
    out = (C.c_int32 * len(keys))()
    lib.scamd_leiden_last_stats(out, len(keys))
    return {k: int(v) for k, v in zip(keys, out) if k is not None}


def leiden_tier_bounds(lanes: int):
    """longest rows (main_max, wave_max, block_max) of the tiers of a Leiden decide step at `lanes` lanes per vertex"""
    a, b, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _check(_lib.load().scamd_leiden_tier_bounds(int(lanes), C.byref(a), C.byref(b), C.byref(c)), "scamd_leiden_tier_bounds")
    return a.value, b.value, c.value


LEVEL_INFO_KEYS = ("merges", "n_coarse", "coarse_nnz", "n_mid", "n_big", "n_split", "skipped")


def leiden_debug_level(indptr: torch.Tensor, indices: torch.Tensor, weights: torch.Tensor, n: int, membership: torch.Tensor, *,
                       refined_in: torch.Tensor | None = None, resolution: float = 1.0, beta: float = 0.01, seed: int = 0) -> dict:
    """Test entry scamd_leiden_debug_level_f32: the refinement of `membership` (skipped when `refined_in` is given) and the
    coarse graph under the refined partition -> dict of device tensors (refined, Kref, Eref, refsize, and, unless `skipped`, cid,
    indptr, indices, wq, k, comm cut to their lengths) plus the integers of LEVEL_INFO_KEYS."""
    dev = require_gpu()
    lib = _lib.load()
    indptr = indptr.to(torch.int64).contiguous()
    indices = indices.to(torch.int32).contiguous()
    weights = weights.to(torch.float32).contiguous()
    membership = membership.to(device=dev, dtype=torch.int32).contiguous()
    given = None if refined_in is None else refined_in.to(device=dev, dtype=torch.int32).contiguous()
    if membership.numel() != n or (given is not None and given.numel() != n):
        raise ValueError(f"membership / refined_in must have {n} entries")
    nnz = weights.numel()
    i32 = lambda m: _empty(max(m, 1), dtype=torch.int32, device=dev)  # noqa: E731
    i64 = lambda m: _empty(max(m, 1), dtype=torch.int64, device=dev)  # noqa: E731
    out = dict(refined=i32(n), Kref=i64(n), Eref=i64(n), refsize=i32(n), cid=i32(n), indptr=i64(n + 1), indices=i32(nnz), wq=i64(nnz),
               k=i64(n), comm=i32(n))
    ws, wsz = _ws(lib.scamd_leiden_workspace_bytes(n, nnz), dev)
    info = (C.c_int64 * 8)()
    rc = lib.scamd_leiden_debug_level_f32(ptr(indptr), ptr(indices), ptr(weights), n, nnz, ptr(membership), ptr(given), float(resolution),
                                          float(beta), int(seed) & (2**64 - 1), *(ptr(out[key]) for key in out), info, ptr(ws), wsz,
                                          stream_ptr())
    _check(rc, "scamd_leiden_debug_level_f32")
    res = dict(zip(LEVEL_INFO_KEYS, (int(v) for v in info)))
    nn, ne = res["n_coarse"], res["coarse_nnz"]
    cut = dict(refined=n, Kref=n, Eref=n, refsize=n, cid=n, indptr=nn + 1, indices=ne, wq=ne, k=nn, comm=nn)
    for key, m in cut.items():
        if not res["skipped"] or key in ("refined", "Kref", "Eref", "refsize"):
            res[key] = out[key][:m]
    return res


LEIDEN_COUNTS_WORDS = 32 + 16 * 32  # counts_host of scamd_leiden_debug_counters_f32: class list lengths, then 16 words per class


def leiden_debug_counters(indptr: torch.Tensor, indices: torch.Tensor, weights: torch.Tensor, n: int, membership: torch.Tensor,
                          decision: torch.Tensor, *, flags: torch.Tensor | None = None, n_cls: int = 8, salt: int = 0) -> dict:
    """Test entry scamd_leiden_debug_counters_f32: the community totals of `membership`, the class lists of one sweep over the
    flagged vertices (`flags` None: all) and one apply step per class with `decision` (per vertex: >= 0 move there, -2 blocked)
    -> dict of device tensors (lists, tier_lists [n_cls, n], giant_lists [n_cls, S], Ktot_before, csize_before, comm_after,
    Ktot_after, csize_after, flags_after [n]) plus the lists list_len [n_cls], tier_len [n_cls][3] and the integers moved,
    blocked, giant_stride, lanes."""
    dev = require_gpu()
    lib = _lib.load()
    indptr = indptr.to(torch.int64).contiguous()
    indices = indices.to(torch.int32).contiguous()
    weights = weights.to(torch.float32).contiguous()
    membership = membership.to(device=dev, dtype=torch.int32).contiguous()
    decision = decision.to(device=dev, dtype=torch.int32).contiguous()
    given = None if flags is None else flags.to(device=dev, dtype=torch.int32).contiguous()
    if membership.numel() != n or decision.numel() != n or (given is not None and given.numel() != n):
        raise ValueError(f"membership / decision / flags must have {n} entries")
    nnz = weights.numel()
    stride = nnz // (leiden_tier_bounds(64)[2] + 1) + 1
    i32 = lambda m: _empty(max(m, 1), dtype=torch.int32, device=dev)  # noqa: E731
    i64 = lambda m: _empty(max(m, 1), dtype=torch.int64, device=dev)  # noqa: E731
    out = dict(lists=i32(n_cls * n), tier_lists=i32(n_cls * n), giant_lists=i32(n_cls * stride), Ktot_before=i64(n), csize_before=i32(n),
               comm_after=i32(n), Ktot_after=i64(n), csize_after=i32(n), flags_after=i32(n))
    ws, wsz = _ws(lib.scamd_leiden_workspace_bytes(n, nnz), dev)
    counts = (C.c_int32 * LEIDEN_COUNTS_WORDS)()
    info = (C.c_int64 * 4)()
    rc = lib.scamd_leiden_debug_counters_f32(ptr(indptr), ptr(indices), ptr(weights), n, nnz, ptr(membership), ptr(given), int(n_cls),
                                             int(salt) & 0xFFFFFFFF, ptr(decision), *(ptr(out[key]) for key in out), counts, info,
                                             ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_leiden_debug_counters_f32")
    res = {key: (val[:n] if key.endswith(("before", "after")) else val.view(n_cls, -1)) for key, val in out.items()}
    res["list_len"] = [int(v) for v in counts[:n_cls]]
    res["tier_len"] = [[int(counts[32 + 16 * c + 8 + t]) for t in range(3)] for c in range(n_cls)]
    res.update(moved=int(info[0]), blocked=int(info[1]), giant_stride=int(info[2]), lanes=int(info[3]))
    assert res["giant_stride"] == stride
    return res


def modularity(indptr: torch.Tensor, indices: torch.Tensor, weights: torch.Tensor, n: int, membership: torch.Tensor,
               *, resolution: float = 1.0) -> float:
    dev = require_gpu()
    lib = _lib.load()
    indptr = indptr.to(torch.int64).contiguous()
    indices = indices.to(torch.int32).contiguous()
    weights = weights.to(torch.float32).contiguous()
    membership = membership.to(torch.int32).contiguous()
    nnz = weights.numel()
    ws, wsz = _ws(lib.scamd_leiden_workspace_bytes(n, nnz), dev)
    q = C.c_double(0.0)
    rc = lib.scamd_modularity_csr_f32(ptr(indptr), ptr(indices), ptr(weights), n, nnz, ptr(membership),
                                      float(resolution), C.byref(q), ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_modularity_csr_f32")
    return float(q.value)


# ---- upstream normalisation chain (csrc/preprocess.hip) ---------------------------------------------------------
def pp_row_sums(indptr, indices, data, n: int, col_skip: torch.Tensor | None = None) -> torch.Tensor:
    dev = require_gpu()
    out = _empty(n, dtype=torch.float32, device=dev)
    rc = _lib.load().scamd_pp_row_sums_f32(ptr(indptr), ptr(indices), ptr(data), n, data.numel(), ptr(col_skip), ptr(out), stream_ptr())
    _check(rc, "scamd_pp_row_sums_f32")
    return out


def pp_row_count_positive(indptr, data, n: int) -> torch.Tensor:
    dev = require_gpu()
    out = _empty(n, dtype=torch.int32, device=dev)
    _check(_lib.load().scamd_pp_row_count_positive_f32(ptr(indptr), ptr(data), n, data.numel(), ptr(out), stream_ptr()),
               "scamd_pp_row_count_positive_f32")
    return out


def pp_count_high(indptr, indices, data, n: int, g: int, row_total: torch.Tensor, max_fraction: float) -> torch.Tensor:
    dev = require_gpu()
    counts = _empty(g, dtype=torch.int32, device=dev)
    rc = _lib.load().scamd_pp_count_high_f32(ptr(indptr), ptr(indices), ptr(data), n, g, data.numel(), ptr(row_total),
                                             float(max_fraction), ptr(counts), stream_ptr())
    _check(rc, "scamd_pp_count_high_f32")
    return counts


def pp_row_divide_(indptr, data, n: int, factor: torch.Tensor) -> None:
    require_gpu()
    assert factor.dtype == torch.float32 and factor.numel() == n
    _check(_lib.load().scamd_pp_row_divide_f32(ptr(indptr), ptr(data), n, data.numel(), ptr(factor), stream_ptr()),
               "scamd_pp_row_divide_f32")


def pp_log1p_(data: torch.Tensor, base: float | None = None) -> None:
    require_gpu()
    assert data.dtype == torch.float32 and data.is_contiguous()
    _check(_lib.load().scamd_pp_log1p_f32(ptr(data), data.numel(), 0.0 if base is None else float(base), stream_ptr()),
               "scamd_pp_log1p_f32")


def pp_col_stats(indptr, indices, data, n: int, g: int, *, row_mask: torch.Tensor | None = None, expm1_scale: float | None = None,
                 count_positive: bool = True):
    """-> (sum float64 [g], sumsq float64 [g], npos int64 [g] or None) over the masked rows; expm1_scale = s: of
    expm1(x * s)."""
    dev = require_gpu()
    s = _empty(g, dtype=torch.float64, device=dev)
    sq = _empty(g, dtype=torch.float64, device=dev)
    npos = _empty(g, dtype=torch.int64, device=dev) if count_positive else None
    if row_mask is not None:
        assert row_mask.dtype == torch.uint8 and row_mask.numel() == n
    rc = _lib.load().scamd_pp_col_stats_f32(ptr(indptr), ptr(indices), ptr(data), n, g, data.numel(), ptr(row_mask),
                                            0 if expm1_scale is None else 1, 1.0 if expm1_scale is None else float(expm1_scale),
                                            ptr(s), ptr(sq), ptr(npos), stream_ptr())
    _check(rc, "scamd_pp_col_stats_f32")
    return s, sq, npos


def pp_col_stats_clip(indptr, indices, data, n: int, g: int, clip: torch.Tensor, *, row_mask: torch.Tensor | None = None):
    """-> (sum float64 [g], sumsq float64 [g]) of min(x, clip[gene]) over the stored values of the masked rows."""
    dev = require_gpu()
    clip = clip.to(torch.float64).contiguous()
    assert clip.numel() == g
    s = _empty(g, dtype=torch.float64, device=dev)
    sq = _empty(g, dtype=torch.float64, device=dev)
    if row_mask is not None:
        assert row_mask.dtype == torch.uint8 and row_mask.numel() == n
    rc = _lib.load().scamd_pp_col_stats_clip_f32(ptr(indptr), ptr(indices), ptr(data), n, g, data.numel(), ptr(row_mask),
                                                 ptr(clip), ptr(s), ptr(sq), stream_ptr())
    _check(rc, "scamd_pp_col_stats_clip_f32")
    return s, sq


def pp_scale_csr_(indptr, indices, data, n: int, std: torch.Tensor, *, max_value: float | None = None,
                  row_mask: torch.Tensor | None = None) -> None:
    require_gpu()
    assert std.dtype == torch.float64
    rc = _lib.load().scamd_pp_scale_csr_f32(ptr(indptr), ptr(indices), ptr(data), n, data.numel(), ptr(std),
                                            0.0 if max_value is None else float(max_value), 0 if max_value is None else 1,
                                            ptr(row_mask), stream_ptr())
    _check(rc, "scamd_pp_scale_csr_f32")


def pp_scale_dense(indptr, indices, data, n: int, g: int, mean: torch.Tensor, std: torch.Tensor, *,
                   max_value: float | None = None, row_mask: torch.Tensor | None = None,
                   out_dtype: torch.dtype = torch.float64) -> torch.Tensor:
    dev = require_gpu()
    assert mean.dtype == torch.float64 and std.dtype == torch.float64 and out_dtype in (torch.float32, torch.float64)
    out = _empty((n, g), dtype=out_dtype, device=dev)
    rc = _lib.load().scamd_pp_scale_dense_f32(ptr(indptr), ptr(indices), ptr(data), n, g, data.numel(), ptr(mean), ptr(std),
                                              0.0 if max_value is None else float(max_value), 0 if max_value is None else 1,
                                              ptr(row_mask), ptr(out), 1 if out_dtype == torch.float64 else 0, stream_ptr())
    _check(rc, "scamd_pp_scale_dense_f32")
    return out


# ---- quality-control metrics (csrc/qc.hip) -----------------------------------------------------------------------
def pp_qc_sweep(indptr, indices, data, n: int, g: int, *, gene_mask: torch.Tensor | None = None, n_masks: int = 0,
                per_gene: bool = True):
    """-> (row_nnz int32 [n], row_total float64 [n], row_masked float64 [n_masks, n] or None, col_nnz int64 [g] or None,
    col_sum float64 [g] or None, flags int32 [1]); gene_mask: int32 [g] holding the uint32 bit masks."""
    dev = require_gpu()
    row_nnz = _empty(n, dtype=torch.int32, device=dev)
    row_total = _empty(n, dtype=torch.float64, device=dev)
    row_masked = _empty((n_masks, n), dtype=torch.float64, device=dev) if n_masks else None
    col_nnz = _empty(g, dtype=torch.int64, device=dev) if per_gene else None
    col_sum = _empty(g, dtype=torch.float64, device=dev) if per_gene else None
    flags = _empty(1, dtype=torch.int32, device=dev)
    if gene_mask is not None:
        assert gene_mask.dtype == torch.int32 and gene_mask.numel() == g
    rc = _lib.load().scamd_pp_qc_sweep_f32(ptr(indptr), ptr(indices), ptr(data), n, g, data.numel(), ptr(gene_mask), int(n_masks),
                                           ptr(row_nnz), ptr(row_total), ptr(row_masked), ptr(col_nnz), ptr(col_sum), ptr(flags),
                                           stream_ptr())
    _check(rc, "scamd_pp_qc_sweep_f32")
    return row_nnz, row_total, row_masked, col_nnz, col_sum, flags


def pp_qc_top(indptr, data, n: int, positions) -> torch.Tensor:
    """-> top float64 [n, len(positions)]: the sum of the positions[j] largest values of every row (rule: include/scanpy_amd.h)"""
    dev = require_gpu()
    pos = (C.c_int32 * len(positions))(*(int(p) for p in positions))
    out = _empty((n, len(positions)), dtype=torch.float64, device=dev)
    rc = _lib.load().scamd_pp_qc_top_f32(ptr(indptr), ptr(data), n, data.numel(), C.cast(pos, C.c_void_p), len(positions),
                                         ptr(out), stream_ptr())
    _check(rc, "scamd_pp_qc_top_f32")
    return out


# ---- regress_out (csrc/regress.hip) --------------------------------------------------------------------------------
def _regress_model(n: int, w, codes, m: int):
    assert (w is None) != (codes is None), "exactly one of w (numeric keys) and codes (a categorical key)"
    if w is not None:
        assert w.dtype == torch.float64 and w.is_contiguous() and tuple(w.shape) == (n, m)
    else:
        assert codes.dtype == torch.int32 and codes.numel() == n


def pp_regress_sums(indptr, indices, data, n: int, g: int, *, w: torch.Tensor | None = None, codes: torch.Tensor | None = None,
                    m: int, wbound: torch.Tensor):
    """-> (sums float64 [m, g] = W^T X in order-independent fixed point, col_min float32 [g], col_max float32 [g] over all n
    cells, flags int32 [1]: bit 0 a stored value was not finite, bit 1 a code outside [0, m)); W: include/scanpy_amd.h"""
    dev = require_gpu()
    lib = _lib.load()
    _regress_model(n, w, codes, m)
    assert wbound.dtype == torch.float64 and wbound.numel() == m
    sums = _empty((m, g), dtype=torch.float64, device=dev)
    col_min = _empty(g, dtype=torch.float32, device=dev)
    col_max = _empty(g, dtype=torch.float32, device=dev)
    flags = _empty(1, dtype=torch.int32, device=dev)
    nbytes = int(lib.scamd_pp_regress_workspace_bytes(g, m))
    ws = _empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    rc = lib.scamd_pp_regress_sums_f32(ptr(indptr), ptr(indices), ptr(data), n, g, data.numel(), ptr(w), ptr(codes), int(m),
                                       ptr(wbound), ptr(sums), ptr(col_min), ptr(col_max), ptr(flags), ptr(ws), nbytes, stream_ptr())
    _check(rc, "scamd_pp_regress_sums_f32")
    return sums, col_min, col_max, flags


def pp_regress_resid(indptr, indices, data, n: int, g: int, keep: torch.Tensor, table: torch.Tensor, *,
                     w: torch.Tensor | None = None, codes: torch.Tensor | None = None,
                     out_dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """-> out [n, g]: x - W @ table in float64, rounded once to out_dtype, for the genes with keep != 0; x for the others"""
    dev = require_gpu()
    m = int(table.shape[0])
    _regress_model(n, w, codes, m)
    assert table.dtype == torch.float64 and table.is_contiguous() and tuple(table.shape) == (m, g)
    assert keep.dtype == torch.uint8 and keep.numel() == g and out_dtype in (torch.float32, torch.float64)
    out = _empty((n, g), dtype=out_dtype, device=dev)
    rc = _lib.load().scamd_pp_regress_resid_f32(ptr(indptr), ptr(indices), ptr(data), n, g, data.numel(), ptr(keep), ptr(table),
                                                ptr(w), ptr(codes), m, ptr(out), 1 if out_dtype == torch.float64 else 0,
                                                stream_ptr())
    _check(rc, "scamd_pp_regress_resid_f32")
    return out


# ---- scrublet (csrc/scrublet.hip) ----------------------------------------------------------------------------------
def pp_scrublet_pairs(indptr, indices, data, n: int, g: int, pairs: torch.Tensor, row_total: torch.Tensor):
    """Row-pair sums: output row r = row pairs[r, 0] + row pairs[r, 1] of a canonical CSR matrix.  Count phase, device scan,
    one read-back of the total, allocation, fill phase.
    -> (out_indptr int64 [n_sim + 1], out_indices int32, out_data float32, total_sim like row_total [n_sim], flags int)"""
    dev = require_gpu()
    lib = _lib.load()
    assert pairs.dtype == torch.int32 and pairs.is_contiguous() and pairs.dim() == 2 and pairs.shape[1] == 2
    assert row_total.dtype in (torch.float32, torch.float64) and row_total.numel() == n
    n_sim = int(pairs.shape[0])
    out_indptr = _empty(n_sim + 1, dtype=torch.int64, device=dev)
    total_sim = _empty(n_sim, dtype=row_total.dtype, device=dev)
    flags = _empty(1, dtype=torch.int32, device=dev)
    ws, wsz = _ws(lib.scamd_pp_scrublet_workspace_bytes(n_sim), dev)
    total = C.c_int64(-1)
    rc = lib.scamd_pp_scrublet_pair_count(ptr(indptr), ptr(indices), n, g, data.numel(), ptr(pairs), n_sim, ptr(row_total),
                                          1 if row_total.dtype == torch.float64 else 0, ptr(out_indptr), ptr(total_sim), ptr(flags),
                                          C.byref(total), ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_pp_scrublet_pair_count")
    out_nnz = int(total.value)
    f = int(flags.cpu()[0])
    out_indices = _empty(out_nnz, dtype=torch.int32, device=dev)
    out_data = _empty(out_nnz, dtype=torch.float32, device=dev)
    rc = lib.scamd_pp_scrublet_pair_fill_f32(ptr(indptr), ptr(indices), ptr(data), n, g, data.numel(), ptr(pairs), n_sim,
                                             ptr(out_indptr), out_nnz, ptr(out_indices), ptr(out_data), ptr(flags), stream_ptr())
    _check(rc, "scamd_pp_scrublet_pair_fill_f32")
    return out_indptr, out_indices, out_data, total_sim, f | int(flags.cpu()[0])


def scrublet_scores(idx: torch.Tensor, n_obs: int, *, rho: float, r: float, se_rho: float):
    """idx int32 [n_all, k], observed rows first -> (n_sim_neigh int32 [n_all], score float64 [n_all], score_err float64 [n_all])"""
    dev = require_gpu()
    assert idx.dtype == torch.int32 and idx.is_contiguous() and idx.dim() == 2
    n_all, k = idx.shape
    cnt = _empty(n_all, dtype=torch.int32, device=dev)
    score = _empty(n_all, dtype=torch.float64, device=dev)
    err = _empty(n_all, dtype=torch.float64, device=dev)
    rc = _lib.load().scamd_scrublet_scores_f64(ptr(idx), n_all, int(k), int(n_obs), float(rho), float(r), float(se_rho), ptr(cnt),
                                               ptr(score), ptr(err), stream_ptr())
    _check(rc, "scamd_scrublet_scores_f64")
    return cnt, score, err


# ---- UMAP layout (csrc/umap.hip) -----------------------------------------------------------------------------------
def rank_genes_group_stats(t_indptr, t_indices, t_data, n: int, g: int, codes: torch.Tensor, n_groups: int, *,
                           expm1_scale: float | None = None):
    """-> (sum float64, sumsq float64, nnz int64), each [n_groups, g], of the cells with code k in gene j; expm1_scale = s:
    of expm1(x * s).  Input: the CSC copy (`csr_transpose`) and codes int32[n] (-1: the cell takes no part)."""
    dev = require_gpu()
    lib = _lib.load()
    assert codes.dtype == torch.int32 and codes.numel() == n
    s = _empty((n_groups, g), dtype=torch.float64, device=dev)
    sq = _empty((n_groups, g), dtype=torch.float64, device=dev)
    nz = _empty((n_groups, g), dtype=torch.int64, device=dev)
    rc = lib.scamd_rank_genes_group_stats_f32(ptr(t_indptr), ptr(t_indices), ptr(t_data), n, g, ptr(codes), n_groups,
                                              0 if expm1_scale is None else 1, 1.0 if expm1_scale is None else float(expm1_scale),
                                              ptr(s), ptr(sq), ptr(nz), None, 0, stream_ptr())
    _check(rc, "scamd_rank_genes_group_stats_f32")
    return s, sq, nz


def rank_genes_wilcoxon(t_indptr, t_indices, t_data, n: int, g: int, codes: torch.Tensor, n_groups: int,
                        group_sizes: torch.Tensor, reference: int, *, tie_term: bool):
    """-> (ranksum2 int64 [n_groups, g], tie term float64 ([g] for reference = -1, else [n_groups, g]) or None)."""
    dev = require_gpu()
    lib = _lib.load()
    assert codes.dtype == torch.int32 and codes.numel() == n
    assert group_sizes.dtype == torch.int64 and group_sizes.numel() == n_groups
    rs = _empty((n_groups, g), dtype=torch.int64, device=dev)
    tie = None
    if tie_term:
        tie = _empty(g if reference < 0 else (n_groups, g), dtype=torch.float64, device=dev)
    ws, wsz = _ws(lib.scamd_rank_genes_workspace_bytes(n, g, t_data.numel(), n_groups), dev)
    rc = lib.scamd_rank_genes_wilcoxon_f32(ptr(t_indptr), ptr(t_indices), ptr(t_data), n, g, ptr(codes), n_groups,
                                           ptr(group_sizes), int(reference), ptr(rs), ptr(tie), ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_rank_genes_wilcoxon_f32")
    return rs, tie


def umap_optimize_(indptr, indices, epochs_per_sample, n: int, y: torch.Tensor, *, n_epochs: int, a: float, b: float,
                   gamma: float = 1.0, initial_alpha: float = 1.0, negative_sample_rate: float = 5.0, seed: int = 0) -> None:
    """y [n, dim] float32 (device, contiguous): initial embedding in, optimised embedding out."""
    dev = require_gpu()
    lib = _lib.load()
    assert y.dtype == torch.float32 and y.is_contiguous() and y.shape[0] == n
    assert epochs_per_sample.dtype == torch.float32
    nnz, dim = int(indices.numel()), int(y.shape[1])
    need = lib.scamd_umap_workspace_bytes(n, nnz, dim)
    if need == 0:
        raise _lib.ScamdError(f"umap: unsupported shape n={n} n_components={dim} (supported: 1..8)")
    ws, wsz = _ws(need, dev)
    rc = lib.scamd_umap_optimize_f32(ptr(indptr), ptr(indices), ptr(epochs_per_sample), n, nnz, dim, int(n_epochs),
                                     float(a), float(b), float(gamma), float(initial_alpha), float(negative_sample_rate),
                                     int(seed) & (2**64 - 1), ptr(y), ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_umap_optimize_f32")


# ---- Harmony batch correction (csrc/harmony.hip) -------------------------------------------------------------------
def _f64c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda:
        raise ValueError(f"harmony: expected a contiguous float64 device tensor, got {t.dtype} on {t.device}, contiguous={t.is_contiguous()}")
    return t


def harmony_permutation(n: int, seed: int, rnd: int) -> torch.Tensor:
    """-> perm int32 [n]: the keyed bijection on [0, n) of (seed, round)."""
    dev = require_gpu()
    perm = _empty(n, dtype=torch.int32, device=dev)
    rc = _lib.load().scamd_harmony_permutation_i32(n, int(seed) & (2**64 - 1), int(rnd) & (2**64 - 1), ptr(perm), None, 0, stream_ptr())
    _check(rc, "scamd_harmony_permutation_i32")
    return perm


def harmony_normalize(x: torch.Tensor) -> torch.Tensor:
    dev = require_gpu()
    n, d = _f64c(x).shape
    out = _empty((n, d), dtype=torch.float64, device=dev)
    rc = _lib.load().scamd_harmony_normalize_f64(ptr(x), n, d, ptr(out), stream_ptr())
    _check(rc, "scamd_harmony_normalize_f64")
    return out


def harmony_kmeans(z_norm: torch.Tensor, n_clusters: int, uniforms, *, max_iter: int = 25):
    """-> (centroids float64 [K, d], labels int32 [n], sweeps): k-means++ by D^2 sampling with the given K uniforms, then Lloyd."""
    dev = require_gpu()
    lib = _lib.load()
    n, d = _f64c(z_norm).shape
    u = (C.c_double * n_clusters)(*[float(v) for v in uniforms])
    cen = _empty((n_clusters, d), dtype=torch.float64, device=dev)
    lab = _empty(n, dtype=torch.int32, device=dev)
    it = C.c_int(0)
    ws, wsz = _ws(lib.scamd_harmony_kmeans_workspace_bytes(n, d, n_clusters), dev)
    rc = lib.scamd_harmony_kmeans_f64(ptr(z_norm), n, d, n_clusters, u, int(max_iter), ptr(cen), ptr(lab), C.byref(it), ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_harmony_kmeans_f64")
    return cen, lab, int(it.value)


def harmony_init(z_norm: torch.Tensor, codes: torch.Tensor, n_levels: int, centroids: torch.Tensor, pr_b: torch.Tensor, theta: torch.Tensor,
                 sigma: float, stabilized: bool, *, n_covariates: int = 1):
    """-> (R [n, K], E [levels, K], O [levels, K], objective [4] = total, k-means error, entropy, diversity), all float64."""
    dev = require_gpu()
    lib = _lib.load()
    n, d = _f64c(z_norm).shape
    k = _f64c(centroids).shape[0]
    assert codes.dtype == torch.int32 and codes.numel() == n and _f64c(pr_b).numel() == n_levels and _f64c(theta).numel() == n_levels
    r = _empty((n, k), dtype=torch.float64, device=dev)
    e = _empty((n_levels, k), dtype=torch.float64, device=dev)
    o = _empty((n_levels, k), dtype=torch.float64, device=dev)
    obj = _empty(4, dtype=torch.float64, device=dev)
    ws, wsz = _ws(lib.scamd_harmony_state_workspace_bytes(n, d, k, n_levels), dev)
    rc = lib.scamd_harmony_init_f64(ptr(z_norm), ptr(codes), n, d, k, n_levels, n_covariates, ptr(centroids), ptr(pr_b), ptr(theta), float(sigma),
                                    int(bool(stabilized)), ptr(r), ptr(e), ptr(o), ptr(obj), ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_harmony_init_f64")
    return r, e, o, obj


def harmony_cluster_round_(z_norm: torch.Tensor, codes: torch.Tensor, n_levels: int, perm: torch.Tensor, n_blocks: int, pr_b: torch.Tensor,
                           theta: torch.Tensor, sigma: float, stabilized: bool, r: torch.Tensor, e: torch.Tensor, o: torch.Tensor,
                           y_norm: torch.Tensor, objective: torch.Tensor, *, n_covariates: int = 1) -> None:
    """one clustering iteration, in place on r, e, o; y_norm [K, d] and objective [4] are written."""
    dev = require_gpu()
    lib = _lib.load()
    n, d = _f64c(z_norm).shape
    k = _f64c(r).shape[1]
    assert codes.dtype == torch.int32 and perm.dtype == torch.int32 and perm.numel() == n and codes.numel() == n
    assert tuple(_f64c(e).shape) == (n_levels, k) == tuple(_f64c(o).shape) and tuple(_f64c(y_norm).shape) == (k, d) and _f64c(objective).numel() == 4
    ws, wsz = _ws(lib.scamd_harmony_state_workspace_bytes(n, d, k, n_levels), dev)
    rc = lib.scamd_harmony_cluster_round_f64(ptr(z_norm), ptr(codes), n, d, k, n_levels, n_covariates, ptr(perm), int(n_blocks), ptr(pr_b), ptr(theta),
                                             float(sigma), int(bool(stabilized)), ptr(r), ptr(e), ptr(o), ptr(y_norm), ptr(objective), ptr(ws), wsz,
                                             stream_ptr())
    _check(rc, "scamd_harmony_cluster_round_f64")


def harmony_correct(x: torch.Tensor, codes: torch.Tensor, n_levels: int, r: torch.Tensor, o: torch.Tensor, e: torch.Tensor, n_b: torch.Tensor, *,
                    dynamic_lambda: bool, alpha: float, batch_prune_threshold: float | None, ridge_lambda: float, want_lambda: bool = False,
                    n_covariates: int = 1):
    """-> (z_hat [n, d], z_norm [n, d], lambda_kb [levels, K] or None)."""
    dev = require_gpu()
    lib = _lib.load()
    n, d = _f64c(x).shape
    k = _f64c(r).shape[1]
    assert codes.dtype == torch.int32 and codes.numel() == n and _f64c(n_b).numel() == n_levels
    _f64c(o), _f64c(e)
    z_hat = _empty((n, d), dtype=torch.float64, device=dev)
    z_norm = _empty((n, d), dtype=torch.float64, device=dev)
    lam = _empty((n_levels, k), dtype=torch.float64, device=dev) if want_lambda else None
    ws, wsz = _ws(lib.scamd_harmony_correct_workspace_bytes(n, d, k, n_levels), dev)
    rc = lib.scamd_harmony_correct_f64(ptr(x), ptr(codes), n, d, k, n_levels, n_covariates, ptr(r), ptr(o), ptr(e), ptr(n_b), int(bool(dynamic_lambda)),
                                       float(alpha), -1.0 if batch_prune_threshold is None else float(batch_prune_threshold), float(ridge_lambda),
                                       ptr(z_hat), ptr(z_norm), ptr(lam), ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_harmony_correct_f64")
    return z_hat, z_norm, lam


# ---- graph autocorrelation (csrc/graph_autocorr.hip) ----------------------------------------------------------------
def graph_autocorr_part_entries(nnz: int) -> int:
    return int(_lib.load().scamd_graph_autocorr_part_entries(int(nnz)))


def graph_weight_sum(weights: torch.Tensor) -> float:
    """W_sum: the float64 sum of the stored weights (float32 or float64) in a fixed order"""
    dev = require_gpu()
    lib = _lib.load()
    assert weights.dtype in (torch.float32, torch.float64) and weights.is_contiguous()
    out = _empty(1, dtype=torch.float64, device=dev)
    ws, wsz = _ws(lib.scamd_graph_autocorr_workspace_bytes(1, weights.numel()), dev)
    rc = lib.scamd_graph_weight_sum_f64(ptr(weights), int(weights.dtype == torch.float64), weights.numel(), ptr(out), ptr(ws), wsz,
                                        stream_ptr())
    _check(rc, "scamd_graph_weight_sum_f64")
    return float(out.cpu()[0])


def graph_autocorr_slab(indptr, indices, weights, n: int, slab: torch.Tensor, ld: int, ncols: int, *, offset: int = 0):
    """slab: float32 / float64 tensor holding the cell-major values; feature l of cell j at element offset + j * ld + l.
    -> (mean, z2, moran, geary, min, max), float64 [ncols] each"""
    dev = require_gpu()
    lib = _lib.load()
    assert slab.dtype in (torch.float32, torch.float64) and slab.is_contiguous() and weights.dtype in (torch.float32, torch.float64)
    assert 1 <= ncols <= ld and offset >= 0 and offset + (n - 1) * ld + ncols <= slab.numel()
    outs = [_empty(ncols, dtype=torch.float64, device=dev) for _ in range(6)]
    nnz = indices.numel()
    ws, wsz = _ws(lib.scamd_graph_autocorr_workspace_bytes(n, nnz), dev)
    entry = lib.scamd_graph_autocorr_slab_f64 if slab.dtype == torch.float64 else lib.scamd_graph_autocorr_slab_f32
    base = C.c_void_p(slab.data_ptr() + offset * slab.element_size())
    rc = entry(ptr(indptr), ptr(indices), ptr(weights), int(weights.dtype == torch.float64), n, nnz, base, int(ld), int(ncols),
               *(ptr(o) for o in outs), ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_graph_autocorr_slab")
    return tuple(outs)


def csr_dense_slab(indptr, indices, data, n: int, g: int, c0: int, ncols: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """columns [c0, c0 + ncols) of a canonical CSR float32 as a dense float32 [n, 64] slab (the first ncols columns are written)"""
    dev = require_gpu()
    slab = _empty((n, 64), dtype=torch.float32, device=dev) if out is None else out
    rc = _lib.load().scamd_csr_dense_slab_f32(ptr(indptr), ptr(indices), ptr(data), n, g, data.numel(), int(c0), int(ncols), ptr(slab),
                                              64, stream_ptr())
    _check(rc, "scamd_csr_dense_slab_f32")
    return slab


def transpose_slab(rows: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """rows [b <= 64, n] feature-major (contiguous) -> the cell-major slab [n, 64] of the same dtype (the first b columns are written)"""
    dev = require_gpu()
    lib = _lib.load()
    assert rows.dtype in (torch.float32, torch.float64) and rows.is_contiguous() and rows.dim() == 2 and rows.shape[0] <= 64
    b, n = rows.shape
    slab = _empty((n, 64), dtype=rows.dtype, device=dev) if out is None else out
    entry = lib.scamd_transpose_slab_f64 if rows.dtype == torch.float64 else lib.scamd_transpose_slab_f32
    _check(entry(ptr(rows), n, n, b, ptr(slab), 64, stream_ptr()), "scamd_transpose_slab")
    return slab


def aggregate(indptr, indices, data, n: int, g: int, codes, order, group_sizes, *, want_m2: bool = False,
              want_median: bool = False, mid_in_f32: bool = True) -> dict:
    """per (group, gene) of a canonical CSR float32 [n, g]: sum (float64), count_nonzero, count_negative (int64), on request m2
    (float64, centred) and median (float64), each [n_groups, g]; flags (int) and, with the median, info = pairs decided from the
    counts / searched by a wave / by a workgroup.  codes int32 [n], order int32 = the rows with a group sorted by group,
    group_sizes int64 [n_groups] (csrc/aggregate.hip)."""
    dev = require_gpu()
    lib = _lib.load()
    nnz, n_groups, n_order = data.numel(), group_sizes.numel(), order.numel()
    assert codes.dtype == torch.int32 and order.dtype == torch.int32 and group_sizes.dtype == torch.int64 and codes.numel() == n
    shape = (n_groups, g)
    out = {"sum": _empty(shape, dtype=torch.float64, device=dev), "count_nonzero": _empty(shape, dtype=torch.int64, device=dev),
           "count_negative": _empty(shape, dtype=torch.int64, device=dev)}
    if want_m2:
        out["m2"] = _empty(shape, dtype=torch.float64, device=dev)
    flags = _empty(1, dtype=torch.int32, device=dev)
    ws, wsz = _ws(lib.scamd_aggregate_workspace_bytes(n, g, nnz, n_groups), dev)
    rc = lib.scamd_aggregate_moments_f32(ptr(indptr), ptr(indices), ptr(data), n, g, nnz, ptr(codes), ptr(order), n_order,
                                         ptr(group_sizes), n_groups, ptr(out["sum"]), ptr(out["count_nonzero"]),
                                         ptr(out["count_negative"]), ptr(out["m2"]) if want_m2 else None, ptr(flags), ptr(ws), wsz,
                                         stream_ptr())
    _check(rc, "scamd_aggregate_moments_f32")
    if want_median:
        out["median"] = _empty(shape, dtype=torch.float64, device=dev)
        info = (C.c_int64 * 3)()
        rc = lib.scamd_aggregate_median_f32(ptr(indptr), ptr(indices), ptr(data), n, g, nnz, ptr(order), n_order, ptr(group_sizes),
                                            n_groups, ptr(out["count_nonzero"]), ptr(out["count_negative"]), int(bool(mid_in_f32)),
                                            ptr(out["median"]), info, ptr(ws), wsz, stream_ptr())
        _check(rc, "scamd_aggregate_median_f32")
        out["info"] = [int(v) for v in info]
    out["flags"] = int(flags.cpu()[0])
    return out


# ---- analytic Pearson residuals (csrc/pearson.hip) ---------------------------------------------------------------------
def pp_pearson_gene_var(t_indptr, t_rows, t_data, n_rows: int, g: int, gene_sum, cell_total, total: float, inv_theta: float,
                        clip: float, tot_u, mult_u, n_batch: int, *, batch_codes: torch.Tensor | None = None,
                        batch_id: int = 0) -> torch.Tensor:
    """-> float64 [g]: the population variance of every gene's clipped Pearson residuals over the n_batch cells of the batch (all
    rows without batch_codes).  (t_indptr, t_rows, t_data): the CSC copy `csr_transpose` makes; gene_sum float64 [g], cell_total
    float64 [n_rows]; tot_u / mult_u float64: the distinct totals of the batch's cells and how often each occurs."""
    dev = require_gpu()
    lib = _lib.load()
    nnz = t_data.numel()
    for a in (gene_sum, cell_total, tot_u, mult_u):
        assert a.dtype == torch.float64 and a.is_contiguous()
    assert gene_sum.numel() == g and cell_total.numel() == n_rows and tot_u.numel() == mult_u.numel()
    assert batch_codes is None or (batch_codes.dtype == torch.int32 and batch_codes.numel() == n_rows)
    var = _empty(g, dtype=torch.float64, device=dev)
    ws, wsz = _ws(lib.scamd_pp_pearson_workspace_bytes(g, nnz), dev)
    rc = lib.scamd_pp_pearson_gene_var_f32(ptr(t_indptr), ptr(t_rows), ptr(t_data), n_rows, g, nnz, ptr(gene_sum), ptr(cell_total),
                                           float(total), float(inv_theta), float(clip), ptr(tot_u), ptr(mult_u), tot_u.numel(),
                                           int(n_batch), ptr(batch_codes), int(batch_id), ptr(var), ptr(ws), wsz, stream_ptr())
    _check(rc, "scamd_pp_pearson_gene_var_f32")
    return var


def pp_pearson_residuals(indptr, indices, data, n: int, g: int, gene_sum, cell_total, total: float, inv_theta: float, clip: float, *,
                         out_dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """-> out [n, g]: the clipped Pearson residual of every cell and gene, float64 arithmetic rounded once to out_dtype"""
    dev = require_gpu()
    assert gene_sum.dtype == torch.float64 and cell_total.dtype == torch.float64 and out_dtype in (torch.float32, torch.float64)
    assert gene_sum.numel() == g and cell_total.numel() == n
    out = _empty((n, g), dtype=out_dtype, device=dev)
    rc = _lib.load().scamd_pp_pearson_residuals_f32(ptr(indptr), ptr(indices), ptr(data), n, g, data.numel(), ptr(gene_sum),
                                                    ptr(cell_total), float(total), float(inv_theta), float(clip), ptr(out),
                                                    1 if out_dtype == torch.float64 else 0, stream_ptr())
    _check(rc, "scamd_pp_pearson_residuals_f32")
    return out
