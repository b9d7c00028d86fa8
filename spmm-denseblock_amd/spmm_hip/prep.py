"""Host-side preprocessing and data feeders (numpy in, numpy out).

Thin wrappers over the C ABI of libspmm_hip.so:
  csr2bsr / bsr2csr / csr2csc / sddmm / calculate_nnzb / partition_rows   (include/spmm_hip.h)
  edge_softmax / edge_softmax_bwd                                        (include/spmm_hip.h)
  sddmm_heads / edge_softmax_heads / edge_softmax_bwd_heads / csrmm_heads (include/spmm_hip.h)
  csrmm_reduce / csrmm_reduce_bwd (max / min aggregation)                (include/spmm_hip.h)
  rng_seed / random_array / random_csr / random_bsr /
  load_csr / dump_csr / load_graph / save_csr_bin / load_csr_bin / load_csr_cached /
  powerlaw_csr / community_csr                                  (include/spmm_host.h)
  reorder / permute_csr / load_permutation / dump_permutation /
  block_metrics / block_heatmap / dump_heatmap                  (include/spmm_reorder.h)
All conversion work happens in the library's C++ (north_star: CPU-side
preprocessing), not in Python.
"""
from __future__ import annotations

import ctypes
from ctypes import byref, c_int, c_int64, c_void_p

import numpy as np

from ._lib import BlockMetrics, check, lib


def _p(a: np.ndarray) -> c_void_p:
    return c_void_p(a.ctypes.data) if a is not None and a.size else c_void_p(0)


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _take(ptr: c_void_p, n: int, dtype) -> np.ndarray:
    """Copy n elements from a malloc'ed C array and free it."""
    if not ptr.value:
        raise MemoryError("libspmm_hip returned a null array")
    if n:
        buf = (ctypes.c_byte * (n * np.dtype(dtype).itemsize)).from_address(ptr.value)
        out = np.frombuffer(buf, dtype=dtype).copy()
    else:
        out = np.zeros(0, dtype=dtype)
    lib().spmm_host_free(ptr)
    return out


# --------------------------------------------------------------- conversions
def csr2bsr(m: int, n: int, rowptr, colind, val, bs: int, direction: int = 0):
    """cusparseXcsr2bsrNnz + cusparseScsr2bsr semantics (run_bsrmm.cu:116-142).
    Returns (bsr_rowptr[mb+1], bsr_colind[nnzb], bsr_val[nnzb*bs*bs])."""
    rowptr, colind, val = _i32(rowptr), _i32(colind), _f32(val)
    mb = (m + bs - 1) // bs
    brp = np.zeros(mb + 1, dtype=np.int32)
    nnzb = c_int(0)
    check(lib().spmm_xcsr2bsr_nnz(direction, m, n, _p(rowptr), _p(colind), bs, _p(brp),
                                  byref(nnzb)), "spmm_xcsr2bsr_nnz")
    bci = np.zeros(nnzb.value, dtype=np.int32)
    bval = np.zeros(nnzb.value * bs * bs, dtype=np.float32)
    check(lib().spmm_scsr2bsr(direction, m, n, _p(val), _p(rowptr), _p(colind), bs, _p(brp),
                              _p(bval), _p(bci)), "spmm_scsr2bsr")
    return brp, bci, bval


def bsr2csr(mb: int, nb: int, rowptr, colind, val, bs: int, direction: int = 0):
    """cusparseSbsr2csr semantics (bsr2csr.cu:177-188): nnz = nnzb*bs*bs."""
    rowptr, colind, val = _i32(rowptr), _i32(colind), _f32(val)
    nnz = int(rowptr[-1] - rowptr[0]) * bs * bs
    rp = np.zeros(mb * bs + 1, dtype=np.int32)
    ci = np.zeros(nnz, dtype=np.int32)
    v = np.zeros(nnz, dtype=np.float32)
    check(lib().spmm_sbsr2csr(direction, mb, nb, _p(val), _p(rowptr), _p(colind), bs, _p(v),
                              _p(rp), _p(ci)), "spmm_sbsr2csr")
    return rp, ci, v


_VALUE_DTYPES = (np.float16, np.float32, np.float64)


def csr2csc(m: int, n: int, rowptr, colind, val=None, *, base: int = 0,
            base_out: int | None = None, return_perm: bool = False):
    """spmm_csr2csc: the CSC form of the m x n CSR matrix, that is the CSR form of its
    transpose, entries of a column in CSR order (the stable sort of the positions by
    column). val: float16 / float32 / float64 (moved as bits) or None (pattern only).
    rowptr[0] may exceed `base` (a view: rowptr[i:j + 1] with the full colind / val).
    Returns (colptr[n+1], rowind[nnz][, val[nnz]][, perm[nnz]]) in `base_out` (default:
    `base`); perm holds the CSR position of each CSC entry."""
    rowptr, colind = _i32(rowptr), _i32(colind)
    if rowptr.size != m + 1:
        raise ValueError(f"csr2csc: rowptr has {rowptr.size} entries, needs m + 1 = {m + 1}")
    vb = 0
    if val is not None:
        val = np.ascontiguousarray(val)
        if val.dtype not in _VALUE_DTYPES:
            raise TypeError(f"csr2csc: val must be float16, float32 or float64, got {val.dtype}")
        vb = val.dtype.itemsize
    nnz = int(rowptr[m]) - int(rowptr[0])
    last = int(rowptr[m]) - base
    if nnz < 0 or colind.size < last or (val is not None and val.size < last):
        raise ValueError("csr2csc: colind / val are shorter than the row pointer says")
    base_out = base if base_out is None else base_out
    colptr = np.zeros(n + 1, dtype=np.int32)
    rowind = np.zeros(nnz, dtype=np.int32)
    cval = None if val is None else np.zeros(nnz, dtype=val.dtype)
    perm = np.zeros(nnz, dtype=np.int32) if return_perm else None
    check(lib().spmm_csr2csc(m, n, nnz, _p(val), _p(rowptr), _p(colind), vb, base, base_out,
                             _p(cval), _p(colptr), _p(rowind), _p(perm)), "spmm_csr2csc")
    out = (colptr, rowind)
    if val is not None:
        out += (cval,)
    if return_perm:
        out += (perm,)
    return out


def sddmm(m: int, n: int, k: int, rowptr, colind, X, Y, *, ldx: int | None = None,
          ldy: int | None = None, out=None, alpha: float = 1.0, beta: float = 0.0,
          base: int = 0) -> np.ndarray:
    """spmm_sddmm_csr_host_f32: out[p] = alpha * <X[row(p), :n], Y[colind[p] - base, :n]>
    (+ beta * out[p]) for every position p of the m x k CSR pattern, by the association
    rule of include/spmm_hip.h (the bits of ops.sddmm). X (m x n) and Y (k x n): float32,
    row-major with leading dimensions ldx, ldy (default n), 2-D or flat. out: float32 of
    colind's length and index (default zeros; returned). rowptr[0] may exceed `base`."""
    rowptr, colind = _i32(rowptr), _i32(colind)
    if rowptr.size != m + 1:
        raise ValueError(f"sddmm: rowptr has {rowptr.size} entries, needs m + 1 = {m + 1}")
    ldx = n if ldx is None else ldx
    ldy = n if ldy is None else ldy
    ops_ = []
    for a, rows, ld, nm in ((X, m, ldx, "X"), (Y, k, ldy, "Y")):
        if not isinstance(a, np.ndarray) or a.dtype != np.float32 or not a.flags.c_contiguous:
            raise TypeError(f"sddmm: {nm} must be a C-contiguous float32 array")
        if ld < n or (rows > 0 and a.size < (rows - 1) * ld + n):
            raise ValueError(f"sddmm: {nm} holds {a.size} floats, {rows} rows of {n} with "
                             f"leading dimension {ld} need {max(rows - 1, 0) * ld + n}")
        ops_.append(a)
    if out is None:
        out = np.zeros(colind.size, dtype=np.float32)
    if not isinstance(out, np.ndarray) or out.dtype != np.float32 or \
            not out.flags.c_contiguous or out.size < colind.size:
        raise TypeError("sddmm: out must be a C-contiguous float32 array of colind's length")
    check(lib().spmm_sddmm_csr_host_f32(m, n, k, colind.size, alpha, _p(rowptr), _p(colind), base,
                                        _p(ops_[0]), ldx, _p(ops_[1]), ldy, beta, _p(out)),
          "spmm_sddmm_csr_host_f32")
    return out


def _softmax_args(where: str, rowptr, m, arrays, out):
    rowptr = _i32(rowptr)
    m = rowptr.size - 1 if m is None else m
    if m < 0 or rowptr.size != m + 1:
        raise ValueError(f"{where}: rowptr has {rowptr.size} entries, needs m + 1 = {m + 1}")
    nnz = arrays[0][1].size
    for nm, a in arrays:
        if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 1 or \
                not a.flags.c_contiguous or a.size != nnz:
            raise TypeError(f"{where}: {nm} must be a contiguous 1-D float32 array of nnz entries")
    if out is None:
        out = np.zeros(nnz, dtype=np.float32)
    if not isinstance(out, np.ndarray) or out.dtype != np.float32 or out.ndim != 1 or \
            not out.flags.c_contiguous or out.size != nnz:
        raise TypeError(f"{where}: out must be a contiguous 1-D float32 array of nnz entries")
    return rowptr, m, nnz, out


def edge_softmax(rowptr, x, *, m: int | None = None, base: int = 0, out=None) -> np.ndarray:
    """spmm_edge_softmax_csr_host_f32: out[p] = softmax of x over the positions of p's CSR
    row, by the rule of include/spmm_hip.h (the bits of ops.edge_softmax). x: float32 of
    nnz entries, indexed like colind. out: the same shape (default zeros; returned; may be
    x itself). rowptr[0] may exceed `base`: positions outside the view are left alone."""
    rowptr, m, nnz, out = _softmax_args("edge_softmax", rowptr, m, (("x", x),), out)
    check(lib().spmm_edge_softmax_csr_host_f32(m, nnz, _p(rowptr), base, _p(x), _p(out)),
          "spmm_edge_softmax_csr_host_f32")
    return out


def edge_softmax_bwd(rowptr, y, g, *, m: int | None = None, base: int = 0,
                     out=None) -> np.ndarray:
    """spmm_edge_softmax_bwd_csr_host_f32: out[p] = y[p] * (g[p] - d(row of p)),
    d = the row's sum of y * g, by the rule of include/spmm_hip.h (the bits of
    ops.edge_softmax_bwd). out may be g itself."""
    rowptr, m, nnz, out = _softmax_args("edge_softmax_bwd", rowptr, m, (("y", y), ("g", g)), out)
    check(lib().spmm_edge_softmax_bwd_csr_host_f32(m, nnz, _p(rowptr), base, _p(y), _p(g),
                                                   _p(out)),
          "spmm_edge_softmax_bwd_csr_host_f32")
    return out


def _f32c(where: str, nm: str, a, size: int | None = None) -> None:
    if not isinstance(a, np.ndarray) or a.dtype != np.float32 or not a.flags.c_contiguous:
        raise TypeError(f"{where}: {nm} must be a C-contiguous float32 array")
    if size is not None and a.size < size:
        raise ValueError(f"{where}: {nm} holds {a.size} floats, needs {size}")


def _feature_suffix(where: str, arrays, bf16: bool) -> str:
    """The entry suffix for the per-node feature arrays `arrays` ((name, array) pairs of one
    dtype): float32 -> "f32", float16 -> "f16", uint16 with bf16=True -> "bf16" (bfloat16
    bit patterns: numpy has no such type)."""
    dt = getattr(arrays[0][1], "dtype", None)
    want = np.dtype(np.uint16) if bf16 else None
    for nm, a in arrays:
        if not isinstance(a, np.ndarray) or not a.flags.c_contiguous or a.dtype != dt or \
                (want is not None and a.dtype != want) or \
                (want is None and a.dtype not in (np.float32, np.float16)):
            raise TypeError(f"{where}: {nm} must be a C-contiguous float32 or float16 array, or "
                            f"uint16 bfloat16 patterns with bf16=True (all of one type)")
    return "bf16" if bf16 else "f16" if dt == np.float16 else "f32"


def _holds(where: str, nm: str, a, size: int | None) -> None:
    if size is not None and a.size < size:
        raise ValueError(f"{where}: {nm} holds {a.size} elements, needs {size}")


def sddmm_heads(m: int, d: int, k: int, heads: int, rowptr, colind, X, Y, *,
                ldx: int | None = None, ldy: int | None = None, out=None, alpha: float = 1.0,
                beta: float = 0.0, base: int = 0, bf16: bool = False) -> np.ndarray:
    """spmm_sddmm_csr_heads_host_f32: out[p, h] = alpha * <X[row(p), h d : (h + 1) d],
    Y[col(p), h d : (h + 1) d]> (+ beta * out[p, h]): prep.sddmm with n = d per head, bit
    for bit. X ([m, heads, d]) and Y ([k, heads, d]): float32 with leading dimensions ldx,
    ldy (default heads * d). out: float32 [nnz, heads] (default zeros; returned).
    X and Y may both be float16, or uint16 bfloat16 patterns with bf16=True
    (spmm_sddmm_csr_heads_host_f16 / _bf16): the bits of the float32 form on the widened
    arrays; out stays float32."""
    rowptr, colind = _i32(rowptr), _i32(colind)
    if rowptr.size != m + 1:
        raise ValueError(f"sddmm_heads: rowptr has {rowptr.size} entries, needs m + 1 = {m + 1}")
    w = max(heads, 0) * d
    ldx = w if ldx is None else ldx
    ldy = w if ldy is None else ldy
    ty = _feature_suffix("sddmm_heads", (("X", X), ("Y", Y)), bf16)
    for a, rows, ld, nm in ((X, m, ldx, "X"), (Y, k, ldy, "Y")):
        _holds("sddmm_heads", nm, a, (rows - 1) * ld + w if rows > 0 and ld >= w else None)
    if out is None:
        out = np.zeros((colind.size, max(heads, 0)), dtype=np.float32)
    _f32c("sddmm_heads", "out", out, colind.size * max(heads, 0))
    entry = "spmm_sddmm_csr_heads_host_" + ty
    check(getattr(lib(), entry)(m, d, k, colind.size, heads, alpha, _p(rowptr), _p(colind), base,
                                _p(X), ldx, _p(Y), ldy, beta, _p(out)), entry)
    return out


def _softmax_heads_args(where: str, rowptr, m, arrays, out):
    rowptr = _i32(rowptr)
    m = rowptr.size - 1 if m is None else m
    if m < 0 or rowptr.size != m + 1:
        raise ValueError(f"{where}: rowptr has {rowptr.size} entries, needs m + 1 = {m + 1}")
    shape = arrays[0][1].shape
    for nm, a in arrays + ((("out", out),) if out is not None else ()):
        if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 2 or \
                not a.flags.c_contiguous or a.shape != shape:
            raise TypeError(f"{where}: {nm} must be a contiguous float32 array [nnz, heads]")
    if out is None:
        out = np.zeros(shape, dtype=np.float32)
    return rowptr, m, shape[0], shape[1], out


def edge_softmax_heads(rowptr, x, *, m: int | None = None, base: int = 0, out=None) -> np.ndarray:
    """spmm_edge_softmax_csr_heads_host_f32: x is [nnz, heads]; column h of out is
    prep.edge_softmax of column h of x, bit for bit. out may be x itself."""
    rowptr, m, nnz, heads, out = _softmax_heads_args("edge_softmax_heads", rowptr, m,
                                                     (("x", x),), out)
    check(lib().spmm_edge_softmax_csr_heads_host_f32(m, nnz, heads, _p(rowptr), base, _p(x),
                                                     _p(out)),
          "spmm_edge_softmax_csr_heads_host_f32")
    return out


def edge_softmax_bwd_heads(rowptr, y, g, *, m: int | None = None, base: int = 0,
                           out=None) -> np.ndarray:
    """spmm_edge_softmax_bwd_csr_heads_host_f32: y and g are [nnz, heads]; column h of out
    is prep.edge_softmax_bwd of their columns h, bit for bit. out may be g itself."""
    rowptr, m, nnz, heads, out = _softmax_heads_args("edge_softmax_bwd_heads", rowptr, m,
                                                     (("y", y), ("g", g)), out)
    check(lib().spmm_edge_softmax_bwd_csr_heads_host_f32(m, nnz, heads, _p(rowptr), base, _p(y),
                                                         _p(g), _p(out)),
          "spmm_edge_softmax_bwd_csr_heads_host_f32")
    return out


def csrmm_heads(m: int, d: int, k: int, heads: int, rowptr, colind, val, B, *,
                ldb: int | None = None, C=None, ldc: int | None = None, alpha: float = 1.0,
                beta: float = 0.0, base: int = 0, bf16: bool = False) -> np.ndarray:
    """spmm_csrmm_heads_host_f32: C[i, h d + c] = alpha * sum_p val[p, h] * B[col(p), h d + c]
    (+ beta * C) under the piece rule of the CSR product, per head. val: float32
    [nnz, heads]; B ([k, heads, d]) and C ([m, heads, d]; default zeros; returned): float32
    with leading dimensions ldb, ldc (default heads * d). B may be float16, or uint16
    bfloat16 patterns with bf16=True (spmm_csrmm_heads_host_f16 / _bf16): the bits of the
    float32 form on the widened B; val and C stay float32."""
    rowptr, colind = _i32(rowptr), _i32(colind)
    if rowptr.size != m + 1:
        raise ValueError(f"csrmm_heads: rowptr has {rowptr.size} entries, needs m + 1 = {m + 1}")
    w = max(heads, 0) * d
    ldb = w if ldb is None else ldb
    ldc = w if ldc is None else ldc
    _f32c("csrmm_heads", "val", val, colind.size * max(heads, 0))
    ty = _feature_suffix("csrmm_heads", (("B", B),), bf16)
    _holds("csrmm_heads", "B", B, (k - 1) * ldb + w if k > 0 and ldb >= w else None)
    if C is None:
        C = np.zeros(max(m - 1, 0) * ldc + w if m > 0 else 0, dtype=np.float32)
        if ldc == w:
            C = C.reshape(m, max(heads, 0), d)
    _f32c("csrmm_heads", "C", C, (m - 1) * ldc + w if m > 0 and ldc >= w else None)
    entry = "spmm_csrmm_heads_host_" + ty
    check(getattr(lib(), entry)(m, d, k, colind.size, heads, alpha, _p(rowptr), _p(colind),
                                _p(val), base, _p(B), ldb, beta, _p(C), ldc), entry)
    return C


_REDUCE_OPS = {"max": 0, "min": 1}


def _reduce_op(where: str, reduce) -> int:
    if reduce not in _REDUCE_OPS:
        raise ValueError(f"{where}: reduce must be 'max' or 'min', got {reduce!r}")
    return _REDUCE_OPS[reduce]


def _i32c(where: str, nm: str, a, size: int | None = None) -> None:
    if not isinstance(a, np.ndarray) or a.dtype != np.int32 or not a.flags.c_contiguous:
        raise TypeError(f"{where}: {nm} must be a C-contiguous int32 array")
    if size is not None and a.size < size:
        raise ValueError(f"{where}: {nm} holds {a.size} entries, needs {size}")


def _dense_out(where: str, nm: str, a, rows: int, ld: int, n: int, dtype, fill):
    """The output `a` checked, or a new one of `rows` rows filled with `fill` (2-D when the
    rows are not padded)."""
    size = (rows - 1) * ld + n if rows > 0 and ld >= n else 0
    if a is None:
        a = np.full(size, fill, dtype=dtype)
        return a.reshape(rows, n) if ld == n and rows > 0 else a
    (_f32c if dtype == np.float32 else _i32c)(where, nm, a, size)
    return a


def csrmm_reduce(m: int, n: int, k: int, rowptr, colind, val, B, *, reduce: str = "max",
                 ldb: int | None = None, C=None, ldc: int | None = None, arg=None,
                 ldarg: int | None = None, return_arg: bool = True, base: int = 0):
    """spmm_csrmm_reduce_host_f32: C[i, j] = max (min) over row i's positions p of
    val[p] * B[col(p), j] (val None: of B[col(p), j] itself) and arg[i, j] = the winning
    0-based position: the lowest NaN position if any, else the lowest position of the
    greatest (least) term; an empty row gives +0 and -1 (the bits of ops.csrmm_reduce). B:
    float32 with leading dimension ldb (default n); C float32 / arg int32 with ldc / ldarg
    (default n; new arrays by default). Returns (C, arg), or C with return_arg=False (arg is
    then not computed)."""
    op = _reduce_op("csrmm_reduce", reduce)
    rowptr, colind = _i32(rowptr), _i32(colind)
    if rowptr.size != m + 1:
        raise ValueError(f"csrmm_reduce: rowptr has {rowptr.size} entries, needs m + 1 = {m + 1}")
    ldb = n if ldb is None else ldb
    ldc = n if ldc is None else ldc
    ldarg = n if ldarg is None else ldarg
    if val is not None:
        _f32c("csrmm_reduce", "val", val, colind.size)
    _f32c("csrmm_reduce", "B", B, (k - 1) * ldb + n if k > 0 and ldb >= n else None)
    C = _dense_out("csrmm_reduce", "C", C, m, ldc, n, np.float32, 0)
    if return_arg:
        arg = _dense_out("csrmm_reduce", "arg", arg, m, ldarg, n, np.int32, -1)
    elif arg is not None:
        raise ValueError("csrmm_reduce: arg given with return_arg=False")
    check(lib().spmm_csrmm_reduce_host_f32(op, m, n, k, colind.size, _p(rowptr), _p(colind),
                                           _p(val), base, _p(B), ldb, _p(C), ldc, _p(arg),
                                           ldarg), "spmm_csrmm_reduce_host_f32")
    return (C, arg) if return_arg else C


def csrmm_reduce_bwd(k: int, n: int, m: int, trowptr, tcolind, perm, val, dC, arg, *,
                     lddc: int | None = None, ldarg: int | None = None, dB=None,
                     lddb: int | None = None, base: int = 0) -> np.ndarray:
    """spmm_csrmm_reduce_bwd_host_f32: dB[c, j] = the sum over the positions q of row c of
    A^T (trowptr, tcolind: k rows) with arg[i, j] == perm[q], i = tcolind[q], of
    val[perm[q]] * dC[i, j] (val None: of dC[i, j]) under the product's piece rule counted
    over all of the row's positions (the bits of ops.csrmm_reduce_bwd). perm: csr2csc's;
    val in A's order. dC float32 [m, lddc], arg int32 [m, ldarg], dB float32 [k, lddb]
    (default a new array; returned). arg is only compared, never used as an index."""
    trowptr, tcolind, perm = _i32(trowptr), _i32(tcolind), _i32(perm)
    if trowptr.size != k + 1:
        raise ValueError(f"csrmm_reduce_bwd: trowptr has {trowptr.size} entries, needs k + 1 = "
                         f"{k + 1}")
    if perm.size != tcolind.size:
        raise ValueError("csrmm_reduce_bwd: perm and tcolind differ in length")
    lddc = n if lddc is None else lddc
    ldarg = n if ldarg is None else ldarg
    lddb = n if lddb is None else lddb
    if val is not None:
        _f32c("csrmm_reduce_bwd", "val", val, tcolind.size)
    _f32c("csrmm_reduce_bwd", "dC", dC, (m - 1) * lddc + n if m > 0 and lddc >= n else None)
    _i32c("csrmm_reduce_bwd", "arg", arg, (m - 1) * ldarg + n if m > 0 and ldarg >= n else None)
    dB = _dense_out("csrmm_reduce_bwd", "dB", dB, k, lddb, n, np.float32, 0)
    check(lib().spmm_csrmm_reduce_bwd_host_f32(k, n, m, tcolind.size, _p(trowptr), _p(tcolind),
                                               _p(perm), _p(val), base, _p(dC), lddc, _p(arg),
                                               ldarg, _p(dB), lddb),
          "spmm_csrmm_reduce_bwd_host_f32")
    return dB


def calculate_nnzb(n: int, rowptr, colind, bs: int) -> int:
    """calculateNnzb (utility.cc:47-69)."""
    rowptr, colind = _i32(rowptr), _i32(colind)
    r = lib().spmm_calculate_nnzb(n, _p(rowptr), _p(colind), bs)
    if r < 0:
        raise ValueError("spmm_calculate_nnzb: invalid input")
    return int(r)


def divide(n: int, rowptr, colind, val, bs: int, density: float):
    """divide_matrix (divide.cu:52-127) with values: blocks with fill >= density
    -> BSR (DIRECTION_ROW), the rest -> CSR remainder. Returns
    (csr_rowptr, csr_colind, csr_val, bsr_rowptr, bsr_colind, bsr_val)."""
    rowptr, colind, val = _i32(rowptr), _i32(colind), _f32(val)
    mb = (n + bs - 1) // bs
    crp = np.zeros(n + 1, dtype=np.int32)
    brp = np.zeros(mb + 1, dtype=np.int32)
    cn, nb = c_int(0), c_int(0)
    check(lib().spmm_divide_nnz(n, _p(rowptr), _p(colind), bs, density, _p(crp), _p(brp),
                                byref(cn), byref(nb)), "spmm_divide_nnz")
    cci = np.zeros(cn.value, dtype=np.int32)
    cv = np.zeros(cn.value, dtype=np.float32)
    bci = np.zeros(nb.value, dtype=np.int32)
    bv = np.zeros(nb.value * bs * bs, dtype=np.float32)
    check(lib().spmm_sdivide(n, _p(rowptr), _p(colind), _p(val), bs, density, _p(crp), _p(brp),
                             _p(cci), _p(cv), _p(bci), _p(bv)), "spmm_sdivide")
    return crp, cci, cv, brp, bci, bv


def hybrid_plan(rowptr, colind, bs: int, K: int, value_bytes: int = 4,
                bsr_bytes_per_s: float = 0.0, csr_bytes_per_s: float = 0.0) -> dict:
    """spmm_hybrid_plan: the divide density threshold minimising the modelled
    hybrid time. Returns {density, nnzb, csr_nnz, est_seconds}."""
    from ctypes import c_double, c_float
    rowptr, colind = _i32(rowptr), _i32(colind)
    d, nb, cn, est = c_float(0), c_int64(0), c_int64(0), c_double(0)
    check(lib().spmm_hybrid_plan(rowptr.size - 1, _p(rowptr), _p(colind), bs, K, value_bytes,
                                 bsr_bytes_per_s, csr_bytes_per_s, byref(d), byref(nb),
                                 byref(cn), byref(est)), "spmm_hybrid_plan")
    return {"density": d.value, "nnzb": nb.value, "csr_nnz": cn.value,
            "est_seconds": est.value}


def partition_rows(rowptr, nparts: int) -> np.ndarray:
    """nnz-balanced contiguous row split: bounds[nparts+1]."""
    rowptr = _i32(rowptr)
    b = np.zeros(nparts + 1, dtype=np.int32)
    check(lib().spmm_csr_partition_rows(rowptr.size - 1, _p(rowptr), nparts, _p(b)),
          "spmm_csr_partition_rows")
    return b


# -------------------------------------------------------------- data feeders
def rng_seed(seed: int = 1234) -> None:
    lib().spmm_host_rng_seed(seed)


def random_array(n: int, lo: float = -1.0, hi: float = 1.0) -> np.ndarray:
    """randomArray (load_data.cc:29-36) from the shared mt19937_64."""
    out = np.empty(n, dtype=np.float32)
    lib().spmm_host_random_array(n, lo, hi, _p(out))
    return out


def random_dense_matrix(n: int, dim: int, lo: float = -1.0, hi: float = 1.0) -> np.ndarray:
    """randomDenseMatrix (load_data.cc:38-40), returned as (n, dim) row-major."""
    return random_array(n * dim, lo, hi).reshape(n, dim)


def random_csr(m: int, n: int, p: float, lo: float = -1.0, hi: float = 1.0):
    """randomCSRMatrix (load_data.cc:42-69) -> (rowptr, colind, val)."""
    rp = np.zeros(m + 1, dtype=np.int32)
    ci, v = c_void_p(), c_void_p()
    nnz = lib().spmm_host_random_csr(m, n, p, lo, hi, _p(rp), byref(ci), byref(v))
    if nnz < 0:
        raise ValueError("spmm_host_random_csr failed")
    return rp, _take(ci, nnz, np.int32), _take(v, nnz, np.float32)


def random_bsr(mb: int, nb: int, bs: int, p: float, lo: float = -1.0, hi: float = 1.0):
    """randomBSRMatrix (load_data.cc:81-113) -> (rowptr, colind, val)."""
    rp = np.zeros(mb + 1, dtype=np.int32)
    ci, v = c_void_p(), c_void_p()
    nnzb = lib().spmm_host_random_bsr(mb, nb, bs, p, lo, hi, _p(rp), byref(ci), byref(v))
    if nnzb < 0:
        raise ValueError("spmm_host_random_bsr failed")
    return rp, _take(ci, nnzb, np.int32), _take(v, nnzb * bs * bs, np.float32)


def dump_csr(prefix: str, rowptr, colind) -> None:
    rowptr, colind = _i32(rowptr), _i32(colind)
    if lib().spmm_host_dump_csr(prefix.encode(), rowptr.size - 1, colind.size, _p(rowptr),
                                _p(colind)) != 0:
        raise OSError(f"dump_csr({prefix}) failed")


def load_csr(prefix: str):
    """loadCSRFromFile (load_data.cc:143-165) -> (rowptr, colind)."""
    rp, ci, n, nnz = c_void_p(), c_void_p(), c_int(0), c_int64(0)
    if lib().spmm_host_load_csr(prefix.encode(), byref(rp), byref(ci), byref(n), byref(nnz)) != 0:
        raise OSError(f"load_csr({prefix}) failed")
    return _take(rp, n.value + 1, np.int32), _take(ci, nnz.value, np.int32)


def save_csr_bin(path: str, rowptr, colind, val=None) -> None:
    """Binary sidecar (magic SPMMCSR1 + per-array checksums), include/spmm_host.h."""
    rowptr, colind = _i32(rowptr), _i32(colind)
    v = None if val is None else _f32(val)
    if lib().spmm_host_save_csr_bin(path.encode(), rowptr.size - 1, colind.size, _p(rowptr),
                                    _p(colind), None if v is None else _p(v)) != 0:
        raise OSError(f"save_csr_bin({path}) failed")


def load_csr_bin(path: str):
    """-> (rowptr, colind, val or None); raises on a missing or corrupt file."""
    rp, ci, v, n, nnz = c_void_p(), c_void_p(), c_void_p(), c_int(0), c_int64(0)
    rc = lib().spmm_host_load_csr_bin(path.encode(), byref(rp), byref(ci), byref(v), byref(n),
                                      byref(nnz))
    if rc == -2:
        raise ValueError(f"load_csr_bin({path}): checksum mismatch (corrupt cache)")
    if rc != 0:
        raise OSError(f"load_csr_bin({path}) failed")
    vals = _take(v, nnz.value, np.float32) if v.value else None
    return _take(rp, n.value + 1, np.int32), _take(ci, nnz.value, np.int32), vals


def load_csr_cached(prefix: str):
    """loadCSRFromFile through <prefix>.csrbin (used when fresh and intact,
    rewritten otherwise) -> (rowptr, colind)."""
    rp, ci, n, nnz = c_void_p(), c_void_p(), c_int(0), c_int64(0)
    if lib().spmm_host_load_csr_cached(prefix.encode(), byref(rp), byref(ci), byref(n),
                                       byref(nnz)) != 0:
        raise OSError(f"load_csr_cached({prefix}) failed")
    return _take(rp, n.value + 1, np.int32), _take(ci, nnz.value, np.int32)


def load_graph(filename: str):
    """loadGraphFromFile (load_data.cc:167-184) + convertGraphToCSR."""
    rp, ci, n, nnz = c_void_p(), c_void_p(), c_int(0), c_int64(0)
    if lib().spmm_host_load_graph(filename.encode(), byref(rp), byref(ci), byref(n),
                                  byref(nnz)) != 0:
        raise OSError(f"load_graph({filename}) failed")
    return _take(rp, n.value + 1, np.int32), _take(ci, nnz.value, np.int32)


def powerlaw_csr(n: int, nnz: int, max_deg: int, gamma: float = 2.3, seed: int = 1234):
    """Chung-Lu power-law stand-in for an OGB graph (include/spmm_host.h)."""
    rp, ci = c_void_p(), c_void_p()
    if lib().spmm_host_gen_powerlaw_csr(n, nnz, max_deg, gamma, seed, byref(rp), byref(ci)) != 0:
        raise ValueError("spmm_host_gen_powerlaw_csr: invalid parameters")
    return _take(rp, n + 1, np.int32), _take(ci, nnz, np.int32)


def community_csr(n: int, avg_deg: float, cmin: int, cmax: int, p_in: float, seed: int = 1234):
    """Community-ordered stand-in for a rabbit-reordered graph (include/spmm_host.h)."""
    rp, ci, nnz = c_void_p(), c_void_p(), c_int64(0)
    if lib().spmm_host_gen_community_csr(n, avg_deg, cmin, cmax, p_in, seed, byref(rp), byref(ci),
                                         byref(nnz)) != 0:
        raise ValueError("spmm_host_gen_community_csr: invalid parameters")
    return _take(rp, n + 1, np.int32), _take(ci, nnz.value, np.int32)


# ------------------------------------------------------- reorder front-end
_REORDER = {"degree": "spmm_reorder_degree", "bfs": "spmm_reorder_bfs",
            "rcm": "spmm_reorder_rcm"}


def _ok(rc: int, where: str) -> None:
    if rc != 0:
        raise ValueError(f"{where}: invalid input")


def reorder(rowptr, colind, method: str = "rcm") -> np.ndarray:
    """old2new permutation: "degree" (maxDegreeSort, reorder_strategy.cc:57-71),
    "bfs" (BFSTraversal, :84-114) or "rcm" (reverseCuthillMcKee, :73-82)."""
    if method not in _REORDER:
        raise ValueError(f"unknown reorder method {method!r}; choose from {sorted(_REORDER)}")
    rowptr, colind = _i32(rowptr), _i32(colind)
    out = np.empty(rowptr.size - 1, dtype=np.int32)
    _ok(getattr(lib(), _REORDER[method])(rowptr.size - 1, _p(rowptr), _p(colind), _p(out)),
        _REORDER[method])
    return out


def permute_csr(rowptr, colind, old2new, val=None):
    """permutate (reorder_strategy.cc:42-55): symmetric renumbering with sorted
    columns; values follow their columns. Returns (rowptr, colind[, val])."""
    rowptr, colind, old2new = _i32(rowptr), _i32(colind), _i32(old2new)
    n = rowptr.size - 1
    nrp = np.empty(n + 1, dtype=np.int32)
    nci = np.empty(colind.size, dtype=np.int32)
    if val is None:
        _ok(lib().spmm_permute_csr(n, _p(rowptr), _p(colind), None, _p(old2new), _p(nrp),
                                   _p(nci), None), "spmm_permute_csr")
        return nrp, nci
    val = _f32(val)
    nv = np.empty(val.size, dtype=np.float32)
    _ok(lib().spmm_permute_csr(n, _p(rowptr), _p(colind), _p(val), _p(old2new), _p(nrp),
                               _p(nci), _p(nv)), "spmm_permute_csr")
    return nrp, nci, nv


def load_permutation(filename: str, n: int) -> np.ndarray:
    """loadPermutation (rabbit_reorder.cc:10-19), validated as a permutation."""
    out = np.empty(n, dtype=np.int32)
    if lib().spmm_load_permutation(filename.encode(), n, _p(out)) != 0:
        raise ValueError(f"load_permutation({filename}): unreadable or not a permutation of {n}")
    return out


def dump_permutation(filename: str, old2new) -> None:
    old2new = _i32(old2new)
    if lib().spmm_dump_permutation(filename.encode(), old2new.size, _p(old2new)) != 0:
        raise OSError(f"dump_permutation({filename}) failed")


def block_metrics(rowptr, colind, bs: int) -> dict:
    """analyzeBlockSparseMetrics (reorder_graph.cc:12-24) at one block size."""
    rowptr, colind = _i32(rowptr), _i32(colind)
    m = BlockMetrics()
    _ok(lib().spmm_block_metrics(rowptr.size - 1, _p(rowptr), _p(colind), bs,
                                 c_void_p(ctypes.addressof(m))), "spmm_block_metrics")
    return {"block_dim": m.block_dim, "nnzb": m.nnzb, "density": m.density,
            "utilization": m.utilization, "average": m.average}


def block_heatmap(rowptr, colind, bs: int) -> np.ndarray:
    """getHeatmap (utility.cc:71-88): nnz per bs x bs block, shape (nb, nb)."""
    rowptr, colind = _i32(rowptr), _i32(colind)
    n = rowptr.size - 1
    nb = (n + bs - 1) // bs
    out = np.empty(nb * nb, dtype=np.int32)
    _ok(lib().spmm_block_heatmap(n, _p(rowptr), _p(colind), bs, _p(out)), "spmm_block_heatmap")
    return out.reshape(nb, nb)


def dump_heatmap(filename: str, heatmap) -> None:
    """dumpHeatmap (utility.cc:90-100) text format."""
    h = np.ascontiguousarray(heatmap, dtype=np.int32)
    if h.ndim != 2 or h.shape[0] != h.shape[1]:
        raise ValueError("heatmap must be square")
    if lib().spmm_dump_heatmap(filename.encode(), h.shape[0], _p(h)) != 0:
        raise OSError(f"dump_heatmap({filename}) failed")
