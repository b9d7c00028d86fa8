"""Matrices and the numpy reference shared by the csr2csc tests (host and device).

The reference is numpy alone, never the code under test: the stable argsort of the
columns gives the order, np.bincount the column pointer, np.repeat the rows."""
from __future__ import annotations

import functools

import numpy as np

# nnz of the one-row / 37-row tail matrices: every size up to two 64-element steps, and
# every power of two up to 16 K at -1, 0, +1 (a tile of the device sort is one of them)
TAIL_SIZES = list(range(0, 131)) + [s + d for s in (256, 1024, 2048, 4096, 8192, 16384)
                                    for d in (-1, 0, 1)]
TAIL_N = 300

VALUE_DTYPES = {0: None, 2: np.float16, 4: np.float32, 8: np.float64}
_VIEW = {2: np.uint16, 4: np.uint32, 8: np.uint64}


def bits(a: np.ndarray) -> np.ndarray:
    """The integer view of a value array (values are compared as bits)."""
    return a.view(_VIEW[a.dtype.itemsize])


def values(nnz: int, vb: int, seed: int = 11):
    """nnz distinct-looking values of valueBytes vb (None for 0)."""
    if vb == 0:
        return None
    return np.random.default_rng(seed).uniform(-1, 1, nnz).astype(VALUE_DTYPES[vb])


def reference(m, n, rowptr, colind, val=None, base=0, base_out=0):
    """(colptr, rowind, val or None, perm) of the contract, by numpy."""
    rowptr = np.asarray(rowptr, np.int64)
    p0 = int(rowptr[0]) - base
    nnz = int(rowptr[m] - rowptr[0])
    cols = np.asarray(colind[p0:p0 + nnz], np.int64) - base
    assert nnz == 0 or (cols.min() >= 0 and cols.max() < n)
    order = np.argsort(cols, kind="stable")
    colptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))]) + base_out
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    perm = (order + p0).astype(np.int32)
    v = None if val is None else np.asarray(val)[perm]
    return colptr.astype(np.int32), (rows[order] + base_out).astype(np.int32), v, perm


def _from_rows(rows, n):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)
    return len(rows), n, rp, ci


def _sorted_rows(rng, m, n, deg_hi):
    rows = [np.sort(rng.choice(n, min(n, int(d)), replace=False))
            for d in rng.integers(0, deg_hi + 1, m)]
    rows[-1] = np.union1d(rows[-1], [0, n - 1])  # the first and the last column are used
    return rows


def tail_matrix(nnz: int, nrows: int):
    """nnz entries over nrows rows (1: one row), n = TAIL_N columns, rows sorted by
    column with duplicates (nnz may exceed n)."""
    rng = np.random.default_rng(1000 + nnz)
    cuts = np.sort(rng.integers(0, nnz + 1, nrows - 1)) if nrows > 1 else np.zeros(0, int)
    rp = np.concatenate([[0], cuts, [nnz]]).astype(np.int32)
    ci = np.concatenate([np.sort(rng.integers(0, TAIL_N, int(b - a)))
                         for a, b in zip(rp[:-1], rp[1:])] or [np.zeros(0)]).astype(np.int32)
    return nrows, TAIL_N, rp, ci


@functools.lru_cache(maxsize=None)
def matrices() -> dict:
    """name -> (m, n, rowptr, colind), base 0. The smallest shapes that reach each
    branch of the device sort: 0, 1, 2, 3 and 4 radix passes, a column longer than any
    tile, a row holding every column, duplicates, empty rows, never-used columns and
    rows that are not sorted by column."""
    from spmm_hip import prep
    rng = np.random.default_rng(3)
    out = {}
    out["n1"] = _from_rows([np.zeros(int(d), int) for d in rng.integers(0, 4, 50)], 1)
    for n in (200, 256, 257, 4096, 4097):  # 4096 / 4097: one scan launch / three
        out[f"n{n}"] = _from_rows(_sorted_rows(rng, 300, n, 8), n)
    prep.rng_seed(1234)
    rp, ci, _ = prep.random_csr(1000, 1200, 0.01)
    out["random"] = (1000, 1200, rp, ci)
    # 3 passes and skew: column 123 in every row, row 7 holds every column
    n, m = 70000, 20000
    rows = [np.union1d(rng.choice(n, int(d), replace=False), [123])
            for d in rng.integers(0, 7, m)]
    rows[7] = np.arange(n)
    out["skew"] = _from_rows(rows, n)
    # 4 passes: more than 2^24 columns
    n = (1 << 24) + 3
    cols = np.union1d(rng.choice(n, 4998, replace=False), [0, n - 1])[:5000]
    cuts = np.sort(rng.integers(0, cols.size + 1, 499))
    out["wide"] = (500, n, np.concatenate([[0], cuts, [cols.size]]).astype(np.int32),
                   np.concatenate([np.sort(c) for c in np.split(rng.permutation(cols), cuts)])
                   .astype(np.int32))
    # duplicates (sorted, repeated columns), empty rows, never-used columns
    rows = [np.sort(rng.integers(0, 700, rng.integers(0, 12))) for _ in range(513)]
    rows[5] = np.zeros(0, int)
    rows[7] = np.array([3, 3, 3, 64, 64])
    out["dups"] = _from_rows(rows, 700)
    # rows that are not sorted by column, with duplicates
    out["unsorted"] = _from_rows([rng.integers(0, 900, rng.integers(0, 40)) for _ in range(400)],
                                 900)
    return out


def view_case():
    """Rows 100 ... 400 of "random" as a view: rowptr[100:402] with the full colind."""
    m, n, rp, ci = matrices()["random"]
    return 301, n, rp[100:402], ci
