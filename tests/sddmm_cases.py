"""Operands and numpy references shared by the sampled dense-dense product's tests
(host and device). The references are numpy alone, never the code under test:
float64 for the tolerance, and an independent restatement of the association rule
(include/spmm_hip.h) for the bits."""
from __future__ import annotations

import functools

import numpy as np

from csr2csc_cases import matrices, view_case

# every lane-group width G = 1 .. 64, whole and ragged last chunks, two and three chunks
# per lane (260, 515)
N_LIST = [0, 1, 3, 4, 5, 16, 60, 64, 68, 128, 132, 256, 260, 515]
# more than four chunks per lane: the device's chunk-loop kernel
N_WIDE = 1030


def pattern(name):
    """(m, k, rowptr, colind) of a csr2csc_cases matrix ("view": view_case())."""
    return view_case() if name == "view" else matrices()[name]


def rows_of(m, rowptr, base=0):
    """(p0, nnz, the row of every position of the pattern)."""
    rowptr = np.asarray(rowptr, np.int64)
    return int(rowptr[0]) - base, int(rowptr[m] - rowptr[0]), np.repeat(np.arange(m),
                                                                        np.diff(rowptr))


@functools.lru_cache(maxsize=None)
def operands(m, k, n, seed=5):
    """X (m x n) and Y (k x n), uniform(-1, 1) float32. Cached: treat as read-only."""
    rng = np.random.default_rng(seed + 7 * n)
    X = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    Y = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


def old_values(size, seed=21):
    return np.random.default_rng(seed).uniform(-1, 1, size).astype(np.float32)


def group_lanes(n):
    chunks = -(-n // 4)
    g = 1
    while g < chunks and g < 64:
        g *= 2
    return g


def reference64(rows, cols, X, Y, alpha=1.0, beta=0.0, old=None):
    """(alpha * <x, y> + beta * old, |alpha| sum |x||y| + |beta||old|) in float64."""
    x, y = X[rows].astype(np.float64), Y[cols].astype(np.float64)
    ref, absd = alpha * (x * y).sum(1), abs(alpha) * (np.abs(x) * np.abs(y)).sum(1)
    if beta != 0.0:
        ref = ref + beta * old.astype(np.float64)
        absd = absd + abs(beta) * np.abs(old.astype(np.float64))
    return ref, absd


def fma32(x, y, a):
    """The exact fp32 FMA of float32 arrays: the product is exact in float64; the float64
    add is made round-to-odd with its two-sum residual, so the one rounding to float32
    that follows is the rounding of the exact x * y + a (no double rounding)."""
    p = x.astype(np.float64) * y.astype(np.float64)
    a = a.astype(np.float64)
    s = p + a
    bb = s - p
    err = (p - (s - bb)) + (a - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def reference_bits(rows, cols, X, Y, alpha=1.0, beta=0.0, old=None):
    """The rule, restated: G(n) chains, chain l over the columns c with (c / 4) mod G == l
    in ascending c by FMA from +0; the chains fold pairwise over adjacent chains, level
    by level; out = alpha * d, or fma(beta, old, alpha * d)."""
    n = X.shape[1]
    G = group_lanes(n)
    x, y = X[rows], Y[cols]
    acc = np.zeros((rows.size, G), np.float32)
    for l in range(G):
        a = np.zeros(rows.size, np.float32)
        for c0 in range(4 * l, n, 4 * G):
            for c in range(c0, min(c0 + 4, n)):
                a = fma32(x[:, c], y[:, c], a)
        acc[:, l] = a
    while acc.shape[1] > 1:
        acc = acc[:, 0::2] + acc[:, 1::2]
    d = acc[:, 0]
    ad = np.float32(alpha) * d
    assert ad.dtype == np.float32
    if beta == 0.0:
        return ad
    return fma32(np.full_like(d, np.float32(beta)), old.astype(np.float32), ad)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
