"""Inputs and references shared by the multi-head tests (host and device): the sampled
product, the edge softmax with its backward and the CSR product over [nnz, heads] edge
values and [rows, heads, d] features (include/spmm_hip.h).

The references are never the code under test: sddmm_cases.reference_bits,
softmax_cases.exp_rule / row_sum and helpers.oracle_csrmm_pieces_f32, each applied per head
to contiguous copies of head h's slices. Everything is cached: treat what comes back as
read-only."""
from __future__ import annotations

import functools

import numpy as np

import sddmm_cases as sd
import softmax_cases as sc
from helpers import load_oracle, oracle_csrmm_pieces_f32

F = np.float32
ALPHA, BETA = 1.7, -0.6


def same(got, want) -> bool:
    """NaN where want is NaN, the same bits everywhere else."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(gn, wn) and \
        bool((wn | (got.view(np.uint32) == want.view(np.uint32))).all())


def assert_same(got, want, where):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    ok = (gn == wn) & (wn | (got.view(np.uint32) == want.view(np.uint32)))
    bad = np.argwhere(~ok)
    assert bad.shape[0] == 0, (f"{where}: {bad.shape[0]} of {want.size} outputs differ, first at "
                               f"{bad[:3].tolist()}: got {got[tuple(bad[0])]}, want "
                               f"{want[tuple(bad[0])]}")


def swap_heads(a):
    """The swapped-head mutant: head h takes head h + 1's column (or slice)."""
    return np.roll(a, -1, axis=1)


# ------------------------------------------------------------------ sampled product
# heads x d: G(d) = 1, 1, 2, 2, 8, 16 and 64 (two chunks per lane)
SDDMM_HD = [(1, 4), (2, 3), (3, 5), (8, 8), (4, 32), (8, 64), (2, 260)]
# the lane-group widths the list above leaves out (G = 4, 32), and d = 0
SDDMM_HD_MORE = [(2, 12), (2, 100), (3, 0)]
SDDMM_PATTERNS = ["n1", "random", "dups", "unsorted", "view"]


@functools.lru_cache(maxsize=None)
def sddmm_operands(m, k, heads, d):
    """X [m, heads, d] and Y [k, heads, d], uniform(-1, 1)."""
    rng = np.random.default_rng(31 + 7 * d + heads)
    X = rng.uniform(-1, 1, (m, heads, d)).astype(F)
    Y = rng.uniform(-1, 1, (k, heads, d)).astype(F)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


@functools.lru_cache(maxsize=None)
def sddmm_old(size, heads):
    a = np.random.default_rng(21).uniform(-1, 1, (size, heads)).astype(F)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def sddmm_reference(name, heads, d, epilogue=False):
    """[nnz, heads] by reference_bits per head; outside the pattern NaN (the old values
    with the epilogue)."""
    m, k, rp, ci = sd.pattern(name)
    X, Y = sddmm_operands(m, k, heads, d)
    p0, nnz, rows = sd.rows_of(m, rp)
    cols = np.asarray(ci[p0:p0 + nnz], np.int64)
    old = sddmm_old(ci.size, heads)
    out = old.copy() if epilogue else np.full((ci.size, heads), np.nan, F)
    for h in range(heads):
        Xh, Yh = np.ascontiguousarray(X[:, h, :]), np.ascontiguousarray(Y[:, h, :])
        if epilogue:
            out[p0:p0 + nnz, h] = sd.reference_bits(rows, cols, Xh, Yh, ALPHA, BETA,
                                                    np.ascontiguousarray(old[p0:p0 + nnz, h]))
        else:
            out[p0:p0 + nnz, h] = sd.reference_bits(rows, cols, Xh, Yh)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------ edge softmax
SOFTMAX_PATTERNS = ["lengths", "short_mixed", "mid", "view", "base1", "special"]
SOFTMAX_HEADS = [1, 3, 8]


def special_kind(r, h):
    """What head h of row r of "special" holds: 0 a -inf beside finite values, 1 a NaN,
    2 a +inf, 3 nothing but -inf, 4 finite values only. It differs from head to head."""
    return (r + h) % 5


@functools.lru_cache(maxsize=None)
def softmax_column(name, h):
    """(x, g) of head h: the case's x drawn with the head's own seed."""
    c = sc.case(name)
    rng = np.random.default_rng(3 + 101 * h)
    x = rng.normal(0, 3, c.nnz).astype(F)
    g = rng.normal(0, 1, c.nnz).astype(F)
    if name == "special":
        for r in range(c.m):
            a, L = int(c.starts[r]), int(c.lens[r])
            what = special_kind(r, h)
            if what == 0:
                x[a + L // 2] = -np.inf
            elif what == 1:
                x[a + L - 1] = np.nan
            elif what == 2:
                x[a] = np.inf
            elif what == 3:
                x[a:a + L] = -np.inf
    x.setflags(write=False)
    g.setflags(write=False)
    return x, g


@functools.lru_cache(maxsize=None)
def softmax_column_forward(name, h):
    """y of head h by the restated rule (exp_rule, row_sum); NaN outside the pattern."""
    c = sc.case(name)
    x, _ = softmax_column(name, h)
    y = np.full(c.nnz, np.nan, F)
    mx = np.full(c.nnz, -np.inf, F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for _, a, L in c.rows():
            xr = x[a:a + L]
            if not np.isnan(xr).all():
                mx[a:a + L] = np.fmax.reduce(xr)  # a NaN operand is dropped
        e = sc.exp_rule(x - mx)
        for _, a, L in c.rows():
            y[a:a + L] = e[a:a + L] / sc.row_sum(e[a:a + L])
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def softmax_column_backward(name, h):
    c = sc.case(name)
    y = softmax_column_forward(name, h)
    _, g = softmax_column(name, h)
    gx = np.full(c.nnz, np.nan, F)
    with np.errstate(invalid="ignore", over="ignore"):
        for _, a, L in c.rows():
            yr, gr = y[a:a + L], g[a:a + L]
            diff = gr - sc.row_sum(yr, gr)
            gx[a:a + L] = yr * diff
    gx.setflags(write=False)
    return gx


def _stack(fn, name, heads):
    a = np.ascontiguousarray(np.stack([fn(name, h) for h in range(heads)], axis=1))
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def softmax_inputs(name, heads):
    """(x, g), each [nnz, heads]."""
    return (_stack(lambda n, h: softmax_column(n, h)[0], name, heads),
            _stack(lambda n, h: softmax_column(n, h)[1], name, heads))


@functools.lru_cache(maxsize=None)
def softmax_forward(name, heads):
    return _stack(softmax_column_forward, name, heads)


@functools.lru_cache(maxsize=None)
def softmax_backward(name, heads):
    return _stack(softmax_column_backward, name, heads)


# ------------------------------------------------------------------ product
# piece boundaries (T = 128 and 129, 64 pieces), empty rows, and many short rows
PRODUCT_LENGTHS = [0, 1, 127, 128, 129, 0, 256, 257, 1000, 8193, 0]
# heads x d: 8 x 40 crosses a tile of 256 columns
PRODUCT_HD = [(1, 128), (2, 3), (3, 5), (8, 8), (8, 40), (4, 64)]
PRODUCT_K = 1500


@functools.lru_cache(maxsize=None)
def product_pattern(small=False):
    """(m, k, rowptr, colind), base 0. small: the long rows and 40 short ones (host)."""
    rng = np.random.default_rng(77)
    lens = np.concatenate([PRODUCT_LENGTHS, rng.poisson(7, 40 if small else 3000)])
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = rng.integers(0, PRODUCT_K, int(rp[-1])).astype(np.int32)
    rp.setflags(write=False)
    ci.setflags(write=False)
    return lens.size, PRODUCT_K, rp, ci


@functools.lru_cache(maxsize=None)
def product_operands(nnz, k, m, heads, d):
    """val [nnz, heads], B [k, heads, d] and the old C [m, heads, d]."""
    rng = np.random.default_rng(5 + 13 * d + heads)
    out = (rng.uniform(-1, 1, (nnz, heads)).astype(F), rng.uniform(-1, 1, (k, heads, d)).astype(F),
           rng.uniform(-1, 1, (m, heads, d)).astype(F))
    for a in out:
        a.setflags(write=False)
    return out


def product_reference_on(m, rp, ci, val, B, alpha=1.0, beta=0.0, C=None):
    """[m, heads, d]: oracle_csrmm_pieces_f32 on (val[:, h], B[:, h, :]) per head."""
    heads, d = B.shape[1], B.shape[2]
    out = np.zeros((m, heads, d), F)
    if d == 0:
        return out
    L = load_oracle()
    for h in range(heads):
        old = None if C is None else np.ascontiguousarray(C[:, h, :]).reshape(-1)
        out[:, h, :] = oracle_csrmm_pieces_f32(
            L, m, d, rp, ci, np.ascontiguousarray(val[:, h]), np.ascontiguousarray(B[:, h, :]),
            d, 0, alpha=alpha, beta=beta, C=old, ldc=d).reshape(m, d)
    return out


@functools.lru_cache(maxsize=None)
def product_reference(heads, d, epilogue=False, small=False):
    m, k, rp, ci = product_pattern(small)
    val, B, C = product_operands(ci.size, k, m, heads, d)
    out = product_reference_on(m, rp, ci, val, B, *((ALPHA, BETA, C) if epilogue else ()))
    out.setflags(write=False)
    return out


def padded(a, ld, offset=0, fill=np.nan):
    """(flat buffer, view): the rows of a ([rows, w]) at leading dimension ld, `offset`
    floats into the buffer, the padding filled with `fill`."""
    rows, w = a.shape
    buf = np.full(offset + max(rows, 1) * ld, fill, F)
    view = buf[offset:offset + rows * ld].reshape(rows, ld)
    view[:, :w] = a
    return buf, view
