"""The cases of the max / min reducers of the CSR product: small seeded
matrices and value sets, shared by tests/test_reduce_host.py (the host forms against a numpy
restatement of the two rules and against torch's CPU sparse.mm(reduce=...)),
tests/test_gpu_reduce.py (the device against the host forms, bit for bit) and
tests/test_gpu_autograd_reduce.py.

Patterns (m <= 400, k <= 300; columns 0-based here, a test adds the base):
  lens     rows of 0, 1, 63, 64, 65, 128, 129, 0, 7, 200 and 12 nonzeros and a last empty
           row: the first and the last row are empty, 128 / 129 sit on the threshold between
           the wave's rows and the workgroup's, the row of 12 repeats its columns
  lens_t   the transpose of lens (300 x 12): the same lengths as rows of A^T's transpose, so
           that the backward meets them as well
  hub_row  300 x 300, rows of 0..6 nonzeros, the first and last empty, row 150 holding 5,000
           (columns repeat: k is smaller): it spans the four waves of its workgroup, 40
           pieces of the backward's rule when it is a row of A^T
  hub_col  400 x 300, every row holding column 7 twelve or thirteen times (5,000 in all) and
           up to three others: the backward's long row of A^T

Value sets (values(pattern, name, reduce, n) -> (val or None, B)); `reduce` picks the sign
where the set is about one:
  generic      normal val and B                 generic_noval  val None
  one_sign     every term negative under max, positive under min: an accumulator started at
               0 would win
  all_inf      val None, every term -inf under max (+inf under min): the winner is the
               row's first position, not -1
  inf          +-inf sprinkled over B, finite val
  subnormal    val and B near 2^-70: every product is subnormal
  zero_tie     val None, the greatest (least) terms are zeros whose sign alternates with
               column + B row: +0 before -0 in some outputs, -0 before +0 in others
  ties         val None, B of small integers: the extreme value recurs at distant positions
  nan_first / nan_last / nan_two   val with a NaN at the first / last / two positions of a row
  nan_middle   B with NaNs in the odd columns of the B row of every row's middle position
TORCH_SETS are those without NaN and without +-0 ties: there torch's CPU
sparse.mm(reduce="amax" / "amin") is defined alike and its C must match on bits."""
from __future__ import annotations

import functools

import numpy as np

WIDTHS = (1, 3, 4, 6, 37, 64, 128, 130, 256, 260)
HUB = 5000
PATTERNS = ("lens", "lens_t", "hub_row", "hub_col")
VALUE_SETS = ("generic", "generic_noval", "one_sign", "all_inf", "inf", "subnormal", "zero_tie",
              "ties", "nan_first", "nan_middle", "nan_last", "nan_two")
TORCH_SETS = ("generic", "generic_noval", "one_sign", "all_inf", "inf", "subnormal", "ties")
REDUCES = ("max", "min")
LENS = (0, 1, 63, 64, 65, 128, 129, 0, 7, 200, 12, 0)


def _csr(rows):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = (np.concatenate([np.asarray(r, np.int64) for r in rows]).astype(np.int32)
          if rp[-1] else np.zeros(0, np.int32))
    return rp, ci


def transpose(m, k, rp, ci):
    """(trp, tci, perm) of the k x m transpose, a column's entries in CSR order: numpy's own
    stable sort, independent of the library's csr2csc."""
    rows = np.repeat(np.arange(m), np.diff(rp))
    perm = np.argsort(ci, kind="stable").astype(np.int32)
    trp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=k))]).astype(np.int32)
    return trp, rows[perm].astype(np.int32), perm


@functools.lru_cache(maxsize=None)
def pattern(name):
    """-> (m, k, rowptr, colind), 0-based."""
    rng = np.random.default_rng({"lens": 11, "lens_t": 11, "hub_row": 12, "hub_col": 13}[name])
    if name in ("lens", "lens_t"):
        k = 300
        rows = [np.sort(rng.choice(k, L, replace=False)) for L in LENS]
        rows[10] = np.array([5, 5, 5, 9, 9, 40, 40, 40, 40, 41, 299, 299])
        rp, ci = _csr(rows)
        if name == "lens":
            return len(LENS), k, rp, ci
        trp, tci, _ = transpose(len(LENS), k, rp, ci)
        return k, len(LENS), trp, tci
    if name == "hub_row":
        m = k = 300
        rows = [np.sort(rng.integers(0, k, d)) for d in rng.integers(0, 7, m)]
        rows[0] = rows[m - 1] = np.zeros(0, np.int64)
        rows[150] = np.sort(rng.integers(0, k, HUB))
        return (m, k) + _csr(rows)
    if name == "hub_col":
        m, k = 400, 300
        rows = [np.sort(np.concatenate([np.full(13 if r < 200 else 12, 7),
                                        rng.integers(0, k, rng.integers(0, 4))]))
                for r in range(m)]
        rp, ci = _csr(rows)
        assert (ci == 7).sum() >= HUB
        return m, k, rp, ci
    raise KeyError(name)


def values(pat, name, reduce, n):
    """-> (val or None, B [k, n]) float32, from a seed of the three names."""
    m, k, rp, ci = pattern(pat)
    nnz = ci.size
    rng = np.random.default_rng([PATTERNS.index(pat), VALUE_SETS.index(name),
                                 REDUCES.index(reduce), n])
    f32 = np.float32
    val = rng.standard_normal(nnz).astype(f32)
    B = rng.standard_normal((k, n)).astype(f32)
    lens = np.diff(rp)
    full = np.flatnonzero(lens > 0)
    first, last = rp[:-1][full], rp[1:][full] - 1
    sgn = f32(-1.0 if reduce == "max" else 1.0)  # the sign that must not win against 0
    if name == "generic":
        return val, B
    if name == "generic_noval":
        return None, B
    if name == "one_sign":
        return (np.abs(val) + f32(0.1)).astype(f32), (sgn * (np.abs(B) + f32(0.1))).astype(f32)
    if name == "all_inf":
        return None, np.full((k, n), sgn * f32(np.inf), f32)
    if name == "inf":
        B[rng.random((k, n)) < 0.05] = np.inf
        B[rng.random((k, n)) < 0.05] = -np.inf
        return (np.sign(val) * rng.uniform(0.5, 2.0, nnz)).astype(f32), B
    if name == "subnormal":
        s = f32(2.0 ** -70)
        return ((np.sign(val) * rng.uniform(0.5, 1.0, nnz)).astype(f32) * s,
                (np.sign(B) * rng.uniform(0.5, 1.0, (k, n))).astype(f32) * s)
    if name == "zero_tie":
        B = (sgn * (np.abs(B) + f32(0.1))).astype(f32)
        zero = rng.random((k, n)) < 0.5
        zero[:, 0] = True
        parity = (np.arange(k)[:, None] + np.arange(n)[None, :]) % 2
        B[zero] = np.where(parity == 0, f32(0.0), f32(-0.0))[zero]
        return None, B
    if name == "ties":
        return None, rng.integers(-3, 4, (k, n)).astype(f32)
    if name == "nan_first":
        val[first] = np.nan
        return val, B
    if name == "nan_last":
        val[last] = np.nan
        return val, B
    if name == "nan_two":
        val[first + (last - first) // 3] = np.nan
        val[first + 2 * (last - first) // 3] = np.nan
        return val, B
    if name == "nan_middle":
        B[ci[(first + last) // 2], 1::2] = np.nan
        B[ci[(first + last) // 2], 0] = np.nan
        return val, B
    raise KeyError(name)


def terms(pat, val, B):
    """The [nnz, n] terms val[p] * B[col(p), :] (one float32 multiply), or B's rows."""
    _, _, _, ci = pattern(pat)
    return B[ci] if val is None else (val[:, None] * B[ci]).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def same_bits(got, want):
    """Equal bit for bit, a NaN matching any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype == np.float32:
        gn, wn = np.isnan(got), np.isnan(want)
        return bool(np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn]))
    return bool(np.array_equal(got, want))


@functools.lru_cache(maxsize=None)
def host_fwd(pat, vs, reduce, n, base=0):
    """(C, arg) of the host form (prep.csrmm_reduce) on a case, computed once; read-only."""
    from spmm_hip import prep
    m, k, rp, ci = pattern(pat)
    val, B = values(pat, vs, reduce, n)
    C, arg = prep.csrmm_reduce(m, n, k, rp + base, ci + base, val, B, reduce=reduce, base=base)
    C.setflags(write=False)
    arg.setflags(write=False)
    return C, arg


def grad_out(pat, n, seed=0):
    """A dC [m, n] for the backward of a case."""
    m = pattern(pat)[0]
    return np.random.default_rng([77, seed, n]).standard_normal((m, n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def host_transpose(pat):
    """(trp, tci, perm) by the library's csr2csc, 0-based."""
    from spmm_hip import prep
    m, k, rp, ci = pattern(pat)
    return prep.csr2csc(m, k, rp, ci, return_perm=True)


def host_bwd(pat, val, dC, arg, base=0):
    """dB of the host form (prep.csrmm_reduce_bwd) on the library's transpose of a pattern."""
    from spmm_hip import prep
    m, k, _, _ = pattern(pat)
    trp, tci, perm = host_transpose(pat)
    return prep.csrmm_reduce_bwd(k, dC.shape[1], m, trp + base, tci + base, perm, val,
                                 np.ascontiguousarray(dC), np.ascontiguousarray(arg), base=base)


def scatter64(pat, val, arg, dC):
    """The gradient of B in float64 by a plain scatter over (row, column) of arg, and the
    sum of the absolute contributions: -> (dB [k, n], absdot [k, n])."""
    m, k, rp, ci = pattern(pat)
    n = dC.shape[1]
    dB, ad = np.zeros((k, n)), np.zeros((k, n))
    i, j = np.nonzero(arg >= 0)
    p = arg[i, j]
    g = dC[i, j].astype(np.float64) * (1.0 if val is None else val[p].astype(np.float64))
    np.add.at(dB, (ci[p], j), g)
    np.add.at(ad, (ci[p], j), np.abs(g))
    return dB, ad
