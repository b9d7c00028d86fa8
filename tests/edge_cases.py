"""IEEE edge values for the product tests (host and device): value classes whose sums
are the same in every association order, and the order-free reference (numpy only,
never the code under test).

The kernels sum in different orders (pieces, interleaved chains, a butterfly, MFMA
order). Each class below draws its operands from sets chosen so that every partial sum
in every order is exact, or saturates the same way; the result is then a function of
the operands alone and one float64 reference serves every kernel, compared on bits:

  S  subnormals: A in {+1, -1, +2, +0, -0}, B and C0 whole multiples of the format's
     smallest subnormal. Every row's sum of |a||u||alpha| + |beta| max|u| stays under
     2^24 (2^53) units, so every partial sum is an exact multiple of the unit.
  Z  signed zeros: A in {+-0, +-1}, B and C0 in {+-0}. The sign of every output follows
     from "a sum starts at +0" and IEEE arithmetic.
  O  overflow: A in {1, 0.5}, B in {MAX, 0, 1}, alpha 1, beta 0. All terms are >= 0: the
     result is +inf exactly where three or more halves of MAX meet, else that many
     halves of MAX (the small terms total less than half an ulp of MAX / 2), else the
     exact small sum.
  N  non-finite: A in {+-1, 0.5, +-0}, B in {0, -0, 1, 2, -3, 0.5} (exact sums), then
     +inf, -inf and NaN planted in rows of B and in two values of A. NaN positions and
     the bits of every other element are order-free; NaN payloads are not compared.

reference() is np.add.at of the float64 products onto an array of +0.0, rounded once to
the output type, then alpha * acc rounded, then fma(beta, C0, .) (sddmm_cases.fma32).
Its three keyword mutants restate what the classes exist to catch: inputs flushed to
zero, absent entries masked by a multiplication with zero, a sum started from -0."""
from __future__ import annotations

import functools

import numpy as np

from sddmm_cases import fma32

FORMATS = {
    # tin: operands; tout: accumulator and C; unit: the exponent of the smallest
    # subnormal of tin; out_unit: the exponent of the unit every sum of class S is a
    # multiple of; bits: integers below 2^bits are exact in tout
    "f32": dict(tin=np.float32, tout=np.float32, word=np.uint32, unit=-149, out_unit=-149,
                bits=24),
    "f64": dict(tin=np.float64, tout=np.float64, word=np.uint64, unit=-1074, out_unit=-1074,
                bits=53),
    # fp16 A and B, fp32 accumulate: units of 2^-24 on both sides, products in 2^-48
    "f16": dict(tin=np.float16, tout=np.float32, word=np.uint32, unit=-24, out_unit=-48,
                bits=24),
}
CLASSES = ("S", "Z", "O", "N")
SPECIAL_B_ROWS = (5, 11, 17, 23)  # class N: +inf, -inf in even columns, NaN, one NaN

# largest unit multiple of class S and the value of a hub row's A entries: a hub of 3000
# nonzeros on a column of top units crosses into the normal range at alpha = -2 and
# stays under the exactness bound (3000 * 2 * 1024 * 2 + 1024 < 2^24; 3000 * 2^40 * 2 +
# 2^40 < 2^53)
S_TOP = {"f32": (1024.0, 2.0), "f64": (2.0 ** 40, 1.0), "f16": (1023.0, None)}
HUB_MAX = 3000


def _units(fmt, u):
    return np.ldexp(np.asarray(u, np.float64), FORMATS[fmt]["unit"])


def value_sets(cls, fmt):
    """(A set, B set, C0 set, [(alpha, beta)]) of a class, float64 arrays holding values
    every operand type of the format represents exactly."""
    F = FORMATS[fmt]
    big = float(np.finfo(F["tin"]).max)
    if cls == "S":
        top = S_TOP[fmt][0]
        b = _units(fmt, [0.0, -0.0, 1, 3, -512, top])
        if fmt == "f16":  # A and B both half subnormals; C0 in units of the products
            a = _units(fmt, [0.0, -0.0, 1, 3, -5, 16])
            c = np.ldexp(np.array([0.0, -0.0, 1, 3, -512, 1024]), F["out_unit"])
        else:
            a, c = np.array([1.0, -1.0, 2.0, 0.0, -0.0]), b
        return a, b, c, [(al, be) for al in (1.0, -2.0) for be in (0.0, 1.0, -1.0)]
    if cls == "Z":
        z = np.array([0.0, -0.0])
        return (np.array([0.0, -0.0, 1.0, -1.0]), z, z,
                [(al, be) for al in (1.0, -1.0) for be in (0.0, 1.0)])
    if cls == "O":
        return np.array([1.0, 0.5]), np.array([big, 0.0, 1.0]), np.array([0.0]), [(1.0, 0.0)]
    if cls == "N":
        b = np.array([0.0, -0.0, 1.0, 2.0, -3.0, 0.5])
        return (np.array([1.0, -1.0, 0.5, 0.0, -0.0]), b, b,
                [(al, be) for al in (1.0, 2.0) for be in (0.0, -1.0)])
    raise KeyError(cls)


def fill(cls, fmt, rng, n_a, shape_b, shape_c, big_frac=0.15):
    """(A values, B, C0) of the class drawn with rng, in the format's operand / output
    types. Class O draws MAX with probability big_frac and 0 / 1 evenly otherwise."""
    F = FORMATS[fmt]
    a_set, b_set, c_set, _ = value_sets(cls, fmt)
    a = rng.choice(a_set, n_a)
    if cls == "O":
        B = np.where(rng.random(shape_b) < big_frac, b_set[0], rng.choice(b_set[1:], shape_b))
    else:
        B = rng.choice(b_set, shape_b)
    C0 = rng.choice(c_set, shape_c)
    out = a.astype(F["tin"]), B.astype(F["tin"]), C0.astype(F["tout"])
    for got, want in zip(out, (a, B, C0)):  # every value is held exactly, zeros' signs too
        assert np.array_equal(got.astype(np.float64).view(np.uint64), want.view(np.uint64))
    return out


def plant_b(B):
    """Class N's special rows of B (or Y), in place: row 5 +inf, row 11 -inf in the even
    columns, row 17 NaN, one NaN at [23, n // 2]."""
    n = B.shape[1]
    B[5, :] = np.inf
    B[11, ::2] = -np.inf
    B[17, :] = np.nan
    B[23, n // 2] = np.nan
    return B


def bits(a, fmt="f32"):
    F = FORMATS[fmt]
    return np.ascontiguousarray(a, F["tout"]).view(F["word"])


def _flush(x):
    t = np.finfo(x.dtype).tiny
    return np.where(np.abs(x) < t, np.copysign(0, x), x).astype(x.dtype)


def epilogue(acc, alpha, beta, C0, fmt):
    """alpha * acc rounded to the output type, then fma(beta, C0, .); beta == 0 never
    reads C0. acc: float64, already a value of the output type."""
    tout = FORMATS[fmt]["tout"]
    with np.errstate(all="ignore"):
        ad = (np.float64(alpha) * acc).astype(tout)  # one rounding: the product is exact in float64
        if beta == 0.0:
            return ad
        C0 = np.asarray(C0, tout)
        plain = np.float64(beta) * C0.astype(np.float64) + ad.astype(np.float64)
        if tout is np.float64:
            # the classes keep beta * C0 and the sum exact (or non-finite), so the fused
            # and the two-step forms agree; S asserts it through its unit bound
            return plain
        out = fma32(np.full(C0.shape, np.float32(beta)), C0, ad)
        nf = ~np.isfinite(plain)
        out[nf] = plain[nf].astype(np.float32)
        return out


def accumulate(rows, a, cols, B, m, *, flush=False, dense_mask=False, start=0.0):
    """float64 sums of a[j] * B[cols[j]] onto row rows[j] of an m x n array of `start`:
    what np.add.at(acc, rows, a[:, None] * B[cols]) gives (test_edge_cases_host.py holds
    it to that), summed by row segments in column chunks so that a block matrix of half
    a million entries takes a moment, not minutes. The mutants: flush (A and B below the
    smallest normal become zeros), dense_mask (a dense zero-filled A times all of B:
    what a multiplication by a zero weight in place of a select computes), start = -0.0."""
    if flush:
        a, B = _flush(a), _flush(B)
    a64, B64 = a.astype(np.float64), B.astype(np.float64)
    n = B.shape[1]
    acc = np.full((m, n), start, np.float64)
    with np.errstate(all="ignore"):
        if dense_mask:
            A = np.zeros((m, B.shape[0]))
            np.add.at(A, (rows, cols), a64)
            for r in range(m):  # every B row takes part in every output row
                acc[r] += (A[r][:, None] * B64).sum(0)
            return acc
        if rows.size == 0:
            return acc
        order = np.argsort(rows, kind="stable")
        srows, a64, scols = np.asarray(rows)[order], a64[order], np.asarray(cols)[order]
        first = np.flatnonzero(np.concatenate([[True], srows[1:] != srows[:-1]]))
        present = srows[first]
        step = max(1, (1 << 23) // rows.size)
        for c0 in range(0, n, step):
            P = a64[:, None] * B64[scols, c0:c0 + step]
            seg = np.add.reduceat(P, first, axis=0)
            # the sign of a zero sum by IEEE's rule, not by the reduction's start: -0 only
            # when every product of the segment is -0
            other = np.add.reduceat(~((P == 0) & np.signbit(P)), first, axis=0, dtype=np.int64)
            seg = np.where(seg == 0, np.where(other == 0, -0.0, 0.0), seg)
            acc[present, c0:c0 + step] = acc[present, c0:c0 + step] + seg
    return acc


def references(rows, a, cols, B, m, C0, ab, fmt="f32", acc=None, **mutant):
    """{(alpha, beta): the order-free product} for every pair of ab: accumulate() rounded
    once to the output type, then the epilogue. rows / cols: the COO form of the
    matrix, base 0, duplicates added."""
    tout = FORMATS[fmt]["tout"]
    if acc is None:
        acc = accumulate(rows, a, cols, B, m, **mutant)
    with np.errstate(all="ignore"):
        acc_t = acc.astype(tout).astype(np.float64)
        if mutant.get("flush") and C0 is not None:
            C0 = _flush(np.asarray(C0, tout))
        return {(al, be): epilogue(acc_t, al, be, C0, fmt) for al, be in ab}


def reference(rows, a, cols, B, m, alpha, beta, C0, fmt="f32", **mutant):
    return references(rows, a, cols, B, m, C0, [(alpha, beta)], fmt, **mutant)[(alpha, beta)]


def reference_dots(rows, cols, X, Y, alpha, beta, old, fmt="f32", *, flush=False, start=0.0):
    """The sampled product's order-free form: out[p] = alpha * <X[rows[p]], Y[cols[p]]>
    (+ beta * old[p]), the dot summed in float64 from `start`."""
    tout = FORMATS[fmt]["tout"]
    if flush:
        X, Y = _flush(X), _flush(Y)
        old = None if old is None else _flush(old)
    with np.errstate(all="ignore"):
        acc = np.full(rows.size, start)
        step = max(1, (1 << 22) // max(X.shape[1], 1))
        for p in range(0, rows.size, step):
            s = slice(p, p + step)
            x, y = X[rows[s]].astype(np.float64), Y[cols[s]].astype(np.float64)
            acc[s] = (x * y).sum(1, initial=start)
        return epilogue(acc.astype(tout).astype(np.float64), alpha, beta, old, fmt)


# ---------------------------------------------------- what each class must assert
def _abs_units(rows, a, cols, B, m, fmt):
    out_unit = FORMATS[fmt]["out_unit"]
    with np.errstate(all="ignore"):
        absacc = accumulate(rows, np.abs(a), cols, np.abs(B), m)
    return np.ldexp(absacc, -out_unit)


def check_order_free(cls, rows, a, cols, B, m, C0, fmt="f32"):
    """Asserts the class's order-freedom condition on these operands (per case) and
    returns accumulate()'s sums for references(acc=)."""
    F = FORMATS[fmt]
    acc = accumulate(rows, a, cols, B, m)
    if cls == "S":
        _, _, c_set, ab = value_sets("S", fmt)
        absu = _abs_units(rows, a, cols, B, m, fmt)
        top_c = np.ldexp(np.abs(c_set).max(), -F["out_unit"])
        worst = absu.max() * max(abs(al) for al, _ in ab) + top_c
        assert worst < 2.0 ** F["bits"], f"class S leaves the exact range: {worst} units"
        # the float64 sum is an integer number of units (exact) and survives the output type
        u = np.ldexp(acc, -F["out_unit"])
        assert np.array_equal(u, np.rint(u)) and np.abs(u).max() <= absu.max()
        assert np.array_equal(acc.astype(F["tout"]).astype(np.float64).view(np.uint64),
                              acc.view(np.uint64)), "class S: the sum does not survive rounding"
    elif cls == "Z":
        assert not acc.any() and not np.asarray(C0).any() and not np.asarray(B).any()
    elif cls == "O":
        big = float(np.finfo(F["tin"]).max)
        a64, B64 = a.astype(np.float64), B.astype(np.float64)
        assert (a64 > 0).all() and (B64 >= 0).all()
        halves = accumulate(rows, 2 * a64, cols, (B64 == big).astype(np.float64), m)
        small = accumulate(rows, a64, cols, np.where(B64 == big, 0.0, B64), m)
        assert small.max() < 2.0 ** 24  # under half an ulp of MAX / 2 in both formats
        with np.errstate(all="ignore"):
            want = np.where(halves >= 3, np.inf,
                            np.where(halves > 0, np.minimum(halves, 2) * (big / 2), small))
            got = acc.astype(F["tout"]).astype(np.float64)
        assert np.array_equal(got, want), "class O: the saturation invariant does not hold"
    elif cls == "N":
        fin = np.isfinite(acc)
        assert np.array_equal(acc[fin].astype(F["tout"]).astype(np.float64), acc[fin])
    else:
        raise KeyError(cls)
    return acc


def check_edge_occurs(cls, wants, fmt="f32", need_cross=False, clean_rows=None, terms=3):
    """Asserts that the edge the class is named for occurs in the expected outputs.
    wants: {(alpha, beta): expected array}. need_cross: a row must reach the normal
    range (only a hub row is long enough for that). clean_rows: class N, rows that
    reference no special value and must be finite. terms: the most products an output
    sums; class O needs three halves of MAX to overflow, which one product (a <= 1)
    cannot reach."""
    F = FORMATS[fmt]
    tiny = float(np.finfo(F["tout"]).tiny)
    if cls == "S":
        if fmt == "f16":  # subnormal inputs, normal fp32 outputs
            assert all((w != 0).mean() >= 1 / 3 for w in wants.values())
            return
        for ab, w in wants.items():
            sub = (w != 0) & (np.abs(w) < tiny)
            assert sub.mean() >= 1 / 3, f"class S {ab}: {sub.mean():.2f} subnormal outputs"
        if need_cross:
            assert any((np.abs(w) >= tiny).any() for w in wants.values()), \
                "class S: no output crosses into the normal range"
    elif cls == "Z":
        for w in wants.values():
            assert not w.any()
        neg = {ab: np.signbit(w) for ab, w in wants.items()}
        assert neg[(-1.0, 1.0)].any() and not neg[(-1.0, 1.0)].all(), "class Z: one sign only"
        assert neg[(-1.0, 0.0)].mean() > 0.5 and not neg[(1.0, 0.0)].any()
    elif cls == "O":
        w = wants[(1.0, 0.0)]
        big = float(np.finfo(F["tout"]).max)
        assert (np.isfinite(w) & (w >= big / 2)).any()
        assert np.isposinf(w).any() == (terms >= 2)
        assert not np.isnan(w).any()
    elif cls == "N":
        for ab, w in wants.items():
            nan = np.isnan(w)
            assert nan.any() and not nan.all() and np.isinf(w).any(), f"class N {ab}"
            if clean_rows is not None:
                assert len(clean_rows) and np.isfinite(w[clean_rows]).all()
                assert w[clean_rows].any()
    else:
        raise KeyError(cls)


def assert_bits(got, want, what, fmt="f32"):
    """NaN positions equal; every other element holds want's bits (signs of zeros and of
    infinities included). NaN payloads are not compared."""
    got = np.asarray(got).reshape(want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        i = tuple(np.argwhere(gn != wn)[0])
        raise AssertionError(f"{what}: NaN positions differ in {int((gn != wn).sum())} of "
                             f"{want.size} elements, first {i}: got {got[i]!r} want {want[i]!r}")
    bad = (bits(got, fmt) != bits(want, fmt)) & ~wn
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {want.size} elements differ in bits, "
                             f"first {i}: got {got[i]!r} ({int(bits(got, fmt)[i]):#x}) want "
                             f"{want[i]!r} ({int(bits(want, fmt)[i]):#x})")


def differs(a, b, fmt="f32"):
    """True when assert_bits(a, b) would fail."""
    an, bn = np.isnan(a), np.isnan(b)
    return bool((an != bn).any() or ((bits(a, fmt) != bits(b, fmt)) & ~bn).any())


# ---------------------------------------------------------------- CSR cases
CSR_M, CSR_K, CSR_HUB_ROW = 96, 80, 40
CSR_CLEAN_ROWS = (3, 4, 6)  # reference no special B row; 3 and 4 carry class N's A values


@functools.lru_cache(maxsize=None)
def csr_pattern(hub=HUB_MAX):
    """96 x 80: row 0 empty, row 1 a single nonzero at column 5, row 2 full, row 40 a
    hub of `hub` nonzeros with repeated columns (24 pieces of 128 at 3000), rows 3, 4
    and 6 away from class N's special rows, the rest 0 .. 12 nonzeros, 20 % empty.
    -> (rowptr, colind, row of every nonzero)."""
    rng = np.random.default_rng(7)
    deg = rng.integers(0, 13, CSR_M)
    deg[rng.random(CSR_M) < 0.2] = 0
    rows = [np.sort(rng.choice(CSR_K, d, replace=False)) for d in deg]
    rows[0] = np.zeros(0, int)
    rows[1] = np.array([5])
    rows[2] = np.arange(CSR_K)
    rows[3] = np.array([0, 1, 2, 3, 40, 41, 42, 43])
    rows[4] = np.array([6, 7, 8])
    rows[6] = np.array([9, 10, 12, 50, 51])
    rows[CSR_HUB_ROW] = np.sort(rng.integers(0, CSR_K, hub))
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    row_of = np.repeat(np.arange(CSR_M), np.diff(rp))
    for a in (rp, ci, row_of):
        a.setflags(write=False)
    return rp, ci, row_of


@functools.lru_cache(maxsize=None)
def csr_case(cls, n, fmt="f32"):
    """The CSR case of a class at width n -> dict(rp, ci, rows, val, B, C0, ab, m, k,
    clean). Cached: treat as read-only. Asserts the class's order-freedom condition."""
    rp, ci, rows = csr_pattern()
    rng = np.random.default_rng(1000 * CLASSES.index(cls) + n + (500 if fmt == "f64" else 0))
    val, B, C0 = fill(cls, fmt, rng, ci.size, (CSR_K, n), (CSR_M, n))
    hub = slice(rp[CSR_HUB_ROW], rp[CSR_HUB_ROW + 1])
    if cls == "S":  # the hub row on a column of top units: the crossing into normals
        top, hub_a = S_TOP[fmt]
        val[hub] = hub_a
        B[:, 0] = _units(fmt, top)
    if cls == "Z":
        # the full row and the hub row (split across waves, summed by pieces) on a column
        # whose products are all -0: the sum still starts from +0
        for r in (2, CSR_HUB_ROW):
            val[rp[r]:rp[r + 1]] = rng.choice(np.array([-0.0, -1.0]).astype(val.dtype),
                                              rp[r + 1] - rp[r])
        B[:, 0] = 0.0
    if cls == "N":
        plant_b(B)
        val[rp[2] + 40] = np.inf  # row 2 is full: the inf meets zeros and finite values
        val[rp[3] + 4] = np.inf   # and once more in a row that holds no other special value
        val[rp[4]] = np.nan
    check_order_free(cls, rows, val, ci, B, CSR_M, C0, fmt)
    out = dict(rp=rp, ci=ci, rows=rows, val=val, B=B, C0=C0, ab=value_sets(cls, fmt)[3],
               m=CSR_M, k=CSR_K, clean=[6] if cls == "N" else None)
    for a in (val, B, C0):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def csr_wants(cls, n, fmt="f32"):
    """{(alpha, beta): the order-free expected m x n output} of csr_case, with the
    class's edge asserted to occur."""
    c = csr_case(cls, n, fmt)
    wants = references(c["rows"], c["val"], c["ci"], c["B"], c["m"], c["C0"], c["ab"], fmt)
    check_edge_occurs(cls, wants, fmt, need_cross=True, clean_rows=c["clean"])
    for w in wants.values():
        w.setflags(write=False)
    return wants


def csr_mutants(cls, n, fmt="f32"):
    """{name: {(alpha, beta): output}} of the three wrong behaviours on csr_case."""
    c = csr_case(cls, n, fmt)
    def ref(**kw):
        return references(c["rows"], c["val"], c["ci"], c["B"], c["m"], c["C0"], c["ab"], fmt,
                          **kw)
    return {"flush": ref(flush=True), "dense_mask": ref(dense_mask=True),
            "minus_zero_start": ref(start=-0.0)}


# ---------------------------------------------------------------- BSR cases
def bsr_coo(brp, bci, bs, direction=0):
    """The blocks expanded to COO, explicit zeros included -> (rows, cols, index into
    val) in the oracle's order (blocks in order, q = 0 .. bs - 1 inside a block)."""
    brp = np.asarray(brp, np.int64)
    nnzb = int(brp[-1])
    brow = np.repeat(np.arange(brp.size - 1), np.diff(brp))
    rr, q = np.meshgrid(np.arange(bs), np.arange(bs), indexing="ij")
    rows = (brow[:, None, None] * bs + rr[None]).reshape(-1)
    cols = (np.asarray(bci, np.int64)[:nnzb, None, None] * bs + q[None]).reshape(-1)
    inner = (rr * bs + q) if direction == 0 else (q * bs + rr)
    idx = (np.arange(nnzb)[:, None, None] * bs * bs + inner[None]).reshape(-1)
    return rows, cols, idx


def bsr_case(cls, brp, bci, val_pattern, mb, kb, bs, n, fmt="f32", direction=0, seed=0):
    """A block pattern filled from a class (N excluded: the BSR non-finite contract has
    tests of its own). val_pattern: the generator's values; where it holds a zero the
    filled matrix holds a zero of the class's set too (column-sparse blocks stay so).
    -> dict(val, B, C0, ab, rows, cols, a) with a the COO values, order-freedom asserted."""
    assert cls in ("S", "Z", "O")
    rng = np.random.default_rng(seed + 77 * bs + n + 1000 * CLASSES.index(cls))
    nnzb = int(brp[-1])
    # MAX meets MAX often in a block row of hundreds of products: thin it out
    per_row = max(1.0, nnzb / max(mb, 1) * bs)
    val, B, C0 = fill(cls, fmt, rng, nnzb * bs * bs, (kb * bs, n), (mb * bs, n),
                      big_frac=min(0.15, 2.0 / per_row))
    zero = np.asarray(val_pattern).reshape(-1)[:val.size] == 0
    if cls != "O":
        zset = np.array([0.0, -0.0]).astype(val.dtype)
        val[zero] = rng.choice(zset, int(zero.sum()))
    else:  # class O's A set holds no zero: an absent column is a plain +0
        val[zero] = 0
    if cls == "Z":  # block rows 0 .. 3 on column 0: products that are all -0
        neg = np.array([-0.0, -1.0]).astype(val.dtype)
        val[:int(brp[4]) * bs * bs] = rng.choice(neg, int(brp[4]) * bs * bs)
        B[:, 0] = 0.0
    rows, cols, idx = bsr_coo(brp, bci, bs, direction)
    a = val[idx]
    if cls == "O":  # the invariant is stated for positive a: drop the zeros from the COO form
        keep = a != 0
        rows, cols, a = rows[keep], cols[keep], a[keep]
    acc = check_order_free(cls, rows, a, cols, B, mb * bs, C0, fmt)
    return dict(val=val, B=B, C0=C0, ab=value_sets(cls, fmt)[3], rows=rows, cols=cols, a=a,
                m=mb * bs, acc=acc)


def bsr_wants(cls, case, fmt="f32"):
    wants = references(case["rows"], case["a"], case["cols"], case["B"], case["m"], case["C0"],
                       case["ab"], fmt, acc=case.get("acc"))
    check_edge_occurs(cls, wants, fmt)
    return wants


# -------------------------------------------------------------- SDDMM cases
@functools.lru_cache(maxsize=None)
def sddmm_case(cls, name, n):
    """X (m x n), Y (k x n) and the old values of a class on a csr2csc_cases pattern
    ("dups", "unsorted", "view") -> dict(m, k, rp, ci, p0, nnz, rows, cols, X, Y, old, ab).
    X plays A's part, Y B's. Class N: Y's special rows as B's, X row 7 holds a NaN, X
    row 9 an inf. Order-freedom is asserted on the COO form of the dots."""
    from sddmm_cases import pattern, rows_of
    m, k, rp, ci = pattern(name)
    p0, nnz, rows = rows_of(m, rp)
    cols = np.asarray(ci[p0:p0 + nnz], np.int64)
    rng = np.random.default_rng(31 * n + 1000 * CLASSES.index(cls) + len(name))
    a_set, _, _, ab = value_sets(cls, "f32")
    _, Y, old = fill(cls, "f32", rng, 0, (k, n), (ci.size,), big_frac=min(0.4, 2.5 / n))
    X = rng.choice(a_set, (m, n)).astype(np.float32)
    if cls == "Z":  # a third of X's rows negative, a third of Y's +0: dots of -0 products alone
        neg = rng.random(m) < 1 / 3
        X[neg] = rng.choice(np.array([-0.0, -1.0], np.float32), (int(neg.sum()), n))
        Y[rng.random(k) < 1 / 3] = 0.0
    if cls == "N":
        plant_b(Y)
        X[7, n // 3] = np.nan
        X[9, 0] = np.inf
    # the dots as a COO product: position p is row p of an nnz x n "A" whose entries are
    # X[rows[p], :], against diag-like B = Y[cols[p], :]; checked column by column
    c = dict(m=m, k=k, rp=rp, ci=ci, p0=p0, nnz=nnz, rows=rows, cols=cols, X=X, Y=Y, old=old,
             ab=ab)
    _check_dots_order_free(cls, c)
    for a in (X, Y, old):
        a.setflags(write=False)
    return c


def _check_dots_order_free(cls, c):
    x = c["X"][c["rows"]].astype(np.float64)
    y = c["Y"][c["cols"]].astype(np.float64)
    with np.errstate(all="ignore"):
        p = x * y
        acc = 0.0 + p.sum(1)
    if cls == "S":
        absu = np.ldexp((np.abs(x) * np.abs(y)).sum(1), 149)
        assert absu.max() * 2 + 1024 < 2.0 ** 24
        assert np.array_equal(acc.astype(np.float32).astype(np.float64), acc)
    elif cls == "Z":
        assert not p.any()
    elif cls == "O":
        big = float(np.finfo(np.float32).max)
        assert (x > 0).all() and (y >= 0).all()
        halves = np.where(y == big, 2 * x, 0).sum(1)
        small = np.where(y == big, 0.0, p).sum(1)
        assert small.max() < 2.0 ** 24
        with np.errstate(all="ignore"):
            want = np.where(halves >= 3, np.inf,
                            np.where(halves > 0, np.minimum(halves, 2) * (big / 2), small))
            assert np.array_equal(acc.astype(np.float32).astype(np.float64), want)
    else:
        fin = np.isfinite(acc)
        assert np.array_equal(acc[fin].astype(np.float32).astype(np.float64), acc[fin])


@functools.lru_cache(maxsize=None)
def sddmm_wants(cls, name, n):
    """{(alpha, beta): expected values of the pattern's nnz positions}, edge asserted."""
    c = sddmm_case(cls, name, n)
    sl = slice(c["p0"], c["p0"] + c["nnz"])
    wants = {ab: reference_dots(c["rows"], c["cols"], c["X"], c["Y"], ab[0], ab[1], c["old"][sl])
             for ab in c["ab"]}
    clean = None
    if cls == "N":
        clean = np.flatnonzero(~np.isin(c["rows"], (7, 9)) & ~np.isin(c["cols"], SPECIAL_B_ROWS))
    check_edge_occurs(cls, wants, "f32", clean_rows=clean, terms=n)
    return wants


# ------------------------------------------- shapes the device tests run (and the host
# tests prove able to detect the three wrong behaviours at)
CSR_N = [1, 4, 8, 16, 32, 48, 64, 66, 68, 131, 256]  # every lane-group width, VEC 1 / 2 / 4
CSR_N_LAYOUT = [1, 36, 130]
GESPMM_N = [32, 128]
HOT_N = [8, 64, 128, 130]
F64_N = [1, 7, 64]
SDDMM_N = [1, 5, 16, 64, 68, 132, 260, 1030]
SDDMM_PATTERNS = ["dups", "unsorted", "view"]
BSR_MB, BSR_KB = 24, 20
BSR_N = [8, 64, 128, 132]
BSR_F16_N = [64, 128, 264]


@functools.lru_cache(maxsize=None)
def bsr_pattern(kind, bs):
    """(brp, bci, the generator's values) of a 24 x 20 block pattern: "rand"
    (helpers.rand_bsr, fill 0.25 or 0.12, block row 2 empty) or "colsparse"
    (helpers.column_sparse_bsr: explicit all-zero blocks, single-column blocks) or
    "shared" (below)."""
    from helpers import column_sparse_bsr, rand_bsr
    rng = np.random.default_rng(400 + bs + len(kind))
    if kind == "shared":
        # runs of 16 block rows on one set of six block columns, each row without one of
        # them, block row 3 empty: far fewer union steps than blocks, so the bs 2 / 4 / 8
        # grouped stream keeps the matrix (its sharing probe gives a uniform pattern up)
        sets = [np.sort(rng.choice(BSR_KB, 6, replace=False)) for _ in range(-(-BSR_MB // 16))]
        rows = [np.delete(sets[br // 16], rng.integers(6)) if br != 3 else np.zeros(0, int)
                for br in range(BSR_MB)]
        rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        return rp, np.concatenate(rows).astype(np.int32), np.ones(rp[-1] * bs * bs, np.float32)
    fill_p = 0.25 if bs <= 16 else 0.12  # large blocks: fewer of them, the same row lengths
    if kind == "rand":
        return rand_bsr(rng, BSR_MB, BSR_KB, bs, fill_p, empty_rows=(2,))
    return column_sparse_bsr(rng, BSR_MB, BSR_KB, bs, fill_p)


@functools.lru_cache(maxsize=None)
def bsr_case_of(cls, kind, bs, n, fmt="f32", direction=0):
    brp, bci, pat = bsr_pattern(kind, bs)
    c = bsr_case(cls, brp, bci, pat, BSR_MB, BSR_KB, bs, n, fmt, direction)
    c.update(brp=brp, bci=bci, wants=bsr_wants(cls, c, fmt))
    return c


# ------------------------------------------------------------- hybrid cases
HYBRID_BS = 32
HYBRID_N = [96, 132]


@functools.lru_cache(maxsize=None)
def hybrid_case(cls, n):
    """helpers.hybrid_ex_matrix()'s parts at bs 32 (a CSR remainder and a BSR part of the
    700 x 700 community matrix) filled from a class: -> dict(parts, B, C0, ab, wants, R),
    wants in the entry's two-product form (BSR part with beta, then the CSR remainder).
    B and C0 hold R = 704 rows (whole blocks); the blocks' cells past row / column 700
    are zeros of the pattern and stay zeros, so B's last rows reach no output."""
    from helpers import HYBRID_EX_M, hybrid_ex_parts
    assert cls in ("S", "Z", "O")
    crp, cci, cv, brp, bci, bv = hybrid_ex_parts(HYBRID_BS)
    bs, m = HYBRID_BS, HYBRID_EX_M
    mb = brp.size - 1
    R = mb * bs
    rng = np.random.default_rng(600 + n + 1000 * CLASSES.index(cls))
    per_row = (cci.size + bci.size * bs * bs) / m
    aval, B, C0 = fill(cls, "f32", rng, cci.size + bv.size, (R, n), (R, n),
                       big_frac=min(0.15, 2.0 / per_row))
    cval, bval = aval[:cci.size].copy(), aval[cci.size:].copy()
    zero = bv == 0
    bval[zero] = (0.0 if cls == "O" else
                  rng.choice(np.array([0.0, -0.0], np.float32), int(zero.sum())))
    if cls == "Z":
        cval[:] = rng.choice(np.array([-0.0, -1.0], np.float32), cval.size)
        bval[~zero] = rng.choice(np.array([-0.0, -1.0], np.float32), int((~zero).sum()))
        bval[zero] = -0.0
        B[:, 0] = 0.0
    brows, bcols, idx = bsr_coo(brp, bci, bs, 0)
    rows = np.concatenate([np.repeat(np.arange(m), np.diff(crp)), brows])
    cols = np.concatenate([cci.astype(np.int64), bcols])
    a = np.concatenate([cval, bval[idx]])
    keep = a != 0
    if cls == "O":
        rows, cols, a = rows[keep], cols[keep], a[keep]
    check_order_free(cls, rows, a, cols, B, R, C0)
    ab = value_sets(cls, "f32")[3]
    # the entry's contract (include/spmm_hip.h): the BSR part writes C with beta, then the
    # CSR remainder accumulates with beta = 1. Each part is order-free; their sum differs
    # from the one-sum form only in the sign of a zero (parts that cancel exactly give +0
    # where alpha * (+0) would be -0 at a negative alpha)
    from_csr = np.arange(rows.size) < (cval.size if cls != "O" else int(keep[:cval.size].sum()))
    with np.errstate(all="ignore"):
        acc_b = accumulate(rows[~from_csr], a[~from_csr], cols[~from_csr], B, R)
        acc_c = accumulate(rows[from_csr], a[from_csr], cols[from_csr], B, R)
        wants = {}
        for al, be in ab:
            first = epilogue(acc_b.astype(np.float32).astype(np.float64), al, be, C0, "f32")
            wants[(al, be)] = epilogue(acc_c.astype(np.float32).astype(np.float64), al, 1.0, first,
                                       "f32")
    check_edge_occurs(cls, wants)
    return dict(parts=(crp, cci, cval, brp, bci, bval), B=B, C0=C0, ab=ab, wants=wants, R=R,
                m=m, coo=(rows, cols, a))
