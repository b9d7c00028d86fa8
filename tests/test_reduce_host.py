"""The host forms of the max / min reducers (spmm_csrmm_reduce_host_f32 and
spmm_csrmm_reduce_bwd_host_f32) against a plain numpy restatement of the two
written rules, bit for bit and arg included, against torch's CPU sparse.mm(reduce=...), and
their refusals and quick returns. No GPU.

The restatements are compared at n = 1, 3 and 37: the host forms have no vector widths or
column tiles, a column is computed on its own, so wider n adds columns, not paths (the widths
of reduce_cases.WIDTHS are the device test's). Mutants of the forward restatement (ties
toward the higher position, NaN ignored, an accumulator started at 0) must each differ from
the host form on some case: the cases exist to tell them apart."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import reduce_cases as rc
from helpers import TOL_F32, assert_normwise
from sddmm_cases import fma32

HOST_WIDTHS = (1, 3, 37)
GRAD_SETS = ("generic", "generic_noval", "one_sign")  # no two distinct B rows tie


def _prep():
    from spmm_hip import prep
    return prep


# ------------------------------------------------------------------ the rules, restated
def restate_fwd(pat, val, B, reduce, mutant=None):
    """C, arg by the forward rule: per row and column the lowest NaN position if any, else
    the lowest position whose term is >= (<=) every other. Mutants: "high" breaks ties toward
    the higher position, "no_nan" looks for the extreme of the other terms, "start0" lets a
    term win only against an accumulator that starts at 0."""
    m, k, rp, ci = rc.pattern(pat)
    n = B.shape[1]
    T = rc.terms(pat, val, B)
    C, arg = np.zeros((m, n), np.float32), np.full((m, n), -1, np.int32)
    cols = np.arange(n)
    for i in range(m):
        a, b = int(rp[i]), int(rp[i + 1])
        if a == b:
            continue
        t = T[a:b]
        isn = np.isnan(t)
        key = np.where(isn, -np.inf, t if reduce == "max" else -t)
        best = key.max(0)
        hit = key == best
        w = hit.argmax(0) if mutant != "high" else (b - a - 1) - hit[::-1].argmax(0)
        has = isn.any(0)
        if mutant != "no_nan":
            w = np.where(has, isn.argmax(0), w)
        C[i], arg[i] = t[w, cols], a + w
        if mutant == "start0":
            lose = ~has & ~(best > 0)
            C[i][lose], arg[i][lose] = 0.0, -1
    return C, arg


def _fma(x, y, a):
    """fma32 that also serves infinities and NaNs (there the sum needs no rounding care)."""
    with np.errstate(all="ignore"):
        s = x.astype(np.float64) * y.astype(np.float64) + a.astype(np.float64)
        return np.where(np.isfinite(s), fma32(x, y, a), s.astype(np.float32))


def restate_bwd(pat, val, dC, arg):
    """dB by the backward rule: per row of A^T, pieces of max(128, ceil(L / 64)) positions,
    each a chain acc = sel ? fma(v, dC[i], acc) : acc from +0, added left to right from -0."""
    m, k, rp, ci = rc.pattern(pat)
    trp, tci, perm = rc.transpose(m, k, rp, ci)
    n = dC.shape[1]
    dB = np.zeros((k, n), np.float32)
    for c in range(k):
        ta, tb = int(trp[c]), int(trp[c + 1])
        if ta == tb:
            continue
        L = tb - ta
        T = max(128, -(-L // 64))
        x = np.full(n, -0.0, np.float32)
        for s in range(ta, tb, T):
            acc = np.zeros(n, np.float32)
            for q in range(s, min(s + T, tb)):
                i = tci[q]
                sel = arg[i] == perm[q]
                if not sel.any():
                    continue
                v = np.full(n, 1.0 if val is None else val[perm[q]], np.float32)
                acc = np.where(sel, _fma(v, dC[i], acc), acc)
            x = x + acc
        dB[c] = x
    return dB


# ------------------------------------------------------------------ shared results
host_fwd, host_bwd, _dC = rc.host_fwd, rc.host_bwd, rc.grad_out
CASES = [(p, v) for p in rc.PATTERNS for v in rc.VALUE_SETS]


# ------------------------------------------------------------------ forward
@pytest.mark.parametrize("pat,vs", CASES)
def test_forward_equals_the_rule(pat, vs):
    for reduce in rc.REDUCES:
        for n in HOST_WIDTHS:
            val, B = rc.values(pat, vs, reduce, n)
            wantC, wantA = restate_fwd(pat, val, B, reduce)
            for base in (0, 1):
                C, arg = host_fwd(pat, vs, reduce, n, base)
                what = f"{pat} {vs} {reduce} n={n} base={base}"
                assert np.array_equal(arg, wantA), what
                assert rc.same_bits(C, wantC), what


def test_transpose_helper_is_csr2csc():
    for pat in rc.PATTERNS:
        m, k, rp, ci = rc.pattern(pat)
        got = _prep().csr2csc(m, k, rp, ci, return_perm=True)
        for g, w in zip(got, rc.transpose(m, k, rp, ci)):
            assert np.array_equal(g, w), pat


def test_cases_hold_what_they_claim():
    m, k, rp, ci = rc.pattern("lens")
    assert tuple(np.diff(rp)) == rc.LENS and rc.LENS[0] == rc.LENS[-1] == 0
    assert {1, 63, 64, 65, 128, 129} <= set(rc.LENS)
    assert (np.diff(ci[rp[10]:rp[11]]) == 0).any()          # repeated columns in a row
    m, k, rp, ci = rc.pattern("hub_row")
    assert m <= 400 and k <= 300 and np.diff(rp).max() == rc.HUB
    assert np.diff(rp)[0] == 0 and np.diff(rp)[-1] == 0
    m, k, rp, ci = rc.pattern("hub_col")
    assert m <= 400 and k <= 300 and np.bincount(ci).max() >= rc.HUB
    # both orders of a +0 / -0 tie, and ties at distant positions of the hub
    T = rc.terms("lens", *rc.values("lens", "zero_tie", "max", 4))
    a, b = rc.pattern("lens")[2][[9, 10]]          # the row of 200
    orders = set()
    for col in T[a:b].T:
        neg = np.signbit(col[col == 0])
        if neg.size > 1 and (neg != neg[0]).any():
            orders.add("-0 first" if neg[0] else "+0 first")
    assert orders == {"-0 first", "+0 first"}
    T = rc.terms("hub_row", *rc.values("hub_row", "ties", "max", 3))
    a = rc.pattern("hub_row")[2][150]
    hit = np.flatnonzero(T[a:a + rc.HUB, 0] == T[a:a + rc.HUB, 0].max())
    assert hit[-1] - hit[0] > 1024
    for vs in rc.TORCH_SETS:
        for reduce in rc.REDUCES:
            t = rc.terms("lens", *rc.values("lens", vs, reduce, 3))
            # (zeros of one sign tie harmlessly: no -0 means no +-0 tie)
            assert not np.isnan(t).any() and not (np.signbit(t) & (t == 0)).any(), vs
    sub = rc.terms("lens", *rc.values("lens", "subnormal", "max", 3))
    assert (np.abs(sub) < np.finfo(np.float32).tiny).all() and (sub != 0).all()


@pytest.mark.parametrize("mutant,sets", [("high", ("ties", "zero_tie", "all_inf")),
                                         ("no_nan", ("nan_first", "nan_middle", "nan_last",
                                                     "nan_two")),
                                         ("start0", ("one_sign", "all_inf"))])
def test_mutants_are_rejected(mutant, sets):
    """A wrong rule differs from the host form on the cases made for it (and the right rule
    does not: test_forward_equals_the_rule)."""
    for vs in sets:
        differs = 0
        for pat in rc.PATTERNS:
            for reduce in rc.REDUCES:
                val, B = rc.values(pat, vs, reduce, 3)
                C, arg = host_fwd(pat, vs, reduce, 3)
                mC, mA = restate_fwd(pat, val, B, reduce, mutant)
                differs += not (np.array_equal(arg, mA) and rc.same_bits(C, mC))
        assert differs, (mutant, vs)


@pytest.mark.parametrize("pat", rc.PATTERNS)
def test_forward_equals_torch_cpu(pat):
    """Without NaN and +-0 ties torch's sparse.mm(A, B, "amax" / "amin") on the CPU is
    defined alike: C equal on every bit."""
    import torch
    m, k, rp, ci = rc.pattern(pat)
    for vs in rc.TORCH_SETS:
        for reduce in rc.REDUCES:
            val, B = rc.values(pat, vs, reduce, 37)
            v = np.ones(ci.size, np.float32) if val is None else val
            A = torch.sparse_csr_tensor(torch.from_numpy(rp.astype(np.int64)),
                                        torch.from_numpy(ci.astype(np.int64)),
                                        torch.from_numpy(v), size=(m, k))
            want = torch.sparse.mm(A, torch.from_numpy(B), "a" + reduce).numpy()
            C, _ = host_fwd(pat, vs, reduce, 37)
            assert np.array_equal(rc.bits(C), rc.bits(want)), f"{pat} {vs} {reduce}"


def test_arg_none_gives_the_same_C():
    m, k, rp, ci = rc.pattern("hub_row")
    val, B = rc.values("hub_row", "generic", "max", 37)
    C = _prep().csrmm_reduce(m, 37, k, rp, ci, val, B, return_arg=False)
    assert rc.same_bits(C, host_fwd("hub_row", "generic", "max", 37)[0])


# ------------------------------------------------------------------ backward
@pytest.mark.parametrize("pat,vs", CASES)
def test_backward_equals_the_rule(pat, vs):
    reduce = rc.REDUCES[rc.VALUE_SETS.index(vs) % 2]
    for n in HOST_WIDTHS:
        val, _ = rc.values(pat, vs, reduce, n)
        _, arg = host_fwd(pat, vs, reduce, n)
        dC = _dC(pat, n)
        want = restate_bwd(pat, val, dC, arg)
        for base in (0, 1):
            got = host_bwd(pat, val, dC, arg, base)
            assert rc.same_bits(got, want), f"{pat} {vs} {reduce} n={n} base={base}"


def test_backward_ignores_what_is_not_selected():
    """An arg that selects nothing (positions >= nnz, negative, INT_MIN) gives +0 everywhere,
    whatever dC and val hold, and is never used as an index."""
    pat = "hub_col"
    m, k, rp, ci = rc.pattern(pat)
    val, _ = rc.values(pat, "nan_two", "max", 3)
    val[::7] = np.inf
    dC = _dC(pat, 3)
    dC[::3] = np.nan
    dC[1::3] = -np.inf
    for bad in (ci.size, ci.size + 12345, -1, -7, np.iinfo(np.int32).min, np.iinfo(np.int32).max):
        got = host_bwd(pat, val, dC, np.full((m, 3), bad, np.int32))
        assert np.array_equal(rc.bits(got), np.zeros((k, 3), np.uint32)), bad


def test_backward_with_every_position_selected_is_the_product():
    """One nonzero per row: every position wins its row, and dB is the sum product of A^T
    with the values val[perm] on dC, bit for bit (prep.csrmm_heads, heads = 1)."""
    prep = _prep()
    rng = np.random.default_rng(5)
    m, k, n = 400, 300, 37
    ci = rng.integers(0, k, m).astype(np.int32)
    ci[:200] = 7                                  # a long row of A^T: two pieces
    rp = np.arange(m + 1, dtype=np.int32)
    val = rng.standard_normal(m).astype(np.float32)
    B = rng.standard_normal((k, n)).astype(np.float32)
    dC = rng.standard_normal((m, n)).astype(np.float32)
    trp, tci, perm = prep.csr2csc(m, k, rp, ci, return_perm=True)
    assert np.diff(trp).max() > 128
    for v in (val, None):
        _, arg = prep.csrmm_reduce(m, n, k, rp, ci, v, B)
        assert np.array_equal(arg, np.broadcast_to(np.arange(m, dtype=np.int32)[:, None], (m, n)))
        got = prep.csrmm_reduce_bwd(k, n, m, trp, tci, perm, v, dC, arg)
        vt = (np.ones(m, np.float32) if v is None else v)[perm].reshape(m, 1)
        want = prep.csrmm_heads(k, n, m, 1, trp, tci, vt, dC)
        assert np.array_equal(rc.bits(got), rc.bits(want.reshape(k, n)))


@pytest.mark.parametrize("pat", rc.PATTERNS)
def test_backward_matches_scatter_and_torch_cpu(pat):
    """The host gradient against a float64 scatter over arg and against torch's CPU gradient
    of sparse.mm(reduce=...), within the fp32 bar of the product (helpers.TOL_F32 times the
    sum of the absolute contributions)."""
    import torch
    m, k, rp, ci = rc.pattern(pat)
    n = 37
    dC = _dC(pat, n, seed=1)
    for vs in GRAD_SETS:
        for reduce in rc.REDUCES:
            val, B = rc.values(pat, vs, reduce, n)
            _, arg = host_fwd(pat, vs, reduce, n)
            got = host_bwd(pat, val, dC, arg)
            ref, absdot = rc.scatter64(pat, val, arg, dC)
            v = np.ones(ci.size, np.float32) if val is None else val
            A = torch.sparse_csr_tensor(torch.from_numpy(rp.astype(np.int64)),
                                        torch.from_numpy(ci.astype(np.int64)),
                                        torch.from_numpy(v), size=(m, k))
            Bt = torch.from_numpy(B).requires_grad_()
            torch.sparse.mm(A, Bt, "a" + reduce).backward(torch.from_numpy(dC))
            tg = Bt.grad.numpy()
            what = f"{pat} {vs} {reduce}"
            print(f"{what}: |host - f64| {np.abs(got - ref).max():.3e}  |torch - f64| "
                  f"{np.abs(tg - ref).max():.3e}  |host - torch| {np.abs(got - tg).max():.3e}  "
                  f"max |ref| {np.abs(ref).max():.3e}")
            assert_normwise(got, ref, absdot, TOL_F32, what + ": host vs float64 scatter")
            assert_normwise(tg, ref, absdot, TOL_F32, what + ": torch vs float64 scatter")
            assert_normwise(got, tg.astype(np.float64), absdot, TOL_F32, what + ": host vs torch")


# ------------------------------------------------------------------ refusals, quick returns
def _lib():
    from spmm_hip._lib import lib
    return lib()


def _p(a):
    return ctypes.c_void_p(a.ctypes.data if a is not None else 0)


def _fwd_status(op=0, m=3, n=2, k=4, nnz=3, rp="ok", ci="ok", val=None, base=0, B="ok", ldb=2,
                C="ok", ldc=2, arg="ok", ldarg=2):
    a = {"rp": np.array([0, 1, 1, 3], np.int32), "ci": np.array([0, 3, 1], np.int32),
         "B": np.ones((4, 2), np.float32), "C": np.zeros((3, 2), np.float32),
         "arg": np.zeros((3, 2), np.int32)}
    pick = lambda nm, x: a[nm] if isinstance(x, str) else x  # noqa: E731
    return _lib().spmm_csrmm_reduce_host_f32(op, m, n, k, nnz, _p(pick("rp", rp)),
                                             _p(pick("ci", ci)), _p(val), base, _p(pick("B", B)),
                                             ldb, _p(pick("C", C)), ldc, _p(pick("arg", arg)), ldarg)


def _bwd_status(k=4, n=2, m=3, nnz=3, trp="ok", tci="ok", perm="ok", val=None, base=0, dC="ok",
                lddc=2, arg="ok", ldarg=2, dB="ok", lddb=2):
    a = {"trp": np.array([0, 1, 2, 2, 3], np.int32), "tci": np.array([0, 2, 2], np.int32),
         "perm": np.array([0, 2, 1], np.int32), "dC": np.ones((3, 2), np.float32),
         "arg": np.zeros((3, 2), np.int32), "dB": np.zeros((4, 2), np.float32)}
    pick = lambda nm, x: a[nm] if isinstance(x, str) else x  # noqa: E731
    return _lib().spmm_csrmm_reduce_bwd_host_f32(k, n, m, nnz, _p(pick("trp", trp)),
                                                 _p(pick("tci", tci)), _p(pick("perm", perm)),
                                                 _p(val), base, _p(pick("dC", dC)), lddc,
                                                 _p(pick("arg", arg)), ldarg, _p(pick("dB", dB)),
                                                 lddb)


def test_refusals_and_quick_returns():
    from spmm_hip._lib import INVALID_VALUE, SUCCESS
    i32 = lambda *x: np.array(x, np.int32)  # noqa: E731
    assert _fwd_status() == SUCCESS and _bwd_status() == SUCCESS
    for kw in (dict(m=-1), dict(n=-1), dict(k=-1), dict(nnz=-1), dict(op=2), dict(op=-1),
               dict(base=2), dict(rp=None), dict(C=None), dict(B=None), dict(ci=None),
               dict(ldb=1), dict(ldc=1), dict(ldarg=1),
               dict(rp=i32(0, 2, 1, 3)), dict(rp=i32(-1, 1, 1, 3)), dict(rp=i32(0, 1, 1, 4)),
               dict(ci=i32(0, 4, 1)), dict(ci=i32(0, -1, 1)), dict(base=1)):
        assert _fwd_status(**kw) == INVALID_VALUE, kw
    # quick returns come before the pointer checks; arg may be NULL, and ldarg is then unused
    assert _fwd_status(m=0, rp=None, C=None) == SUCCESS
    assert _fwd_status(n=0, rp=None, C=None, ldb=0, ldc=0) == SUCCESS
    assert _fwd_status(arg=None, ldarg=0) == SUCCESS
    assert _fwd_status(val=np.ones(3, np.float32)) == SUCCESS
    for kw in (dict(k=-1), dict(n=-1), dict(m=-1), dict(nnz=-1), dict(base=2), dict(trp=None),
               dict(dB=None), dict(tci=None), dict(perm=None), dict(dC=None), dict(arg=None),
               dict(lddc=1), dict(ldarg=1), dict(lddb=1), dict(trp=i32(0, 2, 1, 2, 3)),
               dict(trp=i32(0, 1, 2, 2, 4)), dict(tci=i32(0, 3, 2)), dict(perm=i32(0, 3, 1)),
               dict(perm=i32(0, -1, 1))):
        assert _bwd_status(**kw) == INVALID_VALUE, kw
    assert _bwd_status(k=0, trp=None, dB=None) == SUCCESS
    assert _bwd_status(n=0, trp=None, dB=None) == SUCCESS


def test_nnz_zero_fills_the_outputs():
    prep = _prep()
    rp = np.zeros(4, np.int32)
    e = np.zeros(0, np.int32)
    B = np.ones((2, 5), np.float32)
    C = np.full(3 * 7, np.nan, np.float32)
    arg = np.full(3 * 6, 99, np.int32)
    prep.csrmm_reduce(3, 5, 2, rp, e, None, B, C=C, ldc=7, arg=arg, ldarg=6)
    Cw, aw = np.full((3, 7), np.nan, np.float32), np.full((3, 6), 99, np.int32)
    Cw[:, :5], aw[:, :5] = 0.0, -1
    assert rc.same_bits(C, Cw.reshape(-1)) and np.array_equal(arg, aw.reshape(-1))
    dB = np.full((2, 5), np.nan, np.float32)
    prep.csrmm_reduce_bwd(2, 5, 3, np.zeros(3, np.int32), e, e, None,
                          np.ones((3, 5), np.float32), np.zeros((3, 5), np.int32), dB=dB)
    assert np.array_equal(rc.bits(dB), np.zeros((2, 5), np.uint32))
