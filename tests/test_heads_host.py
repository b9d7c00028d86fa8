"""The host forms of the multi-head entries (prep.sddmm_heads, edge_softmax_heads,
edge_softmax_bwd_heads, csrmm_heads) against the restated single-head rules applied per
head, bit for bit; heads = 1 against the existing host forms; and two checks of the
references themselves: on the seeded inputs the device tests use, the heads' results
differ row by row, so a kernel that reads another head's value or slice cannot pass, and
a swapped-head mutant of the reference fails the comparison at every shape."""
from __future__ import annotations

import numpy as np
import pytest

import heads_cases as hc
import sddmm_cases as sd
import softmax_cases as sc
from heads_cases import F

HEADS = [1, 2, 3, 8]
DS = [0, 1, 3, 4, 5, 8, 32, 64, 68]


def _prep():
    from spmm_hip import prep
    return prep


def _lib():
    from spmm_hip import _lib
    return _lib


# ------------------------------------------------------------------ sampled product
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("heads", HEADS)
def test_sddmm_heads_equals_the_rule_per_head(heads, d):
    prep = _prep()
    m, k, rp, ci = sd.pattern("dups")
    X, Y = hc.sddmm_operands(m, k, heads, d)
    want = hc.sddmm_reference("dups", heads, d)
    got = prep.sddmm_heads(m, d, k, heads, rp, ci, X, Y)
    hc.assert_same(got, want, f"sddmm_heads {heads}x{d}")
    # alpha / beta on old values, padded ldx / ldy one float into their buffers, base 1
    w = heads * d
    bx, vx = hc.padded(X.reshape(m, w), w + 3, 1)
    by, vy = hc.padded(Y.reshape(k, w), w + 5, 1)
    got = prep.sddmm_heads(m, d, k, heads, rp + 1, ci + 1, bx[1:], by[1:], ldx=w + 3, ldy=w + 5,
                           out=hc.sddmm_old(ci.size, heads).copy(), alpha=hc.ALPHA,
                           beta=hc.BETA, base=1)
    hc.assert_same(got, hc.sddmm_reference("dups", heads, d, True), f"sddmm_heads {heads}x{d} epi")
    if heads == 1:  # the existing host form
        one = prep.sddmm(m, d, k, rp, ci, np.ascontiguousarray(X[:, 0]),
                         np.ascontiguousarray(Y[:, 0]))
        hc.assert_same(prep.sddmm_heads(m, d, k, 1, rp, ci, X, Y), one[:, None], "heads = 1")


@pytest.mark.parametrize("heads,d", [(3, 5), (8, 8)])
def test_sddmm_heads_on_a_view(heads, d):
    prep = _prep()
    m, k, rp, ci = sd.pattern("view")
    X, Y = hc.sddmm_operands(m, k, heads, d)
    out = np.full((ci.size, heads), np.nan, F)
    prep.sddmm_heads(m, d, k, heads, rp, ci, X, Y, out=out)
    hc.assert_same(out, hc.sddmm_reference("view", heads, d), "view")  # NaN outside: untouched


# ------------------------------------------------------------------ edge softmax
@pytest.mark.parametrize("heads", HEADS)
@pytest.mark.parametrize("name", ["mid", "view", "base1", "special"])
def test_edge_softmax_heads_equals_the_rule_per_head(name, heads):
    prep = _prep()
    c = sc.case(name)
    x, g = hc.softmax_inputs(name, heads)
    mk = sc.inside(c)
    want_y, want_gx = hc.softmax_forward(name, heads), hc.softmax_backward(name, heads)
    y = prep.edge_softmax_heads(c.rowptr, x, base=c.base, out=np.full(x.shape, -7.25, F))
    hc.assert_same(y[mk], want_y[mk], f"{name} x{heads} forward")
    assert (y[~mk] == F(-7.25)).all()
    gx = prep.edge_softmax_bwd_heads(c.rowptr, want_y, g, base=c.base,
                                     out=np.full(x.shape, -7.25, F))
    hc.assert_same(gx[mk], want_gx[mk], f"{name} x{heads} backward")
    assert (gx[~mk] == F(-7.25)).all()
    # in place
    xi, gi = x.copy(), g.copy()
    prep.edge_softmax_heads(c.rowptr, xi, base=c.base, out=xi)
    prep.edge_softmax_bwd_heads(c.rowptr, want_y, gi, base=c.base, out=gi)
    hc.assert_same(xi[mk], want_y[mk], f"{name} x{heads} in place")
    hc.assert_same(gi[mk], want_gx[mk], f"{name} x{heads} backward in place")
    if heads == 1:  # the existing host forms
        x0, g0 = np.ascontiguousarray(x[:, 0]), np.ascontiguousarray(g[:, 0])
        y0 = prep.edge_softmax(c.rowptr, x0, base=c.base)
        hc.assert_same(y[mk, 0], y0[mk], "heads = 1")
        hc.assert_same(gx[mk, 0], prep.edge_softmax_bwd(c.rowptr, np.ascontiguousarray(
            want_y[:, 0]), g0, base=c.base)[mk], "heads = 1 backward")


def test_a_non_finite_row_leaves_the_other_heads_alone():
    """Rows of "special" are non-finite in some heads and finite in others: the finite
    heads' outputs are finite and the rule's on that column alone."""
    prep = _prep()
    c = sc.case("special")
    x, _ = hc.softmax_inputs("special", 3)
    y = prep.edge_softmax_heads(c.rowptr, x)
    seen = 0
    for r, a, L in c.rows():
        kinds = [hc.special_kind(r, h) for h in range(3)]
        for h in range(3):
            if kinds[h] in (0, 4) and any(kd in (1, 2, 3) for kd in kinds) and L > 1:
                assert np.isfinite(y[a:a + L, h]).all(), (r, h)
                hc.assert_same(y[a:a + L, h], hc.softmax_column_forward("special", h)[a:a + L],
                               f"row {r} head {h}")
                seen += 1
    assert seen >= 8


# ------------------------------------------------------------------ product
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("heads", HEADS)
def test_csrmm_heads_equals_the_piece_rule_per_head(heads, d):
    prep = _prep()
    m, k, rp, ci = hc.product_pattern(True)
    val, B, C = hc.product_operands(ci.size, k, m, heads, d)
    got = prep.csrmm_heads(m, d, k, heads, rp, ci, val, B)
    hc.assert_same(np.asarray(got).reshape(m, heads, d), hc.product_reference(heads, d, False, True),
                   f"csrmm_heads {heads}x{d}")
    if d == 0:
        return
    # alpha / beta on old C, padded ldb / ldc, base 1
    w = heads * d
    bb, _ = hc.padded(B.reshape(k, w), w + 3)
    cb, cv = hc.padded(C.reshape(m, w), w + 2, fill=-7.25)
    prep.csrmm_heads(m, d, k, heads, rp + 1, ci + 1, val, bb, ldb=w + 3, C=cb, ldc=w + 2,
                     alpha=hc.ALPHA, beta=hc.BETA, base=1)
    hc.assert_same(cv[:, :w].reshape(m, heads, d), hc.product_reference(heads, d, True, True),
                   f"csrmm_heads {heads}x{d} epi")
    assert (cv[:, w:] == F(-7.25)).all(), "the padding of C was written"


def test_csrmm_heads_on_a_rowptr_view():
    prep = _prep()
    m, k, rp, ci = hc.product_pattern(True)
    heads, d = 3, 5
    val, B, _ = hc.product_operands(ci.size, k, m, heads, d)
    r0, r1 = 3, 30  # rows [3, 30): rowptr[0] > 0 and rowptr[m] < nnz, the full colind / val
    got = prep.csrmm_heads(r1 - r0, d, k, heads, rp[r0:r1 + 1], ci, val, B)
    hc.assert_same(got, hc.product_reference(heads, d, False, True)[r0:r1], "rowptr view")


# ------------------------------------------------------------------ the references themselves
def _rows_differ(ref, heads, starts, lens, where, min_len=1):
    """Every row of at least min_len entries that is finite in two heads differs between
    them."""
    checked = 0
    for a, L in zip(starts, lens):
        if L < min_len:
            continue
        blk = ref[a:a + L].reshape(L, heads, -1)
        for h in range(heads):
            for h2 in range(h + 1, heads):
                if np.isfinite(blk[:, h]).all() and np.isfinite(blk[:, h2]).all():
                    assert not np.array_equal(blk[:, h], blk[:, h2]), (where, a, h, h2)
                    checked += 1
    return checked


@pytest.mark.parametrize("heads,d", [hd for hd in hc.SDDMM_HD + hc.SDDMM_HD_MORE if hd[0] > 1])
@pytest.mark.parametrize("name", hc.SDDMM_PATTERNS)
def test_sddmm_reference_tells_the_heads_apart(name, heads, d):
    m, k, rp, ci = sd.pattern(name)
    ref = hc.sddmm_reference(name, heads, d)
    p0, nnz, _ = sd.rows_of(m, rp)
    if d > 0 and nnz > 0:
        rpz = np.asarray(rp, np.int64)
        assert _rows_differ(ref, heads, rpz[:-1], np.diff(rpz), name) > 0
        assert not hc.same(hc.swap_heads(ref), ref), "the swapped-head mutant passes"
    else:  # every dot is +0: nothing to tell apart, and nothing a wrong head could change
        assert (ref[p0:p0 + nnz] == 0).all()


@pytest.mark.parametrize("heads", [h for h in hc.SOFTMAX_HEADS if h > 1])
@pytest.mark.parametrize("name", hc.SOFTMAX_PATTERNS)
def test_softmax_reference_tells_the_heads_apart(name, heads):
    """Rows of one position are left out: their softmax is 1.0 and its backward 0 in
    every head, whatever the head's values."""
    c = sc.case(name)
    for ref in (hc.softmax_forward(name, heads), hc.softmax_backward(name, heads)):
        assert _rows_differ(ref, heads, c.starts, c.lens, name, min_len=2) > 0
        assert not hc.same(hc.swap_heads(ref), ref), "the swapped-head mutant passes"


@pytest.mark.parametrize("heads,d", [hd for hd in hc.PRODUCT_HD if hd[0] > 1])
def test_product_reference_tells_the_heads_apart(heads, d):
    m, k, rp, ci = hc.product_pattern()
    for epi in (False, True):
        ref = hc.product_reference(heads, d, epi)
        lens = np.diff(np.asarray(rp, np.int64))
        rows = np.flatnonzero(lens > 0)
        assert _rows_differ(ref.reshape(m, heads * d), heads, rows, np.ones(rows.size, int), "product") > 0
        assert not hc.same(hc.swap_heads(ref), ref), "the swapped-head mutant passes"


# ------------------------------------------------------------------ checks
def test_host_entry_argument_checks():
    from ctypes import c_void_p
    L = _lib()
    lib = L.lib()
    rp = np.array([0, 2], np.int32)
    ci = np.array([0, 1], np.int32)
    f = np.zeros(64, F)
    P = lambda a: c_void_p(a.ctypes.data)  # noqa: E731
    sdd, sm = lib.spmm_sddmm_csr_heads_host_f32, lib.spmm_edge_softmax_csr_heads_host_f32
    smb, mm = lib.spmm_edge_softmax_bwd_csr_heads_host_f32, lib.spmm_csrmm_heads_host_f32
    INV, NS, OK = L.INVALID_VALUE, L.NOT_SUPPORTED, L.SUCCESS
    # heads < 1
    assert sdd(1, 4, 2, 2, 0, 1.0, P(rp), P(ci), 0, P(f), 4, P(f), 4, 0.0, P(f)) == INV
    assert sm(1, 2, 0, P(rp), 0, P(f), P(f)) == INV
    assert smb(1, 2, -1, P(rp), 0, P(f), P(f), P(f)) == INV
    assert mm(1, 4, 2, 2, 0, 1.0, P(rp), P(ci), P(f), 0, P(f), 4, 0.0, P(f), 4) == INV
    # ld below heads * d
    assert sdd(1, 4, 2, 2, 2, 1.0, P(rp), P(ci), 0, P(f), 7, P(f), 8, 0.0, P(f)) == INV
    assert mm(1, 4, 2, 2, 2, 1.0, P(rp), P(ci), P(f), 0, P(f), 8, 0.0, P(f), 7) == INV
    # nnz * heads past INT_MAX, d past 1024: refused before anything is read
    big = 1 << 30
    assert sdd(1, 4, 2, big, 4, 1.0, P(rp), P(ci), 0, P(f), 16, P(f), 16, 0.0, P(f)) == NS
    assert sdd(1, 1025, 2, 2, 1, 1.0, P(rp), P(ci), 0, P(f), 1025, P(f), 1025, 0.0, P(f)) == NS
    assert sm(1, big, 4, P(rp), 0, P(f), P(f)) == NS
    assert smb(1, big, 4, P(rp), 0, P(f), P(f), P(f)) == NS
    assert mm(1, 4, 2, big, 4, 1.0, P(rp), P(ci), P(f), 0, P(f), 16, 0.0, P(f), 16) == NS
    # quick returns, then a bad pattern
    assert sdd(0, 4, 2, 2, 2, 1.0, None, None, 0, None, 8, None, 8, 0.0, None) == INV
    assert sdd(1, 4, 2, 0, 2, 1.0, None, None, 0, None, 8, None, 8, 0.0, None) == OK
    assert mm(0, 4, 2, 2, 2, 1.0, None, None, None, 0, None, 8, 0.0, None, 8) == OK
    assert mm(1, 0, 2, 2, 2, 1.0, None, None, None, 0, None, 0, 0.0, None, 0) == OK
    bad = np.array([0, 3], np.int32)  # past nnz
    assert sm(1, 2, 2, P(bad), 0, P(f), P(f)) == INV
    assert mm(1, 4, 1, 2, 2, 1.0, P(rp), P(ci), P(f), 0, P(f), 8, 0.0, P(f), 8) == INV  # col >= k


def test_prep_wrappers_raise_on_bad_input():
    prep = _prep()
    m, k, rp, ci = sd.pattern("dups")
    X, Y = hc.sddmm_operands(m, k, 2, 3)
    with pytest.raises(ValueError):
        prep.sddmm_heads(m, 3, k, 2, rp[:-1], ci, X, Y)
    with pytest.raises(TypeError):
        prep.sddmm_heads(m, 3, k, 2, rp, ci, X.astype(np.float64), Y)
    with pytest.raises(ValueError):
        prep.sddmm_heads(m, 3, k, 2, rp, ci, X[:-1], Y)
    with pytest.raises(TypeError):
        prep.edge_softmax_heads(rp, np.zeros(ci.size, F))  # one head's 1-D layout
    with pytest.raises(TypeError):
        prep.edge_softmax_bwd_heads(rp, np.zeros((ci.size, 2), F), np.zeros((ci.size, 3), F))
    with pytest.raises(ValueError):
        prep.csrmm_heads(m, 3, k, 2, rp, ci, np.zeros((ci.size, 1), F), Y)
