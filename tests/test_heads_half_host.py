"""The host forms of the fp16 / bf16-feature multi-head entries
(spmm_sddmm_csr_heads_host_f16 / _bf16, spmm_csrmm_heads_host_f16 / _bf16; prep.sddmm_heads
and prep.csrmm_heads on float16 arrays or uint16 patterns with bf16=True) against the fp32
host forms on the widened arrays, bit for bit. The operands are fp32 values rounded to the
storage type (heads_half_cases), so widening them back is the identity and the comparison
has no tolerance."""
from __future__ import annotations

from ctypes import c_void_p

import numpy as np
import pytest

import heads_cases as hc
import heads_half_cases as hh
import sddmm_cases as sd
from heads_cases import F


def _prep():
    from spmm_hip import prep
    return prep


def _lib():
    from spmm_hip import _lib
    return _lib


# ------------------------------------------------------------------ sampled product
@pytest.mark.parametrize("ty", hh.TYPES)
@pytest.mark.parametrize("heads,d", hc.SDDMM_HD + hc.SDDMM_HD_MORE)
@pytest.mark.parametrize("name", hc.SDDMM_PATTERNS)
def test_sddmm_heads_half_equals_f32_on_widened(name, heads, d, ty):
    """Every pattern ("view" included: rowptr[0] > 0, NaN outside stays) and shape; then
    alpha / beta on old values with padded ldx / ldy, one element into the buffers, base 1."""
    prep = _prep()
    m, k, rp, ci = sd.pattern(name)
    xb, yb, xw, yw = hh.sddmm_operands(m, k, heads, d, ty)
    X, kw = hh.stored(xb, ty)
    Y, _ = hh.stored(yb, ty)
    got = prep.sddmm_heads(m, d, k, heads, rp, ci, X, Y, out=np.full((ci.size, heads), np.nan, F),
                           **kw)
    hc.assert_same(got, hh.sddmm_reference(name, heads, d, ty), f"{name} {heads}x{d} {ty}")
    w = heads * d
    bx, _ = hh.padded16(xb.reshape(m, w), w + 3, 1)
    by, _ = hh.padded16(yb.reshape(k, w), w + 5, 1)
    got = prep.sddmm_heads(m, d, k, heads, rp + 1, ci + 1, hh.stored(bx[1:], ty)[0],
                           hh.stored(by[1:], ty)[0], ldx=w + 3, ldy=w + 5,
                           out=hc.sddmm_old(ci.size, heads).copy(), alpha=hc.ALPHA, beta=hc.BETA,
                           base=1, **kw)
    hc.assert_same(got, hh.sddmm_reference(name, heads, d, ty, True),
                   f"{name} {heads}x{d} {ty} padded, alpha beta, base 1")


# ------------------------------------------------------------------ product
@pytest.mark.parametrize("ty", hh.TYPES)
@pytest.mark.parametrize("heads,d", hc.PRODUCT_HD)
def test_csrmm_heads_half_equals_f32_on_widened(heads, d, ty):
    """heads_cases.product_pattern(): rows of 0, 1, 127, 128, 129, 256, 257, 1000 and 8193
    nonzeros; then alpha / beta on old C with padded ldb / ldc, base 1."""
    prep = _prep()
    m, k, rp, ci, val, bb, _, C = hh.product_operands(heads, d, ty)
    B, kw = hh.stored(bb, ty)
    got = prep.csrmm_heads(m, d, k, heads, rp, ci, val, B, **kw)
    hc.assert_same(np.asarray(got).reshape(m, heads, d), hh.product_reference(heads, d, ty),
                   f"{heads}x{d} {ty}")
    w = heads * d
    pb, _ = hh.padded16(bb.reshape(k, w), w + 3, 1)
    cb, cv = hc.padded(C.reshape(m, w), w + 2, fill=-7.25)
    prep.csrmm_heads(m, d, k, heads, rp + 1, ci + 1, val, hh.stored(pb[1:], ty)[0], ldb=w + 3,
                     C=cb, ldc=w + 2, alpha=hc.ALPHA, beta=hc.BETA, base=1, **kw)
    hc.assert_same(cv[:, :w].reshape(m, heads, d), hh.product_reference(heads, d, ty, True),
                   f"{heads}x{d} {ty} padded, alpha beta, base 1")
    assert (cv[:, w:] == F(-7.25)).all(), "the padding of C was written"


@pytest.mark.parametrize("ty", hh.TYPES)
def test_csrmm_heads_half_on_a_rowptr_view(ty):
    prep = _prep()
    heads, d = 3, 5
    m, k, rp, ci, val, bb, _, _ = hh.product_operands(heads, d, ty, True)
    B, kw = hh.stored(bb, ty)
    r0, r1 = 3, 30  # rows [3, 30): rowptr[0] > 0 and rowptr[m] < nnz, the full colind / val
    got = prep.csrmm_heads(r1 - r0, d, k, heads, rp[r0:r1 + 1], ci, val, B, **kw)
    hc.assert_same(got, hh.product_reference(heads, d, ty, False, True)[r0:r1], "rowptr view")


# ------------------------------------------------------------------ the two types
def test_the_same_patterns_mean_different_values_to_the_two_types():
    """The fp16 patterns of the operands, handed to the bf16 entry, give other results (and
    the other way round): a test that passes cannot have mixed the two entries up."""
    prep = _prep()
    m, k, rp, ci = sd.pattern("random")
    heads, d = 8, 8
    xb, yb, _, _ = hh.sddmm_operands(m, k, heads, d, "f16")
    as16 = prep.sddmm_heads(m, d, k, heads, rp, ci, xb.view(np.float16), yb.view(np.float16))
    asbf = prep.sddmm_heads(m, d, k, heads, rp, ci, xb, yb, bf16=True)
    hc.assert_same(as16, hh.sddmm_reference("random", heads, d, "f16"), "f16")
    assert np.isfinite(as16).all() and np.isfinite(asbf).all()
    assert (as16 != asbf).mean() > 0.9
    pm, pk, prp, pci, val, bb, _, _ = hh.product_operands(heads, d, "bf16", True)
    cbf = prep.csrmm_heads(pm, d, pk, heads, prp, pci, val, bb, bf16=True)
    c16 = prep.csrmm_heads(pm, d, pk, heads, prp, pci, val, bb.view(np.float16))
    hc.assert_same(cbf, hh.product_reference(heads, d, "bf16", False, True), "bf16")
    nonempty = np.diff(prp) > 0
    assert (np.asarray(cbf)[nonempty] != np.asarray(c16)[nonempty]).mean() > 0.9


# ------------------------------------------------------------------ edge values
@pytest.mark.parametrize("ty", hh.TYPES)
def test_sddmm_edge_values_reach_their_outputs_with_the_f32_bits(ty):
    """One edge pattern in one X[r, h, c] and in one Y[j, h, c]: the outputs that do not
    reference it keep their bits, the ones that do have the fp32 form's bits on the widened
    arrays (and are non-finite for inf and NaN)."""
    prep = _prep()
    m, k, rp, ci = sd.pattern("random")
    heads, d = 3, 5
    xb, yb, _, _ = hh.sddmm_operands(m, k, heads, d, ty)
    base_out = hh.sddmm_reference("random", heads, d, ty)
    rows = np.repeat(np.arange(m), np.diff(np.asarray(rp, np.int64)))
    r, j = int(rows[ci.size // 2]), int(ci[ci.size // 2])
    for what, pat in hh.EDGE_BITS[ty]:
        for side in "XY":
            x2, y2 = xb.copy(), yb.copy()
            hit = np.zeros((ci.size, heads), bool)
            if side == "X":
                x2[r, 1, 2] = pat
                hit[rows == r, 1] = True
            else:
                y2[j, 2, 4] = pat
                hit[np.asarray(ci) == j, 2] = True
            assert hit.any()
            kw = hh.stored(x2, ty)[1]
            got = prep.sddmm_heads(m, d, k, heads, rp, ci, hh.stored(x2, ty)[0],
                                   hh.stored(y2, ty)[0], **kw)
            want = prep.sddmm_heads(m, d, k, heads, rp, ci, hh.widen(x2, ty), hh.widen(y2, ty))
            hc.assert_same(got, want, f"{ty} {what} in {side}")
            hc.assert_same(got[~hit], base_out[~hit], f"{ty} {what} in {side}: other outputs")
            if what in ("+inf", "-inf", "nan"):
                assert not np.isfinite(got[hit]).any(), (ty, what, side)


@pytest.mark.parametrize("ty", hh.TYPES)
def test_csrmm_edge_values_reach_their_outputs_with_the_f32_bits(ty):
    prep = _prep()
    heads, d = 3, 5
    m, k, rp, ci, val, bb, _, _ = hh.product_operands(heads, d, ty, True)
    base_out = hh.product_reference(heads, d, ty, False, True)
    rows = np.repeat(np.arange(m), np.diff(np.asarray(rp, np.int64)))
    j = int(ci[int(rp[8]) + 500])  # a column of the 1000-nonzero row
    hit = np.zeros((m, heads, d), bool)
    hit[np.unique(rows[np.asarray(ci) == j]), 2, 3] = True
    for what, pat in hh.EDGE_BITS[ty]:
        b2 = bb.copy()
        b2[j, 2, 3] = pat
        B, kw = hh.stored(b2, ty)
        got = np.asarray(prep.csrmm_heads(m, d, k, heads, rp, ci, val, B, **kw))
        want = prep.csrmm_heads(m, d, k, heads, rp, ci, val, hh.widen(b2, ty))
        hc.assert_same(got, want, f"{ty} {what}")
        hc.assert_same(got[~hit], base_out[~hit], f"{ty} {what}: other outputs")
        if what in ("+inf", "-inf", "nan"):
            assert not np.isfinite(got[hit]).any(), (ty, what)


@pytest.mark.parametrize("ty", hh.TYPES)
def test_subnormals_and_signed_zeros_are_kept(ty):
    """A product of the smallest subnormal with 1.0 is that subnormal widened (nothing is
    flushed), and -0 features give -0 * val terms whose sum keeps the fp32 rule's sign."""
    prep = _prep()
    rp = np.array([0, 1, 2], np.int32)
    ci = np.array([0, 1], np.int32)
    one = int(hh.to_bits(np.array([1.0], F), ty)[0])
    tiny = F(2.0 ** -24 if ty == "f16" else 2.0 ** -133)
    Bb = np.array([[0x0001, 0x8001], [0x8000, 0x0000]], np.uint16).reshape(2, 1, 2)
    val = np.array([[1.0], [1.0]], F)
    B, kw = hh.stored(Bb, ty)
    C = np.asarray(prep.csrmm_heads(2, 2, 2, 1, rp, ci, val, B, **kw)).reshape(2, 2)
    assert C[0, 0] == tiny and C[0, 1] == -tiny
    hc.assert_same(C, prep.csrmm_heads(2, 2, 2, 1, rp, ci, val, hh.widen(Bb, ty)).reshape(2, 2),
                   "zeros")
    Xb = np.array([[one, one], [one, one]], np.uint16).reshape(2, 1, 2)
    e = prep.sddmm_heads(2, 2, 2, 1, rp, ci, hh.stored(Xb, ty)[0], B, **kw)
    assert e[0, 0] == 0 and e.shape == (2, 1)  # tiny - tiny
    Xb2 = np.array([[one, 0], [one, 0]], np.uint16).reshape(2, 1, 2)
    e = prep.sddmm_heads(2, 2, 2, 1, rp, ci, hh.stored(Xb2, ty)[0], B, **kw)
    assert e[0, 0] == tiny


# ------------------------------------------------------------------ checks
def test_all_eight_symbols_are_exported_and_bound():
    L = _lib()
    lib = L.lib()
    for ty in hh.TYPES:
        for name in (f"spmm_sddmm_csr_heads_{ty}", f"spmm_sddmm_csr_heads_host_{ty}",
                     f"spmm_csrmm_heads_{ty}", f"spmm_csrmm_heads_host_{ty}"):
            assert name in L._PROTOS, name
            fn = getattr(lib, name)
            assert fn.argtypes == L._PROTOS[name][1] and fn.restype is L._PROTOS[name][0], name


@pytest.mark.parametrize("ty", hh.TYPES)
def test_host_refusals_equal_the_f32_forms(ty):
    """The same bad arguments to the fp32 host form and to the half one: the same status,
    case by case (the half form passes 16-bit buffers of the same element counts)."""
    L = _lib()
    lib = L.lib()
    rp = np.array([0, 2], np.int32)
    ci = np.array([0, 1], np.int32)
    f, hbuf = np.zeros(4096, F), np.zeros(4096, np.uint16)
    o1, o2 = np.zeros(4096, F), np.zeros(4096, F)  # the outputs of the two forms
    P = lambda a: None if a is None else c_void_p(a.ctypes.data)  # noqa: E731
    bad_rp = np.array([0, 3], np.int32)   # past nnz
    dec_rp = np.array([2, 0], np.int32)   # decreasing
    big = 1 << 30
    INV, NS, OK = L.INVALID_VALUE, L.NOT_SUPPORTED, L.SUCCESS
    # (m, d, k, nnz, heads, rowptr, colind, base, X / Y given, ldx, ldy, out given), expected
    sdd_cases = [
        ((1, 4, 2, 2, 0, rp, ci, 0, True, 4, 4, True), INV),       # heads < 1
        ((-1, 4, 2, 2, 2, rp, ci, 0, True, 8, 8, True), INV),      # m < 0
        ((1, 4, 2, 2, 2, rp, ci, 2, True, 8, 8, True), INV),       # another base
        ((1, 4, 2, 2, 2, rp, ci, 0, True, 7, 8, True), INV),       # ldx < heads d
        ((1, 4, 2, 2, 2, rp, ci, 0, True, 8, 7, True), INV),       # ldy < heads d
        ((1, 4, 2, 2, 2, rp, ci, 0, False, 8, 8, True), INV),      # X, Y NULL
        ((1, 4, 2, 2, 2, rp, ci, 0, True, 8, 8, False), INV),      # out NULL
        ((0, 4, 2, 2, 2, None, None, 0, False, 8, 8, False), INV), # NULL before the quick return
        ((1, 4, 2, 0, 2, None, None, 0, False, 8, 8, False), OK),  # nnz = 0
        ((1, 4, 2, big, 4, rp, ci, 0, True, 16, 16, True), NS),    # nnz heads > INT_MAX
        ((1, 1025, 2, 2, 1, rp, ci, 0, True, 1025, 1025, True), NS),  # d > 1024
        ((1, 4, 2, 2, 2, bad_rp, ci, 0, True, 8, 8, True), INV),   # rowptr[m] past nnz
        ((1, 4, 2, 2, 2, dec_rp, ci, 0, True, 8, 8, True), INV),   # rowptr[m] < rowptr[0]
        ((1, 4, 1, 2, 2, rp, ci, 0, True, 8, 8, True), INV),       # column >= k
        ((1, 4, 2, 2, 2, rp, ci, 0, True, 8, 8, True), OK),
        ((1, 0, 2, 2, 2, rp, ci, 0, False, 0, 0, True), OK),       # d = 0 reads no features
    ]
    f32, half = lib.spmm_sddmm_csr_heads_host_f32, getattr(lib, "spmm_sddmm_csr_heads_host_" + ty)
    for (m, d, k, nnz, heads, r, c, base, feats, ldx, ldy, out), want in sdd_cases:
        a = f32(m, d, k, nnz, heads, 1.0, P(r), P(c), base, P(f if feats else None), ldx,
                P(f if feats else None), ldy, 0.0, P(o1 if out else None))
        b = half(m, d, k, nnz, heads, 1.0, P(r), P(c), base, P(hbuf if feats else None), ldx,
                 P(hbuf if feats else None), ldy, 0.0, P(o2 if out else None))
        assert a == want and b == want, (ty, "sddmm", m, d, k, nnz, heads, a, b, want)
    # (m, d, k, nnz, heads, rowptr, colind, val given, base, B given, ldb, C given, ldc)
    mm_cases = [
        ((1, 4, 2, 2, 0, rp, ci, True, 0, True, 4, True, 4), INV),      # heads < 1
        ((1, 4, 2, 2, 2, rp, ci, True, 3, True, 8, True, 8), INV),      # another base
        ((0, 4, 2, 2, 2, None, None, False, 0, False, 8, False, 8), OK),  # m = 0
        ((1, 0, 2, 2, 2, None, None, False, 0, False, 0, False, 0), OK),  # d = 0
        ((1, 4, 2, 2, 2, None, ci, True, 0, True, 8, True, 8), INV),    # rowptr NULL
        ((1, 4, 2, 2, 2, rp, ci, True, 0, False, 8, True, 8), INV),     # B NULL
        ((1, 4, 2, 2, 2, rp, ci, False, 0, True, 8, True, 8), INV),     # val NULL
        ((1, 4, 2, 2, 2, rp, ci, True, 0, True, 8, False, 8), INV),     # C NULL
        ((1, 4, 2, 2, 2, rp, ci, True, 0, True, 7, True, 8), INV),      # ldb < heads d
        ((1, 4, 2, 2, 2, rp, ci, True, 0, True, 8, True, 7), INV),      # ldc < heads d
        ((1, 4, 2, big, 4, rp, ci, True, 0, True, 16, True, 16), NS),   # nnz heads > INT_MAX
        ((1, 4, 2, 2, 2, bad_rp, ci, True, 0, True, 8, True, 8), INV),  # rowptr[m] past nnz
        ((1, 4, 1, 2, 2, rp, ci, True, 0, True, 8, True, 8), INV),      # column >= k
        ((1, 4, 0, 2, 2, rp, ci, True, 0, False, 8, True, 8), INV),     # k = 0 and a column
        ((1, 4, 2, 2, 2, rp, ci, True, 0, True, 8, True, 8), OK),
    ]
    f32, half = lib.spmm_csrmm_heads_host_f32, getattr(lib, "spmm_csrmm_heads_host_" + ty)
    for (m, d, k, nnz, heads, r, c, v, base, Bg, ldb, Cg, ldc), want in mm_cases:
        a = f32(m, d, k, nnz, heads, 1.0, P(r), P(c), P(f if v else None), base,
                P(f if Bg else None), ldb, 0.0, P(o1 if Cg else None), ldc)
        b = half(m, d, k, nnz, heads, 1.0, P(r), P(c), P(f if v else None), base,
                 P(hbuf if Bg else None), ldb, 0.0, P(o2 if Cg else None), ldc)
        assert a == want and b == want, (ty, "csrmm", m, d, k, nnz, heads, a, b, want)


def test_prep_wrappers_raise_on_bad_input():
    prep = _prep()
    m, k, rp, ci = sd.pattern("dups")
    xb, yb, xw, yw = hh.sddmm_operands(m, k, 2, 3, "f16")
    X, Y = xb.view(np.float16), yb.view(np.float16)
    with pytest.raises(TypeError):
        prep.sddmm_heads(m, 3, k, 2, rp, ci, X, yw)            # mixed types
    with pytest.raises(TypeError):
        prep.sddmm_heads(m, 3, k, 2, rp, ci, xb, yb)           # uint16 without bf16=True
    with pytest.raises(TypeError):
        prep.sddmm_heads(m, 3, k, 2, rp, ci, X, Y, bf16=True)  # float16 with bf16=True
    with pytest.raises(TypeError):
        prep.sddmm_heads(m, 3, k, 2, rp, ci, X, Y, out=np.zeros((ci.size, 2), np.float16))
    with pytest.raises(ValueError):
        prep.sddmm_heads(m, 3, k, 2, rp, ci, X[:-1], Y)
    with pytest.raises(TypeError):
        prep.csrmm_heads(m, 3, k, 2, rp, ci, np.zeros((ci.size, 2), np.float16), Y)  # half val
    with pytest.raises(TypeError):
        prep.csrmm_heads(m, 3, k, 2, rp, ci, np.zeros((ci.size, 2), F), Y.astype(np.float64))
