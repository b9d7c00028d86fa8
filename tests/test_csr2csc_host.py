"""spmm_csr2csc (host CSR -> CSC, the CSR form of the transpose) against the numpy
reference of its contract, bit for bit, and the argument checks of both forms that need
no device. CPU only."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from csr2csc_cases import (TAIL_SIZES, bits, matrices, reference, tail_matrix, values,
                           view_case)

NAMES = ["n1", "n200", "n256", "n257", "n4096", "n4097", "random", "skew", "wide", "dups",
         "unsorted"]


def _prep():
    from spmm_hip import prep
    return prep


def _check(got, ref, with_val, what):
    cp, ri = got[0], got[1]
    assert np.array_equal(cp, ref[0]), f"{what}: colptr"
    assert np.array_equal(ri, ref[1]), f"{what}: rowind"
    if with_val:
        assert got[2].dtype == ref[2].dtype
        assert np.array_equal(bits(got[2]), bits(ref[2])), f"{what}: val"
    assert np.array_equal(got[-1], ref[3]), f"{what}: perm"


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("vb", [0, 2, 4, 8])
def test_host_equals_numpy(name, vb):
    m, n, rp, ci = matrices()[name]
    v = values(ci.size, vb)
    got = _prep().csr2csc(m, n, rp, ci, v, return_perm=True)
    assert len(got) == (4 if vb else 3)
    _check(got, reference(m, n, rp, ci, v), vb != 0, f"{name} vb={vb}")
    assert got[0][0] == 0 and got[0][n] == ci.size


@pytest.mark.parametrize("name", ["dups", "unsorted", "n257"])
@pytest.mark.parametrize("base,base_out", [(1, 1), (1, 0), (0, 1)])
def test_host_index_bases(name, base, base_out):
    m, n, rp, ci = matrices()[name]
    v = values(ci.size, 4)
    got = _prep().csr2csc(m, n, rp + base, ci + base, v, base=base, base_out=base_out,
                          return_perm=True)
    _check(got, reference(m, n, rp + base, ci + base, v, base, base_out), True,
           f"{name} base {base}->{base_out}")
    assert got[0][0] == base_out and got[0][n] == ci.size + base_out
    # the permutation is 0-based whatever the bases
    assert np.array_equal(got[3], reference(m, n, rp, ci)[3])


def test_host_perm_is_optional_and_refreshes_values():
    m, n, rp, ci = matrices()["dups"]
    v = values(ci.size, 4)
    cp, ri, cv = _prep().csr2csc(m, n, rp, ci, v)
    ref = reference(m, n, rp, ci, v)
    assert np.array_equal(cp, ref[0]) and np.array_equal(ri, ref[1])
    assert np.array_equal(bits(cv), bits(ref[2]))
    perm = _prep().csr2csc(m, n, rp, ci, return_perm=True)[2]
    v2 = values(ci.size, 4, seed=12)
    assert np.array_equal(bits(v2[perm]), bits(_prep().csr2csc(m, n, rp, ci, v2)[2]))


@pytest.mark.parametrize("base", [0, 1])
def test_host_offset_view(base):
    m, n, rp, ci = view_case()
    assert rp[0] > 0
    v = values(ci.size, 4)
    got = _prep().csr2csc(m, n, rp + base, ci + base, v, base=base, return_perm=True)
    ref = reference(m, n, rp + base, ci + base, v, base, base)
    _check(got, ref, True, "view")
    assert got[3].min() == rp[0] and got[3].max() == rp[m] - 1


@pytest.mark.parametrize("nrows", [1, 37])
def test_host_tails(nrows):
    for nnz in TAIL_SIZES:
        m, n, rp, ci = tail_matrix(nnz, nrows)
        v = values(nnz, 4)
        got = _prep().csr2csc(m, n, rp, ci, v, return_perm=True)
        _check(got, reference(m, n, rp, ci, v), nnz > 0, f"tail nnz={nnz} rows={nrows}")


def test_host_double_transpose_returns_the_matrix():
    for name in ("dups", "random", "skew"):
        m, n, rp, ci = matrices()[name]
        v = values(ci.size, 8)
        cp, ri, cv = _prep().csr2csc(m, n, rp, ci, v)
        rp2, ci2, v2 = _prep().csr2csc(n, m, cp, ri, cv)
        assert np.array_equal(rp2, rp) and np.array_equal(ci2, ci), name
        assert np.array_equal(bits(v2), bits(v)), name


def test_host_thread_count_does_not_change_the_output(monkeypatch):
    """The fill splits the columns over the workers; every count gives the same bytes."""
    m, n, rp, ci = matrices()["skew"]
    v = values(ci.size, 4)
    outs = []
    for nt in ("1", "2", "16"):
        monkeypatch.setenv("OMP_NUM_THREADS", nt)
        outs.append(_prep().csr2csc(m, n, rp, ci, v, return_perm=True))
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert np.array_equal(bits(a) if a.dtype.kind == "f" else a,
                                  bits(b) if b.dtype.kind == "f" else b)


def _raw(L, m, n, nnz, rp, ci, v, vb, base_a=0, base_c=0, null=()):
    """spmm_csr2csc through ctypes with every output allocated; `null` names pointers
    to pass as NULL."""
    cp, ri, perm = np.zeros(n + 1, np.int32), np.zeros(max(nnz, 1), np.int32), \
        np.zeros(max(nnz, 1), np.int32)
    cv = np.zeros(max(nnz, 1), np.float64)
    P = lambda a, nm: None if nm in null else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    return L.spmm_csr2csc(m, n, nnz, P(v, "val"), P(rp, "rowptr"), P(ci, "colind"), vb, base_a,
                          base_c, P(cv, "cscval"), P(cp, "colptr"), P(ri, "rowind"),
                          P(perm, "perm"))


def test_host_error_statuses():
    from spmm_hip import _lib
    L = _lib.lib()
    m, n, rp, ci = matrices()["dups"]
    nnz = int(ci.size)
    v = values(nnz, 4)
    INVALID = _lib.INVALID_VALUE
    assert _raw(L, m, n, nnz, rp, ci, v, 4) == 0
    assert _raw(L, m, n, nnz, rp, ci, v, 4, null=("perm",)) == 0
    assert _raw(L, m, n, nnz, rp, ci, v, 0, null=("val", "cscval", "perm")) == 0
    # negative sizes
    assert _raw(L, -1, n, nnz, rp, ci, v, 4) == INVALID
    assert _raw(L, m, -1, nnz, rp, ci, v, 4) == INVALID
    assert _raw(L, m, n, -1, rp, ci, v, 4) == INVALID
    # valueBytes and bases
    for vb in (1, 3, 16, -4):
        assert _raw(L, m, n, nnz, rp, ci, v, vb) == INVALID
    assert _raw(L, m, n, nnz, rp, ci, v, 4, base_a=2) == INVALID
    assert _raw(L, m, n, nnz, rp, ci, v, 4, base_c=-1) == INVALID
    # a needed pointer that is NULL
    for nm in ("rowptr", "colind", "colptr", "rowind", "val", "cscval"):
        assert _raw(L, m, n, nnz, rp, ci, v, 4, null=(nm,)) == INVALID, nm
    # a decreasing row pointer (its ends still agree with nnz)
    dec = rp.copy()
    dec[10] = dec[12] + 1
    assert dec[11] < dec[10]
    assert _raw(L, m, n, nnz, dec, ci, v, 4) == INVALID
    # nnz that disagrees with the row pointer
    ci1, v1 = np.append(ci, 0).astype(np.int32), np.append(v, 0).astype(np.float32)
    assert _raw(L, m, n, nnz + 1, rp, ci1, v1, 4) == INVALID
    assert _raw(L, m, n, nnz - 1, rp, ci, v, 4) == INVALID
    # a row pointer that starts below the base
    assert _raw(L, m, n, nnz, rp, ci, v, 4, base_a=1) == INVALID
    # a column outside [0, n)
    for bad in (n, n + 5, -1):
        c = ci.copy()
        c[17] = bad
        assert _raw(L, m, n, nnz, rp, c, v, 4) == INVALID, bad
    assert _raw(L, m, n - 1, nnz, rp, ci, v, 4) == (INVALID if ci.max() == n - 1 else 0)
    # empty matrices are fine
    z = np.zeros(1, np.int32)
    assert _raw(L, 0, 5, 0, z, ci, v, 4) == 0
    assert _raw(L, 0, 0, 0, z, ci, v, 4) == 0


def test_prep_wrapper_raises_on_bad_input():
    from spmm_hip._lib import SpmmError
    m, n, rp, ci = matrices()["dups"]
    c = ci.copy()
    c[3] = n
    with pytest.raises(SpmmError) as e:
        _prep().csr2csc(m, n, rp, c)
    assert e.value.status == 3
    with pytest.raises(TypeError):
        _prep().csr2csc(m, n, rp, ci, np.zeros(ci.size, np.int32))
    with pytest.raises(ValueError):
        _prep().csr2csc(m, n, rp, ci[:-1])


def test_device_form_checks_that_need_no_device():
    """spmm_csr2csc_dev: a NULL handle is NOT_INITIALIZED before anything else. The
    INVALID_VALUE checks come before any device work, so they can be reached with a
    handle that is only a non-NULL address: those calls return before the handle is
    read."""
    from spmm_hip import _lib
    L = _lib.lib()
    assert L.spmm_csr2csc_dev(None, 4, 4, 4, None, None, None, None, 4, None, None, None, None,
                              None) == _lib.NOT_INITIALIZED
    assert L.spmm_csr2csc_dev(None, -1, 4, 4, None, None, None, None, 9, None, None, None, None,
                              None) == _lib.NOT_INITIALIZED
    da, dc = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.spmm_create_mat_descr(ctypes.byref(da)) == 0
    assert L.spmm_create_mat_descr(ctypes.byref(dc)) == 0
    fake = (ctypes.c_char * 4096)()  # never dereferenced: every call below is refused first
    h = ctypes.c_void_p(ctypes.addressof(fake))
    buf = np.zeros(16, np.int64)
    p = ctypes.c_void_p(buf.ctypes.data)

    def call(m=4, n=4, nnz=4, a=da, val=p, rp=p, ci=p, vb=4, c=dc, cval=p, cp=p, ri=p):
        return L.spmm_csr2csc_dev(h, m, n, nnz, a, val, rp, ci, vb, c, cval, cp, ri, None)

    INVALID = _lib.INVALID_VALUE
    assert call(m=-1) == INVALID and call(n=-1) == INVALID and call(nnz=-1) == INVALID
    assert call(a=None) == INVALID and call(c=None) == INVALID
    for vb in (1, 3, 6, 16, -2):
        assert call(vb=vb) == INVALID
    assert call(rp=None) == INVALID and call(cp=None) == INVALID
    assert call(ci=None) == INVALID and call(ri=None) == INVALID
    assert call(val=None) == INVALID and call(cval=None) == INVALID
    assert call(n=0) == INVALID  # entries without a column to hold them
    assert L.spmm_destroy_mat_descr(da) == 0 and L.spmm_destroy_mat_descr(dc) == 0
