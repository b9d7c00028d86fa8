"""spmm_sddmm_csr_host_f32 (the sampled dense-dense product's rule in executable form,
prep.sddmm) against numpy: float64 for the tolerance, an independent restatement of the
association rule for the bits; its invariances; and the argument checks of both entries
that need no device. CPU only."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from helpers import TOL_F32, assert_normwise, reversed_rows
from sddmm_cases import (N_LIST, N_WIDE, bits, group_lanes, old_values, operands, pattern,
                         reference64, reference_bits, rows_of)

NAMES = ["n200", "random", "dups", "unsorted", "view"]
ALPHA, BETA = 1.7, -0.6
SENTINEL = np.float32(12345.5)


def _prep():
    from spmm_hip import prep
    return prep


def test_group_lanes_of_the_rule():
    """G(n) = min(64, max(1, pow2ceil(ceil(n / 4)))): 128, 64, 32, 16 and <= 4 columns
    put 2, 4, 8, 16 and 64 positions into a wave instruction, 256 and more one."""
    assert [group_lanes(n) for n in (0, 1, 4, 5, 8, 16, 32, 60, 64, 68, 128, 132, 256, 260,
                                     515, 1030)] == [1, 1, 1, 2, 2, 4, 8, 16, 16, 32, 32, 64,
                                                     64, 64, 64, 64]


@pytest.mark.parametrize("n", N_LIST + [N_WIDE])
@pytest.mark.parametrize("name", NAMES)
def test_host_within_tolerance_of_float64(name, n):
    """Chain plus fold: at most (n / (4 G) * 4 + log2 G) * 2^-24 * sum |x||y|, under
    2e-6 at n <= 1030, against TOL_F32 = 1e-5. Bases 0 and 1, alpha and beta away from
    1 and 0; positions outside a view stay as they were."""
    m, k, rp, ci = pattern(name)
    X, Y = operands(m, k, n)
    p0, nnz, rows = rows_of(m, rp)
    cols = ci[p0:p0 + nnz]
    old = old_values(ci.size)
    for base in (0, 1):
        for alpha, beta in ((1.0, 0.0), (ALPHA, BETA)):
            out = old.copy() if beta != 0.0 else np.full(ci.size, SENTINEL)
            before = out.copy()
            got = _prep().sddmm(m, n, k, rp + base, ci + base, X, Y, out=out, alpha=alpha,
                                beta=beta, base=base)
            assert got is out
            ref, absd = reference64(rows, cols, X, Y, alpha, beta, old[p0:p0 + nnz])
            assert_normwise(got[p0:p0 + nnz], ref, absd, TOL_F32,
                            f"{name} n={n} base={base} alpha={alpha} beta={beta}")
            outside = np.ones(ci.size, bool)
            outside[p0:p0 + nnz] = False
            assert np.array_equal(bits(got[outside]), bits(before[outside]))


@pytest.mark.parametrize("n", [3, 64, 68, 132, 260])
@pytest.mark.parametrize("name", ["dups", "n200"])
def test_host_bits_equal_the_restated_rule(name, n):
    m, k, rp, ci = pattern(name)
    X, Y = operands(m, k, n)
    p0, nnz, rows = rows_of(m, rp)
    old = old_values(ci.size)
    for alpha, beta in ((1.0, 0.0), (ALPHA, BETA)):
        got = _prep().sddmm(m, n, k, rp, ci, X, Y, out=old.copy(), alpha=alpha, beta=beta)
        want = reference_bits(rows, ci, X, Y, alpha, beta, old)
        bad = np.flatnonzero(bits(got) != bits(want))
        assert bad.size == 0, (f"{name} n={n} alpha={alpha} beta={beta}: {bad.size} of {nnz} "
                               f"differ, first at {bad[:1]}: {got[bad[:1]]} vs {want[bad[:1]]}")


def test_restated_rule_is_not_the_sequential_chain():
    """The bits reference is sensitive to the association: at n = 132 it differs from
    one sequential chain somewhere on the matrix (the test above could not tell the rule
    from any other sum otherwise)."""
    m, k, rp, ci = pattern("dups")
    X, Y = operands(m, k, 132)
    _, _, rows = rows_of(m, rp)
    seq = np.zeros(ci.size, np.float32)
    for c in range(132):
        seq = (seq.astype(np.float64) + X[rows, c].astype(np.float64) * Y[ci, c]).astype(np.float32)
    assert (bits(seq) != bits(reference_bits(rows, ci, X, Y))).any()


@pytest.mark.parametrize("n", [5, 64, 132, 260])
def test_equal_pairs_give_equal_outputs(n):
    """The bits of an output depend on its two rows alone: duplicate (row, col) entries
    of `dups` agree, wherever they sit."""
    m, k, rp, ci = pattern("dups")
    X, Y = operands(m, k, n)
    _, _, rows = rows_of(m, rp)
    got = bits(_prep().sddmm(m, n, k, rp, ci, X, Y))
    key = rows.astype(np.int64) * k + ci
    order = np.argsort(key, kind="stable")
    same = key[order][1:] == key[order][:-1]
    assert same.sum() >= 3  # row 7 alone holds (3, 3, 3) and (64, 64)
    assert np.array_equal(got[order][1:][same], got[order][:-1][same])


@pytest.mark.parametrize("n", [16, 68, 260])
@pytest.mark.parametrize("name", ["unsorted", "random"])
def test_reversed_rows_permute_the_outputs(name, n):
    m, k, rp, ci = pattern(name)
    X, Y = operands(m, k, n)
    got = bits(_prep().sddmm(m, n, k, rp, ci, X, Y))
    rp2, ci2, pos = reversed_rows(rp, ci, np.arange(ci.size))
    got2 = bits(_prep().sddmm(m, n, k, rp2, ci2, np.ascontiguousarray(X[::-1]), Y))
    assert not np.array_equal(pos, np.arange(ci.size))
    assert np.array_equal(got2, got[pos])


def _flat(A, ld, off):
    buf = np.full(off + A.shape[0] * ld + 3, np.nan, np.float32)
    buf[off:off + A.shape[0] * ld].reshape(A.shape[0], ld)[:, :A.shape[1]] = A
    return buf[off:]


@pytest.mark.parametrize("n", [3, 64, 68, 260])
def test_padded_ld_and_offset_change_nothing(n):
    m, k, rp, ci = pattern("n200")
    X, Y = operands(m, k, n)
    want = bits(_prep().sddmm(m, n, k, rp, ci, X, Y))
    for (ox, px, oy, py) in ((1, 0, 0, 0), (0, 4, 0, 1), (1, 1, 1, 3), (4, 4, 1, 0)):
        got = _prep().sddmm(m, n, k, rp, ci, _flat(X, n + px, ox), _flat(Y, n + py, oy),
                            ldx=n + px, ldy=n + py)
        assert np.array_equal(bits(got), want), (n, ox, px, oy, py)
    # X and Y the same buffer (the pattern as a square one of max(m, k) rows)
    s = max(m, k)
    H = operands(s, s, n)[1]
    rows = rows_of(m, rp)[2]
    got = _prep().sddmm(m, n, s, rp, ci, H, H)
    assert np.array_equal(bits(got), bits(reference_bits(rows, ci, H, H)))


def test_thread_count_changes_nothing(monkeypatch):
    m, k, rp, ci = pattern("random")  # 12 K positions: more than one worker's share
    assert ci.size >= 2 * 4096
    X, Y = operands(m, k, 132)
    outs = []
    for nt in ("1", "2", "16"):
        monkeypatch.setenv("OMP_NUM_THREADS", nt)
        outs.append(bits(_prep().sddmm(m, 132, k, rp, ci, X, Y, alpha=ALPHA)))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


def _args(m=4, n=8, k=4, nnz=4, ldx=8, ldy=8, base=0, null=(), beta=0.0, rp=None, ci=None):
    keep = {"rp": np.array([0, 1, 2, 3, 4], np.int32) if rp is None else rp,
            "ci": np.array([0, 1, 2, 3], np.int32) if ci is None else ci,
            "X": np.ones(64, np.float32), "Y": np.ones(64, np.float32),
            "out": np.zeros(8, np.float32)}
    P = lambda nm: None if nm in null else ctypes.c_void_p(keep[nm].ctypes.data)  # noqa: E731
    return keep, (m, n, k, nnz, 2.0, P("rp"), P("ci"), base, P("X"), ldx, P("Y"), ldy, beta,
                  P("out"))


def test_host_entry_argument_checks():
    from spmm_hip import _lib
    L = _lib.lib()
    INVALID = _lib.INVALID_VALUE

    def call(**kw):
        keep, a = _args(**kw)
        return L.spmm_sddmm_csr_host_f32(*a), keep["out"]

    st, out = call()
    assert st == 0 and np.array_equal(out[:4], np.full(4, 16.0, np.float32))
    for kw in (dict(m=-1), dict(n=-1), dict(k=-1), dict(nnz=-1), dict(base=2), dict(base=-1),
               dict(ldx=7), dict(ldy=7), dict(null=("rp",)), dict(null=("ci",)),
               dict(null=("out",)), dict(null=("X",)), dict(null=("Y",))):
        assert call(**kw)[0] == INVALID, kw
    # quick returns: nothing is read or written
    assert call(m=0, null=("rp", "ci", "X", "Y", "out"), nnz=0)[0] == 0
    assert call(nnz=0, null=("rp", "ci", "X", "Y", "out"))[0] == 0
    st, out = call(m=0)
    assert st == 0 and not out.any()
    # n = 0: the dot is +0, X and Y are not needed
    st, out = call(n=0, ldx=0, ldy=0, null=("X", "Y"))
    assert st == 0 and np.array_equal(bits(out[:4]), np.zeros(4, np.uint32))
    # what the host form finds in the data, before it writes anything
    for kw in (dict(ci=np.array([0, 1, 2, 4], np.int32)), dict(ci=np.array([0, -1, 2, 3], np.int32)),
               dict(rp=np.array([0, 2, 1, 3, 4], np.int32)), dict(base=1),
               dict(rp=np.array([0, 1, 2, 3, 5], np.int32))):
        st, out = call(**kw)
        assert st == INVALID and not out.any(), kw


def test_device_entry_checks_that_need_no_device():
    """spmm_sddmm_csr_f32: a NULL handle is NOT_INITIALIZED before anything else; the
    INVALID_VALUE checks and the quick returns come before the handle is read, so a
    handle that is only a non-NULL address reaches them."""
    from spmm_hip import _lib
    L = _lib.lib()
    assert L.spmm_sddmm_csr_f32(None, *_args()[1]) == _lib.NOT_INITIALIZED
    assert L.spmm_sddmm_csr_f32(None, *_args(m=-1)[1]) == _lib.NOT_INITIALIZED
    fake = (ctypes.c_char * 4096)()  # never dereferenced: every call below returns first
    h = ctypes.c_void_p(ctypes.addressof(fake))
    for kw in (dict(m=-1), dict(n=-1), dict(k=-1), dict(nnz=-1), dict(base=2), dict(ldx=7),
               dict(ldy=7), dict(null=("rp",)), dict(null=("ci",)), dict(null=("out",)),
               dict(null=("X",)), dict(null=("Y",))):
        keep, a = _args(**kw)
        assert L.spmm_sddmm_csr_f32(h, *a) == _lib.INVALID_VALUE, kw
    for kw in (dict(m=0), dict(nnz=0), dict(m=0, nnz=0, null=("rp", "ci", "X", "Y", "out"))):
        keep, a = _args(**kw)
        assert L.spmm_sddmm_csr_f32(h, *a) == 0 and not keep["out"].any(), kw


def test_prep_wrapper_raises_on_bad_input():
    from spmm_hip._lib import SpmmError
    m, k, rp, ci = pattern("dups")
    X, Y = operands(m, k, 16)
    with pytest.raises(ValueError):
        _prep().sddmm(m + 1, 16, k, rp, ci, X, Y)
    with pytest.raises(TypeError):
        _prep().sddmm(m, 16, k, rp, ci, X.astype(np.float64), Y)
    with pytest.raises(ValueError):
        _prep().sddmm(m, 16, k, rp, ci, X, Y[:-1])
    with pytest.raises(SpmmError) as e:
        _prep().sddmm(m, 16, k - 100, rp, ci, X, Y)  # columns beyond the k given
    assert e.value.status == 3
