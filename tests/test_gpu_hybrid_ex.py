"""spmm_hybrid_csrmm_ex_f32, the hybrid entry with storage orders (divide.cu's own call
shape: column-major z, transB = N or T), through ops.hybrid_csrmm(order_b=, order_c=).

The entry stages a column-major B once (a row-major ceil(k / bs) * bs x n copy, zero
rows past k) and hands that copy to both of its products: the BSR part, whose launcher
writes handle buffers of its own at some block sizes (the bs 64 panel probe's sums, the
bs 2 / 4 / 8 grouped branch's probe sums and dirty flags), and the CSR remainder. The
copy must come through all of that intact: every product here is held to the f64 oracle
of the whole matrix (helpers.oracle_csrmm_f64; alpha * ref + beta * C0 within TOL_F32 of
|alpha| |A||B| + |beta| |C0|, the bar of test_hybrid_divide_spmm) on every row of C the
call owns, ceil(m / bs) * bs of them when the BSR part is non-empty: the padding rows
hold beta * C0, exactly 0 at beta = 0 whatever C held. B and C are framed
(helpers.framed): guards, offset gap and padding columns keep their sentinel bits, B
keeps its bits, and at beta = 0 C's data region starts as NaN.

tests/test_hybrid_helpers.py checks on the host that the matrices reach the branches
named here."""
from __future__ import annotations

import ctypes
import types

import numpy as np
import pytest

from helpers import (HYBRID_EX_LAYOUTS, HYBRID_EX_M, HYBRID_EX_N, HYBRID_EX_ORDERS,
                     PROBE64_CHECKED_BLOCK_ROWS, PROBE64_MB, PROBE64_N, TOL_F32, assert_normwise,
                     framed_operands, hybrid_ex_matrix, hybrid_ex_parts, oracle_bsrmm_f64,
                     oracle_csrmm_f64, panel_probe_bsr64, probe64_block_row_reference, rand_bsr,
                     rand_csr_rows)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

COL = 1
ORDER_IDS = ["colB-colC", "rowB-colC", "colB-rowC"]
_cache: dict = {}


def _ops():
    from spmm_hip import ops
    return ops


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _pad_rows(a, rows):
    out = np.zeros((rows, a.shape[1]), a.dtype)
    out[:a.shape[0]] = a
    return out


def _c_init(C0, beta):
    return C0 if beta != 0.0 else np.full_like(C0, np.nan)


def _case(oracle, n):
    """B (700 x n), C0 (704 x n: the most rows any block size pads to) and the f64
    oracle of the whole matrix, once per n."""
    if n not in _cache:
        rp, ci, v = hybrid_ex_matrix()
        rng = np.random.default_rng(7000 + n)
        Bd = rng.uniform(-1, 1, (HYBRID_EX_M, n)).astype(np.float32)
        C0 = rng.uniform(-1, 1, (704, n)).astype(np.float32)
        ref, absd = oracle_csrmm_f64(oracle, HYBRID_EX_M, n, rp, ci, v, Bd, n, 0)
        _cache[n] = Bd, C0, ref, absd
    return _cache[n]


def _hybrid(ops, parts_dev, dB, dC, *, m, n, k, bs, ldb, ldc, ob, oc, alpha, beta, handle):
    ops.hybrid_csrmm(tuple(parts_dev[0:3]), tuple(parts_dev[3:6]), dB, m=m, n=n, k=k, bs=bs, ldb=ldb,
                     C=dC, ldc=ldc, alpha=alpha, beta=beta, order_b=ob, order_c=oc, handle=handle)


@pytest.mark.parametrize("ab", [(1.0, 0.0), (0.5, -1.5)], ids=["beta0", "beta"])
@pytest.mark.parametrize("n", HYBRID_EX_N)
@pytest.mark.parametrize("orders", HYBRID_EX_ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize("bs", [2, 4, 8, 16, 32, 64, 5])
def test_hybrid_ex_block_sizes(oracle, device, bs, orders, n, ab):
    """Every block size family (the lane-group and grouped kernels at 2 / 4 / 8, the bs 16
    and bs 32 MFMA kernels, the bs 64 sub-block stream, bsr_generic_kernel at 5) times
    the three forms with a column-major operand, at n = 64 (the 64-column tile), 136 (two
    128-column tiles, the second a tail) and 7 (no vector path), on a tight layout, a
    16-byte friendly one and one off 16 bytes. 700 is a multiple of bs only at 2, 4 and
    5: elsewhere the staged B has zeroed tail rows (a column-major B holds the 700 real
    rows only) and C has padding rows. A second handle with SPMM_BSR_SMALL_GROUPED at bs
    2 / 4 / 8 (probe sums and dirty flags in the handle scratch while the staged B is
    read), one with SPMM_HYBRID_SPLIT_BF16 at bs 32 (the column-major-C split kernel),
    also within 2^-18 |A||B| of the plain handle's result (test_hybrid_split_bf16's
    bound)."""
    from spmm_hip._lib import BSR_SMALL_GROUPED, HYBRID_SPLIT_BF16
    ops = _ops()
    ob, oc = orders
    alpha, beta = ab
    m = k = HYBRID_EX_M
    R = -(-m // bs) * bs
    Bd, C0, ref, absd = _case(oracle, n)
    C0 = C0[:R]
    parts = hybrid_ex_parts(bs)
    assert parts[1].size and parts[4].size
    d = _dev(*parts)
    want = alpha * _pad_rows(ref, R) + beta * C0.astype(np.float64)
    scale = abs(alpha) * _pad_rows(absd, R) + abs(beta) * np.abs(C0.astype(np.float64))
    want_pad = np.float32(beta) * C0[m:] if beta != 0.0 else np.zeros_like(C0[m:])
    # a column-major B needs its k real rows only; a row-major one is read to kb * bs rows
    Bh = Bd if ob == COL else _pad_rows(Bd, R)
    handles = {"default": ops.Handle()}
    if bs in (2, 4, 8):
        handles["grouped"] = ops.Handle()
        handles["grouped"].set_bsr_options(BSR_SMALL_GROUPED)
    if bs == 32:
        handles["split"] = ops.Handle()
        handles["split"].set_hybrid_options(HYBRID_SPLIT_BF16)
    for lay in HYBRID_EX_LAYOUTS:
        out = {}
        for name, h in handles.items():
            what = (f"hybrid ex bs={bs} ob={ob} oc={oc} n={n} alpha={alpha} beta={beta} "
                    f"layout={lay} {name}")
            dB, chkB, ldb, dC, ldc, extract = framed_operands(Bh, _c_init(C0, beta), lay, ob, oc)
            _hybrid(ops, d, dB, dC, m=m, n=n, k=k, bs=bs, ldb=ldb, ldc=ldc, ob=ob, oc=oc,
                    alpha=alpha, beta=beta, handle=h)
            out[name] = extract(what)
            chkB.unchanged(what + ": B")
            assert_normwise(out[name], want, scale, TOL_F32, what)
            # rows m .. R hold no matrix row: the epilogue of a zero sum, the fp32 product
            # beta * C0 (one rounding), 0 at beta = 0 whatever C held
            assert np.array_equal(out[name][m:], want_pad), what + ": padding rows"
        if "split" in out:
            assert_normwise(out["split"], out["default"], _pad_rows(absd, R), 2.0 ** -18,
                            f"hybrid ex bs=32 ob={ob} oc={oc} n={n} layout={lay}: split-bf16 "
                            "against the plain handle")
    for h in handles.values():
        h.close()


@pytest.mark.parametrize("oc", [1, 0], ids=["colC", "rowC"])
def test_hybrid_ex_bs64_panel_probe(device, oc):
    """The smallest shape at which the bs 64 branch launches panel_probe_kernel
    (4 * nnzb = 2^15): 128 x 128 dense 64 x 64 blocks per side, 64 per block row, block
    column 0 in every one, n = 8, column-major B, alpha = 1, beta = 0 onto NaN. The
    probe zeroes and sums into 16 bytes of the handle scratch: every row of C meets B
    row 0, where those bytes lay when the staged B lived there. A CSR remainder with
    entries in columns 0..3 reads the same copy. Reference: numpy float64 on the dense
    slabs of four whole block rows."""
    ops = _ops()
    if "probe" not in _cache:
        mats = panel_probe_bsr64()
        Bd = np.random.default_rng(65).uniform(-1, 1, (PROBE64_MB * 64, PROBE64_N)).astype(np.float32)
        refs = {br: probe64_block_row_reference(br, mats, Bd) for br in PROBE64_CHECKED_BLOCK_ROWS}
        _cache["probe"] = mats, Bd, refs
    mats, Bd, refs = _cache["probe"]
    m = k = PROBE64_MB * 64
    n = PROBE64_N
    brp, bci, bval, crp, cci, cv = _dev(*mats)
    what = f"hybrid ex bs=64 panel probe oc={oc}"
    dB, chkB, ldb, dC, ldc, extract = framed_operands(Bd, np.full((m, n), np.nan, np.float32),
                                                      (0, 0, 0, 0), COL, oc)
    h = ops.Handle()
    ops.hybrid_csrmm((crp, cci, cv), (brp, bci, bval), dB, m=m, n=n, k=k, bs=64, ldb=ldb, C=dC,
                     ldc=ldc, order_b=COL, order_c=oc, handle=h)
    got = extract(what)
    chkB.unchanged(what + ": B")
    h.close()
    assert np.isfinite(got).all(), what + ": a row of C was not written"
    for br, (ref, absd) in refs.items():
        assert_normwise(got[br * 64:(br + 1) * 64], ref, absd, TOL_F32, f"{what} block row {br}")


@pytest.mark.parametrize("bs", [8, 32])
def test_hybrid_ex_rectangular_and_empty_parts(oracle, device, bs):
    """m = 300, k = 500 (neither a multiple of bs) with parts built directly: a random BSR
    part whose last block row and block column reach past m and k (the rows past m land
    in C's padding rows, the columns past k meet the staged B's zero rows) plus a random
    CSR remainder, in the three forms; then under column-major B and C an empty BSR part
    (C holds m rows only), an empty remainder, and both empty with beta = 0.5
    (C = beta * C0). Reference: oracle_bsrmm_f64 + oracle_csrmm_f64 summed."""
    ops = _ops()
    rng = np.random.default_rng(300 + bs)
    m, k, n = 300, 500, 40
    mb, kb = -(-m // bs), -(-k // bs)
    R, K = mb * bs, kb * bs
    brp, bci, bval = rand_bsr(rng, mb, kb, bs, 0.15, empty_rows=(2,))
    assert (bci == kb - 1).any() and brp[mb] > brp[mb - 1]
    crp, cci, cv = rand_csr_rows(rng, m, k, 9)
    Bd = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    C0 = rng.uniform(-1, 1, (R, n)).astype(np.float32)
    rb, ab_ = oracle_bsrmm_f64(oracle, 0, mb, n, bs, brp, bci, bval, _pad_rows(Bd, K), n, 0)
    rc, ac = oracle_csrmm_f64(oracle, m, n, crp, cci, cv, Bd, n, 0)
    none_b = (np.zeros(mb + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    none_c = (np.zeros(m + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    zero = np.zeros((R, n))
    cases = [("both", (crp, cci, cv), (brp, bci, bval), rb + _pad_rows(rc, R), ab_ + _pad_rows(ac, R),
              o, 0.7, -1.3) for o in HYBRID_EX_ORDERS]
    cases += [("both beta 0", (crp, cci, cv), (brp, bci, bval), rb + _pad_rows(rc, R),
               ab_ + _pad_rows(ac, R), (COL, COL), 1.0, 0.0),
              ("nnzb 0", (crp, cci, cv), none_b, rc, ac, (COL, COL), 0.7, -1.3),
              ("nnzb 0 beta 0", (crp, cci, cv), none_b, rc, ac, (COL, COL), 1.0, 0.0),
              ("csrNnz 0", none_c, (brp, bci, bval), rb, ab_, (COL, COL), 0.7, -1.3),
              ("both empty", none_c, none_b, zero[:m], zero[:m], (COL, COL), 1.0, 0.5)]
    h = ops.Handle()
    for name, csr, bsr, ref, absd, (ob, oc), alpha, beta in cases:
        rows = ref.shape[0]  # R with a BSR part, m without
        what = f"hybrid ex {m}x{k} bs={bs} {name} ob={ob} oc={oc} alpha={alpha} beta={beta}"
        c0 = C0[:rows]
        want = alpha * ref + beta * c0.astype(np.float64)
        scale = abs(alpha) * absd + abs(beta) * np.abs(c0.astype(np.float64))
        Bh = Bd if ob == COL else _pad_rows(Bd, K)
        for lay in [(0, 0, 0, 0), (1, 3, 1, 1)]:
            dB, chkB, ldb, dC, ldc, extract = framed_operands(Bh, _c_init(c0, beta), lay, ob, oc)
            ops.hybrid_csrmm(tuple(_dev(*csr)), tuple(_dev(*bsr)), dB, m=m, n=n, k=k, bs=bs, ldb=ldb,
                             C=dC, ldc=ldc, alpha=alpha, beta=beta, order_b=ob, order_c=oc, handle=h)
            got = extract(f"{what} layout={lay}")
            chkB.unchanged(f"{what} layout={lay}: B")
            assert_normwise(got, want, scale, TOL_F32, f"{what} layout={lay}")
    h.close()


def test_hybrid_ex_status_codes(device):
    """The argument checks of spmm_hybrid_csrmm_ex_f32 (api.cpp), each through the status
    ops.hybrid_csrmm raises: storage orders outside ROW / COL, ldb short of k (column-major
    B) or of n (row-major B), ldc short of the ceil(m / bs) * bs rows a column-major C
    holds with a BSR part (ldc = m is accepted without one), a null handle. Every buffer
    is large enough for the call a missing check would let through."""
    from spmm_hip._lib import INVALID_VALUE, NOT_INITIALIZED, SpmmError
    ops = _ops()
    bs, n = 8, 8
    m = k = HYBRID_EX_M
    R = -(-m // bs) * bs
    parts = hybrid_ex_parts(bs)
    d = _dev(*parts)
    csr, bsr = tuple(d[0:3]), tuple(d[3:6])
    none_b = tuple(_dev(np.zeros(R // bs + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)))
    B = torch.zeros(2 * R * n, device=device)
    C = torch.zeros(2 * R * n, device=device)
    h = ops.Handle()

    def call(status, bsr_=bsr, handle=h, **kw):
        a = dict(m=m, n=n, k=k, bs=bs, ldb=k, ldc=R, order_b=COL, order_c=COL)
        a.update(kw)
        if status is None:
            ops.hybrid_csrmm(csr, bsr_, B, C=C, handle=handle, **a)
            torch.cuda.synchronize()
            return
        with pytest.raises(SpmmError) as e:
            ops.hybrid_csrmm(csr, bsr_, B, C=C, handle=handle, **a)
        assert e.value.status == status, (kw, e.value)

    call(None)
    for bad in (2, -1, 7):
        call(INVALID_VALUE, order_b=bad)
        call(INVALID_VALUE, order_c=bad)
        call(INVALID_VALUE, order_b=bad, order_c=0, ldc=n)
    call(INVALID_VALUE, ldb=k - 1)                       # column-major B: ldb >= k
    call(None, order_b=0, ldb=n)
    call(INVALID_VALUE, order_b=0, ldb=n - 1)            # row-major B: ldb >= n
    call(INVALID_VALUE, order_c=0, ldc=n - 1)            # row-major C: ldc >= n
    call(INVALID_VALUE, ldc=R - 1)                       # column-major C with a BSR part
    call(INVALID_VALUE, ldc=m)
    call(None, bsr_=none_b, ldc=m)                       # ... and without one: m rows
    call(INVALID_VALUE, bsr_=none_b, ldc=m - 1)
    call(NOT_INITIALIZED, handle=types.SimpleNamespace(raw=ctypes.c_void_p()))
    h.close()
