"""CSR, hybrid and BSR products on padded and offset B / C layouts.

Every other GPU test passes B and C packed tight at the start of a fresh
allocation (ld = the matrix width, a 256-byte aligned base). The launchers
branch on exactly that, so here every product runs on framed operands
(helpers.framed): B and C inside larger buffers, `off` elements into them, with
`pad` extra elements per row. The gaps, the padding columns and the guards
around them hold a signalling-NaN sentinel: C's must come back bit for bit (a
read-modify-write returns the quiet form), and a B padding value read into a
sum poisons the result. At beta = 0 C's data region starts as
NaN (it must not propagate), at beta != 0 it is finite and alpha != 1.

LAYOUTS are (off_B, pad_B, off_C, pad_C) in elements; each cause of a demotion
occurs alone at least once. Which layout reaches which path, read off the
predicates (the tests never call them; ld = width + pad):

CSR fp32 row-major, csr_kernels.hip (pick_vec and the `grouped` predicate of
launch_csrmm_rowmajor); "B/C 4 (8) mod 16" is the base address modulo 16 bytes:

  layout        cause                     n > 128, n % 4 == 0   64 < n <= 128, even   n <= 64, n % 4 == 0
  (0,0,0,0)     none                      VEC 4                 VEC 2                 lane-group kernel
  (0,4,0,8)     none (ld % 4 == 0)        VEC 4                 VEC 2                 lane-group kernel
  (0,1,0,0)     ldb odd                   VEC 1                 VEC 1                 main kernel, VEC 1
  (0,0,0,1)     ldc odd                   VEC 1                 VEC 1                 main kernel, VEC 1
  (0,2,0,0)     ldb % 4 == 2              VEC 2                 VEC 2                 main kernel, VEC 1
  (0,0,0,2)     ldc % 4 == 2              VEC 2                 VEC 2                 main kernel, VEC 1
  (1,0,0,0)     B 4 mod 16                VEC 1                 VEC 1                 main kernel, VEC 1
  (0,0,1,0)     C 4 mod 16                VEC 1                 VEC 1                 main kernel, VEC 1
  (2,0,0,0)     B 8 mod 16                VEC 2                 VEC 2                 main kernel, VEC 1
  (0,0,2,0)     C 8 mod 16                VEC 2                 VEC 2                 main kernel, VEC 1
  (1,3,3,1)     both bases, ldb, ldc      VEC 1                 VEC 1                 main kernel, VEC 1
  (3,1,1,3)     both bases, ldb, ldc      VEC 1                 VEC 1                 main kernel, VEC 1

(odd n is VEC 1 on every layout; at n = 65 / 129 the last two layouts have
ld % 4 == 0 on a misaligned base.) So VEC 4 -> 2 and 4 -> 1 are reached at
n = 132 / 252 / 256 / 260 (where the column-tile count and the piece-slot stride
change with the width: n = 132 is 1 / 2 / 3 tiles), VEC 2 -> 1 at n = 66 / 126 /
128, and the main kernel at n <= 64 with default options at n = 4 / 32 / 64 on
ten layouts. With SPMM_CSR_SEQUENTIAL_ROWS every one of them is the main kernel,
whose bits are the piece oracle's at any width.

Column-major operands go through the staging transposes (transpose4_kernel:
ld = k + pad / m + pad and the offset base on the column-major side); the
product then sees the staged copy tight and aligned, and the row-major operand,
if any, with its layout as above.

Hot-column entry: hot_mode (api.cpp) is 2 at these sizes (one buffer resource,
the row offset from ldb in soffset); n = 100 / 128 are VEC 2 or 1, n = 256 VEC
4 / 2 / 1 by the table.

Hybrid bs = 32 (hybrid32_fusable, bsr_kernels.hip: n % 4, ldb % 4, ldc % 2,
bsrVal and B 16-byte, C 8-byte aligned): fused on (0,0,0,0), (0,4,0,8),
(0,0,0,2) and (0,0,2,0); two launches on the other eight and with bsrVal at an
offset of 1 or 2 floats. In the two-launch form the BSR part is the LDS
dense-block kernel while ldb % 4 == 0 and B / bsrVal are 16-byte aligned (any
C), else the register-fragment kernel (scalar B loads and C stores), else (a
misaligned bsrVal) the generic kernel; the remainder is the CSR launch above.

BSR drop-in (launch_bsrmm_f32 / launch_bsrmm_f16): the column streams (bs 32 /
64 / 16, ROW blocks) need ldb % 4 (8 for fp16) and 16-byte bsrVal and B, bs 32 /
64 also 16-byte row-major C rows; the other layouts and COLUMN blocks fall to the
register-fragment MFMA kernels (bs 16 / 32) and, with bsrVal off 16 bytes or at
bs 64, to the generic kernel; bs 2 / 8 take the lane-group VALU kernel at two
floats per lane when B is 8-byte aligned with an even ldb, else one. Neither
entry documents an alignment requirement for bsrVal, and every kernel a
misaligned bsrVal reaches (generic, lane-group VALU) loads it one element at a
time, so those cases expect the product. The BSR tests also run ALIGNED_LAYOUTS_F32 /
ALIGNED_LAYOUTS_F16 (helpers.py: 16-byte bases off the allocation's 256-byte one, ld a
multiple of 16 bytes, so every fast path stays) and a column-major B (ldb = K + pad_B at
off_B): with ROW blocks and n a multiple of the 16-byte vector it is staged row-major and
tight (bsrmm_staged: transpose4_kernel / transpose16x4_kernel read it from any element
base and ld), otherwise the direct kernels read it (register-fragment with a 16-byte B
and ldb % 4 (8) == 0, else generic)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from helpers import (ALIGNED_LAYOUTS_F16, ALIGNED_LAYOUTS_F32, TOL_F16_ACC, TOL_F32, assert_normwise,
                     framed, long_row_column_sparse_bsr, oracle_bsrmm_f64, oracle_csrmm_d,
                     oracle_csrmm_f64, oracle_csrmm_pieces_f32)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LAYOUTS = [(0, 0, 0, 0), (0, 4, 0, 8), (0, 1, 0, 0), (0, 0, 0, 1), (0, 2, 0, 0), (0, 0, 0, 2),
           (1, 0, 0, 0), (0, 0, 1, 0), (2, 0, 0, 0), (0, 0, 2, 0), (1, 3, 3, 1), (3, 1, 1, 3)]
ABS = [(1.0, 0.0), (0.7, -1.3)]
AB_IDS = ["beta0", "beta"]


def _ops():
    from spmm_hip import ops
    return ops


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _c_init(C0, beta):
    """C's data region before the call: NaN at beta = 0, the finite C0 otherwise."""
    return C0 if beta != 0.0 else np.full_like(C0, np.nan)


def _frames(Bd, Cd, lay, ob=0, oc=0):
    """Bd (k x n) and Cd (m x n) framed in the given storage orders on `lay`:
    (B view, B checker, ldb, C view, C checker, ldc, extract) with extract() the
    checked m x n result."""
    off_b, pad_b, off_c, pad_c = lay
    B2 = Bd if ob == 0 else np.ascontiguousarray(Bd.T)
    C2 = Cd if oc == 0 else np.ascontiguousarray(Cd.T)
    ldb, ldc = B2.shape[1] + pad_b, C2.shape[1] + pad_c
    dB, chkB = framed(B2, ldb, off_b)
    dC, chkC = framed(C2, ldc, off_c)

    def extract(what):
        got = chkC(what + ": C")
        return got if oc == 0 else np.ascontiguousarray(got.T)
    return dB, chkB, ldb, dC, chkC, ldc, extract


def _expect(ref, absd, C0, alpha, beta):
    """(reference, norm-wise scale) of alpha * A B + beta * C0 in float64."""
    C0 = C0.astype(np.float64)
    return alpha * ref + beta * C0, abs(alpha) * absd + abs(beta) * np.abs(C0)


# ------------------------------------------------------------------ CSR fp32
CSR_M, CSR_K = 3000, 5000
CSR_N = [4, 32, 64, 65, 66, 126, 128, 129, 132, 252, 256, 260]
_csr_cache: dict = {}


def _hub_matrix():
    """The matrix of test_power_law_hubs_and_empty_rows (tests/test_gpu_csr.py): four
    hub rows of 4000 nonzeros, rows of 0..6 otherwise, 30 % empty."""
    if "A" not in _csr_cache:
        rng = np.random.default_rng(100)
        m, k = CSR_M, CSR_K
        deg = rng.integers(0, 7, m)
        deg[rng.random(m) < 0.3] = 0
        for r in (0, 1, 1777, m - 1):
            deg[r] = 4000
        rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
        ci = np.concatenate([np.sort(rng.choice(k, d, replace=False)) for d in deg]).astype(np.int32)
        _csr_cache["A"] = rp, ci, rng.uniform(-1, 1, ci.size).astype(np.float32)
    return _csr_cache["A"]


def _csr_case(oracle, n):
    """B, C0 and the f64 oracle of the hub matrix at width n, once per n."""
    key = ("case", n)
    if key not in _csr_cache:
        rp, ci, v = _hub_matrix()
        rng = np.random.default_rng(1000 + n)
        B = rng.uniform(-1, 1, (CSR_K, n)).astype(np.float32)
        C0 = rng.uniform(-1, 1, (CSR_M, n)).astype(np.float32)
        ref, absd = oracle_csrmm_f64(oracle, CSR_M, n, rp, ci, v, B, n, 0)
        _csr_cache[key] = B, C0, ref, absd
    return _csr_cache[key]


def _csr_pieces(oracle, n, alpha, beta):
    key = ("pieces", n, alpha, beta)
    if key not in _csr_cache:
        rp, ci, v = _hub_matrix()
        B, C0, _, _ = _csr_case(oracle, n)
        _csr_cache[key] = oracle_csrmm_pieces_f32(oracle, CSR_M, n, rp, ci, v, B, n, 0, alpha=alpha,
                                                  beta=beta, C=C0).reshape(CSR_M, n)
    return _csr_cache[key]


def _csr_handles():
    from spmm_hip._lib import CSR_NT_STREAMS, CSR_SEQUENTIAL_ROWS
    ops = _ops()
    hseq, hdef = ops.Handle(), ops.Handle()
    hseq.set_csr_options(CSR_NT_STREAMS | CSR_SEQUENTIAL_ROWS)
    return hseq, hdef


def _csr_tight(oracle, n, alpha, beta, h):
    """The row-major product on plain tight tensors with handle h."""
    rp, ci, v = _hub_matrix()
    B, C0, _, _ = _csr_case(oracle, n)
    drp, dci, dv, dB, dC = _dev(rp, ci, v, B, _c_init(C0, beta))
    _ops().csrmm(drp, dci, dv, dB, n=n, k=CSR_K, ldb=n, C=dC, ldc=n, alpha=alpha, beta=beta,
                 handle=h)
    return dC.cpu().numpy()


@pytest.mark.parametrize("ab", ABS, ids=AB_IDS)
@pytest.mark.parametrize("n", CSR_N)
def test_csr_f32_rowmajor_layouts(oracle, device, n, ab):
    """spmm_csrmm_ex_f32 on every layout at 1 and 3 waves per CU (hub rows split over
    waves: piece slots and tickets in use). With SPMM_CSR_SEQUENTIAL_ROWS the result
    is the piece oracle's bit for bit whatever vector width the layout leaves; with
    default options it is within the fp32 bar of the f64 product and, in bits, either
    the default result on the tight layout or the SEQUENTIAL_ROWS result on the same
    layout (so a demoted path cannot be merely close)."""
    alpha, beta = ab
    ops = _ops()
    rp, ci, v = _hub_matrix()
    B, C0, ref, absd = _csr_case(oracle, n)
    want_seq = _csr_pieces(oracle, n, alpha, beta)
    want64, scale = _expect(ref, absd, C0, alpha, beta)
    drp, dci, dv = _dev(rp, ci, v)
    hseq, hdef = _csr_handles()
    hdef.set_csr_waves_per_cu(1)
    tight = _csr_tight(oracle, n, alpha, beta, hdef)
    assert_normwise(tight, want64, scale, TOL_F32, f"n={n} tight tensors")
    took_main = []  # per (layout, grid): default options gave other bits than on tight tensors
    for lay in LAYOUTS:
        ldb, ldc = n + lay[1], n + lay[3]
        dB, chkB = framed(B, ldb, lay[0])
        for wpc in (1, 3):
            got = {}
            for name, h in (("seq", hseq), ("default", hdef)):
                what = f"n={n} layout={lay} wpc={wpc} {name} alpha={alpha} beta={beta}"
                dC, chkC = framed(_c_init(C0, beta), ldc, lay[2])
                h.set_csr_waves_per_cu(wpc)
                ops.csrmm(drp, dci, dv, dB, n=n, k=CSR_K, ldb=ldb, C=dC, ldc=ldc, alpha=alpha,
                          beta=beta, handle=h)
                got[name] = chkC(what + ": C")
            bad = _bits(got["seq"]) != _bits(want_seq)
            assert not bad.any(), (f"n={n} layout={lay} wpc={wpc}: SEQUENTIAL_ROWS differs from the "
                                   f"piece oracle in {int(bad.any(axis=1).sum())} rows, first "
                                   f"{np.flatnonzero(bad.any(axis=1))[:5].tolist()}")
            assert_normwise(got["default"], want64, scale, TOL_F32,
                            f"n={n} layout={lay} wpc={wpc} default")
            assert _same_bits(got["default"], tight) or _same_bits(got["default"], got["seq"]), \
                (f"n={n} layout={lay} wpc={wpc}: default options give neither the tight layout's "
                 "bits nor the SEQUENTIAL_ROWS bits on this layout")
            took_main.append(not _same_bits(got["default"], tight))
        chkB.unchanged(f"n={n} layout={lay}: B")
    if n <= 64 and n % 4 == 0:
        # the lane-group kernel's interleaved chains differ in bits from the main kernel's
        # on this matrix, so the bits show which one ran: both must occur, the main kernel
        # through nothing but a layout (the options are the defaults)
        assert not _same_bits(tight, want_seq), "the two kernels' bits must differ for this check"
        assert not took_main[0] and not took_main[1], "framed but tight: the tight layout's bits"
        assert any(took_main), "no layout sent n <= 64 with default options to the main kernel"
    hseq.close()
    hdef.close()


@pytest.mark.parametrize("n", [64, 260])
def test_csr_f32_index_arrays_at_offset(oracle, device, n):
    """rowptr, colind and val one element into larger buffers (4 bytes off every
    alignment): the same bits as on fresh allocations, and nothing written to them."""
    ops = _ops()
    rp, ci, v = _hub_matrix()
    B, C0, _, _ = _csr_case(oracle, n)
    alpha, beta = ABS[1]
    h = ops.Handle()
    h.set_csr_waves_per_cu(3)
    want = _csr_tight(oracle, n, alpha, beta, h)
    frp, crp = framed(rp.reshape(1, -1), rp.size, 1, fill=0)
    fci, cci = framed(ci.reshape(1, -1), ci.size, 1, fill=0)
    fv, cv = framed(v.reshape(1, -1), v.size, 1)
    dB, dC = _dev(B, C0)
    ops.csrmm(frp[:rp.size], fci[:ci.size], fv[:v.size], dB, n=n, k=CSR_K, ldb=n, C=dC, ldc=n,
              alpha=alpha, beta=beta, handle=h)
    assert _same_bits(dC.cpu().numpy(), want)
    for chk, nm in ((crp, "rowptr"), (cci, "colind"), (cv, "val")):
        chk.unchanged(nm)
    h.close()


# column-major forms: (entry, order_b, order_c)
COL_FORMS = [("ex", 1, 1), ("ex", 0, 1), ("ex", 1, 0), ("scsrmm", 1, 1), ("scsrmm2_N", 1, 1),
             ("scsrmm2_T", 0, 1)]


def _csr_entry(form, dtype, h, m, n, k, drp, dci, dv, base, dB, ldb, dC, ldc, alpha, beta):
    """One CSR product through the entry point the form names."""
    from spmm_hip._lib import check, lib
    ops = _ops()
    entry, ob, oc = form
    if entry == "ex":
        ops.csrmm(drp, dci, dv, dB, m=m, n=n, k=k, ldb=ldb, order_b=ob, C=dC, ldc=ldc,
                  order_c=oc, alpha=alpha, beta=beta, base=base, handle=h)
        return
    ct = ctypes.c_float if dtype == np.float32 else ctypes.c_double
    a, b = ct(alpha), ct(beta)
    d = ops._Descr(base)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    tail = (ctypes.byref(a), d.raw, P(dv), P(drp), P(dci), P(dB), ldb, ctypes.byref(b), P(dC), ldc)
    if entry == "scsrmm":
        check(lib().spmm_scsrmm(h.raw, 0, m, n, k, dci.numel(), *tail), entry)
    else:
        fn = lib().spmm_scsrmm2 if dtype == np.float32 else lib().spmm_dcsrmm2
        check(fn(h.raw, 0, 1 if entry.endswith("_T") else 0, m, n, k, dci.numel(), *tail), entry)


@pytest.mark.parametrize("ab", ABS, ids=AB_IDS)
@pytest.mark.parametrize("form", COL_FORMS, ids=lambda f: f"{f[0]}-b{f[1]}c{f[2]}")
@pytest.mark.parametrize("n", [64, 130])
def test_csr_f32_colmajor_layouts(oracle, device, n, form, ab):
    """Column-major B (ldb = k + pad) and / or C (ldc = m + pad) at the same offsets,
    through spmm_csrmm_ex_f32, spmm_scsrmm and spmm_scsrmm2 (both transB); m = 3000
    and k = 5000 are no multiples of the transposes' 64 x 64 tiles. The staged copies
    are exact and the epilogue is the kernel's own, so the bits are those of the
    row-major tight call (test_colmajor_forms_match_rowmajor's contract). One case
    cannot have them: at n = 64 a row-major operand whose layout rules out the
    lane-group kernel runs the main kernel, whose bits are the SEQUENTIAL_ROWS ones
    of the tight call. Those are accepted only on layouts that offset or pad the
    row-major operand; with both operands column-major, or the row-major one tight,
    the kernel sees tight aligned operands and only the default bits are accepted."""
    alpha, beta = ab
    entry, ob, oc = form
    rp, ci, v = _hub_matrix()
    B, C0, ref, absd = _csr_case(oracle, n)
    want64, scale = _expect(ref, absd, C0, alpha, beta)
    drp, dci, dv = _dev(rp, ci, v)
    hseq, hdef = _csr_handles()
    tight = _csr_tight(oracle, n, alpha, beta, hdef)
    assert_normwise(tight, want64, scale, TOL_F32, f"n={n} tight tensors")
    tight_seq = _csr_tight(oracle, n, alpha, beta, hseq) if n <= 64 else None
    for lay in LAYOUTS:
        what = f"n={n} {entry} orders=({ob},{oc}) layout={lay} alpha={alpha} beta={beta}"
        # the SEQUENTIAL_ROWS bits only where the row-major operand is offset or padded
        accept = [tight]
        if n <= 64 and ((ob == 0 and (lay[0] or lay[1])) or (oc == 0 and (lay[2] or lay[3]))):
            accept.append(tight_seq)
        dB, chkB, ldb, dC, _, ldc, extract = _frames(B, _c_init(C0, beta), lay, ob, oc)
        _csr_entry(form, np.float32, hdef, CSR_M, n, CSR_K, drp, dci, dv, 0, dB, ldb, dC, ldc,
                   alpha, beta)
        got = extract(what)
        assert_normwise(got, want64, scale, TOL_F32, what)
        assert any(_same_bits(got, w) for w in accept), what + ": bits differ from the tight call"
        chkB.unchanged(what + ": B")
    hseq.close()
    hdef.close()


def _hot_tags(device):
    """spmm_csr_hot_analysis of the hub matrix, once: a budget (in B-row pieces of 128
    floats) that holds the columns used more often than the median, so columns go
    both ways."""
    if "tags" not in _csr_cache:
        _, ci, _ = _hub_matrix()
        cnt = np.bincount(ci, minlength=CSR_K)
        thr = int(np.median(cnt[cnt > 0])) + 1
        hot_rows = int((cnt >= thr).sum())
        assert 0 < hot_rows < int((cnt > 0).sum())
        tag = _ops().csr_hot_analysis(torch.from_numpy(ci).to(device), n=128, k=CSR_K,
                                      hot_bytes=hot_rows * 512)
        ntag = int((tag < 0).sum())
        assert 0 < ntag < ci.size, f"{ntag} of {ci.size} indices tagged: columns must go both ways"
        assert np.array_equal(tag.cpu().numpy() & 0x7fffffff, ci)
        _csr_cache["tags"] = tag
    return _csr_cache["tags"]


@pytest.mark.parametrize("ab", ABS, ids=AB_IDS)
@pytest.mark.parametrize("n", [100, 128, 256])
def test_csr_hot_entry_layouts(oracle, device, n, ab):
    """spmm_csrmm_hot_f32 (B addressed through a buffer resource built from ldb) on
    every layout: the bits of spmm_csrmm_ex_f32 on the same layout."""
    alpha, beta = ab
    ops = _ops()
    rp, ci, v = _hub_matrix()
    B, C0, ref, absd = _csr_case(oracle, n)
    want64, scale = _expect(ref, absd, C0, alpha, beta)
    tag = _hot_tags(device)
    drp, dci, dv = _dev(rp, ci, v)
    for lay in LAYOUTS:
        what = f"hot n={n} layout={lay} alpha={alpha} beta={beta}"
        ldb, ldc = n + lay[1], n + lay[3]
        dB, chkB = framed(B, ldb, lay[0])
        dC, chkC = framed(_c_init(C0, beta), ldc, lay[2])
        ops.csrmm(drp, dci, dv, dB, n=n, k=CSR_K, ldb=ldb, C=dC, ldc=ldc, alpha=alpha, beta=beta)
        plain = chkC(what + " (plain entry): C")
        dC, chkC = framed(_c_init(C0, beta), ldc, lay[2])
        ops.csrmm_hot(drp, tag, dv, dB, n=n, k=CSR_K, ldb=ldb, C=dC, ldc=ldc, alpha=alpha,
                      beta=beta)
        hot = chkC(what + ": C")
        assert_normwise(plain, want64, scale, TOL_F32, what + " (plain entry)")
        assert_normwise(hot, want64, scale, TOL_F32, what)
        assert _same_bits(hot, plain), what + ": differs from spmm_csrmm_ex_f32 on this layout"
        chkB.unchanged(what + ": B")


# ------------------------------------------------------------------ CSR fp64
F64_FORMS = [("ex", 0, 0), ("ex", 1, 1), ("ex", 0, 1), ("ex", 1, 0), ("dcsrmm2_N", 1, 1),
             ("dcsrmm2_T", 0, 1)]
_f64_cache: dict = {}


def _f64_case(n):
    if n not in _f64_cache:
        rng = np.random.default_rng(7 * n + 1)
        m, k = 517, 389
        deg = rng.integers(0, 41, m)
        deg[rng.random(m) < 0.1] = 0
        rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
        ci = np.concatenate([np.sort(rng.choice(k, d, replace=False)) for d in deg]).astype(np.int32)
        _f64_cache[n] = (m, k, rp, ci, rng.standard_normal(ci.size), rng.standard_normal((k, n)),
                         rng.standard_normal((m, n)))
    return _f64_cache[n]


@pytest.mark.parametrize("alpha,beta,base", [(1.0, 0.0, 0), (0.75, -1.5, 1)], ids=AB_IDS)
@pytest.mark.parametrize("form", F64_FORMS, ids=lambda f: f"{f[0]}-b{f[1]}c{f[2]}")
@pytest.mark.parametrize("n", [1, 7, 64, 130])
def test_csr_f64_layouts(oracle, device, n, form, alpha, beta, base):
    """spmm_csrmm_ex_f64 (all four order combinations) and spmm_dcsrmm2 (both transB)
    on every layout, in units of doubles: the sequential fp64 oracle bit for bit, as
    tests/test_gpu_f64.py asserts on tight layouts."""
    entry, ob, oc = form
    if entry != "ex":
        base = 0  # the cuSPARSE-shaped entry takes its base from the descriptor: keep 0
    m, k, rp, ci, v, B, C0 = _f64_case(n)
    want = oracle_csrmm_d(oracle, m, n, rp + base, ci + base, v, B, n, 0, alpha, beta,
                          C0.ravel(), n, 0, base).reshape(m, n)
    drp, dci, dv = _dev(rp + base, ci + base, v)
    h = _ops().default_handle()
    for lay in LAYOUTS:
        what = f"f64 n={n} {entry} orders=({ob},{oc}) layout={lay} alpha={alpha} beta={beta}"
        dB, chkB, ldb, dC, _, ldc, extract = _frames(B, _c_init(C0, beta), lay, ob, oc)
        _csr_entry(form, np.float64, h, m, n, k, drp, dci, dv, base, dB, ldb, dC, ldc, alpha, beta)
        got = extract(what)
        bad = _bits(got) != _bits(want)
        assert not bad.any(), f"{what}: {int(bad.sum())} elements differ from the fp64 oracle"
        chkB.unchanged(what + ": B")


# -------------------------------------------------------------- hybrid, bs 32
_hyb_cache: dict = {}


def _hybrid_case(oracle, K):
    """Matrix and prep.divide call of test_hybrid_fused_vs_two_launch (n = 963)."""
    if K not in _hyb_cache:
        from spmm_hip import prep
        n = 963
        rp, ci = prep.community_csr(n, 30.0, 48, 160, 0.9, 7)
        rng = np.random.default_rng(8)
        rows = [ci[rp[i]:rp[i + 1]] for i in range(n)]
        rows[1] = np.arange(0, n, 2)
        rows[n // 2] = np.sort(rng.choice(n, n // 3, replace=False))
        for i in range(n - 40, n):
            rows[i] = np.sort(rng.choice(n, 3, replace=False))
        rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        ci = np.concatenate(rows).astype(np.int32)
        v = rng.uniform(-1, 1, ci.size).astype(np.float32)
        parts = prep.divide(n, rp, ci, v, 32, 0.1)
        assert parts[4].size > 0 and parts[1].size > 0
        nb = (n + 31) // 32
        Bp = np.zeros((nb * 32, K), np.float32)
        Bp[:n] = rng.uniform(-1, 1, (n, K))
        C0 = rng.uniform(-1, 1, (nb * 32, K)).astype(np.float32)
        ref, absd = oracle_csrmm_f64(oracle, n, K, rp, ci, v, Bp, K, 0)
        _hyb_cache[K] = n, parts, Bp, C0, ref, absd
    return _hyb_cache[K]


@pytest.mark.parametrize("ab", ABS, ids=AB_IDS)
@pytest.mark.parametrize("K", [4, 132])
def test_hybrid32_layouts(oracle, device, K, ab):
    """spmm_hybrid_csrmm_f32 with default hybrid options on every layout, and with
    bsrVal 1 and 2 floats into its buffer (two launches): within the fp32 bar on the
    matrix rows, equal bit for bit (padding rows n .. nb * 32 included) to the forced
    HYBRID_FUSED or the forced HYBRID_TWO_LAUNCH result on the same layout. The padding
    rows agree between the forms as test_hybrid_fused_vs_two_launch expects, and hold
    beta * C0 (0 at beta = 0, not the NaN prefill) in every form."""
    from spmm_hip._lib import HYBRID_FUSED, HYBRID_TWO_LAUNCH
    alpha, beta = ab
    ops = _ops()
    n, parts, Bp, C0, ref, absd = _hybrid_case(oracle, K)
    want64, scale = _expect(ref, absd, C0[:n], alpha, beta)
    # rows n .. nb * 32 hold no matrix row: the BSR epilogue of a zero sum, fma(beta, C0, 0)
    # (one rounding, the fp32 product) or 0 at beta = 0 whatever C held
    want_pad = np.float32(beta) * C0[n:] if beta != 0.0 else np.zeros_like(C0[n:])
    d = _dev(*parts)
    handles = {"default": ops.Handle(), "fused": ops.Handle(), "two": ops.Handle()}
    handles["fused"].set_hybrid_options(HYBRID_FUSED)
    handles["two"].set_hybrid_options(HYBRID_TWO_LAUNCH)
    cases = [(lay, 0) for lay in LAYOUTS] + [((0, 0, 0, 0), 1), ((0, 0, 0, 0), 2)]
    forms_differ = []
    for lay, voff in cases:
        bsr = tuple(d[3:6])
        chkV = None
        if voff:
            fv, chkV = framed(parts[5].reshape(1, -1), parts[5].size, voff)
            bsr = (d[3], d[4], fv[:parts[5].size])
        out = {}
        for name, h in handles.items():
            what = f"hybrid K={K} layout={lay} bsrVal+{voff} {name} alpha={alpha} beta={beta}"
            dB, chkB, ldb, dC, _, ldc, extract = _frames(Bp, _c_init(C0, beta), lay)
            ops.hybrid_csrmm(tuple(d[0:3]), bsr, dB, m=n, n=K, k=n, bs=32, ldb=ldb, C=dC, ldc=ldc,
                             alpha=alpha, beta=beta, handle=h)
            out[name] = extract(what)
            chkB.unchanged(what + ": B")
            assert_normwise(out[name][:n], want64, scale, TOL_F32, what)
            assert np.array_equal(out[name][n:], want_pad), what + ": padding rows n .. nb * 32"
        what = f"hybrid K={K} layout={lay} bsrVal+{voff} alpha={alpha} beta={beta}"
        assert _same_bits(out["fused"][n:], out["two"][n:]), what + ": padding rows of the forms"
        assert _same_bits(out["default"], out["fused"]) or _same_bits(out["default"], out["two"]), \
            what + ": default options give neither the fused nor the two-launch bits"
        forms_differ.append(not _same_bits(out["fused"], out["two"]))
        if chkV is not None:
            chkV.unchanged(what + ": bsrVal")
    # the forced forms differ in bits where both exist (the hub rows' remainders), so the
    # comparison above tells them apart; where a layout rules the fused kernel out the
    # forced-fused handle runs two launches too
    assert forms_differ[0], "tight layout: the fused and the two-launch bits must differ"
    assert not forms_differ[-1] and not forms_differ[-2], \
        "bsrVal off 16 bytes: the fused kernel copies whole 16-byte pieces of it, two launches"
    assert not all(forms_differ[:len(LAYOUTS)]), "no layout sent the forced-fused handle to two launches"
    for h in handles.values():
        h.close()


# ------------------------------------------------------------- BSR drop-in
_bsr_cache: dict = {}


def _bsr_case(oracle, bs, n, direction, half):
    """mb = 19, kb = 27, fill 0.3, block row 2 empty (the shape of
    test_bsrmm_f32_bs32_unaligned_row_major_c) with its f64 oracle."""
    key = (bs, n, direction, half)
    if key not in _bsr_cache:
        rng = np.random.default_rng(41 + 10 * bs + direction)
        mb, kb = 19, 27
        rows = [np.nonzero(rng.random(kb) < 0.3)[0] if br != 2 else np.zeros(0, int)
                for br in range(mb)]
        rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
        ci = np.concatenate(rows).astype(np.int32)
        vt = np.float16 if half else np.float32
        v = rng.uniform(-1, 1, rp[-1] * bs * bs).astype(vt)
        B = rng.uniform(-1, 1, (kb * bs, n)).astype(vt)
        C0 = rng.uniform(-1, 1, (mb * bs, n)).astype(np.float32)
        ref, absd = oracle_bsrmm_f64(oracle, direction, mb, n, bs, rp, ci, v, B, n, 0, half=half)
        _bsr_cache[key] = mb, kb, rp, ci, v, B, C0, ref, absd
    return _bsr_cache[key]


def _bsr_layouts(oracle, bs, n, direction, ab, half):
    """Row-major C on every layout (LAYOUTS and the 16-byte ones off the 256-byte base),
    column-major C on the layouts that pad C, column-major B (ldb = K + pad_B, base at
    off_B: the staging transposes or the direct column-major-B kernels) with either C
    on the layouts that pad or offset B, and bsrVal one element into its buffer
    (row-major and column-major C, tight B / C)."""
    alpha, beta = ab
    ops = _ops()
    mb, kb, rp, ci, v, B, C0, ref, absd = _bsr_case(oracle, bs, n, direction, half)
    want64, scale = _expect(ref, absd, C0, alpha, beta)
    tol = TOL_F16_ACC if half else TOL_F32
    mm = ops.bsrmm_f16 if half else ops.bsrmm
    drp, dci, dv = _dev(rp, ci, v)
    fv, chkV = framed(v.reshape(1, -1), v.size, 1)
    lays = LAYOUTS + (ALIGNED_LAYOUTS_F16 if half else ALIGNED_LAYOUTS_F32)
    cases = [(lay, 0, 0, 0) for lay in lays] + [(lay, 0, 1, 0) for lay in lays if lay[3]] + \
        [((0, 0, 0, 0), 0, 0, 1), ((0, 0, 0, 0), 0, 1, 1)] + \
        [(lay, 1, oc, 0) for lay in lays if lay[0] or lay[1] for oc in (0, 1)]
    for lay, ob, oc, voff in cases:
        what = (f"bsr {'f16' if half else 'f32'} bs={bs} n={n} dir={direction} layout={lay} "
                f"order_b={ob} order_c={oc} bsrVal+{voff} alpha={alpha} beta={beta}")
        dB, chkB, ldb, dC, _, ldc, extract = _frames(B, _c_init(C0, beta), lay, ob, oc)
        mm(drp, dci, fv[:v.size] if voff else dv, dB, mb=mb, kb=kb, n=n, bs=bs, ldb=ldb,
           order_b=ob, C=dC, ldc=ldc, order_c=oc, alpha=alpha, beta=beta, direction=direction)
        assert_normwise(extract(what), want64, scale, tol, what)
        chkB.unchanged(what + ": B")
    chkV.unchanged("bsrVal")


@pytest.mark.parametrize("ab", ABS, ids=AB_IDS)
@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("n", [36, 136])
@pytest.mark.parametrize("bs", [2, 8, 16, 32, 64])
def test_bsrmm_f32_layouts(oracle, device, bs, n, direction, ab):
    """spmm_bsrmm_ex_f32 against oracle_bsrmm_f64 within TOL_F32 (the bar of
    test_bsrmm_f32 / test_bsrmm_f32_bs32_unaligned_row_major_c)."""
    _bsr_layouts(oracle, bs, n, direction, ab, half=False)


@pytest.mark.parametrize("ab", ABS, ids=AB_IDS)
@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("n", [136, 264])
def test_bsrmm_f16_layouts(oracle, device, n, direction, ab):
    """spmm_bsrmm_ex_f16 (bs = 16; B's layout in halves, C's in floats) against the
    exact product of the same fp16 values within TOL_F16_ACC, as test_bsrmm_f16."""
    _bsr_layouts(oracle, 16, n, direction, ab, half=True)


# the drop-in column streams' tight-run bits: fp32 layouts in floats, fp16 B parts in halves
_STREAM_LAYOUTS = {False: [(0, 4, 0, 8)] + ALIGNED_LAYOUTS_F32,
                   True: [(0, 8, 0, 8), (8, 0, 0, 0), (8, 8, 4, 8), (0, 16, 4, 8)]}
_DEMOTED_LAYOUTS = {False: [(0, 1, 0, 0), (1, 3, 3, 1), (0, 0, 1, 0)],
                    True: [(0, 4, 0, 0), (1, 3, 3, 1), (4, 0, 0, 0)]}


@pytest.mark.parametrize("ab", ABS, ids=AB_IDS)
@pytest.mark.parametrize("half", [False, True], ids=["bs32-f32", "bs16-f16"])
def test_bsrmm_column_sparse_long_rows_layouts(oracle, device, half, ab):
    """The drop-in bs 32 fp32 and bs 16 fp16 products (ROW blocks, n = 136) on the matrix
    of test_bsrmm_analysed / test_bsrmm_analysed_f16: column-sparse blocks (masked-out
    columns, explicit zero and single-column blocks), an empty block row and one of
    300 blocks (segments at bs 32). On the layouts that keep the column stream
    ((0,4,0,8) in floats / (0,8,0,8) in halves and the 16-byte bases off the 256-byte
    one) the result is the tight run's, bit for bit; on a demoted layout it is within
    the bar."""
    alpha, beta = ab
    ops = _ops()
    bs, mb, kb, n = (16, 21, 320, 136) if half else (32, 23, 320, 136)
    key = ("long", half)
    if key not in _bsr_cache:
        rng = np.random.default_rng(320 + bs)
        rp, ci, v = long_row_column_sparse_bsr(rng, mb, kb, bs)
        vt = np.float16 if half else np.float32
        v = v.astype(vt)
        B = rng.uniform(-1, 1, (kb * bs, n)).astype(vt)
        C0 = rng.uniform(-1, 1, (mb * bs, n)).astype(np.float32)
        ref, absd = oracle_bsrmm_f64(oracle, 0, mb, n, bs, rp, ci, v, B, n, 0, half=half)
        _bsr_cache[key] = rp, ci, v, B, C0, ref, absd
    rp, ci, v, B, C0, ref, absd = _bsr_cache[key]
    want64, scale = _expect(ref, absd, C0, alpha, beta)
    tol = TOL_F16_ACC if half else TOL_F32
    mm = ops.bsrmm_f16 if half else ops.bsrmm
    drp, dci, dv = _dev(rp, ci, v)
    tight = None
    for lay in [(0, 0, 0, 0)] + _STREAM_LAYOUTS[half] + _DEMOTED_LAYOUTS[half]:
        what = f"long rows {'f16' if half else 'f32'} bs={bs} layout={lay} alpha={alpha} beta={beta}"
        dB, chkB, ldb, dC, _, ldc, extract = _frames(B, _c_init(C0, beta), lay)
        mm(drp, dci, dv, dB, mb=mb, kb=kb, n=n, bs=bs, ldb=ldb, C=dC, ldc=ldc, alpha=alpha, beta=beta)
        got = extract(what)
        assert_normwise(got, want64, scale, tol, what)
        chkB.unchanged(what + ": B")
        if tight is None:
            tight = got
        elif lay in _STREAM_LAYOUTS[half]:
            assert _same_bits(got, tight), what + ": bits differ from the tight run"
