"""IEEE edge values through the CSR, hot-column, fp64, SDDMM, autograd, BSR and hybrid
entries: infinities and NaNs, signed zeros, subnormals, sums that overflow.

Operands come from the value classes of tests/edge_cases.py (S subnormals, Z signed
zeros, O overflow, N non-finite), whose sums are the same in every association order,
so one float64 numpy reference serves the merge-path kernel, the lane-group kernel, the
SDDMM butterfly and the MFMA streams alike. What the classes pin:

  every sum starts from +0 (an empty row, and a row whose products are all -0, give +0;
  the sign of a zero output then follows from alpha, beta and C);
  subnormal inputs and outputs are kept, never flushed;
  a non-finite value reaches exactly the outputs whose row references it (a prefetch
  with a clamped index must be dropped by a select, not by a zero weight).

tests/test_edge_cases_host.py proves on the host that each class detects the wrong
behaviour it is named for at every shape used here. Every comparison in this file is on
integer views (uint32 / uint64); NaN positions are compared as a map, payloads not at
all. There is no tolerance in this file."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import edge_cases as E
from helpers import framed, framed_operands

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FINITE = ["S", "Z", "O"]  # the BSR and hybrid entries: their non-finite contract has its own tests


def _ops():
    from spmm_hip import ops
    return ops


def _dev(*arrs):
    return [torch.from_numpy(np.array(a, order="C")).cuda() for a in arrs]  # a writable copy


def _c_init(C0, beta):
    """C before the call: NaN at beta = 0 (never read), C0 otherwise."""
    return C0 if beta != 0.0 else np.full_like(C0, np.nan)


def _csr_handles(ops):
    """(name, handle) over the handle options and the two grids."""
    from spmm_hip._lib import CSR_NT_STREAMS, CSR_SEQUENTIAL_ROWS
    for opt, oname in ((0, "default"), (CSR_NT_STREAMS, "nt"), (CSR_SEQUENTIAL_ROWS, "seq")):
        for wpc in (0, 1):
            h = ops.Handle()
            h.set_csr_options(opt)
            if wpc:
                h.set_csr_waves_per_cu(wpc)
            yield f"{oname} waves/CU={wpc or 'default'}", h
            h.close()


# ------------------------------------------------------------------ CSR, fp32
@pytest.mark.parametrize("n", E.CSR_N)
@pytest.mark.parametrize("cls", E.CLASSES)
def test_csrmm_ex_f32(device, cls, n):
    """spmm_csrmm_ex_f32, row-major: the lane-group kernel at every group width and
    prefetch depth (n <= 64), the merge-path kernel at vector widths 1, 2 and 4, under
    every handle option and on two grids; the hub row is cut across waves (24 pieces)."""
    ops = _ops()
    c, wants = E.csr_case(cls, n), E.csr_wants(cls, n)
    drp, dci, dv, dB = _dev(c["rp"], c["ci"], c["val"], c["B"])
    for name, h in _csr_handles(ops):
        for (alpha, beta), want in wants.items():
            C, = _dev(_c_init(c["C0"], beta))
            ops.csrmm(drp, dci, dv, dB, n=n, k=c["k"], ldb=n, C=C, ldc=n, alpha=alpha, beta=beta,
                      handle=h)
            E.assert_bits(C.cpu().numpy(), want,
                          f"class {cls} n={n} {name} alpha={alpha} beta={beta}")


CSR_FORMS = [(1, 1, 0, (0, 0, 0, 0)), (0, 1, 0, (0, 0, 0, 0)), (1, 0, 0, (0, 0, 0, 0)),
             (0, 0, 1, (0, 0, 0, 0)), (0, 0, 0, (4, 4, 12, 8)), (0, 0, 0, (1, 1, 1, 3)),
             (1, 1, 1, (1, 1, 1, 3))]  # (order_b, order_c, base, (off_B, pad_B, off_C, pad_C))


@pytest.mark.parametrize("n", E.CSR_N_LAYOUT)
@pytest.mark.parametrize("cls", E.CLASSES)
def test_csrmm_ex_f32_orders_base_layouts(device, cls, n):
    """Column-major B and / or C (staged copies), index base 1, padded and offset
    ldb / ldc between sentinel guards (helpers.framed)."""
    ops = _ops()
    c, wants = E.csr_case(cls, n), E.csr_wants(cls, n)
    dv, = _dev(c["val"])
    for ob, oc, base, lay in CSR_FORMS:
        drp, dci = _dev(c["rp"] + base, c["ci"] + base)
        for (alpha, beta), want in wants.items():
            what = f"class {cls} n={n} ob={ob} oc={oc} base={base} {lay} alpha={alpha} beta={beta}"
            dB, chkB, ldb, dC, ldc, extract = framed_operands(c["B"], _c_init(c["C0"], beta), lay,
                                                              ob, oc)
            ops.csrmm(drp, dci, dv, dB, m=c["m"], n=n, k=c["k"], ldb=ldb, order_b=ob, C=dC,
                      ldc=ldc, order_c=oc, alpha=alpha, beta=beta, base=base)
            E.assert_bits(extract(what), want, what)
            chkB.unchanged(what + ": B")


@pytest.mark.parametrize("cls", E.CLASSES)
def test_gespmm_and_scsrmm2_f32(device, cls):
    """The drop-ins: spmm_gespmm_csrmm_f32 (C overwritten, no alpha / beta) at n = 32 and
    128, and the cuSPARSE-shaped spmm_scsrmm2 (transB: row-major B, column-major C)."""
    from spmm_hip._lib import check, lib
    ops = _ops()
    for n in E.GESPMM_N:
        c, wants = E.csr_case(cls, n), E.csr_wants(cls, n)
        drp, dci, dv, dB = _dev(c["rp"], c["ci"], c["val"], c["B"])
        C = torch.full((c["m"], n), float("nan"), device=device)
        ops.gespmm_csrmm(drp, dci, dv, dB, C)
        E.assert_bits(C.cpu().numpy(), wants[(1.0, 0.0)], f"gespmm class {cls} n={n}")
    n = 36
    c, wants = E.csr_case(cls, n), E.csr_wants(cls, n)
    drp, dci, dv, dB = _dev(c["rp"], c["ci"], c["val"], c["B"])
    h, d = ops.default_handle(), ops._Descr(0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for (alpha, beta), want in wants.items():
        C, = _dev(np.ascontiguousarray(_c_init(c["C0"], beta).T))
        a, b = ctypes.c_float(alpha), ctypes.c_float(beta)
        check(lib().spmm_scsrmm2(h.raw, 0, 1, c["m"], n, c["k"], dci.numel(), ctypes.byref(a),
                                 d.raw, P(dv), P(drp), P(dci), P(dB), n, ctypes.byref(b), P(C),
                                 c["m"]), "spmm_scsrmm2")
        E.assert_bits(C.cpu().numpy().T, want, f"scsrmm2 class {cls} alpha={alpha} beta={beta}")


def _piece_bytes(n):
    tile = 256 if n > 128 else (128 if n > 64 else 64)
    return 4 * (n if n < tile else tile)


@pytest.mark.parametrize("n", E.HOT_N)
@pytest.mark.parametrize("cls", E.CLASSES)
def test_csrmm_hot_f32(device, cls, n):
    """spmm_csrmm_hot_f32 on the tags of spmm_csr_hot_analysis, at budgets of 10, 20, 40
    and 60 B rows: at one of them at least, some of class N's special B rows are hot and
    others cold (both gather policies meet an inf / NaN row)."""
    ops = _ops()
    c, wants = E.csr_case(cls, n), E.csr_wants(cls, n)
    drp, dci, dv, dB = _dev(c["rp"], c["ci"], c["val"], c["B"])
    mixed = both = False
    for hot_rows in (10, 20, 40, 60):
        tag = ops.csr_hot_analysis(dci, n=n, k=c["k"], hot_bytes=hot_rows * _piece_bytes(n))
        t = tag.cpu().numpy()
        assert np.array_equal(t & 0x7fffffff, c["ci"])
        both |= 0 < (t < 0).sum() < t.size
        hot = set(np.unique(c["ci"][t < 0]).tolist()) & set(E.SPECIAL_B_ROWS)
        mixed |= 0 < len(hot) < len(E.SPECIAL_B_ROWS)
        for (alpha, beta), want in wants.items():
            C, = _dev(_c_init(c["C0"], beta))
            ops.csrmm_hot(drp, tag, dv, dB, n=n, k=c["k"], ldb=n, C=C, ldc=n, alpha=alpha,
                          beta=beta)
            E.assert_bits(C.cpu().numpy(), want,
                          f"hot class {cls} n={n} hot_rows={hot_rows} alpha={alpha} beta={beta}")
    assert both, "no budget exercises both gather policies"
    assert mixed, "no budget tags some special B rows hot and leaves others cold"


# ------------------------------------------------------------------------ fp64
@pytest.mark.parametrize("n", E.F64_N)
@pytest.mark.parametrize("cls", E.CLASSES)
def test_csrmm_f64(device, cls, n):
    """spmm_csrmm_ex_f64 (both row-major and both column-major) and spmm_gespmm_csrmm_f64
    on the fp64 classes: units of 2^-1074, DBL_MAX."""
    ops = _ops()
    c, wants = E.csr_case(cls, n, "f64"), E.csr_wants(cls, n, "f64")
    drp, dci, dv, dB = _dev(c["rp"], c["ci"], c["val"], c["B"])
    dBt, = _dev(c["B"].T)
    for (alpha, beta), want in wants.items():
        what = f"f64 class {cls} n={n} alpha={alpha} beta={beta}"
        C, = _dev(_c_init(c["C0"], beta))
        ops.csrmm(drp, dci, dv, dB, n=n, k=c["k"], ldb=n, C=C, ldc=n, alpha=alpha, beta=beta)
        E.assert_bits(C.cpu().numpy(), want, what, "f64")
        C, = _dev(_c_init(c["C0"], beta).T)
        ops.csrmm(drp, dci, dv, dBt, m=c["m"], n=n, k=c["k"], ldb=c["k"], order_b=1, C=C,
                  ldc=c["m"], order_c=1, alpha=alpha, beta=beta)
        E.assert_bits(C.cpu().numpy().T, want, what + " column-major", "f64")
    C = torch.full((c["m"], n), float("nan"), dtype=torch.float64, device=device)
    ops.gespmm_csrmm(drp, dci, dv, dB, C)
    E.assert_bits(C.cpu().numpy(), wants[(1.0, 0.0)], f"f64 gespmm class {cls} n={n}", "f64")


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("bs", [2, 16])
@pytest.mark.parametrize("cls", FINITE)
def test_bsrmm_f64(device, cls, bs, direction):
    ops = _ops()
    n = 7 if bs == 2 else 64
    c = E.bsr_case_of(cls, "rand", bs, n, "f64", direction)
    drp, dci, dv, dB = _dev(c["brp"], c["bci"], c["val"], c["B"])
    for (alpha, beta), want in c["wants"].items():
        C, = _dev(_c_init(c["C0"], beta))
        ops.bsrmm(drp, dci, dv, dB, mb=E.BSR_MB, kb=E.BSR_KB, n=n, bs=bs, ldb=n, C=C, ldc=n,
                  alpha=alpha, beta=beta, direction=direction)
        E.assert_bits(C.cpu().numpy(), want,
                      f"f64 bsr class {cls} bs={bs} dir={direction} alpha={alpha} beta={beta}",
                      "f64")


# ----------------------------------------------------------------------- SDDMM
def _sddmm_check(ops, c, wants, what, X=None, Y=None, ldx=None, ldy=None, host=True):
    from spmm_hip import prep
    n = c["X"].shape[1]
    sl = slice(c["p0"], c["p0"] + c["nnz"])
    d_rp, d_ci = _dev(c["rp"], c["ci"])
    if X is None:
        X, Y = _dev(c["X"], c["Y"])
    got = None
    for (alpha, beta), want in wants.items():
        old = c["old"] if beta != 0.0 else np.full_like(c["old"], np.nan)
        out = ops.sddmm(d_rp, d_ci, X, Y, m=c["m"], n=n, k=c["k"], ldx=ldx, ldy=ldy,
                        out=_dev(old)[0], alpha=alpha, beta=beta)
        got = out.cpu().numpy()
        E.assert_bits(got[sl], want, f"{what} alpha={alpha} beta={beta}")
        rest = np.ones(got.size, bool)
        rest[sl] = False  # outside a view nothing is written
        assert np.array_equal(got[rest].view(np.uint32), old[rest].view(np.uint32)), what
        if host:
            hw = prep.sddmm(c["m"], n, c["k"], c["rp"], c["ci"], c["X"], c["Y"], out=old.copy(),
                            alpha=alpha, beta=beta)
            E.assert_bits(got[sl], hw[sl], f"{what} alpha={alpha} beta={beta}: prep.sddmm")
    return got[sl]


@pytest.mark.parametrize("n", E.SDDMM_N)
@pytest.mark.parametrize("name", E.SDDMM_PATTERNS)
@pytest.mark.parametrize("cls", E.CLASSES)
def test_sddmm_f32(device, cls, name, n):
    """spmm_sddmm_csr_f32 at every lane-group width, the ragged scalar and vector forms,
    the full, the multi-chunk and the wide kernel, against the order-free reference and
    the host form. Class N: the NaN in X row 7 reaches exactly that row's positions, the
    +inf row 5 of Y exactly the positions of column 5."""
    c, wants = E.sddmm_case(cls, name, n), E.sddmm_wants(cls, name, n)
    got = _sddmm_check(_ops(), c, wants, f"sddmm class {cls} {name} n={n}")
    if cls == "N":
        assert np.isnan(got[c["rows"] == 7]).all()
        assert not np.isfinite(got[c["cols"] == 5]).any()
        clean = ~np.isin(c["rows"], (7, 9)) & ~np.isin(c["cols"], E.SPECIAL_B_ROWS)
        assert clean.any() and np.isfinite(got[clean]).all()


@pytest.mark.parametrize("cls", E.CLASSES)
def test_sddmm_offset_by_one_float(device, cls):
    """X and Y one float off 16 bytes with odd leading dimensions: the scalar loads."""
    n = 68
    c, wants = E.sddmm_case(cls, "dups", n), E.sddmm_wants(cls, "dups", n)
    dX, chkX = framed(c["X"], n + 1, 1)
    dY, chkY = framed(c["Y"], n + 1, 1)
    _sddmm_check(_ops(), c, wants, f"sddmm class {cls} offset", dX, dY, n + 1, n + 1, host=False)
    chkX.unchanged("X")
    chkY.unchanged("Y")


def test_sddmm_x_is_y_nonfinite(device):
    """X and Y the same buffer holding class N's values: <h_i, h_j> on a square pattern."""
    from sddmm_cases import pattern, rows_of
    ops = _ops()
    n = 68
    m, k, rp, ci = pattern("unsorted")
    s = max(m, k)
    rng = np.random.default_rng(68)
    H = E.plant_b(rng.choice(E.value_sets("N", "f32")[1], (s, n)).astype(np.float32))
    _, _, rows = rows_of(m, rp)
    want = E.reference_dots(rows, ci.astype(np.int64), H, H, 1.0, 0.0, None)
    nan = np.isnan(want)
    assert nan.any() and not nan.all() and (want[~nan] != 0).any()
    d_rp, d_ci, dH = _dev(rp, ci, H)
    got = ops.sddmm(d_rp, d_ci, dH, dH, m=m, n=n, k=s).cpu().numpy()
    E.assert_bits(got, want, "sddmm X is Y, class N")


# -------------------------------------------------------------------- autograd
def test_autograd_spmm_val_nonfinite_grad(device):
    """autograd.spmm(A, B, val=w) with class N in grad_C: B.grad = A^T grad_C on the kept
    transpose and w.grad = the gathered dot products, NaN maps and bits of the order-free
    references."""
    from spmm_hip import autograd
    K = 36
    rp, ci, rows = E.csr_pattern()
    m, k = E.CSR_M, E.CSR_K
    rng = np.random.default_rng(36)
    w, Bh, G = E.fill("N", "f32", rng, ci.size, (k, K), (m, K))
    G = E.plant_b(G.copy())
    cols = ci.astype(np.int64)
    E.check_order_free("N", cols, w, rows, G, k, None)
    # A^T as COO: rows and columns swapped
    want_B = E.reference(cols, w, rows, G, k, 1.0, 0.0, None)
    want_w = E.reference_dots(rows, cols, G, Bh, 1.0, 0.0, None)
    for want in (want_B, want_w):
        nan = np.isnan(want)
        assert nan.any() and not nan.all()
    drp, dci, dw, dB, dG = _dev(rp, ci, w, Bh, G)
    A = autograd.CsrMatrix(drp, dci, torch.zeros_like(dw), m, k)
    dw.requires_grad_(True)
    dB.requires_grad_(True)
    autograd.spmm(A, dB, val=dw).backward(dG)
    E.assert_bits(dB.grad.cpu().numpy(), want_B, "B.grad")
    E.assert_bits(dw.grad.cpu().numpy(), want_w, "w.grad")


# ------------------------------------------------------------------ BSR, fp32
def _bsr_run(ops, c, bs, n, direction, ob, what, handle=None, path=None):
    drp, dci, dv = _dev(c["brp"], c["bci"], c["val"])
    dB, = _dev(c["B"] if ob == 0 else c["B"].T)
    for (alpha, beta), want in c["wants"].items():
        C, = _dev(_c_init(c["C0"], beta))
        ops.bsrmm(drp, dci, dv, dB, mb=E.BSR_MB, kb=E.BSR_KB, n=n, bs=bs,
                  ldb=n if ob == 0 else E.BSR_KB * bs, order_b=ob, C=C, ldc=n, alpha=alpha,
                  beta=beta, direction=direction, handle=handle)
        if path is not None:
            assert handle.small_bsr_path() in path, f"{what}: not the kernel the case is for"
        E.assert_bits(C.cpu().numpy(), want, f"{what} alpha={alpha} beta={beta}")


@pytest.mark.parametrize("n", E.BSR_N)
@pytest.mark.parametrize("bs", [2, 4, 8])
@pytest.mark.parametrize("cls", FINITE)
def test_bsrmm_small_f32(device, cls, bs, n):
    """bs 2 / 4 / 8: the lane-group VALU kernel (default) and, under
    SPMM_BSR_SMALL_GROUPED, the grouped MFMA stream, which a pattern of shared columns
    keeps (path 1) and whose probe may give a uniform one up (path 2); both block
    directions, row- and column-major B."""
    from spmm_hip._lib import BSR_SMALL_GROUPED
    ops = _ops()
    h0, hg = ops.Handle(), ops.Handle()
    hg.set_bsr_options(BSR_SMALL_GROUPED)
    for kind, gpath in (("shared", (1,)), ("rand", (1, 2))):
        for direction, ob in ((0, 0), (1, 0), (0, 1)):
            c = E.bsr_case_of(cls, kind, bs, n, "f32", direction)
            what = f"bsr class {cls} {kind} bs={bs} n={n} dir={direction} ob={ob}"
            _bsr_run(ops, c, bs, n, direction, ob, what + " default", h0, (0,))
            if ob == 0:  # the grouped stream takes a row-major B
                _bsr_run(ops, c, bs, n, direction, ob, what + " grouped", hg, gpath)
    h0.close()
    hg.close()


@pytest.mark.parametrize("n", E.BSR_N)
@pytest.mark.parametrize("bs", [16, 32, 64])
@pytest.mark.parametrize("cls", FINITE)
def test_bsrmm_mfma_f32(device, cls, bs, n):
    """bs 16 / 32 / 64 on the MFMA column streams: dense random blocks, and at n = 64
    column-sparse blocks (explicit all-zero blocks, single-column blocks)."""
    ops = _ops()
    for kind in ("rand",) + (("colsparse",) if n == 64 and bs != 64 else ()):
        # both block directions at n = 64 (the references of bs 64 are the file's largest)
        for direction, ob in ((0, 0), (1, 0), (0, 1), (1, 1)) if n == 64 else ((0, 0), (0, 1)):
            c = E.bsr_case_of(cls, kind, bs, n, "f32", direction)
            _bsr_run(ops, c, bs, n, direction, ob,
                     f"bsr class {cls} {kind} bs={bs} n={n} dir={direction} ob={ob}")


@pytest.mark.parametrize("cls", FINITE)
def test_bsr32_analysed_and_grouped_f32(device, cls):
    """The analysed and grouped bs 32 entries promise the drop-in's bits."""
    ops = _ops()
    n, bs = 128, 32
    for direction in (0, 1):
        c = E.bsr_case_of(cls, "colsparse", bs, n, "f32", direction)
        drp, dci, dv, dB = _dev(c["brp"], c["bci"], c["val"], c["B"])
        masks, vcol = ops.bsr32_analysis(dv, nnzb=c["bci"].size, direction=direction)
        grp = ops.GroupedBsr32(drp, dci, dv, mb=E.BSR_MB, group_rows=2, direction=direction)
        for (alpha, beta), want in c["wants"].items():
            what = f"class {cls} dir={direction} alpha={alpha} beta={beta}"
            C, = _dev(_c_init(c["C0"], beta))
            ops.bsrmm_analysed(drp, dci, vcol, masks, dB, mb=E.BSR_MB, kb=E.BSR_KB, n=n, ldb=n,
                               C=C, ldc=n, alpha=alpha, beta=beta)
            E.assert_bits(C.cpu().numpy(), want, "analysed bs 32 " + what)
            C, = _dev(_c_init(c["C0"], beta))
            grp.mm(dB, kb=E.BSR_KB, n=n, ldb=n, C=C, ldc=n, alpha=alpha, beta=beta)
            E.assert_bits(C.cpu().numpy(), want, "grouped bs 32 " + what)
        grp.close()


# ------------------------------------------------------------------ BSR, fp16
@pytest.mark.parametrize("n", E.BSR_F16_N)
@pytest.mark.parametrize("cls", ["S", "Z"])
def test_bsrmm_f16(device, cls, n):
    """spmm_bsrmm_ex_f16 at bs 16 with half subnormals (units of 2^-24) in A and B, and
    signed zeros; at n = 128 the analysed and grouped fp16 entries too."""
    ops = _ops()
    bs = 16
    for direction, ob in ((0, 0), (1, 0), (0, 1)):
        c = E.bsr_case_of(cls, "colsparse", bs, n, "f16", direction)
        drp, dci, dv = _dev(c["brp"], c["bci"], c["val"])
        dB, = _dev(c["B"] if ob == 0 else c["B"].T)
        extra = n == 128 and ob == 0
        if extra:
            masks, vcol = ops.bsr16_analysis(dv, nnzb=c["bci"].size, direction=direction)
            grp = ops.GroupedBsr16(drp, dci, dv, mb=E.BSR_MB, direction=direction)
        for (alpha, beta), want in c["wants"].items():
            what = f"f16 class {cls} n={n} dir={direction} ob={ob} alpha={alpha} beta={beta}"
            C, = _dev(_c_init(c["C0"], beta))
            ops.bsrmm_f16(drp, dci, dv, dB, mb=E.BSR_MB, kb=E.BSR_KB, n=n, bs=bs,
                          ldb=n if ob == 0 else E.BSR_KB * bs, order_b=ob, C=C, ldc=n,
                          alpha=alpha, beta=beta, direction=direction)
            E.assert_bits(C.cpu().numpy(), want, "bsrmm_f16 " + what)
            if extra:
                C, = _dev(_c_init(c["C0"], beta))
                ops.bsrmm_analysed_f16(drp, dci, vcol, masks, dB, mb=E.BSR_MB, kb=E.BSR_KB, n=n,
                                       ldb=n, C=C, ldc=n, alpha=alpha, beta=beta)
                E.assert_bits(C.cpu().numpy(), want, "analysed " + what)
                C, = _dev(_c_init(c["C0"], beta))
                grp.mm(dB, kb=E.BSR_KB, n=n, ldb=n, C=C, ldc=n, alpha=alpha, beta=beta)
                E.assert_bits(C.cpu().numpy(), want, "grouped " + what)
        if extra:
            grp.close()


# ---------------------------------------------------------------------- hybrid
@pytest.mark.parametrize("n", E.HYBRID_N)
@pytest.mark.parametrize("cls", FINITE)
def test_hybrid_csrmm_f32(device, cls, n):
    """ops.hybrid_csrmm at bs 32 on the community matrix's parts: the row-major entry and
    the storage-order entry (column-major B and C), held to the entry's own two-product
    form (the BSR part writes C with beta, the CSR remainder accumulates): each part is
    order-free, and parts that cancel exactly give +0. Rows 700 .. 703 of C hold no
    matrix row: the epilogue of an empty sum."""
    ops = _ops()
    c = E.hybrid_case(cls, n)
    d = _dev(*c["parts"])
    m, R = c["m"], c["R"]
    for ob, oc in ((0, 0), (1, 1)):
        # a column-major B holds its k real rows only; a row-major one whole blocks
        Bh = c["B"] if ob == 0 else c["B"][:m]
        for (alpha, beta), want in c["wants"].items():
            what = f"hybrid class {cls} n={n} ob={ob} oc={oc} alpha={alpha} beta={beta}"
            dB, chkB, ldb, dC, ldc, extract = framed_operands(Bh, _c_init(c["C0"], beta),
                                                              (0, 0, 0, 0), ob, oc)
            ops.hybrid_csrmm(tuple(d[0:3]), tuple(d[3:6]), dB, m=m, n=n, k=m, bs=E.HYBRID_BS,
                             ldb=ldb, C=dC, ldc=ldc, alpha=alpha, beta=beta, order_b=ob,
                             order_c=oc)
            E.assert_bits(extract(what), want, what)
            chkB.unchanged(what + ": B")
