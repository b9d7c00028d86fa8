"""Dense-operand offsets past 2^31 and 2^32 at every product entry.

Every case puts exactly one dense operand of a call (B, C, X, Y) on a geometry of
tests/far_cases.py: a strided view into one uninitialised 12-GiB arena whose rows start past
2^31 bytes, 2^32 bytes and 2^31 elements, of which only the rows and columns the case uses
are written and read back. The other operands are ordinary helpers.framed buffers. The
matrices are the smallest that reference every far row (the crossing rows and the last row
several times); values are independent uniforms per row, so a gather of the wrong row is off
by O(1), not by a rounding.

What is pinned, one window per launcher bound:
  hot_mode (csrc/api.cpp)         hot_in / hot_out: HOT = 2 with k + base = 1023 rows of 4 MiB
                                  (row offsets in soffset from 2^31 on), HOT = 1 one row later
  panels_in_31_bits               bs32_narrow / bs32_wide: O32 = true at ld = 2^24 - 4 (panel
                                  offsets just under 2^31), O32 = false at 2^25 with rows past
                                  2^31 elements; drop-in, analysed, SUB (bs 64), panel, grouped
  small_grouped_ok                small_in / small_out(bs): the grouped bs 2 / 4 / 8 stream at
                                  the last ld inside ld bs 4 < 2^31 and the lane-group kernel
                                  at the first outside
and, with no switch of their own, every other entry's 64-bit row arithmetic: the CSR product
(fp32 at every VEC and the lane-group kernel, fp16, fp64, column-major staging transposes),
the bs 16 kernels (fp32 column-masked and register-fragment, fp16 stream, analysed, grouped),
the generic BSR kernel, the fp64 BSR product, the SDDMM and the multi-head SDDMM / product on
float32, float16 and bfloat16 features, each with a far input and a far output.

Every case asserts from the handle's launch record (or small_bsr_path) that the kernel and
the side of the switch it was written for ran; the side comes from far_cases.side(), which
tests/test_far_cases.py ties to the launchers. Results are compared as tests/kernel_cases.py
compares them, on the compact operands (a leading dimension does not enter the arithmetic):
the fp64 oracle with assert_normwise at TOL_F32 / TOL_F16_ACC, oracle_csrmm_d / oracle_bsrmm_d
at 1e-12, and bit for bit where the project claims it (the piece oracle for the merge-path CSR
kernels, the sequential fp32 oracle for bs 2 / 4 / 8 and the bs 32 / 64 streams at row-major C,
prep.sddmm, the host forms of the heads entries, csrmm_f16 = the piece oracle on the widened
inputs). A far output is pre-filled with a random C0 and beta != 0; 64 sentinel NaNs before
and after the n columns of every used row are checked unchanged.

A far row-major C of more than 13 rows cannot sit at ld 2^28 inside the arena: such outputs
take the largest ld whose rows fit (far_cases.c_geometry: 2^26 up to 49 rows, 2^25 up to 97).
The 48 rows of the bs 16 outputs and the 96 of the bs 32 and bs 2 / 4 / 8 ones still cross 2^31
and 2^32 bytes and 2^31 elements. bs 64 has whole 64-row blocks only: its far B covers 128 rows
of bs32_narrow and 64 of bs32_wide, and its far C is one block of 64 rows at ld 2^25, which
crosses the two byte bounds but not 2^31 elements (two blocks at a power-of-two ld that does
would be 16 GiB). tests/test_far_cases.py checks these crossings per row count.

Not here: the edge softmax and the converters take no leading dimension (nnz bounds them);
the handle-less gespmm entries have ld = n; the hybrid entries' smallest matrix has more rows
than this arena holds at these leading dimensions; the host forms would need the same bytes
of host memory; the multi-GPU entry splits rows, not offsets.

The only skip is the whole module when the arena cannot be allocated.
"""
from __future__ import annotations

import re
import time

import numpy as np
import pytest

import far_cases as fc
import heads_half_cases as hh
from helpers import (TOL_F16_ACC, TOL_F32, assert_normwise, framed, oracle_bsrmm_d,
                     oracle_bsrmm_f32, oracle_bsrmm_f64, oracle_csrmm_d, oracle_csrmm_f64,
                     oracle_csrmm_pieces_f32)
from kernel_cases import ALPHA, BETA

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def arena(device):
    t0 = time.perf_counter()
    try:
        a = fc.Arena()
    except torch.cuda.OutOfMemoryError:
        pytest.skip(f"no {fc.ARENA_BYTES} bytes of device memory for the arena")
    torch.cuda.synchronize()
    print(f"\nfar arena: {fc.ARENA_BYTES} bytes allocated in {time.perf_counter() - t0:.3f} s")
    yield a
    a.close()


@pytest.fixture
def handle(device):
    from spmm_hip import ops
    h = ops.Handle()
    h.set_csr_options(1)
    yield h
    h.close()


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(x)).to("cuda") for x in arrs]


c_geometry = fc.c_geometry


def operands(arena, Bd, C0, far, ob=0, oc=0, gB=None, gC=None, off=0):
    """Bd (rows_b x n) and C0 (rows_c x n) in the given storage orders, the one named by `far`
    ("B" / "C") on its geometry in the arena, the other framed at its own width. Returns
    (dB, ldb, check_B, dC, ldc, extract); a column-major operand's far rows are its columns.
    off: elements B starts off its 16-byte base, far or not."""
    B2 = Bd if ob == 0 else np.ascontiguousarray(Bd.T)
    C2 = C0 if oc == 0 else np.ascontiguousarray(C0.T)
    if far == "B":
        fb = arena.place(B2, gB.ld, off=off)
        dB, ldb, chkB = fb.view, gB.ld, fb.unchanged
    else:
        dB, chk = framed(B2, B2.shape[1], off)
        ldb, chkB = B2.shape[1], chk.unchanged
    if far == "C":
        getC = arena.place(C2, gC.ld)
        dC, ldc = getC.view, gC.ld
    else:
        dC, getC = framed(C2, C2.shape[1], 0)
        ldc = C2.shape[1]

    def extract(what):
        got = getC(what + ": C")
        return got if oc == 0 else np.ascontiguousarray(got.T)
    return dB, ldb, chkB, dC, ldc, extract


def need(rec, pattern, what):
    assert any(re.search(pattern, k) for k in rec), f"{what}: no {pattern} among {sorted(set(rec))}"


def never(rec, pattern, what):
    hit = [k for k in rec if re.search(pattern, k)]
    assert not hit, f"{what}: {hit} ran"


def same_bits(got, want, what):
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ in bits"


def check_product(got, ref, absd, C0, tol, what):
    ref = ALPHA * ref + BETA * C0.astype(np.float64)
    absd = abs(ALPHA) * absd + abs(BETA) * np.abs(C0.astype(np.float64))
    assert_normwise(got, ref, absd, tol, what)


# ------------------------------------------------------------------------------ 1. CSR fp32
CSR_KERNEL = {8: "csr_group_kernel", 65: r"csr_mergepath_kernelILi1ELb[01]ELi0E",
              66: r"csr_mergepath_kernelILi2ELb[01]ELi0E",
              132: r"csr_mergepath_kernelILi4ELb[01]ELi0E",
              136: r"csr_mergepath_kernelILi4ELb[01]ELi0E"}
CSR_F32 = ([("B", 0, n, base) for n in (8, 65, 66, 132) for base in (0, 1)] +
           [("C", 0, n, 0) for n in (8, 65, 66, 132)] +
           [(far, 1, n, 0) for far in "BC" for n in (9, 12)])


def _csr_shape(far, order, n):
    """(m, k): the far operand has 9 rows (row-major) or n = 9 / 12 columns (column-major)."""
    if order == 1:
        return 70, 40
    return (70, 9) if far == "B" else (9, 20)


def csr_for(rng, m, k):
    """far_csr for _csr_shape's (m, k): with m = 9 the rows are a far C's, and the last one
    (the only one at 2^31 elements) holds entries."""
    return fc.far_csr(rng, m, k, long_row=7 if m > 9 else 4, last_empty=m > 9)


def check_csr(oracle, rec, got, m, n, rp, ci, v32, B32, C0, what):
    """The merge-path kernel to the piece oracle's bits, the lane-group kernel to fp64."""
    if any("csr_mergepath_kernel" in k for k in rec):
        want = oracle_csrmm_pieces_f32(oracle, m, n, rp, ci, v32, B32, n, 0, ALPHA, BETA,
                                       C0.reshape(-1), n, 0).reshape(m, n)
        same_bits(got, want, what)
    else:
        need(rec, "csr_group_kernel", what)
        ref, absd = oracle_csrmm_f64(oracle, m, n, rp, ci, v32, B32, n, 0)
        check_product(got, ref, absd, C0, TOL_F32, what)


@pytest.mark.parametrize(
    "far,order,n,base", CSR_F32,
    ids=[f"far{f}-{'cm' if o else 'rm'}-n{n}-base{b}" for f, o, n, b in CSR_F32])
def test_csr_f32(arena, oracle, handle, far, order, n, base):
    from spmm_hip import ops
    what = f"csrmm far {far} order {order} n {n} base {base}"
    m, k = _csr_shape(far, order, n)
    rng = np.random.default_rng(100 + n + 7 * base)
    rp, ci, v = csr_for(rng, m, k)
    Bd = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    C0 = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    ob, oc = (order if far == "B" else 0), (order if far == "C" else 0)
    dB, ldb, chkB, dC, ldc, extract = operands(arena, Bd, C0, far, ob, oc, fc.F32, fc.F32)
    drp, dci, dv = _dev(rp + base, ci + base, v)
    with handle.launch_record() as rec:
        ops.csrmm(drp, dci, dv, dB, m=m, n=n, k=k, ldb=ldb, order_b=ob, C=dC, ldc=ldc,
                  order_c=oc, alpha=ALPHA, beta=BETA, base=base, handle=handle)
    torch.cuda.synchronize()
    if order == 0:
        need(rec, CSR_KERNEL[n], what)
    else:
        need(rec, "transpose", what)
    got = extract(what)
    chkB(what + ": B")
    check_csr(oracle, rec, got, m, n, rp, ci, v, Bd, C0, what)


# ------------------------------------------------------------------------------ 2. CSR fp16
CSR_F16 = [("B", n, 0) for n in (8, 65, 66, 136)] + [("B", 136, 1), ("C", 136, 0)]
CSR_F16_VEC = {8: 1, 65: 1, 66: 2, 136: 4}


@pytest.mark.parametrize("far,n,odd", CSR_F16, ids=[f"far{f}-n{n}-odd{o}" for f, n, o in CSR_F16])
def test_csr_f16(arena, oracle, handle, far, n, odd):
    """B on h16 (once an odd half into the arena: the one-half-per-lane gather), C on f32:
    the bits of the piece oracle on the widened inputs, which are csrmm's."""
    from spmm_hip import ops
    what = f"csrmm_f16 far {far} n {n} odd {odd}"
    m, k = _csr_shape(far, 0, n)
    rng = np.random.default_rng(200 + n + odd)
    rp, ci, v = csr_for(rng, m, k)
    v = v.astype(np.float16)
    Bd = rng.uniform(-1, 1, (k, n)).astype(np.float16)
    C0 = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    dB, ldb, chkB, dC, ldc, extract = operands(arena, Bd, C0, far, 0, 0, fc.H16, fc.F32, off=odd)
    assert dB.data_ptr() % 4 == (2 if odd else 0)
    drp, dci, dv = _dev(rp, ci, v)
    with handle.launch_record() as rec:
        ops.csrmm_f16(drp, dci, dv, dB, m=m, n=n, k=k, ldb=ldb, C=dC, ldc=ldc, alpha=ALPHA,
                      beta=BETA, handle=handle)
    torch.cuda.synchronize()
    vec = 1 if odd else CSR_F16_VEC[n]
    need(rec, rf"CsrMpIDF16_E20csr_mergepath_kernelILi{vec}E", what)
    got = extract(what)
    chkB(what + ": B")
    want = oracle_csrmm_pieces_f32(oracle, m, n, rp, ci, v.astype(np.float32),
                                   Bd.astype(np.float32), n, 0, ALPHA, BETA, C0.reshape(-1), n,
                                   0).reshape(m, n)
    same_bits(got, want, what)


# --------------------------------------------------------------------------------- 3. fp64
F64 = [("csr", far, 1) for far in "BC"] + [("bsr", far, rowd) for far in "BC" for rowd in (1, 0)]


@pytest.mark.parametrize("kind,far,rowd", F64, ids=[f"{k}-far{f}-rowd{r}" for k, f, r in F64])
def test_f64(arena, oracle, handle, kind, far, rowd):
    from spmm_hip import ops
    what = f"f64 {kind} far {far} rowd {rowd}"
    n, bs = 70, 3
    rng = np.random.default_rng(64 + rowd)
    if kind == "csr":
        m, k = _csr_shape(far, 0, n)
        rp, ci, v = csr_for(rng, m, k)
        rows_b, rows_c = k, m
    else:
        mb, kb = (6, 3) if far == "B" else (3, 5)
        rp, ci, v = fc.far_bsr(rng, mb, kb, bs)
        rows_b, rows_c = kb * bs, mb * bs
    v = v.astype(np.float64)
    Bd = rng.standard_normal((rows_b, n))
    C0 = rng.standard_normal((rows_c, n))
    dB, ldb, chkB, dC, ldc, extract = operands(arena, Bd, C0, far, 0, 0, fc.F64, fc.F64)
    if kind == "csr":
        drp, dci, dv = _dev(rp, ci, v)
        with handle.launch_record() as rec:
            ops.csrmm(drp, dci, dv, dB, m=m, n=n, k=k, ldb=ldb, C=dC, ldc=ldc, alpha=ALPHA,
                      beta=BETA, handle=handle)
        need(rec, "csr_f64_kernel", what)
        want = oracle_csrmm_d(oracle, m, n, rp, ci, v, Bd, n, 0, ALPHA, BETA, C0.reshape(-1), n, 0)
        absd = np.abs(oracle_csrmm_d(oracle, m, n, rp, ci, np.abs(v), np.abs(Bd), n, 0,
                                     abs(ALPHA), abs(BETA), np.abs(C0).reshape(-1), n, 0))
    else:
        src = v if rowd else np.ascontiguousarray(
            v.reshape(-1, bs, bs).transpose(0, 2, 1)).reshape(-1)
        drp, dci, dv = _dev(rp, ci, src)
        with handle.launch_record() as rec:
            ops.bsrmm(drp, dci, dv, dB, mb=mb, kb=kb, n=n, bs=bs, ldb=ldb, C=dC, ldc=ldc,
                      alpha=ALPHA, beta=BETA, direction=1 - rowd, handle=handle)
        need(rec, "bsr_f64_kernel", what)
        want = oracle_bsrmm_d(oracle, 0, mb, n, bs, rp, ci, v, Bd, n, 0, ALPHA, BETA,
                              C0.reshape(-1), n, 0)
        absd = np.abs(oracle_bsrmm_d(oracle, 0, mb, n, bs, rp, ci, np.abs(v), np.abs(Bd), n, 0,
                                     abs(ALPHA), abs(BETA), np.abs(C0).reshape(-1), n, 0))
    torch.cuda.synchronize()
    got = extract(what)
    chkB(what + ": B")
    assert_normwise(got, want.reshape(rows_c, n), absd.reshape(rows_c, n), 1e-12, what)


# ------------------------------------------------------------------- 4. the hot-column entry
HOT = [(g, base, n) for g in (fc.HOT_IN, fc.HOT_OUT) for base in (0, 1) for n in fc.HOT_N]


@pytest.mark.parametrize("g,base,n", HOT, ids=[f"{g.name}-base{b}-n{n}" for g, b, n in HOT])
def test_csr_hot(arena, oracle, handle, g, base, n):
    """k + base = 1023 rows of 4 MiB take HOT = 2 (one resource for all of B, the row offset
    in soffset: from row 512 on its top bit is set), 1024 take HOT = 1. A hot budget of two
    rows tags k - 1 and 512 and leaves k - 2, so rows past 2^31 bytes are gathered both ways."""
    from spmm_hip import ops
    what = f"csrmm_hot {g.name} base {base} n {n}"
    k = fc.hot_k(g, base)
    used = np.array(fc.hot_rows(k))
    rng = np.random.default_rng(300 + n + base)
    rp, ci, v = fc.hot_csr(rng, k)
    m = rp.size - 1
    Bs = rng.uniform(-1, 1, (used.size, n)).astype(np.float32)
    C0 = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    fb = arena.place(Bs, g.ld, rows=used)
    dC, chkC = framed(C0, n, 0)
    dC2, chkC2 = framed(C0, n, 0)
    drp, dci, dv = _dev(rp + base, ci + base, v)
    kw = dict(m=m, n=n, k=k, ldb=g.ld, ldc=n, alpha=ALPHA, beta=BETA, base=base)
    with handle.launch_record() as rec:
        tag = ops.csr_hot_analysis(dci, n=n, k=k, base=base, hot_bytes=2 * 4 * n, handle=handle)
        ops.csrmm_hot(drp, tag, dv, fb.view, C=dC, handle=handle, **kw)
    torch.cuda.synchronize()
    hot = fc.side(g, n, base)["hot"]
    assert hot == (2 if g is fc.HOT_IN else 1)
    need(rec, rf"CsrMpIfE20csr_mergepath_kernelILi\d+ELb[01]ELi{hot}E", what)
    never(rec, rf"csr_mergepath_kernelILi\d+ELb[01]ELi{3 - hot}E", what)
    tagged = tag.cpu().numpy() < 0
    beyond = ci >= 512
    assert (tagged & beyond).any() and (~tagged & beyond).any(), \
        f"{what}: rows past 2^31 bytes tagged {int((tagged & beyond).sum())}, untagged " \
        f"{int((~tagged & beyond).sum())}"
    assert set(ci[tagged]) == {512, k - 1}, f"{what}: tagged rows {sorted(set(ci[tagged]))}"
    h2 = ops.Handle()
    h2.set_csr_options(1)
    with h2.launch_record() as rec2:
        ops.csrmm(drp, dci, dv, fb.view, C=dC2, handle=h2, **kw)
    torch.cuda.synchronize()
    h2.close()
    need(rec2, r"csr_mergepath_kernelILi\d+ELb[01]ELi0E", what + " (plain)")
    got, plain = chkC(what), chkC2(what + " (plain)")
    fb.unchanged(what + ": B")
    same_bits(got, plain, what + ": hot against the untagged indices")
    small = np.searchsorted(used, ci).astype(np.int32)
    want = oracle_csrmm_pieces_f32(oracle, m, n, rp, small, v, Bs, n, 0, ALPHA, BETA,
                                   C0.reshape(-1), n, 0).reshape(m, n)
    same_bits(got, want, what + ": the piece oracle")


# ---------------------------------------------------------------------------------- BSR runner
def run_bsr(arena, oracle, h, what, *, entry, bs, n, mat, far, gB=None, oc=0, rowd=1, f16=False,
            off=0, flags=0, W=2):
    """One BSR product with B (row-major, geometry gB) or C (c_geometry / f32 for a
    column-major C) far. entry: "bsrmm", "analysed" or "grouped". Returns (rec, got, bits),
    the result already held to the fp64 oracle; bits() holds it to the sequential fp32
    oracle."""
    from spmm_hip import ops
    mb, kb, rp, ci, v = mat
    vt = np.float16 if f16 else np.float32
    v = v.astype(vt)
    rng = np.random.default_rng(5 + bs + n)
    Bd = rng.uniform(-1, 1, (kb * bs, n)).astype(vt)
    C0 = rng.uniform(-1, 1, (mb * bs, n)).astype(np.float32)
    gC = None if far != "C" else fc.F32 if oc == 1 else c_geometry(mb * bs)
    dB, ldb, chkB, dC, ldc, extract = operands(arena, Bd, C0, far, 0, oc, gB, gC, off=off)
    src = v if rowd else np.ascontiguousarray(v.reshape(-1, bs, bs).transpose(0, 2, 1)).reshape(-1)
    drp, dci, dv = _dev(rp, ci, src)
    h.set_bsr_options(flags)
    kw = dict(n=n, ldb=ldb, C=dC, ldc=ldc, order_c=oc, alpha=ALPHA, beta=BETA)
    with h.launch_record() as rec:
        if entry == "analysed":
            ana = ops.bsr16_analysis if f16 else ops.bsr32_analysis
            masks, vcol = ana(dv, nnzb=ci.size, direction=1 - rowd, handle=h)
            (ops.bsrmm_analysed_f16 if f16 else ops.bsrmm_analysed)(
                drp, dci, vcol, masks, dB, mb=mb, kb=kb, handle=h, **kw)
        elif entry == "grouped":
            G = ops.GroupedBsr16 if f16 else ops.GroupedBsr32
            with G(drp, dci, dv, mb=mb, group_rows=W, direction=1 - rowd, handle=h) as g:
                g.mm(dB, kb=kb, **kw)
        else:
            (ops.bsrmm_f16 if f16 else ops.bsrmm)(drp, dci, dv, dB, mb=mb, kb=kb, bs=bs,
                                                  direction=1 - rowd, handle=h, **kw)
    torch.cuda.synchronize()
    got = extract(what)
    chkB(what + ": B")
    ref, absd = oracle_bsrmm_f64(oracle, 0, mb, n, bs, rp, ci, v, Bd, n, 0, half=f16)
    check_product(got, ref, absd, C0, TOL_F16_ACC if f16 else TOL_F32, what)

    def bits():
        want = oracle_bsrmm_f32(oracle, 1 - rowd, mb, n, bs, rp, ci, src, Bd, n, 0, ALPHA, BETA,
                                C0.reshape(-1), n, 0).reshape(mb * bs, n)
        whole = np.repeat(np.diff(rp) <= 64, bs)
        same_bits(got[whole], want[whole], what + ": the sequential fp32 oracle")
    return rec, got, bits


def far_mat(bs, kb, mb=6, seed=0):
    rp, ci, v = fc.far_bsr(np.random.default_rng(1000 + bs + seed), mb, kb, bs)
    return mb, kb, rp, ci, v


# ------------------------------------------------------------------------ 5. BSR bs 32 / 64
def cs2(crow, o32, msk=0, sub=0):
    """bsr32_f32_cs2_kernel<CROW, O32, ANT, MSK, SUB, C64>."""
    return rf"bsr32_f32_cs2_kernelILb{int(crow)}ELb{int(o32)}ELb1ELb{msk}ELb{sub}E"


def assert_o32(rec, g, crow, what, msk=0, sub=0):
    o32 = fc.side(g)["o32"]
    need(rec, cs2(crow, o32, msk, sub), what)
    never(rec, rf"bsr32_f32_cs2_kernelILb[01]ELb{int(not o32)}E", what)


BS32 = [(g, oc, n) for g in (fc.BS32_NARROW, fc.BS32_WIDE) for oc, n in ((0, 132), (1, 64))]
BS32_IDS = [f"{g.name}-oc{oc}-n{n}" for g, oc, n in BS32]


@pytest.mark.parametrize("g,oc,n", BS32, ids=BS32_IDS)
def test_bs32_drop_in(arena, oracle, handle, g, oc, n):
    what = f"bsrmm bs 32 {g.name} oc {oc} n {n}"
    rec, _, bits = run_bsr(arena, oracle, handle, what, entry="bsrmm", bs=32, n=n,
                           mat=far_mat(32, g.rows // 32), far="B", gB=g, oc=oc)
    assert_o32(rec, g, 1 - oc, what)
    if oc == 0:
        bits()


@pytest.mark.parametrize("g,oc,n", BS32, ids=BS32_IDS)
def test_bs32_analysed(arena, oracle, handle, g, oc, n):
    what = f"bsrmm_analysed {g.name} oc {oc} n {n}"
    rec, _, bits = run_bsr(arena, oracle, handle, what, entry="analysed", bs=32, n=n,
                           mat=far_mat(32, g.rows // 32, seed=1), far="B", gB=g, oc=oc)
    need(rec, "bsr32_analysis_kernel", what)
    assert_o32(rec, g, 1 - oc, what, msk=1)
    if oc == 0:
        bits()


@pytest.mark.parametrize("g,oc,n", BS32, ids=BS32_IDS)
def test_bs32_grouped(arena, oracle, handle, g, oc, n):
    """The grouped stream has one form for every ld (64-bit row addresses): the record must
    hold it, on both geometries."""
    what = f"GroupedBsr32 {g.name} oc {oc} n {n}"
    rec, _, bits = run_bsr(arena, oracle, handle, what, entry="grouped", bs=32, n=n,
                           mat=far_mat(32, g.rows // 32, seed=2), far="B", gB=g, oc=oc)
    need(rec, "bsr32_f32_grp_kernelILi2E", what)
    if oc == 0:
        bits()


@pytest.mark.parametrize("g,oc,n", BS32, ids=BS32_IDS)
def test_bs64_sub_stream(arena, oracle, handle, g, oc, n):
    """Whole 64-row blocks inside the arena: 128 rows of bs32_narrow (past 2^31 and 2^32
    bytes), 64 of bs32_wide."""
    what = f"bsrmm bs 64 {g.name} oc {oc} n {n}"
    kb = 2 if g is fc.BS32_NARROW else 1
    assert g.start(kb * 64 - 1) >= fc.P32
    rec, _, bits = run_bsr(arena, oracle, handle, what, entry="bsrmm", bs=64, n=n,
                           mat=far_mat(64, kb, mb=4), far="B", gB=g, oc=oc)
    assert_o32(rec, g, 1 - oc, what, sub=1)
    if oc == 0:
        bits()


def panel_mat():
    """24,600 block rows (a deep grid: a row-major C takes the panel stream only there) of
    one or two fully dense blocks over the 5 block columns of bs32_narrow, 2^15 in all."""
    mb, kb = 24600, 5
    lens = np.ones(mb, np.int64)
    lens[:(1 << 15) - mb] = 2
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate([np.sort([i % kb, (i + 2) % kb])[:l] if l == 2 else [(i * 3) % kb]
                         for i, l in enumerate(lens)]).astype(np.int32)
    v = np.random.default_rng(7).random(ci.size * 1024, dtype=np.float32) * 2.0 - 1.0
    assert np.bincount(ci, minlength=kb).min() > 1000
    return mb, kb, rp, ci, v


@pytest.mark.parametrize("oc", [0, 1])
def test_bs32_panel(arena, oracle, handle, oc):
    """Dense blocks from 2^15 on: the probe picks the panel kernel, which only the narrow side
    launches (the column stream of the same call returns at once). The choice is made on the
    device and both kernels are always queued, so the record shows that the panel kernel went
    out, not that it did the work: panel_mat's blocks, uniform and without a zero, are over
    the probe's bound by construction, and the bits are the same either way."""
    g = fc.BS32_NARROW
    what = f"bsrmm bs 32 panel {g.name} oc {oc}"
    rec, _, bits = run_bsr(arena, oracle, handle, what, entry="bsrmm", bs=32, n=8, mat=panel_mat(),
                           far="B", gB=g, oc=oc)
    assert fc.side(g)["o32"]
    need(rec, "panel_probe_kernel", what)
    need(rec, rf"bsr32_f32_panel_kernelILb{1 - oc}E", what)
    assert_o32(rec, g, 1 - oc, what)
    if oc == 0:
        bits()


def test_bs32_panel_far_c(arena, oracle, handle):
    """The panel kernel's own C stores: panel_mat with a column-major C of n = 12 columns at
    ld 2^28 >= 787,200 rows (column 2 at 2^31 bytes, 4 at 2^32, 8 at 2^31 elements). B is
    ordinary at ld 12, the narrow side; with a column-major C no segment path competes with
    the probe. As in test_bs32_panel the record shows the panel kernel queued."""
    what = "bsrmm bs 32 panel, far column-major C"
    rec, _, _ = run_bsr(arena, oracle, handle, what, entry="bsrmm", bs=32, n=12, mat=panel_mat(),
                        far="C", oc=1)
    assert fc.panels_in_31_bits(12) and fc.F32.ld >= 24600 * 32
    need(rec, "panel_probe_kernel", what)
    need(rec, "bsr32_f32_panel_kernelILb0E", what)
    need(rec, cs2(0, True), what)


BS32_FAR_C = ["bsrmm", "analysed", "grouped", "bs64", "cm"]


@pytest.mark.parametrize("entry", BS32_FAR_C)
def test_bs32_far_c(arena, oracle, handle, entry):
    """One far C per entry: 96 rows at ld 2^25 (row 16 at 2^31 bytes, 32 at 2^32, 64 at 2^31
    elements; bs 64: one block, the first 64, so the byte bounds only), and the drop-in once
    with a column-major C of n = 12 columns at ld 2^28. B is ordinary, so the narrow side runs."""
    what = f"far C {entry}"
    bs = 64 if entry == "bs64" else 32
    oc = int(entry == "cm")
    mb = 1 if bs == 64 else 3
    n = 12 if oc else 132
    mat = far_mat(bs, 4, mb=mb, seed=3)
    rec, _, bits = run_bsr(arena, oracle, handle, what, bs=bs, n=n, mat=mat, far="C", oc=oc,
                           entry=entry if entry in ("analysed", "grouped") else "bsrmm")
    assert c_geometry(mb * bs) is fc.BS32_WIDE
    assert oc or fc.c_crossed(mb * bs) == (True, True, bs == 32)
    if entry == "grouped":
        need(rec, "bsr32_f32_grp_kernel", what)
    else:
        assert fc.panels_in_31_bits(n)
        need(rec, cs2(1 - oc, True, int(entry == "analysed"), int(bs == 64)), what)
    if oc == 0:
        bits()


# ----------------------------------------------------------------------------- 6. BSR bs 16
def test_bs16_f32_column_masked(arena, oracle, handle):
    what = "bsrmm bs 16 fp32 column-masked, far B"
    g = fc.BS16_F
    rec, _, _ = run_bsr(arena, oracle, handle, what, entry="bsrmm", bs=16, n=64,
                        mat=far_mat(16, g.rows // 16), far="B", gB=g)
    need(rec, "bsr16_cm_kernelIfLb1E", what)


def test_bs16_f32_fragments(arena, oracle, handle):
    """B one float off 16 bytes: the copy kernels refuse it, the register-fragment kernel
    reads B by scalar loads at (row * ldb + column)."""
    what = "bsrmm bs 16 fp32 register fragments, far B"
    g = fc.BS16_F
    rec, _, _ = run_bsr(arena, oracle, handle, what, entry="bsrmm", bs=16, n=64,
                        mat=far_mat(16, g.rows // 16), far="B", gB=g, off=1)
    need(rec, "bsr16_f32_mfma_kernelILb1ELb1ELb1E", what)


BS16_F16 = [("bsrmm", 136, "bsr16_f16_cs_kernelILb1ELb1ELb0E"),
            ("bsrmm", 64, "bsr16_cm_kernelIDF16_Lb1E"),
            ("analysed", 136, "bsr16_f16_cs_kernelILb1ELb1ELb1E"),
            ("grouped", 136, "bsr16_f16_grp_kernelILi2E")]


@pytest.mark.parametrize("entry,n,kernel", BS16_F16, ids=[f"{e}-n{n}" for e, n, _ in BS16_F16])
def test_bs16_f16(arena, oracle, handle, entry, n, kernel):
    what = f"bs 16 fp16 {entry} n {n}, far B"
    g = fc.BS16_H
    rec, _, _ = run_bsr(arena, oracle, handle, what, entry=entry, bs=16, n=n,
                        mat=far_mat(16, g.rows // 16, seed=n), far="B", gB=g, f16=True)
    need(rec, kernel, what)


BS16_FAR_C = [("bsrmm", False, 64, "bsr16_cm_kernelIfLb1E"),
              ("fragments", False, 64, "bsr16_f32_mfma_kernelILb1ELb1ELb1E"),
              ("bsrmm", True, 136, "bsr16_f16_cs_kernelILb1ELb1ELb0E"),
              ("analysed", True, 136, "bsr16_f16_cs_kernelILb1ELb1ELb1E"),
              ("grouped", True, 136, "bsr16_f16_grp_kernelILi2E")]


@pytest.mark.parametrize("entry,f16,n,kernel", BS16_FAR_C,
                         ids=[f"{e}-{'f16' if h else 'f32'}" for e, h, _, _ in BS16_FAR_C])
def test_bs16_far_c(arena, oracle, handle, entry, f16, n, kernel):
    """48 rows of C at ld 2^26: row 8 at 2^31 bytes, 16 at 2^32, 32 at 2^31 elements. The
    register-fragment kernel (scalar C stores) is selected by an ordinary B one float off 16
    bytes, which the copy kernels refuse."""
    what = f"bs 16 {entry} f16 {f16}, far C"
    frag = entry == "fragments"
    rec, _, _ = run_bsr(arena, oracle, handle, what, entry="bsrmm" if frag else entry, bs=16,
                        n=n, mat=far_mat(16, 4, mb=3, seed=9), far="C", f16=f16, off=int(frag))
    assert c_geometry(48) is fc.BS16_F and fc.c_crossed(48) == (True, True, True)
    need(rec, kernel, what)


# ------------------------------------------------------------------------- 7. BSR bs 2 / 4 / 8
SMALL_GROUPED = 2  # SPMM_BSR_SMALL_GROUPED


def small_mat(bs):
    """Three groups of G = 32 / bs block rows (96 rows of C: at ld 2^25 the last group lies
    past 2^31 elements), every block row holding every block column but block row 1 (empty)
    and 3 (the last column only). The probe's estimate is the mean of 1 / holders over
    sampled blocks: 1 / G in the later groups and at most 1 / (G - 2) in the first, that is
    below 0.1 (bs 2), 0.17 (bs 4) and 0.5 (bs 8) against give-up bounds of 0.25, 0.45 and 0.70.
    So the grouped stream keeps the matrix: small_bsr_path 1, not 2."""
    kb, G = fc.small_kb(bs), 32 // bs
    mb = 3 * G
    rows = [np.arange(kb, dtype=np.int32) for _ in range(mb)]
    rows[1] = np.zeros(0, np.int32)
    rows[3] = np.array([kb - 1], np.int32)
    rp = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows)
    v = np.random.default_rng(20 + bs).uniform(-1, 1, ci.size * bs * bs).astype(np.float32)
    return mb, kb, rp, ci, v


SMALL = [(bs, where, flags, n) for bs in fc.SMALL_BS
         for where, flags, n in (("in", SMALL_GROUPED, 132), ("out", SMALL_GROUPED, 132),
                                 ("in", 0, 132), ("in", 0, 64), ("C", SMALL_GROUPED, 132),
                                 ("C", 0, 132))]


@pytest.mark.parametrize("bs,where,flags,n", SMALL,
                         ids=[f"bs{b}-{w}-flags{f}-n{n}" for b, w, f, n in SMALL])
def test_bs_small(arena, oracle, handle, bs, where, flags, n):
    """Under SPMM_BSR_SMALL_GROUPED the last ld inside ld bs 4 < 2^31 runs the grouped stream
    (path 1: small_mat's probe keeps it) and the first outside the lane-group kernel (path 0);
    without the flag the lane-group kernel runs on small_in, 1 and 2 floats per lane. A far C
    (96 rows at ld 2^25: past 2^31 and 2^32 bytes and 2^31 elements) runs the grouped stream
    and, without the flag, the lane-group kernel on an ordinary B. All bit for bit."""
    what = f"bsrmm bs {bs} small_{where} flags {flags} n {n}"
    g = None if where == "C" else (fc.small_in if where == "in" else fc.small_out)(bs)
    rec, _, bits = run_bsr(arena, oracle, handle, what, entry="bsrmm", bs=bs, n=n,
                           mat=small_mat(bs), far="C" if where == "C" else "B", gB=g, flags=flags)
    grouped = bool(flags) and (g is None or fc.side(g)["small"] == 1)
    assert g is not None or fc.c_crossed(small_mat(bs)[0] * bs) == (True, True, True)
    path = handle.small_bsr_path()
    assert path == (1 if grouped else 0), f"{what}: small_bsr_path {path}"
    if grouped:
        need(rec, rf"bsr_small_grp_kernelILi{bs}E", what)
    else:
        never(rec, "bsr_small_grp_kernel", what)
        need(rec, rf"bsr_small_kernelILi{bs}ELi{2 if n > 64 else 1}E", what)
    bits()


# ------------------------------------------------------------------- 8. the generic BSR kernel
GENERIC = [(bs, rowd, far) for bs in (3, 5) for rowd in (1, 0) for far in "BC"]


@pytest.mark.parametrize("bs,rowd,far", GENERIC,
                         ids=[f"bs{b}-rowd{r}-far{f}" for b, r, f in GENERIC])
def test_bsr_generic(arena, oracle, handle, bs, rowd, far):
    """9 (bs 3) or 10 (bs 5) rows of B or C at ld 2^28."""
    what = f"bsrmm bs {bs} rowd {rowd} far {far}"
    mb, kb = (6, 9 // bs + (bs == 5)) if far == "B" else (9 // bs + (bs == 5), 4)
    rec, _, _ = run_bsr(arena, oracle, handle, what, entry="bsrmm", bs=bs, n=70,
                        mat=far_mat(bs, kb, mb=mb, seed=rowd), far=far, gB=fc.F32, rowd=rowd)
    assert c_geometry(mb * bs) is fc.F32 or far == "B"
    need(rec, "bsr_generic_kernelIfE", what)


# ------------------------------------------------------------------------------- 9. SDDMM
SDDMM_WIDE_N = 1025  # the least n of sddmm_wide_kernel: more than 4 chunks of 4 per lane of 64
SDDMM = [(far, n, 0) for far in "XY" for n in (8, 200, SDDMM_WIDE_N)] + [("Y", 200, 1)]


def sddmm_pattern(rng, far):
    """About 300 positions: far X has m = 9 rows (37 of 40 columns each), far Y k = 9 rows
    (60 rows of 5 columns); the first row empty."""
    m, k, deg = (9, 40, 37) if far == "X" else (60, 9, 5)
    rows = [np.sort(rng.choice(k, deg, replace=False)) for _ in range(m)]
    rows[0] = np.zeros(0, np.int64)
    rp = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    assert 280 <= ci.size <= 320 and (far == "X" or np.bincount(ci, minlength=9).min() >= 3)
    return m, k, rp, ci


@pytest.mark.parametrize("far,n,base", SDDMM, ids=[f"far{f}-n{n}-base{b}" for f, n, b in SDDMM])
def test_sddmm(arena, handle, far, n, base):
    from spmm_hip import ops, prep
    what = f"sddmm far {far} n {n} base {base}"
    rng = np.random.default_rng(90 + n + base)
    m, k, rp, ci = sddmm_pattern(rng, far)
    X = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    Y = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    out0 = rng.uniform(-1, 1, ci.size).astype(np.float32)
    g = fc.F32
    if far == "X":
        fx = arena.place(X, g.ld)
        dX, ldx, chkX = fx.view, g.ld, fx.unchanged
        dY, cy = framed(Y, n, 0)
        ldy, chkY = n, cy.unchanged
    else:
        dX, cx = framed(X, n, 0)
        ldx, chkX = n, cx.unchanged
        fy = arena.place(Y, g.ld)
        dY, ldy, chkY = fy.view, g.ld, fy.unchanged
    dout, chko = framed(out0.reshape(1, -1), ci.size, 0)
    drp, dci = _dev(rp + base, ci + base)
    with handle.launch_record() as rec:
        ops.sddmm(drp, dci, dX, dY, m=m, n=n, k=k, ldx=ldx, ldy=ldy, out=dout, alpha=ALPHA,
                  beta=BETA, base=base, handle=handle)
    torch.cuda.synchronize()
    need(rec, "sddmm_wide_kernelILb0E" if n == SDDMM_WIDE_N else
         rf"12sddmm_kernelILi{2 if n == 8 else 64}ELi1ELb1E", what)
    got = chko(what).reshape(-1)
    chkX(what + ": X")
    chkY(what + ": Y")
    want = prep.sddmm(m, n, k, rp, ci, X, Y, out=out0.copy(), alpha=ALPHA, beta=BETA)
    same_bits(got, want, what)


# -------------------------------------------------------------------------- 10. multi-head
HEADS = 3
TYPES = ["f32", "f16", "bf16"]
TORCH_TYPE = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def features(rng, shape, ty):
    """(what the arena / framed take, the torch dtype, what prep takes, prep's keywords): fp32
    arrays, or uint16 patterns of the half types with their widened fp32 values."""
    a = rng.uniform(-1, 1, shape).astype(np.float32)
    if ty == "f32":
        return a, None, a, {}
    bits = hh.to_bits(a, ty)
    stored, kw = hh.stored(bits, ty)
    return bits, TORCH_TYPE[ty], stored, kw


def half_buffer(bits, ty):
    """An ordinary (near) device tensor of the half type from its uint16 patterns."""
    return torch.from_numpy(bits.view(np.int16)).to("cuda").view(TORCH_TYPE[ty]).reshape(-1)


HEADS_SDDMM = [(ty, far, d) for ty in TYPES for far in "XY" for d in (4, 5)]


@pytest.mark.parametrize("ty,far,d", HEADS_SDDMM,
                         ids=[f"{t}-far{f}-d{d}" for t, f, d in HEADS_SDDMM])
def test_sddmm_heads(arena, handle, ty, far, d):
    """X or Y at ld 2^28 >= heads d (f32 / h16 geometry by the type), d = 4 on vector loads and
    d = 5 on scalar ones: the bits of the host form on the widened features."""
    from spmm_hip import ops, prep
    what = f"sddmm_heads {ty} far {far} d {d}"
    rng = np.random.default_rng(400 + d)
    m, k, rp, ci = sddmm_pattern(rng, far)
    w = HEADS * d
    xb, tdt, xs, kw = features(rng, (m, w), ty)
    yb, _, ys, _ = features(rng, (k, w), ty)
    old = rng.uniform(-1, 1, (ci.size, HEADS)).astype(np.float32)
    g = fc.F32 if ty == "f32" else fc.H16
    near = (lambda a: _dev(a)[0].reshape(-1)) if ty == "f32" else (lambda a: half_buffer(a, ty))
    if far == "X":
        fo = arena.place(xb, g.ld, dtype=tdt)
        dX, ldx, dY, ldy = fo.view, g.ld, near(yb), w
    else:
        fo = arena.place(yb, g.ld, dtype=tdt)
        dX, ldx, dY, ldy = near(xb), w, fo.view, g.ld
    dout, chko = framed(old.reshape(1, -1), old.size, 0)
    drp, dci = _dev(rp, ci)
    with handle.launch_record() as rec:
        ops.sddmm_heads(drp, dci, dX, dY, m=m, d=d, heads=HEADS, k=k, ldx=ldx, ldy=ldy, out=dout,
                        alpha=ALPHA, beta=BETA, handle=handle)
    torch.cuda.synchronize()
    need(rec, rf"sddmm_heads_kernelI\w+Li\d+ELb{int(d % 4 == 0)}E", what)
    got = chko(what).reshape(-1, HEADS)
    fo.unchanged(what + ": the far operand")
    want = prep.sddmm_heads(m, d, k, HEADS, rp, ci, xs, ys, out=old.copy(), alpha=ALPHA, beta=BETA,
                            **kw)
    same_bits(got, want, what)


HEADS_CSRMM = [(ty, far, d) for ty in TYPES for far in "BC" for d in (8, 5)]


@pytest.mark.parametrize("ty,far,d", HEADS_CSRMM,
                         ids=[f"{t}-far{f}-d{d}" for t, f, d in HEADS_CSRMM])
def test_csrmm_heads(arena, handle, ty, far, d):
    """B (f32 / h16 geometry by the type) or the fp32 C (f32 geometry) at ld 2^28: the bits of
    the host form on the widened B."""
    from spmm_hip import ops, prep
    what = f"csrmm_heads {ty} far {far} d {d}"
    rng = np.random.default_rng(500 + d)
    m, k = _csr_shape(far, 0, 0)
    rp, ci, _ = csr_for(rng, m, k)
    w = HEADS * d
    val = rng.uniform(-1, 1, (ci.size, HEADS)).astype(np.float32)
    bb, tdt, bs_, kw = features(rng, (k, w), ty)
    C0 = rng.uniform(-1, 1, (m, w)).astype(np.float32)
    if far == "B":
        ldb = (fc.F32 if ty == "f32" else fc.H16).ld
        fo = arena.place(bb, ldb, dtype=tdt)
        dB = fo.view
        dC, getC = framed(C0, w, 0)
        ldc = w
    else:
        dB = _dev(bb)[0].reshape(-1) if ty == "f32" else half_buffer(bb, ty)
        ldb = w
        getC = arena.place(C0, fc.F32.ld)
        dC, ldc = getC.view, fc.F32.ld
    drp, dci, dval = _dev(rp, ci, val)
    with handle.launch_record() as rec:
        ops.csrmm_heads(drp, dci, dval, dB, m=m, d=d, heads=HEADS, k=k, ldb=ldb, C=dC, ldc=ldc,
                        alpha=ALPHA, beta=BETA, handle=handle)
    torch.cuda.synchronize()
    need(rec, "csrmm_heads_kernel", what)
    got = getC(what + ": C")
    if far == "B":
        fo.unchanged(what + ": B")
    want = prep.csrmm_heads(m, d, k, HEADS, rp, ci, val, bs_, C=C0.copy(), alpha=ALPHA, beta=BETA,
                            **kw)
    same_bits(got, np.asarray(want).reshape(m, w), what)
