"""CSR positions past 2^31 and 2^32 bytes and up to INT_MAX at every CSR entry.

Every case puts the position-indexed arrays of one call (csrColInd, csrVal, csrColIndHot,
outVal, x, y, g, gx) on a window of tests/far_pos_cases.py: flat views into uninitialised
arenas of 8 GiB + 64 MiB in which the matrix sits at position 2^29 (2^31 bytes of a 4-byte
array), 2^30 (2^32 bytes; 2^31 bytes of an fp16 val) or ends at rowptr[m] - base = INT_MAX
exactly (TOP: a short last row; TOPL: the long row last), and for the [nnz, heads] arrays of
the multi-head entries at the same bounds of q = p * heads with TOP = INT_MAX // heads. The
row pointer is start + local (a view, csrRowPtr[0] > base); the view handed to a wrapper ends
at the window's end, so its numel(), the call's nnz, is rowptr[m] - base. Dense operands are
small and near (K = 64 rows of B / Y), except the one far B that makes the hot-column entry
take a buffer resource per row. At most three arenas are alive (module-scoped, freed at the
end); the only skip is the whole module when they cannot be allocated.

Each case asserts:
  bits     the far result equals, bit for bit (integer views, signed zeros included), the
           result of the same entry with the same handle on the near twin: the same window and
           guards at position 1024 + start mod 1024 of a small array, so the residues the
           kernels align their groups to are unchanged;
  oracle   the twin's result is held once to the oracle the entry's own tests use: the piece
           oracle (merge-path fp32 / fp16 products, the heads products), the restated rules of
           sddmm_cases / softmax_cases (prep's host forms, which tests/test_sddmm_host.py and
           tests/test_heads_host.py tie to those rules, on the 150,000-position windows where
           the numpy restatement would take seconds), heads_half_cases' exact widening, the
           host csr2csc restated in numpy, the sequential fp64 oracle (oracle_csrmm_d, the
           fp64 kernel's own chain) on int64 views, and, for the one kernel whose own tests
           have no bit oracle, the bar those tests use: the lane-group kernel (n = 64)
           against the fp64 oracle at TOL_F32. That bar applies to the twin alone; far
           against twin is always bits;
  guards   1024 positions in front of every window and behind it keep their bits (outputs:
           the signalling-NaN sentinel), and every input window is unchanged after the call;
  kernel   the launch record names the kernel the case was written for.

Windows per entry (far_pos_cases.windows): p4 for the single-valued fp32 / fp16 entries, p8
for fp64, q3 / q8 for the multi-head entries. A case on the first W bound of a family runs
at base 1, the others (and every TOP: rowptr[m] = INT_MAX already) at base 0. The "large"
windows run with set_csr_waves_per_cu(1): a merge-path wave then walks several 256-position
chunks, and the in-place chunk reload and split-row pieces run across the bound.

What cannot be expressed:
  * the handle-less drop-ins (spmm_gespmm_csrmm_f32 / _f16 / _f64) have no base argument: they
    run every window at base 0, and leave no launch record;
  * fp64 has no TOP: 2^31 doubles are 16 GiB; its bounds are 2^28, 2^29 and 2^30 positions;
  * the edge softmax launchers choose the lanes per short row from nnz / m: with nnz >= 2^26
    and a few hundred rows only G = 64 can be selected, so edge_softmax_kernel<4, .> and
    <16, .> (and the heads forms) cannot run in a far case. Short rows (one wave's lane
    groups) and long rows (above 1024 positions, by the workgroup) are two phases of the one
    kernel: the small windows run the first alone, the large ones (hub row of 40,000) both.
"""
from __future__ import annotations

import functools
import re
import time
import zlib

import numpy as np
import pytest

import csr2csc_cases as cc
import far_pos_cases as fp
import heads_cases as hc
import heads_half_cases as hh
import sddmm_cases as sd
from helpers import (TOL_F32, assert_normwise, framed, oracle_csrmm_d, oracle_csrmm_f64,
                     oracle_csrmm_pieces_f32)
from kernel_cases import ALPHA, BETA

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F = np.float32
NT, SEQ = 1, 2  # SPMM_CSR_NT_STREAMS, SPMM_CSR_SEQUENTIAL_ROWS
K = fp.K


@pytest.fixture(scope="module")
def arenas(device):
    t0 = time.perf_counter()
    made = []
    try:
        for _ in range(3):
            made.append(fp.PosArena())
    except torch.cuda.OutOfMemoryError:
        for a in made:
            a.close()
        pytest.skip(f"no 3 x {fp.POS_ARENA_BYTES} bytes of device memory for the arenas")
    torch.cuda.synchronize()
    print(f"\nfar-position arenas: 3 x {fp.POS_ARENA_BYTES} bytes allocated in "
          f"{time.perf_counter() - t0:.3f} s")
    yield made
    for a in made:
        a.close()


def handle_for(w, flags=0):
    from spmm_hip import ops
    h = ops.Handle()
    h.set_csr_options(flags)
    if w.size == "large":
        h.set_csr_waves_per_cu(1)
    return h


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda")


def _rng(w, salt=0):
    return np.random.default_rng(zlib.crc32(w.name.encode()) + salt)


class Site:
    """One placement of a window's arrays: far (in the arenas, at w.start) or the near twin
    (every array in a small buffer of its own, at w.twin_start())."""

    def __init__(self, w, arenas, base=None):
        self.w, self.arenas, self.near = w, arenas, arenas is None
        self.base = w.base if base is None else base
        self.start = w.twin_start() if self.near else w.start
        self.end = self.start + w.nnz
        self.inputs = []

    def put(self, slot, host, per=1, byte_off=0, output=False):
        if self.near:
            buf = torch.empty(fp.twin_bytes(self.w, host.dtype.itemsize, per), dtype=torch.uint8,
                              device="cuda")
            byte_off = 0
        else:
            buf = self.arenas[slot].buf
            assert fp.last_byte(self.w, host.dtype.itemsize, per, byte_off) <= buf.numel()
        p = fp.place(buf, self.w, self.near, host, per, byte_off)
        if not output:
            self.inputs.append(p)
        return p

    def rowptr(self):
        rp = self.start + self.w.local + self.base
        assert rp[-1] <= fp.INT_MAX
        return _dev(rp.astype(np.int32))

    def colind(self, slot=0):
        """The window's colind (+ base) between guards of valid columns."""
        ci = fp.colind_of(self.w.size, self.w.long_last)
        front, back = fp.colind_guards(len(self.w.name))
        return self.put(slot, fp.with_guards(ci + self.base, 1, front + self.base,
                                             back + self.base))

    def unchanged(self, what):
        for p in self.inputs:
            p.unchanged(what)


def need(rec, pattern, what):
    assert any(re.search(pattern, k) for k in rec), f"{what}: no {pattern} among {sorted(set(rec))}"


def same_bits(far, near, what):
    far, near = np.ascontiguousarray(far), np.ascontiguousarray(near)
    assert far.shape == near.shape and far.dtype.itemsize == near.dtype.itemsize
    it = fp.INT_TYPE[far.dtype.itemsize]
    bad = far.view(it) != near.view(it)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements of the far result "
                           f"differ in bits from the near twin's, first at "
                           f"{np.argwhere(bad)[0].tolist()}")


def both(w, arenas, run, base=None):
    """run(site) on the far placement and on the near twin: (far result, near result). A
    result is an array or a tuple of arrays; every pair must agree in bits."""
    far = run(Site(w, arenas, base))
    near = run(Site(w, None, base))
    torch.cuda.synchronize()
    fs, ns = (far, near) if isinstance(far, tuple) else ((far,), (near,))
    for i, (f, n) in enumerate(zip(fs, ns)):
        same_bits(f, n, f"{w.name} result {i}")
    return far, near


def local_rp(w):
    return w.local.astype(np.int32)


def ci0(w):
    return fp.colind_of(w.size, w.long_last)


# ------------------------------------------------------------------- 1. the CSR product, fp32
CSRMM_F32 = [(n, seq, nt) for n, seq in ((5, 0), (64, 0), (64, SEQ), (72, 0), (136, 0))
             for nt in (0, NT)]
VEC_OF = {5: 1, 64: 1, 72: 2, 136: 4}


def product_case(w, n, vdt, seed):
    rng = _rng(w, seed)
    v = rng.uniform(-1, 1, w.nnz).astype(vdt)
    Bd = rng.uniform(-1, 1, (K, n)).astype(vdt)
    C0 = rng.uniform(-1, 1, (w.m, n)).astype(np.float64 if vdt == np.float64 else F)
    return v, Bd, C0


def run_product(call, site, v, Bd, C0, what, colind_slot=0):
    """colind and val on the site, B and C framed near: C as the call left it."""
    w = site.w
    ci = site.colind(colind_slot)
    pv = site.put(1, fp.with_guards(v))
    dB, chkB = framed(Bd, Bd.shape[1], 0)
    dC, getC = framed(C0, C0.shape[1], 0)
    tdt = getattr(torch, v.dtype.name)
    call(site.rowptr(), ci.tensor(torch.int32, site.end), pv.tensor(tdt, site.end), dB, dC,
         site.base)
    torch.cuda.synchronize()
    site.unchanged(what)
    chkB.unchanged(what + ": B")
    return getC(what + ": C")


def check_pieces(oracle, w, n, v, Bd, C0, got, what, alpha=ALPHA, beta=BETA):
    want = oracle_csrmm_pieces_f32(oracle, w.m, n, local_rp(w), ci0(w), v.astype(F),
                                   Bd.astype(F), n, 0, alpha, beta, C0.reshape(-1), n,
                                   0).reshape(w.m, n)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: the twin differs from the piece oracle in {int(bad.sum())} bits"


@pytest.mark.parametrize("n,seq,nt", CSRMM_F32,
                         ids=[f"n{n}{'-seq' if s else ''}{'-nt' if t else ''}"
                              for n, s, t in CSRMM_F32])
@pytest.mark.parametrize("w", fp.windows("p4"), ids=fp.ids(fp.windows("p4")))
def test_csrmm_f32(arenas, oracle, w, n, seq, nt):
    from spmm_hip import ops
    what = f"csrmm_ex_f32 {w.name} n {n} seq {seq} nt {nt}"
    v, Bd, C0 = product_case(w, n, F, n + seq)
    h = handle_for(w, seq | nt)
    recs = []

    def call(rp, ci, val, dB, dC, base):
        with h.launch_record() as rec:
            ops.csrmm(rp, ci, val, dB, m=w.m, n=n, k=K, ldb=n, C=dC, ldc=n, alpha=ALPHA, beta=BETA,
                      base=base, handle=h)
        recs.append(rec)

    _, near = both(w, arenas, lambda s: run_product(call, s, v, Bd, C0, what))
    group = n == 64 and not seq
    for rec in recs:
        need(rec, rf"csr_group_kernelILb{int(bool(nt))}E" if group else
             rf"CsrMpIfE20csr_mergepath_kernelILi{VEC_OF[n]}ELb{int(bool(nt))}ELi0E", what)
    if group:
        ref, absd = oracle_csrmm_f64(oracle, w.m, n, local_rp(w), ci0(w), v, Bd, n, 0)
        assert_normwise(near, ALPHA * ref + BETA * C0.astype(np.float64),
                        abs(ALPHA) * absd + abs(BETA) * np.abs(C0.astype(np.float64)), TOL_F32, what)
    else:
        check_pieces(oracle, w, n, v, Bd, C0, near, what)
    h.close()


@pytest.mark.parametrize("n", [64, 72])
@pytest.mark.parametrize("w", fp.windows("p4"), ids=fp.ids(fp.windows("p4")))
def test_gespmm_csrmm_f32(arenas, oracle, w, n):
    """The drop-in reads nnz on the device and sizes its grid without it; base 0, C = A B."""
    from spmm_hip import ops
    what = f"gespmm_csrmm_f32 {w.name} n {n}"
    v, Bd, C0 = product_case(w, n, F, 700 + n)

    def call(rp, ci, val, dB, dC, base):
        ops.gespmm_csrmm(rp, ci, val, dB[:K * n].view(K, n), dC[:w.m * n].view(w.m, n))

    _, near = both(w, arenas, lambda s: run_product(call, s, v, Bd, C0, what), base=0)
    if n == 64:
        ref, absd = oracle_csrmm_f64(oracle, w.m, n, local_rp(w), ci0(w), v, Bd, n, 0)
        assert_normwise(near, ref, absd, TOL_F32, what)
    else:
        check_pieces(oracle, w, n, v, Bd, C0, near, what, 1.0, 0.0)


# ------------------------------------------------------------------- 2. the CSR product, fp16
@pytest.mark.parametrize("nt", [0, NT], ids=["plain", "nt"])
@pytest.mark.parametrize("n", [5, 72, 136])
@pytest.mark.parametrize("w", fp.windows("p4"), ids=fp.ids(fp.windows("p4")))
def test_csrmm_f16(arenas, oracle, w, n, nt):
    """W30 is the 2^31-byte crossing of val and the 2^32-byte crossing of colind. Both stream
    policies: the chunk loads have a plain and a nontemporal arm."""
    from spmm_hip import ops
    what = f"csrmm_ex_f16 {w.name} n {n} nt {nt}"
    v, Bd, C0 = product_case(w, n, np.float16, 200 + n)
    h = handle_for(w, nt)
    recs = []

    def call(rp, ci, val, dB, dC, base):
        with h.launch_record() as rec:
            ops.csrmm_f16(rp, ci, val, dB, m=w.m, n=n, k=K, ldb=n, C=dC, ldc=n, alpha=ALPHA,
                          beta=BETA, base=base, handle=h)
        recs.append(rec)

    _, near = both(w, arenas, lambda s: run_product(call, s, v, Bd, C0, what))
    for rec in recs:
        need(rec, rf"CsrMpIDF16_E20csr_mergepath_kernelILi{VEC_OF[n]}ELb{int(bool(nt))}ELi0E", what)
    check_pieces(oracle, w, n, v, Bd, C0, near, what)
    h.close()


@pytest.mark.parametrize("w", fp.windows("p4"), ids=fp.ids(fp.windows("p4")))
def test_gespmm_csrmm_f16(arenas, oracle, w):
    from spmm_hip import ops
    n = 72
    what = f"gespmm_csrmm_f16 {w.name}"
    v, Bd, C0 = product_case(w, n, np.float16, 272)

    def call(rp, ci, val, dB, dC, base):
        ops.gespmm_csrmm_f16(rp, ci, val, dB[:K * n].view(K, n), dC[:w.m * n].view(w.m, n))

    _, near = both(w, arenas, lambda s: run_product(call, s, v, Bd, C0, what), base=0)
    check_pieces(oracle, w, n, v, Bd, C0, near, what, 1.0, 0.0)


# ------------------------------------------------------------------- 3. the hot-column entry
HOT_LD = 1 << 20  # leading dimension of the far B: 1024 rows of 4 MiB are 2^32 bytes


@pytest.mark.parametrize("n,hot", [(5, 2), (64, 2), (72, 2), (136, 2), (72, 1), (136, 1)],
                         ids=lambda x: str(x))
@pytest.mark.parametrize("w", fp.windows("p4"), ids=fp.ids(fp.windows("p4")))
def test_csrmm_hot(arenas, oracle, w, n, hot):
    """The tagged colind is made by spmm_csr_hot_analysis on the window alone (the pointers at
    the window's start, nnz the window's length) into the far colind_hot array at the same
    positions (colind's arena, HOT_BYTE_OFF bytes on); the product runs on the far arrays.
    hot 2: B near, one buffer resource for all of B. hot 1: k + base = 1024 rows of 4 MiB (B in
    the third arena, of which the 64 rows the matrix uses are written): a resource per row.
    A hot budget of far_pos_cases.HOT_ROWS rows tags some columns and leaves others; the tags
    are held to the analysis' rule restated on the host."""
    from spmm_hip import ops
    what = f"csrmm_hot_f32 {w.name} n {n} hot {hot}"
    v, Bd, C0 = product_case(w, n, F, 300 + n + hot)
    h = handle_for(w, 0)
    k = K if hot == 2 else 1024 - w.base
    if hot == 2:
        dB, chkB = framed(Bd, n, 0)
        ldb, chk_b = n, chkB.unchanged
    else:
        fb = arenas[2].place(Bd, HOT_LD)
        dB, ldb, chk_b = fb.view, HOT_LD, fb.unchanged
    recs, tags = [], []

    def run(site):
        ci = site.colind(0)
        front, back = fp.colind_guards(len(w.name))
        ph = site.put(0, fp.with_guards(np.zeros(w.nnz, np.int32), 1, front + site.base,
                                        back + site.base), byte_off=fp.HOT_BYTE_OFF, output=True)
        pv = site.put(1, fp.with_guards(v))
        dC, getC = framed(C0, n, 0)
        with h.launch_record() as rec:
            ops.csr_hot_analysis(ci.window(torch.int32), n=n, k=k, base=site.base,
                                 hot_bytes=fp.hot_bytes(n), out=ph.window(torch.int32), handle=h)
            ops.csrmm_hot(site.rowptr(), ph.tensor(torch.int32, site.end),
                          pv.tensor(torch.float32, site.end), dB, m=w.m, n=n, k=k, ldb=ldb, C=dC,
                          ldc=n, alpha=ALPHA, beta=BETA, base=site.base, handle=h)
        torch.cuda.synchronize()
        recs.append(rec)
        site.unchanged(what)
        chk_b(what + ": B")
        tag = ph.read(what + ": colind_hot")
        tags.append(tag)
        return getC(what + ": C"), tag

    (_, _), (near, tag) = both(w, arenas, run)
    for rec in recs:
        need(rec, r"hot_tag_kernel", what)
        if n == 64:
            need(rec, r"csr_group_kernelILb1ELi16ELi4ELb1E", what)
        else:
            need(rec, rf"CsrMpIfE20csr_mergepath_kernelILi{VEC_OF[n]}ELb1ELi{hot}E", what)
    tagged = tag < 0
    assert 0 < int(tagged.sum()) < w.nnz, f"{what}: {int(tagged.sum())} tagged of {w.nnz}"
    assert np.array_equal(tag & 0x7fffffff, ci0(w) + w.base), f"{what}: a tagged index changed"
    assert np.array_equal(tagged, fp.hot_columns(ci0(w), k)[ci0(w)]), \
        f"{what}: the tags are not the {fp.HOT_ROWS} most used columns'"
    if n == 64:
        ref, absd = oracle_csrmm_f64(oracle, w.m, n, local_rp(w), ci0(w), v, Bd, n, 0)
        assert_normwise(near, ALPHA * ref + BETA * C0.astype(np.float64),
                        abs(ALPHA) * absd + abs(BETA) * np.abs(C0.astype(np.float64)), TOL_F32, what)
    else:
        check_pieces(oracle, w, n, v, Bd, C0, near, what)
    h.close()


# --------------------------------------------------------------------------------- 4. fp64
@pytest.mark.parametrize("entry", ["ex", "gespmm"])
@pytest.mark.parametrize("w", fp.windows("p8"), ids=fp.ids(fp.windows("p8")))
def test_csrmm_f64(arenas, oracle, w, entry):
    from spmm_hip import ops
    n = 70
    what = f"csrmm_{entry}_f64 {w.name}"
    v, Bd, C0 = product_case(w, n, np.float64, 64)
    h = handle_for(w, 0)
    recs = []

    def call(rp, ci, val, dB, dC, base):
        if entry == "gespmm":
            ops.gespmm_csrmm(rp, ci, val, dB[:K * n].view(K, n), dC[:w.m * n].view(w.m, n))
            return
        with h.launch_record() as rec:
            ops.csrmm(rp, ci, val, dB, m=w.m, n=n, k=K, ldb=n, C=dC, ldc=n, alpha=ALPHA, beta=BETA,
                      base=base, handle=h)
        recs.append(rec)

    _, near = both(w, arenas, lambda s: run_product(call, s, v, Bd, C0, what),
                   base=0 if entry == "gespmm" else None)
    for rec in recs:
        need(rec, "csr_f64_kernel", what)
    al, be = (ALPHA, BETA) if entry == "ex" else (1.0, 0.0)
    # one sequential fp64 fma chain in CSR order: the oracle's own rule, bit for bit
    # (tests/test_gpu_f64.py holds csr_f64_kernel to it the same way)
    want = oracle_csrmm_d(oracle, w.m, n, local_rp(w), ci0(w), v, Bd, n, 0, al, be, C0.reshape(-1),
                          n, 0).reshape(w.m, n)
    bad = np.ascontiguousarray(near).view(np.int64) != want.view(np.int64)
    assert not bad.any(), \
        f"{what}: the twin differs from the sequential fp64 oracle in {int(bad.sum())} elements"
    h.close()


# -------------------------------------------------------------------------------- 5. SDDMM
# n per kernel family (tests/kernel_cases.py): G = 4, G = 64 with two chunks a lane, wide
SDDMM_N = {12: r"12sddmm_kernelILi4ELi1E", 260: r"12sddmm_kernelILi64ELi2E",
           1028: r"17sddmm_wide_kernel"}


def rows_of(w):
    return np.repeat(np.arange(w.m), w.lens)


def sddmm_want(w, n, X, Y, alpha, beta, old):
    """The restated rule on the small windows, its host form on the large ones."""
    if w.size == "small":
        return sd.reference_bits(rows_of(w), ci0(w).astype(np.int64), X, Y, alpha, beta, old)
    from spmm_hip import prep
    out = np.zeros(w.nnz, F) if old is None else old.copy()
    return prep.sddmm(w.m, n, K, local_rp(w), ci0(w), X, Y, out=out, alpha=alpha, beta=beta)


@pytest.mark.parametrize("beta", [0.0, BETA])
@pytest.mark.parametrize("n", list(SDDMM_N))
@pytest.mark.parametrize("w", fp.windows("p4"), ids=fp.ids(fp.windows("p4")))
def test_sddmm(arenas, w, n, beta):
    """beta = 0: the far out holds the sentinel and is never read; beta != 0: old values."""
    from spmm_hip import ops
    what = f"sddmm_csr_f32 {w.name} n {n} beta {beta}"
    rng = _rng(w, 500 + n)
    X = rng.uniform(-1, 1, (w.m, n)).astype(F)
    Y = rng.uniform(-1, 1, (K, n)).astype(F)
    old = rng.uniform(-1, 1, w.nnz).astype(F) if beta else None
    h = handle_for(w, 0)
    dX, chkX = framed(X, n, 0)
    dY, chkY = framed(Y, n, 0)
    recs = []

    def run(site):
        ci = site.colind(0)
        fill = old if beta else np.full(w.nnz, fp.sentinel_bits(4), np.uint32).view(F)
        po = site.put(1, fp.with_guards(fill), output=True)
        with h.launch_record() as rec:
            ops.sddmm(site.rowptr(), ci.tensor(torch.int32, site.end), dX, dY, m=w.m, n=n, k=K,
                      ldx=n, ldy=n, out=po.tensor(torch.float32, site.end), alpha=ALPHA, beta=beta,
                      base=site.base, handle=h)
        torch.cuda.synchronize()
        recs.append(rec)
        site.unchanged(what)
        return po.read(what + ": out").view(F)

    _, near = both(w, arenas, run)
    chkX.unchanged(what + ": X")
    chkY.unchanged(what + ": Y")
    for rec in recs:
        need(rec, SDDMM_N[n], what)
    want = sddmm_want(w, n, X, Y, ALPHA, beta, old)
    assert np.array_equal(sd.bits(near), sd.bits(want)), f"{what}: the twin differs from the rule"
    h.close()


# ------------------------------------------------------------------------- 6. edge softmax
@functools.lru_cache(maxsize=2)  # the forward and the backward case of a window share it
def softmax_case(w, heads):
    rng = _rng(w, 600 + heads)
    x = rng.normal(0, 3, (w.nnz, heads)).astype(F)
    g = rng.normal(0, 1, (w.nnz, heads)).astype(F)
    y = np.stack([fp.softmax_fwd_rule(w.local, np.ascontiguousarray(x[:, h])) for h in range(heads)],
                 axis=1)
    gx = np.stack([fp.softmax_bwd_rule(w.local, np.ascontiguousarray(y[:, h]),
                                    np.ascontiguousarray(g[:, h])) for h in range(heads)], axis=1)
    return x, g, np.ascontiguousarray(y), np.ascontiguousarray(gx)


def run_softmax(w, arenas, heads, bwd):
    """x -> y (bwd: y, g -> gx), every array far, for one head ([nnz]) or several
    ([nnz, heads]); the near twin's output against the restated rule."""
    from spmm_hip import ops
    what = f"edge_softmax{'_bwd' if bwd else ''} {w.name} heads {heads}"
    x, g, y, gx = softmax_case(w, heads)
    h = handle_for(w, 0)
    recs = []
    sent = np.full(w.nnz * heads, fp.sentinel_bits(4), np.uint32).view(F)

    def shaped(p, site):
        t = p.tensor(torch.float32, site.end)
        return t if heads == 1 and w.heads == 1 else t.view(site.end, heads)

    def run(site):
        ins = [site.put(i, fp.with_guards(a, heads), heads)
               for i, a in enumerate((y, g) if bwd else (x,))]
        po = site.put(len(ins), fp.with_guards(sent, heads), heads, output=True)
        many = not (heads == 1 and w.heads == 1)
        fn = {(0, 0): ops.edge_softmax, (1, 0): ops.edge_softmax_bwd,
              (0, 1): ops.edge_softmax_heads, (1, 1): ops.edge_softmax_bwd_heads}[int(bwd), int(many)]
        with h.launch_record() as rec:
            fn(site.rowptr(), *[shaped(p, site) for p in ins], m=w.m, base=site.base,
               out=shaped(po, site), handle=h)
        torch.cuda.synchronize()
        recs.append(rec)
        site.unchanged(what)
        return po.read(what + ": out").view(F).reshape(w.nnz, heads)

    _, near = both(w, arenas, run)
    # far: nnz / m leaves G = 64 alone; the twin's launcher may choose fewer lanes per short
    # row from its small nnz, and the bits must still be the row's
    kern = "edge_softmax_kernel" if heads == 1 and w.heads == 1 else "edge_softmax_heads_kernel"
    need(recs[0], rf"{kern}ILi64ELb{int(bwd)}E", what + " (far)")
    need(recs[1], rf"{kern}ILi\d+ELb{int(bwd)}E", what + " (twin)")
    want = gx if bwd else y
    assert np.array_equal(sd.bits(near), sd.bits(want)), f"{what}: the twin differs from the rule"
    h.close()


@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("w", fp.windows("p4"), ids=fp.ids(fp.windows("p4")))
def test_edge_softmax(arenas, w, bwd):
    """The launcher chooses its kernel from the nnz argument, the window's end here."""
    run_softmax(w, arenas, 1, bwd)


# ---------------------------------------------------------------------------- 7. multi-head
HEADS_W = fp.windows("q3") + fp.windows("q8")
SDDMM_D = {3: 5, 8: 8}     # G = 2, scalar and vector loads
PRODUCT_D = {3: 5, 8: 40}  # W = 15: VEC 1; W = 320: VEC 4, two column tiles
TORCH_TYPE = {"f16": torch.float16, "bf16": torch.bfloat16}


def features(rng, rows, heads, d, ty):
    """([rows, heads, d] device tensor of type ty, the same values widened to float32)."""
    a = rng.uniform(-1, 1, (rows, heads, d)).astype(F)
    if ty == "f32":
        return _dev(a), a
    bits, wide = hh.rounded(a, ty)
    return (_dev(bits.view(np.int16)).view(TORCH_TYPE[ty]),
            np.ascontiguousarray(wide).reshape(rows, heads, d))


@pytest.mark.parametrize("ty", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("w", HEADS_W, ids=fp.ids(HEADS_W))
def test_sddmm_heads(arenas, w, ty):
    from spmm_hip import ops
    heads, d = w.heads, SDDMM_D[w.heads]
    what = f"sddmm_csr_heads_{ty} {w.name} d {d}"
    rng = _rng(w, 700)
    dX, X = features(rng, w.m, heads, d, ty)
    dY, Y = features(rng, K, heads, d, ty)
    old = rng.uniform(-1, 1, (w.nnz, heads)).astype(F)
    h = handle_for(w, 0)
    recs = []

    def run(site):
        ci = site.colind(0)
        po = site.put(1, fp.with_guards(old, heads), heads, output=True)
        with h.launch_record() as rec:
            ops.sddmm_heads(site.rowptr(), ci.tensor(torch.int32, site.end), dX, dY, m=w.m, d=d,
                            heads=heads, k=K, out=po.tensor(torch.float32, site.end).view(site.end, heads),
                            alpha=ALPHA, beta=BETA, base=site.base, handle=h)
        torch.cuda.synchronize()
        recs.append(rec)
        site.unchanged(what)
        return po.read(what + ": out").view(F).reshape(w.nnz, heads)

    _, near = both(w, arenas, run)
    for rec in recs:
        need(rec, r"sddmm_heads_kernelI(f|DF16_|t)Li2E", what)
    if w.size == "small":
        want = np.stack([sd.reference_bits(rows_of(w), ci0(w).astype(np.int64),
                                           np.ascontiguousarray(X[:, hd]),
                                           np.ascontiguousarray(Y[:, hd]), ALPHA, BETA,
                                           np.ascontiguousarray(old[:, hd]))
                         for hd in range(heads)], axis=1)
    else:
        from spmm_hip import prep
        want = prep.sddmm_heads(w.m, d, K, heads, local_rp(w), ci0(w), X, Y, out=old.copy(),
                                alpha=ALPHA, beta=BETA)
    assert np.array_equal(sd.bits(near), sd.bits(want)), f"{what}: the twin differs from the rule"
    h.close()


@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("w", HEADS_W, ids=fp.ids(HEADS_W))
def test_edge_softmax_heads(arenas, w, bwd):
    run_softmax(w, arenas, w.heads, bwd)


@pytest.mark.parametrize("ty", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("w", HEADS_W, ids=fp.ids(HEADS_W))
def test_csrmm_heads(arenas, w, ty):
    from spmm_hip import ops
    heads, d = w.heads, PRODUCT_D[w.heads]
    what = f"csrmm_heads_{ty} {w.name} d {d}"
    rng = _rng(w, 800)
    dB, Bw = features(rng, K, heads, d, ty)
    val = rng.uniform(-1, 1, (w.nnz, heads)).astype(F)
    C0 = rng.uniform(-1, 1, (w.m, heads * d)).astype(F)
    h = handle_for(w, 0)
    recs = []

    def run(site):
        ci = site.colind(0)
        pv = site.put(1, fp.with_guards(val, heads), heads)
        dC, getC = framed(C0, heads * d, 0)
        with h.launch_record() as rec:
            ops.csrmm_heads(site.rowptr(), ci.tensor(torch.int32, site.end),
                            pv.tensor(torch.float32, site.end), dB, m=w.m, d=d, heads=heads, k=K,
                            C=dC, alpha=ALPHA, beta=BETA, base=site.base, handle=h)
        torch.cuda.synchronize()
        recs.append(rec)
        site.unchanged(what)
        return getC(what + ": C")

    _, near = both(w, arenas, run)
    for rec in recs:
        need(rec, rf"csrmm_heads_kernelI(f|DF16_|t)Li{4 if heads == 8 else 1}E", what)
    want = hc.product_reference_on(w.m, local_rp(w), ci0(w), val, Bw, ALPHA, BETA,
                                   C0.reshape(w.m, heads, d))
    assert np.array_equal(sd.bits(near), sd.bits(want.reshape(w.m, heads * d))), \
        f"{what}: the twin differs from the piece oracle"
    h.close()


@pytest.mark.parametrize("heads", fp.HEADS)
def test_heads_one_position_past_top_is_refused(arenas, heads):
    """nnz = INT_MAX // heads + 1, so nnz * heads > INT_MAX: NOT_SUPPORTED from every multi-head
    entry before anything is queued (the launch record stays empty). The TOP cases above, one
    position shorter, return success."""
    from ctypes import c_void_p

    from spmm_hip import ops
    from spmm_hip._lib import NOT_SUPPORTED, lib
    w = fp.BY_NAME[f"q{heads}-TOP-small"]
    assert (w.end + 1) * heads > fp.INT_MAX >= w.end * heads
    L, h = lib(), ops.Handle()
    rp = _dev(w.rowptr())
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    a = [P(x.buf) for x in arenas]
    f = torch.zeros(K * heads * 8, device="cuda")
    g = {"f32": f, "f16": f.to(torch.float16), "bf16": f.to(torch.bfloat16)}
    nnz, m, d = w.end + 1, w.m, 8
    with h.launch_record() as rec:
        for ty in ("f32", "f16", "bf16"):
            sdd = getattr(L, "spmm_sddmm_csr_heads_" + ty)
            mm = getattr(L, "spmm_csrmm_heads_" + ty)
            assert sdd(h.raw, m, d, 1, nnz, heads, 1.0, P(rp), a[0], 0, P(g[ty]), heads * d,
                       P(g[ty]), heads * d, 0.0, a[1]) == NOT_SUPPORTED, ty
            assert mm(h.raw, m, d, 1, nnz, heads, 1.0, P(rp), a[0], a[1], 0, P(g[ty]), heads * d,
                      0.0, P(f), heads * d) == NOT_SUPPORTED, ty
        assert L.spmm_edge_softmax_csr_heads_f32(h.raw, m, nnz, heads, P(rp), 0, a[0],
                                                 a[1]) == NOT_SUPPORTED
        assert L.spmm_edge_softmax_bwd_csr_heads_f32(h.raw, m, nnz, heads, P(rp), 0, a[0], a[1],
                                                     a[2]) == NOT_SUPPORTED
    torch.cuda.synchronize()
    assert rec == [], f"a refused call queued {rec}"
    h.close()


# ------------------------------------------------------------------------------ 8. csr2csc
@pytest.mark.parametrize("vb", [0, 4], ids=["pattern", "values"])
@pytest.mark.parametrize("w", fp.windows("p4"), ids=fp.ids(fp.windows("p4")))
def test_csr2csc_dev(arenas, w, vb):
    """The CSC arrays are near; perm holds the far absolute positions: it equals the twin's
    shifted by the two starts' distance."""
    from spmm_hip import ops
    what = f"csr2csc_dev {w.name} vb {vb}"
    v = cc.values(w.nnz, vb)
    h = handle_for(w, 0)
    starts = []

    def run(site):
        ci = site.colind(0)
        dv = None
        if vb:
            dv = site.put(1, fp.with_guards(v)).tensor(torch.float32, site.end)
        out = ops.csr2csc(site.rowptr(), ci.tensor(torch.int32, site.end), dv, m=w.m, n=K,
                          base=site.base, base_out=0, return_perm=True, handle=h)
        torch.cuda.synchronize()
        site.unchanged(what)
        starts.append(site.start)
        res = [t.cpu().numpy() for t in out]
        res[-1] = res[-1].astype(np.int64) - site.start  # perm, relative to the window
        return tuple(res)

    far, near = both(w, arenas, run)
    assert starts[0] == w.start and starts[1] == w.twin_start()
    colptr, rowind, cv, perm = cc.reference(w.m, K, w.local + w.base, ci0(w) + w.base, v, w.base, 0)
    assert np.array_equal(near[0], colptr) and np.array_equal(near[1], rowind), what
    assert np.array_equal(near[-1], perm), f"{what}: perm"
    if vb:
        assert np.array_equal(cc.bits(near[2]), cc.bits(cv)), f"{what}: values"
    h.close()
