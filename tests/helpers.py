"""Shared test helpers: oracle loading (tests only), golden fixtures,
tolerance checks."""
from __future__ import annotations

import ctypes
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_SO = os.path.join(ORACLE_DIR, "liboracle.so")
REF_SO = os.path.join(ORACLE_DIR, "_ref", "libref.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")

P = ctypes.c_void_p
I, I64, F, D, U64 = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_uint64

# Norm-wise relative tolerance for fp32 SpMM (north_star: 1e-5 relative):
# |C - C_ref| <= TOL_F32 * sum_j |a_j * b_j| + tiny, per element.
TOL_F32 = 1e-5
# fp16 inputs with fp32 accumulation, checked against the exact (float64)
# product of the SAME fp16 values.
TOL_F16_ACC = 1e-5


def _build_oracle():
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, "oracle"], check=True)


def load_oracle() -> ctypes.CDLL:
    if not os.path.exists(ORACLE_SO):
        _build_oracle()
    L = ctypes.CDLL(ORACLE_SO)
    sig = {
        "oracle_rng_seed": (None, [U64]),
        "oracle_random_array": (None, [I64, F, F, P]),
        "oracle_random_csr": (I64, [I, I, F, F, F, P, P, P, I64]),
        "oracle_csrmm_f32": (None, [I, I, P, P, P, I, P, I, I, F, F, P, I, I]),
        "oracle_csrmm_pieces_f32": (None, [I, I, P, P, P, I, P, I, I, F, F, P, I, I]),
        "oracle_csr_piece_len": (I, [I]),
        "oracle_csrmm_f64": (None, [I, I, P, P, P, I, P, I, I, P, P]),
        "oracle_csrmm_d": (None, [I, I, P, P, P, I, P, I, I, ctypes.c_double, ctypes.c_double,
                                  P, I, I]),
        "oracle_bsrmm_d": (None, [I, I, I, I, P, P, P, P, I, I, ctypes.c_double,
                                  ctypes.c_double, P, I, I]),
        "oracle_spmm_cc_csr": (None, [I64, I64, P, P, P, I64, P]),
        "oracle_spmm_cc_coo": (None, [I64, I64, I64, P, P, P, I64, P]),
        "oracle_coo2csr": (None, [P, I, I, I, P]),
        "oracle_num_threads": (I, []),
        "oracle_reorder": (I, [I, I, P, P, P, P, P]),
        "oracle_bsrmm_f32": (None, [I, I, I, I, P, P, P, P, I, I, F, F, P, I, I]),
        "oracle_bsrmm_f64": (None, [I, I, I, I, P, P, P, P, I, I, I, P, P]),
        "oracle_csr2bsr_nnz": (I64, [I, I, P, P, P]),
        "oracle_csr2bsr": (None, [I, I, I, P, P, P, P, P, P]),
        "oracle_bsr2csr": (None, [I, I, I, P, P, P, P, P, P]),
        "oracle_divide": (I, [I, I, F, P, P, P, P, P, P, P, P, P, I64, P]),
    }
    for k, (r, a) in sig.items():
        f = getattr(L, k)
        f.restype = r
        f.argtypes = a
    return L


def ptr(a: np.ndarray | None):
    return ctypes.c_void_p(a.ctypes.data if a is not None and a.size else 0)


def load_golden() -> dict:
    with open(os.path.join(GOLDEN, "kats.json")) as f:
        kats = json.load(f)
    with open(os.path.join(GOLDEN, "ref_config1.json")) as f:
        cfg1 = json.load(f)
    npz = np.load(os.path.join(GOLDEN, "ref_host.npz"), allow_pickle=False)
    return {"kats": kats, "config1": cfg1, "ref": {k: npz[k] for k in npz.files}}


# ------------------------------------------------------------ oracle calls
def oracle_csrmm_f32(L, m, n, rowptr, colind, val, B, ldb, order_b, alpha=1.0, beta=0.0,
                     C=None, ldc=None, order_c=0, base=0):
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    colind = np.ascontiguousarray(colind, np.int32)
    val = np.ascontiguousarray(val, np.float32)
    B = np.ascontiguousarray(B, np.float32)
    if ldc is None:
        ldc = n if order_c == 0 else m
    if C is None:
        C = np.zeros(m * ldc if order_c == 0 else n * ldc, np.float32)
    C = np.ascontiguousarray(C, np.float32).copy()
    L.oracle_csrmm_f32(m, n, ptr(rowptr), ptr(colind), ptr(val), base, ptr(B), ldb, order_b,
                       alpha, beta, ptr(C), ldc, order_c)
    return C


def oracle_csrmm_pieces_f32(L, m, n, rowptr, colind, val, B, ldb, order_b, alpha=1.0,
                            beta=0.0, C=None, ldc=None, order_c=0, base=0):
    """The HIP CSR kernels' association: sequential fp32 FMA
    chains over pieces of max(128, ceil(L / 64)) nonzeros from each row's start,
    added left to right; the main kernel matches it bit for bit at any grid."""
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    colind = np.ascontiguousarray(colind, np.int32)
    val = np.ascontiguousarray(val, np.float32)
    B = np.ascontiguousarray(B, np.float32)
    if ldc is None:
        ldc = n if order_c == 0 else m
    if C is None:
        C = np.zeros(m * ldc if order_c == 0 else n * ldc, np.float32)
    C = np.ascontiguousarray(C, np.float32).copy()
    L.oracle_csrmm_pieces_f32(m, n, ptr(rowptr), ptr(colind), ptr(val), base, ptr(B), ldb,
                              order_b, alpha, beta, ptr(C), ldc, order_c)
    return C


def oracle_csrmm_d(L, m, n, rowptr, colind, val, B, ldb, order_b, alpha=1.0, beta=0.0,
                   C=None, ldc=None, order_c=0, base=0):
    """gespmm_csrmm<double> semantics: sequential fp64 FMA in CSR order."""
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    colind = np.ascontiguousarray(colind, np.int32)
    val = np.ascontiguousarray(val, np.float64)
    B = np.ascontiguousarray(B, np.float64)
    if ldc is None:
        ldc = n if order_c == 0 else m
    if C is None:
        C = np.zeros(m * ldc if order_c == 0 else n * ldc, np.float64)
    C = np.ascontiguousarray(C, np.float64).copy()
    L.oracle_csrmm_d(m, n, ptr(rowptr), ptr(colind), ptr(val), base, ptr(B), ldb, order_b,
                     alpha, beta, ptr(C), ldc, order_c)
    return C


def oracle_bsrmm_d(L, direction, mb, n, bs, rowptr, colind, val, B, ldb, order_b, alpha=1.0,
                   beta=0.0, C=None, ldc=None, order_c=0):
    """rocsparse_bsrmm_template<double> semantics: blocks in order, q = 0..bs-1."""
    m = mb * bs
    if ldc is None:
        ldc = n if order_c == 0 else m
    if C is None:
        C = np.zeros(m * ldc if order_c == 0 else n * ldc, np.float64)
    C = np.ascontiguousarray(C, np.float64).copy()
    args = [np.ascontiguousarray(a, t) for a, t in
            ((rowptr, np.int32), (colind, np.int32), (val, np.float64), (B, np.float64))]
    L.oracle_bsrmm_d(direction, mb, n, bs, *[ptr(a) for a in args], ldb, order_b, alpha, beta,
                     ptr(C), ldc, order_c)
    return C


def oracle_csrmm_f64(L, m, n, rowptr, colind, val, B, ldb, order_b, base=0):
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    colind = np.ascontiguousarray(colind, np.int32)
    val = np.ascontiguousarray(val, np.float32)
    B = np.ascontiguousarray(B, np.float32)
    C = np.zeros((m, n), np.float64)
    A = np.zeros((m, n), np.float64)
    L.oracle_csrmm_f64(m, n, ptr(rowptr), ptr(colind), ptr(val), base, ptr(B), ldb, order_b,
                       ptr(C), ptr(A))
    return C, A


def oracle_bsrmm_f32(L, direction, mb, n, bs, rowptr, colind, val, B, ldb, order_b, alpha=1.0,
                     beta=0.0, C=None, ldc=None, order_c=0):
    m = mb * bs
    if ldc is None:
        ldc = n if order_c == 0 else m
    if C is None:
        C = np.zeros(m * ldc if order_c == 0 else n * ldc, np.float32)
    C = np.ascontiguousarray(C, np.float32).copy()
    args = [np.ascontiguousarray(a, t) for a, t in
            ((rowptr, np.int32), (colind, np.int32), (val, np.float32), (B, np.float32))]
    L.oracle_bsrmm_f32(direction, mb, n, bs, *[ptr(a) for a in args], ldb, order_b, alpha, beta,
                       ptr(C), ldc, order_c)
    return C


def oracle_bsrmm_f64(L, direction, mb, n, bs, rowptr, colind, val, B, ldb, order_b, half=False):
    m = mb * bs
    C = np.zeros((m, n), np.float64)
    A = np.zeros((m, n), np.float64)
    vt = np.float16 if half else np.float32
    args = [np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(colind, np.int32),
            np.ascontiguousarray(val, vt), np.ascontiguousarray(B, vt)]
    L.oracle_bsrmm_f64(direction, mb, n, bs, *[ptr(a) for a in args], ldb, order_b, int(half),
                       ptr(C), ptr(A))
    return C, A


def oracle_divide(L, n, bs, density, rowptr, colind, val):
    """divide_matrix with values -> (csr_rp, csr_ci, csr_v, bsr_rp, bsr_ci, bsr_v)."""
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    colind = np.ascontiguousarray(colind, np.int32)
    val = np.ascontiguousarray(val, np.float32)
    nb = (n + bs - 1) // bs
    cap = nb * nb if density <= 0 else max(colind.size, 1)
    crp, cci, cv = (np.zeros(n + 1, np.int32), np.zeros(max(colind.size, 1), np.int32),
                    np.zeros(max(colind.size, 1), np.float32))
    brp, bci, bv = np.zeros(nb + 1, np.int32), np.zeros(cap, np.int32), \
        np.zeros(cap * bs * bs, np.float32)
    out = np.zeros(2, np.int64)
    assert L.oracle_divide(n, bs, density, ptr(rowptr), ptr(colind), ptr(val), ptr(crp),
                           ptr(cci), ptr(cv), ptr(brp), ptr(bci), ptr(bv), cap, ptr(out)) == 0
    c, b = int(out[0]), int(out[1])
    return crp, cci[:c].copy(), cv[:c].copy(), brp, bci[:b].copy(), bv[:b * bs * bs].copy()


def assert_normwise(got, ref64, absdot, tol, what=""):
    """|got - ref| <= tol * absdot + 1e-30 elementwise (float64 comparison). A NaN or
    an infinity in got where the reference is finite is outside it (`err > bound` alone
    is False for a NaN error and would let an all-NaN result pass)."""
    got = np.asarray(got, np.float64)
    ref64, absdot = np.asarray(ref64, np.float64), np.asarray(absdot, np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref64)
        bound = tol * absdot + 1e-30
        bad = (err > bound) | (np.isfinite(ref64) & np.isfinite(bound) & ~(err <= bound))
    if bad.any():
        i = np.flatnonzero(bad)[np.argmax(np.nan_to_num((err - bound).ravel()[bad.ravel()],
                                                        nan=np.inf, posinf=np.inf))]
        raise AssertionError(
            f"{what}: {int(bad.sum())} / {bad.size} elements outside the norm-wise tolerance "
            f"{tol}; worst flat index {i}: got {got.flat[i]!r} ref {ref64.flat[i]!r} "
            f"|a||b| {absdot.flat[i]!r}")


# ------------------------------------------------------- framed operands
# Sentinels of the words a kernel must leave alone (or never sum): NaNs with a
# payload, compared as raw bits. They are signalling NaNs (quiet bit clear): a copy
# keeps the bits, any arithmetic returns the quiet form, so even an epilogue that
# reads a padding word and writes back beta * word + 0 (a quiet NaN sentinel would
# come back unchanged, payload and all) is caught.
FRAME_GUARD = 256  # elements before and after the matrix (a multiple of 16 bytes in every type)
_FRAME_BITS = {np.dtype(np.float16): (np.uint16, 0x7C2A),
               np.dtype(np.float32): (np.uint32, 0x7F80BEEF),
               np.dtype(np.float64): (np.uint64, 0x7FF00000DEADBEEF)}
_FRAME_WORD = {2: np.uint16, 4: np.uint32, 8: np.uint64}


class FrameChecker:
    """The checker of framed(): calling it reads the whole buffer back, asserts bit
    for bit that every sentinel word (front guard, offset gap, padding columns, back
    guard) still holds the sentinel and returns the rows x cols data region;
    unchanged() asserts that the data region kept its bits too (an input operand)."""

    def __init__(self, buffer, host, rows, cols, ld, off, guard):
        self.buffer, self.host = buffer, host
        self.rows, self.cols, self.ld, self.off, self.guard = rows, cols, ld, off, guard
        self.start = guard + off
        self.word = _FRAME_WORD[host.dtype.itemsize]

    def _read(self):
        return self.buffer.cpu().numpy()

    def _fail(self, what, region, where, got, want):
        raise AssertionError(f"{what}: {region} changed, first at {where}: "
                             f"{int(got):#x}, was {int(want):#x}")

    def __call__(self, what="", _got=None):
        got = self._read() if _got is None else _got
        g, h = got.view(self.word), self.host.view(self.word)
        body0, body1 = self.start, self.start + self.rows * self.ld
        for region, a, b in (("front guard", 0, self.guard), ("offset gap", self.guard, body0),
                             ("back guard", body1, g.size)):
            bad = np.flatnonzero(g[a:b] != h[a:b])
            if bad.size:
                self._fail(what, region, f"index {int(bad[0])} of {b - a}", g[a + bad[0]],
                           h[a + bad[0]])
        gb = g[body0:body1].reshape(self.rows, self.ld)
        hb = h[body0:body1].reshape(self.rows, self.ld)
        bad = np.argwhere(gb[:, self.cols:] != hb[:, self.cols:])
        if bad.size:
            r, c = int(bad[0][0]), self.cols + int(bad[0][1])
            self._fail(what, "padding columns", f"row {r} column {c} (ld {self.ld})", gb[r, c],
                       hb[r, c])
        return got[body0:body1].reshape(self.rows, self.ld)[:, :self.cols].copy()

    def unchanged(self, what=""):
        got = self._read()  # one readback serves both checks
        self(what, got)
        g = got.view(self.word)
        bad = np.flatnonzero(g != self.host.view(self.word))
        if bad.size:
            i = int(bad[0]) - self.start
            self._fail(what, "data region", f"row {i // self.ld} column {i % self.ld}",
                       g[bad[0]], self.host.view(self.word)[bad[0]])


def framed(data2d, ld, off, *, fill=None, device="cuda", guard=FRAME_GUARD):
    """A rows x cols host array inside a flat buffer on `device`, laid out as
      [front guard | off elements | rows x ld, the data in columns 0..cols-1 | back guard]
    with guards of `guard` (>= 256) elements. The off elements, every padding column
    and both guards hold `fill`: by default the type's sentinel NaN (floating types;
    integer arrays name their own, e.g. a valid index). Returns (view, checker): the
    flat tensor that starts at the data (what a caller passes as B or C with leading
    dimension ld) and its FrameChecker. The view's address modulo 16 is asserted to
    be what off implies, so a test reaches the alignment it claims."""
    import torch
    data2d = np.ascontiguousarray(data2d)
    rows, cols = data2d.shape
    dt = data2d.dtype
    assert ld >= cols and off >= 0 and guard >= FRAME_GUARD and guard * dt.itemsize % 16 == 0
    host = np.empty(guard + off + rows * ld + guard, dt)
    if fill is None:
        word, bits = _FRAME_BITS[dt]
        host.view(word)[:] = bits
    else:
        host[:] = fill
    start = guard + off
    host[start:start + rows * ld].reshape(rows, ld)[:, :cols] = data2d
    buffer = torch.from_numpy(host.copy()).to(device)
    assert buffer.data_ptr() % 16 == 0, "the allocation itself must be 16-byte aligned"
    view = buffer[start:]
    assert view.data_ptr() % 16 == off * dt.itemsize % 16
    return view, FrameChecker(buffer, host, rows, cols, ld, off, guard)


# Layouts (off_B, pad_B, off_C, pad_C) in elements that keep every fast path (16-byte
# bases, ld a multiple of 16 bytes) yet leave the allocation's 256-byte alignment.
ALIGNED_LAYOUTS_F32 = [(4, 0, 0, 0), (0, 0, 4, 0), (4, 4, 12, 8), (0, 12, 4, 4)]
# fp16 entries: B's part (off, pad) in halves, a multiple of 8; C (floats) has no
# requirement there, so each B part goes with every C part.
ALIGNED_B_F16 = [(8, 0), (8, 8), (0, 16)]
C_PARTS_F16 = [(0, 0), (4, 8), (1, 0), (0, 1), (3, 1)]
ALIGNED_LAYOUTS_F16 = [b + c for b in ALIGNED_B_F16 for c in C_PARTS_F16]

# The grouped entries' cases (tests/test_gpu_layout_analysed.py runs them,
# tests/test_layout_helpers.py checks on the host that each list reaches what it
# claims): (n, order_b, order_c, (off_B, pad_B, off_C, pad_C)), n = None for "every n
# of the test". A column-major operand's ld is its row count plus the pad.
_COL_PARTS_F32 = [(0, 0), (0, 1), (4, 3), (4, 4)]  # 16-byte bases, every pad of 0 / 1 / 3 / 4
GROUPED_F32_ACCEPTED = (
    [(None, 0, 0, lay) for lay in [(0, 0, 0, 0), (0, 4, 0, 8)] + ALIGNED_LAYOUTS_F32] +
    [(None, 1, 0, b + (12, 8)) for b in _COL_PARTS_F32] +
    [(None, 0, 1, (4, 4) + c) for c in _COL_PARTS_F32] +
    [(None, 1, 1, b + c) for b, c in zip(_COL_PARTS_F32, reversed(_COL_PARTS_F32))])
GROUPED_F32_REJECTED = (
    [(None, 0, 0, lay) for lay in [(0, 1, 0, 0), (0, 2, 0, 0), (0, 0, 0, 1), (0, 0, 0, 2),
                                   (1, 0, 0, 0), (2, 0, 0, 0), (0, 0, 1, 0), (0, 0, 2, 0)]] +
    [(None, 1, 0, (1, 0, 0, 0)), (None, 1, 0, (2, 3, 0, 0)), (None, 0, 1, (0, 0, 1, 0)),
     (None, 0, 1, (0, 0, 2, 1)), (130, 0, 0, (0, 2, 0, 2))])
GROUPED_F16_ACCEPTED = (
    [(None, 0, 0, b + c) for b in [(0, 0)] + ALIGNED_B_F16 for c in C_PARTS_F16] +
    [(None, 0, 1, b + c) for b, c in zip(ALIGNED_B_F16, [c for c in C_PARTS_F16 if c[1]])] +
    [(None, 1, 0, b + (0, 0)) for b in [(0, 0), (8, 1), (0, 8)]])
GROUPED_F16_REJECTED = [(None, 0, 0, (0, 1, 0, 0)), (None, 0, 0, (0, 4, 0, 0)),
                        (None, 0, 0, (1, 0, 0, 0)), (None, 0, 0, (4, 0, 0, 0)),
                        (132, 0, 0, (0, 4, 0, 0))]


# --------------------------------------------------------- BSR test matrices
def rand_bsr(rng, mb, kb, bs, p, empty_rows=()):
    rows = []
    for br in range(mb):
        cols = np.nonzero(rng.random(kb) < p)[0] if br not in empty_rows else np.zeros(0, int)
        rows.append(cols)
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32) if rp[-1] else np.zeros(0, np.int32)
    val = rng.uniform(-1, 1, rp[-1] * bs * bs).astype(np.float32)
    return rp, ci, val


def column_sparse_bsr(rng, mb, kb, bs, p):
    """BSR whose blocks are mostly empty columns, like csr2bsr output of a
    sparse graph: per block a random number of active columns (0 = an
    explicit all-zero block, 1 = a single-column block, up to bs), each
    active column holding a few nonzeros."""
    rp, ci, _ = rand_bsr(rng, mb, kb, bs, p, empty_rows=(3,))
    nnzb = int(rp[-1])
    v = np.zeros((nnzb, bs, bs), np.float32)
    for b in range(nnzb):
        kind = b % 5
        ncols = {0: 0, 1: 1, 2: 2, 3: bs // 4, 4: bs}[kind]
        cols = rng.choice(bs, ncols, replace=False)
        for c in cols:
            rows = rng.random(bs) < 0.3
            rows[rng.integers(bs)] = True
            v[b, rows, c] = rng.uniform(-1, 1, int(rows.sum()))
    return rp, ci, v.reshape(-1)


def long_row_column_sparse_bsr(rng, mb, kb, bs, long_row=5, long_blocks=300):
    """The matrix of test_bsrmm_analysed / test_bsrmm_analysed_f16 (tests/test_gpu_bsr.py):
    column_sparse_bsr at fill 0.1 (block row 3 empty), block row `long_row` replaced
    by `long_blocks` column-sparse blocks (several 64-block chunks, and segments on a
    shallow grid). fp32 ROW-direction values."""
    rp, ci, v = column_sparse_bsr(rng, mb, kb, bs, 0.1)
    rows = [ci[rp[i]:rp[i + 1]] for i in range(mb)]
    vals = [v.reshape(-1, bs * bs)[rp[i]:rp[i + 1]] for i in range(mb)]
    rows[long_row] = np.sort(rng.choice(kb, long_blocks, replace=False)).astype(np.int32)
    _, _, extra = column_sparse_bsr(rng, 1, long_blocks, bs, 1.0)
    vals[long_row] = extra.reshape(-1, bs * bs)[:long_blocks]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    return rp, ci, np.concatenate(vals).reshape(-1).astype(np.float32)


def oracle_reorder(L, kind: str, rowptr, colind, perm=None):
    """Reordered CSR from the oracle's restatement of reorder_strategy.cc."""
    k = {"degree": 0, "bfs": 1, "rcm": 2, "permute": 3}[kind]
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    colind = np.ascontiguousarray(colind, np.int32)
    n = rowptr.size - 1
    perm = np.zeros(max(n, 1), np.int32) if perm is None else np.ascontiguousarray(perm, np.int32)
    orp, oci = np.zeros(n + 1, np.int32), np.zeros(max(colind.size, 1), np.int32)
    assert L.oracle_reorder(k, n, ptr(rowptr), ptr(colind), ptr(perm), ptr(orp), ptr(oci)) == 0
    return orp, oci[:colind.size]


def load_reorder_golden():
    return np.load(os.path.join(GOLDEN, "ref_reorder.npz"), allow_pickle=False)
