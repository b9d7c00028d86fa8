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


# ----------------------------------------- hybrid entry with storage orders
# (tests/test_gpu_hybrid_ex.py runs them, tests/test_gpu_handle_reuse.py reuses the
# matrices, tests/test_hybrid_helpers.py checks on the host that they reach what the
# tests claim)
HYBRID_EX_M = 700
# prep.divide density per block size at which the community matrix below keeps both a
# BSR part and a CSR remainder; 5 is a block size only bsr_generic_kernel takes
HYBRID_EX_DENSITY = {2: 0.5, 4: 0.3, 8: 0.2, 16: 0.2, 32: 0.1, 64: 0.1, 5: 0.2}
HYBRID_EX_ORDERS = [(1, 1), (0, 1), (1, 0)]  # (order_b, order_c): transB = N, T, the mixed form
HYBRID_EX_N = [64, 136, 7]
# (off_B, pad_B, off_C, pad_C) in floats: tight, 16-byte friendly, off 16 bytes
HYBRID_EX_LAYOUTS = [(0, 0, 0, 0), (4, 4, 4, 4), (1, 1, 1, 3)]
_hybrid_ex_cache: dict = {}


def hybrid_ex_matrix():
    """The 700 x 700 community matrix of test_hybrid_divide_spmm with uniform(-1, 1)
    values -> (rowptr, colind, val)."""
    if "A" not in _hybrid_ex_cache:
        from spmm_hip import prep
        rp, ci = prep.community_csr(HYBRID_EX_M, 40.0, 48, 160, 0.9, 3)
        v = np.random.default_rng(4).uniform(-1, 1, ci.size).astype(np.float32)
        _hybrid_ex_cache["A"] = rp, ci, v
    return _hybrid_ex_cache["A"]


def hybrid_ex_parts(bs):
    """prep.divide of hybrid_ex_matrix() at HYBRID_EX_DENSITY[bs] ->
    (csr_rp, csr_ci, csr_v, bsr_rp, bsr_ci, bsr_v)."""
    if bs not in _hybrid_ex_cache:
        from spmm_hip import prep
        rp, ci, v = hybrid_ex_matrix()
        _hybrid_ex_cache[bs] = prep.divide(HYBRID_EX_M, rp, ci, v, bs, HYBRID_EX_DENSITY[bs])
    return _hybrid_ex_cache[bs]


def framed_operands(Bd, Cd, lay, ob=0, oc=0, device="cuda"):
    """Bd (rows_b x n) and Cd (rows_c x n) framed in the given storage orders on
    lay = (off_B, pad_B, off_C, pad_C): a column-major operand's framed rows are its
    columns and its ld is its row count plus the pad. Returns (B view, B checker, ldb,
    C view, ldc, extract) with extract(what) the guard-checked rows_c x n result."""
    off_b, pad_b, off_c, pad_c = lay
    B2 = Bd if ob == 0 else np.ascontiguousarray(Bd.T)
    C2 = Cd if oc == 0 else np.ascontiguousarray(Cd.T)
    ldb, ldc = B2.shape[1] + pad_b, C2.shape[1] + pad_c
    dB, chkB = framed(B2, ldb, off_b, device=device)
    dC, chkC = framed(C2, ldc, off_c, device=device)

    def extract(what):
        got = chkC(what + ": C")
        return got if oc == 0 else np.ascontiguousarray(got.T)
    return dB, chkB, ldb, dC, ldc, extract


def hybrid_ex_staged_b_bytes(k, bs, n):
    """Bytes of the hybrid's staged copy of a column-major B: ceil(k / bs) * bs rows of
    n floats."""
    return -(-k // bs) * bs * n * 4


def small_grouped_scratch_bytes(m, bs, n):
    """Scratch of the bs 2 / 4 / 8 grouped branch (launch_bsrmm_f32): the probe's sums
    in bytes 0..15, one dirty flag per (group of 32 / bs block rows, 128-column tile)
    from byte 256."""
    mb = -(-m // bs)
    return -(-mb // (32 // bs)) * -(-n // 128) * 4 + 256


PANEL_MIN_BLOCKS = 1 << 15  # kPanelMinBlocks (bsr_kernels.hip): 32 x 32 sub-blocks from which the probe runs
PROBE64_MB, PROBE64_N = 128, 8
PROBE64_CHECKED_BLOCK_ROWS = (0, 41, 86, 127)


def panel_probe_bsr64(seed=64):
    """The smallest bs 64 matrix whose product launches panel_probe_kernel
    (4 * nnzb >= kPanelMinBlocks): 128 x 128 block rows / columns, every block row
    holding block column 0 and 63 others, all 8192 blocks fully dense (134 MB), and a
    CSR remainder of three entries per row, one of them in columns 0..3 in every
    fourth row. -> (brp, bci, bval, crp, cci, cv)."""
    rng = np.random.default_rng(seed)
    mb = PROBE64_MB
    cols = [np.concatenate([[0], 1 + np.sort(rng.choice(mb - 1, 63, replace=False))])
            for _ in range(mb)]
    brp = (64 * np.arange(mb + 1)).astype(np.int32)
    bci = np.concatenate(cols).astype(np.int32)
    bval = rng.random(bci.size * 4096, dtype=np.float32)
    bval *= 2.0
    bval -= 1.0
    m = mb * 64
    cci = rng.integers(0, m, (m, 3))
    cci[::4, 0] = rng.integers(0, 4, cci[::4, 0].size)
    cci = np.sort(cci, axis=1)
    crp = (3 * np.arange(m + 1)).astype(np.int32)
    cv = rng.uniform(-1, 1, cci.size).astype(np.float32)
    return brp, bci, bval, crp, cci.reshape(-1).astype(np.int32), cv


def probe64_block_row_reference(br, mats, Bd):
    """float64 (ref, absdot) of block row br of panel_probe_bsr64's matrix times
    Bd (8192 x n): its dense 64 x 8192 slab, BSR blocks plus CSR remainder (an entry
    both parts hold is added, as the two products add it), and the slab of absolute
    values."""
    brp, bci, bval, crp, cci, cv = mats
    k = PROBE64_MB * 64
    slab, aslab = np.zeros((64, k)), np.zeros((64, k))
    for j in range(brp[br], brp[br + 1]):
        blk = bval[j * 4096:(j + 1) * 4096].reshape(64, 64).astype(np.float64)
        slab[:, bci[j] * 64:bci[j] * 64 + 64] = blk
        aslab[:, bci[j] * 64:bci[j] * 64 + 64] = np.abs(blk)
    for r in range(64):
        row = br * 64 + r
        for j in range(crp[row], crp[row + 1]):
            slab[r, cci[j]] += float(cv[j])
            aslab[r, cci[j]] += abs(float(cv[j]))
    B64 = Bd.astype(np.float64)
    return slab @ B64, aslab @ np.abs(B64)


def rand_csr_rows(rng, m, k, deg_hi, empty_frac=0.2):
    """A random m x k CSR: 0..deg_hi sorted distinct columns per row, some rows empty,
    uniform(-1, 1) values."""
    deg = rng.integers(0, deg_hi + 1, m)
    deg[rng.random(m) < empty_frac] = 0
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    ci = (np.concatenate([np.sort(rng.choice(k, d, replace=False)) for d in deg]).astype(np.int32)
          if rp[-1] else np.zeros(0, np.int32))
    return rp, ci, rng.uniform(-1, 1, ci.size).astype(np.float32)


# ------------------------------------------------- handle reuse: step inputs
REUSE_HUB_M, REUSE_HUB_K, REUSE_HUB_NNZ = 3000, 50000, 40000
CSR_PIECE_MIN = 128  # a CSR row longer than this is cut into pieces
REUSE_SEG_SHAPE = (23, 320, 32, 136)  # mb, kb, bs, n of step d


def reuse_hub_csr(seed=2024):
    """Step a's matrix: 3000 x 50000, rows of 0..6 nonzeros (30 % empty) and one hub
    row of 40,000."""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 7, REUSE_HUB_M)
    deg[rng.random(REUSE_HUB_M) < 0.3] = 0
    rows = [np.unique(rng.integers(0, REUSE_HUB_K, d)) for d in deg]
    rows[1234] = np.sort(rng.choice(REUSE_HUB_K, REUSE_HUB_NNZ, replace=False))
    rp = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    return rp, ci, rng.uniform(-1, 1, ci.size).astype(np.float32)


def cs2_segments_splits(rowptr, ntiles, num_cus=256):
    """cs2_segments' rule (bsr_kernels.hip) restated: on a shallow grid (at most
    kLptRounds = 8 rounds of the 12 * num_cus wave slots), when the longest block row
    holds more than twice the mean load per wave slot (2 nnzb / slots blocks), the
    rows longer than L = max(64, nnzb / (2 * slots)) blocks are split. Returns the
    number of rows it splits."""
    rowptr = np.asarray(rowptr, np.int64)
    mb, nnzb = rowptr.size - 1, int(rowptr[-1])
    slots = 12 * num_cus
    if nnzb <= 0 or mb * ntiles > 8 * slots:
        return 0
    L = max(64, -(-nnzb // (2 * slots)))
    lens = np.diff(rowptr)
    if lens.max() <= 2 * -(-nnzb // slots):  # rounded up: the stricter reading
        return 0
    return int((lens > L).sum())


# ------------------------------------------- graph replay: variants of the step inputs
# (tests/test_gpu_graph_replay.py writes them over a captured step's operands, in place;
# tests/test_graph_replay_helpers.py checks on the host that each really differs)
REPLAY_STRUCTURE_STEPS, REPLAY_VALUE_STEPS = "abldef", "cghk"


def reversed_rows(rowptr, colind, val):
    """The CSR / BSR matrix with its (block) rows in reverse order: rowptr rebuilt from
    the reversed lengths (same start), colind and val (val.size / colind.size values per
    entry) concatenated row by row in reverse. Same sizes, same nnz / nnzb."""
    rowptr = np.asarray(rowptr)
    m = rowptr.size - 1
    lens = np.diff(rowptr)[::-1]
    rp = (rowptr[0] + np.concatenate([[0], np.cumsum(lens)])).astype(rowptr.dtype)
    take = (np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in range(m - 1, -1, -1)])
            if m and rowptr[-1] > rowptr[0] else np.zeros(0, np.int64)) - rowptr[0]
    per = val.size // colind.size if colind.size else 0
    return (rp, np.ascontiguousarray(colind[take]),
            np.ascontiguousarray(val.reshape(colind.size, per)[take].reshape(val.shape)))


def _like(rng, a):
    """New contents of a's shape and type from a's own distribution family: uniform(-1, 1)
    for fp32 / fp16, standard normal for fp64."""
    if a.dtype == np.float64:
        return rng.standard_normal(a.shape)
    return rng.uniform(-1, 1, a.shape).astype(np.float32).astype(a.dtype)


def graph_replay_variant(name, I):
    """Host operands that replace those of reuse step `name` (the keys of
    tests/test_gpu_handle_reuse.py's input dict I) under a captured graph: the same
    shapes, nnz / nnzb and dtypes, other contents, from a fixed seed per step.

      a, b, l, d, e, f  the matrix with its (block) rows reversed, a new B and C0
      c, g, h, k        the same structure with new values, B and C0 (a zero of a BSR
                        block stays a zero: the hybrid's parts are the divide of the
                        re-valued matrix)
      i                 a new B and C0 only (the values live in the analysis buffer)"""
    rng = np.random.default_rng(9100 + ord(name))
    new = lambda *keys: {k: _like(rng, I[k]) for k in keys}  # noqa: E731
    if name == "a":
        return {"csr": reversed_rows(*I["csr"]), **new("a_B", "a_C0")}
    if name == "b":
        return {"csr": reversed_rows(*I["csr"]), **new("b_B")}
    if name == "l":
        return {"l_csr": reversed_rows(*I["l_csr"]), **new("l_B")}
    if name == "d":
        return {"seg": reversed_rows(*I["seg"]), **new("seg_B")}
    if name == "e":
        return {"seg": reversed_rows(*I["seg"]), **new("seg_B", "seg_C0")}
    if name == "f":
        out = {}
        for sb in (8, 2):
            out[f"small{sb}"] = reversed_rows(*I[f"small{sb}"])
            out.update(new(f"small{sb}_B", f"small{sb}_C0"))
        return out
    if name == "c":
        rp, ci, v = I["csr"]
        return {"csr": (rp, ci, _like(rng, v)), **new("b_B")}
    if name == "g":
        from spmm_hip import prep
        rp, ci, v = I["hyb_A"]
        v = _like(rng, v)
        return {"hyb_A": (rp, ci, v),
                "hyb": prep.divide(HYBRID_EX_M, rp, ci, v, 32, HYBRID_EX_DENSITY[32]),
                **new("hyb_B", "hyb_C0")}
    if name == "h":
        rp, ci, v = I["h16"]
        return {"h16": (rp, ci, _like(rng, v)), **new("h16_B")}
    if name == "k":
        out = new("c64_Bt", "c64_C0t", "b64_B", "b64_C0")
        for key in ("c64", "b64"):
            rp, ci, v = I[key]
            out[key] = rp, ci, _like(rng, v)
        return out
    if name == "i":
        return new("g16_B", "g32_B", "g_C0")
    raise KeyError(name)
