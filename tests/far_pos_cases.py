"""CSR positions past 2^31 and 2^32 bytes and up to INT_MAX: the geometry, with no GPU needed.

Every CSR-family kernel forms addresses from a position p, the index into csrColInd, csrVal,
outVal, x, y, g, gx; the multi-head entries from q = p * heads + h. A position is an int. The
cases of tests/test_gpu_far_positions.py put a matrix of a few hundred (or 150,000) positions
at position 2^29, 2^30 or just under 2^31 of an uninitialised arena: every CSR entry accepts a
view (csrRowPtr[0] may exceed the base, position p is index p of the arrays as passed, entries
outside the view are left alone: include/spmm_hip.h), so only the window and
its guards are ever written or read. This is what tests/far_cases.py does for the rows of a
dense operand.

A Window is (family, bound, size): its row pointer is start + local, its colind / val are flat
arrays from position 0 on.

Families (which array's edge the bounds are counted for, in positions from its first element):
  p4   4-byte arrays of one value per position (colind, fp32 val, outVal, x, y, g, gx):
       W29 = 2^29 (2^31 bytes), W30 = 2^30 (2^32 bytes; 2^31 bytes of an fp16 val),
       TOP: rowptr[m] - base = 2^31 - 1 exactly
  p8   fp64 val: W28 = 2^28 (2^31 bytes), W29 = 2^29 (2^32 bytes), W30 = 2^30 (2^33 bytes, the
       arena's 8 GiB). No TOP: 2^31 doubles would be a 16-GiB array.
  q3 / q8
       the [nnz, heads] float arrays of the multi-head entries at heads 3 / 8, bounds counted
       in elements q = p * heads: W29 and W30 as p4's, crossed inside position bound // heads;
       TOP: rowptr[m] - base = INT_MAX // heads, the largest p with (p + 1) * heads <= INT_MAX

Sizes: "small" is 40 rows and about 500 positions (row 0 empty, row 7 the long row of 300: more
than one 128-nonzero piece, row 12 of one entry, row 20 empty, the others 0..12, the last row
of 5); "large" is 300 rows and about 150,000 positions with a hub row of 40,000 (row 101), run
with set_csr_waves_per_cu(1) so that a merge-path wave walks several 256-position chunks and
the in-place chunk reload and the split-row pieces run across the bound. In W28 / W29 / W30 the
bound falls strictly inside the long (hub) row, with rows wholly on each side. TOP comes in
two forms: "TOP" with a short last row, "TOPL" with the long row moved to the end, so that it
ends at the top position.

The kernels align their groups to absolute positions, so the window starts take different
residues mod 256 and mod 64. A W window starts at a position congruent mod 256 to RESIDUE[rank
of the bound in its family, size]:
  first bound (W29; p8: W28)   small 37, large 90    (mod 64: 37, 26)
  second bound (W30; p8: W29)  small 171, large 204  (mod 64: 43, 12)
  third bound (p8's W30)       small 249, large 3    (mod 64: 57, 3)
A TOP / TOPL window's start is its end minus the matrix's size, what INT_MAX (or INT_MAX //
heads) minus the size leaves, mod 256 (small TOP, small TOPL, large TOP, large TOPL):
  p4 and q8  19, 15, 152, 29    q3  190, 186, 67, 200
tests/test_far_pos_cases.py asserts these, and that the W starts of one
family differ mod 64 and mod 256 and that the family's starts take at least six residues.

Guards: each array holds GUARD = 1024 positions in front of the window and behind it. Behind
a TOP window no int position is left but 2^31 - 1 itself, yet the arena is 64 MiB longer than
8 GiB, so the guard behind is written and checked all the same: a store past the top, formed
in 64 bits or as an unsigned, lands in it. colind guards hold valid columns in [0, k) (the
kernels prefetch whole aligned groups and may load them: they must be harmless as indices),
input value guards the signalling-NaN sentinel of helpers.framed (consuming one shows in the
result), output guards the sentinel too and must keep its bits.

The near twin of a window is the same window and guards at position GUARD + start mod GUARD
of a small array: the residues the kernels align to are unchanged, and every entry here is
bit-reproducible, so far result == twin result bit for bit.

PosArena is far_cases.Arena at this file's size; Placed is one array's window with its guards,
inside an arena or a twin's small buffer.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import softmax_cases as sc
from far_cases import INT_TYPE, SENTINEL, SENTINEL_BF16, Arena

POS_ARENA_BYTES = (1 << 33) + (1 << 26)  # 8 GiB + 64 MiB
HOT_BYTE_OFF = 1 << 25   # colind_hot lives in colind's arena, this many bytes further on
GUARD = 1024             # positions in front of a window and behind it
P31, P32 = 1 << 31, 1 << 32
INT_MAX = P31 - 1
K = 64                   # columns of the matrix: the rows of B / Y
HEADS = (3, 8)

SMALL_M, SMALL_LONG, SMALL_LONG_LEN = 40, 7, 300
LARGE_M, LARGE_LONG, LARGE_LONG_LEN = 300, 101, 40000


@functools.lru_cache(maxsize=None)
def lens_of(size: str, long_last: bool = False) -> np.ndarray:
    """Row lengths of the "small" / "large" matrix; long_last: the long row is the last one."""
    if size == "small":
        lens = np.random.default_rng(40).integers(0, 13, SMALL_M)
        lens[[0, 12, 20, SMALL_M - 1]] = 0, 1, 0, 5
        lens[SMALL_LONG] = SMALL_LONG_LEN
        if long_last:
            lens[[SMALL_LONG, SMALL_M - 1]] = 9, SMALL_LONG_LEN
    else:
        lens = np.random.default_rng(300).integers(0, 737, LARGE_M)
        lens[[0, 33, 150, LARGE_M - 1]] = 0, 1, 0, 77
        lens[LARGE_LONG] = LARGE_LONG_LEN
        if long_last:
            lens[[LARGE_LONG, LARGE_M - 1]] = 200, LARGE_LONG_LEN
    lens = lens.astype(np.int64)
    lens.setflags(write=False)
    return lens


# element bytes and heads of the array a family's bounds are counted for, and its bounds in
# elements of that array
FAMILY = {
    "p4": dict(elem=4, heads=1, bounds={"W29": 1 << 29, "W30": 1 << 30}, top=INT_MAX),
    "p8": dict(elem=8, heads=1, bounds={"W28": 1 << 28, "W29": 1 << 29, "W30": 1 << 30}, top=None),
    "q3": dict(elem=4, heads=3, bounds={"W29": 1 << 29, "W30": 1 << 30}, top=INT_MAX // 3),
    "q8": dict(elem=4, heads=8, bounds={"W29": 1 << 29, "W30": 1 << 30}, top=INT_MAX // 8),
}
# start mod 256 of a W window, by (rank of the bound in its family, size)
RESIDUE = {(0, "small"): 37, (0, "large"): 90, (1, "small"): 171, (1, "large"): 204,
           (2, "small"): 249, (2, "large"): 3}


@dataclass(frozen=True)
class Window:
    family: str
    bound: str           # "W28" | "W29" | "W30" | "TOP" | "TOPL"
    size: str            # "small" | "large"
    start: int           # position of the matrix's first entry
    long_last: bool

    @property
    def name(self) -> str:
        return f"{self.family}-{self.bound}-{self.size}"

    @property
    def heads(self) -> int:
        return FAMILY[self.family]["heads"]

    @property
    def elem(self) -> int:
        return FAMILY[self.family]["elem"]

    @property
    def lens(self) -> np.ndarray:
        return lens_of(self.size, self.long_last)

    @property
    def local(self) -> np.ndarray:
        """The local row pointer, int64: 0 .. nnz."""
        return np.concatenate([[0], np.cumsum(self.lens)])

    @property
    def m(self) -> int:
        return self.lens.size

    @property
    def nnz(self) -> int:
        return int(self.lens.sum())

    @property
    def end(self) -> int:
        """rowptr[m] - base: one past the last position, the nnz argument of a far call."""
        return self.start + self.nnz

    @property
    def long_row(self) -> int:
        return int(np.argmax(self.lens))

    @property
    def base(self) -> int:
        """The index base a case on this window runs at: 1 on the first W bound of a family
        (a TOP window's rowptr[m] is INT_MAX already at base 0)."""
        fam = FAMILY[self.family]
        return int(self.bound == next(iter(fam["bounds"])))

    def crossing(self):
        """(position, bound in elements, row) of the claimed crossing: the elements of the
        position before lie below the bound, the position holds an element at or past it and
        lies strictly inside `row`; None for TOP / TOPL."""
        fam = FAMILY[self.family]
        if self.bound not in fam["bounds"]:
            return None
        b = fam["bounds"][self.bound]
        return b // fam["heads"], b, self.long_row

    def twin_start(self) -> int:
        return GUARD + self.start % GUARD

    def rowptr(self, near: bool = False) -> np.ndarray:
        rp = (self.twin_start() if near else self.start) + self.local + self.base
        assert rp[-1] <= INT_MAX
        return rp.astype(np.int32)


def _make(family: str, bound: str, size: str) -> Window:
    fam = FAMILY[family]
    if bound in ("TOP", "TOPL"):
        long_last = bound == "TOPL"
        return Window(family, bound, size, fam["top"] - int(lens_of(size, long_last).sum()),
                      long_last)
    lens = lens_of(size)
    long_row = int(np.argmax(lens))
    hub_off = int(lens[:long_row].sum())
    pc = fam["bounds"][bound] // fam["heads"]  # the position that holds element `bound`
    rank = list(fam["bounds"]).index(bound)
    s0 = pc - hub_off - 20                      # the bound 20 positions into the long row
    start = s0 - (s0 - RESIDUE[rank, size]) % 256
    assert 20 <= pc - hub_off - start < 276 < int(lens[long_row])
    return Window(family, bound, size, start, False)


WINDOWS = [_make(f, b, s) for f in FAMILY for b in list(FAMILY[f]["bounds"]) +
           (["TOP", "TOPL"] if FAMILY[f]["top"] else []) for s in ("small", "large")]
BY_NAME = {w.name: w for w in WINDOWS}


def windows(family: str, sizes=("small", "large")) -> list:
    return [w for w in WINDOWS if w.family == family and w.size in sizes]


def ids(ws) -> list:
    return [w.name for w in ws]


# ------------------------------------------------------------------------------ matrices
@functools.lru_cache(maxsize=None)
def colind_of(size: str, long_last: bool) -> np.ndarray:
    """0-based columns in [0, K), drawn with repetition and sorted inside every row; every
    column is used."""
    rng = np.random.default_rng(7 + (size == "large") + 2 * long_last)
    ci = np.concatenate([np.sort(rng.integers(0, K, int(l))) for l in lens_of(size, long_last)])
    assert np.unique(ci).size == K
    ci = ci.astype(np.int32)
    ci.setflags(write=False)
    return ci


HOT_ROWS = 20  # the hot budget of the hot-column cases, in B rows


def hot_bytes(n: int) -> int:
    """The hotBytes that spmm_csr_hot_analysis (csrc/api.cpp) turns into HOT_ROWS rows at n
    columns: a row's gathered piece is the merge-path column tile, or the row when narrower."""
    tile = 256 if n > 128 else 128 if n > 64 else 64
    return HOT_ROWS * 4 * (n if 0 < n < tile else tile)


def hot_columns(ci: np.ndarray, k: int) -> np.ndarray:
    """The analysis' rule restated (csrc/csr_kernels.hip): the count threshold is the smallest
    t at which at most HOT_ROWS columns have min(count, 8191) >= t; those columns are hot.
    Returns the mask over the k columns."""
    c = np.minimum(np.bincount(ci, minlength=k), 8191)
    thr = next(t for t in range(8193) if int((c >= t).sum()) <= HOT_ROWS)
    return c >= thr


def colind_guards(seed: int):
    """(front, back): GUARD valid 0-based columns each."""
    rng = np.random.default_rng(1000 + seed)
    return rng.integers(0, K, GUARD).astype(np.int32), rng.integers(0, K, GUARD).astype(np.int32)


def sentinel_bits(elem: int, bf16: bool = False) -> int:
    return SENTINEL_BF16 if bf16 else SENTINEL[elem]


def with_guards(data: np.ndarray, per: int = 1, front=None, back=None, bf16: bool = False):
    """The integer-typed host image [front guard | data | back guard] of an array of `per`
    elements per position: the guards hold the sentinel of the element's width unless given."""
    data = np.ascontiguousarray(data).reshape(-1)
    it = INT_TYPE[data.dtype.itemsize]
    fill = np.array([sentinel_bits(data.dtype.itemsize, bf16)], "u%d" % data.dtype.itemsize)
    parts = []
    for g in (front, back):
        parts.append(np.full(GUARD * per, fill.view(it)[0], it) if g is None
                     else np.ascontiguousarray(g).view(it))
        assert parts[-1].size == GUARD * per
    return np.concatenate([parts[0], data.view(it), parts[1]])


# --------------------------------------------------- the softmax rule on any pattern
def softmax_fwd_rule(local, x):
    """softmax_cases.forward_bits on any pattern: exp_rule and row_sum per row."""
    y = np.zeros_like(x)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for a, b in zip(local[:-1], local[1:]):
            if b > a:
                e = sc.exp_rule(x[a:b] - np.fmax.reduce(x[a:b]))
                y[a:b] = e / sc.row_sum(e)
    return y


def softmax_bwd_rule(local, y, g):
    gx = np.zeros_like(y)
    with np.errstate(invalid="ignore", over="ignore"):
        for a, b in zip(local[:-1], local[1:]):
            if b > a:
                diff = g[a:b] - sc.row_sum(y[a:b], g[a:b])
                gx[a:b] = y[a:b] * diff
    return gx


# ------------------------------------------------------------------- arenas and placements
class Placed:
    """One array's window with its guards, inside `buf` (an arena's bytes, or a twin's small
    buffer): host is the integer image as placed, `first` the array element host[0] sits at,
    the array itself starting byte_off bytes into buf."""

    def __init__(self, buf, host: np.ndarray, first: int, per: int, byte_off: int = 0):
        import torch
        self.host, self.first, self.per = host, first, per
        elem = host.dtype.itemsize
        assert byte_off % 256 == 0 and first >= 0
        assert byte_off + (first + host.size) * elem <= buf.numel(), "outside the buffer"
        self._bytes = buf[byte_off:]
        ints = self._bytes.view(getattr(torch, host.dtype.name))
        self._win = ints[first:first + host.size]
        self._win.copy_(torch.from_numpy(host).to(buf.device))

    def tensor(self, dtype, end: int):
        """The flat array from its first element to position `end` (exclusive), as passed to a
        wrapper: its numel() is the call's nnz (times heads)."""
        t = self._bytes.view(dtype)[:end * self.per]
        assert t.data_ptr() == self._bytes.data_ptr()
        return t

    def window(self, dtype):
        """The window alone (pointers at the window's start)."""
        g = GUARD * self.per
        return self._bytes.view(dtype)[self.first + g:self.first + self.host.size - g]

    def read(self, what: str = "") -> np.ndarray:
        """The window's data (integer view) as a call left it, after asserting that both
        guards kept their bits."""
        got = self._win.cpu().numpy()
        g = GUARD * self.per
        for nm, sl in (("in front of", slice(0, g)), ("behind", slice(-g, None))):
            bad = np.flatnonzero(got[sl] != self.host[sl])
            assert not bad.size, (f"{what}: the guard {nm} the window changed at element "
                                  f"{int(bad[0])} of {g}")
        return got[g:-g].copy()

    def unchanged(self, what: str = ""):
        g = GUARD * self.per
        bad = np.flatnonzero(self.read(what) != self.host[g:-g])
        assert not bad.size, f"{what}: an input array changed at window element {int(bad[0])}"


class PosArena(Arena):
    """far_cases.Arena at POS_ARENA_BYTES: one uninitialised device allocation in which only
    windows and guards are ever written. place() (a far dense operand, the hot-column case's
    B) checks its rows against this size."""
    BYTES = POS_ARENA_BYTES


def place(buf, w: Window, near: bool, host: np.ndarray, per: int = 1, byte_off: int = 0) -> Placed:
    """host (with_guards) at window w's positions of buf, or at its twin's."""
    start = w.twin_start() if near else w.start
    return Placed(buf, host, (start - GUARD) * per, per, byte_off)


def twin_bytes(w: Window, elem: int, per: int = 1) -> int:
    """Bytes of a near twin's buffer for an array of `per` elements of `elem` bytes."""
    return (w.twin_start() + w.nnz + GUARD) * per * elem


def last_byte(w: Window, elem: int, per: int = 1, byte_off: int = 0) -> int:
    """One past the last arena byte the far placement of such an array touches."""
    return byte_off + (w.end + GUARD) * per * elem


# ------------------------------------------------------------------------------ wraps
def wraps(w: Window, elem: int, per: int = 1):
    """For the window's positions whose byte offset (elem * per bytes a position) no longer
    fits 31 / 32 bits: the positions a 32-bit wrap of that offset would address instead, as
    (sign-extended, unsigned) int64 arrays of element-granular positions (floor division)."""
    p = np.arange(w.start, w.end, dtype=np.int64)
    b = p * (elem * per)
    lo = b & (P32 - 1)
    signed = np.where(lo >= P31, lo - P32, lo)
    return (signed[b >= P31] // (elem * per)), (lo[b >= P32] // (elem * per))
