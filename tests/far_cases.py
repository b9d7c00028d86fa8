"""Dense operands whose rows lie past 2^31 and 2^32: the geometry, with no GPU needed.

Every product kernel addresses a dense operand as row * ld + column, and the fast paths
keep part of that sum in 32 bits behind hand-written launcher bounds. The cases of
tests/test_gpu_far_offsets.py put exactly one operand of a call (B, C, X, Y, out) so far
apart that those sums pass 2^31 and 2^32 bytes, and 2^31 elements, while the matrices stay
tiny: the far operand is a strided view into one uninitialised arena (Arena below) of which
only the rows and columns a case uses are ever written or read.

A Geometry is (element size, leading dimension in elements, rows used, the crossings it
claims). Offsets are counted from the operand's first element, which is what a kernel's
arithmetic sees; the operand starts FAR_BASE bytes into the arena, so that the sentinel
guard in front of row 0 lies inside it. Each ld is an exact power of two unless the case is
the last value on one side of a launcher bound: a 32-bit wrap of a byte or element offset
then lands on another row that the case also holds and checks, not on memory nobody looks
at. A crossing (row, unit, bound) says: row `row` starts at or past `bound` (bytes "B",
elements "E") and the row before it starts below. tests/test_far_cases.py checks every claim
in Python integers.

  f32          4 B, ld 2^28, rows 0..8: row 2 at 2^31 B, row 4 at 2^32 B, row 8 at 2^31 elements
  h16          2 B (fp16, bf16), ld 2^28, rows 0..8: row 4 at 2^31 B, row 8 at 2^32 B and 2^31
               elements
  f64          8 B, ld 2^27, rows 0..8: row 2 at 2^31 B, row 4 at 2^32 B (2^31 elements would
               need a 16-GiB operand: out of this arena's reach)
  bs32_narrow  4 B, ld 2^24 - 4, 160 rows (kb = 5): the last ld with O32 = true; panel offsets
               reach 31 ld 4 + 4 n, just under 2^31. Row 33 passes 2^31 B, row 65 2^32 B and
               row 129 2^31 elements (rows 32, 64 and 128 start 512 bytes / elements short
               of them, ld being 4 short of 2^24)
  bs32_wide    4 B, ld 2^25, 96 rows (kb = 3): O32 = false; row 16 at 2^31 B, row 32 at 2^32 B,
               rows 64..95 past 2^31 elements
  bs16_f       4 B, ld 2^26, 48 rows (kb = 3): row 8 at 2^31 B, row 16 at 2^32 B, row 32 at
               2^31 elements (32 rows of 2^27 floats would be 16 GiB, past the arena)
  bs16_h       2 B, ld 2^27, 32 rows (kb = 2): row 8 at 2^31 B, row 16 at 2^32 B and 2^31
               elements
  small_in(bs) / small_out(bs)
               4 B, ld 2^29 / bs - 2 and 2^29 / bs, bs kb rows with kb = ceil(10 / bs) + 1: the
               last ld inside and the first outside ld bs 4 < 2^31 (bs 2, 4, 8)
  hot_in / hot_out
               4 B, ld 2^20, k + base = 1023 / 1024 rows: the last and the first extent around
               hot_mode's 2^32; rows from 512 on have a row offset (soffset) >= 2^31

Column-major far operands use f32, h16 and f64 with the operand's columns in the part of the
rows: n = 9 or 12 columns at ld 2^28 (2^27 for fp64).

The three launcher predicates are restated here (hot_mode of csrc/api.cpp, panels_in_31_bits
and the ld term of small_grouped_ok of csrc/bsr_kernels.hip); side() gives for a geometry
the side of its switch a case must land on (HOT 0 / 1 / 2, O32, small path), and the GPU
cases take their expectation from it alone.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

ARENA_BYTES = 3 * (1 << 32) + (1 << 26)  # 12 GiB + 64 MiB
FAR_BASE = 512   # bytes from the arena's start to a far operand's first element
GUARD = 64       # sentinel elements before and after the n columns of every used row
P31, P32 = 1 << 31, 1 << 32
N_MAX = 136      # the widest row any case uses


@dataclass(frozen=True)
class Geometry:
    name: str
    elem: int            # bytes per element
    ld: int              # elements
    rows: int            # rows 0 .. rows - 1 are used
    crossings: tuple     # (row, "B" | "E", bound)
    ld_mod: int = 1      # what the kernel family's fast path asks of ld
    base_mod: int = 16   # ... and of the operand's address (bytes)
    bs: int = 0          # the block size a small_in / small_out geometry belongs to

    def start(self, row: int, unit: str = "B") -> int:
        """Offset of row `row` from the operand's first element."""
        return row * self.ld * (self.elem if unit == "B" else 1)

    def last_byte(self, n: int = N_MAX, off: int = 0) -> int:
        """One past the last arena byte a case of n columns touches (the back guard of the
        last row), the operand starting `off` elements past FAR_BASE."""
        return FAR_BASE + (off + self.start(self.rows - 1, "E") + n + GUARD) * self.elem


# ------------------------------------------------------ the launcher predicates, restated
def hot_mode(k: int, base: int, ld: int, n: int, hot: bool = True) -> int:
    """csrc/api.cpp hot_mode: 2 = one buffer resource for all of B, the row offset in
    soffset; 1 = a resource per row; 0 = no tagged indices."""
    if not hot:
        return 0
    return 2 if ((k + base) * ld + n) * 4 + 64 < P32 else 1


def panels_in_31_bits(ldb: int) -> bool:
    """csrc/bsr_kernels.hip: the O32 argument of bsr32_f32_cs2_kernel."""
    return ldb * 128 < P31


def small_grouped_ld_ok(ldb: int, bs: int) -> bool:
    """The leading-dimension term of small_grouped_ok (csrc/bsr_kernels.hip): the grouped
    bs 2 / 4 / 8 stream builds a buffer resource of bs * ldb * 4 bytes per step."""
    return ldb * bs * 4 < P31


# ------------------------------------------------------------------------- geometries
F32 = Geometry("f32", 4, 1 << 28, 9, ((2, "B", P31), (4, "B", P32), (8, "E", P31)), ld_mod=4)
H16 = Geometry("h16", 2, 1 << 28, 9, ((4, "B", P31), (8, "B", P32), (8, "E", P31)), ld_mod=8)
F64 = Geometry("f64", 8, 1 << 27, 9, ((2, "B", P31), (4, "B", P32)))
BS32_NARROW = Geometry("bs32_narrow", 4, (1 << 24) - 4, 160,
                       ((33, "B", P31), (65, "B", P32), (129, "E", P31)), ld_mod=4)
BS32_WIDE = Geometry("bs32_wide", 4, 1 << 25, 96,
                     ((16, "B", P31), (32, "B", P32), (64, "E", P31)), ld_mod=4)
BS16_F = Geometry("bs16_f", 4, 1 << 26, 48, ((8, "B", P31), (16, "B", P32), (32, "E", P31)),
                  ld_mod=4)
BS16_H = Geometry("bs16_h", 2, 1 << 27, 32, ((8, "B", P31), (16, "B", P32), (16, "E", P31)),
                  ld_mod=8)
SMALL_BS = (2, 4, 8)


def small_kb(bs: int) -> int:
    return -(-10 // bs) + 1


def small_in(bs: int) -> Geometry:
    """The last ld inside ld * bs * 4 < 2^31: block column 1 ends 8 bs bytes short of 2^31,
    so row bs + 1 is the first past it."""
    rows = bs * small_kb(bs)
    cross = [(bs + 1, "B", P31), (2 * bs + 1, "B", P32)]
    if 4 * bs + 1 < rows:
        cross.append((4 * bs + 1, "E", P31))
    return Geometry(f"small_in{bs}", 4, (1 << 29) // bs - 2, rows, tuple(cross), ld_mod=2,
                    base_mod=8, bs=bs)


def small_out(bs: int) -> Geometry:
    """The first ld outside: block column 1 starts at 2^31 bytes exactly."""
    rows = bs * small_kb(bs)
    cross = [(bs, "B", P31), (2 * bs, "B", P32)]
    if 4 * bs < rows:
        cross.append((4 * bs, "E", P31))
    return Geometry(f"small_out{bs}", 4, (1 << 29) // bs, rows, tuple(cross), ld_mod=2,
                    base_mod=8, bs=bs)


HOT_LD = 1 << 20
HOT_IN = Geometry("hot_in", 4, HOT_LD, 1023, ((512, "B", P31),), ld_mod=4)
HOT_OUT = Geometry("hot_out", 4, HOT_LD, 1024, ((512, "B", P31),), ld_mod=4)
HOT_N = (65, 66, 132)


def hot_k(g: Geometry, base: int) -> int:
    """k of a hot case: with base 1 one less, so that k + base is the geometry's extent."""
    return g.rows - base


def hot_rows(k: int) -> tuple:
    """The B rows a hot case's colind uses."""
    return (0, 511, 512, k - 2, k - 1)


GEOMETRIES = ([F32, H16, F64, BS32_NARROW, BS32_WIDE, BS16_F, BS16_H, HOT_IN, HOT_OUT] +
              [f(bs) for bs in SMALL_BS for f in (small_in, small_out)])
BY_NAME = {g.name: g for g in GEOMETRIES}


def side(g: Geometry, n: int = N_MAX, base: int = 0) -> dict:
    """The side of its launcher switch a case on g must land on: {"o32": bool} for the bs 32 /
    64 streams, {"small": 1 | 0} for bs 2 / 4 / 8 under SPMM_BSR_SMALL_GROUPED (1: the
    grouped stream is launched), {"hot": 2 | 1} for the hot-column entry."""
    if g.name.startswith("bs32"):
        return {"o32": panels_in_31_bits(g.ld)}
    if g.name.startswith("small"):
        return {"small": int(small_grouped_ld_ok(g.ld, g.bs))}
    if g.name.startswith("hot"):
        return {"hot": hot_mode(hot_k(g, base), base, g.ld, n)}
    return {}


def c_geometry(rows: int) -> Geometry:
    """The geometry of a far row-major fp32 output of `rows` rows: the largest ld whose rows
    fit the arena (2^28 up to 13 rows, 2^26 up to 49, 2^25 up to 97: the 64 MiB past 12 GiB
    hold the columns of one more row)."""
    for g in (F32, BS16_F, BS32_WIDE):
        if (rows - 1) * g.ld * 4 + FAR_BASE + (N_MAX + GUARD) * 4 <= ARENA_BYTES:
            return g
    raise AssertionError(rows)


def c_crossed(rows: int) -> tuple:
    """(2^31 bytes, 2^32 bytes, 2^31 elements): which of them the last of `rows` rows of
    c_geometry(rows) starts at or past."""
    g = c_geometry(rows)
    return (g.start(rows - 1) >= P31, g.start(rows - 1) >= P32, g.start(rows - 1, "E") >= P31)


# ------------------------------------------------------------------------------ matrices
def far_csr(rng, m: int, k: int, long_row: int = 7, long_len: int = 300, deg: int = 12,
            last_empty: bool = True):
    """An m x k CSR for a dense operand of few rows: row 0 empty, row m - 1 empty too or, with
    last_empty=False, holding deg entries (where the rows of a far C are the matrix's, so that
    its last row, the one furthest out, receives a product and not beta * C alone), row
    `long_row` holding long_len entries (more than one 128-nonzero piece), the others
    0 .. deg; columns drawn with repetition (k is smaller than a row) and sorted, every column
    used, values uniform(-1, 1)."""
    lens = rng.integers(0, deg + 1, m)
    lens[[0, m - 1]] = 0, (0 if last_empty else deg)
    if m > 2:
        lens[min(long_row, m - 2)] = long_len
    rows = [np.sort(rng.integers(0, k, l)) for l in lens]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    assert np.unique(ci).size == k, "a column of the far operand is never referenced"
    return rp, ci, rng.uniform(-1, 1, ci.size).astype(np.float32)


HOT_COUNTS = (60, 50, 120, 1, 200)  # uses of hot_rows(k), in that order


def hot_csr(rng, k: int, m: int = 70):
    """rowptr, colind (0-based, over hot_rows(k)), val: rows 0 and m - 1 empty, row 7 holding
    150 entries, column k - 1 used 200 times and 512 120 times (the two a hot budget of two
    rows tags), 0 and 511 60 and 50 times, k - 2 once."""
    cols = np.repeat(np.array(hot_rows(k)), HOT_COUNTS)
    rng.shuffle(cols)
    lens = np.zeros(m, np.int64)
    lens[7] = 150
    rest = cols.size - 150
    other = [r for r in range(1, m - 1) if r != 7]
    cut = np.sort(rng.integers(0, rest + 1, len(other) - 1))
    lens[other] = np.diff(np.concatenate([[0], cut, [rest]]))
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.concatenate([np.sort(cols[rp[i]:rp[i + 1]]) for i in range(m)]).astype(np.int32)
    return rp, ci, rng.uniform(-1, 1, ci.size).astype(np.float32)


def far_bsr(rng, mb: int, kb: int, bs: int, full_row: int = 2):
    """helpers.rand_bsr at fill 0.5 with block row 1 empty, block row `full_row` and the
    last one holding every block column: every block column is used by two block rows or more
    (mb = 1: by the one)."""
    from helpers import rand_bsr
    rp, ci, _ = rand_bsr(rng, mb, kb, bs, 0.5, empty_rows=(1,))
    rows = [ci[rp[i]:rp[i + 1]] for i in range(mb)]
    rows[min(full_row, mb - 1)] = np.arange(kb, dtype=np.int32)
    rows[mb - 1] = np.arange(kb, dtype=np.int32)
    if mb < 4:  # too few block rows to leave the second use of a column to chance
        rows[0] = np.arange(kb, dtype=np.int32)
    rp = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    assert np.bincount(ci, minlength=kb).min() >= min(2, mb)
    return rp, ci, rng.uniform(-1, 1, ci.size * bs * bs).astype(np.float32)


# ----------------------------------------------------------------------------- the arena
_INT = {2: np.int16, 4: np.int32, 8: np.int64}
# signalling NaNs with a payload, as helpers.framed's (a copy keeps the bits, arithmetic on a
# guard word does not): helpers' own for fp16 / fp32 / fp64, and one for bfloat16
_SENTINEL = {2: 0x7C2A, 4: 0x7F80BEEF, 8: 0x7FF00000DEADBEEF}
_SENTINEL_BF16 = 0x7FA5
INT_TYPE, SENTINEL, SENTINEL_BF16 = _INT, _SENTINEL, _SENTINEL_BF16  # for tests/far_pos_cases.py


class FarOperand:
    """A rows x n operand inside the arena at leading dimension ld: `view` is the flat
    tensor from its first element on (what a caller passes as B, C, X, Y or out)."""

    def __init__(self, view, windows, host, dt):
        self.view, self._windows, self._host, self._dt = view, windows, host, dt

    def _read(self):
        return np.concatenate([w.cpu().numpy() for w in self._windows])

    def __call__(self, what=""):
        """The rows x n data as the call left it, after asserting that the GUARD elements
        before and after every row kept the sentinel's bits."""
        got = self._read()
        for nm, sl in (("before", slice(0, GUARD)), ("after", slice(-GUARD, None))):
            bad = np.argwhere(got[:, sl] != self._host[:, sl])
            assert not bad.size, (f"{what}: the guard {nm} row {int(bad[0][0])} changed at "
                                  f"element {int(bad[0][1])}")
        return got[:, GUARD:-GUARD].copy().view(self._dt)

    def unchanged(self, what=""):
        assert np.array_equal(self(what).view(self._host.dtype), self._host[:, GUARD:-GUARD]), \
            f"{what}: an input operand changed"


class Arena:
    """One uninitialised device allocation of BYTES (ARENA_BYTES; a subclass may set its own).
    place() writes the used rows of an operand (and their guards) with one strided copy (one
    per row where `rows` names the rows of a sparser choice); nothing initialises the rest."""
    BYTES = ARENA_BYTES

    def __init__(self):
        import torch
        self.buf = torch.empty(self.BYTES, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0

    def close(self):
        import torch
        self.buf = None
        torch.cuda.empty_cache()

    def place(self, data2d, ld: int, *, off: int = 0, dtype=None, rows=None) -> FarOperand:
        """data2d: host array of the operand's used rows x n (uint16 patterns with
        dtype=torch.bfloat16). rows: the operand's row of each row of data2d (default 0, 1,
        ...). off: elements the operand starts past FAR_BASE. The copies go through integer
        views of the element's width, so every bit arrives as given."""
        import torch
        data2d = np.ascontiguousarray(data2d)
        nrows, n = data2d.shape
        elem = data2d.dtype.itemsize
        it = _INT[elem]
        first = FAR_BASE // elem + off
        last_row = nrows - 1 if rows is None else int(max(rows))
        assert ld >= n + 2 * GUARD and first >= GUARD
        assert (first + last_row * ld + n + GUARD) * elem <= self.BYTES, "outside the arena"
        host = np.empty((nrows, n + 2 * GUARD), it)
        bits = _SENTINEL_BF16 if dtype is torch.bfloat16 else _SENTINEL[elem]
        host[:] = np.array([bits], "u%d" % elem).view(it)[0]
        host[:, GUARD:GUARD + n] = data2d.view(it)
        ints = self.buf.view(getattr(torch, np.dtype(it).name))
        dev = torch.from_numpy(host).to("cuda")
        if rows is None:
            windows = [ints.as_strided((nrows, n + 2 * GUARD), (ld, 1), first - GUARD)]
            windows[0].copy_(dev)
        else:
            windows = [ints.as_strided((1, n + 2 * GUARD), (ld, 1), first - GUARD + int(r) * ld)
                       for r in rows]
            for i, w in enumerate(windows):
                w.copy_(dev[i:i + 1])
        tdt = dtype if dtype is not None else getattr(torch, data2d.dtype.name)
        view = self.buf.view(tdt)[first:]
        assert view.data_ptr() == self.buf.data_ptr() + first * elem
        return FarOperand(view, windows, host, data2d.dtype)
