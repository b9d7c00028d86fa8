"""Patterns, values and numpy references shared by the edge softmax's tests (host and
device). The references are numpy alone, never the code under test: float64 for the
tolerance, and an independent restatement of the rule (include/spmm_hip.h, DESIGN.md
§4i: EXP, SUM, the backward's chains) for the bits, with sddmm_cases.fma32 as the exact
fp32 FMA. Everything is cached: treat what comes back as read-only."""
from __future__ import annotations

import functools

import numpy as np

from sddmm_cases import bits, fma32

PIECE, CHAINS, CUT = 1024, 64, -64.0
F = np.float32

# the smallest lengths at which the rule or the mapping can go wrong: empty, tiny, the
# lane-group boundaries, one piece / two, several pieces, and one hub row (many pieces
# per wave); empty rows first, last and in runs
LENGTHS = [0, 0, 1, 2, 3, 0, 0, 0, 63, 64, 65, 1023, 1024, 1025, 0, 2049, 4099, 70001, 0, 0]
SPECIAL_LENGTHS = [1, 2, 3, 5, 64, 65, 130, 1025, 2049, 7, 1, 4, 70, 1100, 9, 33]


def _rowptr(lengths, start=0):
    return np.concatenate([[start], start + np.cumsum(lengths)]).astype(np.int32)


def _pattern(name):
    """(rowptr, base, length of the value arrays)."""
    rng = np.random.default_rng(11)
    if name == "lengths":
        rp = _rowptr(LENGTHS)
    elif name == "short3000":  # many rows share a wave
        rp = _rowptr(rng.poisson(7, 3000))
    elif name == "short_mixed":  # the narrowest lane group on rows of more than 64 positions
        ln = rng.poisson(6, 3000)
        ln[[5, 1500, 2999]] = [65, 1024, 1025]
        rp = _rowptr(ln)
    elif name == "mid":  # the middle lane group, with its own boundary and long rows
        ln = rng.integers(0, 61, 300)
        ln[[0, 7, 100, 150, 200, 299]] = [1025, 63, 64, 65, 1023, 1024]
        rp = _rowptr(ln)
    elif name == "m1":
        rp = _rowptr([5])
    elif name == "m1_long":
        rp = _rowptr([3000])
    elif name == "nnz0":
        rp = _rowptr([0, 0, 0, 0])
    elif name == "view":  # rowptr[0] > 0 and rowptr[m] < nnz
        rp = _rowptr(rng.integers(0, 40, 50), start=37)
        return rp, 0, int(rp[-1]) + 29
    elif name == "base1":
        rp = _rowptr([3, 0, 64, 1, 100, 1030, 0], start=1)
        return rp, 1, int(rp[-1]) - 1
    elif name == "special":
        rp = _rowptr(SPECIAL_LENGTHS)
    else:
        raise KeyError(name)
    return rp, 0, int(rp[-1])


# name -> (pattern, values)
CASES = {
    "lengths": ("lengths", "normal"),
    "lengths_equal": ("lengths", "equal"),
    "lengths_big": ("lengths", "big"),
    "short3000": ("short3000", "normal"),
    "short_mixed": ("short_mixed", "normal"),
    "mid": ("mid", "normal"),
    "m1": ("m1", "normal"),
    "m1_long": ("m1_long", "normal"),
    "nnz0": ("nnz0", "normal"),
    "view": ("view", "normal"),
    "base1": ("base1", "normal"),
    "special": ("special", "special"),
}
NAMES = list(CASES)


class Case:
    def __init__(self, name):
        pat, kind = CASES[name]
        self.name = name
        self.rowptr, self.base, self.nnz = _pattern(pat)
        self.m = self.rowptr.size - 1
        rp = self.rowptr.astype(np.int64) - self.base
        self.starts, self.lens = rp[:-1], np.diff(rp)
        self.p0, self.p1 = int(rp[0]), int(rp[-1])
        rng = np.random.default_rng(3)
        x = rng.normal(0, 3, self.nnz).astype(F)
        special = np.zeros(self.m, bool)
        if kind == "equal":
            x[:] = F(2.5)
        elif kind == "big":  # the terms of the smaller ones are cut to +0
            x = np.where(rng.integers(0, 2, self.nnz) == 1, F(1e30), F(-1e30)).astype(F)
        elif kind == "special":
            for r in range(self.m):
                a, L = int(self.starts[r]), int(self.lens[r])
                what = r % 4
                if what == 0:  # a -inf beside finite values (alone in a row of one)
                    x[a + L // 2] = -np.inf
                elif what == 1:
                    x[a + L - 1] = np.nan
                elif what == 2:
                    x[a] = np.inf
                else:
                    x[a:a + L] = -np.inf
                special[r] = True
        self.x = x
        self.special = special  # rows that hold a non-finite value
        self.g = rng.normal(0, 1, self.nnz).astype(F)
        for a in (self.rowptr, self.x, self.g, self.special):
            a.setflags(write=False)

    def rows(self):
        """(row, start, length) of every non-empty row."""
        return [(r, int(self.starts[r]), int(self.lens[r])) for r in range(self.m)
                if self.lens[r] > 0]

    def has_long_row(self):
        return bool((self.lens > PIECE).any())

    def group_lanes(self):
        """The device's lane-group width: by the mean row length (softmax_kernels.hip)."""
        mean = -(-self.nnz // self.m)
        return 4 if mean <= 8 else 16 if mean <= 48 else 64

    def depth(self, L):
        """D: the additions on the longest path of the SUM of a row of L positions."""
        return -(-min(L, PIECE) // CHAINS) + 6 + -(-L // PIECE)


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    return Case(name)


# ------------------------------------------------------------------ the rule, restated
def exp_rule(t):
    """EXP of the rule on a float32 array (t <= 0 or NaN)."""
    t = np.asarray(t, F)
    inside = t >= F(CUT)  # False for NaN
    tc = np.where(inside, t, F(0))
    kf = np.rint(tc * F(1.44269504088896341))
    assert kf.dtype == F
    r = fma32(kf, np.full_like(tc, F(-0.693145751953125)), tc)
    r = fma32(kf, np.full_like(tc, F(-1.42860682030941723e-6)), r)
    p = np.full_like(tc, F(1.98412698412698413e-4))
    for c in (1.38888888888888889e-3, 8.33333333333333333e-3, 4.16666666666666667e-2,
              1.66666666666666667e-1, 0.5, 1.0, 1.0):
        p = fma32(p, r, np.full_like(tc, F(c)))
    e = (p.view(np.int32) + kf.astype(np.int32) * np.int32(1 << 23)).view(F)
    return np.where(inside, e, np.where(np.isnan(t), t, F(0))).astype(F)


def _fold(acc):
    """Pairwise over adjacent chains, level by level; acc: (..., 64) float32."""
    while acc.shape[-1] > 1:
        acc = acc[..., 0::2] + acc[..., 1::2]
    return acc[..., 0]


def row_sum(a, b=None):
    """SUM of the rule over one row: of the terms a (b is None), or of a * b by FMA chains."""
    L = a.size
    npieces = -(-L // PIECE)
    pad = npieces * PIECE - L

    def shaped(v):  # [piece, step, chain]
        return np.concatenate([v, np.zeros(pad, F)]).reshape(npieces, PIECE // CHAINS, CHAINS)

    A = shaped(a)
    B = None if b is None else shaped(b)
    acc = np.zeros((npieces, CHAINS), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(min(PIECE // CHAINS, -(-L // CHAINS))):
            acc = acc + A[:, i] if B is None else fma32(A[:, i], B[:, i], acc)
        pieces = _fold(acc)
        s = F(0)
        for v in pieces:
            s = F(s + v)
    return s


@functools.lru_cache(maxsize=None)
def forward_bits(name):
    """y by the restated rule; positions outside the pattern hold NaN."""
    c = case(name)
    y = np.full(c.nnz, np.nan, F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for _, a, L in c.rows():
            xr = c.x[a:a + L]
            mx = F(-np.inf)
            if not np.isnan(xr).all():
                mx = np.fmax.reduce(xr)  # a NaN operand is dropped
            e = exp_rule(xr - mx)
            y[a:a + L] = e / row_sum(e)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def backward_bits(name):
    """gx by the restated rule from y = forward_bits and the case's g."""
    c = case(name)
    y = forward_bits(name)
    gx = np.full(c.nnz, np.nan, F)
    with np.errstate(invalid="ignore", over="ignore"):
        for _, a, L in c.rows():
            yr, gr = y[a:a + L], c.g[a:a + L]
            d = row_sum(yr, gr)
            diff = gr - d
            gx[a:a + L] = yr * diff
    gx.setflags(write=False)
    return gx


@functools.lru_cache(maxsize=None)
def forward64(name):
    """The softmax in float64 (rows with a non-finite value: whatever numpy gives)."""
    c = case(name)
    y = np.full(c.nnz, np.nan, np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for _, a, L in c.rows():
            xr = c.x[a:a + L].astype(np.float64)
            e = np.exp(xr - xr.max())
            y[a:a + L] = e / e.sum()
    y.setflags(write=False)
    return y


def inside(c: Case):
    """Mask of the positions the pattern holds."""
    mk = np.zeros(c.nnz, bool)
    mk[c.p0:c.p1] = True
    return mk


def assert_same(got, want, where, mask=None):
    """NaN where want is NaN, the same bits everywhere else (on mask)."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    if mask is not None:
        got, want = got[mask], want[mask]
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{where}: NaN pattern differs at {np.flatnonzero(gn != wn)[:8]}"
    ok = wn | (bits(got) == bits(want))
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (f"{where}: {bad.size} positions differ, first {bad[:8]}: "
                           f"got {got[bad[:4]]}, want {want[bad[:4]]}")
