"""The far-position geometry (tests/far_pos_cases.py) in Python integers, and the host forms
on the same windows, with no GPU.

Part 1 checks every claim the GPU cases of tests/test_gpu_far_positions.py rest on: each
crossing holds and lies strictly inside the stated row with whole rows on both sides, each
window with its guards fits the arena, the starts take different residues, and a 32-bit wrap
of a byte offset or of a position past the top cannot land on the window or its guards.

Part 2 runs the host forms (spmm_sddmm_csr_host_f32, the edge softmax and its backward, the
multi-head forms on float32 / float16 / bfloat16 features, spmm_csr2csc) on the same windows
of np.empty arrays of the arena's size, of which only the window's pages are touched, and
holds each result to the same call on the near twin, bit for bit, with the guards unchanged,
and the twin to the restated rule of its entry (sddmm_cases.reference_bits, the softmax rule,
the piece oracle per head on the widened features, csr2csc_cases.reference), bit for bit too.
The device is held to these forms elsewhere. If the address space for the arrays cannot be
reserved the host-form tests skip with that reason.
"""
from __future__ import annotations

import numpy as np
import pytest

import csr2csc_cases as cc
import far_pos_cases as fp
import heads_cases as hc
import heads_half_cases as hh
import sddmm_cases as sd
from far_pos_cases import GUARD, INT_MAX, P31, P32

F = np.float32


# ------------------------------------------------------------------------ 1. the geometry
def test_the_windows_are_the_ones_the_gpu_cases_name():
    names = {w.name for w in fp.WINDOWS}
    assert len(names) == len(fp.WINDOWS) == 30
    for fam, n in (("p4", 8), ("p8", 6), ("q3", 8), ("q8", 8)):
        assert len(fp.windows(fam)) == n


@pytest.mark.parametrize("size,long_last", [("small", False), ("small", True), ("large", False),
                                            ("large", True)])
def test_matrix_shapes(size, long_last):
    lens = fp.lens_of(size, long_last)
    m, long_len = (fp.SMALL_M, fp.SMALL_LONG_LEN) if size == "small" else \
        (fp.LARGE_M, fp.LARGE_LONG_LEN)
    assert lens.size == m and lens[0] == 0 and lens[-1] > 0
    assert lens.max() == long_len and (lens == long_len).sum() == 1
    assert (np.argmax(lens) == m - 1) == long_last
    assert (lens == 1).any() and (lens[1:-1] == 0).any()
    if size == "small":
        assert long_len > 2 * 128 and 450 <= lens.sum() <= 650
        assert np.sort(lens)[:-1].max() <= 12
    else:
        assert 140_000 <= lens.sum() <= 160_000
        # more than one 128-nonzero piece in many rows, and a split hub row
        assert (lens > 128).sum() > 100 and long_len > 64 * 128
    ci = fp.colind_of(size, long_last)
    assert ci.size == lens.sum() and ci.min() == 0 and ci.max() == fp.K - 1
    rp = np.concatenate([[0], np.cumsum(lens)])
    assert all((np.diff(ci[a:b]) >= 0).all() for a, b in zip(rp[:-1], rp[1:]))


@pytest.mark.parametrize("w", fp.WINDOWS, ids=fp.ids(fp.WINDOWS))
def test_crossings_hold(w):
    fam = fp.FAMILY[w.family]
    heads, elem = fam["heads"], fam["elem"]
    rp = w.start + w.local
    assert w.start - GUARD >= 0 and rp[-1] == w.end
    if w.bound in ("TOP", "TOPL"):
        # the window ends at the largest position the family has
        assert w.end == fam["top"] and (w.end + 1) * heads > INT_MAX >= w.end * heads
        assert int(w.rowptr()[-1]) == w.end and w.base == 0
        assert (w.lens[-1] == w.lens.max()) == (w.bound == "TOPL")
        # its last element is the last whole position below 2^33 bytes
        assert 2 * P32 - elem * heads - elem < w.end * heads * elem <= 2 * P32 - elem
        return
    pc, bound, row = w.crossing()
    assert bound * elem in (P31, P32, 2 * P32) and w.lens[row] == w.lens.max()
    # the position before lies below the bound, the position holds an element at or past it
    assert ((pc - 1) * heads + heads - 1) < bound <= pc * heads + heads - 1
    assert ((pc - 1) * heads + heads - 1) * elem < bound * elem <= (pc * heads + heads - 1) * elem
    # strictly inside the long row, rows with entries wholly on each side
    assert rp[row] < pc - 1 and pc < rp[row + 1] - 1
    assert (w.lens[:row] > 0).any() and (w.lens[row + 1:] > 0).any()
    assert rp[row] - rp[0] > 0 and rp[-1] - rp[row + 1] > 0


def test_one_case_per_family_runs_at_base_1():
    for fam in fp.FAMILY:
        bases = [w.base for w in fp.windows(fam)]
        assert 1 in bases and 0 in bases
        for w in fp.windows(fam):
            assert int(w.rowptr()[-1]) - w.base == w.end
            assert int(w.rowptr(near=True)[0]) - w.base == w.twin_start()


def test_starts_take_different_residues():
    for fam in fp.FAMILY:
        ws = [w for w in fp.windows(fam) if w.bound.startswith("W")]
        for mod in (64, 256):
            res = [w.start % mod for w in ws]
            assert len(set(res)) == len(res), (fam, mod, res)
        assert all(w.start % 256 == fp.RESIDUE[list(fp.FAMILY[fam]["bounds"]).index(w.bound),
                                               w.size] for w in ws)
        every = {w.start % 64 for w in fp.windows(fam)}
        assert len(every) >= 6, (fam, sorted(every))
    # the TOP / TOPL residues the file states (small TOP, small TOPL, large TOP, large TOPL)
    for fam, want in (("p4", (19, 15, 152, 29)), ("q8", (19, 15, 152, 29)),
                      ("q3", (190, 186, 67, 200))):
        got = tuple(fp.BY_NAME[f"{fam}-{b}-{s}"].start % 256 for s in ("small", "large")
                    for b in ("TOP", "TOPL"))
        assert got == want, (fam, got)


@pytest.mark.parametrize("w", fp.WINDOWS, ids=fp.ids(fp.WINDOWS))
def test_windows_fit_the_arena_and_the_twin_keeps_the_residues(w):
    heads = w.heads
    # every array a case on this family places: 4-byte colind per position, the family's
    # own array, an fp16 val (p4) and colind_hot behind HOT_BYTE_OFF (p4)
    assert fp.last_byte(w, 4) <= fp.POS_ARENA_BYTES
    assert fp.last_byte(w, w.elem, heads) <= fp.POS_ARENA_BYTES
    if w.family == "p4":
        assert fp.last_byte(w, 4, 1, fp.HOT_BYTE_OFF) <= fp.POS_ARENA_BYTES
        # colind and colind_hot share an arena and never overlap
        assert fp.HOT_BYTE_OFF > (w.nnz + 2 * GUARD) * 4 and fp.HOT_BYTE_OFF % 256 == 0
    assert (w.twin_start() - w.start) % 1024 == 0 and w.twin_start() >= GUARD
    assert fp.twin_bytes(w, 8, 8) < 1 << 24


@pytest.mark.parametrize("w", fp.WINDOWS, ids=fp.ids(fp.WINDOWS))
def test_a_32_bit_wrap_lands_outside_the_window(w):
    lo, hi = w.start - GUARD, w.end + GUARD
    layouts = {(4, 1), (w.elem, w.heads)} | ({(2, 1)} if w.family == "p4" else set())
    wrapped_any = False
    for elem, per in layouts:
        for alias in fp.wraps(w, elem, per):
            wrapped_any |= alias.size > 0
            assert not ((alias >= lo) & (alias < hi)).any(), (w.name, elem, per)
    # each family's own array wraps somewhere in every window (a signed 32-bit byte offset)
    assert wrapped_any
    if w.bound in ("TOP", "TOPL"):
        # positions (elements) past the top wrap below zero as an int
        q = w.end * w.heads + np.arange(1, 257 * w.heads, dtype=np.int64)
        q = q[q > INT_MAX]
        assert q.size and ((q.astype(np.uint32).astype(np.int32)) < 0).all()
        if w.heads == 1:
            assert (np.arange(INT_MAX + 1, INT_MAX + 257, dtype=np.int64).astype(np.uint32)
                    .astype(np.int32) < 0).all()


def test_hot_tags_are_not_degenerate():
    for w in fp.windows("p4"):
        ci = fp.colind_of(w.size, w.long_last)
        for k in (fp.K, 1024 - w.base):
            hot = fp.hot_columns(ci, k)
            assert 0 < hot.sum() <= fp.HOT_ROWS and 0 < hot[ci].sum() < ci.size
    assert fp.hot_bytes(5) == 20 * fp.HOT_ROWS and fp.hot_bytes(64) == 256 * fp.HOT_ROWS
    assert fp.hot_bytes(72) == 288 * fp.HOT_ROWS and fp.hot_bytes(136) == 544 * fp.HOT_ROWS


def test_with_guards_and_placed_on_a_host_buffer():
    torch = pytest.importorskip("torch")
    w = fp.BY_NAME["q3-W29-small"]
    data = np.arange(w.nnz * 3, dtype=F)
    host = fp.with_guards(data, 3)
    assert host.size == (w.nnz + 2 * GUARD) * 3 and host.dtype == np.int32
    assert (host[:GUARD * 3].view(np.uint32) == fp.sentinel_bits(4)).all()
    buf = torch.zeros(fp.twin_bytes(w, 4, 3), dtype=torch.uint8)
    p = fp.place(buf, w, True, host, 3)
    t = p.tensor(torch.float32, w.twin_start() + w.nnz)
    assert t.numel() == (w.twin_start() + w.nnz) * 3
    assert np.array_equal(t[w.twin_start() * 3:].numpy(), data)
    assert np.array_equal(p.window(torch.float32).numpy(), data)
    p.unchanged("placed")
    t[w.twin_start() * 3 - 1] = 0.0
    with pytest.raises(AssertionError, match="guard in front"):
        p.read("placed")


# ------------------------------------------------------------------------ 2. the host forms
@pytest.fixture(scope="module")
def host_arenas():
    try:
        bufs = [np.empty(fp.POS_ARENA_BYTES, np.uint8) for _ in range(3)]
    except MemoryError:
        pytest.skip(f"no 3 x {fp.POS_ARENA_BYTES} bytes of address space for the host arrays")
    yield bufs
    del bufs


class HostSite:
    """far: arrays are views of the three host arenas from element 0 to the window's end;
    near: small arrays. put() writes the window and its guards and returns the flat array."""

    def __init__(self, w, bufs):
        self.w, self.bufs, self.near = w, bufs, bufs is None
        self.start = w.twin_start() if self.near else w.start
        self.end = self.start + w.nnz
        self.placed = []

    def put(self, slot, data, per=1, front=None, back=None, check=True):
        host = fp.with_guards(data, per, front, back)
        dt = np.ascontiguousarray(data).dtype
        if self.near:
            flat = np.empty((self.end + GUARD) * per, dt)
        else:
            flat = self.bufs[slot].view(dt)
        lo = (self.start - GUARD) * per
        flat.view(host.dtype)[lo:lo + host.size] = host
        if check:
            self.placed.append((flat, host, lo))
        return flat[:self.end * per], (flat, host, lo, per)

    def rowptr(self):
        return (self.start + self.w.local + self.w.base).astype(np.int32)

    def colind(self, slot=0):
        ci = fp.colind_of(self.w.size, self.w.long_last)
        front, back = fp.colind_guards(len(self.w.name))
        return self.put(slot, ci + self.w.base, 1, front + self.w.base, back + self.w.base)[0]

    def unchanged(self):
        for flat, host, lo in self.placed:
            assert np.array_equal(flat.view(host.dtype)[lo:lo + host.size], host), self.w.name

    @staticmethod
    def result(out):
        """The window of an output array, after checking its guards."""
        flat, host, lo, per = out
        got = flat.view(host.dtype)[lo:lo + host.size]
        g = GUARD * per
        assert np.array_equal(got[:g], host[:g]) and np.array_equal(got[-g:], host[-g:])
        return got[g:-g].copy()


def host_both(w, bufs, run):
    far, near = run(HostSite(w, bufs)), run(HostSite(w, None))
    for f, n in zip(far, near):
        assert f.dtype == n.dtype and np.array_equal(f, n), w.name
    return near


def _rng(w, salt):
    return np.random.default_rng(1000 * salt + fp.WINDOWS.index(w))


HEADS_W = fp.windows("q3") + fp.windows("q8")


def _rows(w):
    return np.repeat(np.arange(w.m), w.lens)


def _cols(w):
    return fp.colind_of(w.size, w.long_last).astype(np.int64)


@pytest.mark.parametrize("w", fp.windows("p4"), ids=fp.ids(fp.windows("p4")))
def test_host_sddmm(host_arenas, w):
    from spmm_hip import prep
    n = 12
    rng = _rng(w, 1)
    X = rng.uniform(-1, 1, (w.m, n)).astype(F)
    Y = rng.uniform(-1, 1, (fp.K, n)).astype(F)
    old = rng.uniform(-1, 1, w.nnz).astype(F)

    def run(site):
        ci = site.colind(0)
        out, o = site.put(1, old, check=False)
        prep.sddmm(w.m, n, fp.K, site.rowptr(), ci, X, Y, out=out, alpha=0.5, beta=-1.5, base=w.base)
        site.unchanged()
        return (site.result(o),)

    near = host_both(w, host_arenas, run)[0].view(F)
    want = sd.reference_bits(_rows(w), _cols(w), X, Y, 0.5, -1.5, old)
    assert np.array_equal(sd.bits(near), sd.bits(want))


@pytest.mark.parametrize("w", fp.windows("p4"), ids=fp.ids(fp.windows("p4")))
def test_host_edge_softmax_and_backward(host_arenas, w):
    from spmm_hip import prep
    rng = _rng(w, 2)
    x = rng.normal(0, 3, w.nnz).astype(F)
    g = rng.normal(0, 1, w.nnz).astype(F)
    sent = np.full(w.nnz, fp.sentinel_bits(4), np.uint32).view(F)

    def run(site):
        xs = site.put(0, x)[0]
        y, yo = site.put(1, sent, check=False)
        prep.edge_softmax(site.rowptr(), xs, base=w.base, out=y)
        yw = site.result(yo)
        site.unchanged()
        site.placed = []
        ys = site.put(0, yw.view(F))[0]
        gs = site.put(1, g)[0]
        gx, go = site.put(2, sent, check=False)
        prep.edge_softmax_bwd(site.rowptr(), ys, gs, base=w.base, out=gx)
        site.unchanged()
        return yw, site.result(go)

    y, gx = host_both(w, host_arenas, run)
    want_y = fp.softmax_fwd_rule(w.local, x)
    assert np.array_equal(y.view(np.uint32), sd.bits(want_y)), "forward against the restated rule"
    assert np.array_equal(gx.view(np.uint32), sd.bits(fp.softmax_bwd_rule(w.local, want_y, g))), \
        "backward against the restated rule"


@pytest.mark.parametrize("ty", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("w", HEADS_W, ids=fp.ids(HEADS_W))
def test_host_heads_forms(host_arenas, w, ty):
    """The multi-head sampled product and product on features of type ty, and (float32) the
    multi-head softmax and its backward, at the q bounds. The twins are held to the restated
    rules per head, on the widened features: sddmm_cases.reference_bits, the piece oracle,
    the softmax rule."""
    from spmm_hip import prep
    heads, d = w.heads, 5
    rng = _rng(w, 3)

    def feats(rows):
        """(the array prep takes, its keyword arguments, the same values as float32)."""
        a = rng.uniform(-1, 1, (rows, heads, d)).astype(F)
        if ty == "f32":
            return a, {}, a
        bits = hh.to_bits(a, ty).reshape(rows, heads, d)
        return hh.stored(bits, ty) + (hh.widen(bits, ty).reshape(rows, heads, d),)

    (X, kw, Xw), (Y, _, Yw) = feats(w.m), feats(fp.K)
    old = rng.uniform(-1, 1, (w.nnz, heads)).astype(F)
    val = rng.uniform(-1, 1, (w.nnz, heads)).astype(F)
    sent = np.full(w.nnz * heads, fp.sentinel_bits(4), np.uint32).view(F)

    def run(site):
        ci = site.colind(0)
        out, o = site.put(1, old, heads, check=False)
        prep.sddmm_heads(w.m, d, fp.K, heads, site.rowptr(), ci, X, Y,
                         out=out.reshape(site.end, heads), alpha=0.5, beta=-1.5, base=w.base, **kw)
        e = site.result(o)
        vs = site.put(2, val, heads)[0]
        C = prep.csrmm_heads(w.m, d, fp.K, heads, site.rowptr(), ci, vs, Y, base=w.base, **kw)
        site.unchanged()
        res = [e, np.ascontiguousarray(C).view(np.int32).reshape(-1)]
        if ty == "f32":
            site.placed = []
            xs = site.put(0, e.view(F), heads)[0]
            y, yo = site.put(1, sent, heads, check=False)
            prep.edge_softmax_heads(site.rowptr(), xs.reshape(site.end, heads), base=w.base,
                                    out=y.reshape(site.end, heads))
            yw = site.result(yo)
            site.unchanged()
            site.placed = []
            gs = site.put(0, val, heads)[0]
            gx, go = site.put(2, sent, heads, check=False)
            prep.edge_softmax_bwd_heads(site.rowptr(), y.reshape(site.end, heads),
                                        gs.reshape(site.end, heads), base=w.base,
                                        out=gx.reshape(site.end, heads))
            site.unchanged()
            assert np.array_equal(site.result(yo), yw)
            res += [yw, site.result(go)]
        return tuple(res)

    near = host_both(w, host_arenas, run)
    e, C = near[0].view(F).reshape(w.nnz, heads), near[1].view(F).reshape(w.m, heads, d)
    for h in range(heads):
        want = sd.reference_bits(_rows(w), _cols(w), np.ascontiguousarray(Xw[:, h]),
                                 np.ascontiguousarray(Yw[:, h]), 0.5, -1.5,
                                 np.ascontiguousarray(old[:, h]))
        assert np.array_equal(sd.bits(e[:, h]), sd.bits(want)), f"sddmm_heads head {h}"
    want_C = hc.product_reference_on(w.m, w.local.astype(np.int32),
                                     fp.colind_of(w.size, w.long_last), val,
                                     np.ascontiguousarray(Yw))
    assert np.array_equal(sd.bits(C), sd.bits(want_C)), "csrmm_heads against the piece oracle"
    if ty == "f32":
        y, gx = (a.view(F).reshape(w.nnz, heads) for a in near[2:])
        for h in range(heads):
            wy = fp.softmax_fwd_rule(w.local, np.ascontiguousarray(e[:, h]))
            assert np.array_equal(sd.bits(y[:, h]), sd.bits(wy)), f"softmax head {h}"
            wg = fp.softmax_bwd_rule(w.local, wy, np.ascontiguousarray(val[:, h]))
            assert np.array_equal(sd.bits(gx[:, h]), sd.bits(wg)), f"softmax backward head {h}"


# an 8-byte val fits the arena up to W30 (2^33 bytes); at the TOP forms it would be 16 GiB
CSR2CSC = [(w, vb) for w in fp.windows("p4") for vb in (0, 2, 4, 8)
           if vb < 8 or w.bound.startswith("W")]


@pytest.mark.parametrize("w,vb", CSR2CSC, ids=[f"{w.name}-vb{vb}" for w, vb in CSR2CSC])
def test_host_csr2csc(host_arenas, w, vb):
    """perm holds the far absolute positions: the twin's, shifted by the starts' distance."""
    from spmm_hip import prep
    v = cc.values(w.nnz, vb)
    ci0 = fp.colind_of(w.size, w.long_last)

    def run(site):
        ci = site.colind(0)
        vs = None if v is None else site.put(1, v)[0]
        out = prep.csr2csc(w.m, fp.K, site.rowptr(), ci, vs, base=w.base, base_out=0,
                           return_perm=True)
        site.unchanged()
        res = [np.ascontiguousarray(a) for a in out]
        res[-1] = res[-1].astype(np.int64) - site.start
        if v is not None:
            res[2] = cc.bits(res[2])
        return tuple(res)

    near = host_both(w, host_arenas, run)
    colptr, rowind, cv, perm = cc.reference(w.m, fp.K, w.local + w.base, ci0 + w.base, v, w.base, 0)
    assert np.array_equal(near[0], colptr) and np.array_equal(near[1], rowind)
    assert np.array_equal(near[-1], perm)
    if v is not None:
        assert np.array_equal(near[2], cc.bits(cv))
