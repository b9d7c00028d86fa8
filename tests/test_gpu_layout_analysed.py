"""The once-per-matrix BSR entries on padded and offset B / C layouts.

tests/test_gpu_layout.py runs the CSR, hybrid and drop-in BSR products on framed
operands (helpers.framed: B and C inside larger buffers, `off` elements in, `pad`
extra elements per row, signalling-NaN sentinels all around). Here the analysed
(spmm_bsrmm_analysed_f32 / _f16) and grouped (spmm_bsrmm_grouped_f32 / _f16) entries
run the same way: the gaps must come back bit for bit, B unchanged, C's data region
starts as NaN at beta = 0 and finite at beta != 0 (ABS of test_gpu_layout.py).

Layouts are (off_B, pad_B, off_C, pad_C) in elements (halves for an fp16 B, floats
otherwise); ld = width + pad, a column-major operand's ld = its row count + pad. Which
layout reaches which kernel or status, read off the launchers' predicates (the tests
never call them):

spmm_bsrmm_analysed_f32 (launch_bsrmm_f32 on valCol as COLUMN blocks with masks; the
masked column stream needs a row-major B, n % 4 == 0, ldb % 4 == 0, 16-byte valCol and
B, and row-major C rows on 16 bytes or a column-major C):

  layout                           row-major B and C
  (0,0,0,0) (0,4,0,8)              masked stream
  ALIGNED_LAYOUTS_F32              masked stream (bases 16 mod 256, ld % 4 == 0)
  (0,1,0,0) (0,2,0,0)              ldb % 4 != 0: register-fragment kernel, COLUMN blocks
  (1,0,0,0) (2,0,0,0)              B off 16 bytes: register-fragment kernel
  (0,0,0,1) (0,0,0,2)              ldc % 4 != 0: register-fragment kernel
  (0,0,1,0) (0,0,2,0)              C off 16 bytes: register-fragment kernel
  (1,3,3,1) (3,1,1,3)              all of them: register-fragment kernel

A column-major C lifts C's requirement (the stream's own transposed epilogue: masked
stream whenever B qualifies). A column-major B is staged row-major and tight in the
workspace (transpose4_kernel reads it at any 4-byte base and any ldb) and the masked
stream runs on the copy. So the masked stream's bits (those of the tight run: same
items, same order) are asserted on (0,4,0,8) and ALIGNED_LAYOUTS_F32 with row-major
operands, and the fp32 bar everywhere. With a row-major C on a shallow grid the column
streams (drop-in and analysed alike) split an outlier block row into segments and add
the partial tiles (cs2_segments, seg_fixup_kernel); the grouped stream never does, so
its bits are theirs on every other block row. A valCol off 16 bytes (the analysis writes it
one element at a time) sends every layout to the generic kernel.

spmm_bsrmm_analysed_f16 (launch_bsrmm_f16; the masked stream needs n >= 128,
n % 8 == 0, a row-major B on 16 bytes with ldb % 8 == 0 and a 16-byte valCol; C may have
any base and ld, in either order): B parts (off, pad) that are multiples of 8 halves
take the masked stream whatever C's part, every other B part the register-fragment
kernel; a column-major B (n >= 128, n % 8 == 0) is staged by transpose16x4_kernel from
any 2-byte base and ldb.

spmm_bsrmm_grouped_f32 (group.cpp): NOT_SUPPORTED, before any launch, when n % 4 != 0,
a row-major ldb % 4 or ldc % 4 != 0, or B or C (either order) is off 16 bytes; every
other case runs bsr32_f32_grp_kernel on row-major operands, a column-major B staged
through launch_transpose with the caller's ldb, a column-major C computed into a tight
row-major tile (beta = 0) and transposed back with beta and the caller's ldc.

spmm_bsrmm_grouped_f16: NOT_SUPPORTED when n % 8 != 0, a row-major ldb % 8 != 0 or B
is off 16 bytes; C may have any base and ld in either order (bsr16_f16_grp_kernel
writes it itself), a column-major B is staged (any ldb).

The group-analysis buffer must be 16-byte aligned (INVALID_VALUE before any launch
otherwise): its sections sit at multiples of 256 bytes from its start and are read as
16-byte vectors."""
from __future__ import annotations

import numpy as np
import pytest

from helpers import (ALIGNED_LAYOUTS_F32, GROUPED_F16_ACCEPTED, GROUPED_F16_REJECTED,
                     GROUPED_F32_ACCEPTED, GROUPED_F32_REJECTED, TOL_F16_ACC, TOL_F32,
                     assert_normwise, column_sparse_bsr, framed, long_row_column_sparse_bsr,
                     oracle_bsrmm_f64, oracle_csrmm_f64, rand_bsr)
from test_gpu_layout import AB_IDS, ABS, LAYOUTS, _c_init, _dev, _expect, _ops, _same_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# (mb, kb, bs, half, builder): the matrices of test_bsrmm_analysed, test_bsrmm_analysed_f16,
# test_bsrmm_grouped_f32 and test_bsrmm_grouped_f16 (tests/test_gpu_bsr.py)
_KINDS = {"an32": (23, 320, 32, False, long_row_column_sparse_bsr),
          "an16": (21, 320, 16, True, long_row_column_sparse_bsr),
          "grp32": (37, 60, 32, False, lambda rng, mb, kb, bs: column_sparse_bsr(rng, mb, kb, bs, 0.3)),
          "grp16": (37, 60, 16, True, lambda rng, mb, kb, bs: column_sparse_bsr(rng, mb, kb, bs, 0.3))}
_cache: dict = {}


class _Case:
    pass


def _matrix(kind):
    if kind not in _cache:
        mb, kb, bs, half, build = _KINDS[kind]
        rng = np.random.default_rng(sum(map(ord, kind)))
        rp, ci, v = build(rng, mb, kb, bs)
        _cache[kind] = rp, ci, v.astype(np.float16 if half else np.float32)
    return _cache[kind]


def _case(oracle, kind, n):
    """The matrix of `kind`, B, C0 and the f64 oracle at width n, once per (kind, n)."""
    key = (kind, n)
    if key not in _cache:
        c = _Case()
        c.mb, c.kb, c.bs, c.half, _ = _KINDS[kind]
        c.rp, c.ci, c.v = _matrix(kind)
        c.K, c.m, c.n, c.nnzb = c.kb * c.bs, c.mb * c.bs, n, c.ci.size
        rng = np.random.default_rng(7000 + n + c.bs)
        c.B = rng.uniform(-1, 1, (c.K, n)).astype(c.v.dtype)
        c.C0 = rng.uniform(-1, 1, (c.m, n)).astype(np.float32)
        c.ref, c.absd = oracle_bsrmm_f64(oracle, 0, c.mb, n, c.bs, c.rp, c.ci, c.v, c.B, n, 0,
                                         half=c.half)
        c.tol = TOL_F16_ACC if c.half else TOL_F32
        _cache[key] = c
    return _cache[key]


def _values(c, direction):
    """The block values as ROW (0) or COLUMN (1) blocks."""
    if direction == 0:
        return c.v
    return np.ascontiguousarray(c.v.reshape(-1, c.bs, c.bs).transpose(0, 2, 1)).reshape(-1)


class _Frames:
    """Framed operands of one case: B once per (order, off, pad) (checked unchanged by
    close()), C fresh per call."""

    def __init__(self, c):
        self.c, self.b = c, {}

    def B(self, ob, off, pad, what):
        key = (ob, off, pad)
        if key not in self.b:
            B2 = self.c.B if ob == 0 else np.ascontiguousarray(self.c.B.T)
            ld = B2.shape[1] + pad
            self.b[key] = framed(B2, ld, off) + (ld, what)
        dB, _, ld, _ = self.b[key]
        return dB, ld

    def C(self, oc, off, pad, init):
        C2 = init if oc == 0 else np.ascontiguousarray(init.T)
        ld = C2.shape[1] + pad
        dC, chk = framed(C2, ld, off)

        def extract(what):
            got = chk(what + ": C")
            return got if oc == 0 else np.ascontiguousarray(got.T)
        return dC, chk, ld, extract

    def close(self):
        for _, chk, _, what in self.b.values():
            chk.unchanged(what + ": B")


def _case_list(lays):
    """Row-major B and C on every layout, a column-major C on those that pad or offset
    C, a column-major B on those that pad or offset B: (layout, order_b, order_c)."""
    return ([(lay, 0, 0) for lay in lays] + [(lay, 0, 1) for lay in lays if lay[2] or lay[3]] +
            [(lay, 1, 0) for lay in lays if lay[0] or lay[1]])


# ----------------------------------------------------- spmm_bsrmm_analysed_f32
AN32_LAYOUTS = LAYOUTS + ALIGNED_LAYOUTS_F32
AN32_STREAM = [(0, 4, 0, 8)] + ALIGNED_LAYOUTS_F32  # the tight run's bits (row-major operands)


@pytest.mark.parametrize("ab", ABS, ids=AB_IDS)
@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("n", [64, 136])
def test_analysed_f32_layouts(oracle, device, n, direction, ab):
    """spmm_bsrmm_analysed_f32 on the analysis of ROW and COLUMN blocks: column-sparse
    blocks, explicit zero and single-column blocks, an empty block row and one of 300
    blocks (segments), within TOL_F32 of oracle_bsrmm_f64 on every layout and order,
    the tight run's bits wherever the masked stream runs on row-major operands, and at
    n = 136 on the tight layout the bits of spmm_bsrmm_ex_f32 and, on every block row
    that the column streams do not split into segments, of the grouped stream
    (include/spmm_hip.h)."""
    alpha, beta = ab
    ops = _ops()
    c = _case(oracle, "an32", n)
    want64, scale = _expect(c.ref, c.absd, c.C0, alpha, beta)
    drp, dci, dv = _dev(c.rp, c.ci, _values(c, direction))
    masks, vcol = ops.bsr32_analysis(dv, nnzb=c.nnzb, direction=direction)
    fr = _Frames(c)

    def run(lay, ob, oc):
        what = (f"analysed f32 n={n} dir={direction} layout={lay} orders=({ob},{oc}) "
                f"alpha={alpha} beta={beta}")
        dB, ldb = fr.B(ob, lay[0], lay[1], what)
        dC, _, ldc, extract = fr.C(oc, lay[2], lay[3], _c_init(c.C0, beta))
        ops.bsrmm_analysed(drp, dci, vcol, masks, dB, mb=c.mb, kb=c.kb, n=n, ldb=ldb, order_b=ob,
                           C=dC, ldc=ldc, order_c=oc, alpha=alpha, beta=beta)
        got = extract(what)
        assert_normwise(got, want64, scale, TOL_F32, what)
        return got, what

    tight, _ = run((0, 0, 0, 0), 0, 0)
    for lay, ob, oc in _case_list(AN32_LAYOUTS):
        got, what = run(lay, ob, oc)
        if ob == 0 and oc == 0 and lay in AN32_STREAM:
            assert _same_bits(got, tight), what + ": bits differ from the tight run"
    fr.close()
    if n == 136:
        # the header: the analysed, the drop-in and the grouped stream agree bit for bit
        drow, dB = _dev(c.v, c.B)
        dC = _dev(_c_init(c.C0, beta))[0]
        ops.bsrmm(drp, dci, drow, dB, mb=c.mb, kb=c.kb, n=n, bs=32, ldb=n, C=dC, ldc=n, alpha=alpha,
                  beta=beta)
        assert _same_bits(dC.cpu().numpy(), tight), "analysed differs from spmm_bsrmm_ex_f32"
        # the grouped stream runs each block row as one chain; the column streams split the
        # 300-block row 5 into segments on this shallow grid (cs2_segments: row-major C, a
        # row past twice the mean load per wave slot) and add their partial tiles, another
        # association: the same bits on every other block row, the bar on that one
        dC = _dev(_c_init(c.C0, beta))[0]
        with ops.GroupedBsr32(drp, dci, dv, mb=c.mb, direction=direction) as grp:
            grp.mm(dB, kb=c.kb, n=n, ldb=n, C=dC, ldc=n, alpha=alpha, beta=beta)
            got = dC.cpu().numpy()
            assert_normwise(got, want64, scale, TOL_F32, "the grouped stream")
            rest = np.arange(c.m) // 32 != 5
            assert _same_bits(got[rest], tight[rest]), "analysed differs from the grouped stream"


# ----------------------------------------------------- spmm_bsrmm_analysed_f16
# B parts in halves: offsets 0 / 1 / 2 / 8, pads 0 / 1 / 8 / 16; C parts in floats: 0 / 1 / 3 / 4
AN16_LAYOUTS = [(0, 0, 0, 0), (8, 0, 0, 0), (8, 8, 4, 4), (0, 16, 1, 0), (0, 8, 0, 1), (8, 16, 3, 3),
                (1, 0, 0, 0), (2, 0, 0, 4), (0, 1, 0, 0), (1, 1, 3, 1), (2, 8, 1, 3)]


def _b_on_8_halves(lay):
    return lay[0] % 8 == 0 and lay[1] % 8 == 0


@pytest.mark.parametrize("ab", ABS, ids=AB_IDS)
@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("n", [136, 264])
def test_analysed_f16_layouts(oracle, device, n, direction, ab):
    """spmm_bsrmm_analysed_f16 (B's layout in halves, C's in floats) within TOL_F16_ACC
    of the exact product of the same fp16 values on every layout and order; the tight
    run's bits on every layout whose B part is a multiple of 8 halves, whatever C's
    part (C's layout does not select the kernel)."""
    alpha, beta = ab
    ops = _ops()
    c = _case(oracle, "an16", n)
    want64, scale = _expect(c.ref, c.absd, c.C0, alpha, beta)
    drp, dci, dv = _dev(c.rp, c.ci, _values(c, direction))
    masks, vcol = ops.bsr16_analysis(dv, nnzb=c.nnzb, direction=direction)
    fr = _Frames(c)

    def run(lay, ob, oc):
        what = (f"analysed f16 n={n} dir={direction} layout={lay} orders=({ob},{oc}) "
                f"alpha={alpha} beta={beta}")
        dB, ldb = fr.B(ob, lay[0], lay[1], what)
        dC, _, ldc, extract = fr.C(oc, lay[2], lay[3], _c_init(c.C0, beta))
        ops.bsrmm_analysed_f16(drp, dci, vcol, masks, dB, mb=c.mb, kb=c.kb, n=n, ldb=ldb,
                               order_b=ob, C=dC, ldc=ldc, order_c=oc, alpha=alpha, beta=beta)
        got = extract(what)
        assert_normwise(got, want64, scale, TOL_F16_ACC, what)
        return got, what

    assert any(lay[0] % 2 and lay[1] % 2 for lay in AN16_LAYOUTS)
    tight, _ = run((0, 0, 0, 0), 0, 0)
    for lay, ob, oc in _case_list(AN16_LAYOUTS):
        got, what = run(lay, ob, oc)
        if ob == 0 and oc == 0 and _b_on_8_halves(lay):
            assert _same_bits(got, tight), what + ": bits differ from the tight run"
    fr.close()


# ------------------------------------------------------ spmm_bsrmm_grouped_f32
def _grouped_run(c, grp, fr, case, n, alpha, beta, init, what):
    """One grouped product on the framed operands of `case`: (C view's checker, extract)."""
    _, ob, oc, lay = case
    dB, ldb = fr.B(ob, lay[0], lay[1], what)
    dC, chk, ldc, extract = fr.C(oc, lay[2], lay[3], init)
    grp.mm(dB, kb=c.kb, n=n, ldb=ldb, order_b=ob, C=dC, ldc=ldc, order_c=oc, alpha=alpha, beta=beta)
    return chk, extract


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("n", [64, 132])
@pytest.mark.parametrize("W", [2, 4])
def test_grouped_f32_accepted_layouts(oracle, device, W, n, direction):
    """spmm_bsrmm_grouped_f32 on every accepted layout (GROUPED_F32_ACCEPTED: 16-byte
    bases off the 256-byte one, ld % 4 == 0 for row-major operands, any pad for
    column-major ones) within TOL_F32; row-major cases give the tight run's bits and
    those of spmm_bsrmm_ex_f32 on the same layout (the column stream on the ROW blocks
    of the same matrix: the same MFMAs in the same order), a column-major C the
    transposed row-major result at beta = 0 (the staged tile is copied)."""
    ops = _ops()
    c = _case(oracle, "grp32", n)
    drp, dci, dv, drow = _dev(c.rp, c.ci, _values(c, direction), c.v)
    fr = _Frames(c)
    with ops.GroupedBsr32(drp, dci, dv, mb=c.mb, group_rows=W, direction=direction) as grp:
        for alpha, beta in ABS:
            want64, scale = _expect(c.ref, c.absd, c.C0, alpha, beta)
            init = _c_init(c.C0, beta)
            tight = None
            for case in GROUPED_F32_ACCEPTED:
                _, ob, oc, lay = case
                what = (f"grouped f32 W={W} n={n} dir={direction} layout={lay} orders=({ob},{oc}) "
                        f"alpha={alpha} beta={beta}")
                _, extract = _grouped_run(c, grp, fr, case, n, alpha, beta, init, what)
                got = extract(what)
                assert_normwise(got, want64, scale, TOL_F32, what)
                if tight is None:
                    assert (ob, oc, lay) == (0, 0, (0, 0, 0, 0))
                    tight = got
                if ob == 0 and oc == 0:
                    assert _same_bits(got, tight), what + ": bits differ from the tight run"
                    dB, ldb = fr.B(0, lay[0], lay[1], what)
                    dC, _, ldc, ex2 = fr.C(0, lay[2], lay[3], init)
                    ops.bsrmm(drp, dci, drow, dB, mb=c.mb, kb=c.kb, n=n, bs=32, ldb=ldb, C=dC,
                              ldc=ldc, alpha=alpha, beta=beta)
                    assert _same_bits(ex2(what + " (spmm_bsrmm_ex_f32)"), got), \
                        what + ": bits differ from spmm_bsrmm_ex_f32 on this layout"
                if oc == 1 and beta == 0.0:
                    assert _same_bits(got, tight), what + ": not the transposed row-major result"
    fr.close()


def _rejected(c, grp, cases, n_default, rng):
    """Each case raises NOT_SUPPORTED and leaves C (data region included) and B as they
    were: nothing was launched."""
    from spmm_hip._lib import NOT_SUPPORTED, SpmmError
    for cn, ob, oc, lay in cases:
        n = cn or n_default
        what = f"rejected n={n} layout={lay} orders=({ob},{oc})"
        B = rng.uniform(-1, 1, (c.K, n)).astype(c.v.dtype)
        C0 = rng.uniform(-1, 1, (c.m, n)).astype(np.float32)
        B2 = B if ob == 0 else np.ascontiguousarray(B.T)
        C2 = C0 if oc == 0 else np.ascontiguousarray(C0.T)
        ldb, ldc = B2.shape[1] + lay[1], C2.shape[1] + lay[3]
        dB, chkB = framed(B2, ldb, lay[0])
        dC, chkC = framed(C2, ldc, lay[2])
        with pytest.raises(SpmmError) as e:
            grp.mm(dB, kb=c.kb, n=n, ldb=ldb, order_b=ob, C=dC, ldc=ldc, order_c=oc, alpha=0.7,
                   beta=-1.3)
        assert e.value.status == NOT_SUPPORTED, what
        torch.cuda.synchronize()
        chkC.unchanged(what + ": C")
        chkB.unchanged(what + ": B")


@pytest.mark.parametrize("n", [64, 132])
@pytest.mark.parametrize("W", [2, 4])
def test_grouped_f32_rejected_layouts(oracle, device, W, n):
    """Each cause of NOT_SUPPORTED alone (GROUPED_F32_REJECTED): ldb % 4 or ldc % 4 of 1
    and 2, B or C 1 and 2 floats off, in either storage order, and n = 130 on
    ld = 132."""
    ops = _ops()
    c = _case(oracle, "grp32", n)
    drp, dci, dv = _dev(c.rp, c.ci, c.v)
    with ops.GroupedBsr32(drp, dci, dv, mb=c.mb, group_rows=W) as grp:
        _rejected(c, grp, GROUPED_F32_REJECTED, n, np.random.default_rng(5))


# ------------------------------------------------------ spmm_bsrmm_grouped_f16
@pytest.mark.parametrize("n", [136, 264])
@pytest.mark.parametrize("W", [2, 4, 8])
def test_grouped_f16_accepted_layouts(oracle, device, W, n):
    """spmm_bsrmm_grouped_f16 on GROUPED_F16_ACCEPTED (B parts that are multiples of 8
    halves with every C part, a column-major C on padded ldc, a column-major B on
    ldb = K + 0 / 1 / 8) within TOL_F16_ACC; every case with a row-major B gives the
    tight run's bits at the same W."""
    ops = _ops()
    c = _case(oracle, "grp16", n)
    drp, dci, dv = _dev(c.rp, c.ci, c.v)
    fr = _Frames(c)
    with ops.GroupedBsr16(drp, dci, dv, mb=c.mb, group_rows=W) as grp:
        for alpha, beta in ABS:
            want64, scale = _expect(c.ref, c.absd, c.C0, alpha, beta)
            init = _c_init(c.C0, beta)
            tight = None
            for case in GROUPED_F16_ACCEPTED:
                _, ob, oc, lay = case
                what = (f"grouped f16 W={W} n={n} layout={lay} orders=({ob},{oc}) alpha={alpha} "
                        f"beta={beta}")
                _, extract = _grouped_run(c, grp, fr, case, n, alpha, beta, init, what)
                got = extract(what)
                assert_normwise(got, want64, scale, TOL_F16_ACC, what)
                if tight is None:
                    assert (ob, oc, lay) == (0, 0, (0, 0, 0, 0))
                    tight = got
                if ob == 0:
                    assert _same_bits(got, tight), what + ": bits differ from the tight run"
    fr.close()


@pytest.mark.parametrize("n", [136, 264])
@pytest.mark.parametrize("W", [2, 4, 8])
def test_grouped_f16_rejected_layouts(oracle, device, W, n):
    """Each cause of NOT_SUPPORTED alone (GROUPED_F16_REJECTED): a row-major ldb % 8 of
    1 and 4, B 1 and 4 halves off, n = 132 on ldb = 136."""
    ops = _ops()
    c = _case(oracle, "grp16", n)
    drp, dci, dv = _dev(c.rp, c.ci, c.v)
    with ops.GroupedBsr16(drp, dci, dv, mb=c.mb, group_rows=W) as grp:
        _rejected(c, grp, GROUPED_F16_REJECTED, n, np.random.default_rng(6))


# ------------------------------------------------ analysis outputs at offsets
def _analysis(ops, bs):
    return (ops.bsr32_analysis, ops.bsrmm_analysed) if bs == 32 else \
        (ops.bsr16_analysis, ops.bsrmm_analysed_f16)


def _analysed_tight(ops, c, bs, drp, dci, vcol, masks, alpha, beta):
    dB, dC = _dev(c.B, c.C0)
    _analysis(ops, bs)[1](drp, dci, vcol, masks, dB, mb=c.mb, kb=c.kb, n=c.n, ldb=c.n, C=dC,
                          ldc=c.n, alpha=alpha, beta=beta)
    return dC.cpu().numpy()


@pytest.mark.parametrize("voff_bytes", [16, "element"])
@pytest.mark.parametrize("bs", [32, 16])
def test_analysis_outputs_at_offsets(oracle, device, bs, voff_bytes):
    """spmm_bsr32_analysis_f32 / spmm_bsr16_analysis_f16 writing valCol and masks into a
    caller's arena: masks 4 bytes into a framed buffer, valCol 16 bytes in (the analysed
    stream: the bits of the run on fresh allocations) or one element in (4 bytes fp32,
    2 bytes fp16: the analysis stores single elements and the product loads them one at
    a time in the generic kernel, so the pair works, within the bar). Both outputs
    equal the fresh ones and every guard word around them is intact."""
    ops = _ops()
    c = _case(oracle, "an32" if bs == 32 else "an16", 136)
    alpha, beta = ABS[1]
    want64, scale = _expect(c.ref, c.absd, c.C0, alpha, beta)
    analyse = _analysis(ops, bs)[0]
    drp, dci, dv = _dev(c.rp, c.ci, c.v)
    masks0, vcol0 = analyse(dv, nnzb=c.nnzb)
    fresh = _analysed_tight(ops, c, bs, drp, dci, vcol0, masks0, alpha, beta)
    assert_normwise(fresh, want64, scale, c.tol, f"bs={bs} fresh allocations")
    nv = c.nnzb * bs * bs
    voff = 16 // c.v.dtype.itemsize if voff_bytes == 16 else 1
    fv, chkV = framed(np.zeros((1, nv), c.v.dtype), nv, voff)
    fm, chkM = framed(np.zeros((1, c.nnzb), np.int32), c.nnzb, 1, fill=0x5EADBEEF)
    assert fv.data_ptr() % 16 == (0 if voff_bytes == 16 else c.v.dtype.itemsize)
    analyse(dv, nnzb=c.nnzb, masks=fm[:c.nnzb], val_col=fv[:nv])
    got = _analysed_tight(ops, c, bs, drp, dci, fv[:nv], fm[:c.nnzb], alpha, beta)
    what = f"bs={bs} valCol + {voff_bytes} bytes, masks + 4 bytes"
    assert_normwise(got, want64, scale, c.tol, what)
    if voff_bytes == 16:
        assert _same_bits(got, fresh), what + ": bits differ from the run on fresh allocations"
    assert _same_bits(chkV(what + ": valCol")[0], vcol0.cpu().numpy()[:nv]), what + ": valCol"
    assert np.array_equal(chkM(what + ": masks")[0], masks0.cpu().numpy()[:c.nnzb]), what + ": masks"


def _group_abi(bs):
    from spmm_hip._lib import lib
    return (getattr(lib(), "spmm_bsr32_group_analysis_f32" if bs == 32 else
                    "spmm_bsr16_group_analysis_f16"),
            getattr(lib(), "spmm_bsrmm_grouped_f32" if bs == 32 else "spmm_bsrmm_grouped_f16"))


@pytest.mark.parametrize("bs", [32, 16])
def test_group_buffer_at_offsets(oracle, device, bs):
    """The group-analysis buffer inside a caller's arena. 4 bytes into it: INVALID_VALUE
    before any launch, the arena untouched (the kernels read the buffer's sections as
    16-byte vectors; include/spmm_hip.h). 16 bytes in: the analysis fills it with the
    bytes of an analysis into a fresh allocation, the product has that run's bits, and
    the arena around the buffer is untouched."""
    from ctypes import byref, c_size_t, c_void_p
    from spmm_hip._lib import INVALID_VALUE, lib
    ops = _ops()
    n = 136
    c = _case(oracle, "grp32" if bs == 32 else "grp16", n)
    alpha, beta = ABS[1]
    want64, scale = _expect(c.ref, c.absd, c.C0, alpha, beta)
    analysis, product = _group_abi(bs)
    drp, dci, dv = _dev(c.rp, c.ci, c.v)
    h = ops.Handle()
    args = (h.raw, ops.DIRECTION_ROW, c.mb, c.nnzb, 2, ops._ptr(drp), ops._ptr(dci), ops._ptr(dv))
    size = c_size_t(0)
    assert analysis(*args, None, byref(size)) == 0
    need, guard = size.value, 256
    arena = torch.full((guard + 16 + need + guard,), 0xA5, dtype=torch.uint8, device=device)
    assert arena.data_ptr() % 256 == 0
    before = arena.cpu()
    assert analysis(*args, c_void_p(arena.data_ptr() + guard + 4), byref(size)) == INVALID_VALUE
    torch.cuda.synchronize()
    assert torch.equal(arena.cpu(), before), "a rejected buffer was written to"
    buf = c_void_p(arena.data_ptr() + guard + 16)
    assert analysis(*args, buf, byref(size)) == 0
    dB, dC = _dev(c.B, c.C0)
    assert product(h.raw, c.mb, c.kb, n, buf, alpha, ops._ptr(dB), n, 0, beta, ops._ptr(dC), n, 0) == 0
    got = dC.cpu().numpy()
    assert_normwise(got, want64, scale, c.tol, f"bs={bs} buffer + 16 bytes")
    fresh_h = ops.Handle()
    cls = ops.GroupedBsr32 if bs == 32 else ops.GroupedBsr16
    with cls(drp, dci, dv, mb=c.mb, group_rows=2, handle=fresh_h) as fresh:
        dC2 = _dev(c.C0)[0]
        fresh.mm(dB, kb=c.kb, n=n, ldb=n, C=dC2, ldc=n, alpha=alpha, beta=beta)
        assert _same_bits(got, dC2.cpu().numpy()), "bits differ from the run on a fresh allocation"
        assert fresh.bytes == need
        after = arena.cpu()
        assert torch.equal(after[guard + 16:guard + 16 + need], fresh.buffer[:need].cpu())
    assert torch.equal(after[:guard + 16], before[:guard + 16]), "arena before the buffer"
    assert torch.equal(after[guard + 16 + need:], before[guard + 16 + need:]), "arena after the buffer"
    lib().spmm_bsr_group_release(h.raw, buf)
    h.close()
    fresh_h.close()


# ------------------------------------------ one handle, other work in between
def _other_work(oracle):
    """Three products that use the handle's shared buffers: a column-major CSR product
    (staged B and C in ws), the product of test_segments_with_staged_col_major_b (bs 32,
    a block row of 400 blocks: segment partials in scratch, staged B in ws, the row
    order in order) and a bs 2 product on the grouped small-block stream (probe sums
    and dirty flags in scratch, the group order in order). Returns run(handle) ->
    results; the first call also checks them against the f64 oracle."""
    if "other" not in _cache:
        rng = np.random.default_rng(99)
        w = _Case()
        w.m, w.k, w.n = 2000, 3000, 128
        deg = rng.integers(0, 30, w.m)
        w.crp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
        w.cci = np.concatenate([np.sort(rng.choice(w.k, d, replace=False)) for d in deg]).astype(np.int32)
        w.cv = rng.uniform(-1, 1, w.cci.size).astype(np.float32)
        w.cB = rng.uniform(-1, 1, (w.k, w.n)).astype(np.float32)
        w.cref = oracle_csrmm_f64(oracle, w.m, w.n, w.crp, w.cci, w.cv, w.cB, w.n, 0)
        w.smb, w.skb = 40, 400
        rp, ci, _ = rand_bsr(rng, w.smb, w.skb, 32, 0.008)
        rows = [ci[rp[i]:rp[i + 1]] for i in range(w.smb)]
        rows[5] = np.arange(w.skb, dtype=np.int32)
        w.srp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        w.sci = np.concatenate(rows).astype(np.int32)
        w.sv = rng.uniform(-1, 1, w.srp[-1] * 1024).astype(np.float32)
        w.sB = rng.uniform(-1, 1, (w.skb * 32, w.n)).astype(np.float32)
        w.sref = oracle_bsrmm_f64(oracle, 0, w.smb, w.n, 32, w.srp, w.sci, w.sv, w.sB, w.n, 0)
        w.tmb, w.tkb = 96, 80
        w.trp, w.tci, w.tv = rand_bsr(rng, w.tmb, w.tkb, 2, 0.2, empty_rows=(7,))
        w.tB = rng.uniform(-1, 1, (w.tkb * 2, w.n)).astype(np.float32)
        w.tref = oracle_bsrmm_f64(oracle, 0, w.tmb, w.n, 2, w.trp, w.tci, w.tv, w.tB, w.n, 0)
        _cache["other"] = w
    w = _cache["other"]
    ops = _ops()
    d = _dev(w.crp, w.cci, w.cv, np.ascontiguousarray(w.cB.T), w.srp, w.sci, w.sv,
             np.ascontiguousarray(w.sB.T), w.trp, w.tci, w.tv, w.tB)

    def run(h, check):
        from spmm_hip._lib import BSR_SMALL_GROUPED
        C1 = torch.full((w.n, w.m), float("nan"), device="cuda")
        ops.csrmm(d[0], d[1], d[2], d[3], m=w.m, n=w.n, k=w.k, ldb=w.k, order_b=1, C=C1, ldc=w.m,
                  order_c=1, handle=h)
        C2 = torch.full((w.smb * 32, w.n), float("nan"), device="cuda")
        ops.bsrmm(d[4], d[5], d[6], d[7], mb=w.smb, kb=w.skb, n=w.n, bs=32, ldb=w.skb * 32,
                  order_b=1, C=C2, ldc=w.n, handle=h)
        C3 = torch.full((w.tmb * 2, w.n), float("nan"), device="cuda")
        h.set_bsr_options(BSR_SMALL_GROUPED)
        ops.bsrmm(d[8], d[9], d[10], d[11], mb=w.tmb, kb=w.tkb, n=w.n, bs=2, ldb=w.n, C=C3,
                  ldc=w.n, handle=h)
        path = h.small_bsr_path()
        h.set_bsr_options(0)
        out = [C1.cpu().numpy().T, C2.cpu().numpy(), C3.cpu().numpy()]
        if check:
            assert path in (1, 2), "the bs 2 product did not take the grouped branch"
            for got, (ref, absd), nm in zip(out, (w.cref, w.sref, w.tref),
                                            ("column-major CSR", "segments + staged B", "bs 2 grouped")):
                assert_normwise(got, ref, absd, TOL_F32, nm)
        return out
    return run


@pytest.mark.parametrize("bs", [32, 16])
def test_group_analysis_shares_the_handle(oracle, device, bs):
    """The handle's ws, scratch, order, grp_pend and grp_cols serve every entry. Between
    the group analysis's size query and its filling call, and again between the filling
    call and the grouped product, one handle runs three products that use them; the
    filled buffer equals byte for byte an uninterrupted analysis on a fresh handle (its
    bytes are a function of the matrix alone, include/spmm_hip.h), C has that handle's
    bits, and the three products give the same bits before and after."""
    from ctypes import byref, c_size_t
    from spmm_hip._lib import lib
    ops = _ops()
    n = 136
    c = _case(oracle, "grp32" if bs == 32 else "grp16", n)
    alpha, beta = ABS[1]
    analysis, product = _group_abi(bs)
    drp, dci, dv = _dev(c.rp, c.ci, c.v)
    other = _other_work(oracle)
    h = ops.Handle()
    args = (h.raw, ops.DIRECTION_ROW, c.mb, c.nnzb, 4, ops._ptr(drp), ops._ptr(dci), ops._ptr(dv))
    size = c_size_t(0)
    assert analysis(*args, None, byref(size)) == 0
    first = other(h, True)
    buf = torch.empty(max(size.value, 1), dtype=torch.uint8, device=device)
    assert analysis(*args, ops._ptr(buf), byref(size)) == 0
    second = other(h, False)
    dB, dC = _dev(c.B, c.C0)
    assert product(h.raw, c.mb, c.kb, n, ops._ptr(buf), alpha, ops._ptr(dB), n, 0, beta,
                   ops._ptr(dC), n, 0) == 0
    got = dC.cpu().numpy()
    want64, scale = _expect(c.ref, c.absd, c.C0, alpha, beta)
    assert_normwise(got, want64, scale, c.tol, f"bs={bs} grouped product after other work")
    for a, b, nm in zip(first, second, ("column-major CSR", "segments + staged B", "bs 2 grouped")):
        assert _same_bits(a, b), nm + ": bits changed after the filling call"
    fresh_h = ops.Handle()
    cls = ops.GroupedBsr32 if bs == 32 else ops.GroupedBsr16
    with cls(drp, dci, dv, mb=c.mb, group_rows=4, handle=fresh_h) as fresh:
        assert fresh.bytes == size.value
        assert torch.equal(buf[:size.value], fresh.buffer[:fresh.bytes]), \
            "the interrupted analysis differs from an uninterrupted one"
        dC2 = _dev(c.C0)[0]
        fresh.mm(dB, kb=c.kb, n=n, ldb=n, C=dC2, ldc=n, alpha=alpha, beta=beta)
        assert _same_bits(got, dC2.cpu().numpy()), "C differs from the fresh handle's product"
    lib().spmm_bsr_group_release(h.raw, ops._ptr(buf))
    h.close()
    fresh_h.close()
