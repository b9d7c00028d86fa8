"""The fp16 / bf16-feature multi-head device entries (ops.sddmm_heads and ops.csrmm_heads on
float16 / bfloat16 features) = their host forms = the fp32 device entries on the widened
operands, bit for bit: aligned layouts, bases one and two elements past alignment (the
narrower load paths), odd leading dimensions, alpha / beta, base 1, views, every vector
width of the product, edge values, another grid, a second handle, a graph replay, no
allocation on a repeat, the Python refusals, and the kernels each case launches: together
every kernel heads_half_kernels.hip ships.

The operands are fp32 values rounded to the storage type (heads_half_cases), so no
comparison has a tolerance; the reference is never the new code."""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np
import pytest
import torch

import heads_cases as hc
import heads_half_cases as hh
import kernel_keys
import sddmm_cases as sd
from heads_cases import F

pytestmark = pytest.mark.gpu

TORCH_TYPE = {"f16": torch.float16, "bf16": torch.bfloat16}


def _ops():
    from spmm_hip import ops
    return ops


def _prep():
    from spmm_hip import prep
    return prep


def _dev(a, device="cuda", offset=0):
    """a on the device, `offset` elements past a 16-byte aligned base; a writable copy."""
    t = torch.from_numpy(np.array(a, order="C"))
    if offset == 0:
        return t.to(device)
    buf = torch.empty(t.numel() + offset + 8, dtype=t.dtype, device=device)
    assert buf.data_ptr() % 16 == 0
    out = buf[offset:offset + t.numel()].view(t.shape)
    out.copy_(t)
    return out


def _dev16(bits, ty, device="cuda", offset=0):
    """The patterns `bits` as a float16 / bfloat16 device tensor, `offset` elements (2 bytes
    each) past a 16-byte aligned base."""
    t = _dev(np.ascontiguousarray(bits, np.uint16).view(np.int16), device, offset)
    return t.view(TORCH_TYPE[ty])


def _np(t):
    return t.detach().cpu().numpy()


@contextlib.contextmanager
def _handle():
    h = _ops().Handle()
    try:
        yield h
    finally:
        torch.cuda.synchronize()
        h.close()


@contextlib.contextmanager
def _side_stream():
    """A non-blocking stream of the test's own, made and destroyed through the HIP runtime
    the library is linked against and wrapped for torch."""
    from spmm_hip._lib import lib
    hip = lib()
    create, destroy = hip.hipStreamCreateWithFlags, hip.hipStreamDestroy
    create.argtypes, create.restype = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint], ctypes.c_int
    destroy.argtypes, destroy.restype = [ctypes.c_void_p], ctypes.c_int
    raw = ctypes.c_void_p()
    assert create(ctypes.byref(raw), 1) == 0, "hipStreamCreateWithFlags"
    s = torch.cuda.ExternalStream(raw.value)
    s.wait_stream(torch.cuda.current_stream())
    try:
        yield s
    finally:
        s.synchronize()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        assert destroy(raw) == 0, "hipStreamDestroy"


def _vec_of(keys):
    """The last literal template argument of the one recorded kernel: VEC (an int for the
    product, a bool for the sampled product)."""
    (key,) = keys
    args = key[key.rindex("I"):]
    lit = args[args.rindex("L"):]
    return int(lit[2:lit.index("E")])


# ------------------------------------------------------------------ sampled product
@pytest.mark.parametrize("ty", hh.TYPES)
@pytest.mark.parametrize("heads,d", hc.SDDMM_HD + hc.SDDMM_HD_MORE)
@pytest.mark.parametrize("name", hc.SDDMM_PATTERNS)
def test_sddmm_heads_half(device, name, heads, d, ty):
    ops, prep = _ops(), _prep()
    m, k, rp, ci = sd.pattern(name)
    xb, yb, xw, yw = hh.sddmm_operands(m, k, heads, d, ty)
    w = heads * d
    want, want_epi = hh.sddmm_reference(name, heads, d, ty), hh.sddmm_reference(name, heads, d, ty,
                                                                                True)
    old = hc.sddmm_old(ci.size, heads)
    nan = np.full((ci.size, heads), np.nan, F)
    X, kw = hh.stored(xb, ty)
    hc.assert_same(prep.sddmm_heads(m, d, k, heads, rp, ci, X, hh.stored(yb, ty)[0],
                                    out=nan.copy(), **kw), want, f"{name} {heads}x{d} {ty} host")
    d_rp, d_ci = _dev(rp), _dev(ci)
    with _handle() as h:
        # the fp32 device entry on the widened operands
        f32 = ops.sddmm_heads(d_rp, d_ci, _dev(xw), _dev(yw), m=m, k=k, out=_dev(nan), handle=h)
        hc.assert_same(_np(f32), want, f"{name} {heads}x{d} {ty}: fp32 entry on widened")
        # aligned: 16-byte bases, ld = heads * d
        with h.launch_record() as rec:
            got = ops.sddmm_heads(d_rp, d_ci, _dev16(xb, ty), _dev16(yb, ty), m=m, k=k,
                                  out=_dev(nan), handle=h)
        hc.assert_same(_np(got), want, f"{name} {heads}x{d} {ty} aligned")
        if d > 0 and ci.size:
            assert _vec_of(rec) == (d % 4 == 0), (rec, "an aligned chunk is one 8-byte load")
        # bases one element (2 bytes) past alignment, odd leading dimensions; alpha / beta
        # on old values; base 1
        ldx, ldy = (w + 1) | 1, (w + 3) | 1
        bx, _ = hh.padded16(xb.reshape(m, w), ldx)
        by, _ = hh.padded16(yb.reshape(k, w), ldy)
        got = ops.sddmm_heads(_dev(rp + 1), _dev(ci + 1), _dev16(bx, ty, offset=1),
                              _dev16(by, ty, offset=1), m=m, d=d, heads=heads, k=k, ldx=ldx,
                              ldy=ldy, out=_dev(old), alpha=hc.ALPHA, beta=hc.BETA, base=1,
                              handle=h)
        hc.assert_same(_np(got), want_epi, f"{name} {heads}x{d} {ty} offset 1, alpha beta, base 1")
        # bases two elements past (4-byte, not 8-byte aligned), ld a multiple of 4: the
        # narrower loads, the same bits
        ld4 = w + 4
        bx, _ = hh.padded16(xb.reshape(m, w), ld4)
        by, _ = hh.padded16(yb.reshape(k, w), ld4)
        with h.launch_record() as rec:
            got = ops.sddmm_heads(d_rp, d_ci, _dev16(bx, ty, offset=2), _dev16(by, ty, offset=2),
                                  m=m, d=d, heads=heads, k=k, ldx=ld4, ldy=ld4, out=_dev(nan),
                                  handle=h)
        hc.assert_same(_np(got), want, f"{name} {heads}x{d} {ty} offset 2")
        if d > 0 and ci.size:
            assert _vec_of(rec) == 0, (rec, "a 4-byte aligned base must not take 8-byte loads")
        # aligned with padding that keeps the 8-byte loads, alpha / beta
        got = ops.sddmm_heads(d_rp, d_ci, _dev16(bx, ty), _dev16(by, ty), m=m, d=d, heads=heads,
                              k=k, ldx=ld4, ldy=ld4, out=_dev(old), alpha=hc.ALPHA, beta=hc.BETA,
                              handle=h)
        hc.assert_same(_np(got), want_epi, f"{name} {heads}x{d} {ty} ld + 4, alpha beta")


@pytest.mark.parametrize("ty", hh.TYPES)
def test_sddmm_heads_1_serves_the_single_head_case(device, ty):
    ops = _ops()
    m, k, rp, ci = sd.pattern("unsorted")
    for d in (5, 64, 260):
        xb, yb, xw, yw = hh.sddmm_operands(m, k, 1, d, ty)
        one = ops.sddmm(_dev(rp), _dev(ci), _dev(xw).view(m, d), _dev(yw).view(k, d), m=m, n=d, k=k)
        got = ops.sddmm_heads(_dev(rp), _dev(ci), _dev16(xb, ty), _dev16(yb, ty), m=m, k=k)
        hc.assert_same(_np(got), _np(one)[:, None], f"{ty} d={d}")


# ------------------------------------------------------------------ product
@pytest.mark.parametrize("ty", hh.TYPES)
@pytest.mark.parametrize("heads,d", hc.PRODUCT_HD)
def test_csrmm_heads_half(device, heads, d, ty):
    ops, prep = _ops(), _prep()
    m, k, rp, ci, val, bb, bw, C = hh.product_operands(heads, d, ty)
    w = heads * d
    want, want_epi = hh.product_reference(heads, d, ty), hh.product_reference(heads, d, ty, True)
    B, kw = hh.stored(bb, ty)
    hc.assert_same(prep.csrmm_heads(m, d, k, heads, rp, ci, val, B, **kw), want,
                   f"{heads}x{d} {ty} host")
    d_rp, d_ci, d_val = _dev(rp), _dev(ci), _dev(val)
    with _handle() as h:
        f32 = ops.csrmm_heads(d_rp, d_ci, d_val, _dev(bw), m=m, d=d, heads=heads, k=k, handle=h)
        hc.assert_same(_np(f32), want, f"{heads}x{d} {ty}: fp32 entry on widened")
        got = ops.csrmm_heads(d_rp, d_ci, d_val, _dev16(bb, ty), m=m, d=d, heads=heads, k=k,
                              handle=h)
        hc.assert_same(_np(got), want, f"{heads}x{d} {ty} aligned")
        # B one element past alignment, odd ldb / ldc (one column per lane); alpha / beta on
        # old C; base 1
        ldb, ldc = (w + 1) | 1, (w + 3) | 1
        pb, _ = hh.padded16(bb.reshape(k, w), ldb)
        cb, _ = hc.padded(C.reshape(m, w), ldc, fill=-7.25)
        dC = _dev(cb)
        with h.launch_record() as rec:
            ops.csrmm_heads(_dev(rp + 1), _dev(ci + 1), d_val, _dev16(pb, ty, offset=1), m=m, d=d,
                            heads=heads, k=k, ldb=ldb, C=dC, ldc=ldc, alpha=hc.ALPHA, beta=hc.BETA,
                            base=1, handle=h)
        assert _vec_of(rec) == 1, rec
        got = _np(dC).reshape(m, ldc)
        hc.assert_same(got[:, :w].reshape(m, heads, d), want_epi,
                       f"{heads}x{d} {ty} offset 1, padded, epilogue")
        assert (got[:, w:] == F(-7.25)).all(), "the padding of C was written"
        # B two elements past (4-byte, not 8-byte aligned), even padding: at most two columns
        # per lane; alpha / beta again
        ldb, ldc = w + 4, w + 8
        pb, _ = hh.padded16(bb.reshape(k, w), ldb)
        cb, _ = hc.padded(C.reshape(m, w), ldc, fill=-7.25)
        dC = _dev(cb)
        with h.launch_record() as rec:
            ops.csrmm_heads(d_rp, d_ci, d_val, _dev16(pb, ty, offset=2), m=m, d=d, heads=heads,
                            k=k, ldb=ldb, C=dC, ldc=ldc, alpha=hc.ALPHA, beta=hc.BETA, handle=h)
        assert _vec_of(rec) <= 2, (rec, "a 4-byte aligned B must not take 8-byte loads")
        got = _np(dC).reshape(m, ldc)
        hc.assert_same(got[:, :w].reshape(m, heads, d), want_epi,
                       f"{heads}x{d} {ty} offset 2, ld + 4, epilogue")
        assert (got[:, w:] == F(-7.25)).all(), "the padding of C was written"


@pytest.mark.parametrize("ty", hh.TYPES)
def test_csrmm_heads_half_on_a_rowptr_view(device, ty):
    ops = _ops()
    heads, d = 3, 5
    m, k, rp, ci, val, bb, _, _ = hh.product_operands(heads, d, ty)
    r0, r1 = 3, 30  # rows [3, 30): rowptr[0] > 0 and rowptr[m] < nnz, the full colind / val
    got = ops.csrmm_heads(_dev(rp[r0:r1 + 1]), _dev(ci), _dev(val), _dev16(bb, ty), m=r1 - r0,
                          d=d, heads=heads, k=k)
    hc.assert_same(_np(got), hh.product_reference(heads, d, ty)[r0:r1], f"{ty} rowptr view")


@pytest.mark.parametrize("ty", hh.TYPES)
def test_csrmm_every_vector_width_gives_the_same_bits(device, ty):
    """4 x 64 (256 columns: one tile at four columns per lane) at B aligned to 8, 4 and 2
    bytes: four, two and one column per lane, every row length of the pattern, one result."""
    ops = _ops()
    heads, d = 4, 64
    m, k, rp, ci, val, bb, _, _ = hh.product_operands(heads, d, ty)
    want = hh.product_reference(heads, d, ty)
    d_rp, d_ci, d_val = _dev(rp), _dev(ci), _dev(val)
    seen = {}
    with _handle() as h:
        for offset in (0, 2, 1):
            with h.launch_record() as rec:
                got = ops.csrmm_heads(d_rp, d_ci, d_val, _dev16(bb, ty, offset=offset), m=m, d=d,
                                      heads=heads, k=k, handle=h)
            hc.assert_same(_np(got), want, f"{ty} B {2 * offset} bytes past alignment")
            seen[offset] = _vec_of(rec)
    assert seen == {0: 4, 2: 2, 1: 1}, seen


# ------------------------------------------------------------------ edge values
@pytest.mark.parametrize("ty", hh.TYPES)
def test_edge_values_reach_their_outputs_with_the_f32_bits(device, ty):
    """As on the host: one edge pattern in one X, Y or B element; the device result has the
    bits of the fp32 host form on the widened arrays, the outputs that do not reference the
    element keep theirs, and inf / NaN make the ones that do non-finite."""
    ops, prep = _ops(), _prep()
    heads, d = 3, 5
    m, k, rp, ci = sd.pattern("random")
    xb, yb, _, _ = hh.sddmm_operands(m, k, heads, d, ty)
    base_e = hh.sddmm_reference("random", heads, d, ty)
    rows = np.repeat(np.arange(m), np.diff(np.asarray(rp, np.int64)))
    r, j = int(rows[ci.size // 2]), int(ci[ci.size // 2])
    pm, pk, prp, pci, val, bb, _, _ = hh.product_operands(heads, d, ty, True)
    base_c = hh.product_reference(heads, d, ty, False, True)
    prow = np.repeat(np.arange(pm), np.diff(np.asarray(prp, np.int64)))
    pj = int(pci[int(prp[8]) + 500])  # a column of the 1000-nonzero row
    d_rp, d_ci = _dev(rp), _dev(ci)
    d_prp, d_pci, d_val = _dev(prp), _dev(pci), _dev(val)
    for what, pat in hh.EDGE_BITS[ty]:
        x2, y2, b2 = xb.copy(), yb.copy(), bb.copy()
        x2[r, 1, 2] = pat
        y2[j, 2, 4] = pat
        b2[pj, 2, 3] = pat
        hit = np.zeros((ci.size, heads), bool)
        hit[rows == r, 1] = True
        hit[np.asarray(ci) == j, 2] = True
        got = _np(ops.sddmm_heads(d_rp, d_ci, _dev16(x2, ty), _dev16(y2, ty), m=m, k=k))
        want = prep.sddmm_heads(m, d, k, heads, rp, ci, hh.widen(x2, ty), hh.widen(y2, ty))
        hc.assert_same(got, want, f"sddmm {ty} {what}")
        hc.assert_same(got[~hit], base_e[~hit], f"sddmm {ty} {what}: other outputs")
        phit = np.zeros((pm, heads, d), bool)
        phit[np.unique(prow[np.asarray(pci) == pj]), 2, 3] = True
        gotc = _np(ops.csrmm_heads(d_prp, d_pci, d_val, _dev16(b2, ty), m=pm, d=d, heads=heads,
                                   k=pk))
        wantc = prep.csrmm_heads(pm, d, pk, heads, prp, pci, val, hh.widen(b2, ty))
        hc.assert_same(gotc, wantc, f"csrmm {ty} {what}")
        hc.assert_same(gotc[~phit], base_c[~phit], f"csrmm {ty} {what}: other outputs")
        if what in ("+inf", "-inf", "nan"):
            assert not np.isfinite(got[hit]).any() and not np.isfinite(gotc[phit]).any(), what


@pytest.mark.parametrize("ty", hh.TYPES)
def test_subnormals_are_kept(device, ty):
    """The smallest subnormal times 1.0 is itself, widened: nothing is flushed on the way;
    zeros keep the fp32 rule's signs."""
    ops, prep = _ops(), _prep()
    rp_h, ci_h = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32)
    rp, ci = _dev(rp_h), _dev(ci_h)
    one = int(hh.to_bits(np.array([1.0], F), ty)[0])
    tiny = F(2.0 ** -24 if ty == "f16" else 2.0 ** -133)
    Bb = np.array([[0x0001, 0x8001], [0x8000, 0x0000]], np.uint16).reshape(2, 1, 2)
    val = _dev(np.array([[1.0], [1.0]], F))
    C = _np(ops.csrmm_heads(rp, ci, val, _dev16(Bb, ty), m=2, d=2, heads=1, k=2)).reshape(2, 2)
    assert C[0, 0] == tiny and C[0, 1] == -tiny
    hc.assert_same(C, prep.csrmm_heads(2, 2, 2, 1, rp_h, ci_h, np.ones((2, 1), F),
                                       hh.widen(Bb, ty)).reshape(2, 2), f"{ty} zeros")
    Xb = np.array([[one, 0], [one, 0]], np.uint16).reshape(2, 1, 2)
    e = _np(ops.sddmm_heads(rp, ci, _dev16(Xb, ty), _dev16(Bb, ty), m=2, k=2))
    assert e[0, 0] == tiny


# ------------------------------------------------------------------ grids, handles, graphs
def _both_ops(h, ty):
    ops = _ops()
    m, k, rp, ci = sd.pattern("unsorted")
    xb, yb, _, _ = hh.sddmm_operands(m, k, 8, 8, ty)
    sdd = (_dev(rp), _dev(ci), _dev16(xb, ty), _dev16(yb, ty))
    pm, pk, prp, pci, val, bb, _, _ = hh.product_operands(8, 40, ty)
    prod = (_dev(prp), _dev(pci), _dev(val), _dev16(bb, ty))
    torch.cuda.synchronize()  # the operands are in place, whichever stream the handle is on
    out = [ops.sddmm_heads(*sdd, m=m, k=k, handle=h),
           ops.csrmm_heads(*prod, m=pm, d=40, heads=8, k=pk, handle=h)]
    torch.cuda.synchronize()
    return [_np(t) for t in out]


@pytest.mark.parametrize("ty", hh.TYPES)
def test_grid_and_handle_do_not_reach_the_bits(device, ty):
    ops = _ops()
    wants = [hh.sddmm_reference("unsorted", 8, 8, ty), hh.product_reference(8, 40, ty)]
    h = ops.Handle()
    try:
        for wv in (1, 32):  # the least and the most the handle takes
            h.set_csr_waves_per_cu(wv)
            for got, want in zip(_both_ops(h, ty), wants):
                hc.assert_same(got, want, f"{ty} {wv} waves per CU")
    finally:
        torch.cuda.synchronize()
        h.close()
    with _side_stream() as s:
        torch.cuda.synchronize()
        h2 = ops.Handle(stream=s)
        try:
            for got, want in zip(_both_ops(h2, ty), wants):
                hc.assert_same(got, want, f"{ty} a second handle on another stream")
        finally:
            torch.cuda.synchronize()
            h2.close()


@pytest.mark.parametrize("ty", hh.TYPES)
def test_graph_replay_equals_eager(device, ty):
    """Both entries captured once on a side stream after an eager call; replayed after the
    features were overwritten: the replay re-reads them and equals the eager call."""
    ops = _ops()
    rng = np.random.default_rng(17)
    m, k, rp, ci = sd.pattern("unsorted")
    heads, d = 4, 8
    nnz, n = ci.size, max(m, k)
    d_rp, d_ci = _dev(rp), _dev(ci)
    H = _dev16(hh.to_bits(rng.uniform(-1, 1, (n, heads, d)).astype(F), ty), ty)
    H2 = _dev16(hh.to_bits(rng.uniform(-1, 1, (n, heads, d)).astype(F), ty), ty)
    a = _dev(rng.uniform(0, 1, (nnz, heads)).astype(F))
    e = torch.zeros((nnz, heads), device=device)
    C = torch.zeros((m, heads, d), device=device)

    def run(h, e, C):
        ops.sddmm_heads(d_rp, d_ci, H, H, m=m, k=k, out=e, handle=h)
        ops.csrmm_heads(d_rp, d_ci, a, H, m=m, d=d, heads=heads, k=k, C=C, handle=h)

    torch.cuda.synchronize()
    with _side_stream() as s:
        h = ops.Handle(stream=s)
        run(h, e, C)
        torch.cuda.synchronize()
        first = [_np(t) for t in (e, C)]
        graph = torch.cuda.CUDAGraph()
        try:
            try:
                with torch.cuda.graph(graph, stream=s):
                    h.set_stream(s)
                    run(h, e, C)
            finally:
                h.set_stream(s)
            H.copy_(H2)
            for t in (e, C):
                t.fill_(0)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                graph.replay()
            torch.cuda.synchronize()
            got = [_np(t) for t in (e, C)]
            want = [torch.zeros_like(t) for t in (e, C)]
            run(h, *want)
            torch.cuda.synchronize()
            for g_, w_, f_ in zip(got, want, first):
                hc.assert_same(g_, _np(w_), f"{ty} replay")
                assert not np.array_equal(g_, f_)  # the new values were read
        finally:
            graph.reset()
            torch.cuda.synchronize()
            h.close()


@pytest.mark.parametrize("ty", hh.TYPES)
def test_repeat_allocates_nothing(device, ty):
    ops = _ops()
    m, k, rp, ci, val, bb, _, _ = hh.product_operands(4, 64, ty)
    d_rp, d_ci, d_val, d_B = _dev(rp), _dev(ci), _dev(val), _dev16(bb, ty)
    e = torch.empty_like(d_val)
    C = torch.empty((m, 4, 64), device=device)
    Bm = torch.rand((m, 4, 64), device=device).to(TORCH_TYPE[ty])
    h = ops.Handle()

    def run():
        ops.sddmm_heads(d_rp, d_ci, Bm, d_B, m=m, k=k, out=e, handle=h)
        ops.csrmm_heads(d_rp, d_ci, d_val, d_B, m=m, d=64, heads=4, k=k, C=C, handle=h)

    try:
        run()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
    finally:
        h.close()


# ------------------------------------------------------------------ checks
@pytest.mark.parametrize("ty", hh.TYPES)
def test_device_status_codes_equal_the_f32_entries(device, ty):
    from ctypes import c_void_p

    from spmm_hip._lib import INVALID_VALUE, NOT_INITIALIZED, NOT_SUPPORTED, SUCCESS, lib
    ops = _ops()
    L = lib()
    rp = _dev(np.array([0, 2], np.int32))
    ci = _dev(np.array([0, 1], np.int32))
    f = torch.zeros(4096, device=device)
    g = torch.zeros(4096, device=device, dtype=TORCH_TYPE[ty])
    o = torch.zeros(4096, device=device)
    h = ops.default_handle().raw
    P = lambda t: None if t is None else c_void_p(t.data_ptr())  # noqa: E731
    big = 1 << 30
    # (handle, m, d, k, nnz, heads, base, features given, ldx, ldy), expected
    sdd_cases = [
        ((None, 1, 4, 2, 2, 2, 0, True, 8, 8), NOT_INITIALIZED),
        ((h, 1, 4, 2, 2, 0, 0, True, 8, 8), INVALID_VALUE),       # heads < 1
        ((h, 1, 4, 2, 2, 2, 2, True, 8, 8), INVALID_VALUE),       # another base
        ((h, 1, 4, 2, 2, 2, 0, True, 7, 8), INVALID_VALUE),       # ldx < heads d
        ((h, 1, 4, 2, 2, 2, 0, False, 8, 8), INVALID_VALUE),      # X, Y NULL
        ((h, 1, 4, 2, 0, 2, 0, False, 8, 8), SUCCESS),            # nnz = 0
        ((h, 1, 4, 2, big, 4, 0, True, 16, 16), NOT_SUPPORTED),   # nnz heads > INT_MAX
        ((h, 1, 1025, 2, 2, 1, 0, True, 1025, 1025), NOT_SUPPORTED),  # d > 1024
        ((h, 1, 4, 2, 2, 2, 0, True, 8, 8), SUCCESS),
    ]
    half = getattr(L, "spmm_sddmm_csr_heads_" + ty)
    for (hd, m, d, k, nnz, heads, base, feats, ldx, ldy), want in sdd_cases:
        a = L.spmm_sddmm_csr_heads_f32(hd, m, d, k, nnz, heads, 1.0, P(rp), P(ci), base,
                                       P(f if feats else None), ldx, P(f if feats else None), ldy,
                                       0.0, P(o))
        b = half(hd, m, d, k, nnz, heads, 1.0, P(rp), P(ci), base, P(g if feats else None), ldx,
                 P(g if feats else None), ldy, 0.0, P(o))
        assert a == want and b == want, (ty, "sddmm", m, d, k, nnz, heads, a, b, want)
    # (handle, m, d, k, nnz, heads, base, B given, ldb, ldc), expected
    mm_cases = [
        ((None, 1, 4, 2, 2, 2, 0, True, 8, 8), NOT_INITIALIZED),
        ((h, 1, 4, 2, 2, 0, 0, True, 8, 8), INVALID_VALUE),       # heads < 1
        ((h, 0, 4, 2, 2, 2, 0, False, 8, 8), SUCCESS),            # m = 0
        ((h, 1, 0, 2, 2, 2, 0, False, 0, 0), SUCCESS),            # d = 0
        ((h, 1, 4, 2, 2, 2, 0, False, 8, 8), INVALID_VALUE),      # B NULL
        ((h, 1, 4, 2, 2, 2, 0, True, 7, 8), INVALID_VALUE),       # ldb < heads d
        ((h, 1, 4, 2, 2, 2, 0, True, 8, 7), INVALID_VALUE),       # ldc < heads d
        ((h, 1, 4, 2, big, 4, 0, True, 16, 16), NOT_SUPPORTED),   # nnz heads > INT_MAX
        ((h, 1, 65536, 2, 2, 64, 0, True, 1 << 22, 1 << 22), NOT_SUPPORTED),  # the grid's extent
        ((h, 1, 4, 2, 2, 2, 0, True, 8, 8), SUCCESS),
    ]
    half = getattr(L, "spmm_csrmm_heads_" + ty)
    for (hd, m, d, k, nnz, heads, base, Bg, ldb, ldc), want in mm_cases:
        a = L.spmm_csrmm_heads_f32(hd, m, d, k, nnz, heads, 1.0, P(rp), P(ci), P(f), base,
                                   P(f if Bg else None), ldb, 0.0, P(o), ldc)
        b = half(hd, m, d, k, nnz, heads, 1.0, P(rp), P(ci), P(f), base, P(g if Bg else None), ldb,
                 0.0, P(o), ldc)
        assert a == want and b == want, (ty, "csrmm", m, d, k, nnz, heads, a, b, want)
    torch.cuda.synchronize()


def test_python_wrappers_refuse_bad_operands(device):
    ops = _ops()
    m, k, rp, ci = sd.pattern("dups")
    xb, yb, xw, yw = hh.sddmm_operands(m, k, 2, 3, "f16")
    d_rp, d_ci = _dev(rp), _dev(ci)
    X16, Y16 = _dev16(xb, "f16"), _dev16(yb, "f16")
    Ybf = _dev16(yb, "bf16")
    e = torch.zeros((ci.size, 2), device=device)
    kw = dict(m=m, k=k)
    with pytest.raises(TypeError):
        ops.sddmm_heads(d_rp, d_ci, X16, Ybf, **kw)               # mixed half types
    with pytest.raises(TypeError):
        ops.sddmm_heads(d_rp, d_ci, X16, _dev(yw), **kw)          # half and fp32
    with pytest.raises(TypeError):
        ops.sddmm_heads(d_rp, d_ci, _dev(xw), Y16, **kw)
    with pytest.raises(TypeError):
        ops.sddmm_heads(d_rp, d_ci, X16, Y16, out=e.half(), **kw)  # a half out
    with pytest.raises(TypeError):
        ops.sddmm_heads(d_rp, d_ci, X16.double(), Y16.double(), **kw)  # float64
    with pytest.raises(TypeError):
        ops.sddmm_heads(d_rp, d_ci, X16.cpu(), Y16.cpu(), **kw)   # CPU tensors
    with pytest.raises(TypeError):
        ops.csrmm_heads(d_rp, d_ci, e.half(), Y16, d=3, heads=2, **kw)  # a half val
    with pytest.raises(TypeError):
        ops.csrmm_heads(d_rp, d_ci, e.bfloat16(), Ybf, d=3, heads=2, **kw)
    with pytest.raises(TypeError):
        ops.csrmm_heads(d_rp, d_ci, e, Y16, d=3, heads=2,
                        C=torch.zeros((m, 2, 3), device=device, dtype=torch.float16), **kw)
    with pytest.raises(TypeError):
        ops.csrmm_heads(d_rp, d_ci, e, Y16.double(), d=3, heads=2, **kw)  # float64
    with pytest.raises(TypeError):
        ops.csrmm_heads(d_rp, d_ci, e, Y16.cpu(), d=3, heads=2, **kw)     # a CPU tensor
    with pytest.raises(ValueError):
        ops.sddmm_heads(d_rp, d_ci, X16[:-1], Y16, heads=2, d=3, **kw)    # too short


# ------------------------------------------------------------------ kernel coverage
def test_kernel_coverage(device):
    """One launch per call, and the union over the shapes of the tests above (the sampled
    product aligned and misaligned at every lane-group width, the product's widths), for
    both types, is every kernel heads_half_kernels.hip ships. d = 0 is the fp32 file's fill
    kernel: it reads no features."""
    ops = _ops()
    shipped = {kernel_keys.launch_key(k)
               for k in kernel_keys.shipped_kernels(("heads_half_kernels",))}
    print(f"heads_half_kernels.hip ships {len(shipped)} kernels")
    zero = {kernel_keys.launch_key(k) for k in kernel_keys.shipped_kernels(("heads_kernels",))
            if "sddmm_heads_zero_kernel" in k}
    assert len(zero) == 1
    seen = set()

    def one(keys, what):
        assert len(keys) == 1, (what, keys)
        seen.update(keys)

    with _handle() as h:
        m, k, rp, ci = sd.pattern("dups")
        d_rp, d_ci = _dev(rp), _dev(ci)
        for ty in hh.TYPES:
            for heads, d in hc.SDDMM_HD + hc.SDDMM_HD_MORE:
                xb, yb, _, _ = hh.sddmm_operands(m, k, heads, d, ty)
                w = heads * d
                with h.launch_record() as rec:
                    ops.sddmm_heads(d_rp, d_ci, _dev16(xb, ty), _dev16(yb, ty), m=m, k=k, handle=h)
                one(rec, f"sddmm {ty} {heads}x{d}")
                bx, _ = hh.padded16(xb.reshape(m, w), w + 1)
                by, _ = hh.padded16(yb.reshape(k, w), w + 1)
                with h.launch_record() as rec:
                    ops.sddmm_heads(d_rp, d_ci, _dev16(bx, ty, offset=1), _dev16(by, ty, offset=1),
                                    m=m, d=d, heads=heads, k=k, ldx=w + 1, ldy=w + 1, handle=h)
                one(rec, f"sddmm {ty} {heads}x{d} misaligned")
            for heads, d in hc.PRODUCT_HD:
                pm, pk, prp, pci, val, bb, _, _ = hh.product_operands(heads, d, ty)
                with h.launch_record() as rec:
                    ops.csrmm_heads(_dev(prp), _dev(pci), _dev(val), _dev16(bb, ty), m=pm, d=d,
                                    heads=heads, k=pk, handle=h)
                one(rec, f"product {ty} {heads}x{d}")
    assert seen - zero == shipped, (f"never launched: {sorted(shipped - seen)}; "
                                    f"unknown: {sorted(seen - zero - shipped)}")
    assert zero <= seen  # d = 0 went to the fill kernel
