"""The multi-head device entries (ops.sddmm_heads, edge_softmax_heads,
edge_softmax_bwd_heads, csrmm_heads) = their host forms = the restated single-head rules
applied per head (heads_cases), bit for bit: aligned and misaligned layouts, alpha / beta,
base 1, views, in place, edge values, another grid, a second handle, a graph replay, no
allocation on a repeat, the new refusals, and the kernels each case launches: together
every kernel heads_kernels.hip ships."""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np
import pytest
import torch

import edge_cases as ec
import heads_cases as hc
import kernel_keys
import sddmm_cases as sd
import softmax_cases as sc
from heads_cases import F

pytestmark = pytest.mark.gpu


def _ops():
    from spmm_hip import ops
    return ops


def _prep():
    from spmm_hip import prep
    return prep


def _dev(a, device="cuda", offset=0):
    """a on the device, `offset` floats past a 16-byte aligned base; a writable copy."""
    t = torch.from_numpy(np.array(a, order="C"))
    if offset == 0:
        return t.to(device)
    buf = torch.empty(t.numel() + offset + 4, dtype=t.dtype, device=device)
    assert buf.data_ptr() % 16 == 0
    out = buf[offset:offset + t.numel()].view(t.shape)
    out.copy_(t)
    return out


def _np(t):
    return t.detach().cpu().numpy()


@contextlib.contextmanager
def _handle():
    """A handle of the test's own, closed behind a device synchronisation."""
    h = _ops().Handle()
    try:
        yield h
    finally:
        torch.cuda.synchronize()
        h.close()


@contextlib.contextmanager
def _side_stream():
    """A non-blocking stream of the test's own, made and destroyed through the HIP runtime the
    library is linked against and wrapped for torch (a torch.cuda.Stream() would come from
    torch's pool and never go back). Gone, queue reference included, when the block ends."""
    from spmm_hip._lib import lib
    hip = lib()
    create, destroy = hip.hipStreamCreateWithFlags, hip.hipStreamDestroy
    create.argtypes, create.restype = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint], ctypes.c_int
    destroy.argtypes, destroy.restype = [ctypes.c_void_p], ctypes.c_int
    raw = ctypes.c_void_p()
    assert create(ctypes.byref(raw), 1) == 0, "hipStreamCreateWithFlags"  # hipStreamNonBlocking
    s = torch.cuda.ExternalStream(raw.value)
    s.wait_stream(torch.cuda.current_stream())
    try:
        yield s
    finally:
        s.synchronize()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        assert destroy(raw) == 0, "hipStreamDestroy"


# ------------------------------------------------------------------ sampled product
@pytest.mark.parametrize("heads,d", hc.SDDMM_HD + hc.SDDMM_HD_MORE)
@pytest.mark.parametrize("name", hc.SDDMM_PATTERNS)
def test_sddmm_heads(device, name, heads, d):
    ops, prep = _ops(), _prep()
    m, k, rp, ci = sd.pattern(name)
    X, Y = hc.sddmm_operands(m, k, heads, d)
    w = heads * d
    want, want_epi = hc.sddmm_reference(name, heads, d), hc.sddmm_reference(name, heads, d, True)
    old = hc.sddmm_old(ci.size, heads)
    nan = np.full((ci.size, heads), np.nan, F)
    hc.assert_same(prep.sddmm_heads(m, d, k, heads, rp, ci, X, Y, out=nan.copy()), want,
                   f"{name} {heads}x{d} host")
    d_rp, d_ci = _dev(rp), _dev(ci)
    with _handle() as h:
        # aligned: 16-byte bases, ld = heads * d
        got = ops.sddmm_heads(d_rp, d_ci, _dev(X), _dev(Y), m=m, k=k, out=_dev(nan), handle=h)
        hc.assert_same(_np(got), want, f"{name} {heads}x{d} aligned")
        # misaligned: bases one float past 16 bytes, odd leading dimensions; alpha / beta on
        # old values; base 1
        ldx, ldy = (w + 1) | 1, (w + 3) | 1
        bx, _ = hc.padded(X.reshape(m, w), ldx)
        by, _ = hc.padded(Y.reshape(k, w), ldy)
        got = ops.sddmm_heads(_dev(rp + 1), _dev(ci + 1), _dev(bx, offset=1), _dev(by, offset=1),
                              m=m, d=d, heads=heads, k=k, ldx=ldx, ldy=ldy, out=_dev(old),
                              alpha=hc.ALPHA, beta=hc.BETA, base=1, handle=h)
        hc.assert_same(_np(got), want_epi, f"{name} {heads}x{d} misaligned, alpha beta, base 1")
        # aligned with alpha / beta, a new out by default
        got = ops.sddmm_heads(d_rp, d_ci, _dev(X), _dev(Y), m=m, k=k, out=_dev(old),
                              alpha=hc.ALPHA, beta=hc.BETA, handle=h)
        hc.assert_same(_np(got), want_epi, f"{name} {heads}x{d} aligned, alpha beta")
        assert ops.sddmm_heads(d_rp, d_ci, _dev(X), _dev(Y), m=m, k=k, handle=h).shape == \
            (ci.size, heads)


def test_sddmm_heads_1_equals_the_single_head_entry(device):
    ops = _ops()
    m, k, rp, ci = sd.pattern("unsorted")
    for d in (5, 64, 260):
        X, Y = hc.sddmm_operands(m, k, 1, d)
        args = (_dev(rp), _dev(ci), _dev(X), _dev(Y))
        one = ops.sddmm(args[0], args[1], args[2].view(m, d), args[3].view(k, d), m=m, n=d, k=k)
        hc.assert_same(_np(ops.sddmm_heads(*args, m=m, k=k)), _np(one)[:, None], f"d={d}")


# ------------------------------------------------------------------ edge softmax
def _softmax_run(c, name, heads, device, handle=None, offset=0, in_place=False):
    ops = _ops()
    x, g = hc.softmax_inputs(name, heads)
    yin = hc.softmax_forward(name, heads)
    rp = _dev(c.rowptr, device)
    dx, dg = _dev(x, device, offset), _dev(g, device, offset)
    if in_place:
        y, gx = dx, dg
    else:
        y, gx = (_dev(np.full(x.shape, -7.25, F), device, offset) for _ in range(2))
    torch.cuda.synchronize()
    assert ops.edge_softmax_heads(rp, dx, base=c.base, out=y, handle=handle) is y
    ops.edge_softmax_bwd_heads(rp, _dev(yin, device, offset), dg, base=c.base, out=gx,
                               handle=handle)
    torch.cuda.synchronize()
    return _np(y), _np(gx)


def _softmax_hold(c, name, heads, y, gx, where, outside=(F(-7.25), F(-7.25))):
    mk = sc.inside(c)
    hc.assert_same(y[mk], hc.softmax_forward(name, heads)[mk], f"{name} x{heads} {where} forward")
    hc.assert_same(gx[mk], hc.softmax_backward(name, heads)[mk],
                   f"{name} x{heads} {where} backward")
    for got, keep in zip((y, gx), outside):
        assert np.array_equal(got[~mk].view(np.uint32),
                              np.broadcast_to(keep, got.shape)[~mk].view(np.uint32)), \
            f"{name} x{heads} {where}: outside the view"


@pytest.mark.parametrize("heads", hc.SOFTMAX_HEADS)
@pytest.mark.parametrize("name", hc.SOFTMAX_PATTERNS)
def test_edge_softmax_heads(device, name, heads):
    prep = _prep()
    c = sc.case(name)
    x, g = hc.softmax_inputs(name, heads)
    mk = sc.inside(c)
    hc.assert_same(prep.edge_softmax_heads(c.rowptr, x, base=c.base)[mk],
                   hc.softmax_forward(name, heads)[mk], f"{name} x{heads} host")
    hc.assert_same(prep.edge_softmax_bwd_heads(c.rowptr, hc.softmax_forward(name, heads), g,
                                               base=c.base)[mk],
                   hc.softmax_backward(name, heads)[mk], f"{name} x{heads} host backward")
    with _handle() as h:
        _softmax_hold(c, name, heads, *_softmax_run(c, name, heads, device, h), "aligned")
        _softmax_hold(c, name, heads, *_softmax_run(c, name, heads, device, h, offset=1),
                      "one float past a 16-byte base")
        y, gx = _softmax_run(c, name, heads, device, h, in_place=True)
        _softmax_hold(c, name, heads, y, gx, "in place", outside=(x, g))


def test_a_non_finite_row_leaves_the_other_heads_alone(device):
    """"special" is non-finite in different rows from head to head: where a row is finite
    in one head and not in another, the finite head's outputs are finite and keep the
    bits of the rule on that column alone."""
    c = sc.case("special")
    heads = 3
    y, gx = _softmax_run(c, "special", heads, device)
    seen = 0
    for r, a, L in c.rows():
        kinds = [hc.special_kind(r, h) for h in range(heads)]
        for h in range(heads):
            if kinds[h] in (0, 4) and any(kd in (1, 2, 3) for kd in kinds) and L > 1:
                assert np.isfinite(y[a:a + L, h]).all(), (r, h)
                hc.assert_same(y[a:a + L, h], hc.softmax_column_forward("special", h)[a:a + L],
                               f"row {r} head {h}")
                hc.assert_same(gx[a:a + L, h], hc.softmax_column_backward("special", h)[a:a + L],
                               f"row {r} head {h} backward")
                seen += 1
    assert seen >= 8


def test_edge_softmax_heads_1_equals_the_single_head_entry(device):
    ops = _ops()
    for name in ("lengths", "short_mixed"):
        c = sc.case(name)
        x, g = hc.softmax_inputs(name, 1)
        rp, dx, dg = _dev(c.rowptr), _dev(x), _dev(g)
        y = ops.edge_softmax_heads(rp, dx)
        y1 = ops.edge_softmax(rp, dx.view(-1))
        hc.assert_same(_np(y)[:, 0], _np(y1), name)
        hc.assert_same(_np(ops.edge_softmax_bwd_heads(rp, y, dg))[:, 0],
                       _np(ops.edge_softmax_bwd(rp, y1, dg.view(-1))), name + " backward")


# ------------------------------------------------------------------ product
def _product_args(heads, d, device):
    m, k, rp, ci = hc.product_pattern()
    val, B, C = hc.product_operands(ci.size, k, m, heads, d)
    return m, k, rp, ci, val, B, C


@pytest.mark.parametrize("heads,d", hc.PRODUCT_HD)
def test_csrmm_heads(device, heads, d):
    ops, prep = _ops(), _prep()
    m, k, rp, ci, val, B, C = _product_args(heads, d, device)
    w = heads * d
    want, want_epi = hc.product_reference(heads, d), hc.product_reference(heads, d, True)
    hc.assert_same(prep.csrmm_heads(m, d, k, heads, rp, ci, val, B), want, f"{heads}x{d} host")
    d_rp, d_ci, d_val, d_B = _dev(rp), _dev(ci), _dev(val), _dev(B)
    with _handle() as h:
        got = ops.csrmm_heads(d_rp, d_ci, d_val, d_B, m=m, d=d, heads=heads, k=k, handle=h)
        hc.assert_same(_np(got), want, f"{heads}x{d}")
        # alpha / beta on old C, padded ldb / ldc (odd: one dword per lane), base 1
        ldb, ldc = (w + 1) | 1, (w + 3) | 1
        bb, _ = hc.padded(B.reshape(k, w), ldb)
        cb, _ = hc.padded(C.reshape(m, w), ldc, fill=-7.25)
        dC = _dev(cb)
        ops.csrmm_heads(_dev(rp + 1), _dev(ci + 1), d_val, _dev(bb), m=m, d=d, heads=heads, k=k,
                        ldb=ldb, C=dC, ldc=ldc, alpha=hc.ALPHA, beta=hc.BETA, base=1, handle=h)
        got = _np(dC).reshape(m, ldc)
        hc.assert_same(got[:, :w].reshape(m, heads, d), want_epi, f"{heads}x{d} padded, epilogue")
        assert (got[:, w:] == F(-7.25)).all(), "the padding of C was written"
        # even padding keeps the wide lanes: alpha / beta again
        ldb, ldc = w + 4, w + 8
        bb, _ = hc.padded(B.reshape(k, w), ldb)
        cb, _ = hc.padded(C.reshape(m, w), ldc, fill=-7.25)
        dC = _dev(cb)
        ops.csrmm_heads(d_rp, d_ci, d_val, _dev(bb), m=m, d=d, heads=heads, k=k, ldb=ldb, C=dC,
                        ldc=ldc, alpha=hc.ALPHA, beta=hc.BETA, handle=h)
        got = _np(dC).reshape(m, ldc)
        hc.assert_same(got[:, :w].reshape(m, heads, d), want_epi, f"{heads}x{d} ld + 4, epilogue")
        assert (got[:, w:] == F(-7.25)).all(), "the padding of C was written"


@pytest.mark.parametrize("heads,d", hc.PRODUCT_HD)
def test_csrmm_heads_equals_csrmm_per_head_under_sequential_rows(device, heads, d):
    from spmm_hip._lib import CSR_NT_STREAMS, CSR_SEQUENTIAL_ROWS
    ops = _ops()
    m, k, rp, ci, val, B, _ = _product_args(heads, d, device)
    d_rp, d_ci = _dev(rp), _dev(ci)
    got = _np(ops.csrmm_heads(d_rp, d_ci, _dev(val), _dev(B), m=m, d=d, heads=heads, k=k))
    h = ops.Handle()
    try:
        h.set_csr_options(CSR_NT_STREAMS | CSR_SEQUENTIAL_ROWS)
        for hd in range(heads):
            Ch = torch.empty((m, d), dtype=torch.float32, device=device)
            ops.csrmm(d_rp, d_ci, _dev(val[:, hd]), _dev(B[:, hd, :]), m=m, n=d, k=k, ldb=d, C=Ch,
                      ldc=d, handle=h)
            hc.assert_same(got[:, hd, :], _np(Ch), f"{heads}x{d} head {hd}")
    finally:
        torch.cuda.synchronize()
        h.close()


def test_csrmm_heads_non_finite_values_reach_their_outputs_only(device):
    """One NaN and one inf in a single val[p, h], and in a single B[j, c]: exactly the
    outputs that reference them are non-finite, every other output keeps its bits."""
    ops = _ops()
    heads, d = 3, 5
    m, k, rp, ci, val, B, _ = _product_args(heads, d, device)
    want = hc.product_reference(heads, d)
    rows = np.repeat(np.arange(m), np.diff(rp))
    for bad in (np.nan, np.inf):
        # val[p, h]: row(p), head h, every column of that head
        p, hd = int(rp[8]) + 500, 1  # inside the 1000-nonzero row
        v2 = val.copy()
        v2[p, hd] = bad
        got = _np(ops.csrmm_heads(_dev(rp), _dev(ci), _dev(v2), _dev(B), m=m, d=d, heads=heads,
                                  k=k))
        hit = np.zeros((m, heads, d), bool)
        hit[rows[p], hd, :] = True
        assert not np.isfinite(got[hit]).any() and np.isfinite(got[~hit]).all(), bad
        hc.assert_same(got[~hit], want[~hit], f"val {bad}")
        # B[j, h, c]: the rows that hold column j, that head and column alone
        j, hd, c = int(ci[p]), 2, 3
        B2 = B.copy()
        B2[j, hd, c] = bad
        got = _np(ops.csrmm_heads(_dev(rp), _dev(ci), _dev(val), _dev(B2), m=m, d=d, heads=heads,
                                  k=k))
        hit = np.zeros((m, heads, d), bool)
        hit[np.unique(rows[ci == j]), hd, c] = True
        assert hit.sum() >= 2
        assert not np.isfinite(got[hit]).any() and np.isfinite(got[~hit]).all(), bad
        hc.assert_same(got[~hit], want[~hit], f"B {bad}")


@pytest.mark.parametrize("cls", ["S", "Z"])
def test_csrmm_heads_edge_classes(device, cls):
    """Subnormals (S) and signed zeros (Z) of tests/edge_cases.py: every head carries the
    class's case at width 8, so each head's slice is the class's order-free output."""
    ops = _ops()
    heads, d = 2, 8
    c = ec.csr_case(cls, d)
    wants = ec.csr_wants(cls, d)
    m, k = c["m"], c["k"]
    val = np.repeat(c["val"][:, None], heads, axis=1)
    B = np.repeat(c["B"][:, None, :], heads, axis=1)
    C0 = np.repeat(c["C0"].reshape(m, 1, d), heads, axis=1)
    for (alpha, beta), want in wants.items():
        dC = _dev(C0)
        ops.csrmm_heads(_dev(c["rp"]), _dev(c["ci"]), _dev(val), _dev(B), m=m, d=d, heads=heads,
                        k=k, C=dC, alpha=alpha, beta=beta)
        got = _np(dC)
        for hd in range(heads):
            ec.assert_bits(got[:, hd, :], want.reshape(m, d), f"class {cls} head {hd} "
                           f"alpha={alpha} beta={beta}")


# ------------------------------------------------------------------ all three
def _all_ops(h, device):
    """One call of each entry on `h` -> the outputs as numpy."""
    ops = _ops()
    m, k, rp, ci = sd.pattern("unsorted")
    X, Y = hc.sddmm_operands(m, k, 8, 8)
    sdd = (_dev(rp), _dev(ci), _dev(X), _dev(Y))
    c = sc.case("mid")
    x, g = hc.softmax_inputs("mid", 3)
    rpd, dx, dg, dy = _dev(c.rowptr), _dev(x), _dev(g), _dev(hc.softmax_forward("mid", 3))
    pm, pk, prp, pci, val, B, _ = _product_args(8, 40, device)
    prod = (_dev(prp), _dev(pci), _dev(val), _dev(B))
    torch.cuda.synchronize()  # the operands are in place, whichever stream the handle is on
    out = [ops.sddmm_heads(*sdd, m=m, k=k, handle=h),
           ops.edge_softmax_heads(rpd, dx, handle=h),
           ops.edge_softmax_bwd_heads(rpd, dy, dg, handle=h),
           ops.csrmm_heads(*prod, m=pm, d=40, heads=8, k=pk, handle=h)]
    torch.cuda.synchronize()
    return [_np(t) for t in out]


def _all_wants():
    return [hc.sddmm_reference("unsorted", 8, 8), hc.softmax_forward("mid", 3),
            hc.softmax_backward("mid", 3), hc.product_reference(8, 40)]


def test_grid_and_handle_do_not_reach_the_bits(device):
    ops = _ops()
    h = ops.Handle()
    try:
        for wv in (1, 7):
            h.set_csr_waves_per_cu(wv)
            for got, want in zip(_all_ops(h, device), _all_wants()):
                hc.assert_same(got, want, f"{wv} waves per CU")
    finally:
        torch.cuda.synchronize()
        h.close()
    with _side_stream() as s:
        torch.cuda.synchronize()
        h2 = ops.Handle(stream=s)
        try:
            for got, want in zip(_all_ops(h2, device), _all_wants()):
                hc.assert_same(got, want, "a second handle on another stream")
        finally:
            torch.cuda.synchronize()
            h2.close()


def test_graph_replay_equals_eager(device):
    """Each entry captured once on a side stream after an eager call; replayed after the
    inputs were overwritten: the replay re-reads them and equals the eager call."""
    ops = _ops()
    rng = np.random.default_rng(17)
    m, k, rp, ci = sd.pattern("unsorted")
    heads, d = 4, 8
    nnz = ci.size
    d_rp, d_ci = _dev(rp), _dev(ci)
    H = _dev(rng.uniform(-1, 1, (max(m, k), heads, d)).astype(F))
    H2 = torch.from_numpy(rng.uniform(-1, 1, (max(m, k), heads, d)).astype(F))
    e, a, ga = (torch.zeros((nnz, heads), device=device) for _ in range(3))
    C = torch.zeros((m, heads, d), device=device)

    def run(h, e, a, ga, C):
        ops.sddmm_heads(d_rp, d_ci, H, H, m=m, k=k, out=e, handle=h)
        ops.edge_softmax_heads(d_rp, e, m=m, out=a, handle=h)
        ops.edge_softmax_bwd_heads(d_rp, a, e, m=m, out=ga, handle=h)
        ops.csrmm_heads(d_rp, d_ci, a, H, m=m, d=d, heads=heads, k=k, C=C, handle=h)

    torch.cuda.synchronize()
    with _side_stream() as s:
        h = ops.Handle(stream=s)
        run(h, e, a, ga, C)
        torch.cuda.synchronize()
        first = [_np(t) for t in (e, a, ga, C)]
        graph = torch.cuda.CUDAGraph()
        try:
            try:
                with torch.cuda.graph(graph, stream=s):
                    h.set_stream(s)
                    run(h, e, a, ga, C)
            finally:
                h.set_stream(s)
            H.copy_(H2)
            for t in (e, a, ga, C):
                t.fill_(0)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                graph.replay()
            torch.cuda.synchronize()
            got = [_np(t) for t in (e, a, ga, C)]
            want = [torch.zeros_like(t) for t in (e, a, ga, C)]
            run(h, *want)
            torch.cuda.synchronize()
            for g_, w_, f_ in zip(got, want, first):
                hc.assert_same(g_, _np(w_), "replay")
                assert not np.array_equal(g_, f_)  # the new values were read
        finally:
            graph.reset()
            torch.cuda.synchronize()
            h.close()


def test_repeat_allocates_nothing(device):
    ops = _ops()
    m, k, rp, ci, val, B, _ = _product_args(4, 64, device)
    d_rp, d_ci, d_val, d_B = _dev(rp), _dev(ci), _dev(val), _dev(B)
    e, y, gx = (torch.empty_like(d_val) for _ in range(3))
    C = torch.empty((m, 4, 64), device=device)
    Bm = torch.rand((m, 4, 64), device=device)
    h = ops.Handle()

    def run():
        ops.sddmm_heads(d_rp, d_ci, Bm, d_B, m=m, k=k, out=e, handle=h)
        ops.edge_softmax_heads(d_rp, e, out=y, handle=h)
        ops.edge_softmax_bwd_heads(d_rp, y, d_val, out=gx, handle=h)
        ops.csrmm_heads(d_rp, d_ci, y, d_B, m=m, d=64, heads=4, k=k, C=C, handle=h)

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


def test_device_status_codes(device):
    from ctypes import c_void_p

    from spmm_hip._lib import INVALID_VALUE, NOT_INITIALIZED, NOT_SUPPORTED, SUCCESS, lib
    ops = _ops()
    L = lib()
    rp = _dev(np.array([0, 2], np.int32))
    ci = _dev(np.array([0, 1], np.int32))
    f = torch.zeros(4096, device=device)
    h = ops.default_handle().raw
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    sdd, sm = L.spmm_sddmm_csr_heads_f32, L.spmm_edge_softmax_csr_heads_f32
    smb, mm = L.spmm_edge_softmax_bwd_csr_heads_f32, L.spmm_csrmm_heads_f32
    big = 1 << 30
    assert sdd(None, 1, 4, 2, 2, 2, 1.0, P(rp), P(ci), 0, P(f), 8, P(f), 8, 0.0, P(f)) == NOT_INITIALIZED
    assert sm(None, 1, 2, 2, P(rp), 0, P(f), P(f)) == NOT_INITIALIZED
    assert smb(None, 1, 2, 2, P(rp), 0, P(f), P(f), P(f)) == NOT_INITIALIZED
    assert mm(None, 1, 4, 2, 2, 2, 1.0, P(rp), P(ci), P(f), 0, P(f), 8, 0.0, P(f), 8) == NOT_INITIALIZED
    # heads < 1
    assert sdd(h, 1, 4, 2, 2, 0, 1.0, P(rp), P(ci), 0, P(f), 8, P(f), 8, 0.0, P(f)) == INVALID_VALUE
    assert sm(h, 1, 2, 0, P(rp), 0, P(f), P(f)) == INVALID_VALUE
    assert smb(h, 1, 2, -3, P(rp), 0, P(f), P(f), P(f)) == INVALID_VALUE
    assert mm(h, 1, 4, 2, 2, 0, 1.0, P(rp), P(ci), P(f), 0, P(f), 8, 0.0, P(f), 8) == INVALID_VALUE
    # ld below heads * d, another base, a NULL pointer
    assert sdd(h, 1, 4, 2, 2, 2, 1.0, P(rp), P(ci), 0, P(f), 7, P(f), 8, 0.0, P(f)) == INVALID_VALUE
    assert mm(h, 1, 4, 2, 2, 2, 1.0, P(rp), P(ci), P(f), 0, P(f), 8, 0.0, P(f), 7) == INVALID_VALUE
    assert sm(h, 1, 2, 2, P(rp), 2, P(f), P(f)) == INVALID_VALUE
    assert smb(h, 1, 2, 2, P(rp), 0, P(f), None, P(f)) == INVALID_VALUE
    # nnz * heads past INT_MAX and d past 1024: refused before anything is queued
    assert sdd(h, 1, 4, 2, big, 4, 1.0, P(rp), P(ci), 0, P(f), 16, P(f), 16, 0.0, P(f)) == NOT_SUPPORTED
    assert sdd(h, 1, 1025, 2, 2, 1, 1.0, P(rp), P(ci), 0, P(f), 1025, P(f), 1025, 0.0, P(f)) == NOT_SUPPORTED
    assert sm(h, 1, big, 4, P(rp), 0, P(f), P(f)) == NOT_SUPPORTED
    assert smb(h, 1, big, 4, P(rp), 0, P(f), P(f), P(f)) == NOT_SUPPORTED
    assert mm(h, 1, 4, 2, big, 4, 1.0, P(rp), P(ci), P(f), 0, P(f), 16, 0.0, P(f), 16) == NOT_SUPPORTED
    # more column tiles than a grid extent holds (heads * d > 65535 * 64)
    wide = 65536 * 64
    assert mm(h, 1, 64, 2, 2, 65536, 1.0, P(rp), P(ci), P(f), 0, P(f), wide, 0.0, P(f), wide) == NOT_SUPPORTED
    # quick returns
    assert sdd(h, 1, 4, 2, 0, 2, 1.0, None, None, 0, None, 8, None, 8, 0.0, None) == SUCCESS
    assert sm(h, 1, 0, 2, None, 0, None, None) == SUCCESS
    assert mm(h, 0, 4, 2, 2, 2, 1.0, None, None, None, 0, None, 8, 0.0, None, 8) == SUCCESS
    assert mm(h, 1, 0, 2, 2, 2, 1.0, None, None, None, 0, None, 0, 0.0, None, 0) == SUCCESS
    torch.cuda.synchronize()


def test_python_wrappers_refuse_bad_operands(device):
    ops = _ops()
    m, k, rp, ci = sd.pattern("dups")
    X, Y = hc.sddmm_operands(m, k, 2, 3)
    d_rp, d_ci, dX, dY = _dev(rp), _dev(ci), _dev(X), _dev(Y)
    e = torch.zeros((ci.size, 2), device=device)
    with pytest.raises(ValueError):
        ops.sddmm_heads(d_rp, d_ci, dX.view(m, 6), dY, m=m, k=k)  # heads and d unknown
    with pytest.raises(ValueError):
        ops.sddmm_heads(d_rp, d_ci, dX[:-1], dY, m=m, k=k, heads=2, d=3)
    with pytest.raises(TypeError):
        ops.sddmm_heads(d_rp, d_ci, dX.double(), dY, m=m, k=k)
    with pytest.raises(ValueError):
        ops.edge_softmax_heads(d_rp, e.view(-1))  # one head's 1-D layout
    with pytest.raises(ValueError):
        ops.edge_softmax_bwd_heads(d_rp, e, e[:, :1].contiguous())
    with pytest.raises(ValueError):
        ops.csrmm_heads(d_rp, d_ci, e[:, :1].contiguous(), dY, m=m, d=3, heads=2, k=k)
    with pytest.raises(ValueError):
        ops.csrmm_heads(d_rp, d_ci, e, dY.cpu(), m=m, d=3, heads=2, k=k)


def test_kernel_coverage(device):
    """One launch per call, and the union over the shapes of the tests above (the sampled
    product aligned and misaligned, the softmax patterns of each lane-group width forward
    and backward, the product's widths) is every kernel heads_kernels.hip ships."""
    ops = _ops()
    shipped = {kernel_keys.launch_key(k)
               for k in kernel_keys.shipped_kernels(("heads_kernels",))}
    assert len(shipped) == 24, sorted(shipped)
    seen = set()

    def one(keys, what):
        assert len(keys) == 1, (what, keys)
        seen.update(keys)

    with _handle() as h:
        m, k, rp, ci = sd.pattern("dups")
        d_rp, d_ci = _dev(rp), _dev(ci)
        for heads, d in hc.SDDMM_HD + hc.SDDMM_HD_MORE:
            X, Y = hc.sddmm_operands(m, k, heads, d)
            w = heads * d
            with h.launch_record() as rec:
                ops.sddmm_heads(d_rp, d_ci, _dev(X), _dev(Y), m=m, k=k, handle=h)
            one(rec, f"sddmm {heads}x{d}")
            bx, _ = hc.padded(X.reshape(m, w), w + 1, fill=0)
            by, _ = hc.padded(Y.reshape(k, w), w + 1, fill=0)
            with h.launch_record() as rec:
                ops.sddmm_heads(d_rp, d_ci, _dev(bx, offset=1), _dev(by, offset=1), m=m, d=d,
                                heads=heads, k=k, ldx=w + 1, ldy=w + 1, handle=h)
            one(rec, f"sddmm {heads}x{d} misaligned")
        for name in ("lengths", "short_mixed", "mid"):
            c = sc.case(name)
            x, g = hc.softmax_inputs(name, 3)
            rpd, dx, dg = _dev(c.rowptr), _dev(x), _dev(g)
            with h.launch_record() as rec:
                y = ops.edge_softmax_heads(rpd, dx, handle=h)
            one(rec, name)
            with h.launch_record() as rec:
                ops.edge_softmax_bwd_heads(rpd, y, dg, handle=h)
            one(rec, name + " backward")
        for heads, d in hc.PRODUCT_HD:
            m, k, rp, ci, val, B, _ = _product_args(heads, d, device)
            with h.launch_record() as rec:
                ops.csrmm_heads(_dev(rp), _dev(ci), _dev(val), _dev(B), m=m, d=d, heads=heads, k=k,
                                handle=h)
            one(rec, f"product {heads}x{d}")
    assert seen == shipped, (f"never launched: {sorted(shipped - seen)}; "
                             f"unknown: {sorted(seen - shipped)}")
