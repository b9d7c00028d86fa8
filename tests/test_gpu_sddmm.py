"""spmm_sddmm_csr_f32 (ops.sddmm, the CSR-sampled dense-dense product on the device)
against the host form (prep.sddmm), bit for bit: every lane-group width, alpha / beta,
bases, views, padded and offset layouts, handle reuse and a captured-graph replay. The
host form is checked against numpy in tests/test_sddmm_host.py."""
from __future__ import annotations

import numpy as np
import pytest

from helpers import framed, reversed_rows
from sddmm_cases import N_LIST, N_WIDE, bits, old_values, operands, pattern, rows_of

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAMES = ["n1", "n200", "n4097", "random", "dups", "unsorted", "view"]
# skew: a 70,000-nonzero row (many waves on one X row) and a column in every row
CASES = [(nm, n) for nm in NAMES for n in N_LIST] + [("skew", 128), ("skew", 32),
                                                     ("dups", N_WIDE), ("view", N_WIDE)]
ALPHA, BETA = 1.7, -0.6


def _ops():
    from spmm_hip import ops
    return ops


def _prep():
    from spmm_hip import prep
    return prep


def _dev(*arrays):
    return [torch.from_numpy(np.array(a, order="C")).cuda() for a in arrays]  # a writable copy


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, (f"{what}: {bad.size} of {want.size} outputs differ from the host "
                           f"form, first at {bad[:1]}: {got[bad[:1]]} vs {want[bad[:1]]}")


@pytest.mark.parametrize("name,n", CASES)
def test_device_equals_host(device, name, n):
    ops, prep = _ops(), _prep()
    m, k, rp, ci = pattern(name)
    X, Y = operands(m, k, n)
    p0, nnz, _ = rows_of(m, rp)
    old = old_values(ci.size)
    dX, dY = _dev(X, Y)
    d_rp, d_ci = _dev(rp, ci)
    # beta == 0: out is never read (a NaN there would spread), and in a view only the
    # view's positions are written
    nan = np.full(ci.size, np.nan, np.float32)
    with ops.default_handle().launch_record() as rec:
        got = ops.sddmm(d_rp, d_ci, dX, dY, m=m, n=n, k=k, out=_dev(nan)[0])
    # N_WIDE is past the lane-group kernel's four chunks per lane: the whole-wave kernel
    assert len(rec) == (1 if nnz else 0), rec
    assert all(("17sddmm_wide_kernelI" in key) == (n == N_WIDE) for key in rec), rec
    want = prep.sddmm(m, n, k, rp, ci, X, Y, out=nan.copy())
    assert not np.isnan(want[p0:p0 + nnz]).any()
    _same(got, want, f"{name} n={n}")
    # a new out tensor by default
    fresh = ops.sddmm(d_rp, d_ci, dX, dY, m=m, k=k)
    assert fresh.shape == (ci.size,) and fresh.dtype == torch.float32
    _same(fresh[p0:p0 + nnz], want[p0:p0 + nnz], f"{name} n={n}: default out")
    # alpha and beta
    got = ops.sddmm(d_rp, d_ci, dX, dY, m=m, n=n, k=k, out=_dev(old)[0], alpha=ALPHA, beta=BETA)
    want = prep.sddmm(m, n, k, rp, ci, X, Y, out=old.copy(), alpha=ALPHA, beta=BETA)
    _same(got, want, f"{name} n={n} alpha beta")
    # base 1
    got1 = ops.sddmm(*_dev(rp + 1, ci + 1), dX, dY, m=m, n=n, k=k, out=_dev(old)[0], alpha=ALPHA,
                     beta=BETA, base=1)
    _same(got1, want, f"{name} n={n} base 1")


LAYOUTS = [(0, 0, 0, 0), (4, 4, 4, 4), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1),
           (1, 1, 1, 1), (4, 0, 0, 4), (1, 4, 4, 1)]  # (off_X, pad_X, off_Y, pad_Y) in floats


@pytest.mark.parametrize("n", [5, 64, 68, 132, 260])
def test_layouts(device, n):
    """Offsets of 0, 4 and 1 floats and pads of 0, 4 and 1 on X and Y: the guards and the
    padding stay untouched, the inputs unchanged, the bits those of the tight layout;
    out sits between guards of its own."""
    ops, prep = _ops(), _prep()
    m, k, rp, ci = pattern("unsorted")
    X, Y = operands(m, k, n)
    old = old_values(ci.size)
    want = prep.sddmm(m, n, k, rp, ci, X, Y, out=old.copy(), alpha=ALPHA, beta=BETA)
    d_rp, d_ci = _dev(rp, ci)
    for lay in LAYOUTS:
        ox, px, oy, py = lay
        dX, chkX = framed(X, n + px, ox)
        dY, chkY = framed(Y, n + py, oy)
        dO, chkO = framed(old.reshape(1, -1), ci.size, ox)
        ops.sddmm(d_rp, d_ci, dX, dY, m=m, n=n, k=k, ldx=n + px, ldy=n + py, out=dO, alpha=ALPHA,
                  beta=BETA)
        _same(chkO(f"n={n} {lay}: out").reshape(-1), want, f"n={n} layout {lay}")
        chkX.unchanged(f"n={n} {lay}: X")
        chkY.unchanged(f"n={n} {lay}: Y")


@pytest.mark.parametrize("n", [16, 68, 260])
def test_x_is_y(device, n):
    """X and Y the same buffer: edge logits <h_i, h_j> on a square pattern."""
    ops, prep = _ops(), _prep()
    m, k, rp, ci = pattern("unsorted")
    s = max(m, k)
    H = operands(s, s, n)[1]
    want = prep.sddmm(m, n, s, rp, ci, H, H)
    d_rp, d_ci = _dev(rp, ci)
    for off, pad in ((0, 0), (1, 1), (4, 4)):
        dH, chk = framed(H, n + pad, off)
        got = ops.sddmm(d_rp, d_ci, dH, dH, m=m, n=n, k=s, ldx=n + pad, ldy=n + pad)
        _same(got, want, f"X is Y, n={n} off={off} pad={pad}")
        chk.unchanged("H")


def test_relaunch_and_reuse(device):
    """Two consecutive calls on one handle after another product on it: the same bits,
    those of the default handle's call; the product's own result is not disturbed."""
    ops, prep = _ops(), _prep()
    m, k, rp, ci = pattern("random")
    n = 132
    X, Y = operands(m, k, n)
    v = old_values(ci.size, seed=3)
    d_rp, d_ci, dv, dX, dY = _dev(rp, ci, v, X, Y)
    h = ops.Handle()
    C = torch.empty((m, n), device=device)
    ops.csrmm(d_rp, d_ci, dv, dY, m=m, n=n, k=k, ldb=n, C=C, ldc=n, handle=h)
    a = ops.sddmm(d_rp, d_ci, dX, dY, m=m, n=n, k=k, handle=h)
    b = ops.sddmm(d_rp, d_ci, dX, dY, m=m, n=n, k=k, handle=h)
    C2 = torch.empty((m, n), device=device)
    ops.csrmm(d_rp, d_ci, dv, dY, m=m, n=n, k=k, ldb=n, C=C2, ldc=n, handle=h)
    c = ops.sddmm(d_rp, d_ci, dX, dY, m=m, n=n, k=k)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(C, C2)
    _same(a, prep.sddmm(m, n, k, rp, ci, X, Y), "reuse")
    h.close()


def test_python_wrapper_refuses_bad_operands(device):
    ops = _ops()
    m, k, rp, ci = pattern("dups")
    X, Y = operands(m, k, 16)
    d_rp, d_ci, dX, dY = _dev(rp, ci, X, Y)
    with pytest.raises(TypeError):
        ops.sddmm(d_rp, d_ci, dX.double(), dY, k=k)
    with pytest.raises(ValueError):
        ops.sddmm(d_rp, d_ci, dX, dY[:-1], k=k)  # Y holds fewer than k rows
    with pytest.raises(ValueError):
        ops.sddmm(d_rp, d_ci, dX, dY, k=k, ldx=15)
    with pytest.raises(ValueError):
        ops.sddmm(d_rp, d_ci, dX, dY, k=k, out=torch.empty(ci.size - 1, device=device))
    with pytest.raises(ValueError):
        ops.sddmm(d_rp, d_ci, dX.t(), dY, k=k)  # not contiguous


def test_captured_graph_replay(device):
    """One ops.sddmm captured on a side stream; X, Y and the pattern's colind are then
    overwritten in place (the same nnz) and the replay equals an eager call on the new
    operands, bit for bit. The call owns no buffer of the handle, so the graph is one
    kernel node."""
    ops, prep = _ops(), _prep()
    m, k, rp, ci = pattern("unsorted")
    n = 68
    X, Y = operands(m, k, n)
    old = old_values(ci.size)
    rp2, ci2, _ = reversed_rows(rp, ci, np.arange(ci.size))
    X2, Y2 = operands(m, k, n, seed=77)
    assert not np.array_equal(ci, ci2)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        h = ops.Handle(stream=s)
        d_rp, d_ci, dX, dY, dO = _dev(rp, ci, X, Y, old)
        # the eager call every capture here is preceded by (include/spmm_hip.h)
        ops.sddmm(d_rp, d_ci, dX, dY, m=m, n=n, k=k, out=_dev(old)[0], alpha=ALPHA, beta=BETA,
                  handle=h)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        try:
            try:
                with torch.cuda.graph(g, stream=s):
                    h.set_stream(s)
                    ops.sddmm(d_rp, d_ci, dX, dY, m=m, n=n, k=k, out=dO, alpha=ALPHA, beta=BETA,
                              handle=h)
            finally:
                h.set_stream(s)
            g.replay()
            s.synchronize()
            _same(dO, prep.sddmm(m, n, k, rp, ci, X, Y, out=old.copy(), alpha=ALPHA, beta=BETA),
                  "first replay")
            for dst, src in ((d_rp, rp2), (d_ci, ci2), (dX, X2), (dY, Y2), (dO, old)):
                dst.copy_(torch.from_numpy(np.array(src, order="C")))
            g.replay()
            s.synchronize()
            eager = ops.sddmm(d_rp, d_ci, dX, dY, m=m, n=n, k=k, out=_dev(old)[0], alpha=ALPHA,
                              beta=BETA, handle=h)
            s.synchronize()
            assert torch.equal(dO, eager)
            _same(dO, prep.sddmm(m, n, k, rp2, ci2, X2, Y2, out=old.copy(), alpha=ALPHA,
                                 beta=BETA), "replay on the overwritten operands")
        finally:
            del g
            h.close()
