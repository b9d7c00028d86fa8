"""spmm_hip.autograd.edge_softmax and autograd.sddmm, and the attention chain they close:
spmm(A, H, val=edge_softmax(A, sddmm(A, H, H))). The gradients are compared with torch's
own autograd on the CPU in float64 over the gather form, (X[rows] * Y[cols]).sum(1) and a
per-row torch.softmax on a padded dense copy, at the project's bar: |got - ref| <= 1e-5 *
(the sum of the absolute values of the terms), the terms' bounds carried through the
stages."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from helpers import TOL_F32, assert_normwise

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

M, K, N, HUB = 300, 200, 20, 2000


@functools.lru_cache(maxsize=None)
def _host(k):
    """An M x k pattern with one row of HUB nonzeros (columns repeat), short rows and
    empty ones, and the operands. Cached: read-only."""
    rng = np.random.default_rng(23)
    lens = rng.integers(0, 12, M)
    lens[17] = HUB
    lens[[0, 40, M - 1]] = 0
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(rp[-1])
    f = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)  # noqa: E731
    return dict(rp=rp, ci=rng.integers(0, k, nnz).astype(np.int32), v=f(nnz), x=3 * f(nnz),
                g=f(nnz), X=f(M, N), Y=f(k, N), G=f(M, N), lens=lens)


def _setup(k=K):
    from spmm_hip import autograd
    host = _host(k)
    d = {key: torch.from_numpy(a).cuda() for key, a in host.items() if key != "lens"}
    return autograd, autograd.CsrMatrix(d["rp"], d["ci"], d["v"], M, k), d, host


def _rows(host):
    return torch.from_numpy(np.repeat(np.arange(M), host["lens"]))


def _softmax64(e, host):
    """The per-row softmax of e (float64, differentiable) on a padded dense copy."""
    lens = host["lens"]
    rows = _rows(host)
    within = torch.from_numpy(np.concatenate([np.arange(n) for n in lens]))
    pad = torch.full((M, int(lens.max())), -np.inf, dtype=torch.float64)
    pad[torch.from_numpy(np.flatnonzero(lens == 0))] = 0.0  # no NaN rows in the copy
    pad = pad.index_put((rows, within), e)
    return torch.softmax(pad, 1)[rows, within]


def _t64(a, grad=False):
    return torch.from_numpy(a.astype(np.float64)).requires_grad_(grad)


def _rowsum(v, rows):
    return torch.zeros(M, dtype=torch.float64).index_add(0, rows, v)[rows]


def test_edge_softmax_gradient(device):
    from spmm_hip import ops
    autograd, A, d, host = _setup()
    x = d["x"].clone().requires_grad_(True)
    y = autograd.edge_softmax(A, x)
    assert torch.equal(y.detach(), ops.edge_softmax(A.rowptr, d["x"]))
    y.backward(d["g"])
    assert torch.equal(x.grad, ops.edge_softmax_bwd(A.rowptr, y.detach(), d["g"]))
    x64, g64 = _t64(host["x"], True), _t64(host["g"])
    y64 = _softmax64(x64, host)
    y64.backward(g64)
    rows = _rows(host)
    yd = y64.detach()
    assert_normwise(y.detach().cpu().numpy(), yd.numpy(), yd.numpy(), TOL_F32, "y")
    absd = yd * (g64.abs() + _rowsum(yd * g64.abs(), rows))
    assert_normwise(x.grad.cpu().numpy(), x64.grad.numpy(), absd.numpy(), TOL_F32, "grad_x")
    # nothing requires grad: a plain call; the argument checks
    assert not autograd.edge_softmax(A, d["x"]).requires_grad
    with pytest.raises(ValueError):
        autograd.edge_softmax(A, d["x"][:-1])
    with pytest.raises(TypeError):
        autograd.edge_softmax(A, d["x"].double())


def test_sddmm_gradients(device):
    from spmm_hip import ops
    autograd, A, d, host = _setup()
    X = d["X"].clone().requires_grad_(True)
    Y = d["Y"].clone().requires_grad_(True)
    e = autograd.sddmm(A, X, Y)
    assert torch.equal(e.detach(), ops.sddmm(A.rowptr, A.colind, d["X"], d["Y"], m=M, n=N, k=K))
    e.backward(d["g"])
    rows, cols = _rows(host), torch.from_numpy(host["ci"].astype(np.int64))
    X64, Y64, g64 = _t64(host["X"], True), _t64(host["Y"], True), _t64(host["g"])
    (X64[rows] * Y64[cols]).sum(1).backward(g64)
    absX = torch.zeros(M, N, dtype=torch.float64).index_add(
        0, rows, g64.abs()[:, None] * Y64.detach().abs()[cols])
    absY = torch.zeros(K, N, dtype=torch.float64).index_add(
        0, cols, g64.abs()[:, None] * X64.detach().abs()[rows])
    assert_normwise(X.grad.cpu().numpy(), X64.grad.numpy(), absX.numpy(), TOL_F32, "grad_X")
    assert_normwise(Y.grad.cpu().numpy(), Y64.grad.numpy(), absY.numpy(), TOL_F32, "grad_Y")


def test_grad_x_alone_builds_no_transpose(device):
    autograd, A, d, host = _setup()
    X = d["X"].clone().requires_grad_(True)
    autograd.sddmm(A, X, d["Y"]).backward(d["g"])
    assert A._t is None and A._perm is None and X.grad is not None
    Y = d["Y"].clone().requires_grad_(True)
    autograd.sddmm(A, d["X"], Y).backward(d["g"])
    assert A._t is not None and Y.grad is not None


def test_attention_chain(device):
    """H' = spmm(A, H, val=edge_softmax(A, sddmm(A, H, H))) on a square pattern: forward
    and the gradient of H against the float64 dense attention; two runs, the same bits."""
    autograd, A, d, host = _setup(M)

    def run():
        H = d["X"].clone().requires_grad_(True)
        out = autograd.spmm(A, H, val=autograd.edge_softmax(A, autograd.sddmm(A, H, H)))
        out.backward(d["G"])
        return out.detach(), H.grad

    out, gH = run()
    out2, gH2 = run()
    assert torch.equal(out, out2) and torch.equal(gH, gH2)

    rows, cols = _rows(host), torch.from_numpy(host["ci"].astype(np.int64))
    H64, G64 = _t64(host["X"], True), _t64(host["G"])
    a64 = _softmax64((H64[rows] * H64[cols]).sum(1), host)
    out64 = torch.zeros(M, N, dtype=torch.float64).index_add(0, rows, a64[:, None] * H64[cols])
    out64.backward(G64)
    # the bounds, stage by stage: every sum with the absolute values of its terms
    Ha, Ga, a = H64.detach().abs(), G64.abs(), a64.detach()
    zeros = lambda: torch.zeros(M, N, dtype=torch.float64)  # noqa: E731
    abs_out = zeros().index_add(0, rows, a[:, None] * Ha[cols])
    abs_ga = (Ga[rows] * Ha[cols]).sum(1)                  # grad of a: <G[row], H[col]>
    abs_ge = a * (abs_ga + _rowsum(a * abs_ga, rows))      # through the softmax
    abs_gH = (zeros().index_add(0, cols, a[:, None] * Ga[rows])          # the product's B
              + zeros().index_add(0, rows, abs_ge[:, None] * Ha[cols])   # sddmm's X
              + zeros().index_add(0, cols, abs_ge[:, None] * Ha[rows]))  # sddmm's Y
    assert_normwise(out.cpu().numpy(), out64.detach().numpy(), abs_out.numpy(), TOL_F32, "H'")
    assert_normwise(gH.cpu().numpy(), H64.grad.numpy(), abs_gH.numpy(), TOL_F32, "grad_H")
