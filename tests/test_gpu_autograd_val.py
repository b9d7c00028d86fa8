"""spmm_hip.autograd.spmm(A, B, val=w): the CSR product on A's pattern with the values
of a tensor that may require grad. grad_val is the sampled dense-dense product
(ops.sddmm), grad_B the product on the kept transpose with w carried over by its
permutation; both are compared bit for bit with the direct ops calls and norm-wise
with torch's own autograd on the CPU in float64."""
from __future__ import annotations

import numpy as np
import pytest

from csr2csc_cases import matrices, values
from helpers import TOL_F32, assert_normwise

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _setup(name, K, seed=8):
    from spmm_hip import autograd
    m, k, rp, ci = matrices()[name]
    rng = np.random.default_rng(seed)
    host = dict(rp=rp, ci=ci, v=values(ci.size, 4),
                w=rng.uniform(-1, 1, ci.size).astype(np.float32),
                B=rng.uniform(-1, 1, (k, K)).astype(np.float32),
                G=rng.uniform(-1, 1, (m, K)).astype(np.float32))
    d = {key: torch.from_numpy(np.ascontiguousarray(a)).cuda() for key, a in host.items()}
    A = autograd.CsrMatrix(d["rp"], d["ci"], d["v"], m, k)
    return autograd, A, d, host, (m, k)


def _float64_autograd(host, m):
    """(C, grad_w, grad_B, |.| bounds of the two gradients) by torch's autograd on the
    CPU in float64; the product is an index_add, so duplicates accumulate."""
    rows = torch.from_numpy(np.repeat(np.arange(m), np.diff(host["rp"])))
    cols = torch.from_numpy(host["ci"].astype(np.int64))
    w = torch.from_numpy(host["w"].astype(np.float64)).requires_grad_(True)
    B = torch.from_numpy(host["B"].astype(np.float64)).requires_grad_(True)
    G = torch.from_numpy(host["G"].astype(np.float64))
    C = torch.zeros((m, B.shape[1]), dtype=torch.float64).index_add(0, rows, w[:, None] * B[cols])
    C.backward(G)
    absw = (G.abs()[rows] * B.detach().abs()[cols]).sum(1)
    absB = torch.zeros_like(B).index_add(0, cols, w.detach().abs()[:, None] * G.abs()[rows])
    return C.detach().numpy(), w.grad.numpy(), B.grad.numpy(), absw.numpy(), absB.numpy()


@pytest.mark.parametrize("K", [64, 136])
@pytest.mark.parametrize("name", ["dups", "random", "unsorted"])
def test_forward_and_both_gradients(device, name, K):
    from spmm_hip import ops
    autograd, A, d, host, (m, k) = _setup(name, K)
    w = d["w"].clone().requires_grad_(True)
    B = d["B"].clone().requires_grad_(True)
    C = autograd.spmm(A, B, val=w)
    want = torch.empty((m, K), device=device)
    ops.csrmm(A.rowptr, A.colind, d["w"], d["B"], m=m, n=K, k=k, ldb=K, C=want, ldc=K)
    assert torch.equal(C.detach(), want)
    C.backward(d["G"])
    assert torch.equal(w.grad, ops.sddmm(A.rowptr, A.colind, d["G"], d["B"], m=m, n=K, k=k))
    # the transpose and its permutation from a conversion of the test's own
    cp, ri, _, perm = ops.csr2csc(A.rowptr, A.colind, d["v"], m=m, n=k, return_perm=True)
    gB = torch.empty((k, K), device=device)
    ops.csrmm(cp, ri, d["w"][perm.long()], d["G"], m=k, n=K, k=m, ldb=K, C=gB, ldc=K)
    assert torch.equal(B.grad, gB)
    C64, gw64, gB64, absw, absB = _float64_autograd(host, m)
    assert_normwise(w.grad.cpu().numpy(), gw64, absw, TOL_F32, f"{name} K={K}: grad_val")
    assert_normwise(B.grad.cpu().numpy(), gB64, absB, TOL_F32, f"{name} K={K}: grad_B")
    # A.val took no part
    assert A.val.grad is None and torch.equal(A.val, d["v"])


def test_only_val_requires_grad_builds_no_transpose(device):
    from spmm_hip import ops
    autograd, A, d, host, (m, k) = _setup("random", 64)
    w = d["w"].clone().requires_grad_(True)
    C = autograd.spmm(A, d["B"], val=w)
    C.backward(d["G"])
    assert A._t is None and A._perm is None
    assert torch.equal(w.grad, ops.sddmm(A.rowptr, A.colind, d["G"], d["B"], m=m, n=64, k=k))


def test_only_b_requires_grad_runs_no_sddmm(device, monkeypatch):
    from spmm_hip import ops
    autograd, A, d, host, (m, k) = _setup("random", 64)
    calls = []
    real = ops.sddmm
    monkeypatch.setattr(ops, "sddmm", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    B = d["B"].clone().requires_grad_(True)
    w = d["w"].clone()
    autograd.spmm(A, B, val=w).backward(d["G"])
    assert calls == [] and w.grad is None and B.grad is not None
    w2 = d["w"].clone().requires_grad_(True)
    autograd.spmm(A, B, val=w2).backward(d["G"])
    assert calls == [1]  # the counter does see a call that happens
    C = autograd.spmm(A, d["B"], val=d["w"])  # nothing requires grad: a plain product
    assert not C.requires_grad


def test_expanded_gradient_accumulation_and_cached_transpose(device):
    autograd, A, d, host, (m, k) = _setup("dups", 136)
    At = A.t()
    w = d["w"].clone().requires_grad_(True)
    B = d["B"].clone().requires_grad_(True)
    autograd.spmm(A, B, val=w).sum().backward()  # an expanded (stride 0) gradient
    w1 = d["w"].clone().requires_grad_(True)
    B1 = d["B"].clone().requires_grad_(True)
    autograd.spmm(A, B1, val=w1).backward(torch.ones((m, 136), device=device))
    assert torch.equal(w.grad, w1.grad) and torch.equal(B.grad, B1.grad)
    # a second backward pass accumulates
    autograd.spmm(A, B1, val=w1).backward(torch.ones((m, 136), device=device))
    assert torch.equal(w1.grad, 2 * w.grad) and torch.equal(B1.grad, 2 * B.grad)
    assert A.t() is At and At.t() is A
    # a non-contiguous val is taken as it is read
    wide = torch.stack([d["w"], d["w"]], 1)[:, 0].requires_grad_(True)
    assert not wide.is_contiguous()
    C = autograd.spmm(A, d["B"], val=wide)
    assert torch.equal(C.detach(), autograd.spmm(A, d["B"], val=d["w"]))


@pytest.mark.parametrize("name", ["dups", "unsorted"])
def test_product_on_a_cached_transpose(device, name):
    """A product whose matrix is itself a cached transpose: the values travel back by
    the inverse permutation."""
    from spmm_hip import ops
    K = 64
    autograd, A, d, host, (m, k) = _setup(name, K)
    cp, ri, _, perm = ops.csr2csc(A.rowptr, A.colind, d["v"], m=m, n=k, return_perm=True)
    At = A.t()
    assert torch.equal(At.rowptr, cp) and torch.equal(At.colind, ri)
    inv = np.empty(perm.numel(), np.int64)
    inv[perm.cpu().numpy()] = np.arange(perm.numel())
    inv = torch.from_numpy(inv).cuda()
    w = d["w"].clone().requires_grad_(True)       # values of At, in At's order
    X = d["G"].clone().requires_grad_(True)       # At is k x m: its B has m rows
    Gt = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, (k, K)).astype(np.float32)).cuda()
    C = autograd.spmm(At, X, val=w)
    want = torch.empty((k, K), device=device)
    ops.csrmm(cp, ri, d["w"], d["G"], m=k, n=K, k=m, ldb=K, C=want, ldc=K)
    assert torch.equal(C.detach(), want)
    C.backward(Gt)
    assert At.t() is A and A.t() is At
    assert torch.equal(At.t_perm().long(), inv) and torch.equal(A.t_perm(), perm)
    gX = torch.empty((m, K), device=device)
    ops.csrmm(A.rowptr, A.colind, d["w"][inv], Gt, m=m, n=K, k=k, ldb=K, C=gX, ldc=K)
    assert torch.equal(X.grad, gX)
    assert torch.equal(w.grad, ops.sddmm(cp, ri, Gt, d["G"], m=k, n=K, k=m))
    # grad_X against float64: X.grad = At^T (w) Gt, that is A's pattern with w[inv]
    rows = np.repeat(np.arange(m), np.diff(host["rp"]))
    wv = host["w"][inv.cpu().numpy()].astype(np.float64)
    Gt64 = Gt.cpu().numpy().astype(np.float64)
    ref, absd = np.zeros((m, K)), np.zeros((m, K))
    np.add.at(ref, rows, wv[:, None] * Gt64[host["ci"]])
    np.add.at(absd, rows, np.abs(wv)[:, None] * np.abs(Gt64[host["ci"]]))
    assert_normwise(X.grad.cpu().numpy(), ref, absd, TOL_F32, f"{name}: grad through At")


def test_val_none_is_todays_path(device):
    from spmm_hip import ops
    K = 64
    autograd, A, d, host, (m, k) = _setup("dups", K)
    B = d["B"].clone().requires_grad_(True)
    C = autograd.spmm(A, B, val=None)
    C2 = autograd.spmm(A, B)
    want = torch.empty((m, K), device=device)
    ops.csrmm(A.rowptr, A.colind, A.val, d["B"], m=m, n=K, k=k, ldb=K, C=want, ldc=K)
    assert torch.equal(C.detach(), want) and torch.equal(C2.detach(), want)
    C.backward(d["G"])
    At = A.t()
    gB = torch.empty((k, K), device=device)
    ops.csrmm(At.rowptr, At.colind, At.val, d["G"], m=k, n=K, k=m, ldb=K, C=gB, ldc=K)
    assert torch.equal(B.grad, gB)
    A.val.requires_grad_(True)
    with pytest.raises(ValueError, match="only B gets a gradient"):
        autograd.spmm(A, d["B"])
    with pytest.raises(ValueError, match="only B gets a gradient"):
        autograd.spmm(A, d["B"], val=None)


def test_val_is_checked(device):
    autograd, A, d, host, (m, k) = _setup("dups", 64)
    with pytest.raises(ValueError):
        autograd.spmm(A, d["B"], val=d["w"][:-1])
    with pytest.raises(TypeError):
        autograd.spmm(A, d["B"], val=d["w"].double())
    with pytest.raises(TypeError):
        autograd.spmm(A, d["B"], val=d["w"].cpu())
