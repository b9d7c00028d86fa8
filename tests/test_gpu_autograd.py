"""spmm_hip.autograd: the fp32 CSR product as a torch.autograd.Function whose backward
is the product on the device-transposed matrix (ops.csr2csc, built once and kept)."""
from __future__ import annotations

import numpy as np
import pytest

from csr2csc_cases import matrices, values
from helpers import TOL_F32, assert_normwise

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K = 128


def _setup(name):
    from spmm_hip import autograd
    m, n, rp, ci = matrices()[name]
    v = values(ci.size, 4)
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rp, ci, v)]
    A = autograd.CsrMatrix(*d, m, n)
    rng = np.random.default_rng(8)
    B = torch.from_numpy(rng.uniform(-1, 1, (n, K)).astype(np.float32)).cuda()
    G = torch.from_numpy(rng.uniform(-1, 1, (m, K)).astype(np.float32)).cuda()
    return autograd, A, B, G, (m, n, rp, ci, v)


@pytest.mark.parametrize("name", ["random", "dups"])
def test_forward_and_grad_b(device, name):
    from spmm_hip import ops
    autograd, A, B, G, (m, n, rp, ci, v) = _setup(name)
    B.requires_grad_(True)
    C = autograd.spmm(A, B)
    want = torch.empty((m, K), device=device)
    ops.csrmm(A.rowptr, A.colind, A.val, B.detach(), m=m, n=K, k=n, ldb=K, C=want, ldc=K)
    assert torch.equal(C.detach(), want)
    C.backward(G)
    At = A.t()
    assert (At.m, At.k) == (n, m)
    gB = torch.empty((n, K), device=device)
    ops.csrmm(At.rowptr, At.colind, At.val, G, m=n, n=K, k=m, ldb=K, C=gB, ldc=K)
    assert torch.equal(B.grad, gB)
    # dense(A)^T G in fp64, |a||b| summed over every entry (duplicates each on its own)
    rows = np.repeat(np.arange(m), np.diff(rp))
    D = np.zeros((m, n))
    Dabs = np.zeros((m, n))
    np.add.at(D, (rows, ci), v.astype(np.float64))
    np.add.at(Dabs, (rows, ci), np.abs(v).astype(np.float64))
    G64 = G.cpu().numpy().astype(np.float64)
    assert_normwise(B.grad.cpu().numpy(), D.T @ G64, Dabs.T @ np.abs(G64), TOL_F32,
                    f"{name}: grad_B")


def test_non_contiguous_grad_and_no_grad_for_b(device):
    autograd, A, B, G, (m, n, *_) = _setup("dups")
    B.requires_grad_(True)
    autograd.spmm(A, B).sum().backward()  # an expanded (stride 0) gradient
    ones = torch.ones((m, K), device=device)
    B2 = B.detach().clone().requires_grad_(True)
    autograd.spmm(A, B2).backward(ones)
    assert torch.equal(B.grad, B2.grad)
    C = autograd.spmm(A, B.detach())  # nothing requires grad: a plain product
    assert not C.requires_grad


def test_val_that_requires_grad_is_refused(device):
    autograd, A, B, G, _ = _setup("dups")
    A.val.requires_grad_(True)
    with pytest.raises(ValueError, match="only B gets a gradient"):
        autograd.spmm(A, B)


def test_transpose_is_built_once(device):
    """A.t().t() is A, and a second backward runs the product alone: on a timing-enabled
    handle the conversion's kernels are counted on the first .t() only."""
    from spmm_hip import ops
    autograd, A, B, G, (m, n, *_) = _setup("random")
    h = ops.Handle()
    h.set_timing(True)
    At = A.t(handle=h)
    first = len(h.kernel_times())
    assert first >= 3  # count, scan, sort passes, gather
    assert A.t(handle=h) is At and At.t() is A and A.t().t().t() is At
    assert len(h.kernel_times()) == 0
    h.set_timing(False)
    B.requires_grad_(True)
    arrays = (At.rowptr.data_ptr(), At.colind.data_ptr(), At.val.data_ptr())
    for _ in range(2):
        autograd.spmm(A, B).backward(G)
        assert A.t() is At
        assert (At.rowptr.data_ptr(), At.colind.data_ptr(), At.val.data_ptr()) == arrays
    assert torch.equal(B.grad, 2 * _grad_once(autograd, A, B, G))


def _grad_once(autograd, A, B, G):
    B1 = B.detach().clone().requires_grad_(True)
    autograd.spmm(A, B1).backward(G)
    return B1.grad
