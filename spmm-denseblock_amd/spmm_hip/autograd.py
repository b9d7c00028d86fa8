"""torch.autograd on top of ops: the fp32 CSR product with a gradient for B.

ops.py stays "torch only owns memory"; this module is the one place where the
engine meets torch's autograd. Both directions run ops.csrmm (the merge-path
kernel): the forward on A, the backward on A^T, which CsrMatrix.t() builds once
per matrix with ops.csr2csc (the device transpose) and keeps.

    A = CsrMatrix(rowptr, colind, val, m, k)      # device tensors, base 0
    H1 = spmm(A, H)                               # H requires grad
    H1.sum().backward()                           # H.grad = A^T * dH1
"""
from __future__ import annotations

import torch

from . import ops


class CsrMatrix:
    """An m x k fp32 CSR matrix on the device (rowptr int32[m+1], colind int32[nnz],
    val float32[nnz], base 0) together with its transpose, built on first use."""

    def __init__(self, rowptr: torch.Tensor, colind: torch.Tensor, val: torch.Tensor, m: int,
                 k: int):
        for t, dt, nm in ((rowptr, torch.int32, "rowptr"), (colind, torch.int32, "colind"),
                          (val, torch.float32, "val")):
            ops._need(t, dt, nm)
        if rowptr.numel() != m + 1:
            raise ValueError(f"CsrMatrix: rowptr has {rowptr.numel()} entries, needs {m + 1}")
        if val.numel() != colind.numel():
            raise ValueError("CsrMatrix: val and colind differ in length")
        self.rowptr, self.colind, self.val = rowptr, colind, val
        self.m, self.k = m, k
        self._t: CsrMatrix | None = None

    def t(self, handle: ops.Handle | None = None) -> "CsrMatrix":
        """The k x m transpose: ops.csr2csc on the first call, the same object on every
        later one; its own .t() is this matrix. Its rows are sorted by column, entries
        of equal (row, col) in this matrix's order."""
        if self._t is None:
            cp, ri, v = ops.csr2csc(self.rowptr, self.colind, self.val.detach(), m=self.m,
                                    n=self.k, nnz=self.colind.numel(), handle=handle)
            At = CsrMatrix(cp, ri, v, self.k, self.m)
            At._t = self
            self._t = At
        return self._t


def _product(A: CsrMatrix, B: torch.Tensor) -> torch.Tensor:
    if B.dim() != 2 or B.shape[0] != A.k:
        raise ValueError(f"spmm: B must be ({A.k}, K), got {tuple(B.shape)}")
    B = B.contiguous()
    K = B.shape[1]
    C = torch.empty((A.m, K), dtype=torch.float32, device=B.device)
    return ops.csrmm(A.rowptr, A.colind, A.val.detach(), B, m=A.m, n=K, k=A.k, ldb=K, C=C, ldc=K)


class _Spmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, B: torch.Tensor, A: CsrMatrix) -> torch.Tensor:
        ctx.A = A
        return _product(A, B)

    @staticmethod
    def backward(ctx, grad_C: torch.Tensor):
        grad_B = _product(ctx.A.t(), grad_C) if ctx.needs_input_grad[0] else None
        return grad_B, None


def spmm(A: CsrMatrix, B: torch.Tensor) -> torch.Tensor:
    """C = A * B (fp32, row-major B[k, K] and C[m, K]): exactly ops.csrmm in the forward,
    and grad_B = ops.csrmm on A.t() applied to grad_C in the backward (the bits of the
    piece rule on A^T). A.val gets no gradient: that is a sampled dense-dense product,
    another kernel, which this library does not have; a val that requires grad is
    refused here, not silently treated as a constant."""
    if not isinstance(A, CsrMatrix):
        raise TypeError("spmm: A must be a CsrMatrix")
    if A.val.requires_grad:
        raise ValueError("spmm: A.val requires grad, but only B gets a gradient (the gradient "
                         "of the values is a sampled dense-dense product, not provided); "
                         "detach A.val")
    if not isinstance(B, torch.Tensor) or B.dtype != torch.float32 or not B.is_cuda:
        raise TypeError("spmm: B must be a float32 tensor on a HIP device")
    return _Spmm.apply(B, A)


__all__ = ["CsrMatrix", "spmm"]
