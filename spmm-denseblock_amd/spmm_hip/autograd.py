"""torch.autograd on top of ops: the fp32 CSR product with gradients for B and for A's
values.

ops.py stays "torch only owns memory"; this module is the one place where the
engine meets torch's autograd. The forward and grad_B run ops.csrmm (the merge-path
kernel), the forward on A, grad_B on A^T, which CsrMatrix.t() builds once per matrix
with ops.csr2csc (the device transpose) and keeps together with the permutation that
carries values over; grad_val runs ops.sddmm (the sampled dense-dense product) on A's
own pattern.

    A = CsrMatrix(rowptr, colind, val, m, k)      # device tensors, base 0
    H1 = spmm(A, H)                               # H requires grad
    H1.sum().backward()                           # H.grad = A^T * dH1

    w = edge_weights(...)                         # nnz floats, requires grad
    H1 = spmm(A, H, val=w)                        # w replaces A.val for this product
    H1.sum().backward()                           # w.grad[p] = <dH1[row(p)], H[col(p)]>

edge_softmax and sddmm close the attention chain on a fixed pattern: the logits
(ops.sddmm, with gradients for X and Y from two CSR products), their softmax over every
row's positions (ops.edge_softmax / ops.edge_softmax_bwd), and the product on them:

    a = edge_softmax(A, sddmm(A, H, H))           # nnz attention weights
    H1 = spmm(A, H, val=a)                        # backpropagates to H on all three paths

sddmm_heads, edge_softmax_heads and spmm_heads are the same chain over several heads, one
launch per op (ops.*_heads): features [rows, heads, d], edge values [nnz, heads]:

    a = edge_softmax_heads(A, sddmm_heads(A, H, H))   # [nnz, heads]
    H1 = spmm_heads(A, H, val=a)                      # [m, heads, d]

H may be float16 or bfloat16 there (ops.*_heads on half features): the logits, the softmax
and every edge gradient stay float32, the kernels accumulate in float32, and a result that
takes the features' place (H1, H.grad) is cast to H's type once, round to nearest even.

spmm_reduce is the product with max or min in place of the sum (GraphSAGE-pool, PNA): the
forward keeps the winning positions, the backward is a masked product over A.t() with no
atomics (ops.csrmm_reduce / ops.csrmm_reduce_bwd):

    P = spmm_reduce(A, H, "max")                      # [m, n]; H.grad through the winners
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
        self._perm: torch.Tensor | None = None  # t().val == val[_perm] (t_perm)

    def t(self, handle: ops.Handle | None = None) -> "CsrMatrix":
        """The k x m transpose: ops.csr2csc on the first call, the same object on every
        later one; its own .t() is this matrix. Its rows are sorted by column, entries
        of equal (row, col) in this matrix's order."""
        if self._t is None:
            cp, ri, v, perm = ops.csr2csc(self.rowptr, self.colind, self.val.detach(), m=self.m,
                                          n=self.k, nnz=self.colind.numel(), return_perm=True,
                                          handle=handle)
            At = CsrMatrix(cp, ri, v, self.k, self.m)
            At._t = self
            self._t = At
            self._perm = perm
        return self._t

    def t_perm(self, handle: ops.Handle | None = None) -> torch.Tensor:
        """int32[nnz] with t().val == val[t_perm()]: the transpose's own permutation
        (ops.csr2csc's perm), kept with it. On a matrix that is itself a cached transpose
        it is the inverse of the other side's, derived once by a scatter of arange (a
        permutation has no repeated target, so the scatter is deterministic)."""
        At = self.t(handle)
        if self._perm is None:
            p = At._perm
            inv = torch.empty_like(p)
            inv[p.long()] = torch.arange(p.numel(), dtype=torch.int32, device=p.device)
            self._perm = inv
        return self._perm


def _product(A: CsrMatrix, B: torch.Tensor, val: torch.Tensor | None = None) -> torch.Tensor:
    if B.dim() != 2 or B.shape[0] != A.k:
        raise ValueError(f"spmm: B must be ({A.k}, K), got {tuple(B.shape)}")
    B = B.contiguous()
    K = B.shape[1]
    C = torch.empty((A.m, K), dtype=torch.float32, device=B.device)
    v = A.val.detach() if val is None else val
    return ops.csrmm(A.rowptr, A.colind, v, B, m=A.m, n=K, k=A.k, ldb=K, C=C, ldc=K)


class _Spmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, B: torch.Tensor, A: CsrMatrix) -> torch.Tensor:
        ctx.A = A
        return _product(A, B)

    @staticmethod
    def backward(ctx, grad_C: torch.Tensor):
        grad_B = _product(ctx.A.t(), grad_C) if ctx.needs_input_grad[0] else None
        return grad_B, None


class _SpmmVal(torch.autograd.Function):
    """The product on A's pattern with the values of a tensor of its own."""

    @staticmethod
    def forward(ctx, B: torch.Tensor, val: torch.Tensor, A: CsrMatrix) -> torch.Tensor:
        ctx.A = A
        B, val = B.detach().contiguous(), val.detach().contiguous()
        ctx.save_for_backward(B, val)
        return _product(A, B, val)

    @staticmethod
    def backward(ctx, grad_C: torch.Tensor):
        A = ctx.A
        B, val = ctx.saved_tensors
        grad_C = grad_C.contiguous()
        grad_B = grad_val = None
        if ctx.needs_input_grad[0]:
            vt = torch.index_select(val, 0, A.t_perm())
            grad_B = _product(A.t(), grad_C, vt)
        if ctx.needs_input_grad[1]:
            grad_val = ops.sddmm(A.rowptr, A.colind, grad_C, B, m=A.m, n=B.shape[1], k=A.k)
        return grad_B, grad_val, None


def spmm(A: CsrMatrix, B: torch.Tensor, val: torch.Tensor | None = None) -> torch.Tensor:
    """C = A * B (fp32, row-major B[k, K] and C[m, K]): exactly ops.csrmm in the forward,
    and grad_B = ops.csrmm on A.t() applied to grad_C in the backward (the bits of the
    piece rule on A^T).

    val=None: the values are A.val, a constant: it gets no gradient, and an A.val that
    requires grad is refused here, not silently treated as a constant; pass it as val.

    val: a float32 device tensor of nnz entries that replaces A.val for this product and
    may require grad (learned or computed edge weights on a fixed pattern). The forward
    is ops.csrmm on (A.rowptr, A.colind, val); the backward gives
    grad_val = ops.sddmm(A.rowptr, A.colind, grad_C, B), the sampled dense-dense product
    grad_val[p] = <grad_C[row(p), :], B[col(p), :]>, and grad_B = ops.csrmm on A.t()'s
    pattern with the values val[A.t_perm()]. Each gradient is computed only when it is
    needed: the transpose is not built for grad_val alone."""
    if not isinstance(A, CsrMatrix):
        raise TypeError("spmm: A must be a CsrMatrix")
    if val is None and A.val.requires_grad:
        raise ValueError("spmm: A.val requires grad, but only B gets a gradient on this "
                         "path; pass the values as spmm(A, B, val=...) to get theirs "
                         "(ops.sddmm), or detach A.val")
    if not isinstance(B, torch.Tensor) or B.dtype != torch.float32 or not B.is_cuda:
        raise TypeError("spmm: B must be a float32 tensor on a HIP device")
    if val is None:
        return _Spmm.apply(B, A)
    if not isinstance(val, torch.Tensor) or val.dtype != torch.float32 or not val.is_cuda:
        raise TypeError("spmm: val must be a float32 tensor on a HIP device")
    if val.dim() != 1 or val.numel() != A.colind.numel():
        raise ValueError(f"spmm: val must hold the pattern's {A.colind.numel()} values, got "
                         f"{tuple(val.shape)}")
    return _SpmmVal.apply(B, val, A)


class _EdgeSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, A: CsrMatrix) -> torch.Tensor:
        ctx.A = A
        y = ops.edge_softmax(A.rowptr, x.detach().contiguous(), m=A.m)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, grad_y: torch.Tensor):
        (y,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        return ops.edge_softmax_bwd(ctx.A.rowptr, y, grad_y.contiguous(), m=ctx.A.m), None


def edge_softmax(A: CsrMatrix, x: torch.Tensor) -> torch.Tensor:
    """y = the softmax of x over the positions of every row of A's pattern
    (ops.edge_softmax; x: float32, nnz entries, one head). The forward saves y; the
    backward is ops.edge_softmax_bwd(A.rowptr, y, grad_y): both a function of the row's
    values alone, so two runs give the same gradient bits."""
    if not isinstance(A, CsrMatrix):
        raise TypeError("edge_softmax: A must be a CsrMatrix")
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda:
        raise TypeError("edge_softmax: x must be a float32 tensor on a HIP device")
    if x.dim() != 1 or x.numel() != A.colind.numel():
        raise ValueError(f"edge_softmax: x must hold the pattern's {A.colind.numel()} values, "
                         f"got {tuple(x.shape)}")
    return _EdgeSoftmax.apply(x, A)


class _Sddmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X: torch.Tensor, Y: torch.Tensor, A: CsrMatrix) -> torch.Tensor:
        ctx.A = A
        X, Y = X.detach().contiguous(), Y.detach().contiguous()
        ctx.save_for_backward(X, Y)
        return ops.sddmm(A.rowptr, A.colind, X, Y, m=A.m, n=X.shape[1], k=A.k)

    @staticmethod
    def backward(ctx, ge: torch.Tensor):
        A = ctx.A
        X, Y = ctx.saved_tensors
        ge = ge.contiguous()
        grad_X = grad_Y = None
        if ctx.needs_input_grad[0]:
            grad_X = _product(A, Y, ge)
        if ctx.needs_input_grad[1]:
            grad_Y = _product(A.t(), X, torch.index_select(ge, 0, A.t_perm()))
        return grad_X, grad_Y, None


def sddmm(A: CsrMatrix, X: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
    """e[p] = <X[row(p), :], Y[col(p), :]> on A's pattern (ops.sddmm; X: m x n, Y: k x n),
    with gradients for X and Y built from the CSR product, ge = the gradient of e:
    grad_X = ops.csrmm on (A's pattern, values ge) applied to Y, and grad_Y = ops.csrmm on
    A.t()'s pattern with the values ge[A.t_perm()] applied to X. Each is computed only
    when it is needed: the transpose is not built for grad_X alone. X may be Y (the edge
    logits <h_i, h_j>); autograd then adds the two."""
    if not isinstance(A, CsrMatrix):
        raise TypeError("sddmm: A must be a CsrMatrix")
    for t, rows, nm in ((X, A.m, "X"), (Y, A.k, "Y")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda:
            raise TypeError(f"sddmm: {nm} must be a float32 tensor on a HIP device")
        if t.dim() != 2 or t.shape[0] != rows:
            raise ValueError(f"sddmm: {nm} must be ({rows}, n), got {tuple(t.shape)}")
    if X.shape[1] != Y.shape[1]:
        raise ValueError("sddmm: X and Y differ in their column count")
    return _Sddmm.apply(X, Y, A)


# ---------------------------------------------------------------- several heads
# The same three functions over [nnz, heads] edge values and [rows, heads, d] features,
# one launch per op (ops.*_heads): per head the bits of the one-head ops.

def _product_heads(A: CsrMatrix, val: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    heads, d = B.shape[1], B.shape[2]
    return ops.csrmm_heads(A.rowptr, A.colind, val, B, m=A.m, d=d, heads=heads, k=A.k)


def _f32_cuda(where: str, t, nm: str) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda:
        raise TypeError(f"{where}: {nm} must be a float32 tensor on a HIP device")


def _feature_cuda(where: str, t, nm: str) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype not in ops._FEATURE_TYPES or not t.is_cuda:
        raise TypeError(f"{where}: {nm} must be a float32, float16 or bfloat16 tensor on a HIP "
                        f"device")


class _SpmmHeads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, B: torch.Tensor, val: torch.Tensor, A: CsrMatrix) -> torch.Tensor:
        ctx.A = A
        B, val = B.detach().contiguous(), val.detach().contiguous()
        ctx.save_for_backward(B, val)
        return _product_heads(A, val, B).to(B.dtype)  # (fp32 features: the same tensor)

    @staticmethod
    def backward(ctx, grad_C: torch.Tensor):
        A = ctx.A
        B, val = ctx.saved_tensors
        grad_C = grad_C.contiguous()
        grad_B = grad_val = None
        if ctx.needs_input_grad[0]:
            vt = torch.index_select(val, 0, A.t_perm())  # a row gather of [nnz, heads]
            grad_B = _product_heads(A.t(), vt, grad_C).to(B.dtype)
        if ctx.needs_input_grad[1]:
            grad_val = ops.sddmm_heads(A.rowptr, A.colind, grad_C, B, m=A.m, k=A.k)
        return grad_B, grad_val, None


def spmm_heads(A: CsrMatrix, H: torch.Tensor, val: torch.Tensor) -> torch.Tensor:
    """C[i, h, :] = sum_p val[p, h] * H[col(p), h, :] on A's pattern (ops.csrmm_heads; H:
    [k, heads, d], val: [nnz, heads], C: [m, heads, d]), one launch for all heads. The
    backward gives grad_val = ops.sddmm_heads(grad_C, H) and grad_H = ops.csrmm_heads on
    A.t()'s pattern with the rows val[A.t_perm()], each only when it is needed: the
    transpose is not built for grad_val alone. No float atomics: two runs give the same
    bits.
    H may be float16 or bfloat16 with float32 val: C is then the fp32 product's bits cast to
    H's type (one round to nearest even), so grad_C arrives in H's type and both backward
    ops run on half features: grad_H is their fp32 result cast to H's type, grad_val stays
    float32."""
    if not isinstance(A, CsrMatrix):
        raise TypeError("spmm_heads: A must be a CsrMatrix")
    _feature_cuda("spmm_heads", H, "H")
    _f32_cuda("spmm_heads", val, "val")
    if H.dim() != 3 or H.shape[0] != A.k:
        raise ValueError(f"spmm_heads: H must be ({A.k}, heads, d), got {tuple(H.shape)}")
    if val.dim() != 2 or val.shape != (A.colind.numel(), H.shape[1]):
        raise ValueError(f"spmm_heads: val must be ({A.colind.numel()}, {H.shape[1]}), got "
                         f"{tuple(val.shape)}")
    return _SpmmHeads.apply(H, val, A)


class _EdgeSoftmaxHeads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, A: CsrMatrix) -> torch.Tensor:
        ctx.A = A
        y = ops.edge_softmax_heads(A.rowptr, x.detach().contiguous(), m=A.m)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, grad_y: torch.Tensor):
        (y,) = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        return ops.edge_softmax_bwd_heads(ctx.A.rowptr, y, grad_y.contiguous(), m=ctx.A.m), None


def edge_softmax_heads(A: CsrMatrix, e: torch.Tensor) -> torch.Tensor:
    """The softmax of every column of e ([nnz, heads]) over the positions of every row of
    A's pattern (ops.edge_softmax_heads); the backward is ops.edge_softmax_bwd_heads on the
    saved output. Heads never mix."""
    if not isinstance(A, CsrMatrix):
        raise TypeError("edge_softmax_heads: A must be a CsrMatrix")
    _f32_cuda("edge_softmax_heads", e, "e")
    if e.dim() != 2 or e.shape[0] != A.colind.numel():
        raise ValueError(f"edge_softmax_heads: e must be ({A.colind.numel()}, heads), got "
                         f"{tuple(e.shape)}")
    return _EdgeSoftmaxHeads.apply(e, A)


class _SddmmHeads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X: torch.Tensor, Y: torch.Tensor, A: CsrMatrix) -> torch.Tensor:
        ctx.A = A
        X, Y = X.detach().contiguous(), Y.detach().contiguous()
        ctx.save_for_backward(X, Y)
        return ops.sddmm_heads(A.rowptr, A.colind, X, Y, m=A.m, k=A.k)

    @staticmethod
    def backward(ctx, ge: torch.Tensor):
        A = ctx.A
        X, Y = ctx.saved_tensors
        ge = ge.contiguous()
        grad_X = grad_Y = None
        if ctx.needs_input_grad[0]:
            grad_X = _product_heads(A, ge, Y).to(X.dtype)
        if ctx.needs_input_grad[1]:
            grad_Y = _product_heads(A.t(), torch.index_select(ge, 0, A.t_perm()), X).to(Y.dtype)
        return grad_X, grad_Y, None


def sddmm_heads(A: CsrMatrix, X: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
    """e[p, h] = <X[row(p), h, :], Y[col(p), h, :]> on A's pattern (ops.sddmm_heads; X:
    [m, heads, d], Y: [k, heads, d]), with grad_X = ops.csrmm_heads(A, ge, Y) and grad_Y =
    ops.csrmm_heads on A.t() with the rows ge[A.t_perm()] applied to X, each only when it
    is needed. X may be Y; autograd then adds the two.
    X and Y may both be float16 or both bfloat16: e stays float32, and each gradient is the
    fp32 product's bits cast to the features' type."""
    if not isinstance(A, CsrMatrix):
        raise TypeError("sddmm_heads: A must be a CsrMatrix")
    for t, rows, nm in ((X, A.m, "X"), (Y, A.k, "Y")):
        _feature_cuda("sddmm_heads", t, nm)
        if t.dim() != 3 or t.shape[0] != rows:
            raise ValueError(f"sddmm_heads: {nm} must be ({rows}, heads, d), got "
                             f"{tuple(t.shape)}")
    if X.shape[1:] != Y.shape[1:]:
        raise ValueError("sddmm_heads: X and Y differ in heads or d")
    if X.dtype != Y.dtype:
        raise TypeError(f"sddmm_heads: X and Y must share a dtype, got {X.dtype} and {Y.dtype}")
    return _SddmmHeads.apply(X, Y, A)


# ---------------------------------------------------------------- max / min aggregation
class _SpmmReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, B: torch.Tensor, val: torch.Tensor | None, A: CsrMatrix,
                reduce: str) -> torch.Tensor:
        ctx.A = A
        B = B.detach().contiguous()
        C, arg = ops.csrmm_reduce(A.rowptr, A.colind, val, B, reduce=reduce, m=A.m,
                                  n=B.shape[1], k=A.k)
        ctx.save_for_backward(arg, *(() if val is None else (val,)))
        return C

    @staticmethod
    def backward(ctx, grad_C: torch.Tensor):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        A = ctx.A
        arg, *rest = ctx.saved_tensors
        At = A.t()
        grad_B = ops.csrmm_reduce_bwd(At.rowptr, At.colind, A.t_perm(), rest[0] if rest else None,
                                      grad_C.contiguous(), arg, k=A.k, n=arg.shape[1], m=A.m)
        return grad_B, None, None, None


def spmm_reduce(A: CsrMatrix, B: torch.Tensor, reduce: str = "max",
                val: torch.Tensor | None = None) -> torch.Tensor:
    """C[i, :] = max (min) over row i's positions p of val[p] * B[col(p), :] on A's pattern
    (ops.csrmm_reduce; B: [k, n] float32): GraphSAGE-pool / PNA aggregation, DGL's
    copy_u_max, PyG's aggr="max"; an empty row gives 0.

    val=None: the unweighted aggregation of B's rows; A.val is not read. val: a float32
    device tensor of nnz edge weights (A.val itself may be passed). It is a constant here:
    its gradient is a masked sampled product this library does not have, so a val that
    requires grad is refused, not silently treated as a constant; detach it.

    The forward keeps the winning positions; the backward is ops.csrmm_reduce_bwd on A.t()
    with A.t_perm(): each grad_C[i, j] goes to the one B row that won, summed over A^T's
    rows under the product's piece rule. No atomics: two runs give the same bits. The
    transpose is built once per matrix, on the first backward."""
    if not isinstance(A, CsrMatrix):
        raise TypeError("spmm_reduce: A must be a CsrMatrix")
    if reduce not in ("max", "min"):
        raise ValueError(f"spmm_reduce: reduce must be 'max' or 'min', got {reduce!r}")
    _f32_cuda("spmm_reduce", B, "B")
    if B.dim() != 2 or B.shape[0] != A.k:
        raise ValueError(f"spmm_reduce: B must be ({A.k}, n), got {tuple(B.shape)}")
    if val is not None:
        _f32_cuda("spmm_reduce", val, "val")
        if val.dim() != 1 or val.numel() != A.colind.numel():
            raise ValueError(f"spmm_reduce: val must hold the pattern's {A.colind.numel()} "
                             f"values, got {tuple(val.shape)}")
        if val.requires_grad:
            raise ValueError("spmm_reduce: val requires grad, but the gradient of the edge "
                             "values of a max / min aggregation is not served (a masked "
                             "sampled product); detach val")
        val = val.contiguous()
    return _SpmmReduce.apply(B, val, A, reduce)


__all__ = ["CsrMatrix", "spmm", "edge_softmax", "sddmm", "spmm_heads", "edge_softmax_heads",
           "sddmm_heads", "spmm_reduce"]
