"""autograd.spmm_reduce: B.grad has the bits of ops.csrmm_reduce_bwd, matches a float64
scatter and torch's CPU gradient of sparse.mm(reduce=...) within the product's fp32 bar on
tie-free inputs, refuses a val that requires grad, back-propagates through a chain with the
sum product, and builds A.t() once."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import reduce_cases as rc
from helpers import TOL_F32, assert_normwise

pytestmark = pytest.mark.gpu

N = 37
GRAD_SETS = ("generic", "generic_noval", "one_sign")  # no two distinct B rows tie


def _mods():
    from spmm_hip import autograd, ops
    return autograd, ops


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to("cuda")


def _matrix(pat, val=None):
    ag, _ = _mods()
    m, k, rp, ci = rc.pattern(pat)
    v = np.ones(ci.size, np.float32) if val is None else val
    return ag.CsrMatrix(_dev(rp), _dev(ci), _dev(v), m, k)


@pytest.mark.parametrize("pat", rc.PATTERNS)
def test_grad_bits_and_references(device, pat):
    import torch
    ag, ops = _mods()
    m, k, rp, ci = rc.pattern(pat)
    dC = rc.grad_out(pat, N, seed=2)
    for vs in GRAD_SETS:
        for reduce in rc.REDUCES:
            val, B = rc.values(pat, vs, reduce, N)
            A = _matrix(pat, val)
            Bd = _dev(B).requires_grad_()
            C = ag.spmm_reduce(A, Bd, reduce, val=_dev(val))
            wantC, wantA = rc.host_fwd(pat, vs, reduce, N)
            assert rc.same_bits(C.detach().cpu().numpy(), wantC)
            C.backward(_dev(dC))
            got = Bd.grad.cpu().numpy()
            At = A.t()
            direct = ops.csrmm_reduce_bwd(At.rowptr, At.colind, A.t_perm(), _dev(val), _dev(dC),
                                          _dev(wantA), k=k, n=N, m=m)
            what = f"{pat} {vs} {reduce}"
            assert rc.same_bits(got, direct.cpu().numpy()), what
            assert rc.same_bits(got, rc.host_bwd(pat, val, dC, wantA)), what
            ref, absdot = rc.scatter64(pat, val, wantA, dC)
            v = np.ones(ci.size, np.float32) if val is None else val
            T = torch.sparse_csr_tensor(torch.from_numpy(rp.astype(np.int64)),
                                        torch.from_numpy(ci.astype(np.int64)),
                                        torch.from_numpy(v), size=(m, k))
            Bt = torch.from_numpy(B).requires_grad_()
            torch.sparse.mm(T, Bt, "a" + reduce).backward(torch.from_numpy(dC))
            tg = Bt.grad.numpy()
            print(f"{what}: |grad - f64| {np.abs(got - ref).max():.3e}  |grad - torch| "
                  f"{np.abs(got - tg).max():.3e}  max |ref| {np.abs(ref).max():.3e}")
            assert_normwise(got, ref, absdot, TOL_F32, what + ": float64 scatter")
            assert_normwise(got, tg.astype(np.float64), absdot, TOL_F32, what + ": torch CPU")


def test_val_requiring_grad_is_refused(device):
    ag, _ = _mods()
    val, B = rc.values("lens", "generic", "max", N)
    A = _matrix("lens", val)
    w = _dev(val).requires_grad_()
    with pytest.raises(ValueError, match="requires grad"):
        ag.spmm_reduce(A, _dev(B), "max", val=w)
    ag.spmm_reduce(A, _dev(B), "max", val=w.detach())
    with pytest.raises(ValueError):
        ag.spmm_reduce(A, _dev(B), "mean")
    with pytest.raises(ValueError):
        ag.spmm_reduce(A, _dev(B)[:-1], "max")
    with pytest.raises(TypeError):
        ag.spmm_reduce(A, _dev(B).double(), "max")


def test_chain_with_linear_and_sum_product(device):
    """spmm_reduce -> linear -> spmm (sum) on a square pattern: the gradient reaches the input
    features and the weight, and equals the float64 chain built from the same arg."""
    ag, _ = _mods()
    pat = "hub_row"
    m, k, rp, ci = rc.pattern(pat)
    assert m == k
    rng = np.random.default_rng(3)
    val = rng.uniform(0.5, 1.5, ci.size).astype(np.float32)
    A = _matrix(pat, val)
    H = _dev(rng.standard_normal((k, N)).astype(np.float32)).requires_grad_()
    W = _dev((rng.standard_normal((N, 8)) / 6).astype(np.float32)).requires_grad_()
    pooled = ag.spmm_reduce(A, H, "max")                 # [m, N], unweighted
    out = ag.spmm(A, pooled @ W)                         # [m, 8]
    g = rng.standard_normal((m, 8)).astype(np.float32)
    out.backward(_dev(g))
    assert H.grad is not None and W.grad is not None
    assert torch.isfinite(H.grad).all() and torch.isfinite(W.grad).all()
    # float64: dZ = A^T g, dpooled = dZ W^T, dH = the scatter over arg
    _, arg = _prep().csrmm_reduce(m, N, k, rp, ci, None, H.detach().cpu().numpy())
    rows = np.repeat(np.arange(m), np.diff(rp))
    dZ, aZ = np.zeros((k, 8)), np.zeros((k, 8))
    np.add.at(dZ, ci, val[:, None].astype(np.float64) * g[rows])
    np.add.at(aZ, ci, np.abs(val[:, None].astype(np.float64) * g[rows]))
    W64 = W.detach().cpu().numpy().astype(np.float64)
    dP, aP = dZ @ W64.T, aZ @ np.abs(W64.T)
    ref, _ = rc.scatter64(pat, None, arg, dP)
    absdot, _ = rc.scatter64(pat, None, arg, aP)
    # three fp32 stages, each within the bar of its own absolute sum
    assert_normwise(H.grad.cpu().numpy(), ref, absdot, 3 * TOL_F32, "chain: H.grad")
    assert_normwise(W.grad.cpu().numpy(), pooled.detach().cpu().numpy().astype(np.float64).T @ dZ,
                    np.abs(pooled.detach().cpu().numpy().astype(np.float64)).T @ aZ,
                    2 * TOL_F32, "chain: W.grad")


def _prep():
    from spmm_hip import prep
    return prep


def test_transpose_is_built_once(device, monkeypatch):
    ag, ops = _mods()
    calls = []
    real = ops.csr2csc
    monkeypatch.setattr(ops, "csr2csc", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    val, B = rc.values("lens", "generic", "max", N)
    A = _matrix("lens", val)
    grads = []
    for _ in range(2):
        Bd = _dev(B).requires_grad_()
        ag.spmm_reduce(A, Bd, "min", val=_dev(val)).sum().backward()
        grads.append(Bd.grad.cpu().numpy())
    assert len(calls) == 1
    assert rc.same_bits(grads[0], grads[1])
