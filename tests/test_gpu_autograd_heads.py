"""spmm_hip.autograd over several heads: sddmm_heads, edge_softmax_heads and spmm_heads, and
the attention chain spmm_heads(A, H, val=edge_softmax_heads(A, sddmm_heads(A, H, H))).
Every gradient is bit-equal to the same composition written with ops.*_heads calls, across
two runs, and to the one-head autograd functions looped over the heads (the product under
SPMM_CSR_SEQUENTIAL_ROWS); a float64 torch composite is checked under the bound of
tests/test_gpu_autograd_softmax.py, derived the same way, per head."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from helpers import TOL_F32, assert_normwise

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

M, HEADS, D, HUB = 300, 4, 8, 2000


@functools.lru_cache(maxsize=None)
def _host():
    """A square M x M pattern with one row of HUB nonzeros (more than one softmax piece,
    16 product pieces; columns repeat), short rows and empty ones. Cached: read-only."""
    rng = np.random.default_rng(29)
    lens = rng.integers(0, 12, M)
    lens[17] = HUB
    lens[[0, 40, M - 1]] = 0
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(rp[-1])
    f = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)  # noqa: E731
    return dict(rp=rp, ci=rng.integers(0, M, nnz).astype(np.int32), v=f(nnz),
                H=f(M, HEADS, D), G=f(M, HEADS, D), w=f(nnz, HEADS), lens=lens)


def _setup():
    from spmm_hip import autograd
    host = _host()
    d = {key: torch.from_numpy(a).cuda() for key, a in host.items() if key != "lens"}
    return autograd, autograd.CsrMatrix(d["rp"], d["ci"], d["v"], M, M), d, host


def _leaves(d):
    """Three leaves with H's values: the product's B and the logits' X and Y, so that each
    gradient is seen on its own (a shared leaf would add the three)."""
    return [d["H"].clone().requires_grad_(True) for _ in range(3)]


def _chain(autograd, A, d):
    B, X, Y = _leaves(d)
    e = autograd.sddmm_heads(A, X, Y)
    e.retain_grad()
    a = autograd.edge_softmax_heads(A, e)
    a.retain_grad()
    out = autograd.spmm_heads(A, B, val=a)
    out.backward(d["G"])
    return [out.detach(), B.grad, X.grad, Y.grad, e.grad, a.grad]


NAMES = ["out", "grad_B", "grad_X", "grad_Y", "grad_e", "grad_a"]


def test_chain_equals_the_composition_of_ops_and_repeats(device):
    from spmm_hip import ops
    autograd, A, d, _ = _setup()
    got = _chain(autograd, A, d)
    again = _chain(autograd, A, d)
    for nm, g1, g2 in zip(NAMES, got, again):
        assert torch.equal(g1, g2), f"{nm}: two runs differ"
    H, G = d["H"], d["G"]
    kw = dict(m=M, k=M)
    e = ops.sddmm_heads(A.rowptr, A.colind, H, H, **kw)
    a = ops.edge_softmax_heads(A.rowptr, e, m=M)
    out = ops.csrmm_heads(A.rowptr, A.colind, a, H, d=D, heads=HEADS, **kw)
    At, perm = A.t(), A.t_perm()
    grad_a = ops.sddmm_heads(A.rowptr, A.colind, G, H, **kw)
    grad_B = ops.csrmm_heads(At.rowptr, At.colind, a[perm.long()].contiguous(), G, d=D,
                             heads=HEADS, **kw)
    grad_e = ops.edge_softmax_bwd_heads(A.rowptr, a, grad_a, m=M)
    grad_X = ops.csrmm_heads(A.rowptr, A.colind, grad_e, H, d=D, heads=HEADS, **kw)
    grad_Y = ops.csrmm_heads(At.rowptr, At.colind, grad_e[perm.long()].contiguous(), H, d=D,
                             heads=HEADS, **kw)
    for nm, g1, g2 in zip(NAMES, got, [out, grad_B, grad_X, grad_Y, grad_e, grad_a]):
        assert torch.equal(g1, g2), f"{nm}: differs from the composition of ops.*_heads"


def test_chain_equals_the_one_head_functions_looped(device):
    from spmm_hip import ops
    from spmm_hip._lib import CSR_NT_STREAMS, CSR_SEQUENTIAL_ROWS
    autograd, A, d, _ = _setup()
    got = _chain(autograd, A, d)
    h = ops.default_handle()
    h.set_csr_options(CSR_NT_STREAMS | CSR_SEQUENTIAL_ROWS)
    try:
        for hd in range(HEADS):
            B, X, Y = (d["H"][:, hd, :].clone().requires_grad_(True) for _ in range(3))
            e = autograd.sddmm(A, X, Y)
            e.retain_grad()
            a = autograd.edge_softmax(A, e)
            a.retain_grad()
            out = autograd.spmm(A, B, val=a)
            out.backward(d["G"][:, hd, :].contiguous())
            one = [out.detach(), B.grad, X.grad, Y.grad, e.grad, a.grad]
            for nm, g, o in zip(NAMES, got, one):
                sl = g[:, hd] if g.dim() == 2 else g[:, hd, :]
                assert torch.equal(sl, o), f"{nm}: head {hd} differs from the one-head functions"
    finally:
        torch.cuda.synchronize()
        h.set_csr_options(CSR_NT_STREAMS)  # the handle's default


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


def _rowsum(v, rows):
    return torch.zeros(M, dtype=torch.float64).index_add(0, rows, v)[rows]


def test_chain_against_float64(device):
    """Per head the float64 dense attention of tests/test_gpu_autograd_softmax.py, under
    its bound: |got - ref| <= 1e-5 * (the sum of the absolute values of the terms), the
    terms' bounds carried through the stages."""
    autograd, A, d, host = _setup()
    out, gB, gX, gY, _, _ = [t.cpu().numpy() for t in _chain(autograd, A, d)]
    rows, cols = _rows(host), torch.from_numpy(host["ci"].astype(np.int64))
    zeros = lambda: torch.zeros(M, D, dtype=torch.float64)  # noqa: E731
    for hd in range(HEADS):
        t64 = lambda a: torch.from_numpy(a[:, hd, :].astype(np.float64))  # noqa: E731
        B64, X64, Y64 = (t64(host["H"]).requires_grad_(True) for _ in range(3))
        G64 = t64(host["G"])
        a64 = _softmax64((X64[rows] * Y64[cols]).sum(1), host)
        out64 = zeros().index_add(0, rows, a64[:, None] * B64[cols])
        out64.backward(G64)
        Ha, Ga, a = B64.detach().abs(), G64.abs(), a64.detach()
        abs_out = zeros().index_add(0, rows, a[:, None] * Ha[cols])
        abs_ga = (Ga[rows] * Ha[cols]).sum(1)                  # grad of a: <G[row], H[col]>
        abs_ge = a * (abs_ga + _rowsum(a * abs_ga, rows))      # through the softmax
        abs_gB = zeros().index_add(0, cols, a[:, None] * Ga[rows])
        abs_gX = zeros().index_add(0, rows, abs_ge[:, None] * Ha[cols])
        abs_gY = zeros().index_add(0, cols, abs_ge[:, None] * Ha[rows])
        for nm, got, ref, absd in (("out", out, out64.detach(), abs_out),
                                   ("grad_B", gB, B64.grad, abs_gB),
                                   ("grad_X", gX, X64.grad, abs_gX),
                                   ("grad_Y", gY, Y64.grad, abs_gY)):
            assert_normwise(np.ascontiguousarray(got[:, hd, :]), ref.numpy(), absd.numpy(),
                            TOL_F32, f"{nm} head {hd}")


def test_gradients_are_computed_only_when_needed(device):
    autograd, A, d, _ = _setup()
    w = d["w"].clone().requires_grad_(True)
    autograd.spmm_heads(A, d["H"], val=w).backward(d["G"])
    assert A._t is None and A._perm is None and w.grad is not None  # grad_val alone
    X = d["H"].clone().requires_grad_(True)
    autograd.sddmm_heads(A, X, d["H"]).backward(d["w"])
    assert A._t is None and X.grad is not None                      # grad_X alone
    x = d["w"].clone().requires_grad_(True)
    autograd.edge_softmax_heads(A, x).backward(d["w"])
    assert A._t is None and x.grad is not None
    assert not autograd.edge_softmax_heads(A, d["w"]).requires_grad
    H = d["H"].clone().requires_grad_(True)
    autograd.spmm_heads(A, H, val=d["w"]).backward(d["G"])
    assert A._t is not None and H.grad is not None


def test_argument_checks(device):
    autograd, A, d, _ = _setup()
    H, w = d["H"], d["w"]
    for fn in (autograd.sddmm_heads, autograd.edge_softmax_heads, autograd.spmm_heads):
        with pytest.raises(TypeError):
            fn(None, H, H) if fn is not autograd.edge_softmax_heads else fn(None, w)
    with pytest.raises(ValueError):
        autograd.sddmm_heads(A, H.view(M, -1), H)          # rank
    with pytest.raises(ValueError):
        autograd.sddmm_heads(A, H[:-1], H)                 # length
    with pytest.raises(ValueError):
        autograd.sddmm_heads(A, H, H[:, :2])               # heads differ
    with pytest.raises(TypeError):
        autograd.sddmm_heads(A, H.double(), H)             # dtype
    with pytest.raises(TypeError):
        autograd.sddmm_heads(A, H.cpu(), H)                # device
    with pytest.raises(ValueError):
        autograd.edge_softmax_heads(A, w.view(-1))
    with pytest.raises(ValueError):
        autograd.edge_softmax_heads(A, w[:-1])
    with pytest.raises(TypeError):
        autograd.edge_softmax_heads(A, w.double())
    with pytest.raises(TypeError):
        autograd.edge_softmax_heads(A, w.cpu())
    with pytest.raises(ValueError):
        autograd.spmm_heads(A, H.view(M, -1), val=w)
    with pytest.raises(ValueError):
        autograd.spmm_heads(A, H, val=w[:, :2])
    with pytest.raises(ValueError):
        autograd.spmm_heads(A, H, val=w[:-1])
    with pytest.raises(TypeError):
        autograd.spmm_heads(A, H, val=w.double())
    with pytest.raises(TypeError):
        autograd.spmm_heads(A, H.cpu(), val=w)
