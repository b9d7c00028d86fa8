"""spmm_hip.autograd over several heads on float16 and bfloat16 features: sddmm_heads and
spmm_heads, and the attention chain spmm_heads(A, Hh, val=edge_softmax_heads(A,
sddmm_heads(A, Hh, Hh))). The logits, the softmax and every edge gradient stay float32; a
result that takes the features' place (the output, a feature gradient) is the fp32 kernels'
result cast to the features' type once. Every tensor of the chain is bit-equal to that
composition written with ops.*_heads calls and .to(dtype) at those points, across two runs;
a float64 dense computation with the same casts at the same points is checked under a
derived bound."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from helpers import TOL_F32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

M, HEADS, D, HUB = 300, 4, 8, 2000
TYPES = {"f16": (torch.float16, 2.0 ** -10), "bf16": (torch.bfloat16, 2.0 ** -7)}


@functools.lru_cache(maxsize=None)
def _host():
    """tests/test_gpu_autograd_heads.py's pattern: M x M, one row of HUB nonzeros, short
    rows and empty ones. Cached: read-only."""
    rng = np.random.default_rng(29)
    lens = rng.integers(0, 12, M)
    lens[17] = HUB
    lens[[0, 40, M - 1]] = 0
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(rp[-1])
    f = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)  # noqa: E731
    return dict(rp=rp, ci=rng.integers(0, M, nnz).astype(np.int32), v=f(nnz),
                H=f(M, HEADS, D), G=f(M, HEADS, D), w=f(nnz, HEADS), lens=lens)


def _setup(ty):
    """H and G rounded to the storage type (torch's cast: round to nearest even)."""
    from spmm_hip import autograd
    host = _host()
    d = {key: torch.from_numpy(a).cuda() for key, a in host.items() if key != "lens"}
    d["H"], d["G"] = d["H"].to(TYPES[ty][0]), d["G"].to(TYPES[ty][0])
    return autograd, autograd.CsrMatrix(d["rp"], d["ci"], d["v"], M, M), d, host


def _chain(autograd, A, d):
    """Three leaves with H's values, so that each gradient is seen on its own."""
    B, X, Y = (d["H"].clone().requires_grad_(True) for _ in range(3))
    e = autograd.sddmm_heads(A, X, Y)
    e.retain_grad()
    a = autograd.edge_softmax_heads(A, e)
    a.retain_grad()
    out = autograd.spmm_heads(A, B, val=a)
    out.backward(d["G"])
    return [out.detach(), B.grad, X.grad, Y.grad, e.grad, a.grad]


NAMES = ["out", "grad_B", "grad_X", "grad_Y", "grad_e", "grad_a"]


@pytest.mark.parametrize("ty", list(TYPES))
def test_chain_equals_the_composition_of_ops_and_repeats(device, ty):
    from spmm_hip import ops
    dt = TYPES[ty][0]
    autograd, A, d, _ = _setup(ty)
    got = _chain(autograd, A, d)
    again = _chain(autograd, A, d)
    for nm, g1, g2 in zip(NAMES, got, again):
        assert torch.equal(g1, g2), f"{nm}: two runs differ"
    for nm, g, want in zip(NAMES, got, [dt, dt, dt, dt, torch.float32, torch.float32]):
        assert g.dtype == want, (nm, g.dtype)
    H, G = d["H"], d["G"]
    kw = dict(m=M, k=M)
    hd = dict(d=D, heads=HEADS, **kw)
    e = ops.sddmm_heads(A.rowptr, A.colind, H, H, **kw)
    assert e.dtype == torch.float32
    a = ops.edge_softmax_heads(A.rowptr, e, m=M)
    out = ops.csrmm_heads(A.rowptr, A.colind, a, H, **hd).to(dt)
    At, perm = A.t(), A.t_perm()
    grad_a = ops.sddmm_heads(A.rowptr, A.colind, G, H, **kw)
    grad_B = ops.csrmm_heads(At.rowptr, At.colind, a[perm.long()].contiguous(), G, **hd).to(dt)
    grad_e = ops.edge_softmax_bwd_heads(A.rowptr, a, grad_a, m=M)
    grad_X = ops.csrmm_heads(A.rowptr, A.colind, grad_e, H, **hd).to(dt)
    grad_Y = ops.csrmm_heads(At.rowptr, At.colind, grad_e[perm.long()].contiguous(), H,
                             **hd).to(dt)
    for nm, g1, g2 in zip(NAMES, got, [out, grad_B, grad_X, grad_Y, grad_e, grad_a]):
        assert torch.equal(g1, g2), f"{nm}: differs from the composition of ops.*_heads"
    # a shared leaf backpropagates on all three paths, with the same bits on every run
    grads = []
    for _ in range(2):
        Hh = H.clone().requires_grad_(True)
        autograd.spmm_heads(A, Hh, val=autograd.edge_softmax_heads(
            A, autograd.sddmm_heads(A, Hh, Hh))).backward(G)
        assert Hh.grad.dtype == dt
        grads.append(Hh.grad)
    assert torch.equal(grads[0], grads[1])
    assert not torch.equal(grads[0], grad_B) and torch.isfinite(grads[0].float()).all()


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


@pytest.mark.parametrize("ty", list(TYPES))
def test_chain_against_float64(device, ty):
    """Per head a float64 dense attention on the rounded H and G (exact in float64), against
    the chain's half results widened.

    Bound, derived and not measured. tests/test_gpu_autograd_heads.py bounds the fp32 chain
    by |got32 - ref| <= TOL_F32 * absd, absd the sum of the absolute values of the terms
    carried through the stages; that part is unchanged, because the kernels compute in
    fp32 on exactly these inputs. On top comes what a cast adds. Every checked quantity is
    one round-to-nearest-even cast of an fp32 result, |cast(x) - x| <= u |x| / 2 with u one
    ulp of the storage type relative to the value (2^-10 for fp16, 2^-7 for bf16), and
    |x| <= |ref| + TOL_F32 absd <= (1 + TOL_F32) absd, because absd bounds |ref| term by
    term. The issue's term of one whole ulp, u * absd, covers u (1 + TOL_F32) absd / 2.
    grad_X and grad_Y also pass through grad_C = G, which is given in the storage type: it
    is an input here (G is rounded before both computations), so it adds no further cast;
    out is not an input of any checked gradient (grad_a = sddmm(G, H) uses G and H alone).
    So for each of out, grad_B, grad_X, grad_Y: |got - ref| <= (TOL_F32 + u) * absd.
    Subnormal results of the storage type are not met (|values| are far above 2^-14)."""
    u = TYPES[ty][1]
    autograd, A, d, host = _setup(ty)
    out, gB, gX, gY, _, _ = [t.float().cpu().numpy() for t in _chain(autograd, A, d)]
    Hr, Gr = d["H"].float().cpu().numpy(), d["G"].float().cpu().numpy()
    rows, cols = _rows(host), torch.from_numpy(host["ci"].astype(np.int64))
    zeros = lambda: torch.zeros(M, D, dtype=torch.float64)  # noqa: E731
    for hd in range(HEADS):
        t64 = lambda a: torch.from_numpy(a[:, hd, :].astype(np.float64))  # noqa: E731
        B64, X64, Y64 = (t64(Hr).requires_grad_(True) for _ in range(3))
        G64 = t64(Gr)
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
            err = np.abs(got[:, hd, :].astype(np.float64) - ref.numpy())
            bound = (TOL_F32 + u) * absd.numpy()
            worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
            print(f"{ty} {nm} head {hd}: worst |err| / bound = {worst:.3f}")
            assert (err <= bound).all(), (ty, nm, hd, worst)


@pytest.mark.parametrize("ty", list(TYPES))
def test_gradients_are_computed_only_when_needed(device, ty):
    dt = TYPES[ty][0]
    autograd, A, d, _ = _setup(ty)
    w = d["w"].clone().requires_grad_(True)
    autograd.spmm_heads(A, d["H"], val=w).backward(d["G"])
    assert A._t is None and A._perm is None                     # grad_val alone: no transpose
    assert w.grad is not None and w.grad.dtype == torch.float32
    X = d["H"].clone().requires_grad_(True)
    autograd.sddmm_heads(A, X, d["H"]).backward(d["w"])
    assert A._t is None and X.grad is not None and X.grad.dtype == dt   # grad_X alone
    H = d["H"].clone().requires_grad_(True)
    autograd.spmm_heads(A, H, val=d["w"]).backward(d["G"])
    assert A._t is not None and H.grad is not None and H.grad.dtype == dt


def test_float32_behaviour_is_unchanged(device):
    """fp32 features give fp32 results with the bits of ops.*_heads, and the type checks of
    the fp32 functions stand: float64 and CPU tensors, a half val, a half e, mixed X / Y."""
    from spmm_hip import ops
    autograd, A, d, _ = _setup("f16")
    H32, G32, w = d["H"].float(), d["G"].float(), d["w"]
    B = H32.clone().requires_grad_(True)
    out = autograd.spmm_heads(A, B, val=w)
    assert out.dtype == torch.float32
    assert torch.equal(out.detach(), ops.csrmm_heads(A.rowptr, A.colind, w, H32, m=M, d=D,
                                                     heads=HEADS, k=M))
    out.backward(G32)
    assert B.grad.dtype == torch.float32
    e = autograd.sddmm_heads(A, H32, H32)
    assert e.dtype == torch.float32
    assert torch.equal(e, ops.sddmm_heads(A.rowptr, A.colind, H32, H32, m=M, k=M))
    with pytest.raises(TypeError):
        autograd.sddmm_heads(A, H32.double(), H32)
    with pytest.raises(TypeError):
        autograd.sddmm_heads(A, H32.cpu(), H32)
    with pytest.raises(TypeError):
        autograd.sddmm_heads(A, d["H"], H32)                 # half X, fp32 Y
    with pytest.raises(TypeError):
        autograd.sddmm_heads(A, d["H"], d["H"].bfloat16())   # fp16 X, bf16 Y
    with pytest.raises(TypeError):
        autograd.spmm_heads(A, d["H"], val=w.half())         # edge values stay fp32
    with pytest.raises(TypeError):
        autograd.spmm_heads(A, H32, val=w.double())
    with pytest.raises(TypeError):
        autograd.edge_softmax_heads(A, w.half())             # no half edge softmax
    with pytest.raises(TypeError):
        autograd.spmm_heads(A, d["H"].cpu(), val=w)
