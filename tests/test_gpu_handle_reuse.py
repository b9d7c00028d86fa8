"""One handle across the entry families: what a product leaves in the handle must not
reach the next one.

A handle owns five device buffers that different entries reinterpret: ws (CSR piece
slots, staged B and C, the converters' and the group analyses' arrays), scratch
(segment partial tiles, probe sums, dirty flags, hot-column counts), order (a block-row
permutation or int4 segment lists), tickets (all zero between launches) and grp_pend;
plus the hybrid's staging buffer. Principle: the same call with the same arguments
gives the same bits on a handle that has just run other entries as on a handle created
for that call alone (the determinism tools/determinism.py and the *_bits tests rely on).

Control first: every step runs on two fresh handles and must give equal bits, and the
first of those results is held to the step's oracle with the bar of the entry's own
test (two equal wrong answers must not pass). Then the steps run in sequence on one
handle, forward (with a, d, f once more at the end: a small request after large ones),
backward, and forward on a handle bound to a side stream from its creation; each
result is compared bit for bit with the fresh handle's. No graph capture, no stream
change inside a sequence, one handle at a time.

  a  CSR, n = 256, column-major B and C, one hub row of 40,000 nonzeros: split rows
     (tickets, piece slots in ws) and both staging areas of ws
  b  the same matrix row-major at n = 64 under set_csr_waves_per_cu(32), (1), (0): the
     carry size and the ticket grid change under one handle
  c  csr_hot_analysis + csrmm_hot: column counts in scratch
  d  bs 32 ROW blocks, row-major C, one block row of 300 blocks on a shallow grid:
     order holds segment lists, scratch the partial tiles
  e  the same with column-major B and C: B staged in ws, order a plain permutation
  f  bs 8, then bs 2, under SPMM_BSR_SMALL_GROUPED, each followed at once by
     small_bsr_path(): probe sums and dirty flags in scratch
  g  the hybrid at bs 32 with column-major B and C, then the row-major form
  h  bs 16 fp16 with a column-major B: halves staged in ws
  i  GroupedBsr16 and GroupedBsr32: analysis (size query + fill) and a product each
  j  csr2bsr and bsr2csr on the device: ws carved up by the converters
  k  the fp64 CSR and BSR entries"""
from __future__ import annotations

import numpy as np
import pytest

from helpers import (HYBRID_EX_M, REUSE_HUB_K, REUSE_HUB_M, REUSE_SEG_SHAPE, TOL_F16_ACC, TOL_F32,
                     assert_normwise, column_sparse_bsr, hybrid_ex_matrix, hybrid_ex_parts,
                     long_row_column_sparse_bsr, oracle_bsrmm_d, oracle_bsrmm_f32, oracle_bsrmm_f64,
                     oracle_csrmm_d, oracle_csrmm_f64, rand_bsr, reuse_hub_csr)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

COL = 1
STEPS = "abcdefghijk"
_state: dict = {}


def _ops():
    from spmm_hip import ops
    return ops


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _read(h, *tensors):
    """One synchronise of the handle's stream, then the readback."""
    h.stream.synchronize()
    return [t.cpu().numpy() for t in tensors]


def _nan(count, device):
    return torch.full((count,), float("nan"), device=device)


def _expect(ref, absd, C0, alpha, beta):
    C0 = C0.astype(np.float64)
    return alpha * ref + beta * C0, abs(alpha) * absd + abs(beta) * np.abs(C0)


def _pad_rows(a, rows):
    out = np.zeros((rows, a.shape[1]), a.dtype)
    out[:a.shape[0]] = a
    return out


# ------------------------------------------------------------------ inputs
def _inputs():
    """Host operands of every step, generated once; "d_*" entries are their device
    copies (inputs only: every run allocates its own C)."""
    if "inputs" in _state:
        return _state["inputs"]
    from spmm_hip import prep
    from test_gpu_bsr import _grouped_small_bsr
    I: dict = {}
    rng = np.random.default_rng(9000)
    # a, b, c: the hub matrix
    m, k = REUSE_HUB_M, REUSE_HUB_K
    I["csr"] = reuse_hub_csr()
    I["a_B"] = rng.uniform(-1, 1, (k, 256)).astype(np.float32)
    I["a_C0"] = rng.uniform(-1, 1, (m, 256)).astype(np.float32)
    I["b_B"] = rng.uniform(-1, 1, (k, 64)).astype(np.float32)
    I["d_csr"] = _dev(*I["csr"])
    I["d_a_Bt"], I["d_b_B"] = _dev(I["a_B"].T, I["b_B"])
    # d, e: one long block row on a shallow grid
    mb, kb, bs, n = REUSE_SEG_SHAPE
    # (a generator of its own: tests/test_hybrid_helpers.py rebuilds the matrix)
    I["seg"] = long_row_column_sparse_bsr(np.random.default_rng(9001), mb, kb, bs)
    I["seg_B"] = rng.uniform(-1, 1, (kb * bs, n)).astype(np.float32)
    I["seg_C0"] = rng.uniform(-1, 1, (mb * bs, n)).astype(np.float32)
    I["d_seg"] = _dev(*I["seg"])
    I["d_seg_B"], I["d_seg_Bt"] = _dev(I["seg_B"], I["seg_B"].T)
    # f: the matrices of test_small_bs_grouped_stream_bit_exact
    for sb in (8, 2):
        G = 32 // sb
        fmb, fkb = 5 * G + 3, 160
        rp, ci, vb = _grouped_small_bsr(rng, sb, fmb, fkb)
        I[f"small{sb}"] = rp, ci, vb.reshape(-1)
        I[f"small{sb}_B"] = rng.uniform(-1, 1, (fkb * sb, 128)).astype(np.float32)
        I[f"small{sb}_C0"] = rng.uniform(-1, 1, (fmb * sb, 128)).astype(np.float32)
        I[f"d_small{sb}"] = _dev(*I[f"small{sb}"])
        I[f"d_small{sb}_B"] = _dev(I[f"small{sb}_B"])[0]
    # g: the hybrid's matrix at bs 32
    I["hyb"] = hybrid_ex_parts(32)
    I["hyb_B"] = rng.uniform(-1, 1, (HYBRID_EX_M, 64)).astype(np.float32)
    I["hyb_C0"] = rng.uniform(-1, 1, (704, 64)).astype(np.float32)
    I["d_hyb"] = _dev(*I["hyb"])
    I["d_hyb_Bt"], I["d_hyb_Bp"] = _dev(I["hyb_B"].T, _pad_rows(I["hyb_B"], 704))
    # h: test_bsrmm_f16's shape
    rp, ci, v = rand_bsr(rng, 19, 25, 16, 0.27, empty_rows=(0,))
    I["h16"] = rp, ci, v.astype(np.float16)
    I["h16_B"] = rng.uniform(-1, 1, (25 * 16, 128)).astype(np.float16)
    I["d_h16"] = _dev(*I["h16"])
    I["d_h16_Bt"] = _dev(I["h16_B"].T)[0]
    # i: test_bsrmm_grouped_f16 / _f32's shape
    rp, ci, v = column_sparse_bsr(rng, 37, 60, 16, 0.3)
    I["g16"] = rp, ci, v.astype(np.float16)
    I["g16_B"] = rng.uniform(-1, 1, (60 * 16, 256)).astype(np.float16)
    I["g32"] = column_sparse_bsr(rng, 37, 60, 32, 0.3)
    I["g32_B"] = rng.uniform(-1, 1, (60 * 32, 128)).astype(np.float32)
    I["g_C0"] = rng.uniform(-1, 1, (37 * 32, 256)).astype(np.float32)
    I["d_g16"], I["d_g32"] = _dev(*I["g16"]), _dev(*I["g32"])
    I["d_g16_B"], I["d_g32_B"] = _dev(I["g16_B"], I["g32_B"])
    # j: the hybrid's whole matrix through the converters
    I["conv"] = hybrid_ex_matrix()
    I["conv_bsr"] = prep.csr2bsr(HYBRID_EX_M, HYBRID_EX_M, *I["conv"], 4)
    I["conv_csr"] = prep.bsr2csr(175, 175, *I["conv_bsr"], 4)
    I["d_conv"] = _dev(*I["conv"])
    # k: test_csrmm_f64 / test_bsrmm_f64's shapes
    deg = rng.integers(0, 41, 517)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    ci = np.concatenate([np.sort(rng.choice(389, d, replace=False)) for d in deg]).astype(np.int32)
    I["c64"] = rp, ci, rng.standard_normal(ci.size)
    I["c64_Bt"] = rng.standard_normal((70, 389))
    I["c64_C0t"] = rng.standard_normal((70, 517))
    mask = rng.random((23, 19)) < 0.25
    I["b64"] = (np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int32),
                np.nonzero(mask)[1].astype(np.int32), rng.standard_normal(int(mask.sum()) * 64))
    I["b64_B"] = rng.standard_normal((19 * 8, 70))
    I["b64_C0"] = rng.standard_normal((23 * 8, 70))
    I["d_c64"], I["d_b64"] = _dev(*I["c64"]), _dev(*I["b64"])
    I["d_c64_Bt"], I["d_b64_B"] = _dev(I["c64_Bt"], I["b64_B"])
    torch.cuda.synchronize()  # every input is ready before the first call on any stream
    _state["inputs"] = I
    return I


# ------------------------------------------------------------------- steps
# run_x(h, I, device) -> list of host arrays; check_x(outs, I, oracle) holds them to the oracle
A_AB = (0.7, -1.3)


def run_a(h, I, device):
    ops = _ops()
    C = _dev(I["a_C0"].T)[0]
    ops.csrmm(*I["d_csr"], I["d_a_Bt"], m=REUSE_HUB_M, n=256, k=REUSE_HUB_K, ldb=REUSE_HUB_K,
              order_b=COL, C=C, ldc=REUSE_HUB_M, order_c=COL, alpha=A_AB[0], beta=A_AB[1], handle=h)
    return _read(h, C)


def check_a(outs, I, oracle):
    ref, absd = oracle_csrmm_f64(oracle, REUSE_HUB_M, 256, *I["csr"], I["a_B"], 256, 0)
    want, scale = _expect(ref, absd, I["a_C0"], *A_AB)
    assert_normwise(outs[0].T, want, scale, TOL_F32, "step a")


def run_b(h, I, device):
    ops = _ops()
    Cs = []
    for w in (32, 1, 0):  # ends on the default
        h.set_csr_waves_per_cu(w)
        C = _nan(REUSE_HUB_M * 64, device)
        ops.csrmm(*I["d_csr"], I["d_b_B"], m=REUSE_HUB_M, n=64, k=REUSE_HUB_K, ldb=64, C=C, ldc=64,
                  handle=h)
        Cs.append(C)
    return _read(h, *Cs)


def check_b(outs, I, oracle):
    ref, absd = oracle_csrmm_f64(oracle, REUSE_HUB_M, 64, *I["csr"], I["b_B"], 64, 0)
    for w, got in zip((32, 1, 0), outs):
        assert_normwise(got.reshape(REUSE_HUB_M, 64), ref, absd, TOL_F32, f"step b waves_per_cu={w}")


def run_c(h, I, device):
    ops = _ops()
    rp, ci, v = I["d_csr"]
    tag = ops.csr_hot_analysis(ci, n=64, k=REUSE_HUB_K, hot_bytes=400 * 256, handle=h)
    C = _nan(REUSE_HUB_M * 64, device)
    ops.csrmm_hot(rp, tag, v, I["d_b_B"], m=REUSE_HUB_M, n=64, k=REUSE_HUB_K, ldb=64, C=C, ldc=64,
                  handle=h)
    return _read(h, tag, C)


def check_c(outs, I, oracle):
    tag, got = outs
    ci = I["csr"][1]
    assert 0 < int((tag < 0).sum()) < ci.size, "step c: tags"
    assert np.array_equal(tag & 0x7FFFFFFF, ci), "step c: tagged indices"
    ref, absd = oracle_csrmm_f64(oracle, REUSE_HUB_M, 64, *I["csr"], I["b_B"], 64, 0)
    assert_normwise(got.reshape(REUSE_HUB_M, 64), ref, absd, TOL_F32, "step c")


def run_d(h, I, device):
    mb, kb, bs, n = REUSE_SEG_SHAPE
    C = _nan(mb * bs * n, device)
    _ops().bsrmm(*I["d_seg"], I["d_seg_B"], mb=mb, kb=kb, n=n, bs=bs, ldb=n, C=C, ldc=n, handle=h)
    return _read(h, C)


def _seg_oracle(I, oracle):
    mb, kb, bs, n = REUSE_SEG_SHAPE
    return oracle_bsrmm_f64(oracle, 0, mb, n, bs, *I["seg"], I["seg_B"], n, 0)


def check_d(outs, I, oracle):
    mb, kb, bs, n = REUSE_SEG_SHAPE
    ref, absd = _seg_oracle(I, oracle)
    assert_normwise(outs[0].reshape(mb * bs, n), ref, absd, TOL_F32, "step d")


E_AB = (0.5, -1.5)


def run_e(h, I, device):
    mb, kb, bs, n = REUSE_SEG_SHAPE
    C = _dev(I["seg_C0"].T)[0]
    _ops().bsrmm(*I["d_seg"], I["d_seg_Bt"], mb=mb, kb=kb, n=n, bs=bs, ldb=kb * bs, order_b=COL,
                 C=C, ldc=mb * bs, order_c=COL, alpha=E_AB[0], beta=E_AB[1], handle=h)
    return _read(h, C)


def check_e(outs, I, oracle):
    want, scale = _expect(*_seg_oracle(I, oracle), I["seg_C0"], *E_AB)
    assert_normwise(outs[0].T, want, scale, TOL_F32, "step e")


F_AB = (0.5, -2.0)


def run_f(h, I, device):
    from spmm_hip._lib import BSR_SMALL_GROUPED
    ops = _ops()
    outs = []
    h.set_bsr_options(BSR_SMALL_GROUPED)
    try:
        for sb in (8, 2):
            rp = I[f"small{sb}"][0]
            mb = rp.size - 1
            C = _dev(I[f"small{sb}_C0"])[0]
            ops.bsrmm(*I[f"d_small{sb}"], I[f"d_small{sb}_B"], mb=mb, kb=160, n=128, bs=sb, ldb=128,
                      C=C, ldc=128, alpha=F_AB[0], beta=F_AB[1], handle=h)
            path = h.small_bsr_path()  # right after the product (include/spmm_hip.h)
            outs += _read(h, C) + [np.array([path], np.int32)]
    finally:
        h.set_bsr_options(0)
    return outs


def check_f(outs, I, oracle):
    for sb, got, path in ((8, outs[0], outs[1]), (2, outs[2], outs[3])):
        rp, ci, v = I[f"small{sb}"]
        mb = rp.size - 1
        want = oracle_bsrmm_f32(oracle, 0, mb, 128, sb, rp, ci, v, I[f"small{sb}_B"], 128, 0, F_AB[0],
                                F_AB[1], I[f"small{sb}_C0"], 128, 0)
        got, want = got.ravel(), want.ravel()
        assert (got == want).all(), f"step f bs {sb}: {int((got != want).sum())} elements differ"
        assert int(path[0]) in (1, 2), f"step f bs {sb}: the grouped branch was not taken ({path[0]})"


G_AB = (0.5, -1.5)


def run_g(h, I, device):
    ops = _ops()
    d = I["d_hyb"]
    m = HYBRID_EX_M
    Cc = _dev(I["hyb_C0"].T)[0]
    ops.hybrid_csrmm(tuple(d[0:3]), tuple(d[3:6]), I["d_hyb_Bt"], m=m, n=64, k=m, bs=32, ldb=m, C=Cc,
                     ldc=704, alpha=G_AB[0], beta=G_AB[1], order_b=COL, order_c=COL, handle=h)
    Cr = _dev(I["hyb_C0"])[0]
    ops.hybrid_csrmm(tuple(d[0:3]), tuple(d[3:6]), I["d_hyb_Bp"], m=m, n=64, k=m, bs=32, ldb=64, C=Cr,
                     ldc=64, alpha=G_AB[0], beta=G_AB[1], handle=h)
    return _read(h, Cc, Cr)


def check_g(outs, I, oracle):
    ref, absd = oracle_csrmm_f64(oracle, HYBRID_EX_M, 64, *hybrid_ex_matrix(), I["hyb_B"], 64, 0)
    want, scale = _expect(_pad_rows(ref, 704), _pad_rows(absd, 704), I["hyb_C0"], *G_AB)
    assert_normwise(outs[0].T, want, scale, TOL_F32, "step g column-major")
    assert_normwise(outs[1], want, scale, TOL_F32, "step g row-major")


def run_h(h, I, device):
    C = _nan(19 * 16 * 128, device)
    _ops().bsrmm_f16(*I["d_h16"], I["d_h16_Bt"], mb=19, kb=25, n=128, bs=16, ldb=25 * 16, order_b=COL,
                     C=C, ldc=128, handle=h)
    return _read(h, C)


def check_h(outs, I, oracle):
    ref, absd = oracle_bsrmm_f64(oracle, 0, 19, 128, 16, *I["h16"], I["h16_B"], 128, 0, half=True)
    assert_normwise(outs[0].reshape(19 * 16, 128), ref, absd, TOL_F16_ACC, "step h")


I_AB = (0.5, -1.0)


def run_i(h, I, device):
    ops = _ops()
    outs = []
    for cls, key, bs, n, W in ((ops.GroupedBsr16, "g16", 16, 256, 4), (ops.GroupedBsr32, "g32", 32, 128, 2)):
        C = _dev(I["g_C0"][:37 * bs, :n])[0]
        with cls(*I[f"d_{key}"], mb=37, group_rows=W, handle=h) as grp:
            grp.mm(I[f"d_{key}_B"], kb=60, n=n, ldb=n, C=C, ldc=n, alpha=I_AB[0], beta=I_AB[1])
            outs += _read(h, C) + [np.array([grp.W, grp.nitems, grp.bytes], np.int64)]
    return outs


def check_i(outs, I, oracle):
    for (key, bs, n, tol), got in zip((("g16", 16, 256, TOL_F16_ACC), ("g32", 32, 128, TOL_F32)),
                                      (outs[0], outs[2])):
        ref, absd = oracle_bsrmm_f64(oracle, 0, 37, n, bs, *I[key], I[f"{key}_B"], n, 0, half=bs == 16)
        want, scale = _expect(ref, absd, I["g_C0"][:37 * bs, :n], *I_AB)
        assert_normwise(got, want, scale, tol, f"step i bs {bs}")


def run_j(h, I, device):
    ops = _ops()
    m = HYBRID_EX_M
    bsr = ops.csr2bsr(*I["d_conv"], m=m, n=m, bs=4, handle=h)
    csr = ops.bsr2csr(*bsr, mb=175, nb=175, bs=4, handle=h)
    return _read(h, *bsr, *csr)


def check_j(outs, I, oracle):
    for got, want, nm in zip(outs, tuple(I["conv_bsr"]) + tuple(I["conv_csr"]),
                             ("bsr rowptr", "bsr colind", "bsr val", "csr rowptr", "csr colind", "csr val")):
        assert got.dtype == want.dtype and np.array_equal(got, want), f"step j: {nm}"


K_AB = (0.75, -1.5)


def run_k(h, I, device):
    ops = _ops()
    Cc, Cb = _dev(I["c64_C0t"], I["b64_C0"])
    ops.csrmm(*I["d_c64"], I["d_c64_Bt"], m=517, n=70, k=389, ldb=389, order_b=COL, C=Cc, ldc=517,
              order_c=COL, alpha=K_AB[0], beta=K_AB[1], handle=h)
    ops.bsrmm(*I["d_b64"], I["d_b64_B"], mb=23, kb=19, n=70, bs=8, ldb=70, C=Cb, ldc=70,
              alpha=K_AB[0], beta=K_AB[1], handle=h)
    return _read(h, Cc, Cb)


def check_k(outs, I, oracle):
    want = oracle_csrmm_d(oracle, 517, 70, *I["c64"], I["c64_Bt"], 389, 1, K_AB[0], K_AB[1],
                          I["c64_C0t"].ravel(), 517, 1)
    assert np.array_equal(outs[0].ravel(), want), "step k csr"
    want = oracle_bsrmm_d(oracle, 0, 23, 70, 8, *I["b64"], I["b64_B"], 70, 0, K_AB[0], K_AB[1],
                          I["b64_C0"].ravel(), 70, 0)
    assert np.array_equal(outs[1].ravel(), want), "step k bsr"


def _step(name):
    g = globals()
    return g["run_" + name], g["check_" + name]


# ------------------------------------------------------------- comparisons
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _differs(outs, fresh):
    """Index of the first array of outs whose bits differ from fresh's, or None."""
    assert len(outs) == len(fresh)
    for i, (a, b) in enumerate(zip(outs, fresh)):
        if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(_bits(a), _bits(b)):
            return i
    return None


def _fresh(name, device):
    """The step on two handles created for it alone: (first result, index of the first
    array on which the second differs or None). Once per step."""
    key = ("fresh", name)
    if key not in _state:
        I = _inputs()
        runs = []
        for _ in range(2):
            h = _ops().Handle()
            runs.append(_step(name)[0](h, I, device))
            h.close()
        _state[key] = runs[0], _differs(runs[1], runs[0])
    return _state[key]


@pytest.mark.parametrize("name", list(STEPS))
def test_fresh_handles_agree_and_match_the_oracle(oracle, device, name):
    """The control: two fresh handles give the same bits, and those bits are right."""
    outs, diff = _fresh(name, device)
    _step(name)[1](outs, _inputs(), oracle)
    assert diff is None, f"step {name}: output {diff} differs between two fresh handles"


def _sequence(order, h, device, oracle):
    """Run the steps of `order` on h; every result must carry the fresh handle's bits. A
    step whose control failed (not reproducible run to run) is held to its oracle."""
    I = _inputs()
    bad = []
    for pos, name in enumerate(order):
        fresh, control = _fresh(name, device)
        outs = _step(name)[0](h, I, device)
        if control is not None:
            _step(name)[1](outs, I, oracle)
            continue
        i = _differs(outs, fresh)
        if i is not None:
            bad.append(f"step {name} (position {pos}, after {order[:pos] or 'nothing'}): output {i}")
    assert not bad, "results changed by what earlier entries left in the handle: " + "; ".join(bad)


def test_reuse_forward(oracle, device):
    h = _ops().Handle()
    _sequence(STEPS + "adf", h, device, oracle)
    h.close()


def test_reuse_reverse(oracle, device):
    h = _ops().Handle()
    _sequence(STEPS[::-1], h, device, oracle)
    h.close()


def test_reuse_on_a_side_stream(oracle, device):
    """The forward order on a handle bound to a side stream from its creation; the C
    buffers are filled on that stream too, so every launch is ordered behind its
    operands."""
    for name in STEPS:
        _fresh(name, device)  # the controls run on the default stream, before the sequence
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        h = _ops().Handle(stream=s)
        _sequence(STEPS + "adf", h, device, oracle)
        h.close()
    s.synchronize()
