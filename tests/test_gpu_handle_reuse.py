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
result is compared bit for bit with the fresh handle's. A handle whose stream changes
between calls is tests/test_gpu_stream_switch.py's subject; here one handle at a time,
every call eager: tests/test_gpu_graph_replay.py captures the same steps and replays
them.

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
  k  the fp64 CSR and BSR entries
  l  csrmm_f16 on the hub matrix (fp16 values and B), n = 128, row-major: the fp16
     merge-path kernel's split rows on the same tickets

Every step but j is cut in three so that its launches can also be captured:
  prepare_x(I, device, src=None)  the step's device buffers {"in", "C", "C0", ...}: its
      own copies of the inputs (never the cached I["d_*"], which later tests read), its
      C tensors and a pristine device copy of each C's initial contents (C0, or NaN where
      the step has beta = 0). src: host arrays that replace those of I, by I's keys
  launch_x(h, I, bufs)            library calls only: no allocation, no readback, no
      small_bsr_path()
  read_x(h, bufs)                 one synchronise and the readback
run_x(h, I, device, src=None) is their composition and returns a list of host arrays;
check_x(outs, I, oracle) holds them to the oracle. Steps f and i interleave host queries
(small_bsr_path(), the analyses) with their products, so run_f and run_i compose the
pieces of launch_f and launch_i one product at a time."""
from __future__ import annotations

import numpy as np
import pytest

from helpers import (HYBRID_EX_M, REUSE_HUB_K, REUSE_HUB_M, REUSE_SEG_SHAPE, TOL_F16_ACC, TOL_F32,
                     assert_normwise, column_sparse_bsr, hybrid_ex_matrix, hybrid_ex_parts,
                     long_row_column_sparse_bsr, oracle_bsrmm_d, oracle_bsrmm_f32, oracle_bsrmm_f64,
                     oracle_csrmm_d, oracle_csrmm_f64, oracle_csrmm_pieces_f32, rand_bsr,
                     reuse_hub_csr)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

COL = 1
STEPS = "abcdefghijkl"
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
def _host_inputs():
    """Host operands of every step, generated once; no device is touched."""
    if "host" in _state:
        return _state["host"]
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
    # l: the same matrix with its values rounded to fp16 (a generator of its own: the
    # draws of the other steps stay what they were)
    rp, ci, v = I["csr"]
    I["l_csr"] = rp, ci, v.astype(np.float16)
    I["l_B"] = np.random.default_rng(9002).uniform(-1, 1, (k, 128)).astype(np.float32).astype(np.float16)
    # d, e: one long block row on a shallow grid
    mb, kb, bs, n = REUSE_SEG_SHAPE
    # (a generator of its own: tests/test_hybrid_helpers.py rebuilds the matrix)
    I["seg"] = long_row_column_sparse_bsr(np.random.default_rng(9001), mb, kb, bs)
    I["seg_B"] = rng.uniform(-1, 1, (kb * bs, n)).astype(np.float32)
    I["seg_C0"] = rng.uniform(-1, 1, (mb * bs, n)).astype(np.float32)
    # f: the matrices of test_small_bs_grouped_stream_bit_exact
    for sb in (8, 2):
        G = 32 // sb
        fmb, fkb = 5 * G + 3, 160
        rp, ci, vb = _grouped_small_bsr(rng, sb, fmb, fkb)
        I[f"small{sb}"] = rp, ci, vb.reshape(-1)
        I[f"small{sb}_B"] = rng.uniform(-1, 1, (fkb * sb, 128)).astype(np.float32)
        I[f"small{sb}_C0"] = rng.uniform(-1, 1, (fmb * sb, 128)).astype(np.float32)
    # g: the hybrid's matrix at bs 32
    I["hyb_A"] = hybrid_ex_matrix()
    I["hyb"] = hybrid_ex_parts(32)
    I["hyb_B"] = rng.uniform(-1, 1, (HYBRID_EX_M, 64)).astype(np.float32)
    I["hyb_C0"] = rng.uniform(-1, 1, (704, 64)).astype(np.float32)
    # h: test_bsrmm_f16's shape
    rp, ci, v = rand_bsr(rng, 19, 25, 16, 0.27, empty_rows=(0,))
    I["h16"] = rp, ci, v.astype(np.float16)
    I["h16_B"] = rng.uniform(-1, 1, (25 * 16, 128)).astype(np.float16)
    # i: test_bsrmm_grouped_f16 / _f32's shape
    rp, ci, v = column_sparse_bsr(rng, 37, 60, 16, 0.3)
    I["g16"] = rp, ci, v.astype(np.float16)
    I["g16_B"] = rng.uniform(-1, 1, (60 * 16, 256)).astype(np.float16)
    I["g32"] = column_sparse_bsr(rng, 37, 60, 32, 0.3)
    I["g32_B"] = rng.uniform(-1, 1, (60 * 32, 128)).astype(np.float32)
    I["g_C0"] = rng.uniform(-1, 1, (37 * 32, 256)).astype(np.float32)
    # j: the hybrid's whole matrix through the converters
    I["conv"] = hybrid_ex_matrix()
    I["conv_bsr"] = prep.csr2bsr(HYBRID_EX_M, HYBRID_EX_M, *I["conv"], 4)
    I["conv_csr"] = prep.bsr2csr(175, 175, *I["conv_bsr"], 4)
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
    _state["host"] = I
    return I


def _inputs():
    """_host_inputs() plus, under "d_*", the device copies of the inputs: read-only
    masters that every prepare_x clones (C is allocated per run)."""
    if "inputs" in _state:
        return _state["inputs"]
    I = dict(_host_inputs())
    for key in ("csr", "l_csr", "seg", "small8", "small2", "hyb", "h16", "g16", "g32", "conv", "c64",
                "b64"):
        I["d_" + key] = _dev(*I[key])
    for key in ("b_B", "l_B", "seg_B", "small8_B", "small2_B", "g16_B", "g32_B", "c64_Bt", "b64_B"):
        I["d_" + key] = _dev(I[key])[0]
    I["d_a_Bt"], I["d_seg_Bt"], I["d_hyb_Bt"], I["d_h16_Bt"] = _dev(I["a_B"].T, I["seg_B"].T,
                                                                  I["hyb_B"].T, I["h16_B"].T)
    I["d_hyb_Bp"] = _dev(_pad_rows(I["hyb_B"], 704))[0]
    torch.cuda.synchronize()  # every input is ready before the first call on any stream
    _state["inputs"] = I
    return I


def _host(I, src, key, base=None):
    """Host array `key` (or, failing that, `base`): src's when it replaces it, else I's."""
    for d in (src or {}, I):
        for name in (key, base):
            if name is not None and name in d:
                return d[name]
    raise KeyError(key)


def _own(I, src, key, dkey=None, f=None):
    """The step's own device copy of input `key` (a tensor, or a list for a tuple of
    arrays): uploaded from src when src replaces it (through f, the host transform of the
    cached form), else cloned from the cached master I[dkey]."""
    if src and key in src:
        a = src[key]
        return _dev(*a) if isinstance(a, tuple) else _dev(f(a) if f else a)[0]
    d = I[dkey or "d_" + key]
    return [t.clone() for t in d] if isinstance(d, list) else d.clone()


def _bufs(ins, Cs, **more):
    Cs = list(Cs)
    return {"in": ins, "C": Cs, "C0": [c.clone() for c in Cs], **more}


def _read_C(h, bufs):
    return _read(h, *bufs["C"])


def _composed(name):
    def run(h, I, device, src=None):
        g = globals()
        bufs = g["prepare_" + name](I, device, src)
        g["launch_" + name](h, I, bufs)
        return g["read_" + name](h, bufs)
    run.__name__ = "run_" + name
    return run


# ------------------------------------------------------------------- steps
A_AB = (0.7, -1.3)


def prepare_a(I, device, src=None):
    rp, ci, v = _own(I, src, "csr")
    Bt = _own(I, src, "a_B", "d_a_Bt", np.transpose)
    return _bufs({"rp": rp, "ci": ci, "v": v, "Bt": Bt}, _dev(_host(I, src, "a_C0").T))


def launch_a(h, I, bufs):
    x = bufs["in"]
    _ops().csrmm(x["rp"], x["ci"], x["v"], x["Bt"], m=REUSE_HUB_M, n=256, k=REUSE_HUB_K,
                 ldb=REUSE_HUB_K, order_b=COL, C=bufs["C"][0], ldc=REUSE_HUB_M, order_c=COL,
                 alpha=A_AB[0], beta=A_AB[1], handle=h)


read_a, run_a = _read_C, _composed("a")


def check_a(outs, I, oracle):
    ref, absd = oracle_csrmm_f64(oracle, REUSE_HUB_M, 256, *I["csr"], I["a_B"], 256, 0)
    want, scale = _expect(ref, absd, I["a_C0"], *A_AB)
    assert_normwise(outs[0].T, want, scale, TOL_F32, "step a")


def prepare_b(I, device, src=None):
    rp, ci, v = _own(I, src, "csr")
    return _bufs({"rp": rp, "ci": ci, "v": v, "B": _own(I, src, "b_B")},
                 [_nan(REUSE_HUB_M * 64, device) for _ in range(3)])


def launch_b(h, I, bufs):
    x = bufs["in"]
    for w, C in zip((32, 1, 0), bufs["C"]):  # ends on the default
        h.set_csr_waves_per_cu(w)
        _ops().csrmm(x["rp"], x["ci"], x["v"], x["B"], m=REUSE_HUB_M, n=64, k=REUSE_HUB_K, ldb=64,
                     C=C, ldc=64, handle=h)


read_b, run_b = _read_C, _composed("b")


def check_b(outs, I, oracle):
    ref, absd = oracle_csrmm_f64(oracle, REUSE_HUB_M, 64, *I["csr"], I["b_B"], 64, 0)
    for w, got in zip((32, 1, 0), outs):
        assert_normwise(got.reshape(REUSE_HUB_M, 64), ref, absd, TOL_F32, f"step b waves_per_cu={w}")


def prepare_c(I, device, src=None):
    rp, ci, v = _own(I, src, "csr")
    return _bufs({"rp": rp, "ci": ci, "v": v, "B": _own(I, src, "b_B")},
                 [_nan(REUSE_HUB_M * 64, device)], tag=torch.empty_like(ci))


def analyse_c(h, I, bufs):
    _ops().csr_hot_analysis(bufs["in"]["ci"], n=64, k=REUSE_HUB_K, hot_bytes=400 * 256,
                            out=bufs["tag"], handle=h)


def launch_c_hot(h, I, bufs):
    x = bufs["in"]
    _ops().csrmm_hot(x["rp"], bufs["tag"], x["v"], x["B"], m=REUSE_HUB_M, n=64, k=REUSE_HUB_K,
                     ldb=64, C=bufs["C"][0], ldc=64, handle=h)


def launch_c(h, I, bufs):
    analyse_c(h, I, bufs)
    launch_c_hot(h, I, bufs)


def read_c(h, bufs):
    return _read(h, bufs["tag"], *bufs["C"])


run_c = _composed("c")


def check_c(outs, I, oracle):
    tag, got = outs
    ci = I["csr"][1]
    assert 0 < int((tag < 0).sum()) < ci.size, "step c: tags"
    assert np.array_equal(tag & 0x7FFFFFFF, ci), "step c: tagged indices"
    ref, absd = oracle_csrmm_f64(oracle, REUSE_HUB_M, 64, *I["csr"], I["b_B"], 64, 0)
    assert_normwise(got.reshape(REUSE_HUB_M, 64), ref, absd, TOL_F32, "step c")


def prepare_d(I, device, src=None):
    mb, kb, bs, n = REUSE_SEG_SHAPE
    rp, ci, v = _own(I, src, "seg")
    return _bufs({"rp": rp, "ci": ci, "v": v, "B": _own(I, src, "seg_B")},
                 [_nan(mb * bs * n, device)])


def launch_d(h, I, bufs):
    mb, kb, bs, n = REUSE_SEG_SHAPE
    x = bufs["in"]
    _ops().bsrmm(x["rp"], x["ci"], x["v"], x["B"], mb=mb, kb=kb, n=n, bs=bs, ldb=n, C=bufs["C"][0],
                 ldc=n, handle=h)


read_d, run_d = _read_C, _composed("d")


def _seg_oracle(I, oracle):
    mb, kb, bs, n = REUSE_SEG_SHAPE
    return oracle_bsrmm_f64(oracle, 0, mb, n, bs, *I["seg"], I["seg_B"], n, 0)


def check_d(outs, I, oracle):
    mb, kb, bs, n = REUSE_SEG_SHAPE
    ref, absd = _seg_oracle(I, oracle)
    assert_normwise(outs[0].reshape(mb * bs, n), ref, absd, TOL_F32, "step d")


E_AB = (0.5, -1.5)


def prepare_e(I, device, src=None):
    rp, ci, v = _own(I, src, "seg")
    Bt = _own(I, src, "seg_B", "d_seg_Bt", np.transpose)
    return _bufs({"rp": rp, "ci": ci, "v": v, "Bt": Bt}, _dev(_host(I, src, "seg_C0").T))


def launch_e(h, I, bufs):
    mb, kb, bs, n = REUSE_SEG_SHAPE
    x = bufs["in"]
    _ops().bsrmm(x["rp"], x["ci"], x["v"], x["Bt"], mb=mb, kb=kb, n=n, bs=bs, ldb=kb * bs,
                 order_b=COL, C=bufs["C"][0], ldc=mb * bs, order_c=COL, alpha=E_AB[0], beta=E_AB[1],
                 handle=h)


read_e, run_e = _read_C, _composed("e")


def check_e(outs, I, oracle):
    want, scale = _expect(*_seg_oracle(I, oracle), I["seg_C0"], *E_AB)
    assert_normwise(outs[0].T, want, scale, TOL_F32, "step e")


F_AB = (0.5, -2.0)


def prepare_f(I, device, src=None):
    ins, Cs = {}, []
    for sb in (8, 2):
        ins[f"rp{sb}"], ins[f"ci{sb}"], ins[f"v{sb}"] = _own(I, src, f"small{sb}")
        ins[f"B{sb}"] = _own(I, src, f"small{sb}_B")
        Cs += _dev(_host(I, src, f"small{sb}_C0"))
    return _bufs(ins, Cs)


def _launch_f_one(h, I, bufs, j):
    """Product j (0: bs 8, 1: bs 2) of step f; the caller has set SPMM_BSR_SMALL_GROUPED."""
    sb = (8, 2)[j]
    x = bufs["in"]
    mb = I[f"small{sb}"][0].size - 1
    _ops().bsrmm(x[f"rp{sb}"], x[f"ci{sb}"], x[f"v{sb}"], x[f"B{sb}"], mb=mb, kb=160, n=128, bs=sb,
                 ldb=128, C=bufs["C"][j], ldc=128, alpha=F_AB[0], beta=F_AB[1], handle=h)


def launch_f(h, I, bufs):
    from spmm_hip._lib import BSR_SMALL_GROUPED
    h.set_bsr_options(BSR_SMALL_GROUPED)
    try:
        for j in range(2):
            _launch_f_one(h, I, bufs, j)
    finally:
        h.set_bsr_options(0)


read_f = _read_C


def run_f(h, I, device, src=None):
    """launch_f one product at a time, each followed at once by small_bsr_path()."""
    from spmm_hip._lib import BSR_SMALL_GROUPED
    bufs = prepare_f(I, device, src)
    outs = []
    h.set_bsr_options(BSR_SMALL_GROUPED)
    try:
        for j in range(2):
            _launch_f_one(h, I, bufs, j)
            path = h.small_bsr_path()  # right after the product (include/spmm_hip.h)
            outs += _read(h, bufs["C"][j]) + [np.array([path], np.int32)]
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


def prepare_g(I, device, src=None):
    """C0 of the column-major / the row-major call: "hyb_C0c" / "hyb_C0r" where given
    (704 x 64 both), else "hyb_C0" for both."""
    ins = dict(zip(("crp", "cci", "cv", "brp", "bci", "bv"), _own(I, src, "hyb")))
    ins["Bt"] = _own(I, src, "hyb_B", "d_hyb_Bt", np.transpose)
    ins["Bp"] = _own(I, src, "hyb_B", "d_hyb_Bp", lambda a: _pad_rows(a, 704))
    return _bufs(ins, _dev(_host(I, src, "hyb_C0c", "hyb_C0").T, _host(I, src, "hyb_C0r", "hyb_C0")))


def launch_g(h, I, bufs):
    ops = _ops()
    x = bufs["in"]
    m = HYBRID_EX_M
    csr, bsr = (x["crp"], x["cci"], x["cv"]), (x["brp"], x["bci"], x["bv"])
    ops.hybrid_csrmm(csr, bsr, x["Bt"], m=m, n=64, k=m, bs=32, ldb=m, C=bufs["C"][0], ldc=704,
                     alpha=G_AB[0], beta=G_AB[1], order_b=COL, order_c=COL, handle=h)
    ops.hybrid_csrmm(csr, bsr, x["Bp"], m=m, n=64, k=m, bs=32, ldb=64, C=bufs["C"][1], ldc=64,
                     alpha=G_AB[0], beta=G_AB[1], handle=h)


read_g, run_g = _read_C, _composed("g")


def check_g(outs, I, oracle):
    ref, absd = oracle_csrmm_f64(oracle, HYBRID_EX_M, 64, *I["hyb_A"], I["hyb_B"], 64, 0)
    ref, absd = _pad_rows(ref, 704), _pad_rows(absd, 704)
    want, scale = _expect(ref, absd, _host(I, None, "hyb_C0c", "hyb_C0"), *G_AB)
    assert_normwise(outs[0].T, want, scale, TOL_F32, "step g column-major")
    want, scale = _expect(ref, absd, _host(I, None, "hyb_C0r", "hyb_C0"), *G_AB)
    assert_normwise(outs[1], want, scale, TOL_F32, "step g row-major")


def prepare_h(I, device, src=None):
    rp, ci, v = _own(I, src, "h16")
    Bt = _own(I, src, "h16_B", "d_h16_Bt", np.transpose)
    return _bufs({"rp": rp, "ci": ci, "v": v, "Bt": Bt}, [_nan(19 * 16 * 128, device)])


def launch_h(h, I, bufs):
    x = bufs["in"]
    _ops().bsrmm_f16(x["rp"], x["ci"], x["v"], x["Bt"], mb=19, kb=25, n=128, bs=16, ldb=25 * 16,
                     order_b=COL, C=bufs["C"][0], ldc=128, handle=h)


read_h, run_h = _read_C, _composed("h")


def check_h(outs, I, oracle):
    ref, absd = oracle_bsrmm_f64(oracle, 0, 19, 128, 16, *I["h16"], I["h16_B"], 128, 0, half=True)
    assert_normwise(outs[0].reshape(19 * 16, 128), ref, absd, TOL_F16_ACC, "step h")


I_AB = (0.5, -1.0)
I_FAMILIES = (("GroupedBsr16", "g16", 16, 256, 4), ("GroupedBsr32", "g32", 32, 128, 2))


def prepare_i(I, device, src=None):
    """C0 of family j: "g16_C0" / "g32_C0" where given (37 * bs x n), else g_C0's corner."""
    ins, Cs = {}, []
    for _, key, bs, n, _ in I_FAMILIES:
        ins[f"rp{bs}"], ins[f"ci{bs}"], ins[f"v{bs}"] = _own(I, src, key)
        ins[f"B{bs}"] = _own(I, src, f"{key}_B")
        Cs += _dev(_host(I, src, f"{key}_C0", "g_C0")[:37 * bs, :n])
    return _bufs(ins, Cs, grp=[None, None])


def analyse_i(h, I, bufs, j):
    """The group analysis of family j on h (size query + fill: host round trips)."""
    cls, _, bs, _, W = I_FAMILIES[j]
    x = bufs["in"]
    bufs["grp"][j] = getattr(_ops(), cls)(x[f"rp{bs}"], x[f"ci{bs}"], x[f"v{bs}"], mb=37,
                                          group_rows=W, handle=h)
    return bufs["grp"][j]


def _launch_i_one(h, I, bufs, j):
    _, _, bs, n, _ = I_FAMILIES[j]
    bufs["grp"][j].mm(bufs["in"][f"B{bs}"], kb=60, n=n, ldb=n, C=bufs["C"][j], ldc=n, alpha=I_AB[0],
                      beta=I_AB[1])


def launch_i(h, I, bufs):
    """Both grouped products, on analyses made on h beforehand (analyse_i)."""
    for j in range(2):
        _launch_i_one(h, I, bufs, j)


read_i = _read_C


def release_i(bufs):
    for grp in bufs["grp"]:
        if grp is not None:
            grp.close()
    bufs["grp"] = [None, None]


def run_i(h, I, device, src=None):
    """Per family: the analysis, its product, the readback, the release."""
    bufs = prepare_i(I, device, src)
    outs = []
    for j in range(2):
        with analyse_i(h, I, bufs, j) as grp:
            _launch_i_one(h, I, bufs, j)
            outs += _read(h, bufs["C"][j]) + [np.array([grp.W, grp.nitems, grp.bytes], np.int64)]
    return outs


def check_i(outs, I, oracle):
    for (key, bs, n, tol), got in zip((("g16", 16, 256, TOL_F16_ACC), ("g32", 32, 128, TOL_F32)),
                                      (outs[0], outs[2])):
        ref, absd = oracle_bsrmm_f64(oracle, 0, 37, n, bs, *I[key], I[f"{key}_B"], n, 0, half=bs == 16)
        want, scale = _expect(ref, absd, _host(I, None, f"{key}_C0", "g_C0")[:37 * bs, :n], *I_AB)
        assert_normwise(got, want, scale, tol, f"step i bs {bs}")


def run_j(h, I, device, src=None):
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


def prepare_k(I, device, src=None):
    ins = dict(zip(("crp", "cci", "cv"), _own(I, src, "c64")))
    ins.update(zip(("brp", "bci", "bv"), _own(I, src, "b64")))
    ins["cBt"], ins["bB"] = _own(I, src, "c64_Bt"), _own(I, src, "b64_B")
    return _bufs(ins, _dev(_host(I, src, "c64_C0t"), _host(I, src, "b64_C0")))


def launch_k(h, I, bufs):
    ops = _ops()
    x = bufs["in"]
    ops.csrmm(x["crp"], x["cci"], x["cv"], x["cBt"], m=517, n=70, k=389, ldb=389, order_b=COL,
              C=bufs["C"][0], ldc=517, order_c=COL, alpha=K_AB[0], beta=K_AB[1], handle=h)
    ops.bsrmm(x["brp"], x["bci"], x["bv"], x["bB"], mb=23, kb=19, n=70, bs=8, ldb=70, C=bufs["C"][1],
              ldc=70, alpha=K_AB[0], beta=K_AB[1], handle=h)


read_k, run_k = _read_C, _composed("k")


def check_k(outs, I, oracle):
    want = oracle_csrmm_d(oracle, 517, 70, *I["c64"], I["c64_Bt"], 389, 1, K_AB[0], K_AB[1],
                          I["c64_C0t"].ravel(), 517, 1)
    assert np.array_equal(outs[0].ravel(), want), "step k csr"
    want = oracle_bsrmm_d(oracle, 0, 23, 70, 8, *I["b64"], I["b64_B"], 70, 0, K_AB[0], K_AB[1],
                          I["b64_C0"].ravel(), 70, 0)
    assert np.array_equal(outs[1].ravel(), want), "step k bsr"


def prepare_l(I, device, src=None):
    rp, ci, v = _own(I, src, "l_csr")
    return _bufs({"rp": rp, "ci": ci, "v": v, "B": _own(I, src, "l_B")},
                 [_nan(REUSE_HUB_M * 128, device)])


def launch_l(h, I, bufs):
    x = bufs["in"]
    _ops().csrmm_f16(x["rp"], x["ci"], x["v"], x["B"], m=REUSE_HUB_M, n=128, k=REUSE_HUB_K, ldb=128,
                     C=bufs["C"][0], ldc=128, handle=h)


read_l, run_l = _read_C, _composed("l")


def check_l(outs, I, oracle):
    """The bar of tests/test_gpu_csr_f16.py: the bits of the fp32 entry on the widened
    inputs (on a handle of its own; n = 128 is past its lane-group kernel) and of the
    piece oracle, and TOL_F16_ACC against the float64 product of the fp16 values."""
    ops = _ops()
    m, k = REUSE_HUB_M, REUSE_HUB_K
    rp, ci, v16 = I["l_csr"]
    v32, B32 = v16.astype(np.float32), I["l_B"].astype(np.float32)
    got = outs[0].reshape(m, 128)
    h = ops.Handle()
    drp, dci, dv, dB = _dev(rp, ci, v32, B32)
    C = _nan(m * 128, dv.device)
    ops.csrmm(drp, dci, dv, dB, m=m, n=128, k=k, ldb=128, C=C, ldc=128, handle=h)
    wide = _read(h, C)[0].reshape(m, 128)
    h.close()
    bad = got.view(np.uint32) != wide.view(np.uint32)
    assert not bad.any(), f"step l: {int(bad.sum())} elements differ from csrmm on the widened inputs"
    pieces = oracle_csrmm_pieces_f32(oracle, m, 128, rp, ci, v32, B32, 128, 0).reshape(m, 128)
    bad = got.view(np.uint32) != pieces.view(np.uint32)
    assert not bad.any(), f"step l: {int(bad.sum())} elements differ from the piece oracle"
    ref, absd = oracle_csrmm_f64(oracle, m, 128, rp, ci, v32, B32, 128, 0)
    assert_normwise(got, ref, absd, TOL_F16_ACC, "step l")


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
