"""CSR x dense with fp16 A values and B, fp32 accumulate and C (spmm_csrmm_ex_f16,
spmm_gespmm_csrmm_f16).

binary16 -> binary32 is exact, so the acceptance bar is equality of bits: the
fp16-input product is the fp32 entry's product of the widened inputs and the piece
oracle's (oracle_csrmm_pieces_f32) at every n, the fp16 entry always
running the merge-path kernel. Inputs are drawn as fp32 uniform(-1, 1), rounded with
.astype(np.float16) and widened back with .astype(np.float32) for the oracle and the
fp32 entry; comparisons are on uint32 views (signed zeros included). No tolerance
is involved anywhere in this file."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from helpers import framed, oracle_csrmm_f32, oracle_csrmm_pieces_f32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _ops():
    from spmm_hip import ops
    return ops


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _halves(x32):
    """(the fp16 rounding of x32, the same values widened back to fp32)."""
    h = np.asarray(x32, np.float32).astype(np.float16)
    return h, h.astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_bits(got, want, what):
    """got and want (2-D fp32) hold the same bits."""
    bad = _bits(got) != _bits(want)
    if bad.any():
        rows = np.flatnonzero(bad.any(axis=1))
        r, c = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} elements in {rows.size} rows differ, first "
                             f"rows {rows[:5].tolist()}; [{r}, {c}] got {got[r, c]!r} want "
                             f"{want[r, c]!r}")


def _c_init(C0, beta):
    """C before the call: NaN at beta = 0 (never read), the finite C0 otherwise."""
    return C0 if beta != 0.0 else np.full_like(C0, np.nan)


def _rand_csr(rng, m, k, deg_hi, hub_rows=(), hub_deg=0, empty_frac=0.0):
    deg = rng.integers(0, deg_hi + 1, m)
    if empty_frac:
        deg[rng.random(m) < empty_frac] = 0
    for r in hub_rows:
        deg[r] = min(hub_deg, k)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    ci = np.concatenate([np.sort(rng.choice(k, d, replace=False)) for d in deg] or
                        [np.zeros(0)]).astype(np.int32)
    return rp, ci, rng.uniform(-1, 1, ci.size).astype(np.float32)


# ------------------------------------------- 1. split rows, every width, every grid
SPLIT_M, SPLIT_NNZ = 40000, 600000
SPLIT_K = [128, 256, 512, 130, 64, 36, 7, 1]  # VEC 2, 4 (one and two tiles), 2 ragged, VEC 1
SPLIT_AB = [(1.0, 0.0), (2.0, 0.5), (0.7, -1.3)]
_split: dict = {}


def _split_matrix():
    """The matrix of test_split_rows_bit_exact_pieces (tests/test_gpu_csr.py) with fp16
    values: host (rp, ci, v16, v32) and device (rp, ci, v16)."""
    if "A" not in _split:
        from spmm_hip import prep
        rp, ci = prep.powerlaw_csr(SPLIT_M, SPLIT_NNZ, 15000, 2.1, 11)
        v16, v32 = _halves(np.random.default_rng(3).uniform(-1, 1, ci.size))
        _split["A"] = (rp, ci, v16, v32), _dev(rp, ci, v16)
    return _split["A"]


def _split_case(K):
    """B (fp16 and widened) and C0 at width K, kept for the K in hand only."""
    if _split.get("K") != K:
        B16, B32 = _halves(np.random.default_rng(4).uniform(-1, 1, (SPLIT_M, K)))
        C0 = np.random.default_rng(5).uniform(-1, 1, (SPLIT_M, K)).astype(np.float32)
        _split["K"], _split["case"] = K, (B16, B32, C0)
    return _split["case"]


@pytest.mark.parametrize("alpha,beta", SPLIT_AB)
@pytest.mark.parametrize("K", SPLIT_K)
def test_split_rows_bit_exact_pieces_f16(oracle, device, K, alpha, beta):
    """Power-law rows with hubs spanning dozens of waves: every row, split or not,
    has the piece oracle's bits on the widened inputs, at every vector width (at
    K <= 64 too: the fp16 entry has no lane-group form), on relaunch (tickets back at
    zero) and at every grid."""
    ops = _ops()
    (rp, ci, _, v32), (drp, dci, dv) = _split_matrix()
    m = SPLIT_M
    B16, B32, C0 = _split_case(K)
    dB, = _dev(B16)
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    nwaves = min(-(-(m + ci.size) // 256), cus * 16)  # kMinItemsPerWave, csr_kernels.hip
    per = -(-(m + ci.size) // nwaves)
    r = np.arange(m)
    split = (r + rp[:-1]) // per != (r + rp[1:]) // per
    assert split.sum() > 50, "the case must split many rows"
    want = oracle_csrmm_pieces_f32(oracle, m, K, rp, ci, v32, B32, K, 0, alpha=alpha, beta=beta,
                                   C=C0).reshape(m, K)
    h = ops.Handle()
    for wpc in (0, 16, 16, 1, 5, 32):  # 0: the default grid first
        if wpc:
            h.set_csr_waves_per_cu(wpc)
        C, = _dev(_c_init(C0, beta))
        ops.csrmm_f16(drp, dci, dv, dB, n=K, k=m, ldb=K, C=C, ldc=K, alpha=alpha, beta=beta,
                      handle=h)
        torch.cuda.synchronize()
        got = C.cpu().numpy()
        bad = _bits(got) != _bits(want)
        assert not bad.any(), (f"K={K} waves/CU={wpc or 'default'}: {int(bad.any(axis=1).sum())} "
                               f"rows differ from the piece oracle "
                               f"({int(bad[split].any(axis=1).sum())} of {int(split.sum())} split)")
    h.close()


# --------------------------------- 2. fp16 entry = fp32 entry on the widened inputs
@pytest.mark.parametrize("m,nnz,K", [(20000, 400000, 128), (20000, 400000, 32),
                                     (6000, 900000, 256)])
def test_f16_entry_equals_f32_entry_on_widened_inputs(device, m, nnz, K):
    """The shapes of test_dropin_equals_ex_entry: spmm_csrmm_ex_f16 equals
    spmm_csrmm_ex_f32 on the widened inputs (under SPMM_CSR_SEQUENTIAL_ROWS at
    n <= 64, where the fp32 entry would otherwise take its lane-group kernel), the
    drop-in equals the handle entry, and two / three contiguous row shards written in
    place equal the whole product."""
    from spmm_hip import prep
    from spmm_hip._lib import CSR_NT_STREAMS, CSR_SEQUENTIAL_ROWS
    ops = _ops()
    rp, ci = prep.powerlaw_csr(m, nnz, m // 2, 2.1, 5)
    v16, v32 = _halves(np.random.default_rng(6).uniform(-1, 1, ci.size))
    B16, B32 = _halves(np.random.default_rng(7).uniform(-1, 1, (m, K)))
    drp, dci, dv16, dv32, dB16, dB32 = _dev(rp, ci, v16, v32, B16, B32)
    h32 = ops.Handle()
    if K <= 64:
        h32.set_csr_options(CSR_NT_STREAMS | CSR_SEQUENTIAL_ROWS)
    C32 = torch.full((m, K), float("nan"), device=device)
    ops.csrmm(drp, dci, dv32, dB32, n=K, k=m, ldb=K, C=C32, ldc=K, handle=h32)
    C16 = torch.full((m, K), float("nan"), device=device)
    ops.csrmm_f16(drp, dci, dv16, dB16, n=K, k=m, ldb=K, C=C16, ldc=K)
    Cd = ops.gespmm_csrmm_f16(drp, dci, dv16, dB16)
    torch.cuda.synchronize()
    assert Cd.dtype == torch.float32 and Cd.shape == (m, K)
    assert torch.equal(C16.view(torch.int32), C32.view(torch.int32)), "fp16 entry != fp32 entry"
    assert torch.equal(Cd.view(torch.int32), C16.view(torch.int32)), "drop-in != handle entry"
    for world in (2, 3):
        Cs = torch.full((m, K), float("nan"), device=device)
        bounds = [m * r // world for r in range(world + 1)]
        for r0, r1 in zip(bounds[:-1], bounds[1:]):
            ops.csrmm_f16(drp[r0:r1 + 1], dci, dv16, dB16, m=r1 - r0, n=K, k=m, ldb=K,
                          C=Cs[r0:r1], ldc=K)
        torch.cuda.synchronize()
        assert torch.equal(Cs.view(torch.int32), C16.view(torch.int32)), f"{world} row shards"
    h32.close()


def test_f32_wrappers_keep_rejecting_halves(device):
    ops = _ops()
    rp = torch.tensor([0, 1], dtype=torch.int32, device=device)
    ci = torch.zeros(1, dtype=torch.int32, device=device)
    v = torch.ones(1, dtype=torch.float16, device=device)
    B = torch.ones((1, 4), dtype=torch.float16, device=device)
    C = torch.zeros((1, 4), dtype=torch.float32, device=device)
    with pytest.raises(TypeError):
        ops.csrmm(rp, ci, v, B, n=4, k=1, ldb=4, C=C, ldc=4)
    with pytest.raises(TypeError):
        ops.gespmm_csrmm(rp, ci, v, B)
    with pytest.raises(TypeError):  # and the fp16 wrapper takes nothing but halves
        ops.csrmm_f16(rp, ci, v.float(), B, n=4, k=1, ldb=4, C=C, ldc=4)
    ops.csrmm_f16(rp, ci, v, B, n=4, k=1, ldb=4, C=C, ldc=4)
    torch.cuda.synchronize()
    assert C.cpu().tolist() == [[1.0] * 4]


# ------------------------------------------------ 3. values at the edges of binary16
EDGE = np.array([0.0, -0.0, 2.0 ** -24, 2.0 ** -20, 2.0 ** -14, 1.0, 65504.0], np.float32)


def _edge_case(n, special):
    """m = k = 64, rows of 0 .. 64 distinct columns (at most 128 nonzeros: one piece, the
    reference's sequential chain); A values and B drawn from EDGE, which every binary16
    holds exactly (2^-24 and 2^-20 as subnormals)."""
    rng = np.random.default_rng(160 + n + (1000 if special else 0))
    m = k = 64
    deg = rng.integers(0, k + 1, m)
    deg[:3] = (0, 1, k)  # row 1: the one product 1 * B[5], a subnormal half (inf when special)
    rp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    ci = np.concatenate([np.sort(rng.choice(k, d, replace=False)) for d in deg]).astype(np.int32)
    v = rng.choice(EDGE, ci.size)
    B = rng.choice(EDGE, (k, n))
    ci[rp[1]], v[rp[1]] = 5, 1.0
    B[5, :] = 2.0 ** -24
    if special:
        B[5, :] = np.inf
        B[11, ::2] = -np.inf
        B[17, :] = np.nan
        B[23, n // 2] = np.nan
        v[rp[2] + 40] = np.inf  # row 2 is full: times B[40], which holds zeros (NaN) too
    v16, v32 = _halves(v)
    B16, B32 = _halves(B)
    assert np.array_equal(_bits(v32), _bits(v)) and np.array_equal(_bits(B32), _bits(B))
    return m, k, rp, ci, v16, v32, B16, B32


@pytest.mark.parametrize("special", [False, True], ids=["finite", "inf-nan"])
@pytest.mark.parametrize("n", [1, 4, 130])
def test_binary16_edge_values(oracle, device, n, special):
    """Signed zeros, fp16 subnormals (2^-24, 2^-20), the smallest normal, 1 and the
    largest finite half: an fp16 flush-to-zero anywhere on the way (the val widen, the B
    widen, a folded fma_mix) is a wrong bit here. With +-inf and NaN in B rows and one
    inf in A the NaN positions are the oracle's and every other element its bits (NaN
    payloads are not compared)."""
    ops = _ops()
    m, k, rp, ci, v16, v32, B16, B32 = _edge_case(n, special)
    want = oracle_csrmm_pieces_f32(oracle, m, n, rp, ci, v32, B32, n, 0).reshape(m, n)
    seq = oracle_csrmm_f32(oracle, m, n, rp, ci, v32, B32, n, 0).reshape(m, n)
    nan = np.isnan(want)
    assert np.array_equal(nan, np.isnan(seq))
    assert np.array_equal(_bits(want)[~nan], _bits(seq)[~nan]), "one piece = the sequential chain"
    if special:
        assert nan.any() and np.isinf(want).any() and not nan.all()
    else:
        assert not nan.any() and (want != 0).any()
        # the subnormal halves matter: flushing them changes the expected bits
        flush = lambda a: np.where(np.abs(a) < 2.0 ** -14, np.copysign(0, a), a).astype(np.float32)  # noqa: E731
        ftz = oracle_csrmm_pieces_f32(oracle, m, n, rp, ci, flush(v32), flush(B32), n, 0)
        assert not np.array_equal(_bits(ftz.reshape(m, n)), _bits(want))
    drp, dci, dv, dB = _dev(rp, ci, v16, B16)
    C = torch.full((m, n), float("nan"), device=device)
    ops.csrmm_f16(drp, dci, dv, dB, n=n, k=k, ldb=n, C=C, ldc=n)
    torch.cuda.synchronize()
    got = C.cpu().numpy()
    assert np.array_equal(np.isnan(got), nan), "NaN positions differ from the oracle's"
    bad = (_bits(got) != _bits(want)) & ~nan
    assert not bad.any(), (f"n={n}: {int(bad.sum())} elements differ, first "
                           f"{np.argwhere(bad)[0].tolist()}: got "
                           f"{got[tuple(np.argwhere(bad)[0])]!r} want "
                           f"{want[tuple(np.argwhere(bad)[0])]!r}")


# ------------------------------------------------------------------- 4. layouts
LAY_M, LAY_K, LAY_HUB = 300, 200, 5000
_lay: dict = {}


def _lay_matrix():
    """300 x 200, rows of 0 .. 6 nonzeros (some empty) and one hub row of 5000 (columns
    repeat: 40 pieces over the waves of the default grid)."""
    if "A" not in _lay:
        rng = np.random.default_rng(31)
        deg = rng.integers(0, 7, LAY_M)
        deg[rng.random(LAY_M) < 0.2] = 0
        rows = [np.sort(rng.choice(LAY_K, d, replace=False)) for d in deg]
        rows[123] = np.sort(rng.integers(0, LAY_K, LAY_HUB))
        rp = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
        ci = np.concatenate(rows).astype(np.int32)
        v16, v32 = _halves(rng.uniform(-1, 1, ci.size))
        _lay["A"] = rp, ci, v16, v32
    return _lay["A"]


def _lay_case(oracle, n, alpha, beta):
    key = (n, alpha, beta)
    if key not in _lay:
        rp, ci, _, v32 = _lay_matrix()
        rng = np.random.default_rng(3100 + n)
        B16, B32 = _halves(rng.uniform(-1, 1, (LAY_K, n)))
        C0 = rng.uniform(-1, 1, (LAY_M, n)).astype(np.float32)
        want = oracle_csrmm_pieces_f32(oracle, LAY_M, n, rp, ci, v32, B32, n, 0, alpha=alpha,
                                       beta=beta, C=C0).reshape(LAY_M, n)
        _lay[key] = B16, C0, want
    return _lay[key]


@pytest.mark.parametrize("n", [66, 128, 260])
def test_rowmajor_layouts_f16(oracle, device, n):
    """Row-major B at half offsets 0 / 1 / 2 / 4 with ldb = n + 0 / 1 / 2 / 8 and C at
    float offsets 0 / 1 / 4 with ldc = n + 0 / 1 / 4 (every vector width the layout
    leaves: a B at an odd half offset or with an odd ldb is gathered one half per
    lane): the piece oracle's bits, the sentinels around C and in its padding bit for
    bit, B unchanged."""
    ops = _ops()
    rp, ci, v16, _ = _lay_matrix()
    drp, dci, dv = _dev(rp, ci, v16)
    h = ops.Handle()
    lays = [(ob, pb, oc, pc) for ob in (0, 1, 2, 4) for pb in (0, 1, 2, 8) for oc in (0, 1, 4)
            for pc in (0, 1, 4)]
    for alpha, beta in ((1.0, 0.0), (0.7, -1.3)):
        B16, C0, want = _lay_case(oracle, n, alpha, beta)
        for off_b, pad_b, off_c, pad_c in lays:
            dB, chkB = framed(B16, n + pad_b, off_b)
            dC, chkC = framed(_c_init(C0, beta), n + pad_c, off_c)
            what = (f"n={n} B off {off_b} ldb n+{pad_b}, C off {off_c} ldc n+{pad_c}, "
                    f"alpha={alpha} beta={beta}")
            ops.csrmm_f16(drp, dci, dv, dB, m=LAY_M, n=n, k=LAY_K, ldb=n + pad_b, C=dC,
                          ldc=n + pad_c, alpha=alpha, beta=beta, handle=h)
            _assert_bits(chkC(what + ": C"), want, what)
            chkB.unchanged(what + ": B")
    h.close()


@pytest.mark.parametrize("beta", [0.0, 0.75])
@pytest.mark.parametrize("n", [1, 36, 128])
def test_colmajor_forms_f16(oracle, device, n, beta):
    """Column-major B (staged in halves through the 16-bit transpose) and / or C (the
    fp32 transposed epilogue), one-based indices, padded leading dimensions at an
    offset: the bits of the row-major product (the piece oracle's)."""
    ops = _ops()
    rp, ci, v16, _ = _lay_matrix()
    drp, dci, dv = _dev(rp + 1, ci + 1, v16)
    alpha = 1.0 if beta == 0.0 else -0.5
    B16, C0, want = _lay_case(oracle, n, alpha, beta)
    h = ops.Handle()
    for ob, oc in ((0, 0), (1, 0), (0, 1), (1, 1)):
        B2 = B16 if ob == 0 else np.ascontiguousarray(B16.T)
        Ci = _c_init(C0, beta)
        C2 = Ci if oc == 0 else np.ascontiguousarray(Ci.T)
        for off_b, pad_b, off_c, pad_c in ((0, 0, 0, 0), (1, 3, 1, 1), (8, 8, 4, 4)):
            ldb, ldc = B2.shape[1] + pad_b, C2.shape[1] + pad_c
            dB, chkB = framed(B2, ldb, off_b)
            dC, chkC = framed(C2, ldc, off_c)
            what = f"n={n} order_b={ob} order_c={oc} layout={(off_b, pad_b, off_c, pad_c)} beta={beta}"
            ops.csrmm_f16(drp, dci, dv, dB, m=LAY_M, n=n, k=LAY_K, ldb=ldb, order_b=ob, C=dC,
                          ldc=ldc, order_c=oc, alpha=alpha, beta=beta, base=1, handle=h)
            got = chkC(what + ": C")
            _assert_bits(got if oc == 0 else np.ascontiguousarray(got.T), want, what)
            chkB.unchanged(what + ": B")
    h.close()


# ------------------------------------------------------------- 5. random shapes
@pytest.mark.parametrize("seed", range(8))
def test_random_shapes_grid_independent_f16(oracle, device, seed):
    """Random matrices (rows of 0 .. 3,000 nonzeros, hubs up to 9,000, empty rows), a
    random K among every width, random alpha / beta and two random grids: the piece
    oracle's bits at both."""
    ops = _ops()
    rng = np.random.default_rng(9100 + seed)
    m = int(rng.integers(1, 30000))
    k = int(rng.integers(1, 20000))
    K = int(rng.choice([1, 2, 6, 8, 36, 64, 66, 96, 128, 130, 192, 256, 260, 512]))
    nhub = int(rng.integers(0, 6))
    hubs = rng.choice(m, min(nhub, m), replace=False) if nhub else ()
    rp, ci, v = _rand_csr(rng, m, k, min(int(rng.choice([0, 3, 20, 200, 3000])), k), hubs,
                          int(rng.integers(1000, 9001)), float(rng.choice([0.0, 0.3])))
    alpha = float(rng.choice([1.0, -0.5, 2.0]))
    beta = float(rng.choice([0.0, 0.0, 0.75]))
    v16, v32 = _halves(v)
    B16, B32 = _halves(rng.uniform(-1, 1, (k, K)))
    C0 = rng.uniform(-1, 1, (m, K)).astype(np.float32)
    drp, dci, dv, dB = _dev(rp, ci, v16, B16)
    what = f"m={m} k={k} K={K} nnz={ci.size} alpha={alpha} beta={beta}"
    want = oracle_csrmm_pieces_f32(oracle, m, K, rp, ci, v32, B32, K, 0, alpha=alpha, beta=beta,
                                   C=C0).reshape(m, K)
    got = []
    for wpc in rng.choice(np.arange(1, 33), 2, replace=False):
        h = ops.Handle()
        h.set_csr_waves_per_cu(int(wpc))
        C, = _dev(_c_init(C0, beta))
        ops.csrmm_f16(drp, dci, dv, dB, n=K, k=k, ldb=K, C=C, ldc=K, alpha=alpha, beta=beta,
                      handle=h)
        torch.cuda.synchronize()
        got.append(C.cpu().numpy())
        h.close()
        _assert_bits(got[-1], want, f"{what} waves/CU={int(wpc)}")
    assert np.array_equal(_bits(got[0]), _bits(got[1])), what + ": grids differ"


# ------------------------------------------- 6. status codes and degenerate shapes
def test_status_codes_f16(device):
    from spmm_hip._lib import INVALID_VALUE, NOT_INITIALIZED, SUCCESS, lib
    L = lib()
    ops = _ops()
    f = L.spmm_csrmm_ex_f16
    assert f(None, 1, 1, 1, 0, 1.0, None, None, None, 0, None, 1, 0, 0.0, None, 1, 0) \
        == NOT_INITIALIZED
    h = ops.default_handle()
    rp = torch.tensor([0, 1, 2], dtype=torch.int32, device=device)
    ci = torch.tensor([0, 1], dtype=torch.int32, device=device)
    v = torch.ones(2, dtype=torch.float16, device=device)
    B = torch.ones(2 * 4, dtype=torch.float16, device=device)
    C = torch.full((2 * 4,), 7.0, dtype=torch.float32, device=device)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(m=2, n=4, k=2, nnz=2, rp_=P(rp), ci_=P(ci), v_=P(v), base=0, B_=P(B), ldb=4, ob=0,
             C_=P(C), ldc=4, oc=0):
        return f(h.raw, m, n, k, nnz, 1.0, rp_, ci_, v_, base, B_, ldb, ob, 0.0, C_, ldc, oc)
    for bad in (dict(m=-1), dict(n=-1), dict(k=-1), dict(nnz=-1), dict(base=2), dict(base=-1),
                dict(ob=2), dict(oc=-1), dict(rp_=None), dict(C_=None), dict(B_=None),
                dict(ci_=None), dict(v_=None), dict(ldb=3), dict(ldc=3), dict(ob=1, ldb=1),
                dict(oc=1, ldc=1)):
        assert call(**bad) == INVALID_VALUE, bad
    # the checks' order: a null handle before bad sizes, bad sizes before the quick return
    assert f(None, -1, 1, 1, 0, 1.0, None, None, None, 0, None, 1, 0, 0.0, None, 1, 0) \
        == NOT_INITIALIZED
    assert call(m=0, n=-1) == INVALID_VALUE
    assert call(m=0, base=5) == INVALID_VALUE
    # quick returns: nothing is needed and C is untouched
    assert call(m=0, rp_=None, C_=None, B_=None) == SUCCESS
    assert call(n=0, rp_=None, ldb=0, ldc=0) == SUCCESS
    torch.cuda.synchronize()
    assert C.cpu().tolist() == [7.0] * 8
    assert call() == SUCCESS
    torch.cuda.synchronize()
    assert C.cpu().tolist() == [1.0] * 8
    g = L.spmm_gespmm_csrmm_f16
    assert g(-1, 4, None, None, None, None, None, None) == INVALID_VALUE
    assert g(4, -1, None, None, None, None, None, None) == INVALID_VALUE
    assert g(0, 4, None, None, None, None, None, None) == SUCCESS
    assert g(4, 0, None, None, None, None, None, None) == SUCCESS
    assert g(4, 4, None, None, None, None, None, None) == INVALID_VALUE
    assert g(2, 4, P(rp), P(ci), P(v), P(B), None, None) == INVALID_VALUE


def test_degenerate_shapes_f16(device):
    ops = _ops()
    ci = torch.zeros(0, dtype=torch.int32, device=device)
    v = torch.zeros(0, dtype=torch.float16, device=device)
    B = torch.randn(10, 64, device=device).half()
    # nnz == 0 with m > 0: every row is empty -> beta * C, +0 at beta = 0
    rp = torch.zeros(51, dtype=torch.int32, device=device)
    C = torch.full((50, 64), float("nan"), device=device)
    ops.csrmm_f16(rp, ci, v, B, n=64, k=10, ldb=64, C=C, ldc=64, alpha=2.0)
    torch.cuda.synchronize()
    assert not C.view(torch.int32).any().item(), "an empty row is +0 at beta = 0"
    C = torch.full((50, 64), 3.0, device=device)
    ops.csrmm_f16(rp, ci, v, B, n=64, k=10, ldb=64, C=C, ldc=64, beta=0.5)
    torch.cuda.synchronize()
    assert bool((C == 1.5).all())
    # k == 0 (B is not needed), row-major and column-major
    none = torch.zeros(0, dtype=torch.float16, device=device)
    for ob, oc, ldc in ((0, 0, 5), (1, 1, 50)):
        C = torch.full((50 * 5,), 3.0, device=device)
        ops.csrmm_f16(rp, ci, v, none, m=50, n=5, k=0, ldb=5 if ob == 0 else 1, order_b=ob, C=C,
                      ldc=ldc, order_c=oc, beta=2.0)
        torch.cuda.synchronize()
        assert bool((C == 6.0).all()), (ob, oc)
    # m == 0 and n == 0 are quick returns: C untouched
    C = torch.full((4, 64), 7.0, device=device)
    ops.csrmm_f16(torch.zeros(1, dtype=torch.int32, device=device), ci, v, B, m=0, n=64, k=10,
                  ldb=64, C=C, ldc=64)
    ops.csrmm_f16(rp, ci, v, B, n=0, k=10, ldb=64, C=C, ldc=64)
    out = ops.gespmm_csrmm_f16(torch.zeros(1, dtype=torch.int32, device=device), ci, v, B)
    torch.cuda.synchronize()
    assert out.shape == (0, 64) and bool((C == 7.0).all())
