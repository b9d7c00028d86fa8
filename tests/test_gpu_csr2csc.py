"""spmm_csr2csc_dev (device CSR -> CSC, the CSR form of the transpose) against the numpy
reference of its contract and the host form, bit for bit: every radix pass count, skew,
duplicates, tile tails, unsorted rows, views, index bases, repeatability on a shared
handle, streams, the argument errors found on the device, and the products that run on
its output."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from csr2csc_cases import (TAIL_SIZES, bits, matrices, reference, tail_matrix, values,
                           view_case)
from helpers import TOL_F32, assert_normwise, oracle_csrmm_pieces_f32

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAMES = ["n1", "n200", "n256", "n257", "n4096", "n4097", "random", "skew", "wide", "dups",
         "unsorted"]


def _ops():
    from spmm_hip import ops
    return ops


def _prep():
    from spmm_hip import prep
    return prep


def _dev(*arrs):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
            for a in arrs]


def _host(ts):
    return [t.cpu().numpy() for t in ts]


@functools.lru_cache(maxsize=None)
def _ref(name, vb):
    """(numpy reference, host form) of a named matrix, computed once."""
    m, n, rp, ci = matrices()[name]
    v = values(ci.size, vb)
    return reference(m, n, rp, ci, v), _prep().csr2csc(m, n, rp, ci, v, return_perm=True)


def _same(got, ref, with_val, what):
    """got = (colptr, rowind[, val], perm) arrays; ref = (colptr, rowind, val, perm)."""
    assert np.array_equal(got[0], ref[0]), f"{what}: colptr"
    assert np.array_equal(got[1], ref[1]), f"{what}: rowind"
    if with_val:
        assert got[2].dtype == ref[2].dtype, f"{what}: val dtype"
        assert np.array_equal(bits(got[2]), bits(ref[2])), f"{what}: val"
    assert np.array_equal(got[-1], ref[3]), f"{what}: perm"


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_numpy_and_host(device, name):
    """0 (n1), 1 (n200, n256), 2 (n257, n4096, n4097, random, dups, unsorted), 3 (skew)
    and 4 (wide) radix passes; n4096 / n4097 sit on either side of the column-count scan's
    one-launch limit; skew holds a column longer than any tile and a row with every column;
    dups and unsorted hold equal (row, col) pairs, whose order perm and val expose."""
    m, n, rp, ci = matrices()[name]
    if name == "skew":
        # more than 16 tiles of 8192: the (digit, tile) counts exceed one 4096-count chunk
        # and take the three-launch scan, as the column counts of skew and wide do
        assert ci.size > 16 * 8192 and n > 4096
    v = values(ci.size, 4)
    with _ops().default_handle().launch_record() as rec:
        got = _host(_ops().csr2csc(*_dev(rp, ci, v), m=m, n=n, return_perm=True))
    # the claims above, from the launch record: one digit_scatter_kernel per radix pass;
    # a scan past 4096 counts is chunk_sum_kernel + scan_kernel + chunk_scan_kernel (the
    # column counts once, the (digit, tile) counts once per pass), else scan_kernel alone
    passes = {"n1": 0, "n200": 1, "n256": 1, "skew": 3, "wide": 4}.get(name, 2)
    chunked = int(n > 4096) + passes * int(256 * -(-ci.size // 8192) > 4096)
    count = lambda kernel: sum(kernel in k for k in rec)  # noqa: E731
    assert count("digit_scatter_kernel") == passes == count("digit_count_kernel"), rec
    assert count("chunk_sum_kernel") == chunked == count("chunk_scan_kernel"), rec
    assert count("11scan_kernelE") == 1 + passes, rec
    assert chunked == {"n4097": 1, "skew": 4, "wide": 1}.get(name, 0)
    ref, host = _ref(name, 4)
    _same(got, ref, True, name)
    for a, b, nm in zip(got, host, ("colptr", "rowind", "val", "perm")):
        assert np.array_equal(bits(a) if nm == "val" else a, bits(b) if nm == "val" else b), \
            f"{name}: {nm} differs from the host form"


@pytest.mark.parametrize("vb", [0, 2, 8])
@pytest.mark.parametrize("name", ["dups", "skew"])
def test_value_widths(device, name, vb):
    m, n, rp, ci = matrices()[name]
    v = values(ci.size, vb)
    got = _host(_ops().csr2csc(*_dev(rp, ci), _dev(v)[0], m=m, n=n, return_perm=True))
    assert len(got) == (4 if vb else 3)
    _same(got, _ref(name, vb)[0], vb != 0, f"{name} vb={vb}")


def test_perm_is_optional(device):
    m, n, rp, ci = matrices()["skew"]
    v = values(ci.size, 4)
    ref = _ref("skew", 4)[0]
    cp, ri, cv = _host(_ops().csr2csc(*_dev(rp, ci, v), m=m, n=n))
    assert np.array_equal(cp, ref[0]) and np.array_equal(ri, ref[1])
    assert np.array_equal(bits(cv), bits(ref[2]))
    cp, ri = _host(_ops().csr2csc(*_dev(rp, ci), m=m, n=n))
    assert np.array_equal(cp, ref[0]) and np.array_equal(ri, ref[1])


@pytest.mark.parametrize("nrows", [1, 37])
def test_tails(device, nrows):
    """nnz = 0 ... 130 and every power of two up to 16 K at -1, 0, +1 (n = 300): the
    last partial step of a wave, the last partial wave and the last partial tile."""
    ops = _ops()
    h = ops.Handle()
    bad = []
    for nnz in TAIL_SIZES:
        m, n, rp, ci = tail_matrix(nnz, nrows)
        v = values(nnz, 4)
        got = _host(ops.csr2csc(*_dev(rp, ci, v), m=m, n=n, return_perm=True, handle=h))
        ref = reference(m, n, rp, ci, v)
        try:
            _same(got, ref, True, f"nnz={nnz}")
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, f"{len(bad)} sizes differ: {bad[:8]}"


def test_offset_view(device):
    m, n, rp, ci = view_case()
    v = values(ci.size, 4)
    drp, dci, dv = _dev(matrices()["random"][2], ci, v)
    got = _host(_ops().csr2csc(drp[100:402], dci, dv, m=m, n=n, return_perm=True))
    _same(got, reference(m, n, rp, ci, v), True, "view")
    assert got[3].min() == rp[0] > 0 and got[3].max() == rp[m] - 1


@pytest.mark.parametrize("name", ["dups", "n257"])
@pytest.mark.parametrize("base,base_out", [(1, 0), (0, 1), (1, 1)])
def test_index_bases(device, name, base, base_out):
    m, n, rp, ci = matrices()[name]
    v = values(ci.size, 4)
    got = _host(_ops().csr2csc(*_dev(rp + base, ci + base, v), m=m, n=n, base=base,
                               base_out=base_out, return_perm=True))
    _same(got, reference(m, n, rp + base, ci + base, v, base, base_out), True,
          f"{name} base {base}->{base_out}")
    assert got[0][0] == base_out and got[0][n] == ci.size + base_out


@pytest.mark.parametrize("name", ["dups", "random", "skew"])
def test_double_transpose_returns_the_matrix(device, name):
    m, n, rp, ci = matrices()[name]  # rows sorted by column (dups: with duplicates)
    drp, dci, dv = _dev(rp, ci, values(ci.size, 4))
    cp, ri, cv = _ops().csr2csc(drp, dci, dv, m=m, n=n)
    rp2, ci2, v2 = _ops().csr2csc(cp, ri, cv, m=n, n=m)
    assert torch.equal(rp2, drp) and torch.equal(ci2, dci)
    assert torch.equal(v2.view(torch.int32), dv.view(torch.int32))


def test_repeatable_on_a_shared_handle(device):
    """Three calls in a row give the same bytes, and so do calls with a CSR product and
    a csr2bsr on the same handle in between (they reinterpret its workspace)."""
    ops = _ops()
    h = ops.Handle()
    m, n, rp, ci = matrices()["skew"]
    v = values(ci.size, 4)
    d = _dev(rp, ci, v)
    ref = _ref("skew", 4)[0]
    outs = [ops.csr2csc(*d, m=m, n=n, return_perm=True, handle=h) for _ in range(3)]
    sm, sn, srp, sci = matrices()["random"]
    sd = _dev(srp, sci, values(sci.size, 4))
    B = torch.rand((sn, 128), device=device)
    C = torch.empty((sm, 128), device=device)
    ops.csrmm(*sd, B, n=128, k=sn, ldb=128, C=C, ldc=128, handle=h)
    outs.append(ops.csr2csc(*d, m=m, n=n, return_perm=True, handle=h))
    ops.csr2bsr(*sd, m=sm, n=sn, bs=16, handle=h)
    outs.append(ops.csr2csc(*d, m=m, n=n, return_perm=True, handle=h))
    for i, o in enumerate(outs):
        _same(_host(o), ref, True, f"call {i}")


def test_steady_state_allocates_nothing(device):
    ops = _ops()
    h = ops.Handle()
    m, n, rp, ci = matrices()["skew"]
    d = _dev(rp, ci, values(ci.size, 4))
    ops.csr2csc(*d, m=m, n=n, return_perm=True, handle=h)
    ops.csr2csc(*d, m=m, n=n, handle=h)  # without perm: one more position buffer
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]  # the outputs below come from torch's cache
    for _ in range(3):
        out = ops.csr2csc(*d, m=m, n=n, return_perm=True, handle=h)
        del out
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0


def test_non_default_stream(device):
    ops = _ops()
    m, n, rp, ci = matrices()["skew"]
    d = _dev(rp, ci, values(ci.size, 4))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    h = ops.Handle(s)
    with torch.cuda.stream(s):
        out = ops.csr2csc(*d, m=m, n=n, return_perm=True, handle=h)
    s.synchronize()
    _same(_host(out), _ref("skew", 4)[0], True, "stream")


def test_refused_under_capture(device):
    """The call reads a flag back: under capture it is refused before anything is
    queued, and the capture stays valid."""
    from spmm_hip._lib import NOT_SUPPORTED, SpmmError
    ops = _ops()
    m, n, rp, ci = matrices()["dups"]
    d = _dev(rp, ci, values(ci.size, 4))
    s = torch.cuda.Stream()
    h = ops.Handle(s)
    with torch.cuda.stream(s):
        ops.csr2csc(*d, m=m, n=n, handle=h)  # sizes the workspace
        s.synchronize()
        x = torch.zeros(8, device=device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            with pytest.raises(SpmmError) as e:
                ops.csr2csc(*d, m=m, n=n, nnz=ci.size, handle=h)
            x += 1
    assert e.value.status == NOT_SUPPORTED
    g.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0


def test_argument_errors_found_on_the_device(device):
    """A column >= n, a negative column, an nnz one larger than the row pointer's and a
    decreasing row pointer: INVALID_VALUE by a flag, and the process stays healthy."""
    from spmm_hip._lib import INVALID_VALUE, SpmmError
    ops = _ops()
    h = ops.Handle()
    m, n, rp, ci = matrices()["dups"]
    v = values(ci.size, 4)
    cases = []
    for bad in (n, n + 70000, -1, -(1 << 30)):
        c = ci.copy()
        c[17] = bad
        cases.append((rp, c, v, ci.size))
    cases.append((rp, np.append(ci, 0).astype(np.int32), np.append(v, 0).astype(np.float32),
                  ci.size + 1))
    dec = rp.copy()
    dec[10] = dec[12] + 1
    cases.append((dec, ci, v, ci.size))
    for r, c, vv, nnz in cases:
        with pytest.raises(SpmmError) as e:
            ops.csr2csc(*_dev(r, c, vv), m=m, n=n, nnz=nnz, return_perm=True, handle=h)
        assert e.value.status == INVALID_VALUE
    with pytest.raises(SpmmError) as e:  # n below the largest column
        ops.csr2csc(*_dev(rp, ci, v), m=m, n=int(ci.max()), handle=h)
    assert e.value.status == INVALID_VALUE
    got = _host(ops.csr2csc(*_dev(rp, ci, v), m=m, n=n, return_perm=True, handle=h))
    _same(got, _ref("dups", 4)[0], True, "after the errors")


def test_empty_matrices(device):
    ops = _ops()
    z = torch.zeros(6, dtype=torch.int32, device=device)
    e = torch.zeros(0, dtype=torch.int32, device=device)
    cp, ri = ops.csr2csc(z, e, m=5, n=7, base_out=1)
    assert cp.tolist() == [1] * 8 and ri.numel() == 0
    cp, ri = ops.csr2csc(z[:1], e, m=0, n=0)
    assert cp.tolist() == [0] and ri.numel() == 0


# ------------------------------------------------------------------ products
def _dense(m, n, rp, ci, v):
    A = np.zeros((m, n), np.float64)
    np.add.at(A, (np.repeat(np.arange(m), np.diff(rp)), ci), v.astype(np.float64))
    return A


@pytest.mark.parametrize("K", [8, 128, 256])
@pytest.mark.parametrize("name", ["random", "dups"])
def test_product_on_the_transposed_matrix(device, oracle, name, K):
    """ops.csrmm on the device-transposed arrays: equal to the product on the
    host-transposed arrays, bit-equal to the piece oracle on them (the main kernel: at
    K = 8 under SPMM_CSR_SEQUENTIAL_ROWS, where the default is the lane-group kernel,
    DESIGN.md §3c), and within |C - C_ref| <= 1e-5 sum |a||b| of the fp64 product of the
    dense transpose."""
    from spmm_hip._lib import CSR_NT_STREAMS, CSR_SEQUENTIAL_ROWS
    ops = _ops()
    m, n, rp, ci = matrices()[name]
    v = values(ci.size, 4)
    tcp, tri, tv = ops.csr2csc(*_dev(rp, ci, v), m=m, n=n)
    hcp, hri, hv = _prep().csr2csc(m, n, rp, ci, v)
    B = np.random.default_rng(5).uniform(-1, 1, (m, K)).astype(np.float32)
    dB = _dev(B)[0]
    h = ops.Handle()
    if K <= 64:
        h.set_csr_options(CSR_NT_STREAMS | CSR_SEQUENTIAL_ROWS)
    outs = []
    for arrs in ((tcp, tri, tv), tuple(_dev(hcp, hri, hv))):
        for hd in (None, h):
            C = torch.full((n, K), float("nan"), device=device)
            ops.csrmm(*arrs, dB, m=n, n=K, k=m, ldb=K, C=C, ldc=K, handle=hd)
            outs.append(C)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[2]), "default kernel: device and host transposes differ"
    assert torch.equal(outs[1], outs[3]), "main kernel: device and host transposes differ"
    pcs = oracle_csrmm_pieces_f32(oracle, n, K, hcp, hri, hv, B, K, 0).reshape(n, K)
    got = outs[1].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), pcs.view(np.uint32)), "piece oracle"
    A = _dense(m, n, rp, ci, v)
    ref = A.T @ B.astype(np.float64)
    # sum |a||b| over the entries, each duplicate on its own
    absd = _dense(m, n, rp, ci, np.abs(v)).T @ np.abs(B).astype(np.float64)
    for C in outs:
        assert_normwise(C.cpu().numpy(), ref, absd, TOL_F32, f"{name} K={K} vs fp64")


@pytest.mark.parametrize("K", [8, 128, 256])
@pytest.mark.parametrize("name", ["random", "dups"])
def test_f16_product_on_the_transposed_matrix(device, name, K):
    """ops.csr2csc with half values, then ops.csrmm_f16: the bits of the fp32 entry on
    the widened transposed inputs under SPMM_CSR_SEQUENTIAL_ROWS."""
    from spmm_hip._lib import CSR_NT_STREAMS, CSR_SEQUENTIAL_ROWS
    ops = _ops()
    m, n, rp, ci = matrices()[name]
    v16 = values(ci.size, 2)
    tcp, tri, tv16 = ops.csr2csc(*_dev(rp, ci, v16), m=m, n=n)
    assert tv16.dtype == torch.float16
    ref = _ref(name, 2)[0]
    assert np.array_equal(bits(tv16.cpu().numpy()), bits(ref[2]))
    B16 = torch.from_numpy(np.random.default_rng(6).uniform(-1, 1, (m, K)).astype(np.float16)).cuda()
    C16 = torch.full((n, K), float("nan"), device=device)
    ops.csrmm_f16(tcp, tri, tv16, B16, m=n, n=K, k=m, ldb=K, C=C16, ldc=K)
    h = ops.Handle()
    h.set_csr_options(CSR_NT_STREAMS | CSR_SEQUENTIAL_ROWS)
    C32 = torch.full((n, K), float("nan"), device=device)
    ops.csrmm(tcp, tri, tv16.float(), B16.float(), m=n, n=K, k=m, ldb=K, C=C32, ldc=K, handle=h)
    torch.cuda.synchronize()
    assert torch.equal(C16.view(torch.int32), C32.view(torch.int32))


@pytest.mark.parametrize("bs", [16, 32])
@pytest.mark.parametrize("name", ["random", "dups"])
def test_device_output_feeds_csr2bsr(device, name, bs):
    """The output's rows are sorted by column, as csr2bsr requires: csr2bsr of the device
    transpose equals the host csr2bsr of the host transpose."""
    ops = _ops()
    m, n, rp, ci = matrices()[name]
    v = values(ci.size, 4)
    tcp, tri, tv = ops.csr2csc(*_dev(rp, ci, v), m=m, n=n)
    got = _host(ops.csr2bsr(tcp, tri, tv, m=n, n=m, bs=bs))
    want = _prep().csr2bsr(n, m, *_prep().csr2csc(m, n, rp, ci, v), bs)
    for a, b, nm in zip(got, want, ("rowptr", "colind", "val")):
        assert np.array_equal(a, b), f"{name} bs={bs}: {nm}"
