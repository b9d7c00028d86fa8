"""The device edge softmax (spmm_edge_softmax_csr_f32 / _bwd_csr_f32) against its host
form's rule, bit for bit, on every case of softmax_cases: out of place, in place, on a
misaligned base, under another grid, on a second handle and stream, captured in a graph;
which kernel each case launches, and that the new file ships no kernel these tests miss."""
import contextlib
import ctypes
import re

import numpy as np
import pytest
import torch

import kernel_keys
import softmax_cases as sc
from softmax_cases import F

pytestmark = pytest.mark.gpu

SENTINEL = F(-7.25)


def _ops():
    from spmm_hip import ops
    return ops


@contextlib.contextmanager
def _side_stream():
    """A stream of the test's own, made and destroyed through the HIP runtime the library
    is linked against (resolved through the library's handle) and wrapped for torch.
    torch.cuda.Stream() would hand out the next stream of torch's pool of 32 and never
    give it back: which pool streams the later test files get, and which hardware queue
    each of them shares, would then depend on how many this file took. This one is gone,
    queue reference included, when the block ends."""
    from spmm_hip._lib import lib
    hip = lib()
    create, destroy = hip.hipStreamCreateWithFlags, hip.hipStreamDestroy
    create.argtypes, create.restype = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint], ctypes.c_int
    destroy.argtypes, destroy.restype = [ctypes.c_void_p], ctypes.c_int
    raw = ctypes.c_void_p()
    assert create(ctypes.byref(raw), 1) == 0, "hipStreamCreateWithFlags"  # hipStreamNonBlocking
    s = torch.cuda.ExternalStream(raw.value)
    s.wait_stream(torch.cuda.current_stream())
    try:
        yield s
    finally:
        s.synchronize()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        assert destroy(raw) == 0, "hipStreamDestroy"


def _dev(a, device, offset=0):
    """a on the device, `offset` floats past a 16-byte aligned base."""
    t = torch.from_numpy(np.array(a))  # a copy: the cases are read-only
    if offset == 0:
        return t.to(device)
    buf = torch.empty(t.numel() + offset + 4, dtype=t.dtype, device=device)
    assert buf.data_ptr() % 16 == 0
    out = buf[offset:offset + t.numel()]
    out.copy_(t)
    return out


def _guarded(n, device, offset=0):
    """(buffer, view): n floats of the sentinel between NaN guards."""
    buf = torch.full((n + 64 + offset,), float("nan"), dtype=torch.float32, device=device)
    view = buf[32 + offset:32 + offset + n]
    view.fill_(float(SENTINEL))
    return buf, view


def _check_guards(buf, n, offset=0):
    b = buf.cpu().numpy()
    assert np.isnan(b[:32 + offset]).all() and np.isnan(b[32 + offset + n:]).all(), "guards"


def _run(c, device, handle=None, offset=0):
    """(y, gx) of the device entries as numpy, with every side condition checked."""
    ops = _ops()
    rp = _dev(c.rowptr, device)
    x, g = _dev(c.x, device, offset), _dev(c.g, device, offset)
    yin = _dev(sc.forward_bits(c.name), device, offset)
    ybuf, y = _guarded(c.nnz, device, offset)
    gbuf, gx = _guarded(c.nnz, device, offset)
    torch.cuda.synchronize()  # the operands are in place, whichever stream the handle is on
    assert ops.edge_softmax(rp, x, base=c.base, out=y, handle=handle) is y
    ops.edge_softmax_bwd(rp, yin, g, base=c.base, out=gx, handle=handle)
    torch.cuda.synchronize()
    _check_guards(ybuf, c.nnz, offset)
    _check_guards(gbuf, c.nnz, offset)
    assert np.array_equal(rp.cpu().numpy(), c.rowptr)
    assert np.array_equal(sc.bits(x.cpu().numpy()), sc.bits(c.x)), "x changed"
    assert np.array_equal(sc.bits(g.cpu().numpy()), sc.bits(c.g)), "g changed"
    return y.cpu().numpy(), gx.cpu().numpy()


def _hold(c, y, gx, where):
    mk = sc.inside(c)
    sc.assert_same(y, sc.forward_bits(c.name), f"{c.name} {where} forward", mk)
    sc.assert_same(gx, sc.backward_bits(c.name), f"{c.name} {where} backward", mk)
    assert (y[~mk] == SENTINEL).all() and (gx[~mk] == SENTINEL).all(), "outside the view"


@pytest.fixture(scope="module")
def host_equals_rule():
    """The host form on every case, once: the device is compared with the restated rule,
    which the host form equals (tests/test_edge_softmax_host.py checks that on its own)."""
    from spmm_hip import prep
    for name in sc.NAMES:
        c = sc.case(name)
        sc.assert_same(prep.edge_softmax(c.rowptr, c.x, base=c.base), sc.forward_bits(name),
                       name + " host", sc.inside(c))
        sc.assert_same(prep.edge_softmax_bwd(c.rowptr, sc.forward_bits(name), c.g, base=c.base),
                       sc.backward_bits(name), name + " host bwd", sc.inside(c))


@pytest.mark.parametrize("name", sc.NAMES)
def test_device_equals_host(device, host_equals_rule, name):
    c = sc.case(name)
    _hold(c, *_run(c, device), "aligned")
    _hold(c, *_run(c, device, offset=1), "one float past a 16-byte base")


@pytest.mark.parametrize("name", sc.NAMES)
def test_in_place(device, name):
    ops = _ops()
    c = sc.case(name)
    mk = sc.inside(c)
    rp = _dev(c.rowptr, device)
    x, g = _dev(c.x, device), _dev(c.g, device)
    ops.edge_softmax(rp, x, base=c.base, out=x)
    ops.edge_softmax_bwd(rp, _dev(sc.forward_bits(name), device), g, base=c.base, out=g)
    torch.cuda.synchronize()
    x, g = x.cpu().numpy(), g.cpu().numpy()
    sc.assert_same(x, sc.forward_bits(name), name + " in place", mk)
    sc.assert_same(g, sc.backward_bits(name), name + " bwd in place", mk)
    assert np.array_equal(sc.bits(x[~mk]), sc.bits(c.x[~mk]))
    assert np.array_equal(sc.bits(g[~mk]), sc.bits(c.g[~mk]))


@pytest.mark.parametrize("name", ["lengths", "short_mixed", "mid", "special"])
def test_grid_and_handle_do_not_reach_the_bits(device, name):
    ops = _ops()
    c = sc.case(name)
    h = ops.Handle()
    try:
        for w in (1, 3, 32):
            h.set_csr_waves_per_cu(w)
            _hold(c, *_run(c, device, handle=h), f"{w} waves per CU")
    finally:
        torch.cuda.synchronize()
        h.close()
    with _side_stream() as s:
        h2 = ops.Handle(stream=s)  # torch's current stream stays the default one
        try:
            _hold(c, *_run(c, device, handle=h2), "a second handle on another stream")
        finally:
            torch.cuda.synchronize()
            h2.close()


def _key_of(G, bwd):
    return re.compile(rf"edge_softmax_kernelILi{G}ELb{int(bwd)}EE")


def test_kernel_coverage(device):
    """Each case launches exactly one kernel per call, the instantiation its mean row
    length selects (rows of more than one piece are done inside it, by the workgroup that
    owns them: there is no second kernel), nothing at nnz = 0; and the union over the
    cases is every kernel softmax_kernels.hip ships."""
    ops = _ops()
    shipped = {kernel_keys.launch_key(k) for k in kernel_keys.shipped_kernels(("softmax_kernels",))}
    assert len(shipped) == 6, sorted(shipped)
    seen = set()
    h = ops.Handle()
    try:
        for name in sc.NAMES:
            c = sc.case(name)
            rp, x, g = _dev(c.rowptr, device), _dev(c.x, device), _dev(c.g, device)
            y = torch.empty_like(x)
            with h.launch_record() as fwd:
                ops.edge_softmax(rp, x, base=c.base, out=y, handle=h)
            with h.launch_record() as bwd:
                ops.edge_softmax_bwd(rp, y, g, base=c.base, out=x, handle=h)
            if c.nnz == 0:
                assert fwd == [] and bwd == [], name
                continue
            assert len(fwd) == 1 and _key_of(c.group_lanes(), False).search(fwd[0]), (name, fwd)
            assert len(bwd) == 1 and _key_of(c.group_lanes(), True).search(bwd[0]), (name, bwd)
            seen |= set(fwd) | set(bwd)
        torch.cuda.synchronize()
    finally:
        h.close()
    assert seen == shipped, f"never launched: {sorted(shipped - seen)}; unknown: {sorted(seen - shipped)}"
    # the cases reach every lane-group width with a row of more than one piece
    assert {sc.case(n).group_lanes() for n in sc.NAMES if sc.case(n).has_long_row()} == {4, 16, 64}


def test_timing_covers_the_kernel(device):
    ops = _ops()
    c = sc.case("mid")
    h = ops.Handle()
    try:
        h.set_timing(True)
        rp, x = _dev(c.rowptr, device), _dev(c.x, device)
        y = ops.edge_softmax(rp, x, handle=h)
        ops.edge_softmax_bwd(rp, y, _dev(c.g, device), handle=h)
        torch.cuda.synchronize()
        times = h.kernel_times()
        assert len(times) == 2 and all(t > 0 for t in times), times
    finally:
        h.close()


def test_device_status_codes(device):
    from ctypes import c_void_p

    from spmm_hip._lib import INVALID_VALUE, NOT_INITIALIZED, SUCCESS, lib
    ops = _ops()
    L = lib()
    c = sc.case("m1")
    rp, x = _dev(c.rowptr, device), _dev(c.x, device)
    y = torch.empty_like(x)
    h = ops.default_handle().raw
    P = lambda t: c_void_p(t.data_ptr())  # noqa: E731
    fwd, bwd = L.spmm_edge_softmax_csr_f32, L.spmm_edge_softmax_bwd_csr_f32
    assert fwd(None, -1, 5, P(rp), 0, P(x), P(y)) == NOT_INITIALIZED
    assert bwd(None, 1, 5, P(rp), 0, P(x), P(x), P(y)) == NOT_INITIALIZED
    assert fwd(h, -1, 5, P(rp), 0, P(x), P(y)) == INVALID_VALUE
    assert fwd(h, 1, -5, P(rp), 0, P(x), P(y)) == INVALID_VALUE
    assert fwd(h, 1, 5, P(rp), 2, P(x), P(y)) == INVALID_VALUE
    assert fwd(h, 1, 5, None, 0, P(x), P(y)) == INVALID_VALUE
    assert fwd(h, 1, 5, P(rp), 0, P(x), None) == INVALID_VALUE
    assert bwd(h, 1, 5, P(rp), 0, P(x), None, P(y)) == INVALID_VALUE
    assert fwd(h, 0, 5, None, 0, None, None) == INVALID_VALUE
    assert fwd(h, 0, 5, P(rp), 0, P(x), P(y)) == SUCCESS
    assert fwd(h, 1, 0, None, 0, None, None) == SUCCESS
    assert bwd(h, 1, 0, None, 0, None, None, None) == SUCCESS
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["lengths", "short_mixed"])
def test_graph_replay_equals_eager(device, name):
    """Captured on a side stream after one eager call; replayed after x (y, g) have been
    overwritten with new values: the replay re-reads them and equals the eager call."""
    ops = _ops()
    c = sc.case(name)
    rng = np.random.default_rng(17)
    x2 = rng.normal(0, 3, c.nnz).astype(F)
    g2 = rng.normal(0, 1, c.nnz).astype(F)
    # every tensor is made on torch's current (default) stream; only the handle's launches
    # and the capture run on the side stream, with device-wide synchronisation between
    rp, x, g = _dev(c.rowptr, device), _dev(c.x, device), _dev(c.g, device)
    y, gx = torch.empty_like(x), torch.empty_like(x)
    want_y, want_gx = torch.empty_like(x), torch.empty_like(x)
    torch.cuda.synchronize()
    with _side_stream() as s:
        h = ops.Handle(stream=s)
        ops.edge_softmax(rp, x, out=y, handle=h)
        ops.edge_softmax_bwd(rp, y, g, out=gx, handle=h)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        try:
            try:
                with torch.cuda.graph(graph, stream=s):
                    h.set_stream(s)
                    ops.edge_softmax(rp, x, out=y, handle=h)
                    ops.edge_softmax_bwd(rp, y, g, out=gx, handle=h)
            finally:
                h.set_stream(s)
            x.copy_(torch.from_numpy(x2))
            g.copy_(torch.from_numpy(g2))
            y.fill_(0)
            gx.fill_(0)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                graph.replay()
            torch.cuda.synchronize()
            got_y, got_gx = y.cpu().numpy(), gx.cpu().numpy()
            ops.edge_softmax(rp, x, out=want_y, handle=h)
            ops.edge_softmax_bwd(rp, want_y, g, out=want_gx, handle=h)
            torch.cuda.synchronize()
            assert np.array_equal(sc.bits(got_y), sc.bits(want_y.cpu().numpy()))
            assert np.array_equal(sc.bits(got_gx), sc.bits(want_gx.cpu().numpy()))
            assert not np.array_equal(got_y, sc.forward_bits(name))  # the new values were read
        finally:
            graph.reset()
            torch.cuda.synchronize()
            h.close()


def test_repeat_allocates_nothing(device):
    ops = _ops()
    c = sc.case("lengths")
    rp, x, g = _dev(c.rowptr, device), _dev(c.x, device), _dev(c.g, device)
    y, gx = torch.empty_like(x), torch.empty_like(x)
    h = ops.Handle()
    try:
        ops.edge_softmax(rp, x, out=y, handle=h)
        ops.edge_softmax_bwd(rp, y, g, out=gx, handle=h)
        torch.cuda.synchronize()
        # the entries take nothing from the handle (no workspace to expose): torch's own
        # count is all there is to watch
        before = torch.cuda.memory_allocated()
        for _ in range(3):
            ops.edge_softmax(rp, x, out=y, handle=h)
            ops.edge_softmax_bwd(rp, y, g, out=gx, handle=h)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
    finally:
        h.close()
