"""The device max / min reducers (ops.csrmm_reduce, ops.csrmm_reduce_bwd) = their host forms,
bit for bit for C, arg and dB (a NaN matching any NaN), over every case of reduce_cases at
every width, tight and padded / offset layouts with their guards, base 0 and 1; after a
relaunch, on another grid, on a second stream and from a graph replay; with arg = NULL; on a
corrupt arg; with each dense operand past 2^31 and 2^32 bytes and 2^31 elements; and the
kernels the calls launch: together every kernel reduce_kernels.hip ships."""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np
import pytest
import torch

import far_cases as fc
import kernel_keys
import reduce_cases as rc
from helpers import framed

pytestmark = pytest.mark.gpu

ARG_FILL = 0x5A5A5A5A  # the sentinel of an int operand's guards and padding


def _ops():
    from spmm_hip import ops
    return ops


def _prep():
    from spmm_hip import prep
    return prep


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _np(t):
    return t.detach().cpu().numpy()


@contextlib.contextmanager
def _handle(stream=None):
    """A handle of the test's own, closed behind a device synchronisation."""
    h = _ops().Handle(stream=stream)
    try:
        yield h
    finally:
        torch.cuda.synchronize()
        h.close()


@contextlib.contextmanager
def _side_stream():
    """A non-blocking stream of the test's own, made and destroyed through the HIP runtime the
    library is linked against and wrapped for torch."""
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


def _frame(a, pad, off):
    """helpers.framed of a 2-D host array at leading dimension columns + pad, `off` elements
    past a 16-byte base; an int array's guards hold ARG_FILL."""
    a = np.ascontiguousarray(a)
    return framed(a, a.shape[1] + pad, off, fill=ARG_FILL if a.dtype == np.int32 else None)


# ------------------------------------------------------------------ every case
LAYOUTS = ((0, 0, 0), (3, 1, 1))  # (padding columns, offset in elements, index base)


@pytest.mark.parametrize("pat,vs", [(p, v) for p in rc.PATTERNS for v in rc.VALUE_SETS])
def test_device_equals_host(device, pat, vs):
    """Forward (C and arg) and backward (dB, on the host form's arg) at every width, tight at
    base 0 and with three padding columns, every operand one element past a 16-byte base, at
    base 1: the vector loads must fall back, and nothing outside the n columns may change."""
    ops = _ops()
    m, k, rp, ci = rc.pattern(pat)
    trp, tci, perm = rc.host_transpose(pat)
    d_perm = _dev(perm)
    csr = {b: (_dev(rp + b), _dev(ci + b), _dev(trp + b), _dev(tci + b)) for b in (0, 1)}
    with _handle() as h:
        for reduce in rc.REDUCES:
            for n in rc.WIDTHS:
                val, B = rc.values(pat, vs, reduce, n)
                wantC, wantA = rc.host_fwd(pat, vs, reduce, n)
                dC = rc.grad_out(pat, n)
                want_dB = rc.host_bwd(pat, val, dC, wantA)
                d_val = _dev(val)
                for pad, off, base in LAYOUTS:
                    what = f"{pat} {vs} {reduce} n={n} pad={pad} off={off} base={base}"
                    d_rp, d_ci, d_trp, d_tci = csr[base]
                    Bv, chkB = _frame(B, pad, off)
                    Cv, chkC = _frame(np.full((m, n), np.nan, np.float32), pad, off)
                    Av, chkA = _frame(np.full((m, n), 7, np.int32), pad, off)
                    ops.csrmm_reduce(d_rp, d_ci, d_val, Bv, reduce=reduce, m=m, n=n, k=k,
                                     ldb=n + pad, C=Cv, ldc=n + pad, arg=Av, ldarg=n + pad,
                                     base=base, handle=h)
                    assert np.array_equal(chkA(what + ": arg"), wantA), what + ": arg"
                    assert rc.same_bits(chkC(what + ": C"), wantC), what + ": C"
                    chkB.unchanged(what + ": B")
                    Gv, chkG = _frame(dC, pad, off)
                    Wv, chkW = _frame(wantA, pad, off)
                    Dv, chkD = _frame(np.full((k, n), np.nan, np.float32), pad, off)
                    ops.csrmm_reduce_bwd(d_trp, d_tci, d_perm, d_val, Gv, Wv, k=k, n=n, m=m,
                                         lddc=n + pad, ldarg=n + pad, dB=Dv, lddb=n + pad,
                                         base=base, handle=h)
                    assert rc.same_bits(chkD(what + ": dB"), want_dB), what + ": dB"
                    chkG.unchanged(what + ": dC")
                    chkW.unchanged(what + ": arg (backward)")


# ------------------------------------------------------------------ relaunch, grid, stream, graph
def _chain(ops, h, pat, vs, reduce, n, C, arg, dB):
    """Forward and backward of a case into C, arg, dB. The operands are in place before the
    first launch and alive until the last has ended, whichever stream the handle is on (they
    are copied on torch's current stream, and their memory goes back to its allocator)."""
    m, k, rp, ci = rc.pattern(pat)
    val, B = rc.values(pat, vs, reduce, n)
    d = [_dev(x) for x in (rp, ci, val, B) + tuple(rc.host_transpose(pat)) +
         (rc.grad_out(pat, n),)]
    torch.cuda.synchronize()
    ops.csrmm_reduce(d[0], d[1], d[2], d[3], reduce=reduce, m=m, n=n, k=k, C=C, arg=arg, handle=h)
    ops.csrmm_reduce_bwd(d[4], d[5], d[6], d[2], d[7], arg, k=k, n=n, m=m, dB=dB, handle=h)
    torch.cuda.synchronize()


def _outs(pat, n, device):
    m, k, _, _ = rc.pattern(pat)
    return (torch.full((m, n), np.nan, device=device),
            torch.full((m, n), 7, dtype=torch.int32, device=device),
            torch.full((k, n), np.nan, device=device))


def _check(outs, pat, vs, reduce, n, what):
    val, _ = rc.values(pat, vs, reduce, n)
    wantC, wantA = rc.host_fwd(pat, vs, reduce, n)
    C, arg, dB = (_np(t) for t in outs)
    assert np.array_equal(arg, wantA), what + ": arg"
    assert rc.same_bits(C, wantC), what + ": C"
    assert rc.same_bits(dB, rc.host_bwd(pat, val, rc.grad_out(pat, n), wantA)), what + ": dB"


RUNS = (("hub_row", "generic", "max", 260), ("hub_col", "ties", "min", 37),
        ("lens", "nan_two", "max", 128))


def test_relaunch_grid_and_stream_do_not_reach_the_bits(device):
    ops = _ops()
    for pat, vs, reduce, n in RUNS:
        with _handle() as h:
            outs = _outs(pat, n, device)
            for i in range(2):  # a relaunch into the same outputs
                _chain(ops, h, pat, vs, reduce, n, *outs)
                _check(outs, pat, vs, reduce, n, f"{pat} launch {i}")
            for wv in (1, 7):   # other grids: other shares of the merge path
                h.set_csr_waves_per_cu(wv)
                outs = _outs(pat, n, device)
                _chain(ops, h, pat, vs, reduce, n, *outs)
                _check(outs, pat, vs, reduce, n, f"{pat}, {wv} waves per CU")
        with _side_stream() as s:
            torch.cuda.synchronize()
            with _handle(s) as h2:
                outs = _outs(pat, n, device)
                torch.cuda.synchronize()
                _chain(ops, h2, pat, vs, reduce, n, *outs)
                torch.cuda.synchronize()
                _check(outs, pat, vs, reduce, n, f"{pat} on a second stream")


def test_graph_replay_equals_eager(device):
    """Forward and backward captured once on a side stream after an eager call; replayed after
    B and the outputs were overwritten: the replay re-reads B and gives the host form's bits."""
    ops = _ops()
    pat, vs, reduce, n = RUNS[0]
    _, B0 = rc.values(pat, vs, reduce, n)
    _, B1 = rc.values(pat, vs, "min", n)          # other contents of the same shape
    B = _dev(B1)
    outs = _outs(pat, n, device)
    m, k, rp, ci = rc.pattern(pat)
    trp, tci, perm = rc.host_transpose(pat)
    val, _ = rc.values(pat, vs, reduce, n)
    d = [_dev(x) for x in (rp, ci, val, trp, tci, perm, rc.grad_out(pat, n))]

    def run(h):
        ops.csrmm_reduce(d[0], d[1], d[2], B, reduce=reduce, m=m, n=n, k=k, C=outs[0],
                         arg=outs[1], handle=h)
        ops.csrmm_reduce_bwd(d[3], d[4], d[5], d[2], d[6], outs[1], k=k, n=n, m=m, dB=outs[2],
                             handle=h)

    torch.cuda.synchronize()
    with _side_stream() as s:
        h = ops.Handle(stream=s)
        run(h)
        torch.cuda.synchronize()
        first = _np(outs[0])
        graph = torch.cuda.CUDAGraph()
        try:
            try:
                with torch.cuda.graph(graph, stream=s):
                    h.set_stream(s)
                    run(h)
            finally:
                h.set_stream(s)
            B.copy_(torch.from_numpy(B0))
            outs[0].fill_(float("nan"))
            outs[1].fill_(7)
            outs[2].fill_(float("nan"))
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                graph.replay()
            torch.cuda.synchronize()
            _check(outs, pat, vs, reduce, n, "replay")
            assert not np.array_equal(_np(outs[0]), first)  # the new B was read
        finally:
            graph.reset()
            torch.cuda.synchronize()
            h.close()


# ------------------------------------------------------------------ arg = NULL, corrupt arg
def test_without_arg_the_same_C(device):
    ops = _ops()
    with _handle() as h:
        for pat, vs, reduce, n in RUNS + (("lens", "zero_tie", "max", 6),):
            m, k, rp, ci = rc.pattern(pat)
            val, B = rc.values(pat, vs, reduce, n)
            C = ops.csrmm_reduce(_dev(rp), _dev(ci), _dev(val), _dev(B), reduce=reduce, m=m, k=k,
                                 return_arg=False, handle=h)
            assert isinstance(C, torch.Tensor)
            assert rc.same_bits(_np(C), rc.host_fwd(pat, vs, reduce, n)[0]), (pat, vs)


def test_corrupt_arg_is_only_compared(device):
    """arg holding positions >= nnz, negative positions and INT_MIN in place of winners: an
    input the contract allows. The run is clean and dB equals the host form on the same arg
    (nothing is selected there; the rest is selected as before)."""
    ops = _ops()
    imin, imax = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    with _handle() as h:
        for pat, n in (("hub_col", 37), ("hub_row", 260), ("lens", 128)):
            m, k, rp, ci = rc.pattern(pat)
            trp, tci, perm = rc.host_transpose(pat)
            val, _ = rc.values(pat, "generic", "max", n)
            arg = rc.host_fwd(pat, "generic", "max", n)[1].copy()
            rng = np.random.default_rng(n)
            junk = rng.choice(np.array([ci.size, ci.size + 1, imax, -1, -2, -ci.size, imin],
                                       np.int64), arg.shape).astype(np.int32)
            arg = np.where(rng.random(arg.shape) < 0.5, junk, arg)
            dC = rc.grad_out(pat, n)
            for a in (arg, np.full_like(arg, imin), np.full_like(arg, ci.size)):
                got = ops.csrmm_reduce_bwd(_dev(trp), _dev(tci), _dev(perm), _dev(val), _dev(dC),
                                           _dev(a), k=k, n=n, m=m, handle=h)
                torch.cuda.synchronize()
                assert rc.same_bits(_np(got), rc.host_bwd(pat, val, dC, a)), (pat, n)


# ------------------------------------------------------------------ far operands
@pytest.fixture(scope="module")
def arena(device):
    a = fc.Arena()
    torch.cuda.synchronize()
    yield a
    a.close()


FAR_N = 136  # the widest row of far_cases' arena; a multiple of 4: the widest lanes


def _far_problem(far_rows_are, seed):
    """A matrix whose far operand has far_cases.F32's nine rows: "k" (B and dB: 20 x 9) or
    "m" (C, arg and dC: 9 x 16); -> m, k, rp, ci, val, B, C, arg, dC, (trp, tci, perm), dB."""
    prep = _prep()
    rng = np.random.default_rng(seed)
    g = fc.F32
    m, k = (20, g.rows) if far_rows_are == "k" else (g.rows, 16)
    rp, ci, val = fc.far_csr(rng, m, k, long_row=min(7, m - 2), last_empty=False)
    B = rng.standard_normal((k, FAR_N)).astype(np.float32)
    C, arg = prep.csrmm_reduce(m, FAR_N, k, rp, ci, val, B)
    dC = rng.standard_normal((m, FAR_N)).astype(np.float32)
    T = prep.csr2csc(m, k, rp, ci, return_perm=True)
    dB = prep.csrmm_reduce_bwd(k, FAR_N, m, *T, val, dC, arg)
    return m, k, rp, ci, val, B, C, arg, dC, T, dB


@pytest.mark.parametrize("which", ["B", "C", "arg", "dC", "dB"])
def test_far_operand(device, arena, which):
    """One dense operand at far_cases.F32's geometry (ld 2^28: row 2 at 2^31 bytes, row 4 at
    2^32 bytes, row 8 at 2^31 elements), the others compact: every row carries the host
    form's bits, and the guards around every far row are untouched."""
    ops = _ops()
    g = fc.F32
    m, k, rp, ci, val, B, C, arg, dC, T, dB = _far_problem("k" if which in ("B", "dB") else "m",
                                                           {"B": 1, "C": 2, "arg": 3, "dC": 4,
                                                            "dB": 5}[which])
    for row, unit, bound in g.crossings:
        assert g.start(row, unit) >= bound > g.start(row - 1, unit)
    junkf = lambda r: np.full((r, FAR_N), np.nan, np.float32)  # noqa: E731
    junki = lambda r: np.full((r, FAR_N), 7, np.int32)         # noqa: E731
    d_rp, d_ci, d_val = _dev(rp), _dev(ci), _dev(val)
    with _handle() as h:
        if which in ("B", "C", "arg"):
            far = arena.place({"B": B, "C": junkf(m), "arg": junki(m)}[which], g.ld)
            Bv = far.view if which == "B" else _dev(B)
            Cv = far.view if which == "C" else _dev(junkf(m))
            Av = far.view if which == "arg" else _dev(junki(m))
            ld = lambda w: g.ld if which == w else FAR_N  # noqa: E731
            ops.csrmm_reduce(d_rp, d_ci, d_val, Bv, m=m, n=FAR_N, k=k, ldb=ld("B"), C=Cv,
                             ldc=ld("C"), arg=Av, ldarg=ld("arg"), handle=h)
            torch.cuda.synchronize()
            gotC = far(which) if which == "C" else _np(Cv).reshape(m, FAR_N)
            gotA = far(which) if which == "arg" else _np(Av).reshape(m, FAR_N)
            if which == "B":
                far.unchanged("B")
            assert np.array_equal(gotA, arg) and rc.same_bits(gotC, C), which
        else:
            far = arena.place(dC if which == "dC" else junkf(k), g.ld)
            Gv = far.view if which == "dC" else _dev(dC)
            Dv = far.view if which == "dB" else _dev(junkf(k))
            ops.csrmm_reduce_bwd(*(_dev(t) for t in T), d_val, Gv, _dev(arg), k=k, n=FAR_N, m=m,
                                 lddc=g.ld if which == "dC" else FAR_N, dB=Dv,
                                 lddb=g.ld if which == "dB" else FAR_N, handle=h)
            torch.cuda.synchronize()
            got = far(which) if which == "dB" else _np(Dv).reshape(k, FAR_N)
            if which == "dC":
                far.unchanged("dC")
            assert rc.same_bits(got, dB), which


def test_far_arg_in_the_backward(device, arena):
    """The backward reads arg as well: arg at the far geometry, dC and dB compact."""
    ops = _ops()
    g = fc.F32
    m, k, rp, ci, val, B, C, arg, dC, T, dB = _far_problem("m", 6)
    far = arena.place(arg, g.ld)
    with _handle() as h:
        got = ops.csrmm_reduce_bwd(*(_dev(t) for t in T), _dev(val), _dev(dC), far.view, k=k,
                                   n=FAR_N, m=m, ldarg=g.ld, handle=h)
        torch.cuda.synchronize()
        far.unchanged("arg")
        assert rc.same_bits(_np(got), dB)


# ------------------------------------------------------------------ kernel coverage
def test_kernel_coverage(device):
    """One launch per call, and the union over the aligned widths of the three lane widths,
    forward and backward, is every kernel reduce_kernels.hip ships: none unlaunched, none
    unknown."""
    ops = _ops()
    shipped = {kernel_keys.launch_key(k) for k in kernel_keys.shipped_kernels(("reduce_kernels",))}
    print(f"reduce_kernels.hip ships {len(shipped)} kernels")
    seen = set()
    pat = "lens"
    m, k, rp, ci = rc.pattern(pat)
    trp, tci, perm = rc.host_transpose(pat)
    with _handle() as h:
        for n, pad in ((256, 0), (128, 0), (64, 0), (256, 3)):
            val, B = rc.values(pat, "generic", "max", n)
            Bv, _ = _frame(B, pad, 0)
            Cv, _ = _frame(np.zeros((m, n), np.float32), pad, 0)
            Av, _ = _frame(np.zeros((m, n), np.int32), pad, 0)
            with h.launch_record() as rec:
                ops.csrmm_reduce(_dev(rp), _dev(ci), _dev(val), Bv, m=m, n=n, k=k, ldb=n + pad,
                                 C=Cv, ldc=n + pad, arg=Av, ldarg=n + pad, handle=h)
            assert len(rec) == 1, (n, pad, rec)
            seen.update(rec)
            Dv, _ = _frame(np.zeros((k, n), np.float32), pad, 0)
            with h.launch_record() as rec:
                ops.csrmm_reduce_bwd(_dev(trp), _dev(tci), _dev(perm), _dev(val), Cv, Av, k=k, n=n,
                                     m=m, lddc=n + pad, ldarg=n + pad, dB=Dv, lddb=n + pad,
                                     handle=h)
            assert len(rec) == 1, (n, pad, rec)
            seen.update(rec)
    assert seen == shipped, (f"never launched: {sorted(shipped - seen)}; "
                             f"unknown: {sorted(seen - shipped)}")
    assert len(shipped) == 6
