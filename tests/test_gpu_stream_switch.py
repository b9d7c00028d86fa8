"""A handle whose stream changes: the new stream runs behind what the handle queued on
the old one (include/spmm_hip.h, "Streams").

A handle's buffers carry one call's state while its kernels run: the CSR merge-path
kernels park the pieces of every split row in ws and count arrivals in tickets, column-major
B and C are staged in ws, the BSR segment lists and partial tiles live in order and
scratch. Two calls of one handle whose kernels overlap on the device share all of that,
and only true overlap shows it: a split row is then "complete" when half of each call's
pieces have arrived. tests/test_gpu_handle_reuse.py keeps every sequence on one stream;
here the stream changes between calls, in each way it can:

  set_stream        Handle.set_stream on an explicit handle, step a of the reuse file
                    (the hub matrix, n = 256, column-major B and C)
  csrmm             ops.csrmm without handle= (step a again) under two torch.cuda.stream
                    blocks: ops.default_handle() follows torch's current stream
  gespmm_csrmm      the fp32 drop-in on the hub matrix at n = 64 (step b's operands): the
                    library's own default handle takes the stream argument
  gespmm_csrmm_f16  the fp16 drop-in, step l's operands (n = 128)
  csrmm_f16         step l on an explicit handle (the overlap test)
  bsrmm             step d (REUSE_SEG_SHAPE) on an explicit handle (the ordering probe only:
                    segment lists in order, partial tiles in scratch)

The fp64 drop-in (spmm_gespmm_csrmm_f64) keeps nothing in the handle (its kernel uses
no handle buffer), so it is held to its results only, between two fp32 drop-in calls on
another stream.

No tolerance: every entry here is bit-reproducible, and every result is
compared bit for bit with the same call on a handle created for it alone, on the first
operand set (the reuse file's) and on a second one of the same shapes
(helpers.graph_replay_variant). Each of those fresh results is held once to its oracle by
the step's check_x, so that two equal wrong answers cannot pass. A drop-in cannot be given
a handle: its fresh result is spmm_csrmm_ex_* with the same operands (alpha = 1, beta = 0,
row-major), whose bits it shares by design (the association is the row's, not the grid's).

Not run, by design: a buffer growing right after a change of stream (on an incomplete
fix that frees memory under a queued kernel; the order comes before any growth, which
context.cpp's switch_stream and grow_buffer show by reading), a destroyed stream, two host
threads on one handle."""
from __future__ import annotations

import time
from ctypes import byref, c_void_p

import numpy as np
import pytest

import test_gpu_handle_reuse as R
from helpers import (REUSE_HUB_K, REUSE_HUB_M, TOL_F32, assert_normwise, graph_replay_variant,
                     oracle_csrmm_d, oracle_csrmm_f64)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GATE_CYCLES = 100_000_000  # test_config4_native_multi_orders_against_default_stream's: ~40-50 ms
CONTROL_DEADLINE_S = 5.0   # the control product alone takes far less than the gate
PAIRS = 16
_state: dict = {}


# ------------------------------------------------------------------- paths
def _prepare_g32(I, device, src=None):
    rp, ci, v = R._own(I, src, "csr")
    return R._bufs({"rp": rp, "ci": ci, "v": v, "B": R._own(I, src, "b_B")},
                   [R._nan(REUSE_HUB_M * 64, device).view(REUSE_HUB_M, 64)])


def _launch_g32(h, I, bufs):
    """h None: the drop-in on torch's current stream; else spmm_csrmm_ex_f32 on h."""
    x = bufs["in"]
    if h is None:
        R._ops().gespmm_csrmm(x["rp"], x["ci"], x["v"], x["B"], C=bufs["C"][0])
    else:
        R._ops().csrmm(x["rp"], x["ci"], x["v"], x["B"], m=REUSE_HUB_M, n=64, k=REUSE_HUB_K,
                       ldb=64, C=bufs["C"][0], ldc=64, handle=h)


def _check_g32(outs, I, oracle):
    ref, absd = oracle_csrmm_f64(oracle, REUSE_HUB_M, 64, *I["csr"], I["b_B"], 64, 0)
    assert_normwise(outs[0], ref, absd, TOL_F32, "gespmm_csrmm on the hub matrix")


def _launch_g16(h, I, bufs):
    x = bufs["in"]
    if h is None:
        R._ops().gespmm_csrmm_f16(x["rp"], x["ci"], x["v"], x["B"],
                                  C=bufs["C"][0].view(REUSE_HUB_M, 128))
    else:
        R.launch_l(h, I, bufs)


# name -> (prepare, launch, check, variant step, on the default handle)
PATHS = {
    "set_stream": (R.prepare_a, R.launch_a, R.check_a, "a", False),
    "csrmm": (R.prepare_a, R.launch_a, R.check_a, "a", True),  # launch_a(None, ...): no handle=
    "gespmm_csrmm": (_prepare_g32, _launch_g32, _check_g32, "b", True),
    "gespmm_csrmm_f16": (R.prepare_l, _launch_g16, R.check_l, "l", True),
    "csrmm_f16": (R.prepare_l, R.launch_l, R.check_l, "l", False),
    "bsrmm": (R.prepare_d, R.launch_d, R.check_d, "d", False),
}


def _sets(path):
    """The two operand sets of a path as prepare's src: None (the reuse file's own) and the
    variant of the same shapes."""
    if ("sets", path) not in _state:
        _state["sets", path] = (None, graph_replay_variant(PATHS[path][3], R._host_inputs()))
    return _state["sets", path]


def _fresh(path, which, device, oracle):
    """The path's product on operand set `which` on two handles created for it alone (the
    reuse file's own _fresh where it has one): equal bits, held to the oracle; once per
    (step, set)."""
    prepare, launch, check, step, _ = PATHS[path]
    key = ("fresh", step, which)
    if key not in _state:
        I, src = R._inputs(), _sets(path)[which]
        if which == 0 and step != "b":
            first, diff = R._fresh(step, device)
        else:
            outs = []
            for _ in range(2):
                h = R._ops().Handle()
                bufs = prepare(I, device, src)
                launch(h, I, bufs)
                outs.append(R._read_C(h, bufs))
                h.close()
            first, diff = outs[0], R._differs(outs[1], outs[0])
        check(first, {**I, **(src or {})}, oracle)
        assert diff is None, f"{path}: output {diff} differs between two fresh handles"
        _state[key] = first
    return _state[key]


def _fresh_differ(path, device, oracle):
    a, b = _fresh(path, 0, device, oracle), _fresh(path, 1, device, oracle)
    assert R._differs(a, b) is not None, f"{path}: the two operand sets give the same result"
    return a, b


def _with_C(base, count):
    """`count` views of prepared buffers that share the inputs and own a C each."""
    return [{**base, "C": [c.clone() for c in base["C0"]]} for _ in range(count)]


class _Driver:
    """One handle fed from several streams: on(s) makes s the handle's stream (set_stream
    on an explicit handle, the torch.cuda.stream block alone on a default handle)."""

    def __init__(self, path, first_stream):
        self.launch = PATHS[path][1]
        self.h = None if PATHS[path][4] else R._ops().Handle(stream=first_stream)

    def product(self, s, I, bufs):
        with torch.cuda.stream(s):
            if self.h is not None:
                self.h.set_stream(s)
            self.launch(self.h, I, bufs)

    def close(self, I, bufs):
        """Leave a default handle on the default stream (one more product there)."""
        if self.h is not None:
            self.h.close()
        else:
            self.product(torch.cuda.default_stream(), I, bufs)
            torch.cuda.synchronize()


def _bits_equal(bufs, fresh):
    return R._differs([c.cpu().numpy() for c in bufs["C"]], fresh) is None


# --------------------------------------------------------- a. the ordering probe
@pytest.mark.parametrize("path", ["set_stream", "csrmm", "gespmm_csrmm", "gespmm_csrmm_f16", "bsrmm"])
def test_new_stream_waits_for_the_old(oracle, device, path):
    """Product 1 sits behind a gate (a ~40-50 ms spin) on s1; the handle changes to s2 and
    queues product 2; a control, product 2 on a third stream with a handle of its own,
    finishes while the gate is still shut. Product 2 on s2 must not have: it is ordered
    behind product 1. The control shows that the probe can see a finished product, so no
    timing constant but the gate's is needed. Then both products carry the fresh bits."""
    prepare, launch, _, _, _ = PATHS[path]
    I = R._inputs()
    fresh1, fresh2 = _fresh_differ(path, device, oracle)
    set1, set2 = _sets(path)
    base1, base2 = prepare(I, device, set1), prepare(I, device, set2)
    warm, b1 = _with_C(base1, 2)
    b2, bc, cwarm = _with_C(base2, 3)
    s1, s2, s3 = (torch.cuda.Stream() for _ in range(3))
    gate_done, e2, e_ctrl = (torch.cuda.Event() for _ in range(3))
    torch.cuda.synchronize()
    d = _Driver(path, s1)
    hc = R._ops().Handle(stream=s3)
    try:
        # 1. both handles at their full size before anything is gated
        d.product(s1, I, warm)
        with torch.cuda.stream(s3):
            launch(hc, I, cwarm)
        torch.cuda.synchronize()
        # 2. - 4.
        with torch.cuda.stream(s1):
            torch.cuda._sleep(GATE_CYCLES)
            gate_done.record()
        d.product(s1, I, b1)
        # 5.
        d.product(s2, I, b2)
        e2.record(s2)
        # 6.
        with torch.cuda.stream(s3):
            launch(hc, I, bc)
            e_ctrl.record()
        deadline = time.monotonic() + CONTROL_DEADLINE_S
        while not e_ctrl.query():
            assert time.monotonic() < deadline, "the control product did not finish in 5 s"
        gate_open, two_done = gate_done.query(), e2.query()
        torch.cuda.synchronize()
        assert not gate_open, ("the gate had opened before the control product finished: the "
                               "probe proved nothing")
        assert not two_done, (f"{path}: the product queued after the change of stream finished "
                              "while the handle's earlier product was still held back")
        assert _bits_equal(bc, fresh2), "the control product"
        assert _bits_equal(b1, fresh1), f"{path}: product 1 (operand set 1, the old stream)"
        assert _bits_equal(b2, fresh2), f"{path}: product 2 (operand set 2, the new stream)"
    finally:
        torch.cuda.synchronize()
        hc.close()
        d.close(I, warm)


def test_f64_dropin_between_streams(oracle, device):
    """spmm_gespmm_csrmm_f64 uses no handle buffer, so no probe: an fp32 drop-in product on
    s1, the fp64 drop-in on s2 (it borrows the default handle and gives it back), the fp32
    one on s1 again; all three are held to their results."""
    ops = R._ops()
    I = R._inputs()
    fresh32 = _fresh("gespmm_csrmm", 0, device, oracle)
    rp, ci, v = I["c64"]
    B = np.ascontiguousarray(I["c64_Bt"].T)  # 389 x 70, row-major
    want = oracle_csrmm_d(oracle, 517, 70, rp, ci, v, B, 70, 0).reshape(517, 70)
    drp, dci, dv, dB = R._dev(rp, ci, v, B)
    C64 = torch.full((517, 70), float("nan"), dtype=torch.float64, device=device)
    first, second = _with_C(_prepare_g32(I, device), 2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    d = _Driver("gespmm_csrmm", s1)
    try:
        d.product(s1, I, first)
        with torch.cuda.stream(s2):
            ops.gespmm_csrmm(drp, dci, dv, dB, C=C64)
        d.product(s1, I, second)
        torch.cuda.synchronize()
        assert np.array_equal(C64.cpu().numpy(), want), "the fp64 drop-in on the side stream"
        assert _bits_equal(first, fresh32) and _bits_equal(second, fresh32)
    finally:
        d.close(I, first)


# ------------------------------------------------------------------ b. overlap
@pytest.mark.parametrize("path", ["set_stream", "csrmm_f16", "gespmm_csrmm"])
def test_alternating_streams_keep_every_product(oracle, device, path):
    """Two streams released through one gate, one handle alternating between them for 16
    pairs of products (operand set 1 on s1, set 2 on s2, a C per call): without the order
    the launches of neighbouring calls overlap and split rows are completed from a mix of
    both calls' pieces. Every C carries the fresh bits of its operand set, and so does one
    more product after a synchronise: the tickets are back at rest."""
    prepare = PATHS[path][0]
    I = R._inputs()
    fresh = _fresh_differ(path, device, oracle)
    set1, set2 = _sets(path)
    base1, base2 = prepare(I, device, set1), prepare(I, device, set2)
    runs1, runs2 = _with_C(base1, PAIRS + 2), _with_C(base2, PAIRS)
    warm, last = runs1.pop(), runs1.pop()
    s1, s2, sg = (torch.cuda.Stream() for _ in range(3))
    opened = torch.cuda.Event()
    torch.cuda.synchronize()
    d = _Driver(path, s1)
    try:
        d.product(s1, I, warm)
        torch.cuda.synchronize()
        with torch.cuda.stream(sg):
            torch.cuda._sleep(GATE_CYCLES)
            opened.record()
        s1.wait_event(opened)
        s2.wait_event(opened)
        for b1, b2 in zip(runs1, runs2):
            d.product(s1, I, b1)
            d.product(s2, I, b2)
        torch.cuda.synchronize()
        bad = [f"call {2 * i + j + 1} (operand set {j + 1})"
               for i, pair in enumerate(zip(runs1, runs2)) for j, b in enumerate(pair)
               if not _bits_equal(b, fresh[j])]
        print(f"{path}: {len(bad)} of {2 * PAIRS} outputs differ from the fresh handle's")
        d.product(s1, I, last)
        torch.cuda.synchronize()
        assert not bad, f"{path}: {len(bad)} of {2 * PAIRS} outputs differ: " + ", ".join(bad)
        assert _bits_equal(last, fresh[0]), f"{path}: one more product after the synchronise"
    finally:
        torch.cuda.synchronize()
        d.close(I, warm)


# ------------------------------------------------------------------ c. capture
def _handle_stream(h):
    p = c_void_p()
    from spmm_hip._lib import check, lib
    check(lib().spmm_get_stream(h.raw, byref(p)), "spmm_get_stream")
    return p.value or 0


def test_switch_under_capture_is_refused(oracle, device):
    """A handle with a product queued on s1 cannot be moved to s2 while s2 is being
    captured: SPMM_STATUS_NOT_SUPPORTED before anything is recorded or waited for, the
    handle keeps s1, the capture (which holds one torch op) ends cleanly and replays it,
    and the handle then runs the step eagerly with the fresh bits. The same with s1
    capturing and s2 not."""
    from spmm_hip._lib import NOT_SUPPORTED, SpmmError
    I = R._inputs()
    fresh1, _ = _fresh_differ("set_stream", device, oracle)
    queued, after_new, after_old = _with_C(R.prepare_a(I, device), 3)
    scratch = torch.zeros(16, device=device)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    h = R._ops().Handle(stream=s1)
    graphs = []
    try:
        R.launch_a(h, I, queued)
        for capturing, runs in ((s2, after_new), (s1, after_old)):
            other = s1 if capturing is s2 else s2
            if capturing is s1:  # the handle goes to s2 eagerly, then s1 is captured
                h.set_stream(s2)
            g = torch.cuda.CUDAGraph()
            graphs.append(g)
            with torch.cuda.graph(g, stream=capturing):
                scratch.add_(1.0)
                with pytest.raises(SpmmError) as err:
                    h.set_stream(capturing)
            assert err.value.status == NOT_SUPPORTED
            assert _handle_stream(h) == other.cuda_stream and h.stream is other
            g.replay()  # the torch op alone
            torch.cuda.synchronize()
            R.launch_a(h, I, runs)  # eagerly, on the stream the handle kept
            torch.cuda.synchronize()
            assert _bits_equal(runs, fresh1), "step a after the refused change of stream"
        assert scratch.cpu().tolist() == [2.0] * 16
        assert _bits_equal(queued, fresh1)
    finally:
        torch.cuda.synchronize()
        for g in graphs:
            g.reset()
        h.close()


def test_same_stream_under_capture_is_a_no_op(oracle, device):
    """spmm_set_stream with the stream the handle already has returns 0 inside a capture
    of that stream, and the replay of the product captured after it equals the eager
    call (tests/test_gpu_graph_replay.py relies on this throughout)."""
    from spmm_hip._lib import lib
    I = R._inputs()
    fresh1, _ = _fresh_differ("set_stream", device, oracle)
    warm, run = _with_C(R.prepare_a(I, device), 2)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        h = R._ops().Handle(stream=s)
        try:
            R.launch_a(h, I, warm)
            s.synchronize()
            with torch.cuda.graph(g, stream=s):
                status = lib().spmm_set_stream(h.raw, c_void_p(s.cuda_stream))
                R.launch_a(h, I, run)
            assert status == 0 and _handle_stream(h) == s.cuda_stream
            g.replay()
            s.synchronize()
            assert _bits_equal(run, fresh1), "the replay after set_stream on the handle's own stream"
        finally:
            s.synchronize()
            g.reset()
            h.close()
