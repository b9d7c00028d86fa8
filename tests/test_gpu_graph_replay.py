"""Captured graphs of the product entries, replayed, against eager calls.

DESIGN.md §2: "The steady state allocates nothing, launches only kernels and async
copies, and is graph-capture safe." The products carry device state from launch to
launch (split-row tickets that each launch returns to zero, probe sums and dirty flags
reset by a memset that must be a node of the graph, segment lists and block-row orders
rebuilt from rowptr on the device, staging areas that other entries reinterpret), and a
replay runs the same baked launches on the same handle buffers: possibly on new data at
the same addresses, with other entries in between.

The steps are tests/test_gpu_handle_reuse.py's, cut into prepare / launch / read; one
graph per step holds the product launches only:

  a, d, e, h, k, l   launch_x as it stands
  b                  the three launches under set_csr_waves_per_cu(32), (1), (0)
  c'                 csrmm_hot only; the tag comes from an eager csr_hot_analysis
  f'                 bs 8 and bs 2 under SPMM_BSR_SMALL_GROUPED, no path query
  g                  both hybrid forms
  i'                 GroupedBsr16.mm and GroupedBsr32.mm; the analyses are eager

Not captured, by design: the analyses and the converters (step j), which hand sizes back
to the host, and spmm_bsr_small_path, which reads the device.

Precondition of a capture (include/spmm_hip.h, "Graph capture"): the handle's buffers
already hold the call's largest request, since growing one synchronises, frees and
allocates. The module's handle therefore runs every step eagerly once before anything is
captured, on the side stream everything here runs on; afterwards nothing on it grows, so
the pointers baked into the graphs stay good. Every graph is dropped before the handle
is closed. A capture that would have to grow a buffer is refused with
SPMM_STATUS_NOT_SUPPORTED (the last test). What a later, larger eager call does to the
graphs of a handle (it frees what they point to) is documented and not run: it would be
a use after free on the device.

No tolerance of this file's own: replays are compared bit for bit with eager calls on
fresh handles, and those are held to the oracles by the steps' check_x (TOL_F32,
TOL_F16_ACC, exact for f and k). Where a step's control (two fresh handles agree) fails,
the replay is held to check_x instead, as the reuse sequences do. The graphs are linear
chains on one stream; no environment variable is set."""
from __future__ import annotations

import gc

import numpy as np
import pytest

import test_gpu_handle_reuse as R
from helpers import graph_replay_variant

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CAPTURED = "abcdefghikl"
BETA_STEPS = "aefgik"  # beta != 0: C is read by the product
# the products' C among run_x's outputs (the rest: c's tag, f's paths, i's analysis figures)
PRODUCT_OUTS = {"c": (1,), "f": (0, 2), "i": (0, 2)}
# a step's outputs as the C0 overrides of its prepare_x
AS_C0 = {"a": lambda o: {"a_C0": o[0].T}, "e": lambda o: {"seg_C0": o[0].T},
         "f": lambda o: {"small8_C0": o[0], "small2_C0": o[1]},
         "g": lambda o: {"hyb_C0c": o[0].T, "hyb_C0r": o[1]},
         "i": lambda o: {"g16_C0": o[0], "g32_C0": o[1]},
         "k": lambda o: {"c64_C0t": o[0], "b64_C0": o[1]}}


def _fn(kind, name):
    return getattr(R, f"{kind}_{name}")


def _before(name, h, I, bufs):
    """The eager part of a captured step: what hands sizes back to the host."""
    if name == "c":
        R.analyse_c(h, I, bufs)
    elif name == "i":
        for j in range(2):
            R.analyse_i(h, I, bufs, j)


def _launch(name, h, I, bufs):
    (R.launch_c_hot if name == "c" else _fn("launch", name))(h, I, bufs)


def _restore(bufs):
    """C back to its pristine contents, ordered on the current stream."""
    for C, C0 in zip(bufs["C"], bufs["C0"]):
        C.copy_(C0)


def _write(bufs, src):
    """src's inputs and pristine C over bufs', in place: the addresses stay."""
    for key, t in bufs["in"].items():
        t.copy_(src["in"][key])
    for C0, V0 in zip(bufs["C0"], src["C0"]):
        C0.copy_(V0)


def _products(name, full):
    idx = PRODUCT_OUTS.get(name, range(len(full)))
    return [full[i] for i in idx]


def _hold(name, got, want_full, control, Ix, oracle, what):
    """got (the products' C) carries the bits of want_full's products; a step whose
    control failed is held to its oracle, in want_full's format."""
    if control is not None:
        full = list(want_full)
        for g, i in zip(got, PRODUCT_OUTS.get(name, range(len(full)))):
            full[i] = g
        _fn("check", name)(full, Ix, oracle)
        return
    i = R._differs(got, _products(name, want_full))
    assert i is None, f"step {name}, {what}: output {i} differs from the eager call on a fresh handle"


def _eager(name, I, device, src):
    """run_x on a handle created for it (bound to the current stream)."""
    h = R._ops().Handle()
    try:
        return _fn("run", name)(h, I, device, src)
    finally:
        h.close()


@pytest.fixture(scope="module")
def env(oracle, device):
    I = R._inputs()
    for name in R.STEPS:
        R._fresh(name, device)  # the controls run on the default stream, before the rest
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graphs: list = []
    with torch.cuda.stream(s):
        h = R._ops().Handle(stream=s)
        for name in R.STEPS:  # every handle buffer at the module's largest request
            _fn("run", name)(h, I, device)
    s.synchronize()
    yield {"h": h, "s": s, "I": I, "graphs": graphs}
    # a graph holds pointers into the handle's buffers: all gone before the handle goes
    while graphs:
        graphs.pop().reset()
    gc.collect()
    s.synchronize()
    h.close()


@pytest.mark.parametrize("name", list(CAPTURED))
def test_replay_equals_eager(env, oracle, device, name):
    """One graph of the step's product launches on the warmed handle:
    1. the capture returns status 0 throughout;
    2. one replay gives the fresh handle's bits;
    3. three more replays with no synchronise between them (C restored from its device
       copy before each, on the stream) still do: tickets, flags and sums are back at
       rest after each; one further replay without restoring C, on a beta != 0 step,
       equals an eager call given the previous output as C0: C is read at replay time;
    4. after every other step has run eagerly on the same handle and stream, the same;
    5. with the variant operands written over the step's own inputs in place, the replay
       equals an eager call on a fresh handle over freshly uploaded variant operands
       (held to check_x on the variant), and with the original operands written back, the
       result of 2 again."""
    h, s, I = env["h"], env["s"], env["I"]
    fresh, control = R._fresh(name, device)
    read = _fn("read", name) if name != "c" else R._read_C
    with torch.cuda.stream(s):
        bufs = _fn("prepare", name)(I, device)
        _before(name, h, I, bufs)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        env["graphs"].append(g)
        try:
            # 1. ops.check raises on any status but 0
            try:
                with torch.cuda.graph(g, stream=s):
                    h.set_stream(s)
                    _launch(name, h, I, bufs)
            finally:
                h.set_stream(s)
            # 2.
            g.replay()
            first = read(h, bufs)
            _hold(name, first, fresh, control, I, oracle, "first replay")
            # 3.
            for _ in range(3):
                _restore(bufs)
                g.replay()
            again = read(h, bufs)
            _hold(name, again, fresh, control, I, oracle, "fourth replay in a row")
            if name in BETA_STEPS:
                g.replay()
                over = AS_C0[name](again)
                _hold(name, read(h, bufs), _eager(name, I, device, over), control, {**I, **over},
                      oracle, "replay on the previous output as C0")
            # 4.
            R._sequence([n for n in R.STEPS if n != name], h, device, oracle)
            _restore(bufs)
            g.replay()
            _hold(name, read(h, bufs), fresh, control, I, oracle, "replay after the other entries")
            # 5.
            var = graph_replay_variant(name, I)
            Iv = {**I, **var}
            want = _eager(name, I, device, var)
            _fn("check", name)(want, Iv, oracle)
            assert R._differs(_products(name, want), _products(name, fresh)) is not None
            vb = _fn("prepare", name)(I, device, var)
            saved = {"in": {key: t.clone() for key, t in bufs["in"].items()},
                     "C0": [t.clone() for t in bufs["C0"]]}
            _write(bufs, vb)
            _restore(bufs)
            g.replay()
            _hold(name, read(h, bufs), want, control, Iv, oracle, "replay on the variant operands")
            _write(bufs, saved)
            _restore(bufs)
            g.replay()
            back = read(h, bufs)
            _hold(name, back, fresh, control, I, oracle, "replay on the operands written back")
            if control is None:
                assert R._differs(back, first) is None
        finally:
            s.synchronize()
            env["graphs"].remove(g)
            g.reset()
            if name == "i":
                R.release_i(bufs)


def test_growth_under_capture_is_refused(oracle, device):
    """A handle with nothing sized cannot run step a under capture: the call is refused
    with SPMM_STATUS_NOT_SUPPORTED before anything is synchronised, freed or allocated
    (a status-code path: no launch is involved in the refusal), the capture, which also
    holds one torch op so that it is not empty, ends cleanly, and the same handle then
    runs the step eagerly with the fresh bits."""
    from spmm_hip._lib import NOT_SUPPORTED, SpmmError
    I = R._inputs()
    fresh, control = R._fresh("a", device)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        h = R._ops().Handle(stream=s)
        bufs = R.prepare_a(I, device)
        scratch = torch.zeros(16, device=device)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        try:
            try:
                with torch.cuda.graph(g, stream=s):
                    scratch.add_(1.0)
                    h.set_stream(s)
                    with pytest.raises(SpmmError) as err:
                        R.launch_a(h, I, bufs)
            finally:
                h.set_stream(s)
            assert err.value.status == NOT_SUPPORTED
            g.replay()  # the torch op alone: the refused call queued nothing
            s.synchronize()
            assert scratch.cpu().tolist() == [1.0] * 16
            assert np.array_equal(bufs["C"][0].cpu().numpy(), bufs["C0"][0].cpu().numpy())
            outs = R.run_a(h, I, device)
            if control is None:
                assert R._differs(outs, fresh) is None, "step a after the refused capture"
            else:
                R.check_a(outs, I, oracle)
        finally:
            s.synchronize()
            g.reset()
            h.close()
