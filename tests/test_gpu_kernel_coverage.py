"""Every kernel instantiation a release build can reach runs on the GPU at least once under
an oracle check, and the test knows that it did.

Parametrised over tests/kernel_cases.py. Each case runs its public entry on a handle whose
launch record is on (spmm_set_launch_record: what the handle queued, by kernel), and is
checked twice: the record holds every kernel the case names (a missing one means the case no
longer tests what it claims; others are reported, not failed), and the result matches a
reference that is not the code under test (the case's runner; frame guards included). The
last test asserts that the kernels recorded over the module, each in a case where it does
the arithmetic (not idle behind a device-side gate: kernel_cases' `idle`), are the shipped
set less the unreachable lists, and prints what remains.
"""
from __future__ import annotations

import re

import pytest

import kernel_cases as kc
from kernel_keys import launch_key, shipped_kernels, unreachable_keys

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_recorded: set = set()
_worked: set = set()  # recorded in a case that expects the kernel and does not mark it idle
_ran: set = set()


@pytest.fixture(scope="module")
def keys():
    return [launch_key(s) for s in shipped_kernels()]


@pytest.fixture(scope="module")
def handle(device):
    from spmm_hip import ops
    h = ops.Handle()
    yield h
    h.close()


@pytest.mark.parametrize("case", kc.CASES, ids=repr)
def test_case(case, oracle, handle, keys):
    handle.set_stream(torch.cuda.current_stream())
    handle.set_bsr_options(0)
    handle.set_hybrid_options(0)
    handle.set_csr_options(1)
    rec = kc.RUNNERS[case.entry](case, oracle, handle)
    _ran.add(case.id)
    _recorded.update(rec)
    _worked.update(set(rec) & kc.covering_keys(case, keys))
    assert set(rec) <= set(keys), f"recorded kernels that do not ship: {set(rec) - set(keys)}"
    want = kc.expected_keys(case, keys)
    missing = sorted(want - set(rec))
    extra = sorted(set(rec) - want)
    assert not missing, (f"{case.id}: the launch record misses {missing}; recorded besides the "
                         f"expected kernels: {extra}")


def test_recording_off_records_nothing(device, oracle):
    """Off by default, and off again after the context manager: a product leaves the
    record as it was."""
    from ctypes import byref, c_char_p, c_int
    from spmm_hip import ops
    from spmm_hip._lib import lib
    h = ops.Handle()
    case = next(c for c in kc.CASES if c.entry == "csrmm")
    rec = kc.run_csr(case, oracle, h)
    assert rec
    h.set_csr_options(1)
    a = torch.zeros(8, dtype=torch.int32, device=device)
    ops.coo2csr(a, 4, handle=h)
    buf, cnt = (c_char_p * 64)(), c_int(-1)
    assert lib().spmm_get_launch_record(h.raw, buf, 64, byref(cnt)) == 0
    assert cnt.value == len(rec), "a launch was recorded with recording off"
    assert lib().spmm_set_launch_record(h.raw, 1) == 0  # on: clears
    assert lib().spmm_get_launch_record(h.raw, buf, 64, byref(cnt)) == 0 and cnt.value == 0
    h.close()


def test_every_reachable_kernel_ran(keys):
    """The union of the records equals the shipped set less the unreachable lists."""
    assert _ran == {c.id for c in kc.CASES}, "run the whole module: this test sums it up"
    unreachable = unreachable_keys(keys) | {k for k in keys for p, _, _ in kc.UNREACHABLE_OTHER
                                            if re.search(p, k)}
    left = sorted(set(keys) - unreachable - _worked)
    print(f"{len(_recorded)} of {len(keys)} shipped kernels recorded, {len(_worked)} of them in a "
          f"case whose result depends on them, {len(unreachable)} listed unreachable, "
          f"{len(left)} uncovered")
    for k in left:
        print("  uncovered:", k)
    assert not left, "never launched under a case:\n" + "\n".join(left)
    assert not _recorded & unreachable, sorted(_recorded & unreachable)
