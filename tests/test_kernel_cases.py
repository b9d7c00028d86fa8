"""The kernel coverage table (tests/kernel_cases.py) against what ships, on the host.

Every `.amdhsa_kernel` of the release library's seven device assembly files is named by a
case of the table or by an unreachable list with its reason, never by both; every pattern
of a case names a shipped kernel; and where a case goes through the CSR / BSR launchers,
bin/dispatch_trace (host-only objects, "cases" mode) is asked which kernels those launchers
pick for the case's arguments: the expectation must be exactly those kernels plus the ones
the entry layer launches itself. A wrong expectation fails here, not on the GPU.
"""
from __future__ import annotations

import os
import re
import subprocess

import pytest

import kernel_cases as kc
from kernel_keys import (HIP_FILES, PKG, UNREACHABLE, launch_key, shipped_kernels,
                         unreachable_keys)

EXE = os.path.join(PKG, "bin", "dispatch_trace")


@pytest.fixture(scope="module")
def keys():
    syms = shipped_kernels()
    ks = [launch_key(s) for s in syms]
    assert len(syms) == len(set(syms)) and len(set(ks)) == len(syms), "keys are not unique"
    return ks


def test_keys_are_one_to_one_with_symbols(keys):
    """253 kernels: the 167 of csr_kernels / bsr_kernels and the 86 of the other five
    files, each with a key of its own (two files define a col_count_kernel)."""
    assert len(keys) == 253
    assert sum("16col_count_kernelE" in k for k in keys) == 2


def test_case_ids_and_entries():
    ids = [c.id for c in kc.CASES]
    assert len(ids) == len(set(ids))
    assert all(c.entry in kc.RUNNERS and c.expect for c in kc.CASES)


def test_every_pattern_names_a_shipped_kernel(keys):
    bad = [(c.id, p) for c in kc.CASES for p in c.expect
           if not any(re.search(p, k) for k in keys)]
    assert not bad, bad


def test_unreachable_lists(keys):
    """The lists hold what they say (nothing today: TUNING-only kernels no longer ship):
    kernels of the traced files that no trace tuple reaches (tests/test_dispatch_trace.py
    checks that) and kernels of the other files that kernel_cases.UNREACHABLE_OTHER proves
    out of reach."""
    assert sum(n for _, n, _ in UNREACHABLE) == 0
    for pat, count, why in UNREACHABLE + kc.UNREACHABLE_OTHER:
        assert sum(bool(re.search(pat, k)) for k in keys) == count, why


def test_every_shipped_kernel_is_named_once(keys):
    unreachable = unreachable_keys(keys) | {k for k in keys for p, _, _ in kc.UNREACHABLE_OTHER
                                            if re.search(p, k)}
    # named by a case in which the kernel does the arithmetic (not idle behind a device gate)
    named = set().union(*(kc.covering_keys(c, keys) for c in kc.CASES))
    both = sorted(set().union(*(kc.expected_keys(c, keys) for c in kc.CASES)) & unreachable)
    assert not both, "listed unreachable and expected by a case:\n" + "\n".join(both)
    missing = [k for k in keys if k not in named and k not in unreachable]
    assert not missing, "no case names:\n" + "\n".join(missing)


def test_gated_kernels_are_marked_idle(keys):
    """A case cannot be the cover of a kernel whose device gate it closes: where the panel
    probe goes out (fully dense blocks: the probe picks the panel kernel) every column
    stream of the case is idle, and a case on SPMM_BSR_SMALL_GROUPED states which of the
    pair does the work (small_path, asserted on the GPU) and marks the other idle."""
    for c in kc.CASES:
        exp = kc.expected_keys(c, keys)
        idle = exp - kc.covering_keys(c, keys)
        assert all(any(p == q for q in c.expect) for p in c.idle), c.id
        if any("panel_probe_kernel" in k for k in exp):
            assert {k for k in exp if "bsr32_f32_cs2_kernel" in k} <= idle, c.id
        if any("bsr_small_grp_kernel" in k for k in exp):
            path = c.args["small_path"]
            gated = "16bsr_small_kernelI" if path == 1 else "bsr_small_grp_kernel"
            assert path in (1, 2) and {k for k in exp if gated in k} <= idle, c.id


def test_expectations_match_the_dispatch_trace(keys):
    """For the cases of the traced launchers: the kernels the launchers pick for the case's
    arguments (as csrc/api.cpp passes them on, kernel_cases.api_launches) plus the entry
    layer's own are exactly the kernels the case expects."""
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", PKG, "-j3", "bin/dispatch_trace"], check=True,
                       capture_output=True)
    traced = [(c, kc.api_launches(c)) for c in kc.CASES]
    traced = [(c, la) for c, la in traced if la is not None]
    assert len(traced) >= 100
    lines = [ln for _, (ls, _) in traced for ln in ls]
    out = subprocess.run([EXE, "cases"], input="\n".join(lines) + "\n", check=True,
                         capture_output=True, text=True).stdout.split("\n")
    i = 0
    for c, (ls, aux) in traced:
        want = {launch_key(t) for ln in out[i:i + len(ls)] for t in ln.split()}
        i += len(ls)
        for p in aux:
            want |= {k for k in keys if re.search(p, k)}
        got = kc.expected_keys(c, keys)
        assert got == want, (f"{c.id}: expects {sorted(got - want)} that the launchers do not "
                             f"pick, misses {sorted(want - got)}")


def test_wide_ldb_cases_cover_the_64_bit_offset_streams(keys):
    """All 12 O32 = false instantiations of bsr32_f32_cs2_kernel (plain, analysed and SUB,
    each by CR x C64) are expected by a case with ldb = 2^24 whose blocks reach B rows past
    2^31 bytes."""
    o32_false = {k for k in keys if re.search(r"20bsr32_f32_cs2_kernelILb[01]ELb0E", k)}
    assert len(o32_false) == 12
    seen = set()
    for c in kc.CASES:
        if c.args.get("shape") != "wide":
            continue
        mb, kb, rp, ci, _ = kc.bsr_matrix(c.args)
        assert (int(ci.max()) * c.args["bs"] + c.args["bs"] - 1) * kc.WIDE_LDB * 4 >= 1 << 31
        seen |= kc.expected_keys(c, keys) & o32_false
    assert seen == o32_false, sorted(o32_false - seen)


def test_all_seven_files_are_read():
    assert len(HIP_FILES) == 7
