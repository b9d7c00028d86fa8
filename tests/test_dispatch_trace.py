"""Which kernel instantiation, grid and arguments each launcher of csr_kernels.hip and
bsr_kernels.hip reaches, pinned on the host ("Where dispatch lives").

bin/dispatch_trace links host-only objects of the two files in which every launch is a
line of text (csrc/dispatch_trace.hpp) and calls each spmm::launch_* over a grid of
arguments (drivers/dispatch_trace.cpp). Its output must equal
tests/golden/dispatch_trace.txt, recorded before the launch macros were replaced by the
typed dispatcher (csrc/dispatch.hpp): a launcher change that alters a kernel choice, a
grid or an argument shows here, without a GPU. To accept an intended change, rerun the
program into the golden file and review the diff.

Cost: when bin/dispatch_trace is missing, the host-only build of its three objects took
36 s one after the other and 22 s with three jobs; the program itself runs in 0.04 s and
the three tests in 0.3 s.
"""
from __future__ import annotations

import os
import re
import subprocess

import pytest

from kernel_keys import UNREACHABLE, kernel_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "spmm-denseblock_amd")
EXE = os.path.join(PKG, "bin", "dispatch_trace")
GOLDEN = os.path.join(ROOT, "tests", "golden", "dispatch_trace.txt")
ASM = [os.path.join(PKG, "build", f"{k}-hip-amdgcn-amd-amdhsa-gfx950.s")
       for k in ("csr_kernels", "bsr_kernels")]

@pytest.fixture(scope="module")
def trace() -> str:
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", PKG, "-j3", "bin/dispatch_trace"], check=True,
                       capture_output=True)
    return subprocess.run([EXE], check=True, capture_output=True, text=True).stdout


def test_trace_matches_golden(trace):
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    got = trace.splitlines()
    diff = [(i + 1, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not diff, "first differing line %d:\n  golden: %s\n  now:    %s" % diff[0]
    assert len(got) == len(want), f"{len(got)} lines, golden has {len(want)}"


def test_kernel_key():
    assert kernel_key("_ZN12_GLOBAL__N_114hot_tag_kernelExPKiiiPKjS3_Pi") == \
        "_ZN12_GLOBAL__N_114hot_tag_kernelE"
    assert kernel_key("_ZN12_GLOBAL__N_15CsrMpIDF16_E20csr_mergepath_kernelILi4ELb1ELi0EEEviiPKi") == \
        "_ZN12_GLOBAL__N_15CsrMpIDF16_E20csr_mergepath_kernelILi4ELb1ELi0EEE"
    assert kernel_key("_ZN12_GLOBAL__N_115bsr16_cm_kernelIfLb1ELi64EEEviiPKi") == \
        "_ZN12_GLOBAL__N_115bsr16_cm_kernelIfLb1ELi64EEE"


def test_every_shipped_kernel_is_reached(trace):
    """Every .amdhsa_kernel of the release csr_kernels / bsr_kernels assembly (the
    compiler's record of what ships) occurs in some tag of the trace."""
    if not all(os.path.exists(p) for p in ASM):
        subprocess.run(["make", "-C", PKG, "lib"], check=True, capture_output=True)
    tags = {ln[2:] for ln in trace.splitlines() if ln.startswith("@ ")}
    blob = "\n".join(tags)
    kernels = []
    for p in ASM:
        with open(p) as f:
            kernels += re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", f.read(), re.M)
    assert len(kernels) == len(set(kernels)) and len(kernels) == 167, len(kernels)
    keys = {k: kernel_key(k) for k in kernels}
    assert len(set(keys.values())) == len(kernels), "two kernels share a name and arguments"
    reached = {k for k in kernels if keys[k] in blob}
    listed = set()
    for pat, count, why in UNREACHABLE:
        named = {k for k in kernels if re.search(pat, keys[k])}
        assert len(named) == count, f"{why}: names {len(named)} kernels, expected {count}"
        assert not named & reached, f"{why}: listed as unreachable but reached: {named & reached}"
        listed |= named
    missing = [k for k in kernels if k not in reached and k not in listed]
    assert not missing, "no argument tuple of the trace reaches:\n" + "\n".join(missing)
