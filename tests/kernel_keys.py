"""The shipped kernels by name: the `.amdhsa_kernel` symbols of the release library's seven
device assembly files, the key that identifies one in a dispatch trace or a handle's launch
record, and the kernels no argument tuple of a release build reaches.

Shared by tests/test_dispatch_trace.py (which argument tuple reaches which instantiation,
on the host), tests/test_kernel_cases.py (the case table names every shipped kernel) and
tests/test_gpu_kernel_coverage.py (every one of them runs on the GPU under an oracle)."""
from __future__ import annotations

import os
import re
import subprocess

from spmm_hip._lib import kernel_key, launch_key  # noqa: F401  (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "spmm-denseblock_amd")
HIP_FILES = ("csr_kernels", "bsr_kernels", "convert_kernels", "f64_kernels", "group_kernels",
             "transpose_kernels", "sddmm_kernels")


def asm_path(name: str) -> str:
    return os.path.join(PKG, "build", f"{name}-hip-amdgcn-amd-amdhsa-gfx950.s")


# Kernels that ship but that no argument tuple of a release build reaches: (pattern over
# the kernel's name and template arguments, how many it names, the condition that keeps
# them out). Findings for a later change; nothing is dropped from the check silently.
# Empty today: the kernels only a TUNING build's overrides select (csr_group_kernel's L x PD
# cross product for SPMM_CSR_GROUP_PD, the column streams without nt A copies for
# SPMM_BSR_VARIANT 4516 / 6104) are instantiated in that build alone.
UNREACHABLE: list[tuple[str, int, str]] = []


def shipped_kernels(files=HIP_FILES) -> list[str]:
    """Every `.amdhsa_kernel` symbol of the release assembly of `files` (the compiler's
    record of what ships), building the library first when an assembly file is missing."""
    paths = [asm_path(f) for f in files]
    if not all(os.path.exists(p) for p in paths):
        subprocess.run(["make", "-C", PKG, "lib"], check=True, capture_output=True)
    kernels: list[str] = []
    for p in paths:
        with open(p) as f:
            kernels += re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", f.read(), re.M)
    return kernels


def unreachable_keys(keys) -> set[str]:
    return {k for k in keys for pat, _, _ in UNREACHABLE if re.search(pat, k)}
