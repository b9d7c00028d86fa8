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
UNREACHABLE = [
    # csr_group_kernel<NT, L, PD, HOT>: the launcher instantiates PD 1 / 2 / 4 at every L,
    # for a TUNING build's SPMM_CSR_GROUP_PD; a release build derives both from n
    # (n <= 16: L 2 / 4 with PD 1; n <= 32: L 8 with PD 2; else L 16 with PD 4)
    (r"16csr_group_kernelILb[01]ELi[24]ELi[24]ELb[01]EE", 12, "L 2 / 4 with PD 2 / 4"),
    (r"16csr_group_kernelILb[01]ELi8ELi[14]ELb[01]EE", 6, "L 8 with PD 1 / 4"),
    (r"16csr_group_kernelILb[01]ELi16ELi[12]ELb[01]EE", 6, "L 16 with PD 1 / 2"),
    # the column streams without nt A copies: SPMM_BSR_VARIANT 4516 / 6104, a TUNING
    # build's override (variant_override() is the constant -1 in a release build)
    (r"20bsr32_f32_cs2_kernelILb[01]ELi32ELi6ELi3ELb1ELb1ELb0ELb0ELb0ELb[01]EE", 4,
     "ANT = false: variant 4516 only"),
    (r"19bsr16_f16_cs_kernelILb[01]ELi2ELi4ELi0ELi48ELb0ELb1ELi256ELb0EE", 2,
     "ANT = false: variant 6104 only"),
]


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
