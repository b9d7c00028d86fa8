"""The host forms, converters, reorderers, generators and loaders of csrc/prep.cpp,
host_data.cpp, host_io.cpp and reorder.cpp under AddressSanitizer + UndefinedBehaviorSanitizer
(bin/host_asan) and ThreadSanitizer (bin/host_tsan): DESIGN.md §6, "What the sanitised driver
sees".

The Python host tests call these entries through ctypes on numpy arrays, which sit inside the
Python heap: a host form that reads the padding columns behind a row, one element before an
offset base or val[nnz] of a view returns the same bits there. drivers/host_sanitize.cpp is a
stand-alone program that gives every operand its own exact-size allocation, poisons what the
contract says is never touched, runs the refusals on fully poisoned outputs and runs every
entry with worker threads at 1 and at 7 workers (memcmp-equal results). Here each group of
its cases runs as a fresh process per binary; the run must exit 0, report nothing, and print
exactly the case names listed below, so a case that silently stops running is noticed.

Cost, measured with two build jobs: both binaries build in 23 to 25 s (guard 900 s); the
slowest runs are `forms` (6 to 8 s under ASan, 11 to 16 s under TSan) and `threads` (3 s and
10 to 13 s), every other run is under a second (guard 600 s each). The guards are for hangs
only.
"""
from __future__ import annotations

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "spmm-denseblock_amd")
BINARIES = {"host_asan": ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"],
            "host_tsan": ["-fsanitize=thread", "-static-libtsan"]}
BUILD_GUARD_S, RUN_GUARD_S = 900, 600
REPORTS = ("AddressSanitizer", "LeakSanitizer", "runtime error:", "ThreadSanitizer")

OPS = ["sddmm", "softmax_fwd", "softmax_bwd", "sddmm_heads_f32", "softmax_heads_fwd",
       "softmax_heads_bwd", "csrmm_heads_f32", "sddmm_heads_f16", "sddmm_heads_bf16",
       "csrmm_heads_f16", "csrmm_heads_bf16", "reduce_fwd", "reduce_bwd", "csr2csc"]
PATTERNS = ["empty_rows", "m0", "nnz0", "softmax_lengths", "reduce_lengths"]
CASES = {
    "forms": [f"{op}.{p}" for op in OPS for p in PATTERNS],
    "convert": ["convert.csr2bsr2csr", "convert.csr2bsr_empty", "convert.calculate_nnzb",
                "convert.partition_rows", "convert.divide", "convert.hybrid_plan"],
    "reorder": ["reorder.degree", "reorder.bfs", "reorder.rcm", "reorder.permute_csr",
                "reorder.metrics_heatmap", "reorder.files"],
    "generators": ["gen.random_array", "gen.random_csr", "gen.random_bsr", "gen.powerlaw",
                   "gen.community"],
    "threads": [f"threads.{op}" for op in OPS] + [
        "threads.csr2bsr", "threads.divide", "threads.hybrid_plan", "threads.reorder_degree",
        "threads.reorder_bfs", "threads.reorder_rcm", "threads.permute_csr",
        "threads.block_metrics", "threads.text_csr", "threads.edge_list", "threads.binary_csr",
        "threads.gen_powerlaw", "threads.gen_community", "threads.shared_generator"],
    "refusals": ["refuse.sddmm", "refuse.softmax", "refuse.sddmm_heads", "refuse.csrmm_heads",
                 "refuse.reduce_fwd", "refuse.reduce_bwd", "refuse.csr2csc", "refuse.reorder"],
    "loaders": ["loaders.text_round_trip", "loaders.edge_list", "loaders.binary_round_trip",
                "loaders.cached", "loaders.malformed_graph", "loaders.malformed_csr",
                "loaders.malformed_csrbin", "loaders.arguments"],
}


def _static_runtimes_missing(tmp) -> str | None:
    """Why g++ cannot link an empty main against the static sanitizer runtimes, or None."""
    src = os.path.join(tmp, "empty.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    for name, flags in BINARIES.items():
        try:
            r = subprocess.run(["g++", *flags, "-o", os.path.join(tmp, "empty_" + name), src],
                               capture_output=True, text=True, timeout=BUILD_GUARD_S)
        except FileNotFoundError:
            return "no g++ on this machine"
        if r.returncode != 0:
            return f"g++ cannot link {' '.join(flags)}: {r.stderr.strip().splitlines()[-1:]}"
    return None


@pytest.fixture(scope="module")
def binaries(tmp_path_factory):
    why = _static_runtimes_missing(str(tmp_path_factory.mktemp("san_probe")))
    if why:
        pytest.skip(why)
    # every time: make is incremental, and a stale binary must not hide a regression
    r = subprocess.run(["make", "-C", PKG, "-j2", *("bin/" + b for b in BINARIES)],
                       capture_output=True, text=True, timeout=BUILD_GUARD_S)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return {b: os.path.join(PKG, "bin", b) for b in BINARIES}


@pytest.mark.parametrize("group", list(CASES))
@pytest.mark.parametrize("binary", list(BINARIES))
def test_group_is_clean(binaries, binary, group, tmp_path):
    r = subprocess.run([binaries[binary], group, str(tmp_path)], capture_output=True, text=True,
                       timeout=RUN_GUARD_S)
    ran = [ln[3:] for ln in r.stdout.splitlines() if ln.startswith("ok ")]
    assert r.returncode == 0, f"exit {r.returncode} after {ran[-1:]}:\n{r.stderr[-6000:]}"
    for word in REPORTS:
        assert word not in r.stderr, r.stderr[-6000:]
    assert ran == CASES[group]
