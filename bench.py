#!/usr/bin/env python3
"""bench.py — BASELINE.json headline: SpMM GFLOP/s (2*nnz*K/t) + achieved HBM
GB/s on ogbn-products at K = 128 (synthetic stand-in with the same n / nnz /
max degree: OGB data is not reachable offline).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload NAME]
    python bench.py --full ...        # + CPU baseline, side entries, kernel-timed roofline
    python bench.py --dump-outputs DIR ...   # the last timed step's C as DIR/C.npy
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N

A plain run sets up, warms up, times the steps and prints the line; whatever
else is measured beside the headline figure (the CPU baseline legs, the
hot-column / grouped / analysed side entries, BASELINE configs 3 and 5 beside
the N = 1 line, the event-timed kernel pass behind a CSR line's `roofline`)
runs with --full.

Workloads (BASELINE.json configs; the default is the metric's own config):
  products_csr       CSR x dense, ogbn-products stand-in, K=128   (metric; config 4 shape at N>1)
  products_csr_k256  same graph, K=256                            (config 4)
  arxiv_csr          ogbn-arxiv stand-in (169,343 / 1,166,243), K=128   (config 2)
  reddit_bsr32       community-ordered reddit stand-in, csr2bsr bs=32, K=128, fp32 MFMA (config 3)
  products_bsr16_f16 community-ordered products stand-in, bs=16, K=512, fp16 MFMA    (config 5)
  reddit_rcm_bsr32, products_rcm_bsr16_f16, products_rcm_bsr32
                     the same with the reorder step in the loop: node ids scrambled,
                     in-repo RCM (spmm_reorder_rcm), then csr2bsr

A step = one pass of the hot path over resident inputs. CSR: the merge-path
kernel + carry fix-up on this rank's rows. With no --workload the N = 1 run is
the metric's own workload (products_csr, K = 128) and an N > 1 launch runs
BASELINE config 4 as written (products_csr_k256, --scaling strong): the one
graph split nnz-balanced over the ranks, the chunked RCCL all-gather of C
inside every step, per-GPU kernel ms and collective ms reported beside the
step, and rank 0's 1-GPU time of the same product for the speed-up. GFLOP/s
normalises K, so the N = 1 headline and the N > 1 config-4 lines form one
series. --scaling weak keeps the weak-scaling form: each rank owns a
products-size row block of a world-times larger graph, B replicated, C
row-sharded, no collective in the step (the C all-gather is timed after the
loop as `exchange`). BSR: one bsrmm. Rank 0 prints ONE JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "spmm-denseblock_amd"))

import numpy as np  # noqa: E402

HBM_PEAK_GBPS = 8000.0    # MI355X_MICROARCH.md chip table (spec)
MFMA_PEAK_TFLOPS = {"fp32": 157.3, "fp16": 2500.0}  # dense (no sparsity)

WORKLOADS = {
    "products_csr": dict(kind="csr", n=2449029, nnz=61859140, max_deg=17481, K=128),
    "products_csr_k256": dict(kind="csr", n=2449029, nnz=61859140, max_deg=17481, K=256),
    # the headline product on hot-column cache hints (spmm_csr_hot_analysis once
    # per matrix, timed apart as analysis_ms; spmm_csrmm_hot_f32 in the step)
    "products_csr_hot": dict(kind="csr", n=2449029, nnz=61859140, max_deg=17481, K=128,
                             hot=True),
    "arxiv_csr": dict(kind="csr", n=169343, nnz=1166243, max_deg=13161, K=128),
    "reddit_bsr32": dict(kind="bsr", n=232965, avg_deg=670.0, cmin=512, cmax=2048, p_in=0.99,
                         bs=32, K=128, dtype="fp32"),
    "products_bsr16_f16": dict(kind="bsr", n=2449029, avg_deg=27.0, cmin=32, cmax=512,
                               p_in=0.97, bs=16, K=512, dtype="fp16"),
    # north_star's BSR target (>= 40 % fp32 MFMA, products, K=128) on the
    # community-ordered products stand-in
    "products_bsr32": dict(kind="bsr", n=2449029, avg_deg=27.0, cmin=32, cmax=512,
                           p_in=0.97, bs=32, K=128, dtype="fp32"),
    # the same products and reddit BSR products on the analysed column stream
    # (spmm_bsr32_analysis_f32 once per matrix, outside the timed region, like
    # cuSPARSE's SpMM preprocess; spmm_bsrmm_analysed_f32 timed)
    "products_bsr32_an": dict(kind="bsr", n=2449029, avg_deg=27.0, cmin=32, cmax=512,
                              p_in=0.97, bs=32, K=128, dtype="fp32", analysed=True),
    "reddit_bsr32_an": dict(kind="bsr", n=232965, avg_deg=670.0, cmin=512, cmax=2048,
                            p_in=0.99, bs=32, K=128, dtype="fp32", analysed=True),
    "products_bsr16_f16_an": dict(kind="bsr", n=2449029, avg_deg=27.0, cmin=32, cmax=512,
                                  p_in=0.97, bs=16, K=512, dtype="fp16", analysed=True),
    # config 5 on the grouped stream (spmm_bsr16_group_analysis_f16 once, groups of
    # `grouped` block rows sharing their B-row copies, "auto" = the library's choice
    # per matrix; spmm_bsrmm_grouped_f16 timed)
    "products_bsr16_f16_grp": dict(kind="bsr", n=2449029, avg_deg=27.0, cmin=32, cmax=512,
                                   p_in=0.97, bs=16, K=512, dtype="fp16", grouped="auto"),
    "products_rcm_bsr16_f16_grp": dict(kind="bsr", n=2449029, avg_deg=27.0, cmin=32, cmax=512,
                                       p_in=0.97, bs=16, K=512, dtype="fp16", reorder="rcm",
                                       grouped="auto"),
    # configs 3 and north_star's products bs 32 on the grouped bs 32 stream
    # (spmm_bsr32_group_analysis_f32 once; spmm_bsrmm_grouped_f32 timed)
    "reddit_bsr32_grp": dict(kind="bsr", n=232965, avg_deg=670.0, cmin=512, cmax=2048, p_in=0.99,
                             bs=32, K=128, dtype="fp32", grouped=2),
    "products_bsr32_grp": dict(kind="bsr", n=2449029, avg_deg=27.0, cmin=32, cmax=512,
                               p_in=0.97, bs=32, K=128, dtype="fp32", grouped=2),
    "products_hybrid32": dict(kind="hybrid", n=2449029, avg_deg=27.0, cmin=32, cmax=512,
                              p_in=0.97, bs=32, K=128, density="auto"),
    # §8f rank 2 in the loop: scrambled ids -> in-repo RCM -> divide + hybrid
    "reddit_rcm_hybrid32": dict(kind="hybrid", n=232965, avg_deg=670.0, cmin=512, cmax=2048,
                                p_in=0.99, bs=32, K=128, density="auto", reorder="rcm"),
    # configs 3 and 5 with the reorder step in the loop (reorder_graph.cc:26-49 ->
    # run_bsrmm.cu): the same stand-ins with node ids scrambled, then the in-repo
    # reorderer, then csr2bsr. The community-ordered workloads above are the
    # upper bound a perfect reorderer reaches.
    "reddit_rcm_bsr32": dict(kind="bsr", n=232965, avg_deg=670.0, cmin=512, cmax=2048,
                             p_in=0.99, bs=32, K=128, dtype="fp32", reorder="rcm"),
    "reddit_rcm_bsr32_an": dict(kind="bsr", n=232965, avg_deg=670.0, cmin=512, cmax=2048,
                                p_in=0.99, bs=32, K=128, dtype="fp32", reorder="rcm",
                                analysed=True),
    "products_rcm_bsr32_an": dict(kind="bsr", n=2449029, avg_deg=27.0, cmin=32, cmax=512,
                                  p_in=0.97, bs=32, K=128, dtype="fp32", reorder="rcm",
                                  analysed=True),
    "products_rcm_bsr16_f16_an": dict(kind="bsr", n=2449029, avg_deg=27.0, cmin=32, cmax=512,
                                      p_in=0.97, bs=16, K=512, dtype="fp16", reorder="rcm",
                                      analysed=True),
    "products_rcm_bsr16_f16": dict(kind="bsr", n=2449029, avg_deg=27.0, cmin=32, cmax=512,
                                   p_in=0.97, bs=16, K=512, dtype="fp16", reorder="rcm"),
    "products_rcm_bsr32": dict(kind="bsr", n=2449029, avg_deg=27.0, cmin=32, cmax=512,
                               p_in=0.97, bs=32, K=128, dtype="fp32", reorder="rcm"),
    # the block sizes benchmark.py:3-19 sweeps besides 16 / 32, on the reddit
    # stand-in: bs 2 / 4 / 8 (lane-group VALU kernel) and bs 64 (the bs 32 column
    # stream on 32 x 32 sub-blocks)
    "reddit_bsr8": dict(kind="bsr", n=232965, avg_deg=670.0, cmin=512, cmax=2048, p_in=0.99,
                        bs=8, K=128, dtype="fp32"),
    "reddit_bsr4": dict(kind="bsr", n=232965, avg_deg=670.0, cmin=512, cmax=2048, p_in=0.99,
                        bs=4, K=128, dtype="fp32"),
    "reddit_bsr2": dict(kind="bsr", n=232965, avg_deg=670.0, cmin=512, cmax=2048, p_in=0.99,
                        bs=2, K=128, dtype="fp32"),
    "reddit_bsr64": dict(kind="bsr", n=232965, avg_deg=670.0, cmin=512, cmax=2048, p_in=0.99,
                         bs=64, K=128, dtype="fp32"),
    # the bs 2 / 4 / 8 inputs re-blocked to 32 on the device (spmm_sbsr_reblock32, once per
    # matrix with the bs 32 analysis) and multiplied on the analysed bs 32 MFMA stream
    "reddit_bsr8_rb32": dict(kind="bsr", n=232965, avg_deg=670.0, cmin=512, cmax=2048,
                             p_in=0.99, bs=8, K=128, dtype="fp32", reblock=32),
    "reddit_bsr4_rb32": dict(kind="bsr", n=232965, avg_deg=670.0, cmin=512, cmax=2048,
                             p_in=0.99, bs=4, K=128, dtype="fp32", reblock=32),
    "reddit_bsr2_rb32": dict(kind="bsr", n=232965, avg_deg=670.0, cmin=512, cmax=2048,
                             p_in=0.99, bs=2, K=128, dtype="fp32", reblock=32),
    # §8f next row: dense-block + CSR remainder (divide.cu) on the reddit stand-in
    "reddit_hybrid32": dict(kind="hybrid", n=232965, avg_deg=670.0, cmin=512, cmax=2048,
                            p_in=0.99, bs=32, K=128, density="auto"),
}
METRIC = "SpMM GFLOP/s (2*nnz*K/t) + achieved HBM GB/s, ogbn-products K=128"


BSR_TRAFFIC = os.path.join(ROOT, "profiles", "r06_final", "bsr_bytes.jsonl")
# counter bytes of the CSR kernels per workload (tools/pmc_bytes.sh)
CSR_TRAFFIC = os.path.join(ROOT, "profiles", "r06_final", "csr_bytes.jsonl")


def csr_counter_bytes(workload: str):
    """PMC bytes per launch (FETCH_SIZE x calibration + WRITE_SIZE) recorded
    for a CSR workload's kernel in CSR_TRAFFIC, else None."""
    rec = None
    try:
        with open(CSR_TRAFFIC) as f:
            for line in f:
                r = json.loads(line)
                if r.get("workload") == workload:
                    rec = r.get("counter_bytes_per_launch")
    except (OSError, ValueError):
        return None
    return rec


def default_wpc(rows_per_launch: int, hot: bool = False) -> int:
    """The CSR grid's default waves per CU for a launch of that many rows, as the
    library sizes it (spmm_csr_default_waves_per_cu)."""
    from spmm_hip import _lib
    return int(_lib.lib().spmm_csr_default_waves_per_cu(int(rows_per_launch), 1 if hot else 0))


def kernel_source_tag() -> str:
    """First 16 hex digits of the SHA-256 of the BSR kernel source: counter
    bytes recorded for one build of the kernels are not reused for another."""
    import hashlib
    try:
        with open(os.path.join(ROOT, "spmm-denseblock_amd", "csrc", "bsr_kernels.hip"), "rb") as f:
            return hashlib.sha256(f.read()).hexdigest()[:16]
    except OSError:
        return "unknown"


def bsr_variant() -> str:
    """The BSR kernel variant the library runs: SPMM_BSR_VARIANT only in a
    TUNING build (spmm_get_build_options), which alone reads it."""
    from spmm_hip import _lib
    if _lib.lib().spmm_get_build_options() & _lib.BUILD_TUNING:
        return os.environ.get("SPMM_BSR_VARIANT", "default")
    return "default"


def bsr_traffic(key: dict):
    """PMC HBM bytes per launch of a BSR / hybrid workload's kernel
    (tools/pmc_bytes.sh: FETCH_SIZE x calibration + WRITE_SIZE,
    MI355X_MICROARCH.md §HBM): the last record of BSR_TRAFFIC whose workload,
    kernel, K, dtype, nnzb, variant and kernel-source tag all equal `key`'s,
    else None (a record of another shape or build is never used)."""
    rec = None
    try:
        with open(BSR_TRAFFIC) as f:
            for line in f:
                r = json.loads(line)
                if all(r.get(k) == v for k, v in key.items()):
                    rec = r
    except (OSError, ValueError):
        return None
    return rec and rec.get("counter_bytes_per_launch")


def csr_roofline(n_rows: int, ci: np.ndarray, K: int, kms: float) -> dict:
    """Roofline fields of a CSR line: SURVEY.md §8(d)'s gather model (one
    B-row read per nonzero) while its rate stays under the HBM peak; when B is
    cache-resident (the gather rate would pass the peak: re-reads served by
    L2 / MALL, e.g. the arxiv stand-in's 87-MB B) the compulsory bytes
    instead — the arrays, each distinct B row once, C once — with the gather
    model's rate kept beside it."""
    nnz = int(ci.size)
    gather = csr_bytes(n_rows, nnz, K)
    t = kms / 1e3
    if gather / t / 1e9 <= HBM_PEAK_GBPS:
        return {"achieved": round(gather / t / 1e9, 1),
                "frac": round(gather / t / 1e9 / HBM_PEAK_GBPS, 4),
                "algorithmic_bytes_per_launch": gather,
                "bytes_model": "SURVEY 8d gather: one B row per nonzero"}
    b_rows = int(np.unique(ci).size)
    comp = 4 * (n_rows + 1) + 8 * nnz + 4 * K * b_rows + 4 * K * n_rows
    return {"achieved": round(comp / t / 1e9, 1), "frac": round(comp / t / 1e9 / HBM_PEAK_GBPS, 4),
            "algorithmic_bytes_per_launch": comp,
            "bytes_model": "compulsory (B cache-resident): arrays, each distinct B row once, C once",
            "gather_model_bytes": gather, "gather_model_GBps": round(gather / t / 1e9, 1)}


def csr_bytes(n_rows: int, nnz: int, K: int) -> int:
    """SURVEY.md §8(d) CSR gather model: rowptr + (colind, val) + one B row per
    nnz + the C write."""
    return 4 * (n_rows + 1) + 8 * nnz + 4 * K * nnz + 4 * K * n_rows


def bsr_bytes(mb: int, nnzb: int, bs: int, K: int, s: int) -> int:
    """SURVEY.md §8(d) BSR model, s = value size."""
    return 4 * (mb + 1) + 4 * nnzb + s * nnzb * bs * bs + s * nnzb * bs * K + 4 * mb * bs * K


def community_graph(W, bs: int):
    """The community stand-in of a BSR / hybrid workload. With W["reorder"] the
    reorder-then-block pipeline of reorder_graph.cc:26-49 / run_bsrmm.cu runs on
    it: node ids scrambled (the graph as downloaded), then the in-repo reorderer
    (spmm_reorder_*). Returns rowptr, colind, the reorder record (None without
    a reorder) and the `data` label."""
    from spmm_hip import prep
    rp, ci = prep.community_csr(W["n"], W["avg_deg"], W["cmin"], W["cmax"], W["p_in"], 1234)
    if not W.get("reorder"):
        return rp, ci, None, ("synthetic community-ordered graph (stand-in for the reordered "
                              "dataset: rabbit_order / Gorder outputs are not reproducible "
                              "offline; the upper bound a reorderer reaches), U(-1,1) values")
    n = rp.size - 1
    upper = prep.block_metrics(rp, ci, bs)
    scr = np.random.default_rng(9).permutation(n).astype(np.int32)
    rp, ci = prep.permute_csr(rp, ci, scr)
    before = prep.block_metrics(rp, ci, bs)["nnzb"]
    t_ro = time.perf_counter()
    o2n = prep.reorder(rp, ci, W["reorder"])
    rp, ci = prep.permute_csr(rp, ci, o2n)
    t_ro = time.perf_counter() - t_ro
    after = prep.block_metrics(rp, ci, bs)
    rec = {"method": W["reorder"], "host_seconds": round(t_ro, 2),
           "nnzb_scrambled": int(before), "nnzb_reordered": int(after["nnzb"]),
           "block_fill_reordered": round(float(after["utilization"]), 4),
           "community_order_upper_bound": {"nnzb": int(upper["nnzb"]),
                                           "block_fill": round(float(upper["utilization"]), 4)}}
    return rp, ci, rec, ("synthetic community graph, node ids scrambled, then reordered "
                         f"in-repo ({W['reorder']}), U(-1,1) values")


def _time_prefix(run, n: int, budget_s: float):
    """Grow a row prefix until one run takes about budget_s / 3 (or covers all
    n rows), then repeat it within budget_s; returns (rows, run times)."""
    rows, spent = 1024, 0.0
    while True:
        rows = min(rows, n)
        t0 = time.perf_counter()
        run(rows)
        dt = time.perf_counter() - t0
        spent += dt
        if rows == n or dt >= budget_s / 3:
            break
        rows = int(rows * min(8.0, max(2.0, (budget_s / 3) / max(dt, 1e-4))))
    times = [dt]
    while spent < budget_s and len(times) < 15:
        t0 = time.perf_counter()
        run(rows)
        times.append(time.perf_counter() - t0)
        spent += times[-1]
    return rows, times


def _progress(msg: str) -> None:
    """One line on stderr per finished CPU-baseline leg (a long silent run
    looks hung to a watchdog)."""
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def _spread(ts) -> dict:
    """min / median / max of per-call times (s) and (max - min) / median."""
    a = np.asarray(ts, dtype=np.float64)
    med = float(np.median(a))
    return {"min_s": round(float(a.min()), 6), "median_s": round(med, 6),
            "max_s": round(float(a.max()), 6),
            "spread": round(float((a.max() - a.min()) / med), 4) if med > 0 else None}


def _batched_samples(run, min_sample_s: float = 0.1, nsamples: int = 11):
    """Per-call times of `run` from samples of back-to-back calls, each sample
    at least min_sample_s long (a short call's median otherwise measures
    thread wake-up, not the loop), after a warm-up sample."""
    run()
    # per-call time from a loop of at least a quarter second: a few calls can
    # land in a throttled period (cgroup CPU quota) and read 10x slow, which
    # made round 3's "1-s" samples 0.11 s long
    t0, calls = time.perf_counter(), 0
    while True:
        run()
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= min(0.25, min_sample_s):
            break
    one = max(dt / calls, 1e-6)
    reps = max(1, int(np.ceil(min_sample_s / one)))
    ts = []
    for _ in range(nsamples + 1):
        t0 = time.perf_counter()
        for _ in range(reps):
            run()
        ts.append((time.perf_counter() - t0) / reps)
    return reps, ts[1:]


def _cpu_model() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _host_cpus() -> dict:
    """Threads this process may run on (affinity / cgroup cpuset), the
    physical cores among them (unique (package, core) pairs in sysfs), and
    the machine's physical cores (unique (package, core) pairs in
    /proc/cpuinfo)."""
    phys, pkg = set(), None
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("physical id"):
                    pkg = line.split(":", 1)[1].strip()
                elif line.startswith("core id"):
                    phys.add((pkg, line.split(":", 1)[1].strip()))
    except OSError:
        pass
    aff = sorted(os.sched_getaffinity(0))
    mine = set()
    for c in aff:
        topo = f"/sys/devices/system/cpu/cpu{c}/topology/"
        try:
            with open(topo + "physical_package_id") as f1, open(topo + "core_id") as f2:
                mine.add((f1.read().strip(), f2.read().strip()))
        except OSError:
            mine.add(("cpu", c))
    quota = None  # cgroup v2 CPU bandwidth limit ("max 100000" = none)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
            quota = "none" if q == "max" else round(int(q) / int(per), 2)
    except (OSError, ValueError):
        pass
    return {"affinity_cpus": len(aff), "physical_cores_in_affinity": len(mine),
            "machine_physical_cores": len(phys) or None, "machine_logical_cpus": os.cpu_count(),
            "cgroup_cpu_quota_cpus": quota}


def cpu_baseline_config1(L) -> dict:
    """BASELINE configs[0] / BASELINE.md §2 row 1 as stated: spmm.cc csr_spmm
    (oracle_spmm_cc_csr: OpenMP rows, k-outer, double, unit values) on
    randomCSRMatrix(16384, 16384, 2^-10) + randomDenseMatrix(16384, 32) from a
    fresh mt19937_64(1234) (the reference generator's stream, bit-exact).
    One call takes well under a millisecond, so each of 5 samples times a
    loop of back-to-back calls of at least 1 s (after a warm-up sample):
    the box's cgroup grants 16 CPUs of time per 100-ms CFS period, so 128
    threads run stop-go, and a sample must span many periods for its mean
    to be the throttled rate rather than the phase it landed in (100-ms
    samples spread 15-180 % in round 3). min / median / max per call are
    reported. coo_spmm (spmm.cc:27-43) beside it."""
    from helpers import ptr
    from spmm_hip import prep
    m, K = 16384, 32
    prep.rng_seed(1234)
    rp, ci, _ = prep.random_csr(m, m, 2.0 ** -10)
    B = prep.random_dense_matrix(m, K).astype(np.float64)
    ip, ix = rp.astype(np.int64), ci.astype(np.int64)
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(rp))
    out = np.empty((m, K))
    res = {}
    for name, run in (("csr_spmm", lambda: L.oracle_spmm_cc_csr(m, K, ptr(ip), ptr(ix), ptr(B), K,
                                                                ptr(out))),
                      ("coo_spmm", lambda: L.oracle_spmm_cc_coo(m, K, ix.size, ptr(row), ptr(ix),
                                                                ptr(B), K, ptr(out)))):
        reps, ts = _batched_samples(run, min_sample_s=1.0, nsamples=5)
        _progress(f"config1 {name} done")
        sp = _spread(ts)
        res[name] = {"GFLOPs": round(2.0 * ci.size * K / sp["median_s"] / 1e9, 3),
                     "calls_per_sample": reps, **sp}
    return {"value": res["csr_spmm"]["GFLOPs"], "unit": "GFLOP/s", "kind": "port",
            "cores": int(L.oracle_num_threads()),
            "sample": (f"BASELINE config 1: spmm.cc csr_spmm restated on randomCSRMatrix(16384, "
                       f"16384, 2^-10) ({ci.size} nnz, mt19937_64(1234)), K=32, double, unit "
                       f"values; 5 samples of {res['csr_spmm']['calls_per_sample']} back-to-back "
                       f"calls (>= 1 s each), median per call"), **res}


def cpu_baseline_child(args) -> None:
    """One thread count of the CPU baseline, in a process of its own (the
    parent sets OMP_NUM_THREADS / OMP_PROC_BIND / OMP_PLACES before the
    OpenMP runtime starts). Regenerates the workload's graph (same generator
    and seed as the GPU leg) and prints one JSON line.

    spmm.cc csr_spmm restated (oracle_spmm_cc_csr: OpenMP rows, k-outer,
    double, unit values) on the SAME graph: a growing row prefix until about
    budget_s of CPU work, or the whole graph repeated, median of the
    repeats. Also the fp32-weighted variant at the same shape:
    the oracle's sequential-FMA csrmm on U(-1,1) values, same prefix rule;
    and BASELINE config 1 (cpu_baseline_config1)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import load_oracle, ptr
    from spmm_hip import prep
    L = load_oracle()
    W = WORKLOADS[args.workload]
    K = args.K or W["K"]
    rp, ci = prep.powerlaw_csr(W["n"], W["nnz"], W["max_deg"], 2.3, 1234)
    n = rp.size - 1
    budget_s = args.cpu_budget
    Bd = np.random.default_rng(1).uniform(-1, 1, (n, K))  # double, as spmm.cc
    ip64, ix64 = rp.astype(np.int64), ci.astype(np.int64)
    out = np.empty((n, K))
    rows, times = _time_prefix(
        lambda r: L.oracle_spmm_cc_csr(r, K, ptr(ip64), ptr(ix64), ptr(Bd), K, ptr(out)),
        n, budget_s)
    del out, Bd
    _progress(f"cpu_baseline csr_spmm ({os.environ.get('OMP_NUM_THREADS')} threads) done")
    sp = _spread(times)
    nnz_s = int(rp[rows])
    res = {"value": round(2.0 * nnz_s * K / sp["median_s"] / 1e9, 3), "unit": "GFLOP/s",
           "cores": int(L.oracle_num_threads()), "kind": "port", "cpu_model": _cpu_model(),
           "omp_env": {k: os.environ.get(k) for k in ("OMP_NUM_THREADS", "OMP_PROC_BIND",
                                                      "OMP_PLACES")},
           "sample": (f"spmm.cc csr_spmm restated (double, unit values, k-outer, OpenMP) on "
                      f"{'all' if rows == n else 'the first'} {rows} rows ({nnz_s} nnz) of the "
                      f"same synthetic graph, K={K}; median of {len(times)} runs "
                      f"({sp['median_s']:.3f} s each, {sum(times):.1f} s total)"), **sp}
    Bf = np.random.default_rng(1).uniform(-1, 1, (n, K)).astype(np.float32)
    vf = np.random.default_rng(2).uniform(-1, 1, ci.size).astype(np.float32)
    outf = np.empty((n, K), np.float32)
    rows, times = _time_prefix(
        lambda r: L.oracle_csrmm_f32(r, K, ptr(rp), ptr(ci), ptr(vf), 0, ptr(Bf), K, 0, 1.0, 0.0,
                                     ptr(outf), K, 0), n, budget_s)
    sp = _spread(times)
    nnz_s = int(rp[rows])
    res["fp32_weighted"] = {
        "value": round(2.0 * nnz_s * K / sp["median_s"] / 1e9, 3), "unit": "GFLOP/s",
        "sample": (f"fp32 values, sequential FMA per element (oracle_csrmm_f32, OpenMP rows) on "
                   f"{'all' if rows == n else 'the first'} {rows} rows ({nnz_s} nnz), K={K}; "
                   f"median of {len(times)} runs ({sp['median_s']:.3f} s each)"), **sp}
    del Bf, vf, outf
    _progress("cpu_baseline fp32_weighted done")
    res["config1"] = cpu_baseline_config1(L)
    print(json.dumps(res), flush=True)


def cpu_baseline(args, K: int) -> dict:
    """BASELINE.md §2's CPU protocol on the GPU box's host: OpenMP threads =
    the physical cores this process may run on (all 128 of the box when the
    affinity mask is the whole machine), one per core (OMP_PROC_BIND=close,
    OMP_PLACES=cores). The box's one-GPU CPU share, 16 threads bound the same
    way, is the labelled second entry. Each thread count runs in a child
    process of its own (cpu_baseline_child), so the OpenMP runtime starts
    with that environment."""
    hc = _host_cpus()
    counts = [("all_physical_cores", hc["physical_cores_in_affinity"])]
    if hc["physical_cores_in_affinity"] != 16:
        counts.append(("gpu_share_16_threads", 16))
    legs = {}
    for label, T in counts:
        env = dict(os.environ, OMP_NUM_THREADS=str(T), OMP_PROC_BIND="close", OMP_PLACES="cores")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-child",
                            "--workload", args.workload, "--K", str(K), "--cpu-budget",
                            str(args.cpu_budget)], env=env, stdout=subprocess.PIPE,
                           stderr=None, text=True, timeout=900)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            legs[label] = {"error": f"rc {r.returncode} (child stderr above)"}
        else:
            legs[label] = json.loads(lines[-1])
    res = dict(legs["all_physical_cores"])
    res["protocol"] = ("BASELINE.md §2: OMP_NUM_THREADS = physical cores in this process's "
                       "affinity, OMP_PROC_BIND=close, OMP_PLACES=cores")
    q = hc.get("cgroup_cpu_quota_cpus")
    T = hc["physical_cores_in_affinity"]
    share = legs.get("gpu_share_16_threads", {})
    if (isinstance(q, (int, float)) and q <= 16 < T and "value" in share):
        # VERDICT round 4 (weak 9): under a CPU quota of at most 16 CPUs the all-cores leg is a
        # contention measurement; the reported baseline is the leg within the quota (the
        # threads actually used), the all-cores leg stays beside it
        res = dict(share)
        res["protocol"] = (f"the cgroup grants {q:g} CPUs: OMP_NUM_THREADS = 16 (one per core, "
                           "OMP_PROC_BIND=close, OMP_PLACES=cores), the box's one-GPU CPU share; "
                           "BASELINE.md §2's all-physical-cores leg is kept as "
                           "all_physical_cores (a contention measurement under the quota)")
        res["all_physical_cores"] = legs["all_physical_cores"]
        res["gpu_share_16_threads"] = "this entry"
        counts = [c for c in counts if c[0] != "gpu_share_16_threads"]
    if isinstance(q, (int, float)) and q < T:
        # the quota, not the core count, is the host's capacity here
        res["quota_note"] = (
            f"the process's cgroup grants {q:g} CPUs of time per CFS period across its {T} "
            f"cores: {T} OpenMP threads run stop-go (all of them stopped whenever the group "
            f"has spent its quota), so the all-cores figure is a contention measurement and "
            f"its per-sample spread cannot be brought under 10 % by longer samples (config 1: "
            f"0.2-0.8 ms calls land anywhere in the stop-go phases); the 16-thread leg, "
            f"within the quota, is the host's usable rate and the reported value")
    for label, _ in counts[1:]:
        res[label] = legs[label]
    res.update(hc)
    return res


GRAPH = False  # --graph: replay the step as a captured HIP graph (N = 1)
GRP32_W = 2    # block rows per group of the bs 32 grouped side line (spmm_bsr32_group_analysis_f32)
DUMP_ROWS = 65536        # --dump-outputs: rows of C kept when C is larger than DUMP_BYTES
DUMP_BYTES = 48 << 20


def dump_outputs(args, rank: int, **arrays) -> None:
    """--dump-outputs DIR: what the timed path left in its output tensors, as
    DIR/<name>.npy (float32; rank 0's tensors at N > 1). A tensor above
    DUMP_BYTES is written as a fixed sample of its leading dimension: DUMP_ROWS
    indices drawn once from default_rng(0), sorted, so two runs with the same
    arguments write the same elements."""
    if not args.dump_outputs or rank != 0:
        return
    import torch
    torch.cuda.synchronize()
    os.makedirs(args.dump_outputs, exist_ok=True)
    for name, t in arrays.items():
        if t.numel() * 4 > DUMP_BYTES and t.shape[0] > DUMP_ROWS:
            idx = np.sort(np.random.default_rng(0).choice(t.shape[0], DUMP_ROWS, replace=False))
            t = t[torch.from_numpy(idx).to(t.device)]
        if t.numel() * 4 > DUMP_BYTES:  # few, very long rows (a column-major C): a column sample
            idx = np.sort(np.random.default_rng(0).choice(t.shape[1], DUMP_BYTES // 4 // t.shape[0],
                                                          replace=False))
            t = t[:, torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(args.dump_outputs, name + ".npy"),
                np.ascontiguousarray(t.float().cpu().numpy()))


def timed_loop(step, h, steps, warmup, world, dist, raw=False, kernel_pass=True, after=None):
    """Warm up, time `steps` calls of step() on the wall clock, call after()
    (the output dump) and, with kernel_pass, run the steps once more under the
    handle's per-launch events for the kernel durations (else none: None / [])."""
    import torch
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    h.kernel_times()
    if GRAPH and world == 1:
        # The launches of one step captured once (workspace already sized by
        # the warm-up, so nothing allocates or syncs inside), replayed K
        # times; the kernel durations come from an event-timed eager pass
        # right after, over the same number of steps.
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            h.set_stream(torch.cuda.current_stream())  # the capture stream
            step()
        h.set_stream(torch.cuda.current_stream())
        g.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            g.replay()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        return elapsed, _kernel_pass(step, h, steps, raw, kernel_pass, after)
    # The timed region runs without the per-launch event pairs (two event
    # records around every launch cost several microseconds per step, 8 % of an
    # arxiv-sized step); the kernel durations come from an event-timed pass of
    # the same number of steps right after it.
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    return elapsed, _kernel_pass(step, h, steps, raw, kernel_pass, after)


def _kernel_pass(step, h, steps, raw, kernel_pass, after):
    """The tail of timed_loop: after() on what the timed steps left, then the
    event-timed pass (the launches' durations, or their mean unless raw)."""
    import torch
    if after is not None:
        after()
    if not kernel_pass:
        return [] if raw else None
    h.set_timing(True)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    h.set_timing(False)
    kt = h.kernel_times()
    if raw:
        return kt
    return float(np.mean(kt)) if kt else float("nan")


def run_csr_weak(args, W, world, rank, dev, dist):
    """N > 1 with --scaling weak (config 4's strong form is the default): every
    rank owns a products-size row block of a world-times larger power-law graph
    (spmm_hip.dist.stacked_block:
    n rows, nnz nonzeros, the 1-GPU workload's per-GPU work), B replicated
    with world*n rows, C row-sharded in place. No collective in the step; the
    all-gather that would assemble C on every rank is timed after the timed
    region and reported beside it (`exchange`)."""
    import torch
    from spmm_hip import dist as sdist
    from spmm_hip import ops
    K = args.K or W["K"]
    t_gen = time.perf_counter()
    rp, ci = sdist.stacked_block(W["n"], W["nnz"], W["max_deg"], rank, world)
    val = np.random.default_rng(2 + rank).uniform(-1, 1, ci.size).astype(np.float32)
    t_gen = time.perf_counter() - t_gen
    n, nnz = rp.size - 1, ci.size
    ncols = world * n
    d_rp, d_ci, d_v = (torch.from_numpy(a).to(dev) for a in (rp, ci, val))
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    B = torch.rand((ncols, K), device=dev, generator=g) * 2 - 1
    C = torch.empty((n, K), device=dev)
    h = ops.Handle()
    if args.waves_per_cu:
        h.set_csr_waves_per_cu(args.waves_per_cu)
    if args.csr_options is not None:
        h.set_csr_options(args.csr_options)

    def step():
        ops.csrmm(d_rp, d_ci, d_v, B, m=n, n=K, k=ncols, ldb=K, C=C, ldc=K, handle=h)

    elapsed, kt = timed_loop(step, h, args.steps, args.warmup, world, dist, raw=True,
                             after=lambda: dump_outputs(args, rank, C=C))
    kms = float(np.sum(kt)) / args.steps if kt else float("nan")
    tot = torch.tensor([nnz], dtype=torch.float64, device=dev)
    dist.all_reduce(tot)
    t = torch.tensor([elapsed, kms], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed, kms_max = float(t[0]), float(t[1])
    exchange = None
    if not args.no_exchange_probe:
        # What assembling the row-sharded C on every rank would cost (one
        # all-gather of n*K fp32 per rank over RCCL / xGMI), outside the step.
        full = torch.empty((world * n, K), device=dev)
        dist.all_gather_into_tensor(full, C)
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        reps = 3
        for _ in range(reps):
            dist.all_gather_into_tensor(full, C)
        torch.cuda.synchronize()
        ag = torch.tensor([(time.perf_counter() - t0) / reps], dtype=torch.float64, device=dev)
        dist.all_reduce(ag, op=dist.ReduceOp.MAX)
        recv = (world - 1) * n * K * 4
        exchange = {"allgather_ms": round(float(ag[0]) * 1e3, 3),
                    "bytes_received_per_rank": recv,
                    "GBps_per_rank": round(recv / float(ag[0]) / 1e9, 1),
                    "note": "timed after the step loop, not part of value"}
        del full
    crf = csr_roofline(n, ci, K, kms)
    vec = 4 if K > 128 and K % 4 == 0 else (2 if K > 64 and K % 2 == 0 else 1)
    rec = dict(
        value=2.0 * float(tot[0]) * K * args.steps / elapsed / 1e9,
        ms_per_step=elapsed / args.steps * 1e3, dtype="fp32",
        data=("synthetic: rank r owns row block r of a (world*n)-node Chung-Lu power-law graph "
              "(each block the 1-GPU stand-in's n / nnz / max degree, seed 1234+r), U(-1,1) "
              "values and replicated B; OGB data not reachable offline"),
        config={"workload": f"{args.workload}: csr_spmm K={K}, weak scaling, row block per rank, "
                            f"B replicated ({ncols} rows), no collective in the step",
                "n_per_rank": n, "nnz_per_rank": nnz, "n_total": ncols,
                "nnz_total": int(tot[0]), "K": K, "parallelism": f"rows{world}",
                "waves_per_cu": args.waves_per_cu or default_wpc(n), "csr_options": args.csr_options},
        roofline={"bound": "hbm", "peak": HBM_PEAK_GBPS, "unit": "GB/s", **crf,
                  "traffic": None, "kernel": f"csr_mergepath_kernel<{vec}>",
                  "kernel_ms": round(kms, 4), "kernel_ms_max_rank": round(kms_max, 4)},
        exchange=exchange, gen_seconds=round(t_gen, 2))
    return rec, None


def run_csr(args, W, world, rank, dev, dist):
    import torch
    from spmm_hip import dist as sdist
    from spmm_hip import ops, prep
    K = args.K or W["K"]
    t_gen = time.perf_counter()
    rp, ci = prep.powerlaw_csr(W["n"], W["nnz"], W["max_deg"], 2.3, 1234)
    val = np.random.default_rng(2).uniform(-1, 1, ci.size).astype(np.float32)
    t_gen = time.perf_counter() - t_gen
    n, nnz = rp.size - 1, ci.size
    shard = sdist.make_shard(rp, ci, val, rank, world)
    d_rp = torch.from_numpy(shard.rowptr).to(dev)
    d_ci = torch.from_numpy(np.ascontiguousarray(shard.colind)).to(dev)
    d_v = torch.from_numpy(np.ascontiguousarray(shard.val)).to(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    B = torch.rand((n, K), device=dev, generator=g) * 2 - 1
    h = ops.Handle()
    if args.waves_per_cu:
        h.set_csr_waves_per_cu(args.waves_per_cu)
    if args.csr_options is not None:
        h.set_csr_options(args.csr_options)
    nch = args.chunks or (4 if world > 1 else 1)
    if nch > 1 and not dist.is_initialized():
        raise SystemExit("--chunks > 1 at N = 1 needs a torch.distributed launcher")
    if (world > 1 or nch > 1) and args.csr_layout == "col":
        raise SystemExit("--csr-layout col is a 1-GPU, one-chunk form")
    hot = bool(W.get("hot"))
    analysis_ms = None
    if hot:
        if world > 1 or nch > 1 or args.csr_layout == "col":
            raise SystemExit("the hot-column line is the 1-GPU row-major product")
        ts = []
        for _ in range(3):  # once per matrix; timed apart from the step
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d_tag = ops.csr_hot_analysis(d_ci, n=K, k=n, handle=h)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        analysis_ms = min(ts) * 1e3
        hot_share = float((d_tag < 0).float().mean())
    if world > 1 or nch > 1:
        # C is the contiguous n x K matrix on every rank: the kernel writes
        # this rank's rows in place, and the exchange of chunk c (batched
        # isend / irecv of exact row shards, RCCL p2p over xGMI) overlaps the
        # compute of chunk c + 1
        C_full = torch.empty((n, K), device=dev)

        def compute_chunk(r0, r1, dest):
            ops.csrmm(d_rp[r0:r1 + 1], d_ci, d_v, B, m=r1 - r0, n=K, k=n, ldb=K, C=dest,
                      ldc=K, handle=h)

        def step():
            sdist.chunked_spmm(shard, C_full, compute_chunk, nch)
        C_out = C_full

        def exchange_only():
            works = []
            for c in range(nch):
                works += sdist.exchange_chunk(C_full, shard, c, nch)
            for w in works:
                w.wait()
    elif args.csr_layout == "col":
        # cusparseScsrmm's layout (run_csrmm.cu:135-137): B and C column-major
        Bc = B.t().contiguous()
        Cc = torch.empty((K, n), device=dev)

        def step():
            ops.csrmm(d_rp, d_ci, d_v, Bc, m=n, n=K, k=n, ldb=n, order_b=ops.ORDER_COL, C=Cc,
                      ldc=n, order_c=ops.ORDER_COL, handle=h)
        C_out = Cc
    else:
        C_slot = torch.empty((n, K), device=dev)
        product, ci_step = ops.csrmm, d_ci
        if hot:
            product, ci_step = ops.csrmm_hot, d_tag

        def step():
            product(d_rp, ci_step, d_v, B, m=shard.rows, n=K, k=n, ldb=K, C=C_slot, ldc=K,
                    handle=h)
        C_out = C_slot

    # the event-timed pass (kernel_ms and the byte rates of `roofline`) is a run of
    # its own: with --full, and in a torch.distributed launch, whose line reports
    # compute and collective apart
    kpass = bool(args.full or dist.is_initialized())
    elapsed, kt = timed_loop(step, h, args.steps, args.warmup, world, dist, raw=True,
                             kernel_pass=kpass,
                             after=lambda: dump_outputs(args, rank, C=C_out))
    # kernel time per step (all chunks of a step; one launch when unchunked)
    kms = float(np.sum(kt)) / args.steps if kt else float("nan")
    t = torch.tensor([elapsed, kms], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed, kms_max = float(t[0]), float(t[1])
    if kpass:
        crf = csr_roofline(shard.rows, shard.colind[int(shard.rowptr[0]):], K, kms)
    else:
        crf = {"achieved": None, "frac": None,
               "algorithmic_bytes_per_launch": csr_bytes(shard.rows, shard.nnz, K),
               "bytes_model": "SURVEY 8d gather: one B row per nonzero (the kernel-timed "
                              "pass and its byte rates: --full)"}
    traffic = None
    if kpass and hot and K == W["K"] and nnz == W["nnz"] and world == 1:
        # counter bytes of the hot kernel on this workload's own shape (tools/pmc_bytes.sh)
        traffic = csr_counter_bytes(args.workload)
        if traffic and crf.get("gather_model_GBps"):
            # The gather rate passed the peak (MALL-served re-reads), and the
            # compulsory model (~3 GB) says nothing about this kernel: its own
            # counter bytes are the roofline here, the two models stay beside.
            t_s = kms / 1e3
            crf.update(achieved=round(traffic / t_s / 1e9, 1),
                       frac=round(traffic / t_s / 1e9 / HBM_PEAK_GBPS, 4),
                       bytes_model=("counter bytes of this kernel on this shape (FETCH_SIZE x "
                                    "calibration + WRITE_SIZE, " +
                                    os.path.relpath(CSR_TRAFFIC, ROOT) + ")"),
                       compulsory_bytes=crf["algorithmic_bytes_per_launch"],
                       algorithmic_bytes_per_launch=crf["gather_model_bytes"],
                       gather_model_frac=round(crf["gather_model_GBps"] / HBM_PEAK_GBPS, 4))
    if os.path.exists(args.traffic_json) and not hot:  # bytes of the plain kernel only
        try:
            with open(args.traffic_json) as f:
                tj = json.load(f)
            if tj.get("K") == K and tj.get("nnz") == shard.nnz:
                traffic = tj.get("hbm_bytes_per_launch")
        except (OSError, ValueError):
            traffic = None
    vec = 4 if K > 128 and K % 4 == 0 else (2 if K > 64 and K % 2 == 0 else 1)
    rec = dict(
        value=2.0 * nnz * K * args.steps / elapsed / 1e9, ms_per_step=elapsed / args.steps * 1e3,
        dtype="fp32",
        data=("synthetic (Chung-Lu power-law digraph with the dataset's n / nnz / max degree, "
              "U(-1,1) values and B; OGB data not reachable offline)"),
        config={"workload": f"{args.workload}: csr_spmm K={K}" +
                (f" row-partitioned over {world} ranks (nnz-balanced) + chunked RCCL exchange of "
                 f"C's row shards in the step (BASELINE config 4's all-gather: exact shards, "
                 f"batched p2p over xGMI, into the contiguous n x K C on every rank), strong "
                 f"scaling" if world > 1 else ""),
                "n": n, "nnz": nnz, "K": K, "max_deg": int(np.diff(rp).max()),
                "parallelism": f"rows{world}" if world > 1 else "single",
                "exchange_chunks": nch, "hip_graph": bool(GRAPH and world == 1),
                "waves_per_cu": args.waves_per_cu or default_wpc(n // max(world, 1) // max(nch, 1), hot),
                "csr_options": args.csr_options, "layout_BC": args.csr_layout},
        roofline={"bound": "hbm", "peak": HBM_PEAK_GBPS, "unit": "GB/s", **crf,
                  "traffic": traffic,
                  "kernel": f"csr_mergepath_kernel<{vec}>" + (" (hot-column hints)" if hot else ""),
                  "kernel_ms": round(kms, 4) if kpass else None,
                  "kernel_ms_max_rank": round(kms_max, 4) if kpass else None},
        gen_seconds=round(t_gen, 2))
    if (not hot and world == 1 and nch == 1 and args.csr_layout != "col"
            and args.workload == "products_csr" and not args.no_hot_side):
        # Beside the drop-in line (not `value`): the same product on the
        # hot-column cache hints, analysis once, timed apart.
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d_tag = ops.csr_hot_analysis(d_ci, n=K, k=n, handle=h)
        torch.cuda.synchronize()
        a_ms = (time.perf_counter() - t0) * 1e3

        def step_hot():
            ops.csrmm_hot(d_rp, d_tag, d_v, B, m=shard.rows, n=K, k=n, ldb=K, C=C_slot, ldc=K,
                          handle=h)
        e_hot, kt_hot = timed_loop(step_hot, h, args.steps, args.warmup, world, dist, raw=True)
        k_hot = float(np.sum(kt_hot)) / args.steps if kt_hot else float("nan")
        side = {
            "entry": "spmm_csr_hot_analysis once + spmm_csrmm_hot_f32 per step (bit-identical C)",
            "value": round(2.0 * nnz * K * args.steps / e_hot / 1e9, 2), "unit": "GFLOP/s",
            "ms_per_step": round(e_hot / args.steps * 1e3, 4), "kernel_ms": round(k_hot, 4),
            "analysis_ms_first_call": round(a_ms, 3),
            # SURVEY 8(d)'s gather model (one B row per nonzero) passes the peak
            # here (the MALL serves the re-reads), so it is a rate, not a fraction
            "gather_model_GBps": round(csr_bytes(shard.rows, shard.nnz, K) /
                                       (k_hot / 1e3) / 1e9, 1)}
        hot_tr = csr_counter_bytes("products_csr_hot")
        if hot_tr:
            # the roofline of this kernel: its own counter bytes, as products_csr_hot
            side.update(counter_bytes_per_launch=hot_tr,
                        achieved=round(hot_tr / (k_hot / 1e3) / 1e9, 1),
                        frac=round(hot_tr / (k_hot / 1e3) / 1e9 / HBM_PEAK_GBPS, 4),
                        bytes_model="counter bytes of the hot kernel (" +
                                    os.path.relpath(CSR_TRAFFIC, ROOT) + ")")
        rec["hot_column_hints"] = side
    if hot:
        rec["analysis_ms"] = round(analysis_ms, 4)
        rec["hot_gather_share"] = round(hot_share, 4)
        rec["config"]["workload"] += (" on hot-column cache hints (spmm_csr_hot_analysis once, "
                                      "analysis_ms apart; spmm_csrmm_hot_f32 per step)")
    if dist.is_initialized() and nch > 1 or world > 1:
        # compute and collective reported separately (a world-1
        # torch.distributed launch with --chunks > 1 rehearses it through RCCL:
        # no peer, so nothing moves).
        #  kernel_ms (roofline): this rank's kernels per step, max over ranks;
        #  exchange_ms: the step's exchanges alone (no compute), max over ranks;
        #  collective_ms_exposed: step minus the slowest rank's kernel time, the
        #    part of the collective the overlap did not hide.
        for _ in range(2):
            exchange_only()
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        reps = 5
        for _ in range(reps):
            exchange_only()
        torch.cuda.synchronize()
        ag = torch.tensor([(time.perf_counter() - t0) / reps * 1e3], dtype=torch.float64,
                          device=dev)
        dist.all_reduce(ag, op=dist.ReduceOp.MAX)
        recv = (n - shard.rows) * K * 4
        rec["exchange"] = ("all-gather of exact row shards: per chunk one batch of isend / irecv "
                           "pairs (RCCL p2p, one per peer and direction) straight into the "
                           "contiguous n x K C of every rank; no padding, no compaction")
        rec["exchange_ms"] = round(float(ag[0]), 4)
        rec["exchange_bytes_received_rank0"] = int(recv)
        rec["exchange_GBps_rank0"] = (round(recv / (float(ag[0]) / 1e3) / 1e9, 1)
                                      if recv else None)
        rec["collective_ms_exposed"] = round(rec["ms_per_step"] - kms_max, 4)
        rec["rows_per_rank"] = [int(b) for b in np.diff(shard.bounds)]
        rec["nnz_per_rank"] = [int(rp[b1] - rp[b0]) for b0, b1 in
                               zip(shard.bounds[:-1], shard.bounds[1:])]
        # rank 0: the same product on one GPU (whole matrix, same kernel), for
        # the speed-up of this strong-scaling run; outside the timed region
        one = torch.zeros(1, dtype=torch.float64, device=dev)
        if rank == 0:
            del d_rp, d_ci, d_v
            a_rp, a_ci, a_v = (torch.from_numpy(a).to(dev) for a in (rp, ci, val))
            Cw = torch.empty((n, K), device=dev)
            h1 = ops.Handle()
            _, one_ms = timed_loop(lambda: ops.csrmm(a_rp, a_ci, a_v, B, n=K, k=n, ldb=K, C=Cw,
                                                     ldc=K, handle=h1), h1, 5, 2, 1, dist)
            t0 = time.perf_counter()
            for _ in range(5):
                ops.csrmm(a_rp, a_ci, a_v, B, n=K, k=n, ldb=K, C=Cw, ldc=K, handle=h1)
            torch.cuda.synchronize()
            one[0] = (time.perf_counter() - t0) / 5 * 1e3
            rec["one_gpu"] = {"ms_per_step": round(float(one[0]), 4),
                              "kernel_ms": round(one_ms, 4),
                              "speedup": round(float(one[0]) / rec["ms_per_step"], 3),
                              "note": "rank 0, whole matrix, same kernel, after the timed region"}
            del a_rp, a_ci, a_v, Cw
        dist.barrier()
    return rec, (rp, ci, K)


def _side_traffic(workload: str, kernel: str, K: int, dt: str, nnzb: int, comp: int,
                  kms: float) -> dict:
    """Counter bytes of a side entry (grouped / analysed) beside a drop-in line: the
    record of the standalone workload that runs the same entry on the same matrix
    (tools/pmc_bytes.sh), under the same key rule as the line's own traffic."""
    tr = bsr_traffic({"workload": workload, "kernel": kernel, "K": K, "dtype": dt, "nnzb": nnzb,
                      "layout_BC": "row", "variant": bsr_variant(),
                      "kernel_src": kernel_source_tag()})
    out = {"compulsory_bytes": comp, "traffic": tr, "traffic_from": workload}
    if tr:
        t = kms / 1e3
        out.update(traffic_GBps=round(tr / t / 1e9, 1),
                   traffic_frac=round(tr / t / 1e9 / HBM_PEAK_GBPS, 4),
                   traffic_over_compulsory=round(tr / comp, 3))
    return out


def _timed_analysis(make):
    """A group analysis timed twice (host wall clock to the end of its work on the
    stream): the first call on the handle (it loads the analysis kernels and grows
    the handle's buffers), then a second on a fresh object, the once-per-matrix
    cost of a warm process. Returns (the second object, first ms, repeat ms)."""
    import torch
    ts, obj = [], None
    for _ in range(2):
        if obj is not None:
            obj.close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        obj = make()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return obj, ts[0], ts[1]


def _epoch_loop(analysis_ms: float, grouped_ms: float, dropin_ms: float, epochs: int = 10):
    """run_csrmm.cu:120-159's loop of 10 products on one matrix: the grouped
    entry pays its analysis once, the drop-in stream nothing."""
    g = analysis_ms + epochs * grouped_ms
    d = epochs * dropin_ms
    return {"epoch_loop": {"epochs": epochs, "grouped_with_analysis_ms": round(g, 3),
                           "drop_in_ms": round(d, 3), "grouped_wins": bool(g < d),
                           "note": "run_csrmm.cu:120-159's epoch loop; analysis_ms_repeat + "
                                   "epochs x grouped ms_per_step against epochs x the drop-in "
                                   "line's ms_per_step"}}


def run_bsr(args, W, world, rank, dev, dist):
    import torch
    from spmm_hip import ops, prep
    if world > 1:
        raise SystemExit("BSR workloads are single-GPU configs (BASELINE configs 3 and 5)")
    K, bs, dt = args.K or W["K"], W["bs"], args.dtype or W["dtype"]
    t_gen = time.perf_counter()
    rp, ci, reorder, data = community_graph(W, bs)
    n, nnz = rp.size - 1, ci.size
    val = np.random.default_rng(2).uniform(-1, 1, nnz).astype(np.float32)
    t_gen = time.perf_counter() - t_gen
    t_conv = time.perf_counter()
    brp, bci, bval = prep.csr2bsr(n, n, rp, ci, val, bs, 0)  # host preprocessing
    t_conv = time.perf_counter() - t_conv
    mb = (n + bs - 1) // bs
    nnzb = int(bci.size)
    s = 4 if dt == "fp32" else 2
    tdt = torch.float32 if dt == "fp32" else torch.float16
    d_brp, d_bci = torch.from_numpy(brp).to(dev), torch.from_numpy(bci).to(dev)
    d_bv = torch.from_numpy(bval).to(dev).to(tdt)
    bs_in, reblock_ms = bs, None
    if W.get("reblock"):
        # small blocks onto the bs 32 MFMA stream: the device re-blocking
        # (spmm_xbsr_reblock32_nnzb + spmm_sbsr_reblock32) is part of the
        # once-per-matrix analysis, timed apart with the bs 32 analysis below
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d_brp, d_bci, d_bv = ops.bsr_reblock32(d_brp, d_bci, d_bv, mb=mb, bs=bs)
        torch.cuda.synchronize()
        reblock_ms = (time.perf_counter() - t0) * 1e3
        bs, mb, nnzb = 32, int(d_brp.numel()) - 1, int(d_bci.numel())
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    B = (torch.rand((mb * bs, K), device=dev, generator=g) * 2 - 1).to(tdt)
    h = ops.Handle()
    fn = ops.bsrmm if dt == "fp32" else ops.bsrmm_f16
    an = bool(W.get("analysed") or W.get("reblock"))
    gsel = args.group_rows or W.get("grouped") or 0
    gw = -1 if gsel == "auto" else int(gsel)  # -1: grouped, W chosen by the library
    analysis_ms = analysis_first_ms = None
    grp = None
    if gw:
        if (bs, dt) not in ((16, "fp16"), (32, "fp32")):
            raise SystemExit("the grouped streams are bs 16 fp16 and bs 32 fp32")
        Grouped = ops.GroupedBsr16 if bs == 16 else ops.GroupedBsr32
        grp, analysis_first_ms, analysis_ms = _timed_analysis(
            lambda: Grouped(d_brp, d_bci, d_bv, mb=mb, group_rows=max(gw, 0), handle=h))
        gw = grp.W
        del d_bv

        def fn(rp_, ci_, _v, B_, *, mb, kb, n, bs, ldb, C, ldc, order_b=ops.ORDER_ROW,
               order_c=ops.ORDER_ROW, handle=None):
            grp.mm(B_, kb=kb, n=n, ldb=ldb, order_b=order_b, C=C, ldc=ldc, order_c=order_c)
        d_bv = None
    if an:
        if (bs, dt) not in ((32, "fp32"), (16, "fp16")):
            raise SystemExit("the analysed column streams are bs 32 fp32 and bs 16 fp16")
        masks = torch.empty(nnzb, dtype=torch.int32, device=dev)
        vcol = torch.empty(nnzb * bs * bs, dtype=tdt, device=dev)
        analysis = ops.bsr32_analysis if bs == 32 else ops.bsr16_analysis
        product = ops.bsrmm_analysed if bs == 32 else ops.bsrmm_analysed_f16
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            analysis(d_bv, nnzb=nnzb, masks=masks, val_col=vcol, handle=h)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        analysis_ms = min(ts) * 1e3 + (reblock_ms or 0.0)
        del d_bv

        def fn(rp_, ci_, _v, B_, *, mb, kb, n, bs, ldb, C, ldc, order_b=ops.ORDER_ROW,
               order_c=ops.ORDER_ROW, handle=None):
            product(rp_, ci_, vcol, masks, B_, mb=mb, kb=kb, n=n, ldb=ldb, order_b=order_b, C=C,
                    ldc=ldc, order_c=order_c, handle=handle)
        d_bv = None
    if args.bsr_layout == "col":
        # cusparseSbsrmm's transB = N layout (run_bsrmm.cu:70-71): B and C
        # column-major with ld = mb*bs.
        Bc = B.t().contiguous()
        C = torch.empty((K, mb * bs), device=dev)

        def step():
            fn(d_brp, d_bci, d_bv, Bc, mb=mb, kb=mb, n=K, bs=bs, ldb=mb * bs,
               order_b=ops.ORDER_COL, C=C, ldc=mb * bs, order_c=ops.ORDER_COL, handle=h)
    else:
        C = torch.empty((mb * bs, K), device=dev)

        def step():
            fn(d_brp, d_bci, d_bv, B, mb=mb, kb=mb, n=K, bs=bs, ldb=K, C=C, ldc=K, handle=h)

    elapsed, kms = timed_loop(step, h, args.steps, args.warmup, 1, dist,
                              after=lambda: dump_outputs(args, rank, C=C))
    # bs 2 / 4 / 8 fp32: which kernel ran (the grouped MFMA stream from 2^20 blocks when its
    # sharing probe keeps the matrix, else the lane-group VALU kernel; spmm_bsr_small_path)
    small_path = h.small_bsr_path() if bs in (2, 4, 8) and dt == "fp32" and not an else None
    # The CSR path on the same matrix (the reference's question: does the
    # reordered BSR beat CSR?), fp32.
    d_rp, d_ci, d_v = (torch.from_numpy(a).to(dev) for a in (rp, ci, val))
    B32 = B.float()
    C2 = torch.empty((n, K), device=dev)
    h2 = ops.Handle()
    if args.csr_options is not None:
        h2.set_csr_options(args.csr_options)
    _, csr_ms = timed_loop(lambda: ops.csrmm(d_rp, d_ci, d_v, B32, m=n, n=K, k=mb * bs, ldb=K,
                                             C=C2, ldc=K, handle=h2), h2, 5, 2, 1, dist)
    # Column-masked kernels (the row-major / ROW-block layout):
    # a block's B rows are fetched only for its nonzero A columns, and bs = 32
    # runs only the MFMA steps whose column pair holds a nonzero. The counts
    # come from the CSR pattern (distinct (block row, column) and (block,
    # column pair) keys, counted on the device).
    # The column-major layout (cusparse transB = N) runs the same kernels on a
    # row-major staged copy of B, with C written column-major by their
    # epilogue; the transposes are separate launches, outside
    # kernel_ms.
    cm = bs in (16, 32, 64) and K % (4 if dt == "fp32" else 8) == 0 and not (bs == 64 and dt != "fp32")
    d_r = torch.repeat_interleave(torch.arange(n, device=dev, dtype=torch.int64),
                                  torch.from_numpy(np.diff(rp)).to(dev))
    d_c = torch.from_numpy(ci).to(dev).to(torch.int64)
    active_cols = int(torch.unique((d_r // bs) * n + d_c).numel())
    active_pairs = int(torch.unique(((d_r // bs) * mb + d_c // bs) * (bs // 2) +
                                    (d_c % bs) % (bs // 2)).numel())
    # bs 64 streams 32 x 32 sub-blocks: nonzero columns per 32-row half
    # (and bs 2 / 4 / 8: the grouped MFMA stream's union over 32-row groups)
    active_cols32 = (int(torch.unique((d_r // 32) * n + d_c).numel()) if bs in (2, 4, 8, 64)
                     else active_cols)
    b_rows = int(torch.unique(d_c).numel())  # distinct B rows the product touches
    del d_r, d_c
    # output columns per workgroup (bs 32: 128; bs 16: 256)
    tile = 256 if bs == 16 else 128
    ntiles = (K + tile - 1) // tile
    dense_flops = 2.0 * nnzb * bs * bs * K    # SURVEY §8d "MFMA-executed" (dense blocks)
    cs16 = cm and bs == 16 and dt == "fp16" and K >= 128
    if cm and bs == 32:
        # column stream: two v_mfma_f32_32x32x1_2b_f32 (32 rows x 64 columns,
        # k = 1) per nonzero column of a block and 128 output columns
        mfma_flops = active_cols * 2.0 * bs * K
    elif cm and bs == 64:
        # the same per nonzero column of a 32 x 32 sub-block
        mfma_flops = active_cols32 * 2.0 * 32 * K
    elif bs in (2, 4, 8) and dt == "fp32":
        # the grouped small-bs stream (bsr_small_grp_kernel) when it ran: two
        # v_mfma_f32_32x32x1_2b_f32 per (32-row group, nonzero column) of the union and 128
        # output columns; the lane-group VALU kernel runs no MFMA
        mfma_flops = active_cols32 * 2.0 * 32 * K if small_path == 1 else None
    elif cs16:
        # column stream: items of 16 nonzero columns packed across blocks, one
        # v_mfma_f32_16x16x16_f16 per item and 16 output columns (the last
        # item of a block row padded: counted as executed work below only
        # for the columns it holds)
        mfma_flops = active_cols * 2.0 * bs * K
    else:
        mfma_flops = dense_flops if bs >= 16 or dt == "fp32" else None
    if grp is not None and bs == 16:
        # one v_mfma_f32_16x16x16_f16 per item, wave and 16 output columns
        mfma_flops = grp.nitems * gw * 2.0 * 16 * 16 * K
    # (bs 32 grouped: each wave runs the MFMAs of its own nonzero columns, the column
    # stream's count above)
    peak = MFMA_PEAK_TFLOPS[dt]
    kbytes = bsr_bytes(mb, nnzb, bs, K, s)
    # Compulsory bytes (the roofline): the block values and the BSR index
    # arrays once per column tile of the kernel, every distinct B row the
    # product touches once, the C write once.
    # (analysed: the masks and only the nonzero columns' values, column-major;
    # grouped: the analysis buffer, item rows and A fragments)
    a_bytes = (4 * nnzb + s * active_cols * bs) if an else s * nnzb * bs * bs
    if grp is not None:
        a_bytes = grp.bytes - 4 * (mb + 1) - 4 * nnzb  # the index terms are added below
    comp_bytes = (ntiles * (4 * (mb + 1) + 4 * nnzb + a_bytes) + s * b_rows * K +
                  4 * mb * bs * K)
    # Upper byte model (round 2's roofline): the same A and indices, the B
    # rows of every (block row, nonzero column) pair with no reuse between
    # block rows, and C.
    cm_bytes = (ntiles * (4 * (mb + 1) + 4 * nnzb + a_bytes) + s * active_cols * K +
                4 * mb * bs * K) if cm else kbytes
    t = kms / 1e3
    kname = (f"bsr{bs}_{'f16' if bs == 16 else 'f32'}_grp_kernel" if grp is not None else
             ("bsr32_f32_cs2_kernel" if bs == 32 else
              "bsr32_f32_cs2_kernel (bs 64 sub-blocks)" if bs == 64 else
              "bsr16_f16_cs_kernel" if cs16 else "bsr16_cm_kernel") if cm else
             # bs 2 / 4 / 8: the grouped MFMA stream (bsr_small_grp_kernel) on matrices whose
             # block rows share their columns, the lane-group kernel on the rest
             f"bsr_small_grp_kernel<{bs}>" if small_path == 1 else
             f"bsr_small_kernel<{bs}> (lane-group VALU)" if small_path in (0, 2) else
             f"bsr{bs} register-fragment kernel")
    tkey = {"workload": args.workload, "kernel": kname, "K": K, "dtype": dt, "nnzb": nnzb,
            "layout_BC": args.bsr_layout,
            "variant": bsr_variant(),
            "kernel_src": kernel_source_tag()}
    rec = dict(
        value=2.0 * nnz * K * args.steps / elapsed / 1e9, ms_per_step=elapsed / args.steps * 1e3,
        dtype=dt,
        data=data,
        config={"workload": f"{args.workload}: " + (f"scrambled ids -> {reorder['method']} -> "
                                                    if reorder else "") +
                            (f"csr2bsr bs={bs_in} + device re-block to 32 + " if reblock_ms
                             else f"csr2bsr bs={bs} + ") + ("analysis + bsrmm_analysed" if an else
                                                     f"group analysis (W={gw}) + bsrmm_grouped"
                                                     if grp is not None else "bsrmm") +
                            f" K={K} {dt}", "n": n,
                "layout_BC": args.bsr_layout,
                "nnz": nnz, "K": K, "bs": bs, "nnzb": nnzb,
                "block_fill": round(nnz / (nnzb * bs * bs), 4),
                "active_column_fraction": round(active_cols / (nnzb * bs), 4),
                "active_pair_fraction": round(active_pairs / (nnzb * bs / 2), 4),
                "distinct_B_rows": b_rows, "parallelism": "single"},
        roofline={"bound": "hbm", "achieved": round(comp_bytes / t / 1e9, 1),
                  "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                  "frac": round(comp_bytes / t / 1e9 / HBM_PEAK_GBPS, 4),
                  "traffic": bsr_traffic(tkey),
                  "kernel": kname + (" (analysed: column masks, column-major A)" if an else "") +
                            (" (column-major C epilogue, B staged row-major)"
                             if args.bsr_layout == "col" and cm else ""),
                  "kernel_ms": round(kms, 4),
                  "bytes_per_launch": comp_bytes,
                  "bytes_model": ("compulsory: A values + BSR indices once per column tile, "
                                  "each distinct B row once, C write once" +
                                  ("; analysed: masks + the nonzero columns' values" if an
                                   else "")),
                  "bytes_model_upper": cm_bytes,
                  "bytes_model_upper_desc": (
                      "A values + indices per column tile, the B rows of every (block row, "
                      "nonzero column) pair (no reuse between block rows), C write" if cm else
                      "SURVEY 8d full-panel model"),
                  "upper_GBps": round(cm_bytes / t / 1e9, 1),
                  "traffic_key": tkey,
                  "mfma_executed_flops_per_launch": mfma_flops,
                  "mfma_executed_TFLOPs": (round(mfma_flops / t / 1e12, 2)
                                           if mfma_flops is not None else None),
                  "mfma_peak": peak,
                  "mfma_frac": (round(mfma_flops / t / 1e12 / peak, 4)
                                if mfma_flops is not None else None),
                  "small_bs_path": small_path,
                  "dense_block_equivalent_TFLOPs": round(dense_flops / t / 1e12, 2),
                  "full_panel_model_bytes_per_launch": kbytes,
                  "full_panel_model_GBps": round(kbytes / t / 1e9, 1)},
        csr_same_matrix_ms=round(csr_ms, 4), csr2bsr_host_seconds=round(t_conv, 2),
        analysis_ms=round(analysis_ms, 4) if (an or grp is not None) else None,
        reblock_ms=round(reblock_ms, 4) if reblock_ms else None,
        analysis_ms_first_call=(round(analysis_first_ms, 4) if grp is not None else None),
        gen_seconds=round(t_gen, 2), reorder=reorder)
    tr = rec["roofline"]["traffic"]
    if tr:
        # the PMC bytes (profiled launch) over this run's kernel time: the HBM
        # rate the kernel actually drives, beside the compulsory-byte rate above
        rec["roofline"]["traffic_GBps"] = round(tr / t / 1e9, 1)
        rec["roofline"]["traffic_frac"] = round(tr / t / 1e9 / HBM_PEAK_GBPS, 4)
        rec["roofline"]["traffic_over_compulsory"] = round(tr / comp_bytes, 3)
    if (not an and grp is None and args.bsr_layout == "row" and not args.no_analysed_side and
            (bs, dt) == (16, "fp16")):
        # Beside the drop-in line (not `value`): the grouped stream (groups of 4 block
        # rows sharing their B-row copies, analysis once, timed apart).
        g4, a_ms, a_rep = _timed_analysis(lambda: ops.GroupedBsr16(d_brp, d_bci, d_bv, mb=mb,
                                                                   group_rows=0, handle=h))
        e_g, k_g = timed_loop(lambda: g4.mm(B, kb=mb, n=K, ldb=K, C=C, ldc=K), h, args.steps,
                              args.warmup, 1, dist)
        ni = g4.nitems
        rec["grouped_entry"] = {
            "entry": f"spmm_bsr16_group_analysis_f16 (groupRows 0: the library chose "
                     f"{g4.W} block rows per group) once + spmm_bsrmm_grouped_f16 per step",
            "group_rows": g4.W,
            "value": round(2.0 * nnz * K * args.steps / e_g / 1e9, 2), "unit": "GFLOP/s",
            "ms_per_step": round(e_g / args.steps * 1e3, 4), "kernel_ms": round(k_g, 4),
            "analysis_ms_first_call": round(a_ms, 3), "analysis_ms_repeat": round(a_rep, 3),
            "items": int(ni),
            "mfma_executed_TFLOPs": round(ni * g4.W * 2.0 * 256 * K / (k_g / 1e3) / 1e12, 2),
            **_side_traffic(args.workload + "_grp", "bsr16_f16_grp_kernel", K, dt, nnzb,
                            ntiles * g4.bytes + s * b_rows * K + 4 * mb * bs * K, k_g),
            **_epoch_loop(a_rep, e_g / args.steps * 1e3, elapsed / args.steps * 1e3)}
        g4.close()
        del g4
    if (not an and grp is None and args.bsr_layout == "row" and not args.no_analysed_side and
            (bs, dt) == (32, "fp32") and K % 4 == 0):
        # Beside the drop-in line (not `value`): the grouped bs 32 stream (groups of 2 block
        # rows sharing their B-row copies, analysis once, timed apart; C bit-identical)
        g2, a_ms, a_rep = _timed_analysis(lambda: ops.GroupedBsr32(d_brp, d_bci, d_bv, mb=mb,
                                                                   group_rows=GRP32_W, handle=h))
        e_g, k_g = timed_loop(lambda: g2.mm(B, kb=mb, n=K, ldb=K, C=C, ldc=K), h, args.steps,
                              args.warmup, 1, dist)
        rec["grouped_entry"] = {
            "entry": f"spmm_bsr32_group_analysis_f32 ({GRP32_W} block rows per group) once + "
                     "spmm_bsrmm_grouped_f32 per step",
            "value": round(2.0 * nnz * K * args.steps / e_g / 1e9, 2), "unit": "GFLOP/s",
            "ms_per_step": round(e_g / args.steps * 1e3, 4), "kernel_ms": round(k_g, 4),
            "analysis_ms_first_call": round(a_ms, 3), "analysis_ms_repeat": round(a_rep, 3),
            "mfma_executed_TFLOPs": round(mfma_flops / (k_g / 1e3) / 1e12, 2),
            "mfma_frac": round(mfma_flops / (k_g / 1e3) / 1e12 / peak, 4),
            **_side_traffic(args.workload + "_grp", "bsr32_f32_grp_kernel", K, dt, nnzb,
                            ntiles * g2.bytes + s * b_rows * K + 4 * mb * bs * K, k_g),
            **_epoch_loop(a_rep, e_g / args.steps * 1e3, elapsed / args.steps * 1e3)}
        g2.close()
        del g2
    if (not an and grp is None and args.bsr_layout == "row" and not args.no_analysed_side and
            (bs, dt) in ((32, "fp32"), (16, "fp16"))):
        # Beside the drop-in line (not `value`): the same product on the analysed
        # entry (column masks + column-major A once per matrix, timed apart).
        del d_rp, d_ci, d_v, B32, C2
        masks = torch.empty(nnzb, dtype=torch.int32, device=dev)
        vcol = torch.empty(nnzb * bs * bs, dtype=tdt, device=dev)
        analysis = ops.bsr32_analysis if bs == 32 else ops.bsr16_analysis
        product = ops.bsrmm_analysed if bs == 32 else ops.bsrmm_analysed_f16
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        analysis(d_bv, nnzb=nnzb, masks=masks, val_col=vcol, handle=h)
        torch.cuda.synchronize()
        a_ms = (time.perf_counter() - t0) * 1e3
        del d_bv
        e_an, k_an = timed_loop(
            lambda: product(d_brp, d_bci, vcol, masks, B, mb=mb, kb=mb, n=K, ldb=K, C=C, ldc=K,
                            handle=h), h, args.steps, args.warmup, 1, dist)
        a_bytes_an = 4 * nnzb + s * active_cols * bs
        comp_an = (ntiles * (4 * (mb + 1) + 4 * nnzb + a_bytes_an) + s * b_rows * K +
                   4 * mb * bs * K)
        t_an = k_an / 1e3
        rec["analysed_entry"] = {
            "entry": ("spmm_bsr32_analysis_f32 once + spmm_bsrmm_analysed_f32 per step" if bs == 32
                      else "spmm_bsr16_analysis_f16 once + spmm_bsrmm_analysed_f16 per step"),
            "value": round(2.0 * nnz * K * args.steps / e_an / 1e9, 2), "unit": "GFLOP/s",
            "ms_per_step": round(e_an / args.steps * 1e3, 4), "kernel_ms": round(k_an, 4),
            "analysis_ms_first_call": round(a_ms, 3),
            "bytes_per_launch": comp_an,
            "achieved": round(comp_an / t_an / 1e9, 1),
            "frac": round(comp_an / t_an / 1e9 / HBM_PEAK_GBPS, 4),
            "bytes_model": "compulsory, analysed: masks + the nonzero columns' values",
            "mfma_executed_TFLOPs": round(mfma_flops / t_an / 1e12, 2),
            "mfma_frac": round(mfma_flops / t_an / 1e12 / peak, 4),
            **_side_traffic(args.workload + "_an", kname, K, dt, nnzb, comp_an, k_an)}
    return rec, None


# BASELINE configs 3 and 5 and north_star's BSR target, measured beside the N = 1
# headline (not `value`): each the drop-in call (spmm_bsrmm_ex_f32 / _f16, what
# run_bsrmm.cu:148-171 calls) with its grouped and analysed entries
BSR_SIDES = (("config3", "reddit_bsr32"), ("config5", "products_bsr16_f16"),
             ("products_bsr32", "products_bsr32"))


def bsr_side(args, workload: str, rank, dev, dist) -> dict:
    """One BSR workload's line, compacted to what a side entry needs."""
    import copy

    import torch
    a = copy.copy(args)
    a.workload, a.K, a.dtype, a.group_rows, a.bsr_layout = workload, 0, None, 0, "row"
    a.dump_outputs = None  # --dump-outputs holds the headline's C only
    r, _ = run_bsr(a, WORKLOADS[workload], 1, rank, dev, dist)
    rf = r["roofline"]
    keys = ("entry", "group_rows", "ms_per_step", "kernel_ms", "analysis_ms_first_call",
            "analysis_ms_repeat", "frac", "mfma_executed_TFLOPs", "mfma_frac", "traffic",
            "traffic_GBps", "traffic_frac", "traffic_over_compulsory", "compulsory_bytes",
            "epoch_loop")
    out = {"workload": r["config"]["workload"], "data": r["data"],
           "value": round(r["value"], 2), "unit": "GFLOP/s",
           "ms_per_step": round(r["ms_per_step"], 4), "kernel": rf["kernel"],
           "kernel_ms": rf["kernel_ms"], "roofline_frac": rf["frac"],
           "bytes_per_launch": rf["bytes_per_launch"],
           "mfma_executed_TFLOPs": rf["mfma_executed_TFLOPs"], "mfma_peak": rf["mfma_peak"],
           "mfma_frac": rf["mfma_frac"], "traffic": rf["traffic"],
           "traffic_frac": rf.get("traffic_frac"),
           "traffic_over_compulsory": rf.get("traffic_over_compulsory"),
           "nnzb": r["config"]["nnzb"], "block_fill": r["config"]["block_fill"],
           "csr_same_matrix_ms": r["csr_same_matrix_ms"]}
    for e in ("grouped_entry", "analysed_entry"):
        if e in r:
            out[e] = {k: r[e][k] for k in keys if k in r[e]}
    torch.cuda.empty_cache()
    return out


def run_hybrid(args, W, world, rank, dev, dist):
    """divide_matrix + hybrid SpMM (divide.cu:348-373): blocks with fill >=
    density on the BSR MFMA kernel, the remainder on the CSR kernel, one C.
    Reported beside pure-BSR and pure-CSR on the same matrix."""
    import torch
    from spmm_hip import ops, prep
    if world > 1:
        raise SystemExit("hybrid workloads are single-GPU")
    K, bs, dens = args.K or W["K"], args.bs or W["bs"], W["density"]
    rp, ci, reorder, data = community_graph(W, bs)
    n, nnz = rp.size - 1, ci.size
    val = np.random.default_rng(2).uniform(-1, 1, nnz).astype(np.float32)
    plan = None
    if args.density is None and dens == "auto":
        args.density = "auto"
    if args.density == "auto":
        plan = prep.hybrid_plan(rp, ci, bs, K)
        dens = plan["density"]
    elif args.density is not None:
        dens = float(args.density)
    t_div = time.perf_counter()
    crp, cci, cv, brp, bci, bv = prep.divide(n, rp, ci, val, bs, dens)
    t_div = time.perf_counter() - t_div
    mb = (n + bs - 1) // bs
    d = [torch.from_numpy(a).to(dev) for a in (crp, cci, cv, brp, bci, bv, rp, ci, val)]
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    B = torch.rand((mb * bs, K), device=dev, generator=g) * 2 - 1
    C = torch.empty((mb * bs, K), device=dev)
    h = ops.Handle()

    def step():
        ops.hybrid_csrmm(tuple(d[0:3]), tuple(d[3:6]), B, m=n, n=K, k=n, bs=bs, ldb=K, C=C,
                         ldc=K, handle=h)

    hopt = args.hybrid_options or 0
    if hopt:
        h.set_hybrid_options(hopt)
    elapsed, kt = timed_loop(step, h, args.steps, args.warmup, 1, dist, raw=True,
                             after=lambda: dump_outputs(args, rank, C=C))
    # Launches per step: one when the library fused both parts (bs = 32; by
    # default when the remainder is short per block row), else
    # the BSR kernel, then the CSR kernel (when both parts exist).
    parts = len(kt) // args.steps if kt else 0
    fused = parts == 1 and bci.size > 0 and cci.size > 0
    kt = np.array(kt[: parts * args.steps]).reshape(args.steps, parts) if parts else None
    h2 = ops.Handle()
    _, csr_ms = timed_loop(lambda: ops.csrmm(d[6], d[7], d[8], B, m=n, n=K, k=mb * bs, ldb=K,
                                             C=C, ldc=K, handle=h2), h2, 5, 2, 1, dist)
    ms = elapsed / args.steps * 1e3
    useful = 2.0 * nnz * K
    nb, nc = int(bci.size), int(cci.size)
    b_rows = int(np.unique(ci).size)  # distinct B rows the product touches
    # Compulsory bytes (the roofline): the BSR part's block values and index
    # arrays and the CSR remainder's arrays once, every distinct B row once,
    # the C write once. Upper model: both parts' own models summed (the BSR
    # part's full B panels, one B row per remainder nonzero).
    comp_bytes = (4 * (mb + 1) + 4 * nb + 4 * nb * bs * bs + 4 * (n + 1) + 8 * nc +
                  4 * b_rows * K + 4 * mb * bs * K)
    upper = csr_bytes(n, nc, K) + bsr_bytes(mb, nb, bs, K, 4)
    t = (float(kt.sum(axis=1).mean()) if kt is not None else ms) / 1e3
    kname = ("bsr32_f32_lds_kernel" if fused else "bsr MFMA kernel + csr_mergepath")
    tkey = {"workload": args.workload, "kernel": kname, "K": K, "dtype": "fp32", "nnzb": nb,
            "csr_remainder_nnz": nc, "hybrid_options": hopt,
            "variant": bsr_variant(),
            "kernel_src": kernel_source_tag()}
    rec = dict(
        value=useful * args.steps / elapsed / 1e9, ms_per_step=ms, dtype="fp32",
        data=data,
        config={"workload": f"{args.workload}: divide(bs={bs}, density={dens}) + hybrid "
                            f"BSR-MFMA/CSR K={K}", "n": n, "nnz": nnz, "K": K, "bs": bs,
                "nnzb": nb, "csr_remainder_nnz": nc,
                "bsr_fill": round((nnz - nc) / max(1, nb * bs * bs), 4),
                "distinct_B_rows": b_rows,
                "parallelism": "single", "hybrid_options": hopt, "fused": bool(fused)},
        roofline={"bound": "hbm", "achieved": round(comp_bytes / t / 1e9, 1),
                  "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                  "frac": round(comp_bytes / t / 1e9 / HBM_PEAK_GBPS, 4),
                  "traffic": bsr_traffic(tkey),
                  "kernel": ("bsr32_f32_lds_kernel<HYB> (fused)" if fused else
                             "bsr MFMA kernel + csr_mergepath"),
                  "kernel_ms": round(t * 1e3, 4),
                  "bytes_per_launch": comp_bytes,
                  "bytes_model": ("compulsory: BSR part values + indices, CSR remainder "
                                  "arrays, each distinct B row once, C write once"),
                  "bytes_model_upper": upper,
                  "bytes_model_upper_desc": ("SURVEY 8d: BSR part full panels + one B row "
                                             "per remainder nonzero"),
                  "upper_GBps": round(upper / t / 1e9, 1), "traffic_key": tkey},
        csr_same_matrix_ms=round(csr_ms, 4), divide_host_seconds=round(t_div, 2),
        plan=plan, reorder=reorder,
        part_kernel_ms=None if kt is None else [round(float(x), 4) for x in kt.mean(axis=0)])
    tr = rec["roofline"]["traffic"]
    if tr:
        rec["roofline"]["traffic_GBps"] = round(tr / t / 1e9, 1)
        rec["roofline"]["traffic_frac"] = round(tr / t / 1e9 / HBM_PEAK_GBPS, 4)
        rec["roofline"]["traffic_over_compulsory"] = round(tr / comp_bytes, 3)
    if kt is not None and parts == 2 and bs == 32:
        # The BSR part runs every MFMA step of its dense blocks and is bound by
        # the MFMA pipe (DESIGN.md §4a PMC), not by HBM.
        bsr_ms = float(kt.mean(axis=0)[0])
        tf = 2.0 * bci.size * bs * bs * K / (bsr_ms / 1e3) / 1e12
        rec["bsr_part"] = {"bound": "mfma", "kernel_ms": round(bsr_ms, 4),
                           "mfma_executed_TFLOPs": round(tf, 1),
                           "mfma_peak": MFMA_PEAK_TFLOPS["fp32"],
                           "mfma_frac": round(tf / MFMA_PEAK_TFLOPS["fp32"], 4)}
    return rec, None


def launch_argv(argv: list[str], n: int, port: int) -> list[str]:
    """The one-process-per-GPU launch of this same command line: the driver's
    own form (torch.distributed.run, one node, n ranks, rendezvous on
    127.0.0.1)."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
            f"--nproc-per-node={n}", "--master-addr", "127.0.0.1", "--master-port", str(port),
            os.path.abspath(__file__), *argv]


def launch_ranks(n: int, argv: list[str]) -> int:
    """`bench.py --gpus N` (N > 1) started without a launcher: start the N
    ranks as a CHILD torch.distributed.run (never an exec: nothing here has
    touched the GPU, and the ranks initialise it themselves), relay its
    output (rank 0's JSON line is the only stdout line) and return its exit
    code. Fewer than N visible devices: an error on stderr, no JSON line,
    exit 2 (a line whose n_gpus differs from --gpus is never printed)."""
    import socket
    import torch
    have = torch.cuda.device_count()  # counts devices without initialising HIP
    if have < n:
        print(f"bench.py: --gpus {n} but {have} GPU(s) visible; no measurement", file=sys.stderr,
              flush=True)
        return 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    return subprocess.run(launch_argv(argv, n, port), env=env).returncode


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default=None, choices=sorted(WORKLOADS),
                    help="default: products_csr at N = 1 (the metric), products_csr_k256 "
                         "(BASELINE config 4) at N > 1")
    ap.add_argument("--K", type=int, default=0, help="override the workload's K")
    ap.add_argument("--density", default=None,
                    help="hybrid workloads: divide threshold (a float, or 'auto' = spmm_hybrid_plan)")
    ap.add_argument("--bs", type=int, default=0, help="override a hybrid workload's block size")
    ap.add_argument("--dtype", choices=["fp32", "fp16"], default=None,
                    help="override a BSR workload's value type")
    ap.add_argument("--bsr-layout", choices=["row", "col"], default="row",
                    help="B/C storage for BSR workloads (col = cusparse transB=N)")
    ap.add_argument("--csr-layout", choices=["row", "col"], default="row",
                    help="B/C storage for CSR workloads (col = cusparseScsrmm, run_csrmm.cu)")
    ap.add_argument("--waves-per-cu", type=int, default=0)
    ap.add_argument("--csr-options", type=int, default=None, help="SPMM_CSR_* flags")
    ap.add_argument("--no-hot-side", action="store_true",
                    help="skip the hot-column side measurement of the products_csr line")
    ap.add_argument("--group-rows", type=int, default=0,
                    help="bs 16 fp16 / bs 32 fp32: run the grouped stream with this many block "
                         "rows per group")
    ap.add_argument("--no-analysed-side", action="store_true",
                    help="skip the analysed-entry side measurement of the bs 32 / bs 16 fp16 lines")
    ap.add_argument("--chunks", type=int, default=0,
                    help="row chunks per rank whose all-gathers overlap the next chunk's compute "
                         "(default 4 when N > 1; 1 = compute, then one all-gather; > 1 at N = 1 "
                         "needs a torch.distributed launcher)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="strong",
                    help="CSR at N > 1: strong = BASELINE config 4 as stated: the one graph "
                         "row-partitioned + RCCL all-gather of C in every step (default); weak = "
                         "a products-size row block per rank, B replicated, no collective in "
                         "the step")
    ap.add_argument("--no-exchange-probe", action="store_true",
                    help="weak scaling: skip timing the C all-gather after the step loop")
    ap.add_argument("--hybrid-options", type=int, default=None,
                    help="SPMM_HYBRID_* flags (0 = library default, 1 = force fused, 2 = force two launches, "
                         "+4 = split-bf16 products in the dense-block part)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-bsr-sides", action="store_true",
                    help="products_csr at N = 1: skip the config 3 / config 5 / products bs 32 "
                         "side entries")
    ap.add_argument("--cpu-budget", type=float, default=6.0,
                    help="seconds of CPU work per cpu_baseline leg (row prefix rule)")
    ap.add_argument("--cpu-baseline-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--traffic-json", default=os.path.join(ROOT, "profiles", "traffic.json"),
                    help="PMC-derived HBM bytes per launch (DESIGN.md §7)")
    ap.add_argument("--graph", action="store_true",
                    help="N = 1: time the step as a replayed HIP graph (launch overhead out)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline figure: the CPU baseline legs, the "
                         "hot-column, grouped and analysed side entries, the config 3 / config 5 / "
                         "products bs 32 side lines and, for the CSR workloads, the kernel-timed "
                         "pass behind `roofline` (the --no-* options drop single parts of it); "
                         "without it the run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the C they left as DIR/C.npy (float32; a "
                         "fixed row sample of a C above 48 MiB)")
    args = ap.parse_args()
    global GRAPH
    GRAPH = args.graph
    if not args.full:
        args.no_cpu_baseline = args.no_hot_side = args.no_bsr_sides = True
        args.no_analysed_side = True
    if args.cpu_baseline_child:
        args.workload = args.workload or "products_csr"
        cpu_baseline_child(args)
        return

    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if local >= torch.cuda.device_count():
        raise SystemExit(f"LOCAL_RANK {local} but {torch.cuda.device_count()} GPU(s) visible")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if "WORLD_SIZE" in os.environ:
        # any torch.distributed launch (world 1 included: rehearses the N > 1
        # code path, its collectives and the max-over-ranks timing on one GPU)
        dist.init_process_group("nccl", device_id=dev)

    if args.workload is None:
        args.workload = "products_csr_k256" if world > 1 else "products_csr"
    W = WORKLOADS[args.workload]
    runner = {"csr": run_csr, "bsr": run_bsr, "hybrid": run_hybrid}[W["kind"]]
    weak = W["kind"] == "csr" and args.scaling == "weak"
    if weak and dist.is_initialized():
        runner = run_csr_weak
    rec, csr_inputs = runner(args, W, world, rank, dev, dist)
    if world == 1 and args.workload == "products_csr" and not args.no_bsr_sides:
        import torch
        torch.cuda.empty_cache()
        for key, wl in BSR_SIDES:
            _progress(f"side entry {key}: {wl}")
            rec[key] = bsr_side(args, wl, rank, dev, dist)

    if rank == 0:
        cpu = None
        if (csr_inputs is not None and world == 1 and not args.no_cpu_baseline):
            cpu = cpu_baseline(args, csr_inputs[2])
        out = {"metric": METRIC if args.workload == "products_csr" else
               f"SpMM GFLOP/s (2*nnz*K/t), {args.workload}",
               "value": round(rec.pop("value"), 2), "unit": "GFLOP/s", "n_gpus": world,
               "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": round(rec.pop("ms_per_step"), 4), "higher_is_better": True,
               # CSR: strong (the one graph, total work fixed) unless --scaling weak;
               # the BSR / hybrid configs are single-GPU (BASELINE configs 3, 5)
               "scaling": (("weak" if weak else "strong") if W["kind"] == "csr" else None),
               "vs_baseline": None}
        out.update(rec)
        rf = out.get("roofline") or {}
        if (rf.get("frac") or 0) > 1.0:  # never reached: every model above is bounded
            rf["note"] = "fraction above 1: the byte model is not the work"
        out["cpu_baseline"] = cpu
        print(json.dumps(out), flush=True)
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
