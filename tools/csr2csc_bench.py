#!/usr/bin/env python3
"""Device CSR transpose (spmm_csr2csc_dev) beside its alternatives.

    python tools/csr2csc_bench.py [--out profiles/csr2csc/bench.jsonl] [--rounds 3]

The products stand-in and the arxiv stand-in of bench.py (its WORKLOADS entries,
generator arguments and value seed), fp32 values. Per workload, interleaved for
--rounds rounds, each method 5 warm-up and 20 timed calls on the wall clock between
device synchronisations:
  device       ops.csr2csc (count, scan, radix passes, rows, gather; one synchronisation
               inside every call, which the time includes)
  host         prep.csr2csc at 16 threads (host arrays in, host arrays out: no copies)
  torch        torch's own route on the same GPU: rows by repeat_interleave,
               torch.sort(colind, stable=True), two gathers, bincount + cumsum
  product      one fp32 CSR product at K = 128 on the original matrix
  product_t    the same on the transposed matrix (B of the same shape: the stand-ins
               are square)
One JSON line per (workload, method, round) with ms per call; per workload one more
line, method "device_kernels", with the kernel times of one timed device call in
launch order (the handle's kernel timing). The device output is compared with the
torch route's (index arrays and value bits) before anything is timed. summary.json
beside it holds the medians over the rounds, the spread of the device rounds, and how
many K = 128 products one transpose costs.

Each workload runs in a child process of its own under a time limit; after a child
that fails or runs out of time nothing more is started.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench  # noqa: E402  (WORKLOADS; adds the package path)

CASES = ["products_csr", "arxiv_csr"]
STEPS, WARMUP, K = 20, 5, 128
HOST_THREADS = 16


def kernel_labels(n: int, count: int) -> list[str]:
    """Names of the kernels of one spmm_csr2csc_dev call, in launch order."""
    passes = 0 if n <= 1 else ((n - 1).bit_length() + 7) // 8
    names = ["col_count", "colptr_scan"]
    for j in range(passes):
        names += [f"pass{j}_digit_count", f"pass{j}_scan", f"pass{j}_scatter"]
    names += ["expand_rows", "gather"]
    return names if len(names) == count else [f"kernel{i}" for i in range(count)]


def timed(step, sync) -> float:
    """ms per call: WARMUP calls, then STEPS calls between two synchronisations."""
    for _ in range(WARMUP):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        step()
    sync()
    return (time.perf_counter() - t0) / STEPS * 1e3


def child(workload: str, rounds: int, out: str) -> None:
    import torch
    from spmm_hip import ops, prep
    W = bench.WORKLOADS[workload]
    dev = torch.device("cuda", 0)
    rp, ci = prep.powerlaw_csr(W["n"], W["nnz"], W["max_deg"], 2.3, 1234)  # bench.run_csr's matrix
    val = np.random.default_rng(2).uniform(-1, 1, ci.size).astype(np.float32)
    m, nnz = rp.size - 1, int(ci.size)
    d_rp, d_ci, d_v = (torch.from_numpy(a).to(dev) for a in (rp, ci, val))
    h = ops.Handle()

    def torch_route():
        rows = torch.repeat_interleave(torch.arange(m, device=dev, dtype=torch.int32),
                                       (d_rp[1:] - d_rp[:-1]).long(), output_size=nnz)
        order = torch.sort(d_ci, stable=True)[1]
        colptr = torch.zeros(m + 1, dtype=torch.int32, device=dev)
        colptr[1:] = torch.cumsum(torch.bincount(d_ci, minlength=m), 0)
        return colptr, rows[order], d_v[order]

    t_cp, t_ri, t_v = ops.csr2csc(d_rp, d_ci, d_v, m=m, n=m, nnz=nnz, handle=h)
    want = torch_route()
    torch.cuda.synchronize()
    if not (torch.equal(t_cp, want[0]) and torch.equal(t_ri, want[1]) and
            torch.equal(t_v.view(torch.int32), want[2].view(torch.int32))):
        raise SystemExit(f"{workload}: the device transpose differs from the torch route")
    del want
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    B = torch.rand((m, K), device=dev, generator=g) * 2 - 1
    C = torch.empty((m, K), device=dev)
    sync = torch.cuda.synchronize
    methods = {
        "device": (lambda: ops.csr2csc(d_rp, d_ci, d_v, m=m, n=m, nnz=nnz, handle=h), sync),
        "host": (lambda: prep.csr2csc(m, m, rp, ci, val), lambda: None),
        "torch": (torch_route, sync),
        "product": (lambda: ops.csrmm(d_rp, d_ci, d_v, B, m=m, n=K, k=m, ldb=K, C=C, ldc=K,
                                      handle=h), sync),
        "product_t": (lambda: ops.csrmm(t_cp, t_ri, t_v, B, m=m, n=K, k=m, ldb=K, C=C, ldc=K,
                                        handle=h), sync),
    }
    with open(out, "a") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)

        for rnd in range(rounds):
            for name, (step, sy) in methods.items():
                emit(dict(workload=workload, method=name, round=rnd,
                          ms_per_call=round(timed(step, sy), 5), m=m, nnz=nnz, steps=STEPS,
                          warmup=WARMUP, K=K if name.startswith("product") else None,
                          host_threads=HOST_THREADS if name == "host" else None))
        h.set_timing(True)
        h.kernel_times()
        methods["device"][0]()
        torch.cuda.synchronize()
        h.set_timing(False)
        kt = h.kernel_times()
        emit(dict(workload=workload, method="device_kernels", round=0, m=m, nnz=nnz,
                  kernel_ms=dict(zip(kernel_labels(m, len(kt)), [round(t, 5) for t in kt])),
                  kernel_ms_total=round(sum(kt), 5)))
    h.close()


def summarise(path: str) -> list[dict]:
    rows: dict = {}
    kernels: dict = {}
    with open(path) as f:
        for line in f:
            r = json.loads(line)
            if r["method"] == "device_kernels":
                kernels[r["workload"]] = r
            else:
                rows.setdefault(r["workload"], {}).setdefault(r["method"], []).append(
                    r["ms_per_call"])
    out = []
    for w, d in rows.items():
        med = {k: statistics.median(v) for k, v in d.items()}
        s = dict(workload=w, rounds=len(d.get("device", [])),
                 **{f"{k}_ms_median": round(v, 5) for k, v in med.items()})
        if "device" in d:
            s["device_round_spread_ms"] = round(max(d["device"]) - min(d["device"]), 5)
        if "device" in med and "torch" in med:
            s["device_over_torch"] = round(med["device"] / med["torch"], 4)
        if "device" in med and "host" in med:
            s["host_over_device"] = round(med["host"] / med["device"], 2)
        if "device" in med and "product" in med:
            s["products_per_transpose"] = round(med["device"] / med["product"], 2)
        if "product" in med and "product_t" in med:
            s["product_t_over_product"] = round(med["product_t"] / med["product"], 4)
        if w in kernels:
            s["device_kernel_ms"] = kernels[w]["kernel_ms"]
            s["device_kernel_ms_total"] = kernels[w]["kernel_ms_total"]
        out.append(s)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr2csc", "bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per workload")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.rounds < 3:
        raise SystemExit("at least three interleaved rounds")
    if args.child:
        child(args.child, args.rounds, args.out)
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").close()
    env = dict(os.environ, OMP_NUM_THREADS=str(HOST_THREADS))
    for workload in CASES:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__),
               "--child", workload, "--rounds", str(args.rounds), "--out", args.out]
        rc = subprocess.run(cmd, env=env).returncode
        if rc != 0:
            raise SystemExit(f"{workload}: the measuring process ended with status {rc}; "
                             "nothing more is started")
    summary = summarise(args.out)
    with open(os.path.join(os.path.dirname(args.out), "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    for s in summary:
        print(json.dumps(s))


if __name__ == "__main__":
    main()
