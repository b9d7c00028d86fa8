#!/usr/bin/env python3
"""The CSR-sampled dense-dense product (spmm_sddmm_csr_f32) beside the forward product
and a torch route.

    python tools/sddmm_bench.py [--out profiles/sddmm/bench.jsonl] [--rounds 3]

The products stand-in and the arxiv stand-in of bench.py (its WORKLOADS entries,
generator arguments and value seed), at n = 64, 128 and 256 columns of X and Y. Per
(workload, n), interleaved for --rounds rounds, on the wall clock between device
synchronisations:
  sddmm        ops.sddmm on the pattern (X of m x n, Y of m x n: the stand-ins are
               square), 5 warm-up and 20 timed calls
  csrmm        ops.csrmm on the same matrix and n (the forward product, which gathers
               the same Y / B rows), 5 warm-up and 20 timed calls
  torch        a gather-multiply-sum, (X[rows] * Y[cols]).sum(1), in chunks of 2^22
               positions so that the two gathered operands fit memory; the row of every
               position and the int64 columns are made once, outside the timing; 2
               warm-up and 5 timed calls
One JSON line per (workload, n, method, round) with ms per call; per (workload, n) one
more line per kernel method, "sddmm_kernel" / "csrmm_kernel", with the handle's kernel
time of one call, and for sddmm the bytes of the model
    nnz * (4 n + 8) + 4 m n + 4 (m + 1)
(one Y-row gather per nonzero, 8 bytes of index and output, every X row once, the row
pointer) and what fraction of 8 TB/s they make at that kernel time. The device output
is compared with the torch route's (norm-wise, 1e-5) before anything is timed.
summary.json beside it holds the medians over the rounds and the two ratios the design
quotes: sddmm over csrmm and torch over sddmm.

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
NS = [64, 128, 256]
STEPS, WARMUP = 20, 5
TORCH_STEPS, TORCH_WARMUP = 5, 2
CHUNK = 1 << 22
PEAK_BYTES_PER_S = 8e12


def model_bytes(m: int, nnz: int, n: int) -> int:
    return nnz * (4 * n + 8) + 4 * m * n + 4 * (m + 1)


def timed(step, sync, steps, warmup) -> float:
    for _ in range(warmup):
        step()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync()
    return (time.perf_counter() - t0) / steps * 1e3


def child(workload: str, rounds: int, out: str) -> None:
    import torch
    from spmm_hip import ops, prep
    W = bench.WORKLOADS[workload]
    dev = torch.device("cuda", 0)
    rp, ci = prep.powerlaw_csr(W["n"], W["nnz"], W["max_deg"], 2.3, 1234)  # bench.run_csr's matrix
    val = np.random.default_rng(2).uniform(-1, 1, ci.size).astype(np.float32)
    m, nnz = rp.size - 1, int(ci.size)
    d_rp, d_ci, d_v = (torch.from_numpy(a).to(dev) for a in (rp, ci, val))
    rows = torch.repeat_interleave(torch.arange(m, device=dev),
                                   (d_rp[1:] - d_rp[:-1]).long(), output_size=nnz)
    cols = d_ci.long()
    h = ops.Handle()
    sync = torch.cuda.synchronize
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    with open(out, "a") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)

        for n in NS:
            X = torch.rand((m, n), device=dev, generator=g) * 2 - 1
            Y = torch.rand((m, n), device=dev, generator=g) * 2 - 1
            C = torch.empty((m, n), device=dev)
            o = torch.empty(nnz, device=dev)
            ot = torch.empty(nnz, device=dev)

            def torch_route():
                for a in range(0, nnz, CHUNK):
                    r, c = rows[a:a + CHUNK], cols[a:a + CHUNK]
                    torch.sum(X[r] * Y[c], 1, out=ot[a:a + CHUNK])
                return ot

            def sddmm():
                return ops.sddmm(d_rp, d_ci, X, Y, m=m, n=n, k=m, out=o, handle=h)

            def csrmm():
                return ops.csrmm(d_rp, d_ci, d_v, Y, m=m, n=n, k=m, ldb=n, C=C, ldc=n, handle=h)

            sddmm()
            torch_route()
            sync()
            # |error| <= 1e-5 sum |x||y|, and sum |x||y| <= n for entries in (-1, 1)
            worst = float((o - ot).abs().max())
            if not worst <= 1e-5 * n:
                raise SystemExit(f"{workload} n={n}: ops.sddmm differs from the torch route "
                                 f"by {worst}")
            methods = {"sddmm": (sddmm, STEPS, WARMUP), "csrmm": (csrmm, STEPS, WARMUP),
                       "torch": (torch_route, TORCH_STEPS, TORCH_WARMUP)}
            for rnd in range(rounds):
                for name, (step, steps, warmup) in methods.items():
                    emit(dict(workload=workload, n=n, method=name, round=rnd,
                              ms_per_call=round(timed(step, sync, steps, warmup), 5), m=m,
                              nnz=nnz, steps=steps, warmup=warmup))
            for name, step in (("sddmm", sddmm), ("csrmm", csrmm)):
                h.set_timing(True)
                h.kernel_times()
                step()
                sync()
                h.set_timing(False)
                kt = h.kernel_times()
                rec = dict(workload=workload, n=n, method=name + "_kernel", round=0, m=m, nnz=nnz,
                           kernel_ms=round(sum(kt), 5), kernels=len(kt))
                if name == "sddmm":
                    b = model_bytes(m, nnz, n)
                    rec["model_bytes"] = b
                    rec["fraction_of_8TBs"] = round(b / (sum(kt) * 1e-3) / PEAK_BYTES_PER_S, 4)
                emit(rec)
            del X, Y, C, o, ot
            torch.cuda.empty_cache()
    h.close()


def summarise(path: str) -> list[dict]:
    rows: dict = {}
    kernels: dict = {}
    with open(path) as f:
        for line in f:
            r = json.loads(line)
            key = (r["workload"], r["n"])
            if r["method"].endswith("_kernel"):
                kernels.setdefault(key, {})[r["method"]] = r
            else:
                rows.setdefault(key, {}).setdefault(r["method"], []).append(r["ms_per_call"])
    out = []
    for (w, n), d in rows.items():
        med = {k: statistics.median(v) for k, v in d.items()}
        s = dict(workload=w, n=n, rounds=len(d.get("sddmm", [])),
                 **{f"{k}_ms_median": round(v, 5) for k, v in med.items()})
        if "sddmm" in d:
            s["sddmm_round_spread_ms"] = round(max(d["sddmm"]) - min(d["sddmm"]), 5)
        if "sddmm" in med and "csrmm" in med:
            s["sddmm_over_csrmm"] = round(med["sddmm"] / med["csrmm"], 4)
        if "sddmm" in med and "torch" in med:
            s["torch_over_sddmm"] = round(med["torch"] / med["sddmm"], 3)
        for name, r in kernels.get((w, n), {}).items():
            s[name + "_ms"] = r["kernel_ms"]
            if "model_bytes" in r:
                s["model_bytes"] = r["model_bytes"]
                s["fraction_of_8TBs"] = r["fraction_of_8TBs"]
        out.append(s)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sddmm", "bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=540, help="seconds per workload")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.rounds < 3:
        raise SystemExit("at least three interleaved rounds")
    if args.child:
        child(args.child, args.rounds, args.out)
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").close()
    for workload in CASES:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__),
               "--child", workload, "--rounds", str(args.rounds), "--out", args.out]
        rc = subprocess.run(cmd).returncode
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
