#!/usr/bin/env python3
"""The edge softmax (spmm_edge_softmax_csr_f32 / _bwd_csr_f32) beside the torch composite
(DESIGN.md §4i).

    python tools/edge_softmax_bench.py [--out profiles/edge_softmax/bench.jsonl] [--rounds 3]

The products, reddit and arxiv stand-ins of bench.py (its WORKLOADS entries, generator
arguments and seed; only the row pointer is used), and two small patterns of the same nnz
for the cost of degree skew: "skew" (one row of 70,001 positions beside 10,000 rows of 7)
and "flat" (the same 140,001 positions in rows of 7). Per pattern, interleaved for
--rounds rounds:
  fwd / bwd    ops.edge_softmax / ops.edge_softmax_bwd, 5 warm-up and 20 timed calls with
               the handle's kernel timing on: ms per call = the mean of the 20 kernel times
               (hipEvents around the one kernel), and the wall clock between
               synchronisations beside it
  torch        scatter_reduce(amax) + gather + exp + index_add_ + gather + divide on the
               same x, the row of every position made once outside the timing; wall clock,
               2 warm-up and 5 timed calls
One JSON line per (pattern, method, round). The kernel lines carry the bytes of the model
    4 (m + 1) + 8 nnz        (the row pointer, x read once, y written once;
                              the backward reads a third array: 4 (m + 1) + 12 nnz)
and what fraction of the plain streaming rate (the best read_GBps of
profiles/r01_hbm_peak.jsonl) they make at the kernel's time. The device output is compared
with the torch composite's before anything is timed. summary.json beside the output holds
the medians over the rounds, the round spread, and torch over fwd.

Each pattern runs in a child process of its own under a time limit; after a child that
fails or runs out of time nothing more is started.
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

CASES = ["skew", "flat", "arxiv_csr", "products_csr", "reddit_bsr32"]
STEPS, WARMUP = 20, 5
TORCH_STEPS, TORCH_WARMUP = 5, 2


def stream_rate() -> float:
    """Bytes per second of a plain read stream, as the project measured it."""
    best = 0.0
    with open(os.path.join(ROOT, "profiles", "r01_hbm_peak.jsonl")) as f:
        for line in f:
            best = max(best, json.loads(line)["read_GBps"])
    return best * 1e9


def row_pointer(case: str) -> np.ndarray:
    from spmm_hip import prep
    if case in ("skew", "flat"):
        nnz = 70001 + 7 * 10000
        lens = [70001] + [7] * 10000 if case == "skew" else [7] * (nnz // 7) + [nnz % 7]
        return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    W = bench.WORKLOADS[case]
    if W["kind"] == "csr":
        return prep.powerlaw_csr(W["n"], W["nnz"], W["max_deg"], 2.3, 1234)[0]
    return prep.community_csr(W["n"], W["avg_deg"], W["cmin"], W["cmax"], W["p_in"], 1234)[0]


def child(case: str, rounds: int, out: str) -> None:
    import torch
    from spmm_hip import ops
    dev = torch.device("cuda", 0)
    rp = row_pointer(case)
    m, nnz = rp.size - 1, int(rp[-1])
    d_rp = torch.from_numpy(rp).to(dev)
    rows = torch.repeat_interleave(torch.arange(m, device=dev), (d_rp[1:] - d_rp[:-1]).long(),
                                   output_size=nnz)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    x = torch.randn(nnz, device=dev, generator=g) * 3
    gy = torch.randn(nnz, device=dev, generator=g)
    y, gx = torch.empty_like(x), torch.empty_like(x)
    h = ops.Handle()
    sync = torch.cuda.synchronize
    rate = stream_rate()

    def torch_route():
        mx = torch.full((m,), -torch.inf, device=dev).scatter_reduce(0, rows, x, "amax")
        e = torch.exp(x - mx[rows])
        s = torch.zeros(m, device=dev).index_add_(0, rows, e)
        return e / s[rows]

    def fwd():
        return ops.edge_softmax(d_rp, x, out=y, handle=h)

    def bwd():
        return ops.edge_softmax_bwd(d_rp, y, gy, out=gx, handle=h)

    fwd()
    want = torch_route()
    sync()
    worst = float(((y - want).abs() / want.clamp_min(1e-30)).max())
    if not worst <= 1e-4:
        raise SystemExit(f"{case}: ops.edge_softmax differs from the torch composite by {worst}")
    del want

    def kernel_timed(step, nbytes):
        for _ in range(WARMUP):
            step()
        sync()
        h.set_timing(True)
        h.kernel_times()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            step()
        sync()
        wall = (time.perf_counter() - t0) / STEPS * 1e3
        h.set_timing(False)
        kt = h.kernel_times()
        assert len(kt) == STEPS, len(kt)
        ms = sum(kt) / STEPS
        return dict(kernel_ms=round(ms, 5), kernel_ms_min=round(min(kt), 5),
                    wall_ms_per_call=round(wall, 5), model_bytes=nbytes,
                    fraction_of_stream=round(nbytes / (ms * 1e-3) / rate, 4))

    def wall_timed(step):
        for _ in range(TORCH_WARMUP):
            step()
        sync()
        t0 = time.perf_counter()
        for _ in range(TORCH_STEPS):
            step()
        sync()
        return dict(wall_ms_per_call=round((time.perf_counter() - t0) / TORCH_STEPS * 1e3, 5))

    with open(out, "a") as f:
        for rnd in range(rounds):
            for name, res in (("fwd", lambda: kernel_timed(fwd, 4 * (m + 1) + 8 * nnz)),
                              ("bwd", lambda: kernel_timed(bwd, 4 * (m + 1) + 12 * nnz)),
                              ("torch", lambda: wall_timed(torch_route))):
                rec = dict(pattern=case, method=name, round=rnd, m=m, nnz=nnz, **res())
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(json.dumps(rec), flush=True)
    h.close()


def summarise(path: str) -> list[dict]:
    by: dict = {}
    with open(path) as f:
        for line in f:
            r = json.loads(line)
            by.setdefault(r["pattern"], {}).setdefault(r["method"], []).append(r)
    out = []
    for pat, d in by.items():
        s = dict(pattern=pat, m=d["fwd"][0]["m"], nnz=d["fwd"][0]["nnz"], rounds=len(d["fwd"]))
        for meth in ("fwd", "bwd"):
            ks = [r["kernel_ms"] for r in d[meth]]
            s[meth + "_kernel_ms_median"] = round(statistics.median(ks), 5)
            s[meth + "_kernel_ms_round_spread"] = round(max(ks) - min(ks), 5)
            s[meth + "_wall_ms_median"] = round(
                statistics.median(r["wall_ms_per_call"] for r in d[meth]), 5)
            s[meth + "_fraction_of_stream"] = round(
                statistics.median(r["fraction_of_stream"] for r in d[meth]), 4)
        s["torch_wall_ms_median"] = round(
            statistics.median(r["wall_ms_per_call"] for r in d["torch"]), 5)
        s["torch_over_fwd_wall"] = round(s["torch_wall_ms_median"] / s["fwd_wall_ms_median"], 3)
        out.append(s)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_softmax", "bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per pattern")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.rounds < 3:
        raise SystemExit("at least three interleaved rounds")
    if args.child:
        child(args.child, args.rounds, args.out)
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").close()
    for case in args.cases.split(","):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__),
               "--child", case, "--rounds", str(args.rounds), "--out", args.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit(f"{case}: the measuring process ended with status {rc}; "
                             "nothing more is started")
    summary = summarise(args.out)
    with open(os.path.join(os.path.dirname(args.out), "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    for s in summary:
        print(json.dumps(s))


if __name__ == "__main__":
    main()
