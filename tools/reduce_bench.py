#!/usr/bin/env python3
"""The max / min reducers (ops.csrmm_reduce, ops.csrmm_reduce_bwd) beside two
yardsticks: the sum product on the same matrix, and what a user does today in torch.

    python tools/reduce_bench.py [--out profiles/reduce/bench.jsonl] [--rounds 3]
    python tools/reduce_bench.py --summarise profiles/reduce/bench.jsonl
    python tools/reduce_bench.py --table profiles/reduce/summary.json

The arxiv, reddit and products stand-ins of bench.py (its WORKLOADS entries, generator
arguments and seed) at n = 32, 64, 128, 256, with val NULL and given. Per pattern, n and val,
interleaved for --rounds rounds:
  fwd_arg / fwd_noarg   ops.csrmm_reduce(reduce="max") with and without the winning positions
  bwd                   ops.csrmm_reduce_bwd on A^T (ops.csr2csc once, outside the timing)
  sum_fwd / sum_bwd     yardstick 1: ops.csrmm on A, and on A^T with the permuted values (the
                        sum product and its gradient; with val NULL the values are ones)
  torch_fwd             yardstick 2: T = B[col] (* val[:, None]), then
                        out.scatter_reduce_(0, row index, T, "amax") with a prebuilt row
                        index: an nnz x n temporary and float atomics, no positions. Timed
                        where the temporary fits in the free device memory; its peak
                        allocation is recorded. A call of more than 2 s is timed once
                        (its second call) and not in every round.
All are timed the same way: the wall clock between two device synchronisations around
`steps` calls after the warm-up calls, steps chosen per method so that its window is about
0.2 s (at least 1 call for the torch route, 3 for the others). One JSON line per (pattern, n,
val, method, round). Before anything is timed the forward is compared with the torch route on
the rows that are not empty, bit for bit.

--summarise writes summary.json beside the lines: per (pattern, n, val) the medians over the
rounds, each method's round-to-round spread (max - min over the median), and per reducer
entry its time over the sum product's (time ratio) beside the ratio of the algorithmic bytes
of the two (byte ratio: the forward reads the same gathered rows and writes 4 m n more for
arg; the backward gathers two rows per nonzero where the product gathers one), and whether
the time ratio exceeds the byte ratio by more than the larger spread.

Each pattern runs in a child process of its own under a time limit; after a child that fails
or runs out of time nothing more is started.
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

import bench  # noqa: E402  (WORKLOADS; adds the package path)

CASES = ["arxiv_csr", "reddit_bsr32", "products_csr"]
WIDTHS = [32, 64, 128, 256]
METHODS = ["fwd_arg", "fwd_noarg", "bwd", "sum_fwd", "sum_bwd", "torch_fwd"]
WARMUP, MIN_STEPS, MAX_STEPS, WINDOW_S = 2, 3, 200, 0.2
TORCH_CALL_MS = 2000.0  # a torch route slower than this per call is timed once, not per round


def pattern(case: str):
    from spmm_hip import prep
    W = bench.WORKLOADS[case]
    if W["kind"] == "csr":
        return prep.powerlaw_csr(W["n"], W["nnz"], W["max_deg"], 2.3, 1234)
    return prep.community_csr(W["n"], W["avg_deg"], W["cmin"], W["cmax"], W["p_in"], 1234)


def model_bytes(m: int, nnz: int, n: int, has_val: bool) -> dict:
    """Algorithmic bytes per call (every array once, a gathered row per nonzero)."""
    v = 4 * nnz if has_val else 0
    return {
        "sum_fwd": nnz * (8 + 4 * n) + 4 * m * n + 4 * (m + 1),
        "fwd_noarg": nnz * (4 + 4 * n) + v + 4 * m * n + 4 * (m + 1),
        "fwd_arg": nnz * (4 + 4 * n) + v + 8 * m * n + 4 * (m + 1),
        "sum_bwd": nnz * (8 + 4 * n) + 4 * m * n + 4 * (m + 1),
        "bwd": nnz * (8 + 8 * n) + v + 4 * m * n + 4 * (m + 1),
    }


def child(case: str, rounds: int, out: str, widths) -> None:
    import torch
    from spmm_hip import ops
    dev = torch.device("cuda", 0)
    rp, ci = pattern(case)
    m, nnz = rp.size - 1, int(ci.size)
    d_rp, d_ci = torch.from_numpy(rp).to(dev), torch.from_numpy(ci).to(dev)
    h = ops.Handle()
    sync = torch.cuda.synchronize
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    val = torch.rand(nnz, device=dev, generator=gen) * 2 - 1
    ones = torch.ones(nnz, device=dev)
    trp, tci, perm = ops.csr2csc(d_rp, d_ci, m=m, n=m, nnz=nnz, return_perm=True, handle=h)
    vt, rows = val[perm.long()], torch.repeat_interleave(
        torch.arange(m, device=dev), (d_rp[1:] - d_rp[:-1]).long())
    ci_long = d_ci.long()
    nonempty = (d_rp[1:] > d_rp[:-1])
    sync()

    def window(step, steps, warmup=WARMUP):
        for _ in range(warmup):
            step()
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        sync()
        return (time.perf_counter() - t0) / steps * 1e3

    with open(out, "a") as f:
        for n in widths:
            B = torch.rand((m, n), device=dev, generator=gen) * 2 - 1
            dC = torch.rand((m, n), device=dev, generator=gen) * 2 - 1
            C, C0, S, dB = (torch.empty((m, n), device=dev) for _ in range(4))
            arg = torch.empty((m, n), dtype=torch.int32, device=dev)
            free = torch.cuda.mem_get_info()[0]
            fits = nnz * n * 4 * 1.25 + m * n * 4 < free
            for has_val in (False, True):
                v = val if has_val else None
                idx = rows[:, None].expand(nnz, n)
                tout = torch.empty((m, n), device=dev) if fits else None

                def fwd_arg():
                    ops.csrmm_reduce(d_rp, d_ci, v, B, reduce="max", m=m, n=n, k=m, C=C, arg=arg,
                                     handle=h)

                def fwd_noarg():
                    ops.csrmm_reduce(d_rp, d_ci, v, B, reduce="max", m=m, n=n, k=m, C=C0,
                                     return_arg=False, handle=h)

                def bwd():
                    ops.csrmm_reduce_bwd(trp, tci, perm, v, dC, arg, k=m, n=n, m=m, dB=dB, handle=h)

                def sum_fwd():
                    ops.csrmm(d_rp, d_ci, val if has_val else ones, B, m=m, n=n, k=m, ldb=n, C=S,
                              ldc=n, handle=h)

                def sum_bwd():
                    ops.csrmm(trp, tci, vt if has_val else ones, dC, m=m, n=n, k=m, ldb=n, C=S,
                              ldc=n, handle=h)

                def torch_fwd():
                    T = B[ci_long]
                    if has_val:
                        T *= val[:, None]
                    tout.fill_(float("-inf"))
                    tout.scatter_reduce_(0, idx, T, "amax", include_self=False)

                routes = dict(fwd_arg=fwd_arg, fwd_noarg=fwd_noarg, bwd=bwd, sum_fwd=sum_fwd,
                              sum_bwd=sum_bwd)
                fwd_arg()
                fwd_noarg()
                sync()
                if not torch.equal(C, C0):
                    raise SystemExit(f"{case} n={n}: C differs with and without arg")
                peak = None
                if fits:
                    torch_fwd()  # the first call: code objects, the allocator's blocks
                    sync()
                    if not torch.equal(C[nonempty], tout[nonempty]):
                        raise SystemExit(f"{case} n={n}: the reducer differs from torch's scatter")
                    torch.cuda.reset_peak_memory_stats()
                    base_alloc = torch.cuda.memory_allocated()
                    second = window(torch_fwd, 1, 0)
                    peak = torch.cuda.max_memory_allocated() - base_alloc
                    if second <= TORCH_CALL_MS:
                        routes["torch_fwd"] = torch_fwd
                    else:  # too slow to repeat in every round: its one warm call stands
                        rec = dict(pattern=case, m=m, nnz=nnz, n=n, val=has_val,
                                   method="torch_fwd", round=-2, steps=1,
                                   wall_ms_per_call=round(second, 5), peak_bytes=int(peak))
                        f.write(json.dumps(rec) + "\n")
                        print(json.dumps(rec), flush=True)
                else:
                    rec = dict(pattern=case, m=m, nnz=nnz, n=n, val=has_val, method="torch_fwd",
                               round=-1, does_not_fit=True, temporary_bytes=nnz * n * 4,
                               free_bytes=int(free))
                    f.write(json.dumps(rec) + "\n")
                steps = {}
                for nm, step in routes.items():
                    lo, wu = (1, 0) if nm == "torch_fwd" else (MIN_STEPS, WARMUP)
                    t1 = window(step, 1, wu)
                    steps[nm] = int(min(MAX_STEPS, max(lo, WINDOW_S * 1e3 / t1)))
                for rnd in range(rounds):
                    for nm, step in routes.items():
                        wu = 0 if nm == "torch_fwd" else WARMUP
                        rec = dict(pattern=case, m=m, nnz=nnz, n=n, val=has_val, method=nm,
                                   round=rnd, steps=steps[nm],
                                   wall_ms_per_call=round(window(step, steps[nm], wu), 5))
                        if nm == "torch_fwd":
                            rec["peak_bytes"] = int(peak)
                        f.write(json.dumps(rec) + "\n")
                        f.flush()
                        print(json.dumps(rec), flush=True)
                del tout
            del B, dC, C, C0, S, dB, arg
            torch.cuda.empty_cache()
    h.close()


def summarise(path: str) -> list[dict]:
    by: dict = {}
    with open(path) as f:
        for line in f:
            r = json.loads(line)
            by.setdefault((r["pattern"], r["n"], r["val"]), {}).setdefault(r["method"], []).append(r)
    out = []
    for (pat, n, has_val), meth in by.items():
        r0 = meth["fwd_arg"][0]
        s = dict(pattern=pat, m=r0["m"], nnz=r0["nnz"], n=n, val=has_val,
                 rounds=len(meth["fwd_arg"]))
        spread = {}
        for nm in METHODS:
            rs = [r for r in meth.get(nm, []) if r["round"] >= 0]
            if not rs:
                if nm == "torch_fwd":
                    once = [r for r in meth.get(nm, []) if r["round"] == -2]
                    s["torch_fwd_fits"] = bool(once)
                    if once:  # one warm call, no rounds: no spread
                        s["torch_fwd_ms"] = once[0]["wall_ms_per_call"]
                        s["torch_fwd_rounds"] = 0
                        s["torch_fwd_peak_bytes"] = once[0]["peak_bytes"]
                        s["torch_over_fwd_arg"] = round(s["torch_fwd_ms"] / s["fwd_arg_ms"], 3)
                continue
            ts = [r["wall_ms_per_call"] for r in rs]
            med = statistics.median(ts)
            s[nm + "_ms"] = round(med, 5)
            spread[nm] = (max(ts) - min(ts)) / med
            s[nm + "_round_spread"] = round(spread[nm], 4)
            if nm == "torch_fwd":
                s["torch_fwd_fits"] = True
                s["torch_fwd_peak_bytes"] = rs[0]["peak_bytes"]
                s["torch_over_fwd_arg"] = round(med / s["fwd_arg_ms"], 3)
        mb = model_bytes(r0["m"], r0["nnz"], n, has_val)
        for nm, ref in (("fwd_arg", "sum_fwd"), ("fwd_noarg", "sum_fwd"), ("bwd", "sum_bwd")):
            tr, br = s[nm + "_ms"] / s[ref + "_ms"], mb[nm] / mb[ref]
            s[nm + "_time_ratio"] = round(tr, 3)
            s[nm + "_byte_ratio"] = round(br, 3)
            s[nm + "_above_bytes_by_more_than_the_spread"] = bool(
                tr > br * (1 + max(spread[nm], spread[ref])))
        out.append(s)
    return out


def write_summary(path: str) -> None:
    summary = summarise(path)
    with open(os.path.join(os.path.dirname(os.path.abspath(path)), "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    for s in summary:
        print(json.dumps(s))


def table(path: str) -> str:
    """The markdown table of DESIGN.md §4l from a summary.json."""
    with open(path) as f:
        rows = json.load(f)
    names = {"arxiv_csr": "arxiv", "products_csr": "products", "reddit_bsr32": "reddit"}

    def cell(s, nm, ref):
        flag = " **above bytes**" if s[nm + "_above_bytes_by_more_than_the_spread"] else ""
        spread = max(s[nm + "_round_spread"], s[ref + "_round_spread"])
        return (f"{s[nm + '_ms']:.3f} ({s[nm + '_time_ratio']:.2f}x of {s[ref + '_ms']:.3f}; bytes "
                f"{s[nm + '_byte_ratio']:.2f}x; spread {spread:.2f}){flag}")

    out = ["| graph | n | val | forward with arg: ms (÷ sum product; byte ratio; spread) | "
           "forward without arg | backward: ms (÷ sum product on Aᵀ; byte ratio; spread) | "
           "torch gather + scatter_reduce_: ms (÷ forward with arg), peak |",
           "|---|---|---|---|---|---|---|"]
    for s in rows:
        if s.get("torch_fwd_fits"):
            once = ", one call" if s.get("torch_fwd_rounds") == 0 else ""
            torch_cell = (f"{s['torch_fwd_ms']:.1f} ({s['torch_over_fwd_arg']:.1f}x{once}), "
                          f"{s['torch_fwd_peak_bytes'] / 2 ** 30:.1f} GiB")
        else:
            torch_cell = "does not fit"
        out.append(f"| {names.get(s['pattern'], s['pattern'])} | {s['n']} | "
                   f"{'given' if s['val'] else 'NULL'} | {cell(s, 'fwd_arg', 'sum_fwd')} | "
                   f"{cell(s, 'fwd_noarg', 'sum_fwd')} | {cell(s, 'bwd', 'sum_bwd')} | "
                   f"{torch_cell} |")
    return "\n".join(out)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduce", "bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=500, help="seconds per pattern")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--widths", default=",".join(str(n) for n in WIDTHS))
    ap.add_argument("--append", action="store_true", help="keep the lines --out already holds")
    ap.add_argument("--summarise", default=None, metavar="JSONL",
                    help="write summary.json beside these lines and measure nothing")
    ap.add_argument("--table", default=None, metavar="SUMMARY_JSON",
                    help="print DESIGN.md §4l's table from a summary.json and measure nothing")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.table:
        print(table(args.table))
        return
    if args.summarise:
        write_summary(args.summarise)
        return
    if args.rounds < 3:
        raise SystemExit("at least three interleaved rounds")
    widths = [int(v) for v in args.widths.split(",")]
    if args.child:
        child(args.child, args.rounds, args.out, widths)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if not args.append:
        open(args.out, "w").close()
    for case in args.cases.split(","):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__),
               "--child", case, "--rounds", str(args.rounds), "--out", args.out,
               "--widths", args.widths]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit(f"{case}: the measuring process ended with status {rc}; "
                             "nothing more is started")
    write_summary(args.out)


if __name__ == "__main__":
    main()
