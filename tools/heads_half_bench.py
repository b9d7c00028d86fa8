#!/usr/bin/env python3
"""The multi-head sampled product and CSR product on fp16 and bf16 features
(ops.sddmm_heads / ops.csrmm_heads on half tensors) beside the fp32 entries
on the same graph, timed in the same session.

    python tools/heads_half_bench.py [--out profiles/heads_half/bench.jsonl] [--rounds 3]
    python tools/heads_half_bench.py --table profiles/heads_half/summary.json   

The arxiv, products and reddit stand-ins of bench.py (its WORKLOADS entries, generator
arguments and seed) at heads x d = 8x8, 8x16, 4x32 and 8x64. Per graph, shape and op the
routes
  fp32   the fp32 entry on (X, Y) / (val, B)
  fp16   the fp16 entry on the operands rounded to binary16
  bf16   the bf16 entry on the operands rounded to bfloat16
run interleaved for --rounds rounds (at least three), each round 5 warm-up and 20 timed
calls (bench.timed_loop): the wall clock between two device synchronisations around the
timed calls, and the handle's kernel time (event pairs around every launch, in a pass of
the same 20 calls right after). Edge values, outVal and C are fp32 on every route. For the
product the half routes are timed once more with the cast autograd.spmm_heads adds
(C.to(dtype), a pass over m heads d elements): wall_ms_with_cast.

Before anything is timed each half route is compared bit for bit with the fp32 entry on its
own operands widened (.float()). One JSON line per (graph, heads, d, op, dtype, round) with
the model bytes and the vector width launched (the last template argument of the recorded
kernel: columns per load for the product, 1 = one 8-byte / 16-byte chunk load for the
sampled product). summary.json beside the output holds, per (graph, shape, op), each
route's median kernel time and wall time over the rounds, its round-to-round spread
((max - min) / median of the kernel time), fp32 over half, and whether the half route is
ahead of fp32 by more than the larger of the two spreads.

Model bytes per call (compulsory traffic, every gathered row counted once per nonzero):
  sddmm  nnz heads (e d + 4) + 4 nnz + e m heads d + 4 (m + 1)
         (the gathered Y slice and the output per nonzero and head, the index per nonzero,
         X once, the row pointer)
  csrmm  nnz heads (e d + 4) + 4 nnz + 4 m heads d + 4 (m + 1)
         (the gathered B slice and val[p, h], the index, C, the row pointer)
with e the feature element size: 4, or 2 for fp16 / bf16.

Each graph runs in a child process of its own under a time limit; after a child that fails
or runs out of time nothing more is started.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (WORKLOADS, timed_loop; adds the package path)

CASES = ["arxiv_csr", "products_csr", "reddit_bsr32"]
SHAPES = [(8, 8), (8, 16), (4, 32), (8, 64)]
OPS = ["sddmm", "csrmm"]
DTYPES = ["fp32", "fp16", "bf16"]
WARMUP, STEPS = 5, 20


def pattern(case: str):
    from spmm_hip import prep
    W = bench.WORKLOADS[case]
    if W["kind"] == "csr":
        return prep.powerlaw_csr(W["n"], W["nnz"], W["max_deg"], 2.3, 1234)
    return prep.community_csr(W["n"], W["avg_deg"], W["cmin"], W["cmax"], W["p_in"], 1234)


def model_bytes(op: str, m: int, nnz: int, heads: int, d: int, esize: int) -> int:
    per = nnz * heads * (esize * d + 4) + 4 * nnz + 4 * (m + 1)
    return per + (esize if op == "sddmm" else 4) * m * heads * d


def launched_vec(keys) -> int:
    """The last literal template argument of the one kernel a call recorded."""
    (key,) = keys
    args = key[key.rindex("I"):]
    lit = args[args.rindex("L"):]
    return int(lit[2:lit.index("E")])


def child(case: str, rounds: int, out: str, shapes) -> None:
    import torch
    from spmm_hip import ops
    dev = torch.device("cuda", 0)
    rp, ci = pattern(case)
    m, nnz = rp.size - 1, int(ci.size)
    d_rp, d_ci = torch.from_numpy(rp).to(dev), torch.from_numpy(ci).to(dev)
    h = ops.Handle()
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    types = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
    with open(out, "a") as f:
        for heads, d in shapes:
            H32 = torch.rand((m, heads, d), device=dev, generator=gen) * 2 - 1
            H = {dt: H32.to(ty) for dt, ty in types.items()}
            val = torch.rand((nnz, heads), device=dev, generator=gen)
            e = torch.empty((nnz, heads), device=dev)
            C = torch.empty((m, heads, d), device=dev)
            half_out = {dt: torch.empty((m, heads, d), device=dev, dtype=ty)
                        for dt, ty in types.items() if dt != "fp32"}

            def sddmm(dt):
                return lambda: ops.sddmm_heads(d_rp, d_ci, H[dt], H[dt], m=m, k=m, out=e, handle=h)

            def csrmm(dt):
                return lambda: ops.csrmm_heads(d_rp, d_ci, val, H[dt], m=m, d=d, heads=heads, k=m,
                                               C=C, handle=h)

            def csrmm_cast(dt):
                def step():
                    ops.csrmm_heads(d_rp, d_ci, val, H[dt], m=m, d=d, heads=heads, k=m, C=C,
                                    handle=h)
                    half_out[dt].copy_(C)  # the cast of autograd.spmm_heads, into a kept tensor
                return step

            routes = {"sddmm": sddmm, "csrmm": csrmm}
            # each half route against the fp32 entry on its own operands widened, bit for bit;
            # and the kernel each route launches
            vec = {}
            for op, outbuf in (("sddmm", e), ("csrmm", C)):
                for dt in DTYPES:
                    with h.launch_record() as rec:
                        routes[op](dt)()
                    vec[op, dt] = launched_vec(rec)
                    if dt == "fp32":
                        continue
                    got = outbuf.clone()
                    if op == "sddmm":
                        Hw = H[dt].float()
                        want = ops.sddmm_heads(d_rp, d_ci, Hw, Hw, m=m, k=m, handle=h)
                    else:
                        want = ops.csrmm_heads(d_rp, d_ci, val, H[dt].float(), m=m, d=d,
                                               heads=heads, k=m, handle=h)
                    torch.cuda.synchronize()
                    if not torch.equal(got.view(torch.int32), want.view(torch.int32)):
                        raise SystemExit(f"{case} {heads}x{d}: {op} {dt} differs from the fp32 "
                                         "entry on the widened operands")
                    del got, want
            for op in OPS:
                for rnd in range(rounds):
                    for dt in DTYPES:
                        elapsed, kt = bench.timed_loop(routes[op](dt), h, STEPS, WARMUP, 1, None,
                                                       raw=True, kernel_pass=True)
                        kms = statistics.median(kt)
                        by = model_bytes(op, m, nnz, heads, d, 4 if dt == "fp32" else 2)
                        rec = dict(graph=case, m=m, nnz=nnz, heads=heads, d=d, op=op, dtype=dt,
                                   round=rnd, steps=STEPS, warmup=WARMUP,
                                   kernel_ms=round(kms, 5), kernel_ms_min=round(min(kt), 5),
                                   kernel_ms_max=round(max(kt), 5), launches=len(kt),
                                   wall_ms_per_call=round(elapsed / STEPS * 1e3, 5),
                                   model_bytes=by,
                                   frac_of_hbm_peak=round(by / (kms / 1e3) / 1e9 /
                                                          bench.HBM_PEAK_GBPS, 4),
                                   vec=vec[op, dt])
                        if op == "csrmm" and dt != "fp32":
                            el2, _ = bench.timed_loop(csrmm_cast(dt), h, STEPS, WARMUP, 1, None,
                                                      raw=True, kernel_pass=False)
                            rec["wall_ms_with_cast"] = round(el2 / STEPS * 1e3, 5)
                        f.write(json.dumps(rec) + "\n")
                        f.flush()
                        print(json.dumps(rec), flush=True)
            del H32, H, val, e, C, half_out
            torch.cuda.empty_cache()
    h.close()


def summarise(path: str) -> list[dict]:
    by: dict = {}
    with open(path) as f:
        for line in f:
            r = json.loads(line)
            by.setdefault((r["graph"], r["heads"], r["d"], r["op"]), {}).setdefault(
                r["dtype"], []).append(r)
    out = []
    for (graph, heads, d, op), routes in by.items():
        first = routes["fp32"][0]
        s = dict(graph=graph, m=first["m"], nnz=first["nnz"], heads=heads, d=d, op=op,
                 rounds=len(routes["fp32"]), steps=first["steps"])
        for dt in DTYPES:
            ks = [r["kernel_ms"] for r in routes[dt]]
            med = statistics.median(ks)
            s[dt + "_kernel_ms_median"] = round(med, 5)
            s[dt + "_round_spread"] = round((max(ks) - min(ks)) / med, 4)
            s[dt + "_wall_ms_median"] = round(statistics.median(
                r["wall_ms_per_call"] for r in routes[dt]), 5)
            s[dt + "_vec"] = routes[dt][0]["vec"]
            s[dt + "_model_bytes"] = routes[dt][0]["model_bytes"]
            if "wall_ms_with_cast" in routes[dt][0]:
                s[dt + "_wall_ms_with_cast_median"] = round(statistics.median(
                    r["wall_ms_with_cast"] for r in routes[dt]), 5)
        for dt in DTYPES[1:]:
            ratio = s["fp32_kernel_ms_median"] / s[dt + "_kernel_ms_median"]
            s["fp32_over_" + dt] = round(ratio, 3)
            s["bytes_fp32_over_" + dt] = round(s["fp32_model_bytes"] / s[dt + "_model_bytes"], 3)
            s[dt + "_ahead_by_more_than_the_spread"] = bool(
                ratio > 1 + max(s["fp32_round_spread"], s[dt + "_round_spread"]))
        out.append(s)
    return out


NAMES = {"arxiv_csr": "arxiv", "products_csr": "products", "reddit_bsr32": "reddit"}


def table(summary: list[dict]) -> str:
    """DESIGN.md §4k's table from summary.json: per graph and shape, for each op the median
    kernel ms of the three routes, fp32 over each half route, the byte model's ratio and the
    larger round spread; a half route that is not ahead of fp32 by more than the spread is
    marked."""
    rows = {}
    for s in summary:
        cells = []
        for dt in DTYPES[1:]:
            spread = max(s["fp32_round_spread"], s[dt + "_round_spread"])
            width = (f"vec {s[dt + '_vec']}" if s["op"] == "csrmm"
                     else "chunk loads" if s[dt + "_vec"] else "column loads")
            cell = (f"{dt} {s[dt + '_kernel_ms_median']:.3f} ({s['fp32_over_' + dt]:.2f}×, "
                    f"{spread:.2f}, {width})")
            if not s[dt + "_ahead_by_more_than_the_spread"]:
                cell += " **not ahead**"
            cells.append(cell)
        rows.setdefault((s["graph"], s["heads"], s["d"]), {})[s["op"]] = (
            f"fp32 {s['fp32_kernel_ms_median']:.3f}; " + "; ".join(cells) +
            f"; bytes {s['bytes_fp32_over_fp16']:.2f}×")
    out = ["| graph | heads × d | sampled product: kernel ms (fp32 ÷ half, spread, width) | "
           "product: kernel ms (fp32 ÷ half, spread, width) |", "|---|---|---|---|"]
    for (graph, heads, d), ops_ in rows.items():
        out.append(f"| {NAMES.get(graph, graph)} | {heads}×{d} | {ops_['sddmm']} | "
                   f"{ops_['csrmm']} |")
    return "\n".join(out)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default=None, metavar="SUMMARY_JSON",
                    help="print DESIGN.md §4k's table from a summary.json and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heads_half", "bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per graph")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--shapes", default=",".join(f"{h}x{d}" for h, d in SHAPES))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.table:
        with open(args.table) as f:
            print(table(json.load(f)))
        return
    if args.rounds < 3:
        raise SystemExit("at least three interleaved rounds")
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    if args.child:
        child(args.child, args.rounds, args.out, shapes)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()
    for case in args.cases.split(","):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__),
               "--child", case, "--rounds", str(args.rounds), "--out", args.out,
               "--shapes", args.shapes]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit(f"{case}: the measuring process ended with status {rc}; "
                             "nothing more is started")
    summary = summarise(args.out)
    with open(os.path.join(os.path.dirname(os.path.abspath(args.out)), "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    for s in summary:
        print(json.dumps(s))


if __name__ == "__main__":
    main()
