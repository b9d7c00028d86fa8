#!/usr/bin/env python3
"""The multi-head entries (ops.sddmm_heads, edge_softmax_heads, edge_softmax_bwd_heads,
csrmm_heads) beside the same work done with the single-head entries.

    python tools/heads_bench.py [--out profiles/heads/bench.jsonl] [--rounds 3]

The products, reddit and arxiv stand-ins of bench.py (its WORKLOADS entries, generator
arguments and seed) at heads x d = 8x8, 8x16, 4x32 and 8x64. The user's data is in the
layouts of the new entries: edge values [nnz, heads], features [rows, heads, d]. Per
pattern, shape and op, interleaved for --rounds rounds:
  heads   one call of the new entry
  loop    the loop over the heads of the unchanged single-head entry (ops.sddmm,
          ops.edge_softmax, ops.edge_softmax_bwd, ops.csrmm with its default options), each
          head's feature slice passed in place through the leading dimension, each head's
          edge values a row of a contiguous [heads, nnz] array, and the layout transposes
          between that array and the user's [nnz, heads] inside the timing: the result out
          (sddmm), x in and y out (softmax), g in and gx out (backward; y is kept in
          [heads, nnz] from the forward), val in (product)
Both are timed the same way: the wall clock between two device synchronisations around
`steps` calls after 2 warm-up calls, steps chosen once per (shape, op) so that the slower
route's window is at least 0.25 s (at least 3 calls). One JSON line per (pattern, heads, d,
op, method, round). Before anything is timed the two routes' outputs are compared: bit for
bit for the sampled product and the softmax, within 1e-4 of the row's magnitude for the
product (the single-head entry's default association differs from the piece rule below
n = 65). summary.json beside the output holds, per (pattern, shape, op), the medians over
the rounds, each route's round-to-round spread (max - min over the median), loop over
heads, and whether that ratio is above 1 by more than the larger spread.

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

CASES = ["arxiv_csr", "products_csr", "reddit_bsr32"]
SHAPES = [(8, 8), (8, 16), (4, 32), (8, 64)]
OPS = ["sddmm", "softmax", "softmax_bwd", "csrmm"]
WARMUP, MIN_STEPS, MAX_STEPS, WINDOW_S = 2, 3, 200, 0.25


def pattern(case: str):
    from spmm_hip import prep
    W = bench.WORKLOADS[case]
    if W["kind"] == "csr":
        return prep.powerlaw_csr(W["n"], W["nnz"], W["max_deg"], 2.3, 1234)
    return prep.community_csr(W["n"], W["avg_deg"], W["cmin"], W["cmax"], W["p_in"], 1234)


def child(case: str, rounds: int, out: str, shapes) -> None:
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

    def window(step, steps):
        for _ in range(WARMUP):
            step()
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        sync()
        return (time.perf_counter() - t0) / steps * 1e3

    with open(out, "a") as f:
        for heads, d in shapes:
            w = heads * d
            H = torch.rand((m, heads, d), device=dev, generator=gen) * 2 - 1
            Hf = H.view(-1)
            e = torch.empty((nnz, heads), device=dev)
            a, ga, gx = torch.empty_like(e), torch.empty_like(e), torch.empty_like(e)
            C = torch.empty((m, heads, d), device=dev)
            # the loop's own buffers: [heads, nnz] edge values, and its outputs
            t_in, t_out = torch.empty((heads, nnz), device=dev), torch.empty((heads, nnz), device=dev)
            a_t = torch.empty((heads, nnz), device=dev)
            e2, a2, gx2, C2 = (torch.empty_like(t) for t in (e, a, gx, C))
            C2f = C2.view(-1)

            def sddmm_heads():
                ops.sddmm_heads(d_rp, d_ci, H, H, m=m, k=m, out=e, handle=h)

            def sddmm_loop():
                for hd in range(heads):
                    ops.sddmm(d_rp, d_ci, Hf[hd * d:], Hf[hd * d:], m=m, n=d, k=m, ldx=w, ldy=w,
                              out=t_out[hd], handle=h)
                e2.copy_(t_out.t())

            def softmax_heads():
                ops.edge_softmax_heads(d_rp, e, m=m, out=a, handle=h)

            def softmax_loop():
                t_in.copy_(e.t())
                for hd in range(heads):
                    ops.edge_softmax(d_rp, t_in[hd], m=m, out=a_t[hd], handle=h)
                a2.copy_(a_t.t())

            def softmax_bwd_heads():
                ops.edge_softmax_bwd_heads(d_rp, a, ga, m=m, out=gx, handle=h)

            def softmax_bwd_loop():
                t_in.copy_(ga.t())
                for hd in range(heads):
                    ops.edge_softmax_bwd(d_rp, a_t[hd], t_in[hd], m=m, out=t_out[hd], handle=h)
                gx2.copy_(t_out.t())

            def csrmm_heads():
                ops.csrmm_heads(d_rp, d_ci, a, H, m=m, d=d, heads=heads, k=m, C=C, handle=h)

            def csrmm_loop():
                t_in.copy_(a.t())
                for hd in range(heads):
                    ops.csrmm(d_rp, d_ci, t_in[hd], Hf[hd * d:], m=m, n=d, k=m, ldb=w,
                              C=C2f[hd * d:], ldc=w, handle=h)

            routes = {"sddmm": (sddmm_heads, sddmm_loop), "softmax": (softmax_heads, softmax_loop),
                      "softmax_bwd": (softmax_bwd_heads, softmax_bwd_loop),
                      "csrmm": (csrmm_heads, csrmm_loop)}
            # once, in the order of the chain, and the two routes against each other
            sddmm_heads()
            sddmm_loop()
            softmax_heads()
            softmax_loop()
            ga.copy_(torch.rand(e.shape, device=dev, generator=gen) * 2 - 1)
            softmax_bwd_heads()
            softmax_bwd_loop()
            csrmm_heads()
            csrmm_loop()
            sync()
            for nm, x, y in (("sddmm", e, e2), ("softmax", a, a2), ("softmax_bwd", gx, gx2)):
                if not torch.equal(x, y):
                    raise SystemExit(f"{case} {heads}x{d}: {nm} differs between the two routes")
            scale = C.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-30)
            worst = float(((C - C2).abs() / scale).max())
            if not worst <= 1e-4:
                raise SystemExit(f"{case} {heads}x{d}: the products differ by {worst} of a row")
            for op in OPS:
                new, loop = routes[op]
                t1 = max(window(new, 1), window(loop, 1))
                steps = int(min(MAX_STEPS, max(MIN_STEPS, WINDOW_S * 1e3 / t1)))
                for rnd in range(rounds):
                    for method, step in (("heads", new), ("loop", loop)):
                        rec = dict(pattern=case, m=m, nnz=nnz, heads=heads, d=d, op=op,
                                   method=method, round=rnd, steps=steps,
                                   wall_ms_per_call=round(window(step, steps), 5))
                        f.write(json.dumps(rec) + "\n")
                        f.flush()
                        print(json.dumps(rec), flush=True)
            del H, Hf, e, a, ga, gx, C, t_in, t_out, a_t, e2, a2, gx2, C2, C2f
            torch.cuda.empty_cache()
    h.close()


def summarise(path: str) -> list[dict]:
    by: dict = {}
    with open(path) as f:
        for line in f:
            r = json.loads(line)
            by.setdefault((r["pattern"], r["heads"], r["d"], r["op"]), {}).setdefault(
                r["method"], []).append(r)
    out = []
    for (pat, heads, d, op), meth in by.items():
        s = dict(pattern=pat, m=meth["heads"][0]["m"], nnz=meth["heads"][0]["nnz"], heads=heads,
                 d=d, op=op, rounds=len(meth["heads"]), steps=meth["heads"][0]["steps"])
        for nm in ("heads", "loop"):
            ts = [r["wall_ms_per_call"] for r in meth[nm]]
            med = statistics.median(ts)
            s[nm + "_ms_median"] = round(med, 5)
            s[nm + "_round_spread"] = round((max(ts) - min(ts)) / med, 4)
        s["loop_over_heads"] = round(s["loop_ms_median"] / s["heads_ms_median"], 3)
        s["ahead_by_more_than_the_spread"] = bool(
            s["loop_over_heads"] > 1 + max(s["heads_round_spread"], s["loop_round_spread"]))
        out.append(s)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heads", "bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=400, help="seconds per pattern")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--shapes", default=",".join(f"{h}x{d}" for h, d in SHAPES))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
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
