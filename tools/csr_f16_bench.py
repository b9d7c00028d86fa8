#!/usr/bin/env python3
"""fp32 entry against fp16 entry of the CSR product on the same matrix.

    python tools/csr_f16_bench.py [--out profiles/csr_f16/bench.jsonl] [--rounds 3]

The products stand-in of bench.py (its WORKLOADS entry, generator arguments and value
seed) at K = 128, 256 and 512 and the arxiv stand-in at K = 128. Per (workload, K):
spmm_csrmm_ex_f32 on (val, B) and spmm_csrmm_ex_f16 on (val.half(), B.half()),
interleaved fp32, fp16, fp32, fp16, ... for --rounds rounds; a round is bench.py's
timed_loop: 5 warm-up steps, 20 steps on the wall clock, then 20 steps under the
handle's kernel timing. One JSON line per (workload, K, dtype, round): ms per step,
kernel ms (median, min and max of the 20 launches), the algorithmic bytes of the
gather model (fp32: 4(m+1) + 8 nnz + 4 K nnz + 4 K m; fp16 A values and B:
4(m+1) + 6 nnz + 2 K nnz + 4 K m), their rate as a fraction of the 8 TB/s peak, and
the vector width the launch took. summary.json beside it holds, per (workload, K),
the median kernel ms of each dtype over the rounds, the round-to-round spread of the
fp32 medians and whether fp16 is faster by more than that spread.

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench  # noqa: E402  (WORKLOADS, csr_bytes, timed_loop, HBM_PEAK_GBPS; adds the package path)

CASES = [("products_csr", (128, 256, 512)), ("arxiv_csr", (128,))]
STEPS, WARMUP = 20, 5


def csr_bytes_f16(m: int, nnz: int, K: int) -> int:
    """bench.csr_bytes with binary16 A values and B (C stays fp32)."""
    return 4 * (m + 1) + 6 * nnz + 2 * K * nnz + 4 * K * m


def picked_vec(n: int, B, ldb: int, C, ldc: int) -> int:
    """pick_vec (csr_kernels.hip) restated: B's alignment in its own elements."""
    eb = B.element_size()
    if (n > 128 and n % 4 == 0 and ldb % 4 == 0 and ldc % 4 == 0 and B.data_ptr() % (4 * eb) == 0
            and C.data_ptr() % 16 == 0):
        return 4
    if (n > 64 and n % 2 == 0 and ldb % 2 == 0 and ldc % 2 == 0 and B.data_ptr() % (2 * eb) == 0
            and C.data_ptr() % 8 == 0):
        return 2
    return 1


def child(workload: str, Ks, rounds: int, out: str) -> None:
    import torch
    from spmm_hip import ops, prep
    W = bench.WORKLOADS[workload]
    dev = torch.device("cuda", 0)
    rp, ci = prep.powerlaw_csr(W["n"], W["nnz"], W["max_deg"], 2.3, 1234)  # bench.run_csr's matrix
    val = np.random.default_rng(2).uniform(-1, 1, ci.size).astype(np.float32)
    m, nnz = rp.size - 1, int(ci.size)
    d_rp, d_ci, d_v = (torch.from_numpy(a).to(dev) for a in (rp, ci, val))
    d_v16 = d_v.half()
    h = ops.Handle()
    with open(out, "a") as f:
        for K in Ks:
            g = torch.Generator(device=dev)
            g.manual_seed(1234)
            B = torch.rand((m, K), device=dev, generator=g) * 2 - 1
            B16 = B.half()
            C = torch.empty((m, K), device=dev)
            steps = {
                "fp32": lambda: ops.csrmm(d_rp, d_ci, d_v, B, m=m, n=K, k=m, ldb=K, C=C, ldc=K,
                                          handle=h),
                "fp16": lambda: ops.csrmm_f16(d_rp, d_ci, d_v16, B16, m=m, n=K, k=m, ldb=K, C=C,
                                              ldc=K, handle=h),
            }
            for rnd in range(rounds):
                for dt, Bx in (("fp32", B), ("fp16", B16)):
                    elapsed, kt = bench.timed_loop(steps[dt], h, STEPS, WARMUP, 1, None, raw=True,
                                                   kernel_pass=True)
                    kms = statistics.median(kt)
                    by = bench.csr_bytes(m, nnz, K) if dt == "fp32" else csr_bytes_f16(m, nnz, K)
                    rec = dict(workload=workload, K=K, dtype=dt, round=rnd,
                               ms_per_step=round(elapsed / STEPS * 1e3, 5),
                               kernel_ms=round(kms, 5), kernel_ms_min=round(min(kt), 5),
                               kernel_ms_max=round(max(kt), 5), launches=len(kt),
                               algorithmic_bytes=by,
                               frac_of_hbm_peak=round(by / (kms / 1e3) / 1e9 / bench.HBM_PEAK_GBPS,
                                                      4),
                               vec=picked_vec(K, Bx, K, C, K), m=m, nnz=nnz,
                               steps=STEPS, warmup=WARMUP)
                    f.write(json.dumps(rec) + "\n")
                    f.flush()
                    print(json.dumps(rec), flush=True)
            del B, B16, C
    h.close()


def summarise(path: str) -> list[dict]:
    rows: dict = {}
    with open(path) as f:
        for line in f:
            r = json.loads(line)
            rows.setdefault((r["workload"], r["K"]), {}).setdefault(r["dtype"], []).append(
                r["kernel_ms"])
    out = []
    for (w, K), d in rows.items():
        if "fp32" not in d or "fp16" not in d:
            continue
        m32, m16 = statistics.median(d["fp32"]), statistics.median(d["fp16"])
        spread = max(d["fp32"]) - min(d["fp32"])
        out.append(dict(workload=w, K=K, fp32_kernel_ms_median=m32, fp16_kernel_ms_median=m16,
                        fp32_round_spread_ms=round(spread, 5), rounds=len(d["fp32"]),
                        margin_ms=round(m32 - m16, 5),
                        fp16_faster_beyond_spread=bool(m32 - m16 > spread)))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_f16", "bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per workload")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--K", type=int, nargs="*", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.rounds < 3:
        raise SystemExit("at least three interleaved rounds")
    if args.child:
        child(args.child, args.K, args.rounds, args.out)
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").close()
    for workload, Ks in CASES:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__),
               "--child", workload, "--rounds", str(args.rounds), "--out", args.out, "--K",
               *[str(k) for k in Ks]]
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
