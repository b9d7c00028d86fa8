"""bench.py end to end on the GPU, on its smallest CSR workload (the arxiv
stand-in): a plain run times exactly --steps steps and measures nothing beside
the line, and --dump-outputs writes the C of the timed path, bit for bit what
the same call computes here on the same seeded inputs."""
from __future__ import annotations

import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_is_lean_and_dumps_the_timed_output(device, tmp_path):
    from spmm_hip import ops, prep
    out = tmp_path / "out"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--workload", "arxiv_csr", "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    b = _bench()
    W = b.WORKLOADS["arxiv_csr"]
    n, K = W["n"], W["K"]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "GFLOP/s" and line["higher_is_better"] is True and line["dtype"] == "fp32"
    assert line["ms_per_step"] > 0
    # value is 2 nnz K over the step time the line reports (both rounded)
    want = 2.0 * line["config"]["nnz"] * K / (line["ms_per_step"] * 1e-3) / 1e9
    assert abs(line["value"] - want) <= 1e-3 * want
    # nothing beside the headline without --full
    assert line["cpu_baseline"] is None and line["roofline"]["kernel_ms"] is None
    assert not {"hot_column_hints", "config3", "config5", "products_bsr32"} & set(line)
    # the dump: float32, within the size bound, the fixed row sample of C
    assert sorted(os.listdir(out)) == ["C.npy"]
    C = np.load(out / "C.npy")
    assert C.dtype == np.float32 and C.shape == (b.DUMP_ROWS, K) and C.nbytes <= 64 << 20
    rp, ci = prep.powerlaw_csr(n, W["nnz"], W["max_deg"], 2.3, 1234)
    val = np.random.default_rng(2).uniform(-1, 1, ci.size).astype(np.float32)
    g = torch.Generator(device=device)
    g.manual_seed(1234)
    B = torch.rand((n, K), device=device, generator=g) * 2 - 1
    d_rp, d_ci, d_v = (torch.from_numpy(a).to(device) for a in (rp, ci, val))
    Cx = torch.empty((n, K), device=device)
    ops.csrmm(d_rp, d_ci, d_v, B, m=n, n=K, k=n, ldb=K, C=Cx, ldc=K)
    torch.cuda.synchronize()
    idx = np.sort(np.random.default_rng(0).choice(n, b.DUMP_ROWS, replace=False))
    assert np.array_equal(C, Cx.cpu().numpy()[idx])
