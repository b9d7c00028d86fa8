"""The kernel coverage table: small cases through the public entries (spmm_hip.ops), each
naming the kernel instantiations it must launch and how its result is checked.

tests/test_kernel_cases.py (no GPU) proves that the table names every shipped kernel that a
release build can reach, and that the kernels a case expects are the ones the launchers pick
for its arguments (bin/dispatch_trace in its "cases" mode). tests/test_gpu_kernel_coverage.py
runs every case on the GPU with the handle's launch record on (ops.Handle.launch_record),
requires the expected kernels in the record and checks the result against a reference that
is not the code under test.

A case is Case(id, entry, args, expect):
  entry   the public entry, a key of RUNNERS (ops.bsrmm, ops.csrmm, ops.csr2csc, ...)
  args    its arguments; what each entry reads is documented at its runner
  expect  patterns (regular expressions, searched) over the kernels' keys
          (kernel_keys.launch_key): each must match a kernel of the call's launch record
  idle    the patterns of expect whose kernel is queued in this case but returns at once on
          a device-side gate, so the result says nothing about it: the column stream where
          the panel probe picks the panel kernel (fully dense blocks), bsr_small_kernel
          where the grouped bs 2 / 4 / 8 stream keeps the matrix (no tile flagged), the
          grouped stream where its probe gives the matrix up. Such a case does not count
          as cover of that kernel (covering_keys); spmm_bsr_small_path is asserted where
          the small-bs probe decides

How results are checked (the runner of each entry):
  CSR products on the merge-path kernel   bit for bit, oracle_csrmm_pieces_f32 (the piece
                                          association)
  CSR products on the group kernel, every BSR / hybrid / grouped product
                                          the fp64 oracles with assert_normwise at TOL_F32
                                          / TOL_F16_ACC, alpha and beta other than 0 and 1
  bs 2 / 4 / 8 BSR products               also bit for bit, oracle_bsrmm_f32 (sequential)
  bs 32 / 64 column stream, panel stream, analysed and grouped bs 32 at row-major C
                                          also bit for bit, oracle_bsrmm_f32, on the block
                                          rows of at most 64 blocks (longer ones may be cut
                                          into segments, summed in segment order)
  fp64 products                           oracle_csrmm_d / oracle_bsrmm_d, 1e-12 norm-wise
  converters, csr2csc, SDDMM, transposes  numpy restatements, bit for bit (SDDMM: prep.sddmm,
                                          the written association rule)
Operands sit in helpers.framed buffers (sentinel guards, offsets, padding columns), and the
guards are checked after the call; only the 4-GiB B of the wide-ldb cases is allocated
uninitialised, with the n columns that are read written in place.

The BSR / CSR / hybrid part of the table was chosen by a greedy cover over the argument grid
of drivers/dispatch_trace.cpp (bs, direction, both orders, n, byte offsets of val / B / C,
leading-dimension additions, wide ldb, shallow / deep / long-row / dense shapes, masks, the
bsr and hybrid flags, fp16), restated on the public entries' arguments; api_launches()
below restates what the entry layer (csrc/api.cpp) does between a public call and its
launcher calls, so the host test can ask the trace for the same launcher arguments.
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field

import numpy as np

from helpers import (HYBRID_EX_M, PROBE64_MB, TOL_F16_ACC, TOL_F32, assert_normwise,
                     column_sparse_bsr, framed, framed_operands, hybrid_ex_parts,
                     long_row_column_sparse_bsr, oracle_bsrmm_d, oracle_bsrmm_f32,
                     oracle_bsrmm_f64, oracle_csrmm_d, oracle_csrmm_f64, oracle_csrmm_pieces_f32,
                     panel_probe_bsr64, rand_bsr, rand_csr_rows)

NUM_CUS = 256  # the MI355X's, and what bin/dispatch_trace fixes
WIDE_LDB = 1 << 24
DEEP_MB = 25000  # block rows: more than 8 * 12 * NUM_CUS waves at one column tile
ALPHA, BETA = 0.5, -1.5


@dataclass(frozen=True)
class Case:
    id: str
    entry: str
    args: dict = field(hash=False)
    expect: tuple
    idle: tuple = ()

    def __repr__(self):
        return self.id


# Kernels of the five files outside the dispatch trace that no argument tuple of a release
# build reaches: (pattern, how many, the launcher lines that prove it).
# Empty today. (launch_sddmm no longer instantiates sddmm_kernel<G, 1, vec, !full> at
# G = 1 / 2: G = group_lanes(n) is the smallest power of two >= ceil(n / 4), vec needs
# n % 4 == 0 and full is n % (4 G) == 0, and the only such n at G = 1 / 2 is 4 G itself.)
UNREACHABLE_OTHER: list[tuple[str, int, str]] = []


# ------------------------------------------------------------------ BSR matrices
def bsr_matrix(a: dict):
    """(mb, kb, rowptr, colind, val) of a BSR-entry case, ROW-direction fp32 values, from
    a["shape"] and a["bs"] alone (so the host test knows nnzb without a GPU):
      shallow  64 x 64 block rows / columns, about 250 column-sparse blocks, row 3 empty
      shared   64 x 64, bands of 16 block rows with the same 5 block columns (bs 2 / 4 / 8)
      long     23 x 320, block row 5 holding 300 blocks: the column streams split it into
               segments on this shallow grid (cs2_segments)
      deep     25,000 block rows (past 8 waves per wave slot at one column tile), about
               300 dense blocks
      deep-panel  bs 32: 24,600 block rows of one or two dense blocks, 2^15 in all (a
               row-major C takes the panel stream only on a deep grid: a shallow one has
               segments)
      panel    2^15 dense 32 x 32 (sub-)blocks, from which the panel probe runs: bs 32
               128 x 256 full; bs 64 helpers.panel_probe_bsr64's BSR part
      wide     for ldb = 2^24: bs 32 two block rows over kb = 2 (blocks (0,0) (0,1) (1,1)),
               bs 64 two block rows over kb = 1, so B rows 32 .. 63 start past 2^31 bytes"""
    bs, shape = a["bs"], a["shape"]
    if (bs, shape) not in _bsr_cache:
        _bsr_cache.clear()  # one at a time: a panel matrix is 128 MB
        _bsr_cache[bs, shape] = _bsr_matrix(bs, shape)
    return _bsr_cache[bs, shape]


_bsr_cache: dict = {}
_bsr_dims_cache: dict = {}


def _bsr_matrix(bs, shape):
    rng = np.random.default_rng(1000 + bs)
    if shape == "shallow":
        mb = kb = 64
        rp, ci, v = (column_sparse_bsr(rng, mb, kb, bs, 0.06) if bs >= 16 else
                     rand_bsr(rng, mb, kb, bs, 0.06, empty_rows=(3,)))
    elif shape == "shared":
        # bands of 16 block rows holding the same 5 block columns: every group of the
        # small-bs grouped stream shares all its columns, so its probe keeps the matrix
        mb = kb = 64
        cols = [np.sort(rng.choice(kb, 5, replace=False)) for _ in range(mb // 16)]
        rp = (5 * np.arange(mb + 1)).astype(np.int32)
        ci = np.concatenate([cols[r // 16] for r in range(mb)]).astype(np.int32)
        v = rng.uniform(-1, 1, ci.size * bs * bs).astype(np.float32)
    elif shape == "long":
        mb, kb = 23, 320
        rp, ci, v = long_row_column_sparse_bsr(rng, mb, kb, bs)
    elif shape == "deep":
        mb, kb = DEEP_MB, 8
        rows = rng.choice(mb, 300, replace=False)
        lens = np.zeros(mb, np.int64)
        lens[rows] = 1
        lens[rows[:20]] = 3
        rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        ci = np.concatenate([np.sort(rng.choice(kb, l, replace=False)) for l in lens[lens > 0]])
        ci = ci.astype(np.int32)
        v = rng.uniform(-1, 1, ci.size * bs * bs).astype(np.float32)
    elif shape == "deep-panel":
        mb, kb = 24600, 2
        lens = np.ones(mb, np.int64)
        lens[:(1 << 15) - mb] = 2
        rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        ci = np.concatenate([np.arange(l, dtype=np.int32) for l in lens])
        v = rng.random(ci.size * bs * bs, dtype=np.float32) * 2.0 - 1.0
    elif shape == "panel" and bs == 64:
        mb = kb = PROBE64_MB
        rp, ci, v = panel_probe_bsr64()[:3]
    elif shape == "panel":
        mb, kb = 128, 256
        rp = (kb * np.arange(mb + 1)).astype(np.int32)
        ci = np.tile(np.arange(kb, dtype=np.int32), mb)
        v = rng.random(ci.size * bs * bs, dtype=np.float32) * 2.0 - 1.0
    elif shape == "wide":
        mb, kb = 2, (2 if bs == 32 else 1)
        rp, ci = (np.array([0, 2, 3], np.int32), np.array([0, 1, 1], np.int32)) if kb == 2 else \
            (np.array([0, 1, 2], np.int32), np.array([0, 0], np.int32))
        v = rng.uniform(-1, 1, ci.size * bs * bs).astype(np.float32)
    else:
        raise KeyError(shape)
    return mb, kb, rp, ci, v


def _bsr_dims(a):
    """(mb, kb, nnzb) without generating values where the structure is known."""
    key = a["bs"], a["shape"]
    if key not in _bsr_dims_cache:
        known = {"deep": (DEEP_MB, 8, 340), "deep-panel": (24600, 2, 1 << 15),
                 "panel": ((128, 256, 1 << 15) if a["bs"] == 32 else
                           (PROBE64_MB, PROBE64_MB, 1 << 13))}.get(a["shape"])
        if known is None:
            mb, kb, _, ci, _ = bsr_matrix(a)
            known = mb, kb, int(ci.size)
        _bsr_dims_cache[key] = known
    return _bsr_dims_cache[key]


# ------------------------------------------- the entry layer, restated (csrc/api.cpp)
T4, T16 = r"17transpose4_kernelILb0EE", r"20transpose16x4_kernelILb0EE"


def _csr_line(f16, m, n, boff, coff, ldb, ldc, nnz, hot, flags):
    return f"csr {int(f16)} {m} {n} {boff} {coff} {ldb} {ldc} {nnz} {hot} {flags}"


def api_launches(case: Case):
    """What the entry layer makes of a case of the BSR / CSR / hybrid entries: (lines,
    aux). lines are the launcher calls in bin/dispatch_trace's "cases" format; aux are
    patterns of the kernels the entry itself launches around them (staging transposes,
    analyses). None for the entries the trace does not cover."""
    a, e = case.args, case.entry
    if e in ("bsrmm", "bsrmm_f16", "bsrmm_analysed", "bsrmm_analysed_f16"):
        f16 = e.endswith("f16")
        elem = 2 if f16 else 4
        vec = 16 // elem
        bs, n = a["bs"], a["n"]
        mb, kb, nnzb = _bsr_dims(a)
        rows_b, rows_c = kb * bs, mb * bs
        ob, oc = a["ob"], a["oc"]
        ldb = WIDE_LDB if a["shape"] == "wide" else (n if ob == 0 else rows_b) + a["pad_b"]
        ldc = (n if oc == 0 else rows_c) + a["pad_c"]
        voff, boff, coff = a["voff"] * elem, a["boff"] * elem, a["coff"] * 4
        aux = []
        analysed = "analysed" in e
        if analysed:
            aux.append("bsr16_analysis_kernelE" if f16 else "bsr32_analysis_kernelE")
            rowd, masks = 0, 1
            stage = ob == 1 and (n >= 128 and n % 8 == 0 if f16 else n >= 4 and n % 4 == 0)
        else:
            rowd, masks = a["rowd"], 0
            f32_stream = not f16 and bs in (2, 4, 8, 32, 64)
            stage = (rowd == 1 and (bs == 16 or f32_stream) and (ob == 1 or oc == 1) and
                     n >= vec and n % vec == 0 and voff % 16 == 0)
        if stage and ob == 1:
            aux.append(T16 if f16 else T4)
            ob, boff, ldb = 0, 0, n
        line = (f"bsr {int(f16)} {bs} {n} {rowd} {1 - ob} {1 - oc} {voff} {boff} {coff} {ldb} "
                f"{ldc} {mb} {kb} {nnzb} {masks} 0 {a['bsr_flags']} 0")
        return [line], aux
    if e == "csrmm_hot_wide":
        n, k, ldb = a["n"], HOT_WIDE_K, HOT_WIDE_LDB
        assert (k * ldb + n) * 4 + 64 >= 1 << 32
        rp = hot_wide_matrix()[0]
        return ([_csr_line(0, rp.size - 1, n, a["boff"] * 4, 0, ldb, n, int(rp[-1]), 1, 1)],
                ["16col_count_kernelExPKi", "count_hist_kernelE", "hot_select_kernelE",
                 "hot_tag_kernelE"])
    if e in ("csrmm", "csrmm_f16", "csrmm_hot"):
        f16 = e == "csrmm_f16"
        elem = 2 if f16 else 4
        m, k, n, ob, oc = a["m"], a["k"], a["n"], a["ob"], a["oc"]
        nnz = int(csr_matrix(a)[0][-1])
        ldb = (n if ob == 0 else k) + a["pad_b"]
        ldc = (n if oc == 0 else m) + a["pad_c"]
        boff, coff = a["boff"] * elem, a["coff"] * 4
        aux = []
        if e == "csrmm_hot":
            aux += ["16col_count_kernelExPKi", "count_hist_kernelE", "hot_select_kernelE",
                    "hot_tag_kernelE"]
        if ob == 1:
            aux.append(T16 if f16 else T4)
            boff, ldb = 0, n
        if oc == 1:
            aux.append(T4)
            coff, ldc = 0, n
        hot = 0 if e != "csrmm_hot" else (2 if (k * ldb + n) * 4 + 64 < (1 << 32) else 1)
        return [_csr_line(f16, m, n, boff, coff, ldb, ldc, nnz, hot, a["csr_flags"])], aux
    if e == "hybrid_csrmm":
        bs, n, ob, oc, flags = a["bs"], a["n"], a["ob"], a["oc"], a["hybrid_flags"]
        crp, cci, cv, brp, bci, bv = hybrid_ex_parts(bs)
        m = k = HYBRID_EX_M
        mb = kb = -(-m // bs)
        ldb = (n if ob == 0 else k) + a["pad_b"]
        ldc = (n if oc == 0 else mb * bs) + a["pad_c"]
        boff, coff = a["boff"] * 4, a["coff"] * 4
        fusable = (n >= 4 and n % 4 == 0 and ldb % 4 == 0 and boff % 16 == 0 and ldc % 2 == 0 and
                   coff % 8 == 0)
        want = bool(flags & 1) or (not flags & 2 and cci.size <= 4096 * -(-m // 32))
        if ob == 0 and oc == 0 and bs == 32 and want and fusable:
            return [f"hybrid {m} {n} {ldb} {ldc} {flags}"], []
        aux = []
        if ob == 1:
            aux.append(T4)
            boff, ldb = 0, n
        lines = [f"bsr 0 {bs} {n} 1 1 {1 - oc} 0 {boff} {coff} {ldb} {ldc} {mb} {kb} {bci.size} "
                 f"0 1 0 {flags}"]
        if oc == 1:
            aux.append(T4)
            lines.append(_csr_line(0, m, n, boff, 0, ldb, n, cci.size, 0, 1))
        else:
            lines.append(_csr_line(0, m, n, boff, coff, ldb, ldc, cci.size, 0, 1))
        return lines, aux
    return None


# ------------------------------------------------------------------ CSR matrices
def csr_matrix(a: dict):
    """rowptr, colind, val of a CSR-entry case: m x k, 0 .. 12 entries per row (a fifth
    of the rows empty) and row 7 holding 400 (several pieces of the merge-path kernel's
    association, split across waves)."""
    m, k = a["m"], a["k"]
    rng = np.random.default_rng(77 + m)
    rp, ci, v = rand_csr_rows(rng, m, k, 12)
    rows = [ci[rp[i]:rp[i + 1]] for i in range(m)]
    rows[7] = np.sort(rng.choice(k, min(400, k), replace=False)).astype(np.int32)
    rp = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows).astype(np.int32)
    return rp, ci, rng.uniform(-1, 1, ci.size).astype(np.float32)


HOT_WIDE_K, HOT_WIDE_LDB = 1_100_000, 1024  # B rows past 4 GB: k * ldb * 4 = 4.5e9


def hot_wide_matrix():
    """rowptr, colind, val, used: 2000 rows over the k = 1,100,000 rows of a B with ldb =
    1024, whose entries fall on 300 B rows (`used`, sorted; the last row of B among them,
    past the 4-GB offset, and row 5 of the matrix holding 250 entries)."""
    rng = np.random.default_rng(41)
    used = np.unique(np.concatenate([rng.choice(HOT_WIDE_K, 299, replace=False),
                                     [HOT_WIDE_K - 1]])).astype(np.int32)
    rp, ci, v = rand_csr_rows(rng, 2000, used.size, 6)
    rows = [ci[rp[i]:rp[i + 1]] for i in range(2000)]
    rows[5] = np.sort(rng.choice(used.size, 250, replace=False)).astype(np.int32)
    rp = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    ci = np.concatenate(rows)
    return rp, used[ci], rng.uniform(-1, 1, ci.size).astype(np.float32), used


# ------------------------------------------------------------------------ runners
def _torch():
    import torch
    return torch


def _dev(*arrs):
    torch = _torch()
    return [torch.from_numpy(np.ascontiguousarray(x)).to("cuda") for x in arrs]


def _offset(arr, off):
    """A device copy of the flat host array that starts `off` elements past a 256-byte
    aligned allocation."""
    torch = _torch()
    buf = torch.empty(arr.size + off, dtype=torch.from_numpy(arr[:1].copy()).dtype, device="cuda")
    buf[off:].copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    view = buf[off:]
    assert view.data_ptr() % 16 == off * arr.itemsize % 16
    return view


def _check_product(got, ref, absd, C0, tol, what):
    ref = ALPHA * ref + BETA * C0.astype(np.float64)
    absd = abs(ALPHA) * absd + abs(BETA) * np.abs(C0.astype(np.float64))
    assert_normwise(got, ref, absd, tol, what)


def _same_bits(got, want, what):
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ from the " \
                          f"sequential fp32 oracle"


def run_bsr(case, oracle, h):
    """ops.bsrmm / bsrmm_f16 / bsrmm_analysed / bsrmm_analysed_f16 on bsr_matrix(args).
    args: bs, n, rowd (1: ROW blocks), ob / oc (0 row-major, 1 column-major B / C), voff /
    boff / coff (elements off a 16-byte base), pad_b / pad_c (added to the leading
    dimension), shape, bsr_flags."""
    from spmm_hip import ops
    torch = _torch()
    a, e = case.args, case.entry
    f16 = e.endswith("f16")
    bs, n, ob, oc = a["bs"], a["n"], a["ob"], a["oc"]
    mb, kb, rp, ci, v = bsr_matrix(a)
    vt = np.float16 if f16 else np.float32
    v = v.astype(vt)
    rng = np.random.default_rng(5)
    Bd = rng.uniform(-1, 1, (kb * bs, n)).astype(vt)
    C0 = rng.uniform(-1, 1, (mb * bs, n)).astype(np.float32)
    lay = (a["boff"], a["pad_b"], a["coff"], a["pad_c"])
    wide = a["shape"] == "wide"
    if wide:  # 4 GiB, uninitialised but for the n columns that are read
        assert ob == 0 and not f16
        dB = torch.empty((kb * bs - 1) * WIDE_LDB + n, dtype=torch.float32, device="cuda")
        dB.as_strided((kb * bs, n), (WIDE_LDB, 1)).copy_(torch.from_numpy(Bd))
        ldb, chkB = WIDE_LDB, None
        _, _, _, dC, ldc, extract = framed_operands(Bd[:1], C0, (0, 0) + lay[2:], 0, oc)
    else:
        dB, chkB, ldb, dC, ldc, extract = framed_operands(Bd, C0, lay, ob, oc)
    rowd = 1 if "analysed" in e else a["rowd"]  # the analysis takes ROW blocks here
    src = v if rowd else np.ascontiguousarray(v.reshape(-1, bs, bs).transpose(0, 2, 1)).reshape(-1)
    drp, dci = _dev(rp, ci)
    dv = _offset(src, a["voff"])
    h.set_bsr_options(a["bsr_flags"])
    kw = dict(mb=mb, kb=kb, n=n, ldb=ldb, order_b=ob, C=dC, ldc=ldc, order_c=oc, alpha=ALPHA,
              beta=BETA, handle=h)
    with h.launch_record() as rec:
        if "analysed" in e:
            ana = ops.bsr16_analysis if f16 else ops.bsr32_analysis
            masks, vcol = ana(dv, nnzb=ci.size, direction=0, handle=h)
            (ops.bsrmm_analysed_f16 if f16 else ops.bsrmm_analysed)(drp, dci, vcol, masks, dB, **kw)
        else:
            (ops.bsrmm_f16 if f16 else ops.bsrmm)(drp, dci, dv, dB, bs=bs, direction=1 - rowd,
                                                  **kw)
    torch.cuda.synchronize()
    got = extract(case.id)
    if chkB is not None:
        chkB.unchanged(case.id + ": B")
    ref, absd = oracle_bsrmm_f64(oracle, 0, mb, n, bs, rp, ci, v, Bd, n, 0, half=f16)
    _check_product(got, ref, absd, C0, TOL_F16_ACC if f16 else TOL_F32, case.id)
    small = any("bsr_small" in p for p in case.expect)
    stream = oc == 0 and any("bsr32_f32_cs2_kernel" in p or "bsr32_f32_panel_kernel" in p
                             for p in case.expect)
    if small or stream:
        # the bits of the sequential fp32 oracle, blocks in order (DESIGN.md 6,
        # tests/test_gpu_bsr.py test_random_shapes_bits): bs 2 / 4 / 8 on the lane-group
        # kernel and the grouped stream; the bs 32 / 64 column stream (drop-in, analysed,
        # SUB) and the panel stream at row-major C, on block rows of at most 64 blocks
        want = oracle_bsrmm_f32(oracle, 1 - rowd, mb, n, bs, rp, ci, src, Bd, n, 0, ALPHA, BETA,
                                C0.reshape(-1), n, 0).reshape(mb * bs, n)
        whole = np.ones(mb * bs, bool) if small else np.repeat(np.diff(rp) <= 64, bs)
        _same_bits(got[whole], want[whole], case.id)
    if "small_path" in a:
        assert h.small_bsr_path() == a["small_path"], \
            f"{case.id}: spmm_bsr_small_path {h.small_bsr_path()}, the case needs {a['small_path']}"
    return rec


def run_csr(case, oracle, h):
    """ops.csrmm / csrmm_f16 / csrmm_hot on csr_matrix(args). args: m, k, n, ob, oc, boff,
    coff, pad_b, pad_c, csr_flags. The merge-path kernel (every case but those whose
    expectation names csr_group_kernel) is held to the piece oracle's bits."""
    from spmm_hip import ops
    torch = _torch()
    a, e = case.args, case.entry
    f16 = e == "csrmm_f16"
    m, k, n, ob, oc = a["m"], a["k"], a["n"], a["ob"], a["oc"]
    rp, ci, v = csr_matrix(a)
    vt = np.float16 if f16 else np.float32
    v = v.astype(vt)
    rng = np.random.default_rng(6)
    Bd = rng.uniform(-1, 1, (k, n)).astype(vt)
    C0 = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    dB, chkB, ldb, dC, ldc, extract = framed_operands(
        Bd, C0, (a["boff"], a["pad_b"], a["coff"], a["pad_c"]), ob, oc)
    drp, dci, dv = _dev(rp, ci, v)
    h.set_csr_options(a["csr_flags"])
    kw = dict(m=m, n=n, k=k, ldb=ldb, order_b=ob, C=dC, ldc=ldc, order_c=oc, alpha=ALPHA,
              beta=BETA, handle=h)
    with h.launch_record() as rec:
        if e == "csrmm_hot":
            tag = ops.csr_hot_analysis(dci, n=n, k=k, hot_bytes=40 * 4 * n, handle=h)
            ops.csrmm_hot(drp, tag, dv, dB, **kw)
        else:
            (ops.csrmm_f16 if f16 else ops.csrmm)(drp, dci, dv, dB, **kw)
    torch.cuda.synchronize()
    got = extract(case.id)
    chkB.unchanged(case.id + ": B")
    v32, B32 = v.astype(np.float32), Bd.astype(np.float32)
    if any("csr_group_kernel" in p for p in case.expect):
        ref, absd = oracle_csrmm_f64(oracle, m, n, rp, ci, v32, B32, n, 0)
        _check_product(got, ref, absd, C0, TOL_F32, case.id)
    else:
        want = oracle_csrmm_pieces_f32(oracle, m, n, rp, ci, v32, B32, n, 0, ALPHA, BETA,
                                       C0.reshape(-1), n, 0).reshape(m, n)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
            f"{case.id}: differs from the piece oracle in " \
            f"{int((got.view(np.uint32) != want.view(np.uint32)).sum())} elements"
    return rec


def run_csr_hot_wide(case, oracle, h):
    """ops.csrmm_hot on a B of 4.5 GB (HOT = 1: a buffer resource per B row), allocated
    uninitialised with only the rows hot_wide_matrix() reads written. Bit for bit the piece
    oracle on the compacted B (the same entries in the same order). args: n, boff."""
    from spmm_hip import ops
    torch = _torch()
    a = case.args
    n, k, ldb = a["n"], HOT_WIDE_K, HOT_WIDE_LDB
    rp, ci, v, used = hot_wide_matrix()
    m = rp.size - 1
    rng = np.random.default_rng(9)
    Bs = rng.uniform(-1, 1, (used.size, n)).astype(np.float32)
    C0 = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    buf = torch.empty(k * ldb + 4, dtype=torch.float32, device="cuda")
    dB = buf[a["boff"]:]
    dB[:k * ldb].view(k, ldb)[torch.from_numpy(used.astype(np.int64)).cuda(), :n] = \
        torch.from_numpy(Bs).cuda()
    dC, chkC = framed(C0, n, 0)
    drp, dci, dv = _dev(rp, ci, v)
    h.set_csr_options(1)
    with h.launch_record() as rec:
        tag = ops.csr_hot_analysis(dci, n=n, k=k, hot_bytes=40 * 4 * n, handle=h)
        ops.csrmm_hot(drp, tag, dv, dB, m=m, n=n, k=k, ldb=ldb, C=dC, ldc=n, alpha=ALPHA,
                      beta=BETA, handle=h)
    torch.cuda.synchronize()
    ntag = int((tag < 0).sum())
    assert 0 < ntag < ci.size, f"{case.id}: {ntag} of {ci.size} entries tagged hot"
    got = chkC(case.id)
    small = np.searchsorted(used, ci).astype(np.int32)
    want = oracle_csrmm_pieces_f32(oracle, m, n, rp, small, v, Bs, n, 0, ALPHA, BETA,
                                   C0.reshape(-1), n, 0).reshape(m, n)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        f"{case.id}: differs from the piece oracle in " \
        f"{int((got.view(np.uint32) != want.view(np.uint32)).sum())} elements"
    return rec


def run_grouped32_captured_fill(case, oracle, h):
    """bsr32_grp_fill_kernel: the bs 32 group analysis of ROW blocks fills from the blocks
    themselves (and not from its compact column copy) when the filling call is captured
    (csrc/group.cpp). The size query runs eagerly, the filling call is captured on the
    handle's stream and replayed, and the grouped product on that buffer is checked."""
    from ctypes import byref, c_size_t, c_void_p
    from spmm_hip import ops
    from spmm_hip._lib import lib
    torch = _torch()
    mb, kb, bs, n, W = 37, 60, 32, 132, 2
    rng = np.random.default_rng(72)
    rp, ci, v = column_sparse_bsr(rng, mb, kb, bs, 0.3)
    Bd = rng.uniform(-1, 1, (kb * bs, n)).astype(np.float32)
    C0 = rng.uniform(-1, 1, (mb * bs, n)).astype(np.float32)
    dB, chkB, ldb, dC, ldc, extract = framed_operands(Bd, C0, (4, 4, 4, 4), 0, 0)
    drp, dci, dv = _dev(rp, ci, v)
    s = torch.cuda.Stream()
    hs = None
    with torch.cuda.stream(s):
        hs = ops.Handle(s)
        with hs.launch_record() as rec:
            eager = ops.GroupedBsr32(drp, dci, dv, mb=mb, group_rows=W, handle=hs)  # grows buffers
            fn = lib().spmm_bsr32_group_analysis_f32
            args = (hs.raw, 0, mb, int(ci.size), W, c_void_p(drp.data_ptr()),
                    c_void_p(dci.data_ptr()), c_void_p(dv.data_ptr()))
            size = c_size_t(0)
            assert fn(*args, None, byref(size)) == 0 and size.value == eager.bytes
            buf = torch.zeros(size.value, dtype=torch.uint8, device="cuda")
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                hs.set_stream(s)
                st = fn(*args, c_void_p(buf.data_ptr()), byref(size))
            assert st == 0
            g.replay()
            s.synchronize()
            assert torch.equal(buf, eager.buffer[:size.value]), \
                case.id + ": the block fill differs from the one-pass fill"
            assert lib().spmm_bsrmm_grouped_f32(
                hs.raw, mb, kb, n, c_void_p(buf.data_ptr()), ALPHA, c_void_p(dB.data_ptr()), ldb,
                0, BETA, c_void_p(dC.data_ptr()), ldc, 0) == 0
            s.synchronize()
        eager.close()
    hs.close()
    got = extract(case.id)
    chkB.unchanged(case.id + ": B")
    ref, absd = oracle_bsrmm_f64(oracle, 0, mb, n, bs, rp, ci, v, Bd, n, 0)
    _check_product(got, ref, absd, C0, TOL_F32, case.id)
    _grouped32_bits(oracle, got, mb, n, rp, ci, v, Bd, C0, case.id)
    return rec


def run_hybrid(case, oracle, h):
    """ops.hybrid_csrmm on helpers.hybrid_ex_parts(bs) (the 700 x 700 community matrix).
    args: bs, n, ob, oc, boff, coff, pad_b, pad_c, hybrid_flags."""
    from spmm_hip import ops
    torch = _torch()
    a = case.args
    bs, n, ob, oc = a["bs"], a["n"], a["ob"], a["oc"]
    parts = hybrid_ex_parts(bs)
    crp, cci, cv, brp, bci, bv = parts
    m = k = HYBRID_EX_M
    mpad = -(-m // bs) * bs
    rng = np.random.default_rng(8)
    Bd = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    C0 = rng.uniform(-1, 1, (mpad, n)).astype(np.float32)
    # a row-major B is read up to the last block's rows: whole blocks of rows
    Bfull = np.zeros((mpad, n), np.float32)
    Bfull[:k] = Bd
    dB, chkB, ldb, dC, ldc, extract = framed_operands(
        Bfull if ob == 0 else Bd, C0, (a["boff"], a["pad_b"], a["coff"], a["pad_c"]), ob, oc)
    d = _dev(*parts)
    h.set_hybrid_options(a["hybrid_flags"])
    with h.launch_record() as rec:
        ops.hybrid_csrmm(tuple(d[:3]), tuple(d[3:]), dB, m=m, n=n, k=k, bs=bs, ldb=ldb, C=dC,
                         ldc=ldc, alpha=ALPHA, beta=BETA, order_b=ob, order_c=oc, handle=h)
    torch.cuda.synchronize()
    got = extract(case.id)
    chkB.unchanged(case.id + ": B")
    r1, a1 = oracle_csrmm_f64(oracle, m, n, crp, cci, cv, Bd, n, 0)
    r2, a2 = oracle_bsrmm_f64(oracle, 0, mpad // bs, n, bs, brp, bci, bv, Bfull, n, 0)
    ref, absd = r2.copy(), a2.copy()
    ref[:m] += r1
    absd[:m] += a1
    # every row of C, the rows m .. mpad that only the BSR part writes included
    _check_product(got, ref, absd, C0, TOL_F32, case.id)
    return rec


def run_grouped(case, oracle, h):
    """ops.GroupedBsr32 / GroupedBsr16 (.mm) on a 37 x 60 column-sparse matrix. args: bs
    (32 fp32, 16 fp16), W (group_rows), rowd, n, ob, oc."""
    from spmm_hip import ops
    torch = _torch()
    a = case.args
    bs, n, ob, oc, rowd = a["bs"], a["n"], a["ob"], a["oc"], a["rowd"]
    f16 = bs == 16
    mb, kb = 37, 60
    rng = np.random.default_rng(40 + bs)
    rp, ci, v = column_sparse_bsr(rng, mb, kb, bs, 0.3)
    vt = np.float16 if f16 else np.float32
    v = v.astype(vt)
    Bd = rng.uniform(-1, 1, (kb * bs, n)).astype(vt)
    C0 = rng.uniform(-1, 1, (mb * bs, n)).astype(np.float32)
    lay = (8, 8, 4, 4) if f16 else (4, 4, 4, 4)
    dB, chkB, ldb, dC, ldc, extract = framed_operands(Bd, C0, lay, ob, oc)
    src = v if rowd else np.ascontiguousarray(v.reshape(-1, bs, bs).transpose(0, 2, 1)).reshape(-1)
    drp, dci, dv = _dev(rp, ci, src)
    G = ops.GroupedBsr16 if f16 else ops.GroupedBsr32
    with h.launch_record() as rec:
        with G(drp, dci, dv, mb=mb, group_rows=a["W"], direction=1 - rowd, handle=h) as g:
            assert g.W == a["W"]
            g.mm(dB, kb=kb, n=n, ldb=ldb, C=dC, ldc=ldc, order_b=ob, order_c=oc, alpha=ALPHA,
                 beta=BETA)
    torch.cuda.synchronize()
    got = extract(case.id)
    chkB.unchanged(case.id + ": B")
    ref, absd = oracle_bsrmm_f64(oracle, 0, mb, n, bs, rp, ci, v, Bd, n, 0, half=f16)
    _check_product(got, ref, absd, C0, TOL_F16_ACC if f16 else TOL_F32, case.id)
    if not f16:  # the grouped bs 32 stream: the drop-in's bits, which are the oracle's
        _grouped32_bits(oracle, got, mb, n, rp, ci, v, Bd, C0, case.id)
    return rec


def _grouped32_bits(oracle, got, mb, n, rp, ci, v, Bd, C0, what):
    want = oracle_bsrmm_f32(oracle, 0, mb, n, 32, rp, ci, v, Bd, n, 0, ALPHA, BETA,
                            C0.reshape(-1), n, 0).reshape(mb * 32, n)
    whole = np.repeat(np.diff(rp) <= 64, 32)
    _same_bits(got[whole], want[whole], what)


def run_f64(case, oracle, h):
    """ops.csrmm / ops.bsrmm on float64 operands. args: kind ("csr" / "bsr"), n, ob, oc."""
    from spmm_hip import ops
    torch = _torch()
    a = case.args
    n, ob, oc = a["n"], a["ob"], a["oc"]
    rng = np.random.default_rng(64)
    if a["kind"] == "csr":
        m, k = 301, 257
        rp, ci, v = rand_csr_rows(rng, m, k, 9)
        rows_b, rows_c = k, m
    else:
        mb, kb, bs = 19, 17, 5
        rp, ci, v = rand_bsr(rng, mb, kb, bs, 0.2, empty_rows=(2,))
        rows_b, rows_c = kb * bs, mb * bs
    v = v.astype(np.float64)
    Bd = rng.standard_normal((rows_b, n))
    C0 = rng.standard_normal((rows_c, n))
    dB, chkB, ldb, dC, ldc, extract = framed_operands(Bd, C0, (1, 3, 2, 1), ob, oc)
    drp, dci, dv = _dev(rp, ci, v)
    with h.launch_record() as rec:
        if a["kind"] == "csr":
            ops.csrmm(drp, dci, dv, dB, m=m, n=n, k=k, ldb=ldb, order_b=ob, C=dC, ldc=ldc,
                      order_c=oc, alpha=ALPHA, beta=BETA, handle=h)
            want = oracle_csrmm_d(oracle, m, n, rp, ci, v, Bd, n, 0, ALPHA, BETA, C0.reshape(-1),
                                  n, 0)
            absd = np.abs(oracle_csrmm_d(oracle, m, n, rp, ci, np.abs(v), np.abs(Bd), n, 0,
                                         abs(ALPHA), abs(BETA), np.abs(C0).reshape(-1), n, 0))
        else:
            ops.bsrmm(drp, dci, dv, dB, mb=mb, kb=kb, n=n, bs=bs, ldb=ldb, order_b=ob, C=dC,
                      ldc=ldc, order_c=oc, alpha=ALPHA, beta=BETA, handle=h)
            want = oracle_bsrmm_d(oracle, 0, mb, n, bs, rp, ci, v, Bd, n, 0, ALPHA, BETA,
                                  C0.reshape(-1), n, 0)
            absd = np.abs(oracle_bsrmm_d(oracle, 0, mb, n, bs, rp, ci, np.abs(v), np.abs(Bd), n,
                                         0, abs(ALPHA), abs(BETA), np.abs(C0).reshape(-1), n, 0))
    torch.cuda.synchronize()
    got = extract(case.id)
    chkB.unchanged(case.id + ": B")
    # sequential fp64 chains in another order than the oracle's at most: a few ulp of |a||b|
    assert_normwise(got, want.reshape(rows_c, n), absd.reshape(rows_c, n), 1e-12, case.id)
    return rec


def run_sddmm(case, oracle, h):
    """ops.sddmm against prep.sddmm (the written association rule), bit for bit. args: n,
    xoff (elements X starts off 16 bytes), pad (added to ldx and ldy)."""
    from spmm_hip import ops, prep
    torch = _torch()
    a = case.args
    n = a["n"]
    m, k = 150, 130
    rng = np.random.default_rng(90 + n)
    rp, ci, _ = rand_csr_rows(rng, m, k, 9)
    nnz = int(rp[-1])
    X = rng.uniform(-1, 1, (m, max(n, 1))).astype(np.float32)[:, :n]
    Y = rng.uniform(-1, 1, (k, max(n, 1))).astype(np.float32)[:, :n]
    out0 = rng.uniform(-1, 1, nnz).astype(np.float32)
    ld = n + a["pad"]
    if n:
        dX, chkX = framed(X, ld, a["xoff"])
        dY, chkY = framed(Y, ld, 0)
    else:
        dX, dY = _dev(np.zeros(4, np.float32), np.zeros(4, np.float32))
    dout, chko = framed(out0.reshape(1, -1), nnz, 0)
    drp, dci = _dev(rp, ci)
    with h.launch_record() as rec:
        ops.sddmm(drp, dci, dX, dY, m=m, n=n, k=k, ldx=ld, ldy=ld, out=dout, alpha=ALPHA,
                  beta=BETA, handle=h)
    torch.cuda.synchronize()
    got = chko(case.id).reshape(-1)
    if n:
        chkX.unchanged(case.id + ": X")
        chkY.unchanged(case.id + ": Y")
    if n:
        want = prep.sddmm(m, n, k, rp, ci, np.ascontiguousarray(X), np.ascontiguousarray(Y),
                          out=out0.copy(), alpha=ALPHA, beta=BETA)
    else:  # every dot is +0: fma(beta, out, alpha * 0), one rounding
        want = np.float32(BETA) * out0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        f"{case.id}: {int((got != want).sum())} of {nnz} values differ"
    return rec


def run_csr2csc(case, oracle, h):
    """ops.csr2csc against a stable numpy sort by column. args: n (columns: 1 radix pass
    per byte of n - 1), m, deg, vt (value dtype name or None), perm."""
    from spmm_hip import ops
    torch = _torch()
    a = case.args
    m, n = a["m"], a["n"]
    rng = np.random.default_rng(30 + n % 97)
    if a["deg"]:
        rp, ci, _ = rand_csr_rows(rng, m, n, a["deg"])
    else:
        rp, ci = np.zeros(m + 1, np.int32), np.zeros(0, np.int32)
    nnz = ci.size
    val = None if a["vt"] is None else rng.uniform(-1, 1, nnz).astype(a["vt"])
    drp, dci = _dev(rp, ci)
    dval = None if val is None else _dev(val)[0]
    with h.launch_record() as rec:
        out = ops.csr2csc(drp, dci, dval, m=m, n=n, return_perm=a["perm"], nnz=nnz, handle=h)
    torch.cuda.synchronize()
    rows = np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))
    order = np.argsort(ci, kind="stable")
    colptr = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=n))]).astype(np.int32)
    assert np.array_equal(out[0].cpu().numpy(), colptr), case.id + ": colptr"
    assert np.array_equal(out[1].cpu().numpy(), rows[order]), case.id + ": rowind"
    i = 2
    if val is not None:
        assert np.array_equal(out[i].cpu().numpy().view(np.uint8), val[order].view(np.uint8)), \
            case.id + ": val"
        i += 1
    if a["perm"]:
        assert np.array_equal(out[i].cpu().numpy(), order.astype(np.int32)), case.id + ": perm"
    return rec


def run_convert(case, oracle, h):
    """The device converters against prep's host forms / numpy. args: op ("csr2bsr",
    "bsr2csr", "coo2csr", "reblock32"), bs, rowd."""
    from spmm_hip import ops, prep
    torch = _torch()
    a = case.args
    op, bs, rowd = a["op"], a.get("bs", 0), a.get("rowd", 1)
    rng = np.random.default_rng(50 + bs)

    def blocks(v, b):  # ROW-direction values as the direction under test stores them
        return v if rowd else np.ascontiguousarray(
            v.reshape(-1, b, b).transpose(0, 2, 1)).reshape(-1)
    with h.launch_record() as rec:
        if op == "coo2csr":
            m = 1000
            rp, _, _ = rand_csr_rows(rng, m, 50, 6)
            coo = np.repeat(np.arange(m, dtype=np.int32), np.diff(rp)) + 1
            got = ops.coo2csr(_dev(coo)[0], m, base=1, handle=h).cpu().numpy()
            assert np.array_equal(got, rp + 1), case.id
        elif op == "csr2bsr":
            m, n = 301, 203  # neither a multiple of bs
            rp, ci, v = rand_csr_rows(rng, m, n, 9)
            brp, bci, bv = prep.csr2bsr(m, n, rp, ci, v, bs)
            g = ops.csr2bsr(*_dev(rp, ci, v), m=m, n=n, bs=bs, direction=1 - rowd, handle=h)
            for got, want, nm in zip(g, (brp, bci, blocks(bv, bs)), ("rowptr", "colind", "val")):
                assert np.array_equal(got.cpu().numpy().view(np.uint32),
                                      np.asarray(want).view(np.uint32)), f"{case.id}: {nm}"
        elif op == "bsr2csr":
            mb, nb = 23, 17
            rp, ci, v = rand_bsr(rng, mb, nb, bs, 0.2, empty_rows=(4,))
            g = ops.bsr2csr(*_dev(rp, ci, blocks(v, bs)), mb=mb, nb=nb, bs=bs,
                            direction=1 - rowd, handle=h)
            v3 = v.reshape(-1, bs, bs)
            crp, cci, cv = [0], [], []
            for br in range(mb):
                for r in range(bs):
                    for j in range(rp[br], rp[br + 1]):
                        cci.append(ci[j] * bs + np.arange(bs))
                        cv.append(v3[j, r])
                    crp.append(crp[-1] + (rp[br + 1] - rp[br]) * bs)
            want = (np.array(crp, np.int32), np.concatenate(cci).astype(np.int32),
                    np.concatenate(cv).astype(np.float32))
            for got, w, nm in zip(g, want, ("rowptr", "colind", "val")):
                assert np.array_equal(got.cpu().numpy().view(np.uint32), w.view(np.uint32)), \
                    f"{case.id}: {nm}"
        else:  # reblock32: the dense matrix of the result equals the dense matrix of the input
            mb, kb = 37, 29
            rp, ci, v = rand_bsr(rng, mb, kb, bs, 0.2, empty_rows=(4,))
            g = ops.bsr_reblock32(*_dev(rp, ci, blocks(v, bs)), mb=mb, bs=bs, direction=1 - rowd,
                                  handle=h)
            rp32, ci32, v32 = [t.cpu().numpy() for t in g]

            def dense(rp_, ci_, v_, b, nbr, nbc):
                D = np.zeros((nbr * b, nbc * b), np.float32)
                v_ = v_.reshape(-1, b, b)
                for br in range(nbr):
                    for j in range(rp_[br], rp_[br + 1]):
                        blk = v_[j] if rowd else v_[j].T
                        D[br * b:(br + 1) * b, ci_[j] * b:(ci_[j] + 1) * b] = blk
                return D
            R = 32 // bs
            mb32, kb32 = -(-mb // R), -(-kb // R)
            want = np.zeros((mb32 * 32, kb32 * 32), np.float32)
            want[:mb * bs, :kb * bs] = dense(rp, ci, blocks(v, bs), bs, mb, kb)
            assert rp32.size == mb32 + 1 and np.all(np.diff(rp32) >= 0), case.id
            for br in range(mb32):
                assert np.all(np.diff(ci32[rp32[br]:rp32[br + 1]]) > 0), f"{case.id}: unsorted"
            got = dense(rp32, ci32, v32, 32, mb32, kb32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), case.id
            # exactly the 32 x 32 blocks that hold an input block
            occ = {(br // R, c // R) for br in range(mb) for c in ci[rp[br]:rp[br + 1]]}
            assert int(rp32[-1]) == len(occ), case.id
    torch.cuda.synchronize()
    return rec


def run_flat_transpose16(case, oracle, h):
    """transpose16x4_kernel<true>: ops.bsrmm_f16 at bs 16 with a column-major B of more than
    64 * 65535 columns, which the entry stages row-major (launch_transpose16 with rows = n).
    One 16 x 16 block; C = A B checked in fp64."""
    from spmm_hip import ops
    torch = _torch()
    bs, n = 16, 64 * 65535 + 8
    rp, ci = np.array([0, 1], np.int32), np.array([0], np.int32)
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, bs * bs).astype(np.float16)
    Bd = rng.uniform(-1, 1, (bs, n)).astype(np.float16)
    C0 = rng.uniform(-1, 1, (bs, n)).astype(np.float32)
    dB, chkB, ldb, dC, ldc, extract = framed_operands(Bd, C0, (3, 1, 4, 0), 1, 0)
    drp, dci, dv = _dev(rp, ci, v)
    with h.launch_record() as rec:
        ops.bsrmm_f16(drp, dci, dv, dB, mb=1, kb=1, n=n, bs=bs, ldb=ldb, order_b=1, C=dC, ldc=ldc,
                      alpha=ALPHA, beta=BETA, handle=h)
    torch.cuda.synchronize()
    got = extract(case.id)
    chkB.unchanged(case.id + ": B")
    A, B64 = v.reshape(bs, bs).astype(np.float64), Bd.astype(np.float64)
    _check_product(got, A @ B64, np.abs(A) @ np.abs(B64), C0, TOL_F16_ACC, case.id)
    return rec


def run_flat_transpose4(case, oracle, h):
    """transpose4_kernel<true>: ops.csrmm with a column-major C of more than 64 * 65535
    rows, which the entry computes row-major in its workspace and transposes back with beta
    (launch_transpose with rows = m). Every 4099th row holds two entries."""
    from spmm_hip import ops
    torch = _torch()
    m, k, n = 64 * 65535 + 1, 3, 4
    rows = np.arange(0, m, 4099)
    lens = np.zeros(m, np.int32)
    lens[rows] = 2
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.tile(np.array([0, 2], np.int32), rows.size)
    rng = np.random.default_rng(4)
    v = rng.uniform(-1, 1, ci.size).astype(np.float32)
    Bd = rng.uniform(-1, 1, (k, n)).astype(np.float32)
    C0 = rng.uniform(-1, 1, (m, n)).astype(np.float32)
    dB, chkB, ldb, dC, ldc, extract = framed_operands(Bd, C0, (0, 0, 0, 0), 0, 1)
    drp, dci, dv = _dev(rp, ci, v)
    with h.launch_record() as rec:
        ops.csrmm(drp, dci, dv, dB, m=m, n=n, k=k, ldb=ldb, C=dC, ldc=ldc, order_c=1,
                  alpha=ALPHA, beta=BETA, handle=h)
    torch.cuda.synchronize()
    got = extract(case.id)
    chkB.unchanged(case.id + ": B")
    ref, absd = np.zeros((m, n)), np.zeros((m, n))
    v2, B64 = v.reshape(-1, 2).astype(np.float64), Bd.astype(np.float64)
    ref[rows] = v2[:, :1] * B64[0] + v2[:, 1:] * B64[2]
    absd[rows] = np.abs(v2[:, :1] * B64[0]) + np.abs(v2[:, 1:] * B64[2])
    _check_product(got, ref, absd, C0, TOL_F32, case.id)
    return rec


RUNNERS = {"flat_transpose4": run_flat_transpose4, "csrmm_hot_wide": run_csr_hot_wide,
           "grouped32_captured_fill": run_grouped32_captured_fill,
           "bsrmm": run_bsr, "bsrmm_f16": run_bsr, "bsrmm_analysed": run_bsr,
           "bsrmm_analysed_f16": run_bsr, "csrmm": run_csr, "csrmm_f16": run_csr,
           "csrmm_hot": run_csr, "hybrid_csrmm": run_hybrid, "grouped": run_grouped,
           "f64": run_f64, "sddmm": run_sddmm, "csr2csc": run_csr2csc, "convert": run_convert,
           "flat_transpose16": run_flat_transpose16}


# -------------------------------------------------------------------- the table
def B(**kw):
    d = dict(rowd=1, ob=0, oc=0, voff=0, boff=0, coff=0, pad_b=0, pad_c=0, shape="shallow",
             bsr_flags=0)
    d.update(kw)
    return d


def Cs(**kw):
    d = dict(m=300, k=500, ob=0, oc=0, boff=0, coff=0, pad_b=0, pad_c=0, csr_flags=1)
    d.update(kw)
    return d


def H(**kw):
    d = dict(bs=32, ob=0, oc=0, boff=0, coff=0, pad_b=0, pad_c=0, hybrid_flags=0)
    d.update(kw)
    return d


def _sddmm_cases():
    """sddmm_kernel<G, NC, VEC, FULL> at every (G, NC): G lanes per position (the smallest
    power of two >= ceil(n / 4), at most 64), NC chunks per lane; VEC needs n % 4 == 0 with
    16-byte X, Y and leading dimensions; FULL is n % (4 G) == 0."""
    out = []

    def add(n, xoff, pad, G, NC, vec, full):
        out.append(Case(f"sddmm-n{n}-xoff{xoff}-pad{pad}", "sddmm", dict(n=n, xoff=xoff, pad=pad),
                        (f"12sddmm_kernelILi{G}ELi{NC}ELb{int(vec)}ELb{int(full)}EE",)))
    for G, NC in [(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3),
                  (64, 4)]:
        nfull = 4 * G * NC
        add(nfull, 0, 0, G, NC, True, True)
        add(nfull, 1, 0, G, NC, False, True)   # X off 16 bytes
        add(nfull - 1, 0, 1, G, NC, False, False)  # n % 4 != 0 (ld stays a multiple of 4)
        if G > 2:
            add(nfull - 4, 0, 4, G, NC, True, False)
    out.append(Case("sddmm-wide-vec", "sddmm", dict(n=1028, xoff=0, pad=0),
                    ("17sddmm_wide_kernelILb1EE",)))
    out.append(Case("sddmm-wide-scalar", "sddmm", dict(n=1027, xoff=0, pad=2),
                    ("17sddmm_wide_kernelILb0EE",)))
    out.append(Case("sddmm-n0", "sddmm", dict(n=0, xoff=0, pad=0), ("17sddmm_zero_kernelE",)))
    return out


def _other_cases():
    out = _sddmm_cases()
    # csr2csc: one radix pass per byte of n - 1 (digit_count / digit_scatter <first, last>),
    # the one-workgroup scan up to 16,384 counts and the chunked scan past it, every value
    # width of the gather, and the empty matrix
    scan1 = ("11scan_kernelE",)
    out += [
        Case("csr2csc-1pass-f32", "csr2csc", dict(m=400, n=200, deg=9, vt="float32", perm=False),
             ("16col_count_kernelEiiiPKi", "18digit_count_kernelILb1EE",
              "20digit_scatter_kernelILb1ELb1EE", "18expand_rows_kernelE",
              "17csc_gather_kernelILi4EE") + scan1),
        Case("csr2csc-2pass-f16-perm", "csr2csc",
             dict(m=400, n=5000, deg=9, vt="float16", perm=True),
             ("18digit_count_kernelILb0EE", "20digit_scatter_kernelILb1ELb0EE",
              "20digit_scatter_kernelILb0ELb1EE", "17csc_gather_kernelILi2EE")),
        Case("csr2csc-3pass-f64", "csr2csc",
             dict(m=3000, n=70000, deg=40, vt="float64", perm=False),
             ("20digit_scatter_kernelILb0ELb0EE", "17csc_gather_kernelILi8EE",
              "16chunk_sum_kernelE", "17chunk_scan_kernelE")),
        Case("csr2csc-pattern", "csr2csc", dict(m=400, n=300, deg=9, vt=None, perm=True),
             ("17csc_gather_kernelILi0EE",)),
        Case("csr2csc-empty", "csr2csc", dict(m=10, n=1000, deg=0, vt="float32", perm=False),
             ("15fill_int_kernelE",)),
    ]
    # converters
    out.append(Case("coo2csr", "convert", dict(op="coo2csr"), ("14coo2csr_kernelE",)))
    for rowd in (1, 0):
        out.append(Case(f"csr2bsr-bs5-rowd{rowd}", "convert", dict(op="csr2bsr", bs=5, rowd=rowd),
                        ("14csr2bsr_kernelILb0ELb1EE", f"14csr2bsr_kernelILb1ELb{rowd}EE",
                         "11scan_kernelE")))
        out.append(Case(f"bsr2csr-bs5-rowd{rowd}", "convert", dict(op="bsr2csr", bs=5, rowd=rowd),
                        (f"14bsr2csr_kernelILb{rowd}EE",)))
    for bs, rowd in ((8, 1), (4, 0), (16, 1)):
        out.append(Case(f"reblock32-bs{bs}-rowd{rowd}", "convert",
                        dict(op="reblock32", bs=bs, rowd=rowd),
                        ("16reblock32_kernelILb0EE", "16reblock32_kernelILb1EE",
                         "23reblock32_values_kernelE", "11scan_kernelE")))
    # fp64
    for kind, k in (("csr", "14csr_f64_kernelE"), ("bsr", "14bsr_f64_kernelE")):
        for ob, oc in ((0, 0), (1, 1)):
            out.append(Case(f"f64-{kind}-ob{ob}-oc{oc}", "f64", dict(kind=kind, n=70, ob=ob, oc=oc),
                            (k,)))
    # the group analyses and the grouped products: every W, both directions (the bs 32
    # analysis fills COLUMN blocks from the values, ROW blocks from its compact column
    # copy), both C orders of the fp16 product
    for W in (2, 4):
        for rowd in (1, 0):
            out.append(Case(f"grouped32-W{W}-rowd{rowd}", "grouped",
                            dict(bs=32, W=W, rowd=rowd, n=132, ob=0, oc=0),
                            (f"16grp_build_kernelILi{W}ELi32ELb0EE",
                             f"16grp_build_kernelILi{W}ELi32ELb1EE", "17grp_mask32_kernelE",
                             "16grp_stats_kernelE", "11scan_kernelE", "16grp_wmask_kernelILi8EE",
                             "22bsr32_grp_fillc_kernelE",
                             f"20bsr32_f32_grp_kernelILi{W}ELi3ELi3ELb0EE")))
    for W in (2, 4, 8):
        for oc in (0, 1):
            out.append(Case(f"grouped16-W{W}-oc{oc}", "grouped",
                            dict(bs=16, W=W, rowd=1 - oc, n=264, ob=0, oc=oc),
                            (f"16grp_build_kernelILi{W}ELi16ELb0EE",
                             f"16grp_build_kernelILi{W}ELi16ELb1EE", "17grp_mask16_kernelE",
                             "16grp_wmask_kernelILi16EE", "21bsr16_grp_fill_kernelE",
                             f"20bsr16_f16_grp_kernelILi{W}ELi3ELb{1 - oc}ELi3ELi1ELb0EE")))
    out.append(Case("grouped32-captured-fill", "grouped32_captured_fill", {},
                    ("21bsr32_grp_fill_kernelE", "20bsr32_f32_grp_kernelILi2ELi3ELi3ELb0EE")))
    out.append(Case("flat-transpose4", "flat_transpose4", {}, ("17transpose4_kernelILb1EE",)))
    out.append(Case("flat-transpose16", "flat_transpose16", {},
                    ("20transpose16x4_kernelILb1EE",)))
    return out


# The BSR / CSR / hybrid cases, chosen over the dispatch trace's grid (module docstring).
# --- generated table begin
TRACED_CASES = [
    Case("bsrmm-bs32-n64-row-br-cr-wide", "bsrmm",
         B(shape='wide', bs=32, n=64),
         ("16seg_build_kernelEiPKiiiiiiP",
          "20bsr32_f32_cs2_kernelILb1ELb0ELb1ELb0ELb0ELb1EEEviiPKi",
          "16seg_fixup_kernelEiPK",)),
    Case("bsrmm_analysed-bs32-n64-col-br-cr-wide", "bsrmm_analysed",
         B(rowd=0, shape='wide', bs=32, n=64),
         ("16seg_build_kernelEiPKiiiiiiP",
          "20bsr32_f32_cs2_kernelILb1ELb0ELb1ELb1ELb0ELb1EEEviiPKi",
          "16seg_fixup_kernelEiPK",
          "21bsr32_analysis_kernelEiiPKfPjPf",)),
    Case("bsrmm-bs32-n132-row-br-cr-wide", "bsrmm",
         B(shape='wide', bs=32, n=132),
         ("16seg_build_kernelEiPKiiiiiiP",
          "20bsr32_f32_cs2_kernelILb1ELb0ELb1ELb0ELb0ELb0EEEviiPKi",
          "16seg_fixup_kernelEiPK",)),
    Case("bsrmm_analysed-bs32-n132-col-br-cr-wide", "bsrmm_analysed",
         B(rowd=0, shape='wide', bs=32, n=132),
         ("16seg_build_kernelEiPKiiiiiiP",
          "20bsr32_f32_cs2_kernelILb1ELb0ELb1ELb1ELb0ELb0EEEviiPKi",
          "16seg_fixup_kernelEiPK",
          "21bsr32_analysis_kernelEiiPKfPjPf",)),
    Case("bsrmm-bs32-n64-row-br-cc-wide", "bsrmm",
         B(oc=1, shape='wide', bs=32, n=64),
         ("22block_row_order_kernelEiPKi",
          "20bsr32_f32_cs2_kernelILb0ELb0ELb1ELb0ELb0ELb1EEEviiPKi",)),
    Case("bsrmm_analysed-bs32-n64-col-br-cc-wide", "bsrmm_analysed",
         B(rowd=0, oc=1, shape='wide', bs=32, n=64),
         ("22block_row_order_kernelEiPKi",
          "20bsr32_f32_cs2_kernelILb0ELb0ELb1ELb1ELb0ELb1EEEviiPKi",
          "21bsr32_analysis_kernelEiiPKfPjPf",)),
    Case("bsrmm-bs32-n132-row-br-cc-wide", "bsrmm",
         B(oc=1, shape='wide', bs=32, n=132),
         ("22block_row_order_kernelEiPKi",
          "20bsr32_f32_cs2_kernelILb0ELb0ELb1ELb0ELb0ELb0EEEviiPKi",)),
    Case("bsrmm_analysed-bs32-n132-col-br-cc-wide", "bsrmm_analysed",
         B(rowd=0, oc=1, shape='wide', bs=32, n=132),
         ("22block_row_order_kernelEiPKi",
          "20bsr32_f32_cs2_kernelILb0ELb0ELb1ELb1ELb0ELb0EEEviiPKi",
          "21bsr32_analysis_kernelEiiPKfPjPf",)),
    Case("bsrmm-bs64-n64-row-br-cr-wide", "bsrmm",
         B(shape='wide', bs=64, n=64),
         ("22block_row_order_kernelEiPKi",
          "20bsr32_f32_cs2_kernelILb1ELb0ELb1ELb0ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs64-n132-row-br-cr-wide", "bsrmm",
         B(shape='wide', bs=64, n=132),
         ("22block_row_order_kernelEiPKi",
          "20bsr32_f32_cs2_kernelILb1ELb0ELb1ELb0ELb1ELb0EEEviiPKi",)),
    Case("bsrmm-bs64-n64-row-br-cc-wide", "bsrmm",
         B(oc=1, shape='wide', bs=64, n=64),
         ("22block_row_order_kernelEiPKi",
          "20bsr32_f32_cs2_kernelILb0ELb0ELb1ELb0ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs64-n132-row-br-cc-wide", "bsrmm",
         B(oc=1, shape='wide', bs=64, n=132),
         ("22block_row_order_kernelEiPKi",
          "20bsr32_f32_cs2_kernelILb0ELb0ELb1ELb0ELb1ELb0EEEviiPKi",)),
    Case("bsrmm-bs32-n8-row-br-cr-panel", "bsrmm",
         B(shape='panel', bs=32, n=8),
         ("16seg_build_kernelEiPKiiiiiiP",
          "20bsr32_f32_cs2_kernelILb1ELb1ELb1ELb0ELb0ELb1EEEviiPKi",
          "16seg_fixup_kernelEiPK",)),
    Case("bsrmm-bs32-n68-row-br-cr-panel", "bsrmm",
         B(shape='panel', bs=32, n=68),
         ("16seg_build_kernelEiPKiiiiiiP",
          "20bsr32_f32_cs2_kernelILb1ELb1ELb1ELb0ELb0ELb0EEEviiPKi",
          "16seg_fixup_kernelEiPK",)),
    Case("bsrmm-bs32-n8-row-br-cc-panel", "bsrmm",
         B(oc=1, shape='panel', bs=32, n=8),
         ("22block_row_order_kernelEiPKi",
          "18panel_probe_kernelExiiPKfPy",
          "20bsr32_f32_cs2_kernelILb0ELb1ELb1ELb0ELb0ELb1EEEviiPKi",
          "22bsr32_f32_panel_kernelILb0ELb1ELb0EEEviiPKi",),
         idle=("20bsr32_f32_cs2_kernelILb0ELb1ELb1ELb0ELb0ELb1EEEviiPKi",)),
    Case("bsrmm-bs32-n68-row-br-cc-panel", "bsrmm",
         B(oc=1, shape='panel', bs=32, n=68),
         ("22block_row_order_kernelEiPKi",
          "18panel_probe_kernelExiiPKfPy",
          "20bsr32_f32_cs2_kernelILb0ELb1ELb1ELb0ELb0ELb0EEEviiPKi",
          "22bsr32_f32_panel_kernelILb0ELb0ELb0EEEviiPKi",),
         idle=("20bsr32_f32_cs2_kernelILb0ELb1ELb1ELb0ELb0ELb0EEEviiPKi",)),
    Case("bsrmm-bs64-n8-row-br-cr-panel", "bsrmm",
         B(shape='panel', bs=64, n=8),
         ("22block_row_order_kernelEiPKi",
          "18panel_probe_kernelExiiPKfPy",
          "20bsr32_f32_cs2_kernelILb1ELb1ELb1ELb0ELb1ELb1EEEviiPKi",
          "22bsr32_f32_panel_kernelILb1ELb1ELb1EEEviiPKi",),
         idle=("20bsr32_f32_cs2_kernelILb1ELb1ELb1ELb0ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs64-n68-row-br-cr-panel", "bsrmm",
         B(shape='panel', bs=64, n=68),
         ("22block_row_order_kernelEiPKi",
          "18panel_probe_kernelExiiPKfPy",
          "20bsr32_f32_cs2_kernelILb1ELb1ELb1ELb0ELb1ELb0EEEviiPKi",
          "22bsr32_f32_panel_kernelILb1ELb0ELb1EEEviiPKi",),
         idle=("20bsr32_f32_cs2_kernelILb1ELb1ELb1ELb0ELb1ELb0EEEviiPKi",)),
    Case("bsrmm-bs64-n8-row-br-cc-panel", "bsrmm",
         B(oc=1, shape='panel', bs=64, n=8),
         ("22block_row_order_kernelEiPKi",
          "18panel_probe_kernelExiiPKfPy",
          "20bsr32_f32_cs2_kernelILb0ELb1ELb1ELb0ELb1ELb1EEEviiPKi",
          "22bsr32_f32_panel_kernelILb0ELb1ELb1EEEviiPKi",),
         idle=("20bsr32_f32_cs2_kernelILb0ELb1ELb1ELb0ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs64-n68-row-br-cc-panel", "bsrmm",
         B(oc=1, shape='panel', bs=64, n=68),
         ("22block_row_order_kernelEiPKi",
          "18panel_probe_kernelExiiPKfPy",
          "20bsr32_f32_cs2_kernelILb0ELb1ELb1ELb0ELb1ELb0EEEviiPKi",
          "22bsr32_f32_panel_kernelILb0ELb0ELb1EEEviiPKi",),
         idle=("20bsr32_f32_cs2_kernelILb0ELb1ELb1ELb0ELb1ELb0EEEviiPKi",)),
    Case("bsrmm-bs32-n8-row-br-cr-deep-panel", "bsrmm",
         B(shape='deep-panel', bs=32, n=8),
         ("18panel_probe_kernelExiiPKfPy",
          "20bsr32_f32_cs2_kernelILb1ELb1ELb1ELb0ELb0ELb1EEEviiPKi",
          "22bsr32_f32_panel_kernelILb1ELb1ELb0EEEviiPKi",),
         idle=("20bsr32_f32_cs2_kernelILb1ELb1ELb1ELb0ELb0ELb1EEEviiPKi",)),
    Case("bsrmm-bs32-n68-row-br-cr-deep-panel", "bsrmm",
         B(shape='deep-panel', bs=32, n=68),
         ("18panel_probe_kernelExiiPKfPy",
          "20bsr32_f32_cs2_kernelILb1ELb1ELb1ELb0ELb0ELb0EEEviiPKi",
          "22bsr32_f32_panel_kernelILb1ELb0ELb0EEEviiPKi",),
         idle=("20bsr32_f32_cs2_kernelILb1ELb1ELb1ELb0ELb0ELb0EEEviiPKi",)),
    Case("bsrmm-bs32-n8-row-br-cr-deep", "bsrmm",
         B(shape='deep', bs=32, n=8),
         ("20bsr32_f32_cs2_kernelILb1ELb1ELb1ELb0ELb0ELb1EEEviiPKi",)),
    Case("bsrmm-bs64-n4-row-br-cc-deep", "bsrmm",
         B(oc=1, shape='deep', bs=64, n=4),
         ("20bsr32_f32_cs2_kernelILb0ELb1ELb1ELb0ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs8-n4-row-br-cr-deep-flags2", "bsrmm",
         B(shape='deep', bsr_flags=2, bs=8, n=4, small_path=2),
         ("22block_row_order_kernelEiPKi",
          "22small_grp_probe_kernelILi8EEEviiPKi",
          "20bsr_small_grp_kernelILi8ELb1ELb1EEEviiPKi",
          "16bsr_small_kernelILi8ELi1ELb1ELb1EEEviiPKi",),
         idle=("20bsr_small_grp_kernelILi8ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs32-n64-row-br-cr-boff4-coff4-padb4-padc4", "bsrmm",
         B(boff=4, coff=4, pad_b=4, pad_c=4, bs=32, n=64),
         ("16seg_build_kernelEiPKiiiiiiP",
          "20bsr32_f32_cs2_kernelILb1ELb1ELb1ELb0ELb0ELb1EEEviiPKi",
          "16seg_fixup_kernelEiPK",)),
    Case("bsrmm-bs32-n64-row-br-cr-voff1", "bsrmm",
         B(voff=1, bs=32, n=64),
         ("18bsr_generic_kernelIfEEviiibPKi",)),
    Case("bsrmm-bs32-n64-row-br-cr-coff1-padc1", "bsrmm",
         B(coff=1, pad_c=1, bs=32, n=64),
         ("21bsr32_f32_mfma_kernelILb1ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs32-n64-row-br-cr-boff1-padb1", "bsrmm",
         B(boff=1, pad_b=1, bs=32, n=64),
         ("21bsr32_f32_mfma_kernelILb1ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs64-n132-row-br-cr-boff4-coff4-padb4-padc4", "bsrmm",
         B(boff=4, coff=4, pad_b=4, pad_c=4, bs=64, n=132),
         ("22block_row_order_kernelEiPKi",
          "20bsr32_f32_cs2_kernelILb1ELb1ELb1ELb0ELb1ELb0EEEviiPKi",)),
    Case("bsrmm-bs64-n132-row-br-cr-voff1", "bsrmm",
         B(voff=1, bs=64, n=132),
         ("18bsr_generic_kernelIfEEviiibPKi",)),
    Case("bsrmm-bs64-n132-row-br-cr-coff1-padc1", "bsrmm",
         B(coff=1, pad_c=1, bs=64, n=132),
         ("18bsr_generic_kernelIfEEviiibPKi",)),
    Case("bsrmm-bs64-n132-row-br-cr-boff1-padb1", "bsrmm",
         B(boff=1, pad_b=1, bs=64, n=132),
         ("18bsr_generic_kernelIfEEviiibPKi",)),
    Case("bsrmm-bs16-n64-row-br-cr-boff4-coff4-padb4-padc4", "bsrmm",
         B(boff=4, coff=4, pad_b=4, pad_c=4, bs=16, n=64),
         ("15bsr16_cm_kernelIfLb1ELi64EEEviiPKi",)),
    Case("bsrmm-bs16-n64-row-br-cr-voff1", "bsrmm",
         B(voff=1, bs=16, n=64),
         ("18bsr_generic_kernelIfEEviiibPKi",)),
    Case("bsrmm-bs16-n64-row-br-cr-coff1-padc1", "bsrmm",
         B(coff=1, pad_c=1, bs=16, n=64),
         ("15bsr16_cm_kernelIfLb1ELi64EEEviiPKi",)),
    Case("bsrmm-bs16-n64-row-br-cr-boff1-padb1", "bsrmm",
         B(boff=1, pad_b=1, bs=16, n=64),
         ("21bsr16_f32_mfma_kernelILb1ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs8-n132-row-br-cr-boff4-coff4-padb4-padc4", "bsrmm",
         B(boff=4, coff=4, pad_b=4, pad_c=4, bs=8, n=132),
         ("16bsr_small_kernelILi8ELi2ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs8-n132-row-br-cr-voff1", "bsrmm",
         B(voff=1, bs=8, n=132),
         ("16bsr_small_kernelILi8ELi2ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs8-n132-row-br-cr-coff1-padc1", "bsrmm",
         B(coff=1, pad_c=1, bs=8, n=132),
         ("16bsr_small_kernelILi8ELi2ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs8-n132-row-br-cr-boff1-padb1", "bsrmm",
         B(boff=1, pad_b=1, bs=8, n=132),
         ("16bsr_small_kernelILi8ELi1ELb1ELb1EEEviiPKi",)),
    Case("bsrmm_f16-bs16-n136-row-br-cr-boff8-coff4-padb8-padc4", "bsrmm_f16",
         B(boff=8, coff=4, pad_b=8, pad_c=4, bs=16, n=136),
         ("22block_row_order_kernelEiPKi",
          "19bsr16_f16_cs_kernelILb1ELb1ELb0EEEviiPKi",)),
    Case("bsrmm_f16-bs16-n136-row-br-cr-voff1", "bsrmm_f16",
         B(voff=1, bs=16, n=136),
         ("18bsr_generic_kernelIDF16_EEviiibPKi",)),
    Case("bsrmm_f16-bs16-n136-row-br-cr-coff1-padc1", "bsrmm_f16",
         B(coff=1, pad_c=1, bs=16, n=136),
         ("22block_row_order_kernelEiPKi",
          "19bsr16_f16_cs_kernelILb1ELb1ELb0EEEviiPKi",)),
    Case("bsrmm_f16-bs16-n136-row-br-cr-boff1-padb1", "bsrmm_f16",
         B(boff=1, pad_b=1, bs=16, n=136),
         ("21bsr16_f16_mfma_kernelILb1ELb1ELb1EEEviiPKi",)),
    Case("bsrmm_analysed-bs32-n132-col-br-cr-boff4-coff4-padb4-padc4", "bsrmm_analysed",
         B(rowd=0, boff=4, coff=4, pad_b=4, pad_c=4, bs=32, n=132),
         ("16seg_build_kernelEiPKiiiiiiP",
          "20bsr32_f32_cs2_kernelILb1ELb1ELb1ELb1ELb0ELb0EEEviiPKi",
          "16seg_fixup_kernelEiPK",
          "21bsr32_analysis_kernelEiiPKfPjPf",)),
    Case("bsrmm_analysed-bs32-n132-col-br-cr-coff1-padc1", "bsrmm_analysed",
         B(rowd=0, coff=1, pad_c=1, bs=32, n=132),
         ("21bsr32_f32_mfma_kernelILb0ELb1ELb1EEEviiPKi",
          "21bsr32_analysis_kernelEiiPKfPjPf",)),
    Case("bsrmm_analysed-bs32-n132-col-br-cr-boff1-padb1", "bsrmm_analysed",
         B(rowd=0, boff=1, pad_b=1, bs=32, n=132),
         ("21bsr32_f32_mfma_kernelILb0ELb1ELb1EEEviiPKi",
          "21bsr32_analysis_kernelEiiPKfPjPf",)),
    Case("hybrid-bs32-n64-br-cr-lay4444", "hybrid_csrmm",
         H(boff=4, coff=4, pad_b=4, pad_c=4, n=64),
         ("22block_row_order_kernelEiPKi",
          "20bsr32_f32_lds_kernelILb1ELb1ELb0EEEviiPKi",)),
    Case("hybrid-bs32-n64-br-cr-lay1113", "hybrid_csrmm",
         H(boff=1, coff=1, pad_b=1, pad_c=3, n=64),
         ("21bsr32_f32_mfma_kernelILb1ELb1ELb1EEEviiPKi",
          "5CsrMpIfE20csr_mergepath_kernelILi1ELb1ELi0EEEviiPKi",)),
    Case("bsrmm-bs32-n132-row-br-cr-long", "bsrmm",
         B(shape='long', bs=32, n=132),
         ("16seg_build_kernelEiPKiiiiiiP",
          "20bsr32_f32_cs2_kernelILb1ELb1ELb1ELb0ELb0ELb0EEEviiPKi",
          "16seg_fixup_kernelEiPK",)),
    Case("bsrmm_analysed-bs32-n132-col-br-cr-long", "bsrmm_analysed",
         B(rowd=0, shape='long', bs=32, n=132),
         ("16seg_build_kernelEiPKiiiiiiP",
          "20bsr32_f32_cs2_kernelILb1ELb1ELb1ELb1ELb0ELb0EEEviiPKi",
          "16seg_fixup_kernelEiPK",
          "21bsr32_analysis_kernelEiiPKfPjPf",)),
    Case("bsrmm_f16-bs16-n136-row-br-cr-long", "bsrmm_f16",
         B(shape='long', bs=16, n=136),
         ("22block_row_order_kernelEiPKi",
          "19bsr16_f16_cs_kernelILb1ELb1ELb0EEEviiPKi",)),
    Case("bsrmm_analysed_f16-bs16-n136-col-br-cr-long", "bsrmm_analysed_f16",
         B(rowd=0, shape='long', bs=16, n=136),
         ("22block_row_order_kernelEiPKi",
          "19bsr16_f16_cs_kernelILb1ELb1ELb1EEEviiPKi",
          "21bsr16_analysis_kernelEiiPKtPjPt",)),
    Case("csrmm_hot-n68-bc-cr", "csrmm_hot",
         Cs(ob=1, n=68),
         ("5CsrMpIfE20csr_mergepath_kernelILi2ELb1ELi2EEEviiPKi",
          "16col_count_kernelExPKiiiPj",
          "17count_hist_kernelEiPKjPj",
          "17hot_select_kernelEPKjxPj",
          "14hot_tag_kernelExPKiiiPKj",
          "17transpose4_kernelILb0EEEviiPKfiPfifj",)),
    Case("bsrmm_f16-bs16-n64-row-bc-cr", "bsrmm_f16",
         B(ob=1, bs=16, n=64),
         ("15bsr16_cm_kernelIDF16_Lb1ELi256EEEviiPKi",
          "20transpose16x4_kernelILb0EEEviiPKtiPtij",)),
    Case("hybrid-bs32-n64-bc-cc-flags0", "hybrid_csrmm",
         H(ob=1, oc=1, n=64),
         ("20bsr32_f32_lds_kernelILb0ELb0ELb0EEEviiPKi",
          "16csr_group_kernelILb1ELi16ELi4ELb0EEEviiPKi",
          "17transpose4_kernelILb0EEEviiPKfiPfifj",)),
    Case("hybrid-bs32-n136-bc-cc-flags5", "hybrid_csrmm",
         H(ob=1, oc=1, hybrid_flags=5, n=136),
         ("20bsr32_f32_lds_kernelILb0ELb0ELb1EEEviiPKi",
          "5CsrMpIfE20csr_mergepath_kernelILi4ELb1ELi0EEEviiPKi",
          "17transpose4_kernelILb0EEEviiPKfiPfifj",)),
    Case("bsrmm-bs2-n64-row-br-cr-shared-flags2", "bsrmm",
         B(shape='shared', bsr_flags=2, bs=2, n=64, small_path=1),
         ("22block_row_order_kernelEiPKi",
          "22small_grp_probe_kernelILi2EEEviiPKi",
          "20bsr_small_grp_kernelILi2ELb1ELb1EEEviiPKi",
          "16bsr_small_kernelILi2ELi1ELb1ELb1EEEviiPKi",),
         idle=("16bsr_small_kernelILi2ELi1ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs4-n64-row-br-cr-shared-flags2", "bsrmm",
         B(shape='shared', bsr_flags=2, bs=4, n=64, small_path=1),
         ("22block_row_order_kernelEiPKi",
          "22small_grp_probe_kernelILi4EEEviiPKi",
          "20bsr_small_grp_kernelILi4ELb1ELb1EEEviiPKi",
          "16bsr_small_kernelILi4ELi1ELb1ELb1EEEviiPKi",),
         idle=("16bsr_small_kernelILi4ELi1ELb1ELb1EEEviiPKi",)),
    Case("csrmm_hot_wide-n256-boff0", "csrmm_hot_wide",
         dict(n=256, boff=0),
         ("5CsrMpIfE20csr_mergepath_kernelILi4ELb1ELi1EEEviiPKi",
          "16col_count_kernelExPKiiiPj",
          "17count_hist_kernelEiPKjPj",
          "17hot_select_kernelEPKjxPj",
          "14hot_tag_kernelExPKiiiPKj",)),
    Case("csrmm_hot_wide-n128-boff0", "csrmm_hot_wide",
         dict(n=128, boff=0),
         ("5CsrMpIfE20csr_mergepath_kernelILi2ELb1ELi1EEEviiPKi",
          "16col_count_kernelExPKiiiPj",
          "17count_hist_kernelEiPKjPj",
          "17hot_select_kernelEPKjxPj",
          "14hot_tag_kernelExPKiiiPKj",)),
    Case("csrmm_hot_wide-n128-boff1", "csrmm_hot_wide",
         dict(n=128, boff=1),
         ("5CsrMpIfE20csr_mergepath_kernelILi1ELb1ELi1EEEviiPKi",
          "16col_count_kernelExPKiiiPj",
          "17count_hist_kernelEiPKjPj",
          "17hot_select_kernelEPKjxPj",
          "14hot_tag_kernelExPKiiiPKj",)),
    Case("bsrmm-bs2-n4-row-br-cr", "bsrmm",
         B(bs=2, n=4),
         ("16bsr_small_kernelILi2ELi1ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs2-n68-row-br-cr", "bsrmm",
         B(bs=2, n=68),
         ("16bsr_small_kernelILi2ELi2ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs2-n4-row-br-cc", "bsrmm",
         B(oc=1, bs=2, n=4),
         ("16bsr_small_kernelILi2ELi1ELb1ELb0EEEviiPKi",)),
    Case("bsrmm-bs2-n68-row-br-cc", "bsrmm",
         B(oc=1, bs=2, n=68),
         ("16bsr_small_kernelILi2ELi2ELb1ELb0EEEviiPKi",)),
    Case("bsrmm-bs2-n4-col-br-cr", "bsrmm",
         B(rowd=0, bs=2, n=4),
         ("16bsr_small_kernelILi2ELi1ELb0ELb1EEEviiPKi",)),
    Case("bsrmm-bs2-n68-col-br-cr", "bsrmm",
         B(rowd=0, bs=2, n=68),
         ("16bsr_small_kernelILi2ELi2ELb0ELb1EEEviiPKi",)),
    Case("bsrmm-bs2-n4-col-br-cc", "bsrmm",
         B(rowd=0, oc=1, bs=2, n=4),
         ("16bsr_small_kernelILi2ELi1ELb0ELb0EEEviiPKi",)),
    Case("bsrmm-bs2-n68-col-br-cc", "bsrmm",
         B(rowd=0, oc=1, bs=2, n=68),
         ("16bsr_small_kernelILi2ELi2ELb0ELb0EEEviiPKi",)),
    Case("bsrmm-bs4-n4-row-br-cr", "bsrmm",
         B(bs=4, n=4),
         ("16bsr_small_kernelILi4ELi1ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs4-n68-row-br-cr", "bsrmm",
         B(bs=4, n=68),
         ("16bsr_small_kernelILi4ELi2ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs4-n4-row-br-cc", "bsrmm",
         B(oc=1, bs=4, n=4),
         ("16bsr_small_kernelILi4ELi1ELb1ELb0EEEviiPKi",)),
    Case("bsrmm-bs4-n68-row-br-cc", "bsrmm",
         B(oc=1, bs=4, n=68),
         ("16bsr_small_kernelILi4ELi2ELb1ELb0EEEviiPKi",)),
    Case("bsrmm-bs4-n4-col-br-cr", "bsrmm",
         B(rowd=0, bs=4, n=4),
         ("16bsr_small_kernelILi4ELi1ELb0ELb1EEEviiPKi",)),
    Case("bsrmm-bs4-n68-col-br-cr", "bsrmm",
         B(rowd=0, bs=4, n=68),
         ("16bsr_small_kernelILi4ELi2ELb0ELb1EEEviiPKi",)),
    Case("bsrmm-bs4-n4-col-br-cc", "bsrmm",
         B(rowd=0, oc=1, bs=4, n=4),
         ("16bsr_small_kernelILi4ELi1ELb0ELb0EEEviiPKi",)),
    Case("bsrmm-bs4-n68-col-br-cc", "bsrmm",
         B(rowd=0, oc=1, bs=4, n=68),
         ("16bsr_small_kernelILi4ELi2ELb0ELb0EEEviiPKi",)),
    Case("bsrmm-bs8-n4-row-br-cc", "bsrmm",
         B(oc=1, bs=8, n=4),
         ("16bsr_small_kernelILi8ELi1ELb1ELb0EEEviiPKi",)),
    Case("bsrmm-bs8-n68-row-br-cc", "bsrmm",
         B(oc=1, bs=8, n=68),
         ("16bsr_small_kernelILi8ELi2ELb1ELb0EEEviiPKi",)),
    Case("bsrmm-bs8-n4-col-br-cr", "bsrmm",
         B(rowd=0, bs=8, n=4),
         ("16bsr_small_kernelILi8ELi1ELb0ELb1EEEviiPKi",)),
    Case("bsrmm-bs8-n68-col-br-cr", "bsrmm",
         B(rowd=0, bs=8, n=68),
         ("16bsr_small_kernelILi8ELi2ELb0ELb1EEEviiPKi",)),
    Case("bsrmm-bs8-n4-col-br-cc", "bsrmm",
         B(rowd=0, oc=1, bs=8, n=4),
         ("16bsr_small_kernelILi8ELi1ELb0ELb0EEEviiPKi",)),
    Case("bsrmm-bs8-n68-col-br-cc", "bsrmm",
         B(rowd=0, oc=1, bs=8, n=68),
         ("16bsr_small_kernelILi8ELi2ELb0ELb0EEEviiPKi",)),
    Case("bsrmm-bs16-n68-row-br-cr", "bsrmm",
         B(bs=16, n=68),
         ("15bsr16_cm_kernelIfLb1ELi128EEEviiPKi",)),
    Case("bsrmm-bs16-n132-row-br-cr", "bsrmm",
         B(bs=16, n=132),
         ("15bsr16_cm_kernelIfLb1ELi256EEEviiPKi",)),
    Case("bsrmm-bs16-n4-row-br-cc", "bsrmm",
         B(oc=1, bs=16, n=4),
         ("15bsr16_cm_kernelIfLb0ELi64EEEviiPKi",)),
    Case("bsrmm-bs16-n30-row-br-cc", "bsrmm",
         B(oc=1, bs=16, n=30),
         ("21bsr16_f32_mfma_kernelILb1ELb1ELb0EEEviiPKi",)),
    Case("bsrmm-bs16-n68-row-br-cc", "bsrmm",
         B(oc=1, bs=16, n=68),
         ("15bsr16_cm_kernelIfLb0ELi128EEEviiPKi",)),
    Case("bsrmm-bs16-n132-row-br-cc", "bsrmm",
         B(oc=1, bs=16, n=132),
         ("15bsr16_cm_kernelIfLb0ELi256EEEviiPKi",)),
    Case("bsrmm-bs16-n30-row-bc-cr", "bsrmm",
         B(ob=1, bs=16, n=30),
         ("21bsr16_f32_mfma_kernelILb1ELb0ELb1EEEviiPKi",)),
    Case("bsrmm-bs16-n30-row-bc-cc", "bsrmm",
         B(ob=1, oc=1, bs=16, n=30),
         ("21bsr16_f32_mfma_kernelILb1ELb0ELb0EEEviiPKi",)),
    Case("bsrmm-bs16-n4-col-br-cr", "bsrmm",
         B(rowd=0, bs=16, n=4),
         ("21bsr16_f32_mfma_kernelILb0ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs16-n4-col-br-cc", "bsrmm",
         B(rowd=0, oc=1, bs=16, n=4),
         ("21bsr16_f32_mfma_kernelILb0ELb1ELb0EEEviiPKi",)),
    Case("bsrmm-bs16-n4-col-bc-cr", "bsrmm",
         B(rowd=0, ob=1, bs=16, n=4),
         ("21bsr16_f32_mfma_kernelILb0ELb0ELb1EEEviiPKi",)),
    Case("bsrmm-bs16-n4-col-bc-cc", "bsrmm",
         B(rowd=0, ob=1, oc=1, bs=16, n=4),
         ("21bsr16_f32_mfma_kernelILb0ELb0ELb0EEEviiPKi",)),
    Case("bsrmm-bs32-n4-row-br-cc", "bsrmm",
         B(oc=1, bs=32, n=4),
         ("22block_row_order_kernelEiPKi",
          "20bsr32_f32_cs2_kernelILb0ELb1ELb1ELb0ELb0ELb1EEEviiPKi",)),
    Case("bsrmm-bs32-n30-row-br-cc", "bsrmm",
         B(oc=1, bs=32, n=30),
         ("21bsr32_f32_mfma_kernelILb1ELb1ELb0EEEviiPKi",)),
    Case("bsrmm-bs32-n68-row-br-cc", "bsrmm",
         B(oc=1, bs=32, n=68),
         ("22block_row_order_kernelEiPKi",
          "20bsr32_f32_cs2_kernelILb0ELb1ELb1ELb0ELb0ELb0EEEviiPKi",)),
    Case("bsrmm-bs32-n30-row-bc-cr", "bsrmm",
         B(ob=1, bs=32, n=30),
         ("21bsr32_f32_mfma_kernelILb1ELb0ELb1EEEviiPKi",)),
    Case("bsrmm-bs32-n30-row-bc-cc", "bsrmm",
         B(ob=1, oc=1, bs=32, n=30),
         ("21bsr32_f32_mfma_kernelILb1ELb0ELb0EEEviiPKi",)),
    Case("bsrmm-bs32-n4-col-br-cc", "bsrmm",
         B(rowd=0, oc=1, bs=32, n=4),
         ("21bsr32_f32_mfma_kernelILb0ELb1ELb0EEEviiPKi",)),
    Case("bsrmm-bs32-n4-col-bc-cr", "bsrmm",
         B(rowd=0, ob=1, bs=32, n=4),
         ("21bsr32_f32_mfma_kernelILb0ELb0ELb1EEEviiPKi",)),
    Case("bsrmm-bs32-n4-col-bc-cc", "bsrmm",
         B(rowd=0, ob=1, oc=1, bs=32, n=4),
         ("21bsr32_f32_mfma_kernelILb0ELb0ELb0EEEviiPKi",)),
    Case("bsrmm-bs64-n4-row-br-cr", "bsrmm",
         B(bs=64, n=4),
         ("22block_row_order_kernelEiPKi",
          "20bsr32_f32_cs2_kernelILb1ELb1ELb1ELb0ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs64-n68-row-br-cc", "bsrmm",
         B(oc=1, bs=64, n=68),
         ("22block_row_order_kernelEiPKi",
          "20bsr32_f32_cs2_kernelILb0ELb1ELb1ELb0ELb1ELb0EEEviiPKi",)),
    Case("bsrmm_f16-bs16-n4-row-br-cc", "bsrmm_f16",
         B(oc=1, bs=16, n=4),
         ("21bsr16_f16_mfma_kernelILb1ELb1ELb0EEEviiPKi",)),
    Case("bsrmm_f16-bs16-n64-row-br-cc", "bsrmm_f16",
         B(oc=1, bs=16, n=64),
         ("15bsr16_cm_kernelIDF16_Lb0ELi256EEEviiPKi",)),
    Case("bsrmm_f16-bs16-n128-row-br-cc", "bsrmm_f16",
         B(oc=1, bs=16, n=128),
         ("22block_row_order_kernelEiPKi",
          "19bsr16_f16_cs_kernelILb0ELb1ELb0EEEviiPKi",)),
    Case("bsrmm_f16-bs16-n4-row-bc-cr", "bsrmm_f16",
         B(ob=1, bs=16, n=4),
         ("21bsr16_f16_mfma_kernelILb1ELb0ELb1EEEviiPKi",)),
    Case("bsrmm_f16-bs16-n4-row-bc-cc", "bsrmm_f16",
         B(ob=1, oc=1, bs=16, n=4),
         ("21bsr16_f16_mfma_kernelILb1ELb0ELb0EEEviiPKi",)),
    Case("bsrmm_f16-bs16-n4-col-br-cr", "bsrmm_f16",
         B(rowd=0, bs=16, n=4),
         ("21bsr16_f16_mfma_kernelILb0ELb1ELb1EEEviiPKi",)),
    Case("bsrmm_f16-bs16-n4-col-br-cc", "bsrmm_f16",
         B(rowd=0, oc=1, bs=16, n=4),
         ("21bsr16_f16_mfma_kernelILb0ELb1ELb0EEEviiPKi",)),
    Case("bsrmm_f16-bs16-n4-col-bc-cr", "bsrmm_f16",
         B(rowd=0, ob=1, bs=16, n=4),
         ("21bsr16_f16_mfma_kernelILb0ELb0ELb1EEEviiPKi",)),
    Case("bsrmm_f16-bs16-n4-col-bc-cc", "bsrmm_f16",
         B(rowd=0, ob=1, oc=1, bs=16, n=4),
         ("21bsr16_f16_mfma_kernelILb0ELb0ELb0EEEviiPKi",)),
    Case("bsrmm_analysed-bs32-n4-col-br-cr", "bsrmm_analysed",
         B(rowd=0, bs=32, n=4),
         ("16seg_build_kernelEiPKiiiiiiP",
          "20bsr32_f32_cs2_kernelILb1ELb1ELb1ELb1ELb0ELb1EEEviiPKi",
          "16seg_fixup_kernelEiPK",
          "21bsr32_analysis_kernelEiiPKfPjPf",)),
    Case("bsrmm_analysed-bs32-n4-col-br-cc", "bsrmm_analysed",
         B(rowd=0, oc=1, bs=32, n=4),
         ("22block_row_order_kernelEiPKi",
          "20bsr32_f32_cs2_kernelILb0ELb1ELb1ELb1ELb0ELb1EEEviiPKi",
          "21bsr32_analysis_kernelEiiPKfPjPf",)),
    Case("bsrmm_analysed-bs32-n68-col-br-cc", "bsrmm_analysed",
         B(rowd=0, oc=1, bs=32, n=68),
         ("22block_row_order_kernelEiPKi",
          "20bsr32_f32_cs2_kernelILb0ELb1ELb1ELb1ELb0ELb0EEEviiPKi",
          "21bsr32_analysis_kernelEiiPKfPjPf",)),
    Case("bsrmm_analysed_f16-bs16-n128-col-br-cc", "bsrmm_analysed_f16",
         B(rowd=0, oc=1, bs=16, n=128),
         ("22block_row_order_kernelEiPKi",
          "19bsr16_f16_cs_kernelILb0ELb1ELb1EEEviiPKi",
          "21bsr16_analysis_kernelEiiPKtPjPt",)),
    Case("hybrid-bs32-n64-br-cr-flags5", "hybrid_csrmm",
         H(hybrid_flags=5, n=64),
         ("22block_row_order_kernelEiPKi",
          "20bsr32_f32_lds_kernelILb1ELb1ELb1EEEviiPKi",)),
    Case("hybrid-bs32-n64-br-cr-flags2", "hybrid_csrmm",
         H(hybrid_flags=2, n=64),
         ("20bsr32_f32_lds_kernelILb1ELb0ELb0EEEviiPKi",
          "16csr_group_kernelILb1ELi16ELi4ELb0EEEviiPKi",)),
    Case("hybrid-bs32-n64-br-cr-flags6", "hybrid_csrmm",
         H(hybrid_flags=6, n=64),
         ("20bsr32_f32_lds_kernelILb1ELb0ELb1EEEviiPKi",
          "16csr_group_kernelILb1ELi16ELi4ELb0EEEviiPKi",)),
    Case("csrmm-n4-flags1-boff0-coff0-padb0-padc0", "csrmm",
         Cs(n=4),
         ("16csr_group_kernelILb1ELi2ELi1ELb0EEEviiPKi",)),
    Case("csrmm-n4-flags0-boff0-coff0-padb0-padc0", "csrmm",
         Cs(csr_flags=0, n=4),
         ("16csr_group_kernelILb0ELi2ELi1ELb0EEEviiPKi",)),
    Case("csrmm-n4-flags2-boff0-coff0-padb0-padc0", "csrmm",
         Cs(csr_flags=2, n=4),
         ("5CsrMpIfE20csr_mergepath_kernelILi1ELb0ELi0EEEviiPKi",)),
    Case("csrmm-n16-flags1-boff0-coff0-padb0-padc0", "csrmm",
         Cs(n=16),
         ("16csr_group_kernelILb1ELi4ELi1ELb0EEEviiPKi",)),
    Case("csrmm-n16-flags0-boff0-coff0-padb0-padc0", "csrmm",
         Cs(csr_flags=0, n=16),
         ("16csr_group_kernelILb0ELi4ELi1ELb0EEEviiPKi",)),
    Case("csrmm-n32-flags1-boff0-coff0-padb0-padc0", "csrmm",
         Cs(n=32),
         ("16csr_group_kernelILb1ELi8ELi2ELb0EEEviiPKi",)),
    Case("csrmm-n32-flags0-boff0-coff0-padb0-padc0", "csrmm",
         Cs(csr_flags=0, n=32),
         ("16csr_group_kernelILb0ELi8ELi2ELb0EEEviiPKi",)),
    Case("csrmm-n48-flags0-boff0-coff0-padb0-padc0", "csrmm",
         Cs(csr_flags=0, n=48),
         ("16csr_group_kernelILb0ELi16ELi4ELb0EEEviiPKi",)),
    Case("csrmm-n68-flags1-boff0-coff0-padb0-padc0", "csrmm",
         Cs(n=68),
         ("5CsrMpIfE20csr_mergepath_kernelILi2ELb1ELi0EEEviiPKi",)),
    Case("csrmm-n68-flags0-boff0-coff0-padb0-padc0", "csrmm",
         Cs(csr_flags=0, n=68),
         ("5CsrMpIfE20csr_mergepath_kernelILi2ELb0ELi0EEEviiPKi",)),
    Case("csrmm-n132-flags0-boff0-coff0-padb0-padc0", "csrmm",
         Cs(csr_flags=0, n=132),
         ("5CsrMpIfE20csr_mergepath_kernelILi4ELb0ELi0EEEviiPKi",)),
    Case("csrmm_f16-n4-flags1-boff0-coff0-padb0-padc0", "csrmm_f16",
         Cs(n=4),
         ("5CsrMpIDF16_E20csr_mergepath_kernelILi1ELb1ELi0EEEviiPKi",)),
    Case("csrmm_f16-n4-flags0-boff0-coff0-padb0-padc0", "csrmm_f16",
         Cs(csr_flags=0, n=4),
         ("5CsrMpIDF16_E20csr_mergepath_kernelILi1ELb0ELi0EEEviiPKi",)),
    Case("csrmm_f16-n68-flags1-boff0-coff0-padb0-padc0", "csrmm_f16",
         Cs(n=68),
         ("5CsrMpIDF16_E20csr_mergepath_kernelILi2ELb1ELi0EEEviiPKi",)),
    Case("csrmm_f16-n68-flags0-boff0-coff0-padb0-padc0", "csrmm_f16",
         Cs(csr_flags=0, n=68),
         ("5CsrMpIDF16_E20csr_mergepath_kernelILi2ELb0ELi0EEEviiPKi",)),
    Case("csrmm_f16-n132-flags1-boff0-coff0-padb0-padc0", "csrmm_f16",
         Cs(n=132),
         ("5CsrMpIDF16_E20csr_mergepath_kernelILi4ELb1ELi0EEEviiPKi",)),
    Case("csrmm_f16-n132-flags0-boff0-coff0-padb0-padc0", "csrmm_f16",
         Cs(csr_flags=0, n=132),
         ("5CsrMpIDF16_E20csr_mergepath_kernelILi4ELb0ELi0EEEviiPKi",)),
    Case("csrmm_hot-n4-flags1-boff0-coff0-padb0-padc0", "csrmm_hot",
         Cs(n=4),
         ("16csr_group_kernelILb1ELi2ELi1ELb1EEEviiPKi",
          "16col_count_kernelExPKiiiPj",
          "17count_hist_kernelEiPKjPj",
          "17hot_select_kernelEPKjxPj",
          "14hot_tag_kernelExPKiiiPKj",)),
    Case("csrmm_hot-n4-flags2-boff0-coff0-padb0-padc0", "csrmm_hot",
         Cs(csr_flags=2, n=4),
         ("5CsrMpIfE20csr_mergepath_kernelILi1ELb1ELi2EEEviiPKi",
          "16col_count_kernelExPKiiiPj",
          "17count_hist_kernelEiPKjPj",
          "17hot_select_kernelEPKjxPj",
          "14hot_tag_kernelExPKiiiPKj",)),
    Case("csrmm_hot-n16-flags1-boff0-coff0-padb0-padc0", "csrmm_hot",
         Cs(n=16),
         ("16csr_group_kernelILb1ELi4ELi1ELb1EEEviiPKi",
          "16col_count_kernelExPKiiiPj",
          "17count_hist_kernelEiPKjPj",
          "17hot_select_kernelEPKjxPj",
          "14hot_tag_kernelExPKiiiPKj",)),
    Case("csrmm_hot-n32-flags1-boff0-coff0-padb0-padc0", "csrmm_hot",
         Cs(n=32),
         ("16csr_group_kernelILb1ELi8ELi2ELb1EEEviiPKi",
          "16col_count_kernelExPKiiiPj",
          "17count_hist_kernelEiPKjPj",
          "17hot_select_kernelEPKjxPj",
          "14hot_tag_kernelExPKiiiPKj",)),
    Case("csrmm_hot-n48-flags1-boff0-coff0-padb0-padc0", "csrmm_hot",
         Cs(n=48),
         ("16csr_group_kernelILb1ELi16ELi4ELb1EEEviiPKi",
          "16col_count_kernelExPKiiiPj",
          "17count_hist_kernelEiPKjPj",
          "17hot_select_kernelEPKjxPj",
          "14hot_tag_kernelExPKiiiPKj",)),
    Case("csrmm_hot-n132-flags1-boff0-coff0-padb0-padc0", "csrmm_hot",
         Cs(n=132),
         ("5CsrMpIfE20csr_mergepath_kernelILi4ELb1ELi2EEEviiPKi",
          "16col_count_kernelExPKiiiPj",
          "17count_hist_kernelEiPKjPj",
          "17hot_select_kernelEPKjxPj",
          "14hot_tag_kernelExPKiiiPKj",)),
    Case("bsrmm-bs8-n64-row-br-cr-shared-flags2", "bsrmm",
         B(shape='shared', bsr_flags=2, bs=8, n=64, small_path=1),
         ("22block_row_order_kernelEiPKi",
          "22small_grp_probe_kernelILi8EEEviiPKi",
          "20bsr_small_grp_kernelILi8ELb1ELb1EEEviiPKi",
          "16bsr_small_kernelILi8ELi1ELb1ELb1EEEviiPKi",),
         idle=("16bsr_small_kernelILi8ELi1ELb1ELb1EEEviiPKi",)),
    Case("bsrmm-bs2-n64-row-br-cc-shared-flags2", "bsrmm",
         B(oc=1, shape='shared', bsr_flags=2, bs=2, n=64, small_path=1),
         ("22block_row_order_kernelEiPKi",
          "22small_grp_probe_kernelILi2EEEviiPKi",
          "20bsr_small_grp_kernelILi2ELb1ELb0EEEviiPKi",
          "16bsr_small_kernelILi2ELi1ELb1ELb0EEEviiPKi",),
         idle=("16bsr_small_kernelILi2ELi1ELb1ELb0EEEviiPKi",)),
    Case("bsrmm-bs4-n64-row-br-cc-shared-flags2", "bsrmm",
         B(oc=1, shape='shared', bsr_flags=2, bs=4, n=64, small_path=1),
         ("22block_row_order_kernelEiPKi",
          "22small_grp_probe_kernelILi4EEEviiPKi",
          "20bsr_small_grp_kernelILi4ELb1ELb0EEEviiPKi",
          "16bsr_small_kernelILi4ELi1ELb1ELb0EEEviiPKi",),
         idle=("16bsr_small_kernelILi4ELi1ELb1ELb0EEEviiPKi",)),
    Case("bsrmm-bs8-n64-row-br-cc-shared-flags2", "bsrmm",
         B(oc=1, shape='shared', bsr_flags=2, bs=8, n=64, small_path=1),
         ("22block_row_order_kernelEiPKi",
          "22small_grp_probe_kernelILi8EEEviiPKi",
          "20bsr_small_grp_kernelILi8ELb1ELb0EEEviiPKi",
          "16bsr_small_kernelILi8ELi1ELb1ELb0EEEviiPKi",),
         idle=("16bsr_small_kernelILi8ELi1ELb1ELb0EEEviiPKi",)),
    Case("bsrmm-bs2-n64-col-br-cr-shared-flags2", "bsrmm",
         B(rowd=0, shape='shared', bsr_flags=2, bs=2, n=64, small_path=1),
         ("22block_row_order_kernelEiPKi",
          "22small_grp_probe_kernelILi2EEEviiPKi",
          "20bsr_small_grp_kernelILi2ELb0ELb1EEEviiPKi",
          "16bsr_small_kernelILi2ELi1ELb0ELb1EEEviiPKi",),
         idle=("16bsr_small_kernelILi2ELi1ELb0ELb1EEEviiPKi",)),
    Case("bsrmm-bs4-n64-col-br-cr-shared-flags2", "bsrmm",
         B(rowd=0, shape='shared', bsr_flags=2, bs=4, n=64, small_path=1),
         ("22block_row_order_kernelEiPKi",
          "22small_grp_probe_kernelILi4EEEviiPKi",
          "20bsr_small_grp_kernelILi4ELb0ELb1EEEviiPKi",
          "16bsr_small_kernelILi4ELi1ELb0ELb1EEEviiPKi",),
         idle=("16bsr_small_kernelILi4ELi1ELb0ELb1EEEviiPKi",)),
    Case("bsrmm-bs8-n64-col-br-cr-shared-flags2", "bsrmm",
         B(rowd=0, shape='shared', bsr_flags=2, bs=8, n=64, small_path=1),
         ("22block_row_order_kernelEiPKi",
          "22small_grp_probe_kernelILi8EEEviiPKi",
          "20bsr_small_grp_kernelILi8ELb0ELb1EEEviiPKi",
          "16bsr_small_kernelILi8ELi1ELb0ELb1EEEviiPKi",),
         idle=("16bsr_small_kernelILi8ELi1ELb0ELb1EEEviiPKi",)),
    Case("bsrmm-bs2-n64-col-br-cc-shared-flags2", "bsrmm",
         B(rowd=0, oc=1, shape='shared', bsr_flags=2, bs=2, n=64, small_path=1),
         ("22block_row_order_kernelEiPKi",
          "22small_grp_probe_kernelILi2EEEviiPKi",
          "20bsr_small_grp_kernelILi2ELb0ELb0EEEviiPKi",
          "16bsr_small_kernelILi2ELi1ELb0ELb0EEEviiPKi",),
         idle=("16bsr_small_kernelILi2ELi1ELb0ELb0EEEviiPKi",)),
    Case("bsrmm-bs4-n64-col-br-cc-shared-flags2", "bsrmm",
         B(rowd=0, oc=1, shape='shared', bsr_flags=2, bs=4, n=64, small_path=1),
         ("22block_row_order_kernelEiPKi",
          "22small_grp_probe_kernelILi4EEEviiPKi",
          "20bsr_small_grp_kernelILi4ELb0ELb0EEEviiPKi",
          "16bsr_small_kernelILi4ELi1ELb0ELb0EEEviiPKi",),
         idle=("16bsr_small_kernelILi4ELi1ELb0ELb0EEEviiPKi",)),
    Case("bsrmm-bs8-n64-col-br-cc-shared-flags2", "bsrmm",
         B(rowd=0, oc=1, shape='shared', bsr_flags=2, bs=8, n=64, small_path=1),
         ("22block_row_order_kernelEiPKi",
          "22small_grp_probe_kernelILi8EEEviiPKi",
          "20bsr_small_grp_kernelILi8ELb0ELb0EEEviiPKi",
          "16bsr_small_kernelILi8ELi1ELb0ELb0EEEviiPKi",),
         idle=("16bsr_small_kernelILi8ELi1ELb0ELb0EEEviiPKi",)),
]
# --- generated table end

CASES = TRACED_CASES + _other_cases()


def expected_keys(case: Case, keys) -> set:
    """The kernels of `keys` that the case's patterns name."""
    return {k for k in keys for p in case.expect if re.search(p, k)}


def covering_keys(case: Case, keys) -> set:
    """The kernels of `keys` that do the case's arithmetic: expected and not idle."""
    return expected_keys(case, keys) - {k for k in keys for p in case.idle if re.search(p, k)}
