"""Regenerates the BSR / CSR / hybrid part of tests/kernel_cases.py (TRACED_CASES, between
the "generated table" markers) after a change of the launchers' kernel choice.

Candidates are the argument grid of drivers/dispatch_trace.cpp restated on the public
entries (plus the shapes that only some kernels need: wide ldb, the panel probe's 2^15
blocks, deep grids, a long block row, a B past 4 GB for the hot-column kernel). Each is
mapped to its launcher calls by kernel_cases.api_launches and handed to bin/dispatch_trace
("cases" mode), which answers with the kernels it launches. The shapes above are always
kept; the rest is a greedy set cover, simplest candidates first. A case is credited only
with the kernels that do its arithmetic: one that it queues but that returns at once on a
device-side gate (idle_of below) is written into the case's `idle` and needs another case. The expectations written
into the table are then checked by tests/test_kernel_cases.py like hand-written ones.

Usage: make -C spmm-denseblock_amd lib bin/dispatch_trace && python tools/gen_kernel_cases.py
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "spmm-denseblock_amd")]
import kernel_cases as kc  # noqa: E402
import kernel_keys as kk  # noqa: E402

EXE = os.path.join(ROOT, "spmm-denseblock_amd", "bin", "dispatch_trace")
TABLE = os.path.join(ROOT, "tests", "kernel_cases.py")
ships = [kk.launch_key(s) for s in kk.shipped_kernels()]
PFX = "_ZN12_GLOBAL__N_1"

cands = []  # (priority, Case without expect)
def add(prio, id_, entry, args):
    cands.append((prio, kc.Case(id_, entry, args, ())))

Ns = [4, 30, 64, 68, 128, 132, 256, 260]
def bid(e, a):
    s = (f"{e}-bs{a['bs']}-n{a['n']}-{'row' if a.get('rowd', 1) else 'col'}-b{'rc'[a['ob']]}"
         f"-c{'rc'[a['oc']]}")
    for k in ("voff", "boff", "coff", "pad_b", "pad_c"):
        if a[k]:
            s += f"-{k.replace('_','')}{a[k]}"
    if a["shape"] != "shallow":
        s += "-" + a["shape"]
    if a["bsr_flags"]:
        s += f"-flags{a['bsr_flags']}"
    return s

# specials first (forced)
for bs in (32, 64):
    for oc in (0, 1):
        for n in (64, 132):
            a = kc.B(bs=bs, n=n, oc=oc, shape="wide")
            add(0, bid("bsrmm", a), "bsrmm", a)
            if bs == 32:
                a = kc.B(bs=bs, n=n, oc=oc, shape="wide", rowd=0)
                add(0, bid("bsrmm_analysed", a), "bsrmm_analysed", a)
for bs in (32, 64):
    for oc in (0, 1):
        for n in (8, 68):
            a = kc.B(bs=bs, n=n, oc=oc, shape="panel")
            add(0, bid("bsrmm", a), "bsrmm", a)
for n in (8, 68):
    a = kc.B(bs=32, n=n, shape="deep-panel")
    add(0, bid("bsrmm", a), "bsrmm", a)
for n, boff in ((256, 0), (128, 0), (128, 1), (68,0), (67, 0)):
    add(1, f"csrmm_hot_wide-n{n}-boff{boff}", "csrmm_hot_wide", dict(n=n, boff=boff))
for bs, n, oc, fl in ((32, 8, 0, 0), (64, 4, 1, 0), (8, 4, 0, 2)):
    a = kc.B(bs=bs, n=n, oc=oc, shape="deep", bsr_flags=fl)
    if fl == 2:  # single blocks scattered over 25,000 block rows: the probe gives it up
        a["small_path"] = 2
    add(0, bid("bsrmm", a), "bsrmm", a)
# padded and offset layouts, one or two per family: the unaligned-val / B / C fallbacks at
# each bs, and the layouts that keep the fast path off the allocation's alignment
for e, bs, n in (("bsrmm", 32, 64), ("bsrmm", 64, 132), ("bsrmm", 16, 64), ("bsrmm", 8, 132),
                 ("bsrmm_f16", 16, 136), ("bsrmm_analysed", 32, 132)):
    rowd = 0 if "analysed" in e else 1
    f = 2 if e.endswith("f16") else 1  # fp16 B: 16 bytes are 8 halves
    for kw in (dict(boff=4 * f, pad_b=4 * f, coff=4, pad_c=4), dict(voff=1), dict(coff=1, pad_c=1),
               dict(boff=1, pad_b=1)):
        if "analysed" in e and "voff" in kw:
            continue
        a = kc.B(bs=bs, n=n, rowd=rowd, **kw)
        add(0, bid(e, a), e, a)
for lay in ((4, 4, 4, 4), (1, 1, 1, 3)):
    a = kc.H(bs=32, n=64, boff=lay[0], pad_b=lay[1], coff=lay[2], pad_c=lay[3])
    add(0, f"hybrid-bs32-n64-br-cr-lay{''.join(map(str, lay))}", "hybrid_csrmm", a)
for e, bs in (("bsrmm", 32), ("bsrmm_analysed", 32), ("bsrmm_f16", 16), ("bsrmm_analysed_f16", 16)):
    a = kc.B(bs=bs, n=132 if bs == 32 else 136, shape="long", rowd=0 if "analysed" in e else 1)
    add(0, bid(e, a), e, a)

# grid
for f16 in (0, 1):
    e = "bsrmm_f16" if f16 else "bsrmm"
    for bs in (2, 3, 4, 8, 16, 32, 64):
        for rowd in (1, 0):
            for ob in (0, 1):
                for oc in (0, 1):
                    for n in Ns:
                        if (bs == 3 or (f16 and bs not in (16, 8))) and n != 64:
                            continue
                        a = kc.B(bs=bs, n=n, rowd=rowd, ob=ob, oc=oc)
                        add(1, bid(e, a), e, a)
    for bs in ([16] if f16 else [8, 16, 32, 64]):
        for rowd in (1, 0):
            for oc in (0, 1):
                for n in (64, 256):
                    for k in ("voff", "boff", "coff"):
                        for off in (1, 2):
                            a = kc.B(bs=bs, n=n, rowd=rowd, oc=oc, **{k: off})
                            add(2, bid(e, a), e, a)
                    for k in ("pad_b", "pad_c"):
                        for p in (1, 4):
                            a = kc.B(bs=bs, n=n, rowd=rowd, oc=oc, **{k: p})
                            add(2, bid(e, a), e, a)
                    a = kc.B(bs=bs, n=n, rowd=rowd, oc=oc, bsr_flags=1)
                    add(2, bid(e, a), e, a)
                    if not f16 and bs == 8:
                        for bs2 in (2, 4, 8):
                            # shared block columns: the probe keeps the grouped stream
                            a = kc.B(bs=bs2, n=n, rowd=rowd, oc=oc, bsr_flags=2, shape="shared",
                                     small_path=1)
                            add(2, bid(e, a), e, a)
for e, bs in (("bsrmm_analysed", 32), ("bsrmm_analysed_f16", 16)):
    for ob in (0, 1):
        for oc in (0, 1):
            for n in Ns:
                a = kc.B(bs=bs, n=n, rowd=0, ob=ob, oc=oc)
                add(1, bid(e, a), e, a)
                for k in ("boff", "coff", "pad_b", "pad_c"):
                    a = kc.B(bs=bs, n=n, rowd=0, ob=ob, oc=oc, **{k: 1})
                    add(2, bid(e, a), e, a)
# hybrid
for bs in (32, 16, 64, 8):
    for flags in (0, 1 | 4, 2, 2 | 4):
        for ob, oc in ((0, 0), (1, 1), (0, 1)):
            for n in (64, 136):
                if bs != 32 and flags:
                    continue
                a = kc.H(bs=bs, n=n, ob=ob, oc=oc, hybrid_flags=flags)
                add(1, f"hybrid-bs{bs}-n{n}-b{'rc'[ob]}-c{'rc'[oc]}-flags{flags}",
                    "hybrid_csrmm", a)
# csr
for e in ("csrmm", "csrmm_f16", "csrmm_hot"):
    for n in (4, 8, 16, 32, 48, 64, 68, 128, 132, 256, 260):
        for flags in (1, 0, 2, 3):
            for al in range(5):
                for ld in range(3):
                    if al and ld and e != "csrmm":
                        continue
                    boff = (0, 1, 2, 0, 0)[al] * (2 if e == "csrmm_f16" else 1)
                    coff = (0, 0, 0, 1, 2)[al]
                    a = kc.Cs(n=n, csr_flags=flags, boff=boff, coff=coff, pad_b=ld,
                              pad_c=2 if ld == 2 else 0)
                    add(1 + (al > 0) + (ld > 0),
                        f"{e}-n{n}-flags{flags}-boff{boff}-coff{coff}-padb{ld}-padc{a['pad_c']}",
                        e, a)
    for ob, oc in ((1, 0), (0, 1), (1, 1)):
        a = kc.Cs(n=68, ob=ob, oc=oc)
        add(1, f"{e}-n68-b{'rc'[ob]}-c{'rc'[oc]}", e, a)

print(len(cands), "candidates")
# evaluate
lines, spans, auxs = [], [], []
for _, c in cands:
    ls, aux = kc.api_launches(c)
    spans.append((len(lines), len(ls)))
    lines += ls
    auxs.append(aux)
out = subprocess.run([EXE, "cases"], input="\n".join(lines) + "\n", capture_output=True,
                     text=True, check=True).stdout.split("\n")
keysets = []
for (s, n), aux in zip(spans, auxs):
    ks = []
    for l in out[s:s + n]:
        ks += [kk.launch_key(t) for t in l.split()]
    for p in aux:
        m = [k for k in ships if re.search(p, k)]
        assert len(m) == 1, (p, m)
        ks += m
    keysets.append(list(dict.fromkeys(ks)))



def idle_of(case, ks):
    """The kernels a case queues that return at once on a device-side gate (kernel_cases'
    module docstring): no cover is credited for them."""
    if any("panel_probe_kernel" in k for k in ks):
        return [k for k in ks if "bsr32_f32_cs2_kernel" in k]
    path = case.args.get("small_path")
    if path == 1:
        return [k for k in ks if "16bsr_small_kernelI" in k]
    if path == 2:
        return [k for k in ks if "bsr_small_grp_kernel" in k]
    return []


idles = [idle_of(c, ks) for (_, c), ks in zip(cands, keysets)]
credit = [set(ks) - set(idle) for ks, idle in zip(keysets, idles)]
covered, chosen = set(), []
order = sorted(range(len(cands)), key=lambda i: cands[i][0])
for i in order:
    if cands[i][0] == 0:
        chosen.append(i)
        covered |= credit[i]
while True:
    best, gain = None, 0
    for i in order:
        g = len(credit[i] - covered)
        # prefer lower priority number at equal gain (order is sorted, strict >)
        if g > gain: best, gain = i, g
    if best is None:
        break
    chosen.append(best)
    covered |= credit[best]

unreach = kk.unreachable_keys(ships)
traced_files = [kk.launch_key(s) for s in kk.shipped_kernels(("csr_kernels", "bsr_kernels"))]
missing = [k for k in traced_files if k not in covered and k not in unreach]
print(len(chosen), "chosen; uncovered of csr/bsr files:")
for k in missing:
    print("  ", k)

def fmt(d, defaults):
    return ", ".join(f"{k}={v!r}" for k, v in d.items() if defaults.get(k, object()) != v)
rows = []
for i in chosen:
    c = cands[i][1]
    ctor, dflt = {"hybrid_csrmm": ("H", kc.H()), "csrmm_hot_wide": ("dict", {})}.get(
        c.entry, ("Cs", kc.Cs()) if c.entry.startswith("csrmm") else ("B", kc.B()))
    pats = "".join(f'\n          "{k[len(PFX):]}",' for k in keysets[i])
    idle = "".join(f'\n               "{k[len(PFX):]}",' for k in idles[i])
    idle = f',\n         idle=({idle[16:]})' if idle else ""
    rows.append(f'    Case("{c.id}", "{c.entry}",\n         {ctor}({fmt(c.args, dflt)}),\n'
                f'         ({pats[11:]}){idle}),\n')
src = open(TABLE).read()
a = src.index("# --- generated table begin")
b = src.index("# --- generated table end")
src = src[:a] + "# --- generated table begin\nTRACED_CASES = [\n" + "".join(rows) + "]\n" + src[b:]
open(TABLE, "w").write(src)
