"""Kernel-by-kernel comparison of two gfx950 device assembly files (hipcc --save-temps).

A host-side refactor moves the order in which kernel templates are instantiated, so the
two files differ as text (function order, the function index in every local label) even
when every kernel is the same. This compares what matters, per kernel:

* the set of `.amdhsa_kernel` names;
* each kernel's descriptor block (`.amdhsa_*` lines: registers, LDS, scratch, ...);
* each kernel's instruction stream, comments stripped and local labels
  (`.LBB<f>_<n>` and the like) renumbered in order of first appearance.

It diffs whole streams and looks for no particular instruction.

Usage: python tools/kernel_isa_diff.py A.s B.s     (exit status 1 if anything differs)
"""
from __future__ import annotations

import re
import sys

_KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
_ENTRY = re.compile(r"^([^\s:]+):")
_LOCAL = re.compile(r"\.L([A-Za-z_]+)(\d+)_(\d+)")


def _strip(line: str) -> str:
    return line.split(";", 1)[0].strip()


def descriptors(text: str) -> dict[str, list[str]]:
    """kernel name -> the lines of its .amdhsa_kernel block."""
    out: dict[str, list[str]] = {}
    cur = None
    for line in text.splitlines():
        m = _KERNEL.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif line.strip() == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None and _strip(line):
            cur.append(_strip(line))
    return out


def streams(text: str, names) -> dict[str, list[str]]:
    """kernel name -> its instructions and labels, from `name:` to `.Lfunc_end`."""
    out: dict[str, list[str]] = {}
    cur = None
    labels: dict[str, str] = {}

    def renumber(m: re.Match) -> str:
        return labels.setdefault(m.group(0), f".L{m.group(1)}_{len(labels)}")

    for line in text.splitlines():
        if cur is None:
            m = _ENTRY.match(line)
            if m and m.group(1) in names and m.group(1) not in out:
                cur, labels = out.setdefault(m.group(1), []), {}
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        s = _strip(line)
        if s:
            cur.append(_LOCAL.sub(renumber, s))
    return out


def compare(a: str, b: str) -> list[tuple[str, str, str]]:
    """Findings as (kind, kernel, detail), kind one of "only in A", "only in B",
    "descriptor", "instructions"; empty when every kernel of a equals its namesake in b."""
    da, db = descriptors(a), descriptors(b)
    out = [("only in A", k, "") for k in sorted(da.keys() - db.keys())]
    out += [("only in B", k, "") for k in sorted(db.keys() - da.keys())]
    common = sorted(da.keys() & db.keys())
    sa, sb = streams(a, set(common)), streams(b, set(common))
    for k in common:
        if da[k] != db[k]:
            out.append(("descriptor", k, "; ".join(sorted(set(da[k]) ^ set(db[k])))))
        x, y = sa.get(k), sb.get(k)
        if x is None or y is None:
            out.append(("instructions", k, "no instruction stream found"))
        elif x != y:
            i = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
            out.append(("instructions", k, "line %d of the stream: %r / %r" %
                        (i, x[i] if i < len(x) else "<end>", y[i] if i < len(y) else "<end>")))
    return out


def main(argv: list[str]) -> int:
    if len(argv) != 3:
        print(__doc__)
        return 2
    with open(argv[1]) as f:
        a = f.read()
    with open(argv[2]) as f:
        b = f.read()
    findings = compare(a, b)
    for kind, kernel, detail in findings:
        print(f"{kind}: {kernel}: {detail}" if detail else f"{kind}: {kernel}")
    names = "differ" if any(k.startswith("only") for k, _, _ in findings) else "identical"
    differing = len({kernel for kind, kernel, _ in findings if not kind.startswith("only")})
    print(f"{len(descriptors(a))} kernels in A, {len(descriptors(b))} in B: name sets {names}, "
          f"{differing} differing kernels")
    return 1 if findings else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
