"""Kernel-by-kernel comparison of two gfx950 device assembly files (hipcc --save-temps).

A host-side refactor moves the order in which kernel templates are instantiated, so the
two files differ as text (function order, the function index in every local label) even
when every kernel is the same. This compares what matters, per kernel:

* the set of `.amdhsa_kernel` names;
* each kernel's descriptor block (`.amdhsa_*` lines: registers, LDS, scratch, ...);
* each kernel's instruction stream, comments stripped and local labels
  (`.LBB<f>_<n>` and the like) renumbered in order of first appearance.

It diffs whole streams and looks for no particular instruction.

A change that takes template parameters away renames kernels without touching them. A
rename map, a text file of `old-symbol new-symbol` lines, is applied to the whole text of A
first, so kernels are compared with their renamed selves and references inside bodies
follow. The map is generated, not written: from the `.amdhsa_kernel` lists of the old and
the new assembly and DROPPED below, which template-argument positions each kernel lost.

Usage: python tools/kernel_isa_diff.py A.s B.s [rename_map.txt]
           (exit status 1 if anything differs)
       python tools/kernel_isa_diff.py --rename-map OLD.s NEW.s [OLD2.s NEW2.s ...]
           (prints the map of every pair of files, release and TUNING say, as one)
"""
from __future__ import annotations

import re
import sys

_KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
_ENTRY = re.compile(r"^([^\s:]+):")
_LOCAL = re.compile(r"\.L([A-Za-z_]+)(\d+)_(\d+)")

# kernel -> the 0-based positions of the template arguments it lost (each was the same
# value at every launch site and is a constant of the kernel body now)
DROPPED = {
    "bsr32_f32_mfma_kernel": (3,),           # VAR
    "bsr16_f32_mfma_kernel": (3,),           # VAR
    "bsr16_f16_mfma_kernel": (3,),           # VAR
    "bsr32_f32_lds_kernel": (1, 2, 4, 6),    # D, XM, HB, PAIR
    "bsr32_f32_cs2_kernel": (1, 2, 3, 5),    # XM, P, NA, PK
    "bsr32_f32_panel_kernel": (2,),          # D
    "bsr16_cm_kernel": (2, 3, 4),            # D, DA, WPE
    "bsr16_f16_cs_kernel": (1, 2, 3, 4, 6, 7),  # P, NA, DA, CAP, CST, COLS
    # These two gained a parameter (the storage type T, `float` in heads_kernels.hip): give
    # the new assembly as OLD / A and the old one as NEW / B, so that the map takes T away.
    # Their pointer parameters depend on T, so the parameter list is spelled differently too
    # (PKT_ for PKf) and the other name is found by its template-id (rename_map).
    "sddmm_heads_kernel": (0,),              # T
    "csrmm_heads_kernel": (0,),              # T
}
# a kernel's own name and its template arguments inside a mangled symbol: literals
# (Lb1E, Li32E) and builtin types (f, DF16_), none of which is a substitution candidate,
# so the rest of the symbol is unchanged when some go
_TEMPLATE_ID = re.compile("(%s)I((?:L[a-z]n?\\d+E|DF16_|[a-z])+)E" %
                          "|".join(f"{len(k)}{k}" for k in DROPPED))
_TEMPLATE_ARG = re.compile(r"L[a-z]n?\d+E|DF16_|[a-z]")


def kernel_names(text: str) -> list[str]:
    return re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)


def renamed(symbol: str) -> str:
    """`symbol` without the template arguments DROPPED lists for its kernel."""
    def drop(m: re.Match) -> str:
        gone = DROPPED[m.group(1).lstrip("0123456789")]
        args = _TEMPLATE_ARG.findall(m.group(2))
        return "%sI%sE" % (m.group(1), "".join(a for i, a in enumerate(args) if i not in gone))
    return _TEMPLATE_ID.sub(drop, symbol, count=1)


def rename_map(old: str, new: str) -> list[tuple[str, str]]:
    """(old symbol, new symbol) for every kernel of `old` that DROPPED renames. Each new
    symbol must be a kernel of `new` and no two old ones may share it; a kernel that is
    gone from `new` altogether (its old name and its new one) gets no pair."""
    have = set(kernel_names(new))

    def template_id(symbol: str) -> str | None:  # the symbol up to the end of its arguments
        m = _TEMPLATE_ID.search(symbol)
        return symbol[:m.end()] if m else None

    def found(r: str) -> str | None:
        """r itself, or the one kernel of `new` with r's template-id when a parameter
        that went was a type the parameter list depends on."""
        if r in have:
            return r
        tid = template_id(r)
        same = [n for n in have if tid is not None and template_id(n) == tid]
        return same[0] if len(same) == 1 else None

    pairs = [(k, found(renamed(k))) for k in kernel_names(old) if renamed(k) != k]
    pairs = [(k, r) for k, r in pairs if r is not None]
    assert len({r for _, r in pairs}) == len(pairs), "two kernels renamed to one symbol"
    return sorted(pairs)


def apply_renames(text: str, pairs) -> str:
    """Every old symbol of `pairs` replaced by its new one, longest first."""
    for old, new in sorted(pairs, key=lambda p: -len(p[0])):
        text = text.replace(old, new)
    return text


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


def _read(path: str) -> str:
    with open(path) as f:
        return f.read()


def main(argv: list[str]) -> int:
    if len(argv) >= 4 and argv[1] == "--rename-map" and len(argv) % 2 == 0:
        pairs = set()
        for old, new in zip(argv[2::2], argv[3::2]):
            pairs |= set(rename_map(_read(old), _read(new)))
        for old, new in sorted(pairs):
            print(old, new)
        return 0
    if len(argv) not in (3, 4) or argv[1].startswith("--"):
        print(__doc__)
        return 2
    a, b = _read(argv[1]), _read(argv[2])
    if len(argv) == 4:
        a = apply_renames(a, [ln.split() for ln in _read(argv[3]).splitlines() if ln.strip()])
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
