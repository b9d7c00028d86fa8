"""tools/kernel_isa_diff.py on a kernel that gained or lost a *type* template argument its
parameter list depends on: the parameter list is then spelled differently too (`PKT_` for
`PKf`, later substitutions renumbered), and the map pairs the kernels by their template-id."""
from __future__ import annotations

import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WITH_T = "_ZN12_GLOBAL__N_118csrmm_heads_kernelIfLi4EEEviiiiPKiS2_PKfiPKT_xffPfx"
WITHOUT = "_ZN12_GLOBAL__N_118csrmm_heads_kernelILi4EEEviiiiPKiS2_PKfiS4_xffPfx"
OTHER = "_ZN12_GLOBAL__N_118csrmm_heads_kernelILi2EEEviiiiPKiS2_PKfiS4_xffPfx"


def _tool():
    spec = importlib.util.spec_from_file_location(
        "kernel_isa_diff", os.path.join(ROOT, "tools", "kernel_isa_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _asm(symbol: str, body: str) -> str:
    return (f"{symbol}:\n\t{body}\n\ts_endpgm\n.Lfunc_end0:\n"
            f"\t.amdhsa_kernel {symbol}\n\t\t.amdhsa_next_free_vgpr 8\n\t.end_amdhsa_kernel\n")


def test_a_dropped_type_argument_is_paired_by_template_id():
    t = _tool()
    new, old = _asm(WITH_T, "v_mov_b32 v0, 0"), _asm(WITHOUT, "v_mov_b32 v0, 0") + _asm(
        OTHER, "v_mov_b32 v0, 1")
    assert t.rename_map(new, old) == [(WITH_T, WITHOUT)]  # not the VEC = 2 kernel
    renamed = t.apply_renames(new, t.rename_map(new, old))
    kinds = {(kind, k) for kind, k, _ in t.compare(renamed, old)}
    assert kinds == {("only in B", OTHER)}
    # another body under the paired name is a finding
    changed = t.apply_renames(_asm(WITH_T, "v_mov_b32 v0, 2"), [(WITH_T, WITHOUT)])
    assert ("instructions", WITHOUT) in {(kind, k) for kind, k, _ in t.compare(changed, old)}


def test_no_pair_without_a_kernel_of_that_template_id():
    t = _tool()
    assert t.rename_map(_asm(WITH_T, "s_nop 0"), _asm(OTHER, "s_nop 0")) == []
