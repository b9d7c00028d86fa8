"""tools/kernel_isa_diff.py on synthetic excerpts: a refactor of the host dispatch moves
kernels around in the device assembly without changing any; the tool must see through
the first and flag the second."""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_isa_diff as kid  # noqa: E402


def _kernel(name: str, f: int, add: str = "v_add_u32_e32 v1, 1, v1", vgpr: int = 8) -> str:
    return f"""\
\t.globl\t{name}
\t.type\t{name},@function
{name}:                                 ; @{name}
; %bb.0:
\ts_load_dword s0, s[4:5], 0x0
\ts_waitcnt lgkmcnt(0)
.LBB{f}_1:                                ; =>This Inner Loop Header: Depth=1
\t{add}
\ts_add_i32 s0, s0, -1                     ; a comment of function {f}
\ts_cbranch_scc1 .LBB{f}_1
; %bb.2:
\ts_endpgm
.Lfunc_end{f}:
\t.size\t{name}, .Lfunc_end{f}-{name}
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 6
\t.end_amdhsa_kernel
\t.text
"""


A = _kernel("_Z1aILb1EEvPf", 0) + _kernel("_Z1aILb0EEvPf", 1, "v_add_u32_e32 v1, 2, v1")


def test_reordered_functions_compare_equal():
    b = _kernel("_Z1aILb0EEvPf", 0, "v_add_u32_e32 v1, 2, v1") + _kernel("_Z1aILb1EEvPf", 1)
    assert A != b
    assert kid.compare(A, b) == []


def test_a_changed_instruction_is_flagged():
    b = _kernel("_Z1aILb1EEvPf", 0, "v_add_u32_e32 v1, 3, v1") + \
        _kernel("_Z1aILb0EEvPf", 1, "v_add_u32_e32 v1, 2, v1")
    got = kid.compare(A, b)
    assert [(k, n) for k, n, _ in got] == [("instructions", "_Z1aILb1EEvPf")], got
    assert "v_add_u32_e32 v1, 3, v1" in got[0][2]


def test_a_changed_descriptor_field_is_flagged():
    b = _kernel("_Z1aILb1EEvPf", 0) + _kernel("_Z1aILb0EEvPf", 1, "v_add_u32_e32 v1, 2, v1", vgpr=9)
    got = kid.compare(A, b)
    assert [(k, n) for k, n, _ in got] == [("descriptor", "_Z1aILb0EEvPf")], got
    assert ".amdhsa_next_free_vgpr 9" in got[0][2]


def test_a_missing_kernel_is_flagged():
    got = kid.compare(A, _kernel("_Z1aILb1EEvPf", 0))
    assert got == [("only in A", "_Z1aILb0EEvPf", "")]


_OLD = "_ZN12_GLOBAL__N_115bsr16_cm_kernelIfLb1ELi2ELi5ELi1ELi64EEEviiPKiS2_PKT_S5_iffPfi"
_NEW = "_ZN12_GLOBAL__N_115bsr16_cm_kernelIfLb1ELi64EEEviiPKiS2_PKT_S5_iffPfi"


def test_a_dropped_template_parameter_renames_the_symbol():
    assert kid.renamed(_OLD) == _NEW
    assert kid.renamed("_ZN12_GLOBAL__N_120bsr32_f32_cs2_kernelILb1ELi32ELi6ELi3ELb0ELb1ELb1ELb0ELb1ELb0EEEviiPKi") \
        == "_ZN12_GLOBAL__N_120bsr32_f32_cs2_kernelILb1ELb0ELb1ELb0ELb1ELb0EEEviiPKi"
    assert kid.renamed("_Z1aILb1EEvPf") == "_Z1aILb1EEvPf"


def test_renamed_kernels_compare_through_the_map():
    """A body that refers to the kernel's own symbol follows the rename; without the map
    the two files share no kernel."""
    ref = "s_getpc_b64 s[0:1]\n\ts_add_u32 s0, s0, {0}@rel32@lo+4"
    a, b = _kernel(_OLD, 0, ref.format(_OLD)), _kernel(_NEW, 0, ref.format(_NEW))
    pairs = kid.rename_map(a, b)
    assert pairs == [(_OLD, _NEW)]
    assert kid.compare(kid.apply_renames(a, pairs), b) == []
    assert {k for k, _, _ in kid.compare(a, b)} == {"only in A", "only in B"}
    changed = _kernel(_NEW, 0, ref.format(_NEW), vgpr=9)
    got = kid.compare(kid.apply_renames(a, pairs), changed)
    assert [(k, n) for k, n, _ in got] == [("descriptor", _NEW)], got


def test_a_kernel_gone_from_the_new_file_gets_no_pair():
    assert kid.rename_map(_kernel(_OLD, 0), _kernel("_Z1aILb1EEvPf", 0)) == []
