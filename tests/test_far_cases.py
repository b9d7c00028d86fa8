"""The far-operand geometries (tests/far_cases.py) on the host: every crossing a geometry
claims is one, every used element lies inside the arena, every leading dimension keeps its
kernel family's fast path, and the restated launcher predicates put the *_in and *_out
geometries on opposite sides of their switch, with the launchers themselves
(bin/dispatch_trace, "cases" mode) agreeing on O32 and on the small grouped stream. A later
change of a launcher bound fails here and does not quietly move a GPU case off its edge.
"""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest

import far_cases as fc
from kernel_keys import PKG, launch_key

EXE = os.path.join(PKG, "bin", "dispatch_trace")
P31, P32 = 1 << 31, 1 << 32


@pytest.mark.parametrize("g", fc.GEOMETRIES, ids=lambda g: g.name)
def test_claimed_crossings_cross(g):
    assert g.crossings, g.name
    for row, unit, bound in g.crossings:
        assert 0 < row < g.rows, (g.name, row)
        assert g.start(row - 1, unit) < bound <= g.start(row, unit), (g.name, row, unit, bound)
        # the row is read or written to its last column from past the bound
        assert g.start(row, unit) + (fc.N_MAX if unit == "E" else fc.N_MAX * g.elem) > bound


def test_the_table_of_the_module():
    """The numbers of the module's docstring, literally."""
    t = {g.name: (g.elem, g.ld, g.rows) for g in fc.GEOMETRIES}
    assert t["f32"] == (4, 1 << 28, 9) and t["h16"] == (2, 1 << 28, 9)
    assert t["f64"] == (8, 1 << 27, 9)
    assert t["bs32_narrow"] == (4, (1 << 24) - 4, 160) and t["bs32_wide"] == (4, 1 << 25, 96)
    assert t["bs16_f"] == (4, 1 << 26, 48) and t["bs16_h"] == (2, 1 << 27, 32)
    assert t["hot_in"] == (4, 1 << 20, 1023) and t["hot_out"] == (4, 1 << 20, 1024)
    for bs in fc.SMALL_BS:
        kb = -(-10 // bs) + 1
        assert t[f"small_in{bs}"] == (4, (1 << 29) // bs - 2, bs * kb)
        assert t[f"small_out{bs}"] == (4, (1 << 29) // bs, bs * kb)
    assert fc.ARENA_BYTES == 3 * P32 + (1 << 26)
    # byte and element crossings of the plain geometries
    assert fc.F32.start(2) == P31 and fc.F32.start(4) == P32 and fc.F32.start(8, "E") == P31
    assert fc.H16.start(4) == P31 and fc.H16.start(8) == P32 and fc.H16.start(8, "E") == P31
    assert fc.F64.start(2) == P31 and fc.F64.start(4) == P32
    assert fc.F64.start(fc.F64.rows - 1, "E") < P31  # 2^31 elements: out of the arena's reach
    assert fc.BS16_H.start(8) == P31 and fc.BS16_H.start(16) == P32
    assert fc.BS16_H.start(16, "E") == P31
    assert fc.BS32_WIDE.start(64, "E") == P31 and fc.BS32_WIDE.rows == 3 * 32
    assert fc.BS32_NARROW.rows == 5 * 32
    # bs32_narrow: a panel's offsets (31 rows below its first, 4 n bytes across) stay under
    # 2^31; row 128 itself starts 512 elements short of 2^31, row 129 is past it
    assert 31 * fc.BS32_NARROW.ld * 4 + 4 * fc.N_MAX < P31 <= 32 * fc.BS32_NARROW.ld * 4 + 512
    assert fc.BS32_NARROW.start(128, "E") == P31 - 512


@pytest.mark.parametrize("g", fc.GEOMETRIES, ids=lambda g: g.name)
def test_inside_the_arena(g):
    # (+ 1 element: the fp16 case that starts an odd half into the arena)
    assert g.last_byte(fc.N_MAX, off=1) <= fc.ARENA_BYTES
    assert fc.FAR_BASE // g.elem >= fc.GUARD, "the guard in front of row 0 would leave it"
    assert g.ld >= fc.N_MAX + 2 * fc.GUARD, "the guards of neighbouring rows would meet"


@pytest.mark.parametrize("g", fc.GEOMETRIES, ids=lambda g: g.name)
def test_alignment_of_the_fast_paths(g):
    """ld % 4 for the bs 32 / 64 and bs 16 fp32 copy kernels and VEC 4, ld % 8 for the fp16
    ones (16-byte row pieces), ld % 2 and an 8-byte base for the small grouped stream; the
    operand's base keeps the arena's alignment to 256 bytes."""
    assert g.ld % g.ld_mod == 0 and fc.FAR_BASE % g.base_mod == 0
    want = {"f32": 4, "h16": 8, "bs32_narrow": 4, "bs32_wide": 4, "bs16_f": 4, "bs16_h": 8,
            "hot_in": 4, "hot_out": 4}.get(g.name, 2 if g.name.startswith("small") else 1)
    assert g.ld_mod == want
    if g.name.startswith("small"):
        assert g.base_mod == 8 and g.bs in fc.SMALL_BS


def test_power_of_two_leading_dimensions():
    """A 32-bit wrap lands on a row the case holds: ld is a power of two, but for the two
    geometries that are the last value on the inner side of a bound."""
    for g in fc.GEOMETRIES:
        pow2 = g.ld & (g.ld - 1) == 0
        assert pow2 != (g.name == "bs32_narrow" or g.name.startswith("small_in")), g.name


def test_sides_of_the_switches():
    assert fc.side(fc.BS32_NARROW) == {"o32": True} and fc.side(fc.BS32_WIDE) == {"o32": False}
    assert not fc.panels_in_31_bits(fc.BS32_NARROW.ld + 4)  # + step (ld % 4): already out
    assert fc.panels_in_31_bits((1 << 24) - 1) and not fc.panels_in_31_bits(1 << 24)
    for bs in fc.SMALL_BS:
        gi, go = fc.small_in(bs), fc.small_out(bs)
        assert fc.side(gi) == {"small": 1} and fc.side(go) == {"small": 0}
        assert go.ld == gi.ld + 2  # + step (ld % 2)
        assert gi.ld * bs * 4 == P31 - 8 * bs and go.ld * bs * 4 == P31
    for base in (0, 1):
        for n in fc.HOT_N:
            assert fc.side(fc.HOT_IN, n, base) == {"hot": 2}
            assert fc.side(fc.HOT_OUT, n, base) == {"hot": 1}
            k = fc.hot_k(fc.HOT_IN, base)
            assert k + base == 1023 and fc.hot_k(fc.HOT_OUT, base) + base == 1024
            assert fc.hot_mode(k + 1, base, fc.HOT_LD, n) == 1  # + step (one row): already out
            # the rows a case uses: below and from 2^31 bytes on, the last two of B
            rows = fc.hot_rows(k)
            assert rows[1] * fc.HOT_LD * 4 < P31 <= rows[2] * fc.HOT_LD * 4
            assert rows[-1] == k - 1 and rows[-2] == k - 2 and len(set(rows)) == 5
    assert fc.hot_mode(5, 0, 8, 8, hot=False) == 0


def test_hot_matrix_tags_one_of_the_last_two_rows():
    """Distinct use counts: a budget of two hot rows takes k - 1 and 512 and leaves k - 2,
    so the rows from 2^31 bytes on are gathered tagged and untagged."""
    k = fc.hot_k(fc.HOT_IN, 0)
    rp, ci, v = fc.hot_csr(np.random.default_rng(3), k)
    assert rp.size == 71 and rp[1] == 0 and rp[-1] == rp[-2] == ci.size
    assert (np.diff(rp) > 128).any()
    cols, cnt = np.unique(ci, return_counts=True)
    assert tuple(cols) == fc.hot_rows(k) and tuple(cnt) == fc.HOT_COUNTS
    top2 = set(cols[np.argsort(cnt)[-2:]])
    assert top2 == {512, k - 1} and cnt[cols == k - 2][0] == 1


def test_matrices_use_every_far_row():
    rng = np.random.default_rng(5)
    rp, ci, v = fc.far_csr(rng, 70, 9)
    assert rp[1] == 0 and rp[-1] == rp[-2] and np.diff(rp).max() > 128
    cnt = np.bincount(ci, minlength=9)
    assert cnt.min() >= 3, "a crossing row or the last row is referenced less than three times"
    for bs, kb in ((32, 5), (32, 3), (64, 2), (16, 2), (16, 3), (2, 6), (4, 4), (8, 3), (3, 3),
                   (5, 2)):
        rp, ci, v = fc.far_bsr(rng, 6, kb, bs)
        assert rp[2] == rp[1] and (np.diff(rp) == kb).any()
        assert np.bincount(ci, minlength=kb).min() >= 2 and v.size == ci.size * bs * bs


def test_far_csr_of_a_far_c_fills_its_last_row():
    """m = 9 (the rows of a far C): row 8, the only one at 2^31 elements, holds entries."""
    rp, ci, v = fc.far_csr(np.random.default_rng(6), 9, 20, long_row=4, last_empty=False)
    assert rp[1] == 0 and rp[-1] - rp[-2] == 12 and np.diff(rp).max() > 128


def test_rows_of_the_far_outputs():
    """What the row counts of the far row-major outputs cross on c_geometry: 9 to 12 rows
    (CSR, generic BSR), 48 (bs 16) and 96 (bs 32, bs 2 / 4 / 8) all three bounds, the single
    64-row block of bs 64 the two byte bounds only."""
    for rows in (9, 10, 12, 48, 96):
        assert fc.c_crossed(rows) == (True, True, True), rows
    assert fc.c_crossed(64) == (True, True, False)
    assert fc.c_geometry(13) is fc.F32 and fc.c_geometry(14) is fc.BS16_F
    assert fc.c_geometry(49) is fc.BS16_F and fc.c_geometry(50) is fc.BS32_WIDE
    assert fc.c_geometry(96) is fc.BS32_WIDE
    with pytest.raises(AssertionError):
        fc.c_geometry(128)  # two 64-row blocks: bs 64 keeps to one
    for bs in fc.SMALL_BS:
        assert 3 * (32 // bs) * bs == 96  # small_mat's three groups of the GPU module


def _trace(lines):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", PKG, "-j3", "bin/dispatch_trace"], check=True,
                       capture_output=True)
    out = subprocess.run([EXE, "cases"], input="\n".join(lines) + "\n", check=True,
                         capture_output=True, text=True).stdout.split("\n")
    return [[launch_key(t) for t in ln.split()] for ln in out[:len(lines)]]


def test_launchers_agree_with_the_restated_predicates():
    """The launchers' own answer for the geometries' leading dimensions: O32 of every column
    stream (drop-in, analysed, SUB), and whether the small grouped stream goes out under
    SPMM_BSR_SMALL_GROUPED."""
    lines, want = [], []
    for g in (fc.BS32_NARROW, fc.BS32_WIDE):
        o32 = fc.side(g)["o32"]
        for crow in (1, 0):
            for n in (64, 132):
                lines.append(f"bsr 0 32 {n} 1 1 {crow} 0 0 0 {g.ld} {n if crow else 192} 6 "
                             f"{g.rows // 32} 12 0 0 0 0")
                lines.append(f"bsr 0 32 {n} 0 1 {crow} 0 0 0 {g.ld} {n if crow else 192} 6 "
                             f"{g.rows // 32} 12 1 0 0 0")
                lines.append(f"bsr 0 64 {n} 1 1 {crow} 0 0 0 {g.ld} {n if crow else 192} 3 "
                             f"{g.rows // 64} 4 0 0 0 0")
                want += [("o32", o32)] * 3
    for bs in fc.SMALL_BS:
        for g in (fc.small_in(bs), fc.small_out(bs)):
            lines.append(f"bsr 0 {bs} 64 1 1 1 0 0 0 {g.ld} 64 6 {fc.small_kb(bs)} 12 0 0 2 0")
            want.append(("small", fc.side(g)["small"]))
    for keys, (what, side) in zip(_trace(lines), want):
        if what == "o32":
            cs2 = [k for k in keys if "bsr32_f32_cs2_kernel" in k]
            assert len(cs2) == 1, keys
            got = re.search(r"cs2_kernelILb[01]ELb([01])E", cs2[0]).group(1) == "1"
            assert got == side, (cs2[0], side)
        else:
            assert int(any("bsr_small_grp_kernel" in k for k in keys)) == side, keys
            assert any("bsr_small_kernel" in k for k in keys), keys
