"""The matrices and layouts of tests/test_gpu_hybrid_ex.py and
tests/test_gpu_handle_reuse.py (built in tests/helpers.py) on the host: each reaches the
branch its GPU test names, so a later edit of a builder or a threshold cannot turn a
test into one that passes without running what it was written for."""
from __future__ import annotations

import numpy as np
import pytest

from helpers import (CSR_PIECE_MIN, HYBRID_EX_DENSITY, HYBRID_EX_LAYOUTS, HYBRID_EX_M, HYBRID_EX_N,
                     HYBRID_EX_ORDERS, PANEL_MIN_BLOCKS, PROBE64_CHECKED_BLOCK_ROWS, PROBE64_MB,
                     REUSE_HUB_K, REUSE_HUB_M, REUSE_HUB_NNZ, REUSE_SEG_SHAPE, cs2_segments_splits,
                     framed_operands, hybrid_ex_matrix, hybrid_ex_parts, hybrid_ex_staged_b_bytes,
                     long_row_column_sparse_bsr, panel_probe_bsr64, probe64_block_row_reference,
                     rand_bsr, rand_csr_rows, reuse_hub_csr, small_grouped_scratch_bytes)

torch = pytest.importorskip("torch")


def test_block_size_set_and_forms():
    assert sorted(HYBRID_EX_DENSITY) == [2, 4, 5, 8, 16, 32, 64]
    assert HYBRID_EX_ORDERS == [(1, 1), (0, 1), (1, 0)]  # every form with a column-major operand
    assert HYBRID_EX_N == [64, 136, 7]
    # 700 is a multiple of the block size at 2, 4 and 5 only: the rest pad B and C
    assert [bs for bs in HYBRID_EX_DENSITY if HYBRID_EX_M % bs == 0] == [2, 4, 5]


@pytest.mark.parametrize("bs", sorted(HYBRID_EX_DENSITY))
def test_divide_keeps_both_parts(bs):
    """At its density every block size keeps a BSR part and a CSR remainder; the two add
    up to the whole matrix; the matrix, the BSR part (block column 0) and the remainder
    all have entries in columns 0..3, the B rows a stray write into the head of a staged
    B would damage."""
    rp, ci, v = hybrid_ex_matrix()
    crp, cci, cv, brp, bci, bv = hybrid_ex_parts(bs)
    assert cci.size > 0 and bci.size > 0
    assert cci.size + np.count_nonzero(bv) == ci.size
    assert brp.size == -(-HYBRID_EX_M // bs) + 1 and bv.size == bci.size * bs * bs
    assert np.isin(ci, [0, 1, 2, 3]).any()
    assert (bci == 0).any() and np.isin(cci, [0, 1, 2, 3]).any()
    assert np.abs(v).max() < 1.0 and np.unique(v).size > ci.size // 2  # values other than 1


@pytest.mark.parametrize("n", [64, 136])
@pytest.mark.parametrize("bs", [2, 4, 8])
def test_grouped_branch_preconditions(bs, n):
    """The bs 2 / 4 / 8 grouped branch (launch_bsrmm_f32) needs n % 4 == 0 and an even
    ldb; the staged B's ldb is n. Its scratch request (probe sums, dirty flags from byte
    256) is smaller than the staged B, so a staged B kept in scratch was overwritten, not
    reallocated."""
    assert n % 4 == 0 and n % 2 == 0
    assert hybrid_ex_staged_b_bytes(HYBRID_EX_M, bs, n) >= small_grouped_scratch_bytes(HYBRID_EX_M, bs, n)
    mb = -(-HYBRID_EX_M // bs)
    assert small_grouped_scratch_bytes(HYBRID_EX_M, bs, n) == -(-mb // (32 // bs)) * -(-n // 128) * 4 + 256
    assert hybrid_ex_staged_b_bytes(HYBRID_EX_M, bs, n) == -(-HYBRID_EX_M // bs) * bs * n * 4


def test_layouts_reach_their_alignment_classes():
    tight, friendly, odd = HYBRID_EX_LAYOUTS
    assert tight == (0, 0, 0, 0)
    assert all(x % 4 == 0 for x in friendly) and any(friendly)
    assert odd[0] % 4 and odd[2] % 4 and odd[1] in (1, 3) and odd[3] in (1, 3)
    # a column-major operand is framed by columns, ld = its row count + pad
    Bd = np.arange(12, dtype=np.float32).reshape(4, 3)
    Cd = np.arange(15, dtype=np.float32).reshape(5, 3)
    dB, chkB, ldb, dC, ldc, extract = framed_operands(Bd, Cd, odd, 1, 1, device="cpu")
    assert (ldb, ldc) == (4 + odd[1], 5 + odd[3])
    assert (chkB.rows, chkB.cols) == (3, 4)
    assert np.array_equal(dB.numpy()[:ldb * 3].reshape(3, ldb)[:, :4], Bd.T)
    assert np.array_equal(extract("fresh"), Cd)
    dB, chkB, ldb, dC, ldc, extract = framed_operands(Bd, Cd, friendly, 0, 1, device="cpu")
    assert (ldb, ldc) == (3 + friendly[1], 5 + friendly[3]) and (chkB.rows, chkB.cols) == (4, 3)


def test_panel_probe_matrix():
    """bs 64 launches the probe from 4 * nnzb = kPanelMinBlocks sub-blocks: this matrix
    sits exactly there, with block column 0 (B rows 0..63) in every block row, dense
    blocks, and a remainder that reads B rows 0..3 too."""
    mats = panel_probe_bsr64()
    brp, bci, bval, crp, cci, cv = mats
    mb = PROBE64_MB
    assert 4 * bci.size == PANEL_MIN_BLOCKS == 2 ** 15
    assert brp.size == mb + 1 and brp[-1] == bci.size and bval.size == bci.size * 4096
    for br in range(mb):
        row = bci[brp[br]:brp[br + 1]]
        assert row[0] == 0 and (np.diff(row) > 0).all() and row[-1] < mb
    assert bval.dtype == np.float32 and np.count_nonzero(bval) > 0.999 * bval.size
    assert -1.0 <= bval.min() < -0.99 and 0.99 < bval.max() <= 1.0
    m = mb * 64
    assert crp.size == m + 1 and crp[-1] == cci.size and (np.diff(crp) == 3).all()
    assert 0 <= cci.min() and cci.max() < m and np.isin(cci, [0, 1, 2, 3]).sum() >= m // 4
    assert PROBE64_CHECKED_BLOCK_ROWS[0] == 0 and PROBE64_CHECKED_BLOCK_ROWS[-1] == mb - 1
    assert len(PROBE64_CHECKED_BLOCK_ROWS) == 4
    # the slab reference on a B that picks single entries out
    Bd = np.zeros((m, 2), np.float32)
    Bd[0, 0] = 1.0           # column 0 of block column 0: every row meets it
    Bd[5 * 64 + 7, 1] = 2.0
    ref, absd = probe64_block_row_reference(41, mats, Bd)
    blk0 = bval[brp[41] * 4096:(brp[41] + 1) * 4096].reshape(64, 64)
    extra = np.zeros(64)
    for r in range(64):
        row = 41 * 64 + r
        for j in range(crp[row], crp[row + 1]):
            if cci[j] == 0:
                extra[r] += cv[j]
    assert np.allclose(ref[:, 0], blk0[:, 0].astype(np.float64) + extra, rtol=0, atol=1e-15)
    assert (absd >= np.abs(ref) - 1e-12).all() and (absd[:, 0] > 0).all()


def test_rectangular_case_reaches_past_m_and_k():
    """test_hybrid_ex_rectangular_and_empty_parts: the BSR part has a block in the last
    block column (columns past k) and in the last block row (rows past m)."""
    for bs in (8, 32):
        rng = np.random.default_rng(300 + bs)
        m, k = 300, 500
        mb, kb = -(-m // bs), -(-k // bs)
        assert mb * bs > m and kb * bs > k
        brp, bci, bval = rand_bsr(rng, mb, kb, bs, 0.15, empty_rows=(2,))
        assert (bci == kb - 1).any() and brp[mb] > brp[mb - 1] and brp[3] == brp[2]
        crp, cci, cv = rand_csr_rows(rng, m, k, 9)
        assert cci.size and (np.diff(crp) == 0).any() and cci.max() < k


def test_step_d_matrix_is_split_into_segments():
    """cs2_segments' rule with 256 CUs: the step's grid is shallow and its one long block
    row is an outlier longer than L, so order holds segment lists and scratch partial
    tiles; without the long row nothing is split."""
    mb, kb, bs, n = REUSE_SEG_SHAPE
    rp, ci, v = long_row_column_sparse_bsr(np.random.default_rng(9001), mb, kb, bs)
    ntiles = -(-n // 128)
    assert mb * ntiles <= 8 * 12 * 256
    assert np.diff(rp).max() == 300 and cs2_segments_splits(rp, ntiles) == 1
    flat = np.minimum(np.diff(rp), 40)
    assert cs2_segments_splits(np.concatenate([[0], np.cumsum(flat)]), ntiles) == 0
    # a deep grid is never split
    deep = np.concatenate([[0], np.cumsum(np.r_[300, np.ones(8 * 12 * 256, int)])])
    assert cs2_segments_splits(deep, 1) == 0


def test_step_a_hub_row_is_cut_into_pieces():
    rp, ci, v = reuse_hub_csr()
    lens = np.diff(rp)
    assert rp.size == REUSE_HUB_M + 1 and ci.max() < REUSE_HUB_K
    assert lens.max() == REUSE_HUB_NNZ > CSR_PIECE_MIN
    assert np.sort(lens)[-2] <= 6 and (lens == 0).any()
    for r in (0, 1234, REUSE_HUB_M - 1):
        assert (np.diff(ci[rp[r]:rp[r + 1]]) > 0).all()
