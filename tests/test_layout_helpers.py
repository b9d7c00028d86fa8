"""framed() (tests/helpers.py) on the host: the layout it builds and the
checker's guard check, which must fail for one changed word of every sentinel
region and pass when only the data region changes (so the GPU layout tests'
"padding untouched" assertions cannot pass vacuously). And the case lists of the
grouped entries' layout tests against the header's documented contract, so that a
later edit of a list cannot silently empty a class."""
from __future__ import annotations

import numpy as np
import pytest

from helpers import FRAME_GUARD, framed

torch = pytest.importorskip("torch")

DTYPES = [np.float16, np.float32, np.float64]


def _frame(dtype, rows=5, cols=7, ld=10, off=3):
    data = np.arange(rows * cols, dtype=dtype).reshape(rows, cols)
    view, chk = framed(data, ld, off, device="cpu")
    return data, view, chk


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_and_extraction(dtype):
    data, view, chk = _frame(dtype)
    assert chk.buffer.numel() == 2 * FRAME_GUARD + 3 + 5 * 10
    assert view.numel() == 5 * 10 + FRAME_GUARD
    assert view.data_ptr() == chk.buffer.data_ptr() + (FRAME_GUARD + 3) * np.dtype(dtype).itemsize
    v = view.numpy()
    assert np.array_equal(v[:50].reshape(5, 10)[:, :7], data)
    # every other word is the NaN sentinel, one bit pattern
    rest = np.concatenate([chk.buffer.numpy()[:FRAME_GUARD + 3], v[:50].reshape(5, 10)[:, 7:].ravel(),
                           v[50:]])
    assert np.isnan(rest).all()
    assert np.unique(rest.view(chk.word)).size == 1
    got = chk("fresh")
    assert got.dtype == dtype and np.array_equal(got, data)
    chk.unchanged("fresh")


@pytest.mark.parametrize("dtype", DTYPES)
def test_data_region_changes_pass(dtype):
    data, view, chk = _frame(dtype)
    body = view[:50].view(5, 10)
    body[:, :7] = 0.5
    body[2, 3] = float("nan")
    got = chk("data only")
    assert np.isnan(got[2, 3]) and (np.delete(got.ravel(), 2 * 7 + 3) == 0.5).all()
    with pytest.raises(AssertionError, match="data region changed, first at row 0 column 0"):
        chk.unchanged("input")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("region,index", [
    ("front guard", 0), ("front guard", FRAME_GUARD - 1),
    ("offset gap", FRAME_GUARD), ("offset gap", FRAME_GUARD + 2),
    ("padding columns", FRAME_GUARD + 3 + 7), ("padding columns", FRAME_GUARD + 3 + 4 * 10 + 9),
    ("back guard", FRAME_GUARD + 3 + 50), ("back guard", 2 * FRAME_GUARD + 3 + 50 - 1)])
def test_one_changed_sentinel_word_fails(dtype, region, index):
    """One word of each region, first and last: a finite value, and a NaN of another
    payload (equal as a float comparison would see it, different in bits)."""
    for value in (1.0, float("nan")):
        _, _, chk = _frame(dtype)
        chk.buffer[index] = value
        with pytest.raises(AssertionError, match=f"case: {region} changed, first at "):
            chk("case")
        with pytest.raises(AssertionError, match=f"{region} changed"):
            chk.unchanged("case")


@pytest.mark.parametrize("dtype", DTYPES)
def test_read_modify_write_of_a_sentinel_fails(dtype):
    """An epilogue that reads a padding word and stores beta * word + 0 hands a quiet
    NaN back with its payload: the sentinels are signalling NaNs, so what any
    arithmetic returns differs from them in bits, while a plain copy does not."""
    _, _, chk = _frame(dtype)
    i = FRAME_GUARD + 3 + 8  # a padding word of row 0
    chk.buffer[i] = chk.buffer[i].clone()
    chk("copied")
    chk.buffer[i] = chk.buffer[i] * 0.5 + 0.0
    assert torch.isnan(chk.buffer[i])
    with pytest.raises(AssertionError, match="padding columns changed, first at row 0 column 8"):
        chk("scaled")


def test_failure_names_the_first_index():
    _, _, chk = _frame(np.float32)
    chk.buffer[FRAME_GUARD + 3 + 2 * 10 + 8] = 0.0
    chk.buffer[FRAME_GUARD + 3 + 3 * 10 + 7] = 0.0
    with pytest.raises(AssertionError, match=r"padding columns changed, first at row 2 column 8 "
                                             r"\(ld 10\): 0x0, was 0x7f80beef"):
        chk("C")
    _, _, chk = _frame(np.float32)
    chk.buffer[FRAME_GUARD + 1] = 0.0
    with pytest.raises(AssertionError, match="offset gap changed, first at index 1 of 3"):
        chk("C")


@pytest.mark.parametrize("dtype,off", [(np.float32, 0), (np.float32, 1), (np.float32, 2),
                                       (np.float32, 3), (np.float32, 4), (np.float64, 1),
                                       (np.float64, 2), (np.float16, 3), (np.float16, 8)])
def test_view_alignment_follows_off(dtype, off):
    data = np.ones((2, 3), dtype)
    view, chk = framed(data, 3, off, device="cpu")
    assert view.data_ptr() % 16 == off * np.dtype(dtype).itemsize % 16
    assert np.array_equal(chk("tight"), data)


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_assert_normwise_rejects_non_finite_results(poison):
    """The layout tests poison a wrong read with NaN: a non-finite result against a
    finite reference must fail the norm-wise check (one element, and every element),
    a result inside the tolerance must pass."""
    from helpers import TOL_F32, assert_normwise
    rng = np.random.default_rng(0)
    ref = rng.standard_normal((6, 5))
    absd = np.abs(ref) + 1.0
    got = (ref + 0.5 * TOL_F32 * absd).astype(np.float64)
    assert_normwise(got, ref, absd, TOL_F32, "close")
    one = got.copy()
    one[4, 3] = poison
    with pytest.raises(AssertionError, match=r"one: 1 / 30 elements .* worst flat index 23: got "):
        assert_normwise(one, ref, absd, TOL_F32, "one")
    with pytest.raises(AssertionError, match="all: 30 / 30 elements"):
        assert_normwise(np.full_like(got, poison), ref, absd, TOL_F32, "all")
    with pytest.raises(AssertionError, match="far: 1 / 30"):
        far = got.copy()
        far[0, 0] += 1.0
        assert_normwise(far, ref, absd, TOL_F32, "far")
    # float32 results too (what the device returns)
    with pytest.raises(AssertionError, match="f32: 30 / 30"):
        assert_normwise(np.full((6, 5), poison, np.float32), ref, absd, TOL_F32, "f32")


def test_integer_arrays_take_their_own_fill():
    idx = np.arange(9, dtype=np.int32).reshape(1, 9)
    view, chk = framed(idx, 9, 1, fill=0, device="cpu")
    assert view[:9].tolist() == list(range(9)) and chk.buffer[FRAME_GUARD].item() == 0
    chk.unchanged("colind")
    chk.buffer[FRAME_GUARD] = 5
    with pytest.raises(AssertionError, match="offset gap changed"):
        chk("colind")


# ------------------------------------------ the grouped entries' case lists
# The documented contract of the two grouped products, restated from include/spmm_hip.h
# (not from the launchers): the causes of SPMM_STATUS_NOT_SUPPORTED for a case
# (n, order_b, order_c, (off_B, pad_B, off_C, pad_C)) on operands made by framed().
_GROUPED = {  # itemsize of B, unit of n and ldb, (K, M) of the tests' matrix, the tests' n
    "f32": (4, 4, (60 * 32, 37 * 32), (64, 132)),
    "f16": (2, 8, (60 * 16, 37 * 16), (136, 264)),
}


def _address(off, itemsize):
    """Address modulo 256 of a framed() view: the allocation is 256-byte aligned and the
    front guard FRAME_GUARD elements long."""
    return (FRAME_GUARD + off) * itemsize % 256


def _causes(kind, n, ob, oc, lay):
    size_b, unit, (K, M), _ = _GROUPED[kind]
    off_b, pad_b, off_c, pad_c = lay
    ldb = (n if ob == 0 else K) + pad_b
    ldc = (n if oc == 0 else M) + pad_c
    causes = set()
    if n % unit:
        causes.add("n")
    if ob == 0 and ldb % unit:
        causes.add("ldb")
    if _address(off_b, size_b) % 16:
        causes.add("B base")
    if kind == "f32":  # "a row-major ldb or ldc % 4 != 0, or B or C is not 16-B aligned"
        if oc == 0 and ldc % 4:
            causes.add("ldc")
        if _address(off_c, 4) % 16:
            causes.add("C base")
    return causes


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_grouped_case_lists_reach_what_they_claim(kind):
    """The rejected list holds every documented cause alone at least once (and nothing
    the header accepts), the accepted list no case that matches a cause."""
    import helpers
    accepted = getattr(helpers, f"GROUPED_{kind.upper()}_ACCEPTED")
    rejected = getattr(helpers, f"GROUPED_{kind.upper()}_REJECTED")
    ns = _GROUPED[kind][3]
    alone = set()
    for cn, ob, oc, lay in rejected:
        for n in ([cn] if cn else ns):
            causes = _causes(kind, n, ob, oc, lay)
            assert len(causes) == 1, f"{(cn, ob, oc, lay)} at n={n}: causes {sorted(causes)}"
            alone |= causes
    want = {"n", "ldb", "B base"} | ({"ldc", "C base"} if kind == "f32" else set())
    assert alone == want
    for cn, ob, oc, lay in accepted:
        for n in ([cn] if cn else ns):
            assert not _causes(kind, n, ob, oc, lay), f"{(cn, ob, oc, lay)} at n={n} is rejected"
    if kind == "f32":  # the residues the issue of each cause names
        lays = [c[3] for c in rejected]
        assert {l[1] % 4 for l in lays if l[1]} >= {1, 2} and {l[3] % 4 for l in lays if l[3]} >= {1, 2}
        assert {l[0] for l in lays if l[0]} >= {1, 2} and {l[2] for l in lays if l[2]} >= {1, 2}
        assert any(c[1] == 1 and c[3][0] for c in rejected) and any(c[2] == 1 and c[3][2] for c in rejected)


def test_accepted_fp32_lists_leave_the_256_byte_base():
    """Every fp32 list of layouts on which a fast path is asserted holds a base that is
    16-byte but not 256-byte aligned, for B and for C."""
    from helpers import ALIGNED_LAYOUTS_F32, GROUPED_F32_ACCEPTED
    from test_gpu_layout import _STREAM_LAYOUTS
    from test_gpu_layout_analysed import AN32_STREAM
    lists = {"ALIGNED_LAYOUTS_F32": ALIGNED_LAYOUTS_F32,
             "GROUPED_F32_ACCEPTED": [c[3] for c in GROUPED_F32_ACCEPTED],
             "GROUPED_F32_ACCEPTED, row-major": [c[3] for c in GROUPED_F32_ACCEPTED if c[1:3] == (0, 0)],
             "AN32_STREAM": AN32_STREAM, "_STREAM_LAYOUTS[fp32]": _STREAM_LAYOUTS[False]}
    for name, lays in lists.items():
        for i, operand in ((0, "B"), (2, "C")):
            addr = [_address(lay[i], 4) for lay in lays]
            assert any(a % 256 != 0 and a % 16 == 0 for a in addr), f"{name}: no such {operand} base"
