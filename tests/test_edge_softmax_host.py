"""The edge softmax's host forms (spmm_edge_softmax_csr_host_f32 / _bwd_) against the numpy
restatement of the rule (bits), float64 (accuracy), and the contract's edges. No GPU."""
from ctypes import c_void_p

import numpy as np
import pytest

import softmax_cases as sc
from softmax_cases import F
from spmm_hip import prep
from spmm_hip._lib import INVALID_VALUE, SUCCESS, lib

# The EXP rule's largest error against float64 exp over [-64, 0], in ulps of the result, as
# measured by test_exp_rule_error and recorded in DESIGN.md §4i.
U_RECORDED = 0.91


def _ulp(v):
    """The spacing of float32 at |v| (v a float64 array of normal magnitudes)."""
    return 2.0 ** (np.floor(np.log2(np.abs(v))) - 23)


@pytest.mark.parametrize("name", sc.NAMES)
def test_forward_bits(name):
    c = sc.case(name)
    y = prep.edge_softmax(c.rowptr, c.x, base=c.base)
    sc.assert_same(y, sc.forward_bits(name), name, sc.inside(c))


@pytest.mark.parametrize("name", sc.NAMES)
def test_backward_bits(name):
    c = sc.case(name)
    gx = prep.edge_softmax_bwd(c.rowptr, sc.forward_bits(name), c.g, base=c.base)
    sc.assert_same(gx, sc.backward_bits(name), name, sc.inside(c))


@pytest.mark.parametrize("name", ["lengths", "view", "special", "base1"])
def test_in_place_and_untouched(name):
    c = sc.case(name)
    mk = sc.inside(c)
    # in place: y is x, gx is g
    x = c.x.copy()
    assert prep.edge_softmax(c.rowptr, x, base=c.base, out=x) is x
    sc.assert_same(x, sc.forward_bits(name), name + " in place", mk)
    assert np.array_equal(sc.bits(x[~mk]), sc.bits(c.x[~mk])), "positions outside the view"
    g = c.g.copy()
    prep.edge_softmax_bwd(c.rowptr, sc.forward_bits(name), g, base=c.base, out=g)
    sc.assert_same(g, sc.backward_bits(name), name + " bwd in place", mk)
    assert np.array_equal(sc.bits(g[~mk]), sc.bits(c.g[~mk]))
    # out of place: a sentinel survives outside the pattern, the inputs are unchanged
    out = np.full(c.nnz, F(-7.25))
    rp, x = c.rowptr.copy(), c.x.copy()
    prep.edge_softmax(rp, x, base=c.base, out=out)
    assert (out[~mk] == F(-7.25)).all()
    assert np.array_equal(rp, c.rowptr) and np.array_equal(sc.bits(x), sc.bits(c.x))


def test_special_values():
    c = sc.case("special")
    y = prep.edge_softmax(c.rowptr, c.x, base=c.base)
    for r, a, L in c.rows():
        xr, yr = c.x[a:a + L], y[a:a + L]
        if np.isnan(xr).any() or (xr == np.inf).any() or (xr == -np.inf).all():
            assert np.isnan(yr).all(), f"row {r}"
        else:  # a -inf beside finite values
            assert (sc.bits(yr[xr == -np.inf]) == 0).all(), f"row {r}: not exactly +0"
            assert np.isfinite(yr).all()
    # one finite value: exactly 1; L equal values, L a power of two: exactly 1 / L
    assert prep.edge_softmax(np.array([0, 1], np.int32), np.array([-3.5], F))[0] == F(1)
    c = sc.case("lengths_equal")
    y = prep.edge_softmax(c.rowptr, c.x)
    for r, a, L in c.rows():
        if L & (L - 1) == 0:
            assert (y[a:a + L] == F(1) / F(L)).all(), f"L = {L}"
    # +-1e30 mixed: the smaller ones are cut to exactly +0
    c = sc.case("lengths_big")
    y = prep.edge_softmax(c.rowptr, c.x)
    for r, a, L in c.rows():
        xr = c.x[a:a + L]
        if (xr > 0).any():
            assert (sc.bits(y[a:a + L][xr < 0]) == 0).all()


def test_status_codes():
    L = lib()
    rp = np.array([0, 2, 3], np.int32)
    x = np.array([1, 2, 3], F)
    y = np.full(3, F(9))
    P = lambda a: c_void_p(a.ctypes.data)  # noqa: E731
    fwd, bwd = L.spmm_edge_softmax_csr_host_f32, L.spmm_edge_softmax_bwd_csr_host_f32
    assert fwd(2, 3, P(rp), 0, P(x), P(y)) == SUCCESS
    assert fwd(-1, 3, P(rp), 0, P(x), P(y)) == INVALID_VALUE
    assert fwd(2, -1, P(rp), 0, P(x), P(y)) == INVALID_VALUE
    assert fwd(2, 3, P(rp), 2, P(x), P(y)) == INVALID_VALUE
    for args in ((None, P(x), P(y)), (P(rp), None, P(y)), (P(rp), P(x), None)):
        assert fwd(2, 3, args[0], 0, args[1], args[2]) == INVALID_VALUE
    assert fwd(0, 3, None, 0, None, None) == INVALID_VALUE  # the NULL check comes first
    assert fwd(0, 3, P(rp), 0, P(x), P(y)) == SUCCESS
    assert fwd(2, 0, None, 0, None, None) == SUCCESS
    assert bwd(2, 3, P(rp), 0, P(x), P(x), P(y)) == SUCCESS
    assert bwd(2, 3, P(rp), 0, P(x), None, P(y)) == INVALID_VALUE
    assert bwd(2, 3, P(rp), 0, P(x), P(x), None) == INVALID_VALUE
    assert bwd(2, 0, None, 0, None, None, None) == SUCCESS
    # a bad row pointer is refused before anything is written
    for bad in ([0, 3, 2], [0, 2, 4], [-1, 2, 3], [1, 0, 3]):
        y[:] = F(9)
        b = np.array(bad, np.int32)
        assert fwd(2, 3, P(b), 0, P(x), P(y)) == INVALID_VALUE, bad
        assert bwd(2, 3, P(b), 0, P(x), P(x), P(y)) == INVALID_VALUE, bad
        assert (y == F(9)).all(), bad
    # base 1: rowptr[0] below the base
    assert fwd(2, 3, P(rp), 1, P(x), P(y)) == INVALID_VALUE
    with pytest.raises(ValueError):
        prep.edge_softmax(rp, x, m=5)
    with pytest.raises(TypeError):
        prep.edge_softmax(rp, x.astype(np.float64))


def test_exp_rule_error():
    """The restated EXP rule (whose bits the host form is held to above) against float64
    exp: 2^20 random t in [-64, 0] plus every boundary. Prints the measured maximum."""
    rng = np.random.default_rng(1)
    t = np.concatenate([rng.uniform(-64, 0, 1 << 20), -np.exp(rng.uniform(-20, 4.15, 1 << 16))])
    t = np.clip(t, -64, 0).astype(F)
    e = sc.exp_rule(t)
    want = np.exp(t.astype(np.float64))
    err = np.abs(e.astype(np.float64) - want) / _ulp(want)
    U = float(err.max())
    print(f"EXP rule: max error {U:.4f} ulp at t = {t[err.argmax()]!r}")
    assert (e >= F(2.0 ** -93)).all() and (e <= 1).all()  # normal numbers
    assert U <= U_RECORDED
    below = np.nextafter(F(-64), F(-np.inf))
    edge = sc.exp_rule(np.array([0.0, -0.0, -64.0, below, -np.inf, np.nan, -1e30], F))
    assert sc.bits(edge[:2]).tolist() == [0x3F800000] * 2
    assert abs(float(edge[2]) - np.exp(-64.0)) <= U_RECORDED * _ulp(np.exp(-64.0))
    assert sc.bits(edge[3:5]).tolist() == [0, 0] and np.isnan(edge[5]) and sc.bits(edge[6:])[0] == 0
    # the host form computes the same EXP: a row [0, t] gives e(t) / (1 + e(t))
    tt = np.concatenate([t[:4096], np.array([-64.0, below, -np.inf], F)])
    x = np.stack([np.zeros_like(tt), tt], 1).reshape(-1)
    rp = np.arange(0, 2 * tt.size + 1, 2, dtype=np.int32)
    y = prep.edge_softmax(rp, x).reshape(-1, 2)
    et = sc.exp_rule(tt)
    s = F(1) + et
    assert np.array_equal(sc.bits(y[:, 1]), sc.bits(et / s))
    assert np.array_equal(sc.bits(y[:, 0]), sc.bits(F(1) / s))


@pytest.mark.parametrize("name", sc.NAMES)
def test_accuracy(name):
    """Per row without a non-finite value: |y - y64| <= (64 + 2U + D + 2) 2^-24 y64 and
    |sum y - 1| <= (D + 2) 2^-23; only the marked special rows are skipped."""
    c = sc.case(name)
    y = prep.edge_softmax(c.rowptr, c.x, base=c.base).astype(np.float64)
    y64 = sc.forward64(name)
    skipped = []
    for r, a, L in c.rows():
        if not np.isfinite(c.x[a:a + L]).all():
            skipped.append(r)
            continue
        D = c.depth(L)
        yr, wr = y[a:a + L], y64[a:a + L]
        bound = (64 + 2 * U_RECORDED + D + 2) * 2.0 ** -24
        assert (yr[wr == 0] == 0).all(), f"{name} row {r}: a zero of float64 is not +0"
        worst = float((np.abs(yr - wr)[wr > 0] / wr[wr > 0]).max())
        assert worst <= bound, f"{name} row {r} (L = {L}): {worst:.3e} > {bound:.3e}"
        assert abs(yr.sum() - 1.0) <= (D + 2) * 2.0 ** -23, f"{name} row {r}: sum {yr.sum()!r}"
    assert set(skipped) <= set(np.flatnonzero(c.special).tolist())
    assert len(skipped) == int(c.special[c.lens > 0].sum())
