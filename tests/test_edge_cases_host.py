"""The IEEE edge-value cases of tests/edge_cases.py, proved on the host: the oracles and
the host form of the sampled product equal the order-free reference bit for bit on
every class, and each class detects the wrong behaviour it exists for (numpy mutants
of the reference) at every shape the device tests run (tests/test_gpu_edge_values.py).
No tolerance anywhere: comparisons are on integer views, NaN positions compared as a
map, payloads not at all."""
from __future__ import annotations

import numpy as np
import pytest

import edge_cases as E
from helpers import oracle_bsrmm_f32, oracle_csrmm_d, oracle_csrmm_f32, oracle_csrmm_pieces_f32
from sddmm_cases import reference_bits


def _prep():
    from spmm_hip import prep
    return prep


# ------------------------------------------------------------- the oracles agree
@pytest.mark.parametrize("n", [1, 12, 130])
@pytest.mark.parametrize("cls", E.CLASSES)
def test_csr_oracles_equal_order_free_reference(oracle, cls, n):
    """The sequential chain and the piece association (24 pieces on the hub row) both
    give the order-free bits: the classes really are order-free."""
    c, wants = E.csr_case(cls, n), E.csr_wants(cls, n)
    for (alpha, beta), want in wants.items():
        for f in (oracle_csrmm_f32, oracle_csrmm_pieces_f32):
            got = f(oracle, c["m"], n, c["rp"], c["ci"], c["val"], c["B"], n, 0, alpha=alpha,
                    beta=beta, C=c["C0"].reshape(-1))
            E.assert_bits(got, want, f"{f.__name__} class {cls} n={n} alpha={alpha} beta={beta}")


@pytest.mark.parametrize("n", [1, 12, 130])
@pytest.mark.parametrize("cls", E.CLASSES)
def test_csr_f64_oracle_equals_order_free_reference(oracle, cls, n):
    c, wants = E.csr_case(cls, n, "f64"), E.csr_wants(cls, n, "f64")
    for (alpha, beta), want in wants.items():
        got = oracle_csrmm_d(oracle, c["m"], n, c["rp"], c["ci"], c["val"], c["B"], n, 0,
                             alpha=alpha, beta=beta, C=c["C0"].reshape(-1))
        E.assert_bits(got, want, f"oracle_csrmm_d class {cls} n={n} alpha={alpha} beta={beta}",
                      "f64")


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("kind,bs", [("rand", 4), ("colsparse", 16), ("rand", 32)])
@pytest.mark.parametrize("cls", ["S", "Z", "O"])
def test_bsr_oracle_equals_order_free_reference(oracle, cls, kind, bs, direction):
    n = 12
    c = E.bsr_case_of(cls, kind, bs, n, "f32", direction)
    for (alpha, beta), want in c["wants"].items():
        got = oracle_bsrmm_f32(oracle, direction, E.BSR_MB, n, bs, c["brp"], c["bci"], c["val"],
                               c["B"], n, 0, alpha=alpha, beta=beta, C=c["C0"].reshape(-1))
        E.assert_bits(got, want, f"oracle_bsrmm_f32 class {cls} {kind} bs={bs} dir={direction} "
                                 f"alpha={alpha} beta={beta}")


@pytest.mark.parametrize("n", [1, 5, 64, 68, 260, 1030])
@pytest.mark.parametrize("name", E.SDDMM_PATTERNS)
@pytest.mark.parametrize("cls", E.CLASSES)
def test_sddmm_host_forms_equal_order_free_reference(cls, name, n):
    """prep.sddmm (spmm_sddmm_csr_host_f32) and the restated association rule
    (sddmm_cases.reference_bits: G chains and a butterfly) on the classes."""
    c, wants = E.sddmm_case(cls, name, n), E.sddmm_wants(cls, name, n)
    sl = slice(c["p0"], c["p0"] + c["nnz"])
    for (alpha, beta), want in wants.items():
        what = f"class {cls} {name} n={n} alpha={alpha} beta={beta}"
        got = _prep().sddmm(c["m"], n, c["k"], c["rp"], c["ci"], c["X"], c["Y"],
                            out=c["old"].copy(), alpha=alpha, beta=beta)
        E.assert_bits(got[sl], want, "prep.sddmm " + what)
        # outside a view nothing is written
        assert np.array_equal(E.bits(np.delete(got, np.arange(sl.start, sl.stop))),
                              E.bits(np.delete(c["old"], np.arange(sl.start, sl.stop))))
        with np.errstate(all="ignore"):
            rule = reference_bits(c["rows"], c["cols"], c["X"], c["Y"], alpha, beta, c["old"][sl])
        E.assert_bits(rule, want, "reference_bits " + what)


# ----------------------------------------------- the cases detect what they are for
MUTANT_OF = {"S": "flush", "N": "dense_mask", "Z": "minus_zero_start"}
CSR_SHAPES = sorted(set(E.CSR_N + E.CSR_N_LAYOUT + E.GESPMM_N + E.HOT_N))


@pytest.mark.parametrize("cls", sorted(MUTANT_OF))
def test_csr_cases_detect_their_mutant(cls):
    """(a) inputs flushed to zero below the smallest normal change class S's bits, (b)
    absent entries masked by a multiplication change class N's NaN map, (c) a sum
    started from -0 changes class Z's bits: at every width the device tests use, for
    every (alpha, beta) of the class (a device test loops over all of them)."""
    for fmt, shapes in (("f32", CSR_SHAPES), ("f64", E.F64_N)):
        for n in shapes:
            wants = E.csr_wants(cls, n, fmt)
            mutant = E.csr_mutants(cls, n, fmt)[MUTANT_OF[cls]]
            for ab, want in wants.items():
                assert E.differs(mutant[ab], want, fmt), f"class {cls} {fmt} n={n} {ab}: vacuous"


@pytest.mark.parametrize("cls", ["S", "Z"])
def test_sddmm_cases_detect_their_mutant(cls):
    for name in E.SDDMM_PATTERNS:
        for n in E.SDDMM_N:
            c, wants = E.sddmm_case(cls, name, n), E.sddmm_wants(cls, name, n)
            sl = slice(c["p0"], c["p0"] + c["nnz"])
            kw = {"flush": True} if cls == "S" else {"start": -0.0}
            for (alpha, beta), want in wants.items():
                bad = E.reference_dots(c["rows"], c["cols"], c["X"], c["Y"], alpha, beta,
                                       c["old"][sl], **kw)
                assert E.differs(bad, want), f"class {cls} {name} n={n}: vacuous"


def test_sddmm_class_n_is_local():
    """Class N on the sampled product: the NaN of X row 7 reaches every position of that
    row, the +inf row 5 of Y every position of column 5 (as inf or NaN), and a position
    whose row and column hold no special value is finite."""
    for name in E.SDDMM_PATTERNS:
        for n in E.SDDMM_N:
            c = E.sddmm_case("N", name, n)
            w = E.sddmm_wants("N", name, n)[(1.0, 0.0)]
            assert (c["rows"] == 7).any() and np.isnan(w[c["rows"] == 7]).all()
            assert (c["cols"] == 5).any() and not np.isfinite(w[c["cols"] == 5]).any()


BSR_SHAPES = ([("f32", kind, bs, E.BSR_N) for bs in (2, 4, 8) for kind in ("shared", "rand")] +
              [("f32", "rand", bs, E.BSR_N) for bs in (16, 32, 64)] +
              [("f32", "colsparse", bs, [64]) for bs in (16, 32)] +
              [("f32", "colsparse", 32, [128]), ("f16", "colsparse", 16, E.BSR_F16_N),
               ("f64", "rand", 2, [7]), ("f64", "rand", 16, [64])])


@pytest.mark.parametrize("fmt,kind,bs,ns", BSR_SHAPES,
                         ids=[f"{f}-{k}-bs{b}" for f, k, b, _ in BSR_SHAPES])
@pytest.mark.parametrize("cls", ["S", "Z"])
def test_bsr_cases_detect_their_mutant(cls, fmt, kind, bs, ns):
    """Flushed inputs change class S's bits and a sum started from -0 class Z's on the
    block patterns, at every block size and width the device tests use (the values do
    not depend on the block direction: one of the two is enough here)."""
    kw = {"flush": True} if cls == "S" else {"start": -0.0}
    for n in ns:
        c = E.bsr_case_of(cls, kind, bs, n, fmt, 0)
        bad = E.references(c["rows"], c["a"], c["cols"], c["B"], c["m"], c["C0"], c["ab"], fmt,
                           **kw)
        for ab, want in c["wants"].items():
            assert E.differs(bad[ab], want, fmt), f"class {cls} {fmt} {kind} bs={bs} n={n} {ab}"


@pytest.mark.parametrize("cls", ["S", "Z"])
def test_hybrid_cases_detect_their_mutant(cls):
    kw = {"flush": True} if cls == "S" else {"start": -0.0}
    for n in E.HYBRID_N:
        c = E.hybrid_case(cls, n)
        rows, cols, a = c["coo"]
        good = E.references(rows, a, cols, c["B"], c["R"], c["C0"], c["ab"])
        bad = E.references(rows, a, cols, c["B"], c["R"], c["C0"], c["ab"], **kw)
        for ab in c["ab"]:
            assert E.differs(bad[ab], good[ab]), f"class {cls} n={n} {ab}"
            # the entry's two-product form and one sum over both parts: the same values,
            # zeros of another sign only where the parts cancel
            w = c["wants"][ab]
            assert np.array_equal(w, good[ab])
            assert ((w == 0) | (E.bits(w) == E.bits(good[ab]))).all()


@pytest.mark.parametrize("cls", E.CLASSES)
def test_accumulate_is_np_add_at(cls):
    """The segment sums of accumulate() are np.add.at's onto +0.0, NaN map and bits."""
    c = E.csr_case(cls, 12)
    want = np.zeros((c["m"], 12))
    with np.errstate(all="ignore"):
        np.add.at(want, c["rows"], c["val"].astype(np.float64)[:, None]
                  * c["B"].astype(np.float64)[c["ci"]])
    E.assert_bits(E.accumulate(c["rows"], c["val"], c["ci"], c["B"], c["m"]), want,
                  f"class {cls}", "f64")


def test_exactness_assertion_catches_a_long_hub():
    """The helper's own guard: a hub row past HUB_MAX leaves class S's exact range and
    the assertion says so (units of the hub's column reach 2^24)."""
    rp, ci, rows = E.csr_pattern(hub=4200)
    rng = np.random.default_rng(0)
    val, B, C0 = E.fill("S", "f32", rng, ci.size, (E.CSR_K, 4), (E.CSR_M, 4))
    val[rp[E.CSR_HUB_ROW]:rp[E.CSR_HUB_ROW + 1]] = 2.0
    B[:, 0] = np.ldexp(1024.0, -149)
    with pytest.raises(AssertionError, match="exact range"):
        E.check_order_free("S", rows, val, ci, B, E.CSR_M, C0)
