"""The variants that tests/test_gpu_graph_replay.py writes over a captured step's operands
(helpers.graph_replay_variant), on the host: each fits the captured buffers and the
host-side arguments baked into the graph (same sizes, dtypes, nnz / nnzb), moves what it
claims to move, and changes the step's product. A replay that kept reading stale
operands, or that froze at capture a decision taken from the data, can therefore not
equal the eager call on the variant."""
from __future__ import annotations

import numpy as np
import pytest

from helpers import (HYBRID_EX_M, REPLAY_STRUCTURE_STEPS, REPLAY_VALUE_STEPS, REUSE_HUB_K,
                     REUSE_HUB_M, REUSE_HUB_NNZ, REUSE_SEG_SHAPE, cs2_segments_splits,
                     graph_replay_variant, oracle_bsrmm_d, oracle_bsrmm_f32, oracle_bsrmm_f64,
                     oracle_csrmm_d, oracle_csrmm_f64, reversed_rows)

torch = pytest.importorskip("torch")

CAPTURED = "abcdefghikl"


def _I():
    from test_gpu_handle_reuse import _host_inputs
    return _host_inputs()


def _products(name, I, oracle):
    """The oracle's results of step `name` on the host operands I (the expected C of each
    of its products, before any rounding question: float64, or the exact fp32 / fp64
    oracles for f and k)."""
    from test_gpu_handle_reuse import A_AB, E_AB, F_AB, G_AB, I_AB, K_AB
    m, k = REUSE_HUB_M, REUSE_HUB_K
    mb, kb, bs, n = REUSE_SEG_SHAPE
    if name == "a":
        ref = oracle_csrmm_f64(oracle, m, 256, *I["csr"], I["a_B"], 256, 0)[0]
        return [A_AB[0] * ref + A_AB[1] * I["a_C0"]]
    if name in "bc":
        return [oracle_csrmm_f64(oracle, m, 64, *I["csr"], I["b_B"], 64, 0)[0]]
    if name == "l":
        rp, ci, v = I["l_csr"]
        return [oracle_csrmm_f64(oracle, m, 128, rp, ci, v.astype(np.float32),
                                 I["l_B"].astype(np.float32), 128, 0)[0]]
    if name in "de":
        ref = oracle_bsrmm_f64(oracle, 0, mb, n, bs, *I["seg"], I["seg_B"], n, 0)[0]
        return [ref if name == "d" else E_AB[0] * ref + E_AB[1] * I["seg_C0"]]
    if name == "f":
        return [oracle_bsrmm_f32(oracle, 0, I[f"small{sb}"][0].size - 1, 128, sb, *I[f"small{sb}"],
                                 I[f"small{sb}_B"], 128, 0, F_AB[0], F_AB[1], I[f"small{sb}_C0"], 128, 0)
                for sb in (8, 2)]
    if name == "g":
        ref = oracle_csrmm_f64(oracle, HYBRID_EX_M, 64, *I["hyb_A"], I["hyb_B"], 64, 0)[0]
        return [G_AB[0] * ref + G_AB[1] * I["hyb_C0"][:HYBRID_EX_M]]
    if name == "h":
        return [oracle_bsrmm_f64(oracle, 0, 19, 128, 16, *I["h16"], I["h16_B"], 128, 0, half=True)[0]]
    if name == "i":
        return [I_AB[0] * oracle_bsrmm_f64(oracle, 0, 37, n_, bs_, *I[key], I[f"{key}_B"], n_, 0,
                                           half=bs_ == 16)[0] + I_AB[1] * I["g_C0"][:37 * bs_, :n_]
                for key, bs_, n_ in (("g16", 16, 256), ("g32", 32, 128))]
    if name == "k":
        return [oracle_csrmm_d(oracle, 517, 70, *I["c64"], I["c64_Bt"], 389, 1, K_AB[0], K_AB[1],
                               I["c64_C0t"].ravel(), 517, 1),
                oracle_bsrmm_d(oracle, 0, 23, 70, 8, *I["b64"], I["b64_B"], 70, 0, K_AB[0], K_AB[1],
                               I["b64_C0"].ravel(), 70, 0)]
    raise KeyError(name)


def test_reversed_rows_on_a_small_matrix():
    rp = np.array([1, 1, 3, 4], np.int32)  # one-based, first row empty
    ci = np.array([7, 9, 2], np.int32)
    v = np.arange(6, dtype=np.float32)  # two values per entry
    rp2, ci2, v2 = reversed_rows(rp, ci, v)
    assert rp2.tolist() == [1, 2, 4, 4] and rp2.dtype == rp.dtype
    assert ci2.tolist() == [2, 7, 9] and v2.tolist() == [4, 5, 0, 1, 2, 3]
    back = reversed_rows(rp2, ci2, v2)
    assert all(np.array_equal(a, b) for a, b in zip(back, (rp, ci, v)))
    empty = reversed_rows(np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    assert empty[0].tolist() == [0] * 4 and empty[1].size == 0 and empty[2].size == 0


@pytest.mark.parametrize("name", list(CAPTURED))
def test_variant_fits_the_captured_buffers_and_changes_the_product(oracle, name):
    I = _I()
    var = graph_replay_variant(name, I)
    assert set(CAPTURED) == set(REPLAY_STRUCTURE_STEPS + REPLAY_VALUE_STEPS + "i")
    for key, new in var.items():
        old = I[key]
        assert isinstance(new, tuple) == isinstance(old, tuple), key
        for a, b in zip(*((new, old) if isinstance(old, tuple) else ((new,), (old,)))):
            assert a.shape == b.shape and a.dtype == b.dtype, f"{key}: shape / dtype"
        if not isinstance(old, tuple):
            assert not np.array_equal(new, old), f"{key}: unchanged"
            continue
        if key == "hyb":  # (csr part, bsr part): both structures kept
            for o in (0, 3):
                assert np.array_equal(new[o], old[o]) and np.array_equal(new[o + 1], old[o + 1])
                assert not np.array_equal(new[o + 2], old[o + 2])
            assert np.array_equal(new[5] == 0, old[5] == 0), "a zero inside a block stays a zero"
            continue
        rp, ci, v = new
        assert rp[0] == old[0][0] and rp[-1] == old[0][-1] and (np.diff(rp) >= 0).all(), key
        assert ci.size == rp[-1] - rp[0] and not np.array_equal(v, old[2]), key
        if name in REPLAY_STRUCTURE_STEPS:
            assert np.array_equal(np.diff(rp), np.diff(old[0])[::-1])
            assert not np.array_equal(rp, old[0]) and not np.array_equal(ci, old[1]), key
            assert np.array_equal(np.sort(v), np.sort(old[2])), key
        else:
            assert np.array_equal(rp, old[0]) and np.array_equal(ci, old[1]), key
    assert name == "i" or any(isinstance(x, tuple) for x in var.values())
    assert name != "i" or sorted(var) == ["g16_B", "g32_B", "g_C0"]
    Iv = {**I, **var}
    for j, (a, b) in enumerate(zip(_products(name, I, oracle), _products(name, Iv, oracle))):
        assert a.shape == b.shape
        assert np.mean(a != b) > 0.25, f"step {name} product {j}: the variant's result is the original's"


def test_structure_variants_move_the_hub_and_the_long_block_row():
    I = _I()
    hub = int(np.argmax(np.diff(I["csr"][0])))
    assert hub == 1234
    for name, key in (("a", "csr"), ("b", "csr"), ("l", "l_csr")):
        rp = graph_replay_variant(name, I)[key][0]
        lens = np.diff(rp)
        assert int(np.argmax(lens)) == REUSE_HUB_M - 1 - hub != hub and lens.max() == REUSE_HUB_NNZ
        assert rp[hub + 1] - rp[hub] <= 6
    mb, kb, bs, n = REUSE_SEG_SHAPE
    lens0 = np.diff(I["seg"][0])
    assert int(np.argmax(lens0)) == 5 and lens0[3] == 0
    for name in "de":
        rp, ci, v = graph_replay_variant(name, I)["seg"]
        lens = np.diff(rp)
        assert int(np.argmax(lens)) == mb - 1 - 5 == 17 and lens.max() == 300
        assert lens[mb - 1 - 3] == 0 and lens[3] > 0 and lens[5] < 300
        assert cs2_segments_splits(rp, -(-n // 128)) == 1  # still split into segments
        assert (np.diff(ci[rp[17]:rp[18]]) > 0).all()
    var = graph_replay_variant("f", I)
    for sb in (8, 2):
        G = 32 // sb
        rp0, rp = I[f"small{sb}"][0], var[f"small{sb}"][0]
        assert rp.size - 1 == 5 * G + 3  # mb = 5 G + 3: the groups of G block rows regroup
        per_group = lambda r: [int(r[min(g + G, r.size - 1)] - r[g]) for g in range(0, r.size - 1, G)]  # noqa: E731
        assert per_group(rp) != per_group(rp0) and per_group(rp) != per_group(rp0)[::-1]
