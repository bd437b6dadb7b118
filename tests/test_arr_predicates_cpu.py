"""CPU: the predicate cases of tests/test_gpu_arr.py (field_edges.pred_cases) carry the verdicts their
construction claims -- judged by the reference's own <C>_arr_mont_is_* where oracle/_ref is built,
and by Python integers everywhere."""
import ctypes

import numpy as np
import pytest

import field_edges as fe

CURVES = ["bn128", "bls12_381"]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", fe.PRED_N)
def test_predicate_cases_vs_reference_and_integers(curve, n):
    from oracle.oracle import Reference
    ref = Reference() if Reference.available() else None
    seen = set()
    for label, pred, ops, want in fe.pred_cases(curve, n, fe.pred_positions(n)):
        assert fe.pred_model(curve, pred, ops) == want, (pred, label)
        if ref is not None:
            got = ref.arr(curve, "arr_mont_" + pred, n, *ops, restype=ctypes.c_uint8)
            assert bool(got) == want, (pred, label)
        seen.add((pred, want))
    # every predicate is seen passing and failing
    assert seen == {(p, v) for p in fe.PREDICATES for v in (True, False)}


@pytest.mark.parametrize("curve", CURVES)
def test_predicate_case_construction(curve):
    """valid_rows are canonical; the is_valid plants sit on the boundary; an offending row differs from
    its clean array in exactly one row, and for is_zero / is_one / is_equal in exactly one bit"""
    r = fe.FR[curve]
    a = fe.valid_rows(curve, 1000, 7)
    assert max(fe.from_limbs(a)) < r and len({tuple(x) for x in a.tolist()}) == 1000
    plants = {name: (fe.from_limbs(row), ok) for name, row, ok in fe.is_valid_plants(curve)}
    assert plants["r_minus_1"] == (r - 1, True) and plants["r"] == (r, False) and plants["r_plus_1"] == (r + 1, False)
    assert plants["all_ones"] == ((1 << 256) - 1, False)
    up = fe.to_row(plants["r_limb0_up"][0], 4)
    assert np.array_equal(up[1:], fe.to_row(r, 4)[1:]) and int(up[0]) == (int(fe.to_row(r, 4)[0]) + 1) % (1 << 64)
    n = 257
    clean = {pred: ops for label, pred, ops, _ in fe.pred_cases(curve, n, []) if label == "clean"}
    for label, pred, ops, want in fe.pred_cases(curve, n, fe.pred_positions(n)):
        if label == "clean":
            continue
        pos = int(label.split("@")[1])
        x, base = ops[-1], clean[pred][-1]
        assert np.nonzero((x != base).any(axis=1))[0].tolist() == [pos], (pred, label)
        if pred != "is_valid":
            diff = x[pos] ^ base[pos]
            assert sum(bin(int(w)).count("1") for w in diff) == 1, (pred, label)
    # the large size's single variant per predicate sits past the first grid of k_pred
    assert fe.pred_positions(fe.PRED_N_LARGE)[1] == fe.PRED_STRIDE + 1 < fe.PRED_N_LARGE - 1
