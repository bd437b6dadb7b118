"""tests/generators.py and the expectations the GPU generator tests rely on, without a GPU: for every
named root the oracle's (and the reference's) transform equals the naive sum in Python integers."""
import numpy as np
import pytest

import generators
from field_edges import FR, field_edges, to_limbs

CURVES = ["bn128", "bls12_381"]
M_LIST = list(range(7))


def inputs(oracle, curve, m):
    """random rows with the first Fr edge values written over the head (r - 1, 0, ... among them)"""
    n = 1 << m
    x = oracle.gen_fr(curve, 0x6E00 + m, 0, n)
    edges = to_limbs(field_edges(f"{curve}_fr")[-(n // 2):], 4) if n >= 2 else x[:0]
    x[:edges.shape[0]] = edges
    return np.ascontiguousarray(x)


def test_names_at_small_sizes():
    assert generators.exponents(0) == {"inv": 0}
    assert generators.exponents(1) == {"inv": 1}
    assert generators.exponents(2) == {"inv": 3}
    assert generators.exponents(3) == {"inv": 7, "cube": 3, "neg": 5}
    assert generators.exponents(4) == {"inv": 15, "cube": 3, "neg": 9, "k5": 5}
    for m in range(1, 21):
        assert all(k & 1 for k in generators.exponents(m).values()), m


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", M_LIST + [8, 13, 20])
def test_roots_are_primitive(oracle, curve, m):
    r = FR[curve]
    g = oracle.fft_generator(curve, m)
    gs = generators.to_std(curve, g)
    rows = generators.roots(curve, m, g)
    assert len({row.tobytes() for row in rows.values()}) == len(rows)
    for name, row in rows.items():
        w = generators.to_std(curve, row)
        assert w == pow(gs, generators.exponents(m)[name], r)
        assert pow(w, 1 << m, r) == 1, name
        if m >= 1:
            assert pow(w, 1 << (m - 1), r) == r - 1, name
        if m >= 2:  # not the canonical generator
            assert not np.array_equal(row, g), name
    if m == 0:
        assert generators.to_std(curve, rows["inv"]) == 1
    if m == 1:
        assert generators.to_std(curve, rows["inv"]) == r - 1
    if m >= 2:
        assert generators.to_std(curve, rows["inv"]) * gs % r == 1
    if "neg" in rows:
        assert generators.to_std(curve, rows["neg"]) == r - gs


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", M_LIST)
def test_oracle_ntt_is_the_naive_sum(oracle, curve, m):
    x = inputs(oracle, curve, m)
    for name, gen in generators.roots(curve, m, oracle.fft_generator(curve, m)).items():
        f = oracle.ntt(curve, m, gen, x)
        assert np.array_equal(f, generators.naive_dft(curve, m, gen, x)), name
        i = oracle.ntt(curve, m, gen, x, inverse=True)
        assert np.array_equal(i, generators.naive_dft(curve, m, gen, x, inverse=True)), name
        assert np.array_equal(oracle.ntt(curve, m, gen, f, inverse=True), x), name
        assert np.array_equal(oracle.ntt(curve, m, gen, i), x), name


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", M_LIST + [8, 12])
def test_reference_ntt_equals_oracle(oracle, reference, curve, m):
    x = inputs(oracle, curve, m)
    for name, gen in generators.roots(curve, m, oracle.fft_generator(curve, m)).items():
        for inverse in (False, True):
            assert np.array_equal(reference.ntt(curve, m, gen, x, inverse), oracle.ntt(curve, m, gen, x, inverse)), \
                (name, inverse)
