"""Big-integer model of the three passes of zk_lindiv.hip (division by x - z as a tiled suffix scan), with the
kernel's index arithmetic restated: lanes per tile, rows per lane, the Kogge-Stone steps, the carry pass's
chunk loop and the write pass's seeding are parameters or code here.  Checked against plain synthetic division,
the oracle's restatement of <C>_poly_mont_div_by_vanishing and the reference's own build of it (expo_n = 1).
CPU only."""
import random

import numpy as np
import pytest

import pairing_model as pm

CURVES = ("bn128", "bls12_381")
R = 1 << 256


def chunk(r, lanes, K, base, n, src, dst, carry, w, wk):
    """ld_chunk: rows [base, base + lanes K) of src (zero at or above n), `carry` the suffix above the chunk;
    w the weight of one row, wk[d] = w^(K 2^d).  Returns the suffix at `base`; dst (a dict, or None) receives
    the suffix at row i under key i - 1 for 1 <= i < n."""
    a = [[src[base + l * K + q] if base + l * K + q < n else 0 for q in range(K)] for l in range(lanes)]
    h = [carry if l == lanes - 1 else 0 for l in range(lanes)]
    for l in range(lanes):
        for q in range(K - 1, -1, -1):
            h[l] = (a[l][q] + w * h[l]) % r
    d = 0
    while (1 << d) < lanes:
        x = list(h)  # the step reads what the previous step left in LDS
        for l in range(lanes):
            if l + (1 << d) < lanes:
                h[l] = (x[l] + wk[d] * x[l + (1 << d)]) % r
        d += 1
    if dst is not None:
        for l in range(lanes):
            s = h[l + 1] if l < lanes - 1 else carry
            for q in range(K - 1, -1, -1):
                s = (a[l][q] + w * s) % r
                i = base + l * K + q
                if 1 <= i < n:
                    assert i - 1 not in dst, "a row is stored once"
                    dst[i - 1] = s
    return h[0]


def weights(r, w, lanes, K):
    """host_weights: (w^(K 2^d) for every step, w^(lanes K))"""
    p, wk, d = pow(w, K, r), [], 0
    while (1 << d) < lanes:
        wk.append(p)
        p = p * p % r
        d += 1
    return wk, p


def model(r, a, z, lanes, K):
    """(quotient rows, value) by the tile pass, the carry pass and the write pass"""
    n = len(a)
    if n == 0:
        return [], 0
    T = lanes * K
    ntiles = (n + T - 1) // T
    wk, y = weights(r, z, lanes, K)
    assert y == pow(z, T, r)
    yk, _ = weights(r, y, lanes, K)
    totals = [chunk(r, lanes, K, t * T, n, a, None, 0, z, wk) for t in range(ntiles)]
    carries = {ntiles - 1: 0}
    carry = 0
    for c in range((ntiles - 1) // T, -1, -1):
        carry = chunk(r, lanes, K, c * T, ntiles, totals, carries, carry, y, yk)
    assert sorted(carries) == list(range(ntiles))
    quot = {}
    for t in range(ntiles):
        chunk(r, lanes, K, t * T, n, a, quot, carries[t], z, wk)
    assert sorted(quot) == list(range(n - 1)), "n - 1 rows, each written once"
    return [quot[j] for j in range(n - 1)], carry


def synthetic(r, a, z):
    q, s = [], 0
    for c in reversed(a):
        s = (c + z * s) % r
        q.append(s)
    return list(reversed(q[:-1])), (q[-1] if q else 0)


def to_rows(r, vals):
    """canonical Montgomery words of plain residues"""
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        m = v * R % r
        out[i] = [(m >> (64 * j)) & (2 ** 64 - 1) for j in range(4)]
    return out


def points(r, rng):
    return [0, 1, r - 1, rng.randrange(r)]


SHAPES = ((2, 1), (2, 2), (4, 2), (4, 3), (8, 1))


@pytest.mark.parametrize("lanes,K", SHAPES)
@pytest.mark.parametrize("curve", CURVES)
def test_model_equals_synthetic_division(curve, lanes, K):
    r = pm.tower(curve).r
    rng = random.Random(0x11D1 + lanes * 16 + K)
    T = lanes * K
    sizes = list(range(0, 3 * T + 3)) + [T * T - 1, T * T, T * T + 1, 2 * T * T + 5]  # the last ones: carry-pass loop
    for n in sizes:
        a = [rng.randrange(r) for _ in range(n)]
        if n > 3:
            a[-1] = a[-2] = 0  # leading zeros give zero rows
        for z in points(r, rng):
            assert model(r, a, z, lanes, K) == synthetic(r, a, z), (n, z)


@pytest.mark.parametrize("curve", CURVES)
def test_model_equals_oracle_words(oracle, curve):
    """the model's rows, as Montgomery words, against the restated reference loop (expo_n = 1)"""
    r = pm.tower(curve).r
    rng = random.Random(0x11D2)
    lanes, K = 4, 2
    for n in range(1, 3 * lanes * K + 3):
        a = [rng.randrange(r) for _ in range(n)]
        for z in points(r, rng):
            quot, val = model(r, a, z, lanes, K)
            wq, wr, _ = oracle.div_by_vanishing(curve, to_rows(r, a), 1, to_rows(r, [z])[0], nquot=n - 1, nrem=1)
            assert np.array_equal(to_rows(r, quot), wq), (n, z)
            assert np.array_equal(to_rows(r, [val]), wr), (n, z)


@pytest.mark.parametrize("curve", CURVES)
def test_model_equals_reference_words(reference, curve):
    """... and against the reference's own <C>_poly_mont_div_by_vanishing"""
    r = pm.tower(curve).r
    rng = random.Random(0x11D3)
    lanes, K = 4, 2
    for n in range(1, 3 * lanes * K + 3):
        a = [rng.randrange(r) for _ in range(n)]
        for z in points(r, rng):
            quot, val = model(r, a, z, lanes, K)
            wq = np.zeros((max(n - 1, 1), 4), dtype=np.uint64)
            wr = np.zeros((1, 4), dtype=np.uint64)
            reference.arr(curve, "poly_mont_div_by_vanishing", n, to_rows(r, a), 1, to_rows(r, [z])[0], n - 1, wq, 1, wr)
            assert np.array_equal(to_rows(r, quot), wq[:n - 1]), (n, z)
            assert np.array_equal(to_rows(r, [val]), wr), (n, z)


def test_refusals_need_no_gpu(zk):
    """negative sizes, missing pointers and an overlapping quotient are refused before a device is opened"""
    lib = zk.load()
    buf = np.zeros((8, 4), dtype=np.uint64)
    z = np.zeros((1, 4), dtype=np.uint64)
    p = buf.ctypes.data
    zk.last_error()
    for fn in (lib.zkg_poly_div_linear, lib.zkg_poly_div_linear_device):
        assert fn(0, -1, p, 1, z.ctypes.data, None, z.ctypes.data) != 0
        assert "negative" in zk.last_error()
        assert fn(0, 4, p, 1, None, None, z.ctypes.data) != 0
        assert "null" in zk.last_error()
        assert fn(7, 4, p, 1, z.ctypes.data, None, z.ctypes.data) != 0
        assert "curve" in zk.last_error()
        assert fn(0, 4, p, 1, z.ctypes.data, p + 32 * 3, z.ctypes.data) != 0  # rows 3 .. 5 lie inside the polynomial
        assert "overlaps" in zk.last_error()
        assert zk.last_error() is None
    out = np.zeros(18, dtype=np.uint64)
    assert lib.zkg_kzg_commit_device(0, -2, None, None, out.ctypes.data) != 0
    assert "negative" in zk.last_error()
    assert lib.zkg_kzg_open_device(1, 4, None, None, 1, z.ctypes.data, z.ctypes.data, out.ctypes.data) != 0
    assert "null" in zk.last_error()
    zk.poly_set_lindiv_tile(1)
    try:
        assert zk.poly_lindiv_tile() == 1
        zk.poly_set_lindiv_tile(3)
        assert zk.poly_lindiv_tile() == 2
        zk.poly_set_lindiv_tile(100)
        assert zk.poly_lindiv_tile() == 8
    finally:
        zk.poly_set_lindiv_tile(0)
    assert zk.poly_lindiv_tile() == 8
