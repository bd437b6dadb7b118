"""Batch pairings on the GPU against the reference's rows (tests/golden/pairing_<curve>.npz) and the
big-integer model (tests/pairing_model.py), bit for bit."""
import os
import random

import numpy as np
import pytest

import pairing_model as pm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ("bn128", "bls12_381")
FF = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def golden():
    return {c: np.load(os.path.join(ROOT, "tests", "golden", f"pairing_{c}.npz")) for c in CURVES}


def words(row):
    return [int(x) for x in row]


def limbs(v, n):
    return [(v >> (64 * i)) & (2 ** 64 - 1) for i in range(n)]


def tiled(g, n):
    K = g["P"].shape[0]
    idx = np.arange(n) % K
    return g["P"][idx].copy(), g["Q"][idx].copy(), g["pairing"][idx]


@pytest.mark.parametrize("curve", CURVES)
def test_rows_equal_reference(gpu, golden, curve):
    g = golden[curve]
    assert np.array_equal(gpu.pairing(curve, g["P"], g["Q"]), g["pairing"])


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 257))
@pytest.mark.parametrize("curve", CURVES)
def test_rows_tiled(gpu, golden, curve, n):
    P, Q, want = tiled(golden[curve], n)
    assert np.array_equal(gpu.pairing(curve, P, Q), want)


@pytest.mark.parametrize("curve", CURVES)
def test_rows_device(gpu, golden, curve):
    g = golden[curve]
    n = g["P"].shape[0]
    bufs = [gpu.DeviceBuffer(np.ascontiguousarray(g["P"])), gpu.DeviceBuffer(np.ascontiguousarray(g["Q"])),
            gpu.DeviceBuffer.empty(g["pairing"].nbytes)]
    try:
        assert gpu.pairing_device(curve, n, *bufs) == 0
        assert np.array_equal(bufs[2].to_host(g["pairing"]), g["pairing"])
        assert np.array_equal(bufs[0].to_host(g["P"]), g["P"])
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("curve", CURVES)
def test_reference_symbols(gpu, golden, curve):
    g, T = golden[curve], pm.tower(curve)
    lib, NP, p = gpu.load(), T.NP, T.p
    rng = random.Random(0xF8A1)
    for i in (0, int(g["twin"][1]), int(g["infinity"][1])):
        P, Q = np.ascontiguousarray(g["P"][i]), np.ascontiguousarray(g["Q"][i])
        out = np.zeros(12 * NP, dtype=np.uint64)
        getattr(lib, f"{curve}_pairing_affine")(gpu._p(P), gpu._p(Q), gpu._p(out))
        assert np.array_equal(out, g["pairing"][i]), i
        assert np.array_equal(gpu.pairing(curve, P, Q), g["pairing"][i])
    for i in (1, 9):  # (x z : y z : z) with random z, scaled on the integers
        x, y = T.g1_from_words(words(g["P"][i]))
        z = rng.randrange(1, p)
        Pp = np.array(sum((T.fp_to_words(v) for v in (x * z % p, y * z % p, z)), []), dtype=np.uint64)
        qx, qy = T.g2_from_words(words(g["Q"][i]))
        z2 = (rng.randrange(1, p), rng.randrange(1, p))
        Qp = np.array(sum((T.f2_to_words(v) for v in (T.f2mul(qx, z2), T.f2mul(qy, z2), z2)), []), dtype=np.uint64)
        assert np.array_equal(gpu.pairing_projective(curve, Pp, Qp), g["pairing"][i]), i


def fresh_pairs(gpu, golden, curve):
    """two pairs that are not in the fixture: ([a] g1, [b] g2) by the batch scalar multiplications"""
    g = golden[curve]
    gen = int(np.nonzero((g["factors"][:, 0] == 1) & (g["factors"][:, 4] == 1) & (g["family"] >= 0))[0][0])
    g1, g2 = g["P"][gen], g["Q"][gen]
    sc = gpu.gen_fr(curve, 0xF8A2, 4)
    P = gpu.scalar_mul_fixed(curve, sc[:2], g1, affine=True)
    Q = gpu.g2_scalar_mul_fixed(curve, sc[2:], g2, affine=True)
    return g1, g2, P, Q


@pytest.mark.parametrize("curve", CURVES)
def test_fresh_pairs_equal_model(gpu, golden, curve):
    T = pm.tower(curve)
    _, _, P, Q = fresh_pairs(gpu, golden, curve)
    got = gpu.pairing(curve, P, Q)
    for i in range(2):
        assert words(got[i]) == T.pairing_words(words(P[i]), words(Q[i])), i


@pytest.mark.parametrize("curve", CURVES)
def test_final_expo(gpu, golden, curve):
    g = golden[curve]
    assert np.array_equal(gpu.final_expo(curve, g["fe_src"]), g["fe_out"])
    assert np.array_equal(gpu.final_expo(curve, g["fe_src"][3]), g["fe_out"][3])
    bufs = [gpu.DeviceBuffer(np.ascontiguousarray(g["fe_src"])), gpu.DeviceBuffer.empty(g["fe_out"].nbytes)]
    try:
        assert gpu.final_expo_device(curve, 8, *bufs) == 0
        assert np.array_equal(bufs[1].to_host(g["fe_out"]), g["fe_out"])
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("curve", CURVES)
def test_product(gpu, golden, curve):
    g, T = golden[curve], pm.tower(curve)
    one = gpu.fp12_one(curve)
    assert np.array_equal(gpu.pairing_product(curve, g["P"][:1], g["Q"][:1]), g["pairing"][0])
    # ([a] P, Q) (-P, [a] Q) = 1
    g1, g2, P, Q = fresh_pairs(gpu, golden, curve)
    a = gpu.gen_fr(curve, 0xF8A3, 1)
    aP = gpu.scalar_mul_fixed(curve, a, P[0], affine=True)[0]
    aQ = gpu.g2_scalar_mul_fixed(curve, a, Q[0], affine=True)[0]
    y = sum(int(P[0][T.NP + j]) << (64 * j) for j in range(T.NP))
    negP = P[0].copy()
    negP[T.NP:] = limbs((T.p - y) % T.p, T.NP)
    Ps, Qs = np.stack([aP, negP]), np.stack([Q[0], aQ])
    assert np.array_equal(gpu.pairing_product(curve, Ps, Qs), one)
    assert gpu.pairing_check(curve, Ps, Qs)
    assert not gpu.pairing_check(curve, Ps, np.stack([Q[0], Q[1]]))
    # 65 tiled rows against the model's product of the reference's rows
    P65, Q65, rows = tiled(g, 65)
    acc = T.one()
    for r in rows:
        acc = T.mul(acc, T.from_words(words(r)))
    assert words(gpu.pairing_product(curve, P65, Q65)) == T.to_words(acc)
    bufs = [gpu.DeviceBuffer(P65), gpu.DeviceBuffer(Q65), gpu.DeviceBuffer.empty(one.nbytes)]
    try:
        assert gpu.pairing_product_device(curve, 65, *bufs) == 0
        assert words(bufs[2].to_host(one)) == T.to_words(acc)
        assert gpu.pairing_product_device(curve, 0, None, None, bufs[2]) == 0
        assert np.array_equal(bufs[2].to_host(one), one)
    finally:
        for b in bufs:
            b.free()
    # infinities only, and no rows
    inf = [int(i) for i in g["infinity"]]
    assert np.array_equal(gpu.pairing_product(curve, g["P"][inf], g["Q"][inf]), one)
    assert np.array_equal(gpu.pairing_product(curve, g["P"][:0], g["Q"][:0]), one)


@pytest.mark.parametrize("curve", CURVES)
def test_kzg_verify(gpu, golden, curve):
    g1, g2, _, _ = fresh_pairs(gpu, golden, curve)
    m = 4
    tau, x0 = gpu.gen_fr(curve, 0xF8A4, 2)
    poly = gpu.gen_fr(curve, 0xF8A5, 1 << m)
    setup = gpu.kzg_setup(curve, tau, m, g1, g2)
    try:
        NP = gpu.NLIMBS_P[curve]
        srs = gpu.batch_to_affine(curve, setup.tau_g1s.to_host(np.empty((1 << m, 3 * NP), dtype=np.uint64)))
        commitment = gpu.msm(curve, poly, srs)
        y0 = gpu.poly_eval_at(curve, poly, x0)
        num = poly.copy()
        num[0] = fr_add(curve, num[0], y0, -1)
        quot = gpu.quot_by_vanishing(curve, num, 1, x0)
        assert quot is not None
        proof = gpu.msm(curve, quot, srs[:quot.shape[0]])
        _, tau_g2 = setup.g2_tau_g2
        tau_g2_aff = gpu.g2_batch_to_affine(curve, tau_g2.reshape(1, -1))[0] if tau_g2.shape[0] == 6 * NP else tau_g2
        assert gpu.kzg_verify(curve, g1, g2, tau_g2_aff, commitment, x0, y0, proof)
        y1 = fr_add(curve, y0, limbs((1 << 256) % pm.tower(curve).r, 4), 1)  # the value plus one
        assert not gpu.kzg_verify(curve, g1, g2, tau_g2_aff, commitment, x0, y1, proof)
        assert not gpu.kzg_verify(curve, g1, g2, tau_g2_aff, commitment, x0, y0, commitment)
    finally:
        setup.free()


def fr_add(curve, a, b, sign):
    """a + sign b on Montgomery Fr rows (the form is linear)"""
    r = pm.tower(curve).r
    v = (sum(int(x) << (64 * i) for i, x in enumerate(a)) + sign * sum(int(x) << (64 * i) for i, x in enumerate(b))) % r
    return np.array(limbs(v, 4), dtype=np.uint64)


@pytest.mark.parametrize("curve", CURVES)
def test_error_mode(gpu, golden, curve):
    g = golden[curve]
    lib, cid = gpu.load(), gpu.CURVE_ID[curve]
    P, Q = np.ascontiguousarray(g["P"][:2]), np.ascontiguousarray(g["Q"][:2])
    out = np.zeros((2, g["pairing"].shape[1]), dtype=np.uint64)
    gpu.set_error_mode(True)
    try:
        assert gpu.last_error() is None
        for fn in (lib.zkg_pairing_rows, lib.zkg_pairing_product, lib.zkg_pairing_rows_device):
            assert fn(cid, -1, gpu._p(P), gpu._p(Q), gpu._p(out)) == -1
            assert "negative" in gpu.last_error()
            assert fn(cid, 2, None, gpu._p(Q), gpu._p(out)) == -1
            assert "null" in gpu.last_error()
        assert lib.zkg_pairing_final_expo(cid, 2, gpu._p(out), None) == -1
        assert "null" in gpu.last_error()
        assert lib.zkg_pairing_final_expo_device(cid, -3, None, None) == -1
        assert gpu.last_error() is not None
        assert np.array_equal(gpu.pairing(curve, P, Q), g["pairing"][:2])
        assert gpu.last_error() is None
    finally:
        gpu.set_error_mode(False)
        gpu.last_error()
