"""Division by a linear factor and the KZG prover on the GPU (zk_lindiv.hip, zkg_kzg_commit_device,
zkg_kzg_open_device), bit for bit against the restated reference loop <C>_poly_mont_div_by_vanishing with
expo_n = 1 (the oracle, as tests/test_gpu_arr.py) and the oracle's MSM."""
import os

import numpy as np
import pytest

import pairing_model as pm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ("bn128", "bls12_381")
K, T = 8, 2048  # rows per lane and per tile by default
SIZES = (1, 2, 3, K - 1, K, K + 1, 64 * K - 1, 64 * K + 1, T - 1, T, T + 1, 2 * T + 5)


def limbs(v):
    return [(v >> (64 * i)) & (2 ** 64 - 1) for i in range(4)]


def mont(curve, v):
    """the Montgomery row of the residue v"""
    return np.array(limbs(v % pm.tower(curve).r * (1 << 256) % pm.tower(curve).r), dtype=np.uint64)


def want_div(oracle, curve, poly, z):
    n = poly.shape[0]
    q, r, _ = oracle.div_by_vanishing(curve, poly, 1, z, nquot=max(0, n - 1), nrem=1)
    return q, r[0]


def check_div(gpu, oracle, curve, poly, z):
    q, v = gpu.poly_div_linear(curve, poly, z)
    wq, wv = want_div(oracle, curve, poly, z)
    assert q.shape == (max(0, poly.shape[0] - 1), 4)
    assert np.array_equal(q, wq)
    assert np.array_equal(v, wv)
    return q, v


@pytest.mark.parametrize("curve", CURVES)
def test_div_linear_equals_reference(gpu, oracle, curve):
    assert gpu.poly_lindiv_tile() == K
    z = gpu.gen_fr(curve, 0x11E0, 1)[0]
    for n in SIZES:
        check_div(gpu, oracle, curve, gpu.gen_fr(curve, 0x11E1 + n, n), z)
    q, v = gpu.poly_div_linear(curve, np.zeros((0, 4), dtype=np.uint64), z)
    assert q.shape == (0, 4) and not v.any()


@pytest.mark.parametrize("curve", CURVES)
def test_div_linear_many_tiles(gpu, oracle, curve):
    """one row per lane: 301 tiles, two iterations of the carry pass"""
    n = 256 * 300 + 7
    poly = gpu.gen_fr(curve, 0x11E2, n)
    z = gpu.gen_fr(curve, 0x11E3, 1)[0]
    gpu.poly_set_lindiv_tile(1)
    try:
        assert gpu.poly_lindiv_tile() == 1
        check_div(gpu, oracle, curve, poly, z)
        gpu.poly_set_lindiv_tile(2)
        check_div(gpu, oracle, curve, poly[:256 * 2 * 3 + 1], z)
        gpu.poly_set_lindiv_tile(4)
        check_div(gpu, oracle, curve, poly[:256 * 4 * 2 + 3], z)
    finally:
        gpu.poly_set_lindiv_tile(0)
    assert gpu.poly_lindiv_tile() == K


@pytest.mark.parametrize("curve", CURVES)
def test_edge_rows(gpu, oracle, curve):
    r = pm.tower(curve).r
    n = T + 37
    poly = gpu.gen_fr(curve, 0x11E4, n)
    zero, one, minus1 = mont(curve, 0), mont(curve, 1), mont(curve, r - 1)
    q, v = check_div(gpu, oracle, curve, poly, zero)  # z = 0: the shifted polynomial and a_0
    assert np.array_equal(q, poly[1:]) and np.array_equal(v, poly[0])
    check_div(gpu, oracle, curve, poly, one)
    check_div(gpu, oracle, curve, poly, minus1)
    z = gpu.gen_fr(curve, 0x11E5, 1)[0]
    q, v = check_div(gpu, oracle, curve, np.zeros((n, 4), dtype=np.uint64), z)  # the zero polynomial
    assert not q.any() and not v.any()
    top0 = poly.copy()
    top0[n - 300:] = 0  # zero top coefficients: zero tail rows
    q, _ = check_div(gpu, oracle, curve, top0, z)
    assert not q[n - 301:].any() and q[n - 302].any()
    check_div(gpu, oracle, curve, np.tile(minus1, (n, 1)), minus1)  # every coefficient and the point r - 1
    # z a root: p = (x - z) g, so the value is exactly zero and the quotient is g
    g = gpu.gen_fr(curve, 0x11E6, n)
    zm = sum(int(x) << (64 * i) for i, x in enumerate(z))  # the Montgomery form is linear: -z is r - zm
    lin = np.stack([np.array(limbs((r - zm) % r), dtype=np.uint64), one])
    p = gpu.poly_mul(curve, g, lin)
    q, v = check_div(gpu, oracle, curve, p, z)
    assert not v.any() and np.array_equal(q, g)


@pytest.mark.parametrize("nz", (1, 2, 5))
@pytest.mark.parametrize("curve", CURVES)
def test_batches(gpu, curve, nz):
    n = T + 11
    poly = gpu.gen_fr(curve, 0x11E7, n)
    zs = gpu.gen_fr(curve, 0x11E8, nz)
    if nz >= 2:
        zs[1] = zs[0]  # a repeated point
    if nz >= 5:
        zs[3] = 0      # and a zero one
    quot, vals = gpu.poly_div_linear(curve, poly, zs)
    assert quot.shape == (nz, n - 1, 4) and vals.shape == (nz, 4)
    for k in range(nz):
        q, v = gpu.poly_div_linear(curve, poly, zs[k])
        assert np.array_equal(quot[k], q) and np.array_equal(vals[k], v), k
        assert np.array_equal(v, gpu.poly_eval_at(curve, poly, zs[k])), k
    d_p = gpu.DeviceBuffer(poly)
    try:
        rc, only = gpu.poly_div_linear_device(curve, n, d_p, zs)  # no quotient buffer: the values alone
        assert rc == 0 and np.array_equal(only, vals)
    finally:
        d_p.free()


@pytest.mark.parametrize("curve", CURVES)
def test_host_and_device_agree_and_overlap_is_refused(gpu, curve):
    n, nz = 2 * T + 5, 2
    poly = gpu.gen_fr(curve, 0x11E9, n)
    zs = gpu.gen_fr(curve, 0x11EA, nz)
    quot, vals = gpu.poly_div_linear(curve, poly, zs)
    d_p, d_q = gpu.DeviceBuffer(poly), gpu.DeviceBuffer.empty(nz * (n - 1) * 32)
    gpu.set_error_mode(True)
    try:
        assert gpu.last_error() is None
        rc, dv = gpu.poly_div_linear_device(curve, n, d_p, zs, d_q)
        assert rc == 0 and np.array_equal(dv, vals)
        assert np.array_equal(d_q.to_host(quot), quot)
        assert np.array_equal(d_p.to_host(poly), poly)  # the input is not written
        rc, _ = gpu.poly_div_linear_device(curve, n, d_p, zs[:1], d_p)  # in place
        assert rc != 0 and "overlaps" in gpu.last_error()
        inside = gpu.DeviceBuffer.__new__(gpu.DeviceBuffer)
        inside.ptr, inside.nbytes = d_p.ptr + 32 * (n - 1), 32  # the last row of the polynomial
        rc, _ = gpu.poly_div_linear_device(curve, n, d_p, zs[:1], inside)
        assert rc != 0 and "overlaps" in gpu.last_error()
        assert np.array_equal(d_p.to_host(poly), poly)
        rc, dv = gpu.poly_div_linear_device(curve, n, d_p, zs, d_q)  # the next call succeeds
        assert rc == 0 and np.array_equal(dv, vals) and gpu.last_error() is None
    finally:
        gpu.set_error_mode(False)
        gpu.last_error()
        d_p.free()
        d_q.free()


# ---------------------------------------------------------------------------- commitments and openings

LOG = 6


@pytest.fixture(scope="module")
def setups(gpu):
    """(setup, g1, g2, affine tau_g1s, affine lagrange_taus) per curve at log_size 6, built once"""
    out = {}
    for curve in CURVES:
        g = np.load(os.path.join(ROOT, "tests", "golden", f"pairing_{curve}.npz"))
        gen = int(np.nonzero((g["factors"][:, 0] == 1) & (g["factors"][:, 4] == 1) & (g["family"] >= 0))[0][0])
        g1, g2 = g["P"][gen], g["Q"][gen]
        tau = gpu.gen_fr(curve, 0x11EB, 1)[0]
        s = gpu.kzg_setup(curve, tau, LOG, g1, g2)
        NP = gpu.NLIMBS_P[curve]
        like = np.empty((1 << LOG, 3 * NP), dtype=np.uint64)
        srs = gpu.batch_to_affine(curve, s.tau_g1s.to_host(like))
        lag = gpu.batch_to_affine(curve, s.lagrange_taus.to_host(like))
        out[curve] = (s, g1, g2, srs, lag)
    yield out
    for s, *_ in out.values():
        s.free()


@pytest.mark.parametrize("curve", CURVES)
def test_commitments(gpu, oracle, setups, curve):
    s, _, _, srs, lag = setups[curve]
    n = 1 << LOG
    for m in (n, n - 5, 1):
        poly = gpu.gen_fr(curve, 0x11EC + m, m)
        want = oracle.normalize(curve, oracle.msm(curve, poly, srs[:m], mont=True, out="proj"))
        assert np.array_equal(gpu.kzg_commit(s, poly), want), m
        assert np.array_equal(gpu.kzg_commit(s, poly, affine=True), oracle.to_affine(curve, want)), m
    values = gpu.gen_fr(curve, 0x11ED, n)
    want = oracle.normalize(curve, oracle.msm(curve, values, lag, mont=True, out="proj"))
    assert np.array_equal(gpu.kzg_commit_values(s, values), want)
    assert np.array_equal(gpu.kzg_commit_interpolate(s, values), want)
    with pytest.raises(ValueError, match="commitValues: expecting a vector of the same size as the KZG setup domain"):
        gpu.kzg_commit_values(s, values[:-1])
    with pytest.raises(ValueError, match="commitInterpolate: expecting"):
        gpu.kzg_commit_interpolate(s, values[:-1])
    with pytest.raises(ValueError):
        gpu.kzg_commit(s, gpu.gen_fr(curve, 0x11EE, n + 1))


@pytest.mark.parametrize("curve", CURVES)
def test_opening_equals_msm_of_reference_quotient(gpu, oracle, setups, curve):
    s, _, _, srs, _ = setups[curve]
    n = 1 << LOG
    poly = gpu.gen_fr(curve, 0x11EF, n)
    zs = gpu.gen_fr(curve, 0x11F0, 3)
    z, val, proof = gpu.kzg_open(s, poly, zs[0])
    wq, wv = want_div(oracle, curve, poly, zs[0])
    assert np.array_equal(z, zs[0]) and np.array_equal(val, wv)
    want = oracle.normalize(curve, oracle.msm(curve, wq, srs[:n - 1], mont=True, out="proj"))
    assert np.array_equal(proof, want)
    assert np.array_equal(gpu.kzg_open(s, poly, zs[0], affine=True)[2], oracle.to_affine(curve, want))
    vals, proofs = gpu.kzg_open_many(s, poly, zs)
    assert vals.shape == (3, 4) and proofs.shape == (3, 3 * gpu.NLIMBS_P[curve])
    for k in range(3):
        _, v, p = gpu.kzg_open(s, poly, zs[k])
        assert np.array_equal(vals[k], v) and np.array_equal(proofs[k], p), k
    with pytest.raises(ValueError):
        gpu.kzg_open(s, gpu.gen_fr(curve, 0x11F1, n + 1), zs[0])


def fr_plus_one(curve, a):
    r = pm.tower(curve).r
    v = (sum(int(x) << (64 * i) for i, x in enumerate(a)) + (1 << 256)) % r
    return np.array(limbs(v), dtype=np.uint64)


def verify_case(gpu, setups, curve, m):
    s, g1, g2, _, _ = setups[curve]
    NP = gpu.NLIMBS_P[curve]
    poly = gpu.gen_fr(curve, 0x11F2 + m, m)
    z, val, proof = gpu.kzg_open(s, poly, gpu.gen_fr(curve, 0x11F3, 1)[0])
    commitment = gpu.kzg_commit(s, poly)
    _, tau_g2 = s.g2_tau_g2
    tau_g2 = gpu.g2_batch_to_affine(curve, tau_g2.reshape(1, -1))[0] if tau_g2.shape[0] == 6 * NP else tau_g2
    assert gpu.kzg_verify(curve, g1, g2, tau_g2, commitment, z, val, proof)
    assert not gpu.kzg_verify(curve, g1, g2, tau_g2, commitment, z, fr_plus_one(curve, val), proof)
    return proof


def test_opening_verifies_bn128(gpu, setups):
    verify_case(gpu, setups, "bn128", 1 << LOG)


def test_opening_verifies_bls12_381(gpu, setups):
    verify_case(gpu, setups, "bls12_381", (1 << LOG) - 3)


@pytest.mark.parametrize("curve", CURVES)
def test_constant_polynomial_opens_at_infinity(gpu, setups, curve):
    NP = gpu.NLIMBS_P[curve]
    proof = verify_case(gpu, setups, curve, 1)
    inf = np.zeros(3 * NP, dtype=np.uint64)
    inf[NP:2 * NP] = gpu.fp12_one(curve)[:NP]  # (0 : 1 : 0)
    assert np.array_equal(proof, inf)
