"""Batch point validation on the GPU (zkg_g{1,2}_check_rows): every flag of every row against the reference --
canonical by integer compare, on-curve and infinity from the reference's predicates, membership as
is_infinity(scl_Fr_std(r, P)) -- on both curves, both groups and every coordinate system of the group.

The rows (tests/check_points.py): subgroup points, infinity in each encoding and its near misses, rows scaled by a
random Z, off-curve rows, non-canonical rows, and on-curve rows outside the subgroup (random curve points,
points of small order, G + T).  A pool of 400 (G1) / 600 (G2) rows per coordinate system goes through the
reference once; the cases at n = 1 .. 1000 draw from it, and every row of every case is compared."""
import ctypes

import numpy as np
import pytest

import check_points as cp

pytestmark = pytest.mark.gpu

GROUPS = [(c, g) for c in cp.CURVES for g in (1, 2)]
CASES = [(c, g, co) for c, g in GROUPS for co in cp.COORDS[g]]
VALID = cp.CANONICAL | cp.ON_CURVE | cp.IN_SUBGROUP


@pytest.fixture(autouse=True)
def _default_hooks(zk):
    yield
    zk.check_set_mode(-1)
    zk.check_set_max_lanes(0)


def _check(zk, group):
    return zk.g1_check if group == 1 else zk.g2_check


def _explain(labels, idx, got, want):
    bad = np.nonzero(got != want)[0]
    return [(int(i), labels[idx[i]], int(got[i]), int(want[i])) for i in bad[:8]]


@pytest.mark.parametrize("curve,group,coords", CASES)
def test_flags_match_the_reference_in_both_modes(gpu, reference, curve, group, coords):
    zk = gpu
    rows, labels, want = cp.pool(zk, reference.lib, curve, group, coords)
    assert set(want.tolist()) >= {0, cp.CANONICAL, VALID}  # the pool holds every kind of row
    if cp.group_order(curve, group) != cp.params(curve)[1]:
        assert cp.CANONICAL | cp.ON_CURVE in want.tolist()  # on the curve, outside the subgroup
    for n in cp.SIZES:
        idx = cp.case_indices(curve, group, coords, n)
        case = np.ascontiguousarray(rows[idx])
        before = case.copy()
        for mode in (0, 1):
            zk.check_set_mode(mode)
            got = _check(zk, group)(curve, case, coords)
            assert got.shape == (n,) and got.dtype == np.uint8
            assert np.array_equal(got, want[idx]), (n, mode, _explain(labels, idx, got, want[idx]))
        assert np.array_equal(case, before)  # inputs are never written
    assert _check(zk, group)(curve, rows[:0], coords).shape == (0,)  # n = 0


@pytest.mark.parametrize("curve,group", GROUPS)
def test_grid_stride_loop_count_and_device_form(gpu, reference, curve, group):
    zk = gpu
    lib = zk.load()
    coords = "proj"
    rows, labels, want = cp.pool(zk, reference.lib, curve, group, coords)
    n = 1000
    idx = cp.case_indices(curve, group, coords, n)
    case = np.ascontiguousarray(rows[idx])
    failing = int(np.count_nonzero((want[idx] & VALID) != VALID))
    assert 0 < failing < n
    f = getattr(lib, f"zkg_g{group}_check_rows")
    fd = getattr(lib, f"zkg_g{group}_check_rows_device")
    cid = zk.CURVE_ID[curve]
    for mode in (0, 1):
        zk.check_set_mode(mode)
        zk.check_set_max_lanes(256)  # 4 rows per lane
        got = _check(zk, group)(curve, case, coords)
        assert np.array_equal(got, want[idx]), (mode, _explain(labels, idx, got, want[idx]))
        zk.check_set_max_lanes(0)
    zk.check_set_mode(0)
    # the count: with flags, and alone
    flags = np.zeros(n, dtype=np.uint8)
    assert f(cid, n, case.ctypes.data, 1, flags.ctypes.data) == failing
    assert f(cid, n, case.ctypes.data, 1, None) == failing
    all_valid = zk.g1_all_valid if group == 1 else zk.g2_all_valid
    assert not all_valid(curve, case, coords)
    good = np.ascontiguousarray(case[(want[idx] & VALID) == VALID])
    assert good.shape[0] == n - failing and all_valid(curve, good, coords)
    # the device form: the same flags, guard bytes after flag n - 1 untouched, the input bit-identical
    d_pts = zk.DeviceBuffer(case)
    guard = np.full(n + 64, 0xA5, dtype=np.uint8)
    d_flags = zk.DeviceBuffer(guard)
    try:
        chk = zk.g1_check_device if group == 1 else zk.g2_check_device
        assert chk(curve, n, d_pts, d_flags, coords=coords) == failing
        out = d_flags.to_host(guard)
        assert np.array_equal(out[:n], want[idx])
        assert np.all(out[n:] == 0xA5)
        assert chk(curve, n, d_pts, None, coords=coords) == failing
        assert np.array_equal(d_flags.to_host(guard), out)
        assert np.array_equal(d_pts.to_host(case), case)
        # refusals write nothing
        zk.last_error()
        assert fd(cid, -1, d_pts.ptr, 1, d_flags.ptr) == -1
        assert fd(cid, n, d_pts.ptr, 7, d_flags.ptr) == -1
        assert fd(9, n, d_pts.ptr, 1, d_flags.ptr) == -1
        if group == 2:
            assert fd(cid, n, d_pts.ptr, 2, d_flags.ptr) == -1
        assert zk.last_error() is None
        assert np.array_equal(d_flags.to_host(guard), out)
    finally:
        d_pts.free()
        d_flags.free()


def _srs(zk, reference, curve):
    NP = zk.NLIMBS_P[curve]
    tau = zk.gen_fr(curve, 0xC0FFEE, 1)[0]
    g1 = zk.gen_points(curve, 11, 1)[0]
    g2 = cp.golden_io.g2_points(reference.lib, curve, 1)[0]
    setup = zk.kzg_setup(curve, tau, 6, g1, g2, g2_powers=3)
    try:
        P = setup.tau_g1s.to_host(np.zeros((64, 3 * NP), dtype=np.uint64))
        Q = setup.tau_g2s.to_host(np.zeros((3, 6 * NP), dtype=np.uint64))
    finally:
        setup.free()
    return P, Q


@pytest.mark.parametrize("curve", cp.CURVES)
def test_srs_check(gpu, reference, curve):
    zk = gpu
    NP = zk.NLIMBS_P[curve]
    P, Q = _srs(zk, reference, curve)
    rho = 0x1234567890ABCDEF1234567
    res = zk.srs_check(curve, P, Q, rho=rho)
    assert res and res.ok and res.failed is None
    assert zk.srs_check(curve, P, Q)  # rho drawn by the call
    # P_5 replaced by another subgroup point
    bad = P.copy()
    bad[5] = zk.batch_from_affine(curve, zk.gen_points(curve, 99, 1))[0]
    res = zk.srs_check(curve, bad, Q, rho=rho)
    assert not res and res.failed == "g1 powers"
    # P_5 replaced by a point that is no subgroup point: on the curve outside the subgroup (BLS12-381), off the
    # curve (BN128: its G1 has cofactor 1)
    bad = P.copy()
    if curve == "bls12_381":
        bad[5] = zk.batch_from_affine(curve, cp.golden_io.bls_nonsubgroup_points(1, 5))[0]
    else:
        bad[5, 0] ^= np.uint64(1)
    res = zk.srs_check(curve, bad, Q, rho=rho)
    assert not res and res.failed == "points"
    # Q_2 replaced by a wrong subgroup point
    badq = Q.copy()
    badq[2] = zk.g2_batch_from_affine(curve, cp.golden_io.g2_points(reference.lib, curve, 1, k0=777))[0]
    res = zk.srs_check(curve, P, badq, rho=rho)
    assert not res and res.failed == "g2 powers"
    # infinity
    bad = P.copy()
    bad[7] = 0
    bad[7, NP:2 * NP] = P[7, NP:2 * NP]  # (0 : y : 0)
    res = zk.srs_check(curve, bad, Q, rho=rho)
    assert not res and res.failed == "points"
    badq = zk.g2_batch_to_affine(curve, Q)
    assert zk.srs_check(curve, zk.batch_to_affine(curve, P), badq, rho=rho)  # affine columns are accepted too
    badq[1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    res = zk.srs_check(curve, P, badq, rho=rho)
    assert not res and res.failed == "points"


@pytest.mark.parametrize("curve", cp.CURVES)
def test_kzg_verify_validate(gpu, reference, curve):
    """validate=True: a good proof is accepted, an off-curve proof row returns False; validate=False is as before"""
    zk = gpu
    NP = zk.NLIMBS_P[curve]
    r = cp.params(curve)[1]
    tau, x0 = 0x1234567, 0x89ABCDE
    coeffs = [3, 1, 4, 1, 5, 9, 2, 6]
    y0 = sum(c * pow(x0, i, r) for i, c in enumerate(coeffs)) % r
    # q = (f - y0) / (X - x0) by synthetic division
    q = [0] * (len(coeffs) - 1)
    acc = 0
    for i in range(len(coeffs) - 1, 0, -1):
        acc = (coeffs[i] + acc * x0) % r
        q[i - 1] = acc
    mont = lambda v: zk._fr_mont(curve, v)
    g1 = zk.gen_points(curve, 11, 1)[0]
    g2 = cp.golden_io.g2_points(reference.lib, curve, 1)[0]
    srs = zk.srs_powers(curve, mont(tau), len(coeffs), g1, affine=True)
    tau_g2 = zk.g2_scalar_mul_fixed(curve, mont(tau).reshape(1, 4), g2, affine=True)[0]
    commitment = zk.msm(curve, np.stack([mont(c) for c in coeffs]), srs)
    proof = zk.msm(curve, np.stack([mont(c) for c in q]), np.ascontiguousarray(srs[:len(q)]))
    args = (curve, g1, g2, tau_g2, commitment, mont(x0), mont(y0))
    assert zk.kzg_verify(*args, proof) is True
    assert zk.kzg_verify(*args, proof, validate=True) is True
    bad = proof.copy()
    bad[0] ^= np.uint64(2)  # one bit of X: off the curve
    assert zk.kzg_verify(*args, bad, validate=True) is False
    bad_tau = tau_g2.copy()
    bad_tau[2 * NP] ^= np.uint64(1)
    assert zk.kzg_verify(*args, proof, validate=True) is True
    assert zk.kzg_verify(args[0], g1, g2, bad_tau, *args[4:], proof, validate=True) is False
