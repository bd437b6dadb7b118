"""The "all openings" derivation and the Python wrappers' argument checks, without a GPU: the pure-Python model
of tests/fk20_model.py (scalars for points) against the directly computed quotients, the layout index maps that
zkalgebra shares with the kernels (zk_fk20.hpp), and every refusal that is raised before a device is touched."""
import random

import numpy as np
import pytest

import fk20_model as fm

CURVES = ("bn128", "bls12_381")
SHAPES = [(m, c) for m in range(1, 6) for c in range(0, m)]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m,c", SHAPES)
def test_model_equals_direct_quotients(zk, curve, m, c):
    R = fm.FR[curve]
    rng = random.Random(0xF20 + 64 * m + c)
    n, l = 1 << m, 1 << c
    g2n, tau = fm.root_of_unity(R, m + 1), rng.randrange(2, R)
    for npoly in sorted({n, n - l + 1, max(1, n // 2 - 1), 1, 0}):
        f = [rng.randrange(R) for _ in range(npoly)]
        got, y = fm.model_proofs(f, m, c, g2n, tau, R, zk.fk20_coeff_index, zk.fk20_srs_index)
        assert got == fm.direct_proofs(f, m, c, g2n, tau, R), (npoly, m, c)
        assert y[n // l - 1] == 0, "y_(r-1) = O by construction"


@pytest.mark.parametrize("curve", CURVES)
def test_single_point_proof_is_the_opening(curve):
    """l = 1: proof k is (f(tau) - f(omega^k)) / (tau - omega^k)"""
    R, m = fm.FR[curve], 4
    rng = random.Random(0xF21)
    g2n, tau = fm.root_of_unity(R, m + 1), rng.randrange(2, R)
    f = [rng.randrange(R) for _ in range(1 << m)]
    ev = lambda x: sum(a * pow(x, i, R) for i, a in enumerate(f)) % R
    omega = g2n * g2n % R
    for k, pi in enumerate(fm.direct_proofs(f, m, 0, g2n, tau, R)):
        z = pow(omega, k, R)
        assert pi == (ev(tau) - ev(z)) * pow(tau - z, -1, R) % R


@pytest.mark.parametrize("r", (2, 4, 8, 64))
def test_index_maps(zk, r):
    cs = [zk.fk20_coeff_index(r, p) for p in range(2 * r)]
    assert cs[0] == r - 1 and cs[1:r + 2] == [-1] * (r + 1) and cs[r + 2:] == list(range(1, r - 1))
    assert 0 not in cs, "F_0 belongs to the remainder and is never read"
    xs = [zk.fk20_srs_index(r, p) for p in range(2 * r)]
    assert xs[:r - 1] == list(range(r - 2, -1, -1)) and xs[r - 1:] == [-1] * (r + 1)
    # the circulant: column entry (t - u) mod 2r meets x_u with F index u' + t + 1, u' = the S index of x_u
    for t in range(r):
        for u in range(r - 1):
            v = cs[(t - u) % (2 * r)]
            assert v == (xs[u] + t + 1 if xs[u] + t + 1 <= r - 1 and u >= t else -1), (t, u)


def fake_setup(zk, curve, log_size):
    return zk.KZGSetup(zk.get_fft_subgroup(curve, log_size), None, None, None)


@pytest.mark.parametrize("curve", CURVES)
def test_open_all_refuses_before_the_gpu(zk, curve):
    s = fake_setup(zk, curve, 4)
    poly = np.zeros((16, 4), dtype=np.uint64)
    with pytest.raises(ValueError, match="larger than the KZG setup"):
        zk.kzg_open_all(s, poly, log_n=5)
    with pytest.raises(ValueError, match="longer than the domain"):
        zk.kzg_open_all(s, poly, log_n=3)
    with pytest.raises(ValueError, match="longer than the domain"):
        zk.kzg_open_all(s, np.zeros((17, 4), dtype=np.uint64))
    with pytest.raises(ValueError, match="at least two points"):
        zk.kzg_open_all(s, poly[:1], log_n=0)
    for c in (-1, 4, 5):
        with pytest.raises(ValueError, match="at least two cosets"):
            zk.kzg_open_all(s, poly, coset_log=c)
    with pytest.raises(ValueError, match="at least two cosets"):
        zk.kzg_open_all(s, poly[:4], log_n=2, coset_log=2)
    with pytest.raises(TypeError):
        zk.kzg_open_all(s, np.zeros((16, 3), dtype=np.uint64))


@pytest.mark.parametrize("curve", CURVES)
def test_rows_sum_and_verify_refuse_before_the_gpu(zk, curve):
    NP = zk.NLIMBS_P[curve]
    k = np.zeros((3, 5, 4), dtype=np.uint64)
    with pytest.raises(ValueError, match="incompatible array dimensions"):
        zk.scalar_mul_rows_sum(curve, k, np.zeros((3, 4, 2 * NP), dtype=np.uint64))
    with pytest.raises(ValueError, match="incompatible array dimensions"):
        zk.scalar_mul_rows_sum(curve, k, np.zeros((3, 5, 3 * NP), dtype=np.uint64))
    with pytest.raises(TypeError):
        zk.scalar_mul_rows_sum(curve, k[0], np.zeros((5, 2 * NP), dtype=np.uint64))
    g1 = np.zeros((4, 2 * NP), dtype=np.uint64)
    g2 = np.zeros(4 * NP, dtype=np.uint64)
    pt = np.zeros(3 * NP, dtype=np.uint64)
    one = np.zeros(4, dtype=np.uint64)
    with pytest.raises(ValueError, match="power of two"):
        zk.kzg_verify_coset(curve, g1, g2, g2, pt, one, np.zeros((3, 4), dtype=np.uint64), pt)
    with pytest.raises(ValueError, match="i < l"):
        zk.kzg_verify_coset(curve, g1[:2], g2, g2, pt, one, np.zeros((4, 4), dtype=np.uint64), pt)
    with pytest.raises(ValueError, match="incompatible array dimensions"):
        zk.kzg_verify_coset(curve, g1, g2, g2, pt[:-1], one, np.zeros((4, 4), dtype=np.uint64), pt)


def test_library_refuses_bad_shapes_without_a_device(zk):
    """the C entries check their arguments before any device call: refusals work on a host without a GPU"""
    lib = zk.load()
    zk.last_error()  # drain anything an earlier test left
    bad = [(0, 0, 0), (0, 6, 6), (0, 6, -1), (0, 28, 0), (0, 29, 3), (1, 28, 1), (2, 6, 0)]
    for curve, log_n, log_l in bad:
        assert lib.zkg_kzg_open_all_table_bytes(curve, log_n, log_l) == 0, (curve, log_n, log_l)
        assert "kzg_open_all" in zk.last_error()
        assert lib.zkg_kzg_open_all_device(curve, log_n, log_l, 0, None, 8, 0, 8) != 0
        assert "kzg_open_all" in zk.last_error()
    for curve, NP in ((0, 4), (1, 6)):
        assert lib.zkg_kzg_open_all_table_bytes(curve, 6, 2) == 2 * 64 * 2 * NP * 8
    assert zk.last_error() is None
    assert lib.zkg_kzg_open_all_device(0, 6, 0, 65, 8, 8, 0, 8) != 0 and "longer than the domain" in zk.last_error()
    assert lib.zkg_kzg_open_all_device(0, 6, 0, -1, 8, 8, 0, 8) != 0 and "longer than the domain" in zk.last_error()
    assert lib.zkg_kzg_open_all_device(0, 6, 0, 4, None, 8, 0, 8) != 0 and "null" in zk.last_error()
    assert lib.zkg_kzg_open_all_device(0, 6, 0, 4, 8, None, 0, 8) != 0 and "null" in zk.last_error()
    assert lib.zkg_kzg_open_all_table_device(0, 6, 0, None, 8) != 0 and "null" in zk.last_error()
    assert lib.zkg_g1_scl_rows_sum_device(0, -1, 1, 8, 1, 8, 0, 8) != 0 and "negative" in zk.last_error()
    assert lib.zkg_g1_scl_rows_sum_device(0, 1, 1, None, 1, 8, 0, 8) != 0 and "null" in zk.last_error()
    assert lib.zkg_g1_scl_rows_sum_device(0, 1 << 20, 1 << 12, 8, 1, 8, 0, 8) != 0 and "31 bits" in zk.last_error()
    assert lib.zkg_g1_scl_rows_sum_device(3, 1, 1, 8, 1, 8, 0, 8) != 0 and "unknown curve" in zk.last_error()
    assert lib.zkg_g1_scl_rows_sum_device(0, 0, 5, None, 1, None, 0, None) == 0 and zk.last_error() is None
