"""Row-wise sums of scalar multiples and every KZG opening of a domain at once (zk_fk20.hip), bit for bit
against what the library already had: the fold of scalar_mul_rows with g1_add, kzg_open_many over the roots of
unity, and kzg_commit of the quotients of div_by_vanishing.  Group elements are compared as affine rows."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ("bn128", "bls12_381")
LOG = 6
FF = np.uint64(0xFFFFFFFFFFFFFFFF)


def words(v, n):
    return np.array([(v >> (64 * i)) & (2 ** 64 - 1) for i in range(n)], dtype=np.uint64)


def neg_affine(zk, curve, row):
    """-(x, y): p - y on the Montgomery words"""
    NP = zk.NLIMBS_P[curve]
    out = row.copy()
    y = sum(int(row[NP + j]) << (64 * j) for j in range(NP))
    out[NP:] = words((zk.FIELD_P[curve] - y) % zk.FIELD_P[curve], NP)
    return out


def fold(zk, curve, scalars, bases, std):
    """the reference: one scalar_mul_rows over every product, then g1_add per row, as affine rows"""
    terms, rows = scalars.shape[:2]
    NP = zk.NLIMBS_P[curve]
    prod = zk.scalar_mul_rows(curve, scalars.reshape(-1, 4), bases.reshape(-1, 2 * NP), std=std).reshape(terms, rows, -1)
    out = []
    for i in range(rows):
        acc = prod[0, i]
        for j in range(1, terms):
            acc = zk.g1_add(curve, acc, prod[j, i])
        out.append(zk.g1_to_affine(curve, acc))
    return np.stack(out)


def planted(zk, curve, rows, terms, std, seed):
    """random rows with the special ones planted where the shape has room for them"""
    NP = zk.NLIMBS_P[curve]
    k = zk.gen_fr(curve, seed, terms * rows).reshape(terms, rows, 4).copy()
    P = zk.gen_points(curve, seed + 1, terms * rows).reshape(terms, rows, 2 * NP).copy()
    # row 0: every term the same base and scalar -- the reduction doubles at every level
    k[:, 0], P[:, 0] = k[0, 0], P[0, 0]
    if rows > 1:  # row 1: P with -P under one scalar, an odd term out multiplied by zero -- the sum is infinity
        for j in range(0, terms - 1, 2):
            k[j + 1, 1], P[j + 1, 1] = k[j, 1], neg_affine(zk, curve, P[j, 1])
        if terms % 2:
            k[terms - 1, 1] = 0
    if rows > 2:  # row 2: zero scalars and infinite bases between ordinary terms
        k[0::3, 2] = 0
        P[1::3, 2] = FF
    if rows > 3 and std:  # row 3: the largest raw scalar
        k[:, 3] = FF
    if rows > 4:  # row 4: nothing but infinity
        P[:, 4] = FF
    return k, P


@pytest.mark.parametrize("terms", (1, 2, 3, 64, 300))
@pytest.mark.parametrize("rows", (1, 5, 64))
@pytest.mark.parametrize("curve", CURVES)
def test_rows_sum_equals_fold(gpu, curve, rows, terms):
    NP = gpu.NLIMBS_P[curve]
    for std in (False, True):
        k, P = planted(gpu, curve, rows, terms, std, 0xF200 + 16 * rows + terms)
        if std and rows == 1:
            k[terms // 2, 0] = FF  # 2^256 - 1 among equal terms
        want = fold(gpu, curve, k, P, std)
        got = gpu.scalar_mul_rows_sum(curve, k, P, std=std, affine=True)
        assert np.array_equal(got, want), (std, np.nonzero((got != want).any(axis=1))[0][:8])
        if rows > 1:
            assert (want[1] == FF).all(), "P with -P sums to infinity"
        if rows > 4:
            assert (want[4] == FF).all()
        proj = gpu.scalar_mul_rows_sum(curve, k, P, std=std)
        assert proj.shape == (rows, 3 * NP)
        assert np.array_equal(gpu.batch_to_affine(curve, proj), want)
        if rows > 1:  # the normalised infinity row (0 : 1 : 0)
            inf = np.zeros(3 * NP, dtype=np.uint64)
            inf[NP:2 * NP] = gpu.fp12_one(curve)[:NP]
            assert np.array_equal(proj[1], inf)


@pytest.mark.parametrize("curve", CURVES)
def test_rows_sum_host_and_device_agree_and_refusals(gpu, curve):
    NP = gpu.NLIMBS_P[curve]
    rows, terms = 5, 3
    k, P = planted(gpu, curve, rows, terms, False, 0xF2A0)
    want = gpu.scalar_mul_rows_sum(curve, k, P, affine=True)
    d_k, d_P = gpu.DeviceBuffer(k), gpu.DeviceBuffer(P)
    d_t = gpu.DeviceBuffer.empty(want.nbytes)
    gpu.set_error_mode(True)
    try:
        gpu.last_error()
        assert gpu.scalar_mul_rows_sum_device(curve, rows, terms, d_k, d_P, d_t, affine=True) == 0
        assert np.array_equal(d_t.to_host(want), want)
        assert np.array_equal(d_k.to_host(k), k) and np.array_equal(d_P.to_host(P), P)  # inputs are not written
        assert gpu.scalar_mul_rows_sum_device(curve, rows, terms, d_k, d_P, d_P, affine=True) != 0
        assert "overlaps" in gpu.last_error()
        assert gpu.scalar_mul_rows_sum_device(curve, rows, terms, d_k, None, d_t) != 0
        assert "null" in gpu.last_error()
        assert gpu.scalar_mul_rows_sum_device(curve, -1, terms, d_k, d_P, d_t) != 0
        assert "negative" in gpu.last_error()
        assert np.array_equal(d_P.to_host(P), P)
        assert gpu.scalar_mul_rows_sum_device(curve, rows, terms, d_k, d_P, d_t, affine=True) == 0  # the next call is clean
        assert gpu.last_error() is None and np.array_equal(d_t.to_host(want), want)
        # no terms: the empty sum
        assert gpu.scalar_mul_rows_sum_device(curve, rows, 0, None, None, d_t, affine=True) == 0
        assert (d_t.to_host(want) == FF).all()
    finally:
        gpu.set_error_mode(False)
        gpu.last_error()
        for b in (d_k, d_P, d_t):
            b.free()
    assert NP in (4, 6)


# ---------------------------------------------------------------------------- all openings

def golden_generators(curve):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"pairing_{curve}.npz"))
    gen = int(np.nonzero((g["factors"][:, 0] == 1) & (g["factors"][:, 4] == 1) & (g["family"] >= 0))[0][0])
    return g["P"][gen], g["Q"][gen]


def make_setup(gpu, curve, seed=0xF2B0, g2_powers=5):
    g1, g2 = golden_generators(curve)
    tau = gpu.gen_fr(curve, seed, 1)[0]
    return gpu.kzg_setup(curve, tau, LOG, g1, g2, g2_powers=g2_powers), g1, g2


@pytest.fixture(scope="module")
def setups(gpu):
    out = {curve: make_setup(gpu, curve) for curve in CURVES}
    yield out
    for s, *_ in out.values():
        s.free()


def roots(gpu, curve, m):
    """omega^k, k < 2^m, as Montgomery rows"""
    one = np.array(gpu._fr_mont(curve, 1))
    return gpu.arr_powers(curve, one, gpu.get_fft_subgroup(curve, m).gen_array(), 1 << m)


def infinity_rows(gpu, curve, rows):
    NP = gpu.NLIMBS_P[curve]
    inf = np.zeros((rows, 3 * NP), dtype=np.uint64)
    inf[:, NP:2 * NP] = gpu.fp12_one(curve)[:NP]
    return inf


@pytest.mark.parametrize("m", (1, 2, 3, 6))
@pytest.mark.parametrize("curve", CURVES)
def test_single_points_equal_open_many(gpu, setups, curve, m):
    s = setups[curve][0]
    n = 1 << m
    zs = roots(gpu, curve, m)
    for npoly in sorted({n, max(1, n - 3)}):  # the whole domain, and a polynomial shorter than it
        poly = gpu.gen_fr(curve, 0xF2C0 + 8 * m + npoly, npoly)
        want_vals, want = gpu.kzg_open_many(s, poly, zs)
        vals, proofs = gpu.kzg_open_all(s, poly, log_n=m)
        assert vals.shape == (n, 4) and np.array_equal(vals, want_vals)
        assert np.array_equal(gpu.batch_to_affine(curve, proofs), gpu.batch_to_affine(curve, want))
        assert np.array_equal(proofs, want)  # both are normalised rows
        _, aff = gpu.kzg_open_all(s, poly, log_n=m, affine=True)
        assert np.array_equal(aff, gpu.batch_to_affine(curve, want))
    if m == LOG:  # log_n defaults to the setup's
        assert np.array_equal(gpu.kzg_open_all(s, poly)[1], proofs)


def coset_case(gpu, s, curve, m, c, poly):
    """kzg_open_all at l = 2^c against kzg_commit of the quotient by x^l - psi^k, every k"""
    n, l = 1 << m, 1 << c
    psis = roots(gpu, curve, m - c)
    vals, proofs = gpu.kzg_open_all(s, poly, log_n=m, coset_log=c, affine=True)
    assert proofs.shape == (n // l, 2 * gpu.NLIMBS_P[curve])
    ext = np.zeros((n, 4), dtype=np.uint64)
    ext[:poly.shape[0]] = poly
    assert np.array_equal(vals, gpu.forward_ntt(gpu.get_fft_subgroup(curve, m), ext))
    for k in range(n // l):
        quot, _ = gpu.div_by_vanishing(curve, ext, l, psis[k])
        assert np.array_equal(proofs[k], gpu.kzg_commit(s, quot, affine=True)), (c, k)
    return vals, proofs


@pytest.mark.parametrize("c", (1, 2, LOG - 1))
@pytest.mark.parametrize("curve", CURVES)
def test_cosets_equal_commitments_to_quotients(gpu, setups, curve, c):
    s = setups[curve][0]
    coset_case(gpu, s, curve, LOG, c, gpu.gen_fr(curve, 0xF2D0 + c, 1 << LOG))


@pytest.mark.parametrize("curve", CURVES)
def test_partly_zero_top_row_and_short_domain(gpu, setups, curve):
    s = setups[curve][0]
    n, c = 1 << LOG, 2
    coset_case(gpu, s, curve, LOG, c, gpu.gen_fr(curve, 0xF2E0, n - (1 << c) + 1))  # npoly = n - l + 1
    coset_case(gpu, s, curve, 4, 3, gpu.gen_fr(curve, 0xF2E1, 11))                  # n below the setup, r = 2


@pytest.mark.parametrize("curve", CURVES)
def test_constant_and_zero_polynomials(gpu, setups, curve):
    s = setups[curve][0]
    const = gpu.gen_fr(curve, 0xF2F0, 1)
    for c in (0, 3):
        r = (1 << LOG) >> c
        vals, proofs = gpu.kzg_open_all(s, const, coset_log=c)
        assert np.array_equal(proofs, infinity_rows(gpu, curve, r))
        assert np.array_equal(vals, np.tile(const, (1 << LOG, 1)))
        for zero in (np.zeros((0, 4), dtype=np.uint64), np.zeros((1 << LOG, 4), dtype=np.uint64)):
            vals, proofs = gpu.kzg_open_all(s, zero, coset_log=c)
            assert not vals.any() and np.array_equal(proofs, infinity_rows(gpu, curve, r))
        _, aff = gpu.kzg_open_all(s, const, coset_log=c, affine=True)
        assert (aff == FF).all()


@pytest.mark.parametrize("curve", CURVES)
def test_table_is_cached_and_freed(gpu, setups, curve):
    s = setups[curve][0]
    poly = gpu.gen_fr(curve, 0xF300, 1 << LOG)
    first = gpu.kzg_open_all(s, poly, coset_log=1)[1]
    table = s.open_all_table(LOG, 1)
    assert np.array_equal(gpu.kzg_open_all(s, poly, coset_log=1)[1], first)
    assert s.open_all_table(LOG, 1) is table and (LOG, 1) in s._open_all
    fresh, *_ = make_setup(gpu, curve, seed=0xF301, g2_powers=0)
    try:
        a = gpu.kzg_open_all(fresh, poly[:8], log_n=3, coset_log=1)[1]
        fresh.free()
        assert fresh._open_all is None
    finally:
        if fresh.tau_g1s.ptr:
            fresh.free()
    again, *_ = make_setup(gpu, curve, seed=0xF301, g2_powers=0)  # a fresh setup after free() still works
    try:
        assert np.array_equal(gpu.kzg_open_all(again, poly[:8], log_n=3, coset_log=1)[1], a)
    finally:
        again.free()
    assert np.array_equal(gpu.kzg_open_all(s, poly, coset_log=1)[1], first)


def g2_affine(gpu, curve, row):
    NP = gpu.NLIMBS_P[curve]
    row = np.asarray(row).reshape(-1)
    return gpu.g2_batch_to_affine(curve, row.reshape(1, -1))[0] if row.shape[0] == 6 * NP else row


@pytest.mark.parametrize("curve", CURVES)
def test_proofs_verify(gpu, setups, curve):
    s, g1, g2 = setups[curve]
    NP = gpu.NLIMBS_P[curve]
    n = 1 << LOG
    poly = gpu.gen_fr(curve, 0xF310, n)
    commitment = gpu.kzg_commit(s, poly)
    omega = roots(gpu, curve, LOG)
    # l = 1 under the existing verifier
    vals, proofs = gpu.kzg_open_all(s, poly)
    tau_g2 = g2_affine(gpu, curve, s.g2_tau_g2[1])
    for k in (0, 1, n - 1):
        assert gpu.kzg_verify(curve, g1, g2, tau_g2, commitment, omega[k], vals[k], proofs[k])
    assert not gpu.kzg_verify(curve, g1, g2, tau_g2, commitment, omega[2], vals[2], proofs[3])
    # l = 4 under the coset verifier
    l, r = 4, n // 4
    vals4, proofs4 = gpu.kzg_open_all(s, poly, coset_log=2)
    assert np.array_equal(vals4, vals)
    tau_g2s = s.tau_g2s.to_host(np.empty((5, 6 * NP), dtype=np.uint64))
    tau_l_g2 = g2_affine(gpu, curve, tau_g2s[l])
    srs = gpu.batch_to_affine(curve, s.tau_g1s.to_host(np.empty((n, 3 * NP), dtype=np.uint64)))[:l]
    assert np.array_equal(srs[0], np.asarray(g1).reshape(-1))
    for k in (0, 5, r - 1):
        assert gpu.kzg_verify_coset(curve, srs, g2, tau_l_g2, commitment, omega[k], vals[k::r], proofs4[k]), k
    assert not gpu.kzg_verify_coset(curve, srs, g2, tau_l_g2, commitment, omega[6], vals[6::r], proofs4[5])
    assert not gpu.kzg_verify_coset(curve, srs, g2, tau_l_g2, commitment, omega[5], vals[6::r], proofs4[5])


@pytest.mark.parametrize("curve", CURVES)
def test_refused_arguments_leave_the_next_call_clean(gpu, setups, curve):
    s = setups[curve][0]
    cid, NP, n = gpu.CURVE_ID[curve], gpu.NLIMBS_P[curve], 1 << LOG
    lib = gpu.load()
    poly = gpu.gen_fr(curve, 0xF320, n)
    want = gpu.kzg_open_all(s, poly)[1]
    table, srs = s.open_all_table(LOG, 0), s.affine_rows("tau_g1s")
    d_p, d_out = gpu.DeviceBuffer(poly), gpu.DeviceBuffer.empty(want.nbytes)
    gpu.set_error_mode(True)
    try:
        gpu.last_error()
        open_all = lib.zkg_kzg_open_all_device
        assert open_all(cid, LOG, LOG, n, d_p.ptr, table.ptr, 0, d_out.ptr) != 0 and "r = n / l" in gpu.last_error()
        assert open_all(cid, LOG, 0, n + 1, d_p.ptr, table.ptr, 0, d_out.ptr) != 0 and "longer" in gpu.last_error()
        assert open_all(cid, LOG, 0, -1, d_p.ptr, table.ptr, 0, d_out.ptr) != 0 and "longer" in gpu.last_error()
        assert open_all(cid, LOG, 0, n, None, table.ptr, 0, d_out.ptr) != 0 and "null" in gpu.last_error()
        assert open_all(cid, LOG, 0, n, d_p.ptr, None, 0, d_out.ptr) != 0 and "null" in gpu.last_error()
        assert open_all(cid, LOG, 0, n, d_p.ptr, table.ptr, 0, None) != 0 and "null" in gpu.last_error()
        assert open_all(cid, LOG, 0, n, d_p.ptr, table.ptr, 0, d_p.ptr) != 0 and "overlapping" in gpu.last_error()
        assert open_all(cid, LOG, 0, n, d_p.ptr, table.ptr, 0, table.ptr + 64) != 0 and "overlapping" in gpu.last_error()
        assert open_all(cid, 29 if curve == "bn128" else 28, 0, n, d_p.ptr, table.ptr, 0, d_out.ptr) != 0
        assert "kzg_open_all" in gpu.last_error()
        assert open_all(cid, 28, 0, n, d_p.ptr, table.ptr, 0, d_out.ptr) != 0 and "2r domain" in gpu.last_error()
        build = lib.zkg_kzg_open_all_table_device
        assert build(cid, LOG, 0, srs.ptr, srs.ptr) != 0 and "overlaps" in gpu.last_error()
        assert build(cid, LOG, 0, None, table.ptr) != 0 and "null" in gpu.last_error()
        assert build(cid, LOG, -1, srs.ptr, table.ptr) != 0 and "r = n / l" in gpu.last_error()
        assert lib.zkg_kzg_open_all_table_bytes(cid, LOG, LOG) == 0 and gpu.last_error() is not None
        assert lib.zkg_kzg_open_all_table_bytes(cid, LOG, 3) == 2 * n * 2 * NP * 8
        assert np.array_equal(d_p.to_host(poly), poly)
        assert open_all(cid, LOG, 0, n, d_p.ptr, table.ptr, 0, d_out.ptr) == 0 and gpu.last_error() is None
        assert np.array_equal(d_out.to_host(want), want)
    finally:
        gpu.set_error_mode(False)
        gpu.last_error()
        d_p.free()
        d_out.free()
    with pytest.raises(ValueError, match="larger than the KZG setup"):
        gpu.kzg_open_all(s, poly, log_n=LOG + 1)
    with pytest.raises(ValueError, match="longer than the domain"):
        gpu.kzg_open_all(s, poly, log_n=LOG - 1)
