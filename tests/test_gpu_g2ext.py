"""GPU G2 batch conversions (<C>_G2_proj_batch_from_affine / _batch_to_affine), the device-pointer
entry, msmProj on projective G2 rows and the G2 `_variable` MSM, bit-exact against the reference's
own C (oracle/_ref).

Inputs are built with the reference library itself: distinct projective rows P0 + i H from its
scl_small / add (their Z is non-trivial), and special rows placed among them:
  (x l, y l, l) with l = (a, 0) and l = (0, b)   one term of the norm z0^2 + z1^2 vanishes
  Z = one                                       the reference's batch_from_affine of affine points
  (0 : 1 : 0) and (X : Y : 0)                    both forms of infinity"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CURVES = ["bn128", "bls12_381"]
NPS = {"bn128": 4, "bls12_381": 6}
FR_FLD = {"bn128": 1, "bls12_381": 3}
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
NBASE = 4099
# special rows of the 4099-row set
LAMBDA_A, LAMBDA_B = 5, 6          # Z = (a, 0), Z = (0, b)
Z_ONE = [7, 40, 2000]
INF_010 = [8, 64, 3000]            # (0 : 1 : 0)
INF_XY0 = [9, 33, 256, 4098]       # (X : Y : 0), X and Y non-zero
INF_ROWS = sorted(INF_010 + INF_XY0)


def progression(reflib, curve, n, k0=4242, k1=977):
    """n distinct projective G2 rows P0 + i H (P0 = k0 G, H = k1 G), kept projective"""
    NP = NPS[curve]
    gen = np.ctypeslib.as_array((ctypes.c_uint64 * (6 * NP)).in_dll(reflib, f"{curve}_G2_proj_gen_G2")).copy()
    scl = getattr(reflib, f"{curve}_G2_proj_scl_small")
    scl.argtypes = [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    add = getattr(reflib, f"{curve}_G2_proj_add")
    add.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    h = np.zeros(6 * NP, np.uint64)
    proj = np.zeros((n, 6 * NP), np.uint64)
    scl(k0, gen.ctypes.data, proj[0].ctypes.data)
    scl(k1, gen.ctypes.data, h.ctypes.data)
    base, row = proj.ctypes.data, 6 * NP * 8
    for i in range(1, n):
        add(base + (i - 1) * row, h.ctypes.data, base + i * row)
    return proj


def ref_to_affine(reference, curve, proj):
    out = np.zeros((proj.shape[0], 4 * NPS[curve]), np.uint64)
    reference.arr(curve, "G2_proj_batch_to_affine", proj.shape[0], proj, out)
    return out


def ref_from_affine(reference, curve, aff):
    out = np.zeros((aff.shape[0], 6 * NPS[curve]), np.uint64)
    reference.arr(curve, "G2_proj_batch_from_affine", aff.shape[0], aff, out)
    return out


def fp2_mul(reference, curve, a, b):
    out = np.zeros(2 * NPS[curve], np.uint64)
    reference.arr(curve, "Fp2_mont_mul", np.ascontiguousarray(a), np.ascontiguousarray(b), out)
    return out


def add_special_rows(reference, curve, proj):
    """overwrite the special positions of a progression (at least NBASE rows) in place"""
    NP = NPS[curve]
    H = NP  # words per Fp element
    aff = ref_to_affine(reference, curve, proj[:64])
    for idx, lam in ((LAMBDA_A, np.concatenate([aff[20, :H], np.zeros(H, np.uint64)])),
                     (LAMBDA_B, np.concatenate([np.zeros(H, np.uint64), aff[21, 3 * H:4 * H]]))):
        assert lam.any()
        x, y = aff[idx, :2 * NP], aff[idx, 2 * NP:]
        proj[idx] = np.concatenate([fp2_mul(reference, curve, x, lam), fp2_mul(reference, curve, y, lam), lam])
    proj[Z_ONE] = ref_from_affine(reference, curve, ref_to_affine(reference, curve, proj[Z_ONE]))
    proj[INF_010] = ref_from_affine(reference, curve, np.full((len(INF_010), 4 * NP), ONES, np.uint64))
    assert all(proj[i, :2 * NP].any() and proj[i, 2 * NP:4 * NP].any() for i in INF_XY0)
    proj[INF_XY0, 4 * NP:] = 0
    return proj


@pytest.fixture(scope="module")
def big(reference):
    """2^16 + 37 distinct projective rows per curve with the special rows among the first NBASE"""
    n = (1 << 16) + 37
    return {c: add_special_rows(reference, c, progression(reference.lib, c, n)) for c in CURVES}


@pytest.fixture(scope="module")
def rows(big):
    return {c: np.ascontiguousarray(big[c][:NBASE]) for c in CURVES}


@pytest.fixture(scope="module")
def rows_affine(reference, rows):
    """the reference's batch_to_affine of the NBASE rows (computed once, never modified)"""
    out = {c: ref_to_affine(reference, c, rows[c]) for c in CURVES}
    for c in CURVES:
        assert np.all(out[c][INF_ROWS] == ONES)
        fin = np.setdiff1d(np.arange(NBASE), INF_ROWS)
        assert not np.any(np.all(out[c][fin] == ONES, axis=1))
        out[c].setflags(write=False)
    return out


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [1, 2, 31, 33, 257, 1000, 4099])
def test_g2_batch_to_affine(gpu, rows, rows_affine, curve, n):
    got = gpu.g2_batch_to_affine(curve, rows[curve][:n])
    assert got.shape == (n, 4 * NPS[curve])
    inf = [i for i in INF_ROWS if i < n]
    assert np.all(got[inf] == ONES)
    bad = np.nonzero(np.any(got != rows_affine[curve][:n], axis=1))[0]
    assert bad.size == 0, bad[:10]


@pytest.mark.parametrize("curve", CURVES)
def test_g2_batch_to_affine_infinity_edges(gpu, reference, rows, curve):
    """infinities in the first row, in the last row, and as the whole input (n = 2, one of each form)"""
    r = rows[curve]
    both = np.ascontiguousarray(r[[INF_010[0], INF_XY0[0]]])
    got = gpu.g2_batch_to_affine(curve, both)
    assert np.all(got == ONES) and np.array_equal(got, ref_to_affine(reference, curve, both))
    for n, first, last in ((33, INF_XY0[0], INF_010[0]), (257, INF_010[0], INF_XY0[0]), (1, INF_XY0[0], None)):
        p = r[:n].copy()
        p[0] = r[first]
        if last is not None:
            p[n - 1] = r[last]
        got = gpu.g2_batch_to_affine(curve, p)
        assert np.all(got[0] == ONES) and np.all(got[n - 1] == ONES)
        assert np.array_equal(got, ref_to_affine(reference, curve, p)), n


@pytest.mark.parametrize("curve", CURVES)
def test_g2_batch_to_affine_chunked(gpu, reference, big, rows, rows_affine, curve):
    """several rows per shared inversion: 2^16 + 37 distinct rows against the reference directly, and
    2^20 + 37 (16 rows per inversion in strided chunks, ragged tail) as the tiled checked rows"""
    p = big[curve]
    got = gpu.g2_batch_to_affine(curve, p)
    bad = np.nonzero(np.any(got != ref_to_affine(reference, curve, p), axis=1))[0]
    assert bad.size == 0, bad[:10]
    n = (1 << 20) + 37
    p = np.ascontiguousarray(np.resize(rows[curve], (n, rows[curve].shape[1])))
    got = gpu.g2_batch_to_affine(curve, p)
    want = np.resize(rows_affine[curve], (n, rows_affine[curve].shape[1]))
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    assert bad.size == 0, bad[:10]


@pytest.mark.parametrize("curve", CURVES)
def test_g2_batch_from_affine(gpu, reference, rows_affine, curve):
    a = rows_affine[curve][300:1300].copy()  # no special row in this range
    assert not np.any(np.all(a == ONES, axis=1))
    a[[0, 3, 500, 999]] = ONES
    got = gpu.g2_batch_from_affine(curve, a)
    assert np.array_equal(got, ref_from_affine(reference, curve, a))
    NP = NPS[curve]
    assert not got[[0, 3, 500, 999], :2 * NP].any() and not got[[0, 3, 500, 999], 4 * NP:].any()


@pytest.mark.parametrize("curve", CURVES)
def test_g2_batch_roundtrip(gpu, rows_affine, curve):
    n = 1 << 16
    a = np.ascontiguousarray(np.resize(rows_affine[curve], (n, rows_affine[curve].shape[1])))
    assert np.all(a[INF_ROWS] == ONES) and np.all(a[NBASE + INF_ROWS[0]] == ONES)
    back = gpu.g2_batch_to_affine(curve, gpu.g2_batch_from_affine(curve, a))
    assert np.array_equal(back, a)


@pytest.mark.parametrize("curve", CURVES)
def test_g2_batch_to_affine_device(gpu, rows, rows_affine, curve):
    lib, cid = gpu.load(), gpu.CURVE_ID[curve]
    want = gpu.g2_batch_to_affine(curve, rows[curve])
    assert np.array_equal(want, rows_affine[curve])
    d_src = gpu.DeviceBuffer(rows[curve])
    fill = np.full_like(want, np.uint64(0x1234567890ABCDEF))
    d_tgt = gpu.DeviceBuffer(fill)
    try:
        lib.zkg_g2_batch_to_affine_device(cid, 0, d_src.ptr, d_tgt.ptr)  # n = 0: nothing is written
        assert np.array_equal(d_tgt.to_host(fill), fill)
        lib.zkg_g2_batch_to_affine_device(cid, NBASE, d_src.ptr, d_tgt.ptr)
        assert np.array_equal(d_tgt.to_host(fill), want)
    finally:
        d_src.free()
        d_tgt.free()
    assert gpu.last_error() is None


def ref_g2_msm(reference, curve, sc, aff, mont, affine):
    out = np.zeros((4 if affine else 6) * NPS[curve], np.uint64)
    name = f"G2_proj_MSM_{'mont' if mont else 'std'}_coeff_{'affine' if affine else 'proj'}_out"
    reference.arr(curve, name, sc.shape[0], sc, aff, out, sc.shape[1])
    return out


def ref_normalize(reference, curve, proj):
    out = np.zeros_like(proj)
    reference.arr(curve, "G2_proj_normalize", proj, out)
    return out


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", [1, 300, 2048])
def test_g2_msm_proj(gpu, oracle, reference, rows, rows_affine, curve, n):
    """msmProj cs gs = msm cs (batchToAffine gs): projective rows with both infinity forms (n >= 300)
    and zero scalars, against the reference's MSM on the reference's batch_to_affine of the rows"""
    p = np.ascontiguousarray(rows[curve][:n])
    aff = np.ascontiguousarray(rows_affine[curve][:n])
    sc = gpu.gen_fr(curve, 900 + n, n)
    if n > 1:
        sc[[2, n // 2]] = 0
    want = ref_g2_msm(reference, curve, sc, aff, True, True)
    assert np.array_equal(gpu.g2_msm_proj(curve, sc, p, affine=True), want)
    std = oracle.to_std(FR_FLD[curve], sc)
    assert np.array_equal(gpu.g2_msm_proj(curve, std, p, std=True, affine=True),
                          ref_g2_msm(reference, curve, std, aff, False, True))
    wantp = ref_normalize(reference, curve, ref_g2_msm(reference, curve, sc, aff, True, False))
    assert np.array_equal(gpu.g2_msm_proj(curve, sc, p, affine=False), wantp)
    assert np.array_equal(gpu.g2_msm_proj(curve, sc, p), wantp)


@pytest.mark.parametrize("curve", CURVES)
def test_g2_msm_proj_all_infinity(gpu, rows, curve):
    p = np.ascontiguousarray(rows[curve][[INF_010[0], INF_XY0[0], INF_XY0[1]]])
    sc = gpu.gen_fr(curve, 77, 3)
    NP = NPS[curve]
    assert np.all(gpu.g2_msm_proj(curve, sc, p, affine=True) == ONES)
    got = gpu.g2_msm_proj(curve, sc, p)
    assert not got[:2 * NP].any() and got[2 * NP:4 * NP].any() and not got[4 * NP:].any()  # (0 : 1 : 0)


# The reference's `_variable` allocates 2^w - 1 buckets of 3 Fp2 elements and adds every one of them
# twice per window: at w = 16 that is 2.1e6 G2 additions (8.6 s on BN128, 12.2 s on BLS12-381 on one
# host core), at w = 25 a 9.7 GB table and 7e8 additions.  Its normalised result is the group element
# sum k_i P_i in canonical form whatever the window, so above this cap the reference is run at the cap.
REF_WINDOW_CAP = 12


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("window", [1, 4, 7, 16, 25])
def test_g2_msm_variable(gpu, oracle, reference, rows_affine, curve, window):
    """the explicit-window entry (clamped into 4..24 here, 1..64 in the reference) against the
    reference's own `_variable` at that window (at REF_WINDOW_CAP beyond it), both normalised by
    the reference"""
    n = 300
    aff = np.ascontiguousarray(rows_affine[curve][:n])
    sc = oracle.to_std(FR_FLD[curve], gpu.gen_fr(curve, 41, n))
    want = np.zeros(6 * NPS[curve], np.uint64)
    reference.arr(curve, "G2_proj_MSM_std_coeff_proj_out_variable", n, sc, aff, want, sc.shape[1],
                  min(window, REF_WINDOW_CAP))
    got = gpu.g2_msm_variable(curve, sc, aff, window)
    assert np.array_equal(ref_normalize(reference, curve, got), ref_normalize(reference, curve, want))
