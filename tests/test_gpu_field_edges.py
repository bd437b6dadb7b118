"""Edge values through the field, inversion and digit-recoding kernels.

The rest of the GPU suite feeds these kernels uniformly random operands (outside the NTT patterns
and the bit-job path).  Here every operand, or every RESULT, is one of the values where a kernel
can be wrong without a random draw ever noticing (tests/field_edges.py): 0, 1, q - 1, the
Montgomery constants, powers of two at the limb widths, the reduction boundaries k q / K of the
radix conversion R -> R' = K R and their pre-images, whole chunks of infinities, signed digits at
+-2^(c-1).  Every expected value is computed without the GPU, by Python big integers
(tests/test_field_edges_cpu.py checks those models against the oracle and the reference C first) or
by the oracle, and every comparison is np.array_equal.  Where oracle/_ref is built the reference's
own C is compared as well."""
import numpy as np
import pytest

import field_edges as fe

pytestmark = pytest.mark.gpu
CURVES = ["bn128", "bls12_381"]


def _ref_or_none(request):
    from oracle.oracle import Reference
    return request.getfixturevalue("reference") if Reference.available() else None


# ---------------------------------------------------------------------------- (a) Fr ops, operands on the edges
@pytest.mark.parametrize("curve", CURVES)
def test_fr_ops_edge_cross_product(gpu, curve):
    """every call of test_gpu_arr.test_elementwise with (a[i], b[i]) over E x E' (23 352 / 23 436
    rows: E the edge set of Fr, E' its part without the k r / 32 values), c a rotation of a and
    kA, kB over {0, R mod r, r - 1, one random value}"""
    a, b, c, ks = fe.fr_cross(curve)
    A, B, C = fe.to_limbs(a, 4), fe.to_limbs(b, 4), fe.to_limbs(c, 4)
    K = [fe.to_row(k, 4) for k in ks]
    want = fe.fr_cross_expected(curve)
    n = A.shape[0]
    assert n > 20000
    bad = []

    def check(name, got):
        if not np.array_equal(got, want[name]):
            rows = np.nonzero((np.atleast_2d(got) != np.atleast_2d(want[name])).any(axis=1))[0]
            bad.append((name, [(hex(a[i]), hex(b[i])) for i in rows[:3]] if len(want[name]) == n else None))
    check("neg", gpu.arr_neg(curve, A))
    check("add", gpu.arr_add(curve, A, B))
    check("sub", gpu.arr_sub(curve, A, B))
    check("sqr", gpu.arr_sqr(curve, A))
    check("mul", gpu.arr_mul(curve, A, B))
    check("mul_add", gpu.arr_mul_add(curve, A, B, C))
    check("mul_sub", gpu.arr_mul_sub(curve, A, B, C))
    check("to_std", gpu.arr_to_std(curve, A))
    check("from_std", gpu.arr_from_std(curve, A))
    check("dot", gpu.arr_dot_prod(curve, A, B).reshape(1, 4))
    for i, k in enumerate(K):
        check(f"scale_{i}", gpu.arr_scale(curve, k, A))
        check(f"Ax_plus_y_{i}", gpu.arr_lin_comb1(curve, (k, A), B))
        check(f"Ax_plus_By_{i}", gpu.arr_lin_comb2(curve, (k, A), (K[(i + 1) % 4], B)))
    assert not bad, bad
    assert np.array_equal(gpu.arr_from_std(curve, gpu.arr_to_std(curve, A)), A)
    assert np.array_equal(gpu.arr_append(curve, A, B), np.concatenate([A, B]))


@pytest.mark.parametrize("curve", CURVES)
def test_fr_powers_edge_bases(gpu, curve):
    """arr_powers with bases 0, the Montgomery one, r - 1 and an element of order 2^5, at
    n in {1, 64, 65, 1000}"""
    M = fe.fr_model(curve)
    for ka, kb in fe.powers_cases(curve):
        for n in fe.POWERS_N:
            got = gpu.arr_powers(curve, fe.to_row(ka, 4), fe.to_row(kb, 4), n)
            assert np.array_equal(got, fe.to_limbs(M.powers(ka, kb, n), 4)), (hex(ka), hex(kb), n)


# ---------------------------------------------------------------------------- (b) Fr ops, results on the edges
@pytest.mark.parametrize("curve", CURVES)
def test_fr_ops_edge_results(gpu, curve):
    """for each edge value t the inputs are solved so that the TRUE result of mul, add, sub, mul_add
    and sqr is exactly t: the store side (fe_div32_small, fe_canon) at 0, r - 1, k r / 32, ...
    sqr reaches the t with t R a square mod r: 176 of 278 (BN254) and 189 of 279 (BLS12-381)
    edge values (tests/test_field_edges_cpu.py asserts these counts)."""
    T = fe.fr_targets(curve)
    calls = {"mul": gpu.arr_mul, "add": gpu.arr_add, "sub": gpu.arr_sub, "mul_add": gpu.arr_mul_add, "sqr": gpu.arr_sqr}
    assert 3 * len(T["sqr"][1]) >= len(fe.field_edges(curve + "_fr"))
    for op, (*ins, t) in T.items():
        got = calls[op](curve, *[fe.to_limbs(v, 4) for v in ins])
        want = fe.to_limbs(t, 4)
        rows = np.nonzero((got != want).any(axis=1))[0]
        assert not len(rows), (op, [hex(t[i]) for i in rows[:5]])


# ---------------------------------------------------------------------------- (c) Fr inversion on the edges
@pytest.mark.parametrize("curve", CURVES)
def test_fr_inversion_edges(gpu, curve):
    """arr_inv and arr_div over E \\ {0} at lengths 1, 33 and all of it against R^2 / a, then the same
    vector with one 0 first, in the middle and last: every output is 0 (Fr_mont.c:258-285)"""
    M = fe.fr_model(curve)
    for name, x, y in fe.inv_vectors(curve):
        X, Y = fe.to_limbs(x, 4), fe.to_limbs(y, 4)
        wi, wd = M.inv(y), M.div(x, y)
        if name.startswith("zero"):
            assert not any(wi) and not any(wd)
        got = gpu.arr_inv(curve, Y)
        rows = np.nonzero((got != fe.to_limbs(wi, 4)).any(axis=1))[0]
        assert not len(rows), (name, [hex(y[i]) for i in rows[:5]])
        assert np.array_equal(gpu.arr_div(curve, X, Y), fe.to_limbs(wd, 4)), name


# ---------------------------------------------------------------------------- (d) Fp through batch_to_affine
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("coords", ["proj", "jac"])
def test_fp_edges_through_batch_to_affine(gpu, request, curve, coords):
    """Rows (X, Y, Z) with Z over every non-zero Fp edge value and X, Y over rotations of the same
    list.  The rows are NOT curve points, and need not be: <C>_G1_{proj,jac}_batch_to_affine never
    evaluates the curve equation, here or in the reference (G1_proj.c:133-145: Z == 0 gives all-0xFF,
    otherwise X Z^-1, Y Z^-1; G1_jac.c:120-136 likewise), so the call is a public window onto the Fp
    load conversion, fe_mul / fe_sqr, fe_inv_sg and the store conversion.  The whole list, and its
    first 1, 2, 3, 31 and 33 rows alone."""
    nl, M = gpu.NLIMBS_P[curve], fe.fp_model(curve)
    rows = fe.offcurve_rows(curve)
    pts = fe.point_rows(rows, nl)
    want = fe.affine_rows(M, rows, coords)
    ref = _ref_or_none(request)
    for n in (len(rows), 1, 2, 3, 31, 33):
        sub = np.ascontiguousarray(pts[:n])
        got = gpu.batch_to_affine(curve, sub, coords=coords)
        bad = np.nonzero((got != want[:n]).any(axis=1))[0]
        assert not len(bad), (n, [tuple(hex(v) for v in rows[i]) for i in bad[:3]])
        if ref is not None:
            w = np.zeros_like(got)
            ref.arr(curve, f"G1_{coords}_batch_to_affine", n, sub, w)
            assert np.array_equal(got, w), n


# ---------------------------------------------------------------------------- (e) infinity layouts in k_norm_chunks
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("coords", ["proj", "jac"])
@pytest.mark.parametrize("n", fe.LAYOUT_N)
def test_infinity_layouts(gpu, oracle, request, curve, coords, n):
    """At the default ZK_NORM_LANES the chunk length is 2 and lane t of ceil(n / 2) owns rows t and
    t + lanes.  All rows infinite; both rows of lanes 0, 1 and the last lane; only the first / only
    the second row of every lane; the single row of the ragged last lane; the last row alone finite.
    Infinities are (0 : l : 0) projective and (l^2 : l^3 : 0) Jacobian.  The case "plain_0_1_0"
    writes them (0 : 1 : 0) in both systems: any row with Z = 0 is infinity here, and to_affine of
    the reference agrees (G1_jac.c:121-125), unlike its Jacobian add
    (test_gpu_g1ext.test_jac_fft_zero_one_zero_row_is_infinity)."""
    nl, M = gpu.NLIMBS_P[curve], fe.fp_model(curve)
    ref = _ref_or_none(request)
    for name, pts in fe.layout_rows(gpu, oracle, curve, coords, n, 2, 700 + n):
        want = fe.affine_rows(M, fe.point_ints(pts, nl), coords)
        inf = ~pts[:, 2 * nl:].any(axis=1)
        assert np.array_equal((want == fe.ALL_ONES).all(axis=1), inf)
        got = gpu.batch_to_affine(curve, pts, coords=coords)
        assert np.array_equal(got, want), (name, np.nonzero((got != want).any(axis=1))[0][:8])
        if ref is not None:
            w = np.zeros_like(got)
            ref.arr(curve, f"G1_{coords}_batch_to_affine", n, pts, w)
            assert np.array_equal(got, w), name


# ---------------------------------------------------------------------------- (f) the same kernel behind the group FFT
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("coords", ["proj", "jac"])
@pytest.mark.parametrize("m", [3, 6])
def test_group_fft_infinity_dense(gpu, oracle, request, curve, coords, m):
    """forward and inverse FFT whose outputs are mostly or wholly infinite (MODE_XYZZ_TO_PROJ of
    k_norm_chunks, bit-reversed stores on the inverse): all inputs infinite; a delta at index 0 and
    at index n - 1; a constant input, whose transform is infinite except at index 0.  Expected: the
    group's result by one oracle.msm per output (field_edges.fft_expected), and the reference's C
    where it is built -- the Jacobian FFT on every input, the projective one on the inputs it
    transforms as a group FFT does (field_edges.REF_PROJ_FFT_IS_GROUP_FFT says which and why)."""
    ref = _ref_or_none(request)
    sg = gpu.get_fft_subgroup(curve, m)
    for name, aff, pts in fe.fft_inputs(gpu, oracle, curve, coords, m):
        for inverse, f in ((False, gpu.forward_fft), (True, gpu.inverse_fft)):
            got = f(sg, pts, coords=coords)
            want = fe.fft_expected(oracle, curve, m, aff, inverse)
            assert np.array_equal(got, want), (name, inverse, np.nonzero((got != want).any(axis=1))[0][:8])
            if ref is not None and (coords == "jac" or name in fe.REF_PROJ_FFT_IS_GROUP_FFT):
                w = np.zeros_like(pts)
                ref.arr(curve, f"G1_{coords}_fft_{'inverse' if inverse else 'forward'}", m, sg.gen_array(), pts, w)
                assert np.array_equal(got, w), (name, inverse)


# ---------------------------------------------------------------------------- (g) digit boundaries in the bucket pipeline
_MSM_WANT = {}


def _digit_case(gpu, oracle, curve, c, name, n=192):
    """(scalars, points, normalised projective result of the oracle), computed once per input"""
    sc = fe.digit_scalars(curve, c, name, n)
    key = (curve, n, sc.tobytes())
    if key not in _MSM_WANT:
        pts = fe.digit_points(gpu.gen_points, curve, n)
        _MSM_WANT[key] = (pts, oracle.normalize(curve, oracle.msm(curve, sc, pts, mont=False, out="proj")))
    return (sc,) + _MSM_WANT[key]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("c", fe.MSM_WINDOWS)
def test_msm_digit_boundaries(gpu, oracle, curve, c):
    """msm_variable (an explicit window always takes the bucket pipeline) on 192 distinct points, rows
    5 and 100 infinite, with 256-bit std scalars used verbatim, one pattern per call: every window's
    raw digit B = 2^(c-1) (positive, no carry), B + 1 (negative, carry), B - 1, 2^c - 1 (the scalar
    2^256 - 1: the carry ripples through every window into the carry-only top window when c | 256),
    B and B + 1 alternating, 2^255, 2^256 - 2^c, r - 1, r, r + 1, only the top window non-zero, and
    all of them rotated by row"""
    for name in fe.DIGIT_PATTERNS:
        sc, pts, want = _digit_case(gpu, oracle, curve, c, name)
        got = gpu.msm_variable(curve, sc, pts, c)
        assert np.array_equal(got, want), (c, name)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("c", [8, 16, 17])
def test_msm_digit_carry_across_groups(gpu, oracle, curve, c):
    """device-resident with one window per pipeline pass (msm_set_group_limit(1)): the carry of the
    2^256 - 1 and the alternating patterns crosses every group boundary"""
    for name in ("all_ones", "alt_B_Bp1", "alt_Bp1_B", "rotated"):
        sc, pts, want = _digit_case(gpu, oracle, curve, c, name)
        ds, dp = gpu.DeviceBuffer(sc), gpu.DeviceBuffer(pts)
        try:
            gpu.msm_set_group_limit(1)
            got = gpu.msm_device(curve, sc.shape[0], ds, dp, mont=False, window=c)
            groups = gpu.msm_last_groups()
        finally:
            gpu.msm_set_group_limit(0)
            ds.free()
            dp.free()
        assert np.array_equal(oracle.normalize(curve, got), want), (c, name)
        assert groups == 256 // c + 1, (c, name)


@pytest.mark.parametrize("curve", CURVES)
def test_msm_digit_sort_ahead_groups(gpu, oracle, curve):
    """the sort-ahead shape (two window groups) at n = 4096, c = 16, on the same patterns"""
    c, n = 16, 4096
    for name in ("all_ones", "alt_B_Bp1", "rotated"):
        sc, pts, want = _digit_case(gpu, oracle, curve, c, name, n)
        ds, dp = gpu.DeviceBuffer(sc), gpu.DeviceBuffer(pts)
        try:
            gpu.msm_set_ahead_min(12)
            got = gpu.msm_device(curve, n, ds, dp, mont=False, window=c)
            assert gpu.msm_last_groups() == 2
        finally:
            gpu.msm_set_ahead_min(-1)
            ds.free()
            dp.free()
        assert np.array_equal(oracle.normalize(curve, got), want), name


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("mode", [0, 1])
def test_msm_digit_ysum_modes(gpu, oracle, curve, mode):
    """both Y-sum kernels on the 2^256 - 1 and alternating patterns, c in {13, 16}"""
    for c in (13, 16):
        for name in ("all_ones", "alt_B_Bp1", "alt_Bp1_B", "rotated"):
            sc, pts, want = _digit_case(gpu, oracle, curve, c, name)
            try:
                gpu.msm_set_ysum_mode(mode)
                got = gpu.msm_variable(curve, sc, pts, c)
            finally:
                gpu.msm_set_ysum_mode(-1)
            assert np.array_equal(got, want), (c, name)
