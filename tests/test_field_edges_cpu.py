"""The big-integer models of tests/field_edges.py against the oracle and the reference's own C, on
the full edge sets of both curves and both fields -- before tests/test_gpu_field_edges.py lets the
models judge a kernel.  CPU only.  Also: the divstep batch counts of zk_params.inc against the
Bernstein-Yang bound, and the oracle's MSM against the reference's on the 256-bit digit patterns."""
import ctypes

import numpy as np
import pytest

import field_edges as fe
import golden_io

CURVES = ["bn128", "bls12_381"]
U64P = ctypes.POINTER(ctypes.c_uint64)


def _ptr(a):
    return a.ctypes.data_as(U64P)


def test_edge_values_hold_the_named_values():
    for field, q in fe.FIELDS.items():
        K = fe.radix_ratio(field)
        assert K == (256 if field == "bls12_381_fp" else 32)
        E = fe.field_edges(field)
        assert E == sorted(set(E)) and all(0 <= e < q for e in E)
        R, Ki = fe.radix(q), pow(K, -1, q)
        named = [0, 1, q - 1, (q - 1) // 2, R % q, R * R % q, 1 << 60, (1 << 58) - 1, q // K, (K - 1) * q // K + 1]
        assert set(named) <= set(E)
        assert {e * Ki % q for e in named} <= set(E)  # K v mod q is on the edge too
        assert len(E) <= 1500


# ---------------------------------------------------------------------------- Fr models
def _fr_arrays(curve):
    a, b, c, ks = fe.fr_cross(curve)
    return fe.to_limbs(a, 4), fe.to_limbs(b, 4), fe.to_limbs(c, 4), [fe.to_row(k, 4) for k in ks]


@pytest.mark.parametrize("curve", CURVES)
def test_fr_models_vs_oracle(oracle, curve):
    a, b, c, ks = _fr_arrays(curve)
    n = a.shape[0]
    want = fe.fr_cross_expected(curve)
    for op in fe.UNARY + fe.BINARY + fe.TERNARY:
        assert np.array_equal(oracle.arr_op(curve, op, n, a, b, c), want[op]), op
    assert np.array_equal(oracle.arr_dot(curve, a, b), want["dot"][0])
    for i, k in enumerate(ks):
        kB = ks[(i + 1) % 4]
        assert np.array_equal(oracle.arr_op(curve, "scale", n, a, kA=k), want[f"scale_{i}"])
        assert np.array_equal(oracle.arr_op(curve, "Ax_plus_y", n, a, b, kA=k), want[f"Ax_plus_y_{i}"])
        assert np.array_equal(oracle.arr_op(curve, "Ax_plus_By", n, a, b, kA=k, kB=kB), want[f"Ax_plus_By_{i}"])
    M = fe.fr_model(curve)
    for ka, kb in fe.powers_cases(curve):
        for m in fe.POWERS_N:
            got = oracle.arr_powers(curve, fe.to_row(ka, 4), fe.to_row(kb, 4), m)
            assert np.array_equal(got, fe.to_limbs(M.powers(ka, kb, m), 4)), (hex(ka), hex(kb), m)
    for name, x, y in fe.inv_vectors(curve):
        ax, ay = fe.to_limbs(x, 4), fe.to_limbs(y, 4)
        assert np.array_equal(oracle.arr_op(curve, "inv", len(y), ay), fe.to_limbs(M.inv(y), 4)), name
        assert np.array_equal(oracle.arr_op(curve, "div", len(y), ax, ay), fe.to_limbs(M.div(x, y), 4)), name
    for op, (*ins, t) in fe.fr_targets(curve).items():
        arrs = [fe.to_limbs(v, 4) for v in ins]
        assert np.array_equal(oracle.arr_op(curve, op, len(t), *arrs), fe.to_limbs(t, 4)), op


@pytest.mark.parametrize("curve", CURVES)
def test_sqr_targets_cover_a_third_of_the_edges(curve):
    """fr_targets reaches an edge value t through sqr only where t R is a square mod r: 176 of 278
    (BN254) and 189 of 279 (BLS12-381) edge values.  That is more than the half of random values:
    the even powers of two and their neighbours' pre-images share their residuosity."""
    a, t = fe.fr_targets(curve)["sqr"]
    E = fe.field_edges(curve + "_fr")
    assert 3 * len(t) >= len(E)
    assert (len(t), len(E)) == {"bn128": (176, 278), "bls12_381": (189, 279)}[curve]


@pytest.mark.parametrize("curve", CURVES)
def test_fr_models_vs_reference(reference, curve):
    a, b, c, ks = _fr_arrays(curve)
    n = a.shape[0]
    want = fe.fr_cross_expected(curve)

    def ref(name, count, *args):
        out = np.zeros((count, 4), dtype=np.uint64)
        reference.arr(curve, "arr_mont_" + name, count, *args, out)
        return out
    for op, args in (("neg", (a,)), ("sqr", (a,)), ("to_std", (a,)), ("from_std", (a,)), ("add", (a, b)),
                     ("sub", (a, b)), ("mul", (a, b)), ("mul_add", (a, b, c)), ("mul_sub", (a, b, c))):
        assert np.array_equal(ref(op, n, *args), want[op]), op
    for i, k in enumerate(ks):
        assert np.array_equal(ref("scale", n, k, a), want[f"scale_{i}"])
        assert np.array_equal(ref("Ax_plus_y", n, k, a, b), want[f"Ax_plus_y_{i}"])
    M = fe.fr_model(curve)
    for name, x, y in fe.inv_vectors(curve):
        ax, ay = fe.to_limbs(x, 4), fe.to_limbs(y, 4)
        assert np.array_equal(ref("inv", len(y), ay), fe.to_limbs(M.inv(y), 4)), name
        assert np.array_equal(ref("div", len(y), ax, ay), fe.to_limbs(M.div(x, y), 4)), name


# ---------------------------------------------------------------------------- Fp models
@pytest.mark.parametrize("curve", CURVES)
def test_fp_models_vs_oracle(oracle, curve):
    """zko_fmul / zko_finv / zko_fadd / zko_fsub over the Fp edge set and a rotation of it"""
    p = fe.FP[curve]
    nl, fid, M = fe.nlimbs(p), golden_io.FP_ID[curve], fe.fp_model(curve)
    E = fe.field_edges(curve + "_fp")
    A, B = fe.to_limbs(E, nl), fe.to_limbs(fe.rotate(E, len(E) // 3), nl)
    out = np.zeros(nl, dtype=np.uint64)
    for i, (x, y) in enumerate(zip(E, fe.rotate(E, len(E) // 3))):
        for f, want in ((oracle.lib.zko_fmul, M.mul1(x, y)), (oracle.lib.zko_fadd, (x + y) % p),
                        (oracle.lib.zko_fsub, (x - y) % p)):
            f(fid, _ptr(A[i]), _ptr(B[i]), _ptr(out))
            assert fe.from_limbs(out) == want, (hex(x), hex(y))
        oracle.lib.zko_finv(fid, _ptr(A[i]), _ptr(out))
        assert fe.from_limbs(out) == M.inv1(x), hex(x)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("coords", ["proj", "jac"])
def test_affine_models_vs_reference(zk, oracle, reference, curve, coords):
    """<C>_G1_{proj,jac}_batch_to_affine of the reference on the off-curve edge rows and on every
    infinity layout: the model gives the same bytes"""
    nl, M = zk.NLIMBS_P[curve], fe.fp_model(curve)

    def ref(pts):
        out = np.zeros((pts.shape[0], 2 * nl), dtype=np.uint64)
        reference.arr(curve, f"G1_{coords}_batch_to_affine", pts.shape[0], pts, out)
        return out
    rows = fe.offcurve_rows(curve)
    assert np.array_equal(ref(fe.point_rows(rows, nl)), fe.affine_rows(M, rows, coords))
    for n in fe.LAYOUT_N:
        for chk in (2, min(max(n, 2), 32)):
            for name, pts in fe.layout_rows(zk, oracle, curve, coords, n, chk, 700 + n):
                assert np.array_equal(ref(pts), fe.affine_rows(M, fe.point_ints(pts, nl), coords)), (n, chk, name)


# ---------------------------------------------------------------------------- group FFT closed form
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("coords", ["proj", "jac"])
def test_fft_closed_form_vs_reference(zk, oracle, reference, curve, coords):
    """field_edges.fft_expected (one oracle.msm per output) equals the reference's group FFT on the
    infinity-dense inputs of the GPU test at m = 3: the Jacobian FFT on every input, the projective
    one where the reference computes a group FFT (field_edges.REF_PROJ_FFT_IS_GROUP_FFT)"""
    m = 3
    gen = oracle.fft_generator(curve, m)
    for name, aff, pts in fe.fft_inputs(zk, oracle, curve, coords, m):
        if coords == "proj" and name not in fe.REF_PROJ_FFT_IS_GROUP_FFT:
            continue  # see the comment at field_edges.REF_PROJ_FFT_IS_GROUP_FFT
        for inverse in (False, True):
            want = np.zeros_like(pts)
            reference.arr(curve, f"G1_{coords}_fft_{'inverse' if inverse else 'forward'}", m, gen, pts, want)
            assert np.array_equal(fe.fft_expected(oracle, curve, m, aff, inverse), want), (name, inverse)


# ---------------------------------------------------------------------------- divstep batch counts
def test_divstep_batch_counts():
    """Bernstein-Yang: ceil((49 d + 57) / 17) divsteps invert every input below a d-bit modulus.
    Both limb layouts of zk_inv.hpp run at least that many (19 x 60 = 1140 >= 1102 and
    13 x 60 = 780 >= 739 for the default; 18 x 62 and 12 x 62 for the other)."""
    d = fe.params()
    for field, q in fe.FIELDS.items():
        bound = -(-(49 * q.bit_length() + 57) // 17)
        P = "ZK_" + field.upper()
        assert d[P + "_S60_BATCHES"] * 60 >= bound, field
        assert d[P + "_S62_BATCHES"] * 62 >= bound, field
    assert -(-(49 * 381 + 57) // 17) == 1102 and -(-(49 * 255 + 57) // 17) == 739


# ---------------------------------------------------------------------------- MSM digit patterns
@pytest.mark.parametrize("curve", CURVES)
def test_digit_patterns_are_what_they_say(curve):
    """the signed-digit recoding of DigitStream::next restated on Python integers: the raw digits of
    each pattern are the ones its name promises, and the recoded digits sum back to the scalar"""
    for c in fe.MSM_WINDOWS:
        B, W = 1 << (c - 1), 256 // c + 1
        raws = {}
        for name, s in fe.digit_patterns(curve, c).items():
            k, carry, digits, raw = s, 0, [], []
            for _ in range(W):
                r = (k & ((1 << c) - 1)) + carry
                k >>= c
                raw.append(r)
                carry = 1 if r > B else 0
                digits.append(r - (1 << c) if r > B else r)
            assert k == 0 and carry == 0, (c, name)  # W windows take the whole scalar and the last carry
            assert sum(d << (c * w) for w, d in enumerate(digits)) == s, (c, name)
            raws[name] = raw
        full = 255 // c + (1 if 256 % c == 0 else 0)  # windows below the truncated / carry-only top
        assert raws["raw_B"][:full] == [B] * full
        assert raws["raw_Bp1"][:full] == [B + 1] * full
        assert raws["raw_Bm1"][:full] == [B - 1] * full
        assert raws["all_ones"][0] == (1 << c) - 1 and raws["all_ones"][1:255 // c] == [1 << c] * (255 // c - 1)
        assert raws["alt_B_Bp1"][:4] == [B, B + 1, B, B + 1]
        if 256 % c == 0:  # the carry-only top window
            assert raws["all_ones"][W - 1] == 1 and raws["raw_Bp1"][W - 1] == 1 and raws["raw_B"][W - 1] == 0


@pytest.mark.parametrize("curve", CURVES)
def test_digit_patterns_oracle_vs_reference(zk, oracle, reference, curve):
    """the oracle takes 256-bit std scalars verbatim as the reference does: n = 8, every pattern"""
    n = 8
    pts = fe.digit_points(zk.gen_points, curve, n)
    seen = set()
    for c in fe.MSM_WINDOWS:
        for name in fe.DIGIT_PATTERNS:
            sc = fe.digit_scalars(curve, c, name, n)
            if sc.tobytes() in seen:
                continue
            seen.add(sc.tobytes())
            want = reference.normalize(curve, reference.msm(curve, sc, pts, mont=False, out="proj"))
            assert np.array_equal(oracle.normalize(curve, oracle.msm(curve, sc, pts, mont=False, out="proj")), want), (c, name)
