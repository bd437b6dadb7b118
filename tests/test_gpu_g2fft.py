"""GPU G2 group FFT (<C>_G2_proj_fft_forward / _fft_inverse, zkg_g2_fft_device), bit-exact against the
reference's own C (oracle/_ref; bls12_381_G2_proj.c:670-781).

Inputs are built with the reference library as test_gpu_g2ext.py builds them: distinct projective rows
P0 + i H from its scl_small / add (their Z is non-trivial), with special rows placed among them:
  rows 0 and N/2 hold the same point   one butterfly pair of the first forward level and of the top
                                       inverse level: u - t is infinity, u + t a doubling
  row 1: (0 : 1 : 0), row 3: (X : Y : 0) with X, Y non-zero (from N = 4), row 5: Z = one (from N = 8)
Any row with Z = 0 is the point at infinity here, whereas the reference's add
(add-2015-rcb) takes (X : Y : 0) with X != 0 for a finite point and returns values that are no group
sums.  As in test_gpu_g1ext.test_jac_fft_zero_one_zero_row_is_infinity, the expected output is therefore
the reference's for the same input with such rows written as its own infinity (0 : 1 : 0).

The reference multiplies N log N times by full-width scalars on one host core, so the direct comparisons
stay at 2^7 and every reference transform is computed once per module.

The reference's transform is not the group's on these rows, and the library reproduces it: the
reference's scalar multiplication maps infinity to (0 : 0 : 0) unless every 4-bit window of the scalar is
0 or 1 (its table holds dbl-2007-bl of (0 : 1 : 0)), its add maps anything plus (0 : 0 : 0) to
(0 : 0 : 0), and normalize writes (0 : 1 : 0) for it.  So the inverse transform of rows that hold an
infinity, or the same point twice in one butterfly pair, returns infinity where the group sum is a finite
point (m = 2: rows 0 and 2, m = 3: the odd rows)."""
import ctypes
import random

import numpy as np
import pytest

import golden_io
from field_edges import FP

pytestmark = pytest.mark.gpu
CURVES = ["bn128", "bls12_381"]
NPS = {"bn128": 4, "bls12_381": 6}
FR_FLD = {"bn128": 1, "bls12_381": 3}
FR = golden_io.FR_ORDER
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
G2_FFT_MAX_LOG = 24  # zk_g2fft.hip


# ---------------------------------------------------------------------------- inputs

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


def ref_normalize(reference, curve, rows):
    out = np.zeros_like(rows)
    for i in range(rows.shape[0]):
        reference.arr(curve, "G2_proj_normalize", np.ascontiguousarray(rows[i]), out[i])
    return out


def inf_010(reference, curve):
    return ref_from_affine(reference, curve, np.full((1, 4 * NPS[curve]), ONES, np.uint64))[0]


def special_rows(reference, curve, proj):
    """place the special rows (module docstring) in a copy of `proj`; returns (rows, rows for the reference)"""
    NP, n = NPS[curve], proj.shape[0]
    rows = proj.copy()
    xy0 = []
    if n >= 4:
        rows[1] = inf_010(reference, curve)
        assert rows[3, :2 * NP].any() and rows[3, 2 * NP:4 * NP].any()
        rows[3, 4 * NP:] = 0  # (X : Y : 0)
        xy0 = [3]
    if n >= 8:
        rows[5] = ref_from_affine(reference, curve, ref_to_affine(reference, curve, rows[5:6]))[0]  # Z = one
    if n >= 2:
        rows[n // 2] = rows[0]
    ref_rows = rows.copy()
    ref_rows[xy0] = inf_010(reference, curve)
    return rows, ref_rows


class Cases:
    """inputs and the reference's transforms of them, computed once and never modified"""

    def __init__(self, gpu, reference):
        self.gpu, self.reference = gpu, reference
        self.prog = {c: progression(reference.lib, c, 1 << 10) for c in CURVES}
        self._rows, self._want = {}, {}

    def rows(self, curve, m, kind="special"):
        key = (curve, m, kind)
        if key not in self._rows:
            if kind == "special":
                r = special_rows(self.reference, curve, np.ascontiguousarray(self.prog[curve][:1 << m]))
            else:
                p = nonsubgroup_rows(self.reference, curve, 1 << m, 700 + m)
                r = (p, p)
            for a in r:
                a.setflags(write=False)
            self._rows[key] = r
        return self._rows[key]

    def want(self, curve, m, inverse, kind="special"):
        key = (curve, m, inverse, kind)
        if key not in self._want:
            ref_rows = self.rows(curve, m, kind)[1]
            out = np.zeros_like(ref_rows)
            name = "G2_proj_fft_inverse" if inverse else "G2_proj_fft_forward"
            self.reference.arr(curve, name, m, self.gpu.get_fft_subgroup(curve, m).gen_array(), ref_rows, out)
            out.setflags(write=False)
            self._want[key] = out
        return self._want[key]


@pytest.fixture(scope="module")
def cases(gpu, reference):
    return Cases(gpu, reference)


def run(gpu, curve, m, rows, inverse):
    sg = gpu.get_fft_subgroup(curve, m)
    return (gpu.g2_inverse_fft if inverse else gpu.g2_forward_fft)(sg, rows)


def is_inf_010(curve, row):
    NP = NPS[curve]
    return not row[:2 * NP].any() and row[2 * NP:4 * NP].any() and not row[4 * NP:].any()


# ---------------------------------------------------------------------------- 1. against the reference

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("m", [0, 1, 2, 3, 5, 7])
def test_g2_fft_vs_reference(gpu, cases, curve, m, inverse):
    rows = cases.rows(curve, m)[0]
    want = cases.want(curve, m, inverse)
    got = run(gpu, curve, m, rows, inverse)
    assert got.shape == want.shape
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    assert bad.size == 0, bad[:10]
    if m == 1:  # the same point twice: forward (2P, infinity), inverse (P, infinity)
        assert is_inf_010(curve, got[1]) and not is_inf_010(curve, got[0])


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_g2_fft_single_infinite_row(gpu, reference, cases, curve, inverse):
    """m = 0 on both forms of infinity: the normalised row is (0 : 1 : 0)"""
    NP = NPS[curve]
    xy0 = cases.prog[curve][7:8].copy()
    xy0[0, 4 * NP:] = 0
    for row in (xy0, inf_010(reference, curve)[None, :].copy()):
        got = run(gpu, curve, 0, row, inverse)
        assert np.array_equal(got[0], inf_010(reference, curve))


@pytest.mark.parametrize("curve", CURVES)
def test_g2_fft_infinity_times_twiddle(gpu, reference, cases, curve):
    """What a twiddle makes of an infinite operand, m = 3 forward, against the reference:
      * rows 2 and 6 infinite: their sum and difference are the v of level 2.  Butterfly j = 0 multiplies by
        1 and keeps the infinity; j = 1 multiplies by w^2 and makes the reference's (0 : 0 : 0), which the
        odd outputs inherit
      * the odd rows infinite: the odd half meets the twiddles w^j, j != 0; only outputs 0 and 4 stay finite
      * the same rows with generator 1: every twiddle is 1, all of whose 4-bit windows are 0 or 1, so
        infinity stays infinity and the outputs are the even half's transform, twice (its entry 3 is
        x0 - x4 - x2 + x6, infinite on the progression P0 + i H)"""
    m, NP = 3, NPS[curve]
    lib, inf = gpu.load(), inf_010(reference, curve)
    base = np.ascontiguousarray(cases.prog[curve][:1 << m])
    w = gpu.get_fft_subgroup(curve, m).gen_array()
    one = gpu.get_fft_subgroup(curve, 0).gen_array()
    for infinite, gen, finite in (([2, 6], w, [0, 2, 4, 6]), ([1, 3, 5, 7], w, [0, 4]),
                                  ([1, 3, 5, 7], one, [0, 1, 2, 4, 5, 6])):
        rows = base.copy()
        rows[infinite] = inf
        want, got = np.zeros_like(rows), np.zeros_like(rows)
        reference.arr(curve, "G2_proj_fft_forward", m, gen, rows, want)
        getattr(lib, f"{curve}_G2_proj_fft_forward")(m, gpu._p(gen), gpu._p(rows), gpu._p(got))
        assert [i for i in range(8) if want[i, 4 * NP:].any()] == list(finite)
        assert np.array_equal(got, want), (infinite, np.nonzero(np.any(got != want, axis=1))[0])


# ---------------------------------------------------------------------------- 2. device entry

@pytest.mark.parametrize("curve", CURVES)
def test_g2_fft_device(gpu, reference, cases, curve):
    lib, cid, m = gpu.load(), gpu.CURVE_ID[curve], 5
    rows = np.ascontiguousarray(cases.rows(curve, m)[0])
    gen = gpu.get_fft_subgroup(curve, m).gen_array()
    d_src = gpu.DeviceBuffer(rows)
    fill = np.full_like(rows, np.uint64(0x1234567890ABCDEF))
    d_tgt = gpu.DeviceBuffer(fill)
    try:
        for inverse in (False, True):
            host = run(gpu, curve, m, rows, inverse)
            assert np.array_equal(host, cases.want(curve, m, inverse))
            gpu.g2_fft_device(curve, m, gen, d_src, d_tgt, inverse=inverse)
            assert np.array_equal(d_tgt.to_host(fill), host)
            assert gpu.last_error() is None
        # m = 0 copies the normalised first row and writes nothing else
        d_tgt.free()
        d_tgt = gpu.DeviceBuffer(fill)
        lib.zkg_g2_fft_device(cid, 0, 0, gpu._p(gpu.get_fft_subgroup(curve, 0).gen_array()), d_src.ptr, d_tgt.ptr)
        back = d_tgt.to_host(fill)
        assert np.array_equal(back[0], ref_normalize(reference, curve, rows[:1])[0])
        assert np.array_equal(back[1:], fill[1:])
        assert gpu.last_error() is None
    finally:
        d_src.free()
        d_tgt.free()


# ---------------------------------------------------------------------------- 3. outside the order-r subgroup

def fp_sqrt(a, p):
    """square root in Fp, p = 3 mod 4, or None"""
    s = pow(a, (p + 1) // 4, p)
    return s if s * s % p == a % p else None


def fp2_sqrt(a, p):
    """square root of a = (a0, a1) in Fp[u] / (u^2 + 1) by the norm method (p = 3 mod 4), or None"""
    a0, a1 = a
    if a1 == 0:
        s = fp_sqrt(a0, p)
        if s is not None:
            return (s, 0)
        s = fp_sqrt(-a0 % p, p)
        return None if s is None else (0, s)
    n = fp_sqrt((a0 * a0 + a1 * a1) % p, p)
    if n is None:
        return None
    inv2 = (p + 1) // 2
    for d in ((a0 + n) * inv2 % p, (a0 - n) * inv2 % p):
        x0 = fp_sqrt(d, p)
        if x0:
            x1 = a1 * pow(2 * x0, p - 2, p) % p
            if ((x0 * x0 - x1 * x1) % p, 2 * x0 * x1 % p) == (a0 % p, a1 % p):
                return (x0, x1)
    return None


def fp2_mul(a, b, p):
    return ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)


def nonsubgroup_rows(reference, curve, n, seed):
    """n projective rows (Z = one) of the twist that lie outside the order-r subgroup, made with Python
    integers; the twist constant is y^2 - x^3 of the reference's generator"""
    NP, p = NPS[curve], FP[curve]
    assert p % 4 == 3

    def conv(name, limbs):
        out = np.zeros(NP, np.uint64)
        reference.arr(curve, name, np.ascontiguousarray(limbs), out)
        return out

    def to_int(limbs):
        return sum(int(x) << (64 * i) for i, x in enumerate(conv("Fp_mont_to_std", limbs)))

    def to_mont(v):
        return conv("Fp_mont_from_std", golden_io._limbs(v, NP))

    g = np.ctypeslib.as_array((ctypes.c_uint64 * (4 * NP)).in_dll(reference.lib, f"{curve}_G2_affine_gen_G2")).copy()
    gx = (to_int(g[:NP]), to_int(g[NP:2 * NP]))
    gy = (to_int(g[2 * NP:3 * NP]), to_int(g[3 * NP:]))
    x3 = fp2_mul(fp2_mul(gx, gx, p), gx, p)
    y2 = fp2_mul(gy, gy, p)
    b = ((y2[0] - x3[0]) % p, (y2[1] - x3[1]) % p)
    rng = random.Random(seed)
    aff = []
    while len(aff) < n:
        x = (rng.randrange(p), rng.randrange(p))
        x3 = fp2_mul(fp2_mul(x, x, p), x, p)
        y = fp2_sqrt(((x3[0] + b[0]) % p, (x3[1] + b[1]) % p), p)
        if y is None:
            continue
        row = np.concatenate([to_mont(x[0]), to_mont(x[1]), to_mont(y[0]), to_mont(y[1])])
        assert reference.arr(curve, "G2_affine_is_on_curve", row, restype=ctypes.c_uint8) == 1
        aff.append(row)
    proj = ref_from_affine(reference, curve, np.stack(aff))
    for i in range(n):
        assert reference.arr(curve, "G2_proj_is_in_subgroup", np.ascontiguousarray(proj[i]),
                             restype=ctypes.c_uint8) == 0
    return proj


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("m", [1, 3, 5])
def test_g2_fft_nonsubgroup_points(gpu, cases, curve, m, inverse):
    """both twists have a cofactor: only the reference's per-level integer scalars reproduce its output"""
    rows = cases.rows(curve, m, "nonsubgroup")[0]
    got = run(gpu, curve, m, rows, inverse)
    bad = np.nonzero(np.any(got != cases.want(curve, m, inverse, "nonsubgroup"), axis=1))[0]
    assert bad.size == 0, bad[:10]


# ---------------------------------------------------------------------------- 4. grid-stride loop

@pytest.fixture
def lanes256(gpu):
    gpu.g2_fft_set_max_lanes(256)
    try:
        yield gpu
    finally:
        gpu.g2_fft_set_max_lanes(0)


@pytest.mark.parametrize("curve", CURVES)
def test_g2_fft_grid_stride_partial(lanes256, cases, curve):
    """m = 7 inverse: 128 outputs in one partial stride of 256 lanes"""
    got = run(lanes256, curve, 7, cases.rows(curve, 7)[0], True)
    assert np.array_equal(got, cases.want(curve, 7, True))


def fr_std(oracle, curve, mont):
    limbs = oracle.to_std(FR_FLD[curve], np.ascontiguousarray(mont).reshape(1, 4))[0]
    return sum(int(x) << (64 * i) for i, x in enumerate(limbs))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_g2_fft_grid_stride_many(lanes256, oracle, reference, cases, curve, inverse):
    """m = 10 with 256 lanes: 512 butterflies (forward) or 1024 outputs (inverse), several strides.
    Eight outputs against the reference's G2 MSM on the same (subgroup) rows: forward out[k] = sum_j
    w^(jk) P_j, inverse out[j] = N^-1 sum_k w^(-jk) P_k, scalars computed with Python integers mod r;
    affine forms compared.  (The index convention is the one the direct comparisons at m <= 7 pin.)"""
    gpu, m = lanes256, 10
    n, NP, r = 1 << m, NPS[curve], FR[curve]
    rows = cases.prog[curve]
    aff = ref_to_affine(reference, curve, rows)
    sg = gpu.get_fft_subgroup(curve, m)
    w = fr_std(oracle, curve, sg.gen_array())
    assert pow(w, n, r) == 1 and pow(w, n // 2, r) == r - 1
    got = run(gpu, curve, m, rows, inverse)
    base, scale = (pow(w, r - 2, r), pow(n, r - 2, r)) if inverse else (w, 1)
    for k in (0, 1, 2, 333, n // 2 - 1, n // 2, n - 2, n - 1):
        sc = np.stack([golden_io._limbs(scale * pow(base, j * k, r) % r, 4) for j in range(n)])
        want = np.zeros(4 * NP, np.uint64)
        reference.arr(curve, "G2_proj_MSM_std_coeff_affine_out", n, sc, aff, want, 4)
        assert got[k, 4 * NP:].any(), k  # finite, normalised: (x : y : 1)
        assert np.array_equal(got[k, :4 * NP], want), k


# ---------------------------------------------------------------------------- 5. round trip

@pytest.mark.parametrize("curve", CURVES)
def test_g2_fft_roundtrip_2_10(gpu, reference, cases, curve):
    """iFFT(FFT(x)) is the reference's normalize of every row of x (subgroup rows, infinities among them).
    The rows are distinct: with rows 0 and N/2 equal, x_0 - x_(N/2) is an infinity that the inverse
    multiplies by a twiddle, which in the reference's schedule (module docstring) loses both rows."""
    m = 10
    rows = special_rows(reference, curve, cases.prog[curve])[0].copy()
    rows[1 << (m - 1)] = cases.prog[curve][1 << (m - 1)]
    sg = gpu.get_fft_subgroup(curve, m)
    back = gpu.g2_inverse_fft(sg, gpu.g2_forward_fft(sg, rows))
    want = ref_normalize(reference, curve, rows)
    assert is_inf_010(curve, want[1]) and is_inf_010(curve, want[3])
    bad = np.nonzero(np.any(back != want, axis=1))[0]
    assert bad.size == 0, bad[:10]


# ---------------------------------------------------------------------------- 6. limits

@pytest.fixture
def recoverable(gpu):
    gpu.set_error_mode(True)
    assert gpu.last_error() is None
    yield gpu
    gpu.set_error_mode(False)
    gpu.last_error()


@pytest.mark.parametrize("curve", CURVES)
def test_g2_fft_size_limits(recoverable, cases, curve):
    """m < 0 and m above the limit report through the error channel (nothing is read or allocated for
    them); the library keeps working afterwards"""
    gpu = recoverable
    lib, cid = gpu.load(), gpu.CURVE_ID[curve]
    row = np.ascontiguousarray(cases.rows(curve, 0)[0])
    out = np.zeros_like(row)
    gen = gpu.get_fft_subgroup(curve, 3).gen_array()
    for m in (-1, G2_FFT_MAX_LOG + 1):
        for d in ("forward", "inverse"):
            getattr(lib, f"{curve}_G2_proj_fft_{d}")(m, gpu._p(gen), gpu._p(row), gpu._p(out))
            msg = gpu.last_error()
            assert msg is not None and "G2 fft" in msg, (m, d)
            assert gpu.last_error() is None  # cleared once read
            assert not out.any()
        lib.zkg_g2_fft_device(cid, 0, m, gpu._p(gen), None, None)
        assert gpu.last_error() is not None, m
    for inverse in (False, True):
        assert np.array_equal(run(gpu, curve, 3, cases.rows(curve, 3)[0], inverse), cases.want(curve, 3, inverse))
    assert gpu.last_error() is None
