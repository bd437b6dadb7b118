"""GPU polynomial layer (<C>_poly_mont_{mul_naive,eval_at,lincomb,add,sub,neg,scale,is_zero,is_equal,
degree} and the zkg_poly_*_device entries): bit for bit against the reference's own C
(oracle/_ref/libzkref.so, built from <C>_poly_mont.c).  No result is compared with another GPU
result; where the reference's quadratic product would take hours the expected value is a closed
form built from the reference's arr_mont / Fr_mont / eval_at functions."""
import ctypes
import itertools

import numpy as np
import pytest

import field_edges as fe

pytestmark = pytest.mark.gpu
CURVES = ["bn128", "bls12_381"]
U64P = ctypes.POINTER(ctypes.c_uint64)
BIG = 1 << 30  # "always the direct kernel"
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)


@pytest.fixture
def hooks(gpu):
    yield gpu
    gpu.poly_set_mul_direct_max(-1)


def fr(gpu, curve, seed, n):
    return gpu.gen_fr(curve, seed, n)


def edges(curve, n, rot=0):
    """n coefficients cycling through the Fr edge list"""
    E = fe.rotate(fe.field_edges(curve + "_fr"), rot)
    return fe.to_limbs([E[i % len(E)] for i in range(n)], 4)


def r_minus_1(curve, n):
    return fe.to_limbs([fe.FR[curve] - 1] * n, 4)


# ---------------------------------------------------------------------------- the reference's C
def ref_mul(reference, curve, a, b):
    out = np.zeros((max(0, a.shape[0] + b.shape[0] - 1), 4), dtype=np.uint64)
    reference.arr(curve, "poly_mont_mul_naive", a.shape[0], a, b.shape[0], b, out)
    return out


def ref_eval(reference, curve, p, x):
    out = np.zeros(4, dtype=np.uint64)
    reference.arr(curve, "poly_mont_eval_at", p.shape[0], p, np.ascontiguousarray(x), out)
    return out


def ref_fr_mul(reference, curve, x, y):
    out = np.zeros(4, dtype=np.uint64)
    reference.arr(curve, "Fr_mont_mul", np.ascontiguousarray(x), np.ascontiguousarray(y), out)
    return out


def ref_lincomb(reference, curve, terms):
    K = len(terms)
    ks = [np.ascontiguousarray(k, dtype=np.uint64) for k, _ in terms]
    ps = [np.ascontiguousarray(p, dtype=np.uint64) for _, p in terms]
    out = np.full((max([p.shape[0] for p in ps], default=0) + 1, 4), SENTINEL, dtype=np.uint64)
    f = getattr(reference.lib, f"{curve}_poly_mont_lincomb")
    f.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(U64P), ctypes.POINTER(U64P), U64P]
    f(K, (ctypes.c_int * max(1, K))(*[p.shape[0] for p in ps]),
      (U64P * max(1, K))(*[k.ctypes.data_as(U64P) for k in ks]),
      (U64P * max(1, K))(*[p.ctypes.data_as(U64P) for p in ps]), out.ctypes.data_as(U64P))
    assert np.all(out[-1] == SENTINEL)
    return out[:-1]


# ---------------------------------------------------------------------------- product
SHAPES = list(itertools.product([1, 2, 3, 31, 32, 33, 64, 65, 257, 1000], [1, 2, 33, 257])) + [
    (1025, 1024), (2049, 2047), (4097, 1)]


def expected_log(n1, n2):
    return max(4, (n1 + n2 - 2).bit_length())


@pytest.mark.parametrize("curve", CURVES)
def test_product_against_mul_naive(hooks, reference, curve):
    gpu = hooks
    default_max = None
    for n1, n2 in SHAPES:
        a, b = fr(gpu, curve, 100 + n1, n1), fr(gpu, curve, 200 + n2, n2)
        want = ref_mul(reference, curve, a, b)
        gpu.poly_set_mul_direct_max(0)
        assert np.array_equal(gpu.poly_mul(curve, a, b), want), (n1, n2, "ntt")
        assert gpu.poly_last_mul_path() == expected_log(n1, n2), (n1, n2)
        gpu.poly_set_mul_direct_max(BIG)
        assert np.array_equal(gpu.poly_mul(curve, a, b), want), (n1, n2, "direct")
        assert gpu.poly_last_mul_path() == 0, (n1, n2)
        gpu.poly_set_mul_direct_max(-1)
        assert np.array_equal(gpu.poly_mul(curve, a, b), want), (n1, n2, "default")
        path = gpu.poly_last_mul_path()
        assert path in (0, expected_log(n1, n2))
        if path == 0:
            default_max = max(default_max or 0, min(n1, n2))
    assert default_max is not None and default_max >= 1  # a linear factor runs on the direct kernel


def default_direct_max(gpu, curve):
    """the longest shorter factor the direct path takes by default, found through the path hook"""
    gpu.poly_set_mul_direct_max(-1)
    one = fr(gpu, curve, 1, 600)
    best = 0
    for ns in range(1, 513):
        gpu.poly_mul(curve, one, one[:ns])
        if gpu.poly_last_mul_path() != 0:
            break
        best = ns
    return best


@pytest.mark.parametrize("curve", CURVES)
def test_product_edge_coefficients(hooks, reference, curve):
    gpu = hooks
    dm = default_direct_max(gpu, curve)
    assert 1 <= dm <= 512
    # all r - 1, the longest inner length of the default direct path, and 257 x 257 on the transform
    a, b = r_minus_1(curve, 300), r_minus_1(curve, dm)
    assert np.array_equal(gpu.poly_mul(curve, a, b), ref_mul(reference, curve, a, b))
    assert gpu.poly_last_mul_path() == 0
    a = r_minus_1(curve, 257)
    gpu.poly_set_mul_direct_max(0)
    assert np.array_equal(gpu.poly_mul(curve, a, a.copy()), ref_mul(reference, curve, a, a))
    assert gpu.poly_last_mul_path() == 10
    # the edge list with zero leading and trailing coefficients, on both paths
    z = np.zeros((3, 4), dtype=np.uint64)
    a = np.concatenate([z, edges(curve, 200), z])
    b = np.concatenate([z[:1], edges(curve, 70, rot=11), z[:2]])
    want = ref_mul(reference, curve, a, b)
    for mode in (0, BIG):
        gpu.poly_set_mul_direct_max(mode)
        assert np.array_equal(gpu.poly_mul(curve, a, b), want), mode
        assert np.array_equal(gpu.poly_mul(curve, b, a), want), mode
    # a zero polynomial times a random one
    zero, rnd = np.zeros((40, 4), dtype=np.uint64), fr(gpu, curve, 7, 90)
    for mode in (0, BIG, -1):
        gpu.poly_set_mul_direct_max(mode)
        assert np.array_equal(gpu.poly_mul(curve, zero, rnd), ref_mul(reference, curve, zero, rnd))
    # squaring: ONE array as both factors (Haskell's sqr x = mul x x)
    for n in (1, 33, 500):
        a = edges(curve, n, rot=5)
        want = ref_mul(reference, curve, a, a)
        for mode in (0, BIG, -1):
            gpu.poly_set_mul_direct_max(mode)
            assert np.array_equal(gpu.poly_sqr(curve, a), want), (n, mode)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n1,n2", [((1 << 16) + 1, 1 << 16), ((1 << 17) + 3, 1 << 15)])
def test_large_transforms_closed_forms(hooks, reference, curve, n1, n2):
    gpu = hooks
    gpu.poly_set_mul_direct_max(-1)
    p = fr(gpu, curve, 31, n1)
    # sparse second factor a + b x^(n2 - 1): the product is a p plus b p shifted by n2 - 1
    ka, kb = fr(gpu, curve, 32, 2)
    q = np.zeros((n2, 4), dtype=np.uint64)
    q[0], q[n2 - 1] = ka, kb
    ap, bp = np.zeros_like(p), np.zeros_like(p)
    reference.arr(curve, "arr_mont_scale", n1, ka, p, ap)
    reference.arr(curve, "arr_mont_scale", n1, kb, p, bp)
    N = n1 + n2 - 1
    lo, hi = np.zeros((N, 4), dtype=np.uint64), np.zeros((N, 4), dtype=np.uint64)
    lo[:n1], hi[n2 - 1:] = ap, bp
    want = np.zeros_like(lo)
    reference.arr(curve, "arr_mont_add", N, lo, hi, want)
    got = gpu.poly_mul(curve, p, q)
    assert gpu.poly_last_mul_path() == (N - 1).bit_length() >= 17
    assert np.array_equal(got, want)
    # dense x dense: eval(p q, z) = eval(p, z) eval(q, z) at three points, all by the reference
    q = fr(gpu, curve, 33, n2)
    got = gpu.poly_mul(curve, p, q)
    for z in (fr(gpu, curve, 34, 1)[0], fe.to_row(fe.FR[curve] - 1, 4), gpu.get_fft_subgroup(curve, 20).gen_array()):
        lhs = ref_eval(reference, curve, got, z)
        rhs = ref_fr_mul(reference, curve, ref_eval(reference, curve, p, z), ref_eval(reference, curve, q, z))
        assert np.array_equal(lhs, rhs)


@pytest.mark.parametrize("curve", CURVES)
def test_long_times_short(hooks, reference, curve):
    gpu = hooks
    a, b = fr(gpu, curve, 41, (1 << 17) + 1), fr(gpu, curve, 42, 3)
    want = ref_mul(reference, curve, a, b)
    for mode, path in ((-1, None), (BIG, 0), (0, 18)):
        gpu.poly_set_mul_direct_max(mode)
        assert np.array_equal(gpu.poly_mul(curve, a, b), want), mode
        assert np.array_equal(gpu.poly_mul(curve, b, a), want), mode
        assert path is None or gpu.poly_last_mul_path() == path


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n1,n2", [(0, 1), (0, 5), (5, 0), (0, 0)])
def test_product_lengths_zero(gpu, reference, curve, n1, n2):
    """what the reference's loop writes (poly_mont.c:203-221), and nothing beyond it"""
    a, b = fr(gpu, curve, 51, max(n1, 1)), fr(gpu, curve, 52, max(n2, 1))
    want = np.full((8, 4), SENTINEL, dtype=np.uint64)
    got = want.copy()
    reference.arr(curve, "poly_mont_mul_naive", n1, a, n2, b, want)
    getattr(gpu.load(), f"{curve}_poly_mont_mul_naive")(n1, a.ctypes.data_as(U64P), n2, b.ctypes.data_as(U64P),
                                                       got.ctypes.data_as(U64P))
    assert np.array_equal(got, want)
    assert np.array_equal(gpu.poly_mul(curve, a[:n1], b[:n2]), want[:max(0, n1 + n2 - 1)])


# ---------------------------------------------------------------------------- evaluation
EVAL_N = [1, 2, 63, 64, 65, 255, 257, 1000, 4099, 65537, (1 << 20) + 1]


def eval_points(gpu, curve):
    r = fe.FR[curve]
    return [fe.to_row(0, 4), fe.to_row(fe.radix(r) % r, 4), fe.to_row(r - 1, 4), fr(gpu, curve, 61, 1)[0],
            gpu.get_fft_subgroup(curve, 10).gen_array()]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", EVAL_N)
def test_eval_at(gpu, reference, curve, n):
    p = edges(curve, n, rot=n)
    for x in eval_points(gpu, curve):
        assert np.array_equal(gpu.poly_eval_at(curve, p, x), ref_eval(reference, curve, p, x)), x
    if n in (65, 4099):
        p = fr(gpu, curve, 62, n)
        zero = np.zeros((n, 4), dtype=np.uint64)
        for x in eval_points(gpu, curve):
            assert np.array_equal(gpu.poly_eval_at(curve, p, x), ref_eval(reference, curve, p, x))
            assert not gpu.poly_eval_at(curve, zero, x).any()


@pytest.mark.parametrize("curve", CURVES)
def test_eval_device_and_empty(gpu, reference, curve):
    x = fr(gpu, curve, 63, 1)[0]
    assert not gpu.poly_eval_device(curve, 0, None, x).any()  # n = 0: the empty sum
    assert np.array_equal(gpu.poly_eval_at(curve, np.zeros((0, 4), dtype=np.uint64), x), ref_eval(
        reference, curve, np.zeros((1, 4), dtype=np.uint64)[:0], x))
    for n in (257, 4099, 65537):
        p = fr(gpu, curve, 64 + n, n)
        d = gpu.DeviceBuffer(p)
        try:
            assert np.array_equal(gpu.poly_eval_device(curve, n, d, x), ref_eval(reference, curve, p, x))
            assert np.array_equal(d.to_host(p), p)  # the operand is only read
        finally:
            d.free()


# ---------------------------------------------------------------------------- linear combination
def lincomb_cases(gpu, curve):
    r = fe.FR[curve]
    one, zero = fe.to_row(fe.radix(r) % r, 4), fe.to_row(0, 4)
    ragged = [1, 257, 64, 1000, 33, 999, 2, 300]
    ks = fr(gpu, curve, 71, 8)
    polys = [fr(gpu, curve, 72 + i, n) for i, n in enumerate(ragged)]
    cases = {f"K{K}": [(ks[i], polys[i]) for i in range(K)] for K in (1, 2, 5, 8)}  # the longest is not first
    cases["coeff_0_1"] = [(zero, polys[3]), (one, polys[1]), (ks[2], polys[5]), (one, polys[4]), (zero, polys[0])]
    cases["equal_lengths"] = [(ks[i], edges(curve, 300, rot=i)) for i in range(7)]
    cases["K70"] = [(ks[i % 8], polys[i % 8][:1 + (37 * i) % 200]) for i in range(70)]  # more than one LDS tile
    return cases


@pytest.mark.parametrize("curve", CURVES)
def test_lincomb(gpu, reference, curve):
    for name, terms in lincomb_cases(gpu, curve).items():
        assert np.array_equal(gpu.poly_lincomb(curve, terms), ref_lincomb(reference, curve, terms)), name
    out = np.full((2, 4), SENTINEL, dtype=np.uint64)  # K = 0 writes nothing
    getattr(gpu.load(), f"{curve}_poly_mont_lincomb")(0, None, None, None, out.ctypes.data_as(U64P))
    assert np.all(out == SENTINEL)


# ---------------------------------------------------------------------------- composed operations
@pytest.mark.parametrize("curve", CURVES)
def test_add_sub_neg_scale(gpu, reference, curve):
    r = fe.FR[curve]
    for n1, n2 in itertools.product([1, 33, 257, 1000], repeat=2):
        a, b = edges(curve, n1, rot=n2), fr(gpu, curve, 81 + n1, n2)
        for op, f in (("add", gpu.poly_add), ("sub", gpu.poly_sub)):
            want = np.zeros((max(n1, n2), 4), dtype=np.uint64)
            reference.arr(curve, "poly_mont_" + op, n1, a, n2, b, want)
            assert np.array_equal(f(curve, a, b), want), (op, n1, n2)
    for n in (1, 33, 257, 1000):
        a = edges(curve, n, rot=3)
        want = np.zeros_like(a)
        reference.arr(curve, "poly_mont_neg", n, a, want)
        assert np.array_equal(gpu.poly_neg(curve, a), want)
        for k in (fe.to_row(0, 4), fe.to_row(fe.radix(r) % r, 4), fr(gpu, curve, 82, 1)[0]):
            reference.arr(curve, "poly_mont_scale", k, n, a, want)
            assert np.array_equal(gpu.poly_scale(curve, k, a), want)


@pytest.mark.parametrize("curve", CURVES)
def test_predicates_and_degree(gpu, reference, curve):
    u8 = ctypes.c_uint8
    for n1, n2 in itertools.product([1, 33, 257, 1000], repeat=2):
        a = fr(gpu, curve, 91, max(n1, n2))
        zt = a.copy()
        zt[min(n1, n2):] = 0  # a zero tail: equal whatever the lengths
        for x, y in ((a[:n1], a[:n2]), (zt[:n1], zt[:n2]), (a[:n1], zt[:n2])):
            x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
            want = reference.arr(curve, "poly_mont_is_equal", n1, x, n2, y, restype=u8)
            assert gpu.poly_is_equal(curve, x, y) == bool(want), (n1, n2)
        d = a[:n1].copy()
        d[n1 // 2] = 0
        assert not gpu.poly_is_equal(curve, d, np.ascontiguousarray(a[:n1]))
    for n in (1, 33, 257, 1000, 70000):
        a = fr(gpu, curve, 92, n)
        for top in sorted({n - 1, n // 2, 0}):
            t = a.copy()
            t[top + 1:] = 0  # trailing zeros above `top`
            assert gpu.poly_degree(curve, t) == reference.arr(curve, "poly_mont_degree", n, t) == top
            assert not gpu.poly_is_zero(curve, t)
        z = np.zeros((n, 4), dtype=np.uint64)
        assert gpu.poly_degree(curve, z) == reference.arr(curve, "poly_mont_degree", n, z) == -1
        assert gpu.poly_is_zero(curve, z) and reference.arr(curve, "poly_mont_is_zero", n, z, restype=u8)
    empty = np.zeros((0, 4), dtype=np.uint64)
    assert gpu.poly_degree(curve, empty) == -1 and gpu.poly_is_zero(curve, empty)


# ---------------------------------------------------------------------------- device entries, errors
@pytest.mark.parametrize("curve", CURVES)
def test_device_entries(hooks, reference, curve):
    gpu = hooks
    for n1, n2 in [(33, 2), (1000, 257), (2049, 2047)]:
        a, b = fr(gpu, curve, 100 + n1, n1), fr(gpu, curve, 200 + n2, n2)
        want = ref_mul(reference, curve, a, b)
        da, db = gpu.DeviceBuffer(a), gpu.DeviceBuffer(b)
        dt = gpu.DeviceBuffer(np.full((n1 + n2, 4), SENTINEL, dtype=np.uint64))
        try:
            for mode in (-1, 0, BIG):
                gpu.poly_set_mul_direct_max(mode)
                assert gpu.poly_mul_device(curve, n1, da, n2, db, dt) == 0
                got = dt.to_host(np.zeros((n1 + n2, 4), dtype=np.uint64))
                assert np.array_equal(got[:-1], want) and np.all(got[-1] == SENTINEL), (n1, n2, mode)
            gpu.poly_set_mul_direct_max(0)  # squaring: the same buffer twice
            ds = gpu.DeviceBuffer.empty((2 * n1 - 1) * 32)
            assert gpu.poly_mul_device(curve, n1, da, n1, da, ds) == 0
            assert np.array_equal(ds.to_host(np.zeros((2 * n1 - 1, 4), dtype=np.uint64)), ref_mul(reference, curve, a, a))
            ds.free()
            assert np.array_equal(da.to_host(a), a) and np.array_equal(db.to_host(b), b)
        finally:
            for d in (da, db, dt):
                d.free()
    terms = lincomb_cases(gpu, curve)["K5"]
    bufs = [gpu.DeviceBuffer(p) for _, p in terms]
    want = ref_lincomb(reference, curve, terms)
    dt = gpu.DeviceBuffer(np.full((want.shape[0] + 1, 4), SENTINEL, dtype=np.uint64))
    try:
        gpu.poly_lincomb_device(curve, [p.shape[0] for _, p in terms], np.stack([k for k, _ in terms]), bufs, dt)
        got = dt.to_host(np.zeros((want.shape[0] + 1, 4), dtype=np.uint64))
        assert np.array_equal(got[:-1], want) and np.all(got[-1] == SENTINEL)
    finally:
        for d in bufs + [dt]:
            d.free()


def test_oversized_product_is_refused(gpu):
    """2^28 + 1 coefficients on BN128: -1 before anything is allocated or read (null operands)"""
    assert gpu.poly_mul_device("bn128", 1 << 28, None, 2, None, None) == -1
    assert gpu.poly_mul_device("bls12_381", 1 << 30, None, 2, None, None) == -1
    assert gpu.last_error() is None  # a return code, not an error


@pytest.mark.parametrize("curve", CURVES)
def test_workspace_refused_then_recovers(gpu, reference, curve):
    """the allocator's refusal only (tests/test_gpu_errors.py): an arena cap below the product's
    workspace makes the host symbol return with an error recorded; the next product succeeds"""
    gpu.set_error_mode(True)
    try:
        assert gpu.last_error() is None
        a, b = fr(gpu, curve, 111, 3000), fr(gpu, curve, 112, 2000)
        gpu.release()
        gpu.arena_set_limit(1 << 19)  # 4 x 2^13 x 32 B = 1 MiB of transform buffers do not fit
        gpu.poly_mul(curve, a, b)
        msg = gpu.last_error()
        assert msg is not None and "memory" in msg
        gpu.arena_set_limit(0)
        got = gpu.poly_mul(curve, a, b)
        assert gpu.last_error() is None
        assert np.array_equal(got, ref_mul(reference, curve, a, b))
    finally:
        gpu.set_error_mode(False)
        gpu.arena_set_limit(0)
        gpu.last_error()
