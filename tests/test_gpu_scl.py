"""Batch G1 scalar multiplication on the GPU (zk_scl.hip) against the reference's own generated C: the
expected row is <C>_G1_proj_scl_Fr_mont / _scl_Fr_std of the base followed by _normalize (projective output)
or _to_affine (affine output), compared bit for bit.  The reference multiplies by the integer value of the
scalar, so bases outside the order-r subgroup and scalars >= r are ordinary inputs here."""
import ctypes
import random
from types import SimpleNamespace

import numpy as np
import pytest

import golden_io

pytestmark = pytest.mark.gpu

CURVES = ("bn128", "bls12_381")
R = {"bn128": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
     "bls12_381": 52435875175126190479447740508185965837690552500527637822603658699938581184513}
BLS_P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
BLS_H = 0x396c8c005555e1568c00aaab0000aaab  # the G1 cofactor: #E(Fp) = BLS_H * r
FF = np.uint64(0xFFFFFFFFFFFFFFFF)
WINDOWS = (2, 4, 5, 8, 13, 16)


def words(k, n=4):
    return np.array([(k >> (64 * i)) & (2 ** 64 - 1) for i in range(n)], dtype=np.uint64)


def std_rows(ks):
    return np.ascontiguousarray(np.stack([words(k) for k in ks]))


def ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


class Ref:
    """the reference's G1 (and one G2) routines of one curve"""

    def __init__(self, reference, zk, curve):
        self.lib, self.curve, self.NP = reference.lib, curve, zk.NLIMBS_P[curve]

    def _f(self, name):
        return getattr(self.lib, f"{self.curve}_{name}")

    def proj(self, aff):
        out = np.zeros(3 * self.NP, dtype=np.uint64)
        self._f("G1_proj_from_affine")(ptr(np.ascontiguousarray(aff)), ptr(out))
        return out

    def scl(self, k, p, mont):
        out = np.zeros(3 * self.NP, dtype=np.uint64)
        self._f("G1_proj_scl_Fr_mont" if mont else "G1_proj_scl_Fr_std")(ptr(np.ascontiguousarray(k)), ptr(p), ptr(out))
        return out

    def scl_generic(self, k, p):
        kw = words(k, 8)
        out = np.zeros(3 * self.NP, dtype=np.uint64)
        self._f("G1_proj_scl_generic")(ptr(kw), ptr(p), ptr(out), 8)
        return out

    def normalize(self, p):
        out = np.zeros(3 * self.NP, dtype=np.uint64)
        self._f("G1_proj_normalize")(ptr(p), ptr(out))
        return out

    def to_affine(self, p):
        out = np.zeros(2 * self.NP, dtype=np.uint64)
        self._f("G1_proj_to_affine")(ptr(p), ptr(out))
        return out

    def expected(self, ks, bases, mont):
        """(normalised projective rows, affine rows) of [k_i] P_i; bases: one affine row, or one per scalar"""
        bases = np.asarray(bases)
        one = self.proj(bases) if bases.ndim == 1 else None
        pr = np.zeros((len(ks), 3 * self.NP), dtype=np.uint64)
        af = np.zeros((len(ks), 2 * self.NP), dtype=np.uint64)
        for i in range(len(ks)):
            q = self.scl(ks[i], one if one is not None else self.proj(bases[i]), mont)
            pr[i] = self.normalize(q)
            af[i] = self.to_affine(q)
        return pr, af


@pytest.fixture(scope="module")
def refs(reference, zk):
    return {c: Ref(reference, zk, c) for c in CURVES}


@pytest.fixture(scope="module")
def bases(gpu):
    return {c: gpu.gen_points(c, 0x5C10, 1)[0] for c in CURVES}


@pytest.fixture(scope="module")
def scalars(gpu, oracle):
    """1000 scalars per curve: Montgomery rows, and raw 256-bit integers (most of them >= r)"""
    rng = random.Random(0x5C11)
    return {c: {True: gpu.gen_fr(c, 0x5C12, 1000), False: std_rows([rng.getrandbits(256) for _ in range(1000)])}
            for c in CURVES}


@pytest.fixture(scope="module")
def fixed_expected(refs, bases, scalars):
    """the reference's rows for the 1000 scalars of `scalars` times the curve's base, computed once"""
    return {(c, mont): refs[c].expected(scalars[c][mont], bases[c], mont) for c in CURVES for mont in (True, False)}


@pytest.fixture
def hooks(gpu):
    try:
        yield gpu
    finally:
        gpu.scl_set_window(0)
        gpu.scl_set_fixed_min(-1)


def run_fixed(zk, curve, ks, base, mont, affine):
    """the device-resident entry; returns the rows"""
    n = ks.shape[0]
    like = np.zeros((n, (2 if affine else 3) * zk.NLIMBS_P[curve]), dtype=np.uint64)
    dk, dt = zk.DeviceBuffer(ks), zk.DeviceBuffer.empty(like.nbytes)
    try:
        assert zk.scalar_mul_fixed_device(curve, n, dk, base, dt, std=not mont, affine=affine) == 0
        return dt.to_host(like)
    finally:
        dk.free()
        dt.free()


@pytest.mark.parametrize("affine", [False, True], ids=["proj", "affine"])
@pytest.mark.parametrize("mont", [True, False], ids=["mont", "std"])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000])
@pytest.mark.parametrize("curve", CURVES)
def test_fixed_base_vs_reference(hooks, fixed_expected, bases, scalars, curve, n, mont, affine):
    zk = hooks
    zk.scl_set_fixed_min(0)
    got = run_fixed(zk, curve, scalars[curve][mont][:n], bases[curve], mont, affine)
    assert zk.scl_last_path() != 0
    assert np.array_equal(got, fixed_expected[(curve, mont)][1 if affine else 0][:n])


def edge_std(curve):
    r = R[curve]
    ks = [0, 1, 2, r - 1, r, r + 1, 2 ** 255, 2 ** 256 - 1, int.from_bytes(b"\x80" * 32, "little"),
          int.from_bytes(b"\x7f" * 32, "little")]
    a = 1
    while a * r < 2 ** 256:
        ks += [a * r + b for b in (-2, -1, 0, 1, 2) if a * r + b < 2 ** 256]
        a += 1
    return ks


@pytest.mark.parametrize("curve", CURVES)
def test_edge_scalars(hooks, refs, bases, oracle, curve):
    zk = hooks
    ks = std_rows(edge_std(curve))
    want = refs[curve].expected(ks, bases[curve], False)
    # the Montgomery forms of 0, 1, -1
    km = np.ascontiguousarray(zk.arr_from_std(curve, std_rows([0, 1, R[curve] - 1])))
    want_m = refs[curve].expected(km, bases[curve], True)
    for fixed_min in (0, 1 << 20):  # the table path, then the per-row kernel
        zk.scl_set_fixed_min(fixed_min)
        for affine in (False, True):
            assert np.array_equal(run_fixed(zk, curve, ks, bases[curve], False, affine), want[1 if affine else 0])
            assert (zk.scl_last_path() != 0) == (fixed_min == 0)
            assert np.array_equal(run_fixed(zk, curve, km, bases[curve], True, affine), want_m[1 if affine else 0])
    # 0 and r give infinity, whatever the path
    assert np.all(want[1][0] == FF) and np.all(want[1][4] == FF)


@pytest.mark.parametrize("curve", CURVES)
def test_window_independence(hooks, fixed_expected, bases, scalars, curve):
    zk = hooks
    zk.scl_set_fixed_min(0)
    ks = scalars[curve][False][:300]
    want = fixed_expected[(curve, False)][0][:300]
    for c in WINDOWS + (0,):
        zk.scl_set_window(c)
        got = run_fixed(zk, curve, ks, bases[curve], False, False)
        assert zk.scl_last_path() == c if c else zk.scl_last_path() != 0
        assert np.array_equal(got, want), c
    zk.scl_set_window(1)  # clamped
    run_fixed(zk, curve, ks[:3], bases[curve], False, False)
    assert zk.scl_last_path() == 2
    zk.scl_set_window(99)
    run_fixed(zk, curve, ks[:3], bases[curve], False, False)
    assert zk.scl_last_path() == 16


def bls_mont(x):
    return words((x << 384) % BLS_P, 6)


def bls_random_point(rng):
    """a random point of y^2 = x^3 + 4 over Fp (p = 3 mod 4), affine Montgomery row: almost surely of
    full order, outside the order-r subgroup"""
    while True:
        x = rng.randrange(BLS_P)
        y2 = (x * x * x + 4) % BLS_P
        y = pow(y2, (BLS_P + 1) // 4, BLS_P)
        if y * y % BLS_P == y2:
            return np.concatenate([bls_mont(x), bls_mont(y)])


def bls_small_order_point(ref, rng, q):
    """a point of order q (q a prime that divides the cofactor): a random point times h r without its
    factors q, stepped by q until the next step is infinity; retried while that gives infinity at once.
    (E(Fp) is not cyclic -- its 11-part is Z/11 x Z/11 -- so [h r / 11] alone sends every point to infinity.)"""
    m = BLS_H * R["bls12_381"]
    assert m % q == 0
    while m % q == 0:
        m //= q
    for _ in range(64):
        p = ref.to_affine(ref.scl_generic(m, ref.proj(bls_random_point(rng))))
        while not np.all(p == FF):
            nxt = ref.to_affine(ref.scl_generic(q, ref.proj(p)))
            if np.all(nxt == FF):
                return p
            p = nxt
    raise AssertionError(f"no point of order {q} found")


@pytest.mark.parametrize("kind", ["full", "order3", "order11"])
def test_bls_bases_outside_the_subgroup(hooks, refs, reference, kind):
    zk, ref, curve = hooks, refs["bls12_381"], "bls12_381"
    rng = random.Random({"full": 1, "order3": 3, "order11": 11}[kind])
    base = bls_random_point(rng) if kind == "full" else bls_small_order_point(ref, rng, int(kind[5:]))
    on_curve = getattr(reference.lib, "bls12_381_G1_proj_is_on_curve")
    on_curve.restype = ctypes.c_uint8
    assert on_curve(ptr(ref.proj(base)))
    if kind == "full":  # outside the order-r subgroup: [r] P is not infinity (a point of order 3 or 11 is by its order)
        assert not np.all(ref.to_affine(ref.scl_generic(R[curve], ref.proj(base))) == FF)
    ks = [rng.getrandbits(256) for _ in range(257)]
    if kind == "order3":
        # The reference's 4-bit table holds 6 P = dbl(3 P) = dbl(infinity), which its doubling turns into
        # (0 : 0 : 0); that triple absorbs every sum, so a scalar with a hex digit 6, 7 or c..f gives
        # infinity (all 257 random ones do) and any other scalar the true multiple: 200 of those as well.
        ok = (0, 1, 2, 3, 4, 5, 8, 9, 10, 11)
        ks += [sum(rng.choice(ok) << (4 * i) for i in range(rng.randrange(1, 65))) for _ in range(200)]
    ks = std_rows(ks)
    want = ref.expected(ks, base, False)
    if kind != "full":  # small order: infinity rows among the results (and in the table), and finite ones
        inf_rows = np.all(want[1] == FF, axis=1)
        assert np.any(inf_rows) and not np.all(inf_rows)
    zk.scl_set_fixed_min(0)
    for c in (0, 4):
        zk.scl_set_window(c)
        assert np.array_equal(run_fixed(zk, curve, ks, base, False, False), want[0]), c
        assert zk.scl_last_path() != 0
    assert np.array_equal(run_fixed(zk, curve, ks, base, False, True), want[1])
    zk.scl_set_fixed_min(1 << 20)
    assert np.array_equal(run_fixed(zk, curve, ks, base, False, True), want[1])
    assert zk.scl_last_path() == 0


@pytest.mark.parametrize("curve", CURVES)
def test_base_at_infinity(hooks, scalars, curve):
    zk = hooks
    NP = zk.NLIMBS_P[curve]
    inf = np.full(2 * NP, FF, dtype=np.uint64)
    ks = scalars[curve][True][:257]
    one = zk.batch_from_affine(curve, zk.gen_points(curve, 1, 1))[0, 2 * NP:]  # Montgomery 1
    proj_inf = np.concatenate([np.zeros(NP, np.uint64), one, np.zeros(NP, np.uint64)])
    for fixed_min in (0, 1 << 20):
        zk.scl_set_fixed_min(fixed_min)
        got = run_fixed(zk, curve, ks, inf, True, False)
        assert np.array_equal(got, np.tile(proj_inf, (257, 1)))
        assert np.all(run_fixed(zk, curve, ks, inf, True, True) == FF)


def mixed_bases(zk, curve, n, rng):
    """n distinct affine rows with infinity rows and (BLS12-381) rows outside the subgroup mixed in"""
    b = zk.gen_points(curve, 0x5C13, n).copy()
    for i in range(0, n, 37):
        b[i] = FF
    if curve == "bls12_381":
        for i in range(5, n, 41):
            b[i] = bls_random_point(rng)
    return b


@pytest.fixture(scope="module")
def rows_case(gpu, refs, scalars):
    out = {}
    for c in CURVES:
        b = mixed_bases(gpu, c, 1000, random.Random(0x5C14))
        out[c] = (b, {mont: refs[c].expected(scalars[c][mont], b, mont) for mont in (True, False)})
    return out


@pytest.mark.parametrize("mont", [True, False], ids=["mont", "std"])
@pytest.mark.parametrize("n", [1, 257, 1000])
@pytest.mark.parametrize("curve", CURVES)
def test_per_row_bases_vs_reference(gpu, rows_case, scalars, curve, n, mont):
    zk = gpu
    b, want = rows_case[curve]
    if n == 1:  # row 0 is an infinity row: take a finite one
        sl = slice(1, 2)
    else:
        sl = slice(0, n)
    ks, bs = np.ascontiguousarray(scalars[curve][mont][sl]), np.ascontiguousarray(b[sl])
    for affine in (False, True):
        like = np.zeros((ks.shape[0], (2 if affine else 3) * zk.NLIMBS_P[curve]), dtype=np.uint64)
        dk, db, dt = zk.DeviceBuffer(ks), zk.DeviceBuffer(bs), zk.DeviceBuffer.empty(like.nbytes)
        try:
            assert zk.scalar_mul_rows_device(curve, ks.shape[0], dk, db, dt, std=not mont, affine=affine) == 0
            got = dt.to_host(like)
            assert np.array_equal(db.to_host(bs), bs) and np.array_equal(dk.to_host(ks), ks)
        finally:
            for d in (dk, db, dt):
                d.free()
        assert np.array_equal(got, want[mont][1 if affine else 0][sl])
        # the host form
        assert np.array_equal(zk.scalar_mul_rows(curve, ks, bs, std=not mont, affine=affine), got)


@pytest.mark.parametrize("curve", CURVES)
def test_fixed_base_below_the_crossover_takes_the_per_row_kernel(hooks, fixed_expected, bases, scalars, curve):
    zk = hooks
    for n in (1, 257, 1000):
        for mont in (True, False):
            ks = scalars[curve][mont][:n]
            zk.scl_set_fixed_min(n + 1)
            rows = run_fixed(zk, curve, ks, bases[curve], mont, False)
            assert zk.scl_last_path() == 0
            zk.scl_set_fixed_min(n)
            table = run_fixed(zk, curve, ks, bases[curve], mont, False)
            assert zk.scl_last_path() != 0
            assert np.array_equal(rows, table)
            assert np.array_equal(rows, fixed_expected[(curve, mont)][0][:n])


@pytest.mark.parametrize("curve", CURVES)
def test_powers(hooks, refs, oracle, bases, curve):
    zk, ref = hooks, refs[curve]
    NP = zk.NLIMBS_P[curve]
    n = 300
    a, tau = zk.gen_fr(curve, 0x5C15, 2)
    one = zk.arr_from_std(curve, std_rows([1]))[0]
    zero = np.zeros(4, dtype=np.uint64)
    like = np.zeros((n, 3 * NP), dtype=np.uint64)
    for ka, kt in ((a, tau), (a, zero), (a, one), (None, tau)):
        ks = oracle.arr_powers(curve, ka if ka is not None else one, kt, n)
        want = ref.expected(ks, bases[curve], True)
        if kt is zero:  # row 0 is [a] P, the rest infinity
            assert np.array_equal(ks[0], a) and not np.any(ks[1:])
            assert np.all(want[1][1:] == FF) and not np.all(want[1][0] == FF)
        for fixed_min in (0, 1 << 20):
            zk.scl_set_fixed_min(fixed_min)
            dt = zk.DeviceBuffer.empty(like.nbytes)
            try:
                assert zk.srs_powers_device(curve, n, kt, bases[curve], dt, a=ka) == 0
                assert np.array_equal(dt.to_host(like), want[0])
            finally:
                dt.free()
            assert (zk.scl_last_path() != 0) == (fixed_min == 0)
        assert np.array_equal(zk.srs_powers(curve, kt, n, bases[curve], a=ka, affine=True), want[1])


@pytest.mark.parametrize("curve", CURVES)
def test_kzg_setup(gpu, refs, reference, oracle, bases, curve):
    zk, ref = gpu, refs[curve]
    NP = zk.NLIMBS_P[curve]
    m, n = 6, 64
    tau = zk.gen_fr(curve, 0x5C16, 1)[0]
    g1 = bases[curve]
    g2 = golden_io.g2_points(reference.lib, curve, 1)[0]
    setup = zk.kzg_setup(curve, tau, m, g1, g2)
    try:
        like = np.zeros((n, 3 * NP), dtype=np.uint64)
        one = zk.arr_from_std(curve, std_rows([1]))[0]
        # tauG1s: acc <**> g1 with acc = tau^i, as `taus` steps it
        taus = ref.expected(oracle.arr_powers(curve, one, tau, n), g1, True)[0]
        assert np.array_equal(setup.tau_g1s.to_host(like), taus)
        want = np.zeros_like(like)
        getattr(reference.lib, f"{curve}_G1_proj_fft_inverse")(m, ptr(setup.domain.gen_array()), ptr(taus), ptr(want))
        assert np.array_equal(setup.lagrange_taus.to_host(like), want)
        g2p, t2, t2n = (np.zeros(6 * NP, dtype=np.uint64) for _ in range(3))
        getattr(reference.lib, f"{curve}_G2_proj_from_affine")(ptr(g2), ptr(g2p))
        getattr(reference.lib, f"{curve}_G2_proj_scl_Fr_mont")(ptr(tau), ptr(g2p), ptr(t2))
        getattr(reference.lib, f"{curve}_G2_proj_normalize")(ptr(t2), ptr(t2n))
        assert np.array_equal(setup.g2_tau_g2[0], g2)
        assert np.array_equal(setup.g2_tau_g2[1], t2n)
    finally:
        setup.free()


@pytest.mark.parametrize("curve", CURVES)
def test_guards(hooks, fixed_expected, bases, scalars, curve):
    """nothing outside rows [0, n) is written, inputs stay, n = 0 and n = -1 write nothing, host = device"""
    zk = hooks
    NP = zk.NLIMBS_P[curve]
    n = 257
    ks = scalars[curve][True][:n]
    b = np.ascontiguousarray(np.tile(bases[curve], (n, 1)))
    for affine in (False, True):
        rw = (2 if affine else 3) * NP
        want = fixed_expected[(curve, True)][1 if affine else 0][:n]
        poison = np.full((n + 2, rw), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        calls = {
            "table": lambda k, t, cnt: zk.scalar_mul_fixed_device(curve, cnt, k, bases[curve], t, affine=affine),
            "rows": lambda k, t, cnt: zk.scalar_mul_rows_device(curve, cnt, k, db, t, affine=affine),
            "powers": lambda k, t, cnt: zk.srs_powers_device(curve, cnt, ks[1], bases[curve], t, a=ks[0], affine=affine),
        }
        for name, call in calls.items():
            zk.scl_set_fixed_min(0)
            dk, db, dt = zk.DeviceBuffer(ks), zk.DeviceBuffer(b), zk.DeviceBuffer(poison)
            inner = SimpleNamespace(ptr=dt.ptr + rw * 8)
            try:
                assert call(dk, inner, 0) == 0  # n = 0: nothing written
                assert call(dk, inner, -1) == -1
                assert np.array_equal(dt.to_host(poison), poison)
                assert call(dk, inner, n) == 0
                got = dt.to_host(poison)
                assert np.array_equal(dk.to_host(ks), ks) and np.array_equal(db.to_host(b), b)
            finally:
                for d in (dk, db, dt):
                    d.free()
            assert np.array_equal(got[0], poison[0]) and np.array_equal(got[-1], poison[-1]), name
            if name != "powers":
                assert np.array_equal(got[1:-1], want), name
    # the host forms equal the device forms (and so the reference)
    for mont in (True, False):
        for affine in (False, True):
            zk.scl_set_fixed_min(0)
            h = zk.scalar_mul_fixed(curve, scalars[curve][mont][:n], bases[curve], std=not mont, affine=affine)
            assert np.array_equal(h, fixed_expected[(curve, mont)][1 if affine else 0][:n])
            # the default route of a short call: host arrays through the per-row kernel
            zk.scl_set_fixed_min(n + 1)
            assert np.array_equal(zk.scalar_mul_fixed(curve, scalars[curve][mont][:n], bases[curve], std=not mont,
                                                      affine=affine), h)
            assert zk.scl_last_path() == 0
    assert zk.load().zkg_g1_scl_fixed(zk.CURVE_ID[curve], 0, None, 1, zk._p(bases[curve]), 0, None) == 0
    with pytest.raises(ValueError):
        zk.scalar_mul_rows(curve, ks, b[:-1])
