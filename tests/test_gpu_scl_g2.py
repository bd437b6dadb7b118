"""Batch G2 scalar multiplication on the GPU (zk_scl_g2_bn.hip / zk_scl_g2_bls.hip) against the reference's own
generated C: the expected row is <C>_G2_proj_scl_Fr_mont / _scl_Fr_std of the base followed by _normalize
(projective output) or _to_affine (affine output), compared bit for bit.  The reference multiplies by the
integer value of the scalar, so bases outside the order-r subgroup of the twist and scalars >= r are
ordinary inputs here.  A base of order 13 makes the table path meet acc == row (the doubling branch of the
Fp2 mixed addition), acc == -row and infinity rows on random scalars, as the a r + b scalars do on a
subgroup base."""
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
# the cofactor of the BLS12-381 twist y^2 = x^3 + 4 (1 + u): #E'(Fp2) = BLS_H2 * r, BLS_H2 = 13^2 23^2 2713 11953 ...
BLS_H2 = int("5d543a95414e7f1091d50792876a202cd91de4547085abaa68a205b2e5a7ddfa628f1cb4d9e82ef21537e293a6691ae"
             "1616ec6e786f0c70cf1c38e31c7238e5", 16)
FF = np.uint64(0xFFFFFFFFFFFFFFFF)
WINDOWS = (2, 4, 5, 8, 13, 16)
NS = 600  # scalars per (curve, form): the reference's G2 multiplication takes 2 to 3 ms


def words(k, n=4):
    return np.array([(k >> (64 * i)) & (2 ** 64 - 1) for i in range(n)], dtype=np.uint64)


def std_rows(ks):
    return np.ascontiguousarray(np.stack([words(k) for k in ks]))


def ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


class Ref:
    """the reference's G2 routines of one curve; NP: the words of an Fp2 element"""

    def __init__(self, reference, zk, curve):
        self.lib, self.curve, self.NP = reference.lib, curve, 2 * zk.NLIMBS_P[curve]

    def _f(self, name):
        return getattr(self.lib, f"{self.curve}_G2_proj_{name}")

    def proj(self, aff):
        out = np.zeros(3 * self.NP, dtype=np.uint64)
        self._f("from_affine")(ptr(np.ascontiguousarray(aff)), ptr(out))
        return out

    def scl(self, k, p, mont):
        out = np.zeros(3 * self.NP, dtype=np.uint64)
        self._f("scl_Fr_mont" if mont else "scl_Fr_std")(ptr(np.ascontiguousarray(k)), ptr(p), ptr(out))
        return out

    def scl_generic(self, k, p):
        kw = words(k, 16)
        out = np.zeros(3 * self.NP, dtype=np.uint64)
        self._f("scl_generic")(ptr(kw), ptr(p), ptr(out), 16)
        return out

    def normalize(self, p):
        out = np.zeros(3 * self.NP, dtype=np.uint64)
        self._f("normalize")(ptr(p), ptr(out))
        return out

    def to_affine(self, p):
        out = np.zeros(2 * self.NP, dtype=np.uint64)
        self._f("to_affine")(ptr(p), ptr(out))
        return out

    def is_on_curve(self, p):
        f = self._f("is_on_curve")
        f.restype = ctypes.c_uint8
        return f(ptr(p)) != 0

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
def points(reference):
    """600 distinct affine G2 rows of the subgroup per curve; row 0 is the fixed base"""
    return {c: golden_io.g2_points(reference.lib, c, NS, k0=0x6C10, k1=0x6C11) for c in CURVES}


@pytest.fixture(scope="module")
def bases(points):
    return {c: points[c][0].copy() for c in CURVES}


@pytest.fixture(scope="module")
def scalars(gpu):
    """600 scalars per curve: Montgomery rows, and raw 256-bit integers (most of them >= r)"""
    rng = random.Random(0x6C12)
    return {c: {True: gpu.gen_fr(c, 0x6C13, NS), False: std_rows([rng.getrandbits(256) for _ in range(NS)])}
            for c in CURVES}


@pytest.fixture(scope="module")
def fixed_expected(refs, bases, scalars):
    """the reference's rows for the 600 scalars of `scalars` times the curve's base, computed once"""
    return {(c, mont): refs[c].expected(scalars[c][mont], bases[c], mont) for c in CURVES for mont in (True, False)}


@pytest.fixture
def hooks(gpu):
    try:
        yield gpu
    finally:
        gpu.g2_scl_set_window(0)
        gpu.g2_scl_set_fixed_min(-1)


def run_fixed(zk, curve, ks, base, mont, affine):
    """the device-resident entry; returns the rows"""
    n = ks.shape[0]
    like = np.zeros((n, (4 if affine else 6) * zk.NLIMBS_P[curve]), dtype=np.uint64)
    dk, dt = zk.DeviceBuffer(ks), zk.DeviceBuffer.empty(like.nbytes)
    try:
        assert zk.g2_scalar_mul_fixed_device(curve, n, dk, base, dt, std=not mont, affine=affine) == 0
        return dt.to_host(like)
    finally:
        dk.free()
        dt.free()


@pytest.mark.parametrize("affine", [False, True], ids=["proj", "affine"])
@pytest.mark.parametrize("mont", [True, False], ids=["mont", "std"])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, NS])
@pytest.mark.parametrize("curve", CURVES)
def test_fixed_base_vs_reference(hooks, fixed_expected, bases, scalars, curve, n, mont, affine):
    zk = hooks
    zk.g2_scl_set_fixed_min(0)
    got = run_fixed(zk, curve, scalars[curve][mont][:n], bases[curve], mont, affine)
    assert zk.g2_scl_last_path() != 0
    assert np.array_equal(got, fixed_expected[(curve, mont)][1 if affine else 0][:n])


def edge_std(curve):
    r = R[curve]
    ks = [0, 1, 2, r - 1, r, r + 1, 2 ** 255, 2 ** 256 - 1]
    a = 1
    while a * r < 2 ** 256:
        ks += [a * r + b for b in (-2, -1, 0, 1, 2) if a * r + b < 2 ** 256]
        a += 1
    return ks


@pytest.mark.parametrize("curve", CURVES)
def test_edge_scalars(hooks, refs, bases, curve):
    zk = hooks
    ks = std_rows(edge_std(curve))
    want = refs[curve].expected(ks, bases[curve], False)
    # the Montgomery forms of 0, 1, -1
    km = np.ascontiguousarray(zk.arr_from_std(curve, std_rows([0, 1, R[curve] - 1])))
    want_m = refs[curve].expected(km, bases[curve], True)
    for fixed_min in (0, 1 << 20):  # the table path, then the per-row kernel
        zk.g2_scl_set_fixed_min(fixed_min)
        for affine in (False, True):
            assert np.array_equal(run_fixed(zk, curve, ks, bases[curve], False, affine), want[1 if affine else 0])
            assert (zk.g2_scl_last_path() != 0) == (fixed_min == 0)
            assert np.array_equal(run_fixed(zk, curve, km, bases[curve], True, affine), want_m[1 if affine else 0])
    # 0 and r give infinity, whatever the path
    assert np.all(want[1][0] == FF) and np.all(want[1][4] == FF)


@pytest.mark.parametrize("curve", CURVES)
def test_window_independence(hooks, fixed_expected, bases, scalars, curve):
    zk = hooks
    zk.g2_scl_set_fixed_min(0)
    ks = scalars[curve][False][:300]
    want = fixed_expected[(curve, False)][0][:300]
    for c in WINDOWS + (0,):
        zk.g2_scl_set_window(c)
        got = run_fixed(zk, curve, ks, bases[curve], False, False)
        assert zk.g2_scl_last_path() == c if c else zk.g2_scl_last_path() != 0
        assert np.array_equal(got, want), c
    zk.g2_scl_set_window(1)  # clamped
    run_fixed(zk, curve, ks[:3], bases[curve], False, False)
    assert zk.g2_scl_last_path() == 2
    zk.g2_scl_set_window(99)
    run_fixed(zk, curve, ks[:3], bases[curve], False, False)
    assert zk.g2_scl_last_path() == 16


def test_the_g1_hooks_are_a_separate_state(hooks, bases, scalars):
    zk = hooks
    zk.scl_set_window(4)
    zk.scl_set_fixed_min(0)
    try:
        zk.g2_scl_set_fixed_min(1 << 20)
        run_fixed(zk, "bn128", scalars["bn128"][True][:3], bases["bn128"], True, False)
        assert zk.g2_scl_last_path() == 0
        zk.g2_scl_set_fixed_min(0)
        zk.g2_scl_set_window(5)
        run_fixed(zk, "bn128", scalars["bn128"][True][:3], bases["bn128"], True, False)
        assert zk.g2_scl_last_path() == 5
    finally:
        zk.scl_set_window(0)
        zk.scl_set_fixed_min(-1)


# ---------------------------------------------------------------------------- BLS12-381 twist points

def bls_mont(x):
    return words((x << 384) % BLS_P, 6)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % BLS_P, (a[0] * b[1] + a[1] * b[0]) % BLS_P)


def fp_sqrt(a):
    s = pow(a, (BLS_P + 1) // 4, BLS_P)  # p = 3 mod 4
    return s if s * s % BLS_P == a % BLS_P else None


def f2_sqrt(a):
    """a square root in Fp[u] / (u^2 + 1), or None: x0^2 = (a0 +- |a|) / 2, x1 = a1 / (2 x0)"""
    a0, a1 = a
    if a1 == 0:
        s = fp_sqrt(a0)
        if s is not None:
            return (s, 0)
        s = fp_sqrt(-a0 % BLS_P)
        return None if s is None else (0, s)
    n = fp_sqrt((a0 * a0 + a1 * a1) % BLS_P)
    if n is None:
        return None
    for d in ((a0 + n) * (BLS_P + 1) // 2 % BLS_P, (a0 - n) * (BLS_P + 1) // 2 % BLS_P):
        x0 = fp_sqrt(d)
        if x0:
            x1 = a1 * pow(2 * x0, BLS_P - 2, BLS_P) % BLS_P
            if f2_mul((x0, x1), (x0, x1)) == (a0, a1):
                return (x0, x1)
    return None


def bls_random_twist_point(rng):
    """a random point of y^2 = x^3 + 4 (1 + u) over Fp2, affine Montgomery row: almost surely of full
    order, outside the order-r subgroup"""
    while True:
        x = (rng.randrange(BLS_P), rng.randrange(BLS_P))
        x3 = f2_mul(f2_mul(x, x), x)
        y = f2_sqrt(((x3[0] + 4) % BLS_P, (x3[1] + 4) % BLS_P))
        if y is not None:
            return np.concatenate([bls_mont(x[0]), bls_mont(x[1]), bls_mont(y[0]), bls_mont(y[1])])


def bls_small_order_twist_point(ref, rng, q):
    """a point of order q (q a prime that divides the twist's cofactor): a random point times h2 r without
    its factors q, stepped by q until the next step is infinity; retried while that gives infinity at once
    (the q-part of the group may not be cyclic)"""
    m = BLS_H2 * R["bls12_381"]
    assert m % q == 0
    while m % q == 0:
        m //= q
    for _ in range(64):
        p = ref.to_affine(ref.scl_generic(m, ref.proj(bls_random_twist_point(rng))))
        while not np.all(p == FF):
            nxt = ref.to_affine(ref.scl_generic(q, ref.proj(p)))
            if np.all(nxt == FF):
                return p
            p = nxt
    raise AssertionError(f"no point of order {q} found")


@pytest.mark.parametrize("kind", ["full", "order13", "order23"])
def test_bls_bases_outside_the_subgroup(hooks, refs, kind):
    """order 13: infinity rows in the table and in the per-lane table (INF_ROWS), and acc == +-row on random
    scalars; order 23: infinity rows in the table for c >= 6 only, none in the per-lane table.  The
    reference returns the true multiple for both (its table doubles d P, d <= 7, only)."""
    zk, ref, curve = hooks, refs["bls12_381"], "bls12_381"
    rng = random.Random({"full": 1, "order13": 13, "order23": 23}[kind])
    base = bls_random_twist_point(rng) if kind == "full" else bls_small_order_twist_point(ref, rng, int(kind[5:]))
    assert ref.is_on_curve(ref.proj(base))
    if kind == "full":  # outside the order-r subgroup: [r] P is not infinity
        assert not np.all(ref.to_affine(ref.scl_generic(R[curve], ref.proj(base))) == FF)
    ks = [rng.getrandbits(256) for _ in range(257)]
    want = ref.expected(std_rows(ks), base, False)
    if kind != "full":  # small order: infinity rows among the results (and in the table), and finite ones
        q = int(kind[5:])
        inf_rows = np.all(want[1] == FF, axis=1)
        assert np.any(inf_rows) and not np.all(inf_rows)
        assert [bool(x) for x in inf_rows] == [k % q == 0 for k in ks]  # the group's multiple, no absorption
    ks = std_rows(ks)
    zk.g2_scl_set_fixed_min(0)
    for c in (0, 4):
        zk.g2_scl_set_window(c)
        assert np.array_equal(run_fixed(zk, curve, ks, base, False, False), want[0]), c
        assert zk.g2_scl_last_path() != 0
    assert np.array_equal(run_fixed(zk, curve, ks, base, False, True), want[1])
    zk.g2_scl_set_fixed_min(1 << 20)
    assert np.array_equal(run_fixed(zk, curve, ks, base, False, True), want[1])
    assert zk.g2_scl_last_path() == 0


@pytest.mark.parametrize("curve", CURVES)
def test_base_at_infinity(hooks, refs, scalars, curve):
    zk = hooks
    NP = 2 * zk.NLIMBS_P[curve]
    inf = np.full(2 * NP, FF, dtype=np.uint64)
    ks = scalars[curve][True][:257]
    proj_inf = refs[curve].normalize(refs[curve].scl(ks[0], refs[curve].proj(inf), True))  # (0 : 1 : 0)
    assert not np.any(proj_inf[:NP]) and not np.any(proj_inf[2 * NP:]) and np.any(proj_inf[NP:2 * NP])
    for fixed_min in (0, 1 << 20):
        zk.g2_scl_set_fixed_min(fixed_min)
        got = run_fixed(zk, curve, ks, inf, True, False)
        assert np.array_equal(got, np.tile(proj_inf, (257, 1)))
        assert np.all(run_fixed(zk, curve, ks, inf, True, True) == FF)


@pytest.fixture(scope="module")
def rows_case(refs, points, scalars):
    """600 distinct affine rows per curve with infinity rows in every 37th place and (BLS12-381) rows outside
    the subgroup in every 41st, and the reference's rows for them"""
    out = {}
    for c in CURVES:
        b = points[c].copy()
        rng = random.Random(0x6C14)
        b[0::37] = FF
        if c == "bls12_381":
            for i in range(5, NS, 41):
                b[i] = bls_random_twist_point(rng)
        out[c] = (b, {mont: refs[c].expected(scalars[c][mont], b, mont) for mont in (True, False)})
    return out


@pytest.mark.parametrize("mont", [True, False], ids=["mont", "std"])
@pytest.mark.parametrize("n", [1, 257, NS])
@pytest.mark.parametrize("curve", CURVES)
def test_per_row_bases_vs_reference(gpu, rows_case, scalars, curve, n, mont):
    zk = gpu
    b, want = rows_case[curve]
    sl = slice(1, 2) if n == 1 else slice(0, n)  # row 0 is an infinity row: n = 1 takes a finite one
    ks, bs = np.ascontiguousarray(scalars[curve][mont][sl]), np.ascontiguousarray(b[sl])
    for affine in (False, True):
        like = np.zeros((ks.shape[0], (4 if affine else 6) * zk.NLIMBS_P[curve]), dtype=np.uint64)
        dk, db, dt = zk.DeviceBuffer(ks), zk.DeviceBuffer(bs), zk.DeviceBuffer.empty(like.nbytes)
        try:
            assert zk.g2_scalar_mul_rows_device(curve, ks.shape[0], dk, db, dt, std=not mont, affine=affine) == 0
            got = dt.to_host(like)
            assert np.array_equal(db.to_host(bs), bs) and np.array_equal(dk.to_host(ks), ks)
        finally:
            for d in (dk, db, dt):
                d.free()
        assert np.array_equal(got, want[mont][1 if affine else 0][sl])
        # the host form
        assert np.array_equal(zk.g2_scalar_mul_rows(curve, ks, bs, std=not mont, affine=affine), got)


@pytest.mark.parametrize("curve", CURVES)
def test_fixed_base_below_the_crossover_takes_the_per_row_kernel(hooks, fixed_expected, bases, scalars, curve):
    zk = hooks
    for n in (1, 257, NS):
        for mont in (True, False):
            ks = scalars[curve][mont][:n]
            zk.g2_scl_set_fixed_min(n + 1)
            rows = run_fixed(zk, curve, ks, bases[curve], mont, False)
            assert zk.g2_scl_last_path() == 0
            zk.g2_scl_set_fixed_min(n)
            table = run_fixed(zk, curve, ks, bases[curve], mont, False)
            assert zk.g2_scl_last_path() != 0
            assert np.array_equal(rows, table)
            assert np.array_equal(rows, fixed_expected[(curve, mont)][0][:n])


@pytest.mark.parametrize("curve", CURVES)
def test_powers(hooks, refs, oracle, bases, curve):
    zk, ref = hooks, refs[curve]
    NP = 2 * zk.NLIMBS_P[curve]
    n = 300
    a, tau = zk.gen_fr(curve, 0x6C15, 2)
    one = zk.arr_from_std(curve, std_rows([1]))[0]
    zero = np.zeros(4, dtype=np.uint64)
    like = np.zeros((n, 3 * NP), dtype=np.uint64)
    for ka, kt in ((a, tau), (a, zero), (a, one), (None, tau)):
        ks = oracle.arr_powers(curve, ka if ka is not None else one, kt, n)
        if kt is zero or kt is one:  # one distinct scalar besides 0: one reference row each
            first = ref.expected(ks[:2], bases[curve], True)
            want = tuple(np.concatenate([w[:1], np.tile(w[1], (n - 1, 1))]) for w in first)
            assert np.array_equal(ks[2:], np.tile(ks[1], (n - 2, 1)))
        else:
            want = ref.expected(ks, bases[curve], True)
        if kt is zero:  # row 0 is [a] P, the rest infinity
            assert np.array_equal(ks[0], a) and not np.any(ks[1:])
            assert np.all(want[1][1:] == FF) and not np.all(want[1][0] == FF)
        for fixed_min in (0, 1 << 20):
            zk.g2_scl_set_fixed_min(fixed_min)
            dt = zk.DeviceBuffer.empty(like.nbytes)
            try:
                assert zk.g2_srs_powers_device(curve, n, kt, bases[curve], dt, a=ka) == 0
                assert np.array_equal(dt.to_host(like), want[0])
            finally:
                dt.free()
            assert (zk.g2_scl_last_path() != 0) == (fixed_min == 0)
        assert np.array_equal(zk.g2_srs_powers(curve, kt, n, bases[curve], a=ka, affine=True), want[1])


@pytest.mark.parametrize("curve", CURVES)
def test_kzg_setup_with_g2_powers(gpu, refs, oracle, bases, curve):
    zk, ref = gpu, refs[curve]
    NP1 = zk.NLIMBS_P[curve]
    m, n, k = 6, 64, 8
    tau = zk.gen_fr(curve, 0x6C16, 1)[0]
    g1 = zk.gen_points(curve, 0x6C17, 1)[0]
    g2 = bases[curve]
    plain = zk.kzg_setup(curve, tau, m, g1, g2)
    setup = zk.kzg_setup(curve, tau, m, g1, g2, g2_powers=k)
    try:
        assert plain.tau_g2s is None
        one = zk.arr_from_std(curve, std_rows([1]))[0]
        want = ref.expected(oracle.arr_powers(curve, one, tau, k), g2, True)[0]
        got = setup.tau_g2s.to_host(np.zeros((k, 6 * NP1), dtype=np.uint64))
        assert np.array_equal(got, want)
        assert np.array_equal(got[1], setup.g2_tau_g2[1])
        # every other field is as in the default call
        like = np.zeros((n, 3 * NP1), dtype=np.uint64)
        assert np.array_equal(setup.tau_g1s.to_host(like), plain.tau_g1s.to_host(like))
        assert np.array_equal(setup.lagrange_taus.to_host(like), plain.lagrange_taus.to_host(like))
        assert np.array_equal(setup.g2_tau_g2[0], plain.g2_tau_g2[0]) and np.array_equal(setup.g2_tau_g2[0], g2)
        assert np.array_equal(setup.g2_tau_g2[1], plain.g2_tau_g2[1])
        assert setup.domain.size == plain.domain.size == n
    finally:
        plain.free()
        setup.free()


@pytest.mark.parametrize("curve", CURVES)
def test_guards(hooks, fixed_expected, bases, scalars, curve):
    """nothing outside rows [0, n) is written, inputs stay, n = 0 and n = -1 write nothing, host = device"""
    zk = hooks
    NP = 2 * zk.NLIMBS_P[curve]
    n = 257
    ks = scalars[curve][True][:n]
    b = np.ascontiguousarray(np.tile(bases[curve], (n, 1)))
    for affine in (False, True):
        rw = (2 if affine else 3) * NP
        want = fixed_expected[(curve, True)][1 if affine else 0][:n]
        poison = np.full((n + 2, rw), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        calls = {
            "table": lambda k, t, cnt: zk.g2_scalar_mul_fixed_device(curve, cnt, k, bases[curve], t, affine=affine),
            "rows": lambda k, t, cnt: zk.g2_scalar_mul_rows_device(curve, cnt, k, db, t, affine=affine),
            "powers": lambda k, t, cnt: zk.g2_srs_powers_device(curve, cnt, ks[1], bases[curve], t, a=ks[0],
                                                                affine=affine),
        }
        for name, call in calls.items():
            zk.g2_scl_set_fixed_min(0)
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
            zk.g2_scl_set_fixed_min(0)
            h = zk.g2_scalar_mul_fixed(curve, scalars[curve][mont][:n], bases[curve], std=not mont, affine=affine)
            assert np.array_equal(h, fixed_expected[(curve, mont)][1 if affine else 0][:n])
            # a short call that takes the per-row kernel: host arrays through it
            zk.g2_scl_set_fixed_min(n + 1)
            assert np.array_equal(zk.g2_scalar_mul_fixed(curve, scalars[curve][mont][:n], bases[curve],
                                                         std=not mont, affine=affine), h)
            assert zk.g2_scl_last_path() == 0
    assert zk.load().zkg_g2_scl_fixed(zk.CURVE_ID[curve], 0, None, 1, zk._p(bases[curve]), 0, None) == 0
    with pytest.raises(ValueError):
        zk.g2_scalar_mul_rows(curve, ks, b[:-1])
    with pytest.raises(ValueError):
        zk.g2_scalar_mul_fixed(curve, ks, bases[curve][:-1])
