"""GPU polynomial division (zkg_poly_long_div / zkg_poly_long_div_device and the Python mirror's
poly_long_div / poly_quot / poly_rem): bit for bit against the reference's own C
(oracle/_ref/libzkref.so: <C>_poly_mont_long_div / _quot / _rem, and _div_by_vanishing for x^k - eta).
No result is compared with another GPU result.  Every reference call respects the reference's
asserts and stays below 2^23 inner products (its loop is quadratic on one core); the one large dense
division is checked through p(z) = q(z) d(z) + r(z) at three points, every term by the reference."""
import ctypes
import itertools

import numpy as np
import pytest

import field_edges as fe

pytestmark = pytest.mark.gpu
CURVES = ["bn128", "bls12_381"]
U64P = ctypes.POINTER(ctypes.c_uint64)
BASES = [-1, 1, 4, 1 << 30]
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
REF_MAX = 1 << 23


@pytest.fixture(autouse=True)
def restore_hooks(gpu):
    yield
    gpu.poly_set_div_base_max(-1)


def rows(n):
    return np.zeros((n, 4), dtype=np.uint64)


def fr(gpu, curve, seed, n):
    return gpu.gen_fr(curve, seed, n) if n else rows(0)


def deg(a):
    nz = np.flatnonzero(a.any(axis=1))
    return int(nz[-1]) if nz.size else -1


def mont(curve, v):
    r = fe.FR[curve]
    return fe.to_row(v * fe.radix(r) % r, 4)


def edges(curve, n, rot=0):
    E = fe.rotate(fe.field_edges(curve + "_fr"), rot)
    return fe.to_limbs([E[i % len(E)] for i in range(n)], 4)


def sizes(p, d):
    """the Haskell sizes (Poly.hs:322-334)"""
    return max(0, p.shape[0] - deg(d)), max(0, deg(d))


def ref_div(reference, curve, p, d, nq=None, nr=None):
    """the reference's long_div into buffers of nq / nr rows (default: the Haskell sizes)"""
    dp, dq = deg(p), deg(d)
    hq, hr = sizes(p, d)
    nq, nr = hq if nq is None else nq, hr if nr is None else nr
    assert nq >= dp - dq + 1 and nr >= dq and (dp >= dq or dq < 0 or nr >= dp + 1)  # its asserts
    assert max(0, dp - dq + 1) * (dq + 1) <= REF_MAX
    q, r = np.full((nq, 4), SENTINEL), np.full((nr, 4), SENTINEL)
    reference.arr(curve, "poly_mont_long_div", p.shape[0], p, d.shape[0], d, nq, q, nr, r)
    return q, r


def expected_steps(gpu, p, d):
    dp, dq = deg(p), deg(d)
    return -1 if dq < 0 or dp < dq else len(gpu.poly_div_plan(dp - dq + 1)) - 1


def check(gpu, reference, curve, p, d, want=None, tag=None):
    want = want or ref_div(reference, curve, p, d)
    q, r = gpu.poly_long_div(curve, p, d)
    steps = gpu.poly_last_div_steps()
    assert q.shape == want[0].shape and r.shape == want[1].shape, tag
    assert np.array_equal(q, want[0]), (tag, "quot")
    assert np.array_equal(r, want[1]), (tag, "rem")
    assert steps == expected_steps(gpu, p, d), tag
    return steps


def raw_div(gpu, curve, p, d, nq, nr, want_q=True, want_r=True):
    """zkg_poly_long_div into buffers with one sentinel row past the end"""
    q, r = np.full((nq + 1, 4), SENTINEL), np.full((nr + 1, 4), SENTINEL)
    rc = gpu.load().zkg_poly_long_div(gpu.CURVE_ID[curve], p.shape[0], p.ctypes.data_as(U64P), d.shape[0],
                                      d.ctypes.data_as(U64P), nq, q.ctypes.data_as(U64P) if want_q else None, nr,
                                      r.ctypes.data_as(U64P) if want_r else None)
    return rc, q, r


# ---------------------------------------------------------------------------- shapes
SHAPES = list(itertools.product([1, 2, 3, 17, 33, 64, 65, 257, 1000], [1, 2, 3, 16, 17, 33, 257])) + [
    (4099, 2050), (4099, 2), (4099, 4098), (2049, 2049), (2049, 2050)]


@pytest.mark.parametrize("curve", CURVES)
def test_shapes_against_long_div(gpu, reference, curve):
    seen = {b: set() for b in BASES}
    for n1, n2 in SHAPES:
        p, d = fr(gpu, curve, 300 + n1, n1), fr(gpu, curve, 400 + n2, n2)
        want = ref_div(reference, curve, p, d)
        for base in BASES:
            gpu.poly_set_div_base_max(base)
            seen[base].add(check(gpu, reference, curve, p, d, want, (n1, n2, base)))
    for base in BASES:  # both ends of the plan ran under every setting
        assert 0 in seen[base] and max(seen[base]) >= 3, (base, seen[base])
    assert -1 in seen[-1]  # and the dividend shorter than the divisor


# ---------------------------------------------------------------------------- coefficient and structure edges
def edge_cases(gpu, reference, curve):
    r = fe.FR[curve]
    one, zero3 = mont(curve, 1), rows(3)
    rnd_p, rnd_d = fr(gpu, curve, 501, 1000), fr(gpu, curve, 502, 300)
    cases = {"edge_list": (edges(curve, 1100, rot=3), edges(curve, 200, rot=17)),
             "all_r_minus_1": (fe.to_limbs([r - 1] * 900, 4), fe.to_limbs([r - 1] * 400, 4))}
    d = rnd_d.copy()
    d[-1] = fe.to_row(r - 1, 4)
    cases["lead_r_minus_1"] = (rnd_p, d)
    d = rnd_d.copy()
    d[-1] = one
    cases["monic"] = (rnd_p, d)
    cases["zero_padded"] = (np.concatenate([rnd_p[:700], zero3, zero3]), np.concatenate([rnd_d[:250], zero3]))
    d = rnd_d.copy()
    d[:7] = 0
    cases["low_zeros"] = (rnd_p, d)
    d = rows(257)
    d[256] = fr(gpu, curve, 503, 1)[0]
    cases["monomial"] = (rnd_p, d)
    cases["constant"] = (rnd_p, np.concatenate([fr(gpu, curve, 504, 1), rows(4)]))
    cases["zero_divisor_1"] = (rnd_p[:200], rows(1))
    cases["zero_divisor_40"] = (rnd_p[:200], rows(40))
    cases["zero_dividend"] = (rows(300), rnd_d[:200])
    cases["dp_lt_dq"] = (rnd_p[:200], rnd_d)
    cases["dp_eq_dq"] = (rnd_p[:300], rnd_d)
    cases["len_0_3"] = (rows(0), rnd_d[:3])
    cases["len_3_0"] = (rnd_p[:3], rows(0))
    cases["len_0_0"] = (rows(0), rows(0))
    return cases


@pytest.mark.parametrize("curve", CURVES)
def test_coefficient_and_structure_edges(gpu, reference, curve):
    for name, (p, d) in edge_cases(gpu, reference, curve).items():
        p, d = np.ascontiguousarray(p), np.ascontiguousarray(d)
        want = ref_div(reference, curve, p, d)
        for base in (-1, 1):
            gpu.poly_set_div_base_max(base)
            check(gpu, reference, curve, p, d, want, (name, base))


@pytest.mark.parametrize("curve", CURVES)
def test_vanishing_divisor_and_exact_division(gpu, reference, curve):
    p = fr(gpu, curve, 511, 1000)
    for k in (256, 300):  # x^k - eta: also what the reference's div_by_vanishing gives
        eta = fr(gpu, curve, 512, 1)[0]
        d = rows(k + 1)
        reference.arr(curve, "arr_mont_neg", 1, eta, d[0])
        d[k] = mont(curve, 1)
        want = ref_div(reference, curve, p, d)
        vq, vr = rows(1000 - k), rows(k)
        reference.arr(curve, "poly_mont_div_by_vanishing", 1000, p, k, eta, 1000 - k, vq, k, vr)
        assert np.array_equal(vq, want[0]) and np.array_equal(vr, want[1])
        for base in (-1, 1):
            gpu.poly_set_div_base_max(base)
            check(gpu, reference, curve, p, d, want, ("vanishing", k, base))
    a, b = fr(gpu, curve, 513, 700), fr(gpu, curve, 514, 400)  # p = a b: quotient a, remainder zero
    ab = rows(1099)
    reference.arr(curve, "poly_mont_mul_naive", 700, a, 400, b, ab)
    for base in (-1, 1):
        gpu.poly_set_div_base_max(base)
        q, r = gpu.poly_long_div(curve, ab, b)
        assert np.array_equal(q, a) and r.shape == (399, 4) and not r.any()
        check(gpu, reference, curve, ab, b, None, ("exact", base))


# ---------------------------------------------------------------------------- output bounds
@pytest.mark.parametrize("curve", CURVES)
def test_output_bounds_and_null_outputs(gpu, reference, curve):
    for n1, n2 in [(1000, 257), (300, 1), (200, 300), (65, 33)]:
        p, d = fr(gpu, curve, 521, n1), fr(gpu, curve, 522, n2)
        nq, nr = max(0, n1 - n2 + 1) + 9, max(n2 - 1, n1 if n1 < n2 else 0) + 5  # larger than needed
        wq, wr = ref_div(reference, curve, p, d, nq, nr)
        rc, q, r = raw_div(gpu, curve, p, d, nq, nr)
        assert rc == 0
        assert np.array_equal(q[:-1], wq) and np.all(q[-1] == SENTINEL), (n1, n2)
        assert np.array_equal(r[:-1], wr) and np.all(r[-1] == SENTINEL), (n1, n2)
        # the reference's quot and rem: a NULL output is never touched
        wq2, wr2 = np.full((nq, 4), SENTINEL), np.full((nr, 4), SENTINEL)
        reference.arr(curve, "poly_mont_quot", n1, p, n2, d, nq, wq2)
        reference.arr(curve, "poly_mont_rem", n1, p, n2, d, nr, wr2)
        rc, q, r = raw_div(gpu, curve, p, d, nq, nr, want_r=False)
        assert rc == 0 and np.array_equal(q[:-1], wq2) and np.all(q[-1] == SENTINEL) and np.all(r == SENTINEL)
        rc, q, r = raw_div(gpu, curve, p, d, nq, nr, want_q=False)
        assert rc == 0 and np.array_equal(r[:-1], wr2) and np.all(r[-1] == SENTINEL) and np.all(q == SENTINEL)
        hq, hr = sizes(p, d)
        assert np.array_equal(gpu.poly_quot(curve, p, d), wq2[:hq])
        assert np.array_equal(gpu.poly_rem(curve, p, d), wr2[:hr])


# ---------------------------------------------------------------------------- large shapes
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n1,n2", [((1 << 17) + 1, 3), ((1 << 17) + 1, (1 << 17) - 2)])
def test_long_by_short_and_short_quotient(gpu, reference, curve, n1, n2):
    p, d = fr(gpu, curve, 531, n1), fr(gpu, curve, 532, n2)
    check(gpu, reference, curve, p, d, None, (n1, n2))


def ref_eval(reference, curve, p, x):
    out = np.zeros(4, dtype=np.uint64)
    reference.arr(curve, "poly_mont_eval_at", p.shape[0], p, np.ascontiguousarray(x), out)
    return out


@pytest.mark.parametrize("curve", CURVES)
def test_large_dense(gpu, reference, curve):
    n1, n2, k = (1 << 17) + 3, (1 << 16) + 1, 1 << 16
    p = fr(gpu, curve, 541, n1)
    # x^(2^16) - eta: bit-exact against the reference's div_by_vanishing
    eta = fr(gpu, curve, 542, 1)[0]
    d = rows(n2)
    reference.arr(curve, "arr_mont_neg", 1, eta, d[0])
    d[k] = mont(curve, 1)
    vq, vr = rows(n1 - k), rows(k)
    reference.arr(curve, "poly_mont_div_by_vanishing", n1, p, k, eta, n1 - k, vq, k, vr)
    q, r = gpu.poly_long_div(curve, p, d)
    assert gpu.poly_last_div_steps() == len(gpu.poly_div_plan(n1 - k)) - 1 >= 3
    assert np.array_equal(q, vq) and np.array_equal(r, vr)
    # dense divisor: p(z) = q(z) d(z) + r(z) at three points fixes (q, r) together with len(r) = deg d
    d = fr(gpu, curve, 543, n2)
    q, r = gpu.poly_long_div(curve, p, d)
    assert q.shape == (n1 - k, 4) and r.shape == (k, 4)
    for z in (fr(gpu, curve, 544, 1)[0], fe.to_row(fe.FR[curve] - 1, 4), gpu.get_fft_subgroup(curve, 20).gen_array()):
        qd, rhs = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        reference.arr(curve, "Fr_mont_mul", ref_eval(reference, curve, q, z), ref_eval(reference, curve, d, z), qd)
        reference.arr(curve, "Fr_mont_add", qd, ref_eval(reference, curve, r, z), rhs)
        assert np.array_equal(ref_eval(reference, curve, p, z), rhs)


# ---------------------------------------------------------------------------- device entries, refusals
@pytest.mark.parametrize("curve", CURVES)
def test_device_entries(gpu, reference, curve):
    for n1, n2 in [(1000, 257), (4099, 2050), (65, 3), (200, 300)]:
        p, d = fr(gpu, curve, 551, n1), fr(gpu, curve, 552, n2)
        nq, nr = max(0, n1 - n2 + 1) + 2, max(n2 - 1, n1 if n1 < n2 else 0) + 2
        wq, wr = ref_div(reference, curve, p, d, nq, nr)
        sent_q, sent_r = np.full((nq + 1, 4), SENTINEL), np.full((nr + 1, 4), SENTINEL)
        dp_, dd_ = gpu.DeviceBuffer(p), gpu.DeviceBuffer(d)
        try:
            for base in (-1, 1):
                gpu.poly_set_div_base_max(base)
                for want_q, want_r in ((True, True), (True, False), (False, True)):
                    bq, br = gpu.DeviceBuffer(sent_q), gpu.DeviceBuffer(sent_r)
                    try:
                        assert gpu.poly_long_div_device(curve, n1, dp_, n2, dd_, nq, bq if want_q else None, nr,
                                                        br if want_r else None) == 0
                        q, r = bq.to_host(sent_q), br.to_host(sent_r)
                    finally:
                        bq.free()
                        br.free()
                    assert gpu.poly_last_div_steps() == expected_steps(gpu, p, d)
                    assert np.array_equal(q, np.concatenate([wq, sent_q[-1:]]) if want_q else sent_q), (n1, n2, base)
                    assert np.array_equal(r, np.concatenate([wr, sent_r[-1:]]) if want_r else sent_r), (n1, n2, base)
            assert np.array_equal(dp_.to_host(p), p) and np.array_equal(dd_.to_host(d), d)  # only read
        finally:
            dp_.free()
            dd_.free()


@pytest.mark.parametrize("curve", CURVES)
def test_refusals(gpu, curve):
    p, d = fr(gpu, curve, 561, 300), fr(gpu, curve, 562, 100)
    for nq, nr in ((200, 99), (201, 98)):  # quot / rem one row too small
        rc, q, r = raw_div(gpu, curve, p, d, nq, nr)
        assert rc == -1 and np.all(q == SENTINEL) and np.all(r == SENTINEL)
    rc, q, r = raw_div(gpu, curve, d, p, 0, 99)  # dp < dq: the remainder holds dp + 1 rows
    assert rc == -1 and np.all(r == SENTINEL)
    lib, cid, P = gpu.load(), gpu.CURVE_ID[curve], lambda a: a.ctypes.data_as(U64P)  # noqa: E731
    q, r = np.full((202, 4), SENTINEL), np.full((100, 4), SENTINEL)
    for n1, n2, nq, nr in ((-1, 100, 201, 99), (300, -5, 201, 99), (300, 100, -1, 99), (300, 100, 201, -1)):
        assert lib.zkg_poly_long_div(cid, n1, P(p), n2, P(d), nq, P(q), nr, P(r)) == -1
    assert np.all(q == SENTINEL) and np.all(r == SENTINEL)
    dp_, dd_ = gpu.DeviceBuffer(p), gpu.DeviceBuffer(d)
    bq, br = gpu.DeviceBuffer(q), gpu.DeviceBuffer(r)
    try:
        assert gpu.poly_long_div_device(curve, 300, dp_, 100, dd_, 200, bq, 99, br) == -1
        assert gpu.poly_long_div_device(curve, 300, dp_, 100, dd_, 201, bq, 98, br) == -1
        assert gpu.poly_long_div_device(curve, -1, dp_, 100, dd_, 201, bq, 99, br) == -1
        assert np.all(bq.to_host(q) == SENTINEL) and np.all(br.to_host(r) == SENTINEL)
    finally:
        for b in (dp_, dd_, bq, br):
            b.free()
    over = (1 << (gpu.POLY_MUL_MAX_LOG[curve] - 1)) + 1  # null pointers: refused on the length alone
    assert gpu.poly_long_div_device(curve, over, None, 2, None, over, None, 1, None) == -1
    assert gpu.poly_last_div_steps() == -1
    assert gpu.last_error() is None  # return codes, nothing on the error channel


@pytest.mark.parametrize("curve", CURVES)
def test_workspace_refused_then_recovers(gpu, reference, curve):
    """the allocator's refusal only: an arena cap below the division's working set records an error
    in the recoverable mode; the next division is correct"""
    gpu.set_error_mode(True)
    try:
        assert gpu.last_error() is None
        p, d = fr(gpu, curve, 571, 3000), fr(gpu, curve, 572, 1000)
        gpu.release()
        gpu.arena_set_limit(1 << 19)  # six transform buffers of 2^12 rows are 768 KiB
        raw_div(gpu, curve, p, d, 2001, 999)
        msg = gpu.last_error()
        assert msg is not None and "memory" in msg
        gpu.arena_set_limit(0)
        check(gpu, reference, curve, p, d, None, "recovered")
        assert gpu.last_error() is None
    finally:
        gpu.set_error_mode(False)
        gpu.arena_set_limit(0)
        gpu.last_error()
