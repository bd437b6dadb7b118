"""The two table caches of the Fr NTT (zk_ntt.hip) through key separation, eviction and rebuild:
  g_tw  twiddle sets, least recently used out beyond a byte limit (zkg_ntt_set_cache_limit lowers the 8 GiB
        default so that sets of 2^12..2^14 evict each other)
  g_sh  coset shift tables, 32 per context
zkg_ntt_cache_bytes reports what a context holds, so every limit below is a condition on reported sizes, not a
tuned number.  Every result is compared bit for bit with the oracle or with the reference composition of
tests/test_gpu_ntt_ext.py; every test restores the hooks it sets and ends with zkg_release."""
import threading

import numpy as np
import pytest

import generators
from field_edges import field_edges, to_limbs
from test_gpu_ntt_ext import batch_input, expected, run_device
from test_gpu_poly import ref_mul

pytestmark = pytest.mark.gpu
CURVES = ["bn128", "bls12_381"]
SH_CACHE_SETS = 32  # zk_ntt.hip
ROT_M = (12, 13, 14)


def canonical(zk, curve, m):
    return zk.get_fft_subgroup(curve, m).gen_array()


def subgroup(zk, curve, m, gen):
    return zk.FFTSubgroup(curve, tuple(int(v) for v in gen), m)


_ROT = {}


def rotation(zk, oracle, curve):
    """[(m, inverse, generator row, input, expected)] over ROT_M x {forward, inverse} x {canonical, cube},
    ordered so that neighbours differ in size; computed once and never modified"""
    if curve not in _ROT:
        rows = []
        for gname in ("canonical", "cube"):
            for inverse in (False, True):
                for m in ROT_M:
                    g0 = canonical(zk, curve, m)
                    gen = g0 if gname == "canonical" else generators.root(curve, m, g0, "cube")
                    n = 1 << m
                    x = zk.gen_fr(curve, 0xCA00 + m, n)
                    e = to_limbs(field_edges(f"{curve}_fr"), 4)[:n // 2]
                    x[:e.shape[0]] = e
                    want = oracle.ntt(curve, m, gen, x, inverse=inverse)
                    for a in (x, want):
                        a.setflags(write=False)
                    rows.append((m, inverse, gen, x, want))
        _ROT[curve] = rows
    return _ROT[curve]


def transform(zk, curve, m, inverse, gen, x):
    return (zk.inverse_ntt if inverse else zk.forward_ntt)(subgroup(zk, curve, m, gen), x)


def set_bytes(zk, curve, m):
    """bytes of one twiddle set of 2^m: what the cache reports after a release and one forward transform"""
    zk.release()
    assert zk.ntt_cache_bytes() == 0
    x = zk.gen_fr(curve, 1, 1 << m)
    zk.forward_ntt(zk.get_fft_subgroup(curve, m), x)
    return zk.ntt_cache_bytes()


# ---------------------------------------------------------------------------- twiddle sets
@pytest.mark.parametrize("curve", CURVES)
def test_twiddle_eviction_and_rebuild(gpu, oracle, curve):
    rot = rotation(gpu, oracle, curve)
    try:
        size = {m: set_bytes(gpu, curve, m) for m in ROT_M}
        assert 0 < size[12] < size[13] < size[14]
        B = size[13]
        gpu.release()
        gpu.ntt_set_cache_limit(B)  # a second set of 2^13 or more does not fit beside any other
        for rep in range(2):
            for m, inverse, gen, x, want in rot:
                assert np.array_equal(transform(gpu, curve, m, inverse, gen, x), want), (rep, m, inverse)
                held = gpu.ntt_cache_bytes()
                assert size[m] <= held <= max(B, size[m]), (rep, m, inverse, held)
                if m >= 13:
                    assert held == size[m]  # everything else was evicted
        gpu.ntt_set_cache_limit(1)  # below any set: every call evicts what there is and rebuilds
        for m, inverse, gen, x, want in rot:
            assert np.array_equal(transform(gpu, curve, m, inverse, gen, x), want), (m, inverse)
            assert gpu.ntt_cache_bytes() == size[m], (m, inverse)
        gpu.ntt_set_cache_limit(0)  # the default again: the sets stay
        for m, inverse, gen, x, want in rot[:4]:
            assert np.array_equal(transform(gpu, curve, m, inverse, gen, x), want), (m, inverse)
        assert gpu.ntt_cache_bytes() > size[14]
    finally:
        gpu.ntt_set_cache_limit(0)
        gpu.release()
    assert gpu.ntt_cache_bytes() == 0


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n1,n2", [(300, 300), (2049, 100)])
def test_product_under_eviction(gpu, reference, curve, n1, n2):
    """the forward and the inverse set of one product evict each other"""
    a, b = gpu.gen_fr(curve, 100 + n1, n1), gpu.gen_fr(curve, 200 + n2, n2)
    want = ref_mul(reference, curve, a, b)
    gpu.release()
    gpu.poly_set_mul_direct_max(0)
    gpu.ntt_set_cache_limit(1)
    try:
        for _ in range(2):
            assert np.array_equal(gpu.poly_mul(curve, a, b), want)
            assert gpu.poly_last_mul_path() == max(4, (n1 + n2 - 2).bit_length())
    finally:
        gpu.ntt_set_cache_limit(0)
        gpu.poly_set_mul_direct_max(-1)
        gpu.release()


# ---------------------------------------------------------------------------- shift tables
def distinct_shifts(zk, curve, count, seed=0x5E70):
    s = zk.gen_fr(curve, seed, count)
    spare = iter(zk.gen_fr(curve, seed + 1, count))
    for i in range(count):
        while not s[i].any():
            s[i] = next(spare)
    assert len({row.tobytes() for row in s}) == count
    return s


@pytest.mark.parametrize("curve", CURVES)
def test_shift_table_eviction(gpu, reference, curve):
    m, batch, count = 8, 2, 40
    x = batch_input(gpu, curve, m, batch)
    sh = distinct_shifts(gpu, curve, count)

    def check(i, inverse):
        got = run_device(gpu, curve, m, x, inverse, sh[i], batch)
        assert np.array_equal(got, expected(reference, gpu, curve, m, x, inverse, sh[i], batch)), (i, inverse)
        return gpu.ntt_cache_bytes()

    try:
        T = set_bytes(gpu, curve, m)  # the forward twiddle set alone
        held = [check(i, False) for i in range(count)]
        s = held[0] - T
        assert s > 0
        assert held[:SH_CACHE_SETS] == [T + (i + 1) * s for i in range(SH_CACHE_SETS)]
        assert all(h == held[SH_CACHE_SETS - 1] for h in held[SH_CACHE_SETS:])  # no growth past 32 keys
        assert check(0, False) == held[-1]   # evicted, rebuilt
        assert check(39, False) == held[-1]  # still cached
        # the inverse's keys are other keys; its twiddle set (as large as the forward one) joins the cache
        assert check(0, True) == held[-1] + T
        assert check(39, True) == held[-1] + T
    finally:
        gpu.release()


@pytest.mark.parametrize("curve", CURVES)
def test_shift_key_fields(gpu, reference, curve):
    """one shift under every field of the shift key: direction, size, and `scaled` (the table carries 1/N when
    the last pass owes it, i.e. when pass 0 has no twiddle table: zkg_ntt_set_table_max flips that at 2^13).
    test_gpu_ntt_ext.test_closing_paths reaches default cap -> lowered cap at 2^13 with one shift, but only
    through the order of its parameters within one process; here both orders run from an empty cache."""
    shift = distinct_shifts(gpu, curve, 1, seed=0x5E7F)[0]

    def check(m, inverse):
        x = batch_input(gpu, curve, m, 2)
        got = run_device(gpu, curve, m, x, inverse, shift, 2)
        assert np.array_equal(got, expected(reference, gpu, curve, m, x, inverse, shift, 2)), (m, inverse)

    gpu.release()
    try:
        for m in (8, 9):
            check(m, False)
            check(m, True)
        check(8, False)
        for caps in ((0, 1, 0), (1, 0, 1)):
            gpu.release()
            for cap in caps:
                gpu.ntt_set_table_max(cap)
                check(13, True)
                check(13, False)
    finally:
        gpu.ntt_set_table_max(0)
        gpu.release()


# ---------------------------------------------------------------------------- threads
def test_eviction_under_threads(gpu, oracle):
    """four threads on one device (one context: calls serialise on its mutex), each over another rotation of the
    eviction test's calls, with the limit at one 2^13 set: every call of one thread may find its set evicted
    by another's"""
    rot = [(c,) + row for c in CURVES for row in rotation(gpu, oracle, c)]
    errors = []

    def run(tid):
        try:
            k = tid * len(rot) // 4
            for rep in range(2):
                for curve, m, inverse, gen, x, want in rot[k:] + rot[:k]:
                    if not np.array_equal(transform(gpu, curve, m, inverse, gen, x), want):
                        errors.append(f"thread {tid}: {curve} m={m} inverse={inverse} rep={rep}")
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(f"thread {tid}: {e!r}")

    try:
        B = set_bytes(gpu, "bn128", 13)
        gpu.release()
        gpu.ntt_set_cache_limit(B)
        threads = [threading.Thread(target=run, args=(t,)) for t in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
        assert not any(t.is_alive() for t in threads), "a thread hung"
        assert not errors, errors[:10]
        assert 0 < gpu.ntt_cache_bytes()
    finally:
        gpu.ntt_set_cache_limit(0)
        gpu.release()
