"""Every entry point that takes the subgroup generator, called with generators OTHER than the one
zkg_fft_generator returns (tests/generators.py: inv, cube, neg, k5 -- primitive 2^m-th roots g^k), bit for bit
against the oracle / the reference's own C called with the same generator.

What depends on the generator: the cached Fr twiddle sets (their key, w^-1 and 1/N of the inverse, the
per-pass tables, the on-the-fly two-level tables), the GLV-decomposed twiddles of the G1 group FFT and the
integer stage scalars of the G1 fallback and of the G2 FFT.  No GPU result is compared with another GPU
result, except the round trips, which come on top."""
import ctypes

import numpy as np
import pytest

import generators
import golden_io
from field_edges import field_edges, to_limbs
from test_gpu_g2fft import cases  # noqa: F401 -- the module-scoped fixture (inputs built with the reference)
from test_gpu_ntt_ext import batch_input, expected, run_device, shifts

pytestmark = pytest.mark.gpu
CURVES = ["bn128", "bls12_381"]
M_LIST = [1, 2, 3, 8, 11, 12, 13, 16, 17, 20]


def canonical(zk, curve, m):
    return zk.get_fft_subgroup(curve, m).gen_array()


def named(zk, curve, m, only=None):
    """[(name, Montgomery row)] of the named roots that exist at m"""
    rows = generators.roots(curve, m, canonical(zk, curve, m))
    return [(k, v) for k, v in rows.items() if only is None or k in only]


def subgroup(zk, curve, m, gen):
    return zk.FFTSubgroup(curve, tuple(int(v) for v in gen), m)


_X = {}


def fr_input(zk, curve, m):
    """random rows, the head overwritten with Fr edge values (at most half of the rows)"""
    if (curve, m) not in _X:
        n = 1 << m
        x = zk.gen_fr(curve, 0x6E10 + m, n)
        e = to_limbs(field_edges(f"{curve}_fr"), 4)[:n // 2]
        x[:e.shape[0]] = e
        x.setflags(write=False)
        _X[curve, m] = x
    return _X[curve, m]


def check_host(zk, oracle, curve, m, name, gen):
    sg, x = subgroup(zk, curve, m, gen), fr_input(zk, curve, m)
    f = zk.forward_ntt(sg, x)
    assert np.array_equal(f, oracle.ntt(curve, m, gen, x)), (name, "forward")
    i = zk.inverse_ntt(sg, x)
    assert np.array_equal(i, oracle.ntt(curve, m, gen, x, inverse=True)), (name, "inverse")
    assert np.array_equal(zk.inverse_ntt(sg, f), x), (name, "round trip")


# ---------------------------------------------------------------------------- Fr NTT, host symbols
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", M_LIST)
def test_ntt_host_symbols(gpu, oracle, curve, m):
    """the single-workgroup pass, the first two-digit split, the host path that consults the device set
    (from 2^16), the three-pass split and the default two-pass 2^20 (inv only, to keep it to seconds)"""
    for name, gen in named(gpu, curve, m, ("inv",) if m == 20 else None):
        check_host(gpu, oracle, curve, m, name, gen)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("radix", [12, 8])
def test_ntt_pass_splits(gpu, oracle, curve, radix):
    m = 17
    gpu.ntt_set_max_radix(radix)
    try:
        for name, gen in named(gpu, curve, m, ("inv", "cube")):
            check_host(gpu, oracle, curve, m, name, gen)
    finally:
        gpu.ntt_set_max_radix(0)


@pytest.mark.parametrize("curve", CURVES)
def test_ntt_otf_twiddles(gpu, oracle, curve):
    """the inter-pass twiddles from the two-level tables tlo / thi, the inverse's 1/N on the closing product"""
    m = 13
    gpu.ntt_set_table_max(1)
    try:
        for name, gen in named(gpu, curve, m, ("inv", "cube")):
            check_host(gpu, oracle, curve, m, name, gen)
    finally:
        gpu.ntt_set_table_max(0)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", [2, 12])
def test_ntt_device(gpu, oracle, curve, m):
    x = fr_input(gpu, curve, m)
    d_src, d_dst = gpu.DeviceBuffer(x), gpu.DeviceBuffer.empty(x.nbytes)
    try:
        for name, gen in named(gpu, curve, m):
            for inverse in (False, True):
                gpu.ntt_device(curve, m, gen, d_src, d_dst, inverse=inverse)
                assert np.array_equal(d_dst.to_host(x), oracle.ntt(curve, m, gen, x, inverse=inverse)), (name, inverse)
    finally:
        d_src.free()
        d_dst.free()


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", [2, 8, 12, 13])
def test_ntt_ext_device(gpu, reference, curve, m):
    """coset transforms of a batch of 3, the expectation composed from the reference as test_gpu_ntt_ext.py does"""
    gen = generators.root(curve, m, canonical(gpu, curve, m), "cube")
    shift = shifts(gpu, curve, m)["random"]
    x = batch_input(gpu, curve, m, 3)
    for inverse in (False, True):
        got = run_device(gpu, curve, m, x, inverse, shift, 3, gen=gen)
        assert np.array_equal(got, expected(reference, gpu, curve, m, x, inverse, shift, 3, gen=gen)), inverse


@pytest.mark.parametrize("curve", CURVES)
def test_twiddle_key_separation(gpu, oracle, curve):
    """canonical and other generators interleaved in one process at one size and pass split: each call must get
    the twiddle set of ITS generator and direction from the cache, before and after a release"""
    m = 12
    g0 = canonical(gpu, curve, m)
    roots = dict(named(gpu, curve, m))
    x = fr_input(gpu, curve, m)
    want = {(k, inv): oracle.ntt(curve, m, g, x, inverse=inv)
            for k, g in (("canonical", g0), ("cube", roots["cube"]), ("inv", roots["inv"])) for inv in (False, True)}
    assert len({w.tobytes() for w in want.values()}) == len(want)  # the six expectations differ
    gens = dict(roots, canonical=g0)

    def call(name, inverse):
        sg = subgroup(gpu, curve, m, gens[name])
        got = (gpu.inverse_ntt if inverse else gpu.forward_ntt)(sg, x)
        assert np.array_equal(got, want[name, inverse]), (name, inverse)

    gpu.release()
    try:
        for name, inverse in (("canonical", False), ("cube", False), ("canonical", False), ("cube", True),
                              ("canonical", True), ("inv", False)):
            call(name, inverse)
        gpu.release()
        call("cube", False)
        call("cube", True)
    finally:
        gpu.release()


# ---------------------------------------------------------------------------- G1 group FFT
G1_FFT_SIZES = [1, 2, 3, 5, 8]
G1_PLAN_SIZES = (5, 8)  # sizes that must run the radix-2^b Stockham stages (a non-empty zkg_g1_fft_plan)


def g1_points(gpu, oracle, curve, coords, m):
    f = golden_io.projective_points if coords == "proj" else golden_io.jacobian_points
    n = 1 << m
    return f(gpu, oracle, curve, n, 0x6F00 + m, min(2, n // 2))


def ref_g1_fft(reference, curve, coords, m, gen, pts, inverse):
    want = np.zeros_like(pts)
    reference.arr(curve, f"G1_{coords}_fft_{'inverse' if inverse else 'forward'}", m, gen, pts, want)
    return want


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("coords", ["proj", "jac"])
@pytest.mark.parametrize("m", G1_FFT_SIZES)
def test_g1_fft(gpu, oracle, reference, curve, coords, m):
    """subgroup points with random Z and an infinity: the GLV stages with twiddles decomposed from another
    generator's powers, normalised outputs as the reference's"""
    if m in G1_PLAN_SIZES:
        assert gpu.g1_fft_plan(curve, m), "this size is meant to run the radix-2^b stages"
    pts = g1_points(gpu, oracle, curve, coords, m)
    for name in ("inv", "cube"):
        gen = generators.root(curve, m, canonical(gpu, curve, m), name)
        sg = subgroup(gpu, curve, m, gen)
        for inverse, f in ((False, gpu.forward_fft), (True, gpu.inverse_fft)):
            got = f(sg, pts, coords=coords)
            assert gpu.g1_fft_last_glv() == 1, (name, inverse)
            assert np.array_equal(got, ref_g1_fft(reference, curve, coords, m, gen, pts, inverse)), (name, inverse)


@pytest.mark.parametrize("m", [1, 3])
def test_g1_fft_nonsubgroup_points_bls(gpu, reference, m):
    """the integer-scalar schedule with another scalar at every position (inputs as
    test_gpu_g1ext.test_fft_nonsubgroup_points_bls)"""
    curve = "bls12_381"
    proj = gpu.batch_from_affine(curve, golden_io.bls_nonsubgroup_points(1 << m, 300 + m))
    gen = generators.root(curve, m, canonical(gpu, curve, m), "cube")
    sg = subgroup(gpu, curve, m, gen)
    for inverse, f in ((False, gpu.forward_fft), (True, gpu.inverse_fft)):
        got = f(sg, proj)
        assert gpu.g1_fft_last_glv() == 0, inverse
        assert np.array_equal(got, ref_g1_fft(reference, curve, "proj", m, gen, proj, inverse)), inverse


# ---------------------------------------------------------------------------- G2 group FFT
def ref_g2_fft(reference, curve, m, gen, rows, inverse):
    want = np.zeros_like(rows)
    reference.arr(curve, f"G2_proj_fft_{'inverse' if inverse else 'forward'}", m, gen, np.ascontiguousarray(rows), want)
    return want


def check_g2(gpu, reference, cases, curve, m, names):  # noqa: F811
    rows, ref_rows = cases.rows(curve, m)
    for name in names:
        gen = generators.root(curve, m, canonical(gpu, curve, m), name)
        sg = subgroup(gpu, curve, m, gen)
        for inverse, f in ((False, gpu.g2_forward_fft), (True, gpu.g2_inverse_fft)):
            got = f(sg, rows)
            want = ref_g2_fft(reference, curve, m, gen, ref_rows, inverse)
            bad = np.nonzero(np.any(got != want, axis=1))[0]
            assert bad.size == 0, (name, inverse, bad[:10])


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", [1, 2, 3, 5])
def test_g2_fft(gpu, reference, cases, curve, m):  # noqa: F811
    check_g2(gpu, reference, cases, curve, m, ("inv", "cube"))


def test_g2_fft_grid_stride(gpu, reference, cases):  # noqa: F811
    """m = 5 under a 256-lane cap: the stages' grid-stride loops"""
    gpu.g2_fft_set_max_lanes(256)
    try:
        check_g2(gpu, reference, cases, "bls12_381", 5, ("cube",))
    finally:
        gpu.g2_fft_set_max_lanes(0)


# ---------------------------------------------------------------------------- device forms
FFT_DEVICE_ARGS = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p,
                   ctypes.c_void_p]


def run_fft_device(gpu, fn, curve, m, gen, rows, inverse):
    fn.argtypes = FFT_DEVICE_ARGS
    rows = np.ascontiguousarray(rows)
    d_src, d_dst = gpu.DeviceBuffer(rows), gpu.DeviceBuffer(np.zeros_like(rows))
    try:
        fn(gpu.CURVE_ID[curve], 1 if inverse else 0, m, gpu._p(np.ascontiguousarray(gen)), d_src.ptr, d_dst.ptr)
        return d_dst.to_host(rows)
    finally:
        d_src.free()
        d_dst.free()


@pytest.mark.parametrize("curve", CURVES)
def test_fft_device_forms(gpu, oracle, reference, cases, curve):  # noqa: F811
    m, lib = 3, gpu.load()
    gen = generators.root(curve, m, canonical(gpu, curve, m), "inv")
    for coords, fn in (("proj", lib.zkg_g1_fft_device), ("jac", lib.zkg_g1_jac_fft_device)):
        pts = g1_points(gpu, oracle, curve, coords, m)
        for inverse in (False, True):
            got = run_fft_device(gpu, fn, curve, m, gen, pts, inverse)
            assert np.array_equal(got, ref_g1_fft(reference, curve, coords, m, gen, pts, inverse)), (coords, inverse)
            assert gpu.g1_fft_last_glv() == 1
    rows, ref_rows = cases.rows(curve, m)
    for inverse in (False, True):
        got = run_fft_device(gpu, lib.zkg_g2_fft_device, curve, m, gen, rows, inverse)
        assert np.array_equal(got, ref_g2_fft(reference, curve, m, gen, ref_rows, inverse)), inverse
