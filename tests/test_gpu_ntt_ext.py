"""Coset and batched NTT (zkg_ntt_ext_device / zkg_ntt_ext) against the reference's own C.

Every expected value is composed from the reference's functions (Reference.arr):
    forward: poly_mont_ntt_forward(arr_mont_mul(src, arr_mont_powers(n, one, shift)))
    inverse: arr_mont_mul(poly_mont_ntt_inverse(src), arr_mont_powers(n, one, Fr_mont_inv(shift)))
    batch:   the reference called once per transform
No GPU result is compared with another GPU result, except the round trip, which comes on top."""
import ctypes

import numpy as np
import pytest

from field_edges import FR, field_edges, to_limbs, to_row

pytestmark = pytest.mark.gpu
CURVES = ["bn128", "bls12_381"]
M_LIST = [0, 1, 2, 5, 8, 11, 12, 13]
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)


# ---------------------------------------------------------------------------- reference compositions
def one(zk, curve):
    return zk.get_fft_subgroup(curve, 0).gen_array()  # the generator of the order-1 subgroup


def ref_powers(ref, zk, curve, n, s):
    out = np.zeros((n, 4), dtype=np.uint64)
    ref.arr(curve, "arr_mont_powers", n, one(zk, curve), np.ascontiguousarray(s, dtype=np.uint64), out)
    return out


def ref_mul(ref, curve, a, b):
    out = np.zeros_like(a)
    ref.arr(curve, "arr_mont_mul", a.shape[0], a, b, out)
    return out


def ref_inv(ref, curve, s):
    out = np.zeros(4, dtype=np.uint64)
    ref.arr(curve, "Fr_mont_inv", np.ascontiguousarray(s, dtype=np.uint64), out)
    return out


def expected_one(ref, zk, curve, m, x, inverse, shift, gen=None):
    """one transform of 2^m rows (gen: the subgroup generator, the canonical one when not given)"""
    n = 1 << m
    if gen is None:
        gen = zk.get_fft_subgroup(curve, m).gen_array()
    x = np.ascontiguousarray(x)
    if shift is None:
        return ref.ntt(curve, m, gen, x, inverse)
    if not inverse:
        return ref.ntt(curve, m, gen, ref_mul(ref, curve, x, ref_powers(ref, zk, curve, n, shift)), False)
    return ref_mul(ref, curve, ref.ntt(curve, m, gen, x, True), ref_powers(ref, zk, curve, n, ref_inv(ref, curve, shift)))


def expected(ref, zk, curve, m, x, inverse, shift, batch, gen=None):
    n = 1 << m
    return np.concatenate([expected_one(ref, zk, curve, m, x[b * n:(b + 1) * n], inverse, shift, gen)
                           for b in range(batch)]) if batch else x[:0]


# ---------------------------------------------------------------------------- inputs
_INPUTS = {}


def batch_input(zk, curve, m, batch):
    """transform 0: gen_fr, 1: the Fr edge list (repeated to 2^m rows), 2: all r - 1, then again"""
    key = (curve, m, batch)
    if key not in _INPUTS:
        n = 1 << m
        edges = to_limbs(field_edges(f"{curve}_fr"), 4)
        kinds = [lambda b: zk.gen_fr(curve, 0xE700 + 16 * m + b, n),
                 lambda b: np.resize(np.roll(edges, -b, axis=0), (n, 4)),
                 lambda b: np.tile(to_row(FR[curve] - 1, 4), (n, 1))]
        _INPUTS[key] = np.ascontiguousarray(np.concatenate([kinds[b % 3](b) for b in range(batch)]), dtype=np.uint64)
    return _INPUTS[key]


def shifts(zk, curve, m):
    return {"one": one(zk, curve), "rm1": to_row(FR[curve] - 1, 4), "random": zk.gen_fr(curve, 0x5EED + m, 1)[0],
            "subgroup": zk.get_fft_subgroup(curve, m + 1).gen_array()}


def run_device(zk, curve, m, x, inverse, shift, batch, inplace=False, gen=None):
    if gen is None:
        gen = zk.get_fft_subgroup(curve, m).gen_array()
    d_src = zk.DeviceBuffer(x)
    d_dst = d_src if inplace else zk.DeviceBuffer.empty(x.nbytes)
    try:
        zk.ntt_ext_device(curve, m, gen, d_src, d_dst, inverse=inverse, shift=shift, batch=batch)
        return d_dst.to_host(x)
    finally:
        d_src.free()
        if not inplace:
            d_dst.free()


# ---------------------------------------------------------------------------- 1. batch, no shift
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", M_LIST)
def test_batch_no_shift(gpu, reference, curve, m):
    for batch in (1, 2, 3, 5):
        x = batch_input(gpu, curve, m, batch)
        for inverse in (False, True):
            got = run_device(gpu, curve, m, x, inverse, None, batch)
            assert np.array_equal(got, expected(reference, gpu, curve, m, x, inverse, None, batch)), (batch, inverse)


# ---------------------------------------------------------------------------- 2. large batch
@pytest.mark.parametrize("curve", CURVES)
def test_large_batch_crosses_grid_limit(gpu, reference, curve):
    """65536 + 3 transforms of 4 points: more tiles than a grid's y or z dimension holds; the first,
    a middle and the last transform differ from the common one"""
    m, batch, n = 2, 65536 + 3, 4
    common = gpu.gen_fr(curve, 0xBA7C, n)
    distinct = {0: gpu.gen_fr(curve, 0xBA7D, n), 40000: to_limbs(field_edges(f"{curve}_fr")[5:9], 4),
                batch - 1: np.tile(to_row(FR[curve] - 1, 4), (n, 1))}
    x = np.tile(common, (batch, 1))
    for b, v in distinct.items():
        x[b * n:(b + 1) * n] = v
    shift = gpu.gen_fr(curve, 0xBA7E, 1)[0]
    for inverse in (False, True):
        for sh in (None, shift):
            want = np.tile(expected_one(reference, gpu, curve, m, common, inverse, sh), (batch, 1))
            for b, v in distinct.items():
                want[b * n:(b + 1) * n] = expected_one(reference, gpu, curve, m, v, inverse, sh)
            got = run_device(gpu, curve, m, x, inverse, sh, batch)
            assert np.array_equal(got, want), (inverse, sh is not None)


@pytest.mark.parametrize("curve", CURVES)
def test_split_launches(gpu, reference, curve):
    """the launch split a batch of more than 2^21 tiles takes, forced at a small size: 3 tiles per
    launch for 3 transforms of 8 tiles per pass"""
    m, batch = 13, 3
    x = batch_input(gpu, curve, m, batch)
    shift = shifts(gpu, curve, m)["random"]
    gpu.ntt_ext_set_max_grid(3)
    try:
        for inverse in (False, True):
            got = run_device(gpu, curve, m, x, inverse, shift, batch)
            assert np.array_equal(got, expected(reference, gpu, curve, m, x, inverse, shift, batch)), inverse
    finally:
        gpu.ntt_ext_set_max_grid(0)


# ---------------------------------------------------------------------------- 3. shift
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", M_LIST)
def test_shift(gpu, reference, curve, m):
    n = 1 << m
    for name, shift in shifts(gpu, curve, m).items():
        for batch in (1, 3):
            x = batch_input(gpu, curve, m, batch)
            for inverse in (False, True):
                got = run_device(gpu, curve, m, x, inverse, shift, batch)
                want = expected(reference, gpu, curve, m, x, inverse, shift, batch)
                assert np.array_equal(got, want), (name, batch, inverse)
                if name == "one":  # the reference's plain transform
                    assert np.array_equal(got, expected(reference, gpu, curve, m, x, inverse, None, batch))
                if name == "subgroup" and not inverse:
                    # independent expectation: the odd-index outputs of the 2^(m+1) transform of the padded input
                    g2 = gpu.get_fft_subgroup(curve, m + 1).gen_array()
                    for b in range(batch):
                        pad = np.zeros((2 * n, 4), dtype=np.uint64)
                        pad[:n] = x[b * n:(b + 1) * n]
                        assert np.array_equal(got[b * n:(b + 1) * n], reference.ntt(curve, m + 1, g2, pad)[1::2]), b


# ---------------------------------------------------------------------------- 4. closing paths
@pytest.fixture(params=[("one_pass", 11, 0, 0), ("table", 13, 0, 0), ("otf", 13, 0, 1), ("big_tiles", 17, 12, 0),
                        ("three_passes", 17, 8, 0)], ids=lambda p: p[0])
def closing_path(gpu, request):
    """(m, pass split hook, table cap hook): P == 1 with the scale at the last pass; 1/N on pass 0's
    table; on-the-fly twiddles with the scale at the last pass; the 1024-thread kernel; three passes
    with an in-place middle pass"""
    _, m, radix, table_max = request.param
    gpu.ntt_set_max_radix(radix)
    gpu.ntt_set_table_max(table_max)
    yield m
    gpu.ntt_set_max_radix(0)
    gpu.ntt_set_table_max(0)


@pytest.mark.parametrize("curve", CURVES)
def test_closing_paths(gpu, reference, curve, closing_path):
    m = closing_path
    shift = shifts(gpu, curve, m)["random"]
    x = batch_input(gpu, curve, m, 2)
    n = 1 << m
    for inverse in (True, False):
        want = expected(reference, gpu, curve, m, x, inverse, shift, 2)
        assert np.array_equal(run_device(gpu, curve, m, x, inverse, shift, 2), want), inverse
        assert np.array_equal(run_device(gpu, curve, m, x[:n], inverse, shift, 1), want[:n]), inverse
    assert np.array_equal(run_device(gpu, curve, m, x, True, None, 2), expected(reference, gpu, curve, m, x, True, None, 2))


# ---------------------------------------------------------------------------- 5. round trip
@pytest.mark.parametrize("curve", CURVES)
def test_round_trip(gpu, curve):
    m, batch = 13, 3
    x = batch_input(gpu, curve, m, batch)
    shift = shifts(gpu, curve, m)["random"]
    f = run_device(gpu, curve, m, x, False, shift, batch)
    assert np.array_equal(run_device(gpu, curve, m, f, True, shift, batch), x)


# ---------------------------------------------------------------------------- 6. in place
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", [5, 13])
def test_in_place(gpu, reference, curve, m):
    x = batch_input(gpu, curve, m, 2)
    shift = shifts(gpu, curve, m)["random"]
    for inverse in (False, True):
        got = run_device(gpu, curve, m, x, inverse, shift, 2, inplace=True)
        assert np.array_equal(got, expected(reference, gpu, curve, m, x, inverse, shift, 2)), inverse


# ---------------------------------------------------------------------------- 7. degenerate cases
def raw_call(zk, curve, inverse, m, shift, batch, d_src, d_dst):
    gen = zk.get_fft_subgroup(curve, min(max(m, 0), 20)).gen_array()
    sp = None if shift is None else shift.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    return zk.load().zkg_ntt_ext_device(zk.CURVE_ID[curve], inverse, m, gen.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                        sp, batch, d_src.ptr, d_dst.ptr)


@pytest.mark.parametrize("curve", CURVES)
def test_degenerate(gpu, reference, curve):
    m, n = 5, 32
    zero = np.zeros(4, dtype=np.uint64)
    x = batch_input(gpu, curve, m, 2)
    # shift = 0 forward: every output is src_b[0], as the reference composition gives
    got = run_device(gpu, curve, m, x, False, zero, 2)
    assert np.array_equal(got, expected(reference, gpu, curve, m, x, False, zero, 2))
    assert np.array_equal(got, np.repeat(x[[0, n]], n, axis=0))
    sentinel = np.full_like(x, SENTINEL)
    d_src, d_dst = gpu.DeviceBuffer(x), gpu.DeviceBuffer(sentinel)
    try:
        assert raw_call(gpu, curve, 1, m, zero, 2, d_src, d_dst) == -1  # no inverse of the shift 0
        assert raw_call(gpu, curve, 0, m, None, -1, d_src, d_dst) == -1
        assert raw_call(gpu, curve, 0, 31, None, 1, d_src, d_dst) == -1
        assert raw_call(gpu, curve, 0, -1, None, 1, d_src, d_dst) == -1
        assert raw_call(gpu, curve, 0, m, None, 0, d_src, d_dst) == 0  # batch 0: a no-op
        assert np.array_equal(d_dst.to_host(x), sentinel)
        with pytest.raises(ValueError):
            gpu.ntt_ext_device(curve, m, gpu.get_fft_subgroup(curve, m).gen_array(), d_src, d_dst, inverse=True,
                               shift=zero, batch=2)
        with pytest.raises(ValueError):
            gpu.coset_intt(gpu.get_fft_subgroup(curve, m), zero, x[:n])
        assert np.array_equal(d_dst.to_host(x), sentinel)
    finally:
        d_src.free()
        d_dst.free()


# ---------------------------------------------------------------------------- 8. chunked degrade path
@pytest.mark.parametrize("curve", CURVES)
def test_chunked_when_the_arena_is_short(gpu, reference, curve):
    """5 transforms of 2^13 rows on host buffers need 3 x 5 x 256 KiB (+ 1 MiB) of arena; under a
    3 MiB cap two fit at a time (2.5 MiB) and three do not (3.25 MiB): chunks of 2, 2, 1"""
    m, batch = 13, 5
    x = batch_input(gpu, curve, m, batch)
    shift = shifts(gpu, curve, m)["random"]
    gen = gpu.get_fft_subgroup(curve, m).gen_array()
    gpu.release()  # the cap only bites when the arena has to grow
    gpu.arena_set_limit(3 << 20)
    try:
        for inverse in (False, True):
            got = gpu.ntt_ext(curve, m, gen, x, inverse=inverse, shift=shift, batch=batch)
            assert np.array_equal(got, expected(reference, gpu, curve, m, x, inverse, shift, batch)), inverse
    finally:
        gpu.arena_set_limit(0)
        gpu.release()


# ---------------------------------------------------------------------------- 9. host form
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("m", [3, 12])
def test_host_form(gpu, reference, curve, m):
    batch = 3
    x = batch_input(gpu, curve, m, batch)
    shift = shifts(gpu, curve, m)["random"]
    sg = gpu.get_fft_subgroup(curve, m)
    n = 1 << m
    for inverse in (False, True):
        want = expected(reference, gpu, curve, m, x, inverse, shift, batch)
        assert np.array_equal(gpu.ntt_ext(curve, m, sg.gen_array(), x, inverse=inverse, shift=shift, batch=batch), want)
        coset = gpu.coset_intt if inverse else gpu.coset_ntt
        assert np.array_equal(coset(sg, shift, x[:n]), want[:n])
        plain = expected(reference, gpu, curve, m, x, inverse, None, batch).reshape(batch, n, 4)
        batch_fn = gpu.inverse_ntt_batch if inverse else gpu.forward_ntt_batch
        assert np.array_equal(batch_fn(sg, x.reshape(batch, n, 4)), plain)


# ---------------------------------------------------------------------------- 10. existing path untouched
@pytest.mark.parametrize("curve", CURVES)
def test_existing_path_untouched(gpu, reference, curve):
    """the ext calls share the twiddle cache with zkg_ntt_device and the host-buffer symbols"""
    m = 13
    sg = gpu.get_fft_subgroup(curve, m)
    x = batch_input(gpu, curve, m, 1)
    shift = shifts(gpu, curve, m)["random"]
    for inverse in (False, True):
        run_device(gpu, curve, m, x, inverse, shift, 1)
    want = reference.ntt(curve, m, sg.gen_array(), x)
    assert np.array_equal(gpu.forward_ntt(sg, x), want)
    d_src, d_dst = gpu.DeviceBuffer(x), gpu.DeviceBuffer.empty(x.nbytes)
    try:
        gpu.ntt_device(curve, m, sg.gen_array(), d_src, d_dst)
        assert np.array_equal(d_dst.to_host(x), want)
        gpu.ntt_device(curve, m, sg.gen_array(), d_src, d_dst, inverse=True)
        assert np.array_equal(d_dst.to_host(x), reference.ntt(curve, m, sg.gen_array(), x, True))
    finally:
        d_src.free()
        d_dst.free()
