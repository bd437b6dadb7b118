"""The host side of the batch scalar multiplication (zk_scl.hpp): the signed-window recoding that the
fixed-base kernel shares with zkg_g1_scl_digits, and the table size.  CPU only: no call reaches the GPU."""
import random

import numpy as np
import pytest

R = {"bn128": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
     "bls12_381": 52435875175126190479447740508185965837690552500527637822603658699938581184513}
WINDOWS = (2, 4, 5, 8, 11, 13, 16)


def words(k):
    return np.array([(k >> (64 * i)) & (2 ** 64 - 1) for i in range(4)], dtype=np.uint64)


def edge_scalars():
    ks = [0, 1, 2 ** 256 - 1, 2 ** 255, int.from_bytes(b"\x80" * 32, "little"), int.from_bytes(b"\x7f" * 32, "little")]
    for r in R.values():
        ks += [r, r - 1, r + 1]
    rng = random.Random(0x5C1)
    return ks + [rng.getrandbits(256) for _ in range(200)]


@pytest.mark.parametrize("c", WINDOWS)
def test_digits_reconstruct_the_scalar(zk, c):
    want_w = -(-257 // c)
    for k in edge_scalars():
        d = zk.scl_digits(c, words(k))
        assert len(d) == want_w, (c, hex(k))
        assert all(abs(x) <= 1 << (c - 1) for x in d), (c, hex(k))
        assert sum(x << (c * w) for w, x in enumerate(d)) == k, (c, hex(k))


def test_digits_entry_contract(zk):
    import ctypes
    lib = zk.load()
    k = words(2 ** 256 - 1)
    buf = (ctypes.c_int * 8)(*([77] * 8))
    # cap smaller than the window count: only cap entries are written, the count is still returned
    assert lib.zkg_g1_scl_digits(16, zk._p(k), buf, 3) == 17
    assert list(buf[3:]) == [77] * 5
    assert list(buf[:3]) == zk.scl_digits(16, k)[:3]
    for c in (-1, 0, 1, 17):
        assert lib.zkg_g1_scl_digits(c, zk._p(k), buf, 8) == -1
        with pytest.raises(ValueError):
            zk.scl_digits(c, k)


@pytest.mark.parametrize("curve", ["bn128", "bls12_381"])
def test_table_bytes_formula(zk, curve):
    for c in range(2, 17):
        assert zk.scl_table_bytes(curve, c) == 2 ** (c - 1) * -(-257 // c) * 2 * zk.NLIMBS_P[curve] * 8
    # the window is clamped as zkg_g1_scl_set_window clamps it; an unknown curve has no table
    assert zk.scl_table_bytes(curve, 1) == zk.scl_table_bytes(curve, 2)
    assert zk.scl_table_bytes(curve, 40) == zk.scl_table_bytes(curve, 16)
    assert zk.load().zkg_g1_scl_table_bytes(7, 8) == 0


@pytest.mark.parametrize("curve", ["bn128", "bls12_381"])
def test_refusals_need_no_gpu(zk, curve):
    """n < 0 and an unknown curve return -1 before a device is opened or a pointer is read"""
    lib = zk.load()
    cid = zk.CURVE_ID[curve]
    assert lib.zkg_g1_scl_fixed(cid, -1, None, 1, None, 0, None) == -1
    assert lib.zkg_g1_scl_rows(cid, -1, None, 1, None, 0, None) == -1
    assert lib.zkg_g1_scl_powers(cid, -1, None, None, None, 0, None) == -1
    assert lib.zkg_g1_scl_fixed_device(5, 1, None, 1, None, 0, None) == -1
    assert lib.zkg_g1_scl_rows_device(-1, 1, None, 1, None, 0, None) == -1
    assert lib.zkg_g1_scl_powers_device(2, 1, None, None, None, 0, None) == -1
