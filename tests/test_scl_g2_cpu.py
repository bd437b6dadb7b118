"""The host side of the batch G2 scalar multiplication: the exported names, the table size, and the refusals
that come before any GPU call.  CPU only: no call reaches the GPU."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ("bn128", "bls12_381")
NAMES = [f"zkg_g2_scl_{k}{d}" for k in ("fixed", "rows", "powers") for d in ("", "_device")] + [
    "zkg_g2_scl_set_window", "zkg_g2_scl_set_fixed_min", "zkg_g2_scl_last_path", "zkg_g2_scl_table_bytes"]


def test_names_are_declared_and_exported(zk):
    with open(os.path.join(ROOT, "include", "zkalgebra_gpu.h")) as f:
        header = f.read()
    lib = zk.load()
    for name in NAMES:
        assert name in zk.EXTENSION_SYMBOLS, name
        assert re.search(r"ZKG_API\s+\w+\s+%s\(" % name, header), name
        assert hasattr(lib, name), name
    for name in ("g2_scalar_mul_fixed", "g2_scalar_mul_rows", "g2_srs_powers"):
        assert callable(getattr(zk, name)) and callable(getattr(zk, name + "_device")), name


@pytest.mark.parametrize("curve", CURVES)
def test_table_bytes_formula(zk, curve):
    np64 = 2 * zk.NLIMBS_P[curve]  # the words of an Fp2 element: 8 / 12
    assert np64 == {"bn128": 8, "bls12_381": 12}[curve]
    for c in range(2, 17):
        assert zk.g2_scl_table_bytes(curve, c) == -(-257 // c) * 2 ** (c - 1) * 2 * np64 * 8
        assert zk.g2_scl_table_bytes(curve, c) == 2 * zk.scl_table_bytes(curve, c)
    # the window is clamped as zkg_g2_scl_set_window clamps it; an unknown curve has no table
    assert zk.g2_scl_table_bytes(curve, 1) == zk.g2_scl_table_bytes(curve, 2)
    assert zk.g2_scl_table_bytes(curve, 40) == zk.g2_scl_table_bytes(curve, 16)
    assert zk.load().zkg_g2_scl_table_bytes(7, 8) == 0


@pytest.mark.parametrize("curve", CURVES)
def test_refusals_need_no_gpu(zk, curve):
    """n < 0 and an unknown curve return -1 before a device is opened or a pointer is read"""
    lib = zk.load()
    cid = zk.CURVE_ID[curve]
    assert lib.zkg_g2_scl_fixed(cid, -1, None, 1, None, 0, None) == -1
    assert lib.zkg_g2_scl_rows(cid, -1, None, 1, None, 0, None) == -1
    assert lib.zkg_g2_scl_powers(cid, -1, None, None, None, 0, None) == -1
    assert lib.zkg_g2_scl_fixed_device(5, 1, None, 1, None, 0, None) == -1
    assert lib.zkg_g2_scl_rows_device(-1, 1, None, 1, None, 0, None) == -1
    assert lib.zkg_g2_scl_powers_device(2, 1, None, None, None, 0, None) == -1


@pytest.mark.parametrize("curve", CURVES)
def test_shape_checks_raise_without_a_gpu(zk, curve):
    n1 = zk.NLIMBS_P[curve]
    ks = np.zeros((3, 4), dtype=np.uint64)
    g1_row = np.zeros(2 * n1, dtype=np.uint64)  # a G1 row where a G2 row (4 n1 words) belongs
    buf = SimpleNamespace(ptr=0)
    with pytest.raises(ValueError):
        zk.g2_scalar_mul_fixed(curve, ks, g1_row)
    with pytest.raises(ValueError):
        zk.g2_scalar_mul_fixed_device(curve, 3, buf, g1_row, buf)
    with pytest.raises(ValueError):
        zk.g2_srs_powers(curve, ks[0], 3, g1_row)
    with pytest.raises(ValueError):
        zk.g2_srs_powers_device(curve, 3, ks[0], g1_row, buf)
    with pytest.raises(ValueError):
        zk.g2_scalar_mul_rows(curve, ks, np.zeros((2, 4 * n1), dtype=np.uint64))
    with pytest.raises(ValueError):
        zk.g2_scalar_mul_rows(curve, ks, np.zeros((3, 2 * n1), dtype=np.uint64))
