"""Polynomial division's surface without a GPU: the header declares the new zkg_ entries, the library
exports them and the Python mirror has them, the reference's own names stay unexported, the
precision plan of the series inverse keeps its four properties under every base setting, and a
dividend over the limit is refused on its length alone."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "zkalgebra_gpu.h")
SYMBOLS = ["zkg_poly_long_div_device", "zkg_poly_long_div", "zkg_poly_set_div_base_max", "zkg_poly_div_base_max",
           "zkg_poly_div_plan", "zkg_poly_last_div_steps"]
DIV_ARGS = ["int", "int", "constuint64_t*", "int", "constuint64_t*", "int", "uint64_t*", "int", "uint64_t*"]


def prototype(name):
    txt = open(HEADER).read()
    m = re.search(r"ZKG_API\s+([\w\s\*]+?)\b" + name + r"\s*(\([^;]*\));", txt)
    assert m, f"{name} is not declared in zkalgebra_gpu.h"
    args = m.group(2)[1:-1].split(",")
    return m.group(1).strip(), [re.sub(r"\w+$", "", a.strip()).replace(" ", "") for a in args]


def test_header_declares_division():
    for name in SYMBOLS:
        prototype(name)
    for name in ("zkg_poly_long_div_device", "zkg_poly_long_div"):  # the curve, then the reference's argument list
        assert prototype(name) == ("int", DIV_ARGS)
    assert prototype("zkg_poly_div_plan") == ("int", ["int", "int*", "int"])
    txt = open(HEADER).read()
    assert "quot and rem are NOT provided" not in txt
    assert re.search(r"get_coeff and is_constant are NOT\s+provided", txt)


def test_library_exports_division(zk):
    out = subprocess.check_output(["nm", "-D", "--defined-only", zk.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(SYMBOLS) <= exported, sorted(set(SYMBOLS) - exported)
    assert set(SYMBOLS) <= set(zk.EXTENSION_SYMBOLS)
    for curve in ("bn128", "bls12_381"):  # the reference's own names stay the reference's
        for op in ("get_coeff", "is_constant", "long_div", "quot", "rem"):
            assert f"{curve}_poly_mont_{op}" not in exported


def test_python_mirror_names(zk):
    for name in ("poly_long_div", "poly_quot", "poly_rem", "poly_long_div_device", "poly_set_div_base_max",
                 "poly_div_base_max", "poly_div_plan", "poly_last_div_steps"):
        assert callable(getattr(zk, name)), name


PLAN_M = list(range(1, 301)) + [(1 << 12) - 1, (1 << 12) + 1, (1 << 16) + 3, (1 << 20) - 64]


@pytest.mark.parametrize("setting", [1, 4, -1, 1 << 30])
def test_plan_properties(zk, setting):
    lib = zk.load()
    try:
        zk.poly_set_div_base_max(setting)
        base = zk.poly_div_base_max()
        assert base >= 1
        if setting in (1, 4):
            assert base == setting
        for m in PLAN_M:
            s = 0
            while base << s < m:  # the smallest s with base * 2^s >= m
                s += 1
            prec = (ctypes.c_int * 64)(*([-7] * 64))
            assert lib.zkg_poly_div_plan(m, prec, 64) == s, m
            prec = list(prec)
            assert all(v == -7 for v in prec[s + 1:])
            assert 1 <= prec[0] <= base, m
            for i in range(s):
                assert prec[i] < prec[i + 1] <= 2 * prec[i], (m, prec[:s + 1])
            assert prec[s] == m
            assert zk.poly_div_plan(m) == prec[:s + 1]
    finally:
        zk.poly_set_div_base_max(-1)


def test_plan_edges(zk):
    lib = zk.load()
    try:
        zk.poly_set_div_base_max(0)  # 0 and 1: a one-term seed
        assert zk.poly_div_base_max() == 1
        zk.poly_set_div_base_max(1 << 30)
        cap = zk.poly_div_base_max()
        zk.poly_set_div_base_max(-1)
        assert 1 <= zk.poly_div_base_max() <= cap < 1 << 30
        for m in (0, -1, -(1 << 20)):
            prec = (ctypes.c_int * 4)(-7, -7, -7, -7)
            assert lib.zkg_poly_div_plan(m, prec, 4) == -1
            assert list(prec) == [-7] * 4
            assert zk.poly_div_plan(m) is None
        zk.poly_set_div_base_max(1)
        prec = (ctypes.c_int * 8)(*([-7] * 8))
        assert lib.zkg_poly_div_plan(1000, prec, 3) == 10  # cap below s + 1: only cap entries are written
        assert list(prec) == [1, 2, 4] + [-7] * 5
        assert lib.zkg_poly_div_plan(1000, None, 0) == 10
    finally:
        zk.poly_set_div_base_max(-1)


def test_oversized_dividend_is_refused_on_its_length(zk):
    """null operands: -1 comes back before a pointer is read, and without a GPU"""
    for curve, lg in (("bn128", 27), ("bls12_381", 29)):
        assert zk.poly_long_div_device(curve, (1 << lg) + 1, None, 2, None, 1 << 20, None, 1, None) == -1
        assert zk.load().zkg_poly_long_div(zk.CURVE_ID[curve], (1 << lg) + 1, None, 2, None, 0, None, 0, None) == -1
    assert zk.load().zkg_poly_long_div(0, -1, None, 2, None, 0, None, 0, None) == -1  # a negative length
    assert zk.poly_last_div_steps() == -1
    assert zk.last_error() is None  # a return code, not an error
