"""The polynomial layer's surface without a GPU: the header declares every reference name with the
parameter types of the reference's definitions, the library exports them, the Python mirror has
them, and the big-integer models of the product's two sizing rules (tools/poly_bounds.py) hold."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import poly_bounds  # noqa: E402

CURVES = ["bn128", "bls12_381"]
PART1 = ["degree", "is_zero", "is_equal", "neg", "add", "sub", "scale", "lincomb", "mul_naive", "eval_at"]
PART2 = ["zkg_poly_mul_device", "zkg_poly_eval_device", "zkg_poly_lincomb_device", "zkg_poly_set_mul_direct_max",
         "zkg_poly_last_mul_path"]
HEADER = os.path.join(ROOT, "include", "zkalgebra_gpu.h")


def ptypes(proto):
    """parameter types of a prototype or definition head, names and spaces dropped"""
    args = proto[proto.index("(") + 1:proto.rindex(")")].split(",")
    return [re.sub(r"\w+$", "", a.strip()).replace(" ", "") for a in args]


def our_prototype(name):
    txt = open(HEADER).read()
    m = re.search(r"ZKG_API\s+([\w\s\*]+?)\b" + name + r"\s*(\([^;]*\));", txt)
    assert m, f"{name} is not declared in zkalgebra_gpu.h"
    return m.group(1).strip(), m.group(2)


@pytest.mark.parametrize("curve", CURVES)
def test_header_declares_polynomial_layer(curve):
    for op in PART1:
        our_prototype(f"{curve}_poly_mont_{op}")
    for name in PART2:
        our_prototype(name)
    assert our_prototype(f"{curve}_poly_mont_degree")[0] == "int"
    assert ptypes(our_prototype(f"{curve}_poly_mont_degree")[1]) == ["int", "constuint64_t*"]  # the .c, not the .h
    for op in ("is_zero", "is_equal"):
        assert our_prototype(f"{curve}_poly_mont_{op}")[0] == "uint8_t"


@pytest.mark.parametrize("curve", CURVES)
def test_parameter_types_equal_the_reference_definitions(curve):
    path = f"/root/reference/lib/cbits/curves/poly/mont/{curve}_poly_mont.c"
    if not os.path.exists(path):
        pytest.skip("reference tree not present")
    src = open(path).read()
    for op in PART1:
        name = f"{curve}_poly_mont_{op}"
        m = re.search(r"^(\w+)\s+" + name + r"\s*(\([^{]*\))\s*\{", src, re.M)
        assert m, name
        ret, args = m.group(1), re.sub(r"//[^\n]*", "", m.group(2))
        ours_ret, ours_args = our_prototype(name)
        assert ours_ret == ret, name
        assert ptypes(ours_args) == ptypes(args), name


def test_library_exports_polynomial_layer(zk):
    out = subprocess.check_output(["nm", "-D", "--defined-only", zk.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    want = {f"{c}_poly_mont_{op}" for c in CURVES for op in PART1} | set(PART2)
    assert want <= exported, sorted(want - exported)
    assert want <= set(zk.REFERENCE_SYMBOLS) | set(zk.EXTENSION_SYMBOLS)
    for op in ("get_coeff", "is_constant", "long_div", "quot", "rem"):  # named as not provided
        assert f"bn128_poly_mont_{op}" not in exported


def test_python_mirror_names(zk):
    for name in ("poly_mul", "poly_sqr", "poly_eval_at", "poly_add", "poly_sub", "poly_neg", "poly_scale",
                 "poly_lincomb", "poly_is_zero", "poly_is_equal", "poly_degree", "poly_mul_device",
                 "poly_eval_device", "poly_lincomb_device", "poly_set_mul_direct_max", "poly_last_mul_path"):
        assert callable(getattr(zk, name)), name


def kernel_constant(name):
    txt = open(os.path.join(ROOT, "zikkurat-algebra_amd", "csrc", "zk_poly.hip")).read()
    return int(re.search(r"constexpr int " + name + r" = (\d+);", txt).group(1))


def test_model_constants_are_the_kernels():
    assert kernel_constant("LAZY_J") == poly_bounds.LAZY_J
    assert kernel_constant("POLY_MUL_MIN_LOG") == poly_bounds.MIN_LOG
    hpp = open(os.path.join(ROOT, "zikkurat-algebra_amd", "csrc", "zk_poly.hpp")).read()
    bn, bls = re.search(r"POLY_MUL_MAX_LOG\[2\] = \{(\d+), (\d+)\}", hpp).groups()
    assert {"bn128": int(bn), "bls12_381": int(bls)} == poly_bounds.MAX_LOG


@pytest.mark.parametrize("curve", CURVES)
def test_accumulation_bound_all_r_minus_1(curve):
    """LAZY_J products of the all-(r - 1) operand with the largest converted short-factor value share
    one reduction: the 64-bit column accumulator does not overflow, the result is exact and < 2r;
    one product more breaks the analytic bound, so the constant is as large as the bound allows"""
    p = poly_bounds.fr_orders()[curve]
    ratio, bits = poly_bounds.check(p)
    assert ratio < 2 and bits <= 64
    for j in range(1, poly_bounds.LAZY_J + 1):  # every partial chunk the kernels run
        val, peak = poly_bounds.worst(p, j)
        assert peak < 1 << 64 and val < 2 * p
        assert (val * poly_bounds.RP - j * (p - 1) * (2 * p - 1)) % p == 0
    assert poly_bounds.largest_j(p) >= poly_bounds.LAZY_J
    # all-ones limbs on both sides, beyond what either operand can be: the accumulator still fits
    ones = (1 << (poly_bounds.N * poly_bounds.RB)) - 1
    assert poly_bounds.replay(p, [(ones, ones)] * poly_bounds.LAZY_J)[1] < 1 << 64


@pytest.mark.parametrize("curve", CURVES)
def test_padded_transform_length(curve):
    mx = poly_bounds.MAX_LOG[curve]
    for n1, n2 in [(1, 1), (2, 1), (9, 8), (9, 9), (32, 33), (33, 33), (1025, 1024), (2049, 2047), (4097, 1),
                   ((1 << 16) + 1, 1 << 16), ((1 << 17) + 3, 1 << 15), (1 << (mx - 1), (1 << (mx - 1)) + 1)]:
        m = poly_bounds.transform_log(curve, n1, n2)
        n = n1 + n2 - 1
        assert m >= poly_bounds.MIN_LOG and (1 << m) >= n  # the cyclic product does not wrap
        assert m == poly_bounds.MIN_LOG or (1 << (m - 1)) < n  # and is not padded twice over
    assert poly_bounds.transform_log(curve, 1 << mx, 2) == -1
    assert poly_bounds.transform_log(curve, 1 << mx, 1) == mx
    assert poly_bounds.transform_log(curve, 0, 5) is None
