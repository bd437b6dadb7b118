"""Big-integer models of the polynomial layer's two sizing rules (zk_poly.hip); no GPU.

1. lazy accumulation (k_poly_mul_direct, k_poly_lincomb): LAZY_J products x_i * s_i share one
   Montgomery reduction.  `replay` runs cols_add + redc_cols on Python integers, limb for limb as
   the kernel does, and records the largest value the 64-bit column accumulator takes; `worst`
   feeds it the operands the kernel can meet: x canonical (< r, all r - 1 here), s any value < 2r
   with normalised limbs (fe_to_int's output range), both as all-ones limbs where the range allows.
2. padded transform length of the NTT product: m = max(4, ceil(log2(n1 + n2 - 1))), refused above
   2^28 (bn128) / 2^30 (bls12_381).

    python3 tools/poly_bounds.py      prints the table quoted in DESIGN.md
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, RB = 9, 29
MASK = (1 << RB) - 1
RP = 1 << (N * RB)  # R' = 2^261
LAZY_J = 6
MIN_LOG = 4
MAX_LOG = {"bn128": 28, "bls12_381": 30}


def fr_orders():
    txt = open(os.path.join(ROOT, "zikkurat-algebra_amd", "csrc", "zk_params.inc")).read()
    out = {}
    for curve, pfx in (("bn128", "ZK_BN128_FR"), ("bls12_381", "ZK_BLS12_381_FR")):
        limbs = re.search(r"#define " + pfx + r"_U_P \{([^}]*)\}", txt).group(1)
        out[curve] = sum(int(v.strip().rstrip("uU"), 0) << (RB * i) for i, v in enumerate(limbs.split(",")))
    return out


def limbs(x):
    return [(x >> (RB * i)) & MASK for i in range(N)]


def replay(p, pairs):
    """(value of redc(sum x_i s_i), largest accumulator value) for operand pairs given as integers"""
    pl = limbs(p)
    minv = (-pow(p, -1, 1 << RB)) & MASK
    T = [0] * (2 * N - 1)
    peak = 0
    for x, s in pairs:
        xl, sl = limbs(x), limbs(s)
        assert x >> (N * RB) == 0 and s >> (N * RB) == 0
        for i in range(N):
            for j in range(N):
                T[i + j] += xl[i] * sl[j]
    peak = max(T)
    m, o, acc = [0] * N, [0] * N, 0
    for k in range(N):
        acc += T[k] + sum(m[i] * pl[k - i] for i in range(k))
        m[k] = (acc * minv) & MASK
        acc += m[k] * pl[0]
        peak = max(peak, acc)
        assert acc & MASK == 0
        acc >>= RB
    for k in range(N, 2 * N - 1):
        acc += T[k] + sum(m[i] * pl[k - i] for i in range(k - N + 1, N))
        peak = max(peak, acc)
        o[k - N] = acc & MASK
        acc >>= RB
    o[N - 1] = acc
    return sum(v << (RB * i) for i, v in enumerate(o)), peak


def worst(p, J=LAZY_J):
    """the all-(r - 1) operand against the largest s < 2r, J times"""
    return replay(p, [(p - 1, 2 * p - 1)] * J)


def check(p, J=LAZY_J):
    """the three statements of zk_poly.hip's header comment; returns (value / p, log2 peak)"""
    val, peak = worst(p, J)
    assert peak < 1 << 64, "column accumulator overflows"
    assert val < 2 * p, "reduced value leaves fe_add's input range"
    assert (val * RP - J * (p - 1) * (2 * p - 1)) % p == 0, "reduction is not exact"
    # the analytic bound covers every operand, not only this one
    assert (J + 1) * N * MASK * MASK + (1 << 35) < 1 << 64
    assert J * 2 * p * p + RP * p < 2 * p * RP
    return val / p, peak.bit_length()


def largest_j(p):
    """largest J for which the analytic bound holds"""
    j = 1
    while (j + 2) * N * MASK * MASK + (1 << 35) < 1 << 64 and (j + 1) * 2 * p * p + RP * p < 2 * p * RP:
        j += 1
    return j


def transform_log(curve, n1, n2):
    """log2 of the padded transform of an n1 x n2 product, None where nothing is transformed
    (an empty factor), -1 where the product is refused"""
    n = n1 + n2 - 1
    if n1 <= 0 or n2 <= 0:
        return None
    if n > 1 << MAX_LOG[curve]:
        return -1
    return max(MIN_LOG, (n - 1).bit_length())


if __name__ == "__main__":
    for curve, p in fr_orders().items():
        v, b = check(p)
        print(f"{curve}: J = {LAZY_J}: reduced value {v:.3f} p, accumulator peak < 2^{b}; largest J = {largest_j(p)}")
