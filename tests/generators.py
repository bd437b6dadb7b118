"""Generators of the order-2^m subgroup of Fr other than the canonical one (imported like
field_edges.py; needs no GPU).

Every transform entry point takes the subgroup generator as an argument, and the header only asks for
a Montgomery generator of the order-2^m subgroup.  With g the canonical generator of that subgroup
(zkg_fft_generator / oracle.fft_generator), the named roots are the powers g^k:

    inv   k = 2^m - 1      g^-1
    cube  k = 3
    neg   k = 2^(m-1) + 1  -g        (m >= 2)
    k5    k = 5                      (m >= 3)

Only odd k are used (k = 0 at m = 0, where the subgroup is {1}): g^k is then a PRIMITIVE 2^m-th root of
unity, (g^k)^(2^(m-1)) = -1.  The reference's recursion (<C>_poly_mont_ntt_forward_noalloc) computes the
DFT only for such a generator; generators of the wrong order are outside the contract of every entry
point and out of scope here.

Names whose exponent repeats an earlier one mod 2^m are dropped, as are names that need a larger m:
m = 0 keeps only inv (= 1), m = 1 only inv (= -1, the canonical generator itself), m = 2 only inv
(= neg = cube), m = 3 inv, cube and neg (k5 = neg)."""
import numpy as np

from field_edges import FR, from_limbs, fr_model, to_row

NAMES = ("inv", "cube", "neg", "k5")


def all_exponents(m):
    """{name: k mod 2^m} of every name that exists at m, duplicates included"""
    n = 1 << m
    cand = [("inv", n - 1, 0), ("cube", 3, 0), ("neg", n // 2 + 1, 2), ("k5", 5, 3)]
    return {name: k % n for name, k, min_m in cand if m >= min_m}


def exponents(m):
    """{name: k} in the order of NAMES, the first name wins among equal k mod 2^m"""
    out = {}
    for name, k in all_exponents(m).items():
        if k not in out.values():
            out[name] = k
    return out


def to_std(curve, row):
    """one Montgomery row -> the integer it stands for"""
    M = fr_model(curve)
    return from_limbs(np.ascontiguousarray(row, dtype=np.uint64)) * M.Ri % M.q


def from_std(curve, v):
    """an integer mod r -> its Montgomery row"""
    M = fr_model(curve)
    return to_row(v % M.q * M.R % M.q, 4)


def roots(curve, m, gen_row):
    """{name: (4,) uint64 Montgomery row of gen^k} for the canonical generator row `gen_row` of the
    order-2^m subgroup"""
    r = FR[curve]
    g = to_std(curve, gen_row)
    assert pow(g, 1 << m, r) == 1 and (m == 0 or pow(g, 1 << (m - 1), r) == r - 1), "not a generator of order 2^m"
    return {name: from_std(curve, pow(g, k, r)) for name, k in exponents(m).items()}


def root(curve, m, gen_row, name):
    """one named root; a name dropped as a duplicate at small m gives the row of the name it repeats
    (cube at m = 2 is inv)"""
    r = FR[curve]
    return from_std(curve, pow(to_std(curve, gen_row), all_exponents(m)[name], r))


def names(m, only=None):
    """the names that exist at m, restricted to `only` when given"""
    return [k for k in exponents(m) if only is None or k in only]


def naive_dft(curve, m, gen_row, x, inverse=False):
    """(2^m, 4) Montgomery rows: out[k] = sum_j x_j gen^(jk), or 1/N sum_j x_j gen^(-jk), in Python integers"""
    r, n = FR[curve], 1 << m
    M = fr_model(curve)
    w = to_std(curve, gen_row)
    if inverse:
        w = pow(w, -1, r)
    scale = pow(n, -1, r) if inverse else 1
    xs = [v * M.Ri % r for v in from_limbs(np.ascontiguousarray(x, dtype=np.uint64).reshape(n, 4))]
    pw = [pow(w, e, r) for e in range(n)]
    out = [sum(xs[j] * pw[j * k % n] for j in range(n)) * scale % r * M.R % r for k in range(n)]
    return np.stack([to_row(v, 4) for v in out])
