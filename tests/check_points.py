"""Point builders and the reference oracle of the batch point validation tests (tests/test_gpu_check.py,
tests/test_check_cpu.py).  Rows are built on Python integers (tools/gen_subgroup.py's curve arithmetic) and
handed over in the library's layout: Montgomery words, Fp2 as c0 || c1.

A pool is a fixed set of labelled rows of one (curve, group, coordinate system); its expected flags come from
the reference once per session: canonical by integer compare, on-curve / infinity from the reference's
predicates, membership as is_infinity(scl_Fr_std(r, P))."""
import ctypes
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_subgroup as gs  # noqa: E402

import golden_io  # noqa: E402

CURVES = ("bn128", "bls12_381")
GS_NAME = {"bn128": "BN254", "bls12_381": "BLS381"}
NP1 = {"bn128": 4, "bls12_381": 6}
COORDS = {1: ("affine", "proj", "jac"), 2: ("affine", "proj")}
CANONICAL, ON_CURVE, IN_SUBGROUP, INFINITY = 1, 2, 4, 8
# rows per pool: 3 x 400 (G1) and 2 x 600 (G2) reference multiplications per (curve, group)
POOL_ROWS = {1: 400, 2: 600}
SIZES = (1, 63, 64, 65, 257, 1000)


def params(curve):
    c = gs.CURVES[GS_NAME[curve]]
    return c["p"], c["r"]


def curve_of(curve, group):
    """tools/gen_subgroup.py's Curve of E(Fp) (group 1, coordinates (v, 0)) or of the twist E'(Fp2)"""
    c = gs.CURVES[GS_NAME[curve]]
    p = c["p"]
    if group == 1:
        return gs.Curve(p, (c["b"], 0))
    E0 = gs.Curve(p, (0, 0))
    return gs.Curve(p, E0.fmul((c["b"], 0), E0.finv(c["xi"]) if c["dtype"] else c["xi"]))


def group_order(curve, group):
    p, r = params(curve)
    if curve == "bn128":
        return r if group == 1 else r * (2 * p - r)
    z = gs.BLS_Z
    if group == 1:
        return (z - 1) ** 2 // 3 * r
    return (z ** 8 - 4 * z ** 7 + 5 * z ** 6 - 4 * z ** 4 + 6 * z ** 3 - 4 * z ** 2 - 4 * z + 13) // 9 * r


def words(v, n):
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(n)]


def fe_words(curve, group, a, raw=False):
    """words of one coordinate: a an Fp2 pair of standard integers (raw: the integers are stored as they are)"""
    p, _ = params(curve)
    NP = NP1[curve]
    R = 1 << (64 * NP)
    m = (lambda v: v) if raw else (lambda v: v * R % p)
    return words(m(a[0]), NP) + (words(m(a[1]), NP) if group == 2 else [])


def fe_ints(curve, group, row):
    """the standard integers (Fp2 pair) of one coordinate's Montgomery words"""
    p, _ = params(curve)
    NP = NP1[curve]
    Rinv = pow(1 << (64 * NP), -1, p)
    v = [sum(int(row[k * NP + j]) << (64 * j) for j in range(NP)) for k in range(group)]
    return (v[0] * Rinv % p, v[1] * Rinv % p if group == 2 else 0)


def affine_of(E, P):
    """(x, y) of a finite Jacobian point of gen_subgroup.Curve"""
    zi = E.finv(P[2])
    zi2 = E.fmul(zi, zi)
    return E.fmul(P[0], zi2), E.fmul(P[1], E.fmul(zi2, zi))


def encode(curve, group, coords, E, xy, rnd, scale=True):
    """the row of the finite affine point xy in `coords`, projective / Jacobian rows scaled by a random Z"""
    x, y = xy
    if coords == "affine":
        cs = [x, y]
    else:
        z = (rnd.randrange(2, E.p), rnd.randrange(E.p) if group == 2 else 0) if scale else (1, 0)
        z2 = E.fmul(z, z)
        cs = [E.fmul(x, z), E.fmul(y, z), z] if coords == "proj" else [E.fmul(x, z2), E.fmul(y, E.fmul(z2, z)), z]
    return sum((fe_words(curve, group, c) for c in cs), [])


def small_order_points(curve, group, rnd):
    """{order: affine point} of prime orders dividing the cofactor: 3 and 11 on BLS12-381 G1, 13 and 23 on its
    twist; BN254's twist has no small factor (its smallest is 10069, used all the same)"""
    want = {("bls12_381", 1): (3, 11), ("bls12_381", 2): (13, 23), ("bn128", 2): (10069,)}.get((curve, group), ())
    E = curve_of(curve, group)
    n = group_order(curve, group)
    out = {}
    for q in want:
        e = 0
        while n % q ** (e + 1) == 0:
            e += 1
        while q not in out:
            T = E.mul(n // q ** e, E.random_point(rnd, group == 1))
            while not E.is_inf(T) and not E.is_inf(E.mul(q, T)):
                T = E.mul(q, T)
            if not E.is_inf(T):
                out[q] = affine_of(E, T)
    return out


def subgroup_points(zk, reflib, curve, group, n, seed):
    """n affine points of the order-r subgroup as (x, y) integer pairs: the library's generator (G1) or the
    reference's G2 generator multiples (golden_io.g2_points)"""
    rows = zk.gen_points(curve, seed, n) if group == 1 else golden_io.g2_points(reflib, curve, n, k0=seed & 0xFFFF)
    w = group * NP1[curve]
    return [(fe_ints(curve, group, r[:w]), fe_ints(curve, group, r[w:])) for r in rows]


def build_pool(zk, reflib, curve, group, coords, seed=0x5A4B31):
    """(rows (POOL_ROWS x words) uint64, labels): the row mix of the point validation tests"""
    rnd = random.Random(seed + 7 * group + (0 if curve == "bn128" else 1000) + COORDS[1].index(coords))
    E = curve_of(curve, group)
    p, r = params(curve)
    NP = NP1[curve]
    w = group * NP
    nc = 2 if coords == "affine" else 3
    total = POOL_ROWS[group]
    rows, labels = [], []

    def put(row, label):
        assert len(row) == nc * w, label
        rows.append(row)
        labels.append(label)

    sub = subgroup_points(zk, reflib, curve, group, total + 100, seed & 0xFFFF)
    small = small_order_points(curve, group, rnd)
    zero, one = (0, 0), (1, 0)
    # infinity in every encoding of the coordinate system, and the near misses
    if coords == "affine":
        put([0xFFFFFFFFFFFFFFFF] * (2 * w), "infinity")
        put([0xFFFFFFFFFFFFFFFF] * w + fe_words(curve, group, sub[0][1]), "ff in x only")
        put(fe_words(curve, group, sub[0][0]) + [0xFFFFFFFFFFFFFFFF] * w, "ff in y only")
        put([0] * (2 * w), "(0, 0)")
    elif coords == "proj":
        put(sum((fe_words(curve, group, c) for c in (zero, one, zero)), []), "infinity (0 : 1 : 0)")
        put(sum((fe_words(curve, group, c) for c in (zero, sub[1][1], zero)), []), "infinity (0 : y : 0)")
        put(sum((fe_words(curve, group, c) for c in (sub[1][0], sub[1][1], zero)), []), "(X : Y : 0), X != 0")
        put([0] * (3 * w), "(0 : 0 : 0)")
        put(sum((fe_words(curve, group, c) for c in (one, zero, zero)), []), "(1 : 0 : 0)")
    else:
        put(sum((fe_words(curve, group, c) for c in (one, one, zero)), []), "infinity (1 : 1 : 0)")
        l = (rnd.randrange(2, p), 0)
        l2 = E.fmul(l, l)
        put(sum((fe_words(curve, group, c) for c in (l2, E.fmul(l2, l), zero)), []), "infinity (l^2 : l^3 : 0)")
        put(sum((fe_words(curve, group, c) for c in (l2, l2, zero)), []), "(X : Y : 0), Y^2 != X^3")
        put([0] * (3 * w), "(0 : 0 : 0)")
        put(sum((fe_words(curve, group, c) for c in (zero, one, zero)), []), "(0 : 1 : 0)")
    # non-canonical rows: one coordinate component equal to p, p + 1, 2^(64 NP) - 1
    good = encode(curve, group, coords, E, sub[2], rnd)
    for v, name in ((p, "p"), (p + 1, "p + 1"), ((1 << (64 * NP)) - 1, "2^(64 NP) - 1")):
        for comp in range(nc * group):
            row = list(good)
            row[comp * NP:(comp + 1) * NP] = words(v, NP)
            put(row, f"component {comp} = {name}")
    # on the curve, outside the subgroup
    h = group_order(curve, group) // r
    outside = []
    if h > 1:
        for q, T in small.items():
            outside.append((T, f"order {q}"))
        if (curve, group) == ("bls12_381", 1):
            for row in golden_io.bls_nonsubgroup_points(8, seed):
                outside.append(((fe_ints(curve, 1, row[:6]), fe_ints(curve, 1, row[6:])), "golden non-subgroup"))
        for _ in range(12):
            outside.append((affine_of(E, E.random_point(rnd, group == 1)), "random curve point"))
        for i, (q, T) in enumerate(small.items()):
            for j in range(3):
                G = sub[10 + 3 * i + j]
                S = E.add((G[0], G[1], one), (T[0], T[1], one))
                outside.append((affine_of(E, S), f"G + T, T of order {q}"))
    for xy, label in outside:
        put(encode(curve, group, coords, E, xy, rnd), label)
    # off the curve: one bit of x or y flipped (kept canonical: a low bit)
    for i in range(24):
        row = encode(curve, group, coords, E, sub[40 + i], rnd)
        row[(i % (2 * group)) * NP] ^= 1 << (i % 40)
        put(row, "one bit flipped")
    # the rest: subgroup points, Z = 1 on every fourth projective / Jacobian row
    i = 100
    while len(rows) < total:
        put(encode(curve, group, coords, E, sub[i], rnd, scale=i % 4 != 0), "subgroup")
        i += 1
    return np.array(rows, dtype=np.uint64), labels


def reference_flags(reflib, curve, group, coords, rows):
    """expected flag bytes of `rows`, from the reference (canonical: integer compare)"""
    p, r = params(curve)
    NP = NP1[curve]
    w = group * NP
    nc = 2 if coords == "affine" else 3
    pre = f"{curve}_G{group}_"
    fn = lambda name, res=ctypes.c_uint8: _cfun(reflib, pre + name, res)
    on_curve, is_inf = fn(f"{coords}_is_on_curve"), fn(f"{coords}_is_infinity")
    sys_ = "proj" if coords == "affine" else coords
    scl, sys_inf = fn(f"{sys_}_scl_Fr_std", None), fn(f"{sys_}_is_infinity")
    from_aff = fn("proj_from_affine", None)
    rw = np.array(words(r, 4), dtype=np.uint64)
    out = np.zeros(rows.shape[0], dtype=np.uint8)
    for i in range(rows.shape[0]):
        row = np.ascontiguousarray(rows[i])
        comps = [sum(int(row[k * NP + j]) << (64 * j) for j in range(NP)) for k in range(nc * group)]
        ones = all(int(v) == 0xFFFFFFFFFFFFFFFF for v in row)
        if not (all(c < p for c in comps) or (coords == "affine" and ones)):
            continue
        f = CANONICAL
        inf = bool(is_inf(row.ctypes.data))
        if on_curve(row.ctypes.data) and inf:
            # infinity is a member by the contract; the reference's windowed projective multiplication does not
            # return its own infinity encoding for an infinite input, so it is not asked
            f |= ON_CURVE | IN_SUBGROUP
        elif on_curve(row.ctypes.data):
            f |= ON_CURVE
            pt = row
            if coords == "affine":
                pt = np.zeros(3 * w, dtype=np.uint64)
                from_aff(row.ctypes.data, pt.ctypes.data)
            res = np.zeros(3 * w, dtype=np.uint64)
            scl(rw.ctypes.data, pt.ctypes.data, res.ctypes.data)
            if sys_inf(res.ctypes.data):
                f |= IN_SUBGROUP
        if inf:
            f |= INFINITY
        out[i] = f
    return out


_CFUN = {}


def _cfun(lib, name, restype):
    if name not in _CFUN:
        f = getattr(lib, name)
        f.restype = restype
        f.argtypes = [ctypes.c_void_p] * (1 if restype is not None else (3 if "scl" in name else 2))
        _CFUN[name] = f
    return _CFUN[name]


_POOLS = {}


def pool(zk, reflib, curve, group, coords):
    """(rows, labels, expected flags) of one pool, built and sent through the reference once per session"""
    key = (curve, group, coords)
    if key not in _POOLS:
        rows, labels = build_pool(zk, reflib, curve, group, coords)
        _POOLS[key] = (rows, labels, reference_flags(reflib, curve, group, coords, rows))
    return _POOLS[key]


def case_indices(curve, group, coords, n):
    """pool indices of the n rows of a case: shuffled; every pool row is in the n = 1000 case, the special rows
    come first in the draw so that the small cases hold them too"""
    total = POOL_ROWS[group]
    rnd = random.Random(n * 31 + group)
    if n >= total:
        idx = list(range(total)) + [rnd.randrange(total) for _ in range(n - total)]
    else:
        special = list(range(min(total, 120)))
        rnd.shuffle(special)
        idx = (special + [rnd.randrange(total) for _ in range(n)])[:n]
    rnd.shuffle(idx)
    return np.array(idx, dtype=np.int64)
