"""Edge values of the four prime fields and big-integer models of the operations the GPU kernels
implement (imported like golden_io.py; needs no GPU).

Python integers are the reference here: arbitrary precision, no code shared with the kernels, the
oracle or the reference C.  tests/test_field_edges_cpu.py checks the models against the oracle and
the reference C before tests/test_gpu_field_edges.py uses them to judge a kernel.

Every value is the RAW word content of a field element as the C ABI carries it: the reference's
Montgomery form with radix R = 2^(64 nlimbs), canonical (< q).  With x' = x R mod q the stored
word of the field element x, and everything mod q:

    add(a, b) = a + b          sub(a, b) = a - b           neg(a) = -a
    mul(a, b) = a b R^-1       sqr(a) = a a R^-1
    inv(a)    = R^2 a^-1       div(a, b) = mul(a, inv(b)) = a b^-1 R
    to_std(a) = a R^-1         from_std(a) = a R
    scale(k, a) = mul(k, a)    mul_add(a, b, c) = mul(a, b) + c     mul_sub(a, b, c) = mul(a, b) - c
    Ax_plus_y(kA, a, b)       = mul(kA, a) + b
    Ax_plus_By(kA, a, kB, b)  = mul(kA, a) + mul(kB, b)
    dot(a, b) = sum_i mul(a_i, b_i)
    powers(a, b, n) = a, mul(a, b), mul(mul(a, b), b), ...   (a b^i in field terms, as arr_powers)
    batch inv / div: one zero input zeroes EVERY output (Fr_mont.c:258-285)
    projective (X : Y : Z) -> affine (mul(X, inv(Z)), mul(Y, inv(Z))) = (X Z^-1 R, Y Z^-1 R)
    Jacobian   (X : Y : Z) -> affine (X Z^-2 R^2, Y Z^-3 R^3)
    (zi = inv(Z) = R^2/Z, zi2 = mul(zi, zi) = R^3/Z^2, zi3 = mul(zi, zi2) = R^4/Z^3,
     x = mul(X, zi2) = X R^2/Z^2, y = mul(Y, zi3) = Y R^3/Z^3: bls12_381_G1_jac.c:120-136);
    Z = 0 gives the all-0xFF affine infinity whatever X and Y are (G1_proj.c:133-145, G1_jac.c:121-125)
"""
import functools
import os
import random
import re

import numpy as np

import golden_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = os.path.join(ROOT, "zikkurat-algebra_amd", "csrc", "zk_params.inc")

P_BN = 21888242871839275222246405745257275088696311157297823662689037894645226208583  # as test_gpu_msm_bits.py
FR = golden_io.FR_ORDER
FP = {"bn128": P_BN, "bls12_381": golden_io.P_BLS}
FIELDS = {"bn128_fp": P_BN, "bn128_fr": FR["bn128"], "bls12_381_fp": golden_io.P_BLS, "bls12_381_fr": FR["bls12_381"]}
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def nlimbs(q):
    return (q.bit_length() + 63) // 64


def radix(q):
    """R = 2^(64 nlimbs), the reference's Montgomery radix"""
    return 1 << (64 * nlimbs(q))


def params():
    """the integer #defines of zk_params.inc: {"ZK_BN128_FP_U_RB": 29, ...}"""
    with open(PARAMS, encoding="utf-8") as f:
        return {k: int(v) for k, v in re.findall(r"^#define (ZK_\w+) (\d+)\s*$", f.read(), re.M)}


def radix_ratio(field):
    """K = R'/R, the ratio of the kernels' internal Montgomery radix R' = 2^(U_RB U_N) to the
    reference's R = 2^(64 N64), read from zk_params.inc (the table in the header comment of
    zk_field.hpp states the same: 2^261 / 2^256 = 32 for the 9 x 29-bit fields, 2^392 / 2^384 = 256
    for BLS12-381 Fp)"""
    d, P = params(), "ZK_" + field.upper()
    return 1 << (d[P + "_U_RB"] * d[P + "_U_N"] - 64 * d[P + "_N64"])


# ---------------------------------------------------------------------------- limbs <-> int
def to_limbs(vals, nl):
    """list of integers -> (n, nl) uint64 rows, little-endian limbs"""
    buf = b"".join(int(v).to_bytes(8 * nl, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u8").astype(np.uint64).reshape(len(vals), nl)


def to_row(v, nl):
    return to_limbs([v], nl)[0]


def from_limbs(a):
    """(n, nl) uint64 rows (or one row) -> list of integers (or one integer)"""
    a = np.ascontiguousarray(a, dtype="<u8")
    if a.ndim == 1:
        return int.from_bytes(a.tobytes(), "little")
    return [int.from_bytes(a[i].tobytes(), "little") for i in range(a.shape[0])]


# ---------------------------------------------------------------------------- edge values
def base_values(q):
    """the part of edge_values that does not depend on K: small and large values, the halves, the
    Montgomery constants, and powers of two at every limb width the kernels and the safegcd use"""
    R, d = radix(q), q.bit_length()
    v = {0, 1, 2, 3, q - 1, q - 2, q - 3, (q - 1) // 2, (q + 1) // 2,
         R % q, R * R % q, q - R % q, 1 << (d - 1), (1 << (d - 1)) - 1}
    for w in (28, 29, 30, 32, 60, 62, 64):
        for j in range(w, d, w):
            v |= {1 << j, (1 << j) - 1}
    assert all(0 <= x < q for x in v)
    return sorted(v)


def edge_values(q, K):
    """deduplicated, sorted canonical integers in [0, q): base_values, the reduction boundaries
    floor(k q / K) and floor(k q / K) + 1 for k = 1 .. K - 1 (the load conversion x R -> K x R
    estimates a quotient from the top limb), and the pre-images e K^-1 of all of these, which put the
    INTERNAL value K v mod q on the same edges"""
    v = set(base_values(q))
    for k in range(1, K):
        v |= {k * q // K, k * q // K + 1}
    Ki = pow(K, -1, q)
    v |= {e * Ki % q for e in v}
    assert all(0 <= x < q for x in v)
    return sorted(v)


def field_edges(field):
    return edge_values(FIELDS[field], radix_ratio(field))


# ---------------------------------------------------------------------------- models (see the module docstring)
class Model:
    """the operations on lists of raw Montgomery words of the field of order q"""

    def __init__(self, q):
        self.q, self.R = q, radix(q)
        self.Ri = pow(self.R, -1, q)
        self.one = self.R % q

    def mul1(self, a, b):
        return a * b * self.Ri % self.q

    def inv1(self, a):
        return self.R * self.R * pow(a, -1, self.q) % self.q if a else 0

    def neg(self, a):
        return [(-x) % self.q for x in a]

    def add(self, a, b):
        return [(x + y) % self.q for x, y in zip(a, b)]

    def sub(self, a, b):
        return [(x - y) % self.q for x, y in zip(a, b)]

    def mul(self, a, b):
        return [self.mul1(x, y) for x, y in zip(a, b)]

    def sqr(self, a):
        return [self.mul1(x, x) for x in a]

    def mul_add(self, a, b, c):
        return [(self.mul1(x, y) + z) % self.q for x, y, z in zip(a, b, c)]

    def mul_sub(self, a, b, c):
        return [(self.mul1(x, y) - z) % self.q for x, y, z in zip(a, b, c)]

    def scale(self, k, a):
        return [self.mul1(k, x) for x in a]

    def Ax_plus_y(self, kA, a, b):
        return [(self.mul1(kA, x) + y) % self.q for x, y in zip(a, b)]

    def Ax_plus_By(self, kA, a, kB, b):
        return [(self.mul1(kA, x) + self.mul1(kB, y)) % self.q for x, y in zip(a, b)]

    def to_std(self, a):
        return [x * self.Ri % self.q for x in a]

    def from_std(self, a):
        return [x * self.R % self.q for x in a]

    def dot(self, a, b):
        return sum(self.mul1(x, y) for x, y in zip(a, b)) % self.q

    def powers(self, a, b, n):
        out = []
        for _ in range(n):
            out.append(a)
            a = self.mul1(a, b)
        return out

    def inv(self, a):
        if any(x == 0 for x in a):  # Fr_mont.c:258-285: one zero input zeroes every output
            return [0] * len(a)
        return [self.inv1(x) for x in a]

    def div(self, a, b):
        if any(y == 0 for y in b):
            return [0] * len(a)
        return [self.mul1(x, self.inv1(y)) for x, y in zip(a, b)]

    def to_affine(self, rows, coords):
        """rows of (X, Y, Z) integers -> rows of (x, y), or None for Z = 0 (the all-0xFF infinity)"""
        out = []
        for X, Y, Z in rows:
            if Z == 0:
                out.append(None)
                continue
            zi = self.inv1(Z)
            if coords == "proj":
                out.append((self.mul1(X, zi), self.mul1(Y, zi)))
            else:
                zi2 = self.mul1(zi, zi)
                out.append((self.mul1(X, zi2), self.mul1(Y, self.mul1(zi, zi2))))
        return out


def fr_model(curve):
    return Model(FR[curve])


def fp_model(curve):
    return Model(FP[curve])


def affine_rows(model, rows, coords):
    """Model.to_affine as the (n, 2 NP) uint64 array batch_to_affine returns"""
    nl = nlimbs(model.q)
    out = np.full((len(rows), 2 * nl), ALL_ONES, dtype=np.uint64)
    for i, xy in enumerate(model.to_affine(rows, coords)):
        if xy is not None:
            out[i] = to_limbs(xy, nl).reshape(-1)
    return out


def point_rows(rows, nl):
    """rows of (X, Y, Z) integers -> (n, 3 nl) uint64"""
    return to_limbs([v for r in rows for v in r], nl).reshape(len(rows), 3 * nl)


def point_ints(a, nl):
    """(n, 3 nl) uint64 -> rows of (X, Y, Z) integers"""
    return [tuple(from_limbs(a[i, k * nl:(k + 1) * nl]) for k in range(3)) for i in range(a.shape[0])]


def rotate(lst, k):
    k %= len(lst)
    return lst[k:] + lst[:k]


def offcurve_rows(curve):
    """(X, Y, Z) rows over the Fp edge set: Z runs over every non-zero edge value, X and Y over
    rotations of the same list.  The rows are NOT curve points."""
    E = [e for e in field_edges(curve + "_fp") if e]
    return list(zip(rotate(E, 1), rotate(E, len(E) // 3), E))


# ---------------------------------------------------------------------------- infinity layouts (k_norm_chunks)
def infinity(model, lam, coords, plain=False):
    """a row at infinity: projective (0 : l : 0), Jacobian (l^2 : l^3 : 0) (the reference's
    jac_is_infinity wants Y^2 = X^3, X, Y != 0), or with plain=True (0 : 1 : 0) in both systems"""
    if plain:
        return (0, model.one, 0)
    if coords == "proj":
        return (0, lam, 0)
    l2 = model.mul1(lam, lam)
    return (l2, model.mul1(l2, lam), 0)


def lane_rows(n, chk):
    """the rows each lane of k_norm_chunks owns: lanes = ceil(n / chk) and lane t owns rows
    t, t + lanes, t + 2 lanes, ... (chk = 2 at the default ZK_NORM_LANES, min(n, 32) at =1)"""
    lanes = -(-n // chk)
    return [list(range(t, n, lanes)) for t in range(lanes)]


def infinity_layouts(n, chk):
    """{name: sorted infinite rows} for n rows at chunk length chk: every layout of a lane's chunk
    that the branch-free path must handle (running product 1, inv(1), first / last element)"""
    lanes = lane_rows(n, chk)
    short = [rows for rows in lanes if len(rows) < len(lanes[0])]  # the ragged tail: lanes one row short
    lay = {"all": range(n),
           "whole_lanes": [r for rows in (lanes[0], lanes[min(1, len(lanes) - 1)], lanes[-1]) for r in rows],
           "first_of_lane": [rows[0] for rows in lanes],
           "second_of_lane": [rows[1] for rows in lanes if len(rows) > 1],
           "last_of_lane": [rows[-1] for rows in lanes if len(rows) > 1],
           "ragged_tail": [rows[-1] for rows in short] if short else [n - 1],
           "only_last_finite": range(n - 1)}
    return {k: sorted(set(v)) for k, v in lay.items()}


# ---------------------------------------------------------------------------- MSM digit patterns (DigitStream::next)
MSM_WINDOWS = (4, 5, 8, 13, 16, 17)
M256 = (1 << 256) - 1


def scalar_from_raw(c, raws):
    """the 256-bit scalar whose window w of c bits PLUS the carry from window w - 1 equals raws[w]
    in the signed-digit recoding (raw > B = 2^(c-1): digit raw - 2^c and carry 1), truncated to
    256 bits (the top window keeps the bits that fit)"""
    B, s, carry = 1 << (c - 1), 0, 0
    for w, raw in enumerate(raws):
        field = raw - carry
        assert 0 <= field < (1 << c)
        s |= field << (c * w)
        carry = 1 if raw > B else 0
    return s & M256


def digit_patterns(curve, c):
    """{name: 256-bit scalar} -- the digit boundaries of window c for 4-limb std scalars (used
    verbatim, W = 256 / c + 1 windows)"""
    B, W, r = 1 << (c - 1), 256 // c + 1, FR[curve]
    top = 255 // c  # the top window that holds scalar bits; window W - 1 is carry-only when c | 256
    return {"raw_B": scalar_from_raw(c, [B] * W),  # positive, no carry
            "raw_Bp1": scalar_from_raw(c, [B + 1] * W),  # negative with a carry, every window
            "raw_Bm1": scalar_from_raw(c, [B - 1] * W),
            "all_ones": M256,  # raw 2^c - 1, then raw 2^c = digit 0 with the carry rippling to the top
            "alt_B_Bp1": scalar_from_raw(c, [B + (w & 1) for w in range(W)]),
            "alt_Bp1_B": scalar_from_raw(c, [B + 1 - (w & 1) for w in range(W)]),
            "two_255": 1 << 255,
            "top_minus_window": (1 << 256) - (1 << c),
            "r_minus_1": r - 1, "r": r, "r_plus_1": r + 1,
            "top_window_only": (1 << 256) - (1 << (c * top))}


def rotl256(s, k):
    k %= 256
    return ((s << k) | (s >> (256 - k))) & M256


def digit_scalars(curve, c, name, n):
    """(n, 4) std scalars: pattern `name` in every row, or for "rotated" every pattern in turn, row i
    rotated left by i bits, so that the rows fall into different buckets"""
    pats = digit_patterns(curve, c)
    if name == "rotated":
        names = sorted(pats)
        return to_limbs([rotl256(pats[names[i % len(names)]], i) for i in range(n)], 4)
    return to_limbs([pats[name]] * n, 4)


DIGIT_PATTERNS = sorted(digit_patterns("bn128", 4)) + ["rotated"]


def digit_points(gen_points, curve, n=192):
    """n distinct points, rows 5 and 100 (where present) the infinity sentinel"""
    pts = gen_points(curve, 0x5A4B0021, n).copy()
    for i in (5, 100):
        if i < n:
            pts[i] = ALL_ONES
    return pts


# ---------------------------------------------------------------------------- group FFT closed form
def fft_expected(oracle, curve, m, affine, inverse):
    """normalised projective rows of the group FFT of the 2^m affine points `affine` (all-0xFF rows
    are infinity) of the order-r subgroup: out[k] = sum_j w^(jk) P_j forward, n^-1 sum_j w^(-jk) P_j
    inverse, each sum one oracle.msm with standard-form scalars from Python's pow.  Finite rows are
    (x : y : 1), infinite rows (0 : 1 : 0) in Montgomery form, in both coordinate systems."""
    r, n = FR[curve], 1 << m
    nl = nlimbs(FP[curve])
    w = from_limbs(oracle.fft_generator(curve, m)) * pow(1 << 256, -1, r) % r
    if inverse:
        w = pow(w, -1, r)
    scale = pow(n, -1, r) if inverse else 1
    one = to_row(radix(FP[curve]) % FP[curve], nl)
    out = np.zeros((n, 3 * nl), dtype=np.uint64)
    fin = [j for j in range(n) if not np.all(affine[j] == ALL_ONES)]  # infinite inputs add nothing
    aff = np.ascontiguousarray(affine[fin])
    for k in range(n):
        sc = to_limbs([pow(w, j * k, r) * scale % r for j in fin], 4)
        xy = oracle.msm(curve, sc, aff, mont=False) if fin else np.full(2 * nl, ALL_ONES)
        if np.all(xy == ALL_ONES):
            out[k, nl:2 * nl] = one
        else:
            out[k, :2 * nl] = xy
            out[k, 2 * nl:] = one
    return out


# ---------------------------------------------------------------------------- Fr test vectors (shared by the CPU and GPU tests)
UNARY = ("neg", "sqr", "to_std", "from_std")
BINARY = ("add", "sub", "mul")
TERNARY = ("mul_add", "mul_sub")


@functools.lru_cache(maxsize=None)
def fr_cross(curve):
    """(a, b, c, ks): (a[i], b[i]) runs over E x E (E x E' with E' = base_values when E x E has more
    than 20 000 rows), c is a rotation of a, ks = (0, R mod r, r - 1, one random value)"""
    r = FR[curve]
    E = field_edges(curve + "_fr")
    E2 = E if len(E) ** 2 <= 20000 else base_values(r)
    a = [x for x in E for _ in E2]
    b = [y for _ in E for y in E2]
    ks = (0, radix(r) % r, r - 1, random.Random(0xED6E).randrange(r))
    return a, b, rotate(a, 7), ks


@functools.lru_cache(maxsize=None)
def fr_cross_expected(curve):
    """{name: (n, 4) uint64} of the big-integer model on fr_cross: every op of
    test_gpu_arr.test_elementwise; the ops with constants once per k as <op>_<i>, kA = ks[i],
    kB = ks[(i + 1) % 4]"""
    a, b, c, ks = fr_cross(curve)
    M = fr_model(curve)
    w = {"neg": M.neg(a), "sqr": M.sqr(a), "to_std": M.to_std(a), "from_std": M.from_std(a),
         "add": M.add(a, b), "sub": M.sub(a, b), "mul": M.mul(a, b),
         "mul_add": M.mul_add(a, b, c), "mul_sub": M.mul_sub(a, b, c), "dot": [M.dot(a, b)]}
    for i, k in enumerate(ks):
        w[f"scale_{i}"] = M.scale(k, a)
        w[f"Ax_plus_y_{i}"] = M.Ax_plus_y(k, a, b)
        w[f"Ax_plus_By_{i}"] = M.Ax_plus_By(k, a, ks[(i + 1) % 4], b)
    return {k: to_limbs(v, 4) for k, v in w.items()}


def element_of_order(q, k):
    """an element of multiplicative order exactly 2^k mod q (standard form)"""
    assert (q - 1) % (1 << k) == 0
    for x in range(2, 100):
        w = pow(x, (q - 1) >> k, q)
        if pow(w, 1 << (k - 1), q) != 1:
            return w
    raise ValueError


POWERS_N = (1, 64, 65, 1000)


def powers_cases(curve):
    """(a, b) raw words for arr_powers: bases 0, the Montgomery one, r - 1 and an element of order
    2^5 (the powers cycle 31 times in 1000), from the Montgomery one and from an edge start"""
    r = FR[curve]
    one = radix(r) % r
    w = element_of_order(r, 5) * radix(r) % r
    return [(one, 0), (one, one), (one, r - 1), (r - 1, r - 1), (one, w), (r - 1, w), (0, w)]


def sqrt_mod(t, q):
    """a square root of t mod q (Tonelli-Shanks), or None for a non-residue"""
    t %= q
    if t == 0:
        return 0
    if pow(t, (q - 1) // 2, q) != 1:
        return None
    s, m = q - 1, 0
    while s % 2 == 0:
        s //= 2
        m += 1
    z = next(x for x in range(2, 200) if pow(x, (q - 1) // 2, q) == q - 1)
    c, x, b = pow(z, s, q), pow(t, (s + 1) // 2, q), pow(t, s, q)
    while b != 1:
        i, b2 = 0, b
        while b2 != 1:
            b2 = b2 * b2 % q
            i += 1
        g = pow(c, 1 << (m - i - 1), q)
        x, b, c, m = x * g % q, b * g * g % q, g * g % q, i
    return x


@functools.lru_cache(maxsize=None)
def fr_targets(curve):
    """inputs whose TRUE result is each edge value t in turn: {op: (inputs..., expected)} with a
    solved for by big integers from t, a random b != 0 and a random c.  "sqr" holds only the t with
    t R a square mod r (both roots are used, one per target in turn)."""
    r = FR[curve]
    R, E = radix(r), field_edges(curve + "_fr")
    rng = random.Random(0x7A26E7)
    b = [rng.randrange(1, r) for _ in E]
    c = [rng.randrange(r) for _ in E]
    bi = [pow(y, -1, r) for y in b]
    out = {"mul": ([t * R * y % r for t, y in zip(E, bi)], b, E),
           "add": ([(t - y) % r for t, y in zip(E, b)], b, E),
           "sub": ([(t + y) % r for t, y in zip(E, b)], b, E),
           "mul_add": ([(t - z) * R * y % r for t, y, z in zip(E, bi, c)], b, c, E)}
    roots = [(t, sqrt_mod(t * R, r)) for t in E]
    sq = [(t, s if i & 1 else (r - s) % r) for i, (t, s) in enumerate(roots) if s is not None]
    out["sqr"] = ([s for _, s in sq], [t for t, _ in sq])
    M = fr_model(curve)  # the solved inputs do give t
    assert M.mul(out["mul"][0], b) == E and M.mul_add(out["mul_add"][0], b, c) == E and M.sqr(out["sqr"][0]) == out["sqr"][1]
    return out


def inv_vectors(curve):
    """[(name, a, b)]: E \\ {0} at lengths 1, 33 and all of it, then the whole vector with one 0 first,
    in the middle and last (the zero rule); a is the numerator of div"""
    r = FR[curve]
    E = [e for e in field_edges(curve + "_fr") if e]
    rows = [(f"n{n}", E[:n]) for n in (1, 33, len(E))]
    for name, pos in (("zero_first", 0), ("zero_middle", len(E) // 2), ("zero_last", len(E) - 1)):
        z = list(E)
        z[pos] = 0
        rows.append((name, z))
    return [(name, rotate(list(reversed(E)), 3)[:len(b)], b) for name, b in rows]


# ---------------------------------------------------------------------------- point rows (shared by the CPU and GPU tests)
LAYOUT_N = (1, 2, 3, 64, 65, 257)


def _coord_points(zk, oracle, curve, coords, n, seed):
    f = golden_io.projective_points if coords == "proj" else golden_io.jacobian_points
    return f(zk, oracle, curve, n, seed, n_inf=0)


def layout_rows(zk, oracle, curve, coords, n, chk, seed):
    """[(name, (n, 3 NP) rows)]: random finite points of golden_io with the infinity layouts of
    infinity_layouts(n, chk), and one case "plain_0_1_0" whose infinities are written (0 : 1 : 0)"""
    base = _coord_points(zk, oracle, curve, coords, n, seed)
    nl, M = nlimbs(FP[curve]), fp_model(curve)
    lam = from_limbs(zk.gen_points(curve, seed + 2, n)[:, :nl])
    lay = infinity_layouts(n, chk)
    out = []
    for name, rows in list(lay.items()) + [("plain_0_1_0", lay["first_of_lane"])]:
        pts = base.copy()
        for i in rows:
            pts[i] = point_rows([infinity(M, lam[i], coords, plain=name == "plain_0_1_0")], nl)[0]
        out.append((name, pts))
    return out


# The reference's PROJECTIVE group FFT is no group FFT where a whole sub-transform is infinite: its
# doubling formula sends (0 : l : 0) to (0 : 0 : 0) (bn128_G1_proj.c:230-260, bls12_381 likewise),
# scl_windowed builds its table with it (:434-438), and the complete addition then returns
# (0 : 0 : 0) for (0 : 0 : 0) + P (:272-317), which normalises to infinity.  A delta input therefore
# loses its point in the reference's projective output, while the reference's Jacobian FFT, whose
# add tests for infinity, returns the group result.  The expected values are the group's
# (fft_expected); the reference's projective C is compared only on the inputs it transforms as a
# group FFT does.
REF_PROJ_FFT_IS_GROUP_FFT = ("all_infinite", "constant")


def fft_inputs(zk, oracle, curve, coords, m):
    """[(name, affine rows, coordinate rows)] of 2^m inputs: all infinite; one finite point at index
    0 / at index n - 1; every row the same point (in different coordinates: random Z per row)"""
    n = 1 << m
    nl, M = nlimbs(FP[curve]), fp_model(curve)
    lam = from_limbs(zk.gen_points(curve, 741 + m, n)[:, :nl])
    inf = point_rows([infinity(M, lam[i], coords) for i in range(n)], nl)
    aff = zk.gen_points(curve, 740 + m, n)
    fin = _coord_points(zk, oracle, curve, coords, n, 740 + m)  # the same affine points with random Z
    out = [("all_infinite", np.full_like(aff, ALL_ONES), inf)]
    for name, i in (("delta_first", 0), ("delta_last", n - 1)):
        a, p = np.full_like(aff, ALL_ONES), inf.copy()
        a[i], p[i] = aff[i], fin[i]
        out.append((name, a, p))
    x, y = from_limbs(aff[0, :nl]), from_limbs(aff[0, nl:])
    const = []
    for X, Y, Z in point_ints(fin, nl):  # (x : y : 1) scaled by the row's Z: (x Z, y Z) or (x Z^2, y Z^3)
        Z2 = M.mul1(Z, Z)
        const.append((M.mul1(x, Z), M.mul1(y, Z), Z) if coords == "proj" else (M.mul1(x, Z2), M.mul1(y, M.mul1(Z2, Z)), Z))
    out.append(("constant", np.tile(aff[0], (n, 1)), point_rows(const, nl)))
    return out


# ---------------------------------------------------------------------------- predicates (shared by the CPU and GPU tests)
PRED_N = (1, 256, 257)
PRED_STRIDE = 4096 * 256  # threads of k_pred's largest grid: rows from here on are reached by its grid-stride loop
PRED_N_LARGE = PRED_STRIDE + 259
PREDICATES = ("is_valid", "is_zero", "is_one", "is_equal")


def valid_rows(curve, n, seed):
    """(n, 4) canonical rows without a Python loop: random low limbs under a top limb below r's own"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, FR[curve] >> 192, size=n, dtype=np.uint64)
    return a


def pred_positions(n):
    """where the offending row goes: first, last, and the second row of the grid-stride loop's second trip"""
    return sorted({0, n - 1} | ({PRED_STRIDE + 1} if n > PRED_STRIDE + 1 else set()))


def is_valid_plants(curve):
    """[(name, row, verdict of is_valid on an otherwise valid array)]: the boundary x < r"""
    r = FR[curve]
    up = to_row(r, 4).copy()
    up[0] += np.uint64(1)  # r with only limb 0 raised by one
    return [("r_minus_1", to_row(r - 1, 4), True), ("r", to_row(r, 4), False), ("r_plus_1", to_row(r + 1, 4), False),
            ("all_ones", to_row(M256, 4), False), ("r_limb0_up", up, False)]


def pred_cases(curve, n, positions, full=True, seed=0x9ED1):
    """yields (label, predicate, operands, expected verdict).  One clean case per predicate (valid rows;
    all zero; all the Montgomery one; an array and its copy), then one offending row at each position:
    is_valid the rows of is_valid_plants, is_zero / is_one a row that differs from the constant in
    exactly one limb (each of the four in turn, one bit of it), is_equal a second array that differs in
    one bit of one limb of that row.  full=False keeps one offending variant per predicate."""
    r = FR[curve]
    a = valid_rows(curve, n, seed)
    zero = np.zeros((n, 4), dtype=np.uint64)
    one = np.tile(to_row(radix(r) % r, 4), (n, 1))
    yield "clean", "is_valid", (a,), True
    yield "clean", "is_zero", (zero,), True
    yield "clean", "is_one", (one,), True
    yield "clean", "is_equal", (a, a.copy()), True
    bits = (0, 63, 31, 62)  # the bit flipped in limb j
    for pos in positions:
        for name, row, verdict in is_valid_plants(curve) if full else is_valid_plants(curve)[1:2]:
            x = a.copy()
            x[pos] = row
            yield f"{name}@{pos}", "is_valid", (x,), verdict
        for j in range(4) if full else (3,):
            flip = np.uint64(1) << np.uint64(bits[j])
            for pred, base in (("is_zero", zero), ("is_one", one)):
                x = base.copy()
                x[pos, j] ^= flip
                yield f"limb{j}@{pos}", pred, (x,), False
            y = a.copy()
            y[pos, j] ^= flip
            yield f"limb{j}@{pos}", "is_equal", (a, y), False


def pred_model(curve, pred, ops):
    """the predicate on Python integers"""
    r = FR[curve]
    x = from_limbs(ops[0])
    if pred == "is_valid":
        return all(v < r for v in x)
    if pred == "is_zero":
        return all(v == 0 for v in x)
    if pred == "is_one":
        return all(v == radix(r) % r for v in x)
    return x == from_limbs(ops[1])
