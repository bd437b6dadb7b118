#!/usr/bin/env python3
"""Emit the instruction streams of the pairing kernels (zikkurat-algebra_amd/csrc/zk_pairing_prog.inc).

The pairing kernel (zk_pairing_impl.hpp k_pair_vm) is one interpreter over a per-lane workspace of Fp2
cells: every Fp2 / Fp12 operation exists once in the code object, and the Miller loop and the final
exponentiation are flat streams of (op, d, a, b) words with no data-dependent control flow.  The streams
are written from the mathematics here (the same formulas as tests/pairing_model.py, which also holds the
big-integer interpreter the CPU tests run them with):

  miller   f = Miller function of (P, Q) into slot F (BN254: 6x+2 and the two Frobenius lines; BLS12-381: |x|)
  fexp     slot F <- F^((p^12 - 1)/r): F^(p^6 - 1) by conjugate / inverse, ^(p^2 + 1), then the hard part
           by powers of x:  BN254  (p^4 - p^2 + 1)/r = l0 + l1 p + l2 p^2 + p^3 (Scott et al.'s addition
           chain over y0 .. y6);  BLS12-381  (p^4 - p^2 + 1)/r = (x - 1)^2/3 (x + p)(x^2 + p^2 - 1) + 1.
           Both identities are asserted below on the integers, so the exponent is exact.

Cells: slots of six cells (an Fp12 value, coefficients of 1, w, .., w^5) from cell 0, named cells after them.
"""
import os

OPS = ["END", "MUL2", "SQR2", "ADD2", "SUB2", "NEG2", "CONJ2", "COPY2", "LDC", "INV2",
       "MUL12", "SQR12", "SPMUL12", "FROB12", "CONJ12", "COPY12", "ONE12"]
OP = {n: i for i, n in enumerate(OPS)}
NSLOT = 8
F = 0
BASE = 6 * NSLOT
XP, YP, QX, QY, TX, TY, TZ, L0, L1, L2, Q1X, Q1Y, Q2X, Q2Y = range(BASE, BASE + 14)
T0 = BASE + 14
NCELL = T0 + 12
C_GAMMA, C_BT, C_ONE = 0, 6, 7   # constant indices (LDC): gamma[0..5], b', one

X = {"bn128": 4965661367192848881, "bls12_381": -0xD201000000010000}
PR = {
    "bn128": (0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47,
              0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001),
    "bls12_381": (0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB,
                  0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001),
}


class Prog:
    def __init__(self):
        self.ins = []
        self.free = []

    def e(self, op, d, a=0, b=0):
        assert max(d, a, b) < 256
        self.ins.append(OP[op] | d << 8 | a << 16 | b << 24)

    def t(self, i): return T0 + i

    # ---- slot values (an allocator over the slots that are free)
    def take(self):
        return self.free.pop()
    def give(self, *slots):
        for s in slots:
            assert s not in self.free
            self.free.append(s)
    def mul(self, a, b):
        d = self.take()
        self.e("MUL12", d, a, b)
        return d
    def sqr(self, a):
        d = self.take()
        self.e("SQR12", d, a)
        return d
    def frob(self, a, times=1):
        d = self.take()
        self.e("FROB12", d, a)
        for _ in range(times - 1):
            self.e("FROB12", d, d)
        return d
    def conj(self, a):
        d = self.take()
        self.e("CONJ12", d, a)
        return d
    def mul_into(self, a, b):
        """a b, giving a back"""
        d = self.mul(a, b)
        self.give(a)
        return d
    def pow(self, a, e):
        """a^|e|, conjugated for e < 0 (the inverse, in the cyclotomic subgroup)"""
        r = None
        for bit in bin(abs(e))[3:]:
            s = self.sqr(a if r is None else r)
            if r is not None:
                self.give(r)
            r = s
            if bit == "1":
                r = self.mul_into(r, a)
        if e < 0:
            self.e("CONJ12", r, r)
        return r


def dbl_step(p):
    t = p.t
    p.e("SQR2", t(0), TY); p.e("SQR2", t(1), TZ); p.e("SQR2", t(2), TX)            # B, C, D
    p.e("ADD2", t(3), t(1), t(1)); p.e("ADD2", t(3), t(3), t(1))
    p.e("LDC", t(4), C_BT); p.e("MUL2", t(3), t(4), t(3))                            # E = 3 b' Z^2
    p.e("ADD2", t(5), t(3), t(3)); p.e("ADD2", t(5), t(5), t(3))                     # F = 3 E
    p.e("ADD2", t(6), TY, TY); p.e("MUL2", t(6), t(6), TZ)                           # H = 2 Y Z
    p.e("MUL2", t(7), TX, TY); p.e("ADD2", t(7), t(7), t(7))                         # 2 X Y
    p.e("SUB2", t(8), t(0), t(5)); p.e("MUL2", TX, t(7), t(8))                       # X3 = 2 X Y (B - F)
    p.e("ADD2", t(8), t(0), t(5)); p.e("SQR2", t(8), t(8))                           # (B + F)^2
    p.e("SQR2", t(9), t(3)); p.e("ADD2", t(10), t(9), t(9)); p.e("ADD2", t(10), t(10), t(9))
    p.e("ADD2", t(10), t(10), t(10)); p.e("ADD2", t(10), t(10), t(10))               # 12 E^2
    p.e("SUB2", TY, t(8), t(10))                                                     # Y3
    p.e("MUL2", t(8), t(0), t(6)); p.e("ADD2", t(8), t(8), t(8)); p.e("ADD2", TZ, t(8), t(8))   # Z3 = 4 B H
    p.e("ADD2", t(8), t(2), t(2)); p.e("ADD2", t(8), t(8), t(2)); p.e("MUL2", t(8), t(8), XP)
    p.e("NEG2", L1, t(8))                                                            # -3 X^2 xP
    p.e("MUL2", L0, t(6), YP)                                                        # 2 Y Z yP
    p.e("SUB2", L2, t(0), t(3))                                                      # Y^2 - 3 b' Z^2


def add_step(p, qx, qy):
    t = p.t
    p.e("MUL2", t(0), qy, TZ); p.e("SUB2", t(0), TY, t(0))                           # theta
    p.e("MUL2", t(1), qx, TZ); p.e("SUB2", t(1), TX, t(1))                           # lambda
    p.e("SQR2", t(2), t(0)); p.e("SQR2", t(3), t(1)); p.e("MUL2", t(4), t(3), t(1))  # C, D, E
    p.e("MUL2", t(5), TZ, t(2)); p.e("MUL2", t(6), TX, t(3))                         # F, G
    p.e("ADD2", t(7), t(4), t(5)); p.e("ADD2", t(8), t(6), t(6)); p.e("SUB2", t(7), t(7), t(8))  # H
    p.e("MUL2", TX, t(1), t(7))
    p.e("SUB2", t(8), t(6), t(7)); p.e("MUL2", t(8), t(0), t(8)); p.e("MUL2", t(9), TY, t(4))
    p.e("SUB2", TY, t(8), t(9))
    p.e("MUL2", TZ, TZ, t(4))
    p.e("MUL2", L0, t(1), YP)
    p.e("MUL2", t(8), t(0), XP); p.e("NEG2", L1, t(8))
    p.e("MUL2", t(8), t(0), qx); p.e("MUL2", t(9), t(1), qy); p.e("SUB2", L2, t(8), t(9))


def miller(curve):
    p = Prog()
    x = X[curve]
    loop = 6 * x + 2 if curve == "bn128" else -x
    p.e("COPY2", TX, QX); p.e("COPY2", TY, QY); p.e("LDC", TZ, C_ONE)
    cur, oth = F, 6
    p.e("ONE12", cur)
    def line():
        nonlocal cur, oth
        p.e("SPMUL12", oth, cur, L0)
        cur, oth = oth, cur
    for bit in bin(loop)[3:]:
        p.e("SQR12", oth, cur)
        cur, oth = oth, cur
        dbl_step(p)
        line()
        if bit == "1":
            add_step(p, QX, QY)
            line()
    if curve == "bn128":
        for sx, sy, dx, dy in ((QX, QY, Q1X, Q1Y), (Q1X, Q1Y, Q2X, Q2Y)):
            p.e("CONJ2", dx, sx); p.e("LDC", p.t(0), C_GAMMA + 2); p.e("MUL2", dx, dx, p.t(0))
            p.e("CONJ2", dy, sy); p.e("LDC", p.t(0), C_GAMMA + 3); p.e("MUL2", dy, dy, p.t(0))
        p.e("NEG2", Q2Y, Q2Y)
        add_step(p, Q1X, Q1Y)
        line()
        add_step(p, Q2X, Q2Y)
        line()
    if cur != F:
        p.e("COPY12", F, cur)
    return p.ins


def fexp(curve):
    p = Prog()
    p.free = [6 * s for s in range(NSLOT - 1, 0, -1)]
    x = X[curve]
    P, r = PR[curve]
    hard = (P ** 4 - P ** 2 + 1) // r
    # ---- easy part: g = conj(F) / F, then g^(p^2) g
    c = p.conj(F)
    n = p.mul(F, c)                      # in Fp6
    n2 = p.frob(n, 2)
    n4 = p.frob(n2, 2)
    m = p.mul_into(n2, n4)
    p.give(n4)
    N = p.mul_into(n, m)                 # in Fp2: cell N + 0
    p.e("INV2", p.t(0), N)
    p.give(N)
    inv = p.mul(c, m)
    p.give(m)
    for k in range(6):
        p.e("MUL2", inv + k, inv + k, p.t(0))
    g = p.mul_into(c, inv)
    p.give(inv)
    g2 = p.frob(g, 2)
    p.e("MUL12", F, g2, g)
    p.give(g, g2)
    # ---- hard part (F is in the cyclotomic subgroup: the inverse is the conjugate)
    if curve == "bls12_381":
        assert (x - 1) % 3 == 0 and hard == (x - 1) ** 2 // 3 * (x + P) * (x * x + P * P - 1) + 1
        a = p.pow(F, (x - 1) // 3)
        t = p.pow(a, x - 1); p.give(a); a = t
        b = p.pow(a, x)
        t = p.frob(a); p.give(a)
        b = p.mul_into(b, t); p.give(t)
        c1 = p.pow(b, x)
        c2 = p.pow(c1, x); p.give(c1)
        t = p.frob(b, 2)
        c2 = p.mul_into(c2, t); p.give(t)
        p.e("CONJ12", b, b)
        c2 = p.mul_into(c2, b); p.give(b)
        t = p.mul(c2, F); p.give(c2)
        p.e("COPY12", F, t)
        p.give(t)
    else:
        l2 = 6 * x * x + 1
        l1 = -36 * x ** 3 - 18 * x * x - 12 * x + 1
        l0 = -36 * x ** 3 - 30 * x * x - 18 * x - 2
        assert hard == l0 + l1 * P + l2 * P ** 2 + P ** 3
        fx = p.pow(F, x)
        fx2 = p.pow(fx, x)
        fx3 = p.pow(fx2, x)
        # result = y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36 (every exponent of l0 .. l2 above, term by term)
        y6 = p.frob(fx3); y6 = p.mul_into(y6, fx3); p.give(fx3); p.e("CONJ12", y6, y6)
        y4 = p.frob(fx2); y4 = p.mul_into(y4, fx); p.e("CONJ12", y4, y4)
        t0 = p.sqr(y6); p.give(y6)
        t0 = p.mul_into(t0, y4); p.give(y4)
        y5 = p.conj(fx2)
        t0 = p.mul_into(t0, y5)
        y3 = p.frob(fx); p.give(fx); p.e("CONJ12", y3, y3)
        t1 = p.mul_into(y3, y5); p.give(y5)
        t1 = p.mul_into(t1, t0)
        y2 = p.frob(fx2, 2); p.give(fx2)
        t0 = p.mul_into(t0, y2); p.give(y2)
        t = p.sqr(t1); p.give(t1); t1 = t
        t1 = p.mul_into(t1, t0); p.give(t0)
        t = p.sqr(t1); p.give(t1); t1 = t
        y1 = p.conj(F)
        t0 = p.mul(t1, y1); p.give(y1)
        y0 = p.frob(F)
        s = p.frob(y0)
        u = p.mul(y0, s); p.give(y0)
        p.e("FROB12", s, s)
        y0 = p.mul_into(u, s); p.give(s)
        t1 = p.mul_into(t1, y0); p.give(y0)
        t = p.sqr(t0); p.give(t0); t0 = t
        p.e("MUL12", F, t0, t1)
        p.give(t0, t1)
    assert sorted(p.free) == [6 * s for s in range(1, NSLOT)], p.free
    return p.ins


def programs():
    return {(c, k): fn(c) for c in ("bn128", "bls12_381") for k, fn in (("miller", miller), ("fexp", fexp))}


def render():
    out = ["// GENERATED by tools/gen_pairing_prog.py -- do not edit by hand.",
           "// Instruction streams of the pairing interpreter (zk_pairing_impl.hpp): op | d << 8 | a << 16 | b << 24.",
           f"#define ZK_PAIR_NSLOT {NSLOT}", f"#define ZK_PAIR_NCELL {NCELL}"]
    for i, n in enumerate(OPS):
        out.append(f"#define ZK_PAIR_OP_{n} {i}")
    for n, v in (("XP", XP), ("YP", YP), ("QX", QX), ("QY", QY)):
        out.append(f"#define ZK_PAIR_CELL_{n} {v}")
    for (c, k), ins in programs().items():
        out.append(f"// {c} {k}: {len(ins)} instructions")
        out.append(f"static const uint32_t ZK_PAIR_PROG_{c.upper()}_{k.upper()}[] = {{")
        for i in range(0, len(ins), 10):
            out.append("  " + ", ".join("0x%08xu" % w for w in ins[i:i + 10]) + ",")
        out.append("};")
    return "\n".join(out) + "\n"


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    dst = os.path.join(here, "..", "zikkurat-algebra_amd", "csrc", "zk_pairing_prog.inc")
    with open(dst, "w") as f:
        f.write(render())
    print("wrote", os.path.normpath(dst))


if __name__ == "__main__":
    main()
