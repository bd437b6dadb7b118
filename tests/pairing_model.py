"""Plain big-integer model of the optimal-ate pairings of BN254 ("bn128") and BLS12-381, written from the
mathematics, for the pairing tests only.

Tower (the reference's irreducibles): Fp2 = Fp[u]/(u^2 + 1), Fp6 = Fp2[v]/(v^3 - xi), Fp12 = Fp6[w]/(w^2 - v),
xi = 9 + u (BN254) or 1 + u (BLS12-381).  An Fp12 element is kept here as the six Fp2 coefficients of
1, w, .., w^5 (w^6 = xi); the word layout of a row is 2 x 3 x 2 Fp in Montgomery form, the coefficient of
w^i v^j = w^(i + 2 j) at Fp2 index 3 i + j.

pairing(curve, P, Q) = f^((p^12 - 1)/r), f the Miller function of the loop
  BN254:      6 x + 2 without its top bit, then the line steps with pi(Q) and -pi^2(Q)   (D-type twist)
  BLS12-381:  |x|, no conjugation for the negative sign                                  (M-type twist)
with the lines scaled by factors of proper subfields, which the exponent kills.
"""

CURVES = {
    "bn128": dict(
        p=0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47,
        r=0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001,
        xi=(9, 1), b=3, dtype=True, x=4965661367192848881, loop=6 * 4965661367192848881 + 2, NP=4),
    "bls12_381": dict(
        p=0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB,
        r=0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
        xi=(1, 1), b=4, dtype=False, x=-0xD201000000010000, loop=0xD201000000010000, NP=6),
}


class Tower:
    def __init__(self, curve):
        c = CURVES[curve]
        self.curve, self.p, self.r, self.xi, self.NP = curve, c["p"], c["r"], c["xi"], c["NP"]
        self.dtype, self.x, self.loop = c["dtype"], c["x"], c["loop"]
        p = self.p
        assert (p ** 4 - p ** 2 + 1) % self.r == 0
        self.R = 1 << (64 * self.NP)
        # twist coefficient b' = b / xi (D-type) or b xi (M-type)
        self.bt = self.f2mul((c["b"], 0), self.f2inv(self.xi)) if self.dtype else self.f2mul((c["b"], 0), self.xi)
        # gamma[k] = xi^(k (p - 1) / 6) = w^(k (p - 1))
        g1 = self.f2pow(self.xi, (p - 1) // 6)
        self.gamma = [(1, 0)]
        for _ in range(5):
            self.gamma.append(self.f2mul(self.gamma[-1], g1))

    # ---- Fp2
    def f2add(self, a, b): return ((a[0] + b[0]) % self.p, (a[1] + b[1]) % self.p)
    def f2sub(self, a, b): return ((a[0] - b[0]) % self.p, (a[1] - b[1]) % self.p)
    def f2neg(self, a): return (-a[0] % self.p, -a[1] % self.p)
    def f2conj(self, a): return (a[0], -a[1] % self.p)
    def f2mul(self, a, b):
        return ((a[0] * b[0] - a[1] * b[1]) % self.p, (a[0] * b[1] + a[1] * b[0]) % self.p)
    def f2inv(self, a):
        n = pow(a[0] * a[0] + a[1] * a[1], -1, self.p)
        return (a[0] * n % self.p, -a[1] * n % self.p)
    def f2pow(self, a, e):
        r = (1, 0)
        while e:
            if e & 1:
                r = self.f2mul(r, a)
            a = self.f2mul(a, a)
            e >>= 1
        return r

    # ---- Fp12 as six Fp2 coefficients of w^k
    def one(self): return [(1, 0)] + [(0, 0)] * 5
    def mul(self, a, b):
        lo = [(0, 0)] * 11
        for i in range(6):
            if a[i] == (0, 0):
                continue
            for j in range(6):
                lo[i + j] = self.f2add(lo[i + j], self.f2mul(a[i], b[j]))
        return [self.f2add(lo[k], self.f2mul(self.xi, lo[k + 6])) if k < 5 else lo[k] for k in range(6)]
    def sqr(self, a): return self.mul(a, a)
    def conj(self, a): return [a[k] if k % 2 == 0 else self.f2neg(a[k]) for k in range(6)]
    def frob(self, a): return [self.f2mul(self.f2conj(a[k]), self.gamma[k]) for k in range(6)]
    def inv(self, a):
        c = self.conj(a)
        n = self.mul(a, c)                    # in Fp6: odd coefficients vanish
        n2 = self.frob(self.frob(n))
        m = self.mul(n2, self.frob(self.frob(n2)))   # n^(p^2) n^(p^4)
        N = self.mul(n, m)                    # in Fp2
        assert all(N[k] == (0, 0) for k in range(1, 6))
        s = self.f2inv(N[0])
        return [self.f2mul(t, s) for t in self.mul(c, m)]
    def pow(self, a, e):
        r = self.one()
        for bit in bin(e)[2:]:
            r = self.sqr(r)
            if bit == "1":
                r = self.mul(r, a)
        return r
    def final_expo(self, f):
        return self.pow(f, (self.p ** 12 - 1) // self.r)

    # ---- rows of u64 words (Montgomery form, the reference's layout)
    def fp_from_words(self, w):
        v = sum(int(x) << (64 * i) for i, x in enumerate(w))
        return v * pow(self.R, -1, self.p) % self.p
    def fp_to_words(self, v):
        v = v * self.R % self.p
        return [(v >> (64 * i)) & (2 ** 64 - 1) for i in range(self.NP)]
    def f2_from_words(self, w):
        return (self.fp_from_words(w[:self.NP]), self.fp_from_words(w[self.NP:2 * self.NP]))
    def f2_to_words(self, a): return self.fp_to_words(a[0]) + self.fp_to_words(a[1])
    def from_words(self, row):
        NP = self.NP
        out = [None] * 6
        for i in range(2):
            for j in range(3):
                o = (3 * i + j) * 2 * NP
                out[i + 2 * j] = self.f2_from_words(row[o:o + 2 * NP])
        return out
    def to_words(self, a):
        out = []
        for i in range(2):
            for j in range(3):
                out += self.f2_to_words(a[i + 2 * j])
        return out
    def is_inf_row(self, row): return all(int(x) == 2 ** 64 - 1 for x in row)
    def g1_from_words(self, row):
        return None if self.is_inf_row(row) else (self.fp_from_words(row[:self.NP]), self.fp_from_words(row[self.NP:]))
    def g2_from_words(self, row):
        NP = self.NP
        return None if self.is_inf_row(row) else (self.f2_from_words(row[:2 * NP]), self.f2_from_words(row[2 * NP:]))

    # ---- Miller loop: T projective (X : Y : Z) on the twist y^2 = x^3 + b'
    def line(self, cy, cx, cc):
        """the sparse line with the yP term cy, the xP term cx and the constant term cc"""
        z = (0, 0)
        return [cy, cx, z, cc, z, z] if self.dtype else [cc, z, cx, cy, z, z]
    def dbl_step(self, T, P):
        X, Y, Z = T
        m, s, a = self.f2mul, self.f2sub, self.f2add
        B, C, D = m(Y, Y), m(Z, Z), m(X, X)
        E = m(self.bt, a(a(C, C), C))          # 3 b' Z^2
        F = a(a(E, E), E)
        H = m(a(Y, Y), Z)                      # 2 Y Z
        XY = m(X, Y)
        X3 = m(a(XY, XY), s(B, F))
        BF = a(B, F)
        E2 = m(E, E)
        E12 = a(a(E2, E2), E2)
        E12 = a(a(E12, E12), a(E12, E12))
        Y3 = s(m(BF, BF), E12)
        BH = m(B, H)
        Z3 = a(a(BH, BH), a(BH, BH))
        D3 = a(a(D, D), D)
        ln = self.line(m(H, (P[1], 0)), self.f2neg(m(D3, (P[0], 0))), s(B, E))
        return (X3, Y3, Z3), ln
    def add_step(self, T, Q, P):
        X, Y, Z = T
        m, s, a = self.f2mul, self.f2sub, self.f2add
        th = s(Y, m(Q[1], Z))
        la = s(X, m(Q[0], Z))
        C, D = m(th, th), m(la, la)
        E = m(D, la)
        F, G = m(Z, C), m(X, D)
        H = s(a(E, F), a(G, G))
        X3 = m(la, H)
        Y3 = s(m(th, s(G, H)), m(Y, E))
        Z3 = m(Z, E)
        ln = self.line(m(la, (P[1], 0)), self.f2neg(m(th, (P[0], 0))), s(m(th, Q[0]), m(la, Q[1])))
        return (X3, Y3, Z3), ln
    def miller(self, P, Q):
        f = self.one()
        T = (Q[0], Q[1], (1, 0))
        for bit in bin(self.loop)[3:]:
            f = self.sqr(f)
            T, ln = self.dbl_step(T, P)
            f = self.mul(ln, f)
            if bit == "1":
                T, ln = self.add_step(T, Q, P)
                f = self.mul(ln, f)
        if self.dtype:  # BN254: pi(Q) and -pi^2(Q)
            pi = lambda q: (self.f2mul(self.f2conj(q[0]), self.gamma[2]), self.f2mul(self.f2conj(q[1]), self.gamma[3]))
            Q1 = pi(Q)
            Q2 = pi(Q1)
            Q2 = (Q2[0], self.f2neg(Q2[1]))
            T, ln = self.add_step(T, Q1, P)
            f = self.mul(ln, f)
            T, ln = self.add_step(T, Q2, P)
            f = self.mul(ln, f)
        return f
    def pairing(self, P, Q):
        """P, Q affine points as integers (None: infinity) -> Fp12 coefficients"""
        if P is None or Q is None:
            return self.one()
        return self.final_expo(self.miller(P, Q))
    def pairing_words(self, Prow, Qrow):
        return self.to_words(self.pairing(self.g1_from_words(Prow), self.g2_from_words(Qrow)))


_towers = {}


def tower(curve):
    if curve not in _towers:
        _towers[curve] = Tower(curve)
    return _towers[curve]


# ---- the big-integer interpreter of the pairing kernels' instruction streams (tools/gen_pairing_prog.py)

def run_program(T, ins, cells, ops, consts):
    """run the (op | d << 8 | a << 16 | b << 24) words `ins` on the list `cells` of Fp2 values, in place"""
    name = {i: n for i, n in enumerate(ops)}
    for w in ins:
        op, d, a, b = name[w & 255], (w >> 8) & 255, (w >> 16) & 255, (w >> 24) & 255
        if op == "MUL2": cells[d] = T.f2mul(cells[a], cells[b])
        elif op == "SQR2": cells[d] = T.f2mul(cells[a], cells[a])
        elif op == "ADD2": cells[d] = T.f2add(cells[a], cells[b])
        elif op == "SUB2": cells[d] = T.f2sub(cells[a], cells[b])
        elif op == "NEG2": cells[d] = T.f2neg(cells[a])
        elif op == "CONJ2": cells[d] = T.f2conj(cells[a])
        elif op == "COPY2": cells[d] = cells[a]
        elif op == "LDC": cells[d] = consts[a]
        elif op == "INV2": cells[d] = T.f2inv(cells[a])
        elif op == "MUL12":
            assert d != a and d != b
            cells[d:d + 6] = T.mul(cells[a:a + 6], cells[b:b + 6])
        elif op == "SQR12":
            assert d != a
            cells[d:d + 6] = T.sqr(cells[a:a + 6])
        elif op == "SPMUL12":
            assert d != a
            cells[d:d + 6] = T.mul(T.line(cells[b], cells[b + 1], cells[b + 2]), cells[a:a + 6])
        elif op == "FROB12": cells[d:d + 6] = T.frob(cells[a:a + 6])
        elif op == "CONJ12": cells[d:d + 6] = T.conj(cells[a:a + 6])
        elif op == "COPY12": cells[d:d + 6] = cells[a:a + 6]
        elif op == "ONE12": cells[d:d + 6] = T.one()
        else: raise ValueError(op)
    return cells


def program_consts(T):
    return T.gamma + [T.bt, (1, 0)]
