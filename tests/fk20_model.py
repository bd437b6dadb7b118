"""Pure-Python model of the "all openings" derivation (DESIGN.md "All openings (FK20)") with Fr scalars standing
in for the points: s_i = tau^i as an integer mod R, so a commitment is the polynomial's value at tau and a group
FFT is an NTT.  Shared by tests/test_fk20_cpu.py; the index maps come from the caller (zkalgebra's, so that the
model and the kernels' layout share one definition)."""

FR = {
    "bn128": 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001,
    "bls12_381": 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
}


def root_of_unity(R, log_order):
    """an element of multiplicative order exactly 2^log_order mod the prime R"""
    assert (R - 1) % (1 << log_order) == 0
    x = 2
    while True:
        g = pow(x, (R - 1) >> log_order, R)
        if log_order == 0 or pow(g, 1 << (log_order - 1), R) != 1:
            return g
        x += 1


def dft(v, gen, R):
    """out[k] = sum_j v[j] gen^(j k): the NTT, and the group FFT of the stand-in points"""
    n = len(v)
    return [sum(v[j] * pow(gen, j * k, R) for j in range(n)) % R for k in range(n)]


def idft(v, gen, R):
    n = len(v)
    ninv = pow(n, -1, R)
    return [x * ninv % R for x in dft(v, pow(gen, -1, R), R)]


def quotient_at_tau(f, l, eta, tau, R):
    """(quotient of f by x^l - eta)(tau), by the division's own recurrence q_i = f_(i+l) + eta q_(i+l)"""
    n = len(f)
    q = [0] * n
    for i in range(n - l - 1, -1, -1):
        q[i] = (f[i + l] + eta * q[i + l]) % R
    return sum(q[i] * pow(tau, i, R) for i in range(n)) % R


def direct_proofs(f, m, c, g2n, tau, R):
    """pi_k = the quotient of f by x^l - psi^k at tau, k < r (f zero-extended to n = 2^m; g2n of order 2n)"""
    n, l = 1 << m, 1 << c
    f = list(f) + [0] * (n - len(f))
    psi = pow(g2n, 2 * l, R)
    return [quotient_at_tau(f, l, pow(psi, k, R), tau, R) for k in range(n // l)]


def model_proofs(f, m, c, g2n, tau, R, coeff_index, srs_index):
    """the derivation, step by step; also returns y (the inverse transform of size 2r) for the y_(r-1) = O check"""
    n, l = 1 << m, 1 << c
    r = n // l
    f = list(f) + [0] * (n - len(f))
    s = [pow(tau, i, R) for i in range(n)]
    psi, rho = pow(g2n, 2 * l, R), pow(g2n, l, R)  # generators of the r- and the 2r-domain, rho^2 = psi
    u_hat = [0] * (2 * r)
    for j in range(l):
        x = [s[l * srs_index(r, p) + j] if srs_index(r, p) >= 0 else 0 for p in range(2 * r)]
        cj = [f[l * coeff_index(r, p) + j] if coeff_index(r, p) >= 0 else 0 for p in range(2 * r)]
        s_hat, c_hat = dft(x, rho, R), dft(cj, rho, R)  # the table row and the batched NTT's row
        for i in range(2 * r):
            u_hat[i] = (u_hat[i] + c_hat[i] * s_hat[i]) % R  # k_scl_rows_sum
    y = idft(u_hat, rho, R)
    return dft(y[:r], psi, R), y
