"""The device-resident entry points of the Fr layer, of division by a vanishing polynomial and of the G1
batch conversion -- zkg_arr_op_device (all 17 op codes), zkg_arr_dot_device, zkg_arr_powers_device,
zkg_poly_div_by_vanishing_device, zkg_g1_batch_to_affine_device, zkg_g1_jac_batch_to_affine_device --
on buffers the caller owns.

The host ABI copies every operand into a buffer of its own and copies exactly n rows back, so it cannot
see a kernel that writes past row n - 1 or into an input, and never runs a kernel in place.  Here every
operand is a guarded window (tests/device_windows.py): after each call the target equals the oracle's
value on host copies of the inputs taken before the call, every input that is not the target is
unchanged, and every guard row of every buffer still holds its sentinel.  Every comparison is
np.array_equal against a value computed without the GPU.

Aliasing: any operand may be exactly the target, and the result is the one of distinct buffers.  The
reference's loops are element-wise (row i of the result depends on row i of the inputs:
<C>_arr_mont.c), so its own C gives the same bytes when aliased the same way -- with three exceptions,
where its loop body writes the product into the target BEFORE it reads the addend (arr_mont.c:124-137,
204-209): mul_add and mul_sub with the target on c, Ax_plus_y with the target on b.  Aliased like
that the reference computes 2 a b, 0 and 2 kA a; the library computes a b + c, a b - c and kA a + b.
test_elementwise pins both facts where oracle/_ref is built.
"""
import functools

import numpy as np
import pytest

import device_windows as dw
import field_edges as fe

pytestmark = pytest.mark.gpu
CURVES = ["bn128", "bls12_381"]

# the wave (64) and workgroup (256) edges of the staged runs
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
REF_N = 65  # the size at which the reference's own C is called on arrays aliased the same way

OPERANDS = {"neg": "a", "sqr": "a", "scale": "a", "from_std": "a", "to_std": "a", "copy": "a", "set_const": "",
            "add": "ab", "sub": "ab", "sub_rev": "ab", "mul": "ab", "Ax_plus_y": "ab", "Ax_plus_By": "ab",
            "mul_add": "abc", "mul_sub": "abc"}
LAYOUTS = {"": ("distinct",), "a": ("distinct", "tgt_is_a"),  # one operand: "every operand the same" is tgt_is_a
           "ab": ("distinct", "tgt_is_a", "tgt_is_b", "a_is_b", "all_same"),
           "abc": ("distinct", "tgt_is_a", "tgt_is_b", "tgt_is_c", "a_is_b", "all_same")}
ELEMENTWISE = [(op, lay) for op, names in OPERANDS.items() for lay in LAYOUTS[names]]
# the reference writes its product into the target before it reads the addend (module docstring)
REF_ADDEND_LOST = {("mul_add", "tgt_is_c"), ("mul_add", "all_same"), ("mul_sub", "tgt_is_c"), ("mul_sub", "all_same"),
                   ("Ax_plus_y", "tgt_is_b"), ("Ax_plus_y", "all_same")}


def _ref_or_none(request):
    from oracle.oracle import Reference
    return request.getfixturevalue("reference") if Reference.available() else None


def _frozen(a):
    a.flags.writeable = False
    return a


def _minus_one(curve):
    return fe.to_row(fe.FR[curve] - 1, 4)


@functools.lru_cache(maxsize=None)
def _input(gpu, curve, n, k):
    """operand k (0: a, 1: b, 2: c) of n gen_fr rows with one row 0 and one row r - 1 (the Montgomery form
    of -1), at rows that differ between the operands; read-only, shared by every test of this size"""
    x = gpu.gen_fr(curve, 0xD1 + k + 16 * n, n)
    x[(n // 2 + k) % n] = 0
    x[(n - 1 - k) % n] = _minus_one(curve)
    return _frozen(x)


def _inputs(gpu, curve, n, names="abc"):
    return tuple(_input(gpu, curve, n, k) if nm in names else None for k, nm in enumerate("abc"))


@functools.lru_cache(maxsize=None)
def _consts(gpu, curve):
    k = gpu.gen_fr(curve, 0xD4, 2)
    return _frozen(k[0].copy()), _frozen(k[1].copy())


def _alias(layout, a, b, c, make_tgt):
    """operands (a, b, c, tgt) of a layout; aliased operands are the SAME object"""
    if layout in ("a_is_b", "all_same"):
        b = a if b is not None else None
    if layout == "all_same":
        c = a if c is not None else None
    tgt = {"tgt_is_a": a, "tgt_is_b": b, "tgt_is_c": c, "all_same": a}.get(layout)
    return a, b, c, (tgt if tgt is not None else make_tgt())


def _reference_call(ref, curve, op, n, a, b, c, kA, kB, t):
    R = lambda name, *args: ref.arr(curve, "arr_mont_" + name, n, *args)
    if op in ("neg", "sqr", "from_std", "to_std", "copy"):
        R(op, a, t)
    elif op == "set_const":
        R(op, kA, t)
    elif op == "scale":
        R(op, kA, a, t)
    elif op in ("add", "sub", "mul"):
        R(op, a, b, t)
    elif op == "sub_rev":
        R("sub", b, a, t)
    elif op == "Ax_plus_y":
        R(op, kA, a, b, t)
    elif op == "Ax_plus_By":
        R(op, kA, kB, a, b, t)
    else:
        R(op, a, b, c, t)


def _run_elementwise(gpu, oracle, curve, op, layout, n, k, ref=None):
    names = OPERANDS[op]
    kA, kB = _consts(gpu, curve)
    ha, hb, hc, _ = _alias(layout, *_inputs(gpu, curve, n, names), lambda: None)
    want = oracle.arr_op(curve, op, n, ha, hb, hc, kA=kA, kB=kB)
    what = f"{op} {layout} n={n}"
    with dw.pool(gpu, k) as P:
        wa = None if ha is None else P.new(ha)
        wb = None if hb is None else (wa if hb is ha else P.new(hb))
        wc = None if hc is None else (wa if hc is ha else P.new(hc))
        tgt = {"tgt_is_a": wa, "tgt_is_b": wb, "tgt_is_c": wc, "all_same": wa}.get(layout) or P.new(n)
        gpu.arr_op_device(curve, op, n, wa, wb, wc, kA, kB, tgt)
        got = tgt.read()
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert not len(bad), (what, "rows", bad[:8].tolist())
        for nm, w, h in (("a", wa, ha), ("b", wb, hb), ("c", wc, hc)):
            if w is not None and w is not tgt:
                assert np.array_equal(w.read(), h), (what, "input changed", nm)
        P.check(what)
    if ref is not None:
        ra, rb, rc = [x.copy() if x is not None else None for x in (ha, hb, hc)]
        ra, rb, rc, rt = _alias(layout, ra, rb, rc, lambda: np.zeros((n, 4), dtype=np.uint64))
        _reference_call(ref, curve, op, n, ra, rb, rc, kA, kB, rt)
        if (op, layout) in REF_ADDEND_LOST:
            prod = oracle.arr_op(curve, "scale", n, ha, kA=kA) if op == "Ax_plus_y" else oracle.arr_op(curve, "mul", n, ha, hb)
            lost = np.zeros_like(prod) if op == "mul_sub" else oracle.arr_op(curve, "add", n, prod, prod)
            assert np.array_equal(rt, lost) and not np.array_equal(rt, want), (what, "reference")
        else:
            assert np.array_equal(rt, got), (what, "reference aliased the same way")


# ---------------------------------------------------------------------------- (a) element-wise ops
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("op,layout", ELEMENTWISE)
def test_elementwise(gpu, oracle, request, curve, op, layout):
    """all 15 element-wise op codes of zkg_arr_op_device at the wave and workgroup edges, with every
    pointer layout the op has: all buffers distinct, the target on a, on b, on c, a on b with a target
    of its own, and every operand the same window.  The windows of one call sit at different offsets
    (0, 1, 3 rows) from their guards, cycling over the cases; a call with four windows repeats one."""
    ref = _ref_or_none(request)
    k0 = ELEMENTWISE.index((op, layout))
    for i, n in enumerate(SIZES):
        _run_elementwise(gpu, oracle, curve, op, layout, n, k0 + i, ref if n == REF_N else None)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("op", ["scale", "sqr", "Ax_plus_By"])
def test_elementwise_in_place_past_the_grid_cap(gpu, oracle, curve, op):
    """n = 8192 * 256 + 321: the ops with a product per element run at most 8192 workgroups, so every
    workgroup takes a second trip of the stage-2 grid-stride loop on the first 321 rows past the cap --
    in place (the target on a), where a store of the first trip must not reach the rows of the second"""
    _run_elementwise(gpu, oracle, curve, op, "tgt_is_a", 8192 * 256 + 321, 1)


# ---------------------------------------------------------------------------- (b) batch inversion
INV_N = (1, 7, 8, 9, 63, 64, 65, 1000, 4099)  # CHK = 8: lanes = ceil(n / 8) own rows t, t + lanes, ...
INV_CASES = [("inv", "distinct"), ("inv", "tgt_is_a"), ("div", "distinct"), ("div", "tgt_is_a"), ("div", "tgt_is_b"),
             ("div", "all_same")]


@functools.lru_cache(maxsize=None)
def _inv_inputs(gpu, curve, n):
    """(numerator, invertible rows): the numerator with a 0 and an r - 1 row, the other with r - 1 alone"""
    a = _input(gpu, curve, n, 0)
    x = gpu.gen_fr(curve, 0xD5 + 16 * n, n)
    x[(n - 1) // 2] = _minus_one(curve)
    assert x.any(axis=1).all()
    return a, _frozen(x)


def _zero_rows(n):
    """first row, last row, the first row of the ragged last chunk of 8 consecutive rows, and the last row
    of the last lane of the strided chunks (a lane one row short when 8 does not divide n)"""
    lanes = -(-n // 8)
    return sorted({0, n - 1, 8 * ((n - 1) // 8), max(range(lanes - 1, n, lanes))})


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("op,layout", INV_CASES)
def test_batch_inversion(gpu, oracle, curve, op, layout):
    """inv (distinct, in place) and div (distinct, the target on a, on b, a = b = the target) at lane
    counts and chunk lengths around k_inv_chunks2's pairs: every row against the oracle; then one zero in
    the inverted operand, which zeroes EVERY row of the target (Fr_mont.c:258-285) and nothing else"""
    one = fe.to_row(fe.radix(fe.FR[curve]) % fe.FR[curve], 4)
    k = INV_CASES.index((op, layout))
    for n in INV_N:
        num, x0 = _inv_inputs(gpu, curve, n)
        for z in [None] + _zero_rows(n):
            x = x0
            if z is not None:
                x = x0.copy()
                x[z] = 0
            # inv inverts a; div divides a by b
            ha, hb = (x, None) if op == "inv" else ((x, x) if layout == "all_same" else (num, x))
            want = oracle.arr_op(curve, op, n, ha, hb)
            if z is not None:
                assert not want.any()
            elif layout == "all_same":
                assert (want == one).all()
            what = f"{op} {layout} n={n} zero={z}"
            k += 1
            with dw.pool(gpu, k) as P:
                wa = P.new(ha)
                wb = None if hb is None else (wa if hb is ha else P.new(hb))
                tgt = {"tgt_is_a": wa, "tgt_is_b": wb, "all_same": wa}.get(layout) or P.new(n)
                gpu.arr_op_device(curve, op, n, wa, wb, d_tgt=tgt)
                got = tgt.read()
                bad = np.nonzero((got != want).any(axis=1))[0]
                assert not len(bad), (what, "rows", bad[:8].tolist())
                for nm, w, h in (("a", wa, ha), ("b", wb, hb)):
                    if w is not None and w is not tgt:
                        assert np.array_equal(w.read(), h), (what, "input changed", nm)
                P.check(what)


# ---------------------------------------------------------------------------- (c) dot product
DOT_N = (1, 255, 256, 257, 65537, 262144 + 257)  # k_dot runs at most 1024 blocks: the last size enters its stride loop


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", DOT_N)
def test_dot(gpu, oracle, curve, n):
    """zkg_arr_dot_device on distinct operands and on a = b; the inputs stay as they were"""
    a, b, _ = _inputs(gpu, curve, n, "ab")
    want = oracle.arr_dot(curve, a, b)
    want_sq = oracle.arr_dot(curve, a, a)
    with dw.pool(gpu, DOT_N.index(n)) as P:
        wa, wb = P.new(a), P.new(b)
        assert np.array_equal(gpu.arr_dot_device(curve, n, wa, wb), want), "distinct"
        assert np.array_equal(gpu.arr_dot_device(curve, n, wa, wa), want_sq), "a is b"
        assert np.array_equal(wa.read(), a) and np.array_equal(wb.read(), b)
        P.check(f"dot n={n}")
    if n == DOT_N[-1]:  # the host symbol through the same loop
        assert np.array_equal(gpu.arr_dot_prod(curve, a, b), want)


# ---------------------------------------------------------------------------- (d) powers
POWERS_N = (1, 2, 63, 64, 65, 1000, 4097)  # 4097: 128 low powers, a ragged high table of 33


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("n", (0,) + POWERS_N)
def test_powers(gpu, oracle, curve, n):
    """zkg_arr_powers_device into a guarded window: the (kA, kB) pairs of field_edges.powers_cases (bases
    0, 1, r - 1 and an element of order 32) and one random pair; n = 0 writes nothing"""
    pairs = [(fe.to_row(ka, 4), fe.to_row(kb, 4)) for ka, kb in fe.powers_cases(curve)] + [_consts(gpu, curve)]
    for i, (ka, kb) in enumerate(pairs):
        with dw.pool(gpu, i) as P:
            tgt = P.new(n if n else 8)
            gpu.arr_powers_device(curve, n, ka, kb, tgt)
            if n:
                assert np.array_equal(tgt.read(), oracle.arr_powers(curve, ka, kb, n)), (i, n)
            else:
                assert tgt.untouched()
            P.check(f"powers pair {i} n={n}")


# ---------------------------------------------------------------------------- (e) division by a vanishing polynomial
# (n1, n, zero rows at the top); "exact": (x^100 - eta) g with 300 coefficients of g
VANISH = [(40, 8, 2), (33, 16, 2), (7, 8, 2), (64, 1, 2), (100, 32, 2), (0, 4, 0), (130, 100, 3), (5000, 37, 0),
          (9000, 64, 4097), "exact"]
VANISH_REF = (100, 32, 2)  # the oversized call of this row is compared with the reference's own C


def _vanish_input(gpu, oracle, curve, case):
    eta = gpu.gen_fr(curve, 0xE1, 1)[0]
    if case == "exact":
        n, m = 100, 300
        g = gpu.gen_fr(curve, 0xE2, m)
        p = np.zeros((n + m, 4), dtype=np.uint64)
        p[n:] = g  # p = x^n g - eta g
        p[:m] = oracle.arr_op(curve, "sub", m, np.ascontiguousarray(p[:m]), oracle.arr_op(curve, "scale", m, g, kA=eta))
        return p, n, eta, g
    n1, n, zero_top = case
    p = gpu.gen_fr(curve, 0xE3 + n1, max(n1, 1))[:n1]
    if zero_top:
        p[-zero_top:] = 0
    return p, n, eta, None


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("case", VANISH, ids=str)
def test_div_by_vanishing(gpu, oracle, request, curve, case):
    """zkg_poly_div_by_vanishing_device with source, quotient and remainder in guarded windows, three ways:
    the smallest legal buffers (deg - n + 1 quotient rows, n remainder rows); five rows more of each,
    which come back zero; and d_rem = NULL, where the return value is the verdict "remainder zero"."""
    ref = _ref_or_none(request)
    p, n, eta, g = _vanish_input(gpu, oracle, curve, case)
    n1 = p.shape[0]
    nz = np.nonzero(p.any(axis=1))[0]
    deg = int(nz[-1]) if len(nz) else -1
    nq0, nr0 = max(0, deg - n + 1), n
    for way, (nq, nr, with_rem) in enumerate(((nq0, nr0, True), (nq0 + 5, nr0 + 5, True), (nq0, 0, False))):
        wq, wr, ok = oracle.div_by_vanishing(curve, p, n, eta, nquot=nq, nrem=nr if with_rem else n)
        if g is not None:
            assert ok and np.array_equal(wq[:g.shape[0]], g)
        if way == 1:
            assert not wq[nq0:].any() and not wr[nr0:].any()
            if case == VANISH_REF and ref is not None:
                rq, rr = np.ones((nq, 4), dtype=np.uint64), np.ones((nr, 4), dtype=np.uint64)
                ref.arr(curve, "poly_mont_div_by_vanishing", n1, p, n, eta, nq, rq, nr, rr)
                assert np.array_equal(rq, wq) and np.array_equal(rr, wr)  # zeroing the tail is the reference's behaviour
        what = f"vanishing {case} way {way}"
        with dw.pool(gpu, way) as P:
            src, quot = P.new(p), P.new(nq)
            rem = P.new(nr) if with_rem else None
            rc = gpu.div_by_vanishing_device(curve, n1, src, n, eta, nq, quot, nr, rem)
            assert np.array_equal(quot.read(), wq), what
            if with_rem:
                assert np.array_equal(rem.read(), wr), what
            else:
                assert rc in (0, 1) and bool(rc) == ok, what
            assert np.array_equal(src.read(), p), (what, "source changed")
            P.check(what)


# ---------------------------------------------------------------------------- (f) G1 batch conversion
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("coords", ["proj", "jac"])
@pytest.mark.parametrize("n", [1, 2, 3, 31, 33, 1000])
def test_g1_batch_to_affine(gpu, oracle, curve, coords, n):
    """zkg_g1_batch_to_affine_device / zkg_g1_jac_batch_to_affine_device: rows of 3 NP words in, rows of
    2 NP words out, in distinct guarded windows; the points of test_gpu_field_edges.test_infinity_layouts
    with infinity in the first row, in the last row, and nowhere"""
    nl, M = gpu.NLIMBS_P[curve], fe.fp_model(curve)
    base = fe._coord_points(gpu, oracle, curve, coords, n, 900 + n)
    lam = fe.from_limbs(gpu.gen_points(curve, 902 + n, n)[:, :nl])
    for k, inf in enumerate((0, n - 1, None)):
        pts = base.copy()
        if inf is not None:
            pts[inf] = fe.point_rows([fe.infinity(M, lam[inf], coords)], nl)[0]
        want = fe.affine_rows(M, fe.point_ints(pts, nl), coords)
        assert np.array_equal((want == fe.ALL_ONES).all(axis=1), np.arange(n) == (-1 if inf is None else inf))
        assert np.array_equal(gpu.batch_to_affine(curve, pts, coords=coords), want)  # the host entry
        what = f"{coords} n={n} infinity at {inf}"
        with dw.pool(gpu, k) as P:
            src, tgt = P.new(pts, width=3 * nl), P.new(n, width=2 * nl)
            gpu.batch_to_affine_device(curve, n, src, tgt, coords=coords)
            got = tgt.read()
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert not len(bad), (what, "rows", bad[:8].tolist())
            assert np.array_equal(src.read(), pts), (what, "source changed")
            P.check(what)
