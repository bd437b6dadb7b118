"""Every ZK_* environment switch of zikkurat-algebra_amd/csrc, forced in a fresh process and
compared bit for bit with the CPU oracle / the reference's own C.

The library reads each switch once per process (function-local statics), and each one selects
another kernel, template instantiation, chunk length or grid behind an exported entry point.  The
rest of the GPU suite runs the defaults only.  Here one child process per environment setting
(tests/env_switch_child.py) runs every battery that the setting affects, on inputs this module
builds and writes to tmp_path; the child returns the outputs and the observables (g1_fft_plan,
g1_fft_last_glv, msm_last_groups) and this module compares them with
  oracle.arr_op / arr_powers / arr_dot / div_by_vanishing / msm      (Fr ops, G1 MSM)
  reference.arr(...)                                                  (batch affine conversion, group FFT, G2 MSM)
Nothing is compared with a GPU result.  The forced values are the ones the code's own size rules
or the hooks' validation produce: they reach designed paths at small sizes (grid-stride loops,
CHK up to 128, chk up to 32, K = BITACC_MAX_K, radix-8 / radix-16 Stockham stages with remainder
stages), they do not push a kernel outside its design.

test_switch_table_is_complete (no GPU) keeps the table equal to the ZK_* switches that csrc reads.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import field_edges as fe
import generators
import golden_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zikkurat-algebra_amd", "csrc")
CHILD = os.path.join(ROOT, "tests", "env_switch_child.py")
CHILD_TIMEOUT = 100  # seconds, the limit of tests/test_gpu_bench_cli.py
CURVES = ["bn128", "bls12_381"]
FR_FLD = {"bn128": 1, "bls12_381": 3}
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)

# switches left untested because no input that a quick test can check against the CPU oracle
# reaches their path; the reason names the size where the path begins
EXCLUDED = {
    "ZK_SORT_SPLIT": "level 1.5 of the bucket sort starts at c >= 19 (fs >= 10) with an average coarse bin above "
                     "half of level 2's LDS staging (n / 256 > 4096): 2^25 pairs at the default window "
                     "(make_shape); an explicit window >= 19 on one unsplit pass reaches it from 2^20 + 256 "
                     "pairs, where the CPU oracle takes more than half a minute per curve",
}


class Ctx:
    """fixtures of the running test; the reference is asked for only by the batteries that need it"""

    def __init__(self, request):
        self.request = request
        self.gpu = request.getfixturevalue("gpu")
        self.oracle = request.getfixturevalue("oracle")

    @property
    def reference(self):
        return self.request.getfixturevalue("reference")


_REF = {}  # inputs and references, computed once and shared by the settings (never modified)


def cached(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


class Battery:
    """arrays for the child, its job list, and (output key, expected array, label) checks"""

    def __init__(self):
        self.arrays, self.jobs, self.checks = {}, [], []

    def put(self, key, a):
        self.arrays[key] = np.ascontiguousarray(a)
        return key

    def job(self, **kw):
        self.jobs.append(kw)
        return kw["id"]

    def expect(self, key, want, label=None):
        self.checks.append((key, np.asarray(want), label or key))


# ---------------------------------------------------------------------------- Fr ops (zk_arr.hip)
ARR_SIZES = [1, 63, 257, 1000, 65537]  # 65537 under ZK_ARR_GRID=3: ~86 loop steps, ragged tail


def _fr_inputs(ctx, curve, n):
    def make():
        a, b, c = (ctx.gpu.gen_fr(curve, s + n, n) for s in (1, 2, 3))
        a[n // 2] = 0
        return a, b, c, ctx.gpu.gen_fr(curve, 4, 1)[0], ctx.gpu.gen_fr(curve, 5, 1)[0]
    return cached(("fr_in", curve, n), make)


def fr_ops(ctx, bt):
    """all 15 op codes of launch_arr_op (copy through append, sub_rev and set_const through the
    reference symbols) and arr_powers / arr_dot_prod, the calls of test_gpu_arr.test_elementwise"""
    o = ctx.oracle
    for curve in CURVES:
        for n in ARR_SIZES:
            a, b, c, kA, kB = _fr_inputs(ctx, curve, n)
            K = {k: bt.put(f"fr_{curve}_{n}_{k}", v) for k, v in (("a", a), ("b", b), ("c", c), ("kA", kA), ("kB", kB))}

            def want():
                w = {op: o.arr_op(curve, op, n, a, b, c, kA=kA, kB=kB)
                     for op in ("neg", "add", "sub", "sqr", "mul", "mul_add", "mul_sub", "scale", "Ax_plus_y",
                                "Ax_plus_By", "to_std", "from_std")}
                w["sub_rev"] = o.arr_op(curve, "sub", n, b, a)  # t = b - t
                w["set_const"] = np.tile(kA, (n, 1))
                w["append"] = np.concatenate([a, b])
                w["dot"] = o.arr_dot(curve, a, b)
                w["powers"] = o.arr_powers(curve, kA, kB, n)
                return w
            for op, w in cached(("fr_want", curve, n), want).items():
                jid = bt.job(id=f"fr_{curve}_{n}_{op}", call="arr", curve=curve, op=op, n=n, **K)
                bt.expect(jid, w)


INV_SIZES = [1, 31, 33, 100, 129, 1000, 4099]  # ZK_INV_LANES=1: CHK = clamp(n, 8, 128); 1000 = 7 x 128 + 104


def fr_inv(ctx, bt):
    """inv and div against the oracle, and the reference's zero rule (Fr_mont.c:258-285: one zero
    input zeroes EVERY output) with the zero in the last, ragged chunk"""
    o = ctx.oracle
    for curve in CURVES:
        for n in INV_SIZES:
            a = cached(("inv_a", curve, n), lambda: ctx.gpu.gen_fr(curve, 50 + n, n))
            b = cached(("inv_b", curve, n), lambda: ctx.gpu.gen_fr(curve, 60 + n, n))
            ka, kb = bt.put(f"inv_{curve}_{n}_a", a), bt.put(f"inv_{curve}_{n}_b", b)
            wi, wd = cached(("inv_want", curve, n),
                            lambda: (o.arr_op(curve, "inv", n, b), o.arr_op(curve, "div", n, a, b)))
            bt.expect(bt.job(id=f"inv_{curve}_{n}", call="arr", curve=curve, op="inv", a=kb), wi)
            bt.expect(bt.job(id=f"div_{curve}_{n}", call="arr", curve=curve, op="div", a=ka, b=kb), wd)
            if n >= 100:
                def zero_last():
                    z = b.copy()
                    z[n - 1] = 0
                    return z
                bz = cached(("inv_bz", curve, n), zero_last)
                kz = bt.put(f"inv_{curve}_{n}_bz", bz)
                zero = np.zeros((n, 4), dtype=np.uint64)
                wzi, wzd = cached(("inv_zwant", curve, n),
                                  lambda: (o.arr_op(curve, "inv", n, bz), o.arr_op(curve, "div", n, a, bz)))
                assert not wzi.any() and not wzd.any()  # the oracle states the same rule
                bt.expect(bt.job(id=f"invz_{curve}_{n}", call="arr", curve=curve, op="inv", a=kz), zero)
                bt.expect(bt.job(id=f"divz_{curve}_{n}", call="arr", curve=curve, op="div", a=ka, b=kz), zero)


# the (n1, n, zero_top) rows of test_gpu_arr.test_div_by_vanishing (its top two coefficients zeroed
# when n1 > 3: zero_top -2) and test_div_by_vanishing_shapes with n1 <= 70000
VANISH_ROWS = [(40, 8, -2, 91 + 40, 92), (33, 16, -2, 91 + 33, 92), (7, 8, -2, 91 + 7, 92), (64, 1, -2, 91 + 64, 92),
               (100, 32, -2, 91 + 100, 92), (0, 4, 0, 91, 92), (3 << 14, 1 << 14, -2, 91 + (3 << 14), 92),
               (5000, 37, 0, 97 + 37, 98), (130, 100, 3, 97 + 100, 98), (9000, 64, 4097, 97 + 64, 98),
               (70000, 65, 0, 97 + 65, 98), (20000, 20000, 0, 97 + 20000, 98), (12288, 1, 12000, 97 + 1, 98)]


VANISH_EXACT = [(100, 300), (64, 40)]  # (n, deg g + 1): chains of 3-4 steps with n % 64 != 0; deg - n < n


def vanish(ctx, bt):
    """quotient, remainder and the quot_by_vanishing verdict: n < 64, n not a multiple of 64,
    deg - n < n, deg < n, degrees far below the buffer's top"""
    for curve in CURVES:
        for n1, n, zt, seed, eseed in VANISH_ROWS:
            def make():
                poly = ctx.gpu.gen_fr(curve, seed, max(n1, 1))[:n1].copy()
                if zt == -2:
                    if n1 > 3:
                        poly[-2:] = 0
                elif zt:
                    poly[-zt:] = 0
                eta = ctx.gpu.gen_fr(curve, eseed, 1)[0]
                return poly, eta, ctx.oracle.div_by_vanishing(curve, poly, n, eta)
            poly, eta, (wq, wr, ok) = cached(("vanish", curve, n1, n), make)
            tag = f"van_{curve}_{n1}_{n}"
            jid = bt.job(id=tag, call="vanish", curve=curve, n=n, poly=bt.put(tag + "_p", poly),
                         eta=bt.put(tag + "_eta", eta))
            bt.expect(jid + "__q", wq)
            bt.expect(jid + "__r", wr)
            bt.expect(jid + "__ok", [ok])
            if ok:
                bt.expect(jid + "__quot", wq)
        # exact divisions p = (x^n - eta) g, built with the oracle: the verdict is True and the
        # quotient of quot_by_vanishing is g, on the forced kernels (the rows above divide exactly
        # only where the polynomial is empty)
        for n, m in VANISH_EXACT:
            def make_exact():
                o = ctx.oracle
                g = ctx.gpu.gen_fr(curve, 93 + n, m)
                eta = ctx.gpu.gen_fr(curve, 94, 1)[0]
                p = np.zeros((n + m, 4), dtype=np.uint64)
                p[n:] = g
                p[:m] = o.arr_op(curve, "sub", m, p[:m].copy(), o.arr_op(curve, "scale", m, g, kA=eta))
                wq, wr, ok = o.div_by_vanishing(curve, p, n, eta)
                assert ok and np.array_equal(wq, g) and not wr.any()
                return p, eta, g
            p, eta, g = cached(("vanish_exact", curve, n, m), make_exact)
            tag = f"vanx_{curve}_{n}_{m}"
            jid = bt.job(id=tag, call="vanish", curve=curve, n=n, poly=bt.put(tag + "_p", p),
                         eta=bt.put(tag + "_eta", eta))
            bt.expect(jid + "__q", g)
            bt.expect(jid + "__r", np.zeros((n, 4), dtype=np.uint64))
            bt.expect(jid + "__ok", [True])
            bt.expect(jid + "__quot", g)


# ---------------------------------------------------------------------------- batch affine conversion, group FFT (zk_g1ext.hip)
AFFINE_SIZES = [1, 2, 31, 33, 1000]  # ZK_NORM_LANES=1: chk = clamp(n, 2, 32); =100: chk = 10 at 1000


def _points(ctx, curve, coords, n, seed, n_inf):
    f = golden_io.projective_points if coords == "proj" else golden_io.jacobian_points
    return cached(("pts", curve, coords, n, seed, n_inf), lambda: f(ctx.gpu, ctx.oracle, curve, n, seed, n_inf))


def to_affine(ctx, bt):
    """batch_to_affine in both coordinate systems, random Z and infinities, against the reference"""
    for curve in CURVES:
        NP = ctx.gpu.NLIMBS_P[curve]
        for coords, seed in (("proj", 102), ("jac", 112)):
            for n in AFFINE_SIZES:
                pts = _points(ctx, curve, coords, n, seed + n, min(3, n // 2))

                def want():
                    w = np.zeros((n, 2 * NP), dtype=np.uint64)
                    ctx.reference.arr(curve, f"G1_{coords}_batch_to_affine", n, pts, w)
                    return w
                tag = f"aff_{curve}_{coords}_{n}"
                jid = bt.job(id=tag, call="to_affine", curve=curve, coords=coords, pts=bt.put(tag + "_in", pts))
                bt.expect(jid, cached(("aff_want", curve, coords, n), want))


FFT_SIZES = [1, 2, 3, 5, 7, 8]  # forced radix 4: [1] [2] [3] [4, 1] [4, 3] [4, 4]; radix 3: ... [3, 2] [3, 3, 1] [3, 3, 2]


def forced_plan(radix, m):
    """radix_plan under ZK_FFT_RADIX (zk_g1ext.hip): 1 = the fused radix-2 stages (no plan), 2..4 =
    that many bits per stage, the last stage taking the remainder"""
    if radix == 1:
        return []
    plan, left = [], m
    while left > 0:
        plan.append(min(radix, left))
        left -= plan[-1]
    return plan


def _fft_case(ctx, bt, curve, coords, m, pts, tag, glv, plan, root=None):
    gen = ctx.gpu.get_fft_subgroup(curve, m).gen_array()
    extra = {}
    if root is not None:  # a named root of tests/generators.py instead of the canonical generator
        gen = generators.root(curve, m, gen, root)
        extra["gen"] = bt.put(tag + "_gen", gen)
    kin = bt.put(tag + "_in", pts)
    for inverse in (False, True):
        name = f"G1_{coords}_fft_{'inverse' if inverse else 'forward'}"

        def want():
            w = np.zeros_like(pts)
            ctx.reference.arr(curve, name, m, gen, pts, w)
            return w
        jid = bt.job(id=f"{tag}_{'inv' if inverse else 'fwd'}", call="fft", curve=curve, coords=coords, m=m,
                     inverse=inverse, pts=kin, **extra)
        bt.expect(jid, cached(("fft_want", tag, inverse), want))
        bt.expect(jid + "__glv", [glv])
        if plan is not None:
            bt.expect(jid + "__plan", np.array(plan, dtype=np.int64))


def fft(ctx, bt, sizes=FFT_SIZES, radix=None, glv=1, nonsubgroup=False):
    """forward and inverse, projective and Jacobian, subgroup points with random Z and up to 2
    infinities, against the reference as test_gpu_g1ext.test_fft_vs_reference; the plan the child
    reports must be the forced one"""
    for curve in CURVES:
        for m in sizes:
            n = 1 << m
            plan = None if radix is None else forced_plan(radix, m)
            for coords, seed in (("proj", 200), ("jac", 210)):
                pts = _points(ctx, curve, coords, n, seed + m, min(2, n // 2))  # m = 1: one finite point
                _fft_case(ctx, bt, curve, coords, m, pts, f"fft_{curve}_{coords}_{m}", glv, plan)
    if nonsubgroup:  # BLS12-381 points outside the r-subgroup (test_fft_nonsubgroup_points_bls, m = 3)
        curve, m = "bls12_381", 3
        aff = golden_io.bls_nonsubgroup_points(1 << m, 300 + m)
        pts = cached(("nonsub", m), lambda: ctx.gpu.batch_from_affine(curve, aff))
        _fft_case(ctx, bt, curve, "proj", m, pts, f"fftns_{curve}_{m}", 0, None)


def fft_other_generator(ctx, bt, radix, m=5, root="cube"):
    """the forced stages with a generator other than the canonical one (tests/generators.py), projective,
    one size per curve: the stage twiddles are derived from the generator argument"""
    for curve in CURVES:
        pts = _points(ctx, curve, "proj", 1 << m, 200 + m, 2)
        _fft_case(ctx, bt, curve, "proj", m, pts, f"fftgen_{curve}_{m}_{root}", 1, forced_plan(radix, m), root=root)


def fft_norm(ctx, bt):
    """the FFT's closing normalisation is k_norm_chunks too (MODE_XYZZ_TO_PROJ, bit-reversed
    output order on the inverse): the inversion / chunk switches reach it through the group FFT"""
    fft(ctx, bt, sizes=[3, 5])


# ---------------------------------------------------------------------------- G2 conversion and transform (zk_g2norm.hpp's chain)
G2_AFFINE_SIZES = [1, 2, 31, 33, 257]  # ZK_NORM_LANES=1: chk = clamp(n, 2, 32), 257 rows = 9 lanes of 28 / 29; =100: chk = 2


def _g2_rows(ctx, curve):
    """distinct finite projective G2 rows (Z != 1) and the infinity (0 : 1 : 0), from the reference"""
    def make():
        NP = ctx.gpu.NLIMBS_P[curve]
        rows = golden_io.g2_proj_points(ctx.reference.lib, curve, max(G2_AFFINE_SIZES))
        inf = np.zeros((1, 6 * NP), np.uint64)
        ctx.reference.arr(curve, "G2_proj_batch_from_affine", 1, np.full((1, 4 * NP), ALL_ONES, np.uint64), inf)
        assert rows[:, 4 * NP:].any(axis=1).all() and not inf[0, 4 * NP:].any()
        return rows, inf[0]
    return cached(("g2rows", curve), make)


def g2_infinity_rows(n):
    """rows written with Z = 0: none at n = 1 (a finite row), the first at n = 2, and from 31 rows the
    first, the last and every row of one of the 9 strided lanes that 257 rows have under
    ZK_NORM_LANES=1 (rows = 3 mod 9: that lane's product is 1 throughout)"""
    if n < 2:
        return []
    return [0] if n == 2 else sorted({0, n - 1} | set(range(3, n, 9)))


def g2_to_affine(ctx, bt):
    """G2 batch_to_affine: finite rows with Z != 1 and both forms of infinity, (0 : 1 : 0) and
    (x : y : 0), alternating over g2_infinity_rows, against the reference's G2_proj_batch_to_affine"""
    for curve in CURVES:
        NP = ctx.gpu.NLIMBS_P[curve]
        rows, inf = _g2_rows(ctx, curve)
        for n in G2_AFFINE_SIZES:
            def make():
                pts = rows[:n].copy()
                for k, i in enumerate(g2_infinity_rows(n)):
                    if k % 2 == 0:
                        pts[i] = inf
                    else:
                        pts[i, 4 * NP:] = 0  # (x : y : 0)
                w = np.zeros((n, 4 * NP), dtype=np.uint64)
                ctx.reference.arr(curve, "G2_proj_batch_to_affine", n, pts, w)
                fin = np.ones(n, bool)
                fin[g2_infinity_rows(n)] = False
                assert (w[~fin] == ALL_ONES).all() and not (w[fin] == ALL_ONES).all(axis=1).any()
                return pts, w
            pts, w = cached(("g2aff", curve, n), make)
            tag = f"g2aff_{curve}_{n}"
            bt.expect(bt.job(id=tag, call="g2_to_affine", curve=curve, pts=bt.put(tag + "_in", pts)), w)


G2_FFT_SIZES = [0, 1, 3, 5]


def g2_fft(ctx, bt):
    """the G2 transform, whose closing normalisation runs the same chain on ZZZ: distinct finite rows,
    at m = 5 with row 0 the infinity (0 : 1 : 0), against the reference's G2_proj_fft_forward / _inverse"""
    for curve in CURVES:
        rows, inf = _g2_rows(ctx, curve)
        for m in G2_FFT_SIZES:
            def make():
                pts = rows[:1 << m].copy()
                if m == 5:
                    pts[0] = inf
                gen = ctx.gpu.get_fft_subgroup(curve, m).gen_array()
                w = {}
                for inverse in (False, True):
                    w[inverse] = np.zeros_like(pts)
                    ctx.reference.arr(curve, f"G2_proj_fft_{'inverse' if inverse else 'forward'}", m, gen, pts, w[inverse])
                return pts, w
            pts, w = cached(("g2fft", curve, m), make)
            kin = bt.put(f"g2fft_{curve}_{m}_in", pts)
            for inverse in (False, True):
                jid = bt.job(id=f"g2fft_{curve}_{m}_{'inv' if inverse else 'fwd'}", call="g2_fft", curve=curve, m=m,
                             inverse=inverse, pts=kin)
                bt.expect(jid, w[inverse])


# ---------------------------------------------------------------------------- G1 MSM (zk_msm_impl.hpp)
R_MOD = golden_io.FR_ORDER
P_MOD = {"bn128": 21888242871839275222246405745257275088696311157297823662689037894645226208583,
         "bls12_381": golden_io.P_BLS}


def _neg(curve, pt, NP):
    """-P of an affine point in Montgomery form: y -> p - y (test_gpu_msm_bits._neg)"""
    y = sum(int(pt[NP + j]) << (64 * j) for j in range(NP))
    out = pt.copy()
    out[NP:] = golden_io._limbs((P_MOD[curve] - y) % P_MOD[curve], NP)
    return out


def _bits_inputs(ctx, curve, n):
    """the all-ones scalars, the infinity mix and the P / -P mixes of tests/test_gpu_msm_bits.py at n
    pairs: (name, scalars, points, mont)"""
    gpu = ctx.gpu
    NP = gpu.NLIMBS_P[curve]
    std = np.zeros((n, 4), dtype=np.uint64)
    std[:] = golden_io._limbs(R_MOD[curve] - 1, 4)  # r - 1, standard form: every bit job holds many points
    base = gpu.gen_points(curve, 94, 3)
    rep = np.tile(base[0], (n, 1))
    rep[::7] = ALL_ONES  # one point repeated, infinity inputs mixed in
    pm = np.empty((n, 2 * NP), dtype=np.uint64)
    pm[0::2] = base[1]
    pm[1::2] = _neg(curve, base[1], NP)  # P, -P, P, ... with equal scalars: the pairs cancel
    mix = pm.copy()
    mix[2::3] = base[2]
    eq = np.tile(gpu.gen_fr(curve, 96, 1), (n, 1))
    return [("ones", std, gpu.gen_points(curve, 91, n), False), ("inf", gpu.gen_fr(curve, 95, n), rep, True),
            ("cancel", eq, pm, True), ("pmmix", eq, mix, True)]


def msm_bits(ctx, bt, sizes):
    """default-window host calls: the bit-job path (k_bitacc / k_bitsum), or with ZK_MSM_BITS_MAX=0
    the bucket pipeline at the default window, against the oracle"""
    for curve in CURVES:
        for n in sizes:
            def make():
                return [(name, sc, pts, mont, ctx.oracle.msm(curve, sc, pts, mont=mont))
                        for name, sc, pts, mont in _bits_inputs(ctx, curve, n)]
            for name, sc, pts, mont, want in cached(("bits", curve, n), make):
                tag = f"bits_{curve}_{n}_{name}"
                jid = bt.job(id=tag, call="msm_affine", curve=curve, std=not mont, sc=bt.put(tag + "_sc", sc),
                             pts=bt.put(tag + "_pts", pts))
                bt.expect(jid, want)


def _bucket_cases(ctx, curve):
    """the (window, n) pairs of test_gpu_msm.test_ysum_kernels_vs_oracle, every 97th point infinity,
    and one all-equal-scalar case at n = 20000 (bucket runs cross chunk boundaries at every CH):
    (name, window, std scalars, points, normalised projective result of the oracle)"""
    def make():
        gpu, o = ctx.gpu, ctx.oracle
        rows = []
        for name, window, n, equal in (("w13", 13, 3000, False), ("w16", 16, 20000, False), ("w20", 20, 5000, False),
                                       ("equal", 16, 20000, True)):
            if equal:
                sc = np.tile(o.to_std(FR_FLD[curve], gpu.gen_fr(curve, 830, 1)), (n, 1))
            else:
                sc = o.to_std(FR_FLD[curve], gpu.gen_fr(curve, 800 + window, n))
            pts = gpu.gen_points(curve, 801 + window, n)
            pts[::97] = ALL_ONES
            rows.append((name, window, sc, pts, o.normalize(curve, o.msm(curve, sc, pts, mont=False, out="proj"))))
        return rows
    return cached(("buckets", curve), make)


def msm_buckets(ctx, bt):
    """explicit windows (always the bucket pipeline), host buffers, through
    <C>_G1_proj_MSM_std_coeff_proj_out_variable"""
    for curve in CURVES:
        for name, window, sc, pts, want in _bucket_cases(ctx, curve):
            tag = f"bkt_{curve}_{name}"
            jid = bt.job(id=tag, call="msm_variable", curve=curve, window=window, sc=bt.put(tag + "_sc", sc),
                         pts=bt.put(tag + "_pts", pts))
            bt.expect(jid, want)


def msm_buckets_device(ctx, bt):
    """the same cases device-resident (zkg_g1_msm_device): under ZK_MSM_AHEAD_MIN=12 BN128 runs two
    window groups from 2^12 pairs (the switch is BN128's: msm_ahead reads it for fields at three
    accumulation waves per SIMD).  The raw projective result is normalised by the oracle."""
    for curve in CURVES:
        for name, window, sc, pts, want in _bucket_cases(ctx, curve):
            tag = f"bktdev_{curve}_{name}"
            jid = bt.job(id=tag, call="msm_device", curve=curve, window=window, mont=False,
                         sc=bt.put(tag + "_sc", sc), pts=bt.put(tag + "_pts", pts))
            bt.expect(jid, want, label="normalize:" + curve)
            if curve == "bn128" and sc.shape[0] >= 1 << 12:
                bt.expect(jid + "__groups", [2])


def msm_split(ctx, bt):
    """host buffers at 2^17 pairs, the smallest size that runs a split pipeline, with the "mix3"
    skewed scalars of test_gpu_msm.test_host_split_pipeline_skewed, against the oracle"""
    n = 1 << 17
    for curve in CURVES:
        def make():
            sc = golden_io.skew_scalars(ctx.gpu.gen_fr, curve, 717, n, "mix3")
            pts = ctx.gpu.gen_points(curve, 718, n)
            return sc, pts, ctx.oracle.msm(curve, sc, pts, mont=True)
        sc, pts, want = cached(("split", curve), make)
        tag = f"split_{curve}"
        jid = bt.job(id=tag, call="msm_affine", curve=curve, std=False, sc=bt.put(tag + "_sc", sc),
                     pts=bt.put(tag + "_pts", pts))
        bt.expect(jid, want)


# ---------------------------------------------------------------------------- G2 MSM
def ysum_block_level(c, bits):
    """make_shape / GroupPass::reduce_tail (zk_msm_impl.hpp) restated: True when the pipeline of
    window c over `bits`-bit scalars runs the block-level Y sums, the only shapes at which
    ZK_YSUM_G2_LDS is read (n0 % 256 == 0 && n1 % 256 == 0: every c from 12 up)"""
    W, B, l0 = bits // c + 1, 1 << (c - 1), c // 2
    l1 = c - 1 - l0
    q = min(max((2 * W * B + 65535) // 65536, 1), 16)
    qy = 1
    while qy < q:
        qy *= 2
    n0 = (1 << l1) * min(max((1 << l0) // qy, 1), 64)
    n1 = (1 << l0) * min(max((1 << l1) // qy, 1), 64)
    return n0 % 256 == 0 and n1 % 256 == 0


G2_SIZES = (1, 257, 2048, 4097)  # 4097: the smallest default-window call past the bit-job path
G2_DEVICE = (2048, 12)  # (pairs, explicit window) of the device-resident case


def g2_msm(ctx, bt):
    """the inputs of test_gpu_g2.test_g2_msm_vs_reference at n in {1, 257, 2048}: Montgomery and
    standard scalars with affine output, and the projective output normalised by the reference.
    Those three sizes are default-window calls of at most msm_bits_max = 4096 pairs, which take the
    bit-job path on G2 as on G1 and never read ZK_YSUM_G2_LDS.  The switch is read by the bucket
    pipeline's block-level Y sums only, so two more cases reach them: a host call at 4097 pairs
    (default window 10; Montgomery scalars, affine output) and a device-resident call of 2048 pairs
    with the explicit window 12, through zkg_g2_msm_device."""
    ref = ctx.reference
    for curve in CURVES:
        NP = ctx.gpu.NLIMBS_P[curve]
        bits = golden_io.FR_ORDER[curve].bit_length()
        assert ctx.gpu.load().zkg_msm_default_window(4097) == 10 and ysum_block_level(10, bits)
        assert ysum_block_level(G2_DEVICE[1], bits) and not ysum_block_level(8, bits)
        allpts = cached(("g2pts", curve), lambda: golden_io.g2_points(ref.lib, curve, max(G2_SIZES)))
        for n in G2_SIZES:
            pts = np.ascontiguousarray(allpts[:n])
            sc = cached(("g2sc", curve, n), lambda: ctx.gpu.gen_fr(curve, 500 + n, n))

            def want():
                w = {}
                for mont in (True, False) if n <= 2048 else (True,):
                    out = np.zeros(4 * NP, np.uint64)
                    ref.arr(curve, f"G2_proj_MSM_{'mont' if mont else 'std'}_coeff_affine_out", n, sc, pts, out, 4)
                    w[mont] = out
                if n > 2048:
                    return w
                proj, nrm = np.zeros(6 * NP, np.uint64), np.zeros(6 * NP, np.uint64)
                ref.arr(curve, "G2_proj_MSM_mont_coeff_proj_out", n, sc, pts, proj, 4)
                ref.arr(curve, "G2_proj_normalize", proj, nrm)
                w["proj"] = nrm
                return w
            w = cached(("g2want", curve, n), want)
            tag = f"g2_{curve}_{n}"
            ks, kp = bt.put(tag + "_sc", sc), bt.put(tag + "_pts", pts)
            for mont in (m for m in (True, False) if m in w):
                jid = bt.job(id=f"{tag}_{'mont' if mont else 'std'}", call="g2_msm", curve=curve, std=not mont,
                             affine=True, sc=ks, pts=kp)
                bt.expect(jid, w[mont])
            if "proj" not in w:
                continue
            bt.expect(bt.job(id=tag + "_proj", call="g2_msm", curve=curve, std=False, affine=False, sc=ks, pts=kp),
                      w["proj"])
            if n == G2_DEVICE[0]:
                bt.expect(bt.job(id=tag + "_dev", call="g2_msm_device", curve=curve, window=G2_DEVICE[1], sc=ks,
                                 pts=kp), w["proj"])


# ---------------------------------------------------------------------------- edge values (tests/field_edges.py)
def fr_edges(ctx, bt):
    """the vectors of test_gpu_field_edges: every Fr op on the edge cross product E x E' with the
    constants 0, R mod r, r - 1 and a random one, and inv / div over E \\ {0} with the zero rule;
    expected values from the big-integer models"""
    for curve in CURVES:
        a, b, c, ks = fe.fr_cross(curve)
        want = fe.fr_cross_expected(curve)
        n = len(a)
        K = {k: bt.put(f"fre_{curve}_{k}", fe.to_limbs(v, 4)) for k, v in (("a", a), ("b", b), ("c", c))}
        kk = [bt.put(f"fre_{curve}_k{i}", fe.to_row(k, 4)) for i, k in enumerate(ks)]
        for op in fe.UNARY + fe.BINARY + fe.TERNARY + ("dot",):
            jid = bt.job(id=f"fre_{curve}_{op}", call="arr", curve=curve, op=op, n=n, **K)
            bt.expect(jid, want[op][0] if op == "dot" else want[op])
        for i in range(4):
            for op in ("scale", "Ax_plus_y", "Ax_plus_By"):
                jid = bt.job(id=f"fre_{curve}_{op}_{i}", call="arr", curve=curve, op=op, n=n, kA=kk[i],
                             kB=kk[(i + 1) % 4], **K)
                bt.expect(jid, want[f"{op}_{i}"])
        M = fe.fr_model(curve)
        for name, x, y in fe.inv_vectors(curve):
            kx, ky = bt.put(f"fre_{curve}_{name}_x", fe.to_limbs(x, 4)), bt.put(f"fre_{curve}_{name}_y", fe.to_limbs(y, 4))
            wi, wd = cached(("fre_inv", curve, name), lambda: (fe.to_limbs(M.inv(y), 4), fe.to_limbs(M.div(x, y), 4)))
            bt.expect(bt.job(id=f"fre_{curve}_{name}_inv", call="arr", curve=curve, op="inv", a=ky), wi)
            bt.expect(bt.job(id=f"fre_{curve}_{name}_div", call="arr", curve=curve, op="div", a=kx, b=ky), wd)


def fp_edges(ctx, bt, chk=2):
    """the off-curve Fp edge rows through batch_to_affine in both coordinate systems, and the
    infinity layouts at n = 257 for lanes that own `chk` rows (2 by default; ZK_NORM_LANES=1 gives
    chk = 32: whole 28- / 29-row lanes infinite, an infinity first and last in a lane); expected
    values from the big-integer model"""
    for curve in CURVES:
        nl, M = ctx.gpu.NLIMBS_P[curve], fe.fp_model(curve)
        for coords in ("proj", "jac"):
            def edge_rows():
                rows = fe.offcurve_rows(curve)
                return fe.point_rows(rows, nl), fe.affine_rows(M, rows, coords)
            pts, want = cached(("fpe", curve, coords), edge_rows)
            tag = f"fpe_{curve}_{coords}"
            bt.expect(bt.job(id=tag, call="to_affine", curve=curve, coords=coords, pts=bt.put(tag + "_in", pts)), want)

            def layouts():
                return [(name, p, fe.affine_rows(M, fe.point_ints(p, nl), coords))
                        for name, p in fe.layout_rows(ctx.gpu, ctx.oracle, curve, coords, 257, chk, 957)]
            for name, p, want in cached(("fpe_lay", curve, coords, chk), layouts):
                tag = f"fpe_{curve}_{coords}_{chk}_{name}"
                bt.expect(bt.job(id=tag, call="to_affine", curve=curve, coords=coords, pts=bt.put(tag + "_in", p)), want)


def msm_digit_edges(ctx, bt):
    """the 2^256 - 1 and alternating B / B + 1 digit patterns (256-bit std scalars, verbatim) at
    c = 16 through the bucket pipeline, and as a default-window call (bit jobs; the bucket pipeline
    under ZK_MSM_BITS_MAX=0), against the oracle"""
    c, n = 16, 192
    for curve in CURVES:
        pts = cached(("dig_pts", curve), lambda: fe.digit_points(ctx.gpu.gen_points, curve, n))
        kp = bt.put(f"dig_{curve}_pts", pts)
        for name in ("all_ones", "alt_B_Bp1", "alt_Bp1_B", "rotated"):
            sc = fe.digit_scalars(curve, c, name, n)
            proj, aff = cached(("dig_want", curve, name), lambda: (
                ctx.oracle.normalize(curve, ctx.oracle.msm(curve, sc, pts, mont=False, out="proj")),
                ctx.oracle.msm(curve, sc, pts, mont=False)))
            tag = f"dig_{curve}_{name}"
            ks = bt.put(tag + "_sc", sc)
            bt.expect(bt.job(id=tag + "_var", call="msm_variable", curve=curve, window=c, sc=ks, pts=kp), proj)
            bt.expect(bt.job(id=tag + "_aff", call="msm_affine", curve=curve, std=True, sc=ks, pts=kp), aff)


# ---------------------------------------------------------------------------- the table
def _rows():
    rows = []

    def add(env, *batteries):
        rows.append((env, batteries))
    # Fr element-wise ops: the four k_arr_op instantiations, each with its one-pass grid and with a
    # 3-workgroup grid (grid-stride loop, stage 4's software pipeline included); the round-5 kernel
    for stage in ("0", "1", "2", "4"):
        add({"ZK_ARR_STAGE": stage}, fr_ops, fr_edges)
        add({"ZK_ARR_STAGE": stage, "ZK_ARR_GRID": "3"}, fr_ops)
    add({"ZK_ARR_MAP": "1"}, fr_ops, fr_edges)
    # Fr batch inversion: the other three k_inv_chunks branches, CHK = clamp(n, 8, 128), and both.
    # ZK_INV_SG and ZK_INV_STRIDE are read by the batch affine conversion (and the FFT's closing
    # normalisation) as well.
    add({"ZK_INV_SG": "0"}, fr_inv, to_affine, fft_norm, fr_edges, fp_edges)
    add({"ZK_INV_STRIDE": "0"}, fr_inv, to_affine, fft_norm, fp_edges)
    add({"ZK_INV_ILP": "0"}, fr_inv, fr_edges)
    add({"ZK_INV_LANES": "1"}, fr_inv, fr_edges)
    for flag in ("ZK_INV_SG", "ZK_INV_STRIDE", "ZK_INV_ILP"):
        add({flag: "0", "ZK_INV_LANES": "1"}, fr_inv)
    add({"ZK_VANISH_LEGACY": "1"}, vanish)
    add({"ZK_VANISH_STAGED": "1"}, vanish)
    # batch affine conversion: the other k_norm_chunks branches, chk = clamp(n, 2, 32), chk = 10
    add({"ZK_NORM_BF": "0"}, to_affine, fft_norm, fp_edges)
    # (the G2 conversion and transform size their shared norm chain with ZK_NORM_LANES as well)
    add({"ZK_NORM_LANES": "1"}, to_affine, fft_norm, lambda ctx, bt: fp_edges(ctx, bt, chk=32), g2_to_affine, g2_fft)
    add({"ZK_NORM_LANES": "100"}, to_affine, fft_norm, g2_to_affine, g2_fft)
    for flag in ("ZK_INV_SG", "ZK_INV_STRIDE", "ZK_NORM_BF"):
        add({flag: "0", "ZK_NORM_LANES": "1"}, to_affine, fft_norm)
    # group FFT: the fused radix-2 stages, radix 4 / 8 / 16 Stockham stages with remainder stages,
    # and the integer stages
    for radix in (1, 2, 3, 4):
        add({"ZK_FFT_RADIX": str(radix)}, lambda ctx, bt, r=radix: fft(ctx, bt, radix=r),
            *([lambda ctx, bt: fft_other_generator(ctx, bt, 1)] if radix == 1 else []))
    add({"ZK_FFT_GLV": "0"}, lambda ctx, bt: fft(ctx, bt, glv=0, nonsubgroup=True))
    # G1 MSM, bit jobs.  ZK_MSM_BITS_G=1 asks for one block, msm_bits_groups caps the chunk at
    # BITACC_MAX_K = 256 and msm_run_bits spreads the pairs evenly over the blocks that leaves:
    # 256 -> G = 1, K = 256 (the LDS staging exactly full); 257 -> G = 2, K = 129 (last block 128);
    # 511 -> G = 2, K = 256 with a ragged last block of 255; 1000 -> G = 4, K = 250 (even).
    # =7: seven blocks.  ZK_MSM_BITS_MAX=0: the bucket pipeline at the default window for small n
    for g in ("1", "7"):
        add({"ZK_MSM_BITS_G": g}, lambda ctx, bt: msm_bits(ctx, bt, [256, 257, 511, 1000]))
    add({"ZK_MSM_BITS_MAX": "0"}, lambda ctx, bt: msm_bits(ctx, bt, [1, 257, 4096]), msm_digit_edges)
    # G1 MSM, bucket pipeline: the chunk rule's own lengths, both ends of the Y-sum bucket count,
    # both Y-sum kernels, the sort-ahead window groups
    for ch in ("4", "64", "128"):
        add({"ZK_MSM_CH": ch}, msm_buckets, msm_digit_edges)
    for qy in ("1", "16"):  # 16 is also the value when the variable is unset: only 1 is a non-default path
        add({"ZK_YSUM_QY": qy}, msm_buckets)
    for mode in ("0", "1"):
        add({"ZK_YSUM3": mode}, msm_buckets, msm_digit_edges)
    add({"ZK_YSUM3_LANES": "1"}, msm_buckets)
    add({"ZK_MSM_AHEAD_MIN": "12"}, msm_buckets_device)
    # G1 MSM, host-buffer split pipeline
    add({"ZK_MSM_SORT_INLINE": "1"}, msm_split)
    add({"ZK_MSM_SPLIT_W": "1,3"}, msm_split)
    # G2 MSM: each value is the non-default one for one of the curves
    for v in ("0", "1"):
        add({"ZK_YSUM_G2_LDS": v}, g2_msm)
    return rows


ROWS = _rows()
ROW_IDS = ["-".join(f"{k}={v}" for k, v in env.items()) for env, _ in ROWS]
TABLE_SWITCHES = {k for env, _ in ROWS for k in env}

_TROUBLE = []  # why a child ended in trouble: no child is started after that


def _trouble(why, tail=""):
    _TROUBLE.append(why)
    pytest.fail(f"{why}\n{tail}", pytrace=False)


def run_child(env, bt, tmp_path):
    """one fresh interpreter with the switches set; never retried.  A child killed by a signal,
    aborted, timed out or reporting a device fault stops every later test of this module."""
    if _TROUBLE:
        pytest.fail(f"not started: an earlier child ended in trouble ({_TROUBLE[0]})", pytrace=False)
    src, dst = tmp_path / "inputs.npz", tmp_path / "outputs.npz"
    np.savez(src, jobs=np.frombuffer(json.dumps(bt.jobs).encode(), dtype=np.uint8), **bt.arrays)
    base = {k: v for k, v in os.environ.items() if k not in TABLE_SWITCHES and k not in EXCLUDED}
    try:
        p = subprocess.run([sys.executable, CHILD, str(src), str(dst)], env=dict(base, **env), capture_output=True,
                           text=True, timeout=CHILD_TIMEOUT, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _trouble(f"child hit its {CHILD_TIMEOUT} s limit under {env}")
    tail = (p.stdout + p.stderr)[-3000:]
    if p.returncode < 0 or p.returncode in (134, 139):
        _trouble(f"child ended with status {p.returncode} under {env}", tail)
    if "illegal memory access" in p.stdout + p.stderr:
        _trouble(f"child reported an illegal memory access under {env}", tail)
    assert p.returncode == 0, tail
    with np.load(dst, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.gpu
@pytest.mark.parametrize("row", range(len(ROWS)), ids=ROW_IDS)
def test_switch(request, tmp_path, row):
    env, batteries = ROWS[row]
    ctx = Ctx(request)
    bt = Battery()
    for b in batteries:
        b(ctx, bt)
    out = run_child(env, bt, tmp_path)
    bad = []
    for key, want, label in bt.checks:
        got = out.get(key)
        if got is not None and label.startswith("normalize:"):
            got = ctx.oracle.normalize(label.split(":")[1], got)
        if got is None or got.shape != want.shape or not np.array_equal(got, want):
            bad.append(key)
    assert not bad, f"{len(bad)} of {len(bt.checks)} outputs differ from the reference under {env}: {bad[:12]}"
    assert len(bt.checks) > 0


def test_switch_table_is_complete():
    """every getenv("ZK_*") of csrc, direct or through zk_runtime.hpp's readers (env_on, env_is1,
    env_pos, env_int), is a key of the table above or of EXCLUDED, and the table names
    no switch the code does not read: a mistyped name or a switch added without a test fails here"""
    found = set()
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name), encoding="utf-8", errors="replace") as f:
            found |= set(re.findall(r'\b(?:getenv|env_on|env_is1|env_pos|env_int)\("(ZK_[A-Z0-9_]+)"', f.read()))
    assert found, "no ZK_* switch found under csrc"
    assert not (TABLE_SWITCHES & set(EXCLUDED)), "a switch is both tested and excluded"
    assert found == TABLE_SWITCHES | set(EXCLUDED), (
        f"untested: {sorted(found - TABLE_SWITCHES - set(EXCLUDED))}; "
        f"not in csrc: {sorted((TABLE_SWITCHES | set(EXCLUDED)) - found)}")
