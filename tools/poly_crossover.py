#!/usr/bin/env python3
"""Crossover of the polynomial product's two paths (GPU box): the shorter factor runs over
1, 2, 4, ... 256 against a long factor of 2^12, 2^16 and 2^20 coefficients, device-resident, once
on the direct kernel and once on the transform path (zkg_poly_set_mul_direct_max).  The default of
POLY_MUL_DIRECT_MAX (zk_poly.hip) is the largest short length at which the direct kernel still
wins at all three long sizes.  Output: profiles/r08a_poly_crossover.txt.

    python tools/poly_crossover.py
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zikkurat-algebra_amd"))

import zkalgebra as zk  # noqa: E402

CURVE = "bls12_381"


def timeit(fn, reps=20):
    fn()
    zk.load().zkg_device_synchronize()
    best = 1e9
    for _ in range(3):
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        zk.load().zkg_device_synchronize()
        best = min(best, (time.perf_counter() - t) / reps)
    return best


def main():
    zk.require_gpu()
    lib, cid = zk.load(), zk.CURVE_ID[CURVE]
    wins = {}
    print(f"# {CURVE}, device-resident, ms per product (best of 3 x 20); direct = k_poly_mul_direct, ntt = transform path")
    print(f"{'long':>8} {'short':>6} {'direct':>9} {'ntt':>9}  winner")
    for lg in (12, 16, 20):
        nl = 1 << lg
        da = zk.DeviceBuffer(zk.gen_fr(CURVE, 1, nl))
        db = zk.DeviceBuffer(zk.gen_fr(CURVE, 2, 256))
        dt = zk.DeviceBuffer.empty((nl + 256) * 32)
        for ns in (1, 2, 4, 8, 16, 32, 64, 128, 256):
            f = lambda: lib.zkg_poly_mul_device(cid, nl, da.ptr, ns, db.ptr, dt.ptr)
            zk.poly_set_mul_direct_max(1 << 30)
            d = timeit(f)
            zk.poly_set_mul_direct_max(0)
            t = timeit(f)
            wins.setdefault(ns, []).append(d < t)
            print(f"{'2^%d' % lg:>8} {ns:6d} {d * 1e3:9.4f} {t * 1e3:9.4f}  {'direct' if d < t else 'ntt'}")
        for d in (da, db, dt):
            d.free()
    zk.poly_set_mul_direct_max(-1)
    best = 0
    for ns in sorted(wins):
        if not all(wins[ns]):
            break
        best = ns
    print(f"# largest short length at which the direct kernel wins at all three long sizes: {best}")


if __name__ == "__main__":
    main()
