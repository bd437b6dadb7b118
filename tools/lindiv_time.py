#!/usr/bin/env python3
"""Division by a linear factor and KZG opening timing (GPU box):
    python tools/lindiv_time.py [--out FILE]     -> profiles/kzg_open_time.json
Device-resident buffers; every entry is synchronous, so a host clock around the call times all of it
(the conventions of tools/poly_div_time.py): one warm-up call per shape, then REPS timed calls, median / min /
max.
  division   zkg_poly_div_linear_device at n = 2^12, 2^16, 2^20, 2^24 with one point and at 2^20 with 16
             points, both curves; bytes per second counted as 96 B per row and point (two reads, one write)
  routes     the two routes the library already had, in the same run, on the same polynomial:
             zkg_poly_long_div_device with a two-coefficient divisor and zkg_poly_div_by_vanishing_device with
             expo_n = 1 (one lane walks the whole chain), at 2^16 and 2^20
  condition  the new division at 2^20, one point, is faster than both (asserted at the end)
  openings   zkg_kzg_open_device at 2^16 and 2^20 beside its two parts in calls of their own: the division
             (zkg_poly_div_linear_device) and the MSM of the n - 1 quotient rows (zkg_kzg_commit_device)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zikkurat-algebra_amd"), ROOT):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import zkalgebra as zk  # noqa: E402

CURVES = ("bn128", "bls12_381")
DIV_SHAPES = [(1 << 12, 1), (1 << 16, 1), (1 << 20, 1), (1 << 24, 1), (1 << 20, 16)]
ROUTE_SIZES = (1 << 16, 1 << 20)
OPEN_SIZES = (1 << 16, 1 << 20)


def reps_for(n):
    return 30 if n <= 1 << 12 else 15 if n <= 1 << 16 else 7


def timed(call, reps):
    call()  # warm-up
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "calls": len(ts)}


def ok(rc):
    assert rc == 0, zk.last_error()


def main():
    zk.require_gpu()
    lib = zk.load()
    path = os.path.join(ROOT, "profiles", "kzg_open_time.json")
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    out = {"rows_per_lane": zk.poly_lindiv_tile(), "bytes_per_row_and_point": 96, "division": {}, "routes": {},
           "openings": {}}
    for curve in CURVES:
        cid = zk.CURVE_ID[curve]
        nmax = max(n for n, _ in DIV_SHAPES)
        d_p = zk.DeviceBuffer(zk.gen_fr(curve, 21, nmax))
        d_q = zk.DeviceBuffer.empty(max(nz * (n - 1) for n, nz in DIV_SHAPES) * 32)
        zs = zk.gen_fr(curve, 22, 16)
        for n, nz in DIV_SHAPES:
            ts = timed(lambda: ok(zk.poly_div_linear_device(curve, n, d_p, zs[:nz], d_q)[0]), reps_for(n))
            r = dict(n=n, nz=nz, **stats(ts))
            r["TB_per_s"] = round(96.0 * n * nz / (r["median_ms"] * 1e-3) / 1e12, 3)
            tv = timed(lambda: ok(zk.poly_div_linear_device(curve, n, d_p, zs[:nz])[0]), reps_for(n))
            r["values_only"] = stats(tv)
            out["division"].setdefault(curve, []).append(r)
            print(curve, "division", json.dumps(r), flush=True)
        # the two existing routes on the same polynomial
        lin = zk.DeviceBuffer(np.stack([zs[0], np.array(zk.gen_fr(curve, 23, 1)[0])]))  # any divisor of degree 1
        d_r = zk.DeviceBuffer.empty(32)
        for n in ROUTE_SIZES:
            reps = reps_for(n)
            new = stats(timed(lambda: ok(zk.poly_div_linear_device(curve, n, d_p, zs[:1], d_q)[0]), reps))
            long_div = stats(timed(lambda: ok(zk.poly_long_div_device(curve, n, d_p, 2, lin, n - 1, d_q, 1, d_r)), reps))
            chain_reps = reps if n <= 1 << 16 else 2  # one lane walks n dependent steps
            vanish = stats(timed(lambda: zk.div_by_vanishing_device(curve, n, d_p, 1, zs[0], n - 1, d_q, 1, d_r),
                                 chain_reps))
            r = {"n": n, "div_linear": new, "long_div_two_coefficient_divisor": long_div,
                 "div_by_vanishing_expo_1": vanish}
            out["routes"].setdefault(curve, []).append(r)
            print(curve, "routes", json.dumps(r), flush=True)
        lin.free()
        d_r.free()
        # openings: the whole call, and its two parts in calls of their own
        NP = zk.NLIMBS_P[curve]
        for n in OPEN_SIZES:
            reps = reps_for(n)
            d_srs = zk.DeviceBuffer(zk.gen_points(curve, 24, n))  # any affine rows time alike
            vals, proof = np.zeros((1, 4), np.uint64), np.zeros(3 * NP, np.uint64)
            whole = stats(timed(lambda: ok(lib.zkg_kzg_open_device(cid, n, d_p.ptr, d_srs.ptr, 1, zs.ctypes.data,
                                                                   vals.ctypes.data, proof.ctypes.data)), reps))
            div = stats(timed(lambda: ok(zk.poly_div_linear_device(curve, n, d_p, zs[:1], d_q)[0]), reps))
            msm = stats(timed(lambda: ok(lib.zkg_kzg_commit_device(cid, n - 1, d_q.ptr, d_srs.ptr, proof.ctypes.data)),
                              reps))
            r = {"n": n, "open": whole, "division": div, "msm": msm,
                 "division_share_of_parts": round(div["median_ms"] / (div["median_ms"] + msm["median_ms"]), 4)}
            out["openings"].setdefault(curve, []).append(r)
            print(curve, "opening", json.dumps(r), flush=True)
            d_srs.free()
        d_p.free()
        d_q.free()
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for curve in CURVES:  # the condition: faster than both existing routes at 2^20, one point
        r = [x for x in out["routes"][curve] if x["n"] == 1 << 20][0]
        new = r["div_linear"]["median_ms"]
        assert new < r["long_div_two_coefficient_divisor"]["median_ms"], (curve, r)
        assert new < r["div_by_vanishing_expo_1"]["median_ms"], (curve, r)
    print("condition met: div_linear at 2^20 is faster than both existing routes on both curves")


if __name__ == "__main__":
    main()
