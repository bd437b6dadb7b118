"""Batch point validation timing (GPU box):
    python tools/check_time.py [--quick] [--out profiles/check_time.json]
Device-resident zkg_g{1,2}_check_rows_device on affine rows of the order-r subgroup ([tau^i] g, made on the
device), n = 2^12, 2^16, 2^20, each (curve, group): the default membership chains (mode 0), the exact chain
[r]P (mode 1) and the curve pass alone (mode 2), count-only calls.  Every entry is synchronous, so a host clock
around the call times all of it.  One warm-up call per shape, then the median of the timed calls.
The yardstick is what a caller had to do before these entries existed: zkg_g{1,2}_scl_rows_device with n copies
of r as raw scalars at the same n (and then a scan of the output for infinity rows, not timed), in the same run."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zikkurat-algebra_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import zkalgebra as zk  # noqa: E402
from oracle.oracle import Reference  # noqa: E402
import golden_io  # noqa: E402


def med(call, reps):
    call()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2^12 and 2^16 only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_time.json"))
    args = ap.parse_args()
    zk.require_gpu()
    ref = Reference()
    sizes = (12, 16) if args.quick else (12, 16, 20)
    top = 1 << sizes[-1]
    out = {"what": "zkg_g{1,2}_check_rows_device, affine subgroup rows, count-only; host clock around the synchronous "
                   "call, one warm-up then the median of reps.  default / exact / curve_only: zkg_check_set_mode 0 / 1 "
                   "/ 2.  parent_route: zkg_g{1,2}_scl_rows_device with n copies of r as raw scalars, affine output, "
                   "the only way to ask the question before.  default_vs_parent = parent_route / default, "
                   "exact_vs_default = exact / default.",
           "groups": {}}
    try:
        for curve in zk.CURVES:
            NP = zk.NLIMBS_P[curve]
            tau = zk.gen_fr(curve, 0x7A0, 1)[0]
            r = zk.FR_ORDER[curve]
            rs = np.tile(np.array([(r >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64), (top, 1))
            d_r = zk.DeviceBuffer(rs)
            for group in (1, 2):
                w = 2 * group * NP
                d_pts = zk.DeviceBuffer.empty(top * w * 8)
                d_out = zk.DeviceBuffer.empty(top * w * 8)
                if group == 1:
                    rc = zk.srs_powers_device(curve, top, tau, zk.gen_points(curve, 11, 1)[0], d_pts, affine=True)
                    chk, scl = zk.g1_check_device, zk.scalar_mul_rows_device
                else:
                    rc = zk.g2_srs_powers_device(curve, top, tau, golden_io.g2_points(ref.lib, curve, 1)[0], d_pts,
                                                 affine=True)
                    chk, scl = zk.g2_check_device, zk.g2_scalar_mul_rows_device
                assert rc == 0
                row = {}
                for m in sizes:
                    n, reps = 1 << m, (3 if m >= 20 else 7)
                    e = {}
                    for name, mode in (("default", 0), ("exact", 1), ("curve_only", 2)):
                        zk.check_set_mode(mode)
                        bad = chk(curve, n, d_pts, None)
                        assert bad == (n if mode == 2 else 0), (curve, group, name, bad)
                        t = med(lambda: chk(curve, n, d_pts, None), reps)
                        e[name] = {"ms": t[0] * 1e3, "min_ms": t[1] * 1e3, "max_ms": t[2] * 1e3, "reps": reps}
                    zk.check_set_mode(0)
                    t = med(lambda: scl(curve, n, d_r, d_pts, d_out, std=True, affine=True), reps)
                    e["parent_route"] = {"ms": t[0] * 1e3, "min_ms": t[1] * 1e3, "max_ms": t[2] * 1e3, "reps": reps}
                    e["default_vs_parent"] = e["parent_route"]["ms"] / e["default"]["ms"]
                    e["exact_vs_default"] = e["exact"]["ms"] / e["default"]["ms"]
                    row[f"2^{m}"] = e
                    print(curve, f"G{group}", f"2^{m}", {k: round(v["ms"], 3) for k, v in e.items() if isinstance(v, dict)},
                          "parent/default", round(e["default_vs_parent"], 2), "exact/default",
                          round(e["exact_vs_default"], 2), flush=True)
                out["groups"][f"{curve}_G{group}"] = row
                d_pts.free()
                d_out.free()
            d_r.free()
    finally:
        zk.check_set_mode(-1)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
