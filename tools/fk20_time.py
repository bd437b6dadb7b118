#!/usr/bin/env python3
"""All KZG openings of a domain at once (zk_fk20.hip) against the route the library had (GPU box):
    python tools/fk20_time.py [--logs 10,12] [--baseline-max-log 12] [--out FILE]   -> profiles/fk20_time.json
Device-resident buffers; every entry is synchronous, so a host clock around the call times all of it (the
conventions of tools/lindiv_time.py): one warm-up call per shape, then REPS timed calls, median / min / max.
Per curve and n = 2^log, in the same run:
  open_all_l1   (a) zkg_kzg_open_all_device with l = 1, the table already built
  table_l1      (b) zkg_kzg_open_all_table_device alone (l = 1: one group FFT of size 2n and the affine conversion)
  open_all_l16, open_all_l64   (c) the coset proofs, table built
  open_many     (d) the baseline: zkg_kzg_open_device over all n roots of unity, as it stands (up to
                --baseline-max-log: it is n divisions and n MSMs)
  parts_l1      (e) the steps of (a) in calls of their own: zkg_g1_scl_rows_sum_device (host clock, and the
                kernel alone from the library's timer) beside the two group FFTs (inverse 2n, forward n)
The one condition, asserted at the end: at n = 2^12, (a) is below (d) on both curves."""
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


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


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
    logs = [int(x) for x in arg("--logs", "10,12").split(",")]
    base_max = int(arg("--baseline-max-log", "12"))
    path = arg("--out", os.path.join(ROOT, "profiles", "fk20_time.json"))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    out = {"logs": logs, "results": {}}
    for curve in CURVES:
        cid, NP = zk.CURVE_ID[curve], zk.NLIMBS_P[curve]
        for m in logs:
            n = 1 << m
            reps = 7 if m <= 10 else 5 if m <= 12 else 3
            d_srs = zk.DeviceBuffer(zk.gen_points(curve, 31, n))  # any subgroup rows time alike
            d_poly = zk.DeviceBuffer(zk.gen_fr(curve, 32, n))
            d_out = zk.DeviceBuffer.empty(2 * n * 3 * NP * 8)
            d_tab = zk.DeviceBuffer.empty(lib.zkg_kzg_open_all_table_bytes(cid, m, 0))
            r = {"n": n}
            r["table_l1"] = stats(timed(lambda: ok(lib.zkg_kzg_open_all_table_device(cid, m, 0, d_srs.ptr, d_tab.ptr)),
                                        reps))
            r["open_all_l1"] = stats(timed(lambda: ok(lib.zkg_kzg_open_all_device(cid, m, 0, n, d_poly.ptr, d_tab.ptr, 0,
                                                                                  d_out.ptr)), reps))
            # (e) the steps of (a) on their own; the scalars and bases are any rows of the right shape
            d_k = zk.DeviceBuffer(zk.gen_fr(curve, 33, 2 * n))
            zk.timer(enable=True, reset=True)
            host = timed(lambda: ok(zk.scalar_mul_rows_sum_device(curve, 2 * n, 1, d_k, d_tab, d_out)), reps)
            kernel_ms, calls = zk.timer()
            zk.timer(enable=False, reset=True)
            gen2, gen1 = zk.get_fft_subgroup(curve, m + 1).gen_array(), zk.get_fft_subgroup(curve, m).gen_array()
            d_y = zk.DeviceBuffer.empty(2 * n * 3 * NP * 8)
            ifft = stats(timed(lambda: zk.g1_fft_device(curve, m + 1, gen2, d_out, d_y, inverse=True), reps))
            fft = stats(timed(lambda: zk.g1_fft_device(curve, m, gen1, d_y, d_out), reps))
            rs = stats(host)
            parts = rs["median_ms"] + ifft["median_ms"] + fft["median_ms"]
            r["parts_l1"] = {"rows_sum": rs, "rows_sum_kernel_ms": round(kernel_ms / max(1, calls), 4),
                             "group_ifft_2n": ifft, "group_fft_n": fft,
                             "rows_sum_share_of_parts": round(rs["median_ms"] / parts, 4)}
            d_k.free()
            d_y.free()
            for c in (4, 6):
                if c > m - 1:
                    continue
                ok(lib.zkg_kzg_open_all_table_device(cid, m, c, d_srs.ptr, d_tab.ptr))
                r[f"open_all_l{1 << c}"] = stats(timed(lambda: ok(lib.zkg_kzg_open_all_device(
                    cid, m, c, n, d_poly.ptr, d_tab.ptr, 0, d_out.ptr)), reps))
            if m <= base_max:
                one = np.array(zk._fr_mont(curve, 1))
                zs = zk.arr_powers(curve, one, zk.get_fft_subgroup(curve, m).gen_array(), n)
                vals, proofs = np.zeros((n, 4), np.uint64), np.zeros((n, 3 * NP), np.uint64)
                r["open_many"] = stats(timed(lambda: ok(lib.zkg_kzg_open_device(
                    cid, n, d_poly.ptr, d_srs.ptr, n, zs.ctypes.data, vals.ctypes.data, proofs.ctypes.data)),
                    1 if m >= 12 else 3))
                r["open_many_over_open_all_l1"] = round(r["open_many"]["median_ms"] / r["open_all_l1"]["median_ms"], 2)
            out["results"].setdefault(curve, []).append(r)
            print(curve, json.dumps(r), flush=True)
            for b in (d_srs, d_poly, d_out, d_tab):
                b.free()
            with open(path, "w") as f:  # after every shape: a partial run leaves what it measured
                json.dump(out, f, indent=1)
                f.write("\n")
    for curve in CURVES:
        for r in out["results"][curve]:
            if r["n"] == 1 << 12 and "open_many" in r:
                assert r["open_all_l1"]["median_ms"] < r["open_many"]["median_ms"], (curve, r)
                print(curve, "condition met at 2^12: open_all", r["open_all_l1"]["median_ms"], "ms < open_many",
                      r["open_many"]["median_ms"], "ms")


if __name__ == "__main__":
    main()
