"""Batch G1 scalar multiplication timing (GPU box):
    python tools/scl_time.py [--quick] [--out profiles/scl_time.json]
Device-resident zkg_g1_scl_fixed_device at n = 2^12, 2^16, 2^20 on both curves, Montgomery scalars, projective
output, through the table path (default window) and through the per-row kernel; the table build (the whole
table-path call at n = 1: the five build launches, then one accumulate lane, one normalised row and the
stream's synchronise, which no host clock can take out); the window sweep at each n; and the row count at which the table path overtakes
the per-row kernel.  Every entry is synchronous, so a host clock around the call times all of it.  One
warm-up call per shape (code objects, arena growth), then the median of REPS calls.
Baselines, neither of them the code under test: the reference's <C>_G1_proj_scl_Fr_mont + _normalize on one
host core (oracle/_ref), and the group FFT's scalar multiplications per second as tools/bench_ext.py counts
them (forward transform at 2^16: N / 2 * m multiplications), the only per-row rate the library had before."""
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

SWEEP = (4, 6, 8, 10, 11, 12, 13, 14, 16)


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
    ap.add_argument("--quick", action="store_true", help="2^12 and 2^16 only, a shorter sweep")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scl_time.json"))
    args = ap.parse_args()
    zk.require_gpu()
    sizes = (12, 16) if args.quick else (12, 16, 20)
    sweep = (6, 8, 11, 13) if args.quick else SWEEP
    out = {"what": "zkg_g1_scl_fixed_device, Montgomery scalars, projective output; host clock around the "
                   "synchronous call, one warm-up then the median of reps. table_build_ms[c]: the whole table-path "
                   "call at n = 1 with window c (build launches + one accumulate lane + one normalised row + "
                   "synchronise). crossover_n: smallest power of two from which the table path (default window) "
                   "is no slower than the per-row kernel. cpu_reference: scl_Fr_mont + normalize on one host "
                   "core (null: oracle/_ref not built). group_fft_forward: scalar multiplications per second "
                   "as tools/bench_ext.py counts them.",
           "curves": {}}
    try:
        for curve in zk.CURVES:
            NP = zk.NLIMBS_P[curve]
            base = zk.gen_points(curve, 0x5C10, 1)[0]
            ks = zk.gen_fr(curve, 0x5C12, 1 << sizes[-1])
            dk = zk.DeviceBuffer(ks)
            dt = zk.DeviceBuffer.empty((1 << sizes[-1]) * 3 * NP * 8)
            row = {"table_bytes": {str(c): zk.scl_table_bytes(curve, c) for c in sweep}}

            def run(n, fixed_min, window, reps):
                zk.scl_set_fixed_min(fixed_min)
                zk.scl_set_window(window)
                t = med(lambda: zk.scalar_mul_fixed_device(curve, n, dk, base, dt), reps)
                return {"ms": t[0] * 1e3, "min_ms": t[1] * 1e3, "max_ms": t[2] * 1e3, "reps": reps,
                        "path": zk.scl_last_path(), "scalar_muls_per_s": n / t[0]}

            for m in sizes:
                n, reps = 1 << m, (3 if m >= 20 else 7)
                r = {"table": run(n, 0, 0, reps), "per_row": run(n, 1 << 30, 0, reps),
                     "window_sweep": {str(c): run(n, 0, c, 3 if m >= 20 else 5) for c in sweep}}
                r["best_window"] = int(min(r["window_sweep"], key=lambda c: r["window_sweep"][c]["ms"]))
                row[f"2^{m}"] = r
                print(curve, f"2^{m}", "table", round(r["table"]["ms"], 3), "ms; per-row", round(r["per_row"]["ms"], 3),
                      "ms; sweep", {c: round(v["ms"], 3) for c, v in r["window_sweep"].items()}, flush=True)
            row["default_window"] = row[f"2^{sizes[0]}"]["table"]["path"]
            row["table_build_ms"] = {str(c): run(1, 0, c, 5)["ms"] for c in sweep}
            # crossover: the smallest n (powers of two) at which the table path is no slower than the per-row kernel
            cross = {}
            for m in range(6, 19):
                cross[f"2^{m}"] = {"table_ms": run(1 << m, 0, 0, 5)["ms"], "per_row_ms": run(1 << m, 1 << 30, 0, 5)["ms"]}
            row["crossover"] = cross
            row["crossover_n"] = next((1 << m for m in range(6, 19)
                                       if cross[f"2^{m}"]["table_ms"] <= cross[f"2^{m}"]["per_row_ms"]), None)
            print(curve, "table build ms", {c: round(v, 3) for c, v in row["table_build_ms"].items()},
                  "crossover n", row["crossover_n"], flush=True)
            dk.free()
            dt.free()

            # baseline 1: the group FFT's scalar multiplications per second (bench_ext.py's count), forward 2^16
            fm = 16 if not args.quick else 12
            N = 1 << fm
            proj = zk.batch_from_affine(curve, zk.gen_points(curve, 7, N))
            g = zk.get_fft_subgroup(curve, fm).gen_array()
            ds, dd = zk.DeviceBuffer(proj), zk.DeviceBuffer.empty(proj.nbytes)
            t = med(lambda: zk.g1_fft_device(curve, fm, g, ds, dd), 3)
            row["group_fft_forward"] = {"log_n": fm, "ms": t[0] * 1e3, "scalar_muls": N // 2 * fm,
                                        "scalar_muls_per_s": N // 2 * fm / t[0], "glv": bool(zk.g1_fft_last_glv())}
            ds.free()
            dd.free()
            # baseline 2: the reference on one host core
            if Reference.available():
                lib = Reference().lib
                P = lambda a: a.ctypes.data_as(zk.U64P)  # noqa: E731
                pr, q, o = proj[0].copy(), np.zeros(3 * NP, np.uint64), np.zeros(3 * NP, np.uint64)
                cnt = 200
                t0 = time.perf_counter()
                for i in range(cnt):
                    getattr(lib, f"{curve}_G1_proj_scl_Fr_mont")(P(ks[i]), P(pr), P(q))
                    getattr(lib, f"{curve}_G1_proj_normalize")(P(q), P(o))
                sec = (time.perf_counter() - t0) / cnt
                row["cpu_reference"] = {"scalar_muls_per_s": 1 / sec, "cores": 1, "sample": cnt}
            else:
                row["cpu_reference"] = None
                print("oracle/_ref/libzkref.so is not built: no host-core baseline", flush=True)
            print(curve, "group FFT", round(row["group_fft_forward"]["scalar_muls_per_s"]), "scl/s; reference",
                  round((row["cpu_reference"] or {}).get("scalar_muls_per_s", 0)), "scl/s", flush=True)
            out["curves"][curve] = row
    finally:
        zk.scl_set_window(0)
        zk.scl_set_fixed_min(-1)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
