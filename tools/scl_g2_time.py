"""Batch G2 scalar multiplication timing (GPU box):
    python tools/scl_g2_time.py [--quick] [--out profiles/scl_g2_time.json]
The G2 twin of tools/scl_time.py.  Device-resident zkg_g2_scl_fixed_device at n = 2^12, 2^16, 2^20 on both
curves, Montgomery scalars, projective output, through the table path (window in force) and through the
per-row kernel; the window sweep at 2^20; the table build (the whole table-path call at n = 1, per window);
and the row count at which the table path overtakes the per-row kernel.  Every entry is synchronous, so a
host clock around the call times all of it.  One warm-up call per shape (code objects, arena growth), then
the median of the timed calls.
Baselines, neither of them the code under test: the G2 group FFT's forward transform at 2^16 (m 2^(m-1)
scalar multiplications, timed as tools/g2fft_time.py times it), the only G2 per-row rate the library had
before, and the reference's <C>_G2_proj_scl_Fr_mont + _normalize on one host core (oracle/_ref)."""
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

SWEEP = (4, 6, 8, 9, 10, 11, 12, 13, 14, 16)


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
    ap.add_argument("--quick", action="store_true", help="2^12 and 2^16 only, a shorter sweep, the FFT at 2^12")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scl_g2_time.json"))
    args = ap.parse_args()
    zk.require_gpu()
    ref = Reference()
    sizes = (12, 16) if args.quick else (12, 16, 20)
    sweep = (6, 8, 11, 13) if args.quick else SWEEP
    top = sizes[-1]
    out = {"what": "zkg_g2_scl_fixed_device, Montgomery scalars, projective output; host clock around the "
                   "synchronous call, one warm-up then the median of reps. window_sweep: at the largest n. "
                   "table_build_ms[c]: the whole table-path call at n = 1 with window c (build launches + one "
                   "accumulate lane + one normalised row + synchronise). crossover_n: smallest power of two from "
                   "which the table path (window in force) stays no slower than the per-row kernel. "
                   "g2_fft_forward: the G2 group FFT's forward transform, m 2^(m-1) scalar multiplications. "
                   "cpu_reference: G2_proj_scl_Fr_mont + normalize on one host core. table_vs_fft: the table "
                   "path's rate at the largest n over the FFT's.",
           "curves": {}}
    try:
        for curve in zk.CURVES:
            NP = 2 * zk.NLIMBS_P[curve]
            fm = 12 if args.quick else 16
            aff = golden_io.g2_points(ref.lib, curve, 1 << fm)
            base = aff[0].copy()
            ks = zk.gen_fr(curve, 0x6C13, 1 << top)
            dk = zk.DeviceBuffer(ks)
            dt = zk.DeviceBuffer.empty((1 << top) * 3 * NP * 8)
            row = {"table_bytes": {str(c): zk.g2_scl_table_bytes(curve, c) for c in sweep}}

            def run(n, fixed_min, window, reps):
                zk.g2_scl_set_fixed_min(fixed_min)
                zk.g2_scl_set_window(window)
                t = med(lambda: zk.g2_scalar_mul_fixed_device(curve, n, dk, base, dt), reps)
                return {"ms": t[0] * 1e3, "min_ms": t[1] * 1e3, "max_ms": t[2] * 1e3, "reps": reps,
                        "path": zk.g2_scl_last_path(), "scalar_muls_per_s": n / t[0]}

            for m in sizes:
                n, reps = 1 << m, (3 if m >= 20 else 7)
                row[f"2^{m}"] = {"table": run(n, 0, 0, reps), "per_row": run(n, 1 << 30, 0, reps)}
                print(curve, f"2^{m}", "table", round(row[f"2^{m}"]["table"]["ms"], 3), "ms; per-row",
                      round(row[f"2^{m}"]["per_row"]["ms"], 3), "ms", flush=True)
            sw = {str(c): run(1 << top, 0, c, 3) for c in sweep}
            row["window_sweep"] = {"log_n": top, "windows": sw, "best_window": int(min(sw, key=lambda c: sw[c]["ms"]))}
            row["window_in_force"] = row[f"2^{sizes[0]}"]["table"]["path"]
            row["table_build_ms"] = {str(c): run(1, 0, c, 5)["ms"] for c in sweep}
            print(curve, "sweep", {c: round(v["ms"], 3) for c, v in sw.items()}, "build ms",
                  {c: round(v, 3) for c, v in row["table_build_ms"].items()}, flush=True)
            cross = {}
            for m in range(8, top + 1):
                cross[f"2^{m}"] = {"table_ms": run(1 << m, 0, 0, 5 if m < 20 else 3)["ms"],
                                   "per_row_ms": run(1 << m, 1 << 30, 0, 5 if m < 20 else 3)["ms"]}
            row["crossover"] = cross
            ahead = [cross[f"2^{m}"]["table_ms"] <= cross[f"2^{m}"]["per_row_ms"] for m in range(8, top + 1)]
            first = next((i for i in range(len(ahead)) if all(ahead[i:])), None)
            row["crossover_n"] = None if first is None else 1 << (8 + first)
            print(curve, "crossover", {k: (round(v["table_ms"], 3), round(v["per_row_ms"], 3)) for k, v in cross.items()},
                  "->", row["crossover_n"], flush=True)
            dk.free()
            dt.free()

            # baseline 1: the G2 group FFT's scalar multiplications per second, forward transform
            N = 1 << fm
            rows = np.zeros((N, 3 * NP), np.uint64)
            ref.arr(curve, "G2_proj_batch_from_affine", N, aff, rows)
            g = zk.get_fft_subgroup(curve, fm).gen_array()
            ds, dd = zk.DeviceBuffer(rows), zk.DeviceBuffer.empty(rows.nbytes)
            t = med(lambda: zk.g2_fft_device(curve, fm, g, ds, dd), 3)
            muls = fm * (N // 2)
            row["g2_fft_forward"] = {"log_n": fm, "ms": t[0] * 1e3, "min_ms": t[1] * 1e3, "max_ms": t[2] * 1e3,
                                     "scalar_muls": muls, "scalar_muls_per_s": muls / t[0]}
            ds.free()
            dd.free()
            row["table_vs_fft"] = row[f"2^{top}"]["table"]["scalar_muls_per_s"] / row["g2_fft_forward"]["scalar_muls_per_s"]
            row["per_row_vs_fft"] = (row[f"2^{top}"]["per_row"]["scalar_muls_per_s"] /
                                     row["g2_fft_forward"]["scalar_muls_per_s"])
            # baseline 2: the reference on one host core
            P = lambda a: a.ctypes.data_as(zk.U64P)  # noqa: E731
            pr, q, o = rows[0].copy(), np.zeros(3 * NP, np.uint64), np.zeros(3 * NP, np.uint64)
            cnt = 200
            t0 = time.perf_counter()
            for i in range(cnt):
                getattr(ref.lib, f"{curve}_G2_proj_scl_Fr_mont")(P(ks[i]), P(pr), P(q))
                getattr(ref.lib, f"{curve}_G2_proj_normalize")(P(q), P(o))
            sec = (time.perf_counter() - t0) / cnt
            row["cpu_reference"] = {"scalar_muls_per_s": 1 / sec, "cores": 1, "sample": cnt}
            print(curve, "G2 FFT", round(row["g2_fft_forward"]["scalar_muls_per_s"]), "scl/s; table path x",
                  round(row["table_vs_fft"], 2), "; per-row x", round(row["per_row_vs_fft"], 2), "; reference",
                  round(1 / sec), "scl/s", flush=True)
            out["curves"][curve] = row
    finally:
        zk.g2_scl_set_window(0)
        zk.g2_scl_set_fixed_min(-1)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
