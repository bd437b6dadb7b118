"""Batch pairing timing (GPU box):
    python tools/pairing_time.py [--quick] [--out profiles/pairing_time.json]
Device-resident zkg_pairing_rows_device at 2^8, 2^12 and 2^16 rows on both curves (rows tiled from
tests/golden/pairing_<curve>.npz), zkg_pairing_final_expo_device on as many rows (the final exponentiation's
kernel alone; the Miller share is the difference, both run the same interpreter kernel on the same lanes), and
zkg_pairing_product_device at 2 and 2^12 rows.  Every entry is synchronous, so a host clock around the call
times all of it: one warm-up call per shape (code object, arena growth), then the median of the timed calls.
The reference's rate (<C>_pairing_affine on one host core) is NOT measured here: the GPU host has no
reference library.  It is passed in with --reference-ms, measured on the build machine where the fixture was
made (tools/make_golden.py pairing prints it), and the file records that."""
import argparse
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


def med(call, reps):
    call()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t)
    return {"ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3, "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2^8 and 2^12 only")
    ap.add_argument("--reference-ms", default="", help="bn128=MS,bls12_381=MS: one <C>_pairing_affine on one host core")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairing_time.json"))
    args = ap.parse_args()
    zk.require_gpu()
    ref_ms = dict(kv.split("=") for kv in args.reference_ms.split(",") if kv)
    sizes = (8, 12) if args.quick else (8, 12, 16)
    out = {"what": "zkg_pairing_rows_device / zkg_pairing_final_expo_device / zkg_pairing_product_device; host clock "
                   "around the synchronous call, one warm-up then the median of reps. miller_ms = rows ms - "
                   "final_expo ms at the same row count. cpu_reference: <C>_pairing_affine of the reference on one "
                   "host core of the BUILD machine (not the GPU host), from the fixture's generation run.",
           "curves": {}}
    for curve in zk.CURVES:
        g = np.load(os.path.join(ROOT, "tests", "golden", f"pairing_{curve}.npz"))
        keep = [i for i in range(g["P"].shape[0]) if i not in set(int(x) for x in g["infinity"])]
        top = 1 << sizes[-1]
        idx = np.array(keep)[np.arange(top) % len(keep)]
        dP, dQ = zk.DeviceBuffer(g["P"][idx].copy()), zk.DeviceBuffer(g["Q"][idx].copy())
        dT = zk.DeviceBuffer.empty(top * g["pairing"].shape[1] * 8)
        dF = zk.DeviceBuffer(g["pairing"][idx].copy())
        row = {}
        for m in sizes:
            n, reps = 1 << m, (3 if m >= 16 else 5)
            r = med(lambda: zk.pairing_device(curve, n, dP, dQ, dT), reps)
            f = med(lambda: zk.final_expo_device(curve, n, dF, dT), reps)
            r["pairings_per_s"] = n / (r["ms"] / 1e3)
            row[f"2^{m}"] = {"pairing_rows": r, "final_expo": f, "miller_ms": r["ms"] - f["ms"],
                             "final_expo_share": f["ms"] / r["ms"]}
            print(curve, f"2^{m}", "rows", round(r["ms"], 2), "ms; final expo", round(f["ms"], 2), "ms;",
                  round(r["pairings_per_s"]), "pairings/s", flush=True)
        for n in (2, 1 << 12):
            row[f"product_{n}"] = med(lambda: zk.pairing_product_device(curve, n, dP, dQ, dT), 5)
            print(curve, "product", n, round(row[f"product_{n}"]["ms"], 2), "ms", flush=True)
        if curve in ref_ms:
            row["cpu_reference"] = {"ms_per_pairing": float(ref_ms[curve]), "pairings_per_s": 1e3 / float(ref_ms[curve]),
                                    "cores": 1, "measured_on": "build machine, not the GPU host"}
            row["vs_reference_at_2^12"] = row["2^12"]["pairing_rows"]["pairings_per_s"] / row["cpu_reference"]["pairings_per_s"]
        for b in (dP, dQ, dT, dF):
            b.free()
        out["curves"][curve] = row
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
