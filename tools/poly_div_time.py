#!/usr/bin/env python3
"""Polynomial division timing (GPU box):
    python tools/poly_div_time.py            -> profiles/poly_div_time.json
    python tools/poly_div_time.py --sweep    -> profiles/poly_div_base_sweep.txt
Device-resident zkg_poly_long_div_device on both curves at dividend / divisor lengths 2^12 / 2^11,
2^16 / 2^15, 2^20 / 2^19, 2^20 / 2 (a linear factor) and 2^20 / (2^20 - 64) (a short quotient).  The
entry is synchronous, so a host clock around the call times the whole division.  One warm-up call
per shape (code objects, arena, twiddle tables), then REPS timed calls: median, min, max.  Beside
each shape, in the same run: zkg_poly_mul_device of two factors of the quotient's length, and the
per-phase split (series inverse, quotient, remainder) by the HIP events the library records while
zkg_poly_div_profile is on (a separate set of calls, medians).  Last, the reference's own long_div
(oracle/_ref, one host core) at 2^14 / 2^13, once, with the library's host entry beside it.
--sweep: whole-division time at quotient lengths m = 2^8, 2^12, 2^16 (dividend 2m - 1, divisor m)
against the base kernel's size, alternating the sizes inside every repetition."""
import ctypes
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
SHAPES = [(1 << 12, 1 << 11), (1 << 16, 1 << 15), (1 << 20, 1 << 19), (1 << 20, 2), (1 << 20, (1 << 20) - 64)]
SWEEP_M = (1 << 8, 1 << 12, 1 << 16)
SWEEP_BASES = (1, 2, 4, 8, 16, 32, 64, 128, 256)


def reps_for(n1):
    return 30 if n1 <= 1 << 12 else 15 if n1 <= 1 << 16 else 7


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


class Division:
    """device buffers of one shape: random operands (the leading coefficients are nonzero)"""

    def __init__(self, curve, n1, n2):
        self.curve, self.n1, self.n2 = curve, n1, n2
        self.m = n1 - n2 + 1
        p, d = zk.gen_fr(curve, 11, n1), zk.gen_fr(curve, 12, n2)
        assert p[-1].any() and d[-1].any()
        self.bufs = [zk.DeviceBuffer(p), zk.DeviceBuffer(d), zk.DeviceBuffer.empty(self.m * 32),
                     zk.DeviceBuffer.empty(max(1, n2 - 1) * 32)]

    def __call__(self):
        dp, dd, dq, dr = self.bufs
        rc = zk.poly_long_div_device(self.curve, self.n1, dp, self.n2, dd, self.m, dq, self.n2 - 1, dr)
        assert rc == 0

    def free(self):
        for b in self.bufs:
            b.free()


def sweep(path):
    lines = ["# whole device-resident division (zkg_poly_long_div_device, quotient and remainder), median ms of 9",
             "# calls per cell; dividend 2m - 1 coefficients, divisor m, quotient m; the base sizes alternate",
             "# inside every repetition.  steps = Newton steps of the plan."]
    lib = zk.load()
    for curve in CURVES:
        for m in SWEEP_M:
            div = Division(curve, 2 * m - 1, m)
            ts = {b: [] for b in SWEEP_BASES}
            steps = {}
            for b in SWEEP_BASES:  # warm-up of every size
                zk.poly_set_div_base_max(b)
                div()
                steps[b] = zk.poly_last_div_steps()
            for _ in range(9):
                for b in SWEEP_BASES:
                    zk.poly_set_div_base_max(b)
                    t = time.perf_counter()
                    div()
                    ts[b].append((time.perf_counter() - t) * 1e3)
            div.free()
            for b in SWEEP_BASES:
                lines.append(f"{curve:10s} m=2^{m.bit_length() - 1:<2d} base={b:<3d} steps={steps[b]:<2d} "
                             f"median {statistics.median(ts[b]):8.4f} ms  min {min(ts[b]):8.4f}  max {max(ts[b]):8.4f}")
                print(lines[-1], flush=True)
    zk.poly_set_div_base_max(-1)
    lines.append(f"# default in force: {lib.zkg_poly_div_base_max()}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    zk.require_gpu()
    lib = zk.load()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    if "--sweep" in sys.argv:
        return sweep(os.path.join(ROOT, "profiles", "poly_div_base_sweep.txt"))
    out = {"base": lib.zkg_poly_div_base_max(), "shapes": {}, "reference": {}}
    for curve in CURVES:
        for n1, n2 in SHAPES:
            div = Division(curve, n1, n2)
            reps = reps_for(n1)
            r = {"n1": n1, "n2": n2, "quotient_len": div.m, "division": stats(timed(div, reps))}
            r["newton_steps"] = zk.poly_last_div_steps()
            r["plan"] = zk.poly_div_plan(div.m)
            # the product of two factors of the quotient's length, beside it
            a, b = zk.DeviceBuffer(zk.gen_fr(curve, 13, div.m)), zk.DeviceBuffer(zk.gen_fr(curve, 14, div.m))
            t = zk.DeviceBuffer.empty((2 * div.m - 1) * 32)
            r["product"] = stats(timed(lambda: zk.poly_mul_device(curve, div.m, a, div.m, b, t), reps))
            r["product_path"] = zk.poly_last_mul_path()
            for x in (a, b, t):
                x.free()
            r["ratio_to_product"] = round(r["division"]["median_ms"] / r["product"]["median_ms"], 2)
            # phases by HIP events, in calls of their own
            lib.zkg_poly_div_profile(1)
            ph = []
            for _ in range(reps):
                div()
                ms = (ctypes.c_double * 3)()
                lib.zkg_poly_last_div_phase_ms(ms)
                ph.append(list(ms))
            lib.zkg_poly_div_profile(0)
            r["phases_ms"] = {k: round(statistics.median(x[i] for x in ph), 4)
                              for i, k in enumerate(("series_inverse", "quotient", "remainder"))}
            div.free()
            out["shapes"].setdefault(curve, []).append(r)
            print(curve, json.dumps(r), flush=True)
    from oracle.oracle import Reference
    if Reference.available():
        ref = Reference()
        n1, n2 = 1 << 14, 1 << 13
        for curve in CURVES:
            p, d = zk.gen_fr(curve, 11, n1), zk.gen_fr(curve, 12, n2)
            wq, wr = np.zeros((n1 - n2 + 1, 4), np.uint64), np.zeros((n2 - 1, 4), np.uint64)
            t = time.perf_counter()
            ref.arr(curve, "poly_mont_long_div", n1, p, n2, d, wq.shape[0], wq, wr.shape[0], wr)
            t_ref = time.perf_counter() - t
            zk.poly_long_div(curve, p, d)
            t = time.perf_counter()
            q, r = zk.poly_long_div(curve, p, d)
            t_gpu = time.perf_counter() - t
            out["reference"][curve] = {"n1": n1, "n2": n2, "reference_one_core_s": round(t_ref, 3),
                                       "library_host_entry_ms": round(t_gpu * 1e3, 3),
                                       "outputs_equal": bool(np.array_equal(q[:wq.shape[0]], wq) and np.array_equal(r, wr))}
            print(curve, json.dumps(out["reference"][curve]), flush=True)
    else:
        out["reference"] = "unmeasured: oracle/_ref/libzkref.so not built"
    with open(os.path.join(ROOT, "profiles", "poly_div_time.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
