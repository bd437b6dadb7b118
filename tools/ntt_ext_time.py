#!/usr/bin/env python3
"""Device-resident timing of the batched / coset NTT against what a caller had before it
(ZK_LIB_PATH selects the build, so the same script times a build without zkg_ntt_ext_device):

   python tools/ntt_ext_time.py [--reps 20] [--out FILE.json] [--curve bls12_381]

batch: one zkg_ntt_ext_device call of `batch` transforms ("ext", when the library has it) against
       `batch` zkg_ntt_device calls ("loop"), shapes (m, batch) = (10, 64) (12, 64) (14, 32) (16, 16) (20, 4)
coset: at 2^20 and 2^24, forward and inverse: the fused call ("ext"), the three-call sequence
       zkg_arr_powers_device, zkg_arr_op_device mul, zkg_ntt_device ("three"), and the plain
       zkg_ntt_device ("plain")
Every figure is the median over the repetitions (after two warm-up rounds) of the wall time of the
synchronous call(s) and of the zkg_timer_* kernel time (the NTT pass chains only: the powers and the
product of "three" are not on the library's timer, so its kernel time understates it).  The ext
results are checked against the loop / the three-call sequence before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zikkurat-algebra_amd"))
import numpy as np  # noqa: E402
import zkalgebra as zk  # noqa: E402

BATCH_SHAPES = [(10, 64), (12, 64), (14, 32), (16, 16), (20, 4)]
COSET_LOGS = [20, 24]


def measure(fn, reps):
    for _ in range(2):
        fn()
    wall, kern = [], []
    for _ in range(reps):
        zk.timer(enable=True, reset=True)
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(zk.timer(enable=False)[0])
    return {"wall_ms": round(statistics.median(wall), 4), "kernel_ms": round(statistics.median(kern), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--curve", default="bls12_381", choices=list(zk.CURVES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-coset", action="store_true")
    a = ap.parse_args()
    curve, reps = a.curve, max(20, a.reps)
    zk.require_gpu()
    lib = zk.load()
    have_ext = hasattr(lib, "zkg_ntt_ext_device")
    res = {"lib": zk.LIB_PATH, "curve": curve, "reps": reps, "have_ext": have_ext, "batch": {}, "coset": {}}
    row = zk.NLIMBS_R * 8

    for m, batch in BATCH_SHAPES:
        n = 1 << m
        g = zk.get_fft_subgroup(curve, m).gen_array()
        x = zk.gen_fr(curve, 0x7E57 + m, batch * n)
        d_x, d_y, d_z = zk.DeviceBuffer(x), zk.DeviceBuffer.empty(x.nbytes), zk.DeviceBuffer.empty(x.nbytes)

        def window(buf, b):  # transform b's rows of a batch buffer (never freed on its own)
            w = zk.DeviceBuffer.__new__(zk.DeviceBuffer)
            w.ptr, w.nbytes = buf.ptr + b * n * row, n * row
            return w

        pairs = [(window(d_x, b), window(d_y, b)) for b in range(batch)]

        def loop():
            for s, d in pairs:
                zk.ntt_device(curve, m, g, s, d)

        entry = {"loop": measure(loop, reps)}
        if have_ext:
            zk.ntt_ext_device(curve, m, g, d_x, d_z, batch=batch)
            loop()
            assert np.array_equal(d_z.to_host(x), d_y.to_host(x)), (m, batch)
            entry["ext"] = measure(lambda: zk.ntt_ext_device(curve, m, g, d_x, d_z, batch=batch), reps)
            entry["ext_over_loop_wall"] = round(entry["ext"]["wall_ms"] / entry["loop"]["wall_ms"], 4)
        res["batch"][f"{m}x{batch}"] = entry
        for d in (d_x, d_y, d_z):
            d.free()

    for m in ([] if a.skip_coset else COSET_LOGS):
        n = 1 << m
        g = zk.get_fft_subgroup(curve, m).gen_array()
        one = zk.get_fft_subgroup(curve, 0).gen_array()
        shift = zk.gen_fr(curve, 0xC05E7, 1)[0]
        sinv = zk.arr_inv(curve, shift.reshape(1, 4))[0]
        x = zk.gen_fr(curve, 0xC05E8, n)
        d_x, d_p, d_t, d_y, d_z = (zk.DeviceBuffer(x), zk.DeviceBuffer.empty(x.nbytes), zk.DeviceBuffer.empty(x.nbytes),
                                   zk.DeviceBuffer.empty(x.nbytes), zk.DeviceBuffer.empty(x.nbytes))

        def three(inverse):
            k = np.ascontiguousarray(sinv if inverse else shift)
            lib.zkg_arr_powers_device(zk.CURVE_ID[curve], n, zk._p(one), zk._p(k), d_p.ptr)
            if inverse:
                zk.ntt_device(curve, m, g, d_x, d_t, inverse=True)
                zk.arr_op_device(curve, "mul", n, d_t, d_p, d_tgt=d_y)
            else:
                zk.arr_op_device(curve, "mul", n, d_x, d_p, d_tgt=d_t)
                zk.ntt_device(curve, m, g, d_t, d_y)

        for inverse in (False, True):
            entry = {"three": measure(lambda: three(inverse), reps),
                     "plain": measure(lambda: zk.ntt_device(curve, m, g, d_x, d_t, inverse=inverse), reps)}
            if have_ext:
                three(inverse)
                zk.ntt_ext_device(curve, m, g, d_x, d_z, inverse=inverse, shift=shift)
                assert np.array_equal(d_z.to_host(x), d_y.to_host(x)), (m, inverse)
                entry["ext"] = measure(lambda: zk.ntt_ext_device(curve, m, g, d_x, d_z, inverse=inverse, shift=shift),
                                       reps)
            res["coset"][f"2^{m} {'inverse' if inverse else 'forward'}"] = entry
        for d in (d_x, d_p, d_t, d_y, d_z):
            d.free()

    txt = json.dumps(res, indent=1)
    print(txt, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
