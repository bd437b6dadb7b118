"""G2 group FFT timing (GPU box):
    python tools/g2fft_time.py [curve ...]
Device-resident zkg_g2_fft_device at 2^12 and 2^16, forward and inverse, on DISTINCT reference-generated
G2 points (golden_io.g2_points, Z = one rows).  The entry is synchronous (it returns after the stream's
synchronise), so a host clock around the call times the whole transform: load, m levels, normalisation.
One warm-up call per shape, then REPS timed calls; prints the median, the spread and a digest of the output.
Then the reference's own <C>_G2_proj_fft_forward / _inverse (oracle/_ref, one host core) at 2^8, once each,
with the library's host entry on the same rows beside it (outputs compared)."""
import hashlib
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

REPS = {12: 7, 16: 3}
NP = {"bn128": 4, "bls12_381": 6}


def main():
    zk.require_gpu()
    ref = Reference()
    for curve in sys.argv[1:] or ("bn128", "bls12_381"):
        aff = golden_io.g2_points(ref.lib, curve, 1 << 16)
        rows = np.zeros((1 << 16, 6 * NP[curve]), np.uint64)
        ref.arr(curve, "G2_proj_batch_from_affine", 1 << 16, aff, rows)
        for m in (12, 16):
            n = 1 << m
            src = np.ascontiguousarray(rows[:n])
            gen = zk.get_fft_subgroup(curve, m).gen_array()
            d_src, d_tgt = zk.DeviceBuffer(src), zk.DeviceBuffer(src)
            for inverse in (False, True):
                call = lambda: zk.g2_fft_device(curve, m, gen, d_src, d_tgt, inverse=inverse)
                call()  # warm-up: code objects, arena
                ts = []
                for _ in range(REPS[m]):
                    t = time.perf_counter()
                    call()
                    ts.append((time.perf_counter() - t) * 1e3)
                out = d_tgt.to_host(src)
                print(f"{curve} G2 fft 2^{m} {'inverse' if inverse else 'forward'}: median {statistics.median(ts):9.3f} ms"
                      f"  (min {min(ts):.3f}, max {max(ts):.3f}, {len(ts)} calls)"
                      f"  output {hashlib.sha256(out.tobytes()).hexdigest()[:16]}", flush=True)
            d_src.free()
            d_tgt.free()
        m = 8
        src = np.ascontiguousarray(rows[:1 << m])
        sg = zk.get_fft_subgroup(curve, m)
        for inverse in (False, True):
            name = "G2_proj_fft_inverse" if inverse else "G2_proj_fft_forward"
            want = np.zeros_like(src)
            t = time.perf_counter()
            ref.arr(curve, name, m, sg.gen_array(), src, want)
            t_ref = time.perf_counter() - t
            f = zk.g2_inverse_fft if inverse else zk.g2_forward_fft
            f(sg, src)
            t = time.perf_counter()
            got = f(sg, src)
            t_gpu = time.perf_counter() - t
            print(f"{curve} G2 fft 2^{m} {'inverse' if inverse else 'forward'}: reference (host, one core) {t_ref:7.3f} s,"
                  f" library host entry {t_gpu * 1e3:8.3f} ms, outputs equal: {bool(np.array_equal(got, want))}", flush=True)


if __name__ == "__main__":
    main()
