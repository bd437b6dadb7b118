"""Child process of tests/test_gpu_env_switches.py (not collected by pytest).

The ZK_* switches are read once per process, so the parent starts this script in a fresh
interpreter with the switches in its environment:

    python env_switch_child.py <inputs.npz> <outputs.npz>

inputs.npz holds the arrays and one JSON job list (key "jobs", UTF-8 bytes): each job names a
call of zkalgebra, its curve and the keys of its array arguments.  The script runs the jobs in
order and writes every result under the job's id (suffixes for calls with several results), plus
the observables the library exposes (g1_fft_plan, g1_fft_last_glv, msm_last_groups).  It computes
no reference and compares nothing: the parent does, against the oracle / the reference.
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "zikkurat-algebra_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import zkalgebra as zk  # noqa: E402

U64P = ctypes.POINTER(ctypes.c_uint64)


def _ptr(a):
    return a.ctypes.data_as(U64P)


def _arr(job, A, out):
    """one Fr vector call; the op names are the oracle's (oracle.Oracle.ARR_OP) plus the calls of
    test_gpu_arr.test_elementwise that are not a single op (dot, powers, append)"""
    c, op = job["curve"], job["op"]
    a, b, cc = (A[job[k]] if k in job else None for k in ("a", "b", "c"))
    kA, kB = (A[job[k]] if k in job else None for k in ("kA", "kB"))
    unary = {"neg": zk.arr_neg, "sqr": zk.arr_sqr, "to_std": zk.arr_to_std, "from_std": zk.arr_from_std,
             "inv": zk.arr_inv}
    binary = {"add": zk.arr_add, "sub": zk.arr_sub, "mul": zk.arr_mul, "div": zk.arr_div}
    if op in unary:
        r = unary[op](c, a)
    elif op in binary:
        r = binary[op](c, a, b)
    elif op == "mul_add":
        r = zk.arr_mul_add(c, a, b, cc)
    elif op == "mul_sub":
        r = zk.arr_mul_sub(c, a, b, cc)
    elif op == "scale":
        r = zk.arr_scale(c, kA, a)
    elif op == "Ax_plus_y":
        r = zk.arr_lin_comb1(c, (kA, a), b)
    elif op == "Ax_plus_By":
        r = zk.arr_lin_comb2(c, (kA, a), (kB, b))
    elif op == "dot":
        r = zk.arr_dot_prod(c, a, b)
    elif op == "powers":
        r = zk.arr_powers(c, kA, kB, job["n"])
    elif op == "append":  # two ARR_COPY launches
        r = zk.arr_append(c, a, b)
    elif op == "sub_rev":  # ARR_SUB_REV has no host mirror: the reference symbol itself (t = b - t)
        r = a.copy()
        getattr(zk.load(), f"{c}_arr_mont_sub_inplace_reverse")(r.shape[0], _ptr(r), _ptr(b))
    elif op == "set_const":
        r = np.zeros((job["n"], 4), dtype=np.uint64)
        getattr(zk.load(), f"{c}_arr_mont_set_const")(job["n"], _ptr(np.ascontiguousarray(kA)), _ptr(r))
    else:
        raise KeyError(op)
    out[job["id"]] = r


def _vanish(job, A, out):
    c, poly, n, eta = job["curve"], A[job["poly"]], job["n"], A[job["eta"]]
    q, r = zk.div_by_vanishing(c, poly, n, eta)
    out[job["id"] + "__q"], out[job["id"] + "__r"] = q, r
    q2 = zk.quot_by_vanishing(c, poly, n, eta)
    out[job["id"] + "__ok"] = np.array([q2 is not None])
    if q2 is not None:
        out[job["id"] + "__quot"] = q2


def _to_affine(job, A, out):
    out[job["id"]] = zk.batch_to_affine(job["curve"], A[job["pts"]], coords=job["coords"])


def _fft(job, A, out):
    c, m = job["curve"], job["m"]
    sg = zk.get_fft_subgroup(c, m)
    if "gen" in job:  # another generator of the same subgroup
        sg = zk.FFTSubgroup(c, tuple(int(v) for v in A[job["gen"]]), m)
    f = zk.inverse_fft if job["inverse"] else zk.forward_fft
    out[job["id"]] = f(sg, A[job["pts"]], coords=job["coords"])
    out[job["id"] + "__glv"] = np.array([zk.g1_fft_last_glv()])
    out[job["id"] + "__plan"] = np.array(zk.g1_fft_plan(c, m), dtype=np.int64)


def _g2_to_affine(job, A, out):
    out[job["id"]] = zk.g2_batch_to_affine(job["curve"], A[job["pts"]])


def _g2_fft(job, A, out):
    sg = zk.get_fft_subgroup(job["curve"], job["m"])
    f = zk.g2_inverse_fft if job["inverse"] else zk.g2_forward_fft
    out[job["id"]] = f(sg, A[job["pts"]])


def _msm_affine(job, A, out):
    out[job["id"]] = zk.msm_affine(job["curve"], A[job["sc"]], A[job["pts"]], std=job["std"])


def _msm_variable(job, A, out):
    out[job["id"]] = zk.msm_variable(job["curve"], A[job["sc"]], A[job["pts"]], job["window"])


def _msm_device(job, A, out):
    sc, pts = A[job["sc"]], A[job["pts"]]
    ds, dp = zk.DeviceBuffer(sc), zk.DeviceBuffer(pts)
    try:
        out[job["id"]] = zk.msm_device(job["curve"], sc.shape[0], ds, dp, mont=job["mont"], window=job["window"])
        out[job["id"] + "__groups"] = np.array([zk.msm_last_groups()])
    finally:
        ds.free()
        dp.free()


def _g2_msm(job, A, out):
    out[job["id"]] = zk.g2_msm(job["curve"], A[job["sc"]], A[job["pts"]], std=job["std"], affine=job["affine"])


def _g2_msm_device(job, A, out):
    """zkg_g2_msm_device: device-resident G2 MSM with an explicit window (always the bucket
    pipeline); the result is the normalised projective point"""
    c, sc, pts = job["curve"], A[job["sc"]], A[job["pts"]]
    lib = zk.load()
    lib.zkg_g2_msm_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_void_p, U64P, ctypes.c_int]
    ds, dp = zk.DeviceBuffer(sc), zk.DeviceBuffer(pts)
    try:
        res = np.zeros(6 * zk.NLIMBS_P[c], dtype=np.uint64)
        lib.zkg_g2_msm_device(zk.CURVE_ID[c], sc.shape[0], ds.ptr, sc.shape[1], 1, dp.ptr, _ptr(res), job["window"])
        out[job["id"]] = res
    finally:
        ds.free()
        dp.free()


CALLS = {"g2_msm_device": _g2_msm_device, "arr": _arr, "vanish": _vanish, "to_affine": _to_affine, "fft": _fft, "g2_to_affine": _g2_to_affine,
         "g2_fft": _g2_fft, "msm_affine": _msm_affine,
         "msm_variable": _msm_variable, "msm_device": _msm_device, "g2_msm": _g2_msm}


def main(src, dst):
    with np.load(src, allow_pickle=False) as z:
        A = {k: z[k] for k in z.files}
    jobs = json.loads(A.pop("jobs").tobytes().decode())
    zk.require_gpu()
    zk.load().zkg_set_device(0)
    out = {}
    for job in jobs:
        CALLS[job["call"]](job, A, out)
    np.savez(dst, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
