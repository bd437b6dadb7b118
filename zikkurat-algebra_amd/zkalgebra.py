"""Host-side mirror of the reference's MSM / NTT API, over the gfx950 C-ABI library.

The reference exposes this path to users through Haskell:

    ZK.Algebra.Curves.<C>.G1.Proj.msm      :: FlatArray Fr -> FlatArray Affine.G1 -> G1   (G1/Proj.hs:237-246)
    ZK.Algebra.Curves.<C>.G1.Proj.msmStd   :: FlatArray Std.Fr -> FlatArray Affine.G1 -> G1 (G1/Proj.hs:253-262)
    ZK.Algebra.Curves.<C>.G1.Proj.msmProj  :: FlatArray Fr -> FlatArray G1 -> G1         (G1/Proj.hs:222-223)
    ZK.Algebra.Curves.<C>.G1.Affine.msm    = toAffine . Proj.msm                           (G1/Affine.hs:143-149)
    ZK.Algebra.Curves.<C>.Poly.forwardNTT  :: FFTSubgroup Fr -> Poly -> FlatArray Fr       (Poly.hs:400-410)
    ZK.Algebra.Curves.<C>.Poly.inverseNTT  :: FFTSubgroup Fr -> FlatArray Fr -> Poly       (Poly.hs:412-422)
    ZK.Algebra.Class.FFT.getFFTSubgroup    :: Log2 -> FFTSubgroup                          (Class/FFT.hs:60-66)

GHC is not available in this image, so this module is the host-language mirror
(same names in snake_case, same argument meaning, same error messages) used by the
tests and the benchmark.  ``FlatArray`` is a C-contiguous ``numpy.uint64`` array of
shape (n, limbs) -- byte-identical to the reference's pinned FlatArray memory
(Class/Flat.hs:81-83).  Every call goes through the C ABI of
``lib/libzkalgebra_gpu.so`` and runs on the GPU; if the library or a GPU is missing,
calls raise -- there is no CPU fallback.
"""
import ctypes
import os
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# ZK_LIB_PATH: A/B experiments with variant builds of the same library (default: in-tree build)
LIB_PATH = os.environ.get("ZK_LIB_PATH") or os.path.join(HERE, "lib", "libzkalgebra_gpu.so")
U64P = ctypes.POINTER(ctypes.c_uint64)

CURVES = ("bn128", "bls12_381")
CURVE_ID = {"bn128": 0, "bls12_381": 1}
NLIMBS_P = {"bn128": 4, "bls12_381": 6}   # base field limbs (NLIMBS_P in G1_proj.c:17)
NLIMBS_R = 4                               # scalar field limbs
FFT_LOG = {"bn128": 28, "bls12_381": 32}   # 2-adicity of the FFT domain (Fr/Mont.hs fftDomain)

# every exported symbol of include/zkalgebra_gpu.h (checked by tests/test_capi.py)
REFERENCE_SYMBOLS = [
    f"{c}_G1_proj_MSM_{k}_coeff_{o}_out" for c in CURVES for k in ("mont", "std") for o in ("proj", "affine")
] + [f"{c}_G1_proj_MSM_std_coeff_proj_out_variable" for c in CURVES] + [
    f"{c}_G1_jac_MSM_{k}_coeff_{o}_out" for c in CURVES for k in ("mont", "std") for o in ("jac", "affine")
] + [f"{c}_poly_mont_ntt_{d}" for c in CURVES for d in ("forward", "inverse")]
# Fr vector ops (lib/cbits/curves/array/mont/<C>_arr_mont.h:3-48) + division by a vanishing polynomial
ARR_OPS = ["is_valid", "is_zero", "is_one", "is_equal", "set_zero", "set_one", "set_const", "copy", "from_std",
           "to_std", "append", "neg", "add", "sub", "sqr", "mul", "inv", "div", "neg_inplace", "add_inplace",
           "sub_inplace", "sqr_inplace", "mul_inplace", "inv_inplace", "div_inplace", "sub_inplace_reverse",
           "mul_add", "mul_sub", "dot_prod", "powers", "scale", "scale_inplace", "Ax_plus_y", "Ax_plus_y_inplace",
           "Ax_plus_By", "Ax_plus_By_inplace"]
REFERENCE_SYMBOLS += [f"{c}_arr_mont_{o}" for c in CURVES for o in ARR_OPS] + [
    f"{c}_poly_mont_{k}_by_vanishing" for c in CURVES for k in ("div", "quot")] + [
    f"{c}_G1_{co}_{f}" for c in CURVES for co in ("proj", "jac")
    for f in ("batch_from_affine", "batch_to_affine", "fft_forward", "fft_inverse")] + [
    f"{c}_G2_proj_MSM_{k}_coeff_{o}_out" for c in CURVES for k in ("mont", "std") for o in ("proj", "affine")] + [
    f"{c}_G2_proj_{f}" for c in CURVES
    for f in ("batch_from_affine", "batch_to_affine", "MSM_std_coeff_proj_out_variable")] + [
    f"{c}_G2_proj_fft_{d}" for c in CURVES for d in ("forward", "inverse")]
EXTENSION_SYMBOLS = [
    "zkg_version", "zkg_device_count", "zkg_set_device", "zkg_device_malloc", "zkg_device_free",
    "zkg_memcpy_htod", "zkg_memcpy_dtoh", "zkg_device_synchronize", "zkg_g1_msm_device", "zkg_ntt_device",
    "zkg_g1_proj_add", "zkg_g1_proj_normalize", "zkg_g1_proj_to_affine", "zkg_gen_fr", "zkg_gen_g1_points",
    "zkg_fft_generator", "zkg_msm_default_window", "zkg_msm_window", "zkg_timer_enable", "zkg_timer_reset", "zkg_timer_read",
    "zkg_arr_op_device", "zkg_arr_dot_device", "zkg_arr_powers_device",
    "zkg_poly_div_by_vanishing_device", "zkg_g1_fft_device", "zkg_g1_batch_to_affine_device",
    "zkg_g1_jac_fft_device", "zkg_g1_jac_batch_to_affine_device", "zkg_g2_msm_device",
    "zkg_msm_profile", "zkg_msm_set_group_limit", "zkg_msm_set_ysum_mode", "zkg_msm_set_ahead_min", "zkg_ntt_set_max_radix", "zkg_ntt_set_table_max",
    "zkg_arena_set_limit", "zkg_msm_last_groups", "zkg_g1_fft_last_glv", "zkg_g1_fft_plan", "zkg_g1_fft_radix_products", "zkg_msm_workspace_bytes", "zkg_set_devices", "zkg_get_devices",
    "zkg_release", "zkg_comm_unique_id", "zkg_comm_init", "zkg_comm_destroy", "zkg_comm_rank", "zkg_comm_world",
    "zkg_comm_allgather", "zkg_comm_barrier", "zkg_comm_max_f64", "zkg_g1_comm_sum_partials",
    "zkg_g1_msm_device_sharded", "zkg_set_error_mode", "zkg_last_error", "zkg_g2_batch_to_affine_device",
    "zkg_g2_fft_device", "zkg_g2_fft_set_max_lanes",
]

# polynomial layer (lib/cbits/curves/poly/mont/<C>_poly_mont.c:26-243)
POLY_OPS = ["degree", "is_zero", "is_equal", "neg", "add", "sub", "scale", "lincomb", "mul_naive", "eval_at"]
REFERENCE_SYMBOLS += [f"{c}_poly_mont_{o}" for c in CURVES for o in POLY_OPS]
EXTENSION_SYMBOLS += ["zkg_poly_mul_device", "zkg_poly_eval_device", "zkg_poly_lincomb_device",
                      "zkg_poly_set_mul_direct_max", "zkg_poly_last_mul_path"]
POLY_MUL_MAX_LOG = {"bn128": 28, "bls12_381": 30}   # largest product, log2 of n1 + n2 - 1
# division with remainder (<C>_poly_mont_{long_div,quot,rem}, poly_mont.c:249-309, as zkg_ entries)
EXTENSION_SYMBOLS += ["zkg_poly_long_div_device", "zkg_poly_long_div", "zkg_poly_set_div_base_max",
                      "zkg_poly_div_base_max", "zkg_poly_div_plan", "zkg_poly_last_div_steps",
                      "zkg_poly_div_profile", "zkg_poly_last_div_phase_ms"]
# coset and batched NTT
EXTENSION_SYMBOLS += ["zkg_ntt_ext_device", "zkg_ntt_ext", "zkg_ntt_ext_set_max_grid"]
# cache hooks of the NTT twiddle and shift tables
EXTENSION_SYMBOLS += ["zkg_ntt_set_cache_limit", "zkg_ntt_cache_bytes"]
# batch G1 scalar multiplication (fixed base, per-row bases, powers of a scalar) and its hooks
EXTENSION_SYMBOLS += [f"zkg_g1_scl_{k}{d}" for k in ("fixed", "rows", "powers") for d in ("", "_device")] + [
    "zkg_g1_scl_set_window", "zkg_g1_scl_set_fixed_min", "zkg_g1_scl_last_path", "zkg_g1_scl_digits",
    "zkg_g1_scl_table_bytes"]
# the same on G2
EXTENSION_SYMBOLS += [f"zkg_g2_scl_{k}{d}" for k in ("fixed", "rows", "powers") for d in ("", "_device")] + [
    "zkg_g2_scl_set_window", "zkg_g2_scl_set_fixed_min", "zkg_g2_scl_last_path", "zkg_g2_scl_table_bytes"]
# pairings: the reference's single-pair symbols, and the batch / product / final-exponentiation extensions
REFERENCE_SYMBOLS += [f"{c}_pairing_{k}" for c in CURVES for k in ("affine", "projective")]
EXTENSION_SYMBOLS += [f"zkg_pairing_{k}{d}" for k in ("rows", "product", "final_expo") for d in ("", "_device")]
# batch point validation: canonical / on-curve / subgroup / infinity flags per row, and its test hooks
EXTENSION_SYMBOLS += [f"zkg_g{g}_check_rows{d}" for g in (1, 2) for d in ("", "_device")] + [
    "zkg_check_set_mode", "zkg_check_set_max_lanes"]
# division by a linear factor, and the KZG prover on it
EXTENSION_SYMBOLS += ["zkg_poly_div_linear_device", "zkg_poly_div_linear", "zkg_poly_set_lindiv_tile",
                      "zkg_poly_lindiv_tile", "zkg_kzg_commit_device", "zkg_kzg_open_device"]
# row-wise sums of scalar multiples, and every KZG opening of a domain at once on them (FK20)
EXTENSION_SYMBOLS += ["zkg_g1_scl_rows_sum_device", "zkg_g1_scl_rows_sum", "zkg_kzg_open_all_table_bytes",
                      "zkg_kzg_open_all_table_device", "zkg_kzg_open_all_device"]
PT_CANONICAL, PT_ON_CURVE, PT_IN_SUBGROUP, PT_INFINITY = 1, 2, 4, 8
PT_VALID = PT_CANONICAL | PT_ON_CURVE | PT_IN_SUBGROUP
COORDS_ID = {"affine": 0, "proj": 1, "jac": 2}

_lib = None


def load():
    """Load the C-ABI library (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"zkalgebra_gpu library not built: {LIB_PATH} (run __graft_entry__.build())")
        lib = ctypes.CDLL(LIB_PATH)
        lib.zkg_version.restype = ctypes.c_char_p
        lib.zkg_device_malloc.restype = ctypes.c_void_p
        lib.zkg_device_malloc.argtypes = [ctypes.c_size_t]
        lib.zkg_device_free.argtypes = [ctypes.c_void_p]
        lib.zkg_memcpy_htod.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        lib.zkg_memcpy_dtoh.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        lib.zkg_g1_msm_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_void_p, U64P, ctypes.c_int]
        lib.zkg_ntt_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, U64P, ctypes.c_void_p,
                                       ctypes.c_void_p]
        if hasattr(lib, "zkg_ntt_ext_device"):  # ZK_LIB_PATH may name an older variant build (A/B timing);
            # calling a symbol it lacks still raises
            lib.zkg_ntt_ext_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, U64P, U64P, ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_void_p]
            lib.zkg_ntt_ext.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, U64P, U64P, ctypes.c_int, U64P,
                                        U64P]
            lib.zkg_ntt_ext_set_max_grid.argtypes = [ctypes.c_uint]
        lib.zkg_g2_msm_device.argtypes = lib.zkg_g1_msm_device.argtypes
        lib.zkg_g2_batch_to_affine_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        lib.zkg_g2_fft_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, U64P, ctypes.c_void_p,
                                          ctypes.c_void_p]
        lib.zkg_g2_fft_set_max_lanes.argtypes = [ctypes.c_int]
        for c in CURVES:
            for d in ("forward", "inverse"):
                getattr(lib, f"{c}_G2_proj_fft_{d}").argtypes = [ctypes.c_int, U64P, U64P, U64P]
        lib.zkg_gen_fr.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, U64P]
        lib.zkg_gen_g1_points.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, U64P]
        lib.zkg_timer_read.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_long)]
        lib.zkg_msm_set_group_limit.argtypes = [ctypes.c_size_t]
        lib.zkg_ntt_set_table_max.argtypes = [ctypes.c_size_t]
        if hasattr(lib, "zkg_ntt_set_cache_limit"):  # as above: absent from an older variant build
            lib.zkg_ntt_set_cache_limit.argtypes = [ctypes.c_size_t]
            lib.zkg_ntt_cache_bytes.restype = ctypes.c_size_t
            lib.zkg_ntt_cache_bytes.argtypes = []
        lib.zkg_arena_set_limit.argtypes = [ctypes.c_size_t]
        lib.zkg_msm_workspace_bytes.restype = ctypes.c_size_t
        lib.zkg_msm_workspace_bytes.argtypes = [ctypes.c_int] * 7
        lib.zkg_set_devices.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
        lib.zkg_get_devices.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
        for c in CURVES:
            for o in ("is_valid", "is_zero", "is_one", "is_equal"):
                getattr(lib, f"{c}_arr_mont_{o}").restype = ctypes.c_uint8
            getattr(lib, f"{c}_poly_mont_quot_by_vanishing").restype = ctypes.c_uint8
            for o in ("is_zero", "is_equal"):
                getattr(lib, f"{c}_poly_mont_{o}").restype = ctypes.c_uint8
            getattr(lib, f"{c}_poly_mont_lincomb").argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                                                ctypes.POINTER(U64P), ctypes.POINTER(U64P), U64P]
        lib.zkg_poly_mul_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                            ctypes.c_void_p]
        lib.zkg_poly_eval_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, U64P, U64P]
        lib.zkg_poly_lincomb_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), U64P,
                                                ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p]
        if hasattr(lib, "zkg_poly_long_div"):  # absent from an older variant build, as above
            lib.zkg_poly_long_div_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                     ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                     ctypes.c_void_p]
            lib.zkg_poly_long_div.argtypes = [ctypes.c_int, ctypes.c_int, U64P, ctypes.c_int, U64P, ctypes.c_int, U64P,
                                              ctypes.c_int, U64P]
            lib.zkg_poly_set_div_base_max.argtypes = [ctypes.c_int]
            lib.zkg_poly_div_plan.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
            lib.zkg_poly_div_profile.argtypes = [ctypes.c_int]
            lib.zkg_poly_last_div_phase_ms.argtypes = [ctypes.POINTER(ctypes.c_double)]
        lib.zkg_arr_op_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, U64P, U64P, ctypes.c_void_p]
        lib.zkg_arr_dot_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, U64P]
        lib.zkg_arr_powers_device.argtypes = [ctypes.c_int, ctypes.c_int, U64P, U64P, ctypes.c_void_p]
        lib.zkg_poly_div_by_vanishing_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                         U64P, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                         ctypes.c_void_p]
        for f in (lib.zkg_g1_batch_to_affine_device, lib.zkg_g1_jac_batch_to_affine_device):
            f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        lib.zkg_g1_fft_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, U64P, ctypes.c_void_p,
                                          ctypes.c_void_p]
        if hasattr(lib, "zkg_g1_scl_fixed"):  # absent from an older variant build, as above
            lib.zkg_g1_scl_fixed_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, U64P,
                                                    ctypes.c_int, ctypes.c_void_p]
            lib.zkg_g1_scl_rows_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                   ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
            for f in (lib.zkg_g1_scl_fixed, lib.zkg_g1_scl_rows):
                f.argtypes = [ctypes.c_int, ctypes.c_int, U64P, ctypes.c_int, U64P, ctypes.c_int, U64P]
            lib.zkg_g1_scl_powers_device.argtypes = [ctypes.c_int, ctypes.c_int, U64P, U64P, U64P, ctypes.c_int,
                                                     ctypes.c_void_p]
            lib.zkg_g1_scl_powers.argtypes = [ctypes.c_int, ctypes.c_int, U64P, U64P, U64P, ctypes.c_int, U64P]
            lib.zkg_g1_scl_set_window.argtypes = [ctypes.c_int]
            lib.zkg_g1_scl_set_fixed_min.argtypes = [ctypes.c_int]
            lib.zkg_g1_scl_digits.argtypes = [ctypes.c_int, U64P, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
            lib.zkg_g1_scl_table_bytes.restype = ctypes.c_size_t
            lib.zkg_g1_scl_table_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
        if hasattr(lib, "zkg_pairing_rows"):  # absent from an older variant build, as above
            vp = ctypes.c_void_p  # host arrays and device addresses alike: never a truncated int
            for k in ("rows", "product"):
                for d in ("", "_device"):
                    getattr(lib, f"zkg_pairing_{k}{d}").argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp]
            for d in ("", "_device"):
                getattr(lib, f"zkg_pairing_final_expo{d}").argtypes = [ctypes.c_int, ctypes.c_int, vp, vp]
            for c in CURVES:
                for k in ("affine", "projective"):
                    getattr(lib, f"{c}_pairing_{k}").argtypes = [vp, vp, vp]
                    getattr(lib, f"{c}_pairing_{k}").restype = None
        if hasattr(lib, "zkg_g2_scl_fixed"):  # absent from an older variant build, as above
            lib.zkg_g2_scl_fixed_device.argtypes = lib.zkg_g1_scl_fixed_device.argtypes
            lib.zkg_g2_scl_rows_device.argtypes = lib.zkg_g1_scl_rows_device.argtypes
            for f in (lib.zkg_g2_scl_fixed, lib.zkg_g2_scl_rows):
                f.argtypes = lib.zkg_g1_scl_fixed.argtypes
            lib.zkg_g2_scl_powers_device.argtypes = lib.zkg_g1_scl_powers_device.argtypes
            lib.zkg_g2_scl_powers.argtypes = lib.zkg_g1_scl_powers.argtypes
            lib.zkg_g2_scl_set_window.argtypes = [ctypes.c_int]
            lib.zkg_g2_scl_set_fixed_min.argtypes = [ctypes.c_int]
            lib.zkg_g2_scl_table_bytes.restype = ctypes.c_size_t
            lib.zkg_g2_scl_table_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
        if hasattr(lib, "zkg_g1_check_rows"):  # absent from an older variant build, as above
            for g in (1, 2):
                for d in ("", "_device"):
                    getattr(lib, f"zkg_g{g}_check_rows{d}").argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                                        ctypes.c_int, ctypes.c_void_p]
            lib.zkg_check_set_mode.argtypes = [ctypes.c_int]
            lib.zkg_check_set_mode.restype = None
            lib.zkg_check_set_max_lanes.argtypes = [ctypes.c_int]
            lib.zkg_check_set_max_lanes.restype = None
        if hasattr(lib, "zkg_poly_div_linear"):  # absent from an older variant build, as above
            vp = ctypes.c_void_p
            for f in (lib.zkg_poly_div_linear_device, lib.zkg_poly_div_linear):
                f.argtypes = [ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, vp, vp]
            lib.zkg_poly_set_lindiv_tile.argtypes = [ctypes.c_int]
            lib.zkg_poly_set_lindiv_tile.restype = None
            lib.zkg_kzg_commit_device.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp]
            lib.zkg_kzg_open_device.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_int, vp, vp, vp]
        if hasattr(lib, "zkg_kzg_open_all_device"):  # absent from an older variant build, as above
            vp = ctypes.c_void_p
            for f in (lib.zkg_g1_scl_rows_sum_device, lib.zkg_g1_scl_rows_sum):
                f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_int, vp]
            lib.zkg_kzg_open_all_table_bytes.restype = ctypes.c_size_t
            lib.zkg_kzg_open_all_table_bytes.argtypes = [ctypes.c_int] * 3
            lib.zkg_kzg_open_all_table_device.argtypes = [ctypes.c_int] * 3 + [vp, vp]
            lib.zkg_kzg_open_all_device.argtypes = [ctypes.c_int] * 4 + [vp, vp, ctypes.c_int, vp]
        lib.zkg_last_error.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
        lib.zkg_comm_unique_id.argtypes = [ctypes.c_void_p]
        lib.zkg_comm_init.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        lib.zkg_comm_allgather.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        lib.zkg_comm_max_f64.argtypes = [ctypes.POINTER(ctypes.c_double)]
        lib.zkg_g1_comm_sum_partials.argtypes = [ctypes.c_int, U64P, ctypes.c_int, U64P]
        lib.zkg_g1_msm_device_sharded.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, U64P]
        _lib = lib
    return _lib


def _p(a):
    if a.dtype != np.uint64 or not a.flags["C_CONTIGUOUS"]:
        raise TypeError("FlatArray buffers must be C-contiguous numpy.uint64 arrays")
    return a.ctypes.data_as(U64P)


def device_count():
    return load().zkg_device_count()


def require_gpu():
    if device_count() < 1:
        raise RuntimeError("zkalgebra_gpu: no GPU visible -- the MSM/NTT path is GPU-only (no CPU fallback)")


# ----------------------------------------------------------------------------- FFT subgroups

@dataclass(frozen=True)
class FFTSubgroup:
    """Mirror of ZK.Algebra.Class.FFT.FFTSubgroup (Class/FFT.hs:26-30): generator (Montgomery
    Fr, 4 limbs) of the multiplicative subgroup of order 2^log_size."""
    curve: str
    gen: tuple
    log_size: int

    @property
    def size(self):
        return 1 << self.log_size

    def gen_array(self):
        return np.array(self.gen, dtype=np.uint64)


def get_fft_subgroup(curve, log_size):
    """getFFTSubgroup (Class/FFT.hs:60-66): gen_m = fftDomain^(2^(M - m))."""
    if not (0 <= log_size <= FFT_LOG[curve]):
        raise ValueError("getFFTSubgroup: subgroup size is too large for this field")
    out = np.zeros(4, dtype=np.uint64)
    load().zkg_fft_generator(CURVE_ID[curve], log_size, _p(out))
    return FFTSubgroup(curve, tuple(int(x) for x in out), log_size)


# ----------------------------------------------------------------------------- MSM

def _check_msm(curve, coeffs, points):
    if coeffs.ndim != 2 or points.ndim != 2 or coeffs.shape[0] != points.shape[0]:
        raise ValueError("msm: incompatible array dimensions")   # G1/Proj.hs:239
    if points.shape[1] != 2 * NLIMBS_P[curve]:
        raise ValueError("msm: points must be affine (x, y) in Montgomery form")
    if coeffs.shape[1] < 1:
        raise ValueError("msm: coefficients need at least one limb")


def msm(curve, coeffs, points):
    """Proj.msm: Montgomery-form Fr coefficients x affine points -> projective G1 (normalised)."""
    _check_msm(curve, coeffs, points)
    require_gpu()
    out = np.zeros(3 * NLIMBS_P[curve], dtype=np.uint64)
    getattr(load(), f"{curve}_G1_proj_MSM_mont_coeff_proj_out")(
        coeffs.shape[0], _p(coeffs), _p(points), _p(out), coeffs.shape[1])
    return out


def msm_std(curve, coeffs, points):
    """Proj.msmStd: standard-form (plain integer) coefficients, used verbatim."""
    _check_msm(curve, coeffs, points)
    require_gpu()
    out = np.zeros(3 * NLIMBS_P[curve], dtype=np.uint64)
    getattr(load(), f"{curve}_G1_proj_MSM_std_coeff_proj_out")(
        coeffs.shape[0], _p(coeffs), _p(points), _p(out), coeffs.shape[1])
    return out


def msm_affine(curve, coeffs, points, std=False):
    """Affine.msm = toAffine . Proj.msm (G1/Affine.hs:143-149); infinity = all-0xFF."""
    _check_msm(curve, coeffs, points)
    require_gpu()
    out = np.zeros(2 * NLIMBS_P[curve], dtype=np.uint64)
    name = f"{curve}_G1_proj_MSM_{'std' if std else 'mont'}_coeff_affine_out"
    getattr(load(), name)(coeffs.shape[0], _p(coeffs), _p(points), _p(out), coeffs.shape[1])
    return out


def msm_variable(curve, coeffs, points, window_size):
    """<C>_G1_proj_MSM_std_coeff_proj_out_variable (exported, unbound by Haskell)."""
    _check_msm(curve, coeffs, points)
    require_gpu()
    out = np.zeros(3 * NLIMBS_P[curve], dtype=np.uint64)
    getattr(load(), f"{curve}_G1_proj_MSM_std_coeff_proj_out_variable")(
        coeffs.shape[0], _p(coeffs), _p(points), _p(out), coeffs.shape[1], int(window_size))
    return out


def msm_jac(curve, coeffs, points, std=False):
    """Jac.msm (G1/Jac.hs:225-259): Jacobian output, normalised; infinity = (1:1:0)."""
    _check_msm(curve, coeffs, points)
    require_gpu()
    out = np.zeros(3 * NLIMBS_P[curve], dtype=np.uint64)
    name = f"{curve}_G1_jac_MSM_{'std' if std else 'mont'}_coeff_jac_out"
    getattr(load(), name)(coeffs.shape[0], _p(coeffs), _p(points), _p(out), coeffs.shape[1])
    return out


def msm_jac_points(curve, coeffs, jac_points):
    """Jac's Curve.msm: msmJac cs gs = msm cs (batchToAffine gs) (G1/Jac.hs:188, 220), with the
    conversion on the GPU (<C>_G1_jac_batch_to_affine) instead of N serial CPU inversions."""
    if jac_points.ndim != 2 or jac_points.shape[1] != 3 * NLIMBS_P[curve]:
        raise ValueError("msm: incompatible array dimensions")
    return msm_jac(curve, coeffs, batch_to_affine(curve, jac_points, coords="jac"))


def msm_proj(curve, coeffs, proj_points):
    """Proj.msmProj cs gs = msm cs (batchToAffine gs) (G1/Proj.hs:222-223)."""
    if proj_points.ndim != 2 or proj_points.shape[1] != 3 * NLIMBS_P[curve]:
        raise ValueError("msm: incompatible array dimensions")
    # batchToAffine on the GPU (<C>_G1_proj_batch_to_affine, Montgomery's trick), as msmProj does
    return msm(curve, coeffs, batch_to_affine(curve, proj_points))


def g2_msm(curve, coeffs, points, std=False, affine=False):
    """G2 MSM (<C>_G2_proj_MSM_*_coeff_*_out): points are affine G2 (x0 x1 y0 y1, Montgomery Fp)"""
    if coeffs.ndim != 2 or points.ndim != 2 or coeffs.shape[0] != points.shape[0]:
        raise ValueError("msm: incompatible array dimensions")
    if points.shape[1] != 4 * NLIMBS_P[curve]:
        raise ValueError("msm: G2 points must be affine (x, y) over Fp2 in Montgomery form")
    require_gpu()
    out = np.zeros((4 if affine else 6) * NLIMBS_P[curve], dtype=np.uint64)
    name = f"{curve}_G2_proj_MSM_{'std' if std else 'mont'}_coeff_{'affine' if affine else 'proj'}_out"
    getattr(load(), name)(coeffs.shape[0], _p(coeffs), _p(points), _p(out), coeffs.shape[1])
    return out


def g2_msm_variable(curve, coeffs, points, window_size):
    """<C>_G2_proj_MSM_std_coeff_proj_out_variable (bls12_381_G2_proj.c:498; exported, unbound by Haskell)."""
    if coeffs.ndim != 2 or points.ndim != 2 or coeffs.shape[0] != points.shape[0]:
        raise ValueError("msm: incompatible array dimensions")
    if points.shape[1] != 4 * NLIMBS_P[curve]:
        raise ValueError("msm: G2 points must be affine (x, y) over Fp2 in Montgomery form")
    require_gpu()
    out = np.zeros(6 * NLIMBS_P[curve], dtype=np.uint64)
    getattr(load(), f"{curve}_G2_proj_MSM_std_coeff_proj_out_variable")(
        coeffs.shape[0], _p(coeffs), _p(points), _p(out), coeffs.shape[1], int(window_size))
    return out


def _g2_rows(name, a, words):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim != 2 or a.shape[1] != words:
        raise ValueError(f"{name}: G2 rows must have {words} limbs")
    return a


def g2_batch_from_affine(curve, aff):
    """G2 Proj.batchFromAffine (G2/Proj.hs:386-394): infinity (all-0xFF) -> (0 : 1 : 0)"""
    aff = _g2_rows("batchFromAffine", aff, 4 * NLIMBS_P[curve])
    require_gpu()
    out = np.zeros((aff.shape[0], 6 * NLIMBS_P[curve]), dtype=np.uint64)
    getattr(load(), f"{curve}_G2_proj_batch_from_affine")(aff.shape[0], _p(aff), _p(out))
    return out


def g2_batch_to_affine(curve, proj):
    """G2 Proj.batchToAffine (G2/Proj.hs:396-405): Z = 0 -> all-0xFF"""
    proj = _g2_rows("batchToAffine", proj, 6 * NLIMBS_P[curve])
    require_gpu()
    out = np.zeros((proj.shape[0], 4 * NLIMBS_P[curve]), dtype=np.uint64)
    getattr(load(), f"{curve}_G2_proj_batch_to_affine")(proj.shape[0], _p(proj), _p(out))
    return out


def g2_msm_proj(curve, coeffs, proj_points, std=False, affine=False):
    """G2 Proj.msmProj cs gs = msm cs (batchToAffine gs) (G2/Proj.hs:223-224).  The projective rows
    are uploaded once, converted on the device (zkg_g2_batch_to_affine_device) and fed to the
    device-resident MSM, so the affine array never crosses the host link."""
    if coeffs.ndim != 2 or proj_points.ndim != 2 or coeffs.shape[0] != proj_points.shape[0]:
        raise ValueError("msm: incompatible array dimensions")
    if proj_points.shape[1] != 6 * NLIMBS_P[curve]:
        raise ValueError("msm: G2 points must be projective (X, Y, Z) over Fp2 in Montgomery form")
    if coeffs.shape[1] < 1:
        raise ValueError("msm: coefficients need at least one limb")
    require_gpu()
    lib, cid, NP = load(), CURVE_ID[curve], NLIMBS_P[curve]
    n = coeffs.shape[0]
    coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64)
    proj_points = np.ascontiguousarray(proj_points, dtype=np.uint64)
    bufs = []
    try:
        bufs.append(DeviceBuffer(coeffs))
        bufs.append(DeviceBuffer(proj_points))
        bufs.append(DeviceBuffer.empty(n * 4 * NP * 8))
        d_sc, d_proj, d_aff = bufs
        lib.zkg_g2_batch_to_affine_device(cid, n, d_proj.ptr, d_aff.ptr)
        res = g2_msm_device(curve, n, d_sc, d_aff, mont=not std, nlimbs=coeffs.shape[1])
    finally:
        for b in bufs:
            b.free()
    if not affine:
        return res  # normalised by zkg_g2_msm_device
    # (x : y : 1) or (0 : 1 : 0) -> affine, as the host-side conversion of the G2 entry points
    out = np.full(4 * NP, np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    if res[4 * NP:].any():
        out[:] = res[:4 * NP]
    return out


def g1_to_affine(curve, proj):
    out = np.zeros(2 * NLIMBS_P[curve], dtype=np.uint64)
    load().zkg_g1_proj_to_affine(CURVE_ID[curve], _p(np.ascontiguousarray(proj)), _p(out))
    return out


def g1_normalize(curve, proj):
    out = np.zeros(3 * NLIMBS_P[curve], dtype=np.uint64)
    load().zkg_g1_proj_normalize(CURVE_ID[curve], _p(np.ascontiguousarray(proj)), _p(out))
    return out


def g1_add(curve, a, b):
    out = np.zeros(3 * NLIMBS_P[curve], dtype=np.uint64)
    load().zkg_g1_proj_add(CURVE_ID[curve], _p(np.ascontiguousarray(a)), _p(np.ascontiguousarray(b)), _p(out))
    return out


def batch_from_affine(curve, aff, coords="proj"):
    """Proj.batchFromAffine (G1/Proj.hs:409-418); coords="jac": Jac.batchFromAffine (G1/Jac.hs:374-380),
    infinity -> (1 : 1 : 0)"""
    aff = np.ascontiguousarray(aff, dtype=np.uint64)
    out = np.zeros((aff.shape[0], 3 * NLIMBS_P[curve]), dtype=np.uint64)
    require_gpu()
    getattr(load(), f"{curve}_G1_{_coords(coords)}_batch_from_affine")(aff.shape[0], _p(aff), _p(out))
    return out


def batch_to_affine(curve, proj, coords="proj"):
    """Proj.batchToAffine (G1/Proj.hs:420-430); coords="jac": Jac.batchToAffine (G1/Jac.hs:382-389);
    infinity -> all-0xFF"""
    proj = np.ascontiguousarray(proj, dtype=np.uint64)
    out = np.zeros((proj.shape[0], 2 * NLIMBS_P[curve]), dtype=np.uint64)
    require_gpu()
    getattr(load(), f"{curve}_G1_{_coords(coords)}_batch_to_affine")(proj.shape[0], _p(proj), _p(out))
    return out


def _coords(coords):
    if coords not in ("proj", "jac"):
        raise ValueError(f"coords must be 'proj' or 'jac', not {coords!r}")
    return coords


def _curve_fft(sg, pts, name, msg, coords):
    pts = np.ascontiguousarray(pts, dtype=np.uint64)
    if pts.ndim != 2 or sg.size != pts.shape[0]:
        raise ValueError(msg)
    require_gpu()
    out = np.zeros_like(pts)
    getattr(load(), f"{sg.curve}_G1_{_coords(coords)}_{name}")(sg.log_size, _p(sg.gen_array()), _p(pts), _p(out))
    return out


def forward_fft(sg, pts, coords="proj"):
    """Proj.forwardFFT = curveFFT (G1/Proj.hs:270-281; Jacobian: G1/Jac.hs:266-276):
    [L_k(tau)] -> [tau^i] points, normalised"""
    return _curve_fft(sg, pts, "fft_forward", "forwardNTT: subgroup size differs from the array size", coords)


def inverse_fft(sg, pts, coords="proj"):
    """Proj.inverseFFT = curveIFFT (G1/Proj.hs:283-294; Jacobian: G1/Jac.hs:278-288):
    [tau^i] -> [L_k(tau)] points, normalised"""
    return _curve_fft(sg, pts, "fft_inverse", "inverseNTT: subgroup size differs from the array size", coords)


curve_fft = forward_fft
curve_ifft = inverse_fft


def _g2_curve_fft(sg, pts, name, msg):
    pts = np.asarray(pts)
    if pts.ndim != 2 or pts.shape[1] != 6 * NLIMBS_P[sg.curve]:
        raise ValueError(f"{name}: G2 rows must be projective, {6 * NLIMBS_P[sg.curve]} limbs")
    if sg.size != pts.shape[0]:
        raise ValueError(msg)
    pts = np.ascontiguousarray(pts, dtype=np.uint64)
    require_gpu()
    out = np.zeros_like(pts)
    getattr(load(), f"{sg.curve}_G2_proj_{name}")(sg.log_size, _p(sg.gen_array()), _p(pts), _p(out))
    return out


def g2_forward_fft(sg, pts):
    """G2 Proj.forwardFFT = curveFFT (G2/Proj.hs): [L_k(tau)]_2 -> [tau^i]_2, normalised rows"""
    return _g2_curve_fft(sg, pts, "fft_forward", "forwardNTT: subgroup size differs from the array size")


def g2_inverse_fft(sg, pts):
    """G2 Proj.inverseFFT = curveIFFT (G2/Proj.hs): [tau^i]_2 -> [L_k(tau)]_2, normalised rows"""
    return _g2_curve_fft(sg, pts, "fft_inverse", "inverseNTT: subgroup size differs from the array size")


def g2_fft_device(curve, m, gen, d_src, d_dst, inverse=False):
    """device-resident G2 group FFT: d_src / d_dst are DeviceBuffers of 2^m projective rows"""
    load().zkg_g2_fft_device(CURVE_ID[curve], 1 if inverse else 0, m, _p(np.ascontiguousarray(gen, dtype=np.uint64)),
                             d_src.ptr, d_dst.ptr)


def g2_fft_set_max_lanes(lanes):
    """test hook: cap on the scalar-multiplication lanes of a G2 FFT stage (0 restores the default)"""
    load().zkg_g2_fft_set_max_lanes(int(lanes))


# ----------------------------------------------------------------------------- NTT

def forward_ntt(sg, poly):
    """Poly.forwardNTT: evaluations f(gen^k), k = 0..n-1 (Poly.hs:400-410)."""
    if poly.ndim != 2 or sg.size != poly.shape[0]:
        raise ValueError("forwardNTT: subgroup size differs from the array size")   # Poly.hs:403
    require_gpu()
    out = np.empty_like(poly)  # every element is written (as the binding's mallocForeignPtrArray)
    getattr(load(), f"{sg.curve}_poly_mont_ntt_forward")(sg.log_size, _p(sg.gen_array()), _p(poly), _p(out))
    return out


def inverse_ntt(sg, values):
    """Poly.inverseNTT: interpolation (Poly.hs:412-422)."""
    if values.ndim != 2 or sg.size != values.shape[0]:
        raise ValueError("inverseNTT: subgroup size differs from the array size")   # Poly.hs:415
    require_gpu()
    out = np.empty_like(values)  # every element is written
    getattr(load(), f"{sg.curve}_poly_mont_ntt_inverse")(sg.log_size, _p(sg.gen_array()), _p(values), _p(out))
    return out


# UnivariateFFT instance (Poly.hs:424-426)
ntt = forward_ntt
intt = inverse_ntt


def _shift_arg(shift):
    return None if shift is None else _p(_k(shift))


def ntt_ext(curve, m, gen, src, inverse=False, shift=None, batch=1):
    """zkg_ntt_ext on host arrays: `batch` transforms of 2^m rows each (src: batch * 2^m rows), on the
    coset shift * <gen> when a shift (one Montgomery Fr) is given"""
    src = _fr(src)
    if batch >= 0 and 0 <= m <= 30 and src.shape[0] != batch << m:
        raise ValueError("ntt_ext: the array does not hold batch * 2^m rows")
    require_gpu()
    out = np.empty_like(src)
    rc = load().zkg_ntt_ext(CURVE_ID[curve], 1 if inverse else 0, m, _p(_k(gen)), _shift_arg(shift), batch, _p(src),
                            _p(out))
    if rc != 0:
        raise ValueError("ntt_ext: log2 size outside 0..30, negative batch, or an inverse with shift 0")
    return out


def _ntt_batch(sg, arr, inverse, name):
    arr = np.ascontiguousarray(arr, dtype=np.uint64)
    if arr.ndim != 3 or arr.shape[1] != sg.size or arr.shape[2] != NLIMBS_R:
        raise ValueError(f"{name}: expected an array of shape (B, subgroup size, 4)")
    out = ntt_ext(sg.curve, sg.log_size, sg.gen_array(), arr.reshape(-1, NLIMBS_R), inverse=inverse,
                  batch=arr.shape[0])
    return out.reshape(arr.shape)


def forward_ntt_batch(sg, polys):
    """forwardNTT of every polynomial of a (B, 2^m, 4) array in one call (every pass one launch)"""
    return _ntt_batch(sg, polys, False, "forwardNTT")


def inverse_ntt_batch(sg, values):
    """inverseNTT of every row block of a (B, 2^m, 4) array in one call"""
    return _ntt_batch(sg, values, True, "inverseNTT")


def coset_ntt(sg, shift, poly):
    """evaluations f(shift * gen^k), k = 0..n-1: the shift powers ride on the first pass's load"""
    if poly.ndim != 2 or sg.size != poly.shape[0]:
        raise ValueError("forwardNTT: subgroup size differs from the array size")
    return ntt_ext(sg.curve, sg.log_size, sg.gen_array(), poly, shift=shift)


def coset_intt(sg, shift, values):
    """interpolation from the values on the coset shift * <gen> (shift != 0)"""
    if values.ndim != 2 or sg.size != values.shape[0]:
        raise ValueError("inverseNTT: subgroup size differs from the array size")
    return ntt_ext(sg.curve, sg.log_size, sg.gen_array(), values, inverse=True, shift=shift)


# ----------------------------------------------------------------------------- Fr vectors

def _fr(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim != 2 or a.shape[1] != NLIMBS_R:
        raise TypeError("FlatArray Fr must have shape (n, 4)")
    return a


def _same(name, *arrs):
    if any(x.shape[0] != arrs[0].shape[0] for x in arrs):
        raise ValueError(f"{name}: incompatible input array lengths")   # Array.hs:217-360


def _arr(curve, op):
    require_gpu()
    return getattr(load(), f"{curve}_arr_mont_{op}")


def arr_is_valid(curve, a):
    a = _fr(a)
    return bool(_arr(curve, "is_valid")(a.shape[0], _p(a)))


def arr_is_zero(curve, a):
    a = _fr(a)
    return bool(_arr(curve, "is_zero")(a.shape[0], _p(a)))


def arr_is_one(curve, a):
    a = _fr(a)
    return bool(_arr(curve, "is_one")(a.shape[0], _p(a)))


def arr_is_equal(curve, a, b):
    a, b = _fr(a), _fr(b)
    _same("isEqual", a, b)
    return bool(_arr(curve, "is_equal")(a.shape[0], _p(a), _p(b)))


def _unary(curve, op, a):
    a = _fr(a)
    out = np.zeros_like(a)
    _arr(curve, op)(a.shape[0], _p(a), _p(out))
    return out


def _binary(curve, op, name, a, b):
    a, b = _fr(a), _fr(b)
    _same(name, a, b)
    out = np.zeros_like(a)
    _arr(curve, op)(a.shape[0], _p(a), _p(b), _p(out))
    return out


def arr_from_std(curve, a): return _unary(curve, "from_std", a)
def arr_to_std(curve, a): return _unary(curve, "to_std", a)
def arr_neg(curve, a): return _unary(curve, "neg", a)
def arr_sqr(curve, a): return _unary(curve, "sqr", a)
def arr_inv(curve, a): return _unary(curve, "inv", a)
def arr_add(curve, a, b): return _binary(curve, "add", "add", a, b)
def arr_sub(curve, a, b): return _binary(curve, "sub", "sub", a, b)
def arr_mul(curve, a, b): return _binary(curve, "mul", "mul", a, b)
def arr_div(curve, a, b): return _binary(curve, "div", "div", a, b)


def arr_append(curve, a, b):
    a, b = _fr(a), _fr(b)
    out = np.zeros((a.shape[0] + b.shape[0], 4), dtype=np.uint64)
    _arr(curve, "append")(a.shape[0], b.shape[0], _p(a), _p(b), _p(out))
    return out


def arr_cons(curve, x, a): return arr_append(curve, np.asarray(x, dtype=np.uint64).reshape(1, 4), a)
def arr_snoc(curve, a, y): return arr_append(curve, a, np.asarray(y, dtype=np.uint64).reshape(1, 4))


def arr_scale(curve, k, a):
    a = _fr(a)
    out = np.zeros_like(a)
    _arr(curve, "scale")(a.shape[0], _p(np.ascontiguousarray(k, dtype=np.uint64)), _p(a), _p(out))
    return out


def arr_dot_prod(curve, a, b):
    a, b = _fr(a), _fr(b)
    _same("dotProd", a, b)
    out = np.zeros(4, dtype=np.uint64)
    _arr(curve, "dot_prod")(a.shape[0], _p(a), _p(b), _p(out))
    return out


def arr_powers(curve, a, b, n):
    """powers a b n = [a b^i | i <- [0..n-1]] (Array.hs:99)"""
    out = np.zeros((n, 4), dtype=np.uint64)
    _arr(curve, "powers")(n, _p(np.ascontiguousarray(a, dtype=np.uint64)),
                          _p(np.ascontiguousarray(b, dtype=np.uint64)), _p(out))
    return out


def _fused(curve, op, name, a, b, c):
    a, b, c = _fr(a), _fr(b), _fr(c)
    _same(name, a, b, c)
    out = np.zeros_like(a)
    _arr(curve, op)(a.shape[0], _p(a), _p(b), _p(c), _p(out))
    return out


def arr_mul_add(curve, a, b, c): return _fused(curve, "mul_add", "mulAdd", a, b, c)
def arr_mul_sub(curve, a, b, c): return _fused(curve, "mul_sub", "mulSub", a, b, c)


def arr_lin_comb1(curve, ax, y):
    """linComb1 (a, x) y = a x + y (Array.hs:135-146)"""
    (a, x), y = ax, _fr(y)
    x = _fr(x)
    if x.shape[0] != y.shape[0]:
        raise ValueError("linComb1: incompatible vector dimensions")
    out = np.zeros_like(x)
    _arr(curve, "Ax_plus_y")(x.shape[0], _p(np.ascontiguousarray(a, dtype=np.uint64)), _p(x), _p(y), _p(out))
    return out


def arr_lin_comb2(curve, ax, by):
    """linComb2 (a, x) (b, y) = a x + b y (Array.hs:148-161)"""
    (a, x), (b, y) = ax, by
    x, y = _fr(x), _fr(y)
    if x.shape[0] != y.shape[0]:
        raise ValueError("linComb2: incompatible vector dimensions")
    out = np.zeros_like(x)
    _arr(curve, "Ax_plus_By")(x.shape[0], _p(np.ascontiguousarray(a, dtype=np.uint64)),
                              _p(np.ascontiguousarray(b, dtype=np.uint64)), _p(x), _p(y), _p(out))
    return out


def div_by_vanishing(curve, poly, expo_n, eta):
    """Poly.divByVanishing (Poly.hs:367-380): (quotient, remainder) by x^n - eta."""
    poly = _fr(poly)
    n1 = poly.shape[0]
    nq, nr = max(0, n1 - expo_n), max(0, expo_n)
    q = np.zeros((nq, 4), dtype=np.uint64)
    r = np.zeros((nr, 4), dtype=np.uint64)
    require_gpu()
    getattr(load(), f"{curve}_poly_mont_div_by_vanishing")(n1, _p(poly), expo_n,
                                                            _p(np.ascontiguousarray(eta, dtype=np.uint64)),
                                                            nq, _p(q), nr, _p(r))
    return q, r


def quot_by_vanishing(curve, poly, expo_n, eta):
    """Poly.quotByVanishing (Poly.hs:383-397): the quotient, or None if the remainder is nonzero."""
    poly = _fr(poly)
    n1 = poly.shape[0]
    nq = max(0, n1 - expo_n)
    q = np.zeros((nq, 4), dtype=np.uint64)
    require_gpu()
    ok = getattr(load(), f"{curve}_poly_mont_quot_by_vanishing")(n1, _p(poly), expo_n,
                                                                  _p(np.ascontiguousarray(eta, dtype=np.uint64)),
                                                                  nq, _p(q))
    return q if ok else None


# ----------------------------------------------------------------------------- polynomials (Poly.hs)

def _poly(curve, op):
    require_gpu()
    return getattr(load(), f"{curve}_poly_mont_{op}")


def _k(x):
    x = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1)
    if x.shape[0] != NLIMBS_R:
        raise TypeError("an Fr element has 4 words")
    return x


def poly_mul(curve, a, b):
    """Poly (*) (Poly.hs:133 binds it to mul_naive): the n1 + n2 - 1 coefficients of a * b, by the
    direct kernel (short factor) or by NTTs; bit-identical to the reference's double loop.  An empty
    factor gives what the reference's loop writes: max(0, n1 + n2 - 1) zeros."""
    a, b = _fr(a), _fr(b)
    n = a.shape[0] + b.shape[0] - 1
    if n > (1 << POLY_MUL_MAX_LOG[curve]):
        raise ValueError(f"poly_mul: more than 2^{POLY_MUL_MAX_LOG[curve]} coefficients")
    out = np.zeros((max(0, n), 4), dtype=np.uint64)
    _poly(curve, "mul_naive")(a.shape[0], _p(a), b.shape[0], _p(b), _p(out))
    return out


def poly_sqr(curve, a):
    """Poly sqr x = mul x x: the same array as both factors (one forward transform)"""
    a = _fr(a)
    return poly_mul(curve, a, a)


def poly_eval_at(curve, poly, x):
    """Poly.evalAt (Poly.hs:229-237)"""
    poly = _fr(poly)
    out = np.zeros(4, dtype=np.uint64)
    _poly(curve, "eval_at")(poly.shape[0], _p(poly), _p(_k(x)), _p(out))
    return out


def _poly_binary(curve, op, a, b):
    a, b = _fr(a), _fr(b)
    out = np.zeros((max(a.shape[0], b.shape[0]), 4), dtype=np.uint64)
    _poly(curve, op)(a.shape[0], _p(a), b.shape[0], _p(b), _p(out))
    return out


def poly_add(curve, a, b): return _poly_binary(curve, "add", a, b)
def poly_sub(curve, a, b): return _poly_binary(curve, "sub", a, b)


def poly_neg(curve, a):
    a = _fr(a)
    out = np.zeros_like(a)
    _poly(curve, "neg")(a.shape[0], _p(a), _p(out))
    return out


def poly_scale(curve, k, a):
    a = _fr(a)
    out = np.zeros_like(a)
    _poly(curve, "scale")(_p(_k(k)), a.shape[0], _p(a), _p(out))
    return out


def poly_lincomb(curve, terms):
    """sum of k_i * p_i over terms = [(k_i, p_i), ...]; max length of the p_i coefficients"""
    ks = [_k(k) for k, _ in terms]
    ps = [_fr(p) for _, p in terms]
    K = len(terms)
    out = np.zeros((max([p.shape[0] for p in ps], default=0), 4), dtype=np.uint64)
    ns = (ctypes.c_int * max(1, K))(*[p.shape[0] for p in ps])
    cs = (U64P * max(1, K))(*[_p(k) for k in ks])
    pp = (U64P * max(1, K))(*[_p(p) for p in ps])
    _poly(curve, "lincomb")(K, ns, cs, pp, _p(out))
    return out


def poly_is_zero(curve, a):
    a = _fr(a)
    return bool(_poly(curve, "is_zero")(a.shape[0], _p(a)))


def poly_is_equal(curve, a, b):
    a, b = _fr(a), _fr(b)
    return bool(_poly(curve, "is_equal")(a.shape[0], _p(a), b.shape[0], _p(b)))


def poly_degree(curve, a):
    a = _fr(a)
    return int(_poly(curve, "degree")(a.shape[0], _p(a)))


def _long_div(curve, p, d, want_q, want_r):
    p, d = _fr(p), _fr(d)
    require_gpu()
    n1, deg = p.shape[0], poly_degree(curve, d)
    if n1 > (1 << (POLY_MUL_MAX_LOG[curve] - 1)):
        raise ValueError(f"poly_long_div: more than 2^{POLY_MUL_MAX_LOG[curve] - 1} coefficients")
    nq, nr = max(0, n1 - deg), max(0, deg)  # the Haskell sizes (Poly.hs:322-334)
    q = np.zeros((nq, 4), dtype=np.uint64) if want_q else None
    r = np.zeros((nr, 4), dtype=np.uint64) if want_r else None
    rc = load().zkg_poly_long_div(CURVE_ID[curve], n1, _p(p), d.shape[0], _p(d), nq, _p(q) if want_q else None,
                                  nr, _p(r) if want_r else None)
    if rc != 0:
        raise RuntimeError("zkg_poly_long_div refused the call")
    return q, r


def poly_long_div(curve, p, d):
    """Poly.polyLongDiv (Poly.hs:322-334): (quotient, remainder) with p = q * d + r, deg r < deg d, bit-identical
    to the reference's schoolbook loop (zkg_poly_long_div: Newton inversion over the NTT)"""
    return _long_div(curve, p, d, True, True)


def poly_quot(curve, p, d):
    """Poly.polyQuot: the quotient alone (the remainder is not computed)"""
    return _long_div(curve, p, d, True, False)[0]


def poly_rem(curve, p, d):
    """Poly.polyRem: the remainder alone"""
    return _long_div(curve, p, d, False, True)[1]


ARR_OP_CODE = {"neg": 0, "add": 1, "sub": 2, "sub_rev": 3, "sqr": 4, "mul": 5, "mul_add": 6, "mul_sub": 7,
               "scale": 8, "Ax_plus_y": 9, "Ax_plus_By": 10, "from_std": 11, "to_std": 12, "copy": 13,
               "set_const": 14, "inv": 15, "div": 16}


# ----------------------------------------------------------------------------- synthetic inputs

def gen_fr(curve, seed, count, start=0):
    out = np.zeros((count, 4), dtype=np.uint64)
    load().zkg_gen_fr(CURVE_ID[curve], seed, start, count, _p(out))
    return out


def gen_points(curve, seed, count, start=0):
    out = np.zeros((count, 2 * NLIMBS_P[curve]), dtype=np.uint64)
    load().zkg_gen_g1_points(CURVE_ID[curve], seed, start, count, _p(out))
    return out


# ----------------------------------------------------------------------------- device-resident helpers

class DeviceBuffer:
    """HBM buffer owned by the library's allocator (used by bench.py and the multi-GPU path)."""

    def __init__(self, host_array):
        self.nbytes = host_array.nbytes
        self.ptr = load().zkg_device_malloc(max(1, self.nbytes))
        load().zkg_memcpy_htod(self.ptr, host_array.ctypes.data, self.nbytes)

    @classmethod
    def empty(cls, nbytes):
        self = cls.__new__(cls)
        self.nbytes = nbytes
        self.ptr = load().zkg_device_malloc(max(1, nbytes))
        return self

    def to_host(self, like):
        out = np.empty_like(like)
        load().zkg_memcpy_dtoh(out.ctypes.data, self.ptr, self.nbytes)
        return out

    def free(self):
        if self.ptr:
            load().zkg_device_free(self.ptr)
            self.ptr = None


def msm_device(curve, n, d_scalars, d_points, mont=True, window=0, nlimbs=4):
    out = np.zeros(3 * NLIMBS_P[curve], dtype=np.uint64)
    load().zkg_g1_msm_device(CURVE_ID[curve], n, d_scalars.ptr, nlimbs, 1 if mont else 0, d_points.ptr, _p(out),
                             window)
    return out


def g2_msm_device(curve, n, d_scalars, d_points, mont=True, window=0, nlimbs=4):
    """device-resident G2 MSM (zkg_g2_msm_device): the normalised projective row, (0 : 1 : 0) at infinity"""
    out = np.zeros(6 * NLIMBS_P[curve], dtype=np.uint64)
    load().zkg_g2_msm_device(CURVE_ID[curve], n, d_scalars.ptr, nlimbs, 1 if mont else 0, d_points.ptr, _p(out),
                             window)
    return out


def msm_profile(on):
    """per-phase HIP-event timing of every MSM call, printed to stderr"""
    load().zkg_msm_profile(1 if on else 0)


def msm_set_ysum_mode(mode):
    """test hook: G1 Y-sum kernel (-1 by size, 0 k_ysum2, 1 k_ysum3)"""
    load().zkg_msm_set_ysum_mode(int(mode))


def msm_set_ahead_min(lg):
    """test hook: sort-ahead window groups from 2^lg device-resident pairs (0 off, -1 default)"""
    load().zkg_msm_set_ahead_min(int(lg))


def msm_set_group_limit(entries):
    """test hook: max sorted entries per MSM pipeline pass (0 = default 2^30)"""
    load().zkg_msm_set_group_limit(int(entries))


def ntt_set_max_radix(r):
    """test hook: NTT pass split -- 12: two passes for 2^17..2^24, 8: <= 2^8-point passes, 0: default"""
    load().zkg_ntt_set_max_radix(int(r))


def arr_op_device(curve, op, n, d_a, d_b=None, d_c=None, kA=None, kB=None, d_tgt=None):
    """device-resident Fr vector op (zkg_arr_op_device); d_* are DeviceBuffers"""
    z = np.zeros(4, dtype=np.uint64)
    ka = np.ascontiguousarray(kA if kA is not None else z, dtype=np.uint64)
    kb = np.ascontiguousarray(kB if kB is not None else z, dtype=np.uint64)
    load().zkg_arr_op_device(CURVE_ID[curve], ARR_OP_CODE[op], n, d_a.ptr if d_a else None,
                             d_b.ptr if d_b else None, d_c.ptr if d_c else None, _p(ka), _p(kb), d_tgt.ptr)


def arr_dot_device(curve, n, d_a, d_b):
    """device-resident dot product (zkg_arr_dot_device): the Montgomery Fr sum of a_i b_i; d_a may be d_b"""
    out = np.zeros(4, dtype=np.uint64)
    load().zkg_arr_dot_device(CURVE_ID[curve], n, d_a.ptr, d_b.ptr, _p(out))
    return out


def arr_powers_device(curve, n, kA, kB, d_tgt):
    """d_tgt[i] = kA kB^i, i < n (zkg_arr_powers_device); n == 0 writes nothing"""
    load().zkg_arr_powers_device(CURVE_ID[curve], n, _p(_k(kA)), _p(_k(kB)), d_tgt.ptr)


def div_by_vanishing_device(curve, n1, d_src, expo_n, eta, nquot, d_quot, nrem=0, d_rem=None):
    """device-resident division by x^expo_n - eta (zkg_poly_div_by_vanishing_device): nquot / nrem rows are
    written, zero past the quotient's / remainder's length.  With d_rem None the return value is 1 when the
    remainder is zero, else 0 (quot_by_vanishing)."""
    return load().zkg_poly_div_by_vanishing_device(CURVE_ID[curve], n1, d_src.ptr, expo_n, _p(_k(eta)), nquot,
                                                   d_quot.ptr, nrem, d_rem.ptr if d_rem else None)


def batch_to_affine_device(curve, n, d_src, d_tgt, coords="proj"):
    """device-resident batchToAffine (zkg_g1_batch_to_affine_device / zkg_g1_jac_batch_to_affine_device): n rows
    of 3 NP words -> n rows of 2 NP words; distinct buffers"""
    f = load().zkg_g1_batch_to_affine_device if _coords(coords) == "proj" else load().zkg_g1_jac_batch_to_affine_device
    f(CURVE_ID[curve], n, d_src.ptr, d_tgt.ptr)


def g1_fft_device(curve, m, gen, d_src, d_dst, inverse=False):
    """device-resident G1 group FFT: d_src / d_dst are DeviceBuffers of 2^m projective rows"""
    load().zkg_g1_fft_device(CURVE_ID[curve], 1 if inverse else 0, m, _p(np.ascontiguousarray(gen, dtype=np.uint64)),
                             d_src.ptr, d_dst.ptr)


# ----------------------------------------------------------------------------- batch scalar multiplication

def _scl_rc(rc, name):
    if rc != 0:
        raise ValueError(f"{name}: negative length or unknown curve")


def _g1_aff(curve, base, name):
    base = np.ascontiguousarray(base, dtype=np.uint64).reshape(-1)
    if base.shape[0] != 2 * NLIMBS_P[curve]:
        raise ValueError(f"{name}: the base must be one affine G1 point (x, y) in Montgomery form")
    return base


def _scl_out(curve, n, affine):
    return np.zeros((n, (2 if affine else 3) * NLIMBS_P[curve]), dtype=np.uint64)


def scalar_mul_fixed(curve, scalars, base, std=False, affine=False):
    """[k_i] P for one affine base P: map (`scalarMul` p) over a FlatArray of scalars (scl_Fr_mont, or
    scl_Fr_std with std: raw 256-bit integers used verbatim) -> normalised projective rows, or affine"""
    scalars = _fr(scalars)
    require_gpu()
    out = _scl_out(curve, scalars.shape[0], affine)
    _scl_rc(load().zkg_g1_scl_fixed(CURVE_ID[curve], scalars.shape[0], _p(scalars), 0 if std else 1,
                                    _p(_g1_aff(curve, base, "scalar_mul_fixed")), 1 if affine else 0, _p(out)),
            "scalar_mul_fixed")
    return out


def scalar_mul_fixed_device(curve, n, d_scalars, base, d_tgt, std=False, affine=False):
    """device-resident scalar_mul_fixed (zkg_g1_scl_fixed_device): the base stays a host row"""
    return load().zkg_g1_scl_fixed_device(CURVE_ID[curve], n, d_scalars.ptr, 0 if std else 1,
                                          _p(_g1_aff(curve, base, "scalar_mul_fixed")), 1 if affine else 0, d_tgt.ptr)


def scalar_mul_rows(curve, scalars, bases, std=False, affine=False):
    """[k_i] P_i: zipWith scalarMul over n affine rows (all-0xFF rows stay infinity)"""
    scalars = _fr(scalars)
    bases = np.ascontiguousarray(bases, dtype=np.uint64)
    if bases.ndim != 2 or bases.shape != (scalars.shape[0], 2 * NLIMBS_P[curve]):
        raise ValueError("scalar_mul_rows: incompatible array dimensions")
    require_gpu()
    out = _scl_out(curve, scalars.shape[0], affine)
    _scl_rc(load().zkg_g1_scl_rows(CURVE_ID[curve], scalars.shape[0], _p(scalars), 0 if std else 1, _p(bases),
                                   1 if affine else 0, _p(out)), "scalar_mul_rows")
    return out


def scalar_mul_rows_device(curve, n, d_scalars, d_bases, d_tgt, std=False, affine=False):
    """device-resident scalar_mul_rows (zkg_g1_scl_rows_device)"""
    return load().zkg_g1_scl_rows_device(CURVE_ID[curve], n, d_scalars.ptr, 0 if std else 1, d_bases.ptr,
                                         1 if affine else 0, d_tgt.ptr)


def scalar_mul_rows_sum(curve, scalars, bases, std=False, affine=False):
    """sum_j [k_(j,i)] P_(j,i) per row i: scalars (terms, rows, 4) and affine bases (terms, rows, 2 NP), term-major
    (zkg_g1_scl_rows_sum) -> `rows` normalised projective rows, or affine; the fold of scalar_mul_rows with g1_add"""
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
    bases = np.ascontiguousarray(bases, dtype=np.uint64)
    if scalars.ndim != 3 or scalars.shape[2] != NLIMBS_R:
        raise TypeError("scalar_mul_rows_sum: the scalars must have shape (terms, rows, 4)")
    terms, rows = scalars.shape[:2]
    if bases.shape != (terms, rows, 2 * NLIMBS_P[curve]):
        raise ValueError("scalar_mul_rows_sum: incompatible array dimensions")
    require_gpu()
    out = _scl_out(curve, rows, affine)
    _lindiv_rc(load().zkg_g1_scl_rows_sum(CURVE_ID[curve], rows, terms, scalars.ctypes.data, 0 if std else 1,
                                          bases.ctypes.data, 1 if affine else 0, out.ctypes.data),
               "scalar_mul_rows_sum")
    return out


def scalar_mul_rows_sum_device(curve, rows, terms, d_scalars, d_bases, d_tgt, std=False, affine=False):
    """device-resident scalar_mul_rows_sum (zkg_g1_scl_rows_sum_device); returns the code, nonzero for a refused
    call (last_error() has the text)"""
    return load().zkg_g1_scl_rows_sum_device(CURVE_ID[curve], rows, terms, d_scalars.ptr if d_scalars else None,
                                             0 if std else 1, d_bases.ptr if d_bases else None, 1 if affine else 0,
                                             d_tgt.ptr if d_tgt else None)


def srs_powers(curve, tau, n, base, a=None, affine=False):
    """[a tau^i] P, i < n: the `taus` of mkKZGSetup (examples/KZG.hs:59-62); tau, a Montgomery Fr (a None = 1)"""
    require_gpu()
    out = _scl_out(curve, n, affine)
    _scl_rc(load().zkg_g1_scl_powers(CURVE_ID[curve], n, _p(_k(a)) if a is not None else None, _p(_k(tau)),
                                     _p(_g1_aff(curve, base, "srs_powers")), 1 if affine else 0, _p(out)),
            "srs_powers")
    return out


def srs_powers_device(curve, n, tau, base, d_tgt, a=None, affine=False):
    """device-resident srs_powers (zkg_g1_scl_powers_device): the scalars are made on the device"""
    return load().zkg_g1_scl_powers_device(CURVE_ID[curve], n, _p(_k(a)) if a is not None else None, _p(_k(tau)),
                                           _p(_g1_aff(curve, base, "srs_powers")), 1 if affine else 0, d_tgt.ptr)


def scl_set_window(c):
    """test hook: window of the fixed-base table (0 restores the default; clamped to 2..16)"""
    load().zkg_g1_scl_set_window(int(c))


def scl_set_fixed_min(n):
    """test hook: fixed-base calls below n rows take the per-row kernel (< 0 default, 0 never)"""
    load().zkg_g1_scl_set_fixed_min(int(n))


def scl_last_path():
    """0: the most recent fixed-base call ran the per-row kernel; otherwise the window of its table path"""
    return load().zkg_g1_scl_last_path()


def scl_digits(c, k):
    """the fixed-base kernel's signed c-bit recoding of the 256-bit integer k (4 words): a list of
    ceil(257 / c) digits with sum d_w 2^(c w) = k; no GPU call"""
    buf = (ctypes.c_int * 129)()
    w = load().zkg_g1_scl_digits(int(c), _p(_k(k)), buf, 129)
    if w < 0:
        raise ValueError("scl_digits: the window must be in 2..16")
    return list(buf[:w])


def scl_table_bytes(curve, c):
    """bytes of the fixed-base table for window c; no GPU call"""
    return load().zkg_g1_scl_table_bytes(CURVE_ID[curve], int(c))


def _g2_aff(curve, base, name):
    base = np.ascontiguousarray(base, dtype=np.uint64).reshape(-1)
    if base.shape[0] != 4 * NLIMBS_P[curve]:
        raise ValueError(f"{name}: the base must be one affine G2 point (x.c0, x.c1, y.c0, y.c1) in Montgomery form")
    return base


def _g2_scl_out(curve, n, affine):
    return np.zeros((n, (4 if affine else 6) * NLIMBS_P[curve]), dtype=np.uint64)


def g2_scalar_mul_fixed(curve, scalars, base, std=False, affine=False):
    """scalar_mul_fixed on G2: [k_i] P for one affine G2 base (4 NLIMBS_P words; G2_proj_scl_Fr_mont, or
    _scl_Fr_std with std) -> normalised projective rows (6 NLIMBS_P words), or affine (4 NLIMBS_P).  The
    integer value of the scalar, no reduction mod r; bases outside the subgroup allowed."""
    scalars = _fr(scalars)
    base = _g2_aff(curve, base, "g2_scalar_mul_fixed")
    require_gpu()
    out = _g2_scl_out(curve, scalars.shape[0], affine)
    _scl_rc(load().zkg_g2_scl_fixed(CURVE_ID[curve], scalars.shape[0], _p(scalars), 0 if std else 1, _p(base),
                                    1 if affine else 0, _p(out)), "g2_scalar_mul_fixed")
    return out


def g2_scalar_mul_fixed_device(curve, n, d_scalars, base, d_tgt, std=False, affine=False):
    """device-resident g2_scalar_mul_fixed (zkg_g2_scl_fixed_device): the base stays a host row"""
    return load().zkg_g2_scl_fixed_device(CURVE_ID[curve], n, d_scalars.ptr, 0 if std else 1,
                                          _p(_g2_aff(curve, base, "g2_scalar_mul_fixed")), 1 if affine else 0,
                                          d_tgt.ptr)


def g2_scalar_mul_rows(curve, scalars, bases, std=False, affine=False):
    """[k_i] P_i on G2: n affine rows (all-0xFF rows stay infinity)"""
    scalars = _fr(scalars)
    bases = np.ascontiguousarray(bases, dtype=np.uint64)
    if bases.ndim != 2 or bases.shape != (scalars.shape[0], 4 * NLIMBS_P[curve]):
        raise ValueError("g2_scalar_mul_rows: incompatible array dimensions")
    require_gpu()
    out = _g2_scl_out(curve, scalars.shape[0], affine)
    _scl_rc(load().zkg_g2_scl_rows(CURVE_ID[curve], scalars.shape[0], _p(scalars), 0 if std else 1, _p(bases),
                                   1 if affine else 0, _p(out)), "g2_scalar_mul_rows")
    return out


def g2_scalar_mul_rows_device(curve, n, d_scalars, d_bases, d_tgt, std=False, affine=False):
    """device-resident g2_scalar_mul_rows (zkg_g2_scl_rows_device)"""
    return load().zkg_g2_scl_rows_device(CURVE_ID[curve], n, d_scalars.ptr, 0 if std else 1, d_bases.ptr,
                                         1 if affine else 0, d_tgt.ptr)


def g2_srs_powers(curve, tau, n, base, a=None, affine=False):
    """[a tau^i] P, i < n, on G2 (a multi-point opening key, a Groth16 G2 column); tau, a Montgomery Fr (a None = 1)"""
    base = _g2_aff(curve, base, "g2_srs_powers")
    require_gpu()
    out = _g2_scl_out(curve, n, affine)
    _scl_rc(load().zkg_g2_scl_powers(CURVE_ID[curve], n, _p(_k(a)) if a is not None else None, _p(_k(tau)), _p(base),
                                     1 if affine else 0, _p(out)), "g2_srs_powers")
    return out


def g2_srs_powers_device(curve, n, tau, base, d_tgt, a=None, affine=False):
    """device-resident g2_srs_powers (zkg_g2_scl_powers_device): the scalars are made on the device"""
    return load().zkg_g2_scl_powers_device(CURVE_ID[curve], n, _p(_k(a)) if a is not None else None, _p(_k(tau)),
                                           _p(_g2_aff(curve, base, "g2_srs_powers")), 1 if affine else 0, d_tgt.ptr)


def g2_scl_set_window(c):
    """test hook: window of the G2 fixed-base table (0 restores the default; clamped to 2..16)"""
    load().zkg_g2_scl_set_window(int(c))


def g2_scl_set_fixed_min(n):
    """test hook: G2 fixed-base calls below n rows take the per-row kernel (< 0 default, 0 never)"""
    load().zkg_g2_scl_set_fixed_min(int(n))


def g2_scl_last_path():
    """0: the most recent G2 fixed-base call ran the per-row kernel; otherwise the window of its table path"""
    return load().zkg_g2_scl_last_path()


def g2_scl_table_bytes(curve, c):
    """bytes of the G2 fixed-base table for window c; no GPU call"""
    return load().zkg_g2_scl_table_bytes(CURVE_ID[curve], int(c))


@dataclass
class KZGSetup:
    """Mirror of examples/KZG.hs KZGSetup: the point arrays stay on the device (projective rows);
    tau_g2s ([tau^i] g2, i < g2_powers) only when kzg_setup was asked for it.  The affine rows the MSM
    takes are made from the projective ones on first use (affine_rows) and kept until free()."""
    domain: FFTSubgroup
    tau_g1s: "DeviceBuffer"
    lagrange_taus: "DeviceBuffer"
    g2_tau_g2: tuple
    tau_g2s: "DeviceBuffer" = None
    _affine: dict = None
    _open_all: dict = None

    def open_all_table(self, log_n, coset_log):
        """the device table of kzg_open_all for (log_n, coset_log), built on first use (zkg_kzg_open_all_table_device)
        and kept until free()"""
        if self._open_all is None:
            self._open_all = {}
        key = (int(log_n), int(coset_log))
        if key not in self._open_all:
            cid = CURVE_ID[self.domain.curve]
            buf = DeviceBuffer.empty(load().zkg_kzg_open_all_table_bytes(cid, *key))
            try:
                _lindiv_rc(load().zkg_kzg_open_all_table_device(cid, key[0], key[1], self.affine_rows("tau_g1s").ptr,
                                                                buf.ptr), "kzg_open_all")
            except Exception:
                buf.free()
                raise
            self._open_all[key] = buf
        return self._open_all[key]

    def affine_rows(self, which):
        """the device buffer of affine rows of `which` ('tau_g1s' or 'lagrange_taus'), made once"""
        if self._affine is None:
            self._affine = {}
        if which not in self._affine:
            curve, n = self.domain.curve, self.domain.size
            buf = DeviceBuffer.empty(n * 2 * NLIMBS_P[curve] * 8)
            try:
                batch_to_affine_device(curve, n, getattr(self, which), buf)
            except Exception:
                buf.free()
                raise
            self._affine[which] = buf
        return self._affine[which]

    def free(self):
        self.tau_g1s.free()
        self.lagrange_taus.free()
        if self.tau_g2s is not None:
            self.tau_g2s.free()
        for b in list((self._affine or {}).values()) + list((self._open_all or {}).values()):
            b.free()
        self._affine = None
        self._open_all = None


def kzg_setup(curve, tau, log_size, g1, g2, g2_powers=0):
    """mkKZGSetup (examples/KZG.hs:42-62): tauG1s = [tau^i] g1 (srs_powers), lagrangeTaus = curveIFFT of it
    (the device group FFT reads the first buffer where it lies) and (g2, tau g2) by the G2 MSM of one pair;
    g1 affine G1, g2 affine G2, tau Montgomery Fr.  g2_powers = k > 0: also tau_g2s, the k projective rows
    [tau^i] g2 on the device (g2_srs_powers)."""
    require_gpu()
    dom = get_fft_subgroup(curve, log_size)
    n = dom.size
    nbytes = n * 3 * NLIMBS_P[curve] * 8
    bufs = [DeviceBuffer.empty(nbytes), DeviceBuffer.empty(nbytes)]
    taus, lag = bufs
    try:
        _scl_rc(srs_powers_device(curve, n, tau, g1, taus), "kzg_setup")
        g1_fft_device(curve, log_size, dom.gen_array(), taus, lag, inverse=True)
        g2 = np.ascontiguousarray(g2, dtype=np.uint64).reshape(1, -1)
        tau_g2 = g2_msm(curve, _k(tau).reshape(1, 4), g2)
        tau_g2s = None
        if g2_powers > 0:
            tau_g2s = DeviceBuffer.empty(g2_powers * 6 * NLIMBS_P[curve] * 8)
            bufs.append(tau_g2s)
            _scl_rc(g2_srs_powers_device(curve, g2_powers, tau, g2, tau_g2s), "kzg_setup")
    except Exception:
        for b in bufs:
            b.free()
        raise
    return KZGSetup(dom, taus, lag, (g2.reshape(-1), tau_g2), tau_g2s)


# ---------------------------------------------------------------------------- KZG prover
# division by x - z (zk_lindiv.hip) and examples/KZG.hs commitPoly / commitValues / commitInterpolate / openingProof

def _lindiv_rc(rc, name):
    if rc != 0:
        raise ValueError(f"{name}: the call was refused ({last_error() or 'bad arguments'})")


def _points(z):
    """(rows (nz, 4), single) of one point or an (nz, 4) array of points"""
    z = np.ascontiguousarray(z, dtype=np.uint64)
    single = z.ndim == 1
    rows = z.reshape(1, -1) if single else z
    if rows.ndim != 2 or rows.shape[1] != NLIMBS_R:
        raise TypeError("a point is one Fr element (4 words), or an (nz, 4) array of them")
    return rows, single


def poly_div_linear(curve, poly, z):
    """the quotient of poly by x - z and the value poly(z), what quot_by_vanishing(poly - val, 1, z) and
    poly_eval_at give, in one sweep (zkg_poly_div_linear).  One point: (quot (n - 1, 4), val (4,)); an (nz, 4)
    array of points: (quot (nz, n - 1, 4), vals (nz, 4)).  n - 1 rows always (zero above the quotient's degree)."""
    poly = _fr(poly)
    zs, single = _points(z)
    n, nz = poly.shape[0], zs.shape[0]
    require_gpu()
    quot = np.zeros((nz, max(0, n - 1), 4), dtype=np.uint64)
    vals = np.zeros((nz, 4), dtype=np.uint64)
    _lindiv_rc(load().zkg_poly_div_linear(CURVE_ID[curve], n, poly.ctypes.data, nz, zs.ctypes.data, quot.ctypes.data,
                                          vals.ctypes.data), "poly_div_linear")
    return (quot[0], vals[0]) if single else (quot, vals)


def poly_div_linear_device(curve, n, d_poly, z, d_quot=None):
    """device-resident poly_div_linear (zkg_poly_div_linear_device): d_quot receives nz x (n - 1) rows (None:
    the values alone) and does not overlap d_poly; returns (rc, vals (nz, 4)), rc nonzero for a refused call
    (last_error() has the text)"""
    zs, _ = _points(z)
    vals = np.zeros((zs.shape[0], 4), dtype=np.uint64)
    rc = load().zkg_poly_div_linear_device(CURVE_ID[curve], n, d_poly.ptr if d_poly else None, zs.shape[0],
                                           zs.ctypes.data, d_quot.ptr if d_quot else None, vals.ctypes.data)
    return rc, vals


def poly_set_lindiv_tile(rows_per_lane):
    """test hook: rows per lane of a tile of the division's scan (1, 2, 4 or 8; 0 restores the default)"""
    load().zkg_poly_set_lindiv_tile(int(rows_per_lane))


def poly_lindiv_tile():
    """rows per lane in force: a tile is 256 times as many rows"""
    return load().zkg_poly_lindiv_tile()


def _g1_out(curve, proj, affine):
    return g1_to_affine(curve, proj) if affine else proj


def _kzg_commit(setup, coeffs, which, name, affine):
    curve = setup.domain.curve
    n = coeffs.shape[0]
    require_gpu()
    d_c = DeviceBuffer(coeffs)
    try:
        out = np.zeros(3 * NLIMBS_P[curve], dtype=np.uint64)
        _lindiv_rc(load().zkg_kzg_commit_device(CURVE_ID[curve], n, d_c.ptr, setup.affine_rows(which).ptr,
                                                out.ctypes.data), name)
    finally:
        d_c.free()
    return _g1_out(curve, out, affine)


def kzg_commit(setup, poly, affine=False):
    """commitPoly (examples/KZG.hs:85-89): msm of the coefficients against the first len(poly) rows of tauG1s;
    the normalised projective row, or the affine one"""
    poly = _fr(poly)
    if poly.shape[0] > setup.domain.size:
        raise ValueError("kzg_commit: the polynomial is longer than the KZG setup")
    return _kzg_commit(setup, poly, "tau_g1s", "kzg_commit", affine)


def kzg_commit_values(setup, values, affine=False):
    """commitValues (examples/KZG.hs:91-98): msm of the values against lagrangeTaus"""
    values = _fr(values)
    if values.shape[0] != setup.domain.size:
        raise ValueError("commitValues: expecting a vector of the same size as the KZG setup domain")
    return _kzg_commit(setup, values, "lagrange_taus", "kzg_commit_values", affine)


def kzg_commit_interpolate(setup, values, affine=False):
    """commitInterpolate (examples/KZG.hs:100-107): commitPoly of the interpolated polynomial"""
    values = _fr(values)
    if values.shape[0] != setup.domain.size:
        raise ValueError("commitInterpolate: expecting a vector of the same size as the KZG setup domain")
    return kzg_commit(setup, inverse_ntt(setup.domain, values), affine=affine)


def kzg_open_many(setup, poly, zs, affine=False):
    """openingProof at every row of zs (nz, 4): (vals (nz, 4), proofs (nz, 3 NP) normalised projective, or
    (nz, 2 NP) affine) -- zkg_kzg_open_device: per point the division by x - z, then the device MSM"""
    poly = _fr(poly)
    zs, _ = _points(zs)
    curve, n, nz = setup.domain.curve, poly.shape[0], zs.shape[0]
    if n > setup.domain.size:
        raise ValueError("kzg_open: the polynomial is longer than the KZG setup")
    require_gpu()
    NP = NLIMBS_P[curve]
    vals = np.zeros((nz, 4), dtype=np.uint64)
    proofs = np.zeros((nz, 3 * NP), dtype=np.uint64)
    d_p = DeviceBuffer(poly)
    try:
        _lindiv_rc(load().zkg_kzg_open_device(CURVE_ID[curve], n, d_p.ptr, setup.affine_rows("tau_g1s").ptr, nz,
                                              zs.ctypes.data, vals.ctypes.data, proofs.ctypes.data), "kzg_open")
    finally:
        d_p.free()
    if affine:
        proofs = np.stack([g1_to_affine(curve, p) for p in proofs]) if nz else np.zeros((0, 2 * NP), dtype=np.uint64)
    return vals, proofs


def kzg_open(setup, poly, z, affine=False):
    """openingProof (examples/KZG.hs:120-127): (z, val, proof) with val = poly(z) and proof the commitment to
    (poly - val) / (x - z); a polynomial of length <= 1 gives the point at infinity"""
    z = _k(z)
    vals, proofs = kzg_open_many(setup, poly, z.reshape(1, 4), affine=affine)
    return z, vals[0], proofs[0]


# ---------------------------------------------------------------------------- all openings (FK20)
# zk_fk20.hip: the proofs of a whole domain from one Toeplitz product; DESIGN.md "All openings (FK20)"

def fk20_coeff_index(r, p):
    """row p < 2r of the circulant column c^(j) holds F^(j)_v, F^(j)_v = f_(l v + j); -1: zero (zk_fk20.hpp)"""
    return r - 1 if p == 0 else (p - r - 1 if p >= r + 2 else -1)


def fk20_srs_index(r, p):
    """row p < 2r of x^(j) holds S^(j)_u, S^(j)_u = s_(l u + j); -1: the point at infinity (zk_fk20.hpp)"""
    return r - 2 - p if p <= r - 2 else -1


def _open_all_shape(setup, npoly, log_n, coset_log):
    """(m, c) of a kzg_open_all call, or ValueError; no GPU call"""
    m = setup.domain.log_size if log_n is None else int(log_n)
    c = int(coset_log)
    if m > setup.domain.log_size:
        raise ValueError("kzg_open_all: the domain is larger than the KZG setup")
    if m < 1:
        raise ValueError("kzg_open_all: the domain has at least two points")
    if npoly > 1 << m:
        raise ValueError("kzg_open_all: the polynomial is longer than the domain")
    if not 0 <= c <= m - 1:
        raise ValueError("kzg_open_all: the coset size 2^coset_log must leave at least two cosets")
    return m, c


def kzg_open_all(setup, poly, log_n=None, coset_log=0, affine=False):
    """every opening of the domain of size n = 2^log_n (default: the setup's) at once: (values (n, 4), proofs).
    values = forward_ntt of the zero-extended polynomial, natural order.  With l = 2^coset_log and r = n / l,
    proofs has r rows (normalised projective, or affine): row k commits to the quotient of poly by
    x^l - omega^(l k) and opens the coset omega^k <omega^r>, the values k, k + r, ..; for l = 1 it is
    kzg_open(setup, poly, omega^k).  The per-setup table is built on first use (KZGSetup.open_all_table)."""
    poly = _fr(poly)
    curve = setup.domain.curve
    m, c = _open_all_shape(setup, poly.shape[0], log_n, coset_log)
    require_gpu()
    n, NP = 1 << m, NLIMBS_P[curve]
    ext = np.zeros((n, 4), dtype=np.uint64)
    ext[:poly.shape[0]] = poly
    values = forward_ntt(get_fft_subgroup(curve, m), ext)
    table = setup.open_all_table(m, c)
    proofs = np.zeros((n >> c, (2 if affine else 3) * NP), dtype=np.uint64)
    d_p, d_out = DeviceBuffer(poly), DeviceBuffer.empty(proofs.nbytes)
    try:
        _lindiv_rc(load().zkg_kzg_open_all_device(CURVE_ID[curve], m, c, poly.shape[0], d_p.ptr if poly.shape[0] else None,
                                                  table.ptr, 1 if affine else 0, d_out.ptr), "kzg_open_all")
        proofs = d_out.to_host(proofs)
    finally:
        d_p.free()
        d_out.free()
    return values, proofs


# ---------------------------------------------------------------------------- pairings
# <C>_pairing_affine / _projective / _final_expo (lib/cbits/curves/pairing); Pairing.hs `pairing`

FIELD_P = {
    "bn128": 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47,
    "bls12_381": 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB,
}


def _pair_rows(curve, P, Q, name, wp=2, wq=4):
    """(P, Q, single): n rows of wp NP and wq NP words, or one row each"""
    NP = NLIMBS_P[curve]
    P = np.ascontiguousarray(P, dtype=np.uint64)
    Q = np.ascontiguousarray(Q, dtype=np.uint64)
    single = P.ndim == 1 and Q.ndim == 1
    if single:
        P, Q = P.reshape(1, -1), Q.reshape(1, -1)
    if P.ndim != 2 or Q.ndim != 2 or P.shape[1] != wp * NP or Q.shape[1] != wq * NP or P.shape[0] != Q.shape[0]:
        raise ValueError(f"{name}: incompatible array dimensions")
    return P, Q, single


def _pair_rc(rc, name):
    if rc != 0:
        raise ValueError(f"{name}: the call was refused ({last_error() or 'bad arguments'})")


def fp12_one(curve):
    """the Montgomery one of Fp12 as a row of 12 NP words; no GPU call"""
    NP = NLIMBS_P[curve]
    out = np.zeros(12 * NP, dtype=np.uint64)
    v = (1 << (64 * NP)) % FIELD_P[curve]
    out[:NP] = [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(NP)]
    return out


def pairing(curve, P, Q):
    """the optimal-ate pairing of affine G1 rows (2 NP words) and affine G2 rows (4 NP words): one pair, or n
    pairs -> (n, 12 NP); row i equals <C>_pairing_affine(P_i, Q_i), an infinite P or Q gives one.  The rows are
    points of the order-r subgroups (or infinity); nothing is checked."""
    P, Q, single = _pair_rows(curve, P, Q, "pairing")
    require_gpu()
    out = np.zeros((P.shape[0], 12 * NLIMBS_P[curve]), dtype=np.uint64)
    _pair_rc(load().zkg_pairing_rows(CURVE_ID[curve], P.shape[0], _p(P), _p(Q), _p(out)), "pairing")
    return out[0] if single else out


def pairing_device(curve, n, d_P, d_Q, d_tgt):
    """device-resident pairing (zkg_pairing_rows_device)"""
    return load().zkg_pairing_rows_device(CURVE_ID[curve], n, d_P.ptr if d_P else None, d_Q.ptr if d_Q else None,
                                          d_tgt.ptr if d_tgt else None)


def pairing_projective(curve, P, Q):
    """<C>_pairing_projective: one projective G1 point (3 NP words) and one projective G2 point (6 NP words)"""
    P, Q, _ = _pair_rows(curve, np.asarray(P).reshape(-1), np.asarray(Q).reshape(-1), "pairing_projective", 3, 6)
    require_gpu()
    out = np.zeros(12 * NLIMBS_P[curve], dtype=np.uint64)
    getattr(load(), f"{curve}_pairing_projective")(_p(P), _p(Q), _p(out))
    return out


def pairing_product(curve, P, Q):
    """prod_i pairing(P_i, Q_i) as one Fp12 row, with a single final exponentiation (no rows: one)"""
    P, Q, _ = _pair_rows(curve, P, Q, "pairing_product")
    require_gpu()
    out = np.zeros(12 * NLIMBS_P[curve], dtype=np.uint64)
    _pair_rc(load().zkg_pairing_product(CURVE_ID[curve], P.shape[0], _p(P), _p(Q), _p(out)), "pairing_product")
    return out


def pairing_product_device(curve, n, d_P, d_Q, d_tgt):
    """device-resident pairing_product (zkg_pairing_product_device): d_tgt receives one Fp12 row"""
    return load().zkg_pairing_product_device(CURVE_ID[curve], n, d_P.ptr if d_P else None, d_Q.ptr if d_Q else None,
                                             d_tgt.ptr if d_tgt else None)


def pairing_check(curve, P, Q):
    """prod_i pairing(P_i, Q_i) == 1"""
    return bool(np.array_equal(pairing_product(curve, P, Q), fp12_one(curve)))


def final_expo(curve, src):
    """x^((p^12 - 1)/r) per Fp12 row (<C>_pairing_final_expo); one row or (n, 12 NP)"""
    src = np.ascontiguousarray(src, dtype=np.uint64)
    single = src.ndim == 1
    rows = src.reshape(1, -1) if single else src
    if rows.ndim != 2 or rows.shape[1] != 12 * NLIMBS_P[curve]:
        raise ValueError("final_expo: incompatible array dimensions")
    require_gpu()
    out = np.zeros_like(rows)
    _pair_rc(load().zkg_pairing_final_expo(CURVE_ID[curve], rows.shape[0], _p(rows), _p(out)), "final_expo")
    return out[0] if single else out


def final_expo_device(curve, n, d_src, d_tgt):
    """device-resident final_expo (zkg_pairing_final_expo_device)"""
    return load().zkg_pairing_final_expo_device(CURVE_ID[curve], n, d_src.ptr if d_src else None,
                                                d_tgt.ptr if d_tgt else None)


def _g1_neg_proj(curve, pt):
    """-(X : Y : Z): Y -> p - Y on the canonical Montgomery words"""
    NP = NLIMBS_P[curve]
    out = np.array(pt, dtype=np.uint64)
    y = sum(int(out[NP + j]) << (64 * j) for j in range(NP))
    y = (FIELD_P[curve] - y) % FIELD_P[curve]
    out[NP:2 * NP] = [(y >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(NP)]
    return out


def kzg_verify(curve, g1, g2, tau_g2, commitment, x0, y0, proof, validate=False):
    """verifyProof (examples/KZG.hs:120-124): pairing(proof, tau g2) == pairing(point, g2) with
    point = commitment + [x0] proof - [y0] g1, evaluated as the two-row product
    pairing(proof, tau g2) pairing(-point, g2) == 1.  g1 affine G1, g2 / tau_g2 affine G2, commitment and
    proof projective G1 rows (what msm returns), x0 / y0 Montgomery Fr.  validate: the commitment, the proof
    and tau_g2 are checked first (g1_all_valid / g2_all_valid: canonical, on the curve, in the subgroup) and
    an invalid point returns False; without it nothing is checked, as before."""
    NP = NLIMBS_P[curve]
    g1 = _g1_aff(curve, g1, "kzg_verify")
    g2 = np.ascontiguousarray(g2, dtype=np.uint64).reshape(-1)
    tau_g2 = np.ascontiguousarray(tau_g2, dtype=np.uint64).reshape(-1)
    commitment = np.ascontiguousarray(commitment, dtype=np.uint64).reshape(-1)
    proof = np.ascontiguousarray(proof, dtype=np.uint64).reshape(-1)
    if g2.shape[0] != 4 * NP or tau_g2.shape[0] != 4 * NP or commitment.shape[0] != 3 * NP or proof.shape[0] != 3 * NP:
        raise ValueError("kzg_verify: incompatible array dimensions")
    x0, y0 = _k(x0), _k(y0)
    require_gpu()
    if validate and not (g1_all_valid(curve, np.stack([commitment, proof]), coords="proj")
                         and g2_all_valid(curve, tau_g2.reshape(1, -1))):
        return False
    proof_aff = g1_to_affine(curve, proof)
    xq = scalar_mul_rows(curve, x0.reshape(1, 4), proof_aff.reshape(1, -1))[0]
    yg = scalar_mul_fixed(curve, y0.reshape(1, 4), g1)[0]
    point = g1_add(curve, g1_add(curve, commitment, xq), _g1_neg_proj(curve, yg))
    neg_aff = g1_to_affine(curve, _g1_neg_proj(curve, point))
    return pairing_check(curve, np.stack([proof_aff, neg_aff]), np.stack([tau_g2, g2]))


def kzg_verify_coset(curve, g1, g2, tau_l_g2, commitment, shift, values_l, proof):
    """the multi-reveal check of one kzg_open_all proof with l = len(values_l) = 2^c: values_l[i] =
    f(shift gen_l^i), gen_l the generator of get_fft_subgroup(curve, c) (row k of the proofs: shift = omega^k,
    values_l = values[k::r]).  With I the interpolation of the values on the coset (coset_intt) it holds when
    pairing(proof, [tau^l] g2 - [shift^l] g2) == pairing(commitment - [I(tau)] g1, g2).  Composition only:
    g1: the affine G1 rows [tau^i] g1, i < l (at least l of them; row 0 is the generator), for the commitment to I;
    g2, tau_l_g2 = [tau^l] g2: affine G2 (kzg_setup(.., g2_powers > l) has the latter); commitment and proof
    projective G1 rows; shift Montgomery Fr."""
    NP = NLIMBS_P[curve]
    values_l = _fr(values_l)
    l = values_l.shape[0]
    c = l.bit_length() - 1
    g1 = np.ascontiguousarray(g1, dtype=np.uint64)
    g2 = np.ascontiguousarray(g2, dtype=np.uint64).reshape(-1)
    tau_l_g2 = np.ascontiguousarray(tau_l_g2, dtype=np.uint64).reshape(-1)
    commitment = np.ascontiguousarray(commitment, dtype=np.uint64).reshape(-1)
    proof = np.ascontiguousarray(proof, dtype=np.uint64).reshape(-1)
    if l < 1 or l != 1 << c:
        raise ValueError("kzg_verify_coset: the number of values is a power of two")
    if g1.ndim != 2 or g1.shape[1] != 2 * NP or g1.shape[0] < l:
        raise ValueError("kzg_verify_coset: g1 must hold the affine rows [tau^i] g1, i < l")
    if g2.shape[0] != 4 * NP or tau_l_g2.shape[0] != 4 * NP or commitment.shape[0] != 3 * NP or proof.shape[0] != 3 * NP:
        raise ValueError("kzg_verify_coset: incompatible array dimensions")
    shift = _k(shift)
    require_gpu()
    r = FR_ORDER[curve]
    s = sum(int(shift[j]) << (64 * j) for j in range(4)) * pow(1 << 256, -1, r) % r
    interp = coset_intt(get_fft_subgroup(curve, c), shift, values_l)
    i_tau = msm(curve, interp, np.ascontiguousarray(g1[:l]))
    point = g1_add(curve, commitment, _g1_neg_proj(curve, i_tau))
    neg_aff = g1_to_affine(curve, _g1_neg_proj(curve, point))
    coeffs = np.stack([_fr_mont(curve, 1), _fr_mont(curve, -pow(s, l, r))])
    d = g2_msm(curve, coeffs, np.stack([tau_l_g2, g2]), affine=True)
    return pairing_check(curve, np.stack([g1_to_affine(curve, proof), neg_aff]), np.stack([d, g2]))


# ---------------------------------------------------------------------------- point validation
# zkg_g{1,2}_check_rows: per row PT_CANONICAL | PT_ON_CURVE | PT_IN_SUBGROUP | PT_INFINITY.  ON_CURVE and
# INFINITY are the reference's <C>_G{1,2}_{affine,proj,jac}_is_on_curve / _is_infinity; IN_SUBGROUP is
# [r]P = O, not the reference's _is_in_subgroup (which multiplies by the cofactor and rejects the generator).

def _check_rows(curve, pts, coords, group, name):
    """(rows, coords id) of a G1 (group 1) or G2 (group 2) point array in coordinate system `coords`"""
    if coords not in COORDS_ID or (group == 2 and coords == "jac"):
        raise ValueError(f"{name}: coords must be 'affine', 'proj'" + (" or 'jac'" if group == 1 else ""))
    pts = np.ascontiguousarray(pts, dtype=np.uint64)
    words = (2 if coords == "affine" else 3) * group * NLIMBS_P[curve]
    if pts.ndim != 2 or pts.shape[1] != words:
        raise ValueError(f"{name}: incompatible array dimensions ({coords} rows have {words} words)")
    return pts, COORDS_ID[coords]


def _check_rc(rc, name):
    if rc < 0:
        raise ValueError(f"{name}: the call was refused ({last_error() or 'bad arguments'})")
    return rc


def _check_host(curve, pts, coords, group, name, want_flags):
    pts, cid = _check_rows(curve, pts, coords, group, name)
    require_gpu()
    flags = np.zeros(pts.shape[0], dtype=np.uint8) if want_flags else None
    f = getattr(load(), f"zkg_g{group}_check_rows")
    rc = _check_rc(f(CURVE_ID[curve], pts.shape[0], pts.ctypes.data, cid, flags.ctypes.data if want_flags else None),
                   name)
    return flags if want_flags else rc


def g1_check(curve, pts, coords="affine"):
    """one flag byte per G1 row (PT_*): affine rows of 2 NP words, 'proj' / 'jac' rows of 3 NP words"""
    return _check_host(curve, pts, coords, 1, "g1_check", True)


def g2_check(curve, pts, coords="affine"):
    """one flag byte per G2 row (PT_*): affine rows of 4 NP words, 'proj' rows of 6 NP words"""
    return _check_host(curve, pts, coords, 2, "g2_check", True)


def g1_all_valid(curve, pts, coords="affine"):
    """every row is canonical, on the curve and in the order-r subgroup (the count-only call; infinity passes)"""
    return _check_host(curve, pts, coords, 1, "g1_all_valid", False) == 0


def g2_all_valid(curve, pts, coords="affine"):
    return _check_host(curve, pts, coords, 2, "g2_all_valid", False) == 0


def _check_device(curve, n, d_pts, coords, d_flags, group, name):
    if coords not in COORDS_ID or (group == 2 and coords == "jac"):
        raise ValueError(f"{name}: coords must be 'affine', 'proj'" + (" or 'jac'" if group == 1 else ""))
    f = getattr(load(), f"zkg_g{group}_check_rows_device")
    return f(CURVE_ID[curve], n, d_pts.ptr if d_pts else None, COORDS_ID[coords], d_flags.ptr if d_flags else None)


def g1_check_device(curve, n, d_pts, d_flags=None, coords="affine"):
    """device-resident g1_check (zkg_g1_check_rows_device): n flag bytes into d_flags (None: the count alone);
    returns the number of invalid rows, or -1"""
    return _check_device(curve, n, d_pts, coords, d_flags, 1, "g1_check_device")


def g2_check_device(curve, n, d_pts, d_flags=None, coords="affine"):
    """device-resident g2_check (zkg_g2_check_rows_device)"""
    return _check_device(curve, n, d_pts, coords, d_flags, 2, "g2_check_device")


def check_set_mode(mode):
    """test hook: 0 the default membership chains, 1 the exact chain [r]P everywhere, 2 the curve pass alone
    (measurement: finite rows then count as failing), < 0 restores the default"""
    load().zkg_check_set_mode(int(mode))


def check_set_max_lanes(lanes):
    """test hook: lanes of the membership kernel (its grid-stride loop at small n); <= 0 restores the default"""
    load().zkg_check_set_max_lanes(int(lanes))


@dataclass
class SRSCheck:
    """result of srs_check: ok, or the first failed stage ("points", "g1 powers", "g2 powers")"""
    ok: bool
    failed: str = None

    def __bool__(self):
        return self.ok


def _fr_mont(curve, v):
    """the Montgomery words of the integer v mod r"""
    r = FR_ORDER[curve]
    v = (v % r) * (1 << 256) % r
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


FR_ORDER = {
    "bn128": 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001,
    "bls12_381": 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
}


def srs_check(curve, g1_powers, g2_powers, rho=None):
    """Is (P_0 .. P_{n-1}; Q_0 .. Q_{k-1}) a powers-of-tau SRS, P_i = [tau^i] P_0 and Q_j = [tau^j] Q_0?  What a
    prover runs on a ceremony file before it commits with it.  g1_powers: n affine (2 NP words) or projective
    (3 NP) G1 rows; g2_powers: k >= 2 affine (4 NP) or projective (6 NP) G2 rows; rho: the random challenge, an
    integer (default: drawn with `secrets`).
      "points"     every row of both columns is canonical, on its curve, in the subgroup and not infinity
      "g1 powers"  e(sum rho^i P_i, Q_1) == e(sum rho^i P_{i+1}, Q_0) over i < n - 1 (two MSMs, one pairing product)
      "g2 powers"  with k > 2: e(P_1, sum rho^j Q_j) == e(P_0, sum rho^j Q_{j+1}) over j < k - 1
    Returns SRSCheck(ok, failed): truthy on success, else `failed` names the first stage that did not hold."""
    NP = NLIMBS_P[curve]
    g1_powers = np.ascontiguousarray(g1_powers, dtype=np.uint64)
    g2_powers = np.ascontiguousarray(g2_powers, dtype=np.uint64)
    if g1_powers.ndim != 2 or g1_powers.shape[1] not in (2 * NP, 3 * NP) or g1_powers.shape[0] < 1:
        raise ValueError("srs_check: g1_powers must be affine or projective G1 rows")
    if g2_powers.ndim != 2 or g2_powers.shape[1] not in (4 * NP, 6 * NP) or g2_powers.shape[0] < 2:
        raise ValueError("srs_check: g2_powers must be at least two affine or projective G2 rows")
    c1 = "affine" if g1_powers.shape[1] == 2 * NP else "proj"
    c2 = "affine" if g2_powers.shape[1] == 4 * NP else "proj"
    require_gpu()
    for flags in (g1_check(curve, g1_powers, c1), g2_check(curve, g2_powers, c2)):
        if np.any((flags & PT_VALID) != PT_VALID) or np.any(flags & PT_INFINITY):
            return SRSCheck(False, "points")
    if rho is None:
        import secrets
        rho = secrets.randbelow(FR_ORDER[curve] - 2) + 2
    P = g1_powers if c1 == "affine" else batch_to_affine(curve, g1_powers)
    Q = g2_powers if c2 == "affine" else g2_batch_to_affine(curve, g2_powers)
    n, k = P.shape[0], Q.shape[0]
    pw = arr_powers(curve, _fr_mont(curve, 1), _fr_mont(curve, rho), max(n, k) - 1) if max(n, k) > 1 else None

    def neg1(aff):  # -(x, y) of an affine G1 row (all-0xFF stays infinity)
        return g1_to_affine(curve, _g1_neg_proj(curve, batch_from_affine(curve, aff.reshape(1, -1))[0]))
    if n > 1:
        a = msm_affine(curve, pw[:n - 1], np.ascontiguousarray(P[:n - 1]))
        b = msm_affine(curve, pw[:n - 1], np.ascontiguousarray(P[1:]))
        if not pairing_check(curve, np.stack([a, neg1(b)]), np.stack([Q[1], Q[0]])):
            return SRSCheck(False, "g1 powers")
    if k > 2 and n > 1:
        sa = g2_msm(curve, pw[:k - 1], np.ascontiguousarray(Q[:k - 1]), affine=True)
        sb = g2_msm(curve, pw[:k - 1], np.ascontiguousarray(Q[1:]), affine=True)
        if not pairing_check(curve, np.stack([P[1], neg1(P[0])]), np.stack([sa, sb])):
            return SRSCheck(False, "g2 powers")
    return SRSCheck(True)


def poly_mul_device(curve, n1, d_a, n2, d_b, d_tgt):
    """device-resident product (zkg_poly_mul_device): 0, or -1 when n1 + n2 - 1 is too large; d_a may be d_b"""
    return load().zkg_poly_mul_device(CURVE_ID[curve], n1, d_a.ptr if d_a else None, n2, d_b.ptr if d_b else None,
                                      d_tgt.ptr if d_tgt else None)


def poly_eval_device(curve, n, d_poly, x):
    out = np.zeros(4, dtype=np.uint64)
    load().zkg_poly_eval_device(CURVE_ID[curve], n, d_poly.ptr if d_poly else None, _p(_k(x)), _p(out))
    return out


def poly_lincomb_device(curve, ns, coeffs, d_polys, d_tgt):
    """d_tgt = sum_k coeffs[k] * d_polys[k][:ns[k]] (zkg_poly_lincomb_device); coeffs: (K, 4) host array"""
    K = len(ns)
    cs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(max(K, 0), 4) if K else np.zeros((1, 4), np.uint64)
    cn = (ctypes.c_int * max(1, K))(*ns)
    pp = (ctypes.c_void_p * max(1, K))(*[d.ptr for d in d_polys])
    load().zkg_poly_lincomb_device(CURVE_ID[curve], K, cn, _p(cs), pp, d_tgt.ptr if d_tgt else None)


def poly_long_div_device(curve, n1, d_p, n2, d_d, nquot, d_quot, nrem, d_rem):
    """device-resident division (zkg_poly_long_div_device): 0, or -1 when the call is refused; d_quot and / or
    d_rem may be None (the remainder / the quotient alone)"""
    return load().zkg_poly_long_div_device(CURVE_ID[curve], n1, d_p.ptr if d_p else None, n2, d_d.ptr if d_d else None,
                                           nquot, d_quot.ptr if d_quot else None, nrem, d_rem.ptr if d_rem else None)


def poly_set_div_base_max(length):
    """test hook: terms of the series inverse's base kernel (< 0: the default, 0 / 1: one term)"""
    load().zkg_poly_set_div_base_max(int(length))


def poly_div_base_max():
    """the base kernel size in force (after clamping to the kernel's capacity)"""
    return load().zkg_poly_div_base_max()


def poly_div_plan(m):
    """the precisions [base terms, after step 1, ..., m] of the series inverse for a quotient of m coefficients
    (len - 1 Newton steps), or None for m <= 0; a host computation"""
    s = load().zkg_poly_div_plan(int(m), None, 0)
    if s < 0:
        return None
    prec = (ctypes.c_int * (s + 1))()
    load().zkg_poly_div_plan(int(m), prec, s + 1)
    return list(prec)


def poly_last_div_steps():
    """Newton steps of the most recent division, -1 when it took an early exit"""
    return load().zkg_poly_last_div_steps()


def poly_set_mul_direct_max(length):
    """test hook: shorter factor <= length takes the direct kernel (0: always the NTT, < 0: default)"""
    load().zkg_poly_set_mul_direct_max(int(length))


def poly_last_mul_path():
    """0: the most recent product ran on the direct kernel; else log2 of its transform size"""
    return load().zkg_poly_last_mul_path()


def ntt_device(curve, m, gen, d_src, d_dst, inverse=False):
    load().zkg_ntt_device(CURVE_ID[curve], 1 if inverse else 0, m, _p(np.ascontiguousarray(gen)), d_src.ptr,
                          d_dst.ptr)


def ntt_ext_device(curve, m, gen, d_src, d_dst, inverse=False, shift=None, batch=1):
    """device-resident batched / coset NTT (zkg_ntt_ext_device): d_src / d_dst are DeviceBuffers of
    batch * 2^m rows (the same buffer transforms in place); raises ValueError on a -1 return"""
    rc = load().zkg_ntt_ext_device(CURVE_ID[curve], 1 if inverse else 0, m, _p(_k(gen)), _shift_arg(shift), batch,
                                   d_src.ptr if d_src else None, d_dst.ptr if d_dst else None)
    if rc != 0:
        raise ValueError("ntt_ext_device: log2 size outside 0..30, negative batch, or an inverse with shift 0")


def ntt_ext_set_max_grid(tiles):
    """test hook: blocks per launch of the batched NTT pass kernel (0: the default, 2^21)"""
    load().zkg_ntt_ext_set_max_grid(int(tiles))


def ntt_set_table_max(entries):
    """test hook: inter-pass twiddle entries above which NTT passes compute twiddles on the fly (0: default)"""
    load().zkg_ntt_set_table_max(int(entries))


def ntt_set_cache_limit(nbytes):
    """test hook: bytes of cached twiddle sets one context keeps before evicting (0: the default, 8 GiB)"""
    load().zkg_ntt_set_cache_limit(int(nbytes))


def ntt_cache_bytes():
    """device bytes of the twiddle sets and coset shift tables cached for the calling thread's device"""
    return int(load().zkg_ntt_cache_bytes())


def arena_set_limit(nbytes):
    """test hook: cap on one working-set arena's device bytes (0: unlimited)"""
    load().zkg_arena_set_limit(int(nbytes))


def msm_last_groups():
    return load().zkg_msm_last_groups()


def g1_fft_plan(curve, m):
    """bits per Stockham radix-2^b GLV stage of a 2^m group FFT ([] = the fused radix-2 stages)"""
    bits = (ctypes.c_int * 32)()
    k = load().zkg_g1_fft_plan(CURVE_ID[curve], m, bits, 32)
    return list(bits[:k])


def g1_fft_glv_products(curve, m, inverse=False):
    """GLV lane-pair scalar multiplications one 2^m group FFT runs on subgroup inputs (the fused
    radix-2 stages: N/2 per stage, minus the j = 0 butterflies; the inverse's first stage: N; the
    radix-2^b stages: D_b N / 2^b per stage, the few unit-twiddle products (a copy) included)"""
    n = 1 << m
    plan = g1_fft_plan(curve, m)
    if not plan:
        per = [n // 2 - (n >> s) for s in range(1, m + 1)]  # the N / 2^s j = 0 butterflies copy
        if inverse:
            per[-1] = n  # the first inverse stage (s = m) multiplies both outputs (N^-1 folded in)
        return sum(per)
    lib = load()
    tot = 0
    for i, b in enumerate(plan):
        tot += lib.zkg_g1_fft_radix_products(b) * (n >> b) + ((n >> b) if inverse and i == 0 else 0)
    return tot


def g1_fft_last_glv():
    """1 when the most recent group FFT ran the GLV stages (all inputs in the order-r subgroup)"""
    return load().zkg_g1_fft_last_glv()


def msm_workspace_bytes(curve, n, nlimbs=4, mont=True, host_inputs=True, window=0, groups=1):
    """device bytes of one G1 MSM's working set with its windows in `groups` passes"""
    return load().zkg_msm_workspace_bytes(CURVE_ID[curve], n, nlimbs, 1 if mont else 0, 1 if host_inputs else 0,
                                          window, groups)


def set_devices(ids):
    """device set of the host-buffer MSM entries (zkg_set_devices); [] = calling thread's device"""
    ids = list(ids)
    arr = (ctypes.c_int * max(1, len(ids)))(*ids)
    if load().zkg_set_devices(arr, len(ids)) != 0:
        raise ValueError(f"set_devices: invalid device id in {ids}")


def get_devices():
    arr = (ctypes.c_int * 64)()
    n = load().zkg_get_devices(arr, 64)
    return list(arr[:min(n, 64)])


def set_error_mode(recoverable):
    """zkg_set_error_mode: False = abort on a device error (default), True = the failing call
    returns and last_error() reports it"""
    load().zkg_set_error_mode(1 if recoverable else 0)


def last_error():
    """the calling thread's last recorded library error (cleared), or None"""
    buf = ctypes.create_string_buffer(512)
    return buf.value.decode() if load().zkg_last_error(buf, 512) else None


def release():
    """free every device buffer the library caches (zkg_release)"""
    load().zkg_release()


def timer(enable=None, reset=False):
    lib = load()
    if enable is not None:
        lib.zkg_timer_enable(1 if enable else 0)
    if reset:
        lib.zkg_timer_reset()
    ms = ctypes.c_double()
    n = ctypes.c_long()
    lib.zkg_timer_read(ctypes.byref(ms), ctypes.byref(n))
    return ms.value, n.value
