/*
 * zkalgebra_gpu.h -- C ABI of the MI355X (gfx950) MSM / NTT library.
 *
 * Part 1 exports EXACTLY the symbols and signatures of the reference's generated C
 * that its Haskell FFI modules bind with `foreign import ccall unsafe` (drop-in
 * boundary).  Part 2 adds device-resident and helper entry points that
 * the reference does not have (benchmarking, multi-GPU sharding, input generation).
 *
 * Layouts (identical to the reference, Class/Flat.hs:81-83):
 *   u64 little-endian limbs; Fr = 4 limbs; Fp = 4 (bn128) or 6 (bls12_381) limbs;
 *   affine G1 = x || y (Montgomery Fp), infinity = all bytes 0xFF;
 *   projective G1 = X || Y || Z (x = X/Z, y = Y/Z), Jacobian = X || Y || Z (x = X/Z^2).
 * All buffers are caller-owned and are not retained after the call returns.
 * Every call is synchronous and thread-safe.  There are no error codes on the
 * reference ABI: by default, on a device error the library prints a message and aborts (the
 * reference asserts, bls12_381_G1_proj.c:518,632) -- it never falls back to a CPU path.
 * zkg_set_error_mode(1) makes errors recoverable: the failing call prints the message,
 * returns early (outputs unspecified) and zkg_last_error() reports it to the calling thread.
 *
 * Projective / Jacobian outputs are returned NORMALISED (Z = 1, or the canonical
 * infinity (0:1:0) / Jacobian (1:1:0)); they are equal as points to the reference's
 * un-normalised outputs (whose exact coordinates depend on its operation order and
 * are not reproducible).  Affine outputs are bit-identical.
 */
#ifndef ZKALGEBRA_GPU_H
#define ZKALGEBRA_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZKG_API __attribute__((visibility("default")))

/* ------------------------------------------------------------------------------
 * Part 1: reference symbols.  <C> in {bn128, bls12_381}.
 * ---------------------------------------------------------------------------- */

/* MSM, G1, homogeneous projective.
 *   lib/cbits/curves/g1/proj/bls12_381_G1_proj.h:43-46 (bn128_G1_proj.h same lines)
 *   mont_coeff_proj_out  <- Haskell `msm`    (lib/src/ZK/Algebra/Curves/<C>/G1/Proj.hs:229,245)
 *   std_coeff_proj_out   <- Haskell `msmStd` (G1/Proj.hs:228,262)
 *   _affine_out          <- bls12_381_G1_proj.c:654-670
 *   expos: npoints x expo_nlimbs u64 (Montgomery Fr for mont_coeff, plain integers for
 *   std_coeff, used verbatim -- no reduction mod r).  expo_nlimbs: any >= 1; std scalars
 *   are 64*expo_nlimbs-bit integers (G1_proj.c:511,552); for mont the first min(nl,4) limbs
 *   of each row are the Montgomery value (the reference's result is undefined for nl != 4).
 *   grps : npoints affine points.  tgt: 3*NP (proj) or 2*NP (affine) u64. */
ZKG_API void bn128_G1_proj_MSM_mont_coeff_proj_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bn128_G1_proj_MSM_std_coeff_proj_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bn128_G1_proj_MSM_mont_coeff_affine_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bn128_G1_proj_MSM_std_coeff_affine_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
/* bn128_G1_proj.c:506 -- window_size is honoured as the GPU window (clamped to [4,24]) */
ZKG_API void bn128_G1_proj_MSM_std_coeff_proj_out_variable(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs, int window_size);

ZKG_API void bls12_381_G1_proj_MSM_mont_coeff_proj_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bls12_381_G1_proj_MSM_std_coeff_proj_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bls12_381_G1_proj_MSM_mont_coeff_affine_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bls12_381_G1_proj_MSM_std_coeff_affine_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
/* bls12_381_G1_proj.c:507 */
ZKG_API void bls12_381_G1_proj_MSM_std_coeff_proj_out_variable(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs, int window_size);

/* MSM, G1, Jacobian output (secondary; bls12_381_G1_jac.h:43-46, bound by G1/Jac.hs:225-226) */
ZKG_API void bn128_G1_jac_MSM_std_coeff_jac_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bn128_G1_jac_MSM_mont_coeff_jac_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bn128_G1_jac_MSM_std_coeff_affine_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bn128_G1_jac_MSM_mont_coeff_affine_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bls12_381_G1_jac_MSM_std_coeff_jac_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bls12_381_G1_jac_MSM_mont_coeff_jac_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bls12_381_G1_jac_MSM_std_coeff_affine_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bls12_381_G1_jac_MSM_mont_coeff_affine_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);

/* NTT over Fr, natural order in/out, 2^m elements, gen = Montgomery generator of the
 * order-2^m subgroup (Haskell passes fftSubgroupGen).  Out-of-place.
 *   lib/cbits/curves/poly/mont/bls12_381_poly_mont.h:27-28 (bn128_poly_mont.h same)
 *   forward <- Haskell forwardNTT (lib/src/ZK/Algebra/Curves/<C>/Poly.hs:397,409)
 *   inverse <- Haskell inverseNTT (Poly.hs:398,421) */
ZKG_API void bn128_poly_mont_ntt_forward(int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt);
ZKG_API void bn128_poly_mont_ntt_inverse(int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt);
ZKG_API void bls12_381_poly_mont_ntt_forward(int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt);
ZKG_API void bls12_381_poly_mont_ntt_inverse(int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt);

/* MSM on G2: the twist over Fp2 = Fp[u]/(u^2+1), same conventions
 * as G1 with NP doubled (Fp2 element = c0 || c1); affine infinity = all-0xFF.
 *   bls12_381_G2_proj.h:43-46 (bn128_G2_proj.h same lines), bound by G2/Proj.hs */
ZKG_API void bn128_G2_proj_MSM_std_coeff_proj_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bn128_G2_proj_MSM_mont_coeff_proj_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bn128_G2_proj_MSM_std_coeff_affine_out (int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bn128_G2_proj_MSM_mont_coeff_affine_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bls12_381_G2_proj_MSM_std_coeff_proj_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bls12_381_G2_proj_MSM_mont_coeff_proj_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bls12_381_G2_proj_MSM_std_coeff_affine_out (int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
ZKG_API void bls12_381_G2_proj_MSM_mont_coeff_affine_out(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs);
/* explicit window (bls12_381_G2_proj.c:498): clamped to 4..24 like the G1 twin; the result does not depend on it */
ZKG_API void bn128_G2_proj_MSM_std_coeff_proj_out_variable(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs, int window_size);
ZKG_API void bls12_381_G2_proj_MSM_std_coeff_proj_out_variable(int npoints, const uint64_t *expos, const uint64_t *grps, uint64_t *tgt, int expo_nlimbs, int window_size);

/* G2 batch conversions (bls12_381_G2_proj.h:9-10; Haskell batchFromAffine / batchToAffine,
 * G2/Proj.hs:386-405, and msmProj = msm . batchToAffine, :223-224).  Host buffers; rows are
 * 4 NP (affine) and 6 NP (projective) words.  Affine infinity (all-0xFF) <-> (0 : 1 : 0); every
 * row with Z = 0 converts to all-0xFF.  One Fp inversion is shared by many points. */
ZKG_API void bn128_G2_proj_batch_from_affine( int N, const uint64_t *src , uint64_t *tgt );
ZKG_API void bn128_G2_proj_batch_to_affine  ( int N, const uint64_t *src , uint64_t *tgt );
ZKG_API void bls12_381_G2_proj_batch_from_affine( int N, const uint64_t *src , uint64_t *tgt );
ZKG_API void bls12_381_G2_proj_batch_to_affine  ( int N, const uint64_t *src , uint64_t *tgt );

/* G2 group (curve) FFT (bls12_381_G2_proj.h:48-49, bn128_G2_proj.h same lines; Haskell forwardFFT /
 * inverseFFT = curveFFT / curveIFFT of the G2 instance, G2/Proj.hs).  Host buffers of 2^m projective
 * rows (6 NP words), m in 0..24; gen is the Montgomery generator of the order-2^m subgroup of Fr.
 * Every level multiplies by the integer value of the reference's canonical scalar at that position
 * (both twists have a cofactor), so the output equals the reference's for every on-curve input.
 * Outputs are normalised like the reference's (bls12_381_G2_proj.c:70-89, 716-718): (x : y : 1),
 * infinity (0 : 1 : 0); an input row with Z = 0 is the point at infinity. */
ZKG_API void bn128_G2_proj_fft_forward( int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt );
ZKG_API void bn128_G2_proj_fft_inverse( int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt );
ZKG_API void bls12_381_G2_proj_fft_forward( int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt );
ZKG_API void bls12_381_G2_proj_fft_inverse( int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt );

/* G1 batch conversions and the group (curve) FFT.
 *   bls12_381_G1_proj.h:9-10, 48-49 (bn128_G1_proj.h same lines); Haskell batchFromAffine /
 *   batchToAffine (G1/Proj.hs:409-430), forwardFFT / inverseFFT = curveFFT / curveIFFT
 *   (G1/Proj.hs:270-294).  Projective outputs of the FFT are normalised, like the
 *   reference's (bls12_381_G1_proj.c:719, 785). */
ZKG_API void bn128_G1_proj_batch_from_affine( int N, const uint64_t *src , uint64_t *tgt );
ZKG_API void bn128_G1_proj_batch_to_affine  ( int N, const uint64_t *src , uint64_t *tgt );
ZKG_API void bn128_G1_proj_fft_forward( int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt );
ZKG_API void bn128_G1_proj_fft_inverse( int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt );
ZKG_API void bls12_381_G1_proj_batch_from_affine( int N, const uint64_t *src , uint64_t *tgt );
ZKG_API void bls12_381_G1_proj_batch_to_affine  ( int N, const uint64_t *src , uint64_t *tgt );
ZKG_API void bls12_381_G1_proj_fft_forward( int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt );
ZKG_API void bls12_381_G1_proj_fft_inverse( int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt );

/* Jacobian twins (round 6): bls12_381_G1_jac.h:9-10, 48-49 (bn128_G1_jac.h same lines); bound by the
 * Jacobian G1 instance -- batchFromAffine / batchToAffine (G1/Jac.hs:374-389; Curve.msm on Jac.G1 is
 * msmJac cs gs = msm cs (batchToAffine gs), Jac.hs:188, 220) and forwardFFT / inverseFFT = curveFFT /
 * curveIFFT (Jac.hs:189-190, 264-291).  Conventions: affine infinity -> (1 : 1 : 0)
 * (bls12_381_G1_jac.c:108-116, 183-187); Z = 0 -> all-0xFF (to_affine, :120-125); FFT outputs
 * normalised (x : y : 1), infinity (0 : 1 : 0) (jac normalize, :62-67, applied at :773-775, :835-837). */
ZKG_API void bn128_G1_jac_batch_from_affine( int N, const uint64_t *src , uint64_t *tgt );
ZKG_API void bn128_G1_jac_batch_to_affine  ( int N, const uint64_t *src , uint64_t *tgt );
ZKG_API void bn128_G1_jac_fft_forward( int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt );
ZKG_API void bn128_G1_jac_fft_inverse( int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt );
ZKG_API void bls12_381_G1_jac_batch_from_affine( int N, const uint64_t *src , uint64_t *tgt );
ZKG_API void bls12_381_G1_jac_batch_to_affine  ( int N, const uint64_t *src , uint64_t *tgt );
ZKG_API void bls12_381_G1_jac_fft_forward( int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt );
ZKG_API void bls12_381_G1_jac_fft_inverse( int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt );

/* Fr vector operations around the NTT.  <C> in {bn128, bls12_381}.
 *   lib/cbits/curves/array/mont/bls12_381_arr_mont.h:3-48 (bn128_arr_mont.h same lines),
 *   bound by Haskell ZK.Algebra.Curves.<C>.Array (Array.hs:108-352).
 *   n elements of Montgomery Fr (4 u64 each); coefficients are single elements.
 *   inv / div follow the reference's batch inversion (Fr_mont.c:258-285): if ANY
 *   (divisor) element is zero, EVERY output element is zero.  n == 0 is a no-op (the
 *   reference asserts n >= 1 in batch_inv). */
ZKG_API uint8_t bn128_arr_mont_is_valid ( int n, const uint64_t *src );
ZKG_API uint8_t bn128_arr_mont_is_zero  ( int n, const uint64_t *src );
ZKG_API uint8_t bn128_arr_mont_is_one   ( int n, const uint64_t *src );
ZKG_API uint8_t bn128_arr_mont_is_equal ( int n, const uint64_t *src1, const uint64_t *src2 );
ZKG_API void bn128_arr_mont_set_zero ( int n, uint64_t *tgt );
ZKG_API void bn128_arr_mont_set_one  ( int n, uint64_t *tgt );
ZKG_API void bn128_arr_mont_set_const( int n, const uint64_t *src, uint64_t *tgt );
ZKG_API void bn128_arr_mont_copy     ( int n, const uint64_t *src, uint64_t *tgt );
ZKG_API void bn128_arr_mont_from_std ( int n, const uint64_t *src, uint64_t *tgt );
ZKG_API void bn128_arr_mont_to_std   ( int n, const uint64_t *src, uint64_t *tgt );
ZKG_API void bn128_arr_mont_append( int n1, int n2, const uint64_t *src1, const uint64_t *src2, uint64_t *tgt );
ZKG_API void bn128_arr_mont_neg ( int n, const uint64_t *src, uint64_t *tgt );
ZKG_API void bn128_arr_mont_add ( int n, const uint64_t *src1, const uint64_t *src2, uint64_t *tgt );
ZKG_API void bn128_arr_mont_sub ( int n, const uint64_t *src1, const uint64_t *src2, uint64_t *tgt );
ZKG_API void bn128_arr_mont_sqr ( int n, const uint64_t *src, uint64_t *tgt );
ZKG_API void bn128_arr_mont_mul ( int n, const uint64_t *src1, const uint64_t *src2, uint64_t *tgt );
ZKG_API void bn128_arr_mont_inv ( int n, const uint64_t *src, uint64_t *tgt );
ZKG_API void bn128_arr_mont_div ( int n, const uint64_t *src1, const uint64_t *src2, uint64_t *tgt );
ZKG_API void bn128_arr_mont_neg_inplace ( int n, uint64_t *tgt );
ZKG_API void bn128_arr_mont_add_inplace ( int n, uint64_t *tgt, const uint64_t *src2 );
ZKG_API void bn128_arr_mont_sub_inplace ( int n, uint64_t *tgt, const uint64_t *src2 );
ZKG_API void bn128_arr_mont_sqr_inplace ( int n, uint64_t *tgt );
ZKG_API void bn128_arr_mont_mul_inplace ( int n, uint64_t *tgt, const uint64_t *src2 );
ZKG_API void bn128_arr_mont_inv_inplace ( int n, uint64_t *tgt );
ZKG_API void bn128_arr_mont_div_inplace ( int n, uint64_t *tgt, const uint64_t *src2 );
ZKG_API void bn128_arr_mont_sub_inplace_reverse ( int n, uint64_t *tgt, const uint64_t *src1 );
ZKG_API void bn128_arr_mont_mul_add ( int n, const uint64_t *src1, const uint64_t *src2, const uint64_t *src3, uint64_t *tgt );
ZKG_API void bn128_arr_mont_mul_sub ( int n, const uint64_t *src1, const uint64_t *src2, const uint64_t *src3, uint64_t *tgt );
ZKG_API void bn128_arr_mont_dot_prod ( int n, const uint64_t *src1, const uint64_t *src2, uint64_t *tgt );
ZKG_API void bn128_arr_mont_powers ( int n, const uint64_t *coeffA, const uint64_t *coeffB, uint64_t *tgt );
ZKG_API void bn128_arr_mont_scale ( int n, const uint64_t *coeff, const uint64_t *src2, uint64_t *tgt );
ZKG_API void bn128_arr_mont_scale_inplace ( int n, const uint64_t *coeff, uint64_t *tgt );
ZKG_API void bn128_arr_mont_Ax_plus_y ( int n, const uint64_t *coeffA, const uint64_t *src1, const uint64_t *src2, uint64_t *tgt );
ZKG_API void bn128_arr_mont_Ax_plus_y_inplace ( int n, const uint64_t *coeffA, uint64_t *tgt, const uint64_t *src2 );
ZKG_API void bn128_arr_mont_Ax_plus_By ( int n, const uint64_t *coeffA, const uint64_t *coeffB, const uint64_t *src1, const uint64_t *src2, uint64_t *tgt );
ZKG_API void bn128_arr_mont_Ax_plus_By_inplace ( int n, const uint64_t *coeffA, const uint64_t *coeffB, uint64_t *tgt, const uint64_t *src2 );
/* division by the vanishing polynomial x^expo_n - eta (bls12_381_poly_mont.c:317-413) */
ZKG_API void bn128_poly_mont_div_by_vanishing ( int n1, const uint64_t *src1, int expo_n, const uint64_t *eta, int nquot, uint64_t *quot, int nrem, uint64_t *rem );
ZKG_API uint8_t bn128_poly_mont_quot_by_vanishing( int n1, const uint64_t *src1, int expo_n, const uint64_t *eta, int nquot, uint64_t *quot );

ZKG_API uint8_t bls12_381_arr_mont_is_valid ( int n, const uint64_t *src );
ZKG_API uint8_t bls12_381_arr_mont_is_zero  ( int n, const uint64_t *src );
ZKG_API uint8_t bls12_381_arr_mont_is_one   ( int n, const uint64_t *src );
ZKG_API uint8_t bls12_381_arr_mont_is_equal ( int n, const uint64_t *src1, const uint64_t *src2 );
ZKG_API void bls12_381_arr_mont_set_zero ( int n, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_set_one  ( int n, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_set_const( int n, const uint64_t *src, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_copy     ( int n, const uint64_t *src, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_from_std ( int n, const uint64_t *src, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_to_std   ( int n, const uint64_t *src, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_append( int n1, int n2, const uint64_t *src1, const uint64_t *src2, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_neg ( int n, const uint64_t *src, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_add ( int n, const uint64_t *src1, const uint64_t *src2, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_sub ( int n, const uint64_t *src1, const uint64_t *src2, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_sqr ( int n, const uint64_t *src, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_mul ( int n, const uint64_t *src1, const uint64_t *src2, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_inv ( int n, const uint64_t *src, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_div ( int n, const uint64_t *src1, const uint64_t *src2, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_neg_inplace ( int n, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_add_inplace ( int n, uint64_t *tgt, const uint64_t *src2 );
ZKG_API void bls12_381_arr_mont_sub_inplace ( int n, uint64_t *tgt, const uint64_t *src2 );
ZKG_API void bls12_381_arr_mont_sqr_inplace ( int n, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_mul_inplace ( int n, uint64_t *tgt, const uint64_t *src2 );
ZKG_API void bls12_381_arr_mont_inv_inplace ( int n, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_div_inplace ( int n, uint64_t *tgt, const uint64_t *src2 );
ZKG_API void bls12_381_arr_mont_sub_inplace_reverse ( int n, uint64_t *tgt, const uint64_t *src1 );
ZKG_API void bls12_381_arr_mont_mul_add ( int n, const uint64_t *src1, const uint64_t *src2, const uint64_t *src3, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_mul_sub ( int n, const uint64_t *src1, const uint64_t *src2, const uint64_t *src3, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_dot_prod ( int n, const uint64_t *src1, const uint64_t *src2, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_powers ( int n, const uint64_t *coeffA, const uint64_t *coeffB, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_scale ( int n, const uint64_t *coeff, const uint64_t *src2, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_scale_inplace ( int n, const uint64_t *coeff, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_Ax_plus_y ( int n, const uint64_t *coeffA, const uint64_t *src1, const uint64_t *src2, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_Ax_plus_y_inplace ( int n, const uint64_t *coeffA, uint64_t *tgt, const uint64_t *src2 );
ZKG_API void bls12_381_arr_mont_Ax_plus_By ( int n, const uint64_t *coeffA, const uint64_t *coeffB, const uint64_t *src1, const uint64_t *src2, uint64_t *tgt );
ZKG_API void bls12_381_arr_mont_Ax_plus_By_inplace ( int n, const uint64_t *coeffA, const uint64_t *coeffB, uint64_t *tgt, const uint64_t *src2 );
/* division by the vanishing polynomial x^expo_n - eta (bls12_381_poly_mont.c:317-413) */
ZKG_API void bls12_381_poly_mont_div_by_vanishing ( int n1, const uint64_t *src1, int expo_n, const uint64_t *eta, int nquot, uint64_t *quot, int nrem, uint64_t *rem );
ZKG_API uint8_t bls12_381_poly_mont_quot_by_vanishing( int n1, const uint64_t *src1, int expo_n, const uint64_t *eta, int nquot, uint64_t *quot );


/* Polynomial layer over Fr (lib/cbits/curves/poly/mont/bls12_381_poly_mont.c:26-243, bn128 same
 * lines; Poly.hs:199-209).  Parameter types are those of the DEFINITIONS in the .c file and of
 * the Haskell foreign imports: the reference header declares degree(const uint64_t*) without the
 * length, the .c file and Poly.hs:199 have (int, const uint64_t*), which is what is exported here.
 * mul_naive is what Haskell's (*) and sqr on Poly call (Poly.hs:133); it computes the same
 * coefficients by a direct kernel (short factor) or by NTTs, so n1 + n2 - 1 is limited to 2^28
 * (bn128) / 2^30 (bls12_381): beyond it the call fails through the error channel.  src1 == src2
 * is allowed; tgt aliases no input of mul_naive, lincomb and eval_at.  long_div, quot and rem are
 * provided in Part 2 as zkg_poly_long_div / zkg_poly_long_div_device (the curve as first argument,
 * then the reference's argument list; quot and rem are that call with a NULL output), not under
 * the reference's names: the reference's symbols stay the reference's own CPU definitions until a
 * separate change exports aliases.  get_coeff and is_constant are NOT provided. */
ZKG_API int     bn128_poly_mont_degree   ( int n1, const uint64_t *src1 );
ZKG_API uint8_t bn128_poly_mont_is_zero  ( int n1, const uint64_t *src1 );
ZKG_API uint8_t bn128_poly_mont_is_equal ( int n1, const uint64_t *src1, int n2, const uint64_t *src2 );
ZKG_API void    bn128_poly_mont_neg      ( int n1, const uint64_t *src1, uint64_t *tgt );
ZKG_API void    bn128_poly_mont_add      ( int n1, const uint64_t *src1, int n2, const uint64_t *src2, uint64_t *tgt );
ZKG_API void    bn128_poly_mont_sub      ( int n1, const uint64_t *src1, int n2, const uint64_t *src2, uint64_t *tgt );
ZKG_API void    bn128_poly_mont_scale    ( const uint64_t *kst1, int n2, const uint64_t *src2, uint64_t *tgt );
ZKG_API void    bn128_poly_mont_lincomb  ( int K, const int *ns, const uint64_t **coeffs, const uint64_t **polys, uint64_t *tgt );
ZKG_API void    bn128_poly_mont_mul_naive( int n1, const uint64_t *src1, int n2, const uint64_t *src2, uint64_t *tgt );
ZKG_API void    bn128_poly_mont_eval_at  ( int n1, const uint64_t *src1, const uint64_t *loc, uint64_t *tgt );
ZKG_API int     bls12_381_poly_mont_degree   ( int n1, const uint64_t *src1 );
ZKG_API uint8_t bls12_381_poly_mont_is_zero  ( int n1, const uint64_t *src1 );
ZKG_API uint8_t bls12_381_poly_mont_is_equal ( int n1, const uint64_t *src1, int n2, const uint64_t *src2 );
ZKG_API void    bls12_381_poly_mont_neg      ( int n1, const uint64_t *src1, uint64_t *tgt );
ZKG_API void    bls12_381_poly_mont_add      ( int n1, const uint64_t *src1, int n2, const uint64_t *src2, uint64_t *tgt );
ZKG_API void    bls12_381_poly_mont_sub      ( int n1, const uint64_t *src1, int n2, const uint64_t *src2, uint64_t *tgt );
ZKG_API void    bls12_381_poly_mont_scale    ( const uint64_t *kst1, int n2, const uint64_t *src2, uint64_t *tgt );
ZKG_API void    bls12_381_poly_mont_lincomb  ( int K, const int *ns, const uint64_t **coeffs, const uint64_t **polys, uint64_t *tgt );
ZKG_API void    bls12_381_poly_mont_mul_naive( int n1, const uint64_t *src1, int n2, const uint64_t *src2, uint64_t *tgt );
ZKG_API void    bls12_381_poly_mont_eval_at  ( int n1, const uint64_t *src1, const uint64_t *loc, uint64_t *tgt );

/* ------------------------------------------------------------------------------
 * Part 2: extensions (not in the reference).  curve: 0 = bn128, 1 = bls12_381.
 * ---------------------------------------------------------------------------- */
#define ZKG_BN128 0
#define ZKG_BLS12_381 1

ZKG_API const char *zkg_version(void);
/* error channel: mode 0 = print and abort on a device error (default, reference-like),
 * 1 = print, return from the failing call (outputs unspecified) and record the message;
 * zkg_last_error returns 1 and copies the calling thread's last message (cleared), else 0 */
ZKG_API void zkg_set_error_mode(int mode);
ZKG_API int zkg_last_error(char *msg, size_t cap);
ZKG_API int zkg_device_count(void);
ZKG_API void zkg_set_device(int device);           /* binds the calling thread */
ZKG_API void *zkg_device_malloc(size_t bytes);
ZKG_API void zkg_device_free(void *ptr);
ZKG_API void zkg_memcpy_htod(void *dst, const void *src, size_t bytes);
ZKG_API void zkg_memcpy_dtoh(void *dst, const void *src, size_t bytes);
ZKG_API void zkg_device_synchronize(void);

/* Device set of the host-buffer MSM entry points (G1 and G2, every Part-1 MSM symbol): the
 * pairs are split into n contiguous chunks, chunk k computed on device ids[k] (copying only its
 * own chunk over that device's PCIe link), the partial sums added in list order.  A device may
 * be listed more than once (one stream / arena per occurrence).  n <= 1: the calling thread's
 * device only (the default; also set by the environment variable ZKG_DEVICES = "all" or
 * "0,1,..." at first use).  A one-entry set pins the host-buffer MSMs (and NTTs) to that device.
 * The host-buffer NTT symbols (2^16 points and up) compute on the calling thread's device when the
 * set lists it, else on the first listed device, and move chunk k of the input / output over
 * listed device k's PCIe link (peer copies over xGMI).  In a one-process-per-GPU job (bench.py
 * --gpus N, or any RCCL job) leave the set empty: every rank would otherwise push its host copies
 * through every GPU's link.  Returns 0, or -1 (set unchanged) for an invalid id.  The
 * device-resident zkg_*_device calls always run on the calling thread's device. */
ZKG_API int zkg_set_devices(const int *ids, int n);
ZKG_API int zkg_get_devices(int *ids, int cap);  /* returns the set's size; copies min(size, cap) ids */

/* Frees every device buffer the library holds (per-device working-set arenas, pinned staging,
 * cached NTT twiddle tables) after waiting for the calls in flight; later calls re-allocate. */
ZKG_API void zkg_release(void);

/* Multi-GPU exchange owned by the library (RCCL over xGMI, linked from /opt/rocm): one
 * communicator per process, one process per GPU.  The reference is single-device
 * (bls12_381_G1_proj.c:630-644); these calls shard its MSM by contiguous chunk of the pairs.
 * Rendezvous is the caller's: rank 0 writes the 128-byte id with zkg_comm_unique_id, every rank
 * calls zkg_comm_init with it on the device it will use (zkg_set_device first).  Every rank must
 * make the same sequence of zkg_comm_* / *_sharded calls.  Return 0 on success, -1 on misuse
 * (no communicator, bad arguments), else the RCCL error code (a message goes to stderr). */
#define ZKG_COMM_ID_BYTES 128
ZKG_API int zkg_comm_unique_id(void *out);
ZKG_API int zkg_comm_init(int rank, int world, const void *unique_id);
ZKG_API int zkg_comm_destroy(void);
ZKG_API int zkg_comm_rank(void);   /* -1 without a communicator */
ZKG_API int zkg_comm_world(void);  /* 0 without a communicator */
/* ncclAllGather of `bytes` host bytes per rank into recv (world * bytes, rank order) */
ZKG_API int zkg_comm_allgather(const void *send, void *recv, size_t bytes);
ZKG_API int zkg_comm_barrier(void);
ZKG_API int zkg_comm_max_f64(double *x);  /* in place: the maximum over ranks */
/* every rank passes `count` projective G1 partials (3 NP u64 each, host); all ranks receive
 * the normalised sum of the world * count partials, added in (rank, index) order */
ZKG_API int zkg_g1_comm_sum_partials(int curve, const uint64_t *partials, int count, uint64_t *tgt_proj);
/* Device-resident sharded MSM: this rank's chunk (npoints_local pairs, DEVICE pointers) is
 * computed on the communicator's device as `local_shards` contiguous sub-chunks, the
 * world * local_shards partial sums are all-gathered by ncclAllGather on the library's stream and
 * added in (rank, sub-chunk) order; tgt_proj (HOST, 3 NP u64) receives the normalised total on
 * every rank.  local_shards must be the same on every rank (1 = one partial per rank). */
ZKG_API int zkg_g1_msm_device_sharded(int curve, int npoints_local, const uint64_t *d_expos, int expo_nlimbs,
                                      int expos_mont, const uint64_t *d_grps, int window_size, int local_shards,
                                      uint64_t *tgt_proj);

/* device-resident MSM: d_expos / d_grps are DEVICE pointers (already in HBM);
 * tgt_proj is a HOST buffer of 3*NP u64 receiving the normalised projective sum. */
ZKG_API void zkg_g1_msm_device(int curve, int npoints, const uint64_t *d_expos, int expo_nlimbs, int expos_mont,
                               const uint64_t *d_grps, uint64_t *tgt_proj, int window_size);
/* device-resident G2 MSM (same contract as zkg_g1_msm_device; tgt_proj = 3 Fp2 elements) */
ZKG_API void zkg_g2_msm_device(int curve, int npoints, const uint64_t *d_expos, int expo_nlimbs, int expos_mont,
                               const uint64_t *d_grps, uint64_t *tgt_proj, int window_size);
/* device-resident NTT: d_src / d_tgt DEVICE pointers; gen on the host */
ZKG_API void zkg_ntt_device(int curve, int inverse, int m, const uint64_t *gen, const uint64_t *d_src, uint64_t *d_tgt);
/* batch transforms of 2^m Montgomery Fr each, transform b at row offset b * 2^m.  gen as in
 * zkg_ntt_device; shift: HOST pointer to one Montgomery Fr, or NULL for the plain transform.
 *   forward: tgt_b[k] = sum_j src_b[j] * shift^j * gen^(j k)            (= p_b(shift * gen^k))
 *   inverse: tgt_b[j] = shift^(-j) * (1/N) * sum_k src_b[k] * gen^(-j k)
 * Outputs canonical.  d_tgt may equal d_src (whole buffer); no partial overlap.
 * Returns 0; -1 (nothing written) for m outside 0..30, batch < 0, or inverse with shift == 0.
 * batch == 0 is a no-op.  shift == 0 forward is defined (0^0 = 1: every output is src_b[0]).
 * Every pass of the whole batch is one launch, and the shift rides on the first pass's load
 * (forward) or the last pass's closing product (inverse).  When the batch's working set (batch * 2^m
 * rows of scratch; three times that for the host form) does not fit, it runs in contiguous chunks
 * of transforms; the result does not depend on the chunking. */
ZKG_API int zkg_ntt_ext_device(int curve, int inverse, int m, const uint64_t *gen, const uint64_t *shift,
                               int batch, const uint64_t *d_src, uint64_t *d_tgt);
/* the same on HOST buffers (calling thread's device; the device set does not spread it) */
ZKG_API int zkg_ntt_ext(int curve, int inverse, int m, const uint64_t *gen, const uint64_t *shift,
                        int batch, const uint64_t *src, uint64_t *tgt);

/* device-resident Fr vector ops: d_* are DEVICE pointers, kA/kB and dot's tgt HOST.
 * op codes: 0 neg, 1 add, 2 sub, 3 sub_rev (b - a), 4 sqr, 5 mul, 6 mul_add, 7 mul_sub,
 * 8 scale (kA a), 9 Ax_plus_y, 10 Ax_plus_By, 11 from_std, 12 to_std, 13 copy,
 * 14 set_const (kA), 15 inv, 16 div (a / b)
 * Aliasing (tests/test_gpu_arr_device.py): any operand may be EXACTLY the target (d_tgt == d_a, d_b or d_c;
 * operands may also be each other), for every op code, and the result is the one of distinct buffers
 * computed from the inputs as they were before the call -- also for mul_add / mul_sub with d_tgt == d_c
 * and Ax_plus_y with d_tgt == d_b, where the reference's loops, aliased like that, lose the addend
 * (arr_mont.c:124-137, 204-209).  Partial overlap (a target shifted against an input) is undefined.
 * Nothing outside rows [0, n) of the target is written, and no input that is not the target is written;
 * powers with n == 0 writes nothing.  dot's operands may be the same buffer.  div_by_vanishing writes
 * exactly nquot / nrem rows (zero past deg - expo_n + 1 quotient and expo_n remainder rows, as the
 * reference does), aliases nothing, and with d_rem == NULL returns 1 when the remainder is zero, else 0.
 * The G1 conversions below (rows of 3 NP words in, 2 NP words out) need distinct buffers. */
ZKG_API void zkg_arr_op_device(int curve, int op, int n, const uint64_t *d_a, const uint64_t *d_b,
                               const uint64_t *d_c, const uint64_t *kA, const uint64_t *kB, uint64_t *d_tgt);
ZKG_API void zkg_arr_dot_device(int curve, int n, const uint64_t *d_a, const uint64_t *d_b, uint64_t *tgt);
ZKG_API void zkg_arr_powers_device(int curve, int n, const uint64_t *kA, const uint64_t *kB, uint64_t *d_tgt);
ZKG_API int zkg_poly_div_by_vanishing_device(int curve, int n1, const uint64_t *d_src, int expo_n,
                                             const uint64_t *eta, int nquot, uint64_t *d_quot, int nrem,
                                             uint64_t *d_rem);

/* polynomial layer on device-resident operands (zk_poly.hip).  zkg_poly_mul_device returns 0, or
 * -1 (nothing done) when n1 + n2 - 1 exceeds 2^28 (bn128) / 2^30 (bls12_381); d_a == d_b squares;
 * d_tgt (n1 + n2 - 1 rows) aliases neither.  x, tgt of eval and coeffs (K x 4 words), ns and the
 * array d_polys of K device pointers of lincomb are HOST memory. */
ZKG_API int zkg_poly_mul_device(int curve, int n1, const uint64_t *d_a, int n2, const uint64_t *d_b, uint64_t *d_tgt);
ZKG_API void zkg_poly_eval_device(int curve, int n, const uint64_t *d_poly, const uint64_t *x, uint64_t *tgt);
ZKG_API void zkg_poly_lincomb_device(int curve, int K, const int *ns, const uint64_t *coeffs, const uint64_t *const *d_polys, uint64_t *d_tgt);
/* test hooks: a product whose shorter factor has <= len coefficients takes the direct kernel
 * (0: always the transform, < 0: the default); the path of the most recent product (0: direct,
 * else log2 of the transform size) */
ZKG_API void zkg_poly_set_mul_direct_max(int len);
ZKG_API int zkg_poly_last_mul_path(void);

/* Division with remainder: src1 = quot * src2 + rem, deg rem < deg src2 -- the contract of
 * <C>_poly_mont_long_div (bls12_381_poly_mont.c:249-297), every output word bit-identical to it for
 * canonical Montgomery inputs; computed by Newton inversion of the reversed divisor over the NTT.
 * With dp, dq the degrees (-1: zero polynomial or length 0): quot[0, dp - dq] and rem[0, dq) are
 * written and the rest of the nquot / nrem rows is zero; the divisor need not be monic; dq < 0
 * zeroes both outputs; dp < dq gives quotient 0 and rem[0, dp] = src1.  quot and / or rem may be
 * NULL (<C>_poly_mont_rem / _quot) and are then never touched.  Outputs alias no input and not each
 * other.  Returns 0, or -1 with nothing written (a return code; the error channel stays clear) for
 * a negative length, quot with nquot < dp - dq + 1, rem with nrem < dq (nrem < dp + 1 when
 * dp < dq), or n1 > 2^27 (bn128) / 2^29 (bls12_381) -- the last on the length alone, before a
 * pointer is read.  A workspace that does not fit goes through the error channel.  Synchronous and
 * thread-safe, on the calling thread's device. */
ZKG_API int zkg_poly_long_div_device(int curve, int n1, const uint64_t *d_src1, int n2, const uint64_t *d_src2,
                                     int nquot, uint64_t *d_quot, int nrem, uint64_t *d_rem);   /* DEVICE pointers */
ZKG_API int zkg_poly_long_div(int curve, int n1, const uint64_t *src1, int n2, const uint64_t *src2,
                              int nquot, uint64_t *quot, int nrem, uint64_t *rem);               /* HOST pointers */
/* test hooks: terms of the series inverse's base kernel (< 0: the default; 0, 1: one term; larger
 * values are clamped to the kernel's capacity) and the value in force; the precision plan for a
 * quotient of m coefficients (returns the Newton steps s, the smallest with base * 2^s >= m, and
 * writes prec[0] = base kernel terms, prec[1..s] = precision after each step, prec[s] = m, at most
 * cap entries; -1 for m <= 0; no GPU call); the Newton steps of the most recent division (-1: it
 * took an early exit: zero divisor, dp < dq, refused) */
ZKG_API void zkg_poly_set_div_base_max(int len);
ZKG_API int  zkg_poly_div_base_max(void);
ZKG_API int  zkg_poly_div_plan(int m, int *prec, int cap);
ZKG_API int  zkg_poly_last_div_steps(void);
/* timing hook: while on, a division records events around its phases; ms[0..2] = series inverse,
 * quotient, remainder of the most recent profiled division */
ZKG_API void zkg_poly_div_profile(int on);
ZKG_API void zkg_poly_last_div_phase_ms(double *ms);

/* Division by a linear factor x - z, for nz points at once: what <C>_poly_mont_div_by_vanishing computes
 * with expo_n = 1 (bls12_381_poly_mont.c:317-397; examples/KZG.hs openingProof), every word bit-identical
 * to it for canonical Montgomery inputs.  z: HOST, nz x 4 words.  For point k, quot rows
 * [k (n - 1), (k + 1)(n - 1)) receive the n - 1 quotient coefficients (zero rows above the quotient's
 * degree, as the reference's cleared tail) and vals[k] (HOST, nz x 4 words) receives p(z_k), the
 * remainder.  quot may be NULL: the values alone.  n = 1 writes no quotient and the value a_0; n = 0 the
 * value 0.  A tiled suffix scan in three launches (zk_lindiv.hip): two reads and one write of the
 * coefficients per point.  Return 0, or -1 with nothing written and the text in zkg_last_error (in either
 * error mode) for an unknown curve, a negative size, NULL where a pointer is required, or a quotient
 * buffer that overlaps the polynomial: the write pass stores across tile boundaries, so aliasing would be
 * a race.  A device error goes through the error channel as everywhere.  Synchronous and thread-safe, on the
 * calling thread's device. */
ZKG_API int zkg_poly_div_linear_device(int curve, int n, const uint64_t *d_poly, int nz, const uint64_t *z,
                                       uint64_t *d_quot, uint64_t *vals);                 /* DEVICE poly, quot */
ZKG_API int zkg_poly_div_linear(int curve, int n, const uint64_t *poly, int nz, const uint64_t *z, uint64_t *quot,
                                uint64_t *vals);                                          /* HOST pointers */
/* test hook: rows per lane of a tile of the scan (a tile is 256 lanes x rows), so that a few thousand
 * coefficients span many tiles and several iterations of the carry pass; the kernels exist for 1, 2, 4 and 8
 * (the default) rows: 0 restores the default, larger values are clamped to it, 3 counts as 2 and 5 .. 7 as 4.
 * zkg_poly_lindiv_tile: the value in force.  The results do not depend on it. */
ZKG_API void zkg_poly_set_lindiv_tile(int rows_per_lane);
ZKG_API int  zkg_poly_lindiv_tile(void);

/* KZG prover on a device-resident polynomial (n Montgomery Fr rows) and SRS (affine G1 rows, 2 NP words:
 * what zkg_g1_batch_to_affine_device makes of a setup's projective rows); examples/KZG.hs commitPoly and
 * openingProof.  commit: tgt_proj (HOST, 3 NP words) = the normalised projective sum of coeffs_i srs_i,
 * i < n: zkg_g1_msm_device with Montgomery coefficients.  open: for every point z_k (HOST, nz x 4 words),
 * vals[k] = p(z_k) and proofs_proj row k (HOST, 3 NP words, normalised; (0 : 1 : 0) for n <= 1) = the
 * commitment to the quotient of p by x - z_k against the first n - 1 SRS rows -- per point, the division
 * above into a buffer of the call, then the device MSM, on the same stream.  Return codes and refusals as
 * for zkg_poly_div_linear. */
ZKG_API int zkg_kzg_commit_device(int curve, int n, const uint64_t *d_coeffs, const uint64_t *d_srs_affine,
                                  uint64_t *tgt_proj);
ZKG_API int zkg_kzg_open_device(int curve, int n, const uint64_t *d_poly, const uint64_t *d_srs_affine, int nz,
                                const uint64_t *z, uint64_t *vals, uint64_t *proofs_proj);


/* device-resident G1 group FFT / batch_to_affine (d_* DEVICE pointers, gen on the host) */
ZKG_API void zkg_g1_fft_device(int curve, int inverse, int m, const uint64_t *gen, const uint64_t *d_src,
                               uint64_t *d_tgt);
ZKG_API void zkg_g1_batch_to_affine_device(int curve, int n, const uint64_t *d_src, uint64_t *d_tgt);
/* the same on Jacobian rows (the <C>_G1_jac_fft_* / _batch_to_affine conventions above) */
ZKG_API void zkg_g1_jac_fft_device(int curve, int inverse, int m, const uint64_t *gen, const uint64_t *d_src,
                                   uint64_t *d_tgt);
ZKG_API void zkg_g1_jac_batch_to_affine_device(int curve, int n, const uint64_t *d_src, uint64_t *d_tgt);
/* device-resident G2 batch_to_affine: n projective rows (6 NP words) -> n affine rows (4 NP words) */
ZKG_API void zkg_g2_batch_to_affine_device(int curve, int n, const uint64_t *d_src, uint64_t *d_tgt);
/* device-resident G2 group FFT (d_* DEVICE pointers, gen on the host; the <C>_G2_proj_fft_* contract) */
ZKG_API void zkg_g2_fft_device(int curve, int inverse, int m, const uint64_t *gen, const uint64_t *d_src, uint64_t *d_tgt);
/* test hook: cap on the scalar-multiplication lanes of a G2 FFT stage (rounded up to 256; 0 restores the default),
 * so that the grid-stride loop of a stage is exercised at small sizes */
ZKG_API void zkg_g2_fft_set_max_lanes(int lanes);

/* Batch G1 scalar multiplication (the reference's <C>_G1_proj_scl_Fr_mont / _scl_Fr_std, G1_proj.c:462-489,
 * followed by _normalize or _to_affine, once per row).
 *   fixed:  tgt[i] = [k_i] P     one affine base P (HOST, 2 NP words, all-0xFF = infinity) and n scalars
 *   rows:   tgt[i] = [k_i] P_i   n affine bases (all-0xFF rows stay infinity)
 *   powers: tgt[i] = [a tau^i] P a, tau one Montgomery Fr each (HOST; a NULL = 1): the KZG `taus`
 * Scalars are rows of 4 words: expos_mont = 1 Montgomery Fr, brought to canonical standard form first;
 * expos_mont = 0 raw 256-bit integers used verbatim (values >= r, up to 2^256 - 1, included).  The
 * multiplication is by the integer, so the result equals the reference's for every on-curve base, also
 * outside the order-r subgroup.  That includes the one place where the reference's row is not the group's:
 * for a base of order 3 (x = 0: (0, +-2) on BLS12-381; BN128 has none) its 4-bit table holds the double of
 * infinity as (0 : 0 : 0), which absorbs every sum, so a scalar with a hexadecimal digit 6, 7 or c .. f gives
 * infinity there and here, whatever k mod 3 is (DESIGN.md "Batch scalar multiplication").  Target rows: affine_out = 0 normalised projective (x : y : 1), infinity
 * (0 : 1 : 0), 3 NP words; affine_out = 1 affine (x, y), infinity all-0xFF, 2 NP words.
 * Returns 0, or -1 with nothing written for n < 0 or a curve that is neither ZKG_BN128 nor ZKG_BLS12_381.
 * n == 0 is a no-op.  Outputs alias no input; nothing outside rows [0, n) of the target is written.
 * Synchronous and thread-safe, on the calling thread's device; device errors go through the error
 * channel (zkg_set_error_mode / zkg_last_error). */
ZKG_API int zkg_g1_scl_fixed_device(int curve, int n, const uint64_t *d_expos, int expos_mont,
                                    const uint64_t *base_affine, int affine_out, uint64_t *d_tgt);  /* DEVICE expos, tgt */
ZKG_API int zkg_g1_scl_fixed(int curve, int n, const uint64_t *expos, int expos_mont, const uint64_t *base_affine,
                             int affine_out, uint64_t *tgt);                                        /* HOST pointers */
ZKG_API int zkg_g1_scl_rows_device(int curve, int n, const uint64_t *d_expos, int expos_mont, const uint64_t *d_bases,
                                   int affine_out, uint64_t *d_tgt);                                /* DEVICE pointers */
ZKG_API int zkg_g1_scl_rows(int curve, int n, const uint64_t *expos, int expos_mont, const uint64_t *bases,
                            int affine_out, uint64_t *tgt);                                         /* HOST pointers */
ZKG_API int zkg_g1_scl_powers_device(int curve, int n, const uint64_t *a, const uint64_t *tau,
                                     const uint64_t *base_affine, int affine_out, uint64_t *d_tgt); /* DEVICE tgt */
ZKG_API int zkg_g1_scl_powers(int curve, int n, const uint64_t *a, const uint64_t *tau, const uint64_t *base_affine,
                              int affine_out, uint64_t *tgt);                                       /* HOST tgt */
/* test hooks.  set_window: the window c of the fixed-base table (0 restores the default; other values
 * are clamped to 2..16).  set_fixed_min: fixed-base and powers calls below n rows take the per-row
 * kernel instead of building the table (< 0: the default, 0: never).  last_path: 0 when the most recent
 * fixed-base or powers call ran the per-row kernel (or built no table: base at infinity), else the
 * window its table path ran with.  The results do not depend on either setting. */
ZKG_API void zkg_g1_scl_set_window(int c);
ZKG_API void zkg_g1_scl_set_fixed_min(int n);
ZKG_API int  zkg_g1_scl_last_path(void);
/* the signed-window recoding of the fixed-base kernel (no GPU call): digits[w], w < W = ceil(257 / c), of
 * the 256-bit integer k with sum_w digits[w] 2^(c w) = k and |digits[w]| <= 2^(c - 1); at most cap
 * entries are written.  Returns W, or -1 for c outside 2..16. */
ZKG_API int  zkg_g1_scl_digits(int c, const uint64_t k[4], int *digits, int cap);
/* bytes of the fixed-base table for window c (clamped to 2..16): 2^(c-1) ceil(257 / c) rows of 2 NP
 * words (no GPU call); 0 for an unknown curve */
ZKG_API size_t zkg_g1_scl_table_bytes(int curve, int c);

/* Batch G2 scalar multiplication: the mirror of the G1 set above on the twist (the reference's
 * <C>_G2_proj_scl_Fr_mont / _scl_Fr_std, G2_proj.c:453-480, followed by _normalize or _to_affine, once per
 * row).  Same arguments, same return codes, same scalar rows.  A coordinate is an Fp2 element c0 || c1, so
 * here NP = 8 (BN128) / 12 (BLS12-381) words: an affine row x.c0 x.c1 y.c0 y.c1 is 2 NP words (all-0xFF =
 * infinity), a target row 3 NP (affine_out = 0: (x : y : 1), infinity (0 : 1 : 0)) or 2 NP words
 * (affine_out = 1).  Contract: the multiplication is by the INTEGER value of the scalar -- nothing is reduced
 * mod r -- so the rows equal the reference's for every on-curve base, also outside the order-r subgroup of
 * the twist (both twists have a cofactor).  No reference special case arises on G2: neither twist order
 * has a factor <= 7, so every row is the group's multiple (DESIGN.md "Batch G2 scalar multiplication").
 * Returns 0, or -1 with nothing written for n < 0 or an unknown curve; n == 0 is a no-op. */
ZKG_API int zkg_g2_scl_fixed_device(int curve, int n, const uint64_t *d_expos, int expos_mont,
                                    const uint64_t *base_affine, int affine_out, uint64_t *d_tgt);  /* DEVICE expos, tgt */
ZKG_API int zkg_g2_scl_fixed(int curve, int n, const uint64_t *expos, int expos_mont, const uint64_t *base_affine,
                             int affine_out, uint64_t *tgt);                                        /* HOST pointers */
ZKG_API int zkg_g2_scl_rows_device(int curve, int n, const uint64_t *d_expos, int expos_mont, const uint64_t *d_bases,
                                   int affine_out, uint64_t *d_tgt);                                /* DEVICE pointers */
ZKG_API int zkg_g2_scl_rows(int curve, int n, const uint64_t *expos, int expos_mont, const uint64_t *bases,
                            int affine_out, uint64_t *tgt);                                         /* HOST pointers */
ZKG_API int zkg_g2_scl_powers_device(int curve, int n, const uint64_t *a, const uint64_t *tau,
                                     const uint64_t *base_affine, int affine_out, uint64_t *d_tgt); /* DEVICE tgt */
ZKG_API int zkg_g2_scl_powers(int curve, int n, const uint64_t *a, const uint64_t *tau, const uint64_t *base_affine,
                              int affine_out, uint64_t *tgt);                                       /* HOST tgt */
/* test hooks of the G2 entries, as the G1 ones, with a state of their own (the defaults differ per group) */
ZKG_API void zkg_g2_scl_set_window(int c);
ZKG_API void zkg_g2_scl_set_fixed_min(int n);
ZKG_API int  zkg_g2_scl_last_path(void);
/* bytes of the G2 fixed-base table for window c (clamped to 2..16): 2^(c-1) ceil(257 / c) rows of 2 NP
 * words (no GPU call); 0 for an unknown curve */
ZKG_API size_t zkg_g2_scl_table_bytes(int curve, int c);

/* host helpers on G1 (projective, reference Montgomery form) */
ZKG_API void zkg_g1_proj_add(int curve, const uint64_t *a, const uint64_t *b, uint64_t *out);
ZKG_API void zkg_g1_proj_normalize(int curve, const uint64_t *a, uint64_t *out);
ZKG_API void zkg_g1_proj_to_affine(int curve, const uint64_t *a, uint64_t *out);

/* deterministic synthetic inputs (spec: zikkurat-algebra_amd/csrc/zk_gen.cpp) */
ZKG_API void zkg_gen_fr(int curve, uint64_t seed, int64_t start, int64_t count, uint64_t *out);
ZKG_API void zkg_gen_g1_points(int curve, uint64_t seed, int64_t start, int64_t count, uint64_t *out);
/* Montgomery generator of the order-2^m subgroup: fftDomain gen^(2^(M-m))
 * (Class/FFT.hs:60-66; BLS12_381/Fr/Mont.hs:145-151, BN128/Fr/Mont.hs:146-148) */
ZKG_API void zkg_fft_generator(int curve, int m, uint64_t *out);

/* MSM window heuristic used when window_size is not given */
ZKG_API int zkg_msm_default_window(int npoints);
/* the window a G1 MSM of `npoints` pairs runs with by default on `curve` (ZKG_BN128 /
 * ZKG_BLS12_381) for its scalar form (Montgomery Fr, or std integers of expo_nlimbs limbs):
 * zkg_msm_default_window's table, made curve-aware where a full top window measured faster */
ZKG_API int zkg_msm_window(int curve, int npoints, int expo_nlimbs, int expos_mont);

/* per-phase HIP-event profile of every MSM call, printed to stderr (diagnostics) */
ZKG_API void zkg_msm_profile(int on);
/* test hook: cap on the sorted (window, point) entries one MSM pipeline pass handles
 * (default and maximum 2^30; 0 restores it).  Larger MSMs run in window groups. */
ZKG_API void zkg_msm_set_group_limit(size_t entries);
/* test hook: the G1 MSM's Y-sum kernel -- -1: by size (k_ysum3, two waves per SIMD, when the
 * Y-sum lanes fill several rounds of the chip: c = 20 from 2^23 pairs), 0: always k_ysum2,
 * 1: always k_ysum3 (block-level shapes, c >= 12) */
ZKG_API void zkg_msm_set_ysum_mode(int mode);
/* test hook: device-resident G1/G2 MSMs of at least 2^lg pairs whose windows fit one pass run as
 * two window groups with both bucket sorts on a second stream (B's beside A's accumulation);
 * lg = 0 disables it, lg < 0 restores the default: from 2^23 pairs (or the environment's
 * ZK_MSM_AHEAD_MIN) for the curves whose accumulation leaves VGPRs for the sort (BN128 G1), off
 * otherwise */
ZKG_API void zkg_msm_set_ahead_min(int lg);
/* test hook: NTT pass split -- 12: two passes of 2^9..2^12-point DFTs (4096-element tiles) for
 * every 2^17..2^24; 8: passes of <= 2^8-point DFTs only; 0: the default (two passes at 2^20 only) */
ZKG_API void zkg_ntt_set_max_radix(int r);
/* test hook: inter-pass twiddle table entries above which an NTT pass computes its twiddles on
 * the fly (default 2^25, i.e. only transforms of 2^26 and more; 0 restores it) */
ZKG_API void zkg_ntt_set_table_max(size_t entries);
/* test hook: blocks per launch of the batched pass kernel of zkg_ntt_ext* (a pass with more tiles
 * runs as several launches; default and maximum 2^21, 0 restores it) */
ZKG_API void zkg_ntt_ext_set_max_grid(unsigned tiles);
/* test hook: device bytes of cached NTT twiddle sets one context keeps; building a set that would
 * exceed it first frees the least recently used ones (default 8 GiB; 0 restores it) */
ZKG_API void zkg_ntt_set_cache_limit(size_t bytes);
/* device bytes of the NTT twiddle sets and coset shift tables cached for the calling thread's device */
ZKG_API size_t zkg_ntt_cache_bytes(void);
/* test hook: device bytes one working-set arena may hold (0: unlimited), to exercise the
 * out-of-memory degrade path (smaller MSM window groups) */
ZKG_API void zkg_arena_set_limit(size_t bytes);
/* window groups (pipeline passes) of the most recent single-device MSM pass */
ZKG_API int zkg_msm_last_groups(void);
/* 1 when the most recent group FFT (G1 fft / ifft) ran the GLV stages (every input point in the
 * order-r subgroup), 0 when it ran the integer-scalar stages */
ZKG_API int zkg_g1_fft_last_glv(void);
/* the GLV-stage plan of a 2^m group FFT (zk_g1ext.hip radix_plan): writes the bits of each
 * Stockham radix-2^b stage into bits[0..cap) and returns the stage count (0: the fused radix-2
 * stages, m of them); zkg_g1_fft_radix_products(b) = GLV lane-pair products per group of 2^b points */
ZKG_API int zkg_g1_fft_plan(int curve, int m, int *bits, int cap);
ZKG_API int zkg_g1_fft_radix_products(int b);
/* device bytes of one G1 MSM's working set (the arena it reserves) with its windows split into
 * `groups` passes; window_size <= 0: the default window */
ZKG_API size_t zkg_msm_workspace_bytes(int curve, int npoints, int expo_nlimbs, int expos_mont, int host_inputs,
                                       int window_size, int groups);

/* Batch optimal-ate pairings (the reference's <C>_pairing_affine / _pairing_projective / _pairing_final_expo,
 * lib/cbits/curves/pairing/<C>_pairing.c), NP = 4 (BN128) or 6 (BLS12-381) u64 words per Fp:
 *   P rows    affine G1, 2 NP words (x || y, Montgomery form); all-0xFF = infinity
 *   Q rows    affine G2, 4 NP words (x.c0 x.c1 y.c0 y.c1); all-0xFF = infinity
 *   Fp12 rows 12 NP words, 2 x 3 x 2 Fp in Montgomery form (the reference's Fp12 layout)
 * Every row equals <C>_pairing_affine(P_i, Q_i) bit for bit; a row whose P or Q is infinity gives Montgomery
 * one.  Domain: the rows are on-curve points of the order-r subgroups, or infinity.  For any other input the
 * result is unspecified, but the call terminates and does not fault (every trip count is fixed); there is no
 * subgroup or on-curve check here (zkg_g1_check_rows / zkg_g2_check_rows below are that check).
 * zkg_pairing_product: one Fp12 row, prod_i pairing(P_i, Q_i), with a single final exponentiation over the
 * device-side product of the Miller values (infinity rows contribute one; n = 0 gives one).
 * zkg_pairing_final_expo: row i = src_i^((p^12 - 1)/r) = <C>_pairing_final_expo for nonzero rows.
 * Return 0, or -1 (negative n, unknown curve, null buffer, device error; the error channel has the text). */
ZKG_API void bn128_pairing_affine(const uint64_t *P, const uint64_t *Q, uint64_t *tgt);
ZKG_API void bn128_pairing_projective(const uint64_t *P, const uint64_t *Q, uint64_t *tgt);
ZKG_API void bls12_381_pairing_affine(const uint64_t *P, const uint64_t *Q, uint64_t *tgt);
ZKG_API void bls12_381_pairing_projective(const uint64_t *P, const uint64_t *Q, uint64_t *tgt);
ZKG_API int zkg_pairing_rows(int curve, int n, const uint64_t *P, const uint64_t *Q, uint64_t *tgt);
ZKG_API int zkg_pairing_rows_device(int curve, int n, const uint64_t *d_P, const uint64_t *d_Q, uint64_t *d_tgt);
ZKG_API int zkg_pairing_product(int curve, int n, const uint64_t *P, const uint64_t *Q, uint64_t *tgt);
ZKG_API int zkg_pairing_product_device(int curve, int n, const uint64_t *d_P, const uint64_t *d_Q, uint64_t *d_tgt);
ZKG_API int zkg_pairing_final_expo(int curve, int n, const uint64_t *src, uint64_t *tgt);
ZKG_API int zkg_pairing_final_expo_device(int curve, int n, const uint64_t *d_src, uint64_t *d_tgt);

/* Batch point validation: what a caller runs on points it was handed (a proof, a commitment, an SRS file)
 * before the entries above, whose domain is the order-r subgroup.  Row i of `pts` is one point in the
 * coordinate system `coords` (Montgomery words as everywhere; G1: NP = 4 / 6 words per coordinate, G2:
 * NP = 8 / 12, c0 || c1), and flags[i] receives one byte:
 *   ZKG_PT_CANONICAL    every coordinate, read as an integer (per Fp component), is < p; the affine all-0xFF
 *                       row (infinity) is canonical too, and is the only row with a coordinate >= p that is.
 *                       A row that is not canonical has the other three flags cleared, whatever its words.
 *   ZKG_PT_ON_CURVE     the reference's <C>_G{1,2}_{affine,proj,jac}_is_on_curve of that coordinate system:
 *   ZKG_PT_INFINITY     ... and its _is_infinity.  Affine infinity (all-0xFF) is on the curve; projective
 *                       infinity is (0 : Y : 0) with Y != 0, so (X : Y : 0) with X != 0 and (0 : 0 : 0) are not on
 *                       the curve; Jacobian infinity is (X : Y : 0) with Y^2 = X^3, X, Y != 0.
 *   ZKG_PT_IN_SUBGROUP  ON_CURVE and [r]P = O; infinity is a member.  This is deliberately NOT the reference's
 *                       _is_in_subgroup: that routine multiplies by the curve's cofactor constant instead of r
 *                       (and reads 4 limbs of it), so it answers 0 for the subgroup generator of all four
 *                       groups and 1 only at infinity, while its own scl_Fr_std(r, generator) is infinity.
 *                       The definition here is [r]P = O with the reference's scalar multiplication as oracle.
 * Return value: the number of rows that lack any of CANONICAL | ON_CURVE | IN_SUBGROUP (0: the batch is
 * valid), counted on the device; flags may be NULL for the count alone.  -1 with nothing written for n < 0,
 * an unknown curve or coords, or ZKG_COORDS_JAC on G2 (a return code: the error channel stays clear), and -1
 * with the error channel set for a device error.  n == 0 returns 0.  Inputs are never written and nothing
 * outside flag bytes [0, n) is; the calls are synchronous, thread-safe and run on the calling thread's
 * device.  No data-dependent trip count: rows that are not points cost what points cost and nothing faults.
 * zkg_check_set_mode (test hook): 0 the default membership chains (BN128 G1: cofactor 1, none; BLS12-381 G1:
 * phi(P) == [z^2 - 1]P; BLS12-381 G2: psi(P) == [z]P; BN128 G2: [x + 1]P + psi([x]P) + psi^2([x]P) ==
 * psi^3([2x]P)), 1 the exact chain [r]P everywhere (the definition), 2 the curve pass alone (a measurement
 * hook: IN_SUBGROUP stays clear on finite rows, which therefore count as failing), < 0 restores the default.
 * zkg_check_set_max_lanes (test hook, as zkg_g2_fft_set_max_lanes): lanes of the membership kernel, so that
 * its grid-stride loop runs at small n; <= 0 restores the default. */
#define ZKG_PT_CANONICAL 1
#define ZKG_PT_ON_CURVE 2
#define ZKG_PT_IN_SUBGROUP 4
#define ZKG_PT_INFINITY 8
#define ZKG_COORDS_AFFINE 0 /* 2 NP words */
#define ZKG_COORDS_PROJ 1   /* 3 NP words */
#define ZKG_COORDS_JAC 2    /* 3 NP words, G1 only */
ZKG_API int zkg_g1_check_rows(int curve, int n, const uint64_t *pts, int coords, uint8_t *flags);
ZKG_API int zkg_g1_check_rows_device(int curve, int n, const uint64_t *d_pts, int coords, uint8_t *d_flags);
ZKG_API int zkg_g2_check_rows(int curve, int n, const uint64_t *pts, int coords, uint8_t *flags);
ZKG_API int zkg_g2_check_rows_device(int curve, int n, const uint64_t *d_pts, int coords, uint8_t *d_flags);
ZKG_API void zkg_check_set_mode(int mode);
ZKG_API void zkg_check_set_max_lanes(int lanes);

/* Row-wise sum of scalar multiples: tgt[i] = sum_(j < terms) [k_(j,i)] P_(j,i), i < rows.  Term-major layout:
 * term j's rows lie at j * rows + i in `expos` (4 words each) and `bases` (affine rows, 2 NP words, all-0xFF =
 * infinity).  The contract of zkg_g1_scl_rows holds per product (expos_mont: Montgomery Fr brought to its
 * canonical integer, otherwise raw 256-bit integers; no reduction mod r).  Equal terms, opposite terms and
 * infinities are ordinary inputs; terms = 0 gives rows of infinity.  tgt: `rows` normalised projective rows
 * (3 NP words), or affine rows (affine_out).  Returns 0, or -1 with the error channel set and nothing written:
 * unknown curve, negative size, rows * terms >= 2^31, null buffer, tgt overlapping an input, device error. */
ZKG_API int zkg_g1_scl_rows_sum_device(int curve, int rows, int terms, const uint64_t *d_expos, int expos_mont,
                                       const uint64_t *d_bases, int affine_out, uint64_t *d_tgt);
ZKG_API int zkg_g1_scl_rows_sum(int curve, int rows, int terms, const uint64_t *expos, int expos_mont,
                                const uint64_t *bases, int affine_out, uint64_t *tgt);

/* Every KZG opening of a domain at once (Feist-Khovratovich).  n = 2^log_n, l = 2^log_l (0 <= log_l <=
 * log_n - 1), r = n / l, omega the generator of zkg_fft_generator(curve, log_n), psi = omega^l.  Proof k < r is
 * the commitment to the quotient of the polynomial by x^l - psi^k: it opens the coset omega^k <omega^r>, and
 * for l = 1 it is the proof of zkg_kzg_open_device at omega^k.
 *   zkg_kzg_open_all_table_bytes   bytes of the table of (log_n, log_l): 2 n affine rows (0 for a refused shape)
 *   zkg_kzg_open_all_table_device  builds it from d_srs_affine, the first n affine rows [tau^i] g1: l group
 *                                  FFTs of size 2 r, term-major; once per setup and (log_n, log_l)
 *   zkg_kzg_open_all_device        d_poly: npoly <= n Montgomery coefficients (zero-extended); d_proofs: r
 *                                  normalised projective rows, or affine (affine_out)
 * Return 0, or -1 with the error channel set and nothing written: unknown curve, log_n outside 1..28, log_l
 * outside 0..log_n - 1, a 2 r domain beyond the field's 2-adicity or the group FFT's 2^26, npoly outside 0..n,
 * a null buffer, overlapping buffers, a device error.  Synchronous, on the calling thread's device. */
ZKG_API size_t zkg_kzg_open_all_table_bytes(int curve, int log_n, int log_l);
ZKG_API int zkg_kzg_open_all_table_device(int curve, int log_n, int log_l, const uint64_t *d_srs_affine,
                                          uint64_t *d_table);
ZKG_API int zkg_kzg_open_all_device(int curve, int log_n, int log_l, int npoly, const uint64_t *d_poly,
                                    const uint64_t *d_table, int affine_out, uint64_t *d_proofs);

/* timing probe of the dominant kernel (MSM bucket accumulation / NTT pass chain),
 * measured with HIP events on each device's own stream; read sums over devices */
ZKG_API void zkg_timer_enable(int on);
ZKG_API void zkg_timer_reset(void);
ZKG_API void zkg_timer_read(double *total_ms, long *launches);

#ifdef __cplusplus
}
#endif
#endif /* ZKALGEBRA_GPU_H */
