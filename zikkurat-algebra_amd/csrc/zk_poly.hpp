// zk_poly.hpp -- C++ interface of the device polynomial layer (zk_poly.hip).
//
// Replaces the reference's generated per-curve polynomial code
//   <C>_poly_mont_mul_naive   lib/cbits/curves/poly/mont/bls12_381_poly_mont.c:199-222
//   <C>_poly_mont_eval_at     bls12_381_poly_mont.c:225-243
//   <C>_poly_mont_lincomb     bls12_381_poly_mont.c:169-195
// (bn128_poly_mont.c same lines).  Coefficients are Fr in the reference's Montgomery form
// (4 x u64, canonical); every result is the canonical representative, so it is bit-identical to
// the reference's loops whatever schedule computes it.
#pragma once
#include <stdint.h>

namespace zk {

// largest product (n1 + n2 - 1 coefficients) as log2: the 2-adicity of BN128's Fr, and ntt's
// own limit on BLS12-381
constexpr int POLY_MUL_MAX_LOG[2] = {28, 30};

// tgt[0, n1 + n2 - 1) = a * b.  Host or device pointers (host_io); a may equal b (squaring),
// tgt aliases neither.  Returns 0, or -1 (nothing done) when n1 + n2 - 1 > 2^POLY_MUL_MAX_LOG.
// n1 + n2 - 1 <= 0 writes nothing; one length 0 and the other n >= 2 writes n - 1 zeros (the
// reference's loop, poly_mont.c:203-221).
int poly_mul(int curve, int n1, const uint64_t *a, int n2, const uint64_t *b, uint64_t *tgt, bool host_io);
// *tgt_host = poly(x); x and tgt_host are single HOST elements; n <= 0 gives 0
void poly_eval(int curve, int n, const uint64_t *poly, const uint64_t *x, uint64_t *tgt_host, bool host_io);
// tgt[i] = sum over the k with ns[k] > i of coeffs[k] * polys[k][i], i < max ns[k].  ns, coeffs
// (K x 4 u64) and the pointer array polys are host memory; polys[k] and tgt are host or device
// pointers (host_io).  K = 0 writes nothing.
void poly_lincomb(int curve, int K, const int *ns, const uint64_t *coeffs, const uint64_t *const *polys,
                  uint64_t *tgt, bool host_io);
// test hooks: the direct kernel takes a product whose shorter factor has <= len coefficients
// (0: always the transform, < 0: the default); the path of the most recent product (0 direct,
// else log2 of the transform size)
void poly_set_mul_direct_max(int len);
int poly_last_mul_path();

// p = quot * d + rem with deg rem < deg d: the contract of <C>_poly_mont_long_div
// (bls12_381_poly_mont.c:249-297), computed by Newton inversion of the reversed divisor over the
// NTT.  Host or device pointers (host_io); quot and / or rem may be null (the reference's rem and
// quot) and are then never touched; with dp, dq the degrees, quot[0, dp - dq] and rem[0, dq) are
// written and the rest of nquot / nrem rows is zero; dq < 0 zeroes both; dp < dq gives quotient 0 and
// remainder p.  Returns 0, or -1 with nothing written for a negative length, quot with
// nquot < dp - dq + 1, rem with nrem < dq (nrem < dp + 1 when dp < dq), or
// n1 > 2^(POLY_MUL_MAX_LOG - 1) -- that last check before any pointer is read or a device is opened.
int poly_long_div(int curve, int n1, const uint64_t *p, int n2, const uint64_t *d, int nquot, uint64_t *quot, int nrem,
                  uint64_t *rem, bool host_io);
// test hooks.  Terms of the series inverse's base kernel (< 0: the default, 0 and 1: one term,
// above the kernel's capacity: the capacity) and the value in force; the precision plan for a
// quotient of m coefficients (returns the Newton steps s, writes prec[0 .. s] up to cap entries; -1
// for m <= 0; no GPU call); the Newton steps of the most recent division (-1: it took an early exit)
void poly_set_div_base_max(int len);
int poly_div_base_max();
int poly_div_plan(int m, int *prec, int cap);
int poly_last_div_steps();
// timing hook (tools/poly_div_time.py): while on, a division records HIP events around its three
// phases; ms[0..2] = series inverse, quotient, remainder of the most recent profiled division
void poly_div_profile(int on);
void poly_last_div_phase_ms(double *ms);

}  // namespace zk
