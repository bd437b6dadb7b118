// zk_capi_arr.cpp -- extern "C" boundary of the Fr vector operations.
//
// One entry per symbol of the reference's generated headers, same signature:
//   lib/cbits/curves/array/mont/bls12_381_arr_mont.h:3-48   (bn128_arr_mont.h same lines)
//   lib/cbits/curves/poly/mont/bls12_381_poly_mont.h:22-23  (div/quot_by_vanishing)
// bound by Haskell's ZK.Algebra.Curves.<C>.Array (Array.hs:108-352) and Poly.hs.  All
// of them run on the GPU (zk_arr.hip); buffers are host memory, staged per call.
#include <string.h>
#include "../../include/zkalgebra_gpu.h"
#include "zk_arr.hpp"
#include "zk_host.hpp"
#include "zk_runtime.hpp"

using namespace zk;
#include "zk_g1ext.hpp"

// catch points of the recoverable error mode (zk_runtime.hpp guard): every entry point below
// calls the library through these, so no zk::Error crosses the C ABI
namespace {
void arr_op_g(int curve, int op, int n, const uint64_t *a, const uint64_t *b, const uint64_t *c, const uint64_t *kA,
              const uint64_t *kB, uint64_t *tgt, bool host_io) {
  guard([&] { zk::arr_op(curve, op, n, a, b, c, kA, kB, tgt, host_io); });
}
int arr_pred_g(int curve, int pred, int n, const uint64_t *a, const uint64_t *b, bool host_io) {
  return guard_ret(0, [&] { return zk::arr_pred(curve, pred, n, a, b, host_io); });
}
void arr_dot_g(int curve, int n, const uint64_t *a, const uint64_t *b, uint64_t *tgt, bool host_io) {
  guard([&] { zk::arr_dot(curve, n, a, b, tgt, host_io); });
}
void arr_powers_g(int curve, int n, const uint64_t *kA, const uint64_t *kB, uint64_t *tgt, bool host_io) {
  guard([&] { zk::arr_powers(curve, n, kA, kB, tgt, host_io); });
}
int poly_div_g(int curve, int n1, const uint64_t *src, int expo_n, const uint64_t *eta, int nquot, uint64_t *quot,
               int nrem, uint64_t *rem, bool host_io) {
  return guard_ret(0, [&] { return zk::poly_div_by_vanishing(curve, n1, src, expo_n, eta, nquot, quot, nrem, rem, host_io); });
}
void from_affine_g(int curve, int n, const uint64_t *src, uint64_t *tgt, bool host_io, bool jac = false) {
  guard([&] { zk::g1_batch_from_affine(curve, n, src, tgt, host_io, jac); });
}
void to_affine_g(int curve, int n, const uint64_t *src, uint64_t *tgt, bool host_io, bool jac = false) {
  guard([&] { zk::g1_batch_to_affine(curve, n, src, tgt, host_io, jac); });
}
void fft_g(int curve, int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt, bool host_io, bool inverse,
           bool jac = false) {
  guard([&] { zk::g1_fft(curve, m, gen, src, tgt, host_io, inverse, jac); });
}
}  // namespace

ZKG_API int zkg_g1_fft_last_glv(void) { return zk::g1_fft_last_glv().load(); }
ZKG_API int zkg_g1_fft_plan(int curve, int m, int *bits, int cap) { return zk::g1_fft_plan(curve, m, bits, cap); }
ZKG_API int zkg_g1_fft_radix_products(int b) { return zk::g1_fft_radix_products(b); }

namespace {
const uint64_t kZero[4] = {0, 0, 0, 0};
template <class Fh>
const uint64_t *mont_one() { return Fh::ONE; }
}  // namespace

extern "C" {

#define ZKG_ARR_ENTRIES(PFX, CID, FH)                                                                               \
  ZKG_API uint8_t PFX##_arr_mont_is_valid(int n, const uint64_t *s) { return (uint8_t)arr_pred_g(CID, PRED_IS_VALID, n, s, nullptr, true); } \
  ZKG_API uint8_t PFX##_arr_mont_is_zero(int n, const uint64_t *s) { return (uint8_t)arr_pred_g(CID, PRED_IS_ZERO, n, s, nullptr, true); }   \
  ZKG_API uint8_t PFX##_arr_mont_is_one(int n, const uint64_t *s) { return (uint8_t)arr_pred_g(CID, PRED_IS_ONE, n, s, nullptr, true); }     \
  ZKG_API uint8_t PFX##_arr_mont_is_equal(int n, const uint64_t *a, const uint64_t *b) {                            \
    return (uint8_t)arr_pred_g(CID, PRED_IS_EQUAL, n, a, b, true);                                                    \
  }                                                                                                                 \
  ZKG_API void PFX##_arr_mont_set_zero(int n, uint64_t *t) { arr_op_g(CID, ARR_SET_CONST, n, 0, 0, 0, kZero, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_set_one(int n, uint64_t *t) {                                                        \
    arr_op_g(CID, ARR_SET_CONST, n, 0, 0, 0, mont_one<FH>(), 0, t, true);                                            \
  }                                                                                                                 \
  ZKG_API void PFX##_arr_mont_set_const(int n, const uint64_t *s, uint64_t *t) { arr_op_g(CID, ARR_SET_CONST, n, 0, 0, 0, s, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_copy(int n, const uint64_t *s, uint64_t *t) { arr_op_g(CID, ARR_COPY, n, s, 0, 0, 0, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_from_std(int n, const uint64_t *s, uint64_t *t) { arr_op_g(CID, ARR_FROM_STD, n, s, 0, 0, 0, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_to_std(int n, const uint64_t *s, uint64_t *t) { arr_op_g(CID, ARR_TO_STD, n, s, 0, 0, 0, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_append(int n1, int n2, const uint64_t *s1, const uint64_t *s2, uint64_t *t) {         \
    arr_op_g(CID, ARR_COPY, n1, s1, 0, 0, 0, 0, t, true);                                                             \
    arr_op_g(CID, ARR_COPY, n2, s2, 0, 0, 0, 0, t + 4 * (size_t)(n1 > 0 ? n1 : 0), true);                             \
  }                                                                                                                 \
  ZKG_API void PFX##_arr_mont_neg(int n, const uint64_t *s, uint64_t *t) { arr_op_g(CID, ARR_NEG, n, s, 0, 0, 0, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_add(int n, const uint64_t *a, const uint64_t *b, uint64_t *t) { arr_op_g(CID, ARR_ADD, n, a, b, 0, 0, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_sub(int n, const uint64_t *a, const uint64_t *b, uint64_t *t) { arr_op_g(CID, ARR_SUB, n, a, b, 0, 0, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_sqr(int n, const uint64_t *s, uint64_t *t) { arr_op_g(CID, ARR_SQR, n, s, 0, 0, 0, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_mul(int n, const uint64_t *a, const uint64_t *b, uint64_t *t) { arr_op_g(CID, ARR_MUL, n, a, b, 0, 0, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_inv(int n, const uint64_t *s, uint64_t *t) { arr_op_g(CID, ARR_INV, n, s, 0, 0, 0, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_div(int n, const uint64_t *a, const uint64_t *b, uint64_t *t) { arr_op_g(CID, ARR_DIV, n, a, b, 0, 0, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_neg_inplace(int n, uint64_t *t) { arr_op_g(CID, ARR_NEG, n, t, 0, 0, 0, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_add_inplace(int n, uint64_t *t, const uint64_t *b) { arr_op_g(CID, ARR_ADD, n, t, b, 0, 0, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_sub_inplace(int n, uint64_t *t, const uint64_t *b) { arr_op_g(CID, ARR_SUB, n, t, b, 0, 0, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_sqr_inplace(int n, uint64_t *t) { arr_op_g(CID, ARR_SQR, n, t, 0, 0, 0, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_mul_inplace(int n, uint64_t *t, const uint64_t *b) { arr_op_g(CID, ARR_MUL, n, t, b, 0, 0, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_inv_inplace(int n, uint64_t *t) { arr_op_g(CID, ARR_INV, n, t, 0, 0, 0, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_div_inplace(int n, uint64_t *t, const uint64_t *b) { arr_op_g(CID, ARR_DIV, n, t, b, 0, 0, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_sub_inplace_reverse(int n, uint64_t *t, const uint64_t *s1) {                         \
    arr_op_g(CID, ARR_SUB_REV, n, t, s1, 0, 0, 0, t, true);                                                           \
  }                                                                                                                 \
  ZKG_API void PFX##_arr_mont_mul_add(int n, const uint64_t *a, const uint64_t *b, const uint64_t *c, uint64_t *t) { \
    arr_op_g(CID, ARR_MUL_ADD, n, a, b, c, 0, 0, t, true);                                                            \
  }                                                                                                                 \
  ZKG_API void PFX##_arr_mont_mul_sub(int n, const uint64_t *a, const uint64_t *b, const uint64_t *c, uint64_t *t) { \
    arr_op_g(CID, ARR_MUL_SUB, n, a, b, c, 0, 0, t, true);                                                            \
  }                                                                                                                 \
  ZKG_API void PFX##_arr_mont_dot_prod(int n, const uint64_t *a, const uint64_t *b, uint64_t *t) { arr_dot_g(CID, n, a, b, t, true); } \
  ZKG_API void PFX##_arr_mont_powers(int n, const uint64_t *kA, const uint64_t *kB, uint64_t *t) { arr_powers_g(CID, n, kA, kB, t, true); } \
  ZKG_API void PFX##_arr_mont_scale(int n, const uint64_t *k, const uint64_t *s, uint64_t *t) { arr_op_g(CID, ARR_SCALE, n, s, 0, 0, k, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_scale_inplace(int n, const uint64_t *k, uint64_t *t) { arr_op_g(CID, ARR_SCALE, n, t, 0, 0, k, 0, t, true); } \
  ZKG_API void PFX##_arr_mont_Ax_plus_y(int n, const uint64_t *kA, const uint64_t *x, const uint64_t *y, uint64_t *t) { \
    arr_op_g(CID, ARR_AXPY, n, x, y, 0, kA, 0, t, true);                                                              \
  }                                                                                                                 \
  ZKG_API void PFX##_arr_mont_Ax_plus_y_inplace(int n, const uint64_t *kA, uint64_t *t, const uint64_t *y) {        \
    arr_op_g(CID, ARR_AXPY, n, t, y, 0, kA, 0, t, true);                                                              \
  }                                                                                                                 \
  ZKG_API void PFX##_arr_mont_Ax_plus_By(int n, const uint64_t *kA, const uint64_t *kB, const uint64_t *x,          \
                                         const uint64_t *y, uint64_t *t) {                                          \
    arr_op_g(CID, ARR_AXPBY, n, x, y, 0, kA, kB, t, true);                                                            \
  }                                                                                                                 \
  ZKG_API void PFX##_arr_mont_Ax_plus_By_inplace(int n, const uint64_t *kA, const uint64_t *kB, uint64_t *t,        \
                                                 const uint64_t *y) {                                               \
    arr_op_g(CID, ARR_AXPBY, n, t, y, 0, kA, kB, t, true);                                                            \
  }                                                                                                                 \
  ZKG_API void PFX##_poly_mont_div_by_vanishing(int n1, const uint64_t *s, int expo_n, const uint64_t *eta,         \
                                                int nquot, uint64_t *quot, int nrem, uint64_t *rem) {               \
    poly_div_g(CID, n1, s, expo_n, eta, nquot, quot, rem ? nrem : 0, rem, true);                        \
  }                                                                                                                 \
  ZKG_API uint8_t PFX##_poly_mont_quot_by_vanishing(int n1, const uint64_t *s, int expo_n, const uint64_t *eta,     \
                                                    int nquot, uint64_t *quot) {                                    \
    return (uint8_t)poly_div_g(CID, n1, s, expo_n, eta, nquot, quot, 0, nullptr, true);                 \
  }

ZKG_ARR_ENTRIES(bn128, ZKG_BN128, zkh::BN_Fr)
ZKG_ARR_ENTRIES(bls12_381, ZKG_BLS12_381, zkh::BLS_Fr)

// device-resident forms (pointers already in HBM; coefficients / scalar results on the host)
ZKG_API void zkg_arr_op_device(int curve, int op, int n, const uint64_t *d_a, const uint64_t *d_b,
                               const uint64_t *d_c, const uint64_t *kA, const uint64_t *kB, uint64_t *d_tgt) {
  arr_op_g(curve, op, n, d_a, d_b, d_c, kA, kB, d_tgt, false);
}
ZKG_API void zkg_arr_dot_device(int curve, int n, const uint64_t *d_a, const uint64_t *d_b, uint64_t *tgt) {
  arr_dot_g(curve, n, d_a, d_b, tgt, false);
}
ZKG_API void zkg_arr_powers_device(int curve, int n, const uint64_t *kA, const uint64_t *kB, uint64_t *d_tgt) {
  arr_powers_g(curve, n, kA, kB, d_tgt, false);
}
ZKG_API int zkg_poly_div_by_vanishing_device(int curve, int n1, const uint64_t *d_src, int expo_n,
                                             const uint64_t *eta, int nquot, uint64_t *d_quot, int nrem,
                                             uint64_t *d_rem) {
  return poly_div_g(curve, n1, d_src, expo_n, eta, nquot, d_quot, d_rem ? nrem : 0, d_rem, false);
}

}  // extern "C"

// ---------------------------------------------------------------------------- polynomial layer
// <C>_poly_mont_{degree,is_zero,is_equal,neg,add,sub,scale,lincomb,mul_naive,eval_at}
//   lib/cbits/curves/poly/mont/bls12_381_poly_mont.c:26-243, bound by Poly.hs:199-209.
// add / sub / neg / scale / is_zero / is_equal are the Fr vector ops above on the common prefix and
// the tail; the product, the evaluation and the linear combination are zk_poly.hip.
#include <vector>
#include "zk_poly.hpp"

namespace {
inline int nn(int n) { return n > 0 ? n : 0; }
// tgt[0, max) = a (+|-) b: the op on the common prefix, then the longer operand's tail copied
// (src1's, or src2's for add) or negated (src2's for sub), poly_mont.c:95-143
void poly_addsub_g(int curve, bool sub, int n1, const uint64_t *a, int n2, const uint64_t *b, uint64_t *t) {
  n1 = nn(n1);
  n2 = nn(n2);
  const int M = n1 < n2 ? n1 : n2;
  const size_t off = 4 * (size_t)M;
  arr_op_g(curve, sub ? ARR_SUB : ARR_ADD, M, a, b, 0, 0, 0, t, true);
  if (n1 > M) arr_op_g(curve, ARR_COPY, n1 - M, a + off, 0, 0, 0, 0, t + off, true);
  else if (n2 > M) arr_op_g(curve, sub ? ARR_NEG : ARR_COPY, n2 - M, b + off, 0, 0, 0, 0, t + off, true);
}
uint8_t poly_is_equal_g(int curve, int n1, const uint64_t *a, int n2, const uint64_t *b) {
  n1 = nn(n1);
  n2 = nn(n2);
  const int M = n1 < n2 ? n1 : n2;
  if (!arr_pred_g(curve, PRED_IS_EQUAL, M, a, b, true)) return 0;
  if (n1 > M) return (uint8_t)arr_pred_g(curve, PRED_IS_ZERO, n1 - M, a + 4 * (size_t)M, nullptr, true);
  if (n2 > M) return (uint8_t)arr_pred_g(curve, PRED_IS_ZERO, n2 - M, b + 4 * (size_t)M, nullptr, true);
  return 1;
}
void poly_mul_g(int curve, int n1, const uint64_t *a, int n2, const uint64_t *b, uint64_t *t) {
  guard([&] {
    ZK_REQUIRE(zk::poly_mul(curve, n1, a, n2, b, t, true) == 0,
               "poly_mul: n1 + n2 - 1 exceeds the largest transform of this curve");
  });
}
void poly_lincomb_g(int curve, int K, const int *ns, const uint64_t **coeffs, const uint64_t **polys, uint64_t *t) {
  guard([&] {
    std::vector<uint64_t> c((size_t)nn(K) * 4);
    for (int k = 0; k < K; k++) memcpy(&c[(size_t)k * 4], coeffs[k], 32);
    zk::poly_lincomb(curve, K, ns, c.data(), polys, t, true);
  });
}
}  // namespace

extern "C" {

#define ZKG_POLY_ENTRIES(PFX, CID)                                                                                  \
  ZKG_API int PFX##_poly_mont_degree(int n1, const uint64_t *s) {                                                   \
    return guard_ret(-1, [&] { return zk::poly_degree(CID, n1, s, true); });                                        \
  }                                                                                                                 \
  ZKG_API uint8_t PFX##_poly_mont_is_zero(int n1, const uint64_t *s) {                                              \
    return (uint8_t)arr_pred_g(CID, PRED_IS_ZERO, nn(n1), s, nullptr, true);                                        \
  }                                                                                                                 \
  ZKG_API uint8_t PFX##_poly_mont_is_equal(int n1, const uint64_t *a, int n2, const uint64_t *b) {                  \
    return poly_is_equal_g(CID, n1, a, n2, b);                                                                      \
  }                                                                                                                 \
  ZKG_API void PFX##_poly_mont_neg(int n1, const uint64_t *s, uint64_t *t) { arr_op_g(CID, ARR_NEG, nn(n1), s, 0, 0, 0, 0, t, true); } \
  ZKG_API void PFX##_poly_mont_add(int n1, const uint64_t *a, int n2, const uint64_t *b, uint64_t *t) {             \
    poly_addsub_g(CID, false, n1, a, n2, b, t);                                                                     \
  }                                                                                                                 \
  ZKG_API void PFX##_poly_mont_sub(int n1, const uint64_t *a, int n2, const uint64_t *b, uint64_t *t) {             \
    poly_addsub_g(CID, true, n1, a, n2, b, t);                                                                      \
  }                                                                                                                 \
  ZKG_API void PFX##_poly_mont_scale(const uint64_t *k, int n2, const uint64_t *s, uint64_t *t) {                   \
    arr_op_g(CID, ARR_SCALE, nn(n2), s, 0, 0, k, 0, t, true);                                                       \
  }                                                                                                                 \
  ZKG_API void PFX##_poly_mont_lincomb(int K, const int *ns, const uint64_t **coeffs, const uint64_t **polys,       \
                                       uint64_t *t) {                                                               \
    poly_lincomb_g(CID, K, ns, coeffs, polys, t);                                                                   \
  }                                                                                                                 \
  ZKG_API void PFX##_poly_mont_mul_naive(int n1, const uint64_t *a, int n2, const uint64_t *b, uint64_t *t) {       \
    poly_mul_g(CID, n1, a, n2, b, t);                                                                               \
  }                                                                                                                 \
  ZKG_API void PFX##_poly_mont_eval_at(int n1, const uint64_t *s, const uint64_t *loc, uint64_t *t) {               \
    guard([&] { zk::poly_eval(CID, n1, s, loc, t, true); });                                                        \
  }

ZKG_POLY_ENTRIES(bn128, ZKG_BN128)
ZKG_POLY_ENTRIES(bls12_381, ZKG_BLS12_381)

ZKG_API int zkg_poly_mul_device(int curve, int n1, const uint64_t *d_a, int n2, const uint64_t *d_b, uint64_t *d_tgt) {
  return guard_ret(-1, [&] { return zk::poly_mul(curve, n1, d_a, n2, d_b, d_tgt, false); });
}
ZKG_API void zkg_poly_eval_device(int curve, int n, const uint64_t *d_poly, const uint64_t *x, uint64_t *tgt) {
  guard([&] { zk::poly_eval(curve, n, d_poly, x, tgt, false); });
}
ZKG_API void zkg_poly_lincomb_device(int curve, int K, const int *ns, const uint64_t *coeffs,
                                     const uint64_t *const *d_polys, uint64_t *d_tgt) {
  guard([&] { zk::poly_lincomb(curve, K, ns, coeffs, d_polys, d_tgt, false); });
}
// <C>_poly_mont_{long_div,quot,rem} (bls12_381_poly_mont.c:249-309) with the curve as first argument
ZKG_API int zkg_poly_long_div_device(int curve, int n1, const uint64_t *d_src1, int n2, const uint64_t *d_src2,
                                     int nquot, uint64_t *d_quot, int nrem, uint64_t *d_rem) {
  return guard_ret(-1, [&] { return zk::poly_long_div(curve, n1, d_src1, n2, d_src2, nquot, d_quot, nrem, d_rem, false); });
}
ZKG_API int zkg_poly_long_div(int curve, int n1, const uint64_t *src1, int n2, const uint64_t *src2, int nquot,
                              uint64_t *quot, int nrem, uint64_t *rem) {
  return guard_ret(-1, [&] { return zk::poly_long_div(curve, n1, src1, n2, src2, nquot, quot, nrem, rem, true); });
}
ZKG_API void zkg_poly_set_div_base_max(int len) { zk::poly_set_div_base_max(len); }
ZKG_API int zkg_poly_div_base_max(void) { return zk::poly_div_base_max(); }
ZKG_API int zkg_poly_div_plan(int m, int *prec, int cap) { return zk::poly_div_plan(m, prec, cap); }
ZKG_API int zkg_poly_last_div_steps(void) { return zk::poly_last_div_steps(); }
ZKG_API void zkg_poly_div_profile(int on) { zk::poly_div_profile(on); }
ZKG_API void zkg_poly_last_div_phase_ms(double *ms) { zk::poly_last_div_phase_ms(ms); }
ZKG_API void zkg_poly_set_mul_direct_max(int len) { zk::poly_set_mul_direct_max(len); }
ZKG_API int zkg_poly_last_mul_path(void) { return zk::poly_last_mul_path(); }

}  // extern "C"

// ---------------------------------------------------------------------------- division by x - z
// <C>_poly_mont_div_by_vanishing with expo_n = 1 (bls12_381_poly_mont.c:317-397), many points at once
#include "zk_lindiv.hpp"

namespace {
// a refusal: the message on the calling thread's error channel and a nonzero code, in either error mode
int refuse(const char *msg) {
  zk::record_error(msg);
  return -1;
}
int div_linear_g(int curve, int n, const uint64_t *poly, int nz, const uint64_t *z, uint64_t *quot, uint64_t *vals,
                 bool host_io) {
  if (curve != ZKG_BN128 && curve != ZKG_BLS12_381) return refuse("poly_div_linear: unknown curve");
  if (n < 0 || nz < 0) return refuse("poly_div_linear: negative size");
  if (nz > 0 && (!z || !vals)) return refuse("poly_div_linear: null points or values");
  if (nz > 0 && n > 0 && !poly) return refuse("poly_div_linear: null polynomial");
  if (quot && n > 1 && nz > 0) {  // the write pass stores across tile boundaries: aliasing is a race
    const uintptr_t p0 = (uintptr_t)poly, p1 = p0 + (size_t)n * 32;
    const uintptr_t q0 = (uintptr_t)quot, q1 = q0 + (size_t)nz * ((size_t)n - 1) * 32;
    if (p0 < q1 && q0 < p1) return refuse("poly_div_linear: the quotient overlaps the polynomial");
  }
  return guard_ret<int>(-1, [&] {
    zk::poly_div_linear(curve, n, poly, nz, z, quot, vals, host_io);
    return 0;
  });
}
}  // namespace

extern "C" {

ZKG_API int zkg_poly_div_linear_device(int curve, int n, const uint64_t *d_poly, int nz, const uint64_t *z,
                                       uint64_t *d_quot, uint64_t *vals) {
  return div_linear_g(curve, n, d_poly, nz, z, d_quot, vals, false);
}
ZKG_API int zkg_poly_div_linear(int curve, int n, const uint64_t *poly, int nz, const uint64_t *z, uint64_t *quot,
                                uint64_t *vals) {
  return div_linear_g(curve, n, poly, nz, z, quot, vals, true);
}
ZKG_API void zkg_poly_set_lindiv_tile(int rows_per_lane) { zk::poly_set_lindiv_tile(rows_per_lane); }
ZKG_API int zkg_poly_lindiv_tile(void) { return zk::poly_lindiv_tile(); }

}  // extern "C"

// ---------------------------------------------------------------------------- G1
#include "zk_g1ext.hpp"

extern "C" {

#define ZKG_G1EXT_ENTRIES(PFX, CID)                                                                         \
  ZKG_API void PFX##_G1_proj_batch_from_affine(int N, const uint64_t *src, uint64_t *tgt) {                 \
    from_affine_g(CID, N, src, tgt, true);                                                           \
  }                                                                                                         \
  ZKG_API void PFX##_G1_proj_batch_to_affine(int N, const uint64_t *src, uint64_t *tgt) {                   \
    to_affine_g(CID, N, src, tgt, true);                                                             \
  }                                                                                                         \
  ZKG_API void PFX##_G1_proj_fft_forward(int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt) {  \
    fft_g(CID, m, gen, src, tgt, true, false);                                                             \
  }                                                                                                         \
  ZKG_API void PFX##_G1_proj_fft_inverse(int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt) {  \
    fft_g(CID, m, gen, src, tgt, true, true);                                                              \
  }                                                                                                         \
  /* Jacobian twins (bls12_381_G1_jac.c:139-158, 727-838; G1/Jac.hs:264-265, 374-389) */                   \
  ZKG_API void PFX##_G1_jac_batch_from_affine(int N, const uint64_t *src, uint64_t *tgt) {                  \
    from_affine_g(CID, N, src, tgt, true, true);                                                           \
  }                                                                                                         \
  ZKG_API void PFX##_G1_jac_batch_to_affine(int N, const uint64_t *src, uint64_t *tgt) {                    \
    to_affine_g(CID, N, src, tgt, true, true);                                                             \
  }                                                                                                         \
  ZKG_API void PFX##_G1_jac_fft_forward(int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt) {   \
    fft_g(CID, m, gen, src, tgt, true, false, true);                                                       \
  }                                                                                                         \
  ZKG_API void PFX##_G1_jac_fft_inverse(int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt) {   \
    fft_g(CID, m, gen, src, tgt, true, true, true);                                                        \
  }

ZKG_G1EXT_ENTRIES(bn128, ZKG_BN128)
ZKG_G1EXT_ENTRIES(bls12_381, ZKG_BLS12_381)

ZKG_API void zkg_g1_fft_device(int curve, int inverse, int m, const uint64_t *gen, const uint64_t *d_src,
                               uint64_t *d_tgt) {
  fft_g(curve, m, gen, d_src, d_tgt, false, inverse != 0);
}
ZKG_API void zkg_g1_batch_to_affine_device(int curve, int n, const uint64_t *d_src, uint64_t *d_tgt) {
  to_affine_g(curve, n, d_src, d_tgt, false);
}
ZKG_API void zkg_g1_jac_fft_device(int curve, int inverse, int m, const uint64_t *gen, const uint64_t *d_src,
                                   uint64_t *d_tgt) {
  fft_g(curve, m, gen, d_src, d_tgt, false, inverse != 0, true);
}
ZKG_API void zkg_g1_jac_batch_to_affine_device(int curve, int n, const uint64_t *d_src, uint64_t *d_tgt) {
  to_affine_g(curve, n, d_src, d_tgt, false, true);
}

}  // extern "C"

// ---------------------------------------------------------------------------- G1 and G2 batch scalar multiplication
// a host loop over <C>_G1_proj_scl_Fr_mont / _scl_Fr_std (bls12_381_G1_proj.c:462-489) and normalize / to_affine
#include "zk_scl.hpp"

namespace {
bool scl_args_ok(int curve, int n) { return n >= 0 && (curve == ZKG_BN128 || curve == ZKG_BLS12_381); }
}  // namespace

extern "C" {

#define ZKG_SCL_ENTRY(NAME, FN, HOST_IO)                                                                              \
  ZKG_API int NAME(int curve, int n, const uint64_t *expos, int expos_mont, const uint64_t *bases, int affine_out,    \
                   uint64_t *tgt) {                                                                                   \
    if (!scl_args_ok(curve, n)) return -1;                                                                            \
    guard([&] { zk::FN(curve, n, expos, expos_mont != 0, bases, affine_out != 0, tgt, HOST_IO); });                   \
    return 0;                                                                                                         \
  }
ZKG_SCL_ENTRY(zkg_g1_scl_fixed_device, g1_scl_fixed, false)
ZKG_SCL_ENTRY(zkg_g1_scl_fixed, g1_scl_fixed, true)
ZKG_SCL_ENTRY(zkg_g1_scl_rows_device, g1_scl_rows, false)
ZKG_SCL_ENTRY(zkg_g1_scl_rows, g1_scl_rows, true)

ZKG_API int zkg_g1_scl_powers_device(int curve, int n, const uint64_t *a, const uint64_t *tau,
                                     const uint64_t *base_affine, int affine_out, uint64_t *d_tgt) {
  if (!scl_args_ok(curve, n)) return -1;
  guard([&] { zk::g1_scl_powers(curve, n, a, tau, base_affine, affine_out != 0, d_tgt, false); });
  return 0;
}
ZKG_API int zkg_g1_scl_powers(int curve, int n, const uint64_t *a, const uint64_t *tau, const uint64_t *base_affine,
                              int affine_out, uint64_t *tgt) {
  if (!scl_args_ok(curve, n)) return -1;
  guard([&] { zk::g1_scl_powers(curve, n, a, tau, base_affine, affine_out != 0, tgt, true); });
  return 0;
}
ZKG_API void zkg_g1_scl_set_window(int c) { zk::g1_scl_set_window(c); }
ZKG_API void zkg_g1_scl_set_fixed_min(int n) { zk::g1_scl_set_fixed_min(n); }
ZKG_API int zkg_g1_scl_last_path(void) { return zk::g1_scl_last_path(); }
ZKG_API int zkg_g1_scl_digits(int c, const uint64_t k[4], int *digits, int cap) {
  if (c < zk::SCL_WINDOW_MIN || c > zk::SCL_WINDOW_MAX) return -1;
  const int W = zk::scl_windows(c);
  int carry = 0;
  for (int w = 0; w < W; w++) {
    const int d = zk::scl_digit(k, c, w, carry);
    if (w < cap) digits[w] = d;
  }
  return W;
}
ZKG_API size_t zkg_g1_scl_table_bytes(int curve, int c) {
  return curve == ZKG_BN128 || curve == ZKG_BLS12_381 ? zk::g1_scl_table_bytes(curve, c) : 0;
}

}  // extern "C"

// the row-wise sum of scalar multiples (zk_fk20.hip)
#include "zk_fk20.hpp"

namespace {
bool ranges_overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return abytes && bbytes && a0 < b0 + bbytes && b0 < a0 + abytes;
}
int rows_sum_g(int curve, int rows, int terms, const uint64_t *expos, int expos_mont, const uint64_t *bases,
               int affine_out, uint64_t *tgt, bool host_io) {
  if (curve != ZKG_BN128 && curve != ZKG_BLS12_381) return refuse("g1_scl_rows_sum: unknown curve");
  if (rows < 0 || terms < 0) return refuse("g1_scl_rows_sum: negative size");
  const size_t E = (size_t)rows * (size_t)terms, NP = curve == ZKG_BN128 ? 4 : 6;
  if (E > (size_t)0x7fffffff) return refuse("g1_scl_rows_sum: rows x terms does not fit 31 bits");
  if (rows > 0 && (!tgt || (E > 0 && (!expos || !bases)))) return refuse("g1_scl_rows_sum: null buffer");
  const size_t out_bytes = (size_t)rows * (affine_out ? 2 : 3) * NP * 8;
  if (ranges_overlap(tgt, out_bytes, expos, E * 32) || ranges_overlap(tgt, out_bytes, bases, E * 2 * NP * 8))
    return refuse("g1_scl_rows_sum: the target overlaps an input");
  return guard_ret<int>(-1, [&] {
    zk::g1_scl_rows_sum(curve, rows, terms, expos, expos_mont != 0, bases, affine_out != 0, tgt, host_io);
    return 0;
  });
}
}  // namespace

extern "C" {

ZKG_API int zkg_g1_scl_rows_sum_device(int curve, int rows, int terms, const uint64_t *d_expos, int expos_mont,
                                       const uint64_t *d_bases, int affine_out, uint64_t *d_tgt) {
  return rows_sum_g(curve, rows, terms, d_expos, expos_mont, d_bases, affine_out, d_tgt, false);
}
ZKG_API int zkg_g1_scl_rows_sum(int curve, int rows, int terms, const uint64_t *expos, int expos_mont,
                                const uint64_t *bases, int affine_out, uint64_t *tgt) {
  return rows_sum_g(curve, rows, terms, expos, expos_mont, bases, affine_out, tgt, true);
}

// the same on G2: <C>_G2_proj_scl_Fr_mont / _scl_Fr_std (bls12_381_G2_proj.c:453-480) and normalize / to_affine
ZKG_SCL_ENTRY(zkg_g2_scl_fixed_device, g2_scl_fixed, false)
ZKG_SCL_ENTRY(zkg_g2_scl_fixed, g2_scl_fixed, true)
ZKG_SCL_ENTRY(zkg_g2_scl_rows_device, g2_scl_rows, false)
ZKG_SCL_ENTRY(zkg_g2_scl_rows, g2_scl_rows, true)

ZKG_API int zkg_g2_scl_powers_device(int curve, int n, const uint64_t *a, const uint64_t *tau,
                                     const uint64_t *base_affine, int affine_out, uint64_t *d_tgt) {
  if (!scl_args_ok(curve, n)) return -1;
  guard([&] { zk::g2_scl_powers(curve, n, a, tau, base_affine, affine_out != 0, d_tgt, false); });
  return 0;
}
ZKG_API int zkg_g2_scl_powers(int curve, int n, const uint64_t *a, const uint64_t *tau, const uint64_t *base_affine,
                              int affine_out, uint64_t *tgt) {
  if (!scl_args_ok(curve, n)) return -1;
  guard([&] { zk::g2_scl_powers(curve, n, a, tau, base_affine, affine_out != 0, tgt, true); });
  return 0;
}
ZKG_API void zkg_g2_scl_set_window(int c) { zk::g2_scl_set_window(c); }
ZKG_API void zkg_g2_scl_set_fixed_min(int n) { zk::g2_scl_set_fixed_min(n); }
ZKG_API int zkg_g2_scl_last_path(void) { return zk::g2_scl_last_path(); }
ZKG_API size_t zkg_g2_scl_table_bytes(int curve, int c) {
  return curve == ZKG_BN128 || curve == ZKG_BLS12_381 ? zk::g2_scl_table_bytes(curve, c) : 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------- G2 batch conversions
// <C>_G2_proj_batch_from_affine / _batch_to_affine (bls12_381_G2_proj.c:139-158; G2/Proj.hs:386-405)
#include "zk_g2ext.hpp"

extern "C" {

#define ZKG_G2EXT_ENTRIES(PFX, CID)                                                            \
  ZKG_API void PFX##_G2_proj_batch_from_affine(int N, const uint64_t *src, uint64_t *tgt) {    \
    guard([&] { zk::g2_batch_from_affine(CID, N, src, tgt, true); });                          \
  }                                                                                            \
  ZKG_API void PFX##_G2_proj_batch_to_affine(int N, const uint64_t *src, uint64_t *tgt) {      \
    guard([&] { zk::g2_batch_to_affine(CID, N, src, tgt, true); });                            \
  }                                                                                            \
  /* the G2 group FFT (bls12_381_G2_proj.c:670-781; G2/Proj.hs forwardFFT / inverseFFT) */      \
  ZKG_API void PFX##_G2_proj_fft_forward(int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt) { \
    guard([&] { zk::g2_fft(CID, m, gen, src, tgt, true, false); });                            \
  }                                                                                            \
  ZKG_API void PFX##_G2_proj_fft_inverse(int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt) { \
    guard([&] { zk::g2_fft(CID, m, gen, src, tgt, true, true); });                             \
  }

ZKG_G2EXT_ENTRIES(bn128, ZKG_BN128)
ZKG_G2EXT_ENTRIES(bls12_381, ZKG_BLS12_381)

ZKG_API void zkg_g2_batch_to_affine_device(int curve, int n, const uint64_t *d_src, uint64_t *d_tgt) {
  guard([&] { zk::g2_batch_to_affine(curve, n, d_src, d_tgt, false); });
}
ZKG_API void zkg_g2_fft_device(int curve, int inverse, int m, const uint64_t *gen, const uint64_t *d_src,
                               uint64_t *d_tgt) {
  guard([&] { zk::g2_fft(curve, m, gen, d_src, d_tgt, false, inverse != 0); });
}
ZKG_API void zkg_g2_fft_set_max_lanes(int lanes) { zk::g2_fft_set_max_lanes(lanes); }

}  // extern "C"

// ---------------------------------------------------------------------------- pairings
// <C>_pairing_affine / _pairing_projective / _pairing_final_expo (bls12_381_pairing.c, bn128_pairing.c)
#include "zk_pairing.hpp"

extern "C" {

#define ZKG_PAIRING_ENTRIES(PFX, CID)                                                                  \
  ZKG_API void PFX##_pairing_affine(const uint64_t *P, const uint64_t *Q, uint64_t *tgt) {             \
    guard([&] { zk::pairing_rows(CID, 1, P, Q, tgt, true); });                                         \
  }                                                                                                    \
  ZKG_API void PFX##_pairing_projective(const uint64_t *P, const uint64_t *Q, uint64_t *tgt) {         \
    guard([&] { zk::pairing_projective(CID, P, Q, tgt); });                                            \
  }
ZKG_PAIRING_ENTRIES(bn128, ZKG_BN128)
ZKG_PAIRING_ENTRIES(bls12_381, ZKG_BLS12_381)

#define ZKG_PAIRING_ROWS(NAME, FN, HOST_IO)                                                            \
  ZKG_API int NAME(int curve, int n, const uint64_t *P, const uint64_t *Q, uint64_t *tgt) {            \
    return guard_ret<int>(-1, [&] {                                                                    \
      zk::FN(curve, n, P, Q, tgt, HOST_IO);                                                            \
      return 0;                                                                                        \
    });                                                                                                \
  }
ZKG_PAIRING_ROWS(zkg_pairing_rows, pairing_rows, true)
ZKG_PAIRING_ROWS(zkg_pairing_rows_device, pairing_rows, false)
ZKG_PAIRING_ROWS(zkg_pairing_product, pairing_product, true)
ZKG_PAIRING_ROWS(zkg_pairing_product_device, pairing_product, false)

ZKG_API int zkg_pairing_final_expo(int curve, int n, const uint64_t *src, uint64_t *tgt) {
  return guard_ret<int>(-1, [&] {
    zk::pairing_final_expo(curve, n, src, tgt, true);
    return 0;
  });
}
ZKG_API int zkg_pairing_final_expo_device(int curve, int n, const uint64_t *d_src, uint64_t *d_tgt) {
  return guard_ret<int>(-1, [&] {
    zk::pairing_final_expo(curve, n, d_src, d_tgt, false);
    return 0;
  });
}

}  // extern "C"

// ---------------------------------------------------------------------------- batch point validation
// <C>_G{1,2}_{affine,proj,jac}_is_on_curve / _is_infinity per row, and [r]P = O for membership
#include "zk_check.hpp"

namespace {
// the refusals: a return code, before any device is opened
bool check_args_ok(int curve, int n, int coords, bool g2) {
  return n >= 0 && (curve == ZKG_BN128 || curve == ZKG_BLS12_381) &&
         (coords == ZKG_COORDS_AFFINE || coords == ZKG_COORDS_PROJ || (coords == ZKG_COORDS_JAC && !g2));
}
}  // namespace

extern "C" {

#define ZKG_CHECK_ENTRY(NAME, FN, G2, HOST_IO)                                                  \
  ZKG_API int NAME(int curve, int n, const uint64_t *pts, int coords, uint8_t *flags) {         \
    if (!check_args_ok(curve, n, coords, G2)) return -1;                                        \
    if (n == 0) return 0;                                                                       \
    return guard_ret<int>(-1, [&] { return zk::FN(curve, n, pts, coords, flags, HOST_IO); });   \
  }
ZKG_CHECK_ENTRY(zkg_g1_check_rows, g1_check_rows, false, true)
ZKG_CHECK_ENTRY(zkg_g1_check_rows_device, g1_check_rows, false, false)
ZKG_CHECK_ENTRY(zkg_g2_check_rows, g2_check_rows, true, true)
ZKG_CHECK_ENTRY(zkg_g2_check_rows_device, g2_check_rows, true, false)
ZKG_API void zkg_check_set_mode(int mode) { zk::check_set_mode(mode); }
ZKG_API void zkg_check_set_max_lanes(int lanes) { zk::check_set_max_lanes(lanes); }

}  // extern "C"
