// zk_arr.hpp -- C++ interface of the device Fr vector operations (zk_arr.hip).
//
// Replaces the reference's generated per-curve vector code around the NTT:
//   <C>_arr_mont_*                      lib/cbits/curves/array/mont/bls12_381_arr_mont.h:3-48
//   <C>_poly_mont_div_by_vanishing      lib/cbits/curves/poly/mont/bls12_381_poly_mont.c:317-397
//   <C>_poly_mont_quot_by_vanishing     bls12_381_poly_mont.c:402-413
// All operands are Fr in the reference's Montgomery form (4 x u64, canonical).
#pragma once
#include <stdint.h>

namespace zk {

enum ArrOp : int {
  ARR_NEG = 0,      // tgt = -a
  ARR_ADD,          // tgt = a + b
  ARR_SUB,          // tgt = a - b
  ARR_SUB_REV,      // tgt = b - a            (sub_inplace_reverse: tgt = src1 - tgt)
  ARR_SQR,          // tgt = a^2
  ARR_MUL,          // tgt = a * b
  ARR_MUL_ADD,      // tgt = a * b + c
  ARR_MUL_SUB,      // tgt = a * b - c
  ARR_SCALE,        // tgt = kA * a
  ARR_AXPY,         // tgt = kA * a + b
  ARR_AXPBY,        // tgt = kA * a + kB * b
  ARR_FROM_STD,     // tgt = a * R  (standard -> Montgomery)
  ARR_TO_STD,       // tgt = a / R  (Montgomery -> standard)
  ARR_COPY,         // tgt = a
  ARR_SET_CONST,    // tgt = kA
  ARR_INV,          // tgt = 1/a  (batch inversion; any zero input -> every output 0)
  ARR_DIV,          // tgt = a / b (a * batch_inv(b), same zero rule on b)
  ARR_NUM_OPS
};

enum ArrPred : int { PRED_IS_VALID = 0, PRED_IS_ZERO, PRED_IS_ONE, PRED_IS_EQUAL };

// device or host pointers (host_io): a, b, c are n-element Fr arrays (unused ones may be
// null); kA, kB are single HOST elements.  tgt may alias a or b (the in-place forms).
void arr_op(int curve, int op, int n, const uint64_t *a, const uint64_t *b, const uint64_t *c, const uint64_t *kA,
            const uint64_t *kB, uint64_t *tgt, bool host_io);
int arr_pred(int curve, int pred, int n, const uint64_t *a, const uint64_t *b, bool host_io);
void arr_dot(int curve, int n, const uint64_t *a, const uint64_t *b, uint64_t *tgt_host, bool host_io);
void arr_powers(int curve, int n, const uint64_t *kA, const uint64_t *kB, uint64_t *tgt, bool host_io);
// returns 1 if the remainder is zero (quot_by_vanishing); rem may be null
int poly_div_by_vanishing(int curve, int n1, const uint64_t *src, int expo_n, const uint64_t *eta, int nquot,
                          uint64_t *quot, int nrem, uint64_t *rem, bool host_io);
// degree of a[0, n) (-1: the zero polynomial or n <= 0), <C>_poly_mont_degree (poly_mont.c:26-32)
int poly_degree(int curve, int n, const uint64_t *a, bool host_io);
struct Device;
// d_tgt = d_a * d_b element-wise on DEVICE buffers, enqueued on dev.stream without touching the
// arena and without waiting (caller holds dev.mu; n < 2^31): the pointwise step of zk_poly.hip
void arr_mul_enqueue(Device &dev, int curve, size_t n, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_tgt);
// d_tgt[i] = kA kB^i, i < n (kA, kB on the host), the two launches of arr_powers enqueued on dev.stream
// without resetting the arena and without waiting (caller holds dev.mu): the power tables are taken from
// the arena, arr_powers_scratch_bytes(n) of it.  The scalars of zk_scl.hip's powers entry.
size_t arr_powers_scratch_bytes(size_t n);
void arr_powers_enqueue(Device &dev, int curve, int n, const uint64_t *kA, const uint64_t *kB, uint64_t *d_tgt);
// *d_deg = degree of the DEVICE array d_a[0, n) (-1: zero or n <= 0), the reduction of poly_degree
// enqueued on dev.stream without touching the arena and without waiting (caller holds dev.mu): the
// division of zk_poly.hip finds both of its degrees with one wait
void poly_degree_enqueue(Device &dev, int n, const uint64_t *d_a, int *d_deg);

}  // namespace zk
