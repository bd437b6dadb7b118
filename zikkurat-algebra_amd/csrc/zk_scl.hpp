// zk_scl.hpp -- C++ interface of the batch scalar multiplications on G1 (zk_scl.hip) and G2
// (zk_scl_g2_bn.hip, zk_scl_g2_bls.hip), and the signed-window recoding that the fixed-base kernel and the
// host hook zkg_g1_scl_digits share
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZK_SCL_HD __host__ __device__
#else
#define ZK_SCL_HD
#endif

namespace zk {

constexpr int SCL_WINDOW_MIN = 2, SCL_WINDOW_MAX = 16;

// windows of a c-bit recoding of a 256-bit integer: ceil(257 / c), the last one takes the carry (the
// raw top window holds at most c - 1 bits, so with the carry it stays <= 2^(c - 1))
ZK_SCL_HD inline int scl_windows(int c) { return (257 + c - 1) / c; }

// Digit w of the signed c-bit recoding of k (4 u64, little endian), exact over the integers:
// sum_w d_w 2^(c w) = k and -2^(c - 1) < d_w <= 2^(c - 1).  Call with w = 0, 1, .. scl_windows(c) - 1
// in order; `carry` starts at 0 and is 0 again after the last window.
ZK_SCL_HD inline int scl_digit(const uint64_t k[4], int c, int w, int &carry) {
  const int b = c * w, j = b >> 6, o = b & 63;
  const uint64_t lo = j == 0 ? k[0] : j == 1 ? k[1] : j == 2 ? k[2] : j == 3 ? k[3] : 0;
  const uint64_t hi = j == 0 ? k[1] : j == 1 ? k[2] : j == 2 ? k[3] : 0;
  uint64_t v = lo >> o;
  if (o + c > 64) v |= hi << (64 - o);
  const int d = (int)(v & ((1u << c) - 1)) + carry;
  carry = d > (1 << (c - 1)) ? 1 : 0;
  return d - (carry << c);
}

// bytes of the fixed-base table of window c: scl_windows(c) windows of 2^(c - 1) affine rows (2 NP u64)
size_t g1_scl_table_bytes(int curve, int c);

// tgt[i] = [k_i] P, i < n: `base` one affine row on the HOST (all-0xFF: infinity, every row infinity);
// expos n rows of 4 u64 -- Montgomery Fr (expos_mont, brought to canonical standard form first) or raw
// 256-bit integers taken verbatim; tgt rows normalised projective (x : y : 1) / (0 : 1 : 0), or affine
// with all-0xFF at infinity (affine_out).  host_io: expos and tgt are host arrays.
void g1_scl_fixed(int curve, int n, const uint64_t *expos, bool expos_mont, const uint64_t *base, bool affine_out,
                  uint64_t *tgt, bool host_io);
// tgt[i] = [k_i] P_i with n affine rows `bases` (device, or host with host_io)
void g1_scl_rows(int curve, int n, const uint64_t *expos, bool expos_mont, const uint64_t *bases, bool affine_out,
                 uint64_t *tgt, bool host_io);
// tgt[i] = [a tau^i] P: a, tau Montgomery Fr on the HOST (a null: 1), the scalars never leave the device
void g1_scl_powers(int curve, int n, const uint64_t *a, const uint64_t *tau, const uint64_t *base, bool affine_out,
                   uint64_t *tgt, bool host_io);

// test hooks: the window (0: default; clamped to 2..16), the row count from which a fixed-base call
// builds the table (< 0: default, 0: always), and the path of the most recent fixed-base or powers call
// on this process (0: the per-row kernel, otherwise the window of the table path)
void g1_scl_set_window(int c);
void g1_scl_set_fixed_min(int n);
int g1_scl_last_path();

// The same on G2 (zk_scl_g2_bn.hip, zk_scl_g2_bls.hip): a coordinate is an Fp2 element c0 || c1, so NP is
// twice the base field's word count -- an affine row 2 NP = 16 (BN254) / 24 (BLS12-381) words.  Same
// contract: the integer value of the scalar, no reduction mod r, bases outside the order-r subgroup of the
// twist allowed.  The hooks have a state of their own (the defaults differ per group).
size_t g2_scl_table_bytes(int curve, int c);
void g2_scl_fixed(int curve, int n, const uint64_t *expos, bool expos_mont, const uint64_t *base, bool affine_out,
                  uint64_t *tgt, bool host_io);
void g2_scl_rows(int curve, int n, const uint64_t *expos, bool expos_mont, const uint64_t *bases, bool affine_out,
                 uint64_t *tgt, bool host_io);
void g2_scl_powers(int curve, int n, const uint64_t *a, const uint64_t *tau, const uint64_t *base, bool affine_out,
                   uint64_t *tgt, bool host_io);
void g2_scl_set_window(int c);
void g2_scl_set_fixed_min(int n);
int g2_scl_last_path();

}  // namespace zk
