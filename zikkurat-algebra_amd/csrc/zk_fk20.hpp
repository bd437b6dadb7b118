// zk_fk20.hpp -- C++ interface of the row-wise sum of scalar multiples and of the KZG "all openings" on it
// (zk_fk20.hip; DESIGN.md "All openings (FK20)"), and the index maps of its two layout kernels
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ZK_FK20_HD __host__ __device__
#else
#define ZK_FK20_HD
#endif

namespace zk {

// Row p < 2r of the circulant's first column c^(j) holds F^(j)_v: v = r - 1 at p = 0, v = p - r - 1 from
// p = r + 2 on, and zero between (-1).  F^(j)_v = f_(l v + j).
ZK_FK20_HD inline long long fk20_coeff_index(long long r, long long p) {
  return p == 0 ? r - 1 : (p >= r + 2 ? p - r - 1 : -1);
}
// Row p < 2r of x^(j) holds S^(j)_u: u = r - 2 - p up to p = r - 2, and the point at infinity behind (-1).
// S^(j)_u = s_(l u + j).
ZK_FK20_HD inline long long fk20_srs_index(long long r, long long p) { return p <= r - 2 ? r - 2 - p : -1; }

// tgt[i] = sum_(j < terms) [k_(j,i)] P_(j,i), i < rows; term-major: term j's rows lie at j rows + i.  bases:
// affine rows (all-0xFF: infinity), expos: rows of 4 u64, Montgomery Fr or raw 256-bit integers (the contract
// of g1_scl_rows, zk_scl.hpp); tgt rows normalised projective, or affine (affine_out).  terms = 0: every row
// infinity.  host_io: all three are host arrays.
void g1_scl_rows_sum(int curve, int rows, int terms, const uint64_t *expos, bool expos_mont, const uint64_t *bases,
                     bool affine_out, uint64_t *tgt, bool host_io);

// The table of (n = 2^log_n, l = 2^log_l), r = n / l: the l group FFTs of size 2r of the reversed, strided
// SRS rows, as l x 2r affine rows, term-major.  d_srs_affine: the first n affine rows [tau^i] g1.
size_t kzg_open_all_table_bytes(int curve, int log_n, int log_l);
void kzg_open_all_table(int curve, int log_n, int log_l, const uint64_t *d_srs_affine, uint64_t *d_table);
// d_proofs[k] = the commitment to the quotient of the polynomial by x^l - psi^k, k < r (psi = omega^l):
// r normalised projective rows, or affine.  d_poly: npoly <= n Montgomery coefficients.
void kzg_open_all(int curve, int log_n, int log_l, int npoly, const uint64_t *d_poly, const uint64_t *d_table,
                  bool affine_out, uint64_t *d_proofs);

}  // namespace zk
