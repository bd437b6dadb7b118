// zk_lindiv.hpp -- C++ interface of the division by a linear factor (zk_lindiv.hip).
//
// What the reference computes with <C>_poly_mont_div_by_vanishing and expo_n = 1
// (bls12_381_poly_mont.c:317-397; examples/KZG.hs openingProof), for one or many points at once.
#pragma once
#include <stdint.h>

namespace zk {

// For every point z_k, k < nz (HOST, nz x 4 words, Montgomery): quot[k (n - 1) + j] = the coefficient j
// of the quotient of poly by x - z_k, j < n - 1, and vals[k] = poly(z_k) (HOST, nz x 4 words).  poly
// and quot are host or device pointers (host_io); quot may be null (the values alone); it does not
// overlap poly.  n - 1 rows are always written (zero rows above the quotient's degree); n = 1 writes
// no quotient and the value a_0; n <= 0 the value 0.
void poly_div_linear(int curve, int n, const uint64_t *poly, int nz, const uint64_t *z, uint64_t *quot, uint64_t *vals,
                     bool host_io);
// test hook: rows per lane of a tile, so that a few thousand coefficients span many tiles (1, 2, 4 or 8; 0
// or below: the default, 8; larger values are clamped to it, others count as the power of two below), and
// the value in force
void poly_set_lindiv_tile(int rows_per_lane);
int poly_lindiv_tile();

}  // namespace zk
