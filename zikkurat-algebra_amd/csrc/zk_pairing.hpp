// zk_pairing.hpp -- batch optimal-ate pairings on gfx950 (zk_pairing_impl.hpp; one unit per curve,
// zk_pairing_bn.hip with the public entries and zk_pairing_bls.hip).  Replaces a host loop over
// <C>_pairing_affine (lib/cbits/curves/pairing/<C>_pairing.c) and <C>_pairing_final_expo.
#pragma once
#include <cstdint>

namespace zk {

// tgt row i = pairing(P_i, Q_i): n affine G1 rows (2 NP words), n affine G2 rows (4 NP), n Fp12 rows (12 NP);
// a row with P or Q all-0xFF (infinity) gives one
void pairing_rows(int curve, int n, const uint64_t *P, const uint64_t *Q, uint64_t *tgt, bool host_io);
// tgt = prod_i pairing(P_i, Q_i), one Fp12 row, with a single final exponentiation (n = 0: one)
void pairing_product(int curve, int n, const uint64_t *P, const uint64_t *Q, uint64_t *tgt, bool host_io);
// tgt row i = src row i ^ ((p^12 - 1) / r)
void pairing_final_expo(int curve, int n, const uint64_t *src, uint64_t *tgt, bool host_io);
// the single-pair projective form: P (3 NP words), Q (6 NP words) on the host
void pairing_projective(int curve, const uint64_t *P, const uint64_t *Q, uint64_t *tgt);

}  // namespace zk
