// zk_pairing_bn.hip -- batch pairings on gfx950: the public entries and the BN254 instantiation of
// zk_pairing_impl.hpp's templates (BLS12-381's is zk_pairing_bls.hip).  Replaces a host loop over
// <C>_pairing_affine / _pairing_projective / _pairing_final_expo (bn128_pairing.c:303-374).
#include "zk_g1ext.hpp"
#include "zk_g2ext.hpp"
#include "zk_pairing_impl.hpp"

namespace zk {

ZK_PAIRING_INSTANCES(, BN254_G2)
ZK_PAIRING_INSTANCES(extern, BLS381_G2)

namespace {
void check_args(int curve, int n, const void *a, const void *b, const void *tgt) {
  ZK_REQUIRE(curve == 0 || curve == 1, "pairing: unknown curve");
  ZK_REQUIRE(n >= 0, "pairing: negative row count");
  ZK_REQUIRE(tgt != nullptr && (n == 0 || (a != nullptr && b != nullptr)), "pairing: null buffer");
}
}  // namespace

void pairing_rows(int curve, int n, const uint64_t *P, const uint64_t *Q, uint64_t *tgt, bool host_io) {
  check_args(curve, n, P, Q, tgt);
  with_g2(curve, [&](Device &dev, auto c) { pairing_rows_t<decltype(c)>(dev, n, P, Q, tgt, host_io); });
}
void pairing_product(int curve, int n, const uint64_t *P, const uint64_t *Q, uint64_t *tgt, bool host_io) {
  check_args(curve, n, P, Q, tgt);
  with_g2(curve, [&](Device &dev, auto c) { pairing_product_t<decltype(c)>(dev, n, P, Q, tgt, host_io); });
}
void pairing_final_expo(int curve, int n, const uint64_t *src, uint64_t *tgt, bool host_io) {
  check_args(curve, n, src, src, tgt);
  with_g2(curve, [&](Device &dev, auto c) { pairing_final_expo_t<decltype(c)>(dev, n, src, tgt, host_io); });
}
void pairing_projective(int curve, const uint64_t *P, const uint64_t *Q, uint64_t *tgt) {
  check_args(curve, 1, P, Q, tgt);
  uint64_t ap[2 * 6], aq[4 * 6];  // the existing to-affine conversions, then the affine form
  g1_batch_to_affine(curve, 1, P, ap, true, false);
  g2_batch_to_affine(curve, 1, Q, aq, true);
  pairing_rows(curve, 1, ap, aq, tgt, true);
}

}  // namespace zk
