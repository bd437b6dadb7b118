// zk_check_g2_bn.hip -- batch G2 point validation on gfx950: the public entry and the BN254 G2 instantiation of
// zk_check_impl.hpp's kernels (BLS12-381's is zk_check_g2_bls.hip).  Replaces a host loop over
// <C>_G2_{affine,proj}_is_on_curve / _is_infinity (bn128_G2_affine.c:62-110, bn128_G2_proj.c:164-195) and over
// scl_Fr_std(r, P) for membership.
#include "zk_check_g2.hpp"

namespace zk {

ZK_CHECK_G2_INSTANCE(, BN254_G2)
ZK_CHECK_G2_INSTANCE(extern, BLS381_G2)

int g2_check_rows(int curve, int n, const uint64_t *pts, int coords, uint8_t *flags, bool host_io) {
  int bad = 0;
  with_g2(curve, [&](Device &dev, auto c) {
    bad = check_rows_t<decltype(c), true>(dev, n, pts, coords, flags, host_io);
  });
  return bad;
}

}  // namespace zk
