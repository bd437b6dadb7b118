// zk_check.hip -- batch point validation on gfx950: the hooks, the G1 entry and the G1 instantiations (BN254,
// BLS381) of zk_check_impl.hpp's kernels, which describes the passes.  The G2 instantiations are
// zk_check_g2_bn.hip / zk_check_g2_bls.hip.  Replaces a host loop over <C>_G1_{affine,proj,jac}_is_on_curve /
// _is_infinity (bls12_381_G1_affine.c:62-110, _G1_proj.c:173-205, _G1_jac.c:164-209) and, for membership, over
// scl_Fr_std(r, P) (the reference's own _is_in_subgroup multiplies by the cofactor: include/zkalgebra_gpu.h).
#include "zk_check_impl.hpp"

namespace zk {

namespace {
CheckHooks g_hooks;
}  // namespace
CheckHooks &check_hooks() { return g_hooks; }

int g1_check_rows(int curve, int n, const uint64_t *pts, int coords, uint8_t *flags, bool host_io) {
  int bad = 0;
  with_g1(curve, [&](Device &dev, auto c) {
    bad = check_rows_t<decltype(c), false>(dev, n, pts, coords, flags, host_io);
  });
  return bad;
}
void check_set_mode(int mode) {
  g_hooks.mode.store(mode == CHECK_MODE_EXACT || mode == CHECK_MODE_CURVE_ONLY ? mode : CHECK_MODE_DEFAULT);
}
void check_set_max_lanes(int lanes) { g_hooks.max_lanes.store(lanes > 0 ? lanes : 0); }

}  // namespace zk
