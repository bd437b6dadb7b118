// zk_scl_g2_bn.hip -- batch G2 scalar multiplication on gfx950: the hooks, the public entries, and the
// BN254 G2 instantiation of zk_scl_impl.hpp's templates (BLS12-381's is zk_scl_g2_bls.hip).  Replaces a host
// loop over <C>_G2_proj_scl_Fr_mont / _scl_Fr_std (bn128_G2_proj.c:453-480) and _normalize / _to_affine.
#include "zk_scl_g2.hpp"

namespace zk {

ZK_SCL_G2_INSTANCES(, BN254_G2)
ZK_SCL_G2_INSTANCES(extern, BLS381_G2)

namespace {
SclHooks g_hooks;
}  // namespace
SclHooks &SclG2::hooks() { return g_hooks; }

// ---------------------------------------------------------------------------- public

size_t g2_scl_table_bytes(int curve, int c) {
  c = std::min(std::max(c, SCL_WINDOW_MIN), SCL_WINDOW_MAX);
  return on_curve<BN254_G2, BLS381_G2>(curve, [&](auto cv) { return table_rows(c) * 2 * decltype(cv)::NP64 * 8; });
}
void g2_scl_fixed(int curve, int n, const uint64_t *expos, bool expos_mont, const uint64_t *base, bool affine_out,
                  uint64_t *tgt, bool host_io) {
  with_g2(curve, [&](Device &dev, auto c) {
    scl_fixed_t<decltype(c), SclG2>(dev, n, expos, expos_mont, nullptr, nullptr, base, affine_out, tgt, host_io);
  });
}
void g2_scl_rows(int curve, int n, const uint64_t *expos, bool expos_mont, const uint64_t *bases, bool affine_out,
                 uint64_t *tgt, bool host_io) {
  with_g2(curve, [&](Device &dev, auto c) {
    scl_rows_t<decltype(c), SclG2>(dev, n, expos, expos_mont, bases, affine_out, tgt, host_io);
  });
}
void g2_scl_powers(int curve, int n, const uint64_t *a, const uint64_t *tau, const uint64_t *base, bool affine_out,
                   uint64_t *tgt, bool host_io) {
  with_g2(curve, [&](Device &dev, auto c) {
    scl_fixed_t<decltype(c), SclG2>(dev, n, nullptr, true, a, tau, base, affine_out, tgt, host_io);
  });
}
void g2_scl_set_window(int c) { g_hooks.set_window(c); }
void g2_scl_set_fixed_min(int n) { g_hooks.set_fixed_min(n); }
int g2_scl_last_path() { return g_hooks.last_path.load(); }

}  // namespace zk
