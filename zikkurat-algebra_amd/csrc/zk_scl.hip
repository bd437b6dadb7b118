// zk_scl.hip -- batch G1 scalar multiplication on gfx950: the G1 instantiation (BN254, BLS381) of the
// kernel templates and call bodies of zk_scl_impl.hpp, which describes the algorithm.  The G2 instantiations
// are zk_scl_g2_bn.hip / zk_scl_g2_bls.hip.
#include "zk_scl_impl.hpp"

namespace zk {

// Default window of the table path and the row count from which a fixed-base call takes it, both
// measured on the MI355X by tools/scl_time.py (profiles/scl_time.json; DESIGN.md "Batch scalar
// multiplication").  "window_sweep": c = 13 is the fastest window at 2^20 rows on both curves (4.49 ms
// BN254, 9.62 ms BLS12-381, against 5.58 / 11.87 ms at c = 8 and 4.55 / 9.78 ms at c = 16) and no slower
// than any other at 2^12 and 2^16, where the build is the whole cost.  "crossover": the build's serial
// doubling chain (2.7 / 5.8 ms) is longer than one round of the per-row kernel, which holds 2^17 rows, so
// the table path loses at 2^17 (2.82 against 2.76 ms, 6.05 against 5.83 ms) and is the faster one from
// 2^18 rows (3.05 against 5.21 ms, 6.53 against 10.93 ms).
constexpr int SCL_WINDOW_DEFAULT = 13;
constexpr int SCL_FIXED_MIN_DEFAULT = 1 << 18;

namespace {
SclHooks g_hooks;
struct SclG1 {
  static constexpr int WINDOW_DEFAULT = SCL_WINDOW_DEFAULT, FIXED_MIN_DEFAULT = SCL_FIXED_MIN_DEFAULT;
  static constexpr size_t MAX_LANES = (size_t)1 << 17;
  static SclHooks &hooks() { return g_hooks; }
  static void norm(int curve, hipStream_t st, int n, const uint32_t *acc, uint64_t *scratch, uint64_t *out,
                   bool affine) {
    g1_norm_xyzz_enqueue(curve, st, n, acc, scratch, out, affine);
  }
};
}  // namespace

// ---------------------------------------------------------------------------- public

size_t g1_scl_table_bytes(int curve, int c) {
  c = std::min(std::max(c, SCL_WINDOW_MIN), SCL_WINDOW_MAX);
  return on_curve<BN254, BLS381>(curve, [&](auto cv) { return table_rows(c) * 2 * decltype(cv)::NP64 * 8; });
}
void g1_scl_fixed(int curve, int n, const uint64_t *expos, bool expos_mont, const uint64_t *base, bool affine_out,
                  uint64_t *tgt, bool host_io) {
  with_g1(curve, [&](Device &dev, auto c) {
    scl_fixed_t<decltype(c), SclG1>(dev, n, expos, expos_mont, nullptr, nullptr, base, affine_out, tgt, host_io);
  });
}
void g1_scl_rows(int curve, int n, const uint64_t *expos, bool expos_mont, const uint64_t *bases, bool affine_out,
                 uint64_t *tgt, bool host_io) {
  with_g1(curve, [&](Device &dev, auto c) {
    scl_rows_t<decltype(c), SclG1>(dev, n, expos, expos_mont, bases, affine_out, tgt, host_io);
  });
}
void g1_scl_powers(int curve, int n, const uint64_t *a, const uint64_t *tau, const uint64_t *base, bool affine_out,
                   uint64_t *tgt, bool host_io) {
  with_g1(curve, [&](Device &dev, auto c) {
    scl_fixed_t<decltype(c), SclG1>(dev, n, nullptr, true, a, tau, base, affine_out, tgt, host_io);
  });
}
void g1_scl_set_window(int c) { g_hooks.set_window(c); }
void g1_scl_set_fixed_min(int n) { g_hooks.set_fixed_min(n); }
int g1_scl_last_path() { return g_hooks.last_path.load(); }

}  // namespace zk
