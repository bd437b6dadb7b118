// zk_scl_g2.hpp -- what the two G2 units of the batch scalar multiplication (zk_scl_g2_bn.hip: BN254_G2, the
// hooks and the public entries; zk_scl_g2_bls.hip: BLS381_G2) share: the group policy of zk_scl_impl.hpp's
// templates and the per-curve instantiations.  One unit per curve keeps the compile time down, as
// zk_msm_g2_{bn,bls}.hip do.
#pragma once
#include "zk_g2norm.hpp"
#include "zk_scl_impl.hpp"

namespace zk {

// Default window of the G2 table path and the row count from which a fixed-base call takes it, both measured
// on the MI355X by tools/scl_g2_time.py (profiles/scl_g2_time.json; DESIGN.md "Batch G2 scalar
// multiplication").  "window_sweep" at 2^20 rows: the time falls up to c = 13 (12.61 ms BN254, 28.87 ms
// BLS12-381, against 15.50 / 36.02 ms at c = 8 and 13.14 / 30.13 ms at c = 12) and is flat from there (c = 14:
// 12.61 / 28.82 ms, c = 16: 12.68 / 28.61 ms, within 1 %), while the table doubles per step (10.5 / 15.7 MiB at
// 13, 68 / 102 MiB at 16) and c = 13 has the shortest build (7.83 / 17.34 ms): 13, as on G1, though nothing here
// was taken from G1.  "crossover": the build's serial doubling chain makes the table path cost 7.8 / 17.3 ms
// however few rows there are, and one round of the per-row kernel (2^16 lanes) costs 5.5 / 11.6 ms, so the
// per-row kernel wins up to 2^16 rows (5.52 against 7.84 ms, 11.61 against 17.42 ms) and the table path from
// 2^17 (8.13 against 10.70 ms, 18.16 against 22.63 ms); at 2^20 it is 6.7 / 6.2 times the faster one.
constexpr int SCL_G2_WINDOW_DEFAULT = 13;
constexpr int SCL_G2_FIXED_MIN_DEFAULT = 1 << 17;

struct SclG2 {
  static constexpr int WINDOW_DEFAULT = SCL_G2_WINDOW_DEFAULT, FIXED_MIN_DEFAULT = SCL_G2_FIXED_MIN_DEFAULT;
  // the G2 group FFT's lane count (G2_FFT_LANES, zk_g2fft.hip): a lane's table is 10 KB on BLS12-381, 7.5 KB
  // on BN254, so the per-row kernel's scratch stays at 640 / 480 MB
  static constexpr size_t MAX_LANES = (size_t)1 << 16;
  static SclHooks &hooks();  // zk_scl_g2_bn.hip
  static void norm(int curve, hipStream_t st, int n, const uint32_t *acc, uint64_t *scratch, uint64_t *out,
                   bool affine) {
    g2_norm_xyzz_enqueue(curve, st, n, acc, scratch, out, affine);
  }
};

#define ZK_SCL_G2_INSTANCES(KW, C)                                                                                   \
  KW template void scl_fixed_t<C, SclG2>(Device &, int, const uint64_t *, bool, const uint64_t *, const uint64_t *, \
                                         const uint64_t *, bool, uint64_t *, bool);                                 \
  KW template void scl_rows_t<C, SclG2>(Device &, int, const uint64_t *, bool, const uint64_t *, bool, uint64_t *, bool);

}  // namespace zk
