// zk_check.hpp -- batch point validation (zk_check.hip: G1 and the hooks; zk_check_g2_bn.hip /
// zk_check_g2_bls.hip: G2), the bodies behind zkg_g{1,2}_check_rows (include/zkalgebra_gpu.h has the contract)
#pragma once
#include <stdint.h>

namespace zk {

enum { PT_CANONICAL = 1, PT_ON_CURVE = 2, PT_IN_SUBGROUP = 4, PT_INFINITY = 8 };
enum { COORDS_AFFINE = 0, COORDS_PROJ = 1, COORDS_JAC = 2 };
// zkg_check_set_mode's values
enum { CHECK_MODE_DEFAULT = 0, CHECK_MODE_EXACT = 1, CHECK_MODE_CURVE_ONLY = 2 };

// n > 0 rows `pts` in coordinate system `coords` -> one flag byte per row (flags may be null) and the number
// of rows lacking any of CANONICAL | ON_CURVE | IN_SUBGROUP.  host_io: pts / flags are host arrays.
int g1_check_rows(int curve, int n, const uint64_t *pts, int coords, uint8_t *flags, bool host_io);
int g2_check_rows(int curve, int n, const uint64_t *pts, int coords, uint8_t *flags, bool host_io);
void check_set_mode(int mode);
void check_set_max_lanes(int lanes);

}  // namespace zk
