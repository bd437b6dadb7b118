// zk_g2ext.hpp -- C++ interface of the G2 batch conversions (zk_g2ext.hip)
#pragma once
#include <stdint.h>

namespace zk {

// affine G2 (x || y over Fp2, all-0xFF = infinity) -> projective (x : y : 1), infinity -> (0 : 1 : 0)
void g2_batch_from_affine(int curve, int n, const uint64_t *src, uint64_t *tgt, bool host_io);
// projective G2 -> affine (X/Z, Y/Z), Z = 0 -> all-0xFF
void g2_batch_to_affine(int curve, int n, const uint64_t *src, uint64_t *tgt, bool host_io);

}  // namespace zk
