// zk_g2ext.hpp -- C++ interface of the G2 batch conversions (zk_g2ext.hip)
#pragma once
#include <stdint.h>

namespace zk {

// affine G2 (x || y over Fp2, all-0xFF = infinity) -> projective (x : y : 1), infinity -> (0 : 1 : 0)
void g2_batch_from_affine(int curve, int n, const uint64_t *src, uint64_t *tgt, bool host_io);
// projective G2 -> affine (X/Z, Y/Z), Z = 0 -> all-0xFF
void g2_batch_to_affine(int curve, int n, const uint64_t *src, uint64_t *tgt, bool host_io);

// group FFT of 2^m projective G2 rows (zk_g2fft.hip) with Fr generator `gen` (host, Montgomery), m in
// 0..24; outputs normalised (x : y : 1), infinity (0 : 1 : 0); the reference's integer-scalar schedule
void g2_fft(int curve, int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt, bool host_io, bool inverse);
// cap on a stage's scalar-multiplication lanes (rounded up to 256; <= 0: the default 2^16)
void g2_fft_set_max_lanes(int lanes);

}  // namespace zk
