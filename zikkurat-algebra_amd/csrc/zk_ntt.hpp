// zk_ntt.hpp -- C++ interface of the device NTT (used by the C ABI layer)
#pragma once
#include <stddef.h>
#include <stdint.h>
namespace zk {
// curve: 0 = bn128, 1 = bls12_381.  gen_mont: generator of the order-2^m subgroup
// (Montgomery Fr, HOST pointer).  src/dst: 2^m x 4 u64 Montgomery Fr; host pointers
// when host_io, device pointers otherwise.  inverse: interpolation incl. the 1/N factor.
void ntt(int curve, int m, const uint64_t *gen_mont, const uint64_t *src, uint64_t *dst, bool host_io,
         bool inverse);
// `batch` transforms of 2^m elements each (transform b at row offset b * 2^m), evaluated on /
// interpolated from the coset shift * <gen> when shift_mont (HOST pointer, Montgomery Fr) is given:
//   forward: dst_b[k] = sum_j src_b[j] shift^j gen^(j k);  inverse: dst_b[j] = shift^-j / N sum_k src_b[k] gen^(-j k)
// On the calling thread's device; dst may equal src.  Returns 0, or -1 (nothing written) for m
// outside 0..30, batch < 0 or an inverse with shift == 0.  When the working set of the whole batch
// does not fit the arena the batch runs in contiguous chunks of transforms.
int ntt_ext(int curve, int m, const uint64_t *gen_mont, const uint64_t *shift_mont, int batch, const uint64_t *src,
            uint64_t *dst, bool host_io, bool inverse);
// test hook: blocks per launch of the batched pass kernel (0 or above 2^21: the default, 2^21)
void ntt_ext_set_max_grid(unsigned tiles);
// test hook: pass split, 12 (two passes for every 2^17..2^24), 8 (<= 2^8-point passes only) or
// 0 (default: two passes at 2^20 only)
void ntt_set_max_radix(int r);
// test hook: entries above which a pass computes its inter-pass twiddles on the fly instead of
// reading a cached table (default 2^25; 0 restores it)
void ntt_set_table_max(size_t entries);
// test hook: bytes of cached twiddle sets one context keeps before it evicts the least recently used
// (default 8 GiB; 0 restores it)
void ntt_set_cache_limit(size_t bytes);
// bytes of the twiddle sets and coset shift tables cached for the calling thread's device
size_t ntt_cache_bytes();
struct Device;
// one transform between DEVICE buffers, enqueued on dev.stream without touching the arena and
// without waiting (caller holds dev.mu): d_src -> d_dst through `scratch`, three distinct buffers
// of 2^m elements.  The polynomial product (zk_poly.hip) runs its transforms through this.
void ntt_enqueue(Device &dev, int curve, int m, const uint64_t *gen_mont, const uint64_t *d_src, uint64_t *d_dst,
                 uint64_t *scratch, bool inverse);
// frees every cached twiddle table of this context (caller holds dev.mu)
void ntt_release(Device &dev);
}  // namespace zk
