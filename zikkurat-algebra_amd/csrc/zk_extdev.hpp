// zk_extdev.hpp -- device helpers shared by the batch conversions of G1 (zk_g1ext.hip) and G2
// (zk_g2ext.hip): reference-form loads / stores around the internal Montgomery radix.
#pragma once
#include "zk_field.hpp"
#include "zk_field2.hpp"

namespace zk {

struct W6 {
  uint64_t w[6];
};

template <class F>
__device__ __forceinline__ void ld_int(Fe<F> &r, const uint64_t *p) {  // reference form -> internal
  Fe<F> t;
  fe_load_ref(t, p);
  fe_to_int(r, t);
}
template <class F>
__device__ __forceinline__ void st_ref(uint64_t *p, const Fe<F> &a) {  // internal -> canonical reference form
  Fe<F> t;
  fe_to_ref(t, a);
  fe_store_ref(p, t);
}
template <class F>
__device__ __forceinline__ bool ref_all_ones(const uint64_t *p, int words) {
  uint64_t a = ~0ull;
  for (int i = 0; i < words; i++) a &= p[i];
  return a == ~0ull;
}
// canonical reference-form words of a (internal form), or `alt` where !keep, stored as 16-B runs
template <class F>
__device__ __forceinline__ void st_ref_or(uint64_t *p, const Fe<F> &a, bool keep, const uint32_t (&alt)[F::NW]) {
  Fe<F> t;
  fe_to_ref(t, a);
  fe_canon(t);
  uint32_t w[F::NW];
  fe_pack(w, t);
#pragma unroll
  for (int i = 0; i < F::NW; i++) w[i] = keep ? w[i] : alt[i];
  uint4 *q = reinterpret_cast<uint4 *>(p);
#pragma unroll
  for (int i = 0; i < F::NW / 4; i++) q[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}

}  // namespace zk
