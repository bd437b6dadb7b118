// zk_frdev.hpp -- device helpers shared by the Fr units (zk_arr.hip, zk_poly.hip): rows in the
// reference form x R around the internal radix (zk_arr.hip's header has the representation), the
// 256-thread block sum and the kernel that adds up block partials with it.
#pragma once
#include "zk_field.hpp"

namespace zk {

struct U256 {
  uint64_t w[4];
};

template <class F>
__device__ __forceinline__ void ld(Fe<F> &x, const uint64_t *p, size_t i) { fe_load_ref(x, p + i * 4); }
template <class F>
__device__ __forceinline__ void st(uint64_t *p, size_t i, const Fe<F> &x) { fe_store_ref(p + i * 4, x); }
template <class F>
__device__ __forceinline__ void ld_const(Fe<F> &x, const U256 &k) {
  uint32_t w[8];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    w[2 * j] = (uint32_t)k.w[j];
    w[2 * j + 1] = (uint32_t)(k.w[j] >> 32);
  }
  fe_unpack(x, w);
}
// reference-form product: (xR)(yR) -> xyR
template <class F>
__device__ __forceinline__ void mul_ref(Fe<F> &r, const Fe<F> &a, const Fe<F> &b) {
  Fe<F> t;
  fe_mul(t, a, b);
  fe_to_int(r, t);
}
template <class F>
__device__ __forceinline__ void lds_get(Fe<F> &x, const uint32_t *p) {
#pragma unroll
  for (int q = 0; q < F::N; q++) x.v[q] = p[q];
}
template <class F>
__device__ __forceinline__ void lds_put(uint32_t *p, const Fe<F> &x) {
#pragma unroll
  for (int q = 0; q < F::N; q++) p[q] = x.v[q];
}

// Block sum of one value per thread over DOT_THREADS * F::N words of LDS: thread 0 holds the sum
constexpr int DOT_THREADS = 256;
template <class F>
__device__ __forceinline__ void block_sum(Fe<F> &acc, uint32_t *lds) {
  lds_put(lds + threadIdx.x * F::N, acc);
  __syncthreads();
  for (int s = DOT_THREADS / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) {
      Fe<F> o, r;
      lds_get(o, lds + (threadIdx.x + s) * F::N);
      fe_add(r, acc, o);
      acc = r;
      lds_put(lds + threadIdx.x * F::N, acc);
    }
    __syncthreads();
  }
}
// The sum of nparts block partials: one block, each thread adding every DOT_THREADS-th partial, then
// block_sum (round 5 summed the 1024 partials of a dot product on ONE thread: 0.34 ms of a 0.55 ms
// 2^24 dot product, profiles/r06c_prof).  TO_INT closes with fe_to_int: partials in the R^2/R' form
// of k_dot leave as x y R^2/R' * R'/R = x y R (the product by 32 on the 9 x 29-bit fields).
template <class F, bool TO_INT>
__global__ void __launch_bounds__(DOT_THREADS) k_dot_final(int nparts, const uint64_t *__restrict__ part,
                                                           uint64_t *__restrict__ out) {
  __shared__ uint32_t lds[DOT_THREADS * F::N];
  Fe<F> acc;
  fe_zero(acc);
  for (int i = threadIdx.x; i < nparts; i += DOT_THREADS) {
    Fe<F> x, s;
    ld(x, part, i);
    fe_add(s, acc, x);
    acc = s;
  }
  block_sum(acc, lds);
  if (threadIdx.x == 0) {
    if (TO_INT) {
      Fe<F> r;
      fe_to_int(r, acc);
      st(out, 0, r);
    } else {
      st(out, 0, acc);
    }
  }
}

}  // namespace zk
