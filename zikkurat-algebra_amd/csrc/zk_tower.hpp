// zk_tower.hpp -- the tower above Fp2 for the pairing kernels, over a per-lane workspace of Fp2 cells.
//
// Replaces, on the GPU, <C>_Fp6_mont_* / <C>_Fp12_mont_{mul,sqr,inv,frobenius} (lib/cbits/curves/fields/mont/
// <C>_Fp6_mont.c, <C>_Fp12_mont.c) with the reference's irreducibles: Fp6 = Fp2[v]/(v^3 - xi),
// Fp12 = Fp6[w]/(w^2 - v), xi = 9 + u (BN254) or 1 + u (BLS12-381).  An Fp12 value is held as the six Fp2
// coefficients of 1, w, .., w^5 (w^6 = xi) in six consecutive cells; the coefficient of w^i v^j is cell
// i + 2 j, and the reference's row keeps it at Fp2 index 3 i + j (tw_row_index).
//
// A BLS12-381 Fp12 value is 168 limbs, so no Fp12 value is ever held in registers: a cell lives in global
// memory at ws[(cell * 2 N + limb) * stride] (the lane's pointer is offset by the lane, so a wavefront's
// accesses are contiguous), and every product below is a rolled loop over ONE Fp2-product body with two Fp2
// accumulators.  All sums are the reduced fe_add / fe_sub (values < 2p): no new lazy accumulation.
#pragma once
#include "zk_extdev.hpp"
#include "zk_field2.hpp"

namespace zk {

__device__ __constant__ static const uint32_t kPairConstsBN[] = ZK_BN128_PAIR_CONSTS;
__device__ __constant__ static const uint32_t kPairConstsBLS[] = ZK_BLS12_381_PAIR_CONSTS;

template <class B>
struct TowerOf;
template <>
struct TowerOf<BN_Fp> {
  static constexpr int XI_A = ZK_BN128_PAIR_XI_A;
  static constexpr bool DTYPE = ZK_BN128_PAIR_DTYPE != 0;
  __device__ static const uint32_t *consts() { return kPairConstsBN; }
};
template <>
struct TowerOf<BLS_Fp> {
  static constexpr int XI_A = ZK_BLS12_381_PAIR_XI_A;
  static constexpr bool DTYPE = ZK_BLS12_381_PAIR_DTYPE != 0;
  __device__ static const uint32_t *consts() { return kPairConstsBLS; }
};
constexpr int TW_GAMMA = 0, TW_BT = 6, TW_ONE = 7;  // constant indices: gamma_0 .. gamma_5, b', one

// Fp2 index of cell k (the coefficient of w^k) in the reference's Fp12 row
__host__ __device__ constexpr int tw_row_index(int k) { return 3 * (k & 1) + (k >> 1); }

template <class B>
struct Cells {  // one lane's view of the workspace
  using F = F2<B>;
  uint32_t *p;
  size_t stride;
  __device__ __forceinline__ void ld(Fe<F> &r, int cell) const {
    const uint32_t *q = p + (size_t)cell * F::N * stride;
#pragma unroll
    for (int i = 0; i < F::N; i++) r.v[i] = q[(size_t)i * stride];
  }
  __device__ __forceinline__ void st(int cell, const Fe<F> &a) const {
    uint32_t *q = p + (size_t)cell * F::N * stride;
#pragma unroll
    for (int i = 0; i < F::N; i++) q[(size_t)i * stride] = a.v[i];
  }
};

template <class B>
__device__ __forceinline__ void tw_const(Fe<F2<B>> &r, int idx) {
  const uint32_t *c = TowerOf<B>::consts() + idx * 2 * B::N;
#pragma unroll
  for (int i = 0; i < 2 * B::N; i++) r.v[i] = c[i];
}
template <class B>
__device__ __forceinline__ void f2_conj(Fe<F2<B>> &r, const Fe<F2<B>> &a) {
  Fe<B> a0, a1, n1;
  f2_split(a0, a1, a);
  fe_neg(n1, a1);
  f2_join(r, a0, n1);
}
// a xi, xi = A + u: (A a0 - a1) + (A a1 + a0) u, A = 1 or 9 (8 a + a)
template <class B>
__device__ __forceinline__ void f2_mul_xi(Fe<F2<B>> &r, const Fe<F2<B>> &a) {
  Fe<F2<B>> s = a;
  if constexpr (TowerOf<B>::XI_A == 9) {
    Fe<F2<B>> t;
    fe_add(t, a, a);
    fe_add(s, t, t);
    fe_add(t, s, s);
    fe_add(s, t, a);
  } else {
    static_assert(TowerOf<B>::XI_A == 1, "xi = 1 + u or 9 + u");
  }
  Fe<B> s0, s1, a0, a1, r0, r1;
  f2_split(s0, s1, s);
  f2_split(a0, a1, a);
  fe_sub(r0, s0, a1);
  fe_add(r1, s1, a0);
  f2_join(r, r0, r1);
}
// 1 / a = conj(a) / (a0^2 + a1^2); 0 gives 0
template <class B>
__device__ __forceinline__ void f2_inv(Fe<F2<B>> &r, const Fe<F2<B>> &a) {
  Fe<B> a0, a1, s, t, n, r0, r1;
  f2_split(a0, a1, a);
  fe_sqr(s, a0);
  fe_sqr(t, a1);
  fe_add(n, s, t);
  fe_inv_sg(s, n);
  fe_mul(r0, a0, s);
  fe_mul(t, a1, s);
  fe_neg(r1, t);
  f2_join(r, r0, r1);
}

// the Fp12 products, cells d .. d + 5 <- (a .. a + 5) times b; d is distinct from a and b.
//   TW_FULL    b is six cells
//   TW_SQUARE  b = a: the 21 products a_i a_j, i <= j, the off-diagonal ones doubled
//   TW_SPARSE  b is the three cells (cy, cx, cc) of a line: cy + cx w + cc w^3 on the D-type twist,
//              cc + cx w^2 + cy w^3 on the M-type
enum { TW_FULL = 0, TW_SQUARE = 1, TW_SPARSE = 2 };
template <class B>
__device__ __forceinline__ void tw_mul12(const Cells<B> &ws, int d, int a, int b, int mode) {
  using F = F2<B>;
  const int terms = mode == TW_SPARSE ? 3 : 6;
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    Fe<F> lo, hi;
    fe_zero(lo);
    fe_zero(hi);
#pragma unroll 1
    for (int t = 0; t < terms; t++) {
      int ia, cb;
      bool wrap, dbl = false;
      if (mode == TW_SPARSE) {
        const int j = TowerOf<B>::DTYPE ? (t == 2 ? 3 : t) : (3 - t - (t == 2 ? 1 : 0));  // D: 0 1 3; M: 3 2 0
        ia = k - j;
        wrap = ia < 0;
        ia += wrap ? 6 : 0;
        cb = b + t;
      } else {
        ia = t;
        int j = k - t;
        wrap = j < 0;
        j += wrap ? 6 : 0;
        if (mode == TW_SQUARE) {
          if (ia > j) continue;
          dbl = ia < j;
        }
        cb = b + j;
      }
      Fe<F> x, y, pr;
      ws.ld(x, a + ia);
      ws.ld(y, cb);
      fe_mul(pr, x, y);
      if (dbl) fe_add(pr, pr, pr);
      if (wrap) fe_add(hi, hi, pr);
      else fe_add(lo, lo, pr);
    }
    Fe<F> h;
    f2_mul_xi(h, hi);
    fe_add(lo, lo, h);
    ws.st(d + k, lo);
  }
}
// (sum c_k w^k)^p = sum conj(c_k) gamma_k w^k; d may be a
template <class B>
__device__ __forceinline__ void tw_frob12(const Cells<B> &ws, int d, int a) {
  using F = F2<B>;
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    Fe<F> x, c, g, r;
    ws.ld(x, a + k);
    f2_conj(c, x);
    tw_const<B>(g, TW_GAMMA + k);
    fe_mul(r, c, g);
    ws.st(d + k, r);
  }
}
// the conjugate over Fp6 (x^(p^6)): the odd coefficients negated; d may be a
template <class B>
__device__ __forceinline__ void tw_conj12(const Cells<B> &ws, int d, int a) {
  using F = F2<B>;
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    Fe<F> x, r;
    ws.ld(x, a + k);
    if (k & 1) fe_neg(r, x);
    else r = x;
    ws.st(d + k, r);
  }
}
template <class B>
__device__ __forceinline__ void tw_one12(const Cells<B> &ws, int d) {
  using F = F2<B>;
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    Fe<F> r;
    if (k == 0) fe_one(r);
    else fe_zero(r);
    ws.st(d + k, r);
  }
}
// an Fp12 row of the reference (12 NP words, Montgomery form) <-> six cells
template <class B>
__device__ __forceinline__ void tw_load_row(const Cells<B> &ws, int d, const uint64_t *row) {
  using F = F2<B>;
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    Fe<F> x;
    ld_int(x, row + (size_t)tw_row_index(k) * 2 * B::N64);
    ws.st(d + k, x);
  }
}
template <class B>
__device__ __forceinline__ void tw_store_row(uint64_t *row, const Cells<B> &ws, int a) {
  using F = F2<B>;
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    Fe<F> x;
    ws.ld(x, a + k);
    st_ref(row + (size_t)tw_row_index(k) * 2 * B::N64, x);
  }
}

}  // namespace zk
