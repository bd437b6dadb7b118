// zk_member.hpp -- the fixed multiplication chains of the subgroup membership tests, shared by the group
// FFT's all-or-nothing test (zk_g1ext.hip, k_subgroup_check) and the batch point validation (zk_check*.hip).
// Every chain is the same for every lane: the scalar is a constant of the curve, so the trip counts and the
// positions of the additions are uniform and nothing depends on the point.  Jacobian doublings and cached
// additions of zk_fftdev.hpp; instantiates on the base fields and on Fp2.
#pragma once
#include "zk_fftdev.hpp"

namespace zk {

// r = [|z|] p for BLS12-381's z = -0xd201000000010000 (bits 63, 62, 60, 57, 48, 16): 63 doublings
// and 5 additions, the membership test's chain (k_subgroup_check)
template <class F>
__device__ __forceinline__ void jac_mul_absz(Jac<F> &r, const Jac<F> &p) {
  JacC<F> pc;
  jac_cache(pc, p);
  r = p;
  // runs of doublings between the set bits, each a rolled loop: the fully unrolled chain (63
  // inlined doublings) held 512 VGPRs and spilled 230 of them to scratch
  constexpr int kRun[6] = {1, 2, 3, 9, 32, 16};  // doublings before the additions at bits 62, 60, 57, 48, 16; tail
  for (int s = 0; s < 6; s++) {
#pragma unroll 1
    for (int i = 0; i < kRun[s]; i++) jac_dbl(r);
    if (s < 5 && !jac_is_inf(p)) jac_add_cached(r, pc);
  }
}

// The chains below keep the cached point (p with its Z^2, Z^3: 5 field elements) in the lane's `slot` of global
// scratch and read it back at every addition, as xyzz_scl reads its table: held in registers beside the
// accumulator and the temporaries of an Fp2 doubling it spilled (BLS12-381 G2: 162 to 350 VGPRs).  The empty
// asm keeps the compiler from hoisting the (loop-invariant) reads out of the loop, which would undo that.
template <class F>
constexpr int member_slot_words() { return 5 * F::SN; }
template <class F>
__device__ __forceinline__ void jac_slot_put(uint32_t *slot, const Jac<F> &p) {
  JacC<F> pc;
  jac_cache(pc, p);
  jacc_store(slot, pc);
}
template <class F>
__device__ __forceinline__ void jac_slot_get(JacC<F> &e, const uint32_t *slot) {
  asm volatile("" ::: "memory");
  jacc_load(e, slot);
}

// acc = [k] p for a uniform k > 0, binary from the top: one rolled loop whose body holds one doubling and one
// cached addition (p finite; acc may pass through infinity, which both routines take)
template <class F>
__device__ __forceinline__ void jac_mul_u64(Jac<F> &acc, const Jac<F> &p, uint64_t k, uint32_t *slot) {
  jac_slot_put(slot, p);
  acc = p;
  const int top = 63 - __builtin_clzll(k);
  uint64_t sh = top ? k << (64 - top) : 0;  // the bits below the top one, first at bit 63
#pragma unroll 1
  for (int i = 0; i < top; i++) {
    jac_dbl(acc);
    if (sh >> 63) {
      JacC<F> e;
      jac_slot_get(e, slot);
      jac_add_cached(acc, e);
    }
    sh <<= 1;
  }
}

// 256 digits in {-1, 0, 1} as two masks, most significant digit at bit 255 of w[3]
struct NafMask {
  uint64_t pos[4], neg[4];
};
// acc = [k] p for k = 2^count + sum of the `count` signed digits below it (a non-adjacent form with its top
// digit taken off, shifted so that the next digit is bit 255): count doublings, an addition of p or -p per
// non-zero digit.  The masks are uniform (kernel arguments) and shifted in registers, never indexed.
template <class F>
__device__ __forceinline__ void jac_mul_naf(Jac<F> &acc, const Jac<F> &p, const NafMask &m, int count,
                                            uint32_t *slot) {
  jac_slot_put(slot, p);
  acc = p;
  uint64_t a3 = m.pos[3], a2 = m.pos[2], a1 = m.pos[1], a0 = m.pos[0];
  uint64_t s3 = m.neg[3], s2 = m.neg[2], s1 = m.neg[1], s0 = m.neg[0];
#pragma unroll 1
  for (int i = 0; i < count; i++) {
    jac_dbl(acc);
    const bool add = (a3 >> 63) != 0, sub = (s3 >> 63) != 0;
    if (add || sub) {
      JacC<F> e;
      jac_slot_get(e, slot);
      if (sub) {
        Fe<F> ny;
        fe_neg(ny, e.Y);
        e.Y = ny;
      }
      jac_add_cached(acc, e);
    }
    a3 = (a3 << 1) | (a2 >> 63); a2 = (a2 << 1) | (a1 >> 63); a1 = (a1 << 1) | (a0 >> 63); a0 <<= 1;
    s3 = (s3 << 1) | (s2 >> 63); s2 = (s2 << 1) | (s1 >> 63); s1 = (s1 << 1) | (s0 >> 63); s0 <<= 1;
  }
}

// acc += b, either may be infinity
template <class F>
__device__ __forceinline__ void jac_add_full(Jac<F> &acc, const Jac<F> &b) {
  if (jac_is_inf(b)) return;
  JacC<F> c;
  jac_cache(c, b);
  jac_add_cached(acc, c);
}

}  // namespace zk
