// zk_fftdev.hpp -- device routines of the group (curve) FFT's integer-scalar stages, shared by the G1
// transform (zk_g1ext.hip) and the G2 transform (zk_g2fft.hip): the XYZZ load, the Jacobian scalar
// multiplication (xyzz_scl) and the radix-2 stage kernels.  The templates instantiate on the base
// fields and on Fp2 (F2<B>, zk_field2.hpp); the Fp2 overloads of the Jacobian routines below take the
// exact formulas, the lazy forms are bounded for the base fields only (tools/lazy_bounds.py).
#pragma once
#include <hip/hip_runtime.h>
#include "zk_curve.hpp"
#include "zk_extdev.hpp"

namespace zk {

template <class F>
constexpr int xw() { return xyzz_words<F>(); }  // u32 words per stored XYZZ point

// reference projective -> device XYZZ (x = X/Z -> X' = X Z, ZZ = Z^2; y = Y/Z -> Y' = Y Z^2,
// ZZZ = Z^3), stored at bitrev_m(i) when m > 0 (forward FFT input order); Jacobian (x = X/Z^2,
// y = Y/Z^3) -> X' = X, Y' = Y, ZZ = Z^2, ZZZ = Z^3
template <class C, bool JAC>
__global__ void __launch_bounds__(256) k_fft_load(int n, int bitrev_m, const uint64_t *__restrict__ src,
                                                  uint32_t *__restrict__ dst) {
  using F = typename C::Fp;
  constexpr int NP = C::NP64;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n) return;
  Fe<F> X, Y, Z;
  ld_int(X, src + i * 3 * NP);
  ld_int(Y, src + i * 3 * NP + NP);
  ld_int(Z, src + i * 3 * NP + 2 * NP);
  Xyzz<F> p;
  if (fe_is_zero(Z)) {
    xyzz_set_inf(p);
  } else {
    fe_sqr(p.ZZ, Z);
    fe_mul(p.ZZZ, p.ZZ, Z);
    if (JAC) {
      p.X = X;
      p.Y = Y;
    } else {
      fe_mul(p.X, X, Z);
      fe_mul(p.Y, Y, p.ZZ);
    }
  }
  const size_t o = bitrev_m > 0 ? (size_t)(__builtin_bitreverse32((uint32_t)i) >> (32 - bitrev_m)) : i;
  xyzz_store(dst + o * xw<F>(), p);
}

template <class F>
__device__ __forceinline__ void xyzz_neg(Xyzz<F> &r, const Xyzz<F> &a) {
  r = a;
  fe_neg(r.Y, a.Y);
}

// Scalar multiplication r = k P for the group FFT (k a 256-bit integer, 4 u64), computed with
// the accumulator in JACOBIAN coordinates: the chain is 255 doublings, and a Jacobian doubling
// (dbl-2009-l, a = 0) is 7 products against XYZZ's 9; additions take the table entry with its
// Z^2, Z^3 cached (add-1998-cmo-2: 14 products, as XYZZ's).  Digits: signed 5-bit windows
// (K = k + sum_i 16 * 32^i, digit i = bits [5i, 5i + 5) of K minus 16, in [-16, 15]; K < 2^260
// as k < 2^256 - 2^255), so at most 52 additions instead of 64 with a 16-point table.
// 255 x 7 + 52 x 14 + table 241 = ~2750 products per multiplication (was ~3350).
template <class F>
struct Jac {
  Fe<F> X, Y, Z;  // x = X / Z^2, y = Y / Z^3; Z = 0: infinity
};
// Round 5 form (ZK_FFT_DBL2, default): D = 4 X B as one product instead of 2((X + B)^2 - A - C),
// and Y3 = E (D - X3) + (-8B) B as ONE shared-reduction pair (fe_mul2k: Karatsuba columns of both
// products, one Montgomery reduction), so C = B^2 is never reduced on its own: 4 products + 1
// pair, 6 reductions instead of 7, and three exact additions fewer.  Bounds: every operand < 2p,
// E (D - X3) + (-8B) B < 8 p^2 < p R' (R' / p = 2^11), so the pair's output is < 2p like fe_mul's.
#ifndef ZK_FFT_DBL2
#define ZK_FFT_DBL2 1
#endif
// the point routines' products: Karatsuba columns (fe_mulk, 436 vs 472 issue slots per 381-bit
// product) with ZK_FFT_DBL2, the schoolbook fe_mul of round 4 otherwise (A/B)
template <class F>
__device__ __forceinline__ void fft_mul(Fe<F> &r, const Fe<F> &a, const Fe<F> &b) {
#if ZK_FFT_DBL2
  fe_mulk(r, a, b);
#else
  fe_mul(r, a, b);
#endif
}
// Fp2: fe_mulk has no Fp2 form; the product is zk_field2.hpp's two shared-reduction pairs
template <class B>
__device__ __forceinline__ void fft_mul(Fe<F2<B>> &r, const Fe<F2<B>> &a, const Fe<F2<B>> &b) {
  fe_mul(r, a, b);
}
// Lazy form (ZK_FFT_LAZY, default, both base fields): the doubling and the cached addition take no
// exact addition / subtraction (each two carry chains, ~56 issue slots) except the two whose
// results are tested for zero (the addition's H and r): multiples are folded into products (4X B,
// (2Y) Z), differences are a + K p - b (fe_sub_lazy) re-normalised where a product takes them.
// Invariant of a Jacobian accumulator / table entry: X < 10p, Y, Z < 2p, normalised limbs (every
// consumer of X multiplies it: the XYZZ it is converted to keeps X < 10p, which xyzz_add and the
// normalisation only multiply).  tools/lazy_bounds.py (jac_dbl_lazy, jac_add_cached_lazy) replays
// both routines on that invariant for each field: outputs X < 9p, every column < 2^64, and Y, Z < 1.02p
// on BLS12-381 (R'/p ~ 2520) but Y < 1.41p, Z < 1.05p on BN254 (R'/p ~ 169: the Y3 pair's larger
// quotient) -- still inside the < 2p invariant; `python tools/lazy_bounds.py` prints these per field.
#ifndef ZK_FFT_LAZY
#define ZK_FFT_LAZY 1
#endif
template <class F>
__device__ __forceinline__ void jac_dbl(Jac<F> &p) {  // in place; infinity stays infinity
#if ZK_FFT_LAZY
  if constexpr (F::N == 14 || (F::N == 9 && F::RB == 29)) {
    Fe<F> A, B, D, E, F2, X3, t, x4, y2, nb, nb8;
    fe_sqr(A, p.X);                        // X < 10p
    fe_sqr(B, p.Y);
    fe_add_lazy(x4, p.X, p.X);
    fe_add_lazy(x4, x4, x4);               // 4X < 40p, limbs < 2^30
    fe_mulk(D, x4, B);                     // D = 4 X B
    fe_add_lazy(E, A, A);
    fe_add_lazy(E, E, A);                  // E = 3A < 6p
    if constexpr (F::N == 9) fe_norm(E);  // 29-bit limbs: the doubled limbs of the square
    fe_sqr(F2, E);                         // F = E^2
    fe_add_lazy(t, D, D);                  // 2D < 4p
    fe_sub_lazy<F, 8, 2>(X3, F2, t);       // X3 = F - 2D < 9p
    fe_norm(X3);
    fe_add_lazy(y2, p.Y, p.Y);
    fe_mulk(p.Z, y2, p.Z);                 // Z3 = (2Y) Z
    fe_sub_lazy<F, 10, 1>(t, D, X3);       // D - X3 < 12p
    fe_norm(t);
    fe_sub_lazy<F, 2, 1>(nb, Fe<F>{}, B);  // 2p - B
    fe_norm(nb);
    fe_add_lazy(nb8, nb, nb);
    fe_add_lazy(nb8, nb8, nb8);
    fe_add_lazy(nb8, nb8, nb8);            // 8 (2p - B) < 16p
    if constexpr (F::N == 9) fe_norm(nb8);  // 29-bit limbs: 8x would reach 2^32
    fe_mul2k(p.Y, E, t, nb8, B);           // Y3 = E (D - X3) - 8 B^2
    p.X = X3;
    return;
  }
#endif
#if ZK_FFT_DBL2
  Fe<F> A, B, D, E, F2, X3, t, u;
  fe_sqr(A, p.X);
  fe_sqr(B, p.Y);
  fe_mulk(t, p.X, B);
  fe_add(t, t, t);
  fe_add(D, t, t);          // D = 4 X B  (= 2((X + B)^2 - A - C))
  fe_mul3(E, A);            // E = 3A
  fe_sqr(F2, E);            // F = E^2
  fe_sub(t, F2, D);
  fe_sub(X3, t, D);         // X3 = F - 2D
  fe_mulk(u, p.Y, p.Z);
  fe_add(p.Z, u, u);        // Z3 = 2 Y Z
  fe_sub(t, D, X3);
  Fe<F> b8, nb8;
  fe_add(b8, B, B);
  fe_add(b8, b8, b8);
  fe_add(b8, b8, b8);       // 8B
  fe_neg(nb8, b8);
  fe_mul2k(p.Y, E, t, nb8, B);  // Y3 = E (D - X3) - 8 B^2
  p.X = X3;
#else
  Fe<F> A, B, C, D, E, t, u;
  fe_sqr(A, p.X);
  fe_sqr(B, p.Y);
  fe_sqr(C, B);
  fe_add(t, p.X, B);
  fe_sqr(u, t);
  fe_sub(u, u, A);
  fe_sub(u, u, C);
  fe_add(D, u, u);          // D = 2((X + B)^2 - A - C)
  fe_mul3(E, A);            // E = 3A
  fe_sqr(t, E);             // F = E^2
  fe_sub(t, t, D);
  Fe<F> X3;
  fe_sub(X3, t, D);         // X3 = F - 2D
  fe_mul(u, p.Y, p.Z);
  fe_add(p.Z, u, u);        // Z3 = 2 Y Z
  fe_sub(t, D, X3);
  fe_mul(u, E, t);          // E (D - X3)
  fe_add(C, C, C);
  fe_add(C, C, C);
  fe_add(C, C, C);          // 8C
  fe_sub(p.Y, u, C);
  p.X = X3;
#endif
}
// Fp2 (the G2 transform): the exact dbl-2009-l, every value < 2p -- 5 squarings and 2 products (an Fp2
// squaring is two base products, an Fp2 product four limb products in two reductions, so the form with
// C = B^2 and (X + B)^2 is the cheaper one here).  No lazy form: the bounds are derived for the base
// fields only.
template <class B>
__device__ __forceinline__ void jac_dbl(Jac<F2<B>> &p) {  // in place; infinity stays infinity
  using F = F2<B>;
  Fe<F> A, Bq, C, D, E, t, u, X3;
  fe_sqr(A, p.X);
  fe_sqr(Bq, p.Y);
  fe_sqr(C, Bq);
  fe_add(t, p.X, Bq);
  fe_sqr(u, t);
  fe_sub(u, u, A);
  fe_sub(u, u, C);
  fe_add(D, u, u);          // D = 2((X + B)^2 - A - C)
  fe_mul3(E, A);            // E = 3A
  fe_sqr(t, E);             // F = E^2
  fe_sub(t, t, D);
  fe_sub(X3, t, D);         // X3 = F - 2D
  fe_mul(u, p.Y, p.Z);
  fe_add(p.Z, u, u);        // Z3 = 2 Y Z
  fe_sub(t, D, X3);
  fe_mul(u, E, t);          // E (D - X3)
  fe_add(C, C, C);
  fe_add(C, C, C);
  fe_add(C, C, C);          // 8C
  fe_sub(p.Y, u, C);
  p.X = X3;
}
// table entry: the point and its Z^2, Z^3
template <class F>
struct JacC {
  Fe<F> X, Y, Z, ZZ, ZZZ;
};
template <class F>
__device__ __forceinline__ void jac_cache(JacC<F> &c, const Jac<F> &p) {
  c.X = p.X;
  c.Y = p.Y;
  c.Z = p.Z;
  fe_sqr(c.ZZ, p.Z);
  fe_mul(c.ZZZ, c.ZZ, p.Z);
}
template <class F>
__device__ __forceinline__ bool jac_is_inf(const Jac<F> &p) { return fe_is_zero(p.Z); }
// acc += b (b cached, b not infinity); all special cases handled
template <class F>
__device__ __forceinline__ void jac_add_cached(Jac<F> &acc, const JacC<F> &b) {
  if (jac_is_inf(acc)) {
    acc.X = b.X;
    acc.Y = b.Y;
    acc.Z = b.Z;
    return;
  }
  Fe<F> Z1Z1, U1, U2, S1, S2, H, r, t;
  fe_sqr(Z1Z1, acc.Z);
  fft_mul(U1, acc.X, b.ZZ);
  fft_mul(U2, b.X, Z1Z1);
  fft_mul(S1, acc.Y, b.ZZZ);
  fft_mul(t, acc.Z, Z1Z1);
  fft_mul(S2, b.Y, t);
  fe_sub(H, U2, U1);
  fe_sub(r, S2, S1);
  if (fe_is_zero(H)) {
    if (fe_is_zero(r)) jac_dbl(acc);  // acc == b
    else fe_zero(acc.Z);              // acc == -b
    return;
  }
  Fe<F> HH, HHH, V, X3;
  fe_sqr(HH, H);
  fft_mul(HHH, H, HH);
  fft_mul(V, U1, HH);
#if ZK_FFT_LAZY
  if constexpr (F::N == 14 || (F::N == 9 && F::RB == 29)) {
    Fe<F> RR, v2, nS1;
    fe_sqr(RR, r);
    fe_sub_lazy<F, 2, 1>(t, RR, HHH);      // RR - HHH < 4p
    fe_add_lazy(v2, V, V);
    fe_sub_lazy<F, 6, 2>(X3, t, v2);       // X3 = r^2 - HHH - 2V < 9p
    fe_norm(X3);
    fe_sub_lazy<F, 12, 1>(t, V, X3);       // V - X3 < 14p
    fe_norm(t);
    fe_sub_lazy<F, 2, 1>(nS1, Fe<F>{}, S1);
    fe_norm(nS1);
    fe_mul2k(acc.Y, r, t, nS1, HHH);       // Y3 = r (V - X3) - S1 HHH
    fft_mul(t, acc.Z, b.Z);
    fft_mul(acc.Z, t, H);                  // Z3 = Z1 Z2 H
    acc.X = X3;
    return;
  }
#endif
  fe_sqr(t, r);
  fe_sub(t, t, HHH);
  fe_sub(t, t, V);
  fe_sub(X3, t, V);         // X3 = r^2 - HHH - 2V
  fe_sub(t, V, X3);
#if ZK_FFT_DBL2
  Fe<F> nS1;
  fe_neg(nS1, S1);
  fe_mul2k(acc.Y, r, t, nS1, HHH);  // Y3 = r (V - X3) - S1 HHH, one shared reduction (< 8 p^2 < p R')
#else
  fe_mul(V, r, t);          // r (V - X3)
  fe_mul(t, S1, HHH);
  fe_sub(acc.Y, V, t);
#endif
  fft_mul(t, acc.Z, b.Z);
  fft_mul(acc.Z, t, H);     // Z3 = Z1 Z2 H
  acc.X = X3;
}
// Fp2: the exact add-1998-cmo-2 (every value < 2p), the same special cases
template <class B>
__device__ __forceinline__ void jac_add_cached(Jac<F2<B>> &acc, const JacC<F2<B>> &b) {
  using F = F2<B>;
  if (jac_is_inf(acc)) {
    acc.X = b.X;
    acc.Y = b.Y;
    acc.Z = b.Z;
    return;
  }
  Fe<F> Z1Z1, U1, U2, S1, S2, H, r, t;
  fe_sqr(Z1Z1, acc.Z);
  fft_mul(U1, acc.X, b.ZZ);
  fft_mul(U2, b.X, Z1Z1);
  fft_mul(S1, acc.Y, b.ZZZ);
  fft_mul(t, acc.Z, Z1Z1);
  fft_mul(S2, b.Y, t);
  fe_sub(H, U2, U1);
  fe_sub(r, S2, S1);
  if (fe_is_zero(H)) {
    if (fe_is_zero(r)) jac_dbl(acc);  // acc == b
    else fe_zero(acc.Z);              // acc == -b
    return;
  }
  Fe<F> HH, HHH, V, X3;
  fe_sqr(HH, H);
  fft_mul(HHH, H, HH);
  fft_mul(V, U1, HH);
  fe_sqr(t, r);
  fe_sub(t, t, HHH);
  fe_sub(t, t, V);
  fe_sub(X3, t, V);         // X3 = r^2 - HHH - 2V
  fe_sub(t, V, X3);
  fft_mul(V, r, t);         // r (V - X3)
  fft_mul(t, S1, HHH);
  fe_sub(acc.Y, V, t);
  fft_mul(t, acc.Z, b.Z);
  fft_mul(acc.Z, t, H);     // Z3 = Z1 Z2 H
  acc.X = X3;
}
template <class F>
__device__ __forceinline__ void jacc_store(uint32_t *p, const JacC<F> &c) {
  fe_store_u(p + 0 * F::SN, c.X);
  fe_store_u(p + 1 * F::SN, c.Y);
  fe_store_u(p + 2 * F::SN, c.Z);
  fe_store_u(p + 3 * F::SN, c.ZZ);
  fe_store_u(p + 4 * F::SN, c.ZZZ);
}
template <class F>
__device__ __forceinline__ void jacc_load(JacC<F> &c, const uint32_t *p) {
  fe_load_u(c.X, p + 0 * F::SN);
  fe_load_u(c.Y, p + 1 * F::SN);
  fe_load_u(c.Z, p + 2 * F::SN);
  fe_load_u(c.ZZ, p + 3 * F::SN);
  fe_load_u(c.ZZZ, p + 4 * F::SN);
}
constexpr int SCL_TAB = 16;                                  // table entries d P, d = 1..16
template <class F>
constexpr int scl_tab_words() { return SCL_TAB * 5 * F::SN; }  // u32 words of one lane's table
// window i (5 bits) of the 261-bit K held in 5 u64 words
__device__ __forceinline__ uint32_t win5(const uint64_t *K, int i) {
  const int b = 5 * i, w = b >> 6, o = b & 63;
  uint64_t v = K[w] >> o;
  if (o > 59 && w < 4) v |= K[w + 1] << (64 - o);
  return (uint32_t)v & 31u;
}
// Every point routine of the group FFT is inlined into its kernel.  Round 4's first Jacobian
// build left xyzz_scl outlined (a real call: s_swappc_b64 into it, s_setpc_b64 s[30:31] back), and
// LLVM's branch relaxation of a long branch inside the callee took s[30:31] -- the return address
// -- as its scratch pair without saving it, so the return jumped into the callee's own body and
// the kernel never finished (profiles/r05*_fft_outlined_scl.txt holds the disassembly of that
// variant, built with -DZK_FFT_SCL_ATTR=__noinline__).  tests/test_isa_guard.py checks the
// shipped code object: no group-FFT kernel may contain a call.
#ifndef ZK_FFT_SCL_ATTR
#define ZK_FFT_SCL_ATTR __forceinline__
#endif
// INF_ROWS: a table entry d P may be the point at infinity (P of an order <= 16: 3 and 11 divide the
// BLS12-381 G1 cofactor) and is then skipped; jac_add_cached takes finite entries only.  The group FFT's
// stages are compiled without it, as before; the per-row scalar multiplications (zk_scl.hip) with it.
template <class F, bool INF_ROWS = false>
__device__ ZK_FFT_SCL_ATTR void xyzz_scl(Xyzz<F> &r, const Xyzz<F> &P, const uint64_t *k, uint32_t *__restrict__ tab) {
  if (xyzz_is_inf(P)) {
    r = P;
    return;
  }
  {  // P in Jacobian form: Z' = ZZ ZZZ, X' = X ZZ ZZZ^2, Y' = Y ZZZ^4 (valid XYZZ has ZZ^3 = ZZZ^2)
    Jac<F> p, acc;
    Fe<F> z2, z4, t;
    fe_sqr(z2, P.ZZZ);
    fe_mul(t, P.X, P.ZZ);
    fe_mul(p.X, t, z2);
    fe_sqr(z4, z2);
    fe_mul(p.Y, P.Y, z4);
    fe_mul(p.Z, P.ZZ, P.ZZZ);
    JacC<F> pc, c;
    jac_cache(pc, p);
    jacc_store(tab, pc);
    acc = p;
    jac_dbl(acc);
    jac_cache(c, acc);
    jacc_store(tab + 1 * 5 * F::SN, c);
    for (int d = 3; d <= SCL_TAB; d++) {
      jac_add_cached(acc, pc);
      jac_cache(c, acc);
      jacc_store(tab + (size_t)(d - 1) * 5 * F::SN, c);
    }
  }
  uint64_t K[5];
  {
    const uint64_t H[5] = {0x0842108421084210ull, 0x1084210842108421ull, 0x2108421084210842ull,
                           0x4210842108421084ull, 0x8ull};
    uint64_t cy = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
      const uint64_t a = j < 4 ? k[j] : 0, s1 = a + H[j];
      const uint64_t c1 = s1 < a ? 1 : 0, s2 = s1 + cy;
      K[j] = s2;
      cy = c1 | (s2 < s1 ? 1 : 0);
    }
  }
  Jac<F> acc;
  fe_one(acc.X);
  fe_one(acc.Y);
  fe_zero(acc.Z);
  for (int i = 51; i >= 0; i--) {
    if (i != 51)
      for (int z = 0; z < 5; z++) jac_dbl(acc);
    const int d = (int)win5(K, i) - 16;
    if (d) {
      JacC<F> e;
      jacc_load(e, tab + (size_t)((d < 0 ? -d : d) - 1) * 5 * F::SN);
      if (d < 0) {
        Fe<F> ny;
        fe_neg(ny, e.Y);
        e.Y = ny;
      }
      if (!INF_ROWS || !fe_is_zero(e.Z)) jac_add_cached(acc, e);
    }
  }
  if (jac_is_inf(acc)) {
    xyzz_set_inf(r);
    return;
  }
  r.X = acc.X;
  r.Y = acc.Y;
  fe_sqr(r.ZZ, acc.Z);
  fe_mul(r.ZZZ, r.ZZ, acc.Z);
}

// forward DIT stage s (block 2^s): lane = butterfly (blk, j); t = w_s^j v (w_s^j = tw[j 2^(m-s)],
// canonical Fr in standard form, = 1 for j = 0); out = (u + t, u - t)
template <class C>
__global__ void __launch_bounds__(256) k_fft_fwd_stage(int m, int s, const uint32_t *__restrict__ A,
                                                       uint32_t *__restrict__ B, const uint64_t *__restrict__ tw,
                                                       uint32_t *__restrict__ scratch, int lanes) {
  using F = typename C::Fp;
  const int half = 1 << (s - 1);
  const size_t nb = (size_t)1 << (m - 1);
  for (size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += (size_t)lanes) {
    const size_t blk = b >> (s - 1), j = b & (half - 1);
    const size_t k0 = (blk << s) + j;
    Xyzz<F> u, v, t;
    xyzz_load(u, A + k0 * xw<F>());
    xyzz_load(v, A + (k0 + half) * xw<F>());
    if (j == 0) {
      t = v;
    } else {
      const uint64_t *k = tw + (j << (m - s)) * 4;
      xyzz_scl(t, v, k, scratch + ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * scl_tab_words<F>());
    }
    Xyzz<F> x = u, nt;
    xyzz_add(x, t);
    xyzz_neg(nt, t);
    xyzz_add(u, nt);
    xyzz_store(B + k0 * xw<F>(), x);
    xyzz_store(B + (k0 + half) * xw<F>(), u);
  }
}

// inverse DIF stage s: lane = output (butterfly, which): which 0 -> (u + v) * 1/2,
// which 1 -> (u - v) * (w_s^-j / 2) (tw[e] = inv(w)^e / 2, standard form); half = std(1/2)
template <class C>
__global__ void __launch_bounds__(256) k_fft_inv_stage(int m, int s, const uint32_t *__restrict__ A,
                                                       uint32_t *__restrict__ B, const uint64_t *__restrict__ tw,
                                                       uint32_t *__restrict__ scratch, int lanes) {
  using F = typename C::Fp;
  const int half = 1 << (s - 1);
  const size_t no = (size_t)1 << m;
  for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < no; o += (size_t)lanes) {
    const size_t b = o >> 1;
    const int which = (int)(o & 1);
    const size_t blk = b >> (s - 1), j = b & (half - 1);
    const size_t k0 = (blk << s) + j;
    Xyzz<F> u, v, t;
    xyzz_load(u, A + k0 * xw<F>());
    xyzz_load(v, A + (k0 + half) * xw<F>());
    if (which == 0) {
      xyzz_add(u, v);
    } else {
      Xyzz<F> nv;
      xyzz_neg(nv, v);
      xyzz_add(u, nv);
    }
    const uint64_t *k = tw + (which ? (j << (m - s)) : 0) * 4;  // tw[0] = 1/2
    xyzz_scl(t, u, k, scratch + ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * scl_tab_words<F>());
    xyzz_store(B + (k0 + (which ? half : 0)) * xw<F>(), t);
  }
}

// the integer stages' twiddles, enqueued on st (zk_g1ext.hip): tw[e] = std(w^e) forward, std((w^-1)^e / 2)
// inverse, e < cnt, 4 u64 each -- the reference's gpow sequences (G1_proj.c:705-711, 758-764; the G2
// file's are the same), canonical Fr in standard form; gen: the host's Montgomery generator
void fft_int_twiddles(int curve, hipStream_t st, const uint64_t *gen, bool inverse, size_t cnt, uint64_t *tw);

// the group FFT's closing normalisation on its own, enqueued on st (zk_g1ext.hip, k_norm_chunks): n G1 XYZZ
// rows `src` (ZZ = 0: infinity) -> rows (x : y : 1) / (0 : 1 : 0) of 3 NP words, or with `affine` rows
// (x, y) of 2 NP words, all-0xFF at infinity; scratch: n NP words.  The scalar multiplications of
// zk_scl.hip end with it.
void g1_norm_xyzz_enqueue(int curve, hipStream_t st, int n, const uint32_t *src, uint64_t *scratch, uint64_t *tgt,
                          bool affine);

}  // namespace zk
