// zk_check_impl.hpp -- kernel templates and the call body of the batch point validation
// (zkg_g{1,2}_check_rows; instantiated by zk_check.hip for G1 and zk_check_g2_{bn,bls}.hip for G2).
//
// Two passes and a count, all on the call's stream:
//   k_check_curve   one lane per row, one pass over the row: CANONICAL by an integer compare of every Fp
//                   component with p, ON_CURVE / INFINITY by the curve equation of the row's coordinate system
//                   with the reduced field routines -- exactly the reference's _is_on_curve / _is_infinity
//                   (bls12_381_G1_affine.c:62-110, _G1_proj.c:173-205, _G1_jac.c:164-209 and their G2 / BN128
//                   twins).  Memory-bound; writes the flag byte.  A row that is not canonical is computed on
//                   like any other (fixed trip counts) and gets flag 0.
//   k_check_member  the hot path: rows that are on the curve and finite get IN_SUBGROUP from a multiplication
//                   chain that is the same for every lane (zk_member.hpp); the others leave their lane idle.
//                   EXACT is the definition, [r]P = O over r's non-adjacent form; the other kinds are the
//                   endomorphism tests tools/gen_subgroup.py checks against it:
//                     BLS12-381 G1   phi(P) == [z^2 - 1]P  (the group FFT's k_subgroup_check arithmetic)
//                     BLS12-381 G2   psi(P) + [|z|]P == O
//                     BN254 G2       [x + 1]P + psi([x]P) + psi^2([x]P) - psi^3([2x]P) == O
//                   BN254 G1 has cofactor 1: k_check_curve sets IN_SUBGROUP itself and no chain runs.
//   k_check_count   rows lacking any of CANONICAL | ON_CURVE | IN_SUBGROUP, one word read back.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstring>
#include <type_traits>
#include "zk_check.hpp"
#include "zk_curve.hpp"
#include "zk_dispatch.hpp"
#include "zk_extdev.hpp"
#include "zk_member.hpp"
#include "zk_runtime.hpp"

namespace zk {

#include "zk_check.inc"

enum { CHK_NONE = 0, CHK_EXACT = 1, CHK_BLS_G1 = 2, CHK_BLS_G2 = 3, CHK_BN_G2 = 4 };
template <class C>
constexpr int chk_default_kind() {
  return std::is_same<C, BN254>::value ? CHK_NONE
         : std::is_same<C, BLS381>::value ? CHK_BLS_G1
         : std::is_same<C, BLS381_G2>::value ? CHK_BLS_G2
                                             : CHK_BN_G2;
}

template <class F>
struct BaseWords {
  static constexpr int value = F::N64;
};
template <class B>
struct BaseWords<F2<B>> {
  static constexpr int value = B::N64;
};

// constants of one group (kernel argument): p; b (G1) or b' (G2); cx, cy: psi's factors on G2, cx = beta on
// BLS12-381 G1; r's digits for the exact chain; k: |z| or x
template <class C>
struct ChkConsts {
  static constexpr int NP = C::NP64, NB = BaseWords<typename C::Fp>::value;
  uint64_t p[NB], b[NP], cx[NP], cy[NP];
  NafMask naf;
  int naf_count;
  uint64_t k;
};

// x < p as integers (NB words each): the borrow of x - p
template <int NB>
__device__ __forceinline__ bool chk_lt_p(const uint64_t *__restrict__ x, const uint64_t *p) {
  uint64_t br = 0;
#pragma unroll
  for (int j = 0; j < NB; j++) {
    const uint64_t a = x[j], d = a - p[j];
    const uint64_t b1 = a < p[j] ? 1 : 0, b2 = d < br ? 1 : 0;
    br = b1 | b2;
  }
  return br != 0;
}

template <class C, int COORDS>
__global__ void __launch_bounds__(256) k_check_curve(int n, const uint64_t *__restrict__ pts, ChkConsts<C> cc,
                                                     int curve_is_member, uint8_t *__restrict__ flags) {
  using F = typename C::Fp;
  constexpr int NP = C::NP64, NB = ChkConsts<C>::NB, NC = COORDS == COORDS_AFFINE ? 2 : 3;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n) return;
  const uint64_t *row = pts + i * NC * NP;
  bool canon = true;
#pragma unroll
  for (int k = 0; k < NC * NP / NB; k++) canon = canon && chk_lt_p<NB>(row + k * NB, cc.p);
  const bool aff_inf = COORDS == COORDS_AFFINE && ref_all_ones<F>(row, 2 * NP);
  canon = canon || aff_inf;
  Fe<F> X, Y, b, lhs, rhs, t, d;
  ld_int(X, row);
  ld_int(Y, row + NP);
  ld_int(b, cc.b);
  fe_sqr(t, X);
  fe_mul(rhs, t, X);  // X^3
  fe_sqr(lhs, Y);     // Y^2
  bool on, inf;
  if constexpr (COORDS == COORDS_AFFINE) {
    fe_add(rhs, rhs, b);
    fe_sub(d, lhs, rhs);  // y^2 - x^3 - b
    on = aff_inf || fe_is_zero(d);
    inf = aff_inf;
  } else {
    Fe<F> Z, z2, z3;
    ld_int(Z, row + 2 * NP);
    fe_sqr(z2, Z);
    if constexpr (COORDS == COORDS_PROJ) {
      fe_mul(z3, z2, Z);
      fe_mul(t, lhs, Z);
      lhs = t;  // Y^2 Z
    } else {
      fe_sqr(t, z2);
      fe_mul(z3, t, z2);  // Z^6
    }
    fe_mul(t, z3, b);
    fe_add(rhs, rhs, t);
    fe_sub(d, lhs, rhs);
    const bool zz = fe_is_zero(Z);
    on = fe_is_zero(d) && (!zz || !fe_is_zero(Y));
    inf = on && zz;  // projective: X^3 = 0 there, so (0 : Y : 0), Y != 0; Jacobian: Y^2 = X^3 with X, Y != 0
  }
  uint8_t f = 0;
  if (canon) {
    f = PT_CANONICAL;
    if (on) f |= PT_ON_CURVE;
    if (inf) f |= PT_INFINITY;
    if (on && (inf || curve_is_member)) f |= PT_IN_SUBGROUP;
  }
  flags[i] = f;
}

// the row as a Jacobian point (the row is on the curve and finite, so Z != 0)
template <class C>
__device__ __forceinline__ void chk_load_jac(Jac<typename C::Fp> &p, const uint64_t *__restrict__ row, int coords) {
  using F = typename C::Fp;
  constexpr int NP = C::NP64;
  ld_int(p.X, row);
  ld_int(p.Y, row + NP);
  if (coords == COORDS_AFFINE) {
    fe_one(p.Z);
    return;
  }
  ld_int(p.Z, row + 2 * NP);
  if (coords == COORDS_PROJ) {  // (X / Z, Y / Z) = (X Z / Z^2, Y Z^2 / Z^3)
    Fe<F> t, z2;
    fe_mul(t, p.X, p.Z);
    p.X = t;
    fe_sqr(z2, p.Z);
    fe_mul(t, p.Y, z2);
    p.Y = t;
  }
}

template <class B>
__device__ __forceinline__ void chk_conj(Fe<F2<B>> &r, const Fe<F2<B>> &a) {
  Fe<B> a0, a1, n1;
  f2_split(a0, a1, a);
  fe_neg(n1, a1);
  f2_join(r, a0, n1);
}
// psi(X : Y : Z) = (cx conj(X) : cy conj(Y) : conj(Z)) on the twist; r may be a
template <class F>
__device__ __forceinline__ void jac_psi(Jac<F> &r, const Jac<F> &a, const Fe<F> &cx, const Fe<F> &cy) {
  Fe<F> t;
  chk_conj(t, a.X);
  fe_mul(r.X, cx, t);
  chk_conj(t, a.Y);
  fe_mul(r.Y, cy, t);
  chk_conj(t, a.Z);
  r.Z = t;
}

template <class C, int KIND>
__global__ void __launch_bounds__(256) k_check_member(int n, const uint64_t *__restrict__ pts, int coords,
                                                      ChkConsts<C> cc, uint8_t *__restrict__ flags, int lanes,
                                                      uint32_t *scratch) {
  using F = typename C::Fp;
  constexpr int NP = C::NP64;
  const int nc = coords == COORDS_AFFINE ? 2 : 3;
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t *slot = scratch + lane * member_slot_words<F>();  // lane < lanes: the grid is lanes / 256 blocks
  for (size_t i = lane; i < (size_t)n; i += (size_t)lanes) {
    const uint8_t f = flags[i];
    if ((f & (PT_ON_CURVE | PT_INFINITY)) != PT_ON_CURVE) continue;
    const uint64_t *row = pts + i * nc * NP;
    Jac<F> p;
    chk_load_jac<C>(p, row, coords);
    bool ok = false;
    if constexpr (KIND == CHK_EXACT) {
      Jac<F> r;
      jac_mul_naf(r, p, cc.naf, cc.naf_count, slot);
      ok = jac_is_inf(r);
    } else if constexpr (KIND == CHK_BLS_G1) {
      // [z^2 - 1]P = [|z|]([|z|]P) - P against phi(P) = (beta X : Y : Z).  As in k_subgroup_check the two
      // chains are one rolled loop and P is read again afterwards instead of staying live across them.
      Jac<F> r = p;
#pragma unroll 1
      for (int rep = 0; rep < 2; rep++) {
        Jac<F> t;
        jac_mul_absz(t, r);
        r = t;
      }
      chk_load_jac<C>(p, row, coords);
      {
        Jac<F> np = p;
        fe_neg(np.Y, p.Y);
        jac_add_full(r, np);
      }
      if (!jac_is_inf(r)) {
        // Xr Zp^2 == beta Xp Zr^2 and Yr Zp^3 == Yp Zr^3
        Fe<F> beta, zp2, zr2, zp3, zr3, a, b, c;
        ld_int(beta, cc.cx);
        fe_sqr(zp2, p.Z);
        fe_sqr(zr2, r.Z);
        fe_mul(zp3, zp2, p.Z);
        fe_mul(zr3, zr2, r.Z);
        fe_mul(a, r.X, zp2);
        fe_mul(c, p.X, beta);
        fe_mul(b, c, zr2);
        fe_sub(c, a, b);
        ok = fe_is_zero(c);
        fe_mul(a, r.Y, zp3);
        fe_mul(b, p.Y, zr3);
        fe_sub(c, a, b);
        ok = ok && fe_is_zero(c);
      }
    } else if constexpr (KIND == CHK_BLS_G2) {
      // [|z|]P == -psi(P) (z < 0), compared by cross-multiplication: Xq Zs^2 == Xs Zq^2, Yq Zs^3 == -Ys Zq^3.
      // psi(P) is finite, so an infinite [|z|]P is a rejection.
      Jac<F> q, s;
      jac_mul_u64(q, p, cc.k, slot);
      chk_load_jac<C>(p, row, coords);
      {
        Fe<F> cx, cy;
        ld_int(cx, cc.cx);
        ld_int(cy, cc.cy);
        jac_psi(s, p, cx, cy);
      }
      if (!jac_is_inf(q)) {
        Fe<F> zs2, zq2, a, b, c;
        fe_sqr(zs2, s.Z);
        fe_sqr(zq2, q.Z);
        fe_mul(a, q.X, zs2);
        fe_mul(b, s.X, zq2);
        fe_sub(c, a, b);
        ok = fe_is_zero(c);
        fe_mul(a, zs2, s.Z);
        fe_mul(b, zq2, q.Z);
        fe_mul(c, q.Y, a);
        fe_mul(a, s.Y, b);
        fe_add(b, c, a);
        ok = ok && fe_is_zero(b);
      }
    } else if constexpr (KIND == CHK_BN_G2) {
      Jac<F> t, s;
      jac_mul_u64(t, p, cc.k, slot);  // [x]P
      s = t;
      // the chain is done with its cached point: the slot now keeps [x]P, read back by every step below
      fe_store_u(slot, t.X);
      fe_store_u(slot + F::SN, t.Y);
      fe_store_u(slot + 2 * F::SN, t.Z);
      Fe<F> cx, cy;
      ld_int(cx, cc.cx);
      ld_int(cy, cc.cy);
      // s = [x]P + P + psi([x]P) + psi^2([x]P) - psi^3([2x]P): one rolled loop, one addition in its body
#pragma unroll 1
      for (int step = 0; step < 4; step++) {
        Jac<F> b;
        if (step == 0) {
          chk_load_jac<C>(b, row, coords);
        } else {
          asm volatile("" ::: "memory");
          fe_load_u(t.X, slot);
          fe_load_u(t.Y, slot + F::SN);
          fe_load_u(t.Z, slot + 2 * F::SN);
        }
        if (step == 1 || step == 2) {
          jac_psi(b, t, cx, cy);
          if (step == 2) jac_psi(b, b, cx, cy);
        } else if (step == 3) {
          b = t;
          jac_dbl(b);
          for (int k = 0; k < 3; k++) jac_psi(b, b, cx, cy);
          Fe<F> ny;
          fe_neg(ny, b.Y);
          b.Y = ny;
        }
        jac_add_full(s, b);
      }
      ok = jac_is_inf(s);
    }
    if (ok) flags[i] = f | PT_IN_SUBGROUP;
  }
}

template <int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_check_count(int n, const uint8_t *__restrict__ flags,
                                                       uint32_t *__restrict__ count) {
  constexpr uint8_t ALL = PT_CANONICAL | PT_ON_CURVE | PT_IN_SUBGROUP;
  uint32_t c = 0;
  for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * BLOCK)
    c += (flags[i] & ALL) != ALL ? 1u : 0u;
  for (int off = 32; off; off >>= 1) c += (uint32_t)__shfl_down((int)c, off);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

// ---------------------------------------------------------------------------- host side

struct CheckHooks {
  std::atomic<int> mode{CHECK_MODE_DEFAULT}, max_lanes{0};
};
CheckHooks &check_hooks();  // zk_check.hip
// lanes of the membership kernel: every lane owns a slot of 5 field elements in the call's scratch (80 MiB at
// most, BLS12-381 G2), and 2^17 lanes are 2 wavefronts per SIMD of the 256 CUs -- more than the one a lane's
// 350 to 512 registers let a SIMD hold
constexpr size_t CHECK_MAX_LANES_DEFAULT = (size_t)1 << 17;
inline size_t check_lanes(size_t n) {
  const int ml = check_hooks().max_lanes.load();
  const size_t cap = ml > 0 ? (size_t)ml : CHECK_MAX_LANES_DEFAULT;
  return (std::min(n, cap) + 255) & ~(size_t)255;
}

// dst = src << sh as 256-bit integers, 0 < sh < 256
inline void chk_shl256(uint64_t *dst, const uint64_t *src, int sh) {
  const int w = sh >> 6, o = sh & 63;
  for (int i = 3; i >= 0; i--) {
    uint64_t v = i - w >= 0 ? src[i - w] << o : 0;
    if (o && i - w - 1 >= 0) v |= src[i - w - 1] >> (64 - o);
    dst[i] = v;
  }
}

template <class C>
inline ChkConsts<C> chk_consts() {
  ChkConsts<C> c = {};
  auto cp = [](uint64_t *d, const uint64_t *s, int n) { memcpy(d, s, (size_t)n * 8); };
  auto naf = [&](const uint64_t *pos, const uint64_t *neg, int top) {
    chk_shl256(c.naf.pos, pos, 256 - top);
    chk_shl256(c.naf.neg, neg, 256 - top);
    c.naf_count = top;
  };
  constexpr int NP = C::NP64, NB = ChkConsts<C>::NB;
  if constexpr (NB == 4) {
    cp(c.p, CHK_BN254_P, NB);
    naf(CHK_BN254_R_NAF_POS, CHK_BN254_R_NAF_NEG, CHK_BN254_R_NAF_TOP);
    c.k = CHK_BN254_X;
    if constexpr (NP == NB) {
      cp(c.b, CHK_BN254_B_REF, NP);
    } else {
      cp(c.b, CHK_BN254_G2_B_REF, NP);
      cp(c.cx, CHK_BN254_PSI_X_REF, NP);
      cp(c.cy, CHK_BN254_PSI_Y_REF, NP);
    }
  } else {
    cp(c.p, CHK_BLS381_P, NB);
    naf(CHK_BLS381_R_NAF_POS, CHK_BLS381_R_NAF_NEG, CHK_BLS381_R_NAF_TOP);
    c.k = CHK_BLS381_ABSZ;
    if constexpr (NP == NB) {
      cp(c.b, CHK_BLS381_B_REF, NP);
      cp(c.cx, CHK_BLS381_BETA_REF, NP);
    } else {
      cp(c.b, CHK_BLS381_G2_B_REF, NP);
      cp(c.cx, CHK_BLS381_PSI_X_REF, NP);
      cp(c.cy, CHK_BLS381_PSI_Y_REF, NP);
    }
  }
  return c;
}

template <class C, bool G2>
int check_rows_t(Device &dev, int n, const uint64_t *pts, int coords, uint8_t *flags, bool host_io) {
  using F = typename C::Fp;
  constexpr int NP = C::NP64;
  const size_t N = (size_t)n, in_words = N * (coords == COORDS_AFFINE ? 2 : 3) * NP;
  hipStream_t st = dev.stream;
  const int mode = check_hooks().mode.load();
  const size_t lanes = check_lanes(N);
  dev.arena.reserve((host_io ? in_words * 8 : 0) + N + lanes * member_slot_words<F>() * 4 + (1 << 20));
  dev.arena.reset();
  const uint64_t *d_pts = pts;
  if (host_io) {
    uint64_t *a = dev.arena.take<uint64_t>(in_words);
    ZK_CHECK(hipMemcpyAsync(a, pts, in_words * 8, hipMemcpyHostToDevice, st));
    d_pts = a;
  }
  uint8_t *d_flags = (host_io || !flags) ? dev.arena.take<uint8_t>(N) : flags;
  uint32_t *d_count = dev.arena.take<uint32_t>(1);
  ZK_CHECK(hipMemsetAsync(d_count, 0, 4, st));
  const ChkConsts<C> cc = chk_consts<C>();
  constexpr int DK = chk_default_kind<C>();
  const int member_free = mode == CHECK_MODE_DEFAULT && DK == CHK_NONE ? 1 : 0;
  const dim3 grid(div_up(N, 256)), block(256);
  if (coords == COORDS_AFFINE)
    hipLaunchKernelGGL((k_check_curve<C, COORDS_AFFINE>), grid, block, 0, st, n, d_pts, cc, member_free, d_flags);
  else if (coords == COORDS_PROJ)
    hipLaunchKernelGGL((k_check_curve<C, COORDS_PROJ>), grid, block, 0, st, n, d_pts, cc, member_free, d_flags);
  else if constexpr (!G2)
    hipLaunchKernelGGL((k_check_curve<C, COORDS_JAC>), grid, block, 0, st, n, d_pts, cc, member_free, d_flags);
  ZK_CHECK(hipGetLastError());
  if (mode != CHECK_MODE_CURVE_ONLY && !member_free) {
    uint32_t *scratch = dev.arena.take<uint32_t>(lanes * member_slot_words<F>());
    const dim3 mgrid((unsigned)(lanes / 256));
    if (mode == CHECK_MODE_EXACT)
      hipLaunchKernelGGL((k_check_member<C, CHK_EXACT>), mgrid, block, 0, st, n, d_pts, coords, cc, d_flags, (int)lanes,
                         scratch);
    else if constexpr (DK != CHK_NONE)
      hipLaunchKernelGGL((k_check_member<C, DK>), mgrid, block, 0, st, n, d_pts, coords, cc, d_flags, (int)lanes,
                         scratch);
    ZK_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL((k_check_count<256>), dim3(std::min(div_up(N, 256), 1024u)), block, 0, st, n, d_flags, d_count);
  ZK_CHECK(hipGetLastError());
  if (host_io && flags) copy_to_host(dev, st, flags, d_flags, N);
  return (int)*read_back(dev, d_count);
}

}  // namespace zk
