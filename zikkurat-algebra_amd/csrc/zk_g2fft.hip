// zk_g2fft.hip -- the G2 group (curve) FFT on gfx950.
//
// Replaces <C>_G2_proj_fft_forward / _fft_inverse (bls12_381_G2_proj.c:670-781, bn128_G2_proj.c same
// lines; Haskell forwardFFT / inverseFFT = curveFFT / curveIFFT of the G2 instance, G2/Proj.hs).
//
// The schedule is the reference recursion's, level by level, exactly as the G1 integer stages run it
// (zk_g1ext.hip run_int): iterative radix-2 DIT forward (bit-reversed load), DIF inverse with a factor
// 1/2 per level (bit-reversed store), and every scalar multiplication by the INTEGER value of the
// canonical Fr scalar the reference uses at that position (zk_fftdev.hpp xyzz_scl; the twiddles are
// fft_int_twiddles' sequences).  Both twists have a cofactor, so only this makes the output equal the
// reference's for every on-curve input; scalars are never combined mod r.  There is no GLV stage, no
// subgroup test and no second stream.
//
// A level is two kernels, because Fp2 points do not fit beside the multiplication (an XYZZ point is
// 112 VGPRs on BLS12-381, the multiplication's accumulator, table entry and temporaries take the
// register file on their own):
//   k_g2_fft_scl   the level's scalar multiplications, in place, one per lane, grid-strided over a
//                  bounded number of lanes (each lane owns a 16-entry table in global scratch)
//   k_g2_fft_bfly  (u, v) -> (u + v, u - v), two lanes per butterfly, out of place
// forward level s: scl (v <- w_s^j v, j != 0), then bfly; inverse level s: bfly, then scl (1/2 and
// w_s^-j / 2).
//
// Normalisation (x = X / ZZ, y = Y / ZZZ as (x : y : 1), infinity (0 : 1 : 0), canonical limbs, the
// reference's normalize, G2_proj.c:70-89) inverts ZZZ over Fp2 by the norm trick of zk_g2ext.hip:
// 1 / ZZZ = conj(ZZZ) / N(ZZZ), N = z0^2 + z1^2 in the base field, the norms sharing inversions by
// Montgomery's trick (the chain and the inverse-from-norm step are zk_g2norm.hpp's, shared with that
// unit); then x = X (ZZ / ZZZ)^2, y = Y / ZZZ.  Chain and apply are separate kernels for the reason given
// in zk_g2ext.hip.  An input row with Z = 0 is the point at infinity.
#include <algorithm>
#include <atomic>
#include <cstring>
#include "zk_curve.hpp"
#include "zk_dispatch.hpp"
#include "zk_extdev.hpp"
#include "zk_fftdev.hpp"
#include "zk_g1ext.hpp"
#include "zk_g2ext.hpp"
#include "zk_g2norm.hpp"
#include "zk_host.hpp"
#include "zk_msm.hpp"
#include "zk_runtime.hpp"

namespace zk {

// ---------------------------------------------------------------------------- the reference's (0 : 0 : 0)
//
// The reference's transform is not the group's on every input, and this one reproduces it.  Its scalar
// multiplication (scl_windowed, G2_proj.c:426-454) builds the table [d P], d = 1..15, with dbl-2007-bl,
// which sends infinity (0 : y : 0) to (0 : 0 : 0); its complete addition (add-2015-rcb) returns
// (0 : 0 : 0) whenever an operand is (0 : 0 : 0); normalize writes (0 : 1 : 0) for it.  So k * infinity
// is infinity only while every 4-bit window of k is 0 or 1 (the accumulator then only ever adds table
// entry 1, infinity itself), otherwise it is (0 : 0 : 0), which absorbs every later sum: an infinite
// input, or a butterfly pair u = +-v, can turn a whole sub-transform into infinities.  A row in that
// state is kept here as an infinite XYZZ row (ZZ = 0) whose Y is 0; every other infinity has Y = 1
// (xyzz_set_inf).  Not reproduced: points of order <= 15 on the twist (no such point lies in the order-r
// subgroup), whose table would meet infinity on the way.
template <class F>
__device__ __forceinline__ bool g2_is_dead(const Xyzz<F> &a) {
  return fe_is_zero(a.ZZ) && fe_is_zero(a.Y);
}
template <class F>
__device__ __forceinline__ void g2_set_dead(Xyzz<F> &r) {
  fe_zero(r.X);
  fe_zero(r.Y);
  fe_zero(r.ZZ);
  fe_zero(r.ZZZ);
}
// every 4-bit window of the 256-bit k is 0 or 1
__device__ __forceinline__ bool g2_windows_01(const uint64_t *k) {
  return ((k[0] | k[1] | k[2] | k[3]) & 0xEEEEEEEEEEEEEEEEull) == 0;
}

// ---------------------------------------------------------------------------- stages

// The scalar multiplications of level s, in place.  Forward: lane = butterfly (blk, j), j != 0:
// A[k0 + half] <- w_s^j A[k0 + half] (w_s^j = tw[j 2^(m-s)]).  Inverse: lane = output (butterfly,
// which): which 0 -> A[k0] / 2 (tw[0] = 1/2), which 1 -> A[k0 + half] (w_s^-j / 2).
template <class C, bool INV>
__global__ void __launch_bounds__(256) k_g2_fft_scl(int m, int s, uint32_t *__restrict__ A,
                                                    const uint64_t *__restrict__ tw, uint32_t *__restrict__ scratch,
                                                    int lanes) {
  using F = typename C::Fp;
  const size_t half = (size_t)1 << (s - 1);
  const size_t nw = (size_t)1 << (INV ? m : m - 1);
  uint32_t *tab = scratch + ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * scl_tab_words<F>();
  for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < nw; w += (size_t)lanes) {
    const size_t b = INV ? w >> 1 : w;
    const bool second = INV ? (w & 1) != 0 : true;
    const size_t blk = b >> (s - 1), j = b & (half - 1);
    if (!INV && j == 0) continue;  // w^0 = 1
    const size_t pos = (blk << s) + j + (second ? half : 0);
    const uint64_t *k = tw + (second ? (j << (m - s)) : 0) * 4;
    Xyzz<F> v, t;
    xyzz_load(v, A + pos * xw<F>());
    if (xyzz_is_inf(v)) {  // k * infinity in the reference (above); k is a twiddle, never 0
      if (!g2_is_dead(v) && !g2_windows_01(k)) {
        g2_set_dead(v);
        xyzz_store(A + pos * xw<F>(), v);
      }
      continue;
    }
    xyzz_scl(t, v, k, tab);
    xyzz_store(A + pos * xw<F>(), t);
  }
}

// xyzz_add (add-2008-s, zk_curve.hpp) without its doubling: returns true, with acc untouched, where
// acc == b, and the butterfly then doubles a freshly loaded point.  With xyzz_dbl inlined inside xyzz_add
// the BLS12-381 butterfly returned a wrong x for 2P on an MI355X, although the same source gives the
// reference's words when replayed on a host; the cause in that code object is not found.
// This form is checked against the reference on both curves (tests/test_gpu_g2fft.py); it spills no less.
template <class F>
__device__ __forceinline__ bool g2_add_distinct(Xyzz<F> &acc, const Xyzz<F> &b) {
  if (xyzz_is_inf(b)) return false;
  if (xyzz_is_inf(acc)) { acc = b; return false; }
  Fe<F> U1, S1, P, R, t;
  fe_mul(U1, acc.X, b.ZZ);     // U1 = X1*ZZ2
  fe_mul(P, b.X, acc.ZZ);      // U2 = X2*ZZ1
  fe_sub(P, P, U1);            // P = U2 - U1
  fe_mul(S1, acc.Y, b.ZZZ);    // S1 = Y1*ZZZ2
  fe_mul(R, b.Y, acc.ZZZ);     // S2 = Y2*ZZZ1
  fe_sub(R, R, S1);            // R = S2 - S1
  if (fe_is_zero(P)) {
    if (fe_is_zero(R)) return true;
    xyzz_set_inf(acc);
    return false;
  }
  Fe<F> PP, PPP, Q;
  fe_sqr(PP, P);
  fe_mul(PPP, P, PP);
  fe_mul(Q, U1, PP);
  fe_sqr(t, R);
  fe_sub(t, t, PPP);
  fe_sub(t, t, Q);
  fe_sub(t, t, Q);             // X3
  fe_sub(Q, Q, t);
  fe_mul(Q, R, Q);
  fe_mul(S1, S1, PPP);
  fe_sub(acc.Y, Q, S1);
  acc.X = t;
  fe_mul(acc.ZZ, acc.ZZ, b.ZZ);
  fe_mul(acc.ZZ, acc.ZZ, PP);
  fe_mul(acc.ZZZ, acc.ZZZ, b.ZZZ);
  fe_mul(acc.ZZZ, acc.ZZZ, PPP);
  return false;
}

// level s: lane = (butterfly, which); which 0 -> B[k0] = u + v, which 1 -> B[k0 + half] = u - v
template <class C>
__global__ void __launch_bounds__(256) k_g2_fft_bfly(int m, int s, const uint32_t *__restrict__ A,
                                                     uint32_t *__restrict__ B) {
  using F = typename C::Fp;
  const size_t half = (size_t)1 << (s - 1);
  const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= ((size_t)1 << m)) return;
  const size_t b = o >> 1;
  const bool which = (o & 1) != 0;
  const size_t blk = b >> (s - 1), j = b & (half - 1);
  const size_t k0 = (blk << s) + j;
  Xyzz<F> u, v;
  xyzz_load(u, A + k0 * xw<F>());
  xyzz_load(v, A + (k0 + half) * xw<F>());
  const bool dead = g2_is_dead(u) || g2_is_dead(v);  // the reference's (0 : 0 : 0) absorbs the sum
  if (which) {
    Fe<F> ny;
    fe_neg(ny, v.Y);
    v.Y = ny;
  }
  if (g2_add_distinct(u, v)) {  // u == +-v: the sum is 2u
    xyzz_load(v, A + k0 * xw<F>());
    xyzz_dbl(u, v);
  }
  if (dead) g2_set_dead(u);
  xyzz_store(B + (k0 + (which ? half : 0)) * xw<F>(), u);
}

// ---------------------------------------------------------------------------- normalisation

// ZZZ of XYZZ row i split into its base-field halves; false = infinity
template <class F>
__device__ __forceinline__ bool g2_load_zzz(Fe<typename F::Base> &z0, Fe<typename F::Base> &z1,
                                            const uint32_t *__restrict__ A, size_t i) {
  Fe<F> z;
  fe_load_u(z, A + i * xw<F>() + 3 * F::SN);
  f2_split(z0, z1, z);
  return !(fe_is_zero(z0) && fe_is_zero(z1));
}

// the shared chain (g2_norm_chain_body, zk_g2norm.hpp) on the XYZZ rows' ZZZ: ninv[i] = 1 / N(ZZZ_i) on
// return, infinity taking the factor 1
template <class C>
__global__ void __launch_bounds__(256) k_g2_fft_norm_chain(int n, int CHK, const uint32_t *__restrict__ A,
                                                           uint64_t *__restrict__ ninv, int lanes) {
  using F = typename C::Fp;
  using B = typename F::Base;
  g2_norm_chain_body<C>(n, CHK, ninv, lanes,
                        [&](size_t i, Fe<B> &z0, Fe<B> &z1) { return g2_load_zzz<F>(z0, z1, A, i); });
}

// one thread per point: 1 / ZZZ = conj(ZZZ) / N(ZZZ), 1 / Z = ZZ / ZZZ, x = X / Z^2, y = Y / ZZZ, written
// as the normalised reference row at bitrev_m(i) when bitrev_m > 0 (the inverse's output order); AFF: the
// affine row x || y instead, all-0xFF at infinity (<C>_G2_proj_to_affine, G2_proj.c:139-151)
template <class C, bool AFF>
__global__ void __launch_bounds__(256) k_g2_fft_norm_apply(int n, int bitrev_m, const uint32_t *__restrict__ A,
                                                           const uint64_t *__restrict__ ninv,
                                                           uint64_t *__restrict__ tgt) {
  using F = typename C::Fp;
  using B = typename F::Base;
  constexpr int NP = C::NP64, NB = NP / 2;  // u64 words per Fp2 / Fp element
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n) return;
  Fe<B> z0, z1, ni;
  const bool fin = g2_load_zzz<F>(z0, z1, A, i);
  Fe<F> izzz, iz, iz2, x, y;
  fe_load_ref(ni, ninv + i * NB);
  g2_inv_from_norm(izzz, z0, z1, ni);
  Xyzz<F> p;
  xyzz_load(p, A + i * xw<F>());
  fe_mul(iz, p.ZZ, izzz);  // ZZ / ZZZ = 1 / Z
  fe_sqr(iz2, iz);
  fe_mul(x, p.X, iz2);
  fe_mul(y, p.Y, izzz);
  Fe<B> one_int, x0, x1, y0, y1;
  fe_one(one_int);
  f2_split(x0, x1, x);
  f2_split(y0, y1, y);
  uint32_t zeros[B::NW], oneref[B::NW];
  {
    Fe<B> t;
    fe_to_ref(t, one_int);
    fe_canon(t);
    fe_pack(oneref, t);
  }
#pragma unroll
  for (int l = 0; l < B::NW; l++) zeros[l] = 0;
  const size_t o = bitrev_m > 0 ? (size_t)(__builtin_bitreverse32((uint32_t)i) >> (32 - bitrev_m)) : i;
  if constexpr (AFF) {
    uint32_t ones[B::NW];
#pragma unroll
    for (int l = 0; l < B::NW; l++) ones[l] = ~0u;
    uint64_t *q = tgt + o * 2 * NP;
    st_ref_or(q, x0, fin, ones);
    st_ref_or(q + NB, x1, fin, ones);
    st_ref_or(q + NP, y0, fin, ones);
    st_ref_or(q + NP + NB, y1, fin, ones);
    return;
  }
  uint64_t *q = tgt + o * 3 * NP;
  st_ref_or(q, x0, fin, zeros);  // infinity: (0 : 1 : 0), G2_proj.c:72-76
  st_ref_or(q + NB, x1, fin, zeros);
  st_ref_or(q + NP, y0, fin, oneref);
  st_ref_or(q + NP + NB, y1, fin, zeros);
  st_ref_or(q + 2 * NP, one_int, fin, zeros);
  st_ref_or(q + 2 * NP + NB, one_int, false, zeros);
}

// ---------------------------------------------------------------------------- host side

// Largest transform: 2^24 rows.  Every kernel indexes with size_t and takes N as an int; the working
// set is N (2 x 6 NP x 8 host rows + 2 x 4 SN x 4 XYZZ + NP/2 x 8 norms + 16 twiddle) bytes plus the
// lanes' tables -- 1664 bytes per row, 28 GB, on BLS12-381 at 2^24 -- which the arena holds in one size_t sum.
constexpr int G2_FFT_MAX_LOG = 24;
// scalar-multiplication lanes of a stage: one wavefront per SIMD of the whole chip (256 CUs x 4 SIMDs x 64
// lanes); a lane's table is 10 KB on BLS12-381, 7.5 KB on BN254
constexpr size_t G2_FFT_LANES = (size_t)1 << 16;
static std::atomic<size_t> g2_fft_max_lanes{G2_FFT_LANES};

// chain and apply over the n XYZZ rows A -> tgt (ninv: n NP / 2 words of scratch)
template <class C, bool AFF>
static void g2_norm_launch(hipStream_t st, size_t N, int bitrev_m, const uint32_t *A, uint64_t *ninv, uint64_t *tgt) {
  const int chk = norm_chk(N);  // rows per shared inversion, as the batch conversions
  const size_t nlanes = (N + chk - 1) / chk;
  hipLaunchKernelGGL(k_g2_fft_norm_chain<C>, dim3(div_up(nlanes, 256)), dim3(256), 0, st, (int)N, chk, A, ninv,
                     (int)nlanes);
  ZK_CHECK(hipGetLastError());
  hipLaunchKernelGGL((k_g2_fft_norm_apply<C, AFF>), dim3(div_up(N, 256)), dim3(256), 0, st, (int)N, bitrev_m, A, ninv,
                     tgt);
  ZK_CHECK(hipGetLastError());
}

template <class C>
static void g2_fft_t(Device &dev, int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt, bool host_io,
                     bool inverse) {
  using F = typename C::Fp;
  constexpr int NP = C::NP64, NB = NP / 2;
  hipStream_t st = dev.stream;
  const size_t N = (size_t)1 << m;
  const size_t work = inverse ? N : N / 2;
  size_t lanes = std::min(work, g2_fft_max_lanes.load());
  lanes = (lanes + 255) & ~(size_t)255;
  if (lanes == 0) lanes = 256;
  const size_t tw_cnt = N > 1 ? N / 2 : 1;
  dev.arena.reserve((host_io ? 2 : 0) * N * 3 * NP * 8 + 2 * N * xw<F>() * 4 + lanes * scl_tab_words<F>() * 4 +
                    tw_cnt * 32 + N * NB * 8 + (1 << 20));
  dev.arena.reset();
  StagedIO io(dev, host_io, src, N * 3 * NP, tgt, N * 3 * NP);
  uint32_t *A = dev.arena.take<uint32_t>(N * xw<F>());
  uint32_t *Bf = dev.arena.take<uint32_t>(N * xw<F>());
  uint32_t *scratch = dev.arena.take<uint32_t>(lanes * scl_tab_words<F>());
  uint64_t *tw = dev.arena.take<uint64_t>(tw_cnt * 4);
  uint64_t *ninv = dev.arena.take<uint64_t>(N * NB);

  // input order: bit-reversed for the forward (DIT) stages, natural for the inverse (DIF)
  hipLaunchKernelGGL((k_fft_load<C, false>), dim3(div_up(N, 256)), dim3(256), 0, st, (int)N, inverse ? 0 : m, io.in,
                     A);
  ZK_CHECK(hipGetLastError());
  if (m > 0) {
    fft_int_twiddles(C::ID, st, gen, inverse, tw_cnt, tw);
    const dim3 sgrid((unsigned)(lanes / 256)), bgrid(div_up(N, 256));
    for (int k = 0; k < m; k++) {
      const int s = inverse ? m - k : k + 1;
      if (!inverse && s > 1) {
        hipLaunchKernelGGL((k_g2_fft_scl<C, false>), sgrid, dim3(256), 0, st, m, s, A, tw, scratch, (int)lanes);
        ZK_CHECK(hipGetLastError());
      }
      hipLaunchKernelGGL(k_g2_fft_bfly<C>, bgrid, dim3(256), 0, st, m, s, A, Bf);
      ZK_CHECK(hipGetLastError());
      if (inverse) {
        hipLaunchKernelGGL((k_g2_fft_scl<C, true>), sgrid, dim3(256), 0, st, m, s, Bf, tw, scratch, (int)lanes);
        ZK_CHECK(hipGetLastError());
      }
      std::swap(A, Bf);
    }
  }
  g2_norm_launch<C, false>(st, N, inverse ? m : 0, A, ninv, io.out);
  io.finish();
}

// ---------------------------------------------------------------------------- public

void g2_norm_xyzz_enqueue(int curve, hipStream_t st, int n, const uint32_t *src, uint64_t *scratch, uint64_t *tgt,
                          bool affine) {
  if (n <= 0) return;
  on_curve<BN254_G2, BLS381_G2>(curve, [&](auto c) {
    using C = decltype(c);
    if (affine) g2_norm_launch<C, true>(st, (size_t)n, 0, src, scratch, tgt);
    else g2_norm_launch<C, false>(st, (size_t)n, 0, src, scratch, tgt);
  });
}
void g2_fft(int curve, int m, const uint64_t *gen, const uint64_t *src, uint64_t *tgt, bool host_io, bool inverse) {
  ZK_REQUIRE(m >= 0 && m <= G2_FFT_MAX_LOG, "G2 fft: log2 size out of range (0..24)");
  with_g2(curve, [&](Device &dev, auto c) { g2_fft_t<decltype(c)>(dev, m, gen, src, tgt, host_io, inverse); });
}
void g2_fft_set_max_lanes(int lanes) {
  g2_fft_max_lanes.store(lanes > 0 ? (((size_t)lanes + 255) & ~(size_t)255) : G2_FFT_LANES);
}

}  // namespace zk
