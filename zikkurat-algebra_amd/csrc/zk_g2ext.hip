// zk_g2ext.hip -- G2 batch affine conversion on gfx950.
//
// Replaces <C>_G2_proj_batch_from_affine / _batch_to_affine (bls12_381_G2_proj.c:112-158; Haskell
// batchFromAffine / batchToAffine, G2/Proj.hs:386-405; msmProj = msm . batchToAffine, :223-224).
//
// batch_to_affine: the reference inverts every Z over Fp2 separately (Fp2_mont_inv per point,
// G2_proj.c:124-136).  Here 1/Z = conj(Z) / N(Z) with the norm N(Z) = z0^2 + z1^2 in the BASE field
// (u^2 = -1; p = 3 mod 4 on both curves, so N(Z) = 0 only for Z = 0), and the norms share inversions
// by Montgomery's trick exactly as the G1 conversion's denominators do (k_norm_chunks,
// zk_g1ext.hip): per lane a strided chunk of prefix products, one safegcd inversion, the walk back.
// Two kernels, because Fp2 coordinates do not fit beside the inversion (the G1 kernel already sits
// at 248-254 VGPRs on BLS12-381):
//   k_g2_norm_chain  reads only Z, leaves 1/N(Z_i) (Fp, internal form) in scratch; the chain itself
//                    (g2_norm_chain_body, zk_g2norm.hpp) is shared with the G2 transform's normalisation
//   k_g2_apply       one thread per point: X conj(Z) / N(Z), Y conj(Z) / N(Z), canonical
// Rows with Z = 0 (whatever X and Y hold) take the factor 1 in the chain and come out as the
// all-0xFF affine sentinel, like the reference.
#include "zk_curve.hpp"
#include "zk_dispatch.hpp"
#include "zk_extdev.hpp"
#include "zk_g1ext.hpp"
#include "zk_g2ext.hpp"
#include "zk_g2norm.hpp"
#include "zk_host.hpp"
#include "zk_msm.hpp"
#include "zk_runtime.hpp"

namespace zk {

// ---------------------------------------------------------------------------- batch_from_affine

template <class C>
__global__ void __launch_bounds__(256) k_g2_from_affine(int n, const uint64_t *__restrict__ src,
                                                        uint64_t *__restrict__ tgt, W6 one_ref) {
  constexpr int NP = C::NP64, NB = NP / 2;  // u64 words per Fp2 / Fp element
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n) return;
  const uint64_t *a = src + i * 2 * NP;
  uint64_t *o = tgt + i * 3 * NP;
  const bool inf = ref_all_ones<typename C::Fp>(a, 2 * NP);  // affine infinity -> (0 : 1 : 0), G2_proj.c:112-120
  for (int k = 0; k < NP; k++) o[k] = inf ? 0 : a[k];
  for (int k = 0; k < NB; k++) {
    o[NP + k] = inf ? one_ref.w[k] : a[NP + k];
    o[NP + NB + k] = inf ? 0 : a[NP + NB + k];
    o[2 * NP + k] = inf ? 0 : one_ref.w[k];  // Z = Fp2 one
    o[2 * NP + NB + k] = 0;
  }
}

// ---------------------------------------------------------------------------- batch_to_affine

// Z of row i (internal form); false = Z is zero
template <class B, int NP>
__device__ __forceinline__ bool g2_load_z(Fe<B> &z0, Fe<B> &z1, const uint64_t *__restrict__ src, size_t i) {
  ld_int(z0, src + i * 3 * NP + 2 * NP);
  ld_int(z1, src + i * 3 * NP + 2 * NP + NP / 2);
  return !(fe_is_zero(z0) && fe_is_zero(z1));
}

// the shared chain (zk_g2norm.hpp) on the projective rows' Z
template <class C>
__global__ void __launch_bounds__(256) k_g2_norm_chain(int n, int CHK, const uint64_t *__restrict__ src,
                                                       uint64_t *__restrict__ ninv, int lanes) {
  using B = typename C::Fp::Base;
  g2_norm_chain_body<C>(n, CHK, ninv, lanes,
                        [&](size_t i, Fe<B> &z0, Fe<B> &z1) { return g2_load_z<B, C::NP64>(z0, z1, src, i); });
}

template <class C>
__global__ void __launch_bounds__(256) k_g2_apply(int n, const uint64_t *__restrict__ src,
                                                  const uint64_t *__restrict__ ninv, uint64_t *__restrict__ tgt) {
  using F = typename C::Fp;
  using B = typename F::Base;
  constexpr int NP = C::NP64, NB = NP / 2;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n) return;
  Fe<B> z0, z1, ni;
  const bool fin = g2_load_z<B, NP>(z0, z1, src, i);
  Fe<F> zi, X, Y, x, y;
  fe_load_ref(ni, ninv + i * NB);
  g2_inv_from_norm(zi, z0, z1, ni);
  ld_int(X, src + i * 3 * NP);
  ld_int(Y, src + i * 3 * NP + NP);
  fe_mul(x, X, zi);
  fe_mul(y, Y, zi);
  uint32_t ones[B::NW];
#pragma unroll
  for (int l = 0; l < B::NW; l++) ones[l] = ~0u;
  Fe<B> x0, x1, y0, y1;
  f2_split(x0, x1, x);
  f2_split(y0, y1, y);
  uint64_t *o = tgt + i * 2 * NP;
  st_ref_or(o, x0, fin, ones);  // Z = 0: all-ones row, G2_proj.c:124-129
  st_ref_or(o + NB, x1, fin, ones);
  st_ref_or(o + NP, y0, fin, ones);
  st_ref_or(o + NP + NB, y1, fin, ones);
}

// ---------------------------------------------------------------------------- host drivers

template <class HB>
static W6 one_ref_base() {
  W6 o = {{0, 0, 0, 0, 0, 0}};
  for (int j = 0; j < HB::N; j++) o.w[j] = HB::ONE[j];
  return o;
}

template <class C>
static void g2_batch_from_affine_t(Device &dev, int n, const uint64_t *src, uint64_t *tgt, bool host_io) {
  using HB = typename HostOf<C>::Fp::Base;
  constexpr int NP = C::NP64;
  if (n <= 0) return;
  hipStream_t st = dev.stream;
  const size_t N = (size_t)n;
  dev.arena.reserve(N * 5 * NP * 8 + (1 << 20));
  dev.arena.reset();
  StagedIO io(dev, host_io, src, N * 2 * NP, tgt, N * 3 * NP);
  hipLaunchKernelGGL(k_g2_from_affine<C>, dim3(div_up(N, 256)), dim3(256), 0, st, n, io.in, io.out,
                     one_ref_base<HB>());
  ZK_CHECK(hipGetLastError());
  io.finish();
}

template <class C>
static void g2_batch_to_affine_t(Device &dev, int n, const uint64_t *src, uint64_t *tgt, bool host_io) {
  constexpr int NP = C::NP64, NB = NP / 2;
  if (n <= 0) return;
  hipStream_t st = dev.stream;
  const size_t N = (size_t)n;
  dev.arena.reserve(N * 6 * NP * 8 + (1 << 20));
  dev.arena.reset();
  StagedIO io(dev, host_io, src, N * 3 * NP, tgt, N * 2 * NP);
  uint64_t *ninv = dev.arena.take<uint64_t>(N * NB);
  const int chk = norm_chk(N);  // points per inversion, as the G1 conversion
  const size_t lanes = (N + chk - 1) / chk;
  hipLaunchKernelGGL(k_g2_norm_chain<C>, dim3(div_up(lanes, 256)), dim3(256), 0, st, n, chk, io.in, ninv,
                     (int)lanes);
  ZK_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_g2_apply<C>, dim3(div_up(N, 256)), dim3(256), 0, st, n, io.in, ninv, io.out);
  ZK_CHECK(hipGetLastError());
  io.finish();
}

// ---------------------------------------------------------------------------- public

void g2_batch_from_affine(int curve, int n, const uint64_t *src, uint64_t *tgt, bool host_io) {
  with_g2(curve, [&](Device &dev, auto c) { g2_batch_from_affine_t<decltype(c)>(dev, n, src, tgt, host_io); });
}
void g2_batch_to_affine(int curve, int n, const uint64_t *src, uint64_t *tgt, bool host_io) {
  with_g2(curve, [&](Device &dev, auto c) { g2_batch_to_affine_t<decltype(c)>(dev, n, src, tgt, host_io); });
}

}  // namespace zk
