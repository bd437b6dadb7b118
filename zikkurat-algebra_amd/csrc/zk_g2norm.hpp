// zk_g2norm.hpp -- shared inversion of Fp2 denominators by their norms, for the G2 batch conversion
// (zk_g2ext.hip, Z of a projective row) and the G2 transform's normalisation (zk_g2fft.hip, ZZZ of an
// XYZZ row): 1 / Z = conj(Z) / N(Z), N(Z) = z0^2 + z1^2 in the base field, the norms sharing
// inversions by Montgomery's trick.
#pragma once
#include "zk_extdev.hpp"

namespace zk {

// Lane t walks the strided chunk {t, t + T, ...} (T = lanes), CHK rows at most: prefix products of the
// norms, one safegcd inversion, the walk back.  load(i, z0, z1) gives row i's denominator (internal
// form) and returns false where it is zero; such rows take the factor 1, so every step is branch-free
// and every load and store unconditional, as in k_norm_chunks (zk_g1ext.hip).  ninv[i] holds the
// running product on the way up and 1 / N(Z_i) on return.
template <class C, class Load>
__device__ __forceinline__ void g2_norm_chain_body(int n, int CHK, uint64_t *__restrict__ ninv, int lanes,
                                                   Load load) {
  using B = typename C::Fp::Base;
  constexpr int NB = C::NP64 / 2;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t T = (size_t)lanes;
  if (t >= T || t >= (size_t)n) return;
  const size_t left = ((size_t)n - t + T - 1) / T;
  const size_t cnt = left < (size_t)CHK ? left : (size_t)CHK;
  Fe<B> P, one_int;
  fe_one(P);
  fe_one(one_int);
  auto norm = [&](size_t i, Fe<B> &f) {  // z0^2 + z1^2 (one shared reduction), or 1 where Z = 0
    Fe<B> z0, z1, nn;
    const bool fin = load(i, z0, z1);
    fe_mul2(nn, z0, z0, z1, z1);
#pragma unroll
    for (int l = 0; l < B::N; l++) f.v[l] = fin ? nn.v[l] : one_int.v[l];
  };
  for (size_t k = 0; k < cnt; k++) {
    const size_t i = t + k * T;
    Fe<B> f, q;
    norm(i, f);
    fe_mul(q, P, f);
    P = q;
    fe_store_ref(ninv + i * NB, P);  // running product (internal form, packed)
  }
  Fe<B> inv;
  fe_inv_sg(inv, P);
  for (size_t kk = cnt; kk-- > 0;) {
    const size_t i = t + kk * T;
    Fe<B> f, e, prev, dinv, q;
    norm(i, f);
    fe_load_ref(e, ninv + (kk > 0 ? i - T : i) * NB);
#pragma unroll
    for (int l = 0; l < B::N; l++) prev.v[l] = kk > 0 ? e.v[l] : one_int.v[l];
    fe_mul(dinv, inv, prev);  // 1 / N(Z_i)
    fe_mul(q, inv, f);
    inv = q;
    fe_store_ref(ninv + i * NB, dinv);
  }
}

// zi = 1 / Z = conj(Z) / N(Z) from Z's halves and the chain's ni = 1 / N(Z)
template <class F>
__device__ __forceinline__ void g2_inv_from_norm(Fe<F> &zi, const Fe<typename F::Base> &z0,
                                                 const Fe<typename F::Base> &z1, const Fe<typename F::Base> &ni) {
  Fe<typename F::Base> c0, c1, m;
  fe_mul(c0, z0, ni);
  fe_mul(m, z1, ni);
  fe_neg(c1, m);
  f2_join(zi, c0, c1);
}

// the G2 group FFT's closing normalisation on its own, enqueued on st (zk_g2fft.hip, k_g2_fft_norm_chain /
// k_g2_fft_norm_apply): n G2 XYZZ rows `src` (ZZZ = 0: infinity) -> rows (x : y : 1) / (0 : 1 : 0) of 3 NP
// words as <C>_G2_proj_normalize writes them, or with `affine` rows x || y of 2 NP words, all-0xFF at
// infinity, as _to_affine does (NP: the words of an Fp2 element); scratch: n NP / 2 words.  The twin of
// g1_norm_xyzz_enqueue (zk_fftdev.hpp); the G2 scalar multiplications (zk_scl_g2_*.hip) end with it.
void g2_norm_xyzz_enqueue(int curve, hipStream_t st, int n, const uint32_t *src, uint64_t *scratch, uint64_t *tgt,
                          bool affine);

}  // namespace zk
