// zk_poly.hip -- polynomial product, evaluation and linear combination over Fr on gfx950.
//
// Replaces the reference's generated polynomial code between a prover's NTTs:
//   <C>_poly_mont_mul_naive   lib/cbits/curves/poly/mont/bls12_381_poly_mont.c:199-222
//       (what Haskell's (*) and sqr on Poly bind to: Poly.hs:133 "mul = mulNaive")
//   <C>_poly_mont_eval_at     bls12_381_poly_mont.c:225-243   (serial Horner loop)
//   <C>_poly_mont_lincomb     bls12_381_poly_mont.c:169-195
//   <C>_poly_mont_long_div / _quot / _rem   bls12_381_poly_mont.c:249-309   (as zkg_poly_long_div:
//       Newton inversion of the reversed divisor over the NTT, "division" below)
// Every coefficient of every result is an exact canonical field element, so the output is
// bit-identical to the reference's loops whatever algorithm computes it.
//
// Product: a short factor (a linear factor x - z, a blinding polynomial) runs on the direct
// kernel, one lane per output coefficient; everything else is zero-pad, forward transforms,
// pointwise product, inverse transform on the NTT of zk_ntt.hip.  The crossover is measured
// (profiles/r08a_poly_crossover.txt, POLY_MUL_DIRECT_MAX below).
//
// Lazy accumulation (k_poly_mul_direct, k_poly_lincomb): the 17 product-scanning column sums of
// up to LAZY_J = 6 products x_i * s_i are added up in 64-bit accumulators and share ONE Montgomery
// reduction.  Bound, 9 x 29-bit limbs (both Fr fields), x_i canonical (< p), s_i < 2p with
// normalised limbs: a column holds at most 9 limb products of each x_i * s_i and 9 of the
// reduction's m * p, each < (2^29 - 1)^2, plus a carry < 2^35:
//     (6 + 1) * 9 * (2^29 - 1)^2 + 2^35 < 2^64,
// and the reduced value is < (6 * p * 2p + R' p) / R' = p (1 + 12 p / R') <= 1.19 p < 2p since
// R' / p >= 2^261 / 2^255 = 64.  tools/poly_bounds.py replays the reduction on the all-(r - 1)
// operand with Python integers; tests/test_poly_cpu.py runs it.
//
// Shared with zk_arr.hip: the row helpers, block_sum and k_dot_final (zk_frdev.hpp),
// CfgBN / CfgBLS, with_fr, ceil_log2 and PowSplit (zk_frcfg.hpp), Stage and read_back (zk_runtime.hpp).
#include "zk_frdev.hpp"
#include "zk_frcfg.hpp"
#include "zk_arr.hpp"
#include "zk_ntt.hpp"
#include "zk_poly.hpp"
#include "../../include/zkalgebra_gpu.h"

namespace zk {

namespace {

constexpr int LAZY_J = 6;  // products per reduction (the bound in the header comment)
// T += the product-scanning columns of a * b
template <class F>
__device__ __forceinline__ void cols_add(uint64_t (&T)[2 * F::N - 1], const Fe<F> &a, const Fe<F> &b) {
  static_assert(F::N == 9 && F::RB == 29, "the accumulation bound is stated for the 9 x 29-bit fields");
#pragma unroll
  for (int i = 0; i < F::N; i++)
#pragma unroll
    for (int j = 0; j < F::N; j++) T[i + j] += (uint64_t)a.v[i] * b.v[j];
}

// ---------------------------------------------------------------------------- direct product

// tgt[k] = sum_j s[j] l[k - j]: one lane per output coefficient k < nl + ns - 1, looping over the
// SHORTER factor s; consecutive lanes read consecutive rows of the longer factor l (coalesced
// 32-B rows, re-read from cache by the neighbouring j).  The short factor sits in LDS in tiles of
// PM_TILE rows, converted once to the internal radix: (s R')(l R) / R' = s l R, reference form.
constexpr int PM_TILE = 256;
template <class F>
__global__ void __launch_bounds__(256) k_poly_mul_direct(int nl, const uint64_t *__restrict__ l, int ns,
                                                         const uint64_t *__restrict__ s, uint64_t *__restrict__ tgt) {
  __shared__ uint32_t sh[PM_TILE * F::N];
  const long long N = (long long)nl + ns - 1;
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  Fe<F> acc;
  fe_zero(acc);
  for (int j0 = 0; j0 < ns; j0 += PM_TILE) {
    const int cnt = min(PM_TILE, ns - j0);
    __syncthreads();  // the previous tile has been read
    if ((int)threadIdx.x < cnt) {
      Fe<F> v, vi;
      ld(v, s, (size_t)(j0 + threadIdx.x));
      fe_to_int(vi, v);
      lds_put(sh + threadIdx.x * F::N, vi);
    }
    __syncthreads();
    for (int jj = 0; jj < cnt; jj += LAZY_J) {  // block-uniform trip counts
      const int mq = min(LAZY_J, cnt - jj);
      uint64_t T[2 * F::N - 1];
#pragma unroll
      for (int q = 0; q < 2 * F::N - 1; q++) T[q] = 0;
#pragma unroll
      for (int u = 0; u < LAZY_J; u++) {
        if (u < mq) {
          const long long i = k - (j0 + jj + u);
          const bool in = k < N && i >= 0 && i < nl;
          Fe<F> x, c;
          ld(x, l, (size_t)(in ? i : 0));  // row 0 exists (nl >= 1); its product is masked out
          if (!in) fe_zero(x);
          lds_get(c, sh + (jj + u) * F::N);
          cols_add(T, x, c);
        }
      }
      Fe<F> r, t;
      redc_cols(r, T);
      fe_add(t, acc, r);
      acc = t;
    }
  }
  if (k < N) st(tgt, (size_t)k, acc);
}

// ---------------------------------------------------------------------------- transform product

// Both operands into their zero-padded transform buffers in ONE launch, 16 B per lane: x[0, n1) =
// a, x[n1, N) = 0, and the same for (b, n2, y).  A null source leaves the head alone (the rows
// were copied from the host already); a null y skips the second operand (squaring).
__global__ void __launch_bounds__(256) k_poly_pad2(size_t N, size_t n1, const uint64_t *__restrict__ a,
                                                   uint64_t *__restrict__ x, size_t n2,
                                                   const uint64_t *__restrict__ b, uint64_t *__restrict__ y) {
  const size_t per = N * 2;  // 16-B chunks per buffer
  const size_t total = y ? 2 * per : per;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const uint4 z = make_uint4(0, 0, 0, 0);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const bool second = i >= per;
    const size_t c = second ? i - per : i;
    const size_t nsrc = (second ? n2 : n1) * 2;
    const uint4 *src = reinterpret_cast<const uint4 *>(second ? b : a);
    uint4 *dst = reinterpret_cast<uint4 *>(second ? y : x);
    if (c >= nsrc) dst[c] = z;
    else if (src) dst[c] = src[c];
  }
}

// ---------------------------------------------------------------------------- evaluation

// x^e (internal form) by square and multiply, e < 2^31
template <class F>
__device__ __forceinline__ void fe_pow_u32(Fe<F> &r, const Fe<F> &x, uint32_t e) {
  Fe<F> acc, base = x, t;
  fe_one(acc);
  for (; e; e >>= 1) {
    if (e & 1) { fe_mul(t, acc, base); acc = t; }
    fe_sqr(t, base);
    base = t;
  }
  r = acc;
}
// tlo[i] = x^i (i < nlo = 2^h), thi[j] = x^(j 2^h) (j < nhi), ypow = x^T: internal form, the
// two-level table of k_pow_tables
template <class F>
__global__ void k_poly_eval_tables(int h, int nlo, int nhi, uint32_t T, U256 xr, uint64_t *__restrict__ tlo,
                                   uint64_t *__restrict__ thi, uint64_t *__restrict__ ypow) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  Fe<F> xref, x, r;
  ld_const(xref, xr);
  fe_to_int(x, xref);
  if (i < nlo) {
    fe_pow_u32(r, x, (uint32_t)i);
    st(tlo, i, r);
  }
  if (i < nhi) {
    fe_pow_u32(r, x, (uint32_t)i << h);
    st(thi, i, r);
  }
  if (i == 0) {
    fe_pow_u32(r, x, T);
    st(ypow, 0, r);
  }
}
// Lane t of T runs ONE Horner chain in y = x^T over its coefficients c[t], c[t + T], c[t + 2T], ...
// (a wavefront's loads are 64 consecutive rows; four rows are in flight per lane), multiplies the
// chain's value by x^t from the two-level table and the block adds its 256 terms: every
// coefficient is read once and nothing of length n is written.  part[block] is in reference form
// ((c R)(y R') / R' = c y R at every step).
template <class F>
__global__ void __launch_bounds__(256) k_poly_eval(int n, int T, int h, const uint64_t *__restrict__ c,
                                                   const uint64_t *__restrict__ tlo, const uint64_t *__restrict__ thi,
                                                   const uint64_t *__restrict__ ypow, uint64_t *__restrict__ part) {
  __shared__ uint32_t lds[256 * F::N];
  const int t = blockIdx.x * 256 + threadIdx.x;  // < T
  Fe<F> acc;
  fe_zero(acc);
  if (t < n) {
    Fe<F> y;
    ld(y, ypow, 0);
    const size_t cnt = ((size_t)n - t + T - 1) / T;  // >= 1
    size_t j = cnt;
    for (; j >= 4; j -= 4) {
      Fe<F> c0, c1, c2, c3, p;
      ld(c0, c, (size_t)t + (j - 1) * T);
      ld(c1, c, (size_t)t + (j - 2) * T);
      ld(c2, c, (size_t)t + (j - 3) * T);
      ld(c3, c, (size_t)t + (j - 4) * T);
      fe_mul(p, acc, y); fe_add(acc, p, c0);
      fe_mul(p, acc, y); fe_add(acc, p, c1);
      fe_mul(p, acc, y); fe_add(acc, p, c2);
      fe_mul(p, acc, y); fe_add(acc, p, c3);
    }
    for (; j >= 1; j--) {
      Fe<F> c0, p;
      ld(c0, c, (size_t)t + (j - 1) * T);
      fe_mul(p, acc, y);
      fe_add(acc, p, c0);
    }
    Fe<F> lo, hi, xt, term;
    ld(lo, tlo, (size_t)(t & ((1 << h) - 1)));
    ld(hi, thi, (size_t)(t >> h));
    fe_mul(xt, hi, lo);      // x^t, internal
    fe_mul(term, acc, xt);   // reference form
    acc = term;
  }
  block_sum(acc, lds);
  if (threadIdx.x == 0) st(part, blockIdx.x, acc);
}
// the partials are in reference form already: their sum is k_dot_final<F, false> (zk_frdev.hpp)

// ---------------------------------------------------------------------------- linear combination

struct LcRow {
  const uint64_t *p;
  int n;
};
// tgt[i] = sum_{k : rows[k].n > i} coef[k] rows[k].p[i], one lane per coefficient index i < N.
// The K coefficients are converted once per block into LDS (tiles of LC_TILE), as ARR_SCALE
// converts its one; the products of LAZY_J polynomials share a reduction.
constexpr int LC_TILE = 64;
template <class F>
__global__ void __launch_bounds__(256) k_poly_lincomb(int K, int N, const LcRow *__restrict__ rows,
                                                      const uint64_t *__restrict__ coef, uint64_t *__restrict__ tgt) {
  __shared__ uint32_t sc[LC_TILE * F::N];
  __shared__ LcRow sr[LC_TILE];
  const int i = blockIdx.x * 256 + threadIdx.x;
  Fe<F> acc;
  fe_zero(acc);
  for (int k0 = 0; k0 < K; k0 += LC_TILE) {
    const int cnt = min(LC_TILE, K - k0);
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
      Fe<F> v, vi;
      ld(v, coef, (size_t)(k0 + threadIdx.x));
      fe_to_int(vi, v);
      lds_put(sc + threadIdx.x * F::N, vi);
      sr[threadIdx.x] = rows[k0 + threadIdx.x];
    }
    __syncthreads();
    for (int kk = 0; kk < cnt; kk += LAZY_J) {
      const int mq = min(LAZY_J, cnt - kk);
      uint64_t T[2 * F::N - 1];
#pragma unroll
      for (int q = 0; q < 2 * F::N - 1; q++) T[q] = 0;
#pragma unroll
      for (int u = 0; u < LAZY_J; u++) {
        if (u < mq) {
          const LcRow row = sr[kk + u];
          Fe<F> x, c;
          if (i < row.n) ld(x, row.p, (size_t)i);  // i < row.n <= N
          else fe_zero(x);
          lds_get(c, sc + (kk + u) * F::N);
          cols_add(T, x, c);
        }
      }
      Fe<F> r, t;
      redc_cols(r, T);
      fe_add(t, acc, r);
      acc = t;
    }
  }
  if (i < N) st(tgt, (size_t)i, acc);
}

// ---------------------------------------------------------------------------- division

// Series inverse, base case: g = f^-1 mod x^k for k <= DIV_BASE_CAP, where f_j = d[dq - j] for
// j < kf and 0 above (f = rev(d), f_0 the divisor's leading coefficient, nonzero).  One wavefront:
//   g_0 = f_0^-1,   g_i = -g_0 sum_{j = 1..i} f_j g_{i-j}.
// f (converted once to the internal radix, < 2p) and g (reference form, canonical) sit in LDS; lane
// t takes the LAZY_J products j = 1 + LAZY_J t ... of term i under one reduction (the bound of
// k_poly_mul_direct: x = g canonical, s = f < 2p), the lanes' sums are added across the wavefront,
// and lane 0 closes the term: (g_0 R')(S R) / R' = g_0 S R.
constexpr int DIV_BASE_CAP = 256;
static_assert(64 * LAZY_J >= DIV_BASE_CAP, "one wavefront covers every j of the last term");
template <class F>
__global__ void __launch_bounds__(64) k_div_inv_base(int k, int kf, int dq, const uint64_t *__restrict__ d,
                                                     uint64_t *__restrict__ g) {
  __shared__ uint32_t sf[DIV_BASE_CAP * F::N];
  __shared__ uint32_t sg[DIV_BASE_CAP * F::N];
  const int lane = threadIdx.x;
  for (int j = lane; j < k; j += 64) {
    Fe<F> v, vi;
    fe_zero(vi);
    if (j < kf) {
      ld(v, d, (size_t)(dq - j));
      fe_to_int(vi, v);
    }
    lds_put(sf + j * F::N, vi);
  }
  __syncthreads();
  Fe<F> g0i;  // f_0^-1 R'
  {
    Fe<F> f0;
    lds_get(f0, sf);
    fe_inv_sg(g0i, f0);
  }
  if (lane == 0) {
    Fe<F> g0;
    fe_to_ref(g0, g0i);
    lds_put(sg, g0);
  }
  __syncthreads();
  for (int i = 1; i < k; i++) {
    uint64_t T[2 * F::N - 1];
#pragma unroll
    for (int q = 0; q < 2 * F::N - 1; q++) T[q] = 0;
    const int j0 = 1 + lane * LAZY_J;
#pragma unroll
    for (int u = 0; u < LAZY_J; u++) {
      const int j = j0 + u;
      if (j <= i) {
        Fe<F> x, c;
        lds_get(x, sg + (i - j) * F::N);
        lds_get(c, sf + j * F::N);
        cols_add(T, x, c);
      }
    }
    Fe<F> r, t;
    redc_cols(r, T);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      Fe<F> other;
#pragma unroll
      for (int q = 0; q < F::N; q++) other.v[q] = __shfl_down(r.v[q], o, 64);
      fe_add(t, r, other);
      r = t;
    }
    if (lane == 0) {
      Fe<F> gi, ng;
      fe_mul(gi, g0i, r);
      fe_neg(ng, gi);
      fe_canon(ng);
      lds_put(sg + i * F::N, ng);
    }
    __syncthreads();
  }
  for (int i = lane; i < k; i += 64) {
    Fe<F> x;
    lds_get(x, sg + i * F::N);
    st(g, (size_t)i, x);
  }
}

// Both operands of a Newton step or of the quotient's product into their zero-padded transform
// buffers in ONE launch, 16 B per lane: x[j] = a[atop - j] for j < na (the reversal: rows walked
// down from the leading coefficient), y[j] = b[j] for j < nb, zero up to N.
__global__ void __launch_bounds__(256) k_div_rev_pad2(size_t N, size_t na, const uint64_t *__restrict__ a, size_t atop,
                                                      uint64_t *__restrict__ x, size_t nb,
                                                      const uint64_t *__restrict__ b, uint64_t *__restrict__ y) {
  const size_t per = N * 2;  // 16-B chunks per buffer
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const uint4 z = make_uint4(0, 0, 0, 0);
  const uint4 *ua = reinterpret_cast<const uint4 *>(a), *ub = reinterpret_cast<const uint4 *>(b);
  uint4 *ux = reinterpret_cast<uint4 *>(x), *uy = reinterpret_cast<uint4 *>(y);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * per; i += stride) {
    if (i < per) {
      const size_t row = i >> 1;
      ux[i] = row < na ? ua[(atop - row) * 2 + (i & 1)] : z;
    } else {
      const size_t c = i - per;
      uy[c] = c < nb * 2 ? ub[c] : z;
    }
  }
}
// The second operand of a Newton step: y[j] = -w[k + j] for j < cnt (the coefficients k .. k' - 1 of
// f g, negated here so that the step's last product is the correction itself), zero up to N
template <class F>
__global__ void __launch_bounds__(256) k_div_neg_shift_pad(size_t N, const uint64_t *__restrict__ w, size_t k, size_t cnt,
                                                           uint64_t *__restrict__ y) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < N; j += stride) {
    Fe<F> v, nv;
    fe_zero(nv);
    if (j < cnt) {
      ld(v, w, k + j);
      fe_neg(nv, v);
    }
    st(y, j, nv);
  }
}
// quot[i] = w[m - 1 - i], i < m: the truncation of the reversed quotient's product to m
// coefficients, written back in natural order
__global__ void __launch_bounds__(256) k_div_rev_trunc(size_t m, const uint64_t *__restrict__ w,
                                                       uint64_t *__restrict__ quot) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const uint4 *uw = reinterpret_cast<const uint4 *>(w);
  uint4 *uq = reinterpret_cast<uint4 *>(quot);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * m; i += stride)
    uq[i] = uw[(m - 1 - (i >> 1)) * 2 + (i & 1)];
}
// The quotient on the direct kernel's terms (m <= POLY_MUL_DIRECT_MAX): rev(q) = rev(p) g mod x^m is
//   quot[i] = sum_{j = 0..m-1-i} g[j] p[dq + i + j],   i < m,
// one lane per coefficient i, g in LDS tiles in the internal radix, the accumulation of
// k_poly_mul_direct.  The largest row read is p[dq + m - 1] = p[dp].
template <class F>
__global__ void __launch_bounds__(256) k_div_quot_direct(int m, int dq, const uint64_t *__restrict__ p,
                                                         const uint64_t *__restrict__ g, uint64_t *__restrict__ quot) {
  __shared__ uint32_t sh[PM_TILE * F::N];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  Fe<F> acc;
  fe_zero(acc);
  for (int j0 = 0; j0 < m; j0 += PM_TILE) {
    const int cnt = min(PM_TILE, m - j0);
    __syncthreads();  // the previous tile has been read
    if ((int)threadIdx.x < cnt) {
      Fe<F> v, vi;
      ld(v, g, (size_t)(j0 + threadIdx.x));
      fe_to_int(vi, v);
      lds_put(sh + threadIdx.x * F::N, vi);
    }
    __syncthreads();
    for (int jj = 0; jj < cnt; jj += LAZY_J) {  // block-uniform trip counts
      const int mq = min(LAZY_J, cnt - jj);
      uint64_t T[2 * F::N - 1];
#pragma unroll
      for (int q = 0; q < 2 * F::N - 1; q++) T[q] = 0;
#pragma unroll
      for (int u = 0; u < LAZY_J; u++) {
        if (u < mq) {
          const long long j = j0 + jj + u;
          const bool in = i < m && i + j < m;
          Fe<F> x, c;
          ld(x, p, (size_t)(in ? dq + i + j : 0));  // row 0 exists; its product is masked out
          if (!in) fe_zero(x);
          lds_get(c, sh + (jj + u) * F::N);
          cols_add(T, x, c);
        }
      }
      Fe<F> r, t;
      redc_cols(r, T);
      fe_add(t, acc, r);
      acc = t;
    }
  }
  if (i < m) st(quot, (size_t)i, acc);
}
// dst[j] = sum over t of src[j + t N], j < N (rows at or above len count as zero): the image of
// src mod x^N - 1.  One lane per j; the host folds by at most DIV_FOLD_MAX terms per pass.
constexpr int DIV_FOLD_MAX = 64;
template <class F>
__global__ void __launch_bounds__(256) k_div_fold(size_t len, const uint64_t *__restrict__ src, size_t N,
                                                  uint64_t *__restrict__ dst) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= N) return;
  Fe<F> acc, x, t;
  fe_zero(acc);
  for (size_t i = j; i < len; i += N) {
    ld(x, src, i);
    fe_add(t, acc, x);
    acc = t;
  }
  st(dst, j, acc);
}
// rem[j] = a[j] - w[j], j < n: fold(p) minus the cyclic product fold(q) fold(d), truncated to deg d
template <class F>
__global__ void __launch_bounds__(256) k_div_rem(size_t n, const uint64_t *__restrict__ a, const uint64_t *__restrict__ w,
                                                 uint64_t *__restrict__ rem) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
    Fe<F> x, y, r;
    ld(x, a, j);
    ld(y, w, j);
    fe_sub(r, x, y);
    st(rem, j, r);
  }
}

// ---------------------------------------------------------------------------- host side

U256 load_u256(const uint64_t *p) {
  U256 u;
  for (int j = 0; j < 4; j++) u.w[j] = p[j];
  return u;
}
// The transforms of one length 2^lg on device buffers, enqueued on dev.stream: the generator (the
// table of zkg_fft_generator, fetched once; an inverse transform inverts it itself) and the NTT's
// scratch of 2^lg rows
struct Xform {
  Device &dev;
  int curve, lg;
  uint64_t *scratch;
  uint64_t gen[4];
  Xform(Device &d, int c, int l, uint64_t *scr) : dev(d), curve(c), lg(l), scratch(scr) {
    zkg_fft_generator(curve, lg, gen);
  }
  void fwd(const uint64_t *src, uint64_t *dst) const { ntt_enqueue(dev, curve, lg, gen, src, dst, scratch, false); }
  void inv(const uint64_t *src, uint64_t *dst) const { ntt_enqueue(dev, curve, lg, gen, src, dst, scratch, true); }
  void mul(const uint64_t *a, const uint64_t *b, uint64_t *dst) const {  // pointwise, 2^lg rows
    arr_mul_enqueue(dev, curve, (size_t)1 << lg, a, b, dst);
  }
};

// Shorter factor <= this: the direct kernel.  Measured (profiles/r08a_poly_crossover.txt, short
// length 1, 2, 4, ... 256 against 2^12, 2^16 and 2^20 long coefficients): the direct kernel wins up
// to 128 at all three long sizes (2^20 x 128: 0.59 vs 0.82 ms) and loses at 256 at all three.
constexpr int POLY_MUL_DIRECT_MAX = 128;
// the transform path never runs below 2^4 points: smaller products reach it only through the
// test hook, and 2^4 is the smallest size the NTT's own suite covers
constexpr int POLY_MUL_MIN_LOG = 4;
std::atomic<int> g_direct_max{-1};
std::atomic<int> g_last_path{0};

template <class Cfg>
int poly_mul_t(Device &dev, int curve, int n1, const uint64_t *a, int n2, const uint64_t *b, uint64_t *tgt,
               bool host_io) {
  using F = typename Cfg::Fd;
  hipStream_t s = dev.stream;
  const long long NN = (long long)n1 + n2 - 1;
  if (NN <= 0) return 0;  // the reference's loop does not run
  if (NN > ((long long)1 << POLY_MUL_MAX_LOG[curve])) return -1;
  const size_t N = (size_t)NN;
  if (n1 <= 0 || n2 <= 0) {  // one factor empty: every sum is empty (poly_mont.c:209-219)
    if (host_io) memset(tgt, 0, N * 32);
    else ZK_CHECK(hipMemsetAsync(tgt, 0, N * 32, s));
    ZK_CHECK(hipStreamSynchronize(s));
    return 0;
  }
  const bool same = a == b && n1 == n2;
  const int dm = g_direct_max.load();
  const int direct_max = dm < 0 ? POLY_MUL_DIRECT_MAX : dm;
  const bool swap = n2 > n1;  // l: the longer factor
  const int nl = swap ? n2 : n1, ns = swap ? n1 : n2;
  Stage sg(dev, host_io);
  if (ns <= direct_max) {
    dev.arena.reserve((host_io ? ((size_t)n1 + n2 + N) * 32 : 0) + (1 << 20));
    dev.arena.reset();
    const uint64_t *da = sg.in(a, (size_t)n1), *db = same ? da : sg.in(b, (size_t)n2);  // squaring: one upload
    uint64_t *dt = sg.out(tgt, N);
    hipLaunchKernelGGL(k_poly_mul_direct<F>, dim3(div_up(N, 256)), dim3(256), 0, s, nl, swap ? db : da, ns,
                       swap ? da : db, dt);
    ZK_CHECK(hipGetLastError());
    sg.back(tgt, dt, N);
    ZK_CHECK(hipStreamSynchronize(s));
    g_last_path.store(0);
    return 0;
  }
  const int m = std::max(ceil_log2(N), POLY_MUL_MIN_LOG);
  const size_t M = (size_t)1 << m;
  // workspace: x, y (operands, then spectra / product), z (spectrum / result), the NTT's scratch
  dev.arena.reserve(4 * M * 32 + (1 << 20));
  dev.arena.reset();
  uint64_t *x = dev.arena.take<uint64_t>(M * 4);
  uint64_t *y = dev.arena.take<uint64_t>(M * 4);
  uint64_t *z = dev.arena.take<uint64_t>(M * 4);
  const Xform t(dev, curve, m, dev.arena.take<uint64_t>(M * 4));
  sg.into(x, a, (size_t)n1);  // host rows go straight into the transform buffers
  if (!same) sg.into(y, b, (size_t)n2);
  {
    const size_t chunks = (same ? 1 : 2) * M * 2;
    const unsigned grid = (unsigned)std::min<size_t>((chunks + 255) / 256, 8192);
    hipLaunchKernelGGL(k_poly_pad2, dim3(grid), dim3(256), 0, s, M, (size_t)n1, host_io ? nullptr : a, x,
                       (size_t)n2, host_io ? nullptr : b, same ? nullptr : y);
    ZK_CHECK(hipGetLastError());
  }
  t.fwd(x, z);  // z = NTT(a)
  if (same) {
    t.mul(z, z, y);  // y = z^2
  } else {
    t.fwd(y, x);     // x = NTT(b)
    t.mul(z, x, y);  // y = z x
  }
  t.inv(y, z);  // z = a b, zero above N
  if (host_io) sg.back(tgt, z, N);
  else ZK_CHECK(hipMemcpyAsync(tgt, z, N * 32, hipMemcpyDeviceToDevice, s));  // the truncating copy
  ZK_CHECK(hipStreamSynchronize(s));
  g_last_path.store(m);
  return 0;
}

template <class Cfg>
void poly_eval_t(Device &dev, int n, const uint64_t *poly, const uint64_t *x, uint64_t *tgt_host, bool host_io) {
  using F = typename Cfg::Fd;
  hipStream_t s = dev.stream;
  if (n <= 0) {  // poly_mont.c:227: the empty sum
    memset(tgt_host, 0, 32);
    return;
  }
  const size_t N = (size_t)n;
  // lanes: one chain of ~8 coefficients each, in whole blocks, at most 2^18 (four wavefronts per
  // SIMD); a short input gets one block, not a grid of empty chains
  size_t T = ((N + 7) / 8 + 255) & ~(size_t)255;
  if (T > ((size_t)1 << 18)) T = (size_t)1 << 18;
  const PowSplit ps(T);
  const int blocks = (int)(T / 256);
  dev.arena.reserve((host_io ? N * 32 : 0) + ((size_t)ps.nlo + ps.nhi + blocks + 2) * 256 + (1 << 20));
  dev.arena.reset();
  const uint64_t *dp = Stage(dev, host_io).in(poly, N);
  uint64_t *tlo = dev.arena.take<uint64_t>((size_t)ps.nlo * 4);
  uint64_t *thi = dev.arena.take<uint64_t>((size_t)ps.nhi * 4);
  uint64_t *ypow = dev.arena.take<uint64_t>(4);
  uint64_t *part = dev.arena.take<uint64_t>((size_t)blocks * 4);
  uint64_t *out = dev.arena.take<uint64_t>(4);
  hipLaunchKernelGGL(k_poly_eval_tables<F>, dim3(div_up(std::max(ps.nlo, ps.nhi), 256)), dim3(256), 0, s, ps.h, ps.nlo,
                     ps.nhi, (uint32_t)T, load_u256(x), tlo, thi, ypow);
  ZK_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_poly_eval<F>, dim3(blocks), dim3(256), 0, s, n, (int)T, ps.h, dp, tlo, thi, ypow, part);
  ZK_CHECK(hipGetLastError());
  hipLaunchKernelGGL((k_dot_final<F, false>), dim3(1), dim3(DOT_THREADS), 0, s, blocks, part, out);
  ZK_CHECK(hipGetLastError());
  memcpy(tgt_host, read_back(dev, out, 4), 32);
}

template <class Cfg>
void poly_lincomb_t(Device &dev, int K, const int *ns, const uint64_t *coeffs, const uint64_t *const *polys,
                    uint64_t *tgt, bool host_io) {
  using F = typename Cfg::Fd;
  hipStream_t s = dev.stream;
  size_t N = 0, total = 0;
  for (int k = 0; k < K; k++) {
    const size_t nk = ns[k] > 0 ? (size_t)ns[k] : 0;
    N = std::max(N, nk);
    total += nk;
  }
  if (K <= 0 || N == 0) return;  // no rows exist
  const size_t tab = (size_t)K * (sizeof(LcRow) + 32);
  dev.arena.reserve((host_io ? (total + N) * 32 + (size_t)K * 256 : 0) + tab + (1 << 20));
  dev.arena.reset();
  // the coefficients, then the pointer / length table: one pinned block, one copy
  char *hst = reinterpret_cast<char *>(dev.host_staging(tab));
  LcRow *hrows = reinterpret_cast<LcRow *>(hst + (size_t)K * 32);
  memcpy(hst, coeffs, (size_t)K * 32);
  Stage sg(dev, host_io);
  for (int k = 0; k < K; k++) {
    const size_t nk = ns[k] > 0 ? (size_t)ns[k] : 0;
    hrows[k].n = (int)nk;
    hrows[k].p = nk ? sg.in(polys[k], nk) : polys[k];
  }
  uint64_t *dt = sg.out(tgt, N);
  char *dtab = dev.arena.take<char>(tab);
  ZK_CHECK(hipMemcpyAsync(dtab, hst, tab, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_poly_lincomb<F>, dim3(div_up(N, 256)), dim3(256), 0, s, K, (int)N,
                     reinterpret_cast<const LcRow *>(dtab + (size_t)K * 32),
                     reinterpret_cast<const uint64_t *>(dtab), dt);
  ZK_CHECK(hipGetLastError());
  sg.back(tgt, dt, N);
  ZK_CHECK(hipStreamSynchronize(s));
}

// ---------------------------------------------------------------------------- division, host side
//
// p = q d + r with deg r < deg d, by Newton inversion of the reversed divisor (m = dp - dq + 1):
//   g = rev(d)^-1 mod x^m,   rev(q) = rev(p) g mod x^m,   r = p - q d mod x^dq.
// Series inverse: the base kernel gives prec[0] terms, every Newton step takes k to k' <= 2k terms
// with transforms of length N = 2^ceil(log2 k') only: the cyclic product c = f_{<k'} g_{<k} mod
// x^N - 1 wraps k + k' - 1 - N <= k coefficients onto places whose true value is known (f g = 1 mod
// x^k), so c[k, k') are the coefficients h of f g there, and g[k, k') = -(g_{<k} h) mod x^(k'-k),
// a product of k' - 1 <= N coefficients that does not wrap.  Five transforms of length N a step.
// Quotient: one product of 2m - 1 coefficients (three transforms), or the direct kernel.
// Remainder: one cyclic product of length 2^ceil(log2 dq) on the folded operands (three transforms).

// Base kernel terms by default: 16.  Measured (profiles/poly_div_base_sweep.txt: whole division at
// m = 2^8, 2^12, 2^16 against base sizes 1 .. 256, both curves): 16 is the fastest at all three
// sizes (0.540 / 1.137 / 1.940 ms on bn128), 8 and 32 within 3 % of it, 256 up to twice as slow --
// a base term costs one serial pass through the wavefront, a Newton step about a dozen launches.
constexpr int DIV_BASE_DEFAULT = 16;
std::atomic<int> g_div_base{-1};
std::atomic<int> g_last_div_steps{-1};
std::atomic<int> g_div_profile{0};
std::mutex g_div_phase_mu;
double g_div_phase_ms[3] = {0, 0, 0};

int div_base_in_force() {
  const int v = g_div_base.load();
  if (v < 0) return DIV_BASE_DEFAULT;
  return v <= 1 ? 1 : std::min(v, DIV_BASE_CAP);
}
// precisions of the series inverse: prec[0] from the base kernel, prec[i] after step i; s is the
// smallest count with base 2^s >= m and prec[i] = ceil(m / 2^(s - i)), so every step at most
// doubles and the last one ends at exactly m
int div_plan(int m, int base, int *prec, int cap) {
  if (m <= 0) return -1;
  int s = 0;
  while (((long long)base << s) < m) s++;
  for (int i = 0; i <= s && i < cap; i++) prec[i] = (int)(((long long)m + ((1ll << (s - i)) - 1)) >> (s - i));
  return s;
}
int host_degree(int n, const uint64_t *a) {
  for (long long i = (long long)n - 1; i >= 0; i--)
    if (a[4 * i] | a[4 * i + 1] | a[4 * i + 2] | a[4 * i + 3]) return (int)i;
  return -1;
}
unsigned copy_grid(size_t items) { return (unsigned)std::min<size_t>((items + 255) / 256, 8192); }

struct DivBufs {
  uint64_t *x, *y, *fx, *fg, *z, *scratch;
};
// fx = NTT(x), fg = NTT(y), x = the cyclic product of t's length of what x and y held
void div_cyclic_product(const Xform &t, const DivBufs &b) {
  t.fwd(b.x, b.fx);
  t.fwd(b.y, b.fg);
  t.mul(b.fx, b.fg, b.z);
  t.inv(b.z, b.x);
}
// rows of the first fold pass of a source of len rows down to N (0: one pass is enough)
size_t fold_first(size_t len, size_t N) {
  if (len <= (size_t)DIV_FOLD_MAX * N) return 0;
  return ((size_t)1 << ceil_log2(len)) / DIV_FOLD_MAX;  // a power of two above N
}
// dst[0, N) = src[0, len) mod x^N - 1, through t0 / t1 when one lane would add more than DIV_FOLD_MAX rows
template <class F>
void div_fold(hipStream_t s, const uint64_t *src, size_t len, size_t N, uint64_t *dst, uint64_t *t0, uint64_t *t1) {
  for (size_t Np = fold_first(len, N); Np; Np = fold_first(len, N)) {
    hipLaunchKernelGGL(k_div_fold<F>, dim3(div_up(Np, 256)), dim3(256), 0, s, len, src, Np, t0);
    ZK_CHECK(hipGetLastError());
    src = t0;
    len = Np;
    std::swap(t0, t1);
  }
  hipLaunchKernelGGL(k_div_fold<F>, dim3(div_up(N, 256)), dim3(256), 0, s, len, src, N, dst);
  ZK_CHECK(hipGetLastError());
}

template <class Cfg>
int poly_div_t(Device &dev, int curve, int n1, const uint64_t *p, int n2, const uint64_t *d, int nquot, uint64_t *quot,
               int nrem, uint64_t *rem, bool host_io) {
  using F = typename Cfg::Fd;
  hipStream_t s = dev.stream;
  g_last_div_steps.store(-1);
  // degrees: the device reduction for device operands (one wait for both); host operands are read
  // from the top where they lie, so that only the rows up to the degree are staged, once
  int dp, dq;
  if (host_io) {
    dp = host_degree(n1, p);
    dq = host_degree(n2, d);
  } else {
    dev.arena.reserve(1 << 20);
    dev.arena.reset();
    int *ddeg = dev.arena.take<int>(2);
    poly_degree_enqueue(dev, n1, p, ddeg);
    poly_degree_enqueue(dev, n2, d, ddeg + 1);
    const int *hdeg = read_back(dev, ddeg, 2);
    dp = hdeg[0];
    dq = hdeg[1];
  }
  // what the reference asserts (poly_mont.c:252-253, 267)
  if (quot && (long long)nquot < (long long)dp - dq + 1) return -1;
  if (rem && dq >= 0 && nrem < (dp < dq ? dp + 1 : dq)) return -1;
  auto zero_rows = [&](uint64_t *t, size_t from, size_t to) {
    if (!t || to <= from) return;
    if (host_io) memset(t + from * 4, 0, (to - from) * 32);
    else ZK_CHECK(hipMemsetAsync(t + from * 4, 0, (to - from) * 32, s));
  };
  if (dq < 0 || dp < dq) {  // division by zero: all zero; dp < dq: quotient 0, remainder p (poly_mont.c:255-271)
    zero_rows(quot, 0, (size_t)nquot);
    const size_t keep = dq < 0 ? 0 : (size_t)(dp + 1);
    if (rem && keep) {
      if (host_io) memcpy(rem, p, keep * 32);
      else ZK_CHECK(hipMemcpyAsync(rem, p, keep * 32, hipMemcpyDeviceToDevice, s));
    }
    zero_rows(rem, keep, (size_t)nrem);
    if (!host_io) ZK_CHECK(hipStreamSynchronize(s));
    return 0;
  }
  const int m = dp - dq + 1, kf = std::min(m, dq + 1);  // only kf coefficients of d reach the quotient
  int prec[40];
  const int steps = div_plan(m, div_base_in_force(), prec, 40);
  const int dm = g_direct_max.load();
  const bool direct_q = m <= (dm < 0 ? POLY_MUL_DIRECT_MAX : dm);
  const bool want_rem = rem && dq >= 1;
  const int lgq = std::max(ceil_log2((size_t)2 * m - 1), POLY_MUL_MIN_LOG);
  const int lgr = want_rem ? std::max(ceil_log2((size_t)dq), POLY_MUL_MIN_LOG) : 0;
  // working set, reserved once: six transform buffers of the largest length any phase needs, g, the
  // quotient where the caller's is not a device buffer, and the staged operands and remainder
  size_t NB = 0;
  for (int i = 1; i <= steps; i++) NB = std::max(NB, (size_t)1 << std::max(ceil_log2((size_t)prec[i]), POLY_MUL_MIN_LOG));
  if (!direct_q) NB = std::max(NB, (size_t)1 << lgq);
  if (want_rem) NB = std::max({NB, (size_t)1 << lgr, fold_first((size_t)dp + 1, (size_t)1 << lgr)});
  const bool own_q = host_io || !quot;
  const size_t M = (size_t)m;
  dev.arena.reserve((6 * NB + M + (own_q ? M : 0) +
                     (host_io ? (size_t)dp + 1 + (size_t)dq + 1 + (want_rem ? (size_t)dq : 0) : 0)) * 32 + (1 << 20));
  dev.arena.reset();
  Stage sg(dev, host_io);
  const uint64_t *dpl = sg.in(p, (size_t)dp + 1), *ddv = sg.in(d, (size_t)dq + 1);  // the rows up to each degree
  DivBufs B;
  B.x = dev.arena.take<uint64_t>(NB * 4);
  B.y = dev.arena.take<uint64_t>(NB * 4);
  B.fx = dev.arena.take<uint64_t>(NB * 4);
  B.fg = dev.arena.take<uint64_t>(NB * 4);
  B.z = dev.arena.take<uint64_t>(NB * 4);
  B.scratch = dev.arena.take<uint64_t>(NB * 4);
  uint64_t *g = dev.arena.take<uint64_t>(M * 4);
  uint64_t *dqo = own_q ? dev.arena.take<uint64_t>(M * 4) : quot;
  uint64_t *dro = want_rem ? sg.out(rem, (size_t)dq) : nullptr;

  const bool prof = g_div_profile.load() != 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  auto mark = [&](int i) {
    if (!prof) return;
    ZK_CHECK(hipEventCreate(&ev[i]));
    ZK_CHECK(hipEventRecord(ev[i], s));
  };
  mark(0);
  // ---- series inverse
  int k = prec[0];
  hipLaunchKernelGGL(k_div_inv_base<F>, dim3(1), dim3(64), 0, s, k, std::min(k, kf), dq, ddv, g);
  ZK_CHECK(hipGetLastError());
  for (int i = 1; i <= steps; i++) {
    const int kn = prec[i], lg = std::max(ceil_log2((size_t)kn), POLY_MUL_MIN_LOG);
    const size_t N = (size_t)1 << lg;
    const Xform t(dev, curve, lg, B.scratch);
    hipLaunchKernelGGL(k_div_rev_pad2, dim3(copy_grid(4 * N)), dim3(256), 0, s, N, (size_t)std::min(kn, kf), ddv,
                       (size_t)dq, B.x, (size_t)k, g, B.y);
    ZK_CHECK(hipGetLastError());
    div_cyclic_product(t, B);  // x = f_{<k'} g_{<k} mod x^N - 1, fg = NTT(g_{<k})
    hipLaunchKernelGGL(k_div_neg_shift_pad<F>, dim3(copy_grid(N)), dim3(256), 0, s, N, B.x, (size_t)k,
                       (size_t)(kn - k), B.y);
    ZK_CHECK(hipGetLastError());
    t.fwd(B.y, B.fx);
    t.mul(B.fx, B.fg, B.z);
    t.inv(B.z, B.x);  // x[0, k' - k) = g[k, k')
    ZK_CHECK(hipMemcpyAsync(g + (size_t)k * 4, B.x, (size_t)(kn - k) * 32, hipMemcpyDeviceToDevice, s));
    k = kn;
  }
  mark(1);
  // ---- quotient
  if (direct_q) {
    hipLaunchKernelGGL(k_div_quot_direct<F>, dim3(div_up(M, 256)), dim3(256), 0, s, m, dq, dpl, g, dqo);
    ZK_CHECK(hipGetLastError());
  } else {
    const size_t N = (size_t)1 << lgq;
    hipLaunchKernelGGL(k_div_rev_pad2, dim3(copy_grid(4 * N)), dim3(256), 0, s, N, M, dpl, (size_t)dp, B.x, M, g, B.y);
    ZK_CHECK(hipGetLastError());
    div_cyclic_product(Xform(dev, curve, lgq, B.scratch), B);  // 2m - 1 <= N: nothing wraps
    hipLaunchKernelGGL(k_div_rev_trunc, dim3(copy_grid(2 * M)), dim3(256), 0, s, M, B.x, dqo);
    ZK_CHECK(hipGetLastError());
  }
  mark(2);
  // ---- remainder: fold(p) - fold(q) fold(d) mod x^N - 1, N >= dq
  if (want_rem) {
    const size_t N = (size_t)1 << lgr;
    div_fold<F>(s, dpl, (size_t)dp + 1, N, B.z, B.fx, B.fg);
    div_fold<F>(s, dqo, M, N, B.x, B.fx, B.fg);
    div_fold<F>(s, ddv, (size_t)dq + 1, N, B.y, B.fx, B.fg);
    const Xform t(dev, curve, lgr, B.scratch);
    // fold(p) stays in z: the pointwise product goes back into x and the inverse transform into y
    t.fwd(B.x, B.fx);
    t.fwd(B.y, B.fg);
    t.mul(B.fx, B.fg, B.x);
    t.inv(B.x, B.y);
    hipLaunchKernelGGL(k_div_rem<F>, dim3(copy_grid((size_t)dq)), dim3(256), 0, s, (size_t)dq, B.z, B.y, dro);
    ZK_CHECK(hipGetLastError());
  }
  mark(3);
  // ---- write-out: the tails are zero (poly_mont.c:273-274)
  zero_rows(quot, M, (size_t)nquot);
  zero_rows(rem, (size_t)dq, (size_t)nrem);
  if (quot) sg.back(quot, dqo, M);
  if (want_rem) sg.back(rem, dro, (size_t)dq);
  ZK_CHECK(hipStreamSynchronize(s));
  if (prof) {
    float ms[3];
    for (int i = 0; i < 3; i++) ZK_CHECK(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
    for (int i = 0; i < 4; i++) ZK_CHECK(hipEventDestroy(ev[i]));
    std::lock_guard<std::mutex> lock(g_div_phase_mu);
    for (int i = 0; i < 3; i++) g_div_phase_ms[i] = ms[i];
  }
  g_last_div_steps.store(steps);
  return 0;
}

}  // namespace

// ---------------------------------------------------------------------------- public

int poly_mul(int curve, int n1, const uint64_t *a, int n2, const uint64_t *b, uint64_t *tgt, bool host_io) {
  ZK_REQUIRE(curve == 0 || curve == 1, "poly_mul: unknown curve");
  return with_fr(curve, [&](Device &dev, auto cfg) {
    return poly_mul_t<decltype(cfg)>(dev, curve, n1, a, n2, b, tgt, host_io);
  });
}
void poly_eval(int curve, int n, const uint64_t *poly, const uint64_t *x, uint64_t *tgt_host, bool host_io) {
  with_fr(curve, [&](Device &dev, auto cfg) { poly_eval_t<decltype(cfg)>(dev, n, poly, x, tgt_host, host_io); });
}
void poly_lincomb(int curve, int K, const int *ns, const uint64_t *coeffs, const uint64_t *const *polys,
                  uint64_t *tgt, bool host_io) {
  with_fr(curve, [&](Device &dev, auto cfg) { poly_lincomb_t<decltype(cfg)>(dev, K, ns, coeffs, polys, tgt, host_io); });
}
int poly_long_div(int curve, int n1, const uint64_t *p, int n2, const uint64_t *d, int nquot, uint64_t *quot, int nrem,
                  uint64_t *rem, bool host_io) {
  // refusals on the lengths alone, before a pointer is read or a device is opened
  g_last_div_steps.store(-1);
  if (curve != 0 && curve != 1) return -1;
  if (n1 < 0 || n2 < 0 || (quot && nquot < 0) || (rem && nrem < 0)) return -1;
  if (n1 > (1 << (POLY_MUL_MAX_LOG[curve] - 1))) return -1;
  return with_fr(curve, [&](Device &dev, auto cfg) {
    return poly_div_t<decltype(cfg)>(dev, curve, n1, p, n2, d, nquot, quot, nrem, rem, host_io);
  });
}
void poly_set_div_base_max(int len) { g_div_base.store(len < 0 ? -1 : len); }
int poly_div_base_max() { return div_base_in_force(); }
int poly_div_plan(int m, int *prec, int cap) { return div_plan(m, div_base_in_force(), prec, prec ? cap : 0); }
int poly_last_div_steps() { return g_last_div_steps.load(); }
void poly_div_profile(int on) { g_div_profile.store(on); }
void poly_last_div_phase_ms(double *ms) {
  std::lock_guard<std::mutex> lock(g_div_phase_mu);
  for (int i = 0; i < 3; i++) ms[i] = g_div_phase_ms[i];
}
void poly_set_mul_direct_max(int len) { g_direct_max.store(len < 0 ? -1 : len); }
int poly_last_mul_path() { return g_last_path.load(); }

}  // namespace zk
