// zk_poly.hip -- polynomial product, evaluation and linear combination over Fr on gfx950.
//
// Replaces the reference's generated polynomial code between a prover's NTTs:
//   <C>_poly_mont_mul_naive   lib/cbits/curves/poly/mont/bls12_381_poly_mont.c:199-222
//       (what Haskell's (*) and sqr on Poly bind to: Poly.hs:133 "mul = mulNaive")
//   <C>_poly_mont_eval_at     bls12_381_poly_mont.c:225-243   (serial Horner loop)
//   <C>_poly_mont_lincomb     bls12_381_poly_mont.c:169-195
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
#include "zk_field.hpp"
#include "zk_host.hpp"
#include "zk_runtime.hpp"
#include "zk_arr.hpp"
#include "zk_ntt.hpp"
#include "zk_poly.hpp"
#include "../../include/zkalgebra_gpu.h"

namespace zk {

namespace {

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

// Block sum of one value per thread (256 threads), the LDS tree of k_dot: thread 0 holds the sum
template <class F>
__device__ __forceinline__ void block_sum(Fe<F> &acc, uint32_t *lds) {
  lds_put(lds + threadIdx.x * F::N, acc);
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
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
template <class F>
__global__ void __launch_bounds__(256) k_poly_eval_final(int nparts, const uint64_t *__restrict__ part,
                                                         uint64_t *__restrict__ out) {
  __shared__ uint32_t lds[256 * F::N];
  Fe<F> acc;
  fe_zero(acc);
  for (int i = threadIdx.x; i < nparts; i += 256) {
    Fe<F> x, s;
    ld(x, part, i);
    fe_add(s, acc, x);
    acc = s;
  }
  block_sum(acc, lds);
  if (threadIdx.x == 0) st(out, 0, acc);
}

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

// ---------------------------------------------------------------------------- host side

struct CfgBN { using Fd = BN_Fr; using Fh = zkh::BN_Fr; };
struct CfgBLS { using Fd = BLS_Fr; using Fh = zkh::BLS_Fr; };

U256 load_u256(const uint64_t *p) {
  U256 u;
  for (int j = 0; j < 4; j++) u.w[j] = p[j];
  return u;
}
int ceil_log2(size_t n) {
  int lg = 0;
  while (((size_t)1 << lg) < n) lg++;
  return lg;
}

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
  if (ns <= direct_max) {
    dev.arena.reserve((host_io ? ((size_t)n1 + n2 + N) * 32 : 0) + (1 << 20));
    dev.arena.reset();
    const uint64_t *da = a, *db = b;
    uint64_t *dt = tgt;
    if (host_io) {
      uint64_t *xa = dev.arena.take<uint64_t>((size_t)n1 * 4);
      ZK_CHECK(hipMemcpyAsync(xa, a, (size_t)n1 * 32, hipMemcpyHostToDevice, s));
      da = db = xa;
      if (!same) {
        uint64_t *xb = dev.arena.take<uint64_t>((size_t)n2 * 4);
        ZK_CHECK(hipMemcpyAsync(xb, b, (size_t)n2 * 32, hipMemcpyHostToDevice, s));
        db = xb;
      }
      dt = dev.arena.take<uint64_t>(N * 4);
    }
    hipLaunchKernelGGL(k_poly_mul_direct<F>, dim3(div_up(N, 256)), dim3(256), 0, s, nl, swap ? db : da, ns,
                       swap ? da : db, dt);
    ZK_CHECK(hipGetLastError());
    if (host_io) copy_to_host(dev, s, tgt, dt, N * 32);
    ZK_CHECK(hipStreamSynchronize(s));
    g_last_path.store(0);
    return 0;
  }
  const int m = std::max(ceil_log2(N), POLY_MUL_MIN_LOG);
  const size_t M = (size_t)1 << m;
  uint64_t gen[4];  // the table of zkg_fft_generator; an inverse transform inverts it itself
  zkg_fft_generator(curve, m, gen);
  // workspace: x, y (operands, then spectra / product), z (spectrum / result), the NTT's scratch
  dev.arena.reserve(4 * M * 32 + (1 << 20));
  dev.arena.reset();
  uint64_t *x = dev.arena.take<uint64_t>(M * 4);
  uint64_t *y = dev.arena.take<uint64_t>(M * 4);
  uint64_t *z = dev.arena.take<uint64_t>(M * 4);
  uint64_t *scratch = dev.arena.take<uint64_t>(M * 4);
  if (host_io) {
    ZK_CHECK(hipMemcpyAsync(x, a, (size_t)n1 * 32, hipMemcpyHostToDevice, s));
    if (!same) ZK_CHECK(hipMemcpyAsync(y, b, (size_t)n2 * 32, hipMemcpyHostToDevice, s));
  }
  {
    const size_t chunks = (same ? 1 : 2) * M * 2;
    const unsigned grid = (unsigned)std::min<size_t>((chunks + 255) / 256, 8192);
    hipLaunchKernelGGL(k_poly_pad2, dim3(grid), dim3(256), 0, s, M, (size_t)n1, host_io ? nullptr : a, x,
                       (size_t)n2, host_io ? nullptr : b, same ? nullptr : y);
    ZK_CHECK(hipGetLastError());
  }
  ntt_enqueue(dev, curve, m, gen, x, z, scratch, false);  // z = NTT(a)
  if (same) {
    arr_mul_enqueue(dev, curve, M, z, z, y);  // y = z^2
  } else {
    ntt_enqueue(dev, curve, m, gen, y, x, scratch, false);  // x = NTT(b)
    arr_mul_enqueue(dev, curve, M, z, x, y);                // y = z x
  }
  ntt_enqueue(dev, curve, m, gen, y, z, scratch, true);  // z = a b, zero above N
  if (host_io) copy_to_host(dev, s, tgt, z, N * 32);
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
  const int lg = ceil_log2(T), h = (lg + 1) / 2;
  const int nlo = 1 << h, nhi = (int)((T + nlo - 1) >> h);
  const int blocks = (int)(T / 256);
  dev.arena.reserve((host_io ? N * 32 : 0) + ((size_t)nlo + nhi + blocks + 2) * 256 + (1 << 20));
  dev.arena.reset();
  const uint64_t *dp = poly;
  if (host_io) {
    uint64_t *d = dev.arena.take<uint64_t>(N * 4);
    ZK_CHECK(hipMemcpyAsync(d, poly, N * 32, hipMemcpyHostToDevice, s));
    dp = d;
  }
  uint64_t *tlo = dev.arena.take<uint64_t>((size_t)nlo * 4);
  uint64_t *thi = dev.arena.take<uint64_t>((size_t)nhi * 4);
  uint64_t *ypow = dev.arena.take<uint64_t>(4);
  uint64_t *part = dev.arena.take<uint64_t>((size_t)blocks * 4);
  uint64_t *out = dev.arena.take<uint64_t>(4);
  hipLaunchKernelGGL(k_poly_eval_tables<F>, dim3(div_up(std::max(nlo, nhi), 256)), dim3(256), 0, s, h, nlo, nhi,
                     (uint32_t)T, load_u256(x), tlo, thi, ypow);
  ZK_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_poly_eval<F>, dim3(blocks), dim3(256), 0, s, n, (int)T, h, dp, tlo, thi, ypow, part);
  ZK_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_poly_eval_final<F>, dim3(1), dim3(256), 0, s, blocks, part, out);
  ZK_CHECK(hipGetLastError());
  uint64_t *hres = reinterpret_cast<uint64_t *>(dev.host_staging(32));
  ZK_CHECK(hipMemcpyAsync(hres, out, 32, hipMemcpyDeviceToHost, s));
  ZK_CHECK(hipStreamSynchronize(s));
  memcpy(tgt_host, hres, 32);
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
  for (int k = 0; k < K; k++) {
    const size_t nk = ns[k] > 0 ? (size_t)ns[k] : 0;
    hrows[k].n = (int)nk;
    hrows[k].p = polys[k];
    if (host_io && nk) {
      uint64_t *d = dev.arena.take<uint64_t>(nk * 4);
      ZK_CHECK(hipMemcpyAsync(d, polys[k], nk * 32, hipMemcpyHostToDevice, s));
      hrows[k].p = d;
    }
  }
  uint64_t *dt = host_io ? dev.arena.take<uint64_t>(N * 4) : tgt;
  char *dtab = dev.arena.take<char>(tab);
  ZK_CHECK(hipMemcpyAsync(dtab, hst, tab, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_poly_lincomb<F>, dim3(div_up(N, 256)), dim3(256), 0, s, K, (int)N,
                     reinterpret_cast<const LcRow *>(dtab + (size_t)K * 32),
                     reinterpret_cast<const uint64_t *>(dtab), dt);
  ZK_CHECK(hipGetLastError());
  if (host_io) copy_to_host(dev, s, tgt, dt, N * 32);
  ZK_CHECK(hipStreamSynchronize(s));
}

}  // namespace

// ---------------------------------------------------------------------------- public

int poly_mul(int curve, int n1, const uint64_t *a, int n2, const uint64_t *b, uint64_t *tgt, bool host_io) {
  ZK_REQUIRE(curve == 0 || curve == 1, "poly_mul: unknown curve");
  Device &dev = current_device();
  std::lock_guard<std::mutex> lock(dev.mu);
  return curve == 0 ? poly_mul_t<CfgBN>(dev, curve, n1, a, n2, b, tgt, host_io)
                    : poly_mul_t<CfgBLS>(dev, curve, n1, a, n2, b, tgt, host_io);
}
void poly_eval(int curve, int n, const uint64_t *poly, const uint64_t *x, uint64_t *tgt_host, bool host_io) {
  Device &dev = current_device();
  std::lock_guard<std::mutex> lock(dev.mu);
  if (curve == 0) poly_eval_t<CfgBN>(dev, n, poly, x, tgt_host, host_io);
  else poly_eval_t<CfgBLS>(dev, n, poly, x, tgt_host, host_io);
}
void poly_lincomb(int curve, int K, const int *ns, const uint64_t *coeffs, const uint64_t *const *polys,
                  uint64_t *tgt, bool host_io) {
  Device &dev = current_device();
  std::lock_guard<std::mutex> lock(dev.mu);
  if (curve == 0) poly_lincomb_t<CfgBN>(dev, K, ns, coeffs, polys, tgt, host_io);
  else poly_lincomb_t<CfgBLS>(dev, K, ns, coeffs, polys, tgt, host_io);
}
void poly_set_mul_direct_max(int len) { g_direct_max.store(len < 0 ? -1 : len); }
int poly_last_mul_path() { return g_last_path.load(); }

}  // namespace zk
