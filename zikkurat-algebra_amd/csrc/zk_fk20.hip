// zk_fk20.hip -- every KZG opening of a domain at once (Feist-Khovratovich, "FK20"), single points and
// cosets, and the kernel it needed: a row-wise sum of scalar multiples.  DESIGN.md "All openings (FK20)" has
// the derivation; the short form, with n = 2^m, l = 2^c, r = n / l, psi = omega^l and s_i = [tau^i] g1:
//
//   proof k = commitment to the quotient of f by x^l - psi^k = sum_(t < r) psi^(k t) h_t,
//   h_t = sum_(j < l) sum_(u = 0 .. r - 2 - t) F^(j)_(u + t + 1) S^(j)_u,   F^(j)_v = f_(l v + j), S^(j)_u = s_(l u + j)
//
// so the proofs are the group FFT of size r of h, and h is l upper-triangular Toeplitz products of size r.
// Each is embedded in a circulant of size 2r (rho: the generator of the 2r-domain, rho^2 = psi):
//
//   table (per setup)   S^(j) = groupFFT_2r(x^(j)),  x^(j) = (S^(j)_(r-2), .., S^(j)_0, O x (r + 1))     k_fk20_srs
//   per polynomial      C^(j) = NTT_2r(c^(j)),  c^(j) = (F^(j)_(r-1), 0 x (r + 1), F^(j)_1 .. F^(j)_(r-2)) k_fk20_coeffs
//                       u_i = sum_(j < l) [C^(j)_i] S^(j)_i,  i < 2r                                    k_scl_rows_sum
//                       y = groupIFFT_2r(u),  h = y[0 .. r - 1] (y_(r-1) = O),  proofs = groupFFT_r(h)
//
// The group FFTs, the batched NTT and the closing conversions are the library's own entry points (g1_fft,
// ntt_ext, g1_batch_to_affine); every one of them resets the context's arena, so what passes from one step to
// the next lies in a buffer of the call.
//
// k_scl_rows_sum.  tgt[i] = sum_(j < terms) [k_(j,i)] P_(j,i), term-major (term j's rows at j rows + i).  A
// workgroup of 256 lanes holds 256 / T rows, T = the power of two >= min(terms, 256): lane (g, t) of row
// group g walks the terms t, t + T, .. of its row with xyzz_scl (one 16-entry table per lane in arena scratch,
// as k_scl_rows) and adds the products up with the complete xyzz_add -- equal operands (the sum doubles),
// opposite ones (infinity) and infinities are ordinary inputs here.  The T partial sums of a row then fold in
// log2 T halving steps through LDS (128 XYZZ slots: the upper half of a step's lanes stores, the lower half
// adds), and lane t = 0 stores the row for the shared-inversion normalisation.  Row groups are grid-strided
// with a block-uniform trip count, so every lane reaches every barrier; no workgroup waits on another.
#include <climits>
#include "../../include/zkalgebra_gpu.h"
#include "zk_fk20.hpp"
#include "zk_g1ext.hpp"
#include "zk_ntt.hpp"
#include "zk_scl_impl.hpp"

namespace zk {

namespace {

constexpr int FK_LANES = 256;             // lanes of a workgroup of k_scl_rows_sum
constexpr int FK_SLOTS = FK_LANES / 2;    // XYZZ slots of its LDS fold
constexpr size_t FK_MAX_LANES = (size_t)1 << 17;  // as the per-row kernel: bounds the per-lane table scratch

template <class C>
__global__ void __launch_bounds__(FK_LANES) k_scl_rows_sum(int rows, int terms, int lg_t,
                                                           const uint64_t *__restrict__ expos, int mont,
                                                           const uint64_t *__restrict__ bases,
                                                           uint32_t *__restrict__ scratch,
                                                           uint32_t *__restrict__ acc_out) {
  using F = typename C::Fp;
  constexpr int NP = C::NP64, XW = xw<F>();
  __shared__ __attribute__((aligned(16))) uint32_t sh[FK_SLOTS * XW];
  const int T = 1 << lg_t, rpb = FK_LANES >> lg_t;  // lanes per row, rows per workgroup
  const int t = (int)threadIdx.x & (T - 1), g = (int)threadIdx.x >> lg_t;
  uint32_t *tab = scratch + ((size_t)blockIdx.x * FK_LANES + threadIdx.x) * scl_tab_words<F>();
  const size_t R = (size_t)rows, groups = (R + rpb - 1) / rpb;
  for (size_t b = blockIdx.x; b < groups; b += gridDim.x) {  // block-uniform: every lane meets every barrier
    const size_t i = b * rpb + g;
    Xyzz<F> acc;
    xyzz_set_inf(acc);
    if (i < R) {
      for (int j = t; j < terms; j += T) {
        const size_t e = (size_t)j * R + i;
        const uint64_t *bp = bases + e * 2 * NP;
        if (ref_all_ones<F>(bp, 2 * NP)) continue;
        Aff<F> a;
        ld_int(a.x, bp);
        ld_int(a.y, bp + NP);
        Xyzz<F> P, r;
        xyzz_from_aff(P, a);
        uint64_t k[4];
        scl_load_k<typename C::Fr>(k, expos + e * 4, mont != 0);
        xyzz_scl<F, true>(r, P, k, tab);
        if constexpr (scl_ref_special<F>()) {
          uint64_t x0 = 0;
          for (int w = 0; w < NP; w++) x0 |= bp[w];
          if (x0 == 0 && scl_ref_absorbs(k)) xyzz_set_inf(r);  // a base of order 3: as k_scl_rows
        }
        xyzz_add(acc, r);
      }
    }
    for (int h = T >> 1; h >= 1; h >>= 1) {  // lanes [h, 2h) of a row hand their sums to lanes [0, h)
      if (t >= h && t < 2 * h) xyzz_store(sh + (size_t)(g * h + t - h) * XW, acc);
      __syncthreads();
      if (t < h) {
        Xyzz<F> o;
        xyzz_load(o, sh + (size_t)(g * h + t) * XW);
        xyzz_add(acc, o);
      }
      __syncthreads();
    }
    if (t == 0 && i < R) xyzz_store(acc_out + i * XW, acc);
  }
}

// the l x 2r rows of the batched NTT's input, zeros written: row (j, p) = f_(l v + j), v = fk20_coeff_index(r, p)
__global__ void __launch_bounds__(256) k_fk20_coeffs(int lg_l, int lg_r, int npoly, const uint64_t *__restrict__ poly,
                                                     uint64_t *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)2 << (lg_l + lg_r)) return;
  const long long r = 1ll << lg_r, j = (long long)(i >> (lg_r + 1)), p = (long long)(i & (2 * r - 1));
  const long long v = fk20_coeff_index(r, p), src = v < 0 ? -1 : (v << lg_l) + j;
  const bool live = src >= 0 && src < npoly;
#pragma unroll
  for (int w = 0; w < 4; w++) out[i * 4 + w] = live ? poly[(size_t)src * 4 + w] : 0;
}

// the l x 2r projective rows of the table's group FFTs: row (j, p) = s_(l u + j), u = fk20_srs_index(r, p),
// as (x : y : 1); (0 : 1 : 0) behind them and for an all-0xFF SRS row
template <class C>
__global__ void __launch_bounds__(256) k_fk20_srs(int lg_l, int lg_r, const uint64_t *__restrict__ srs,
                                                  uint64_t *__restrict__ out, W6 one_ref) {
  constexpr int NP = C::NP64;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)2 << (lg_l + lg_r)) return;
  const long long r = 1ll << lg_r, j = (long long)(i >> (lg_r + 1)), p = (long long)(i & (2 * r - 1));
  const long long u = fk20_srs_index(r, p);
  const uint64_t *a = u < 0 ? nullptr : srs + (size_t)((u << lg_l) + j) * 2 * NP;
  uint64_t *o = out + i * 3 * NP;
  if (!a || ref_all_ones<typename C::Fp>(a, 2 * NP)) {
    for (int w = 0; w < NP; w++) { o[w] = 0; o[NP + w] = one_ref.w[w]; o[2 * NP + w] = 0; }
  } else {
    for (int w = 0; w < 2 * NP; w++) o[w] = a[w];
    for (int w = 0; w < NP; w++) o[2 * NP + w] = one_ref.w[w];
  }
}

template <class HF>
W6 host_one() {
  W6 o = {{0, 0, 0, 0, 0, 0}};
  for (int j = 0; j < HF::N; j++) o.w[j] = HF::ONE[j];
  return o;
}

// lanes per row: the power of two >= min(terms, FK_LANES), at least 1
int lanes_log(int terms) {
  int lg = 0;
  while ((1 << lg) < terms && (1 << lg) < FK_LANES) lg++;
  return lg;
}

template <class C>
void rows_sum_t(Device &dev, int rows, int terms, const uint64_t *expos, bool mont, const uint64_t *bases,
                bool affine_out, uint64_t *tgt, bool host_io) {
  using F = typename C::Fp;
  constexpr int NP = C::NP64;
  const size_t R = (size_t)rows, E = R * (size_t)terms, out_words = R * (affine_out ? 2 : 3) * NP;
  const int lg_t = lanes_log(terms), rpb = FK_LANES >> lg_t;
  const size_t groups = (R + rpb - 1) / rpb, grid = std::min(groups, FK_MAX_LANES / FK_LANES);
  const size_t tab_words = grid * FK_LANES * scl_tab_words<F>();
  dev.arena.reserve(tab_words * 4 + R * xw<F>() * 4 + R * NP * 8 +
                    (host_io ? E * 32 + E * 2 * NP * 8 + out_words * 8 : 0) + (1 << 20));
  dev.arena.reset();
  StagedIO io(dev, host_io, expos, E * 4, tgt, out_words);
  const uint64_t *d_bases = bases;
  if (host_io) {
    uint64_t *db = dev.arena.take<uint64_t>(E * 2 * NP);
    if (E) ZK_CHECK(hipMemcpyAsync(db, bases, E * 2 * NP * 8, hipMemcpyHostToDevice, dev.stream));
    d_bases = db;
  }
  uint32_t *scratch = dev.arena.take<uint32_t>(tab_words);
  uint32_t *pts = dev.arena.take<uint32_t>(R * xw<F>());
  uint64_t *nscr = dev.arena.take<uint64_t>(R * NP);
  timer_begin(dev);
  hipLaunchKernelGGL(k_scl_rows_sum<C>, dim3((unsigned)grid), dim3(FK_LANES), 0, dev.stream, rows, terms, lg_t, io.in,
                     mont ? 1 : 0, d_bases, scratch, pts);
  ZK_CHECK(hipGetLastError());
  timer_end(dev);
  g1_norm_xyzz_enqueue(C::ID, dev.stream, rows, pts, nscr, io.out, affine_out);
  io.finish();
  timer_collect(dev);
}

// device rows of one call (also while a zk::Error unwinds it)
struct CallBuffer {
  uint64_t *p = nullptr;
  explicit CallBuffer(size_t words) { ZK_CHECK(hipMalloc(reinterpret_cast<void **>(&p), std::max(words, (size_t)1) * 8)); }
  CallBuffer(const CallBuffer &) = delete;
  CallBuffer &operator=(const CallBuffer &) = delete;
  ~CallBuffer() {
    if (p && hipFree(p) != hipSuccess) (void)hipGetLastError();
  }
};

struct Shape {  // sizes of one (log_n, log_l)
  int lg_l, lg_r;
  size_t n, l, r;
  uint64_t rho[4], psi[4];  // generators of the 2r- and the r-domain (Montgomery)
  Shape(int curve, int log_n, int log_l)
      : lg_l(log_l), lg_r(log_n - log_l), n((size_t)1 << log_n), l((size_t)1 << log_l), r(n >> log_l) {
    zkg_fft_generator(curve, lg_r + 1, rho);
    zkg_fft_generator(curve, lg_r, psi);
  }
};

}  // namespace

void g1_scl_rows_sum(int curve, int rows, int terms, const uint64_t *expos, bool expos_mont, const uint64_t *bases,
                     bool affine_out, uint64_t *tgt, bool host_io) {
  ZK_REQUIRE(curve == 0 || curve == 1, "g1_scl_rows_sum: unknown curve");
  ZK_REQUIRE(rows >= 0 && terms >= 0 && (size_t)rows * (size_t)terms <= (size_t)INT_MAX,
             "g1_scl_rows_sum: sizes out of range");
  if (rows == 0) return;
  with_g1(curve, [&](Device &dev, auto c) {
    rows_sum_t<decltype(c)>(dev, rows, terms, expos, expos_mont, bases, affine_out, tgt, host_io);
  });
}

size_t kzg_open_all_table_bytes(int curve, int log_n, int log_l) {
  (void)log_l;  // l x 2r = 2n rows whatever the split
  return ((size_t)2 << log_n) * 2 * (curve == 0 ? BN254::NP64 : BLS381::NP64) * 8;
}

void kzg_open_all_table(int curve, int log_n, int log_l, const uint64_t *d_srs_affine, uint64_t *d_table) {
  const Shape s(curve, log_n, log_l);
  const int NP = curve == 0 ? BN254::NP64 : BLS381::NP64;
  const size_t rows = 2 * s.n, T = 2 * s.r * 3 * NP;  // words of one transform
  CallBuffer x(rows * 3 * NP), fx(rows * 3 * NP);
  with_g1(curve, [&](Device &dev, auto c) {
    using C = decltype(c);
    hipLaunchKernelGGL(k_fk20_srs<C>, dim3(div_up(rows, 256)), dim3(256), 0, dev.stream, s.lg_l, s.lg_r, d_srs_affine,
                       x.p, host_one<typename HostOf<C>::Fp>());
    ZK_CHECK(hipGetLastError());
    ZK_CHECK(hipStreamSynchronize(dev.stream));
  });
  for (size_t j = 0; j < s.l; j++) g1_fft(curve, s.lg_r + 1, s.rho, x.p + j * T, fx.p + j * T, false, false);
  g1_batch_to_affine(curve, (int)rows, fx.p, d_table, false);
}

void kzg_open_all(int curve, int log_n, int log_l, int npoly, const uint64_t *d_poly, const uint64_t *d_table,
                  bool affine_out, uint64_t *d_proofs) {
  const Shape s(curve, log_n, log_l);
  const int NP = curve == 0 ? BN254::NP64 : BLS381::NP64;
  const size_t rows = 2 * s.n;
  CallBuffer ch(rows * 4), u(2 * s.r * 3 * NP), y(2 * s.r * 3 * NP), pi(affine_out ? s.r * 3 * NP : 0);
  with_g1(curve, [&](Device &dev, auto) {
    hipLaunchKernelGGL(k_fk20_coeffs, dim3(div_up(rows, 256)), dim3(256), 0, dev.stream, s.lg_l, s.lg_r, npoly, d_poly,
                       ch.p);
    ZK_CHECK(hipGetLastError());
    ZK_CHECK(hipStreamSynchronize(dev.stream));
  });
  ZK_REQUIRE(ntt_ext(curve, s.lg_r + 1, s.rho, nullptr, (int)s.l, ch.p, ch.p, false, false) == 0,
             "kzg_open_all: the batched NTT refused its arguments");
  g1_scl_rows_sum(curve, (int)(2 * s.r), (int)s.l, ch.p, true, d_table, false, u.p, false);
  g1_fft(curve, s.lg_r + 1, s.rho, u.p, y.p, false, true);
  g1_fft(curve, s.lg_r, s.psi, y.p, affine_out ? pi.p : d_proofs, false, false);  // h = y[0 .. r - 1]
  if (affine_out) g1_batch_to_affine(curve, (int)s.r, pi.p, d_proofs, false);
}

}  // namespace zk
