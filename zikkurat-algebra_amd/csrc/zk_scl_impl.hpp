// zk_scl_impl.hpp -- kernel templates and call bodies of the batch scalar multiplications, over the curve
// type C (G1: BN254 / BLS381, instantiated by zk_scl.hip; G2: BN254_G2 / BLS381_G2 over Fp2, by
// zk_scl_g2_bn.hip / zk_scl_g2_bls.hip) and a group policy G (below).  One base times n scalars (a per-call
// window table, additions only), n bases times n scalars (xyzz_scl per row), and [a tau^i] P (the KZG `taus`).
//
// Replaces a host loop over (SURVEY.md call stack (E), examples/KZG.hs:42-62):
//   <C>_G1_proj_scl_Fr_mont / _scl_Fr_std      bls12_381_G1_proj.c:462-489 (scl_windowed, :435)
//   <C>_G2_proj_scl_Fr_mont / _scl_Fr_std      bls12_381_G2_proj.c:453-480 (scl_windowed, :426)
// followed by <C>_G?_proj_normalize or _to_affine per row.  The reference multiplies by the INTEGER value of
// the scalar (a Montgomery scalar is brought to its canonical standard form first, a standard one is used
// verbatim, values >= r included), so for a point outside the order-r subgroup (BLS12-381 G1 and both twists
// have a cofactor) the result depends on the integer, not on its residue: nothing here reduces a scalar mod
// r or splits it with the endomorphism.
//
// Fixed base.  For a window c the 256-bit integer is recoded into W = ceil(257 / c) signed digits,
// k = sum_w d_w 2^(c w), |d_w| <= 2^(c - 1) (scl_digit, zk_scl.hpp), and
//   [k] P = sum_w sign(d_w) T[w][|d_w|],     T[w][d] = [d 2^(c w)] P,  d = 1 .. 2^(c - 1):
// one mixed addition per non-zero digit and no doubling.  The table is built per call on the device:
//   k_scl_bases      one lane: the W window bases [2^(c w)] P, c Jacobian doublings apart
//   (normalisation)  the group FFT's shared-inversion chain (G::norm: g1_norm_xyzz_enqueue / g2_norm_xyzz_enqueue)
//   k_scl_multiples  one lane per run of SCL_RUN consecutive d of a window: [d0] B by double-and-add,
//                    then + B per row
//   (normalisation)  the same chain over all W 2^(c - 1) rows
//   k_scl_table_int  the rows to the internal Montgomery radix, in place, packed to 2 NP u64 words
// (NP = C::NP64, the u64 words of one coordinate: over Fp2 both halves, c0 || c1.)  A row is x || y in
// internal form (what xyzz_add_aff takes after fe_load_ref's unpacking), or all-0xFF for the point at
// infinity, which a base of small order reaches (order 3: every third d); k_scl_fixed skips such rows.  The
// additions are the complete xyzz_add_aff: with a base of small order, or a scalar near a multiple of the
// group order, the accumulator meets T[w][d] itself (doubling), its negative (infinity) and infinity (copy)
// on ordinary inputs.
//
// Per-row bases: k_scl_rows, one lane per row, xyzz_scl (zk_fftdev.hpp: 255 Jacobian doublings, signed
// 5-bit windows, a 16-entry table per lane in arena scratch; its INF_ROWS form, which skips the entries
// that a base of order <= 16 sends to infinity) -- also the path of a fixed-base call too
// short to pay for the table (G::FIXED_MIN_DEFAULT).  Both paths end in the shared-inversion normalisation.
//
// The group policy G gives what differs between G1 and G2:
//   G::WINDOW_DEFAULT, G::FIXED_MIN_DEFAULT   the measured defaults of the table path
//   G::MAX_LANES                              lanes of the per-row kernel (bounds the per-lane table scratch)
//   G::hooks()                                the group's SclHooks (the test hooks' state)
//   G::norm(curve, st, n, acc, scratch, out, affine)   the normalisation of n XYZZ rows
#pragma once
#include <algorithm>
#include <atomic>
#include <cstring>
#include "zk_arr.hpp"
#include "zk_curve.hpp"
#include "zk_dispatch.hpp"
#include "zk_extdev.hpp"
#include "zk_fftdev.hpp"
#include "zk_host.hpp"
#include "zk_msm.hpp"
#include "zk_runtime.hpp"
#include "zk_scl.hpp"

namespace zk {

// consecutive multiples d B per lane of k_scl_multiples
constexpr int SCL_RUN = 8;

// the test hooks of one group: window (0: default), fixed_min (< 0: default), path of the last fixed-base call
struct SclHooks {
  std::atomic<int> window{0}, fixed_min{-1}, last_path{0};
  void set_window(int c) { window.store(c == 0 ? 0 : std::min(std::max(c, SCL_WINDOW_MIN), SCL_WINDOW_MAX)); }
  void set_fixed_min(int n) { fixed_min.store(n < 0 ? -1 : n); }
};

template <int NWORDS>
struct RowArg {  // one reference-form row as a kernel argument
  uint64_t w[NWORDS];
};

// the scalar of row i as a 256-bit integer: a Montgomery row's canonical standard form (the reference's
// to_std, Fr_mont.c:330-335), a standard row verbatim
template <class Fr>
__device__ __forceinline__ void scl_load_k(uint64_t k[4], const uint64_t *__restrict__ p, bool mont) {
  if (mont) {
    Fe<Fr> a, s;
    fe_load_ref(a, p);
    fe_ref_to_std(s, a);
    uint32_t w[8];
    fe_pack(w, s);
#pragma unroll
    for (int j = 0; j < 4; j++) k[j] = (uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32);
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) k[j] = p[j];
  }
}

// The reference on a base of order 3.  Its 4-bit table (precalc_expos_window_16, G1_proj.c:414-430) takes
// 6 P as dbl(3 P), and its doubling (dbl-2007-bl, :231-264) sends the infinity (0 : Y : 0) that 3 P is to
// the triple (0 : 0 : 0), which the complete addition then carries into 7 P, 12 P .. 15 P and into every
// sum it meets; _normalize and _to_affine read Z = 0 as infinity.  So for such a base the reference
// returns infinity as soon as one 4-bit digit of the scalar is 6, 7 or 12 .. 15, and the true multiple
// otherwise (3 P, 9 P come from additions and are proper).  On y^2 = x^3 + b the points of order 3 over
// the base fields here are those with x = 0 (BLS12-381 G1: (0, +-2); BN254 has none), the orders 5 and 7
// that would meet 10 P, 14 P do not divide the group orders, and from order 9 on no table entry is the
// double of infinity.  Both kernels reproduce it: scl_ref_absorbs on a base with x = 0.
// G2 needs none of it (scl_ref_special): the table doubles entries 1 .. 7 only, and neither twist order
// (BLS12-381: r 13^2 23^2 2713 11953 ..; BN254: r 10069 ..) has a factor <= 7, so no d P, d <= 7, of a finite
// base is infinity and the reference returns the true multiple (tests/test_gpu_scl_g2.py: orders 13, 23).
template <class F>
constexpr bool scl_ref_special() { return is_base_field<F>(); }
__device__ __forceinline__ bool scl_ref_absorbs(const uint64_t k[4]) {
  uint64_t m = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) m |= (k[j] >> 2) & ((k[j] >> 1) | (k[j] >> 3)) & 0x1111111111111111ull;
  return m != 0;  // a digit with bit 2 and one of bits 1, 3
}

// ---------------------------------------------------------------------------- the table

// bx[w] = [2^(c w)] P (XYZZ), w < W: one lane, c doublings between two rows
template <class C>
__global__ void __launch_bounds__(64) k_scl_bases(RowArg<2 * C::NP64> base, int W, int c, uint32_t *__restrict__ bx) {
  using F = typename C::Fp;
  constexpr int NP = C::NP64;
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  Jac<F> acc;
  ld_int(acc.X, base.w);
  ld_int(acc.Y, base.w + NP);
  fe_one(acc.Z);
  for (int w = 0; w < W; w++) {
    Xyzz<F> r;
    if (jac_is_inf(acc)) {
      xyzz_set_inf(r);
    } else {
      r.X = acc.X;
      r.Y = acc.Y;
      fe_sqr(r.ZZ, acc.Z);
      fe_mul(r.ZZZ, r.ZZ, acc.Z);
    }
    xyzz_store(bx + (size_t)w * xw<F>(), r);
#pragma unroll 1
    for (int z = 0; z < c; z++) jac_dbl(acc);
  }
}

// tx[w H + d - 1] = [d] B_w (XYZZ), d = 1 .. H = 2^(c - 1): lane (w, j) takes the run d0 = 1 + j run, ..
// (baff: the normalised window bases, reference-form affine rows, all-0xFF at infinity)
template <class C>
__global__ void __launch_bounds__(256) k_scl_multiples(int W, int H, int run, const uint64_t *__restrict__ baff,
                                                       uint32_t *__restrict__ tx) {
  using F = typename C::Fp;
  constexpr int NP = C::NP64;
  const int runs = (H + run - 1) / run;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)W * runs) return;
  const int w = (int)(t / runs), d0 = 1 + (int)(t % runs) * run;
  const uint64_t *b = baff + (size_t)w * 2 * NP;
  uint32_t *out = tx + ((size_t)w * H + d0 - 1) * xw<F>();
  const int cnt = H - d0 + 1 < run ? H - d0 + 1 : run;
  Xyzz<F> S;
  if (ref_all_ones<F>(b, 2 * NP)) {
    xyzz_set_inf(S);
    for (int i = 0; i < cnt; i++) xyzz_store(out + (size_t)i * xw<F>(), S);
    return;
  }
  Aff<F> B;
  ld_int(B.x, b);
  ld_int(B.y, b + NP);
  xyzz_from_aff(S, B);
  for (int bit = 30 - __clz(d0); bit >= 0; bit--) {  // [d0] B, most significant bit first
    Xyzz<F> D;
    xyzz_dbl(D, S);
    S = D;
    if ((d0 >> bit) & 1) xyzz_add_aff(S, B);
  }
  for (int i = 0; i < cnt; i++) {
    if (i) xyzz_add_aff(S, B);
    xyzz_store(out + (size_t)i * xw<F>(), S);
  }
}

// table rows from the normalisation's reference Montgomery form to the internal radix, in place (packed
// to the same 2 NP words; the all-0xFF infinity rows stay)
template <class C>
__global__ void __launch_bounds__(256) k_scl_table_int(size_t rows, uint64_t *table) {
  using F = typename C::Fp;
  constexpr int NP = C::NP64;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows) return;
  uint64_t *row = table + t * 2 * NP;
  if (ref_all_ones<F>(row, 2 * NP)) return;
  Fe<F> x, y;
  ld_int(x, row);
  ld_int(y, row + NP);
  fe_store_ref(row, x);
  fe_store_ref(row + NP, y);
}

// ---------------------------------------------------------------------------- accumulate

// acc[i] = [k_i] P from the table: one lane per scalar, one complete mixed addition per non-zero digit
template <class C>
__global__ void __launch_bounds__(256) k_scl_fixed(int n, int c, const uint64_t *__restrict__ expos, int mont,
                                                   const uint64_t *__restrict__ table, int base_x0,
                                                   uint32_t *__restrict__ acc_out) {
  using F = typename C::Fp;
  constexpr int NP = C::NP64;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n) return;
  uint64_t k[4];
  scl_load_k<typename C::Fr>(k, expos + i * 4, mont != 0);
  const int W = scl_windows(c);
  const size_t H = (size_t)1 << (c - 1);
  Xyzz<F> acc;
  xyzz_set_inf(acc);
  int carry = 0;
  for (int w = 0; w < W; w++) {
    const int d = scl_digit(k, c, w, carry);
    if (d == 0) continue;
    const uint64_t *row = table + ((size_t)w * H + (size_t)((d < 0 ? -d : d) - 1)) * 2 * NP;
    // the row is the point at infinity: a canonical x never has this top word (over Fp2 it is x.c1's)
    if (row[NP - 1] == ~0ull) continue;
    Aff<F> a;
    fe_load_ref(a.x, row);
    fe_load_ref(a.y, row + NP);
    if (d < 0) {
      Fe<F> ny;
      fe_neg(ny, a.y);
      a.y = ny;
    }
    xyzz_add_aff(acc, a);
  }
  if constexpr (scl_ref_special<F>()) {
    if (base_x0 && scl_ref_absorbs(k)) xyzz_set_inf(acc);  // a base of order 3: the reference's answer (above)
  }
  xyzz_store(acc_out + i * xw<F>(), acc);
}

// acc[i] = [k_i] P_i, P_i = bases[i] (reference-form affine rows); ONE: every P_i is the row `one`, passed
// by value as k_scl_bases takes it (a fixed-base call below the crossover)
template <class C, bool ONE>
__global__ void __launch_bounds__(256) k_scl_rows(RowArg<2 * C::NP64> one, int n, const uint64_t *__restrict__ expos,
                                                  int mont, const uint64_t *__restrict__ bases,
                                                  uint32_t *__restrict__ scratch, uint32_t *__restrict__ acc_out,
                                                  int lanes) {
  using F = typename C::Fp;
  constexpr int NP = C::NP64;
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t *tab = scratch + lane * scl_tab_words<F>();
  for (size_t i = lane; i < (size_t)n; i += (size_t)lanes) {
    const uint64_t *b = ONE ? one.w : bases + i * 2 * NP;
    Xyzz<F> r;
    if (ref_all_ones<F>(b, 2 * NP)) {
      xyzz_set_inf(r);
    } else {
      Aff<F> a;
      ld_int(a.x, b);
      ld_int(a.y, b + NP);
      Xyzz<F> P;
      xyzz_from_aff(P, a);
      uint64_t k[4];
      scl_load_k<typename C::Fr>(k, expos + i * 4, mont != 0);
      xyzz_scl<F, true>(r, P, k, tab);
      if constexpr (scl_ref_special<F>()) {
        uint64_t x0 = 0;
        for (int j = 0; j < NP; j++) x0 |= b[j];
        if (x0 == 0 && scl_ref_absorbs(k)) xyzz_set_inf(r);  // a base of order 3: the reference's answer (above)
      }
    }
    xyzz_store(acc_out + i * xw<F>(), r);
  }
}

// ---------------------------------------------------------------------------- host side

// lanes of the per-row kernel: at most G::MAX_LANES (as the group FFT's stages) so that the per-lane table
// scratch stays bounded, in whole workgroups
template <class G>
inline size_t rows_lanes(size_t n) { return (std::min(n, G::MAX_LANES) + 255) & ~(size_t)255; }

inline bool row_is_inf(const uint64_t *row, int words) {
  for (int i = 0; i < words; i++)
    if (row[i] != ~0ull) return false;
  return true;
}

inline size_t table_rows(int c) { return (size_t)scl_windows(c) << (c - 1); }
// rows of the buffers every phase of a call shares (XYZZ rows, the normalisation's scratch): the n results,
// the table's rows (window c; 0: no table) and the window bases
inline size_t shared_rows(size_t N, int c) {
  return std::max(std::max(N, c ? table_rows(c) : 0), (size_t)scl_windows(SCL_WINDOW_MIN));
}

template <class C, class G>
struct SclCall {  // one call's buffers; `scalars`: how the device scalars come to be
  using F = typename C::Fp;
  static constexpr int NP = C::NP64;
  Device &dev;
  int n;
  bool affine_out;
  size_t N, out_words;
  SclCall(Device &d, int n_, bool aff) : dev(d), n(n_), affine_out(aff), N((size_t)n_), out_words(N * (aff ? 2 : 3) * NP) {}

  // d_out = the normalised rows of the XYZZ rows acc
  void finish(const uint32_t *acc, uint64_t *nscr, uint64_t *d_out) {
    G::norm(C::ID, dev.stream, n, acc, nscr, d_out, affine_out);
  }

  // the table path: d_k device scalars, base one host row (not infinity)
  void run_table(int c, const uint64_t *d_k, bool mont, const uint64_t *base, uint32_t *pts, uint64_t *nscr,
                 uint64_t *d_out) {
    hipStream_t st = dev.stream;
    const int W = scl_windows(c), H = 1 << (c - 1);
    const size_t R = (size_t)W * H;
    const int run = std::min(H, SCL_RUN), runs = (H + run - 1) / run;
    uint32_t *bx = dev.arena.take<uint32_t>((size_t)W * xw<F>());
    uint64_t *baff = dev.arena.take<uint64_t>((size_t)W * 2 * NP);
    uint64_t *table = dev.arena.take<uint64_t>(R * 2 * NP);
    RowArg<2 * NP> b;
    memcpy(b.w, base, sizeof b.w);
    hipLaunchKernelGGL(k_scl_bases<C>, dim3(1), dim3(64), 0, st, b, W, c, bx);
    ZK_CHECK(hipGetLastError());
    G::norm(C::ID, st, W, bx, nscr, baff, true);
    hipLaunchKernelGGL(k_scl_multiples<C>, dim3(div_up((size_t)W * runs, 256)), dim3(256), 0, st, W, H, run, baff, pts);
    ZK_CHECK(hipGetLastError());
    G::norm(C::ID, st, (int)R, pts, nscr, table, true);
    hipLaunchKernelGGL(k_scl_table_int<C>, dim3(div_up(R, 256)), dim3(256), 0, st, R, table);
    ZK_CHECK(hipGetLastError());
    const int base_x0 = std::all_of(base, base + NP, [](uint64_t w) { return w == 0; }) ? 1 : 0;
    hipLaunchKernelGGL(k_scl_fixed<C>, dim3(div_up(N, 256)), dim3(256), 0, st, n, c, d_k, mont ? 1 : 0, table, base_x0,
                       pts);
    ZK_CHECK(hipGetLastError());
    finish(pts, nscr, d_out);
  }

  // the per-row kernel: d_bases n device rows, or (d_bases null) the one host row `base`
  void run_rows(const uint64_t *d_k, bool mont, const uint64_t *d_bases, const uint64_t *base, uint32_t *pts,
                uint64_t *nscr, uint64_t *d_out) {
    const size_t lanes = rows_lanes<G>(N);
    uint32_t *scratch = dev.arena.take<uint32_t>(lanes * scl_tab_words<F>());
    RowArg<2 * NP> b = {};
    if (base) memcpy(b.w, base, sizeof b.w);
    const auto kern = d_bases ? k_scl_rows<C, false> : k_scl_rows<C, true>;
    hipLaunchKernelGGL(kern, dim3((unsigned)(lanes / 256)), dim3(256), 0, dev.stream, b, n, d_k, mont ? 1 : 0, d_bases,
                       scratch, pts, (int)lanes);
    ZK_CHECK(hipGetLastError());
    finish(pts, nscr, d_out);
  }
};

// arena bytes of a call of n rows besides its staged I/O: the table path with window c (0: the per-row kernel)
template <class C, class G>
inline size_t scl_arena_bytes(size_t N, int c) {
  using F = typename C::Fp;
  constexpr int NP = C::NP64;
  const size_t W = c ? scl_windows(c) : 0, R = c ? table_rows(c) : 0, M = shared_rows(N, c);
  size_t b = M * xw<F>() * 4 + M * NP * 8 + (1 << 20);
  if (c) b += W * xw<F>() * 4 + W * 2 * NP * 8 + R * 2 * NP * 8;
  else b += rows_lanes<G>(N) * scl_tab_words<F>() * 4;
  return b;
}

// one base times n scalars.  expos null: the scalars are a tau^i (a, tau on the host), made on the device.
template <class C, class G>
void scl_fixed_t(Device &dev, int n, const uint64_t *expos, bool mont, const uint64_t *a, const uint64_t *tau,
                 const uint64_t *base, bool affine_out, uint64_t *tgt, bool host_io) {
  using F = typename C::Fp;
  using HR = typename HostOf<C>::Fr;
  constexpr int NP = C::NP64;
  if (n <= 0) return;
  SclHooks &hk = G::hooks();
  SclCall<C, G> call(dev, n, affine_out);
  const size_t N = call.N;
  const bool powers = expos == nullptr;
  const int fmin = hk.fixed_min.load(), cw = hk.window.load();
  const bool inf = row_is_inf(base, 2 * NP);
  const int c = (N >= (size_t)(fmin < 0 ? G::FIXED_MIN_DEFAULT : fmin)) ? (cw ? cw : G::WINDOW_DEFAULT) : 0;
  const size_t M = shared_rows(N, c);
  dev.arena.reserve(scl_arena_bytes<C, G>(N, c) + (host_io ? (powers ? 0 : N * 32) + call.out_words * 8 : 0) +
                    (powers ? N * 32 + arr_powers_scratch_bytes(N) : 0));
  dev.arena.reset();
  StagedIO io(dev, host_io, powers ? tgt : expos, powers ? 0 : N * 4, tgt, call.out_words);
  const uint64_t *d_k = io.in;
  if (powers) {
    uint64_t *pk = dev.arena.take<uint64_t>(N * 4);
    arr_powers_enqueue(dev, C::ID, n, a ? a : HR::ONE, tau, pk);
    d_k = pk;
  }
  uint32_t *pts = dev.arena.take<uint32_t>(M * xw<F>());
  uint64_t *nscr = dev.arena.take<uint64_t>(M * NP);
  if (inf) {  // every row infinity: ZZ = 0 rows through the normalisation
    ZK_CHECK(hipMemsetAsync(pts, 0, N * xw<F>() * 4, dev.stream));
    call.finish(pts, nscr, io.out);
  } else if (c) {
    call.run_table(c, d_k, mont, base, pts, nscr, io.out);
  } else {
    call.run_rows(d_k, mont, nullptr, base, pts, nscr, io.out);
  }
  hk.last_path.store(inf ? 0 : c);
  io.finish();
}

template <class C, class G>
void scl_rows_t(Device &dev, int n, const uint64_t *expos, bool mont, const uint64_t *bases, bool affine_out,
                uint64_t *tgt, bool host_io) {
  using F = typename C::Fp;
  constexpr int NP = C::NP64;
  if (n <= 0) return;
  SclCall<C, G> call(dev, n, affine_out);
  const size_t N = call.N;
  dev.arena.reserve(scl_arena_bytes<C, G>(N, 0) + (host_io ? N * 32 + N * 2 * NP * 8 + call.out_words * 8 : 0));
  dev.arena.reset();
  StagedIO io(dev, host_io, expos, N * 4, tgt, call.out_words);
  const uint64_t *d_bases = bases;
  if (host_io) {
    uint64_t *db = dev.arena.take<uint64_t>(N * 2 * NP);
    ZK_CHECK(hipMemcpyAsync(db, bases, N * 2 * NP * 8, hipMemcpyHostToDevice, dev.stream));
    d_bases = db;
  }
  uint32_t *pts = dev.arena.take<uint32_t>(N * xw<F>());
  uint64_t *nscr = dev.arena.take<uint64_t>(N * NP);
  call.run_rows(io.in, mont, d_bases, nullptr, pts, nscr, io.out);
  io.finish();
}

}  // namespace zk
