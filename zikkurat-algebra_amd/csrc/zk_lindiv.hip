// zk_lindiv.hip -- division of a polynomial by a linear factor x - z on gfx950: the quotient and the
// value p(z) in one sweep, for one or many points z.
//
// What a KZG opening needs (examples/KZG.hs openingProof: quotByVanishing (p - val) (1, loc), i.e.
// <C>_poly_mont_div_by_vanishing with expo_n = 1, bls12_381_poly_mont.c:317-397).  With
//   S_j = sum_{i >= j} a_i z^(i - j)          (S_n = 0,  S_j = a_j + z S_(j+1))
// the quotient of p by x - z is q_j = S_(j+1), j < n - 1, and the remainder is p(z) = S_0; subtracting
// the value from a_0 first, as openingProof does, changes no S_j with j >= 1, so the quotient is the
// same.  Every row is a canonical Fr element: the words equal the reference's whatever the schedule.
//
// S is a suffix scan over the maps v -> a_i + z v.  It runs in three launches, and no kernel waits on
// another workgroup (no look-back, no flags):
//   k_lindiv_tile   a workgroup owns a tile of T = 256 K consecutive rows, K rows per lane.  A lane runs
//                   Horner over its rows from the top, h_l = sum_r a[l K + r] z^r; the 256 values are
//                   combined by a Kogge-Stone suffix scan through LDS, X_l += z^(K 2^d) X_(l + 2^d) for
//                   d = 0 .. 7, after which X_l is the suffix at the lane's first row.  The weight of a
//                   step is the same for every lane: one product per lane and step.  The tile's total
//                   X_0 (carry-in 0) goes to totals[tile].
//   k_lindiv_carry  one workgroup runs the same scan over the totals, in y = z^T, in chunks of T totals
//                   from the top, the carry of a chunk seeding the top lane of the next: it leaves
//                   carries[t] = the suffix above tile t, and the value S_0.
//   k_lindiv_write  the tile again: the top lane's Horner starts from the tile's carry-in, the same scan
//                   gives every lane the suffix above it (X_(l + 1)) as its seed, and the lane reruns
//                   its K Horner steps from that seed, storing S_i at row i - 1.
// Products per row: (K + 8) / K in the tile pass and (2 K + 8) / K in the write pass, 5 at K = 8; bytes
// per row and point: two reads and one write of 32 B.  The 2 x 9 weights of a point (z, z^(K 2^d), and
// the same in y) are computed on the host (zk_host.hpp) and read from a small device table.
//
// Representation (zk_arr.hip's header): rows stay in the reference form a R; a weight is converted
// once per workgroup to the internal radix (w R'), so (a R)(w R') / R' = a w R at every step.  Only
// the fully reduced fe_mul / fe_add: every value is < 2p with normalised limbs.
#include "zk_frdev.hpp"
#include "zk_frcfg.hpp"
#include "zk_lindiv.hpp"

namespace zk {

namespace {

constexpr int LD_LANES = 256, LD_STEPS = 8;  // 2^LD_STEPS lanes
constexpr int LD_KMAX = 8;                   // rows per lane, and the default
constexpr int LD_NW = 1 + LD_STEPS;          // weights of one level: w, then w^(K 2^d), d < LD_STEPS
static_assert((1 << LD_STEPS) == LD_LANES, "the scan covers the workgroup");

struct LdShared {
  uint32_t w[LD_NW * 9];      // this level's weights, internal radix
  uint32_t x[LD_LANES * 9];   // the scan's values (odd row stride: no bank conflicts)
};

// this level's weights of point zi into LDS (caller: __syncthreads before use)
template <class F>
__device__ __forceinline__ void ld_weights(LdShared &sh, const uint64_t *__restrict__ tab) {
  static_assert(F::N == 9, "LdShared is laid out for the 9-limb scalar fields");
  if (threadIdx.x < LD_NW) {
    Fe<F> v, vi;
    ld(v, tab, threadIdx.x);
    fe_to_int(vi, v);
    lds_put(sh.w + threadIdx.x * F::N, vi);
  }
}

// The chunk of 256 K rows of src that starts at row `base` (rows at or above n count as zero), with
// `carry` the suffix above the chunk.  Returns in `total` the suffix at row `base`; WRITE: stores the
// suffix at row i to dst[i - 1] for every row i of the chunk with 1 <= i < n.  Block-uniform control
// flow around the barriers; all 256 threads call it.
template <class F, int K, bool WRITE>
__device__ __forceinline__ void ld_chunk(LdShared &sh, long long base, long long n,
                                         const uint64_t *__restrict__ src, uint64_t *__restrict__ dst,
                                         const Fe<F> &carry, Fe<F> &total) {
  const int tid = threadIdx.x;
  const long long i0 = base + (long long)tid * K;
  Fe<F> w, a[K];
  lds_get(w, sh.w);
#pragma clang loop unroll(full)
  for (int r = 0; r < K; r++) {
    Fe<F> v;
    fe_zero(v);
    if (i0 + r < n) ld(v, src, (size_t)(i0 + r));
    a[r] = v;
  }
  Fe<F> h, t;
  if (tid == LD_LANES - 1) h = carry;
  else fe_zero(h);
#pragma clang loop unroll(full)
  for (int r = K - 1; r >= 0; r--) {
    Fe<F> u;
    fe_mul(t, h, w);
    fe_add(u, a[r], t);
    h = u;
  }
  for (int d = 0; d < LD_STEPS; d++) {
    lds_put(sh.x + tid * F::N, h);
    __syncthreads();
    if (tid + (1 << d) < LD_LANES) {
      Fe<F> o, wd, s;
      lds_get(o, sh.x + (tid + (1 << d)) * F::N);
      lds_get(wd, sh.w + (1 + d) * F::N);
      fe_mul(t, o, wd);
      fe_add(s, h, t);
      h = s;
    }
    __syncthreads();  // every read of this step before the next step's writes
  }
  lds_put(sh.x + tid * F::N, h);
  __syncthreads();
  lds_get(total, sh.x);
  if (WRITE) {
    Fe<F> s = carry;
    if (tid < LD_LANES - 1) lds_get(s, sh.x + (tid + 1) * F::N);
#pragma clang loop unroll(full)
    for (int r = K - 1; r >= 0; r--) {
      Fe<F> u;
      fe_mul(t, s, w);
      fe_add(u, a[r], t);
      s = u;
      const long long i = i0 + r;
      if (i >= 1 && i < n) st(dst, (size_t)(i - 1), s);
    }
  }
  __syncthreads();  // sh.x is free again (the carry pass calls this in a loop)
}

// tab: nz x 2 x LD_NW rows (level 0 in z, level 1 in y = z^T); totals, carries: nz x ntiles rows
template <class F, int K>
__global__ void __launch_bounds__(LD_LANES) k_lindiv_tile(int n, const uint64_t *__restrict__ poly,
                                                          const uint64_t *__restrict__ tab, int ntiles,
                                                          uint64_t *__restrict__ totals) {
  __shared__ LdShared sh;
  const int zi = blockIdx.y;
  ld_weights<F>(sh, tab + (size_t)zi * 2 * LD_NW * 4);
  __syncthreads();
  Fe<F> zero, total;
  fe_zero(zero);
  ld_chunk<F, K, false>(sh, (long long)blockIdx.x * LD_LANES * K, n, poly, nullptr, zero, total);
  if (threadIdx.x == 0) st(totals, (size_t)zi * ntiles + blockIdx.x, total);
}

template <class F, int K>
__global__ void __launch_bounds__(LD_LANES) k_lindiv_carry(int ntiles, const uint64_t *__restrict__ tab,
                                                           const uint64_t *__restrict__ totals,
                                                           uint64_t *__restrict__ carries, uint64_t *__restrict__ vals) {
  __shared__ LdShared sh;
  const int zi = blockIdx.x;
  ld_weights<F>(sh, tab + ((size_t)zi * 2 + 1) * LD_NW * 4);
  __syncthreads();
  const uint64_t *src = totals + (size_t)zi * ntiles * 4;
  uint64_t *dst = carries + (size_t)zi * ntiles * 4;
  Fe<F> carry, total;
  fe_zero(carry);
  if (threadIdx.x == 0) st(dst, (size_t)(ntiles - 1), carry);  // nothing lies above the top tile
  const long long chunk = (long long)LD_LANES * K;
  for (long long c = ((long long)ntiles - 1) / chunk; c >= 0; c--) {  // block-uniform trip count
    ld_chunk<F, K, true>(sh, c * chunk, ntiles, src, dst, carry, total);
    carry = total;
  }
  if (threadIdx.x == 0) st(vals, (size_t)zi, carry);
}

template <class F, int K>
__global__ void __launch_bounds__(LD_LANES) k_lindiv_write(int n, const uint64_t *__restrict__ poly,
                                                           const uint64_t *__restrict__ tab, int ntiles,
                                                           const uint64_t *__restrict__ carries,
                                                           uint64_t *__restrict__ quot) {
  __shared__ LdShared sh;
  const int zi = blockIdx.y;
  ld_weights<F>(sh, tab + (size_t)zi * 2 * LD_NW * 4);
  __syncthreads();
  Fe<F> carry, total;
  ld(carry, carries, (size_t)zi * ntiles + blockIdx.x);
  ld_chunk<F, K, true>(sh, (long long)blockIdx.x * LD_LANES * K, n, poly, quot + (size_t)zi * ((size_t)n - 1) * 4,
                    carry, total);
}

// ---------------------------------------------------------------------------- host side

std::atomic<int> g_tile_rows{0};  // test hook: rows per lane (0: the default)
// the kernels are built for 1, 2, 4 and 8 rows per lane: another value counts as the power of two below it
int rows_in_force() {
  const int v = g_tile_rows.load();
  if (v <= 0 || v >= LD_KMAX) return LD_KMAX;
  return v >= 4 ? 4 : (v >= 2 ? 2 : 1);
}
// fn(std::integral_constant<int, K>) for the rows per lane in force
template <class Fn>
void with_rows(int K, Fn fn) {
  switch (K) {
    case 1: fn(std::integral_constant<int, 1>{}); break;
    case 2: fn(std::integral_constant<int, 2>{}); break;
    case 4: fn(std::integral_constant<int, 4>{}); break;
    default: fn(std::integral_constant<int, LD_KMAX>{}); break;
  }
}

// one level's weights in reference form: w, then w^(K 2^d); returns w^(256 K) in `next`
template <class Fh>
void host_weights(uint64_t *out, const zkh::Fe<Fh> &w, int K, zkh::Fe<Fh> &next) {
  memcpy(out, w.v, 32);
  zkh::Fe<Fh> p = w;
  for (int r = 1; r < K; r++) zkh::mul(p, p, w);
  for (int d = 0; d < LD_STEPS; d++) {
    memcpy(out + 4 * (1 + d), p.v, 32);
    zkh::sqr(p, p);
  }
  next = p;
}

constexpr int LD_ZMAX = 32768;  // points per launch group (gridDim.y)

template <class Cfg>
void lindiv_t(Device &dev, int n, const uint64_t *poly, int nz, const uint64_t *z, uint64_t *quot, uint64_t *vals,
              bool host_io) {
  using F = typename Cfg::Fd;
  using Fh = typename Cfg::Fh;
  hipStream_t s = dev.stream;
  const int K = rows_in_force();
  const size_t N = (size_t)n, T = (size_t)LD_LANES * K;
  const int ntiles = (int)((N + T - 1) / T);
  const bool want_q = quot != nullptr && n > 1;
  const int zb = std::min(nz, LD_ZMAX);  // points per group
  const size_t tab_rows = (size_t)zb * 2 * LD_NW;
  dev.arena.reserve((host_io ? (N + (want_q ? (size_t)zb * (N - 1) : 0)) * 32 : 0) +
                    (tab_rows + 2 * (size_t)zb * ntiles + zb) * 32 + (1 << 20));
  dev.arena.reset();
  Stage sg(dev, host_io);
  const uint64_t *dp = sg.in(poly, N);
  uint64_t *dq = want_q ? sg.out(quot, (size_t)zb * (N - 1)) : nullptr;
  uint64_t *tab = dev.arena.take<uint64_t>(tab_rows * 4);
  uint64_t *totals = dev.arena.take<uint64_t>((size_t)zb * ntiles * 4);
  uint64_t *carries = dev.arena.take<uint64_t>((size_t)zb * ntiles * 4);
  uint64_t *dvals = dev.arena.take<uint64_t>((size_t)zb * 4);
  // pinned block: the weight table on its way in, then the values on their way out
  uint64_t *hst = reinterpret_cast<uint64_t *>(dev.host_staging(tab_rows * 32));
  for (int z0 = 0; z0 < nz; z0 += zb) {
    const int cnt = std::min(zb, nz - z0);
    for (int k = 0; k < cnt; k++) {
      zkh::Fe<Fh> w, y, unused;
      memcpy(w.v, z + (size_t)(z0 + k) * 4, 32);
      host_weights<Fh>(hst + (size_t)k * 2 * LD_NW * 4, w, K, y);
      host_weights<Fh>(hst + ((size_t)k * 2 + 1) * LD_NW * 4, y, K, unused);
    }
    ZK_CHECK(hipMemcpyAsync(tab, hst, (size_t)cnt * 2 * LD_NW * 32, hipMemcpyHostToDevice, s));
    uint64_t *q0 = want_q ? (host_io ? dq : quot + (size_t)z0 * (N - 1) * 4) : nullptr;
    with_rows(K, [&](auto rows) {
      constexpr int KR = decltype(rows)::value;
      hipLaunchKernelGGL((k_lindiv_tile<F, KR>), dim3(ntiles, cnt), dim3(LD_LANES), 0, s, n, dp, tab, ntiles, totals);
      ZK_CHECK(hipGetLastError());
      hipLaunchKernelGGL((k_lindiv_carry<F, KR>), dim3(cnt), dim3(LD_LANES), 0, s, ntiles, tab, totals, carries, dvals);
      ZK_CHECK(hipGetLastError());
      if (want_q) {
        hipLaunchKernelGGL((k_lindiv_write<F, KR>), dim3(ntiles, cnt), dim3(LD_LANES), 0, s, n, dp, tab, ntiles, carries,
                           q0);
        ZK_CHECK(hipGetLastError());
      }
    });
    ZK_CHECK(hipMemcpyAsync(hst, dvals, (size_t)cnt * 32, hipMemcpyDeviceToHost, s));
    if (want_q) sg.back(quot + (size_t)z0 * (N - 1) * 4, q0, (size_t)cnt * (N - 1));  // host_io only
    ZK_CHECK(hipStreamSynchronize(s));
    memcpy(vals + (size_t)z0 * 4, hst, (size_t)cnt * 32);
  }
}

}  // namespace

void poly_div_linear(int curve, int n, const uint64_t *poly, int nz, const uint64_t *z, uint64_t *quot, uint64_t *vals,
                     bool host_io) {
  ZK_REQUIRE(curve == 0 || curve == 1, "poly_div_linear: unknown curve");
  if (nz <= 0) return;
  if (n <= 0) {  // the empty sum and no quotient rows: no device is opened
    memset(vals, 0, (size_t)nz * 32);
    return;
  }
  with_fr(curve, [&](Device &dev, auto cfg) { lindiv_t<decltype(cfg)>(dev, n, poly, nz, z, quot, vals, host_io); });
}
void poly_set_lindiv_tile(int rows_per_lane) { g_tile_rows.store(rows_per_lane < 0 ? 0 : rows_per_lane); }
int poly_lindiv_tile() { return rows_in_force(); }

}  // namespace zk
