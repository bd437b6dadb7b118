// zk_frcfg.hpp -- a curve's scalar field on the device and on the host, and the one curve dispatch
// of the Fr units (zk_arr.hip, zk_poly.hip, zk_ntt.hip).  Host code only, and without
// zk_curve.hpp: the group units have zk_dispatch.hpp.
#pragma once
#include <mutex>
#include "zk_field.hpp"
#include "zk_host.hpp"
#include "zk_runtime.hpp"

namespace zk {

struct CfgBN { using Fd = BN_Fr; using Fh = zkh::BN_Fr; static constexpr int curve = 0; };
struct CfgBLS { using Fd = BLS_Fr; using Fh = zkh::BLS_Fr; static constexpr int curve = 1; };
// fn(CfgBN{}) for curve 0, fn(CfgBLS{}) otherwise ...
template <class Fn>
inline auto with_cfg(int curve, Fn fn) {
  return curve == 0 ? fn(CfgBN{}) : fn(CfgBLS{});
}
// ... and fn(dev, cfg) on the calling thread's device context with its mutex held, as every entry
// point of zk_arr.hip and zk_poly.hip runs
template <class Fn>
inline auto with_fr(int curve, Fn fn) {
  Device &dev = current_device();
  std::lock_guard<std::mutex> lock(dev.mu);
  return with_cfg(curve, [&](auto cfg) { return fn(dev, cfg); });
}

inline int ceil_log2(size_t n) {
  int lg = 0;
  while (((size_t)1 << lg) < n) lg++;
  return lg;
}
// Two-level power table over the exponents [0, count): x^i = hi[i >> h] * lo[i & (2^h - 1)] with
// nlo = 2^h low and nhi high entries (k_pow_tables, k_poly_eval_tables)
struct PowSplit {
  int h, nlo, nhi;
  explicit PowSplit(size_t count) : h((ceil_log2(count) + 1) / 2), nlo(1 << h), nhi((int)((count + nlo - 1) >> h)) {}
};

}  // namespace zk
