// zk_dispatch.hpp -- the one curve dispatch of the group units (zk_g1ext.hip, zk_g2ext.hip,
// zk_g2fft.hip); device code comes in with zk_curve.hpp, so only those units include it
#pragma once
#include <mutex>
#include "zk_curve.hpp"
#include "zk_runtime.hpp"

namespace zk {

// fn(tag) with the descriptor of curve index `curve` (0: BN254, otherwise BLS12-381) ...
template <class BN, class BLS, class Fn>
inline auto on_curve(int curve, Fn fn) {
  return curve == 0 ? fn(BN{}) : fn(BLS{});
}
// ... and fn(dev, tag) on the calling thread's device context with its mutex held, as every entry
// point runs
template <class BN, class BLS, class Fn>
inline void on_device_curve(int curve, Fn fn) {
  Device &dev = current_device();
  std::lock_guard<std::mutex> lock(dev.mu);
  on_curve<BN, BLS>(curve, [&](auto c) { fn(dev, c); });
}
template <class Fn>
inline void with_g1(int curve, Fn fn) { on_device_curve<BN254, BLS381>(curve, fn); }
template <class Fn>
inline void with_g2(int curve, Fn fn) { on_device_curve<BN254_G2, BLS381_G2>(curve, fn); }

}  // namespace zk
