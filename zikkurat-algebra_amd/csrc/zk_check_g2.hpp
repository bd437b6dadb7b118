// zk_check_g2.hpp -- what the two G2 units of the batch point validation share (zk_check_g2_bn.hip: BN254_G2
// and the public entry; zk_check_g2_bls.hip: BLS381_G2): the per-curve instantiation of zk_check_impl.hpp's
// call body.  One unit per curve keeps the compile time down, as zk_scl_g2_{bn,bls}.hip do.
#pragma once
#include "zk_check_impl.hpp"

namespace zk {

#define ZK_CHECK_G2_INSTANCE(KW, C) \
  KW template int check_rows_t<C, true>(Device &, int, const uint64_t *, int, uint8_t *, bool);

}  // namespace zk
