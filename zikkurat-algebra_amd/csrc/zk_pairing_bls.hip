// zk_pairing_bls.hip -- BLS12-381 instantiation of the pairing kernel (bodies in zk_pairing_impl.hpp).
// Replaces a host loop over bls12_381_pairing_affine / _final_expo (bls12_381_pairing.c).
#include "zk_pairing_impl.hpp"

namespace zk {

ZK_PAIRING_INSTANCES(, BLS381_G2)

}  // namespace zk
