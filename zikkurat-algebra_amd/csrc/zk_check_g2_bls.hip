// zk_check_g2_bls.hip -- BLS12-381 G2 instantiation of the batch point validation (kernel templates and call
// body in zk_check_impl.hpp).  Replaces a host loop over bls12_381_G2_{affine,proj}_is_on_curve / _is_infinity
// (bls12_381_G2_affine.c:62-110, bls12_381_G2_proj.c:164-195) and over scl_Fr_std(r, P) for membership.
#include "zk_check_g2.hpp"

namespace zk {

ZK_CHECK_G2_INSTANCE(, BLS381_G2)

}  // namespace zk
