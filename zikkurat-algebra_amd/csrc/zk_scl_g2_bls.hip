// zk_scl_g2_bls.hip -- BLS12-381 G2 instantiation of the batch scalar multiplications (template bodies in
// zk_scl_impl.hpp, the group policy in zk_scl_g2.hpp).  Replaces a host loop over
// bls12_381_G2_proj_scl_Fr_mont / _scl_Fr_std (bls12_381_G2_proj.c:453-480) and _normalize / _to_affine.
#include "zk_scl_g2.hpp"

namespace zk {

ZK_SCL_G2_INSTANCES(, BLS381_G2)

}  // namespace zk
