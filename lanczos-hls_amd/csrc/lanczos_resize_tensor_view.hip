// lanczos_resize_tensor_view.hip -- the fused instances of a lanczos_tensor_view with a channel map or flips that stores
// floats: k_rs_fused<RsSample<1>, C, K, ALPHA, 4 + kRsMapped> for every tap-count bucket x C = 1, 3, 4 and alpha.  A
// translation unit of their own, so that they compile beside the others; the kernel is lanczos_resize_fused.hpp's, and the rest
// of the request (validation, the table, the converted route) is lanczos_resize_tensor.hip's.
#include "lanczos_resize_fused.hpp"

namespace lz {

template hipError_t rs_launch_fused<1, 4 + kRsMapped>(const RsFusedLaunch&);

}  // namespace lz
