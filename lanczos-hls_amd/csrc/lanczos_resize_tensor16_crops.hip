// lanczos_resize_tensor16_crops.hip -- the fused instances of a lanczos_resize_crops request that stores 16-bit elements:
// k_rs_fused<RsSample<1>, C, K, ALPHA, 2 + kRsMapped + kRsCrops> for every tap-count bucket x C = 1, 3, 4 and alpha.  A
// translation unit of their own, so that they compile beside the others; the kernel is lanczos_resize_fused.hpp's, and the rest
// of the request (the converted route) is lanczos_resize_tensor_crops.hip's.
#include "lanczos_resize_fused.hpp"

namespace lz {

template hipError_t rs_launch_fused<1, 2 + kRsMapped + kRsCrops>(const RsFusedLaunch&);

}  // namespace lz
