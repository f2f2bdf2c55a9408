// lanczos_resize_tensor_norm32.hip -- the fused instances of a lanczos_tensor_norm request over LANCZOS_RESIZE_F32 samples:
// k_rs_fused<RsSample<4>, C, K, false, kRsNorm> for every tap-count bucket and C = 1, 3, 4 (float samples resized as Pillow
// resizes mode F and stored as normalised float32, bfloat16 or float16 elements).  The kernel and its norm
// epilogue are in lanczos_resize_fused.hpp; a translation unit of their own so that they compile beside the others.
#include "lanczos_resize_fused.hpp"

namespace lz {

template hipError_t rs_launch_fused<4, kRsNorm>(const RsFusedLaunch&);

}  // namespace lz
