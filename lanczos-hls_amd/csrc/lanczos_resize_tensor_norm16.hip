// lanczos_resize_tensor_norm16.hip -- the fused instances of a lanczos_tensor_norm request over LANCZOS_RESIZE_U16 samples:
// k_rs_fused<RsSample<2>, C, K, false, kRsNorm> for every tap-count bucket and C = 1, 3, 4 (16-bit samples resized as Pillow
// resizes mode I;16 and stored as normalised float32, bfloat16 or float16 elements).  The kernel and its norm
// epilogue are in lanczos_resize_fused.hpp; a translation unit of their own so that they compile beside the others.
#include "lanczos_resize_fused.hpp"

namespace lz {

template hipError_t rs_launch_fused<2, kRsNorm>(const RsFusedLaunch&);

}  // namespace lz
