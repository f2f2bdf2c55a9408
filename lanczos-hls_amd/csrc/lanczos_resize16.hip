// lanczos_resize16.hip -- the fused instances of LANCZOS_RESIZE_U16: k_rs_fused<RsSample<2>, C, K> for every tap-count bucket
// and C = 1, 3, 4 (16-bit samples resized as Pillow resizes mode I;16).  The kernel and RsSample<2>, which says
// why the bytes are Pillow's, are in lanczos_resize_fused.hpp; a translation unit of their own so that they compile beside
// the others.
#include "lanczos_resize_fused.hpp"

namespace lz {

template hipError_t rs_launch_fused<2, 0>(const RsFusedLaunch&);

}  // namespace lz
