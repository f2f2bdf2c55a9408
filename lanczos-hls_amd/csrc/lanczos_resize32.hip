// lanczos_resize32.hip -- the fused instances of LANCZOS_RESIZE_F32: k_rs_fused<RsSample<4>, C, K> for every tap-count bucket
// and C = 1, 3, 4 (float samples resized as Pillow resizes mode F).  The kernel and RsSample<4>, which says why
// the bits are Pillow's, are in lanczos_resize_fused.hpp; a translation unit of their own so that they compile beside the
// others.
#include "lanczos_resize_fused.hpp"

namespace lz {

template hipError_t rs_launch_fused<4, 0>(const RsFusedLaunch&);

}  // namespace lz
