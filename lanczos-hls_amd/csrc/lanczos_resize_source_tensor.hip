// lanczos_resize_source_tensor.hip -- the fused instances of a planar source (lanczos_resize_source) that store floats:
// k_rs_fused<RsSample<1>, C, K, ALPHA, 4 + kRsMapped + kRsPlanar> for every tap-count bucket x C = 3, 4 and alpha.  Every tensor
// request of a planar source runs them, one without a channel map with the identity map.  A translation unit of their own, so
// that they compile beside the others; the kernel is lanczos_resize_fused.hpp's.
#include "lanczos_resize_fused.hpp"

namespace lz {

template hipError_t rs_launch_fused<1, 4 + kRsMapped + kRsPlanar>(const RsFusedLaunch&);
// ... and the ALPHA instances of pitched interleaved rows whose pitch is no dword multiple (kRsRowShift)
template hipError_t rs_launch_fused<1, 4 + kRsMapped + kRsRowShift>(const RsFusedLaunch&);

}  // namespace lz
