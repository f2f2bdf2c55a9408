// lanczos_resize_source_tensor16.hip -- the fused instances of a planar source (lanczos_resize_source) that store 16-bit
// elements: k_rs_fused<RsSample<1>, C, K, ALPHA, 2 + kRsMapped + kRsPlanar>, as lanczos_resize_source_tensor.hip's for floats.
#include "lanczos_resize_fused.hpp"

namespace lz {

template hipError_t rs_launch_fused<1, 2 + kRsMapped + kRsPlanar>(const RsFusedLaunch&);
// ... and the ALPHA instances of pitched interleaved rows whose pitch is no dword multiple (kRsRowShift)
template hipError_t rs_launch_fused<1, 2 + kRsMapped + kRsRowShift>(const RsFusedLaunch&);

}  // namespace lz
