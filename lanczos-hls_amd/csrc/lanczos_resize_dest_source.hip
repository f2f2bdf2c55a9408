// lanczos_resize_dest_source.hip -- the instances of the fused resize kernel that read a planar source and store a planar
// destination (k_rs_fused<RsSample<1>, C, K, ALPHA, kRsPlanar + kRsPlanarOut>, lanczos_resize_fused.hpp): uint8 N x C x H x W in,
// uint8 N x C x h x w out, one launch.  lanczos_resize_source.hip and lanczos_resize_dest.hip describe the two halves.
#include "lanczos_resize_fused.hpp"

namespace lz {

template hipError_t rs_launch_fused<1, kRsPlanar + kRsPlanarOut>(const RsFusedLaunch&);

}  // namespace lz
