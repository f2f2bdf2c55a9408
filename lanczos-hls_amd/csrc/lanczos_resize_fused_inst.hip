// lanczos_resize_fused_inst.hip -- one instance of rs_launch_fused with its k_rs_fused kernels: entry LZ_RS_INST of
// LZ_RS_FUSED_INSTANCES (lanczos_resize.hpp).  The Makefile compiles this file once per entry, side by side.
#include "lanczos_resize_fused.hpp"

#ifndef LZ_RS_INST
#error "compile with -DLZ_RS_INST=<index of an entry of LZ_RS_FUSED_INSTANCES>"
#endif

namespace lz {

static_assert(LZ_RS_INST >= 0 && LZ_RS_INST < kRsFusedInstances, "LZ_RS_INST is no entry of LZ_RS_FUSED_INSTANCES");

template <int I>
struct RsInst;
#define X(I, BPS, FLAGS)                        \
    template <>                                 \
    struct RsInst<I> {                          \
        static constexpr int bps = BPS, flags = FLAGS; \
    };
LZ_RS_FUSED_INSTANCES(X)
#undef X

template hipError_t rs_launch_fused<RsInst<LZ_RS_INST>::bps, RsInst<LZ_RS_INST>::flags>(const RsFusedLaunch&);

}  // namespace lz
