// lanczos_resize_dest.hip -- a destination layout beside the descriptor (lanczos_resize_dest, include/lanczos_hip.h): planar
// (CHW) and row-pitched result frames without a repack by the caller.  Here: k_rs_unpack_dest, the streaming scatter of the
// UNPACKED route (planes stored DIRECT are the kRsPlanarOut instances of the fused kernel, whose epilogue alone differs).  Pitched interleaved rows need no kernel code (RsFused::out_pitch);
// the layout is validated and the routes are chosen in lanczos_resize_route.cpp (resize_dest_resolve, rs_route).
#include "lanczos_resize_fused.hpp"

namespace lz {

// ---- k_rs_unpack_dest --------------------------------------------------------------------------------------------------
//
// Tightly packed interleaved frames in context scratch (base and frame stride dword multiples) -> the destination of the UNPACKED
// route.  A wave serves 64 groups of four bytes (or pixels) of one row of one frame (blockIdx.y), the four waves of a workgroup
// four such runs, so that narrow rows fill workgroups too; 64-bit addresses throughout, plain global accesses.
// A thread's dwords of the packed row are put together from the aligned ones around them (rs_load_dword_at: a packed row starts
// at any byte); the block is readable past its last frame for that.
struct RsUnpack {
    const uint8_t* in;
    uint8_t* out;
    unsigned long long in_fs, out_fs, row_stride, chan_stride;
    unsigned w, row_bytes;   // pixels and bytes of a packed row
    unsigned h, runs;        // rows, and runs of 64 groups per row
};
// this lane's row and group of four: wave blockIdx.x * 4 + threadIdx.x / 64 is run (y, k) in raster order; false: past the frame
__device__ __forceinline__ bool rs_unpack_place(const RsUnpack& p, unsigned long long* y, unsigned* i) {
    const unsigned run = blockIdx.x * 4 + (threadIdx.x >> 6);
    const unsigned row = run / p.runs;
    *y = row, *i = (run - row * p.runs) * 64 + (threadIdx.x & 63);
    return row < p.h;
}

// planar, C = 3 or 4: a thread takes pixels 4 i .. 4 i + 3 of the row as C interleaved dwords and writes one dword per plane
template <int C>
__global__ __launch_bounds__(256) void k_rs_unpack_dest(RsUnpack p) {
    unsigned i;
    unsigned long long y;
    const bool have = rs_unpack_place(p, &y, &i) && 4ull * i < p.w;
    const uint8_t* src = p.in + blockIdx.y * p.in_fs + y * p.row_bytes + 4ull * i * C;
    uint8_t* fout = p.out + blockIdx.y * p.out_fs + y * p.row_stride;
    uint32_t o[C];
#pragma unroll
    for (int c = 0; c < C; c++) o[c] = have ? rs_load_dword_at(src + 4 * c) : 0u;
#pragma unroll
    for (int c = 0; c < C; c++) {
        uint32_t pl = 0u;   // byte k: sample c of pixel 4 i + k, byte k * C + c of the C dwords
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = k * C + c;
            pl |= ((o[j >> 2] >> (8 * (j & 3))) & 255u) << (8 * k);
        }
        rs_store_segment<1>(fout + c * p.chan_stride, i, p.w, pl, have);
    }
}

// interleaved, pitched rows: a thread per dword of the packed row (any sample width: the bytes are only moved)
__global__ __launch_bounds__(256) void k_rs_unpack_dest_rows(RsUnpack p) {
    unsigned i;
    unsigned long long y;
    const bool have = rs_unpack_place(p, &y, &i) && 4ull * i < p.row_bytes;
    const uint8_t* src = p.in + blockIdx.y * p.in_fs + y * p.row_bytes + 4ull * i;
    const uint32_t v = have ? rs_load_dword_at(src) : 0u;
    rs_store_segment<1>(p.out + blockIdx.y * p.out_fs + y * p.row_stride, i, p.row_bytes, v, have);
}

hipError_t rs_unpack_dest_launch(const uint8_t* in, size_t in_fs, uint8_t* out, size_t out_fs, const RsDest& s, int w, int h,
                                 int C, int B, int frames, RsIssue& is) {
    RsUnpack p{};
    p.in_fs = in_fs, p.out_fs = out_fs, p.row_stride = s.row_stride, p.chan_stride = s.chan_stride;
    p.w = (unsigned)w, p.row_bytes = (unsigned)(w * C * B);
    if (s.planar && (B != 1 || (C != 3 && C != 4))) return hipErrorInvalidValue;
    const unsigned groups = ((s.planar ? p.w : p.row_bytes) + 3) / 4;
    p.h = (unsigned)h, p.runs = (groups + 63) / 64;   // h * runs < 2^16 * 2^13
    void (*const kern)(RsUnpack) = !s.planar ? k_rs_unpack_dest_rows : C == 3 ? k_rs_unpack_dest<3> : k_rs_unpack_dest<4>;
    return rs_for_frame_groups(is, frames, [&](int f0, int nf) {
        p.in = in + (size_t)f0 * in_fs;
        p.out = out + (size_t)f0 * out_fs;
        hipLaunchKernelGGL(kern, dim3((p.h * p.runs + 3) / 4, nf), dim3(256), 0, is.stream, p);
    });
}

}  // namespace lz
