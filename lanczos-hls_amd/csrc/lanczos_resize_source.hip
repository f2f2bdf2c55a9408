// lanczos_resize_source.hip -- a source layout beside the descriptor (lanczos_resize_source, include/lanczos_hip.h): planar
// (CHW) and row-pitched frames without a repack.  Here: k_rs_pack_source, the streaming gather of the PACKED route (planes read
// DIRECT are the kRsPlanar instances of the fused kernel, whose staging loads alone differ).  The layout is validated and the
// routes are chosen in lanczos_resize_route.cpp (resize_source_resolve, rs_route).
#include "lanczos_resize_fused.hpp"

namespace lz {

// ---- k_rs_pack_source ------------------------------------------------------------------------------------------------
//
// The source of the PACKED route -> tightly packed interleaved frames in context scratch, whose base and frame stride are dword
// multiples.  Every store is a dword of the packed frame; 64-bit addresses throughout (a frame may exceed 4 GiB), plain global
// loads.  A source dword at any byte address is put together from the two aligned dwords around it (the second loaded only
// where the residue is not 0): both hold bytes the layout names, so nothing outside [frame base rounded down to a dword, frame
// end rounded up to one) is read.
struct RsPack {
    const uint8_t* in;
    uint8_t* out;
    unsigned long long in_fs, out_fs, row_stride, chan_stride;
    unsigned long long frame_bytes;   // of a packed frame
    unsigned w, row_bytes;            // pixels and bytes of a packed row
    unsigned npix;                    // w * h (planar: below 2^32)
};

// planar, C = 3 or 4: a thread takes pixels q0 .. q0 + 3 of the frame in raster order (q0 a multiple of 4, so its C dwords of the
// packed frame are aligned).  Where the four lie in one row: a dword per plane and the byte transpose of the fused staging;
// across a row end: byte loads
template <int C>
__global__ __launch_bounds__(256) void k_rs_pack_source(RsPack p) {
    const unsigned long long g = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (g * 4 >= p.npix) return;
    const unsigned q0 = (unsigned)(g * 4);
    const uint8_t* fin = p.in + blockIdx.y * p.in_fs;
    uint32_t* dst = (uint32_t*)(p.out + blockIdx.y * p.out_fs + (unsigned long long)q0 * C);
    const unsigned y = q0 / p.w, x = q0 - y * p.w;
    uint32_t o[C];
    if (x + 4 <= p.w) {
        uint32_t pl[C];
#pragma unroll
        for (int c = 0; c < C; c++) pl[c] = rs_load_dword_at(fin + c * p.chan_stride + y * p.row_stride + x);
        rs_interleave4<C>(pl, o);
    } else {
#pragma unroll
        for (int c = 0; c < C; c++) o[c] = 0u;
        unsigned yy = y, xx = x;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (q0 + i < p.npix) {
#pragma unroll
                for (int c = 0; c < C; c++) {
                    const int j = i * C + c;
                    o[j >> 2] |= (uint32_t)fin[c * p.chan_stride + yy * p.row_stride + xx] << (8 * (j & 3));
                }
            }
            if (++xx == p.w) xx = 0, yy++;
        }
    }
#pragma unroll
    for (int c = 0; c < C; c++)
        if ((unsigned long long)q0 * C + 4 * c < p.frame_bytes) dst[c] = o[c];
}

// interleaved, pitched rows: a thread per dword of the packed frame (any sample width: the bytes are only moved)
__global__ __launch_bounds__(256) void k_rs_pack_source_rows(RsPack p) {
    const unsigned long long at = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (at >= p.frame_bytes) return;
    const uint8_t* fin = p.in + blockIdx.y * p.in_fs;
    const unsigned long long y = at / p.row_bytes;
    const unsigned xb = (unsigned)(at - y * p.row_bytes);
    uint32_t v = 0u;
    if (xb + 4 <= p.row_bytes) {
        v = rs_load_dword_at(fin + y * p.row_stride + xb);
    } else {
        unsigned long long yy = y;
        unsigned xx = xb;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            if (at + b < p.frame_bytes) v |= (uint32_t)fin[yy * p.row_stride + xx] << (8 * b);
            if (++xx == p.row_bytes) xx = 0, yy++;
        }
    }
    *(uint32_t*)(p.out + blockIdx.y * p.out_fs + at) = v;
}

hipError_t rs_pack_source_launch(const uint8_t* in, size_t in_fs, const RsSource& s, uint8_t* out, size_t out_fs, int w, int h,
                                 int C, int B, int frames, RsIssue& is) {
    RsPack p{};
    p.in_fs = in_fs, p.out_fs = out_fs, p.row_stride = s.row_stride, p.chan_stride = s.chan_stride;
    p.w = (unsigned)w, p.row_bytes = (unsigned)(w * C * B);
    p.frame_bytes = (unsigned long long)p.row_bytes * h;
    p.npix = (unsigned)w * (unsigned)h;
    if (s.planar && (B != 1 || (C != 3 && C != 4))) return hipErrorInvalidValue;
    const unsigned long long threads = s.planar ? ((unsigned long long)p.npix + 3) / 4 : (p.frame_bytes + 3) / 4;
    void (*const kern)(RsPack) = !s.planar ? k_rs_pack_source_rows : C == 3 ? k_rs_pack_source<3> : k_rs_pack_source<4>;
    return rs_for_frame_groups(is, frames, [&](int f0, int nf) {
        p.in = in + (size_t)f0 * in_fs;
        p.out = out + (size_t)f0 * out_fs;
        hipLaunchKernelGGL(kern, dim3((unsigned)((threads + 255) / 256), nf), dim3(256), 0, is.stream, p);
    });
}

}  // namespace lz
