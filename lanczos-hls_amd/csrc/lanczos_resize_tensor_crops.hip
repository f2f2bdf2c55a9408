// lanczos_resize_tensor_crops.hip -- a tensor view with a crop origin per frame (include/lanczos_hip.h, lanczos_resize_crops;
// DESIGN.md 4.5): every frame stores the w x h window of its resize that starts at its own (x0, y0), read from device memory
// and clamped when the kernels run.  Two kernels:
//
//   fused      k_rs_fused<RsSample<1>, C, K, ALPHA, 4 + kRsMapped + kRsCrops> for every tap-count bucket x C = 1, 3, 4 and alpha
//              (lanczos_resize_fused.hpp), and the same with 16-bit elements.
//   converted  k_rs_to_tensor_crops<C, E> behind every other resize, which then computes the bytes of the whole output into
//              context scratch -- or behind none, where the request changes neither axis: it reads the caller's frames.
#include "lanczos_resize_fused.hpp"

#include <algorithm>

namespace lz {

struct RsToTensorCrops {
    const uint8_t* src;
    uint8_t* out;
    unsigned long long src_fs, out_fs;   // frame strides (bytes)
    unsigned long long src_pitch;        // bytes between source rows
    int w, h;                            // pixels of a stored frame
    int max_x0, max_y0;                  // the source frame's size less w, h
    const void* lut;                     // [out_channels][256] words of the stored element's width
    long long cs, rs, ps;
    unsigned dst;                        // byte c: the output channel of source channel c, 255 where it is dropped
    int flip;                            // bit 0: mirror x, bit 1: mirror y
    const uint8_t* d_flip;               // NULL, or one byte per frame of the launch, XORed with flip
    const int32_t* d_origin;             // a pair (x0, y0) per frame of the launch
};

constexpr int kCropsRowBlock = 4 * kRsThreads;   // bytes of a row per workgroup: one dword load per thread

// A workgroup owns 256 dwords of one stored row (blockIdx.y) of one frame (blockIdx.z).  The row's source is w * C bytes at
// any alignment -- an origin moves it by C bytes a pixel, and an RGB pitch is rarely a dword multiple -- so, as k_rs_crop does,
// a thread owns one dword of the ADDRESS grid the source row lies on and loads it whole: the bytes it shares with the
// neighbouring pixels of the same source row, or, at the two ends of a frame, with bytes of the same dword and hence the same
// page, are loaded and dropped.  The wave then exchanges its 64 dwords as k_rs_to_tensor does, so that in round r lane i
// stores byte 64 r + i of the wave's 256: neighbouring lanes store neighbouring samples.  Origin and flips are two uniform
// loads and one per workgroup; the origin is clamped here because nothing else can (lanczos_resize_crops).
template <int C, class E>
__global__ __launch_bounds__(kRsThreads) void k_rs_to_tensor_crops(RsToTensorCrops g) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.z, y = blockIdx.y;
    const int ox = __builtin_amdgcn_readfirstlane(g.d_origin[2 * f]);
    const int oy = __builtin_amdgcn_readfirstlane(g.d_origin[2 * f + 1]);
    const int cx = min(max(ox, 0), g.max_x0), cy = min(max(oy, 0), g.max_y0);
    const uint8_t* srow = g.src + f * g.src_fs + (unsigned long long)(cy + y) * g.src_pitch + (size_t)cx * C;
    const int a0 = (int)((uintptr_t)srow & 3);   // bytes of the row's first dword that lie in front of the row
    const int n = g.w * C;                       // bytes of the row
    const int s0 = (blockIdx.x * kRsThreads + tid) * 4 - a0;   // this thread's dword: bytes s0 .. s0 + 3 of the row
    const uint32_t dw = s0 + 4 > 0 && s0 < n ? *(const uint32_t*)(srow + s0) : 0u;   // (srow - a0) + 4 * q: aligned
    E* fout = (E*)(g.out + f * g.out_fs);
    const int m = g.flip ^ (g.d_flip ? __builtin_amdgcn_readfirstlane((int)g.d_flip[f]) : 0);
    const long long t_rs = (m & 2) ? -g.rs : g.rs, t_ps = (m & 1) ? -g.ps : g.ps;
    const long long t_base = ((m & 2) ? (g.h - 1) * g.rs : 0) + ((m & 1) ? (g.w - 1) * g.ps : 0) + y * t_rs;
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
        const uint32_t wd = (uint32_t)__shfl((int)dw, 16 * rr + (lane >> 2), 64);
        const int j = blockIdx.x * kCropsRowBlock + wave * 256 + 64 * rr + lane - a0;   // byte of the row
        if (j >= 0 && j < n) {
            const int x = j / C, c = j - x * C;
            const unsigned oc = (g.dst >> (8 * c)) & 255u;
            if (oc < 4) {
                const E v = ((const E*)g.lut)[oc * 256 + ((wd >> (8 * (lane & 3))) & 255u)];
                fout[t_base + (long long)oc * g.cs + (long long)x * t_ps] = v;
            }
        }
    }
}

hipError_t rs_to_tensor_crops_launch(const uint8_t* src, size_t src_fs, size_t src_pitch, int src_w, int src_h, uint8_t* out,
                                     size_t out_fs, int w, int h, int channels, const RsTensorOut& t, const int32_t* d_origin,
                                     int frames, RsIssue& is) {
    RsToTensorCrops g{};
    g.src_fs = src_fs, g.out_fs = out_fs, g.src_pitch = src_pitch;
    g.w = w, g.h = h, g.max_x0 = src_w - w, g.max_y0 = src_h - h;
    g.lut = t.d_lut;
    g.cs = t.chan_stride, g.rs = t.row_stride, g.ps = t.pix_stride;
    g.dst = t.dst_of_src(), g.flip = t.flip & 3;
    const int row_bytes = w * channels + 3;   // of the address grid a row can touch, a misaligned start included
    void (*kern)(RsToTensorCrops);
    if (t.elem == 2)
        kern = channels == 1 ? k_rs_to_tensor_crops<1, uint16_t> : channels == 3 ? k_rs_to_tensor_crops<3, uint16_t> : k_rs_to_tensor_crops<4, uint16_t>;
    else
        kern = channels == 1 ? k_rs_to_tensor_crops<1, uint32_t> : channels == 3 ? k_rs_to_tensor_crops<3, uint32_t> : k_rs_to_tensor_crops<4, uint32_t>;
    return rs_for_frame_groups(is, frames, [&](int f0, int nf) {
        g.src = src + (size_t)f0 * src_fs;
        g.out = out + (size_t)f0 * out_fs;
        g.d_flip = t.d_flip ? t.d_flip + f0 : nullptr;   // a byte per frame
        g.d_origin = d_origin + 2 * (size_t)f0;          // a pair per frame
        hipLaunchKernelGGL(kern, dim3((row_bytes + kCropsRowBlock - 1) / kCropsRowBlock, h, nf), dim3(kRsThreads), 0, is.stream, g);
    });
}

}  // namespace lz
