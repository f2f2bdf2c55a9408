// lanczos_resize_nearest.hip -- the kernel of LANCZOS_FILTER_NEAREST: Pillow's Image.resize(size, Image.NEAREST, box)
// (include/lanczos_hip.h).  There is no arithmetic: out[y][x] = in[vidx[y]][hidx[x]] with two index tables the
// host builds with Pillow's running sum (resize_build_axis) and caches like the tap tables of an axis.
//
//   k_rs_nearest<B, C>  pixels of C samples of B bytes (1 or 4: 8-bit and float frames; pixel sizes 1, 3, 4, 12 and 16 bytes).
//                One launch gathers both axes: a workgroup owns 256 dwords of one output row of one frame (blockIdx.x,
//                .y, .z).  The source row is workgroup-uniform (one scalar load of vidx).  A thread owns one dword of the
//                output row's ADDRESS grid -- the dwords as memory aligns them, wherever the row starts -- gathers the
//                samples that fall into it (a load per sample; four byte loads, or one dword load for an aligned 4-byte
//                pixel) and stores it packed: a wave writes 256 contiguous bytes whatever the pixel size is, and a 3-byte
//                pixel costs no byte stores.  Only the dwords a row shares with its neighbours (a row pitch or a base that
//                is no dword multiple) go out sample by sample.
//
//   k_rs_crop    the window of a resize that changes neither axis (lanczos_resize_window with both passes idle): a copy of
//                the window's rows into a tightly packed frame, for samples of any width (bytes are moved, never looked at:
//                RGBA is not premultiplied, as in the plain copy).  As in the gather, a thread owns one dword of the stored
//                row's ADDRESS grid and stores it whole -- a wave writes 256 contiguous bytes whatever the alignment of the two
//                frames, also for an 8-bit source with an odd row pitch -- and loads it as one dword where the source lies
//                on a dword as well, else as four bytes; only the dwords a row shares with its neighbours go out byte by
//                byte.  The thread walks the frames from blockIdx.z in steps of the grid's depth: any frame count is one launch.
//
// Loads and stores are plain global accesses with 64-bit addresses: frames of any size, bases at any sample boundary.  Every
// index is checked on the host to lie inside the source before a table is cached, and a store is predicated on its sample
// lying inside the row.
#include "lanczos_resize.hpp"

#include <algorithm>
#include <type_traits>

namespace lz {

struct NnArgs {
    const uint8_t* in;
    uint8_t* out;
    unsigned long long in_fs, out_fs;   // frame strides (bytes)
    unsigned in_pitch, out_pitch;       // bytes of a source row, of an output row
    int n_samples;                      // samples of an output row: out_w * C
    const int32_t *hidx, *vidx;
};

template <int B, int C>
__global__ __launch_bounds__(kRsThreads) void k_rs_nearest(NnArgs g) {
    static_assert(B == 1 || B == 4, "8-bit and float samples");
    using T = typename std::conditional<B == 1, uint8_t, uint32_t>::type;
    constexpr int SPD = 4 / B;   // samples per dword
    const int oy = blockIdx.y;
    const uint8_t* srow = g.in + blockIdx.z * g.in_fs + (size_t)g.vidx[oy] * g.in_pitch;
    uint8_t* orow = g.out + blockIdx.z * g.out_fs + (size_t)oy * g.out_pitch;
    const int a0 = (int)((uintptr_t)orow & 3) / B;      // samples of the row's first dword that lie in front of the row
    const int q = blockIdx.x * kRsThreads + threadIdx.x;   // dword of the row's address grid
    const int s0 = q * SPD - a0;                         // its first sample
    if (s0 >= g.n_samples) return;
    const bool whole = s0 >= 0 && s0 + SPD <= g.n_samples;
    uint32_t packed = 0u;
    if (B == 1 && C == 4 && whole && a0 == 0 && ((uintptr_t)srow & 3) == 0) {   // the dword is pixel q
        packed = *(const uint32_t*)(srow + (size_t)g.hidx[q] * 4);
    } else {
#pragma unroll
        for (int j = 0; j < SPD; j++) {
            const int s = s0 + j;
            if (s < 0 || s >= g.n_samples) continue;
            const int px = s / C, c = s - px * C;
            packed |= (uint32_t)((const T*)srow)[g.hidx[px] * C + c] << (8 * B * j);
        }
    }
    if (whole) {
        *(uint32_t*)(orow + (ptrdiff_t)s0 * B) = packed;   // (orow - a0 * B) + 4 * q: aligned
    } else {
#pragma unroll
        for (int j = 0; j < SPD; j++)
            if (s0 + j >= 0 && s0 + j < g.n_samples) ((T*)orow)[s0 + j] = (T)(packed >> (8 * B * j));
    }
}

hipError_t rs_nearest_launch(const uint8_t* in, uint8_t* out, int in_w, int out_w, int out_h, int channels, int bps,
                             const int32_t* hidx, const int32_t* vidx, int frames, size_t in_fs, size_t out_fs,
                             RsIssue& is) {
    NnArgs g{};
    g.in_fs = in_fs, g.out_fs = out_fs;
    g.in_pitch = (unsigned)in_w * channels * bps, g.out_pitch = (unsigned)out_w * channels * bps;
    g.n_samples = out_w * channels;
    g.hidx = hidx, g.vidx = vidx;
    const int spd = 4 / bps;
    const int ndw = (g.n_samples + 2 * (spd - 1)) / spd;   // dwords of the address grid a row can touch, misaligned start included
    void (*kern)(NnArgs);
    if (bps == 1) kern = channels == 1 ? k_rs_nearest<1, 1> : channels == 3 ? k_rs_nearest<1, 3> : k_rs_nearest<1, 4>;
    else if (bps == 4) kern = channels == 1 ? k_rs_nearest<4, 1> : channels == 3 ? k_rs_nearest<4, 3> : k_rs_nearest<4, 4>;
    else return hipErrorInvalidValue;
    return rs_for_frame_groups(is, frames, [&](int f0, int nf) {
        g.in = in + (size_t)f0 * in_fs;
        g.out = out + (size_t)f0 * out_fs;
        hipLaunchKernelGGL(kern, dim3((ndw + kRsThreads - 1) / kRsThreads, out_h, nf), dim3(kRsThreads), 0, is.stream, g);
    });
}

struct CropArgs {
    const uint8_t* in;   // the window's first byte of frame 0
    uint8_t* out;
    unsigned long long in_fs, out_fs;         // frame strides (bytes)
    unsigned long long in_pitch, out_pitch;   // bytes of a source row, of a stored row
    int row_bytes;                            // of a stored row: at most 65535 pixels of 16 bytes
    int frames;
};

__global__ __launch_bounds__(kRsThreads) void k_rs_crop(CropArgs g) {
    const int q = blockIdx.x * kRsThreads + threadIdx.x;   // dword of the stored row's address grid
    const unsigned long long y = blockIdx.y;
    for (int f = blockIdx.z; f < g.frames; f += gridDim.z) {
        const uint8_t* srow = g.in + f * g.in_fs + y * g.in_pitch;
        uint8_t* orow = g.out + f * g.out_fs + y * g.out_pitch;
        const int s0 = q * 4 - (int)((uintptr_t)orow & 3);   // the dword's first byte of the row
        if (s0 >= g.row_bytes) continue;
        if (s0 >= 0 && s0 + 4 <= g.row_bytes) {
            const uint8_t* s = srow + s0;
            const uint32_t v = ((uintptr_t)s & 3) == 0 ? *(const uint32_t*)s
                                                      : (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
            *(uint32_t*)(orow + s0) = v;   // (orow - its offset in the dword) + 4 * q: aligned
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (s0 + j >= 0 && s0 + j < g.row_bytes) orow[s0 + j] = srow[s0 + j];
        }
    }
}

hipError_t rs_crop_launch(const uint8_t* in, uint8_t* out, size_t in_pitch, size_t row_bytes, int rows, int frames,
                          size_t in_fs, size_t out_fs, RsIssue& is) {
    CropArgs g{};
    g.in = in, g.out = out;
    g.in_fs = in_fs, g.out_fs = out_fs;
    g.in_pitch = in_pitch, g.out_pitch = row_bytes;
    g.row_bytes = (int)row_bytes, g.frames = frames;
    const int ndw = ((int)row_bytes + 6) / 4;   // dwords of the address grid a row can touch, a misaligned start included
    // one launch whatever the batch: the kernel strides over the frames with gridDim.z
    const dim3 grid((ndw + kRsThreads - 1) / kRsThreads, rows, std::min(frames, kRsMaxGridFrames));
    hipLaunchKernelGGL(k_rs_crop, grid, dim3(kRsThreads), 0, is.stream, g);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) is.launches++;
    return e;
}

}  // namespace lz
