// lanczos_resize_tensor_norm.hip -- 16-bit and float resizes that leave as normalised float32, bfloat16 or float16 tensors
// (include/lanczos_hip.h, lanczos_tensor_norm): out[oc * cs + Y * rs + X * ps] = cvt(((float)P / div[oc] -
// mean[oc]) / std[oc]), P the sample lanczos_resize_window_device stores.  There is no table: a 16-bit sample would need 256 KiB
// of it per channel and a float has none, and the three operations on the sample give torch's result bit for bit
// (rs_norm_elem, lanczos_resize_fused.hpp).  Two kernels:
//
//   fused      the kRsNorm instances of k_rs_fused: the vertical pass turns the sum it holds into the stored sample and that
//              into the element.
//   converted  k_rs_to_tensor_norm, here, behind any other resize: the samples go to context scratch, tightly packed, and one
//              streaming launch turns them into elements.  A request that changes neither axis and has no window runs it on the
//              caller's frames.
#include "lanczos_resize_fused.hpp"

#include <algorithm>

namespace lz {

struct RsToTensorNorm {
    const uint8_t* src;
    uint8_t* out;
    unsigned long long src_fs, out_fs;   // frame strides (bytes)
    unsigned long long samples;          // of one frame
    unsigned pitch;                      // samples of one row
    long long cs, rs, ps;                // elements
    unsigned dst;                        // byte c: the output channel of source channel c, 255 where it is dropped
    int flip;                            // bit 0: mirror x, bit 1: mirror y
    const uint8_t* d_flip;               // NULL, or one byte per frame of the launch, XORed with flip; read when the kernel runs
    int w, h;                            // pixels of a frame
    int format;                          // LANCZOS_TENSOR_F32 / _BF16 / _F16
    float div[4], mean[4], std[4];       // by SOURCE channel: those of the output channel it goes to
};

constexpr int kToTensorNormDwords = kRsThreads;   // dwords per workgroup: one load per thread

// A thread loads one dword of the frame, 4 / BPS samples (coalesced; rows tightly packed, so the frame is one run of samples),
// and stores an element per sample: neighbouring lanes store neighbouring samples' elements.  A 16-bit frame may start off a
// dword and end in the middle of one: such a thread loads its samples one by one, and none outside the frame.  Addresses are
// 64-bit; the row of a sample costs one division, a 64-bit one only for frames of 2^32 samples and more.
template <int BPS, int C>
__global__ __launch_bounds__(kRsThreads) void k_rs_to_tensor_norm(RsToTensorNorm g) {
    constexpr int SPD = 4 / BPS;
    const unsigned long long i0 = ((unsigned long long)blockIdx.x * kToTensorNormDwords + threadIdx.x) * SPD;
    if (i0 >= g.samples) return;
    const uint8_t* fsrc = g.src + blockIdx.y * g.src_fs;
    uint32_t dw;
    if constexpr (BPS == 4) {
        dw = *(const uint32_t*)(fsrc + 4 * i0);
    } else {
        const uint16_t* p = (const uint16_t*)fsrc + i0;
        const bool both = i0 + 1 < g.samples;
        if (both && ((uintptr_t)p & 2) == 0) dw = *(const uint32_t*)p;
        else dw = (uint32_t)p[0] | (both ? (uint32_t)p[1] << 16 : 0u);
    }
    unsigned long long y;
    unsigned rem;
    if (g.samples <= 0xffffffffull) {
        const unsigned q = (unsigned)i0 / g.pitch;
        y = q, rem = (unsigned)i0 - q * g.pitch;
    } else {
        y = i0 / g.pitch, rem = (unsigned)(i0 - y * g.pitch);
    }
    const int m = g.flip ^ (g.d_flip ? __builtin_amdgcn_readfirstlane((int)g.d_flip[blockIdx.y]) : 0);
    const long long t_rs = (m & 2) ? -g.rs : g.rs, t_ps = (m & 1) ? -g.ps : g.ps;
    const long long t_base = ((m & 2) ? (g.h - 1) * g.rs : 0) + ((m & 1) ? (g.w - 1) * g.ps : 0);
    uint8_t* fout = g.out + blockIdx.y * g.out_fs;
#pragma unroll
    for (int s = 0; s < SPD; s++) {
        if (i0 + s >= g.samples) break;
        unsigned r = rem + s;
        unsigned long long ys = y;
        if (r >= g.pitch) r -= g.pitch, ys++;   // (the second sample of a dword may open the next row)
        const unsigned x = r / C, c = r - x * C;
        const unsigned oc = (g.dst >> (8 * c)) & 255u;
        if (oc < 4) {
            const float v = rs_norm_sample<BPS>(BPS == 4 ? dw : (dw >> (16 * s)) & 0xffffu);
            const uint32_t e = rs_norm_elem(v, rs_norm_pick(g.div, (int)c), rs_norm_pick(g.mean, (int)c), rs_norm_pick(g.std, (int)c), g.format);
            const long long to = t_base + (long long)oc * g.cs + (long long)ys * t_rs + (long long)x * t_ps;
            if (g.format == LANCZOS_TENSOR_F32) ((uint32_t*)fout)[to] = e;
            else ((uint16_t*)fout)[to] = (uint16_t)e;
        }
    }
}

hipError_t rs_to_tensor_norm_launch(const uint8_t* src, size_t src_fs, uint8_t* out, size_t out_fs, int w, int h, int channels,
                                    int bps, const RsTensorOut& t, int frames, RsIssue& is) {
    RsToTensorNorm g{};
    g.src_fs = src_fs, g.out_fs = out_fs;
    g.samples = (unsigned long long)w * h * channels;
    g.pitch = (unsigned)(w * channels);
    g.cs = t.chan_stride, g.rs = t.row_stride, g.ps = t.pix_stride;
    g.dst = t.dst_of_src(), g.flip = t.flip & 3, g.w = w, g.h = h, g.format = t.format;
    for (int oc = 0; oc < t.out_channels; oc++) {
        const int sc = t.src_channel[oc];
        g.div[sc] = t.div[oc], g.mean[sc] = t.mean[oc], g.std[sc] = t.std[oc];
    }
    const unsigned long long dwords = (g.samples * (unsigned)bps + 3) / 4;
    const unsigned blocks = (unsigned)((dwords + kToTensorNormDwords - 1) / kToTensorNormDwords);   // below 2^27
    void (*kern)(RsToTensorNorm);
    if (bps == 2) kern = channels == 1 ? k_rs_to_tensor_norm<2, 1> : channels == 3 ? k_rs_to_tensor_norm<2, 3> : k_rs_to_tensor_norm<2, 4>;
    else if (bps == 4) kern = channels == 1 ? k_rs_to_tensor_norm<4, 1> : channels == 3 ? k_rs_to_tensor_norm<4, 3> : k_rs_to_tensor_norm<4, 4>;
    else return hipErrorInvalidValue;
    return rs_for_frame_groups(is, frames, [&](int f0, int nf) {
        g.src = src + (size_t)f0 * src_fs;
        g.out = out + (size_t)f0 * out_fs;
        g.d_flip = t.d_flip ? t.d_flip + f0 : nullptr;   // a byte per frame
        hipLaunchKernelGGL(kern, dim3(blocks, nf), dim3(kRsThreads), 0, is.stream, g);
    });
}

}  // namespace lz
