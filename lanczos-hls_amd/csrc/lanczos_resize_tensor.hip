// lanczos_resize_tensor.hip -- 8-bit resizes that leave as float, bfloat16 or float16 tensors (include/lanczos_hip.h,
// lanczos_tensor_out, lanczos_tensor16_out and lanczos_tensor_view): out[c * cs + y * rs + x * ps] =
// lut[c][P(y, x, c)], P the byte lanczos_resize_device_ex stores; a view also maps the channels and mirrors frames.  The table entries are moved as 32-bit or 16-bit words, never computed on.  Two kernels:
//
//   fused      the tensor instances of k_rs_fused (lanczos_resize_fused.hpp): the vertical pass stores the elements itself.  A
//              tensor request runs them exactly where the byte request runs the fused kernel, on the same plan.  (The converter
//              of a request with a crop origin per frame, k_rs_to_tensor_crops, is in lanczos_resize_tensor_crops.hip.)
//   converted  k_rs_to_tensor behind any other resize (two passes, one pass, nearest, the plain copy, an element frame of 2^31
//              bytes or more): the bytes go to context scratch, tightly packed, and one streaming launch turns them into
//              elements (k_rs_to_tensor<C, uint16_t> is the k_rs_to_tensor16 of the documents; k_rs_to_tensor_map is the
//              form with a channel map and flips).
//
// The table of ToTensor + Normalize and its rounding to 16 bits are here as well; the validation of a request is
// lanczos_resize_route.cpp's (tensor_validate).
#include "lanczos_resize_fused.hpp"

#include <algorithm>
#include <cstring>

namespace lz {

// ---- host: the normalisation table --------------------------------------------------------------------------------

// ToTensor() then Normalize(mean, std), operation for operation in float: this translation unit is built with
// -ffp-contract=off, and the divisions are IEEE divisions (no reciprocal)
void tensor_lut_normalize(int channels, const float* mean, const float* std, float* lut) {
    for (int c = 0; c < channels; c++) {
        const float m = mean ? mean[c] : 0.0f, s = std ? std[c] : 1.0f;
        for (int v = 0; v < 256; v++) lut[c * 256 + v] = ((float)v / 255.0f - m) / s;
    }
}

// Round to nearest, ties to even, on the bits, as a CPU cast does.  bfloat16 is the upper half-word of the float: half a unit
// less one, plus the unit bit, carries into it (and on into the exponent, up to inf).  float16 re-biases the exponent (127 ->
// 15) and rounds the 13 bits that go the same way, which carries a full mantissa into the exponent and the largest exponent
// into inf; below 2^-14 the result is the integer nearest to value * 2^24, a subnormal (or 0, or 2^-14 itself).  A NaN stays a
// quiet NaN of its sign.
static uint16_t bf16_word(uint32_t b) {
    if ((b & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((b >> 16) | 0x7fc0u);
    return (uint16_t)((b + 0x7fffu + ((b >> 16) & 1u)) >> 16);
}
static uint16_t f16_word(uint32_t b) {
    const uint32_t sign = (b >> 16) & 0x8000u;
    b &= 0x7fffffffu;
    if (b > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
    if (b >= 0x38800000u) {   // 2^-14 and up: a normal float16, or inf
        uint32_t v = b - 0x38000000u;
        v += 0xfffu + ((v >> 13) & 1u);
        return (uint16_t)(sign | std::min(v >> 13, 0x7c00u));
    }
    const uint32_t shift = 126u - (b >> 23);   // value * 2^24 = mantissa >> shift, shift 14 and up
    if (shift > 24u) return (uint16_t)sign;    // below 2^-25: nearer to 0 than to the smallest subnormal
    const uint32_t m = (b & 0x7fffffu) | 0x800000u;
    uint32_t h = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    h += rem > half || (rem == half && (h & 1u));
    return (uint16_t)(sign | h);
}
bool tensor_lut_convert16(const float* in, int n, int format, uint16_t* out) {
    if (format != LANCZOS_TENSOR_BF16 && format != LANCZOS_TENSOR_F16) return false;
    for (int i = 0; i < n; i++) {
        uint32_t b;
        std::memcpy(&b, in + i, 4);
        out[i] = format == LANCZOS_TENSOR_BF16 ? bf16_word(b) : f16_word(b);
    }
    return true;
}

// ---- kernels --------------------------------------------------------------------------------------------------------

struct RsToTensor {
    const uint8_t* src;
    uint8_t* out;
    unsigned long long src_fs, out_fs;   // frame strides (bytes)
    unsigned long long frame_bytes;      // samples of one frame
    unsigned pitch;                      // samples of one row
    const void* lut;   // words of the stored element's width
    long long cs, rs, ps;
};
// ... with a channel map and flips: lut is [out_channels][256]
struct RsToTensorMap : RsToTensor {
    unsigned dst;            // byte c: the output channel of source channel c, 255 where it is dropped
    int flip;                // bit 0: mirror x, bit 1: mirror y
    const uint8_t* d_flip;   // NULL, or one byte per frame of the launch, XORed with flip; read when the kernel runs
    int w, h;                // pixels of a frame
};

constexpr int kToTensorBlock = 4 * kRsThreads;   // samples per workgroup: one dword load per thread

// A thread loads one dword of the frame (coalesced, rows tightly packed, so the frame is one run of bytes) and the wave
// exchanges its 64 dwords as the fused epilogue does: in round r lane i stores sample 64 r + i of the wave's 256.  Addresses
// are 64-bit; the row of the workgroup's first sample costs one division per thread, a 64-bit one only for frames of 4 GiB.
// E is the word of a stored element: uint32_t for floats, uint16_t for bfloat16 and float16.
template <int C, class E>
__global__ __launch_bounds__(kRsThreads) void k_rs_to_tensor(RsToTensor g) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long base = (unsigned long long)blockIdx.x * kToTensorBlock;
    const uint8_t* fsrc = g.src + blockIdx.y * g.src_fs;
    const unsigned long long mine = base + 4ull * tid;
    const uint32_t dw = mine < g.frame_bytes ? *(const uint32_t*)(fsrc + mine) : 0u;
    unsigned long long y0;
    unsigned rem0;
    if (g.frame_bytes <= 0xffffffffull) {
        const unsigned q = (unsigned)base / g.pitch;
        y0 = q, rem0 = (unsigned)base - q * g.pitch;
    } else {
        y0 = base / g.pitch, rem0 = (unsigned)(base - y0 * g.pitch);
    }
    E* fout = (E*)(g.out + blockIdx.y * g.out_fs);
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
        const uint32_t w = (uint32_t)__shfl((int)dw, 16 * rr + (lane >> 2), 64);
        const unsigned local = (unsigned)(wave * 256 + 64 * rr + lane);
        if (base + local < g.frame_bytes) {
            unsigned rem = rem0 + local;   // pitch and the block are below 2^19 samples
            const unsigned dy = rem / g.pitch;
            rem -= dy * g.pitch;
            const unsigned x = rem / C, c = rem - x * C;
            const E v = ((const E*)g.lut)[c * 256 + ((w >> (8 * (lane & 3))) & 255u)];
            fout[(long long)c * g.cs + (long long)(y0 + dy) * g.rs + (long long)x * g.ps] = v;
        }
    }
}

// The same with a channel map and flips, as the fused epilogue's mapped form has them: channel c goes to dst[c] or nowhere,
// and the frame's flips are a base and two signed strides, worked out once per workgroup from one uniform byte load.  A kernel
// of its own and not a branch of the one above: shared through an inlined body, the instances above came out of the compiler
// with another schedule than they had.
template <int C, class E>
__global__ __launch_bounds__(kRsThreads) void k_rs_to_tensor_map(RsToTensorMap g) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long base = (unsigned long long)blockIdx.x * kToTensorBlock;
    const uint8_t* fsrc = g.src + blockIdx.y * g.src_fs;
    const unsigned long long mine = base + 4ull * tid;
    const uint32_t dw = mine < g.frame_bytes ? *(const uint32_t*)(fsrc + mine) : 0u;
    unsigned long long y0;
    unsigned rem0;
    if (g.frame_bytes <= 0xffffffffull) {
        const unsigned q = (unsigned)base / g.pitch;
        y0 = q, rem0 = (unsigned)base - q * g.pitch;
    } else {
        y0 = base / g.pitch, rem0 = (unsigned)(base - y0 * g.pitch);
    }
    E* fout = (E*)(g.out + blockIdx.y * g.out_fs);
    const int m = g.flip ^ (g.d_flip ? __builtin_amdgcn_readfirstlane((int)g.d_flip[blockIdx.y]) : 0);
    const long long t_rs = (m & 2) ? -g.rs : g.rs, t_ps = (m & 1) ? -g.ps : g.ps;
    const long long t_base = ((m & 2) ? (g.h - 1) * g.rs : 0) + ((m & 1) ? (g.w - 1) * g.ps : 0);
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
        const uint32_t w = (uint32_t)__shfl((int)dw, 16 * rr + (lane >> 2), 64);
        const unsigned local = (unsigned)(wave * 256 + 64 * rr + lane);
        if (base + local < g.frame_bytes) {
            unsigned rem = rem0 + local;   // pitch and the block are below 2^19 samples
            const unsigned dy = rem / g.pitch;
            rem -= dy * g.pitch;
            const unsigned x = rem / C, c = rem - x * C;
            const unsigned oc = (g.dst >> (8 * c)) & 255u;
            if (oc < 4) {
                const E v = ((const E*)g.lut)[oc * 256 + ((w >> (8 * (lane & 3))) & 255u)];
                fout[t_base + (long long)oc * g.cs + (long long)(y0 + dy) * t_rs + (long long)x * t_ps] = v;
            }
        }
    }
}

hipError_t rs_to_tensor_launch(const uint8_t* src, size_t src_fs, uint8_t* out, size_t out_fs, int w, int h, int channels,
                               const RsTensorOut& t, int frames, RsIssue& is) {
    RsToTensorMap g{};
    g.src_fs = src_fs, g.out_fs = out_fs;
    g.frame_bytes = (unsigned long long)w * h * channels;
    g.pitch = (unsigned)(w * channels);
    g.lut = t.d_lut;
    g.cs = t.chan_stride, g.rs = t.row_stride, g.ps = t.pix_stride;
    g.dst = t.dst_of_src(), g.flip = t.flip & 3, g.w = w, g.h = h;
    const unsigned blocks = (unsigned)((g.frame_bytes + kToTensorBlock - 1) / kToTensorBlock);   // at most 2^24
    void (*kern)(RsToTensor);
    if (t.elem == 2) kern = channels == 1 ? k_rs_to_tensor<1, uint16_t> : channels == 3 ? k_rs_to_tensor<3, uint16_t> : k_rs_to_tensor<4, uint16_t>;
    else kern = channels == 1 ? k_rs_to_tensor<1, uint32_t> : channels == 3 ? k_rs_to_tensor<3, uint32_t> : k_rs_to_tensor<4, uint32_t>;
    void (*kern_map)(RsToTensorMap);
    if (t.elem == 2) kern_map = channels == 1 ? k_rs_to_tensor_map<1, uint16_t> : channels == 3 ? k_rs_to_tensor_map<3, uint16_t> : k_rs_to_tensor_map<4, uint16_t>;
    else kern_map = channels == 1 ? k_rs_to_tensor_map<1, uint32_t> : channels == 3 ? k_rs_to_tensor_map<3, uint32_t> : k_rs_to_tensor_map<4, uint32_t>;
    return rs_for_frame_groups(is, frames, [&](int f0, int nf) {
        g.src = src + (size_t)f0 * src_fs;
        g.out = out + (size_t)f0 * out_fs;
        g.d_flip = t.d_flip ? t.d_flip + f0 : nullptr;   // a byte per frame
        const dim3 grid(blocks, nf);
        if (t.mapped) hipLaunchKernelGGL(kern_map, grid, dim3(kRsThreads), 0, is.stream, g);
        else hipLaunchKernelGGL(kern, grid, dim3(kRsThreads), 0, is.stream, static_cast<const RsToTensor&>(g));
    });
}

}  // namespace lz
