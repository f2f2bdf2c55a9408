// lanczos_resize_ycc16.hip -- YCbCr frames of 16-bit words (P010, P016, P210, planes of 10 / 12 / 16-bit samples) into packed RGB
// of 16-bit samples and normalised tensor elements (include/lanczos_hip.h, lanczos_resize_ycc16 with a matrix):
// the kernel behind the three resized planes of lanczos_resize_ycc.hip's composition.
//
//   k_rs_ycc16_merge   the three resized planes (ResizeState::ycc_planes: `frames` luma planes, then `frames` pairs Cbo | Cro)
//                      through the integer matrix into RGB words, or through it and rs_norm_elem into tensor elements
//
// A plane in scratch holds its words rounded up to a dword multiple, so every plane starts on a dword.
#include <hip/hip_runtime.h>

#include "lanczos_resize_fused.hpp"

namespace lz {

// ---- k_rs_ycc16_merge --------------------------------------------------------------------------------------------------------

struct RsYcc16Merge {
    const uint8_t *y, *c;                  // the luma plane and the (Cb | Cr) pair of the launch's first frame
    unsigned long long y_fs, c_fs, plane_bytes;   // frames a plane (luma) and a pair (chroma) apart; Cr lies plane_bytes behind Cb
    uint8_t* out;
    unsigned long long out_fs;
    unsigned long long n;                  // pixels of a frame
    // the matrix, by value: hi = (max << shift) | ((1 << shift) - 1), the largest sum whose shift stays at max
    int k[3][3], sub[3], shift;
    long long rnd, hi;
    // tensor elements: the view, as RsToTensorNorm has it (div, mean and std by SOURCE channel)
    long long cs, rs, ps;
    unsigned dst;
    int flip;
    const uint8_t* d_flip;
    int w, h, format;
    float div[4], mean[4], std[4];
};

constexpr int kYcc16Group = 2;                         // pixels per thread: one dword of each plane
constexpr int kYcc16Block = kYcc16Group * kRsThreads;   // pixels per workgroup

// channel c of the two pixels whose words are the dwords y, cb, cr: two result words in one dword.  The sum is int64 (|k| < 2^24
// times a difference of words, three of them and the rounding, stays below 2^42); the clamp stands in front of the shift, so
// what is shifted lies in [0, hi] and what comes out in [0, max] -- the same value as clamp(sum >> shift, 0, max), without a
// packed shift-and-saturate instruction in the way (lanczos_resize.hpp, ycc_clip8_shift6)
__device__ __forceinline__ uint32_t ycc16_convert2(const RsYcc16Merge& g, int c, uint32_t y, uint32_t cb, uint32_t cr) {
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < kYcc16Group; i++) {
        const int vy = (int)((y >> (16 * i)) & 0xffffu) - g.sub[0], vb = (int)((cb >> (16 * i)) & 0xffffu) - g.sub[1],
                  vr = (int)((cr >> (16 * i)) & 0xffffu) - g.sub[2];
        long long s = (long long)g.k[c][0] * vy + (long long)g.k[c][1] * vb + (long long)g.k[c][2] * vr + g.rnd;
        s = s < 0 ? 0 : s > g.hi ? g.hi : s;
        r |= (uint32_t)(s >> g.shift) << (16 * i);
    }
    return r;
}

// RGB words.  A plane is one run of words and so is the tight RGB frame: a thread loads one dword of each plane at the same
// offset (2 pixels, coalesced) and stores the three dwords 3 * offset into the frame, which is dword-aligned since the frame
// is.  The one pixel behind the last whole group goes as a dword and a word: nothing is written past 3 n words.  (The dword of
// that pixel is read whole: a plane in scratch is a dword multiple.)
__global__ __launch_bounds__(kRsThreads) void k_rs_ycc16_merge_words(RsYcc16Merge g) {
    const unsigned long long mine = (unsigned long long)blockIdx.x * kYcc16Block + (unsigned long long)kYcc16Group * threadIdx.x;
    if (mine >= g.n) return;
    const uint8_t* fy = g.y + blockIdx.y * g.y_fs + 2ull * mine;
    const uint8_t* fc = g.c + blockIdx.y * g.c_fs + 2ull * mine;
    const uint32_t y = *(const uint32_t*)fy, cb = *(const uint32_t*)fc, cr = *(const uint32_t*)(fc + g.plane_bytes);
    const uint32_t R = ycc16_convert2(g, 0, y, cb, cr), G = ycc16_convert2(g, 1, y, cb, cr), B = ycc16_convert2(g, 2, y, cb, cr);
    uint8_t* o = g.out + blockIdx.y * g.out_fs + 6ull * mine;
    uint32_t* od = (uint32_t*)o;
    od[0] = (R & 0xffffu) | (G << 16);
    if (mine + 2 <= g.n) {
        od[1] = (B & 0xffffu) | (R & 0xffff0000u);
        od[2] = (G >> 16) | (B & 0xffff0000u);
    } else {
        *(uint16_t*)(o + 4) = (uint16_t)B;
    }
}

// Tensor elements, as k_rs_ycc_merge_tensor stores them.  The conversion is the one above; then the wave exchanges its result
// dwords so that in round r lane i stores pixel 64 r + i of the wave's 128 for every output channel: coalesced where pix_stride
// is 1.  The row of the workgroup's first pixel costs one division, a 64-bit one only for frames of 4 Gi pixels; flips are a
// base and two signed strides from one uniform byte load; a channel nobody names is not stored; addresses are 64-bit.  The
// element is rs_norm_elem's, three IEEE operations on the word.  E: the word of an element
template <class E>
__global__ __launch_bounds__(kRsThreads) void k_rs_ycc16_merge_tensor(RsYcc16Merge g) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long base = (unsigned long long)blockIdx.x * kYcc16Block;
    const unsigned long long mine = base + (unsigned long long)kYcc16Group * tid;
    uint32_t y = 0, cb = 0, cr = 0;
    if (mine < g.n) {
        const uint8_t* fy = g.y + blockIdx.y * g.y_fs + 2ull * mine;
        const uint8_t* fc = g.c + blockIdx.y * g.c_fs + 2ull * mine;
        y = *(const uint32_t*)fy, cb = *(const uint32_t*)fc, cr = *(const uint32_t*)(fc + g.plane_bytes);
    }
    uint32_t res[3];
#pragma unroll
    for (int c = 0; c < 3; c++) res[c] = ycc16_convert2(g, c, y, cb, cr);
    unsigned long long y0;
    unsigned rem0;
    const unsigned w = (unsigned)g.w;
    if (g.n <= 0xffffffffull) {
        const unsigned q = (unsigned)base / w;
        y0 = q, rem0 = (unsigned)base - q * w;
    } else {
        y0 = base / w, rem0 = (unsigned)(base - y0 * w);
    }
    E* fout = (E*)(g.out + blockIdx.y * g.out_fs);
    const int m = g.flip ^ (g.d_flip ? __builtin_amdgcn_readfirstlane((int)g.d_flip[blockIdx.y]) : 0);
    const long long t_rs = (m & 2) ? -g.rs : g.rs, t_ps = (m & 1) ? -g.ps : g.ps;
    const long long t_base = ((m & 2) ? (g.h - 1) * g.rs : 0) + ((m & 1) ? (g.w - 1) * g.ps : 0);
#pragma unroll
    for (int rr = 0; rr < kYcc16Group; rr++) {
        uint32_t px[3];
#pragma unroll
        for (int c = 0; c < 3; c++) px[c] = ((uint32_t)__shfl((int)res[c], 32 * rr + (lane >> 1), 64) >> (16 * (lane & 1))) & 0xffffu;
        const unsigned local = (unsigned)(wave * (64 * kYcc16Group) + 64 * rr + lane);
        if (base + local < g.n) {
            const unsigned rem = rem0 + local;   // a row and the block are below 2^17 pixels
            const unsigned dy = rem / w;
            const unsigned x = rem - dy * w;
            const long long at = t_base + (long long)(y0 + dy) * t_rs + (long long)x * t_ps;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const unsigned oc = (g.dst >> (8 * c)) & 255u;
                if (oc < 4) fout[at + (long long)oc * g.cs] = (E)rs_norm_elem((float)px[c], g.div[c], g.mean[c], g.std[c], g.format);
            }
        }
    }
}

hipError_t ycc16_merge_launch(const uint8_t* planes, size_t plane_bytes, uint8_t* out, size_t out_fs, int w, int h,
                              const lanczos_ycc16_matrix& m, const RsTensorOut* t, int frames, RsIssue& is) {
    RsYcc16Merge g{};
    g.y_fs = plane_bytes, g.c_fs = 2 * plane_bytes, g.plane_bytes = plane_bytes;
    g.out_fs = out_fs, g.n = (unsigned long long)w * h, g.w = w, g.h = h;
    for (int c = 0; c < 3; c++) {
        for (int j = 0; j < 3; j++) g.k[c][j] = m.k[c][j];
        g.sub[c] = m.sub[c];
    }
    g.shift = m.shift, g.rnd = m.shift ? 1ll << (m.shift - 1) : 0;
    g.hi = ((long long)m.max << m.shift) | ((1ll << m.shift) - 1);
    void (*kern)(RsYcc16Merge) = k_rs_ycc16_merge_words;
    if (t) {
        g.cs = t->chan_stride, g.rs = t->row_stride, g.ps = t->pix_stride;
        g.dst = t->dst_of_src(), g.flip = t->flip & 3, g.format = t->format;
        for (int oc = 0; oc < t->out_channels; oc++) {
            const int sc = t->src_channel[oc];
            g.div[sc] = t->div[oc], g.mean[sc] = t->mean[oc], g.std[sc] = t->std[oc];
        }
        kern = t->elem == 2 ? k_rs_ycc16_merge_tensor<uint16_t> : k_rs_ycc16_merge_tensor<uint32_t>;
    }
    const unsigned blocks = (unsigned)((g.n + kYcc16Block - 1) / kYcc16Block);   // at most 2^23
    return rs_for_frame_groups(is, frames, [&](int f0, int nf) {
        g.y = planes + (size_t)f0 * plane_bytes;
        g.c = planes + (size_t)frames * plane_bytes + (size_t)f0 * 2 * plane_bytes;
        g.out = out + (size_t)f0 * out_fs;
        g.d_flip = t && t->d_flip ? t->d_flip + f0 : nullptr;
        hipLaunchKernelGGL(kern, dim3(blocks, nf), dim3(kRsThreads), 0, is.stream, g);
    });
}

}  // namespace lz
