// lanczos_resize_ycc_out.hip -- packed RGB bytes into YCbCr frames (include/lanczos_hip.h, lanczos_resize_ycc_out with src NULL;
// DESIGN.md 4.5): the kernel behind the three-channel resize of lanczos_resize_ycc.hip's composition.
//
//   k_rs_ycc_encode   converts tight RGB frames through the forward table, averages the chroma blocks and stores Y rows and chroma
//                planes or interleaved chroma rows, in one pass.
#include <hip/hip_runtime.h>

#include "lanczos_resize.hpp"

namespace lz {

struct RsYccEncode {
    const uint8_t* in;                 // tight RGB frames, 3 w h bytes each, at any byte address
    unsigned long long in_fs;
    uint8_t* out;
    unsigned long long out_fs, y_rs, c_rs, cb_off, cr_off;
    int w, h, ch;                      // the frame, and its chroma rows
    int nv;                            // 0: planes; 1: interleaved (Cb, Cr); 2: interleaved (Cr, Cb)
    const int32_t* table;              // [3][3][256], rows Y, Cb, Cr
};

constexpr int kYccEncRows = 4;   // chroma rows per workgroup: one staging of the table serves up to 8 luma rows of 1024 pixels

// byte n of the twelve in d[0 .. 2]
__device__ __forceinline__ unsigned ycc_byte12(const uint32_t* d, int n) { return (d[n >> 2] >> (8 * (n & 3))) & 255u; }

// `n` bytes at any address, the last of them v's highest
__device__ __forceinline__ void ycc_store_bytes(uint8_t* p, uint32_t v, int n) {
    for (int i = 0; i < n; i++) p[i] = (uint8_t)(v >> (8 * i));
}

// One thread owns four neighbouring pixels of 1 << SY rows: whole chroma blocks (two of 2 x (1 << SY) pixels under SX, four of
// 1 x (1 << SY) without), so the average needs no exchange; ragged blocks at the right and bottom edges divide by the 1, 2 or 4
// bytes they hold.  A workgroup covers 1024 pixels of kYccEncRows chroma rows of one frame.  The twelve bytes of a row's four
// pixels are three dwords where the address is a dword multiple, and four aligned dwords shifted together where it is not and
// those lie inside the frame; at the frame's edges, and for the pixels behind the last whole group of four, bytes.  Y goes out as
// one dword, chroma as one dword (four samples of a plane, or two interleaved pairs) or one 16-bit word (two samples of a
// subsampled plane) where the address allows and all of them exist, else as bytes: only named bytes are written, and nothing is
// read outside a frame's 3 w h bytes.
template <int SX, int SY>
__global__ __launch_bounds__(kRsThreads) void k_rs_ycc_encode(RsYccEncode g) {
    __shared__ int32_t t[9 * 256];
    for (int i = threadIdx.x; i < 9 * 256; i += kRsThreads) t[i] = g.table[i];
    __syncthreads();
    const unsigned gx = blockIdx.x * kRsThreads + threadIdx.x;
    const int x0 = 4 * (int)gx;
    if (x0 >= g.w) return;
    const int npx = g.w - x0 < 4 ? g.w - x0 : 4;
    const uint8_t* const fin = g.in + blockIdx.z * g.in_fs;
    const uintptr_t f_begin = (uintptr_t)fin, f_end = f_begin + 3ull * (unsigned long long)g.w * g.h;
    uint8_t* const fout = g.out + blockIdx.z * g.out_fs;
    const int c_end = min((int)(blockIdx.y + 1) * kYccEncRows, g.ch);
    for (int cy = blockIdx.y * kYccEncRows; cy < c_end; cy++) {
        int sb[4] = {0, 0, 0, 0}, sr[4] = {0, 0, 0, 0};   // the sums of the thread's chroma samples: per pixel, or per pair under SX
        int rows = 0;
#pragma unroll
        for (int r = 0; r <= SY; r++) {
            const int y = (cy << SY) + r;
            if (y >= g.h) break;
            rows++;
            const uint8_t* const p = fin + 3ull * ((unsigned long long)y * g.w + x0);
            const uintptr_t al = (uintptr_t)p & ~(uintptr_t)3;
            const unsigned sh = (unsigned)((uintptr_t)p & 3u);
            uint32_t d[3] = {0, 0, 0};
            if (npx == 4 && al >= f_begin && al + (sh ? 16u : 12u) <= f_end) {
                const uint32_t* const q = (const uint32_t*)al;
                const uint32_t q0 = q[0], q1 = q[1], q2 = q[2], q3 = sh ? q[3] : 0u;
                d[0] = __builtin_amdgcn_alignbyte(q1, q0, sh), d[1] = __builtin_amdgcn_alignbyte(q2, q1, sh);
                d[2] = __builtin_amdgcn_alignbyte(q3, q2, sh);
            } else {
                for (int i = 0; i < 3 * npx; i++) d[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
            }
            uint32_t yy = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const unsigned R = ycc_byte12(d, 3 * i), G = ycc_byte12(d, 3 * i + 1), B = ycc_byte12(d, 3 * i + 2);
                yy |= ycc_clip8_shift6(t[R] + t[256 + G] + t[512 + B]) << (8 * i);
                if (i < npx) {   // (a pixel past the row's end is no part of a block)
                    sb[SX ? i >> 1 : i] += (int)ycc_clip8_shift6(t[768 + R] + t[1024 + G] + t[1280 + B]);
                    sr[SX ? i >> 1 : i] += (int)ycc_clip8_shift6(t[1536 + R] + t[1792 + G] + t[2048 + B]);
                }
            }
            uint8_t* const yo = fout + (unsigned long long)y * g.y_rs + x0;
            if (npx == 4 && ((uintptr_t)yo & 3u) == 0) *(uint32_t*)yo = yy;
            else ycc_store_bytes(yo, yy, npx);
        }
        // the samples: block i of the thread holds `rows` rows of 2 pixels (the last one of an odd row 1) under SX, of 1 without
        const int nc = SX ? (npx + 1) >> 1 : npx;
        uint32_t cb = 0, cr = 0;
#pragma unroll
        for (int i = 0; i < (SX ? 2 : 4); i++) {
            const int cols = SX ? (npx - 2 * i >= 2 ? 2 : 1) : 1;
            const int dn = cols * rows;   // 1, 2 or 4: ((sum + d / 2) * floor(2^24 / d)) >> 24 is the rounding shift
            const int vb = dn == 1 ? sb[i] : dn == 2 ? (sb[i] + 1) >> 1 : (sb[i] + 2) >> 2;
            const int vr = dn == 1 ? sr[i] : dn == 2 ? (sr[i] + 1) >> 1 : (sr[i] + 2) >> 2;
            cb |= (uint32_t)vb << (8 * i), cr |= (uint32_t)vr << (8 * i);
        }
        uint8_t* const crow = fout + (unsigned long long)cy * g.c_rs;
        if (SX && g.nv) {   // two pairs: the thread's four bytes of the interleaved row
            const uint32_t first = g.nv == 2 ? cr : cb, second = g.nv == 2 ? cb : cr;
            const uint32_t v = (first & 0xffu) | ((second & 0xffu) << 8) | ((first & 0xff00u) << 8) | ((second & 0xff00u) << 16);
            uint8_t* const o = crow + g.cb_off + 4ull * gx;
            if (nc == 2 && ((uintptr_t)o & 3u) == 0) *(uint32_t*)o = v;
            else ycc_store_bytes(o, v, 2 * nc);
        } else {
            const unsigned long long cx0 = SX ? 2ull * gx : 4ull * gx;
            uint8_t* const ob = crow + g.cb_off + cx0;
            uint8_t* const orr = crow + g.cr_off + cx0;
            if (SX) {
                if (nc == 2 && ((uintptr_t)ob & 1u) == 0) *(uint16_t*)ob = (uint16_t)cb;
                else ycc_store_bytes(ob, cb, nc);
                if (nc == 2 && ((uintptr_t)orr & 1u) == 0) *(uint16_t*)orr = (uint16_t)cr;
                else ycc_store_bytes(orr, cr, nc);
            } else {
                if (nc == 4 && ((uintptr_t)ob & 3u) == 0) *(uint32_t*)ob = cb;
                else ycc_store_bytes(ob, cb, nc);
                if (nc == 4 && ((uintptr_t)orr & 3u) == 0) *(uint32_t*)orr = cr;
                else ycc_store_bytes(orr, cr, nc);
            }
        }
    }
}

hipError_t ycc_encode_launch(const uint8_t* in, size_t in_fs, uint8_t* out, size_t out_fs, const YccLayout& t, int w, int h,
                             const int32_t* table, int frames, RsIssue& is) {
    RsYccEncode g{};
    g.in_fs = in_fs, g.out_fs = out_fs, g.y_rs = t.y_rs, g.c_rs = t.c_rs, g.cb_off = t.cb_off, g.cr_off = t.cr_off;
    g.w = w, g.h = h, g.ch = t.ch, g.table = table;
    g.nv = t.layout == LANCZOS_YCC_NV12 ? 1 : t.layout == LANCZOS_YCC_NV21 ? 2 : 0;
    void (*kern)(RsYccEncode) = t.sx ? (t.sy ? k_rs_ycc_encode<1, 1> : k_rs_ycc_encode<1, 0>)
                                     : (t.sy ? k_rs_ycc_encode<0, 1> : k_rs_ycc_encode<0, 0>);
    const unsigned groups = ((unsigned)w + 3u) / 4u;
    const dim3 grid((groups + kRsThreads - 1) / kRsThreads, (t.ch + kYccEncRows - 1) / kYccEncRows, 1);   // at most 64 x 16384
    return rs_for_frame_groups(is, frames, [&](int f0, int nf) {
        g.in = in + (size_t)f0 * in_fs, g.out = out + (size_t)f0 * out_fs;
        hipLaunchKernelGGL(kern, dim3(grid.x, grid.y, nf), dim3(kRsThreads), 0, is.stream, g);
    });
}

}  // namespace lz
