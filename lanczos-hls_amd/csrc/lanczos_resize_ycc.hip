// lanczos_resize_ycc.hip -- the YCbCr entries (include/lanczos_hip.h: lanczos_resize_ycc_*, lanczos_resize_ycc_out,
// lanczos_resize_ycc16): frames of 8-bit or 16-bit samples (I420, 4:2:2 and 4:4:4 planes, NV12 / NV21, P010 / P016 /
// P210) into YCbCr frames, packed RGB and tensor elements, and packed RGB bytes into YCbCr frames.  The contract is Pillow's: every
// plane resized as an "L" or "I;16" image (chroma with the box scaled to its plane).  Nothing here resizes: the planes go through
// resize_device as one-channel requests with a pitched source and a pitched destination, so rs_route decides for each of them
// what it decides for any one-channel frame.  What is here stands around those calls, once for both sample widths:
//
//   k_rs_ycc_split, k_rs_ycc_split16   interleaved chroma in: the pairs of every frame into two tight planes (ResizeState::ycc_in,
//                    a pair of planes Cb | Cr per frame), so that the chroma resize is one call of 2 * frames frames.
//   k_rs_ycc_join, k_rs_ycc_join16     interleaved chroma out: the two tight planes (ResizeState::ycc_out, a pair per frame) into the
//                    pitched rows of the destination: the split backwards.
//   k_rs_ycc_merge   RGB bytes and elements out: the three resized planes (ResizeState::ycc_planes) through the colour table into
//                    interleaved RGB bytes, or through it and the element table of a view into float32 / 16-bit tensor elements.
//                    Modelled on k_rs_to_tensor_map (lanczos_resize_tensor.hip).  The merge of words through an integer matrix,
//                    k_rs_ycc16_merge, is in lanczos_resize_ycc16.hip.
//   from RGB         the three-channel request stores tight RGB into ResizeState::ycc_rgb (a request that resizes nothing is not
//                    issued at all: the caller's frames are read) and k_rs_ycc_encode (lanczos_resize_ycc_out.hip) converts,
//                    averages and stores the planes.
//
// A plane in scratch holds its samples rounded up to a dword multiple, so every plane starts on a dword.  ycc_planes holds
// `frames` luma planes and behind them `frames` pairs (Cbo | Cro): planar chroma is stored with two calls a pair apart, split
// chroma with one call of 2 * frames frames a plane apart.  All strides, offsets and extents of a YccLayout are bytes.  The
// layouts' validation and the standard tables are host-only code: lanczos_resize_ycc_layout.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "lanczos_resize.hpp"

namespace lz {

// ---- k_rs_ycc_split / k_rs_ycc_join ------------------------------------------------------------------------------------------

struct RsYccSplit {
    const uint8_t* in;         // the interleaved plane of the launch's first frame
    uint8_t* out;              // its first-component plane; the second one lies plane_bytes behind, the next frame's 2 * plane_bytes
    unsigned long long in_fs, c_rs, plane_bytes;
    int cw;                    // pairs of a row
    int second_first;          // NV21: the pair's first byte belongs to the second output plane (Cr, Cb -> Cb | Cr)
};

// One row of one frame per (blockIdx.y, blockIdx.z).  The row's bytes [A, A + 2 cw) are covered by the dwords at dword-aligned
// addresses inside them, one per thread, and by the up to three bytes in front of the first and behind the last of those, one
// per thread too: nothing outside the row is read, whatever the residues of base, pitch and frame stride.  Byte j of the row
// belongs to component j & 1 and pair j >> 1, so a dword holds two bytes of each plane, neighbours there.
__global__ __launch_bounds__(kRsThreads) void k_rs_ycc_split(RsYccSplit g) {
    const uint8_t* row = g.in + blockIdx.z * g.in_fs + blockIdx.y * g.c_rs;
    uint8_t* const o0 = g.out + blockIdx.z * 2ull * g.plane_bytes + (unsigned long long)blockIdx.y * g.cw;
    uint8_t* const p0 = g.second_first ? o0 + g.plane_bytes : o0;   // where component 0 of a pair goes, and component 1
    uint8_t* const p1 = g.second_first ? o0 : o0 + g.plane_bytes;
    const unsigned len = 2u * (unsigned)g.cw;
    const unsigned to_dword = (unsigned)(-(uintptr_t)row & 3u), head = to_dword < len ? to_dword : len;
    const unsigned nd = (len - head) >> 2, rest = len - head - 4u * nd;
    const unsigned k = blockIdx.x * kRsThreads + threadIdx.x;
    if (k < nd) {
        const unsigned j = head + 4u * k;                                // even or odd, as head is
        const uint32_t dw = *(const uint32_t*)(row + j);
        const unsigned a = j & 1u;                                       // the component of the dword's bytes 0 and 2
        const unsigned pa = j >> 1, pb = (j + 1u) >> 1;                  // the pairs of bytes 0 and 1
        uint8_t* da = (a ? p1 : p0) + pa;                                    // bytes 0, 2
        uint8_t* db = (a ? p0 : p1) + pb;                               // bytes 1, 3
        const uint32_t va = (dw & 0xffu) | ((dw >> 8) & 0xff00u), vb = ((dw >> 8) & 0xffu) | ((dw >> 16) & 0xff00u);
        if (((uintptr_t)da & 1u) == 0) *(uint16_t*)da = (uint16_t)va;
        else da[0] = (uint8_t)va, da[1] = (uint8_t)(va >> 8);
        if (((uintptr_t)db & 1u) == 0) *(uint16_t*)db = (uint16_t)vb;
        else db[0] = (uint8_t)vb, db[1] = (uint8_t)(vb >> 8);
    } else if (k < nd + head + rest) {
        const unsigned i = k - nd;
        const unsigned j = i < head ? i : 4u * nd + i;                   // the bytes in front, then those behind
        ((j & 1u) ? p1 : p0)[j >> 1] = row[j];
    }
}

struct RsYccJoin {
    const uint8_t* in;         // the Cb plane of the launch's first frame; Cr lies plane_bytes behind, the next frame's 2 * plane_bytes
    uint8_t* out;              // the interleaved plane of the launch's first frame
    unsigned long long out_fs, c_rs, plane_bytes;
    int cw;                    // pairs of a row
    int second_first;          // NV21: the pair's first byte comes from the second plane (Cb | Cr -> Cr, Cb)
};

// two neighbouring bytes of a tight plane, at any address
__device__ __forceinline__ uint32_t ycc_load2(const uint8_t* p) {
    if (((uintptr_t)p & 1u) == 0) return *(const uint16_t*)p;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8);
}

// k_rs_ycc_split backwards, under k_rs_unpack_dest's store discipline.  One row of one frame per (blockIdx.y, blockIdx.z).  The
// row's bytes [A, A + 2 cw) are covered by the dwords at dword-aligned addresses inside them, one per thread, and by the up to
// three bytes in front of the first and behind the last of those, one per thread too: nothing outside the row is written,
// whatever the residues of base, pitch and frame stride.  Byte j of the row is component j & 1 of pair j >> 1, so a dword takes
// two neighbouring bytes of each plane; nothing is read outside the row's cw bytes of either plane.
__global__ __launch_bounds__(kRsThreads) void k_rs_ycc_join(RsYccJoin g) {
    uint8_t* row = g.out + blockIdx.z * g.out_fs + blockIdx.y * g.c_rs;
    const uint8_t* const i0 = g.in + blockIdx.z * 2ull * g.plane_bytes + (unsigned long long)blockIdx.y * g.cw;
    const uint8_t* const p0 = g.second_first ? i0 + g.plane_bytes : i0;   // where component 0 of a pair comes from, and component 1
    const uint8_t* const p1 = g.second_first ? i0 : i0 + g.plane_bytes;
    const unsigned len = 2u * (unsigned)g.cw;
    const unsigned to_dword = (unsigned)(-(uintptr_t)row & 3u), head = to_dword < len ? to_dword : len;
    const unsigned nd = (len - head) >> 2, rest = len - head - 4u * nd;
    const unsigned k = blockIdx.x * kRsThreads + threadIdx.x;
    if (k < nd) {
        const unsigned j = head + 4u * k;                                // even or odd, as head is
        const unsigned a = j & 1u;                                       // the component of the dword's bytes 0 and 2
        const uint32_t va = ycc_load2((a ? p1 : p0) + (j >> 1));         // bytes 0, 2: pairs j >> 1 and the next
        const uint32_t vb = ycc_load2((a ? p0 : p1) + ((j + 1u) >> 1));  // bytes 1, 3
        *(uint32_t*)(row + j) = (va & 0xffu) | ((vb & 0xffu) << 8) | ((va & 0xff00u) << 8) | ((vb & 0xff00u) << 16);
    } else if (k < nd + head + rest) {
        const unsigned i = k - nd;
        const unsigned j = i < head ? i : 4u * nd + i;                   // the bytes in front, then those behind
        row[j] = ((j & 1u) ? p1 : p0)[j >> 1];
    }
}

// ---- k_rs_ycc_split16 / k_rs_ycc_join16 --------------------------------------------------------------------------------------

struct RsYcc16Pairs {
    const uint8_t* in;         // split: the interleaved plane of the launch's first frame; join: its first tight plane
    uint8_t* out;              // split: the first tight plane of the launch's first frame; join: its interleaved plane
    unsigned long long fs, c_rs, plane_bytes;   // of the interleaved side: frame stride and row pitch; of the tight side: the
                                                // second plane lies plane_bytes behind the first, the next frame's 2 * plane_bytes
    int cw;                    // pairs of a row
    int second_first;          // the pair's first word belongs to the second tight plane (Cr, Cb <-> Cb | Cr)
};

// One row of one frame per (blockIdx.y, blockIdx.z).  A pair is one dword of the interleaved row and a word of each tight plane.
// The row's words [o, o + cw) of a tight plane (o = row * cw) are covered by the dwords at dword-aligned addresses inside them,
// one per thread -- two pairs -- and by the one word in front of the first and behind the last of those, one per thread too.
// The two pairs of a thread are 8 bytes of the interleaved row at a multiple of 2: one 8-byte access where that address is a
// multiple of 8, two dwords where it is a multiple of 4, and else a word, the dword between the pairs and a word.  Every access
// is naturally aligned and lies inside [row, row + 4 cw), whatever the residues of base, pitch and frame stride.
__device__ __forceinline__ void ycc16_cover(unsigned long long o, unsigned cw, unsigned* head, unsigned* nd, unsigned* rest) {
    *head = (unsigned)(o & 1u);   // cw >= 1
    *nd = (cw - *head) >> 1;
    *rest = cw - *head - 2u * *nd;
}

__global__ __launch_bounds__(kRsThreads) void k_rs_ycc_split16(RsYcc16Pairs g) {
    const uint8_t* const row = g.in + blockIdx.z * g.fs + blockIdx.y * g.c_rs;
    const unsigned cw = (unsigned)g.cw;
    const unsigned long long o = (unsigned long long)blockIdx.y * cw;
    uint16_t* const o0 = (uint16_t*)(g.out + blockIdx.z * 2ull * g.plane_bytes) + o;
    uint16_t* const o1 = (uint16_t*)((uint8_t*)o0 + g.plane_bytes);
    uint16_t* const p0 = g.second_first ? o1 : o0;   // where the first word of a pair goes, and the second
    uint16_t* const p1 = g.second_first ? o0 : o1;
    unsigned head, nd, rest;
    ycc16_cover(o, cw, &head, &nd, &rest);
    const unsigned k = blockIdx.x * kRsThreads + threadIdx.x;
    if (k < nd) {
        const unsigned p = head + 2u * k;   // pairs p and p + 1
        const uint8_t* const a = row + 4ull * p;
        uint32_t d0, d1;
        if (((uintptr_t)a & 7u) == 0) {
            const uint2 v = *(const uint2*)a;
            d0 = v.x, d1 = v.y;
        } else if (((uintptr_t)a & 3u) == 0) {
            d0 = ((const uint32_t*)a)[0], d1 = ((const uint32_t*)a)[1];
        } else {
            const uint32_t lo = *(const uint16_t*)a, mid = *(const uint32_t*)(a + 2), hi = *(const uint16_t*)(a + 6);
            d0 = lo | (mid << 16), d1 = (mid >> 16) | (hi << 16);
        }
        *(uint32_t*)(p0 + p) = (d0 & 0xffffu) | (d1 << 16);
        *(uint32_t*)(p1 + p) = (d0 >> 16) | (d1 & 0xffff0000u);
    } else if (k < nd + head + rest) {
        const unsigned p = k - nd < head ? 0u : cw - 1u;   // the pair in front, then the one behind
        const uint8_t* const a = row + 4ull * p;
        p0[p] = *(const uint16_t*)a;
        p1[p] = *(const uint16_t*)(a + 2);
    }
}

__global__ __launch_bounds__(kRsThreads) void k_rs_ycc_join16(RsYcc16Pairs g) {
    uint8_t* const row = g.out + blockIdx.z * g.fs + blockIdx.y * g.c_rs;
    const unsigned cw = (unsigned)g.cw;
    const unsigned long long o = (unsigned long long)blockIdx.y * cw;
    const uint16_t* const i0 = (const uint16_t*)(g.in + blockIdx.z * 2ull * g.plane_bytes) + o;
    const uint16_t* const i1 = (const uint16_t*)((const uint8_t*)i0 + g.plane_bytes);
    const uint16_t* const p0 = g.second_first ? i1 : i0;   // where the first word of a pair comes from, and the second
    const uint16_t* const p1 = g.second_first ? i0 : i1;
    unsigned head, nd, rest;
    ycc16_cover(o, cw, &head, &nd, &rest);
    const unsigned k = blockIdx.x * kRsThreads + threadIdx.x;
    if (k < nd) {
        const unsigned p = head + 2u * k;
        const uint32_t va = *(const uint32_t*)(p0 + p), vb = *(const uint32_t*)(p1 + p);
        const uint32_t d0 = (va & 0xffffu) | (vb << 16), d1 = (va >> 16) | (vb & 0xffff0000u);
        uint8_t* const a = row + 4ull * p;
        if (((uintptr_t)a & 7u) == 0) {
            *(uint2*)a = make_uint2(d0, d1);
        } else if (((uintptr_t)a & 3u) == 0) {
            ((uint32_t*)a)[0] = d0, ((uint32_t*)a)[1] = d1;
        } else {
            *(uint16_t*)a = (uint16_t)d0;
            *(uint32_t*)(a + 2) = (d0 >> 16) | (d1 << 16);
            *(uint16_t*)(a + 6) = (uint16_t)(d1 >> 16);
        }
    } else if (k < nd + head + rest) {
        const unsigned p = k - nd < head ? 0u : cw - 1u;
        uint8_t* const a = row + 4ull * p;
        *(uint16_t*)a = p0[p];
        *(uint16_t*)(a + 2) = p1[p];
    }
}

// ---- the one launcher of the four ----------------------------------------------------------------------------------------------

// the frame stride of the interleaved side, by the name each parameter block gives it
static unsigned long long& ycc_pairs_fs(RsYccSplit& g) { return g.in_fs; }
static unsigned long long& ycc_pairs_fs(RsYccJoin& g) { return g.out_fs; }
static unsigned long long& ycc_pairs_fs(RsYcc16Pairs& g) { return g.fs; }

// G: the kernel's parameter block -- RsYccSplit, RsYccJoin or RsYcc16Pairs, filled by field name
template <class G>
static hipError_t ycc_pairs_issue(void (*kern)(G), unsigned items, bool split, const uint8_t* in, uint8_t* out, const YccLayout& l,
                                  size_t fs, size_t plane_bytes, int frames, RsIssue& is) {
    G g{};
    ycc_pairs_fs(g) = fs, g.c_rs = l.c_rs, g.plane_bytes = plane_bytes, g.cw = l.cw, g.second_first = l.layout == LANCZOS_YCC_NV21;
    return rs_for_frame_groups(is, frames, [&](int f0, int nf) {
        g.in = in + (size_t)f0 * (split ? fs : 2 * plane_bytes), g.out = out + (size_t)f0 * (split ? 2 * plane_bytes : fs);
        hipLaunchKernelGGL(kern, dim3((items + kRsThreads - 1) / kRsThreads, l.ch, nf), dim3(kRsThreads), 0, is.stream, g);
    });
}

// split: the interleaved chroma rows of layout l (frames fs apart) at `in` into tight pairs of planes at `out`; join: tight
// pairs at `in` into l's rows at `out`.  Samples of B bytes; a thread's items are the dwords of a tight plane's row (8-bit: of
// the interleaved row) and the up to three bytes, or the one word, at either end
static hipError_t ycc_pairs_launch(size_t B, bool split, const uint8_t* in, uint8_t* out, const YccLayout& l, size_t fs,
                                   size_t plane_bytes, int frames, RsIssue& is) {
    if (B == 2)
        return ycc_pairs_issue<RsYcc16Pairs>(split ? k_rs_ycc_split16 : k_rs_ycc_join16, (unsigned)l.cw / 2u + 2u, split, in, out, l, fs,
                                             plane_bytes, frames, is);
    const unsigned items = (2u * (unsigned)l.cw) / 4u + 6u;
    return split ? ycc_pairs_issue<RsYccSplit>(k_rs_ycc_split, items, split, in, out, l, fs, plane_bytes, frames, is)
                 : ycc_pairs_issue<RsYccJoin>(k_rs_ycc_join, items, split, in, out, l, fs, plane_bytes, frames, is);
}

// ---- k_rs_ycc_merge ----------------------------------------------------------------------------------------------------------

struct RsYccMerge {
    const uint8_t *y, *c;                  // the luma plane and the (Cb | Cr) pair of the launch's first frame
    unsigned long long y_fs, c_fs, plane_bytes;   // frames a plane (luma) and a pair (chroma) apart; Cr lies plane_bytes behind Cb
    uint8_t* out;
    unsigned long long out_fs;
    unsigned long long n;                  // pixels of a frame
    const int32_t* table;                  // [3][3][256]
    // tensor elements: the view, as RsToTensorMap has it
    const void* lut;
    long long cs, rs, ps;
    unsigned dst;
    int flip;
    const uint8_t* d_flip;
    int w, h;
};

constexpr int kYccBlock = 4 * kRsThreads;   // pixels per workgroup: one dword of each plane per thread

// (ycc_clip8_shift6, the clamp in front of the shift, is in lanczos_resize.hpp: k_rs_ycc_encode shares it)

// The 9 KiB table goes to LDS once per workgroup; -DLZ_YCC_TABLE_GLOBAL reads it through the caches instead (the A/B of
// DESIGN.md 4.5).  Returns the pointer the conversions index
__device__ __forceinline__ const int32_t* ycc_stage_table(const int32_t* table, int32_t* lds) {
#ifdef LZ_YCC_TABLE_GLOBAL
    (void)lds;
    return table;
#else
    for (int i = threadIdx.x; i < 9 * 256; i += kRsThreads) lds[i] = table[i];
    __syncthreads();
    return lds;
#endif
}

// channel c of the four pixels whose bytes are the dwords y, cb, cr: four result bytes in one dword
__device__ __forceinline__ uint32_t ycc_convert4(const int32_t* t, int c, uint32_t y, uint32_t cb, uint32_t cr) {
    const int32_t *ty = t + (c * 3 + 0) * 256, *tb = t + (c * 3 + 1) * 256, *tr = t + (c * 3 + 2) * 256;
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int sum = ty[(y >> (8 * i)) & 255u] + tb[(cb >> (8 * i)) & 255u] + tr[(cr >> (8 * i)) & 255u];
        r |= ycc_clip8_shift6(sum) << (8 * i);
    }
    return r;
}

// RGB bytes.  A plane is one run of bytes and so is the tight RGB frame: a thread loads one dword of each plane at the same
// offset (4 pixels, coalesced) and stores the three dwords 3 * offset into the frame, which is dword-aligned since the frame
// is.  The pixels behind the last whole group of four go as bytes: nothing is written past 3 n.
__global__ __launch_bounds__(kRsThreads) void k_rs_ycc_merge_bytes(RsYccMerge g) {
    __shared__ int32_t lds[9 * 256];
    const int32_t* t = ycc_stage_table(g.table, lds);
    const unsigned long long mine = (unsigned long long)blockIdx.x * kYccBlock + 4ull * threadIdx.x;
    if (mine >= g.n) return;
    const uint8_t* fy = g.y + blockIdx.y * g.y_fs + mine;
    const uint8_t* fc = g.c + blockIdx.y * g.c_fs + mine;
    const uint32_t y = *(const uint32_t*)fy, cb = *(const uint32_t*)fc, cr = *(const uint32_t*)(fc + g.plane_bytes);
    const uint32_t R = ycc_convert4(t, 0, y, cb, cr), G = ycc_convert4(t, 1, y, cb, cr), B = ycc_convert4(t, 2, y, cb, cr);
    uint8_t* o = g.out + blockIdx.y * g.out_fs + 3ull * mine;
    if (mine + 4 <= g.n) {
        uint32_t* od = (uint32_t*)o;
        od[0] = (R & 0xffu) | ((G & 0xffu) << 8) | ((B & 0xffu) << 16) | ((R & 0xff00u) << 16);
        od[1] = ((G >> 8) & 0xffu) | (((B >> 8) & 0xffu) << 8) | (R & 0xff0000u) | ((G & 0xff0000u) << 8);
        od[2] = ((B >> 16) & 0xffu) | ((R >> 24) << 8) | ((G >> 24) << 16) | ((B >> 24) << 24);
    } else {
        const unsigned left = (unsigned)(g.n - mine);   // 1 .. 3
        for (unsigned i = 0; i < left; i++) {
            o[3 * i + 0] = (uint8_t)(R >> (8 * i));
            o[3 * i + 1] = (uint8_t)(G >> (8 * i));
            o[3 * i + 2] = (uint8_t)(B >> (8 * i));
        }
    }
}

// Tensor elements.  The conversion is the one above; then the wave exchanges its result dwords as k_rs_to_tensor does, so that
// in round r lane i stores pixel 64 r + i of the wave's 256 for every output channel: coalesced where pix_stride is 1.  The
// row of the workgroup's first pixel costs one division, a 64-bit one only for frames of 4 Gi pixels; flips are a base and two
// signed strides from one uniform byte load; a channel nobody names is not stored.  E: the word of an element
template <class E>
__global__ __launch_bounds__(kRsThreads) void k_rs_ycc_merge_tensor(RsYccMerge g) {
    __shared__ int32_t lds[9 * 256];
    const int32_t* t = ycc_stage_table(g.table, lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long base = (unsigned long long)blockIdx.x * kYccBlock;
    const unsigned long long mine = base + 4ull * tid;
    uint32_t y = 0, cb = 0, cr = 0;
    if (mine < g.n) {
        const uint8_t* fy = g.y + blockIdx.y * g.y_fs + mine;
        const uint8_t* fc = g.c + blockIdx.y * g.c_fs + mine;
        y = *(const uint32_t*)fy, cb = *(const uint32_t*)fc, cr = *(const uint32_t*)(fc + g.plane_bytes);
    }
    uint32_t res[3];
#pragma unroll
    for (int c = 0; c < 3; c++) res[c] = ycc_convert4(t, c, y, cb, cr);
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
    for (int rr = 0; rr < 4; rr++) {
        uint32_t px[3];
#pragma unroll
        for (int c = 0; c < 3; c++) px[c] = ((uint32_t)__shfl((int)res[c], 16 * rr + (lane >> 2), 64) >> (8 * (lane & 3))) & 255u;
        const unsigned local = (unsigned)(wave * 256 + 64 * rr + lane);
        if (base + local < g.n) {
            unsigned rem = rem0 + local;   // a row and the block are below 2^17 pixels
            const unsigned dy = rem / w;
            const unsigned x = rem - dy * w;
            const long long at = t_base + (long long)(y0 + dy) * t_rs + (long long)x * t_ps;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const unsigned oc = (g.dst >> (8 * c)) & 255u;
                if (oc < 4) fout[at + (long long)oc * g.cs] = ((const E*)g.lut)[oc * 256 + px[c]];
            }
        }
    }
}

hipError_t ycc_merge_launch(const uint8_t* planes, size_t plane_bytes, uint8_t* out, size_t out_fs, int w, int h,
                            const int32_t* table, const RsTensorOut* t, int frames, RsIssue& is) {
    RsYccMerge g{};
    g.y_fs = plane_bytes, g.c_fs = 2 * plane_bytes, g.plane_bytes = plane_bytes;
    g.out_fs = out_fs, g.n = (unsigned long long)w * h, g.table = table, g.w = w, g.h = h;
    void (*kern)(RsYccMerge) = k_rs_ycc_merge_bytes;
    if (t) {
        g.lut = t->d_lut, g.cs = t->chan_stride, g.rs = t->row_stride, g.ps = t->pix_stride;
        g.dst = t->dst_of_src(), g.flip = t->flip & 3;
        kern = t->elem == 2 ? k_rs_ycc_merge_tensor<uint16_t> : k_rs_ycc_merge_tensor<uint32_t>;
    }
    const unsigned blocks = (unsigned)((g.n + kYccBlock - 1) / kYccBlock);   // at most 2^22
    return rs_for_frame_groups(is, frames, [&](int f0, int nf) {
        g.y = planes + (size_t)f0 * plane_bytes;
        g.c = planes + (size_t)frames * plane_bytes + (size_t)f0 * 2 * plane_bytes;
        g.out = out + (size_t)f0 * out_fs;
        g.d_flip = t && t->d_flip ? t->d_flip + f0 : nullptr;
        hipLaunchKernelGGL(kern, dim3(blocks, nf), dim3(kRsThreads), 0, is.stream, g);
    });
}

// ---- the composition ---------------------------------------------------------------------------------------------------------

static int ycc_hip(YccRequest& q, hipError_t e) {
    if (e == hipSuccess) return LANCZOS_OK;
    *q.last_hip = (int)e;
    return LANCZOS_ERR_HIP;
}

// the bytes of a tight plane of n samples in scratch: a dword multiple
static size_t ycc_plane_bytes(size_t n, size_t B) { return (n * B + 3) & ~(size_t)3; }

// one plane: a one-channel request of q.B-byte samples with a pitched source and a pitched destination (tight rows resolve to
// none: rs_route drops a tight layout before it decides anything)
static int ycc_plane(ResizeState* st, YccRequest& q, const lanczos_resize_desc* d1, const lanczos_resize_opts* o,
                     const lanczos_resize_window* win, size_t in_rs, const uint8_t* in, size_t in_fs, size_t out_rs, uint8_t* out,
                     size_t out_fs, int frames, int* kernel) {
    RsRequest r;
    r.d = d1, r.o = o, r.win = win;
    r.in = in, r.out = out, r.frames = frames, r.in_frame_stride = in_fs, r.out_frame_stride = out_fs, r.stream = q.stream;
    r.last_kernel = kernel, r.last_hip = q.last_hip;
    const lanczos_resize_source src{(int64_t)in_rs, q.B, q.B, {0, 0, 0}};
    const lanczos_resize_dest dst{(int64_t)out_rs, q.B, q.B, {0, 0, 0}};
    r.source = r.dest = true;
    RsWindow w;
    int rc = resize_window_resolve(d1, win, &w);
    if (rc == LANCZOS_OK) rc = resize_source_resolve(d1, &src, &r.sc.s);
    if (rc == LANCZOS_OK) rc = resize_dest_resolve(d1, w, &dst, &r.dc.s);
    if (rc == LANCZOS_OK) rc = resize_device(st, r);
    q.info.launches += r.launches;
    if (rc == LANCZOS_OK && r.copied) *kernel = LANCZOS_KERNEL_NONE;   // a plain copy is no kernel
    return rc;
}

// The planes of YCbCr frames: luma, the split of interleaved chroma, chroma in one call or two, the join of interleaved chroma.
// t: the destination (out_fs its frame stride), whose planes resize_device stores into; NULL for RGB and elements, whose three
// planes go tight into ycc_planes, where the caller's merge reads them
static int ycc_planes_run(ResizeState* st, YccRequest& q, const RsWindow& w, const YccLayout* t, size_t out_fs) {
    const lanczos_resize_desc* const d = q.d;
    const YccLayout& s = q.s;
    const size_t B = (size_t)q.B;
    const int frames = q.frames;
    const size_t in_fs = q.in_frame_stride ? q.in_frame_stride : s.extent;
    if (in_fs < s.extent || (((uintptr_t)q.in | in_fs) & (B - 1)) != 0) return LANCZOS_ERR_BAD_ARG;

    const hipStream_t stream = q.stream;
    RsIssue is{stream};   // the split and the join; the planes' launches come back in RsRequest::launches
    const bool capturing = stream_capturing(stream);
    const size_t plane = ycc_plane_bytes((size_t)w.w * w.h, B);
    const size_t in_plane = ycc_plane_bytes((size_t)s.cw * s.ch, B);
    const size_t out_plane = t ? ycc_plane_bytes((size_t)t->cw * t->ch, B) : plane;
    const bool in_pairs = s.interleaved(), join = t && t->interleaved();
    hipError_t e = hipSuccess;
    if (in_pairs) e = st->ycc_in.reserve(st->life, (size_t)frames * 2 * in_plane, stream, capturing);
    if (e == hipSuccess && join) e = st->ycc_out.reserve(st->life, (size_t)frames * 2 * out_plane, stream, capturing);
    if (e == hipSuccess && !t) e = st->ycc_planes.reserve(st->life, (size_t)frames * 3 * plane, stream, capturing);
    if (e != hipSuccess) return ycc_hip(q, e);

    // the planes' descriptors, boxes and windows: luma is the request with one channel; chroma has its plane's sizes and the box
    // scaled by the source's subsampling on its doubles, which is exact.  Into YCbCr the chroma output is the destination's chroma
    // size and its window the luma window divided by the destination's subsampling; into RGB it is the luma output and window
    lanczos_resize_desc dy = *d, dc = *d;
    dy.channels = dc.channels = 1;
    dc.in_w = s.cw, dc.in_h = s.ch;
    lanczos_resize_opts oc{};
    const double bl[4] = {q.o ? q.o->box[0] : 0.0, q.o ? q.o->box[1] : 0.0, q.o ? q.o->box[2] : (double)d->in_w,
                          q.o ? q.o->box[3] : (double)d->in_h};
    const double kx = s.sx ? 0.5 : 1.0, ky = s.sy ? 0.5 : 1.0;
    oc.box[0] = bl[0] * kx, oc.box[1] = bl[1] * ky, oc.box[2] = bl[2] * kx, oc.box[3] = bl[3] * ky;
    oc.reducing_gap = q.o ? q.o->reducing_gap : 0.0;
    if (q.o) memcpy(oc.reserved, q.o->reserved, sizeof(oc.reserved));   // resize_resolve refuses what is not 0 there
    lanczos_resize_window wc{};
    const lanczos_resize_window* c_win = q.win;
    if (t) {
        dc.out_w = (d->out_w + t->sx) >> t->sx, dc.out_h = (d->out_h + t->sy) >> t->sy;
        wc.x0 = w.x0 >> t->sx, wc.y0 = w.y0 >> t->sy, wc.w = t->cw, wc.h = t->ch;
        c_win = &wc;
    }

    const uint8_t* const in = (const uint8_t*)q.in;
    uint8_t* const out = (uint8_t*)q.out;
    uint8_t* const yo = (uint8_t*)st->ycc_planes.p;   // RGB and elements: the resized planes
    int k_luma = 0, k_chroma = 0;
    int rc = t ? ycc_plane(st, q, &dy, q.o, q.win, s.y_rs, in, in_fs, t->y_rs, out, out_fs, frames, &k_luma)
               : ycc_plane(st, q, &dy, q.o, q.win, s.y_rs, in, in_fs, (size_t)w.w * B, yo, plane, frames, &k_luma);
    if (rc != LANCZOS_OK) return rc;
    // where the chroma planes are read: the caller's, or the split ones, a pair of planes per frame
    const uint8_t *cb_in = in + s.cb_off, *cr_in = in + s.cr_off;
    size_t c_in_rs = s.c_rs, c_in_fs = in_fs;
    if (in_pairs) {
        uint8_t* const split = (uint8_t*)st->ycc_in.p;
        rc = ycc_hip(q, ycc_pairs_launch(B, true, in + s.cb_off, split, s, in_fs, in_plane, frames, is));
        q.info.launches += is.launches, is.launches = 0;   // counted as issued, like the planes': a later failure keeps it
        if (rc != LANCZOS_OK) return rc;
        q.info.split = 1;
        cb_in = split, cr_in = split + in_plane, c_in_rs = (size_t)s.cw * B, c_in_fs = 2 * in_plane;
    }
    // ... and stored: the caller's planes, the tight pairs the join reads, or the tight pairs the merge reads
    uint8_t *cb_out, *cr_out;
    size_t c_out_rs, c_out_fs;
    if (t && !join) cb_out = out + t->cb_off, cr_out = out + t->cr_off, c_out_rs = t->c_rs, c_out_fs = out_fs;
    else if (join) cb_out = (uint8_t*)st->ycc_out.p, cr_out = cb_out + out_plane, c_out_rs = (size_t)t->cw * B, c_out_fs = 2 * out_plane;
    else cb_out = yo + (size_t)frames * plane, cr_out = cb_out + plane, c_out_rs = (size_t)w.w * B, c_out_fs = 2 * plane;
    if (in_pairs && (join || !t)) {   // pairs in, pairs out: one call of 2 * frames frames a plane apart
        rc = ycc_plane(st, q, &dc, &oc, c_win, c_in_rs, cb_in, in_plane, c_out_rs, cb_out, out_plane, 2 * frames, &k_chroma);
    } else {
        rc = ycc_plane(st, q, &dc, &oc, c_win, c_in_rs, cb_in, c_in_fs, c_out_rs, cb_out, c_out_fs, frames, &k_chroma);
        if (rc == LANCZOS_OK) rc = ycc_plane(st, q, &dc, &oc, c_win, c_in_rs, cr_in, c_in_fs, c_out_rs, cr_out, c_out_fs, frames, &k_chroma);
    }
    if (rc != LANCZOS_OK) return rc;
    if (join) {
        rc = ycc_hip(q, ycc_pairs_launch(B, false, (const uint8_t*)st->ycc_out.p, out + t->cb_off, *t, out_fs, out_plane, frames, is));
        q.info.join = 1;
    }
    q.info.launches += is.launches;
    q.info.luma_kernel = k_luma, q.info.chroma_kernel = k_chroma;
    return rc;
}

// Packed RGB bytes into YCbCr frames: the three-channel resize into scratch, then the encode
static int ycc_from_rgb(ResizeState* st, YccRequest& q, const RsWindow& w, const YccLayout& t, size_t out_fs) {
    const lanczos_resize_desc* const d = q.d;
    const int frames = q.frames;
    if ((uintptr_t)q.table & 3) return LANCZOS_ERR_BAD_ARG;
    RsResolved r;
    int rc = resize_resolve(d, q.o, &r);
    if (rc != LANCZOS_OK) return rc;
    const size_t in_frame = (size_t)d->in_w * d->in_h * 3;
    size_t rgb_fs = q.in_frame_stride ? q.in_frame_stride : in_frame;
    if (rgb_fs < in_frame) return LANCZOS_ERR_BAD_ARG;
    const uint8_t* rgb = (const uint8_t*)q.in;
    int k_rgb = LANCZOS_KERNEL_NONE;
    // a request that resizes nothing is a colour conversion of the caller's frames: no copy of them
    if (r.need_h || r.need_v || r.reduces() || !w.whole(d)) {
        const size_t fs = ((size_t)w.w * w.h * 3 + 3) & ~(size_t)3;
        const hipError_t e = st->ycc_rgb.reserve(st->life, (size_t)frames * fs, q.stream, stream_capturing(q.stream));
        if (e != hipSuccess) return ycc_hip(q, e);
        RsRequest rr;
        rr.d = d, rr.o = q.o, rr.win = q.win;
        rr.in = q.in, rr.out = st->ycc_rgb.p, rr.frames = frames, rr.in_frame_stride = rgb_fs, rr.out_frame_stride = fs;
        rr.stream = q.stream, rr.last_kernel = &k_rgb, rr.last_hip = q.last_hip;
        rc = resize_device(st, rr);
        q.info.launches += rr.launches;
        if (rc != LANCZOS_OK) return rc;
        if (rr.copied) k_rgb = LANCZOS_KERNEL_NONE;
        rgb = (const uint8_t*)st->ycc_rgb.p, rgb_fs = fs;
    }
    RsIssue is{q.stream};
    rc = ycc_hip(q, ycc_encode_launch(rgb, rgb_fs, (uint8_t*)q.out, out_fs, t, w.w, w.h, q.table, frames, is));
    q.info.encode = 1, q.info.launches += is.launches;
    q.info.luma_kernel = k_rgb, q.info.chroma_kernel = LANCZOS_KERNEL_NONE;
    return rc;
}

int resize_ycc_device(ResizeState* st, YccRequest& q) {
    RsWindow w;
    int rc = resize_window_resolve(q.d, q.win, &w);
    if (rc != LANCZOS_OK) return rc;
    const size_t B = (size_t)q.B;
    YccLayout t;
    size_t out_fs, out_mask = B - 1;   // samples lie on samples
    if (q.to_ycc()) {
        if ((rc = ycc_layout_resolve(q.dst, w.w, w.h, q.B, q.kind != kYccOutYccFromRgb, w.x0, w.y0, &t)) != LANCZOS_OK) return rc;
        // a destination's frames may overlap each other's padding: the stride has to clear the named bytes only
        out_fs = q.out_frame_stride ? q.out_frame_stride : t.extent;
        if (out_fs < t.named) return LANCZOS_ERR_BAD_ARG;
    } else {
        const size_t rgb = (size_t)w.w * w.h * 3 * B, out_frame = q.tensor() ? tensor_extent_bytes(q.d, w, q.t) : (rgb + 3) & ~(size_t)3;
        out_fs = q.out_frame_stride ? q.out_frame_stride : out_frame;
        if (out_fs < (q.tensor() ? out_frame : rgb)) return LANCZOS_ERR_BAD_ARG;
        // the RGB frames are stored by dwords; element frames lie on multiples of their element
        out_mask = q.tensor() ? (size_t)(q.t.elem - 1) : (size_t)3;
        if (B == 1 && ((uintptr_t)q.table & 3)) return LANCZOS_ERR_BAD_ARG;
    }
    if ((((uintptr_t)q.out | out_fs) & out_mask) != 0) return LANCZOS_ERR_BAD_ARG;
    q.info = YccInfo{};
    if (q.kind == kYccOutYccFromRgb) return ycc_from_rgb(st, q, w, t, out_fs);
    rc = ycc_planes_run(st, q, w, q.to_ycc() ? &t : nullptr, out_fs);
    if (rc != LANCZOS_OK || q.to_ycc()) return rc;
    // RGB and elements: the merge of the three planes, through the table of bytes or the matrix of words
    RsIssue is{q.stream};
    const uint8_t* const planes = (const uint8_t*)st->ycc_planes.p;
    const size_t plane = ycc_plane_bytes((size_t)w.w * w.h, B);
    const RsTensorOut* const view = q.tensor() ? &q.t : nullptr;
    const hipError_t e = B == 1 ? ycc_merge_launch(planes, plane, (uint8_t*)q.out, out_fs, w.w, w.h, q.table, view, q.frames, is)
                                : ycc16_merge_launch(planes, plane, (uint8_t*)q.out, out_fs, w.w, w.h, q.m, view, q.frames, is);
    q.info.merge = 1, q.info.launches += is.launches;
    return ycc_hip(q, e);
}

// The staging of resize_host: the frames, and behind them from the next multiple of 256 bytes on, back to back, what the kernels
// read beside them (the offsets each family had: table, then element table, then flips): the colour table
// of an 8-bit request that has one, the element table of a view and the flips of an element request.  A destination's and a
// tensor's frames go up before they come back, so that what the layout does not name keeps what it held; RGB frames lie back to
// back on the host and a dword multiple apart on the device
int resize_ycc_host(ResizeState* st, YccRequest& q) {
    RsWindow w;
    int rc = resize_window_resolve(q.d, q.win, &w);
    if (rc != LANCZOS_OK) return rc;
    const size_t B = (size_t)q.B, frames = (size_t)q.frames;
    const bool from_rgb = q.kind == kYccOutYccFromRgb, tensor = q.tensor();
    YccLayout t;
    if (q.to_ycc() && (rc = ycc_layout_resolve(q.dst, w.w, w.h, q.B, !from_rgb, w.x0, w.y0, &t)) != LANCZOS_OK) return rc;
    if (q.in_frame_stride || q.out_frame_stride) return LANCZOS_ERR_BAD_ARG;
    if (((uintptr_t)q.in & (B - 1)) != 0 || ((uintptr_t)q.out & (tensor ? (uintptr_t)(q.t.elem - 1) : (uintptr_t)(B - 1))) != 0)
        return LANCZOS_ERR_BAD_ARG;
    const size_t in_bytes = (from_rgb ? (size_t)q.d->in_w * q.d->in_h * 3 : q.s.extent) * frames;
    const size_t rgb = (size_t)w.w * w.h * 3 * B, rgb_fs = (rgb + 3) & ~(size_t)3;
    const bool out_up = q.to_ycc() || tensor;
    const size_t out_bytes = q.to_ycc() ? t.extent * (frames - 1) + t.named : tensor ? tensor_extent_bytes(q.d, w, q.t) * frames : rgb_fs * frames;
    struct Side {
        const void* host;
        size_t bytes, at;
    } sides[3] = {{q.table, B == 1 && q.kind != kYccOutYcc ? (size_t)9 * 256 * 4 : 0, 0},
                  {q.t.d_lut, B == 1 && tensor ? (size_t)q.t.out_channels * 256 * q.t.elem : 0, 0},
                  {q.t.d_flip, tensor && q.t.d_flip ? frames : 0, 0}};
    const Side &table = sides[0], &lut = sides[1], &flips = sides[2];
    size_t need = (in_bytes + 255) & ~(size_t)255;   // the first block on 256 bytes, the others directly behind: both tables
    for (Side& b : sides)                            // are multiples of 256 bytes long
        if (b.bytes) b.at = need, need += b.bytes;
    const hipStream_t stream = q.stream;
    hipError_t e = st->stage_in.reserve(st->life, need, stream, false);   // (the context's own stream: never captured)
    if (e == hipSuccess) e = st->stage_out.reserve(st->life, out_bytes, stream, false);
    uint8_t* const up = (uint8_t*)st->stage_in.p;
    if (e == hipSuccess) e = hipMemcpyAsync(up, q.in, in_bytes, hipMemcpyHostToDevice, stream);
    for (const Side& b : sides)
        if (e == hipSuccess && b.bytes) e = hipMemcpyAsync(up + b.at, b.host, b.bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && out_up) e = hipMemcpyAsync(st->stage_out.p, q.out, out_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        void* const host_out = q.out;
        q.in = up, q.out = st->stage_out.p;
        q.out_frame_stride = out_up ? 0 : rgb_fs;
        if (table.bytes) q.table = (const int32_t*)(up + table.at);
        if (lut.bytes) q.t.d_lut = up + lut.at;
        if (flips.bytes) q.t.d_flip = up + flips.at;
        rc = resize_ycc_device(st, q);
        if (rc == LANCZOS_OK)
            e = out_up ? hipMemcpyAsync(host_out, st->stage_out.p, out_bytes, hipMemcpyDeviceToHost, stream)
                       : hipMemcpy2DAsync(host_out, rgb, st->stage_out.p, rgb_fs, rgb, frames, hipMemcpyDeviceToHost, stream);
    }
    const hipError_t es = hipStreamSynchronize(stream);   // nothing stays in flight on the caller's buffers
    if (rc != LANCZOS_OK) return rc;
    return ycc_hip(q, e != hipSuccess ? e : es);
}

}  // namespace lz
