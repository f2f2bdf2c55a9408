// lanczos_resize_ycc16.hip -- YCbCr frames of 16-bit words (P010, P016, P210, planes of 10 / 12 / 16-bit samples) into wide YCbCr
// frames, packed RGB of 16-bit samples and normalised tensor elements (include/lanczos_hip.h, lanczos_resize_ycc16; DESIGN.md
// 4.5).  The contract is Pillow's mode I;16 on the raw words, plane by plane.  As in lanczos_resize_ycc.hip and
// lanczos_resize_ycc_out.hip nothing here resizes: every plane is a one-channel LANCZOS_RESIZE_U16 request through resize_device
// with a pitched source and, for YCbCr out, a pitched destination.  What is here stands around those calls:
//
//   k_rs_ycc_split16   interleaved chroma of word pairs -> two tight word planes (ResizeState::ycc_in, a pair of planes per frame)
//   k_rs_ycc_join16    two tight word planes (ResizeState::ycc_out) -> pitched interleaved rows: the split backwards
//   k_rs_ycc16_merge   the three resized planes (ResizeState::ycc_planes: `frames` luma planes, then `frames` pairs Cbo | Cro)
//                      through the integer matrix into RGB words, or through it and rs_norm_elem into tensor elements
//
// A plane in scratch holds its words rounded up to a dword multiple, so every plane starts on a dword.  All strides, offsets
// and extents of YccSource / YccDest are bytes; the validators below refuse the odd ones.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "lanczos_resize_fused.hpp"

namespace lz {

// ---- host: validation and the standard matrices ------------------------------------------------------------------------------

int ycc16_desc_validate(const lanczos_resize_desc* d) {
    if (!d) return LANCZOS_ERR_BAD_ARG;
    if (!(d->reserved[0] & LANCZOS_RESIZE_U16) || (d->reserved[0] & (LANCZOS_RESIZE_ALPHA | LANCZOS_RESIZE_F32)))
        return LANCZOS_ERR_UNSUPPORTED;
    const int rc = resize_validate(d);   // (LANCZOS_FILTER_NEAREST on words: LANCZOS_ERR_UNSUPPORTED)
    if (rc != LANCZOS_OK) return rc;
    return d->channels == 3 ? LANCZOS_OK : LANCZOS_ERR_BAD_ARG;
}

// what a source and a destination share: the planes of a w x h luma frame in layout l, in bytes
struct Ycc16Planes {
    long long cw, ch, c_row, b0, b1, r0, r1;
};
template <class L>
static int ycc16_planes(const L* l, long long w, long long h, Ycc16Planes* p) {
    if (!l) return LANCZOS_ERR_BAD_ARG;
    for (int32_t r : l->reserved)
        if (r != 0) return LANCZOS_ERR_BAD_ARG;
    if (l->layout != LANCZOS_YCC_PLANAR && l->layout != LANCZOS_YCC_NV12 && l->layout != LANCZOS_YCC_NV21) return LANCZOS_ERR_BAD_ARG;
    if ((l->sub_x | l->sub_y) & ~1) return LANCZOS_ERR_BAD_ARG;
    const bool nv = l->layout != LANCZOS_YCC_PLANAR;
    if (nv && (l->sub_x != 1 || l->cb_offset != l->cr_offset)) return LANCZOS_ERR_BAD_ARG;
    p->cw = (w + l->sub_x) >> l->sub_x, p->ch = (h + l->sub_y) >> l->sub_y;
    p->c_row = (nv ? 4 : 2) * p->cw;
    const long long cap = (long long)1 << 40;
    if (l->y_row_stride < 2 * w || l->c_row_stride < p->c_row || l->y_row_stride > cap || l->c_row_stride > cap) return LANCZOS_ERR_BAD_ARG;
    if (l->cb_offset < 0 || l->cr_offset < 0 || l->cb_offset > ((long long)1 << 56) || l->cr_offset > ((long long)1 << 56))
        return LANCZOS_ERR_BAD_ARG;
    if ((l->y_row_stride | l->c_row_stride | l->cb_offset | l->cr_offset) & 1) return LANCZOS_ERR_BAD_ARG;   // words lie on words
    // a plane is its pitched rows, all of them, as for the 8-bit layouts
    const long long y_end = h * l->y_row_stride, c_len = p->ch * l->c_row_stride;
    p->b0 = l->cb_offset, p->b1 = p->b0 + c_len, p->r0 = l->cr_offset, p->r1 = p->r0 + c_len;
    if (p->b0 < y_end || p->r0 < y_end) return LANCZOS_ERR_BAD_ARG;                  // a chroma plane inside the luma plane
    if (!nv && p->b0 < p->r1 && p->r0 < p->b1) return LANCZOS_ERR_BAD_ARG;           // Cb over Cr
    return LANCZOS_OK;
}

int ycc16_source_resolve(const lanczos_resize_desc* d, const lanczos_ycc_source* src, YccSource* s) {
    Ycc16Planes p;
    const int rc = ycc16_planes(src, d->in_w, d->in_h, &p);
    if (rc != LANCZOS_OK) return rc;
    s->layout = src->layout, s->sx = src->sub_x, s->sy = src->sub_y, s->cw = (int)p.cw, s->ch = (int)p.ch;
    s->y_rs = (size_t)src->y_row_stride, s->c_rs = (size_t)src->c_row_stride;
    s->cb_off = (size_t)p.b0, s->cr_off = (size_t)p.r0;
    s->extent = (size_t)std::max(p.b1, p.r1);
    return LANCZOS_OK;
}

int ycc16_dest_resolve(const RsWindow& w, const lanczos_ycc_dest* dst, bool aligned_origin, YccDest* s) {
    Ycc16Planes p;
    const int rc = ycc16_planes(dst, w.w, w.h, &p);
    if (rc != LANCZOS_OK) return rc;
    if (aligned_origin && ((w.x0 & dst->sub_x) || (w.y0 & dst->sub_y))) return LANCZOS_ERR_BAD_ARG;   // (a subsampling is 0 or 1)
    s->layout = dst->layout, s->sx = dst->sub_x, s->sy = dst->sub_y, s->cw = (int)p.cw, s->ch = (int)p.ch;
    s->y_rs = (size_t)dst->y_row_stride, s->c_rs = (size_t)dst->c_row_stride;
    s->cb_off = (size_t)p.b0, s->cr_off = (size_t)p.r0;
    s->extent = (size_t)std::max(p.b1, p.r1);
    s->named = (size_t)(std::max(p.b0, p.r0) + (p.ch - 1) * dst->c_row_stride + p.c_row);
    return LANCZOS_OK;
}

int ycc16_matrix_validate(const lanczos_ycc16_matrix* m) {
    if (!m) return LANCZOS_ERR_BAD_ARG;
    for (int c = 0; c < 3; c++) {
        for (int j = 0; j < 3; j++)
            if (m->k[c][j] <= -(1 << 24) || m->k[c][j] >= (1 << 24)) return LANCZOS_ERR_BAD_ARG;
        if (m->sub[c] < 0 || m->sub[c] > 65535) return LANCZOS_ERR_BAD_ARG;
    }
    if (m->shift < 0 || m->shift > 30 || m->max < 0 || m->max > 65535) return LANCZOS_ERR_BAD_ARG;
    for (int32_t r : m->reserved)
        if (r != 0) return LANCZOS_ERR_BAD_ARG;
    return LANCZOS_OK;
}

bool ycc16_matrix_init(lanczos_ycc16_matrix* m, int standard, int depth, bool msb_aligned, bool full_range) {
    double kr, kb;
    if (standard == LANCZOS_YCC_JFIF || standard == LANCZOS_YCC_BT601) kr = 0.299, kb = 0.114;
    else if (standard == LANCZOS_YCC_BT709) kr = 0.2126, kb = 0.0722;
    else if (standard == LANCZOS_YCC_BT2020) kr = 0.2627, kb = 0.0593;
    else return false;
    if (depth < 8 || depth > 16) return false;
    const double kg = 1.0 - kr - kb;
    const double unit = msb_aligned ? (double)(1 << (16 - depth)) : 1.0;
    const double full = (double)((1 << depth) - 1);
    const double ky = 65535.0 / ((full_range ? full : (double)(219 << (depth - 8))) * unit);
    const double kc = 65535.0 / ((full_range ? full : (double)(224 << (depth - 8))) * unit);
    const double real[3][3] = {{ky, 0.0, 2.0 * (1.0 - kr) * kc},
                               {ky, -2.0 * (1.0 - kb) * kb / kg * kc, -2.0 * (1.0 - kr) * kr / kg * kc},
                               {ky, 2.0 * (1.0 - kb) * kc, 0.0}};
    *m = lanczos_ycc16_matrix{};
    // the largest shift that keeps every rounded entry below 2^23 in magnitude
    for (int shift = 30; shift >= 0; shift--) {
        bool fits = true;
        for (int c = 0; c < 3; c++)
            for (int j = 0; j < 3; j++) {
                const long long v = llround(real[c][j] * (double)(1ll << shift));
                if (v <= -(1ll << 23) || v >= (1ll << 23)) fits = false;
                else m->k[c][j] = (int32_t)v;
            }
        if (fits) {
            m->shift = shift;
            break;
        }
        if (shift == 0) return false;   // (no standard gets here: the largest coefficient is below 600)
    }
    m->sub[0] = full_range ? 0 : (int32_t)((16 << (depth - 8)) * unit);
    m->sub[1] = m->sub[2] = (int32_t)((1 << (depth - 1)) * unit);
    m->max = 65535;
    return true;
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

// rows: the chroma rows of a frame.  `tight` is the split's destination or the join's source
static hipError_t ycc16_pairs_launch(bool split, const uint8_t* in, uint8_t* out, size_t fs, size_t c_rs, size_t plane_bytes, int cw,
                                     int rows, bool second_first, int frames, RsIssue& is) {
    RsYcc16Pairs g{};
    g.fs = fs, g.c_rs = c_rs, g.plane_bytes = plane_bytes, g.cw = cw, g.second_first = second_first;
    const unsigned items = (unsigned)cw / 2u + 2u;   // dwords of a plane's row, and at most one word at either end
    return rs_for_frame_groups(is, frames, [&](int f0, int nf) {
        g.in = in + (size_t)f0 * (split ? fs : 2 * plane_bytes), g.out = out + (size_t)f0 * (split ? 2 * plane_bytes : fs);
        hipLaunchKernelGGL(split ? k_rs_ycc_split16 : k_rs_ycc_join16, dim3((items + kRsThreads - 1) / kRsThreads, rows, nf),
                           dim3(kRsThreads), 0, is.stream, g);
    });
}

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

static hipError_t ycc16_merge_launch(const uint8_t* planes, size_t plane_bytes, uint8_t* out, size_t out_fs, int w, int h,
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

// ---- the composition ---------------------------------------------------------------------------------------------------------

static int ycc16_hip(Ycc16Request& q, hipError_t e) {
    if (e == hipSuccess) return LANCZOS_OK;
    *q.last_hip = (int)e;
    return LANCZOS_ERR_HIP;
}

// the bytes of a tight plane of n words in scratch: a dword multiple
static size_t ycc16_plane_bytes(size_t n) { return ((n + 1) & ~(size_t)1) * 2; }

// one plane: a one-channel request of words with a pitched source and a pitched destination (tight rows resolve to none)
static int ycc16_plane(ResizeState* st, Ycc16Request& q, const lanczos_resize_desc* d1, const lanczos_resize_opts* o,
                       const lanczos_resize_window* win, size_t in_rs, const uint8_t* in, size_t in_fs, size_t out_rs, uint8_t* out,
                       size_t out_fs, int frames, int* kernel) {
    RsRequest r;
    r.d = d1, r.o = o, r.win = win;
    r.in = in, r.out = out, r.frames = frames, r.in_frame_stride = in_fs, r.out_frame_stride = out_fs, r.stream = q.stream;
    r.last_kernel = kernel, r.last_hip = q.last_hip;
    const lanczos_resize_source src{(int64_t)in_rs, 2, 2, {0, 0, 0}};
    const lanczos_resize_dest dst{(int64_t)out_rs, 2, 2, {0, 0, 0}};
    r.source = r.dest = true;
    RsWindow w;
    int rc = resize_window_resolve(d1, win, &w);
    if (rc == LANCZOS_OK) rc = resize_source_resolve(d1, &src, &r.sc.s);
    if (rc == LANCZOS_OK) rc = resize_dest_resolve(d1, w, &dst, &r.dc.s);
    if (rc == LANCZOS_OK) rc = resize_device(st, r);
    q.info.launches += r.launches;
    if (rc == LANCZOS_OK && r.copied) *kernel = LANCZOS_KERNEL_NONE;   // lanczos_ycc16_info: a plain copy is no kernel
    return rc;
}

int resize_ycc16_device(ResizeState* st, Ycc16Request& q) {
    const lanczos_resize_desc* const d = q.d;
    const YccSource& s = q.s;
    RsWindow w;
    int rc = resize_window_resolve(d, q.win, &w);
    if (rc != LANCZOS_OK) return rc;
    const int frames = q.frames;
    const bool to_ycc = q.dst != nullptr;
    const size_t in_fs = q.in_frame_stride ? q.in_frame_stride : s.extent;
    if (in_fs < s.extent || (((uintptr_t)q.in | in_fs) & 1) != 0) return LANCZOS_ERR_BAD_ARG;
    YccDest t;
    const size_t px = (size_t)w.w * w.h, plane = ycc16_plane_bytes(px);
    size_t out_fs;
    if (to_ycc) {
        if ((rc = ycc16_dest_resolve(w, q.dst, true, &t)) != LANCZOS_OK) return rc;
        // a destination's frames may overlap each other's padding: the stride has to clear the named bytes only
        out_fs = q.out_frame_stride ? q.out_frame_stride : t.extent;
        if (out_fs < t.named || (((uintptr_t)q.out | out_fs) & 1) != 0) return LANCZOS_ERR_BAD_ARG;
    } else {
        const size_t out_frame = q.tensor ? tensor_extent_bytes(d, w, q.t) : (px * 6 + 3) & ~(size_t)3;
        out_fs = q.out_frame_stride ? q.out_frame_stride : out_frame;
        if (out_fs < (q.tensor ? out_frame : px * 6)) return LANCZOS_ERR_BAD_ARG;
        // the RGB frames are stored by dwords; element frames lie on multiples of their element
        if ((((uintptr_t)q.out | out_fs) & (q.tensor ? (size_t)(q.t.elem - 1) : (size_t)3)) != 0) return LANCZOS_ERR_BAD_ARG;
    }

    const hipStream_t stream = q.stream;
    RsIssue is{stream};   // the split, the join and the merge; the planes' launches come back in RsRequest::launches
    const bool capturing = stream_capturing(stream);
    const size_t in_plane = ycc16_plane_bytes((size_t)s.cw * s.ch);
    const size_t out_plane = to_ycc ? ycc16_plane_bytes((size_t)t.cw * t.ch) : plane;
    const bool in_pairs = s.interleaved(), join = to_ycc && t.interleaved();
    hipError_t e = hipSuccess;
    if (in_pairs) e = st->ycc_in.reserve(st->life, (size_t)frames * 2 * in_plane, stream, capturing);
    if (e == hipSuccess && join) e = st->ycc_out.reserve(st->life, (size_t)frames * 2 * out_plane, stream, capturing);
    if (e == hipSuccess && !to_ycc) e = st->ycc_planes.reserve(st->life, (size_t)frames * 3 * plane, stream, capturing);
    if (e != hipSuccess) return ycc16_hip(q, e);
    q.info = lanczos_ycc16_info{};

    // the planes' descriptors, boxes and windows: luma is the request with one channel; chroma has its plane's sizes and the box
    // scaled by the source's subsampling on its doubles, which is exact.  Into YCbCr the chroma output is the destination's chroma
    // size and its window the luma window divided by the destination's subsampling; into RGB it is the luma output and window
    lanczos_resize_desc dy = *d, dc = *d;
    dy.channels = dc.channels = 1;
    dc.in_w = s.cw, dc.in_h = s.ch;
    if (to_ycc) dc.out_w = (d->out_w + t.sx) >> t.sx, dc.out_h = (d->out_h + t.sy) >> t.sy;
    lanczos_resize_opts oc{};
    const double bl[4] = {q.o ? q.o->box[0] : 0.0, q.o ? q.o->box[1] : 0.0, q.o ? q.o->box[2] : (double)d->in_w,
                          q.o ? q.o->box[3] : (double)d->in_h};
    const double kx = s.sx ? 0.5 : 1.0, ky = s.sy ? 0.5 : 1.0;
    oc.box[0] = bl[0] * kx, oc.box[1] = bl[1] * ky, oc.box[2] = bl[2] * kx, oc.box[3] = bl[3] * ky;
    oc.reducing_gap = q.o ? q.o->reducing_gap : 0.0;
    if (q.o) memcpy(oc.reserved, q.o->reserved, sizeof(oc.reserved));   // resize_resolve refuses what is not 0 there
    lanczos_resize_window wc{};
    wc.x0 = w.x0 >> t.sx, wc.y0 = w.y0 >> t.sy, wc.w = t.cw, wc.h = t.ch;   // (read into YCbCr only)
    const lanczos_resize_window* const c_win = to_ycc ? &wc : q.win;

    const uint8_t* const in = (const uint8_t*)q.in;
    uint8_t* const out = (uint8_t*)q.out;
    uint8_t* const yo = (uint8_t*)st->ycc_planes.p;   // RGB and elements: the resized planes
    int k_luma = 0, k_chroma = 0;
    rc = to_ycc ? ycc16_plane(st, q, &dy, q.o, q.win, s.y_rs, in, in_fs, t.y_rs, out, out_fs, frames, &k_luma)
                : ycc16_plane(st, q, &dy, q.o, q.win, s.y_rs, in, in_fs, (size_t)w.w * 2, yo, plane, frames, &k_luma);
    if (rc != LANCZOS_OK) return rc;
    // where the chroma planes are read: the caller's, or the split ones, a pair of planes per frame
    const uint8_t *cb_in = in + s.cb_off, *cr_in = in + s.cr_off;
    size_t c_in_rs = s.c_rs, c_in_fs = in_fs;
    if (in_pairs) {
        uint8_t* const split = (uint8_t*)st->ycc_in.p;
        rc = ycc16_hip(q, ycc16_pairs_launch(true, in + s.cb_off, split, in_fs, s.c_rs, in_plane, s.cw, s.ch,
                                             s.layout == LANCZOS_YCC_NV21, frames, is));
        q.info.launches += is.launches, is.launches = 0;   // counted as issued, like the planes': a later failure keeps it
        if (rc != LANCZOS_OK) return rc;
        q.info.split = 1;
        cb_in = split, cr_in = split + in_plane, c_in_rs = (size_t)s.cw * 2, c_in_fs = 2 * in_plane;
    }
    // ... and stored: the caller's planes, the tight pairs the join reads, or the tight pairs the merge reads
    uint8_t *cb_out, *cr_out;
    size_t c_out_rs, c_out_fs;
    if (to_ycc && !join) cb_out = out + t.cb_off, cr_out = out + t.cr_off, c_out_rs = t.c_rs, c_out_fs = out_fs;
    else if (join) cb_out = (uint8_t*)st->ycc_out.p, cr_out = cb_out + out_plane, c_out_rs = (size_t)t.cw * 2, c_out_fs = 2 * out_plane;
    else cb_out = yo + (size_t)frames * plane, cr_out = cb_out + plane, c_out_rs = (size_t)w.w * 2, c_out_fs = 2 * plane;
    if (in_pairs && (join || !to_ycc)) {   // pairs in, pairs out: one call of 2 * frames frames a plane apart
        rc = ycc16_plane(st, q, &dc, &oc, c_win, c_in_rs, cb_in, in_plane, c_out_rs, cb_out, out_plane, 2 * frames, &k_chroma);
    } else {
        rc = ycc16_plane(st, q, &dc, &oc, c_win, c_in_rs, cb_in, c_in_fs, c_out_rs, cb_out, c_out_fs, frames, &k_chroma);
        if (rc == LANCZOS_OK) rc = ycc16_plane(st, q, &dc, &oc, c_win, c_in_rs, cr_in, c_in_fs, c_out_rs, cr_out, c_out_fs, frames, &k_chroma);
    }
    if (rc != LANCZOS_OK) return rc;
    if (join) {
        rc = ycc16_hip(q, ycc16_pairs_launch(false, (const uint8_t*)st->ycc_out.p, out + t.cb_off, out_fs, t.c_rs, out_plane, t.cw, t.ch,
                                             t.layout == LANCZOS_YCC_NV21, frames, is));
        q.info.join = 1;
    } else if (!to_ycc) {
        rc = ycc16_hip(q, ycc16_merge_launch(yo, plane, out, out_fs, w.w, w.h, q.m, q.tensor ? &q.t : nullptr, frames, is));
        q.info.merge = 1;
    }
    q.info.launches += is.launches;
    q.info.luma_kernel = k_luma, q.info.chroma_kernel = k_chroma;
    return rc;
}

// The staging of resize_host: the frames, behind them on 256 bytes the flips of a tensor request.  A destination's and a
// tensor's frames go up before they come back, so that what the layout does not name keeps what it held; RGB frames lie back
// to back on the host and a dword multiple apart on the device
int resize_ycc16_host(ResizeState* st, Ycc16Request& q) {
    RsWindow w;
    int rc = resize_window_resolve(q.d, q.win, &w);
    if (rc != LANCZOS_OK) return rc;
    const bool to_ycc = q.dst != nullptr;
    YccDest t;
    if (to_ycc && (rc = ycc16_dest_resolve(w, q.dst, true, &t)) != LANCZOS_OK) return rc;
    if (q.in_frame_stride || q.out_frame_stride) return LANCZOS_ERR_BAD_ARG;
    if (((uintptr_t)q.in & 1) != 0 || ((uintptr_t)q.out & (q.tensor ? (uintptr_t)(q.t.elem - 1) : (uintptr_t)1)) != 0)
        return LANCZOS_ERR_BAD_ARG;
    const size_t frames = (size_t)q.frames, in_bytes = q.s.extent * frames;
    const size_t rgb = (size_t)w.w * w.h * 6, rgb_fs = (rgb + 3) & ~(size_t)3;
    const size_t out_bytes = to_ycc ? t.extent * (frames - 1) + t.named : q.tensor ? tensor_extent_bytes(q.d, w, q.t) * frames : rgb_fs * frames;
    const bool out_up = to_ycc || q.tensor;
    const size_t flips_at = (in_bytes + 255) & ~(size_t)255, flips_bytes = q.tensor && q.t.d_flip ? frames : 0;
    const hipStream_t stream = q.stream;
    hipError_t e = st->stage_in.reserve(st->life, flips_at + flips_bytes, stream, false);   // (the context's own stream: never captured)
    if (e == hipSuccess) e = st->stage_out.reserve(st->life, out_bytes, stream, false);
    uint8_t* const up = (uint8_t*)st->stage_in.p;
    if (e == hipSuccess) e = hipMemcpyAsync(up, q.in, in_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && flips_bytes) e = hipMemcpyAsync(up + flips_at, q.t.d_flip, flips_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && out_up) e = hipMemcpyAsync(st->stage_out.p, q.out, out_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        void* const host_out = q.out;
        q.in = up, q.out = st->stage_out.p;
        q.out_frame_stride = out_up ? 0 : rgb_fs;
        if (flips_bytes) q.t.d_flip = up + flips_at;
        rc = resize_ycc16_device(st, q);
        if (rc == LANCZOS_OK)
            e = out_up ? hipMemcpyAsync(host_out, st->stage_out.p, out_bytes, hipMemcpyDeviceToHost, stream)
                       : hipMemcpy2DAsync(host_out, rgb, st->stage_out.p, rgb_fs, rgb, frames, hipMemcpyDeviceToHost, stream);
    }
    const hipError_t es = hipStreamSynchronize(stream);   // nothing stays in flight on the caller's buffers
    if (rc != LANCZOS_OK) return rc;
    return ycc16_hip(q, e != hipSuccess ? e : es);
}

}  // namespace lz
