// lanczos_resize_ycc.hip -- YCbCr frames (I420, 4:2:2 and 4:4:4 planes, NV12, NV21) into RGB bytes and tensor elements
// (include/lanczos_hip.h, lanczos_resize_ycc_*).  The contract is Pillow's: every plane resized as an "L" image
// (chroma with the box scaled to its plane), Image.merge("YCbCr", ...) and convert("RGB").  Nothing here resizes: the planes go
// through resize_device as one-channel requests with a pitched source, so rs_route decides for each of them what it decides for
// any one-channel frame.  What is here is what stands around those calls:
//
//   k_rs_ycc_split   NV12 / NV21 only: the interleaved chroma plane of every frame into tight Cb and Cr planes (ResizeState::
//                    ycc_in, 2 * frames one-channel frames a plane apart), so that the chroma resize is one call.
//   k_rs_ycc_merge   the three resized planes (ResizeState::ycc_planes) through the colour table into interleaved RGB bytes, or
//                    through it and the element table of a view into float32 / 16-bit tensor elements.  Modelled on
//                    k_rs_to_tensor_map (lanczos_resize_tensor.hip).
//
// ycc_planes holds `frames` luma planes and behind them `frames` pairs (Cbo | Cro), every plane rounded up to a dword multiple:
// a planar source stores its chroma with two calls a pair apart, split chroma with one call of 2 * frames frames a plane apart.
// The standard colour tables and the validation of a lanczos_ycc_source are here as well.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "lanczos_resize.hpp"

namespace lz {

// ---- host: validation and the standard tables --------------------------------------------------------------------------------

int ycc_desc_validate(const lanczos_resize_desc* d) {
    if (!d) return LANCZOS_ERR_BAD_ARG;
    if (d->reserved[0] & (LANCZOS_RESIZE_ALPHA | LANCZOS_RESIZE_U16 | LANCZOS_RESIZE_F32)) return LANCZOS_ERR_UNSUPPORTED;
    const int rc = resize_validate(d);
    if (rc != LANCZOS_OK) return rc;
    return d->channels == 3 ? LANCZOS_OK : LANCZOS_ERR_BAD_ARG;
}

int ycc_source_resolve(const lanczos_resize_desc* d, const lanczos_ycc_source* src, YccSource* s) {
    if (!src) return LANCZOS_ERR_BAD_ARG;
    for (int32_t r : src->reserved)
        if (r != 0) return LANCZOS_ERR_BAD_ARG;
    if (src->layout != LANCZOS_YCC_PLANAR && src->layout != LANCZOS_YCC_NV12 && src->layout != LANCZOS_YCC_NV21)
        return LANCZOS_ERR_BAD_ARG;
    if ((src->sub_x | src->sub_y) & ~1) return LANCZOS_ERR_BAD_ARG;
    const bool nv = src->layout != LANCZOS_YCC_PLANAR;
    if (nv && (src->sub_x != 1 || src->cb_offset != src->cr_offset)) return LANCZOS_ERR_BAD_ARG;
    const long long cw = (d->in_w + src->sub_x) >> src->sub_x, ch = (d->in_h + src->sub_y) >> src->sub_y;
    const long long c_row = nv ? 2 * cw : cw, cap = (long long)1 << 40;
    if (src->y_row_stride < d->in_w || src->c_row_stride < c_row || src->y_row_stride > cap || src->c_row_stride > cap)
        return LANCZOS_ERR_BAD_ARG;
    if (src->cb_offset < 0 || src->cr_offset < 0 || src->cb_offset > ((long long)1 << 56) || src->cr_offset > ((long long)1 << 56))
        return LANCZOS_ERR_BAD_ARG;
    // a plane is its pitched rows, all of them: the resize kernels' range checks cover whole rows
    const long long y_end = d->in_h * src->y_row_stride, c_len = ch * src->c_row_stride;
    const long long b0 = src->cb_offset, b1 = b0 + c_len, r0 = src->cr_offset, r1 = r0 + c_len;
    if (b0 < y_end || r0 < y_end) return LANCZOS_ERR_BAD_ARG;                 // a chroma plane inside the luma plane
    if (!nv && b0 < r1 && r0 < b1) return LANCZOS_ERR_BAD_ARG;                // Cb over Cr
    s->layout = src->layout, s->sx = src->sub_x, s->sy = src->sub_y, s->cw = (int)cw, s->ch = (int)ch;
    s->y_rs = (size_t)src->y_row_stride, s->c_rs = (size_t)src->c_row_stride;
    s->cb_off = (size_t)b0, s->cr_off = (size_t)r0;
    s->extent = (size_t)std::max(b1, r1);
    return LANCZOS_OK;
}

// (int)(k * (i - off) * 64 + 0.5): in double, truncated toward zero, as Pillow's ImagingConvertYCbCr2RGB tables are built
static int32_t ycc_entry(double k, int i, int off) { return (int32_t)(k * (i - off) * 64 + 0.5); }

bool ycc_table(int standard, int32_t* t) {
    double ky = 1.0, r_cr, g_cb, g_cr, b_cb;
    int y_off = 0, y_add = 0;
    if (standard == LANCZOS_YCC_JFIF) {
        r_cr = 1.402, g_cb = -0.34414, g_cr = -0.71414, b_cb = 1.772;
    } else if (standard == LANCZOS_YCC_BT601 || standard == LANCZOS_YCC_BT709) {
        const double kr = standard == LANCZOS_YCC_BT601 ? 0.299 : 0.2126, kb = standard == LANCZOS_YCC_BT601 ? 0.114 : 0.0722;
        const double kg = 1.0 - kr - kb, kc = 255.0 / 224.0;
        ky = 255.0 / 219.0, y_off = 16, y_add = 32;
        r_cr = 2.0 * (1.0 - kr) * kc, b_cb = 2.0 * (1.0 - kb) * kc;
        g_cb = -2.0 * (1.0 - kb) * kb / kg * kc, g_cr = -2.0 * (1.0 - kr) * kr / kg * kc;
    } else {
        return false;
    }
    const double k[3][2] = {{0.0, r_cr}, {g_cb, g_cr}, {b_cb, 0.0}};   // [c][cb, cr]
    for (int c = 0; c < 3; c++)
        for (int i = 0; i < 256; i++) {
            // the full-range luma entry is 64 i exactly; a limited-range one carries the + 32 that makes the shift round
            t[(c * 3 + 0) * 256 + i] = standard == LANCZOS_YCC_JFIF ? 64 * i : ycc_entry(ky, i, y_off) + y_add;
            t[(c * 3 + 1) * 256 + i] = k[c][0] == 0.0 ? 0 : ycc_entry(k[c][0], i, 128);
            t[(c * 3 + 2) * 256 + i] = k[c][1] == 0.0 ? 0 : ycc_entry(k[c][1], i, 128);
        }
    return true;
}

// ---- k_rs_ycc_split ----------------------------------------------------------------------------------------------------------

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

hipError_t ycc_split_launch(const uint8_t* in, size_t in_fs, const YccSource& s, uint8_t* out, size_t plane_bytes, int frames,
                            RsIssue& is) {
    RsYccSplit g{};
    g.in_fs = in_fs, g.c_rs = s.c_rs, g.plane_bytes = plane_bytes, g.cw = s.cw, g.second_first = s.layout == LANCZOS_YCC_NV21;
    const unsigned items = (2u * (unsigned)s.cw) / 4u + 6u;   // dwords, and at most three bytes at either end
    return rs_for_frame_groups(is, frames, [&](int f0, int nf) {
        g.in = in + (size_t)f0 * in_fs, g.out = out + (size_t)f0 * 2 * plane_bytes;
        hipLaunchKernelGGL(k_rs_ycc_split, dim3((items + kRsThreads - 1) / kRsThreads, s.ch, nf), dim3(kRsThreads), 0, is.stream, g);
    });
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

static hipError_t ycc_merge_launch(const uint8_t* planes, size_t plane_bytes, uint8_t* out, size_t out_fs, int w, int h,
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

// one plane: a one-channel request with a pitched source into ycc_planes
static int ycc_plane(ResizeState* st, YccRequest& q, const lanczos_resize_desc* d1, const lanczos_resize_opts* o, size_t row_stride,
                     const uint8_t* in, size_t in_fs, uint8_t* out, size_t out_fs, int frames, int* kernel) {
    RsRequest r;
    r.d = d1, r.o = o, r.win = q.win;
    r.in = in, r.out = out, r.frames = frames, r.in_frame_stride = in_fs, r.out_frame_stride = out_fs, r.stream = q.stream;
    r.last_kernel = kernel, r.last_hip = q.last_hip;
    const lanczos_resize_source src{(int64_t)row_stride, 1, 1, {0, 0, 0}};
    r.source = true;
    int rc = resize_source_resolve(d1, &src, &r.sc.s);
    if (rc == LANCZOS_OK) rc = resize_device(st, r);
    q.info.launches += r.launches;
    if (rc == LANCZOS_OK && r.copied) *kernel = LANCZOS_KERNEL_NONE;   // lanczos_ycc_info: a plain copy is no kernel
    return rc;
}

int resize_ycc_device(ResizeState* st, YccRequest& q) {
    const lanczos_resize_desc* const d = q.d;
    const YccSource& s = q.s;
    RsWindow w;
    int rc = resize_window_resolve(d, q.win, &w);
    if (rc != LANCZOS_OK) return rc;
    const int frames = q.frames;
    const size_t in_fs = q.in_frame_stride ? q.in_frame_stride : s.extent;
    const size_t px = (size_t)w.w * w.h, plane = (px + 3) & ~(size_t)3;
    const size_t out_frame = q.tensor ? tensor_extent_bytes(d, w, q.t) : (px * 3 + 3) & ~(size_t)3;
    const size_t out_fs = q.out_frame_stride ? q.out_frame_stride : out_frame;
    if (in_fs < s.extent || out_fs < (q.tensor ? out_frame : px * 3)) return LANCZOS_ERR_BAD_ARG;
    // the RGB frames are stored by dwords; element frames lie on multiples of their element
    if ((((uintptr_t)q.out | out_fs) & (q.tensor ? (size_t)(q.t.elem - 1) : (size_t)3)) != 0) return LANCZOS_ERR_BAD_ARG;
    if ((uintptr_t)q.table & 3) return LANCZOS_ERR_BAD_ARG;

    const hipStream_t stream = q.stream;
    RsIssue is{stream};   // the split and the merge; the planes' launches come back in RsRequest::launches
    const bool capturing = stream_capturing(stream);
    const size_t c_plane = ((size_t)s.cw * s.ch + 3) & ~(size_t)3;
    hipError_t e = st->ycc_planes.reserve(st->life, (size_t)frames * 3 * plane, stream, capturing);
    if (e == hipSuccess && s.interleaved()) e = st->ycc_in.reserve(st->life, (size_t)frames * 2 * c_plane, stream, capturing);
    if (e != hipSuccess) return ycc_hip(q, e);
    q.info = lanczos_ycc_info{};

    // the three planes' descriptors and boxes: luma is the request with one channel, chroma has its plane's size and the box
    // scaled on its doubles, which is exact
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

    const uint8_t* in = (const uint8_t*)q.in;
    uint8_t* const yo = (uint8_t*)st->ycc_planes.p;
    uint8_t* const co = yo + (size_t)frames * plane;
    int k_luma = 0, k_chroma = 0;
    rc = ycc_plane(st, q, &dy, q.o, s.y_rs, in, in_fs, yo, plane, frames, &k_luma);
    if (rc != LANCZOS_OK) return rc;
    if (s.interleaved()) {
        uint8_t* const split = (uint8_t*)st->ycc_in.p;
        rc = ycc_hip(q, ycc_split_launch(in + s.cb_off, in_fs, s, split, c_plane, frames, is));
        q.info.launches += is.launches, is.launches = 0;   // counted as issued, like the planes': a later failure keeps it
        if (rc != LANCZOS_OK) return rc;
        q.info.split = 1;
        rc = ycc_plane(st, q, &dc, &oc, (size_t)s.cw, split, c_plane, co, plane, 2 * frames, &k_chroma);
    } else {
        rc = ycc_plane(st, q, &dc, &oc, s.c_rs, in + s.cb_off, in_fs, co, 2 * plane, frames, &k_chroma);
        if (rc == LANCZOS_OK) rc = ycc_plane(st, q, &dc, &oc, s.c_rs, in + s.cr_off, in_fs, co + plane, 2 * plane, frames, &k_chroma);
    }
    if (rc != LANCZOS_OK) return rc;
    rc = ycc_hip(q, ycc_merge_launch(yo, plane, (uint8_t*)q.out, out_fs, w.w, w.h, q.table, q.tensor ? &q.t : nullptr, frames, is));
    q.info.launches += is.launches;
    q.info.luma_kernel = k_luma, q.info.chroma_kernel = k_chroma;
    return rc;
}

// The staging of resize_host: the frames, behind them on 256 bytes the colour table, of a tensor request its element table and
// its flips; element frames go up before they come back, so that what the view does not name keeps what it held.  RGB frames
// lie back to back on the host and a dword multiple apart on the device
int resize_ycc_host(ResizeState* st, YccRequest& q) {
    RsWindow w;
    const int rc0 = resize_window_resolve(q.d, q.win, &w);
    if (rc0 != LANCZOS_OK) return rc0;
    const size_t frames = (size_t)q.frames, in_bytes = q.s.extent * frames;
    const size_t rgb = (size_t)w.w * w.h * 3, rgb_fs = (rgb + 3) & ~(size_t)3;
    const size_t ext = q.tensor ? tensor_extent_bytes(q.d, w, q.t) : 0;
    if (q.tensor && ((uintptr_t)q.out & (uintptr_t)(q.t.elem - 1)) != 0) return LANCZOS_ERR_BAD_ARG;
    const size_t out_bytes = q.tensor ? ext * frames : rgb_fs * frames;
    const size_t table_at = (in_bytes + 255) & ~(size_t)255, table_bytes = 9 * 256 * 4;
    const size_t lut_at = table_at + table_bytes, lut_bytes = q.tensor ? (size_t)q.t.out_channels * 256 * q.t.elem : 0;
    const size_t flips_at = lut_at + lut_bytes, flips_bytes = q.tensor && q.t.d_flip ? frames : 0;
    const hipStream_t stream = q.stream;
    hipError_t e = st->stage_in.reserve(st->life, flips_at + flips_bytes, stream, false);   // (the context's own stream: never captured)
    if (e == hipSuccess) e = st->stage_out.reserve(st->life, out_bytes, stream, false);
    uint8_t* const up = (uint8_t*)st->stage_in.p;
    if (e == hipSuccess) e = hipMemcpyAsync(up, q.in, in_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(up + table_at, q.table, table_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && lut_bytes) e = hipMemcpyAsync(up + lut_at, q.t.d_lut, lut_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && flips_bytes) e = hipMemcpyAsync(up + flips_at, q.t.d_flip, flips_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && q.tensor) e = hipMemcpyAsync(st->stage_out.p, q.out, out_bytes, hipMemcpyHostToDevice, stream);
    int rc = LANCZOS_OK;
    if (e == hipSuccess) {
        void* const host_out = q.out;
        q.in = up, q.out = st->stage_out.p, q.table = (const int32_t*)(up + table_at);
        q.in_frame_stride = 0, q.out_frame_stride = q.tensor ? 0 : rgb_fs;
        if (lut_bytes) q.t.d_lut = up + lut_at;
        if (flips_bytes) q.t.d_flip = up + flips_at;
        rc = resize_ycc_device(st, q);
        if (rc == LANCZOS_OK)
            e = q.tensor ? hipMemcpyAsync(host_out, st->stage_out.p, out_bytes, hipMemcpyDeviceToHost, stream)
                         : hipMemcpy2DAsync(host_out, rgb, st->stage_out.p, rgb_fs, rgb, frames, hipMemcpyDeviceToHost, stream);
    }
    const hipError_t es = hipStreamSynchronize(stream);   // nothing stays in flight on the caller's buffers
    if (rc != LANCZOS_OK) return rc;
    return ycc_hip(q, e != hipSuccess ? e : es);
}

}  // namespace lz
