// lanczos_resize_ycc_out.hip -- resize INTO YCbCr frames (I420, 4:2:2 and 4:4:4 planes, NV12, NV21) from YCbCr frames or from
// packed RGB bytes (include/lanczos_hip.h, lanczos_resize_ycc_out).  The mirror of lanczos_resize_ycc.hip, and as
// there nothing here resizes: the planes, or the RGB frames, go through resize_device.
//
//   from YCbCr   luma and planar chroma are one-channel requests with a pitched source and a pitched destination: the caller's
//                planes are what resize_device stores into.  Interleaved chroma in is split by k_rs_ycc_split (ResizeState::
//                ycc_in); for interleaved chroma out the two planes go tight into ResizeState::ycc_out, `frames` pairs (Cb | Cr)
//                of planes rounded up to a dword multiple, and
//   k_rs_ycc_join   interleaves every pair into the pitched rows of the destination: k_rs_ycc_split backwards.
//   from RGB     the three-channel request stores tight RGB into ResizeState::ycc_rgb (a request that resizes nothing is not
//                issued at all: the caller's frames are read), and
//   k_rs_ycc_encode   converts through the forward table, averages the chroma blocks and stores Y rows and chroma planes or
//                interleaved chroma rows, in one pass.
// The validation of a lanczos_ycc_dest and the standard forward tables are here as well.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "lanczos_resize.hpp"

namespace lz {

// ---- host: validation and the standard tables --------------------------------------------------------------------------------

int ycc_dest_resolve(const RsWindow& w, const lanczos_ycc_dest* dst, bool aligned_origin, YccDest* s) {
    if (!dst) return LANCZOS_ERR_BAD_ARG;
    for (int32_t r : dst->reserved)
        if (r != 0) return LANCZOS_ERR_BAD_ARG;
    if (dst->layout != LANCZOS_YCC_PLANAR && dst->layout != LANCZOS_YCC_NV12 && dst->layout != LANCZOS_YCC_NV21)
        return LANCZOS_ERR_BAD_ARG;
    if ((dst->sub_x | dst->sub_y) & ~1) return LANCZOS_ERR_BAD_ARG;
    const bool nv = dst->layout != LANCZOS_YCC_PLANAR;
    if (nv && (dst->sub_x != 1 || dst->cb_offset != dst->cr_offset)) return LANCZOS_ERR_BAD_ARG;
    if (aligned_origin && ((w.x0 & dst->sub_x) || (w.y0 & dst->sub_y))) return LANCZOS_ERR_BAD_ARG;   // (a subsampling is 0 or 1)
    const long long cw = (w.w + dst->sub_x) >> dst->sub_x, ch = (w.h + dst->sub_y) >> dst->sub_y;
    const long long c_row = nv ? 2 * cw : cw, cap = (long long)1 << 40;
    if (dst->y_row_stride < w.w || dst->c_row_stride < c_row || dst->y_row_stride > cap || dst->c_row_stride > cap)
        return LANCZOS_ERR_BAD_ARG;
    if (dst->cb_offset < 0 || dst->cr_offset < 0 || dst->cb_offset > ((long long)1 << 56) || dst->cr_offset > ((long long)1 << 56))
        return LANCZOS_ERR_BAD_ARG;
    // a plane is its pitched rows, all of them, as a source's is
    const long long y_end = w.h * dst->y_row_stride, c_len = ch * dst->c_row_stride;
    const long long b0 = dst->cb_offset, b1 = b0 + c_len, r0 = dst->cr_offset, r1 = r0 + c_len;
    if (b0 < y_end || r0 < y_end) return LANCZOS_ERR_BAD_ARG;                 // a chroma plane inside the luma plane
    if (!nv && b0 < r1 && r0 < b1) return LANCZOS_ERR_BAD_ARG;                // Cb over Cr
    s->layout = dst->layout, s->sx = dst->sub_x, s->sy = dst->sub_y, s->cw = (int)cw, s->ch = (int)ch;
    s->y_rs = (size_t)dst->y_row_stride, s->c_rs = (size_t)dst->c_row_stride;
    s->cb_off = (size_t)b0, s->cr_off = (size_t)r0;
    s->extent = (size_t)std::max(b1, r1);
    s->named = (size_t)(std::max(b0, r0) + (ch - 1) * dst->c_row_stride + c_row);
    return LANCZOS_OK;
}

// (int)(k * i * 64 + 0.5): in double, truncated toward zero, as Pillow's ImagingConvertRGB2YCbCr tables are built
static int32_t ycc_forward_entry(double k, int i) { return (int32_t)(k * i * 64 + 0.5); }

bool ycc_table_forward(int standard, int32_t* t) {
    double k[3][3];
    int add[3];
    if (standard == LANCZOS_YCC_JFIF) {
        const double jfif[3][3] = {{0.299, 0.587, 0.114}, {-0.16874, -0.33126, 0.5}, {0.5, -0.41869, -0.08131}};
        memcpy(k, jfif, sizeof(k));
        add[0] = 0, add[1] = add[2] = 128 * 64;
    } else if (standard == LANCZOS_YCC_BT601 || standard == LANCZOS_YCC_BT709) {
        const double kr = standard == LANCZOS_YCC_BT601 ? 0.299 : 0.2126, kb = standard == LANCZOS_YCC_BT601 ? 0.114 : 0.0722;
        const double kg = 1.0 - kr - kb, sy = 219.0 / 255.0, sc = 224.0 / 255.0;
        const double ub = 2.0 * (1.0 - kb), ur = 2.0 * (1.0 - kr);
        const double m[3][3] = {{kr * sy, kg * sy, kb * sy}, {-kr / ub * sc, -kg / ub * sc, 0.5 * sc}, {0.5 * sc, -kg / ur * sc, -kb / ur * sc}};
        memcpy(k, m, sizeof(k));
        add[0] = 16 * 64 + 32, add[1] = add[2] = 128 * 64 + 32;   // the + 32 makes the shift round
    } else {
        return false;
    }
    for (int c = 0; c < 3; c++)
        for (int j = 0; j < 3; j++)
            for (int i = 0; i < 256; i++) t[(c * 3 + j) * 256 + i] = ycc_forward_entry(k[c][j], i) + (j == 0 ? add[c] : 0);
    return true;
}

// ---- k_rs_ycc_join -----------------------------------------------------------------------------------------------------------

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

static hipError_t ycc_join_launch(const uint8_t* in, size_t plane_bytes, uint8_t* out, size_t out_fs, const YccDest& t, int frames,
                                  RsIssue& is) {
    RsYccJoin g{};
    g.out_fs = out_fs, g.c_rs = t.c_rs, g.plane_bytes = plane_bytes, g.cw = t.cw, g.second_first = t.layout == LANCZOS_YCC_NV21;
    const unsigned items = (2u * (unsigned)t.cw) / 4u + 6u;   // dwords, and at most three bytes at either end
    return rs_for_frame_groups(is, frames, [&](int f0, int nf) {
        g.in = in + (size_t)f0 * 2 * plane_bytes, g.out = out + (size_t)f0 * out_fs;
        hipLaunchKernelGGL(k_rs_ycc_join, dim3((items + kRsThreads - 1) / kRsThreads, t.ch, nf), dim3(kRsThreads), 0, is.stream, g);
    });
}

// ---- k_rs_ycc_encode ---------------------------------------------------------------------------------------------------------

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

static hipError_t ycc_encode_launch(const uint8_t* in, size_t in_fs, uint8_t* out, size_t out_fs, const YccDest& t, int w, int h,
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

// ---- the composition ---------------------------------------------------------------------------------------------------------

static int ycc_out_hip(YccOutRequest& q, hipError_t e) {
    if (e == hipSuccess) return LANCZOS_OK;
    *q.last_hip = (int)e;
    return LANCZOS_ERR_HIP;
}

// one plane: a one-channel request with a pitched source and a pitched destination
static int ycc_out_plane(ResizeState* st, YccOutRequest& q, const lanczos_resize_desc* d1, const lanczos_resize_opts* o,
                         const lanczos_resize_window* win, size_t in_rs, const uint8_t* in, size_t in_fs, size_t out_rs, uint8_t* out,
                         size_t out_fs, int frames, int* kernel) {
    RsRequest r;
    r.d = d1, r.o = o, r.win = win;
    r.in = in, r.out = out, r.frames = frames, r.in_frame_stride = in_fs, r.out_frame_stride = out_fs, r.stream = q.stream;
    r.last_kernel = kernel, r.last_hip = q.last_hip;
    const lanczos_resize_source src{(int64_t)in_rs, 1, 1, {0, 0, 0}};
    const lanczos_resize_dest dst{(int64_t)out_rs, 1, 1, {0, 0, 0}};
    r.source = r.dest = true;
    RsWindow w;
    int rc = resize_window_resolve(d1, win, &w);
    if (rc == LANCZOS_OK) rc = resize_source_resolve(d1, &src, &r.sc.s);
    if (rc == LANCZOS_OK) rc = resize_dest_resolve(d1, w, &dst, &r.dc.s);
    if (rc == LANCZOS_OK) rc = resize_device(st, r);
    q.info.launches += r.launches;
    if (rc == LANCZOS_OK && r.copied) *kernel = LANCZOS_KERNEL_NONE;   // lanczos_ycc_out_info: a plain copy is no kernel
    return rc;
}

static int ycc_out_from_ycc(ResizeState* st, YccOutRequest& q, const RsWindow& w, const YccDest& t, size_t out_fs) {
    const lanczos_resize_desc* const d = q.d;
    const YccSource& s = q.s;
    const int frames = q.frames;
    const size_t in_fs = q.in_frame_stride ? q.in_frame_stride : s.extent;
    if (in_fs < s.extent) return LANCZOS_ERR_BAD_ARG;
    const hipStream_t stream = q.stream;
    RsIssue is{stream};   // the split and the join; the planes' launches come back in RsRequest::launches
    const bool capturing = stream_capturing(stream);
    const size_t in_plane = ((size_t)s.cw * s.ch + 3) & ~(size_t)3, out_plane = ((size_t)t.cw * t.ch + 3) & ~(size_t)3;
    hipError_t e = hipSuccess;
    if (s.interleaved()) e = st->ycc_in.reserve(st->life, (size_t)frames * 2 * in_plane, stream, capturing);
    if (e == hipSuccess && t.interleaved()) e = st->ycc_out.reserve(st->life, (size_t)frames * 2 * out_plane, stream, capturing);
    if (e != hipSuccess) return ycc_out_hip(q, e);

    // the planes' descriptors, boxes and windows: luma is the request with one channel; chroma has its plane's sizes, the box
    // scaled by the source's subsampling on its doubles, which is exact, and the window divided by the destination's
    lanczos_resize_desc dy = *d, dc = *d;
    dy.channels = dc.channels = 1;
    dc.in_w = s.cw, dc.in_h = s.ch;
    dc.out_w = (d->out_w + t.sx) >> t.sx, dc.out_h = (d->out_h + t.sy) >> t.sy;
    lanczos_resize_opts oc{};
    const double bl[4] = {q.o ? q.o->box[0] : 0.0, q.o ? q.o->box[1] : 0.0, q.o ? q.o->box[2] : (double)d->in_w,
                          q.o ? q.o->box[3] : (double)d->in_h};
    const double kx = s.sx ? 0.5 : 1.0, ky = s.sy ? 0.5 : 1.0;
    oc.box[0] = bl[0] * kx, oc.box[1] = bl[1] * ky, oc.box[2] = bl[2] * kx, oc.box[3] = bl[3] * ky;
    oc.reducing_gap = q.o ? q.o->reducing_gap : 0.0;
    if (q.o) memcpy(oc.reserved, q.o->reserved, sizeof(oc.reserved));   // resize_resolve refuses what is not 0 there
    lanczos_resize_window wc{};
    wc.x0 = w.x0 >> t.sx, wc.y0 = w.y0 >> t.sy, wc.w = t.cw, wc.h = t.ch;

    const uint8_t* const in = (const uint8_t*)q.in;
    uint8_t* const out = (uint8_t*)q.out;
    int k_luma = 0, k_chroma = 0;
    int rc = ycc_out_plane(st, q, &dy, q.o, q.win, s.y_rs, in, in_fs, t.y_rs, out, out_fs, frames, &k_luma);
    if (rc != LANCZOS_OK) return rc;
    // where the chroma planes are read: the caller's, or the split ones, a pair of planes per frame
    const uint8_t *cb_in = in + s.cb_off, *cr_in = in + s.cr_off;
    size_t c_in_rs = s.c_rs, c_in_fs = in_fs;
    if (s.interleaved()) {
        uint8_t* const split = (uint8_t*)st->ycc_in.p;
        rc = ycc_out_hip(q, ycc_split_launch(in + s.cb_off, in_fs, s, split, in_plane, frames, is));
        q.info.launches += is.launches, is.launches = 0;   // counted as issued, like the planes': a later failure keeps it
        if (rc != LANCZOS_OK) return rc;
        q.info.split = 1;
        cb_in = split, cr_in = split + in_plane, c_in_rs = (size_t)s.cw, c_in_fs = 2 * in_plane;
    }
    // ... and stored: the caller's, or the tight pairs the join reads
    uint8_t *cb_out = out + t.cb_off, *cr_out = out + t.cr_off;
    size_t c_out_rs = t.c_rs, c_out_fs = out_fs;
    if (t.interleaved()) cb_out = (uint8_t*)st->ycc_out.p, cr_out = cb_out + out_plane, c_out_rs = (size_t)t.cw, c_out_fs = 2 * out_plane;
    if (s.interleaved() && t.interleaved()) {   // pairs in, pairs out: one call of 2 * frames frames a plane apart
        rc = ycc_out_plane(st, q, &dc, &oc, &wc, c_in_rs, cb_in, in_plane, c_out_rs, cb_out, out_plane, 2 * frames, &k_chroma);
    } else {
        rc = ycc_out_plane(st, q, &dc, &oc, &wc, c_in_rs, cb_in, c_in_fs, c_out_rs, cb_out, c_out_fs, frames, &k_chroma);
        if (rc == LANCZOS_OK) rc = ycc_out_plane(st, q, &dc, &oc, &wc, c_in_rs, cr_in, c_in_fs, c_out_rs, cr_out, c_out_fs, frames, &k_chroma);
    }
    if (rc != LANCZOS_OK) return rc;
    if (t.interleaved()) {
        rc = ycc_out_hip(q, ycc_join_launch((const uint8_t*)st->ycc_out.p, out_plane, out + t.cb_off, out_fs, t, frames, is));
        q.info.join = 1;
    }
    q.info.launches += is.launches;
    q.info.luma_kernel = k_luma, q.info.chroma_kernel = k_chroma;
    return rc;
}

static int ycc_out_from_rgb(ResizeState* st, YccOutRequest& q, const RsWindow& w, const YccDest& t, size_t out_fs) {
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
        if (e != hipSuccess) return ycc_out_hip(q, e);
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
    rc = ycc_out_hip(q, ycc_encode_launch(rgb, rgb_fs, (uint8_t*)q.out, out_fs, t, w.w, w.h, q.table, frames, is));
    q.info.encode = 1, q.info.launches += is.launches;
    q.info.luma_kernel = k_rgb, q.info.chroma_kernel = LANCZOS_KERNEL_NONE;
    return rc;
}

int resize_ycc_out_device(ResizeState* st, YccOutRequest& q) {
    RsWindow w;
    int rc = resize_window_resolve(q.d, q.win, &w);
    if (rc != LANCZOS_OK) return rc;
    YccDest t;
    if ((rc = ycc_dest_resolve(w, q.dst, !q.from_rgb, &t)) != LANCZOS_OK) return rc;
    // a destination's frames may overlap each other's padding: the stride has to clear the named bytes only
    const size_t out_fs = q.out_frame_stride ? q.out_frame_stride : t.extent;
    if (out_fs < t.named) return LANCZOS_ERR_BAD_ARG;
    q.info = lanczos_ycc_out_info{};
    return q.from_rgb ? ycc_out_from_rgb(st, q, w, t, out_fs) : ycc_out_from_ycc(st, q, w, t, out_fs);
}

// The staging of resize_host: the frames, behind them on 256 bytes the forward table of an RGB request; the destination's frames
// go up before they come back, so that what the layout does not name keeps what it held
int resize_ycc_out_host(ResizeState* st, YccOutRequest& q) {
    RsWindow w;
    int rc = resize_window_resolve(q.d, q.win, &w);
    if (rc != LANCZOS_OK) return rc;
    YccDest t;
    if ((rc = ycc_dest_resolve(w, q.dst, !q.from_rgb, &t)) != LANCZOS_OK) return rc;
    if (q.in_frame_stride || q.out_frame_stride) return LANCZOS_ERR_BAD_ARG;
    const size_t frames = (size_t)q.frames;
    const size_t in_bytes = (q.from_rgb ? (size_t)q.d->in_w * q.d->in_h * 3 : q.s.extent) * frames;
    const size_t out_bytes = t.extent * (frames - 1) + t.named;
    const size_t table_at = (in_bytes + 255) & ~(size_t)255, table_bytes = q.from_rgb ? 9 * 256 * 4 : 0;
    const hipStream_t stream = q.stream;
    hipError_t e = st->stage_in.reserve(st->life, table_at + table_bytes, stream, false);   // (the context's own stream: never captured)
    if (e == hipSuccess) e = st->stage_out.reserve(st->life, out_bytes, stream, false);
    uint8_t* const up = (uint8_t*)st->stage_in.p;
    if (e == hipSuccess) e = hipMemcpyAsync(up, q.in, in_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && table_bytes) e = hipMemcpyAsync(up + table_at, q.table, table_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(st->stage_out.p, q.out, out_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        void* const host_out = q.out;
        q.in = up, q.out = st->stage_out.p;
        if (table_bytes) q.table = (const int32_t*)(up + table_at);
        rc = resize_ycc_out_device(st, q);
        if (rc == LANCZOS_OK) e = hipMemcpyAsync(host_out, st->stage_out.p, out_bytes, hipMemcpyDeviceToHost, stream);
    }
    const hipError_t es = hipStreamSynchronize(stream);   // nothing stays in flight on the caller's buffers
    if (rc != LANCZOS_OK) return rc;
    return ycc_out_hip(q, e != hipSuccess ? e : es);
}

}  // namespace lz
