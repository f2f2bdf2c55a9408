// lanczos_resize.hip -- resize to any size, downscaling included, with Pillow's contract (include/lanczos_hip.h,
// lanczos_resize_*).  The per-context cache of the tap tables, the context scratch, the executor of a route
// (resize_device) and the host entry points; the tables themselves, the planning and the route (rs_route) are host code without
// a device, in lanczos_resize_route.cpp.  The kernels are templates over the sample width (RsSample<BPS>, lanczos_resize_fused.hpp); there are two paths:
//
//   fused     k_rs_fused: a workgroup owns a strip of output columns (all channels) of one frame and a chunk of its output
//             rows.  It marches down the rows in blocks of kRsOB: the input rows the block's vertical taps need are staged
//             in LDS (buffer loads, range-checked zero fill), the horizontal pass turns them into rows of an LDS ring, stored
//             as Pillow stores its intermediate, and the vertical pass reads the ring and stores the block's output rows.
//             Horizontal coefficients stay in registers for the whole march (a thread keeps one output column); vertical
//             ones are workgroup-uniform scalar loads.
//   two-pass  k_rs_pass_h writes the intermediate (the rows the vertical taps read x out_w x C per frame) to context
//             scratch, k_rs_pass_v reads it: any tap count, every sample width, all compiled here.  It also serves a resize
//             that changes one axis only (one kernel) -- as Pillow, a pass whose axis keeps its size is skipped.  And it alone
//             serves the frames Pillow resizes in the other order (rs_vertical_first: more than 100 times as tall as wide and
//             shrinking in height): k_rs_pass_v first, over the full width, into scratch of out_h rows, then k_rs_pass_h.
//
// LANCZOS_RESIZE_ALPHA (four channels, Pillow's RGBA mode): both paths premultiply the colour samples by alpha where they
// read the frame and divide alpha out where they write it (lanczos_alpha.hpp), the ALPHA instances of k_rs_fused and
// k_rs_h_alpha / k_rs_v_alpha; tables, plan and scratch are those of the same request without the flag.
//
// LANCZOS_RESIZE_U16 (16-bit samples, Pillow's I;16) and LANCZOS_RESIZE_F32 (float samples, Pillow's mode F): the same tap
// geometry with double coefficients (one set of tables and cache entries for both) and Pillow's double accumulation; a u16 or
// float intermediate.
//
// A source box (lanczos_resize_opts) only changes the tables: an axis is built over a span of the source given as two floats,
// `first` still indexes the whole axis, and the kernels are the ones above.  reducing_gap puts lanczos_reduce.hip in front:
// reduce into context scratch, then the resize of the reduced frames with the box that remains (resize_resolve).
//
// A window of the output (lanczos_resize_window) changes no table and no kernel: the tables stay those of the full axes, cached
// under the full axes' keys, and every launch gets them from the window's first output on, with the window's extent as its
// output size.  Plan, scratch and output strides follow the window.  Only the request that changes neither axis has device
// code of its own for it, the crop copy k_rs_crop (lanczos_resize_nearest.hip).
//
// A crop origin per frame (lanczos_resize_crops, tensor requests only) is a window whose size is known here and whose origin
// only the kernels see: the fused plan is the largest over every origin (rs_fused_plan_crops), the crops instances of k_rs_fused
// move their table pointers by the frame's origin, and every other route resizes the whole output and lets
// k_rs_to_tensor_crops gather the windows (lanczos_resize_tensor_crops.hip).
//
// A source layout (lanczos_resize_source: planar frames, pitched rows) changes where a source byte is fetched from and nothing
// else: the fused kernel reads such frames as they lie (a pitch is one of its arguments; planar frames have staging loads and
// instances of their own), every other route gets them packed into context scratch by
// k_rs_pack_source first (lanczos_resize_source.hip).
//
// A destination layout (lanczos_resize_dest: planar frames, pitched rows) changes where a result byte is stored and nothing
// else: the fused kernel stores pitched interleaved rows itself (a pitch is one of its arguments) and planes through an epilogue
// and instances of their own, every other route stores the packed result in context scratch and
// k_rs_unpack_dest scatters it (lanczos_resize_dest.hip).
//
// The arithmetic is Pillow's and exact by construction; RsSample<BPS> says how for each width.
#include "lanczos_resize.hpp"

#include "lanczos_alpha.hpp"
#include "lanczos_resize_fused.hpp"
#include "lanczos_env.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

namespace lz {

// ---- kernels -----------------------------------------------------------------------------------------------------

// LANCZOS_RESIZE_ALPHA on the two-pass path: one thread per four-channel pixel, so that a colour sample has its alpha next
// to it.  The horizontal kernel premultiplies what it reads; with UN (no vertical pass follows) it also divides alpha out
// of what it writes, otherwise the intermediate holds premultiplied pixels.  The vertical kernel divides alpha out of what
// it writes; with PRE (no horizontal pass ran) it premultiplies what it reads.  Frames may start at any byte: byte accesses.
__device__ __forceinline__ uint32_t rs_load_px(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ __forceinline__ void rs_store_px(uint8_t* p, uint32_t v) {
#pragma unroll
    for (int b = 0; b < 4; b++) p[b] = (uint8_t)(v >> (8 * b));
}
__device__ __forceinline__ void rs_mad_px(uint32_t px, int k, int (&acc)[4]) {
#pragma unroll
    for (int b = 0; b < 4; b++) acc[b] = RsSample<1>::mad(RsSample<1>::get(px, b), k, acc[b]);
}
__device__ __forceinline__ uint32_t rs_clip_px(const int (&acc)[4]) {
    using S = RsSample<1>;
    return S::store(acc[0]) | (S::store(acc[1]) << 8) | (S::store(acc[2]) << 16) | (S::store(acc[3]) << 24);
}

template <bool UN>
__global__ __launch_bounds__(kRsThreads) void k_rs_h_alpha(RsPass<int32_t> p) {
    const int o = blockIdx.x * kRsThreads + threadIdx.x;   // output pixel of row blockIdx.y (n_cols counts samples)
    if (o * 4 >= p.n_cols) return;
    const int f = p.first[o], n = p.count[o];
    const uint8_t* src = p.src + blockIdx.z * p.src_fs + blockIdx.y * p.src_pitch + (size_t)f * 4;
    const int32_t* k = p.coeffs + (size_t)o * p.ksize;
    int acc[4] = {1 << (kResizePrecision - 1), 1 << (kResizePrecision - 1), 1 << (kResizePrecision - 1),
                  1 << (kResizePrecision - 1)};
#pragma unroll 4
    for (int i = 0; i < n; i++) rs_mad_px(rs_premul_px(rs_load_px(src + (size_t)i * 4)), k[i], acc);
    const uint32_t px = rs_clip_px(acc);
    rs_store_px(p.dst + blockIdx.z * p.dst_fs + blockIdx.y * p.dst_pitch + (size_t)o * 4, UN ? rs_unpremul_px(px) : px);
}

template <bool PRE>
__global__ __launch_bounds__(kRsThreads) void k_rs_v_alpha(RsPass<int32_t> p) {
    const int x = blockIdx.x * kRsThreads + threadIdx.x;   // pixel column
    if (x * 4 >= p.n_cols) return;
    const int o = blockIdx.y;
    const int f = p.first[o], n = p.count[o];
    const int32_t* k = p.coeffs + (size_t)o * p.ksize;
    const uint8_t* src = p.src + blockIdx.z * p.src_fs + (size_t)f * p.src_pitch + (size_t)x * 4;
    int acc[4] = {1 << (kResizePrecision - 1), 1 << (kResizePrecision - 1), 1 << (kResizePrecision - 1),
                  1 << (kResizePrecision - 1)};
#pragma unroll 4
    for (int i = 0; i < n; i++) {
        const uint32_t px = rs_load_px(src + (size_t)i * p.src_pitch);
        rs_mad_px(PRE ? rs_premul_px(px) : px, k[i], acc);
    }
    rs_store_px(p.dst + blockIdx.z * p.dst_fs + o * p.dst_pitch + (size_t)x * 4, rs_unpremul_px(rs_clip_px(acc)));
}

// The other order (rs_vertical_first): the vertical pass runs first and premultiplies what it reads into an intermediate of
// premultiplied pixels, the horizontal pass runs last and divides alpha out of what it writes.
__global__ __launch_bounds__(kRsThreads) void k_rs_v_alpha_first(RsPass<int32_t> p) {
    const int x = blockIdx.x * kRsThreads + threadIdx.x;   // pixel column
    if (x * 4 >= p.n_cols) return;
    const int o = blockIdx.y;
    const int f = p.first[o], n = p.count[o];
    const int32_t* k = p.coeffs + (size_t)o * p.ksize;
    const uint8_t* src = p.src + blockIdx.z * p.src_fs + (size_t)f * p.src_pitch + (size_t)x * 4;
    int acc[4] = {1 << (kResizePrecision - 1), 1 << (kResizePrecision - 1), 1 << (kResizePrecision - 1),
                  1 << (kResizePrecision - 1)};
#pragma unroll 4
    for (int i = 0; i < n; i++) rs_mad_px(rs_premul_px(rs_load_px(src + (size_t)i * p.src_pitch)), k[i], acc);
    rs_store_px(p.dst + blockIdx.z * p.dst_fs + o * p.dst_pitch + (size_t)x * 4, rs_clip_px(acc));
}

__global__ __launch_bounds__(kRsThreads) void k_rs_h_alpha_last(RsPass<int32_t> p) {
    const int o = blockIdx.x * kRsThreads + threadIdx.x;   // output pixel of row blockIdx.y (n_cols counts samples)
    if (o * 4 >= p.n_cols) return;
    const int f = p.first[o], n = p.count[o];
    const uint8_t* src = p.src + blockIdx.z * p.src_fs + blockIdx.y * p.src_pitch + (size_t)f * 4;
    const int32_t* k = p.coeffs + (size_t)o * p.ksize;
    int acc[4] = {1 << (kResizePrecision - 1), 1 << (kResizePrecision - 1), 1 << (kResizePrecision - 1),
                  1 << (kResizePrecision - 1)};
#pragma unroll 4
    for (int i = 0; i < n; i++) rs_mad_px(rs_load_px(src + (size_t)i * 4), k[i], acc);
    rs_store_px(p.dst + blockIdx.z * p.dst_fs + blockIdx.y * p.dst_pitch + (size_t)o * 4, rs_unpremul_px(rs_clip_px(acc)));
}

// ---- host side: cache, planning, launch ---------------------------------------------------------------------------

// The tables of one axis shape, built and uploaded on first use: first | count | coeffs in one block.  The upload is eager, so
// an entry is valid from the moment it is cached.  The call's use of the tables on `stream` is noted on the entry.
static int rs_axis(ResizeState* st, int in_n, int out_n, int a, int filter, RsSpan span, bool f64, hipStream_t stream,
                   bool capturing, ResizeAxis** out, int* last_hip) {
    ResizeAxisKey key;
    memset(&key, 0, sizeof(key));
    key.in_n = in_n, key.out_n = out_n, key.a = a, key.f64 = (int)f64, key.filter = filter;
    memcpy(&key.span_bits[0], &span.b0, 4);
    memcpy(&key.span_bits[1], &span.b1, 4);
    ResizeState::AxisCache::Item* it = st->axes.find(key);
    if (!it) {
        ResizeAxis ax;
        if (!resize_build_axis(in_n, out_n, a, filter, span, &ax.host, f64)) return LANCZOS_ERR_UNSUPPORTED;
        const ResizeAxisHost& h = ax.host;
        std::vector<int32_t> block((size_t)2 * h.out_n + h.coeffs.size() + 2 * h.coeffs64.size());
        memcpy(block.data(), h.first.data(), (size_t)h.out_n * 4);
        memcpy(block.data() + h.out_n, h.count.data(), (size_t)h.out_n * 4);
        if (f64) memcpy(block.data() + 2 * (size_t)h.out_n, h.coeffs64.data(), h.coeffs64.size() * 8);
        else memcpy(block.data() + 2 * (size_t)h.out_n, h.coeffs.data(), h.coeffs.size() * 4);
        hipError_t e = hipSuccess;
        it = st->axes.insert(key, std::move(ax), block.data(), block.size() * 4, stream, Upload::eager, &e);
        if (!it) {
            *last_hip = (int)e;
            return LANCZOS_ERR_HIP;
        }
        it->dev = (const int32_t*)it->dev_block;
    }
    (void)st->axes.use(it, stream, capturing);   // (an eager entry has no upload to wait for: nothing here can fail)
    *out = it;
    return LANCZOS_OK;
}


// One pass of the two-pass path over `rows` rows of `n_cols` samples of `bps` bytes; src / dst row pitches in samples, frame
// strides in bytes.  alpha: the LANCZOS_RESIZE_ALPHA kernels (8-bit, a thread per pixel); `only`: the other pass does not run.
// o0: the output of the axis the pass starts at (a window); the kernels count their outputs from it
// v_first: both passes run, the vertical one first (rs_vertical_first); it only changes which alpha kernel a pass is
static hipError_t rs_launch_pass(int bps, bool horizontal, const ResizeAxis* ax, int o0, int channels, const uint8_t* src, size_t src_fs,
                                 size_t src_pitch, uint8_t* dst, size_t dst_fs, size_t dst_pitch, int n_cols, int rows, int frames,
                                 RsIssue& is, bool alpha, bool only, bool v_first = false) {
    if (alpha && bps != 1) return hipErrorInvalidValue;
    auto run = [&](auto sample) {
        using S = decltype(sample);
        RsPass<typename S::coeff_t> p{};
        p.src_fs = src_fs, p.dst_fs = dst_fs, p.src_pitch = src_pitch, p.dst_pitch = dst_pitch;
        p.n_cols = n_cols, p.channels = channels;
        p.ksize = ax->host.ksize;
        p.first = ax->first() + o0, p.count = ax->count() + o0;
        p.coeffs = ax->coeffs<typename S::coeff_t>() + (size_t)o0 * p.ksize;
        void (*kern)(RsPass<typename S::coeff_t>) = horizontal ? k_rs_pass_h<S> : k_rs_pass_v<S>;
        if constexpr (S::BPS == 1) {   // alpha is 8-bit only (checked above)
            if (alpha && v_first) kern = horizontal ? k_rs_h_alpha_last : k_rs_v_alpha_first;
            else if (alpha && horizontal) kern = only ? k_rs_h_alpha<true> : k_rs_h_alpha<false>;
            else if (alpha) kern = only ? k_rs_v_alpha<true> : k_rs_v_alpha<false>;
        }
        return rs_for_frame_groups(is, frames, [&](int f0, int nf) {
            p.src = src + (size_t)f0 * src_fs;
            p.dst = dst + (size_t)f0 * dst_fs;
            const int n_threads = alpha ? n_cols / 4 : n_cols;
            hipLaunchKernelGGL(kern, dim3((n_threads + kRsThreads - 1) / kRsThreads, rows, nf), dim3(kRsThreads), 0, is.stream, p);
        });
    };
    return bps == 4 ? run(RsSample<4>()) : bps == 2 ? run(RsSample<2>()) : run(RsSample<1>());
}

// the instance of the fused kernel a route names: a case per entry of LZ_RS_FUSED_INSTANCES
static hipError_t rs_launch_fused_any(int bps, int flags, const RsFusedLaunch& c) {
    switch (bps << 12 | flags) {
#define X(I, BPS, FLAGS) \
    case (BPS) << 12 | (FLAGS): return rs_launch_fused<BPS, FLAGS>(c);
        LZ_RS_FUSED_INSTANCES(X)
#undef X
        default: return hipErrorInvalidValue;
    }
}

// Resolve, check strides and alignment, get the tables, ask rs_route, grow the scratch it names, and issue what it lists in its
// order: pack, reduce, main, follower or unpack.  No decision is taken here
int resize_device(ResizeState* st, RsRequest& q) {
    const lanczos_resize_desc* const d0 = q.d;
    RsResolved r;
    RsWindow w;
    int rc = resize_resolve(d0, q.o, &r);
    if (rc == LANCZOS_OK) rc = resize_window_resolve(d0, q.win, &w);
    if (rc != LANCZOS_OK) return rc;
    const int C = d0->channels, frames = q.frames;
    const size_t B = (size_t)resize_bps(d0);   // bytes per sample
    const hipStream_t stream = q.stream;
    if (q.tensor) q.tc.extent_bytes = tensor_extent_bytes(d0, w, q.tc.t);
    const size_t in_frame = q.source ? q.sc.s.extent : (size_t)d0->in_w * d0->in_h * C * B;
    const size_t out_frame = q.tensor ? q.tc.extent_bytes : q.dest ? q.dc.s.extent : (size_t)w.w * w.h * C * B;
    size_t in_fs = q.in_frame_stride ? q.in_frame_stride : in_frame;
    const size_t out_fs = q.out_frame_stride ? q.out_frame_stride : out_frame;
    // a destination's frames may overlap each other's padding: the stride has to clear the named bytes only
    if (in_fs < in_frame || out_fs < (q.dest ? q.dc.s.named : out_frame)) return LANCZOS_ERR_BAD_ARG;
    // samples lie on multiples of their width; the frames of a tensor request hold elements, which lie on multiples of theirs
    if ((((uintptr_t)q.in | in_fs) & (B - 1)) != 0) return LANCZOS_ERR_BAD_ARG;
    if ((((uintptr_t)q.out | out_fs) & (q.tensor ? (size_t)(q.tc.t.elem - 1) : B - 1)) != 0) return LANCZOS_ERR_BAD_ARG;

    // the tables: of an axis that runs, and both index tables of the gather
    const lanczos_resize_desc* const d = &r.inner;   // the frames the resize reads: the caller's, or the reduced ones
    const int filter = resize_filter(d);
    const bool tables_of_both = filter == LANCZOS_FILTER_NEAREST && (r.need_h || r.need_v);
    const bool capturing = stream_capturing(stream);
    ResizeAxis *H = nullptr, *V = nullptr;
    if ((r.need_h || tables_of_both) &&
        (rc = rs_axis(st, d->in_w, d->out_w, d->a, filter, r.h, B > 1, stream, capturing, &H, q.last_hip)) != LANCZOS_OK)
        return rc;
    if ((r.need_v || tables_of_both) &&
        (rc = rs_axis(st, d->in_h, d->out_h, d->a, filter, r.v, B > 1, stream, capturing, &V, q.last_hip)) != LANCZOS_OK)
        return rc;

    RsRouteQuery rq;
    rq.d = d0, rq.r = &r, rq.win = w, rq.frames = frames, rq.force = st->force;
    rq.tensor = q.tensor, rq.mapped = q.tc.t.mapped, rq.crops = q.tensor && q.tc.d_origin, rq.elem = q.tc.t.elem;
    rq.extent_bytes = q.tc.extent_bytes, rq.norm = q.tensor && q.tc.t.norm;
    rq.src = q.source ? &q.sc.s : nullptr, rq.dst = q.dest ? &q.dc.s : nullptr;
    rq.H = H ? &H->host : nullptr, rq.V = V ? &V->host : nullptr;
    const RsRoute rt = rs_route(rq);
    if (rt.err != LANCZOS_OK) return rt.err;
    int rb[4];
    const int32_t box[4] = {r.rb[0], r.rb[1], r.rb[2], r.rb[3]};
    if (rt.reduce && (rc = reduce_validate(d0->in_w, d0->in_h, C, r.fx, r.fy, box, rb)) != LANCZOS_OK) return rc;
    const struct {
        ScratchBlock* blk;
        size_t bytes;
    } blocks[5] = {{&st->packed, rt.packed.bytes},     {&st->reduced, rt.reduced.bytes}, {&st->tensor_bytes, rt.tensor_bytes.bytes},
                   {&st->unpacked, rt.unpacked.bytes}, {&st->scratch, rt.scratch.bytes}};
    for (const auto& b : blocks) {
        const hipError_t ge = b.bytes ? b.blk->reserve(st->life, b.bytes, stream, capturing) : hipSuccess;
        if (ge != hipSuccess) {
            *q.last_hip = (int)ge;
            return LANCZOS_ERR_HIP;
        }
    }

    const uint8_t* in = (const uint8_t*)q.in;
    hipError_t e = hipSuccess;
    RsIssue is{stream};   // every launch below goes out through it and is counted where it does
    if (rt.pack) {
        e = rs_pack_source_launch(in, in_fs, q.sc.s, (uint8_t*)st->packed.p, rt.packed.fs, d0->in_w, d0->in_h, C, (int)B, frames, is);
        in = (const uint8_t*)st->packed.p, in_fs = rt.packed.fs;
    }
    if (rt.reduce && e == hipSuccess) {   // reducing_gap: reduce into context scratch, then resize the reduced frames
        e = reduce_launch(in, (uint8_t*)st->reduced.p, d0->in_w, C, r.fx, r.fy, rb, frames, in_fs, rt.reduced.fs, is);
        in = (const uint8_t*)st->reduced.p, in_fs = rt.reduced.fs;
    }
    if (e != hipSuccess) {
        q.launches = is.launches;
        *q.last_hip = (int)e;
        return LANCZOS_ERR_HIP;
    }
    // where the main step stores: the caller's frames, or the packed bytes a follower or the unpack reads
    uint8_t* out = (uint8_t*)q.out;
    size_t step_fs = out_fs;
    if (rt.tensor_bytes.bytes) out = (uint8_t*)st->tensor_bytes.p, step_fs = rt.tensor_bytes.fs;
    if (rt.unpacked.bytes) out = (uint8_t*)st->unpacked.p, step_fs = rt.unpacked.fs;
    const RsWindow& win = rt.win;
    const bool alpha = (d->reserved[0] & LANCZOS_RESIZE_ALPHA) != 0;
    const size_t px = (size_t)C * B, in_pitch = (size_t)d->in_w * px;
    const int in_cols = d->in_w * C, out_cols = win.w * C;   // samples of a row
    uint8_t* const mid = (uint8_t*)st->scratch.p;            // the intermediate of two passes
    switch (rt.main) {
        case kRsMainFused: {
            const RsFusedLaunch c{d, win, &rt.fp, H, V, in, out, in_fs, step_fs, frames, q.tensor ? &q.tc : nullptr, is,
                                  rt.src_direct ? &q.sc.s : nullptr, rt.dst_direct ? &q.dc.s : nullptr};
            e = rs_launch_fused_any(rt.bps, rt.flags, c);
            break;
        }
        case kRsMainNearest:
            e = rs_nearest_launch(in, out, d->in_w, win.w, win.h, C, (int)B, H->first() + win.x0, V->first() + win.y0, frames, in_fs,
                                  step_fs, is);
            break;
        case kRsMainNone: break;   // nothing to copy: the gather below reads the caller's frames
        case kRsMainCopy:
            e = hipMemcpy2DAsync(out, step_fs, in, in_fs, (size_t)d->in_h * in_pitch, frames, hipMemcpyDeviceToDevice, stream);
            if (e == hipSuccess) is.launches++;
            break;
        case kRsMainCrop:
            e = rs_crop_launch(in + (size_t)win.y0 * in_pitch + (size_t)win.x0 * px, out, in_pitch, (size_t)win.w * px, win.h, frames,
                               in_fs, step_fs, is);
            break;
        case kRsMainVFirst:
            // The vertical pass turns the window's rows of the source's full width (Pillow's, and at most 655 pixels) into win.h
            // rows of context scratch, stored as every intermediate is; the horizontal pass reads them through the window's slice
            // of its table, whose `first` indexes that full width, and writes the output.
            e = rs_launch_pass((int)B, false, V, win.y0, C, in, in_fs, in_cols, mid, rt.scratch.fs, in_cols, in_cols, win.h, frames,
                               is, alpha, false, true);
            if (e == hipSuccess)
                e = rs_launch_pass((int)B, true, H, win.x0, C, mid, rt.scratch.fs, in_cols, out, step_fs, out_cols, out_cols, win.h,
                                   frames, is, alpha, false, true);
            break;
        case kRsMainPassH:   // the window's rows, which are the source's
            e = rs_launch_pass((int)B, true, H, win.x0, C, in + (size_t)win.y0 * in_pitch, in_fs, in_cols, out, step_fs, out_cols,
                               out_cols, win.h, frames, is, alpha, true);
            break;
        case kRsMainPassV:   // the window's columns of the source's full rows
            e = rs_launch_pass((int)B, false, V, win.y0, C, in + (size_t)win.x0 * px, in_fs, in_cols, out, step_fs, out_cols, out_cols,
                               win.h, frames, is, alpha, true);
            break;
        case kRsMainTwoPass: {
            // the scratch holds rows mid_row0 .. mid_row0 + mid_rows of the horizontal pass's result; the vertical pass indexes it
            // through a base mid_row0 rows in front of it, which it never dereferences below the block (its first tap is mid_row0)
            const size_t mid_pitch = (size_t)win.w * px;
            e = rs_launch_pass((int)B, true, H, win.x0, C, in + (size_t)rt.mid_row0 * in_pitch, in_fs, in_cols, mid, rt.scratch.fs,
                               out_cols, out_cols, rt.mid_rows, frames, is, alpha, false);
            if (e == hipSuccess)
                e = rs_launch_pass((int)B, false, V, win.y0, C,
                                   (const uint8_t*)((uintptr_t)mid - (uintptr_t)((size_t)rt.mid_row0 * mid_pitch)), rt.scratch.fs,
                                   out_cols, out, step_fs, out_cols, out_cols, win.h, frames, is, alpha, false);
            break;
        }
    }
    if (e == hipSuccess) switch (rt.follower) {
            case kRsFollowNone: break;
            case kRsFollowToTensor:
                e = rs_to_tensor_launch(out, step_fs, (uint8_t*)q.out, out_fs, win.w, win.h, C, q.tc.t, frames, is);
                break;
            case kRsFollowToTensorNorm:   // from the scratch the main step filled, or from the frames no step had to touch
                e = rs_to_tensor_norm_launch(rt.follow_src ? in : out, rt.follow_src ? in_fs : step_fs, (uint8_t*)q.out, out_fs, win.w,
                                             win.h, C, (int)B, q.tc.t, frames, is);
                break;
            case kRsFollowCropsScratch:
                e = rs_to_tensor_crops_launch(out, step_fs, (size_t)win.w * C, win.w, win.h, (uint8_t*)q.out, out_fs, w.w, w.h, C,
                                              q.tc.t, q.tc.d_origin, frames, is);
                break;
            case kRsFollowCropsDirect:
                e = rs_to_tensor_crops_launch(in, in_fs, in_pitch, d->in_w, d->in_h, (uint8_t*)q.out, out_fs, w.w, w.h, C, q.tc.t,
                                              q.tc.d_origin, frames, is);
                break;
        }
    if (rt.unpacked.bytes && e == hipSuccess)
        e = rs_unpack_dest_launch(out, step_fs, (uint8_t*)q.out, out_fs, q.dc.s, win.w, win.h, C, (int)B, frames, is);
    q.launches = is.launches;
    q.copied = !rt.reduce && (rt.main == kRsMainNone || rt.main == kRsMainCopy || rt.main == kRsMainCrop);
    *q.last_kernel = rt.kernel;
    q.tc.route = rt.tensor_route, q.sc.route = rt.source_route, q.dc.route = rt.dest_route;
    if (e != hipSuccess) {
        *q.last_hip = (int)e;
        return LANCZOS_ERR_HIP;
    }
    return LANCZOS_OK;
}


// What the host entry points share: both staging blocks grown, the input copied up, `call` (the device entry on the staged
// blocks; it returns a LANCZOS_ status), the output copied down and the stream drained.  A tensor request has more to upload:
// its table, `table_at` bytes into the input block (a view's flip array rides behind it, `flips_at` bytes in), and the output
// block starts as a copy of `out` (out_up)
struct RsStagedExtra {
    const void* table = nullptr;
    size_t table_at = 0, table_bytes = 0;
    const void* flips = nullptr;
    size_t flips_at = 0, flips_bytes = 0;
    const void* origins = nullptr;   // of a lanczos_resize_crops request, behind the flips on a dword
    size_t origins_at = 0, origins_bytes = 0;
    bool out_up = false;
};
template <class F>
static int rs_staged_call(ResizeState* st, const void* in, size_t in_bytes, void* out, size_t out_bytes, const RsStagedExtra& x,
                          hipStream_t stream, int* last_hip, F&& call) {
    const size_t in_need = std::max({in_bytes, x.table_at + x.table_bytes, x.flips_at + x.flips_bytes, x.origins_at + x.origins_bytes});
    hipError_t e = st->stage_in.reserve(st->life, in_need, stream, false);   // (the context's own stream: never captured)
    if (e == hipSuccess) e = st->stage_out.reserve(st->life, out_bytes, stream, false);
    if (e == hipSuccess) e = hipMemcpyAsync(st->stage_in.p, in, in_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && x.table)
        e = hipMemcpyAsync((uint8_t*)st->stage_in.p + x.table_at, x.table, x.table_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && x.flips)
        e = hipMemcpyAsync((uint8_t*)st->stage_in.p + x.flips_at, x.flips, x.flips_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && x.origins)
        e = hipMemcpyAsync((uint8_t*)st->stage_in.p + x.origins_at, x.origins, x.origins_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && x.out_up) e = hipMemcpyAsync(st->stage_out.p, out, out_bytes, hipMemcpyHostToDevice, stream);
    int rc = LANCZOS_OK;
    if (e == hipSuccess) {
        rc = call();
        if (rc == LANCZOS_OK) e = hipMemcpyAsync(out, st->stage_out.p, out_bytes, hipMemcpyDeviceToHost, stream);
    }
    const hipError_t es = hipStreamSynchronize(stream);   // nothing stays in flight on the caller's buffers
    if (rc != LANCZOS_OK) return rc;
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
        *last_hip = (int)e;
        return LANCZOS_ERR_HIP;
    }
    return LANCZOS_OK;
}

// Stage, call the device entry, copy back.  Of a tensor request the table rides behind the input frames in the input staging
// block, behind it the flip array of a view and, on a dword, the origins of a crops request.
int resize_host(ResizeState* st, RsRequest& q) {
    const lanczos_resize_desc* d = q.d;
    const size_t B = (size_t)resize_bps(d), frames = (size_t)q.frames;
    if (((uintptr_t)q.in & (B - 1)) != 0) return LANCZOS_ERR_BAD_ARG;
    if (((uintptr_t)q.out & (q.tensor ? (uintptr_t)(q.tc.t.elem - 1) : (uintptr_t)(B - 1))) != 0) return LANCZOS_ERR_BAD_ARG;
    RsWindow w;
    const int rc = resize_window_resolve(d, q.win, &w);
    if (rc != LANCZOS_OK) return rc;
    const size_t in_bytes = (q.source ? q.sc.s.extent : (size_t)d->in_w * d->in_h * d->channels * B) * frames;
    const size_t out_bytes = q.tensor ? tensor_extent_bytes(d, w, q.tc.t) * frames
                             : q.dest ? q.dc.s.extent * (frames - 1) + q.dc.s.named
                                      : (size_t)w.w * w.h * d->channels * B * frames;
    RsStagedExtra x;
    x.out_up = q.tensor || q.dest;   // what the layout does not name keeps what it held
    if (q.tensor) {
        const RsTensorOut& t = q.tc.t;
        x.table = t.d_lut, x.table_at = (in_bytes + 255) & ~(size_t)255;
        x.table_bytes = t.norm ? 0 : (size_t)t.out_channels * 256 * t.elem;   // (a norm request has no table: d_lut is NULL)
        if (t.d_flip) x.flips = t.d_flip, x.flips_at = x.table_at + x.table_bytes, x.flips_bytes = frames;
        if (q.tc.d_origin) {
            x.origins = q.tc.d_origin, x.origins_bytes = frames * 8;
            x.origins_at = (x.table_at + x.table_bytes + x.flips_bytes + 3) & ~(size_t)3;
        }
    }
    return rs_staged_call(st, q.in, in_bytes, q.out, out_bytes, x, q.stream, q.last_hip, [&] {
        const uint8_t* up = (const uint8_t*)st->stage_in.p;
        q.in = st->stage_in.p, q.out = st->stage_out.p, q.in_frame_stride = q.out_frame_stride = 0;
        if (q.tensor && x.table) q.tc.t.d_lut = up + x.table_at;
        if (x.flips) q.tc.t.d_flip = up + x.flips_at;
        if (x.origins) q.tc.d_origin = (const int32_t*)(up + x.origins_at);
        return resize_device(st, q);
    });
}


int reduce_device(ResizeState* st, int in_w, int in_h, int channels, int fx, int fy, const int32_t* box, const void* d_in,
                  void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride, hipStream_t stream, int* last_hip) {
    (void)st;
    int rb[4];
    const int rc = reduce_validate(in_w, in_h, channels, fx, fy, box, rb);
    if (rc != LANCZOS_OK) return rc;
    const size_t in_frame = (size_t)in_w * in_h * channels;
    const size_t out_frame = (size_t)((rb[2] - rb[0] + fx - 1) / fx) * ((rb[3] - rb[1] + fy - 1) / fy) * channels;
    const size_t in_fs = in_frame_stride ? in_frame_stride : in_frame;
    const size_t out_fs = out_frame_stride ? out_frame_stride : out_frame;
    if (in_fs < in_frame || out_fs < out_frame) return LANCZOS_ERR_BAD_ARG;
    RsIssue is{stream};
    const hipError_t e = reduce_launch((const uint8_t*)d_in, (uint8_t*)d_out, in_w, channels, fx, fy, rb, frames, in_fs, out_fs, is);
    if (e != hipSuccess) {
        *last_hip = (int)e;
        return LANCZOS_ERR_HIP;
    }
    return LANCZOS_OK;
}

int reduce_host(ResizeState* st, int in_w, int in_h, int channels, int fx, int fy, const int32_t* box, const void* in,
                void* out, int frames, hipStream_t stream, int* last_hip) {
    int rb[4];
    int rc = reduce_validate(in_w, in_h, channels, fx, fy, box, rb);
    if (rc != LANCZOS_OK) return rc;
    const size_t in_bytes = (size_t)in_w * in_h * channels * frames;
    const size_t out_bytes = (size_t)((rb[2] - rb[0] + fx - 1) / fx) * ((rb[3] - rb[1] + fy - 1) / fy) * channels * frames;
    return rs_staged_call(st, in, in_bytes, out, out_bytes, {}, stream, last_hip, [&] {
        return reduce_device(st, in_w, in_h, channels, fx, fy, box, st->stage_in.p, st->stage_out.p, frames, 0, 0, stream, last_hip);
    });
}

}  // namespace lz
