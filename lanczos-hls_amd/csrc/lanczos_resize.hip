// lanczos_resize.hip -- resize to any size, downscaling included, with Pillow's contract (include/lanczos_hip.h,
// lanczos_resize_*).  Host tap tables, their per-context cache, planning, dispatch and the host entry points.
// The kernels are templates over the sample width (RsSample<BPS>, lanczos_resize_fused.hpp); there are two paths:
//
//   fused     k_rs_fused: a workgroup owns a strip of output columns (all channels) of one frame and a chunk of its output
//             rows.  It marches down the rows in blocks of kRsOB: the input rows the block's vertical taps need are staged
//             in LDS (buffer loads, range-checked zero fill), the horizontal pass turns them into rows of an LDS ring, stored
//             as Pillow stores its intermediate, and the vertical pass reads the ring and stores the block's output rows.
//             Horizontal coefficients stay in registers for the whole march (a thread keeps one output column); vertical
//             ones are workgroup-uniform scalar loads.  This file compiles the 8-bit instances that store bytes.
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
// float intermediate.  Their fused instances are compiled by lanczos_resize16.hip and lanczos_resize32.hip.
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
// instances of their own, lanczos_resize_source*.hip), every other route gets them packed into context scratch by
// k_rs_pack_source first (lanczos_resize_source.hip).
//
// A destination layout (lanczos_resize_dest: planar frames, pitched rows) changes where a result byte is stored and nothing
// else: the fused kernel stores pitched interleaved rows itself (a pitch is one of its arguments) and planes through an epilogue
// and instances of their own (lanczos_resize_dest*.hip), every other route stores the packed result in context scratch and
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

// ---- host tables -------------------------------------------------------------------------------------------------

int resize_validate(const lanczos_resize_desc* d) {
    if (!d) return LANCZOS_ERR_BAD_ARG;
    const int sizes[4] = {d->in_w, d->in_h, d->out_w, d->out_h};
    for (int s : sizes)
        if (s < 1 || s > kResizeMaxSize) return LANCZOS_ERR_BAD_ARG;
    if (d->channels != 1 && d->channels != 3 && d->channels != 4) return LANCZOS_ERR_BAD_ARG;
    if (d->a < 2 || d->a > 4) return LANCZOS_ERR_BAD_ARG;
    constexpr int kFlags = LANCZOS_RESIZE_ALPHA | LANCZOS_RESIZE_U16 | LANCZOS_RESIZE_F32;
    if ((d->reserved[0] & ~(kFlags | LANCZOS_RESIZE_FILTER(15))) != 0 || d->reserved[1] != 0) return LANCZOS_ERR_BAD_ARG;
    const int filter = resize_filter(d);
    if (filter > LANCZOS_FILTER_NEAREST) return LANCZOS_ERR_BAD_ARG;
    if (filter != LANCZOS_FILTER_LANCZOS && d->a != 3) return LANCZOS_ERR_BAD_ARG;   // one descriptor per request
    if ((d->reserved[0] & LANCZOS_RESIZE_ALPHA) && (d->reserved[0] & LANCZOS_RESIZE_U16)) return LANCZOS_ERR_BAD_ARG;
    if ((d->reserved[0] & LANCZOS_RESIZE_F32) && (d->reserved[0] & kFlags) != LANCZOS_RESIZE_F32) return LANCZOS_ERR_BAD_ARG;
    if ((d->reserved[0] & LANCZOS_RESIZE_ALPHA) && d->channels != 4) return LANCZOS_ERR_BAD_ARG;
    // Pillow resizes I;16 with NEAREST through its generic transform: other indices than the running sum's.  Not built
    if (filter == LANCZOS_FILTER_NEAREST && (d->reserved[0] & LANCZOS_RESIZE_U16)) return LANCZOS_ERR_UNSUPPORTED;
    return LANCZOS_OK;
}

// Pillow's sinc_filter / lanczos_filter with a as a parameter (libm sin, double)
static double rs_sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}
static double rs_filter(double x, int a) {
    if (-a <= x && x < a) return rs_sinc(x) * rs_sinc(x / a);
    return 0.0;
}
// Pillow's box_filter, bilinear_filter, hamming_filter and bicubic_filter, operation for operation
static double rs_box(double x) { return x > -0.5 && x <= 0.5 ? 1.0 : 0.0; }
static double rs_bilinear(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}
static double rs_hamming(double x) {
    if (x < 0.0) x = -x;
    if (x == 0.0) return 1.0;
    if (x >= 1.0) return 0.0;
    x = x * M_PI;
    return sin(x) / x * (0.54f + 0.46f * cos(x));   // float literals, widened: Pillow's bytes depend on it
}
static double rs_bicubic(double x) {
    constexpr double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
static double rs_weight(double x, int a, int filter) {
    switch (filter) {
        case LANCZOS_FILTER_BOX: return rs_box(x);
        case LANCZOS_FILTER_BILINEAR: return rs_bilinear(x);
        case LANCZOS_FILTER_HAMMING: return rs_hamming(x);
        case LANCZOS_FILTER_BICUBIC: return rs_bicubic(x);
        default: return rs_filter(x, a);
    }
}

// the extent of a span is taken in float, as Pillow's C does with its float box[4]; for the whole axis it is in_n exactly
static double rs_span_scale(RsSpan s, int out_n) { return (double)(float)(s.b1 - s.b0) / out_n; }

int resize_ksize(int in_n, int out_n, int a, int filter, RsSpan s) {
    (void)in_n;
    if (filter == LANCZOS_FILTER_NEAREST) return 1;
    const double scale = rs_span_scale(s, out_n);
    const double fs = scale > 1.0 ? scale : 1.0;
    return (int)ceil(rs_filter_support(filter, a) * fs) * 2 + 1;
}

// LANCZOS_FILTER_NEAREST: Pillow's ImagingScaleAffine steps through the source with a running sum
static bool rs_build_nearest(int in_n, int out_n, RsSpan s, ResizeAxisHost* t, bool f64) {
    const double step = rs_span_scale(s, out_n);
    t->ksize = 1, t->scale = step;
    t->first.assign(out_n, 0);
    t->count.assign(out_n, 1);
    t->coeffs.assign(f64 ? 0 : (size_t)out_n, 1 << kResizePrecision);
    t->coeffs64.assign(f64 ? (size_t)out_n : 0, 1.0);
    bool ok = true;
    double xo = (double)s.b0 + step * 0.5;
    for (int o = 0; o < out_n; o++) {
        const int i = xo < 0.0 ? -1 : (int)xo;
        if (i < 0 || i >= in_n) ok = false;   // Pillow leaves such a pixel untouched; no box inside the frame gets here
        t->first[o] = std::min(std::max(i, 0), in_n - 1);
        xo += step;
    }
    return ok;
}

bool resize_build_axis(int in_n, int out_n, int a, int filter, RsSpan s, ResizeAxisHost* t, bool f64) {
    t->in_n = in_n, t->out_n = out_n, t->a = a, t->filter = filter;
    if (filter == LANCZOS_FILTER_NEAREST) return rs_build_nearest(in_n, out_n, s, t, f64);
    const double scale = rs_span_scale(s, out_n);
    const double fs = scale > 1.0 ? scale : 1.0;
    const double support = rs_filter_support(filter, a) * fs;
    const double ss = 1.0 / fs;
    const int ksize = (int)ceil(support) * 2 + 1;
    t->ksize = ksize, t->scale = scale;
    t->first.assign(out_n, 0);
    t->count.assign(out_n, 0);
    t->coeffs.assign(f64 ? 0 : (size_t)out_n * ksize, 0);
    t->coeffs64.assign(f64 ? (size_t)out_n * ksize : 0, 0.0);
    std::vector<double> w(ksize);
    bool ok = true;
    for (int o = 0; o < out_n; o++) {
        const double center = (double)s.b0 + (o + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_n) xmax = in_n;
        const int n = xmax - xmin;
        double ww = 0.0;
        for (int i = 0; i < n; i++) {
            w[i] = rs_weight((i + xmin - center + 0.5) * ss, a, filter);
            ww += w[i];
        }
        t->first[o] = xmin;
        t->count[o] = n;
        if (f64) {
            double* k64 = &t->coeffs64[(size_t)o * ksize];
            for (int i = 0; i < n; i++) k64[i] = ww != 0.0 ? w[i] / ww : w[i];
            continue;
        }
        int32_t* k = &t->coeffs[(size_t)o * ksize];
        long long abs_sum = 0;
        for (int i = 0; i < n; i++) {
            const double v = ww != 0.0 ? w[i] / ww : w[i];
            k[i] = v < 0 ? (int32_t)(-0.5 + v * (1 << kResizePrecision)) : (int32_t)(0.5 + v * (1 << kResizePrecision));
            if (k[i] <= -(1 << 23) || k[i] >= (1 << 23)) ok = false;
            abs_sum += k[i] < 0 ? -(long long)k[i] : k[i];
        }
        if (255 * abs_sum + (1 << (kResizePrecision - 1)) >= (1ll << 31)) ok = false;
    }
    return ok;
}

// Options -> the reduction in front of the resize and the resize that remains (include/lanczos_hip.h).  The gap arithmetic is
// Pillow's Python, in double on the caller's box; only the inner box is rounded to float.
int resize_resolve(const lanczos_resize_desc* d, const lanczos_resize_opts* o, RsResolved* r) {
    *r = RsResolved();
    r->inner = *d;
    r->rb[2] = d->in_w, r->rb[3] = d->in_h;
    double box[4] = {0.0, 0.0, (double)d->in_w, (double)d->in_h};
    double gap = 0.0;
    if (o) {
        for (int i = 0; i < 4; i++) {
            if (o->reserved[i] != 0 || !std::isfinite(o->box[i])) return LANCZOS_ERR_BAD_ARG;
            box[i] = o->box[i];
        }
        if (!(box[0] >= 0.0 && box[0] < box[2] && box[2] <= d->in_w)) return LANCZOS_ERR_BAD_ARG;
        if (!(box[1] >= 0.0 && box[1] < box[3] && box[3] <= d->in_h)) return LANCZOS_ERR_BAD_ARG;
        gap = o->reducing_gap;
        if (gap != 0.0 && !(gap >= 1.0)) return LANCZOS_ERR_BAD_ARG;   // NaN included
        // Pillow drops the gap in mode RGBA and refuses it for I;16: no oracle for either.  It does reduce mode F, but the
        // summation order of its float box average is not pinned down: not built
        if (gap != 0.0 && (d->reserved[0] & (LANCZOS_RESIZE_ALPHA | LANCZOS_RESIZE_U16 | LANCZOS_RESIZE_F32)))
            return LANCZOS_ERR_BAD_ARG;
        if (gap != 0.0 && resize_nearest(d)) return LANCZOS_ERR_BAD_ARG;   // Pillow drops it there as well
    }
    if (gap != 0.0) {
        const double ex = (box[2] - box[0]) / d->out_w / gap, ey = (box[3] - box[1]) / d->out_h / gap;
        const long long fx = ex >= 1.0 ? (long long)ex : 1, fy = ey >= 1.0 ? (long long)ey : 1;
        if (fx > 1 || fy > 1) {
            if (fx * fy >= 65536) return LANCZOS_ERR_UNSUPPORTED;
            const double sup = rs_filter_support(resize_filter(d), d->a) - 0.5;
            const double sx = sup * ((box[2] - box[0]) / d->out_w), sy = sup * ((box[3] - box[1]) / d->out_h);
            r->rb[0] = std::max(0, (int)(box[0] - sx));
            r->rb[1] = std::max(0, (int)(box[1] - sy));
            r->rb[2] = (int)std::min((double)d->in_w, ceil(box[2] + sx));
            r->rb[3] = (int)std::min((double)d->in_h, ceil(box[3] + sy));
            r->fx = (int)fx, r->fy = (int)fy;
            r->inner.in_w = (r->rb[2] - r->rb[0] + r->fx - 1) / r->fx;
            r->inner.in_h = (r->rb[3] - r->rb[1] + r->fy - 1) / r->fy;
            box[0] = (box[0] - r->rb[0]) / r->fx, box[2] = (box[2] - r->rb[0]) / r->fx;
            box[1] = (box[1] - r->rb[1]) / r->fy, box[3] = (box[3] - r->rb[1]) / r->fy;
        }
    }
    for (int i = 0; i < 4; i++) r->inner_box[i] = box[i];
    r->h = RsSpan{(float)box[0], (float)box[2]};
    r->v = RsSpan{(float)box[1], (float)box[3]};
    if (!(r->h.b0 < r->h.b1) || !(r->v.b0 < r->v.b1)) return LANCZOS_ERR_BAD_ARG;   // empty once rounded to float
    r->need_h = rs_axis_runs(r->inner.in_w, r->inner.out_w, r->h);
    r->need_v = rs_axis_runs(r->inner.in_h, r->inner.out_h, r->v);
    return LANCZOS_OK;
}

int resize_window_resolve(const lanczos_resize_desc* d, const lanczos_resize_window* win, RsWindow* w) {
    *w = RsWindow{0, 0, d->out_w, d->out_h};
    if (!win) return LANCZOS_OK;
    for (int32_t r : win->reserved)
        if (r != 0) return LANCZOS_ERR_BAD_ARG;
    if (win->x0 < 0 || win->w < 1 || win->w > d->out_w || win->x0 > d->out_w - win->w) return LANCZOS_ERR_BAD_ARG;
    if (win->y0 < 0 || win->h < 1 || win->h > d->out_h || win->y0 > d->out_h - win->h) return LANCZOS_ERR_BAD_ARG;
    *w = RsWindow{win->x0, win->y0, win->w, win->h};
    return LANCZOS_OK;
}

// An axis that runs reads the union of its outputs' tap ranges (an index per output for LANCZOS_FILTER_NEAREST, whose count
// is 1); an idle one is only cropped.  With a gap that reduces, the reduction covers the whole safe box whatever the window.
int resize_window_source(const lanczos_resize_desc* d, const lanczos_resize_opts* o, const lanczos_resize_window* win,
                         int32_t rect[4]) {
    RsResolved r;
    RsWindow w;
    int rc = resize_resolve(d, o, &r);
    if (rc == LANCZOS_OK) rc = resize_window_resolve(d, win, &w);
    if (rc != LANCZOS_OK) return rc;
    if (r.reduces()) {
        for (int i = 0; i < 4; i++) rect[i] = r.rb[i];
        return LANCZOS_OK;
    }
    const struct {
        bool runs;
        int in_n, out_n, o0, n;
        RsSpan span;
    } axes[2] = {{r.need_h, d->in_w, d->out_w, w.x0, w.w, r.h}, {r.need_v, d->in_h, d->out_h, w.y0, w.h, r.v}};
    for (int ax = 0; ax < 2; ax++) {
        int lo = axes[ax].o0, hi = axes[ax].o0 + axes[ax].n;
        if (axes[ax].runs) {
            ResizeAxisHost t;
            if (!resize_build_axis(axes[ax].in_n, axes[ax].out_n, d->a, resize_filter(d), axes[ax].span, &t, resize_bps(d) > 1))
                return LANCZOS_ERR_UNSUPPORTED;
            lo = axes[ax].in_n, hi = 0;
            for (int i = axes[ax].o0; i < axes[ax].o0 + axes[ax].n; i++) {
                lo = std::min(lo, t.first[i]);
                hi = std::max(hi, t.first[i] + t.count[i]);
            }
        }
        rect[ax] = lo, rect[ax + 2] = hi;
    }
    return LANCZOS_OK;
}

// ---- kernels -----------------------------------------------------------------------------------------------------

constexpr int kRsFusedMaxLds = 80 * 1024;   // at least two fused workgroups per CU (160 KiB of LDS)
constexpr int kRsRowsPerChunkMin = 4 * kRsOB;
constexpr int kRsTargetWgs = 2048;

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

// the 8-bit instances of k_rs_fused that store bytes
template hipError_t rs_launch_fused<1, 0>(const RsFusedLaunch&);

// the tap count of the smallest fused instance that holds ksize (0: none; small: the instances with 3 and 5 taps count, which
// they do for every filter but Lanczos)
static int rs_bucket(int ksize, bool small) {
    int k = 0;
    if ((!small || env().rs_no_small_buckets) && ksize < 7) ksize = 7;
#define X(KB) \
    if (!k && ksize <= KB) k = KB;
    LZ_RS_BUCKETS(X)
#undef X
    return k;
}

// ---- host side: cache, planning, launch ---------------------------------------------------------------------------

// a block that launches on `streams` may still read: freed by a later call once they have drained.  A stream that is being
// captured gets no event (it would become a graph node): such a block waits for the final reap behind a device-wide sync.
static void rs_retire(RetireList& rl, void* p, const std::vector<hipStream_t>& streams) {
    std::vector<hipStream_t> live;
    bool captured = false;
    for (hipStream_t s : streams) {
        if (stream_capturing(s)) captured = true;
        else live.push_back(s);
    }
    rl.retire({p}, {}, live);
    if (captured) rl.list.back().unrecorded = true;
}

ResizeState::~ResizeState() {   // the owner has drained the device
    retired.reap(true);
    for (ResizeAxis* a : axes) {
        (void)hipFree(a->dev);
        delete a;
    }
    for (void* p : kept) (void)hipFree(p);
    if (scratch.p) (void)hipFree(scratch.p);
    if (reduced.p) (void)hipFree(reduced.p);
    if (tensor_bytes.p) (void)hipFree(tensor_bytes.p);
    if (packed.p) (void)hipFree(packed.p);
    if (unpacked.p) (void)hipFree(unpacked.p);
    if (stage_in) (void)hipFree(stage_in);
    if (stage_out) (void)hipFree(stage_out);
    if (upload) (void)hipStreamDestroy(upload);
}

// The tables of one axis shape, built and uploaded on first use.  The upload is eager: a copy on the private stream and a
// wait for it, so an entry is valid from the moment it is cached -- also when the caller's stream is being captured
// (a copy queued on it would only run when the graph is replayed, perhaps never).
static int rs_axis(ResizeState* st, int in_n, int out_n, int a, int filter, RsSpan span, bool f64, ResizeAxis** out,
                   int* last_hip) {
    uint32_t bits[2];
    memcpy(&bits[0], &span.b0, 4);
    memcpy(&bits[1], &span.b1, 4);
    for (size_t i = 0; i < st->axes.size(); i++) {
        ResizeAxis* ax = st->axes[i];
        if (ax->key[0] == in_n && ax->key[1] == out_n && ax->key[2] == a && ax->key[3] == (int)f64 &&
            ax->key[4] == filter && ax->span_bits[0] == bits[0] && ax->span_bits[1] == bits[1]) {
            st->axes.erase(st->axes.begin() + i);
            st->axes.push_back(ax);   // most recent last
            *out = ax;
            return LANCZOS_OK;
        }
    }
    st->retired.reap(false);
    ResizeAxis* ax = new (std::nothrow) ResizeAxis();
    if (!ax) return LANCZOS_ERR_NOMEM;
    ax->key[0] = in_n, ax->key[1] = out_n, ax->key[2] = a, ax->key[3] = (int)f64, ax->key[4] = filter;
    ax->span_bits[0] = bits[0], ax->span_bits[1] = bits[1];
    if (!resize_build_axis(in_n, out_n, a, filter, span, &ax->host, f64)) {
        delete ax;
        return LANCZOS_ERR_UNSUPPORTED;
    }
    const ResizeAxisHost& h = ax->host;
    std::vector<int32_t> block((size_t)2 * h.out_n + h.coeffs.size() + 2 * h.coeffs64.size());
    memcpy(block.data(), h.first.data(), (size_t)h.out_n * 4);
    memcpy(block.data() + h.out_n, h.count.data(), (size_t)h.out_n * 4);
    if (f64) memcpy(block.data() + 2 * (size_t)h.out_n, h.coeffs64.data(), h.coeffs64.size() * 8);
    else memcpy(block.data() + 2 * (size_t)h.out_n, h.coeffs.data(), h.coeffs.size() * 4);
    hipError_t e = hipSuccess;
    if (!st->upload) e = hipStreamCreateWithFlags(&st->upload, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&ax->dev, block.size() * 4);
    if (e == hipSuccess) e = hipMemcpyAsync(ax->dev, block.data(), block.size() * 4, hipMemcpyHostToDevice, st->upload);
    if (e == hipSuccess) e = hipStreamSynchronize(st->upload);
    if (e != hipSuccess) {
        *last_hip = (int)e;
        if (ax->dev) (void)hipFree(ax->dev);   // nothing else has seen the block
        delete ax;
        return LANCZOS_ERR_HIP;
    }
    if (st->axes.size() >= ResizeState::kMaxAxes) {   // bounded: the least recently used shape goes once its launches drained
        ResizeAxis* old = st->axes.front();
        rs_retire(st->retired, old->dev, old->streams);
        delete old;
        st->axes.erase(st->axes.begin());
    }
    st->axes.push_back(ax);
    *out = ax;
    return LANCZOS_OK;
}

// context scratch of at least `bytes`.  A block a captured launch used may still be named by a live graph: it is kept until
// the context goes instead of being freed when a larger one replaces it.
static int rs_scratch(ResizeState* st, ResizeState::Block* blk, size_t bytes, hipStream_t stream, bool capturing,
                      int* last_hip) {
    if (blk->bytes < bytes) {
        if (blk->p) {
            if (blk->captured) st->kept.push_back(blk->p);
            else rs_retire(st->retired, blk->p, blk->streams);
        }
        blk->p = nullptr;
        blk->bytes = 0;
        blk->captured = false;
        blk->streams.clear();
        hipError_t e = hipMalloc(&blk->p, bytes);
        if (e != hipSuccess) {
            *last_hip = (int)e;
            blk->p = nullptr;
            return LANCZOS_ERR_HIP;
        }
        blk->bytes = bytes;
    }
    if (capturing) blk->captured = true;
    else note_stream(blk->streams, stream);
    return LANCZOS_OK;
}

// The two sizes of the plan that depend on where a window lies.  stage_dw: the dwords of a staged row, the widest span of
// source bytes one of the window's strips reads.  ring_rows: the most intermediate rows a march step of kRsOB output rows
// reads; the steps start every kRsOB rows from the window's first (chunks are whole steps) and the last one may be short.
static int rs_plan_stage_dw(const RsAxisView& H, int x_at, int w, int SW, int C, int NE) {
    int span_dw = 0;
    for (int x0 = 0; x0 < w; x0 += SW) {
        const int x1 = std::min(w, x0 + SW) - 1;
        const int hoffb = (H.first[x_at + x1] - H.first[x_at + x0]) * C;
        span_dw = std::max(span_dw, ((3 + hoffb) >> 2) + NE + 1);
    }
    return span_dw;
}
static int rs_plan_ring_rows(const RsAxisView& V, int y_at, int h) {
    int ring = 1;
    for (int o0 = 0; o0 < h; o0 += kRsOB) {
        const int last = std::min(o0 + kRsOB, h) - 1;
        ring = std::max(ring, V.first[y_at + last] + V.count[y_at + last] - V.first[y_at + o0]);
    }
    return ring;
}

// The fused kernel's launch shape for a w x h window of the output of H x V whose origin is any of nx x ny places from the
// views' first outputs on: stage_dw and ring_rows are the largest any of them needs.  One place is the window itself.
static bool rs_fused_plan_at(const lanczos_resize_desc* d, const RsAxisView& H, const RsAxisView& V, int w, int h, int nx, int ny,
                             int frames, RsFusedPlan* fp, size_t src_extent) {
    const int bps = resize_bps(d);
    const int C = d->channels * bps;   // bytes per pixel
    const int out_w = w, out_h = h;
    // 32-bit buffer offsets, into the frame as the kernel addresses it: a pitched or planar source has its own extent
    if (src_extent >= ((size_t)1 << 31)) return false;
    if ((src_extent ? (long long)src_extent : (long long)d->in_w * d->in_h * C) + 4 >= (1ll << 31)) return false;
    if ((long long)out_w * out_h * C >= (1ll << 31)) return false;
    const bool small = resize_filter(d) != LANCZOS_FILTER_LANCZOS;   // the instances with 3 and 5 taps
    fp->K = rs_bucket(H.ksize, small);
    if (!fp->K) return false;
    const int SW = rs_strip_width(d->channels, bps);
    const int NE = (fp->K * C + 3) / 4;
    fp->strips = (out_w + SW - 1) / SW;
    fp->stage_dw = 0;
    for (int x = 0; x < nx; x++) fp->stage_dw = std::max(fp->stage_dw, rs_plan_stage_dw(H, x, out_w, SW, C, NE));
    int ring = 1;
    for (int y = 0; y < ny; y++) ring = std::max(ring, rs_plan_ring_rows(V, y, out_h));
    fp->ring_rows = ring;
    const double scale_v = V.scale;
    fp->stage_rows = std::min(16, (int)ceil(kRsOB * scale_v) + 1);
    auto lds = [&]() { return (size_t)ring * SW * C + (size_t)fp->stage_rows * fp->stage_dw * 4; };
    while (lds() > (size_t)kRsFusedMaxLds && fp->stage_rows > 4) fp->stage_rows--;   // wide spans: fewer rows per staging
    fp->lds = lds();
    if (fp->lds > (size_t)kRsFusedMaxLds) return false;
    // row chunks: enough workgroups to fill the chip, each chunk a whole number of march steps
    int rpc = (out_h + kRsOB - 1) / kRsOB * kRsOB;
    const long long base = (long long)fp->strips * frames;
    while (base * ((out_h + rpc - 1) / rpc) < kRsTargetWgs && rpc > kRsRowsPerChunkMin)
        rpc = std::max(kRsRowsPerChunkMin, (rpc / 2 + kRsOB - 1) / kRsOB * kRsOB);
    fp->rows_per_chunk = rpc;
    fp->chunks = (out_h + rpc - 1) / rpc;
    return (long long)fp->strips * fp->chunks < (1ll << 31);
}

// the fused kernel's launch shape for this request, both of whose passes run (false: it cannot run it).  The output is that
// of the two views, a window of d's
bool rs_fused_plan(const lanczos_resize_desc* d, const RsAxisView& H, const RsAxisView& V, int frames, RsFusedPlan* fp,
                   size_t src_extent) {
    return rs_fused_plan_at(d, H, V, H.n, V.n, 1, 1, frames, fp, src_extent);
}

// ... and for a w x h window at any origin inside the output of the two views, which are the full axes: brute force over the
// origins of each axis, a few hundred at most times a handful of strips or march steps
bool rs_fused_plan_crops(const lanczos_resize_desc* d, const RsAxisView& H, const RsAxisView& V, int w, int h, int frames,
                         RsFusedPlan* fp, size_t src_extent) {
    return rs_fused_plan_at(d, H, V, w, h, H.n - w + 1, V.n - h + 1, frames, fp, src_extent);
}

int resize_crops_validate(const lanczos_resize_desc* d, const lanczos_resize_crops* c) {
    const int rc = resize_validate(d);
    if (rc != LANCZOS_OK) return rc;
    if (!c || !c->d_origin) return LANCZOS_ERR_BAD_ARG;
    for (int32_t r : c->reserved)
        if (r != 0) return LANCZOS_ERR_BAD_ARG;
    if (c->w < 1 || c->w > d->out_w || c->h < 1 || c->h > d->out_h) return LANCZOS_ERR_BAD_ARG;
    if (((uintptr_t)c->d_origin & 3) != 0) return LANCZOS_ERR_BAD_ARG;
    return LANCZOS_OK;
}

int resize_plan_host(const lanczos_resize_desc* d, const lanczos_resize_opts* o, const lanczos_resize_window* win, int frames,
                     lanczos_resize_plan_ex* out, const lanczos_resize_crops* crops) {
    memset(out, 0, sizeof(*out));
    RsResolved r;
    RsWindow w;
    int rc = resize_resolve(d, o, &r);
    if (rc == LANCZOS_OK) rc = resize_window_resolve(d, win, &w);
    if (rc != LANCZOS_OK) return rc;
    out->fx = r.fx, out->fy = r.fy;
    for (int i = 0; i < 4; i++) out->safe_box[i] = r.rb[i], out->inner_box[i] = r.inner_box[i];
    out->reduced_w = r.inner.in_w, out->reduced_h = r.inner.in_h;
    out->pass_h = r.need_h, out->pass_v = r.need_v;
    const bool u16 = resize_bps(d) > 1;   // the double tables
    const int filter = resize_filter(d);
    if (filter == LANCZOS_FILTER_NEAREST) return LANCZOS_OK;   // one gather launch: no intermediate, nothing to fuse
    ResizeAxisHost H, V;
    if (r.need_v) {
        if (!resize_build_axis(r.inner.in_h, r.inner.out_h, d->a, filter, r.v, &V, u16)) return LANCZOS_ERR_UNSUPPORTED;
        if (r.need_h) rs_mid_rows(rs_axis_view(V, w.y0, w.h), &out->mid_row0, &out->mid_rows);
    }
    if (!r.need_h || !r.need_v) return LANCZOS_OK;   // as resize_device: no table for an idle axis, nothing to fuse
    if (rs_vertical_first(&r.inner, true, true)) return LANCZOS_OK;   // the pass kernels, vertical first: never fused
    if (!resize_build_axis(r.inner.in_w, r.inner.out_w, d->a, filter, r.h, &H, u16)) return LANCZOS_ERR_UNSUPPORTED;
    RsFusedPlan fp;
    if (crops ? !rs_fused_plan_crops(&r.inner, rs_axis_view(H, 0, H.out_n), rs_axis_view(V, 0, V.out_n), crops->w, crops->h, frames, &fp)
              : !rs_fused_plan(&r.inner, rs_axis_view(H, w.x0, w.w), rs_axis_view(V, w.y0, w.h), frames, &fp))
        return LANCZOS_OK;
    lanczos_resize_plan* in = &out->inner;
    in->fused = 1;
    in->K = fp.K, in->strips = fp.strips, in->rows_per_chunk = fp.rows_per_chunk, in->chunks = fp.chunks;
    in->ring_rows = fp.ring_rows, in->stage_rows = fp.stage_rows, in->stage_dw = fp.stage_dw;
    in->lds_bytes = (int32_t)fp.lds;
    return LANCZOS_OK;
}

// One pass of the two-pass path over `rows` rows of `n_cols` samples of `bps` bytes; src / dst row pitches in samples, frame
// strides in bytes.  alpha: the LANCZOS_RESIZE_ALPHA kernels (8-bit, a thread per pixel); `only`: the other pass does not run.
// o0: the output of the axis the pass starts at (a window); the kernels count their outputs from it
// v_first: both passes run, the vertical one first (rs_vertical_first); it only changes which alpha kernel a pass is
static hipError_t rs_launch_pass(int bps, bool horizontal, const ResizeAxis* ax, int o0, int channels, const uint8_t* src, size_t src_fs,
                                 size_t src_pitch, uint8_t* dst, size_t dst_fs, size_t dst_pitch, int n_cols, int rows, int frames,
                                 hipStream_t stream, bool alpha, bool only, bool v_first = false) {
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
        for (int f0 = 0; f0 < frames; f0 += 65535) {
            const int nf = std::min(65535, frames - f0);
            p.src = src + (size_t)f0 * src_fs;
            p.dst = dst + (size_t)f0 * dst_fs;
            const int n_threads = alpha ? n_cols / 4 : n_cols;
            const dim3 grid((n_threads + kRsThreads - 1) / kRsThreads, rows, nf);
            hipLaunchKernelGGL(kern, grid, dim3(kRsThreads), 0, stream, p);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    return bps == 4 ? run(RsSample<4>()) : bps == 2 ? run(RsSample<2>()) : run(RsSample<1>());
}

// the resize that remains once the options are resolved: `d` describes the frames at `in` (the caller's, or the reduced
// ones), sh / sv are the source spans of its two axes
// tc: a tensor request, `out` / `out_fs` then being the element frames.  Where the fused kernel runs it stores them itself;
// everything else writes its bytes to context scratch and k_rs_to_tensor follows
// win: the window of d's output that is stored, as a tightly packed win.w x win.h frame.  The passes that run and the tables
// are those of the full request; plan, scratch and every launch are the window's
// tc->d_origin (a crop origin per frame): win is (0, 0, w, h).  The fused kernel runs on the plan that holds for every origin;
// everything else resizes the whole output into context scratch and k_rs_to_tensor_crops gathers each frame's window from it --
// or from the caller's frames where no pass runs
// sc: the frames at `in` lie in that layout, which is not the tight one (the tight one is no source at all).  Where the fused
// kernel runs and has the staging for it, it reads them as they lie (LANCZOS_SOURCE_DIRECT); everything else gets them packed
// into context scratch first (rs_pack_source) and is then the request it always was
// dc: the window is stored in that layout, which is not the tight one (never with tc).  Where the fused kernel runs it stores
// pitched rows and planes itself (LANCZOS_DEST_DIRECT); everything else stores the tightly packed window in context scratch, as
// the request it always was, and k_rs_unpack_dest scatters it (LANCZOS_DEST_UNPACKED)
static int resize_inner(ResizeState* st, const lanczos_resize_desc* d, RsSpan sh, RsSpan sv, const RsWindow& win_in,
                        const uint8_t* in, uint8_t* out, int frames, size_t in_fs, size_t out_fs, hipStream_t stream,
                        int* last_kernel, int* last_hip, RsTensorCall* tc, RsSourceCall* sc = nullptr, RsDestCall* dc = nullptr);

// the PACKED route of a source: `frames` frames at *in, in layout s, gathered tightly packed into the context's block; *in and
// *in_fs then name that block
static int rs_pack_source(ResizeState* st, const lanczos_resize_desc* d, const RsSource& s, const uint8_t** in, size_t* in_fs,
                          int frames, hipStream_t stream, int* last_hip) {
    const size_t fs = ((size_t)d->in_w * d->in_h * d->channels * resize_bps(d) + 3) & ~(size_t)3;
    const int rc = rs_scratch(st, &st->packed, (size_t)frames * fs, stream, stream_capturing(stream), last_hip);
    if (rc != LANCZOS_OK) return rc;
    const hipError_t e = rs_pack_source_launch(*in, *in_fs, s, (uint8_t*)st->packed.p, fs, d->in_w, d->in_h, d->channels,
                                               resize_bps(d), frames, stream);
    if (e != hipSuccess) {
        *last_hip = (int)e;
        return LANCZOS_ERR_HIP;
    }
    *in = (const uint8_t*)st->packed.p, *in_fs = fs;
    return LANCZOS_OK;
}

static int resize_inner(ResizeState* st, const lanczos_resize_desc* d, RsSpan sh, RsSpan sv, const RsWindow& win_in,
                        const uint8_t* in, uint8_t* out, int frames, size_t in_fs, size_t out_fs, hipStream_t stream,
                        int* last_kernel, int* last_hip, RsTensorCall* tc, RsSourceCall* sc, RsDestCall* dc) {
    const int C = d->channels;
    const size_t B = (size_t)resize_bps(d);   // bytes per sample
    const bool f32 = B == 4;
    const bool u16 = B > 1;   // samples wider than a byte: the double tables
    const size_t in_frame = (size_t)d->in_w * d->in_h * C * B;
    const bool capturing = stream_capturing(stream);
    const bool need_h = rs_axis_runs(d->in_w, d->out_w, sh), need_v = rs_axis_runs(d->in_h, d->out_h, sv);
    const bool alpha = (d->reserved[0] & LANCZOS_RESIZE_ALPHA) != 0;
    const int filter = resize_filter(d);
    // the gather reads both index tables, also that of an axis that keeps its size (the identity) -- unless both do
    const bool nearest = filter == LANCZOS_FILTER_NEAREST && (need_h || need_v);
    // Pillow's order for a tall frame that shrinks: never the fused kernel, the pass kernels vertical first
    const bool v_first = rs_vertical_first(d, need_h, need_v);

    ResizeAxis *H = nullptr, *V = nullptr;
    int rc;
    if ((need_h || nearest) && (rc = rs_axis(st, d->in_w, d->out_w, d->a, filter, sh, u16, &H, last_hip)) != LANCZOS_OK)
        return rc;
    if ((need_v || nearest) && (rc = rs_axis(st, d->in_h, d->out_h, d->a, filter, sv, u16, &V, last_hip)) != LANCZOS_OK)
        return rc;
    for (ResizeAxis* ax : {H, V})
        if (ax && !capturing) note_stream(ax->streams, stream);

    const bool crops = tc && tc->d_origin;
    RsWindow win = win_in;
    RsFusedPlan fp;
    // the source as the fused kernel would read it: a planar one needs the instances, which crops have none of, and AUTO's leave
    const RsSource* src = sc ? &sc->s : nullptr;
    // ALPHA stages whole pixels and shifts them by the frame's residue: rows whose pitch is no dword multiple need the instances
    // that shift by the row's, which crops have none of either
    const bool rowshift = src && !src->planar && alpha && (src->row_stride & 3) != 0;
    if (src && (st->force == LANCZOS_RESIZE_CONVERT || st->force == LANCZOS_RESIZE_TWO_PASS || (rowshift && crops) ||
                (src->planar && (crops || (st->force == LANCZOS_RESIZE_AUTO && !kRsPlanarAutoDirect)))))
        src = nullptr;
    auto plan = [&](size_t extent) {
        return !nearest && need_h && need_v && !v_first &&
               (crops ? rs_fused_plan_crops(d, rs_axis_view(H->host, 0, d->out_w), rs_axis_view(V->host, 0, d->out_h), win.w, win.h,
                                            frames, &fp, extent)
                      : rs_fused_plan(d, rs_axis_view(H->host, win.x0, win.w), rs_axis_view(V->host, win.y0, win.h), frames, &fp,
                                      extent));
    };
    bool fused_ok = src ? plan(src->extent) : false;
    if (!fused_ok) src = nullptr, fused_ok = plan(0);   // no source, or one the kernel cannot address: the packed frame's plan
    if (st->force == LANCZOS_RESIZE_FUSED && !fused_ok) return LANCZOS_ERR_UNSUPPORTED;
    bool fused = fused_ok && st->force != LANCZOS_RESIZE_TWO_PASS;
    // 32-bit buffer offsets into the element frame: a larger one is converted, and refused where the fused kernel is forced
    const bool t_fits = tc && tc->extent_bytes < ((size_t)1 << 31);
    if (tc && st->force == LANCZOS_RESIZE_FUSED && !t_fits) return LANCZOS_ERR_UNSUPPORTED;
    const bool t_fused = fused && t_fits && st->force != LANCZOS_RESIZE_CONVERT;
    uint8_t* const t_out = out;
    const size_t t_fs = out_fs;
    const bool crops_gather = crops && !t_fused;
    if (sc) {
        if (crops_gather || !fused) src = nullptr;   // the fused kernel alone reads a source as it lies
        sc->route = src ? LANCZOS_SOURCE_DIRECT : LANCZOS_SOURCE_PACKED;
        if (!src && (rc = rs_pack_source(st, d, sc->s, &in, &in_fs, frames, stream, last_hip)) != LANCZOS_OK) return rc;
    }
    const bool crops_direct = crops_gather && !nearest && !need_h && !need_v;   // no pass runs: the caller's frames are the bytes
    if (crops_gather) {   // the bytes of the whole output, by the plan of the whole output
        win = RsWindow{0, 0, d->out_w, d->out_h};
        fused_ok = !nearest && need_h && need_v && !v_first &&
                   rs_fused_plan(d, rs_axis_view(H->host, 0, win.w), rs_axis_view(V->host, 0, win.h), frames, &fp);
        fused = fused_ok && st->force != LANCZOS_RESIZE_TWO_PASS;
    }
    if (tc && !t_fused && !crops_direct) {
        const size_t bytes_fs = ((size_t)win.w * win.h * C + 3) & ~(size_t)3;
        rc = rs_scratch(st, &st->tensor_bytes, (size_t)frames * bytes_fs, stream, capturing, last_hip);
        if (rc != LANCZOS_OK) return rc;
        out = (uint8_t*)st->tensor_bytes.p, out_fs = bytes_fs;
    }
    // 32-bit buffer offsets into the pitched frame, whose range the kernel takes as rows x pitch
    uint8_t* const d_out = out;
    const size_t d_fs = out_fs;
    // a planar destination has instances of its own (8-bit, three or four channels), none of them with the row shift of an ALPHA
    // source pitched off a dword: that one keeps its direct staging and is unpacked
    const bool dst_direct = dc && fused && !dc->unpack_only && st->force != LANCZOS_RESIZE_CONVERT &&
                            std::max(dc->s.named, (size_t)win.h * dc->s.row_stride) < ((size_t)1 << 31) &&
                            (!dc->s.planar || ((st->force != LANCZOS_RESIZE_AUTO || kRsPlanarOutAutoDirect) && !(src && rowshift)));
    if (dc) {
        if (tc) return LANCZOS_ERR_BAD_ARG;
        dc->route = dst_direct ? LANCZOS_DEST_DIRECT : LANCZOS_DEST_UNPACKED;
        if (!dst_direct) {   // the packed window, readable a few dwords past its end (k_rs_unpack_dest)
            const size_t bytes_fs = ((size_t)win.w * win.h * C * B + 3) & ~(size_t)3;
            rc = rs_scratch(st, &st->unpacked, (size_t)frames * bytes_fs + 32, stream, capturing, last_hip);
            if (rc != LANCZOS_OK) return rc;
            out = (uint8_t*)st->unpacked.p, out_fs = bytes_fs;
        }
    }
    // two passes: the horizontal one produces the rows the vertical taps read and no others, mid_rows of them from source
    // row mid_row0 on, and the scratch holds exactly those; the vertical pass indexes it through a base mid_row0 rows in
    // front of it, which it never dereferences below the block (its first tap is row mid_row0)
    // (a horizontal pass alone runs the window's rows, which are the source's)
    int mid_row0 = win.y0, mid_rows = win.h;
    if (need_h && need_v) rs_mid_rows(rs_axis_view(V->host, win.y0, win.h), &mid_row0, &mid_rows);
    const size_t mid_pitch = (size_t)win.w * C * B, mid_fs = (size_t)mid_rows * mid_pitch;
    const size_t in_pitch = (size_t)d->in_w * C * B;
    hipError_t e = hipSuccess;
    if (fused) {
        const RsFusedLaunch c{d, win, &fp, H, V, in, out, in_fs, out_fs, frames, tc, stream, src, dst_direct ? &dc->s : nullptr};
        e = dst_direct && dc->s.planar ? (src && src->planar ? rs_launch_fused<1, kRsPlanar + kRsPlanarOut>(c)
                                                             : rs_launch_fused<1, kRsPlanarOut>(c))
            : src && src->planar ? (!t_fused           ? rs_launch_fused<1, kRsPlanar>(c)
                                  : tc->t.elem == 2 ? rs_launch_fused<1, 2 + kRsMapped + kRsPlanar>(c)
                                                    : rs_launch_fused<1, 4 + kRsMapped + kRsPlanar>(c))
            : src && rowshift  ? (!t_fused           ? rs_launch_fused<1, kRsRowShift>(c)
                                  : tc->t.elem == 2 ? rs_launch_fused<1, 2 + kRsMapped + kRsRowShift>(c)
                                                    : rs_launch_fused<1, 4 + kRsMapped + kRsRowShift>(c))
            : t_fused && crops ? (tc->t.elem == 2 ? rs_launch_fused<1, 2 + kRsMapped + kRsCrops>(c)
                                                : rs_launch_fused<1, 4 + kRsMapped + kRsCrops>(c))
            : t_fused && tc->t.mapped ? (tc->t.elem == 2 ? rs_launch_fused<1, 2 + kRsMapped>(c) : rs_launch_fused<1, 4 + kRsMapped>(c))
            : t_fused ? (tc->t.elem == 2 ? rs_launch_fused<1, 2>(c) : rs_launch_fused<1, 4>(c))
            : f32   ? rs_launch_fused<4, 0>(c)
            : u16   ? rs_launch_fused<2, 0>(c)
                    : rs_launch_fused<1, 0>(c);
        *last_kernel = LANCZOS_KERNEL_RESIZE_FUSED;
    } else if (nearest) {
        e = rs_nearest_launch(in, out, d->in_w, win.w, win.h, C, (int)B, H->first() + win.x0, V->first() + win.y0, frames, in_fs,
                              out_fs, stream);
        *last_kernel = LANCZOS_KERNEL_RESIZE_NEAREST;
    } else if (!need_h && !need_v) {   // Pillow returns a copy (also of RGBA: no premultiply round trip); a window crops it
        if (crops_direct)
            ;   // nothing to copy: the gather below reads the caller's frames
        else if (win.whole(d))
            e = hipMemcpy2DAsync(out, out_fs, in, in_fs, in_frame, frames, hipMemcpyDeviceToDevice, stream);
        else
            e = rs_crop_launch(in + (size_t)win.y0 * in_pitch + (size_t)win.x0 * C * B, out, in_pitch, (size_t)win.w * C * B,
                               win.h, frames, in_fs, out_fs, stream);
        *last_kernel = LANCZOS_KERNEL_RESIZE_TWO_PASS;
    } else if (v_first) {
        // The vertical pass turns the window's rows of the source's full width (Pillow's, and at most 655 pixels) into win.h
        // rows of context scratch, stored as every intermediate is; the horizontal pass reads them through the window's slice
        // of its table, whose `first` indexes that full width, and writes the output.
        const int in_cols = d->in_w * C, out_cols = win.w * C;   // samples of a row
        const size_t vmid_fs = (size_t)win.h * in_pitch;
        rc = rs_scratch(st, &st->scratch, (size_t)frames * vmid_fs, stream, capturing, last_hip);
        if (rc != LANCZOS_OK) return rc;
        uint8_t* const vmid = (uint8_t*)st->scratch.p;
        e = rs_launch_pass((int)B, false, V, win.y0, C, in, in_fs, in_cols, vmid, vmid_fs, in_cols, in_cols, win.h, frames, stream,
                           alpha, false, true);
        if (e == hipSuccess)
            e = rs_launch_pass((int)B, true, H, win.x0, C, vmid, vmid_fs, in_cols, out, out_fs, out_cols, out_cols, win.h, frames,
                               stream, alpha, false, true);
        *last_kernel = LANCZOS_KERNEL_RESIZE_TWO_PASS;
    } else {
        const int in_cols = d->in_w * C, out_cols = win.w * C;   // samples of a row
        const uint8_t* mid = in;   // what the vertical pass reads
        size_t v_fs = in_fs;
        if (need_h) {
            uint8_t* dst = out;
            size_t dst_fs = out_fs;
            if (need_v) {
                rc = rs_scratch(st, &st->scratch, (size_t)frames * mid_fs, stream, capturing, last_hip);
                if (rc != LANCZOS_OK) return rc;
                dst = (uint8_t*)st->scratch.p, dst_fs = mid_fs;
            }
            e = rs_launch_pass((int)B, true, H, win.x0, C, in + (size_t)mid_row0 * in_pitch, in_fs, in_cols, dst, dst_fs,
                               out_cols, out_cols, mid_rows, frames, stream, alpha, !need_v);
            mid = (const uint8_t*)((uintptr_t)dst - (uintptr_t)((size_t)mid_row0 * mid_pitch)), v_fs = dst_fs;
        } else {
            mid = in + (size_t)win.x0 * C * B;   // the vertical pass alone: the window's columns of the source's full rows
        }
        if (e == hipSuccess && need_v)
            e = rs_launch_pass((int)B, false, V, win.y0, C, mid, v_fs, need_h ? out_cols : in_cols, out, out_fs, out_cols,
                               out_cols, win.h, frames, stream, alpha, !need_h);
        *last_kernel = LANCZOS_KERNEL_RESIZE_TWO_PASS;
    }
    if (tc) {
        if (crops_direct)
            e = rs_to_tensor_crops_launch(in, in_fs, in_pitch, d->in_w, d->in_h, t_out, t_fs, win_in.w, win_in.h, C, tc->t,
                                          tc->d_origin, frames, stream);
        else if (crops_gather && e == hipSuccess)
            e = rs_to_tensor_crops_launch(out, out_fs, (size_t)win.w * C, win.w, win.h, t_out, t_fs, win_in.w, win_in.h, C, tc->t,
                                          tc->d_origin, frames, stream);
        else if (!t_fused && e == hipSuccess)
            e = rs_to_tensor_launch(out, out_fs, t_out, t_fs, win.w, win.h, C, tc->t, frames, stream);
        tc->route = t_fused ? LANCZOS_TENSOR_FUSED : LANCZOS_TENSOR_CONVERTED;
    }
    if (dc && !dst_direct && e == hipSuccess)
        e = rs_unpack_dest_launch(out, out_fs, d_out, d_fs, dc->s, win.w, win.h, C, (int)B, frames, stream);
    if (capturing) {   // a live graph may name these tables: they stay until the context goes
        for (ResizeAxis* ax : {H, V})
            if (ax) {
                auto it = std::find(st->axes.begin(), st->axes.end(), ax);
                if (it != st->axes.end()) {
                    st->kept.push_back(ax->dev);
                    ax->dev = nullptr;
                    st->axes.erase(it);
                    delete ax;
                }
            }
    }
    if (e != hipSuccess) {
        *last_hip = (int)e;
        return LANCZOS_ERR_HIP;
    }
    return LANCZOS_OK;
}

int resize_device(ResizeState* st, const lanczos_resize_desc* d, const lanczos_resize_opts* o, const lanczos_resize_window* win,
                  const void* d_in, void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride, hipStream_t stream,
                  int* last_kernel, int* last_hip, RsTensorCall* tc, RsSourceCall* sc, RsDestCall* dc) {
    RsResolved r;
    RsWindow w;
    int rc = resize_resolve(d, o, &r);
    if (rc == LANCZOS_OK) rc = resize_window_resolve(d, win, &w);
    if (rc != LANCZOS_OK) return rc;
    const int C = d->channels;
    const size_t B = (size_t)resize_bps(d);   // bytes per sample
    if (sc && sc->s.tight) sc->route = LANCZOS_SOURCE_DIRECT, sc = nullptr;   // the call without a source
    const size_t in_frame = sc ? sc->s.extent : (size_t)d->in_w * d->in_h * C * B;
    if (dc && dc->s.tight) dc->route = LANCZOS_DEST_DIRECT, dc = nullptr;     // the call without a destination
    const size_t out_frame = tc ? tc->extent_bytes : dc ? dc->s.extent : (size_t)w.w * w.h * C * B;
    const size_t in_fs = in_frame_stride ? in_frame_stride : in_frame;
    const size_t out_fs = out_frame_stride ? out_frame_stride : out_frame;
    // a destination's frames may overlap each other's padding: the stride has to clear the named bytes only
    if (in_fs < in_frame || out_fs < (dc ? dc->s.named : out_frame)) return LANCZOS_ERR_BAD_ARG;
    if ((((uintptr_t)d_in | (uintptr_t)d_out | in_fs | out_fs) & (B - 1)) != 0) return LANCZOS_ERR_BAD_ARG;
    if (tc && (((uintptr_t)d_out | out_fs) & (size_t)(tc->t.elem - 1)) != 0) return LANCZOS_ERR_BAD_ARG;   // element frames
    const uint8_t* in = (const uint8_t*)d_in;
    size_t in_fs_r = in_fs;
    if (sc && r.reduces()) {   // the reduction reads packed frames
        sc->route = LANCZOS_SOURCE_PACKED;
        if ((rc = rs_pack_source(st, d, sc->s, &in, &in_fs_r, frames, stream, last_hip)) != LANCZOS_OK) return rc;
    }
    if (dc && r.reduces()) dc->unpack_only = true;   // as a source is packed for the reduction, whatever resizes the reduced frames
    if (r.reduces()) {   // reducing_gap: reduce into context scratch, then resize the reduced frames
        int rb[4];
        const int32_t box[4] = {r.rb[0], r.rb[1], r.rb[2], r.rb[3]};
        if ((rc = reduce_validate(d->in_w, d->in_h, C, r.fx, r.fy, box, rb)) != LANCZOS_OK) return rc;
        const size_t red_fs = (size_t)r.inner.in_w * r.inner.in_h * C;
        rc = rs_scratch(st, &st->reduced, (size_t)frames * red_fs, stream, stream_capturing(stream), last_hip);
        if (rc != LANCZOS_OK) return rc;
        const hipError_t e = reduce_launch(in, (uint8_t*)st->reduced.p, d->in_w, C, r.fx, r.fy, rb, frames, in_fs_r, red_fs, stream);
        if (e != hipSuccess) {
            *last_hip = (int)e;
            return LANCZOS_ERR_HIP;
        }
        return resize_inner(st, &r.inner, r.h, r.v, w, (const uint8_t*)st->reduced.p, (uint8_t*)d_out, frames, red_fs, out_fs,
                            stream, last_kernel, last_hip, tc, nullptr, dc);   // (dc->unpack_only: set above)
    }
    return resize_inner(st, d, r.h, r.v, w, in, (uint8_t*)d_out, frames, in_fs, out_fs, stream, last_kernel, last_hip, tc, sc, dc);
}

// staging buffers of the host entry points (resize and reduce)
static hipError_t rs_grow_stage(ResizeState* st, void** p, size_t* have, size_t need, hipStream_t stream) {
    if (*have >= need) return hipSuccess;
    if (*p) {
        rs_retire(st->retired, *p, {stream});
        *p = nullptr;
        *have = 0;
    }
    const hipError_t e = hipMalloc(p, need);
    if (e == hipSuccess) *have = need;
    else *p = nullptr;
    return e;
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
    hipError_t e = rs_grow_stage(st, &st->stage_in, &st->stage_in_bytes, in_need, stream);
    if (e == hipSuccess) e = rs_grow_stage(st, &st->stage_out, &st->stage_out_bytes, out_bytes, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(st->stage_in, in, in_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && x.table)
        e = hipMemcpyAsync((uint8_t*)st->stage_in + x.table_at, x.table, x.table_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && x.flips)
        e = hipMemcpyAsync((uint8_t*)st->stage_in + x.flips_at, x.flips, x.flips_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && x.origins)
        e = hipMemcpyAsync((uint8_t*)st->stage_in + x.origins_at, x.origins, x.origins_bytes, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && x.out_up) e = hipMemcpyAsync(st->stage_out, out, out_bytes, hipMemcpyHostToDevice, stream);
    int rc = LANCZOS_OK;
    if (e == hipSuccess) {
        rc = call();
        if (rc == LANCZOS_OK) e = hipMemcpyAsync(out, st->stage_out, out_bytes, hipMemcpyDeviceToHost, stream);
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

int resize_host(ResizeState* st, const lanczos_resize_desc* d, const lanczos_resize_opts* o, const lanczos_resize_window* win,
                const void* in, void* out, int frames, hipStream_t stream, int* last_kernel, int* last_hip, RsSourceCall* sc,
                RsDestCall* dc) {
    const size_t B = (size_t)resize_bps(d);
    if ((((uintptr_t)in | (uintptr_t)out) & (B - 1)) != 0) return LANCZOS_ERR_BAD_ARG;
    RsWindow w;
    const int rc = resize_window_resolve(d, win, &w);
    if (rc != LANCZOS_OK) return rc;
    const size_t in_bytes = (sc ? sc->s.extent : (size_t)d->in_w * d->in_h * d->channels * B) * frames;
    const size_t out_bytes = dc ? dc->s.extent * (frames - 1) + dc->s.named : (size_t)w.w * w.h * d->channels * B * frames;
    RsStagedExtra x;
    x.out_up = dc != nullptr;   // the bytes the layout does not name keep what they held
    return rs_staged_call(st, in, in_bytes, out, out_bytes, x, stream, last_hip, [&] {
        return resize_device(st, d, o, win, st->stage_in, st->stage_out, frames, 0, 0, stream, last_kernel, last_hip, nullptr, sc, dc);
    });
}

// The table rides behind the input frames in the input staging block, and behind it the flip array of a view.  The element
// frames go up before they come back, so that the elements of `out` the strides leave out keep what they held.
int resize_tensor_host(ResizeState* st, const lanczos_resize_desc* d, const lanczos_resize_opts* o,
                       const lanczos_resize_window* win, const RsTensorOut& t, const void* in, void* out, int frames,
                       hipStream_t stream, int* last_kernel, int* last_hip, int* route, const int32_t* origins, RsSourceCall* sc) {
    if (((uintptr_t)out & (uintptr_t)(t.elem - 1)) != 0) return LANCZOS_ERR_BAD_ARG;
    RsWindow w;
    const int wrc = resize_window_resolve(d, win, &w);
    if (wrc != LANCZOS_OK) return wrc;
    RsTensorCall tc;
    tc.t = t;
    tc.extent_bytes = tensor_extent_bytes(d, w, t);
    const size_t in_bytes = (sc ? sc->s.extent : (size_t)d->in_w * d->in_h * d->channels) * frames;
    RsStagedExtra x;
    x.table = t.d_lut, x.table_at = (in_bytes + 255) & ~(size_t)255, x.table_bytes = (size_t)t.out_channels * 256 * t.elem;
    if (t.d_flip) x.flips = t.d_flip, x.flips_at = x.table_at + x.table_bytes, x.flips_bytes = (size_t)frames;
    if (origins) {
        x.origins = origins, x.origins_bytes = (size_t)frames * 8;
        x.origins_at = (x.table_at + x.table_bytes + x.flips_bytes + 3) & ~(size_t)3;
    }
    x.out_up = true;
    return rs_staged_call(st, in, in_bytes, out, tc.extent_bytes * frames, x, stream, last_hip, [&] {
        tc.t.d_lut = (const uint8_t*)st->stage_in + x.table_at;
        if (t.d_flip) tc.t.d_flip = (const uint8_t*)st->stage_in + x.flips_at;
        if (origins) tc.d_origin = (const int32_t*)((const uint8_t*)st->stage_in + x.origins_at);
        const int rc = resize_device(st, d, o, win, st->stage_in, st->stage_out, frames, 0, 0, stream, last_kernel, last_hip, &tc, sc);
        *route = tc.route;
        return rc;
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
    const hipError_t e = reduce_launch((const uint8_t*)d_in, (uint8_t*)d_out, in_w, channels, fx, fy, rb, frames, in_fs, out_fs,
                                       stream);
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
        return reduce_device(st, in_w, in_h, channels, fx, fy, box, st->stage_in, st->stage_out, frames, 0, 0, stream, last_hip);
    });
}

}  // namespace lz
