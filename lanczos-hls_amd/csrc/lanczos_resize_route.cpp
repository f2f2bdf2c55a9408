// lanczos_resize_route.cpp -- the part of the resize (lanczos_resize.hpp) that needs no device, and holds no
// kernel: the validation of a descriptor, Pillow's tap tables built on the host, the options, the window and the layouts
// beside the descriptor resolved, the plan of the fused kernel, and rs_route: which launches a resolved request is, decided in
// one place.  resize_device (lanczos_resize.hip) issues what rs_route says, resize_plan_host reports it, and a host program
// can link this file alone (tests/native/resize_route_check.hip).
#include "lanczos_resize.hpp"

#include "lanczos_env.hpp"

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstring>

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

// the descriptor of a YCbCr request: three channels of B-byte samples (1, or 2 with LANCZOS_RESIZE_U16), nothing else
int ycc_desc_validate(const lanczos_resize_desc* d, int B) {
    if (!d) return LANCZOS_ERR_BAD_ARG;
    const int wide = B == 2 ? LANCZOS_RESIZE_U16 : 0;
    if ((d->reserved[0] & (LANCZOS_RESIZE_ALPHA | LANCZOS_RESIZE_U16 | LANCZOS_RESIZE_F32)) != wide) return LANCZOS_ERR_UNSUPPORTED;
    const int rc = resize_validate(d);   // (LANCZOS_FILTER_NEAREST on words: LANCZOS_ERR_UNSUPPORTED)
    if (rc != LANCZOS_OK) return rc;
    return d->channels == 3 ? LANCZOS_OK : LANCZOS_ERR_BAD_ARG;
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

// ---- the layouts beside the descriptor: tensor elements, source, destination -----------------------------------

size_t tensor_extent_bytes(const lanczos_resize_desc* d, const RsWindow& win, const RsTensorOut& t) {
    const int oc = t.out_channels ? t.out_channels : d->channels;
    return (size_t)((oc - 1) * t.chan_stride + (win.h - 1) * t.row_stride + (win.w - 1) * t.pix_stride + 1) *
           (size_t)t.elem;
}

int tensor_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win, RsTensorOut* t, const int32_t* reserved) {
    int rc = resize_validate(d);
    if (rc != LANCZOS_OK) return rc;
    RsWindow w;   // the frame the strides describe
    if ((rc = resize_window_resolve(d, win, &w)) != LANCZOS_OK) return rc;
    if (!t || (!t->d_lut && !t->norm)) return LANCZOS_ERR_BAD_ARG;   // (a norm request has no table)
    for (int i = 0; i < 4; i++)
        if (reserved[i] != 0) return LANCZOS_ERR_BAD_ARG;
    // the channel map: out_channels 0 is every channel in its place.  Injective, and nothing set behind out_channels
    if (t->elem != 2 && t->elem != 4) return LANCZOS_ERR_BAD_ARG;
    if (t->out_channels == 0) {
        t->out_channels = d->channels;
        for (int c = 0; c < 4; c++) t->src_channel[c] = c < d->channels ? c : 0;
    }
    if (t->out_channels < 1 || t->out_channels > d->channels || (t->flip & ~3) != 0) return LANCZOS_ERR_BAD_ARG;
    bool identity = t->out_channels == d->channels;
    for (int oc = 0; oc < 4; oc++) {
        const int sc = t->src_channel[oc];
        if (oc >= t->out_channels ? sc != 0 : (sc < 0 || sc >= d->channels)) return LANCZOS_ERR_BAD_ARG;
        for (int k = 0; k < oc && oc < t->out_channels; k++)
            if (t->src_channel[k] == sc) return LANCZOS_ERR_BAD_ARG;
        if (oc < t->out_channels && sc != oc) identity = false;
    }
    t->mapped = !identity || t->flip != 0 || t->d_flip != nullptr;
    // a table serves 8-bit samples and no others; 16-bit and float samples have the request that computes its elements
    // (lanczos_tensor_norm, tensor_norm_validate), which in turn takes no 8-bit ones
    if (((d->reserved[0] & (LANCZOS_RESIZE_U16 | LANCZOS_RESIZE_F32)) != 0) != t->norm) return LANCZOS_ERR_UNSUPPORTED;
    struct Dim {
        int64_t stride, extent;
    } dims[3] = {{t->chan_stride, t->out_channels}, {t->row_stride, w.h}, {t->pix_stride, w.w}};
    constexpr int64_t kMaxStride = (int64_t)1 << 40;   // stride x extent stays far inside int64
    for (const Dim& m : dims)
        if (m.stride <= 0 || m.stride > kMaxStride) return LANCZOS_ERR_BAD_ARG;
    // no two (c, y, x) share an address: by rising stride, each stride covers the whole extent of the one before.  An axis of
    // extent 1 never moves, so its stride takes no part
    std::sort(dims, dims + 3, [](const Dim& a, const Dim& b) { return a.stride < b.stride; });
    int64_t covered = 1;   // elements the axes so far span
    for (const Dim& m : dims) {
        if (m.extent == 1) continue;
        if (m.stride < covered) return LANCZOS_ERR_BAD_ARG;
        covered = m.stride * m.extent;
    }
    return LANCZOS_OK;
}

int tensor_view_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win, const lanczos_tensor_view* v,
                         RsTensorOut* lay) {
    if (v) {
        *lay = RsTensorOut{v->d_lut, v->chan_stride, v->row_stride, v->pix_stride, v->elem_bytes, v->out_channels};
        for (int c = 0; c < 4; c++) lay->src_channel[c] = v->src_channel[c];
        lay->flip = v->flip, lay->d_flip = v->d_flip;
        // 0 channels is no view (and stands for "all of them" inside): refused here, once the descriptor has been looked at
        if (v->out_channels == 0) {
            const int rc = resize_validate(d);
            return rc != LANCZOS_OK ? rc : LANCZOS_ERR_BAD_ARG;
        }
    }
    return tensor_validate(d, win, v ? lay : nullptr, v ? v->reserved : nullptr);
}

int tensor_norm_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win, const lanczos_tensor_norm* n,
                         RsTensorOut* lay) {
    if (n) {
        const bool known = n->format == LANCZOS_TENSOR_F32 || n->format == LANCZOS_TENSOR_BF16 || n->format == LANCZOS_TENSOR_F16;
        *lay = RsTensorOut{nullptr, n->chan_stride, n->row_stride, n->pix_stride, n->format == LANCZOS_TENSOR_F32 ? 4 : 2, n->out_channels};
        for (int c = 0; c < 4; c++)
            lay->src_channel[c] = n->src_channel[c], lay->div[c] = n->div[c], lay->mean[c] = n->mean[c], lay->std[c] = n->std[c];
        lay->flip = n->flip, lay->d_flip = n->d_flip;
        lay->norm = true, lay->format = n->format;
        // an unknown format and 0 channels (no view, as above) are refused once the descriptor has been looked at
        if (!known || n->out_channels == 0) {
            const int rc = resize_validate(d);
            return rc != LANCZOS_OK ? rc : LANCZOS_ERR_BAD_ARG;
        }
    }
    return tensor_validate(d, win, n ? lay : nullptr, n ? n->reserved : nullptr);
}

int resize_source_resolve(const lanczos_resize_desc* d, const lanczos_resize_source* src, RsSource* s) {
    const long long C = d->channels, B = resize_bps(d);
    const long long tight_row = (long long)d->in_w * C * B;
    *s = RsSource{false, true, (size_t)tight_row, (size_t)B, (size_t)(d->in_h * tight_row)};
    if (!src) return LANCZOS_OK;
    for (int32_t r : src->reserved)
        if (r != 0) return LANCZOS_ERR_BAD_ARG;
    const long long rs = src->row_stride, cs = src->chan_stride, ps = src->pix_stride;
    if (rs < 1 || cs < 1 || ps < 1 || rs % B != 0) return LANCZOS_ERR_BAD_ARG;
    // a plane of in_h pitched rows: what chan_stride has to clear.  rs * in_h stays far below 2^63 only for a sane pitch
    if (rs > ((long long)1 << 40)) return LANCZOS_ERR_BAD_ARG;
    const long long plane = (d->in_h - 1) * rs + (long long)d->in_w * B;
    const bool planar_shape = ps == B && rs >= (long long)d->in_w * B && cs >= plane && cs <= ((long long)1 << 56);
    if (ps == C * B && cs == B && rs >= tight_row) {   // interleaved; with one channel this is every planar source as well
        s->row_stride = (size_t)rs, s->tight = rs == tight_row, s->extent = (size_t)(d->in_h * rs);
        return LANCZOS_OK;
    }
    if (!planar_shape) return LANCZOS_ERR_BAD_ARG;
    if (C == 1) {   // one plane: the interleaved shape, whatever chan_stride says
        s->row_stride = (size_t)rs, s->tight = rs == tight_row, s->extent = (size_t)(d->in_h * rs);
        return LANCZOS_OK;
    }
    if (B != 1) return LANCZOS_ERR_UNSUPPORTED;   // planar wide samples: frames * C one-channel frames for the plain entries
    s->planar = true, s->tight = false;
    s->row_stride = (size_t)rs, s->chan_stride = (size_t)cs, s->extent = (size_t)(C * cs);
    return LANCZOS_OK;
}

int resize_dest_resolve(const lanczos_resize_desc* d, const RsWindow& w, const lanczos_resize_dest* dst, RsDest* s) {
    const long long C = d->channels, B = resize_bps(d);
    const long long tight_row = (long long)w.w * C * B;
    *s = RsDest{false, true, (size_t)tight_row, (size_t)B, (size_t)(w.h * tight_row), (size_t)(w.h * tight_row)};
    if (!dst) return LANCZOS_OK;
    for (int32_t r : dst->reserved)
        if (r != 0) return LANCZOS_ERR_BAD_ARG;
    const long long rs = dst->row_stride, cs = dst->chan_stride, ps = dst->pix_stride;
    if (rs < 1 || cs < 1 || ps < 1 || rs % B != 0) return LANCZOS_ERR_BAD_ARG;
    // a plane of h pitched rows: what chan_stride has to clear.  rs * h stays far below 2^63 only for a sane pitch
    if (rs > ((long long)1 << 40)) return LANCZOS_ERR_BAD_ARG;
    const long long plane = (w.h - 1) * rs + (long long)w.w * B;
    const bool planar_shape = ps == B && rs >= (long long)w.w * B && cs >= plane && cs <= ((long long)1 << 56);
    const auto interleaved = [&] {
        s->row_stride = (size_t)rs, s->tight = rs == tight_row;
        s->extent = (size_t)(w.h * rs), s->named = (size_t)((w.h - 1) * rs + tight_row);
        return LANCZOS_OK;
    };
    if (ps == C * B && cs == B && rs >= tight_row) return interleaved();   // with one channel: every planar destination as well
    if (!planar_shape) return LANCZOS_ERR_BAD_ARG;
    if (C == 1) return interleaved();             // one plane: the interleaved shape, whatever chan_stride says
    if (B != 1) return LANCZOS_ERR_UNSUPPORTED;   // planar wide samples: frames * C one-channel frames for the plain entries
    s->planar = true, s->tight = false;
    s->row_stride = (size_t)rs, s->chan_stride = (size_t)cs;
    s->extent = (size_t)(C * cs), s->named = (size_t)((C - 1) * cs + plane);
    return LANCZOS_OK;
}

// ---- planning ----------------------------------------------------------------------------------------------------

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

// ---- the route ------------------------------------------------------------------------------------------------------

// What a resolved request launches.  q.r->inner describes the frames the resize reads (the caller's, or the reduced ones), and
// the tables are those of its full axes: a window changes which slice of them the plan and every launch see, nothing else.
//   tensor   where the fused kernel runs it stores the elements itself (LANCZOS_TENSOR_FUSED); everything else writes its bytes
//            to context scratch and k_rs_to_tensor follows
//   norm     a tensor request of wide samples: the same rule with the kRsNorm instances and k_rs_to_tensor_norm, which reads the
//            caller's frames where no pass runs and there is no window
//   crops    q.win is (0, 0, w, h).  The fused kernel runs on the plan that holds for every origin; everything else resizes the
//            whole output into context scratch and k_rs_to_tensor_crops gathers each frame's window from it -- or from the
//            caller's frames where no pass runs
//   source   where the fused kernel runs and has the staging for it, it reads the frames as they lie (LANCZOS_SOURCE_DIRECT);
//            everything else, the reduction in front included, gets them packed into context scratch first
//   dest     where the fused kernel runs it stores pitched rows and planes itself (LANCZOS_DEST_DIRECT); everything else stores
//            the tightly packed window in context scratch and k_rs_unpack_dest scatters it.  A request with a reducing gap is
//            unpacked whatever resizes the reduced frames, as its source is packed for the reduction
RsRoute rs_route(const RsRouteQuery& q) {
    RsRoute rt;
    const RsResolved& r = *q.r;
    const lanczos_resize_desc* d = &r.inner;
    const int C = d->channels, force = q.force, frames = q.frames;
    const size_t B = (size_t)resize_bps(d);   // bytes per sample
    const auto refuse = [&](int err) {
        rt = RsRoute();
        rt.err = err;
        return rt;
    };
    if (q.dst && q.tensor) return refuse(LANCZOS_ERR_BAD_ARG);
    // a layout that is given but tight is the call without it, reported as DIRECT
    const RsSource* const given = q.src && !q.src->tight ? q.src : nullptr;
    const RsDest* const dst = q.dst && !q.dst->tight ? q.dst : nullptr;
    if (q.src) rt.source_route = LANCZOS_SOURCE_DIRECT;
    if (q.dst) rt.dest_route = LANCZOS_DEST_DIRECT;
    rt.reduce = r.reduces();
    if (rt.reduce) rt.reduced.fs = (size_t)d->in_w * d->in_h * C, rt.reduced.bytes = (size_t)frames * rt.reduced.fs;
    const bool need_h = r.need_h, need_v = r.need_v;
    const bool alpha = (d->reserved[0] & LANCZOS_RESIZE_ALPHA) != 0;
    // the gather reads both index tables, also that of an axis that keeps its size (the identity) -- unless both do
    const bool nearest = resize_nearest(d) && (need_h || need_v);
    // Pillow's order for a tall frame that shrinks: never the fused kernel, the pass kernels vertical first
    const bool v_first = rs_vertical_first(d, need_h, need_v);
    const bool crops = q.crops;
    const RsWindow whole{0, 0, d->out_w, d->out_h};
    rt.win = q.win;

    // the source as the fused kernel would read it: the reduction reads packed frames; a planar one needs the instances, which
    // crops have none of, and AUTO's leave
    const RsSource* src = rt.reduce ? nullptr : given;
    // ALPHA stages whole pixels and shifts them by the frame's residue: rows whose pitch is no dword multiple need the instances
    // that shift by the row's, which crops have none of either
    const bool rowshift = src && !src->planar && alpha && (src->row_stride & 3) != 0;
    if (src && (force == LANCZOS_RESIZE_CONVERT || force == LANCZOS_RESIZE_TWO_PASS || (rowshift && crops) ||
                (src->planar && (crops || (force == LANCZOS_RESIZE_AUTO && !kRsPlanarAutoDirect)))))
        src = nullptr;
    const auto plan = [&](const RsWindow& w, bool any_origin, size_t extent) {
        if (nearest || !need_h || !need_v || v_first) return false;
        return any_origin ? rs_fused_plan_crops(d, rs_axis_view(*q.H, 0, d->out_w), rs_axis_view(*q.V, 0, d->out_h), w.w, w.h, frames,
                                                &rt.fp, extent)
                          : rs_fused_plan(d, rs_axis_view(*q.H, w.x0, w.w), rs_axis_view(*q.V, w.y0, w.h), frames, &rt.fp, extent);
    };
    bool fused_ok = src ? plan(rt.win, crops, src->extent) : false;
    if (!fused_ok) src = nullptr, fused_ok = plan(rt.win, crops, 0);   // no source, or one the kernel cannot address: the packed frame's plan
    if (force == LANCZOS_RESIZE_FUSED && !fused_ok) return refuse(LANCZOS_ERR_UNSUPPORTED);
    bool fused = fused_ok && force != LANCZOS_RESIZE_TWO_PASS;
    // 32-bit buffer offsets into the element frame: a larger one is converted, and refused where the fused kernel is forced
    const bool t_fits = q.tensor && q.extent_bytes < ((size_t)1 << 31);
    if (q.tensor && force == LANCZOS_RESIZE_FUSED && !t_fits) return refuse(LANCZOS_ERR_UNSUPPORTED);
    const bool t_fused = fused && t_fits && force != LANCZOS_RESIZE_CONVERT;
    const bool crops_gather = crops && !t_fused;
    if (crops_gather || !fused) src = nullptr;   // the fused kernel alone reads a source as it lies
    rt.src_direct = src != nullptr;
    if (given) {
        rt.source_route = src ? LANCZOS_SOURCE_DIRECT : LANCZOS_SOURCE_PACKED;
        rt.pack = !src;
        if (rt.pack) {
            rt.packed.fs = ((size_t)q.d->in_w * q.d->in_h * C * B + 3) & ~(size_t)3;
            rt.packed.bytes = (size_t)frames * rt.packed.fs;
        }
    }
    const bool crops_direct = crops_gather && !nearest && !need_h && !need_v;   // no pass runs: the caller's frames are the bytes
    if (crops_gather) {   // the bytes of the whole output, by the plan of the whole output
        rt.win = whole;
        fused = plan(whole, false, 0) && force != LANCZOS_RESIZE_TWO_PASS;
    }
    const RsWindow& win = rt.win;
    if (q.tensor) {
        rt.tensor_route = t_fused ? LANCZOS_TENSOR_FUSED : LANCZOS_TENSOR_CONVERTED;
        rt.follower = crops_direct ? kRsFollowCropsDirect : crops_gather ? kRsFollowCropsScratch : t_fused ? kRsFollowNone
                      : q.norm     ? kRsFollowToTensorNorm : kRsFollowToTensor;
        // a norm request that changes neither axis and has no window: the caller's frames are the samples, read where they lie
        rt.follow_src = q.norm && !t_fused && !nearest && !need_h && !need_v && win.whole(d);
        if (!t_fused && !crops_direct && !rt.follow_src) {
            rt.tensor_bytes.fs = ((size_t)win.w * win.h * C * (q.norm ? B : 1) + 3) & ~(size_t)3;
            rt.tensor_bytes.bytes = (size_t)frames * rt.tensor_bytes.fs;
        }
    }
    if (dst) {
        // 32-bit buffer offsets into the pitched frame, whose range the kernel takes as rows x pitch.  A planar destination has
        // instances of its own (8-bit, three or four channels), none of them with the row shift of an ALPHA source pitched off a
        // dword: that one keeps its direct staging and is unpacked
        rt.dst_direct = fused && !rt.reduce && force != LANCZOS_RESIZE_CONVERT &&
                        std::max(dst->named, (size_t)win.h * dst->row_stride) < ((size_t)1 << 31) &&
                        (!dst->planar || ((force != LANCZOS_RESIZE_AUTO || kRsPlanarOutAutoDirect) && !(src && rowshift)));
        rt.dest_route = rt.dst_direct ? LANCZOS_DEST_DIRECT : LANCZOS_DEST_UNPACKED;
        if (!rt.dst_direct) {   // the packed window, readable a few dwords past its end (k_rs_unpack_dest)
            rt.unpacked.fs = ((size_t)win.w * win.h * C * B + 3) & ~(size_t)3;
            rt.unpacked.bytes = (size_t)frames * rt.unpacked.fs + 32;
        }
    }
    // two passes: the horizontal one produces the rows the vertical taps read and no others, mid_rows of them from source row
    // mid_row0 on, and the scratch holds exactly those.  Of a crops request these are the whole output's, which the converted
    // route resizes
    if (need_h && need_v && !nearest) rs_mid_rows(crops ? rs_axis_view(*q.V, 0, d->out_h) : rs_axis_view(*q.V, win.y0, win.h), &rt.mid_row0, &rt.mid_rows);
    rt.kernel = LANCZOS_KERNEL_RESIZE_TWO_PASS;
    if (fused) {
        const int t = t_fused ? q.elem : 0, tm = t_fused ? q.elem + kRsMapped : 0;
        rt.main = kRsMainFused, rt.kernel = LANCZOS_KERNEL_RESIZE_FUSED;
        rt.flags = t_fused && q.norm           ? kRsNorm
                   : rt.dst_direct && dst->planar ? kRsPlanarOut + (src && src->planar ? kRsPlanar : 0)
                   : src && src->planar      ? tm + kRsPlanar
                   : src && rowshift         ? tm + kRsRowShift
                   : t_fused && crops        ? tm + kRsCrops
                   : t_fused && q.mapped     ? tm
                                             : t;
        rt.bps = rt.flags && rt.flags != kRsNorm ? 1 : (int)B;   // every instance with another flag is an 8-bit one
        assert(rs_fused_instance_exists(rt.bps, rt.flags));     // an entry of LZ_RS_FUSED_INSTANCES, not rs_launch_fused_any's default
    } else if (nearest) {
        rt.main = kRsMainNearest, rt.kernel = LANCZOS_KERNEL_RESIZE_NEAREST;
    } else if (!need_h && !need_v) {   // Pillow returns a copy (also of RGBA: no premultiply round trip); a window crops it
        rt.main = crops_direct || rt.follow_src ? kRsMainNone : win.whole(d) ? kRsMainCopy : kRsMainCrop;
    } else if (v_first) {   // win.h rows of the source's full width in between
        rt.main = kRsMainVFirst;
        rt.scratch.fs = (size_t)win.h * d->in_w * C * B;
    } else {
        rt.main = need_h && need_v ? kRsMainTwoPass : need_h ? kRsMainPassH : kRsMainPassV;
        if (need_h && need_v) rt.scratch.fs = (size_t)rt.mid_rows * win.w * C * B;
    }
    rt.scratch.bytes = (size_t)frames * rt.scratch.fs;
    return rt;
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
    // the tables planning reads: none of the index tables, none of an idle axis, the horizontal one only beside the vertical one
    ResizeAxisHost H, V;
    if (filter != LANCZOS_FILTER_NEAREST && r.need_v) {
        if (!resize_build_axis(r.inner.in_h, r.inner.out_h, d->a, filter, r.v, &V, u16)) return LANCZOS_ERR_UNSUPPORTED;
        if (r.need_h && !resize_build_axis(r.inner.in_w, r.inner.out_w, d->a, filter, r.h, &H, u16)) return LANCZOS_ERR_UNSUPPORTED;
    }
    // AUTO's route for bytes out; a crops request is a tensor one (the element does not change the plan)
    RsRouteQuery q;
    q.d = d, q.r = &r, q.frames = frames, q.H = &H, q.V = &V;
    q.win = crops ? RsWindow{0, 0, crops->w, crops->h} : w;
    if (crops) q.tensor = q.crops = q.mapped = true, q.elem = 4;
    const RsRoute rt = rs_route(q);
    out->mid_row0 = rt.mid_row0, out->mid_rows = rt.mid_rows;
    if (rt.main != kRsMainFused || rt.follower != kRsFollowNone) return LANCZOS_OK;   // (a crops gather: no plan for every origin)
    lanczos_resize_plan* in = &out->inner;
    in->fused = 1;
    in->K = rt.fp.K, in->strips = rt.fp.strips, in->rows_per_chunk = rt.fp.rows_per_chunk, in->chunks = rt.fp.chunks;
    in->ring_rows = rt.fp.ring_rows, in->stage_rows = rt.fp.stage_rows, in->stage_dw = rt.fp.stage_dw;
    in->lds_bytes = (int32_t)rt.fp.lds;
    return LANCZOS_OK;
}

}  // namespace lz
