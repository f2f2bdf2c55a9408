// lanczos_resize.hpp -- resize to any size with Pillow's contract (include/lanczos_hip.h, lanczos_resize_*): host tap tables,
// their per-context cache, and the entry points lanczos_api.hip forwards to.  What needs no device is in lanczos_resize_route.cpp:
// validation, tables, resolution, planning and rs_route, the one decision of what a request launches.  The table cache, the
// scratch, the executor of a route (resize_device), the staging of the host entries and the alpha pass kernels are in
// lanczos_resize.hip.  The kernels are written once for 8-bit, 16-bit (LANCZOS_RESIZE_U16) and float (LANCZOS_RESIZE_F32)
// samples in lanczos_resize_fused.hpp; LZ_RS_FUSED_INSTANCES below lists the fused instances and says which unit compiles what
// (the converter of lanczos_tensor_norm is in lanczos_resize_tensor_norm.hip).  YCbCr frames (lanczos_resize_ycc_*,
// lanczos_resize_ycc_out, lanczos_resize_ycc16) are one-channel requests through resize_device with a split in front and a join
// or a merge behind, one composition for the three families in lanczos_resize_ycc.hip; their host-only part is
// lanczos_resize_ycc_layout.cpp (the section at the end of this file).  The filter of a request (LANCZOS_RESIZE_FILTER)
// only changes the tables; LANCZOS_FILTER_NEAREST has index tables and a kernel of its own (lanczos_resize_nearest.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/lanczos_hip.h"
#include "lanczos_cache.hpp"

namespace lz {

constexpr int kResizePrecision = 22;   // Pillow's PRECISION_BITS for 8-bit samples (32 - 8 - 2)
constexpr int kResizeMaxSize = 65535;

int resize_validate(const lanczos_resize_desc* d);

// Fixed-point tables of one axis, computed on the host in double exactly as Pillow's precompute_coeffs +
// normalize_coeffs_8bpc do.  Returns false if a coefficient or an accumulator could leave the ranges the kernels rely on
// (|coeff| < 2^23 for the 24-bit multiply, 255 * sum|coeff| + 2^21 < 2^31); no shape met so far does.
struct ResizeAxisHost {
    int in_n = 0, out_n = 0, a = 0, filter = 0, ksize = 0;
    double scale = 1.0;                          // source pixels per output pixel: the box's extent / out_n
    std::vector<int32_t> first, count, coeffs;   // [out_n], [out_n], [out_n][ksize]
    std::vector<double> coeffs64;                // [out_n][ksize]: the 16-bit and float paths' tables, which have no `coeffs`
};
// The source interval of one axis as Pillow's C sees it: both ends rounded to float.  The whole axis is (0, in_n).
struct RsSpan {
    float b0 = 0.0f, b1 = 0.0f;
};
inline RsSpan rs_full_span(int in_n) { return RsSpan{0.0f, (float)in_n}; }
// the pass rule: an axis runs its pass iff it changes size or its span is not the whole axis
inline bool rs_axis_runs(int in_n, int out_n, RsSpan s) { return out_n != in_n || s.b0 != 0.0f || s.b1 != (float)in_n; }
// The order rule, Pillow 12.2.0's Image.resize: a frame more than 100 times as tall as wide that shrinks in height runs the
// vertical pass first, over the full width, and the horizontal pass on its result.  d is the request the resize runs on: the
// reduced frame under a reducing_gap (RsResolved::inner).  It only matters where both passes run, and never for NEAREST
inline bool rs_vertical_first(const lanczos_resize_desc* d, bool need_h, bool need_v) {
    return need_h && need_v && LANCZOS_RESIZE_FILTER_OF(d->reserved[0]) != LANCZOS_FILTER_NEAREST && d->in_h > 100 * d->in_w &&
           d->out_h < d->in_h;
}
// the filter of a request (LANCZOS_FILTER_*) and the support S of its weight function, which stands where Lanczos has a
inline int resize_filter(const lanczos_resize_desc* d) { return LANCZOS_RESIZE_FILTER_OF(d->reserved[0]); }
inline bool resize_nearest(const lanczos_resize_desc* d) { return resize_filter(d) == LANCZOS_FILTER_NEAREST; }
inline double rs_filter_support(int filter, int a) {
    return filter == LANCZOS_FILTER_BOX ? 0.5 : filter == LANCZOS_FILTER_BICUBIC ? 2.0 : filter == LANCZOS_FILTER_LANCZOS ? (double)a : 1.0;
}
int resize_ksize(int in_n, int out_n, int a, int filter, RsSpan s);
// f64: the tables of the 16-bit path instead -- the normalised weights as they are (Pillow's precompute_coeffs alone),
// in coeffs64; always true.  LANCZOS_FILTER_NEAREST: first = Pillow's source index of every output (a running sum), count = 1,
// ksize = 1, the coefficient 2^22 or 1.0; false if an index leaves the source.
bool resize_build_axis(int in_n, int out_n, int a, int filter, RsSpan s, ResizeAxisHost* t, bool f64 = false);

// A request with its options resolved (lanczos_resize_opts; NULL = the full box, no gap): the reduction in front of the
// resize, if any, and the resize that remains -- `inner` is the caller's descriptor, or one whose source is the reduced frame.
struct RsResolved {
    int fx = 1, fy = 1;
    int rb[4] = {0, 0, 0, 0};   // the safe box the reduction covers (the whole frame without one)
    lanczos_resize_desc inner{};
    double inner_box[4] = {0, 0, 0, 0};
    RsSpan h, v;                // inner_box rounded to float, per axis
    bool need_h = false, need_v = false;
    bool reduces() const { return fx > 1 || fy > 1; }
};
int resize_resolve(const lanczos_resize_desc* d, const lanczos_resize_opts* o, RsResolved* r);

// A window of the output (lanczos_resize_window), resolved: NULL is the whole output.  A windowed request runs the kernels of
// the full request on slices of its tables -- outputs x0 .. x0 + w of the horizontal axis, y0 .. y0 + h of the vertical one --
// so its sample (x, y) is the full request's (x0 + x, y0 + y) by construction.
struct RsWindow {
    int x0 = 0, y0 = 0, w = 0, h = 0;
    bool whole(const lanczos_resize_desc* d) const { return x0 == 0 && y0 == 0 && w == d->out_w && h == d->out_h; }
};
int resize_window_resolve(const lanczos_resize_desc* d, const lanczos_resize_window* win, RsWindow* w);
// `n` outputs of an axis from output `o0` on: what planning reads of the tables
struct RsAxisView {
    const int32_t *first, *count;
    int n, ksize;
    double scale;
};
inline RsAxisView rs_axis_view(const ResizeAxisHost& t, int o0, int n) {
    return RsAxisView{t.first.data() + o0, t.count.data() + o0, n, t.ksize, t.scale};
}
// the rows of the inner source the horizontal pass of the two-pass path produces: what the vertical taps of V's outputs read
inline void rs_mid_rows(const RsAxisView& V, int* row0, int* rows) {
    *row0 = V.first[0];
    *rows = V.first[V.n - 1] + V.count[V.n - 1] - *row0;
}
// the source rectangle (x0, y0, x1, y1) a windowed request's result depends on (lanczos_resize_window_source)
int resize_window_source(const lanczos_resize_desc* d, const lanczos_resize_opts* o, const lanczos_resize_window* win,
                         int32_t rect[4]);

inline bool resize_u16(const lanczos_resize_desc* d) { return (d->reserved[0] & LANCZOS_RESIZE_U16) != 0; }
inline bool resize_f32(const lanczos_resize_desc* d) { return (d->reserved[0] & LANCZOS_RESIZE_F32) != 0; }
// bytes per sample: 1, 2 (LANCZOS_RESIZE_U16) or 4 (LANCZOS_RESIZE_F32); samples wider than a byte run on the double tables
inline int resize_bps(const lanczos_resize_desc* d) { return resize_f32(d) ? 4 : resize_u16(d) ? 2 : 1; }

// launch geometry the translation units share
constexpr int kRsThreads = 256;
constexpr int kRsOB = 8;             // output rows per march step of the fused kernels
constexpr int kRsLoadBatch = 16;     // staging loads in flight per thread
constexpr int kRsFusedMaxLds = 80 * 1024;   // at least two fused workgroups per CU (160 KiB of LDS)
constexpr int kRsRowsPerChunkMin = 4 * kRsOB;
constexpr int kRsTargetWgs = 2048;
// Where a launcher issues and what it has issued: the stream, and the launches (kernels and copies) that went out on it, counted
// where each goes out.  Every launcher below takes one in place of a stream
struct RsIssue {
    hipStream_t stream = nullptr;
    int launches = 0;
};
// A grid dimension holds at most 65535 frames, so a batch goes out in groups of that many: launch(f0, nf) issues exactly one
// launch for the nf frames from f0 on
constexpr int kRsMaxGridFrames = 65535;
template <class F>
hipError_t rs_for_frame_groups(RsIssue& is, int frames, F&& launch) {
    for (int f0 = 0; f0 < frames; f0 += kRsMaxGridFrames) {
        launch(f0, frames - f0 < kRsMaxGridFrames ? frames - f0 : kRsMaxGridFrames);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        is.launches++;
    }
    return hipSuccess;
}
// horizontal tap counts with a fused instance (a request runs on the smallest one >= its ksize, zero-padded), for every
// sample width.  3 and 5 serve the upscales of the short filters (box and bilinear: ksize 3, bicubic: 5) and only them: a
// Lanczos request keeps the instance it always had (a = 2 upscales, ksize 5, run on 7).  LANCZOS_RS_NO_SMALL_BUCKETS=1 pads
// the short filters to 7 too
#define LZ_RS_BUCKETS(X) X(3) X(5) X(7) X(9) X(11) X(13) X(17) X(25)
// output pixels per strip of the fused kernels by channels and bytes per sample: ring rows of 256 / 768 / 256 bytes (8-bit),
// 256 / 768 / 512 bytes (16-bit), 512 / 768 / 1024 bytes (float)
constexpr int rs_strip_width(int channels, int bps) {
    return bps == 4 ? (channels == 1 ? 128 : 64) : channels == 4 ? 64 : bps == 2 ? 128 : 256;
}

// The fused kernel's launch shape for a request (false: it cannot run it).  H and V are the tables of the two axes, both of
// which run, cut to the window: the output is H.n x V.n pixels (d's out_w / out_h are not read).  lanczos_resize_device plans
// with it; lanczos_resize_plan_host reports what it returns.
struct RsFusedPlan {
    int K = 0, strips = 0, rows_per_chunk = 0, chunks = 0, ring_rows = 0, stage_rows = 0, stage_dw = 0;
    size_t lds = 0;
};
// src_extent: the bytes of a source frame as the kernel addresses it, where that is not the packed frame (0)
bool rs_fused_plan(const lanczos_resize_desc* d, const RsAxisView& H, const RsAxisView& V, int frames, RsFusedPlan* fp,
                   size_t src_extent = 0);
// The plan of a w x h window whose origin is only known when the kernel runs (lanczos_resize_crops).  H and V are the full
// axes.  K, strips, rows_per_chunk and chunks depend on the window's size alone; stage_dw is the largest over every x origin
// and ring_rows the largest over every y origin of what rs_fused_plan computes for the window there; stage_rows and lds follow
// from those by its rule.  false where that does not fit, even if the window at some origins would
bool rs_fused_plan_crops(const lanczos_resize_desc* d, const RsAxisView& H, const RsAxisView& V, int w, int h, int frames,
                         RsFusedPlan* fp, size_t src_extent = 0);
// crops: the plan of a request with a crop origin per frame (win is then NULL; mid_row0 / mid_rows are the whole output's,
// which the converted route resizes)
int resize_plan_host(const lanczos_resize_desc* d, const lanczos_resize_opts* o, const lanczos_resize_window* win, int frames,
                     lanczos_resize_plan_ex* out, const lanczos_resize_crops* crops);
// a crop size per request: 1..out_w x 1..out_h, origins given, reserved words 0
int resize_crops_validate(const lanczos_resize_desc* d, const lanczos_resize_crops* c);

// One axis shape on the device: first | count | coeffs in one block (int32 coefficients, or double ones for 16-bit samples:
// the two int32 arrays in front of them keep those 8-byte aligned).
struct ResizeAxisKey {
    int in_n, out_n, a, f64, filter;   // f64: double coefficients
    uint32_t span_bits[2];             // the bit patterns of the span's two floats: two boxes over one (in, out, a) are two entries
};
struct ResizeAxis {
    ResizeAxisHost host;
    const int32_t* dev = nullptr;   // the cache item's block
    const int32_t* first() const { return dev; }
    const int32_t* count() const { return dev + host.out_n; }
    template <class KT>   // int32_t, or double for the tables of samples wider than a byte
    const KT* coeffs() const { return (const KT*)(dev + 2 * (size_t)host.out_n); }
};

// What a context keeps for its resizes.  Callers serialise per context (ctx->mu).
struct ResizeState {
    Lifetime* const life;                    // the context's
    // 32 axis shapes, uploaded eagerly: an entry is complete from the moment it is cached
    using AxisCache = UploadCache<ResizeAxisKey, ResizeAxis>;
    AxisCache axes;
    int force = LANCZOS_RESIZE_AUTO;
    ScratchBlock scratch;                    // intermediate of the two-pass path (the rows the vertical taps read x out_w x C)
    ScratchBlock reduced;                    // the reduced frames of a request with reducing_gap, tightly packed
    ScratchBlock tensor_bytes;               // the sample result of a tensor request on the converted route (k_rs_to_tensor[_norm] reads it)
    ScratchBlock packed;                     // the tightly packed copy of a source on the PACKED route (k_rs_pack_source writes it)
    ScratchBlock unpacked;                   // the tightly packed result of a destination on the UNPACKED route (k_rs_unpack_dest reads it)
    ScratchBlock stage_in, stage_out;        // staging of lanczos_resize_host
    ScratchBlock ycc_in;                     // the Cb and Cr planes k_rs_ycc_split[16] makes of interleaved chroma (lanczos_resize_ycc.hip)
    ScratchBlock ycc_planes;                 // the resized Y, Cb and Cr planes k_rs_ycc_merge / k_rs_ycc16_merge reads
    ScratchBlock ycc_out;                    // the tight Cb and Cr planes k_rs_ycc_join[16] interleaves
    ScratchBlock ycc_rgb;                    // the tight resized RGB frames k_rs_ycc_encode reads
    explicit ResizeState(Lifetime* l) : life(l), axes(l, 32) {}
};

// The table and the layout of a tensor request, whatever its element: lanczos_tensor_out (elem 4, floats),
// lanczos_tensor16_out (elem 2, bfloat16 or float16 words) and lanczos_tensor_view (either, with a channel map and flips) are
// all this.  Strides in elements.
struct RsTensorOut {
    const void* d_lut = nullptr;   // out_channels * 256 elements
    int64_t chan_stride = 0, row_stride = 0, pix_stride = 0;
    int elem = 4;                  // bytes of an element
    // the view: output channel oc is source channel src_channel[oc].  out_channels 0 stands for every channel in its place
    // (the two structs without a map); tensor_validate fills it in
    int out_channels = 0;
    int src_channel[4] = {0, 0, 0, 0};
    int flip = 0;                      // bit 0: mirror x, bit 1: mirror y, every frame
    const uint8_t* d_flip = nullptr;   // one byte per frame, XORed with flip; read when the kernels run
    // set by tensor_validate: false where the view is the identity without flips, which runs the kernels without a map
    bool mapped = false;
    // lanczos_tensor_norm (16-bit and float samples): no table; the element is computed from the sample, cvt(((float)P / div -
    // mean) / std) per OUTPUT channel.  format: LANCZOS_TENSOR_F32 / _BF16 / _F16, elem its width
    bool norm = false;
    int format = 0;
    float div[4] = {1, 1, 1, 1}, mean[4] = {0, 0, 0, 0}, std[4] = {1, 1, 1, 1};
    // dst[c] in byte c: the output channel source channel c goes to, 255 where none does
    unsigned dst_of_src() const {
        unsigned dst = 0xffffffffu;
        for (int oc = 0; oc < out_channels; oc++) dst = (dst & ~(255u << (8 * src_channel[oc]))) | ((unsigned)oc << (8 * src_channel[oc]));
        return dst;
    }
};
// The tensor part of a request (lanczos_resize_tensor.hip): `out` and out_frame_stride of the request are then those of the
// element frames.  route: out, LANCZOS_TENSOR_FUSED or LANCZOS_TENSOR_CONVERTED once the launches are out.
struct RsTensorCall {
    RsTensorOut t;             // validated (tensor_validate)
    size_t extent_bytes = 0;   // of one element frame: from its first element to its last (set by resize_device)
    int route = 0;
    // lanczos_resize_crops: a pair (x0, y0) per frame, read and clamped when the kernels run.  The window of the call is then
    // (0, 0, w, h), the size of every frame's crop
    const int32_t* d_origin = nullptr;
};
// t NULL: the caller passed no struct; reserved: its four words.  The frame the strides describe is the window's (win NULL:
// the whole output).  On LANCZOS_OK t->out_channels, src_channel and mapped are resolved
int tensor_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win, RsTensorOut* t, const int32_t* reserved);
// the request of either public struct without a map (T): *lay is filled where there is one
template <class T>
int tensor_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win, const T* t, int elem, RsTensorOut* lay) {
    if (t) *lay = RsTensorOut{t->d_lut, t->chan_stride, t->row_stride, t->pix_stride, elem};
    return tensor_validate(d, win, t ? lay : nullptr, t ? t->reserved : nullptr);
}
// ... and of lanczos_tensor_view
int tensor_view_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win, const lanczos_tensor_view* v,
                         RsTensorOut* lay);
// ... and of lanczos_tensor_norm: the view's rules without a table, for wide samples only
int tensor_norm_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win, const lanczos_tensor_norm* n,
                         RsTensorOut* lay);
size_t tensor_extent_bytes(const lanczos_resize_desc* d, const RsWindow& win, const RsTensorOut& t);
void tensor_lut_normalize(int channels, const float* mean, const float* std, float* lut);
// float32 -> bfloat16 (LANCZOS_TENSOR_BF16) or float16 (LANCZOS_TENSOR_F16) words, round to nearest even; false: no such format
bool tensor_lut_convert16(const float* in, int n, int format, uint16_t* out);
// k_rs_to_tensor: tightly packed interleaved bytes (frames `src_fs` apart, base and stride dword multiples, readable up to the
// next dword multiple behind each frame) -> strided elements through the table
// (t.mapped: through the channel map and the frames' flips)
hipError_t rs_to_tensor_launch(const uint8_t* src, size_t src_fs, uint8_t* out, size_t out_fs, int w, int h, int channels,
                               const RsTensorOut& t, int frames, RsIssue& is);
// k_rs_to_tensor_norm (lanczos_resize_tensor_norm.hip): tightly packed interleaved samples of `bps` bytes (2 or 4; frames `src_fs`
// apart at any multiple of bps, nothing read outside a frame) -> strided elements computed from them, through the map and flips
hipError_t rs_to_tensor_norm_launch(const uint8_t* src, size_t src_fs, uint8_t* out, size_t out_fs, int w, int h, int channels,
                                    int bps, const RsTensorOut& t, int frames, RsIssue& is);
// k_rs_to_tensor_crops (lanczos_resize_tensor_crops.hip): frame f's w x h window at its clamped origin of interleaved byte frames
// of src_w x src_h pixels (rows src_pitch bytes apart, any alignment) -> strided elements through the map, flips and table
hipError_t rs_to_tensor_crops_launch(const uint8_t* src, size_t src_fs, size_t src_pitch, int src_w, int src_h, uint8_t* out,
                                     size_t out_fs, int w, int h, int channels, const RsTensorOut& t, const int32_t* d_origin,
                                     int frames, RsIssue& is);

// A source layout (lanczos_resize_source), resolved by resize_source_resolve: sample (y, x, c) of a frame lies c * chan_stride +
// y * row_stride + x * (planar ? 1 : C * B) bytes into it.  tight: interleaved with packed rows, the call without a source
struct RsSource {
    bool planar = false, tight = true;
    size_t row_stride = 0, chan_stride = 0;   // bytes; chan_stride of an interleaved source is B
    size_t extent = 0;                         // of one frame: in_h * row_stride, or channels * chan_stride
};
// src NULL: the tight interleaved layout.  Planar with one channel resolves to the interleaved shape
int resize_source_resolve(const lanczos_resize_desc* d, const lanczos_resize_source* src, RsSource* s);
// the source of a call and the route it took (LANCZOS_SOURCE_*); meaningful where the call returns LANCZOS_OK
struct RsSourceCall {
    RsSource s;
    int route = 0;
};
// AUTO takes the planar instances of the fused kernel where they exist (false: PACKED, the instances by force only); the
// measurements behind the choice are in DESIGN.md 4.5
constexpr bool kRsPlanarAutoDirect = true;
// k_rs_pack_source (lanczos_resize_source.hip): `frames` frames of w x h pixels of C samples of B bytes in layout s, in_fs
// bytes apart at any byte address, to tightly packed interleaved frames out_fs bytes apart (out and out_fs dword multiples)
hipError_t rs_pack_source_launch(const uint8_t* in, size_t in_fs, const RsSource& s, uint8_t* out, size_t out_fs, int w, int h,
                                 int C, int B, int frames, RsIssue& is);

// A destination layout (lanczos_resize_dest), resolved by resize_dest_resolve for a w x h window: sample (y, x, c) of a frame goes
// c * chan_stride + y * row_stride + x * (planar ? 1 : C * B) bytes into it.  tight: interleaved with packed rows, the call
// without a destination
struct RsDest {
    bool planar = false, tight = true;
    size_t row_stride = 0, chan_stride = 0;   // bytes; chan_stride of an interleaved destination is B
    size_t extent = 0;                         // of one frame, the default frame stride: h * row_stride, or channels * chan_stride
    size_t named = 0;                          // from a frame's first byte to the last one the layout names, + 1
};
// dst NULL: the tight interleaved layout.  Planar with one channel resolves to the interleaved shape
int resize_dest_resolve(const lanczos_resize_desc* d, const RsWindow& w, const lanczos_resize_dest* dst, RsDest* s);
// the destination of a call and the route it took (LANCZOS_DEST_*); meaningful where the call returns LANCZOS_OK
struct RsDestCall {
    RsDest s;
    int route = 0;
};
// AUTO takes the planar-out instances of the fused kernel where they exist (false: UNPACKED, the instances by force only); the
// measurements behind the choice are in DESIGN.md 4.5
constexpr bool kRsPlanarOutAutoDirect = true;
// k_rs_unpack_dest (lanczos_resize_dest.hip): `frames` tightly packed interleaved frames of w x h pixels of C samples of B bytes,
// in_fs bytes apart (in and in_fs dword multiples, readable 32 bytes past the last frame), scattered into layout s at any byte
// address, frames out_fs bytes apart.  Only bytes the layout names are written
hipError_t rs_unpack_dest_launch(const uint8_t* in, size_t in_fs, uint8_t* out, size_t out_fs, const RsDest& s, int w, int h,
                                 int C, int B, int frames, RsIssue& is);

// One resize request, as every entry of lanczos_api.hip fills it in and the entry points below take it.
struct RsRequest {
    const lanczos_resize_desc* d = nullptr;        // validated (resize_validate)
    const lanczos_resize_opts* o = nullptr;        // NULL: the full box, no gap
    const lanczos_resize_window* win = nullptr;    // the window of the output that is computed and stored (NULL: all of it)
    const void* in = nullptr;
    void* out = nullptr;
    int frames = 0;
    size_t in_frame_stride = 0, out_frame_stride = 0;   // bytes; 0: the frames lie back to back
    hipStream_t stream = nullptr;
    int *last_kernel = nullptr, *last_hip = nullptr;     // as in lanczos_ctx
    int launches = 0;      // out: the launches (kernels and copies) resize_device issued for the request
    bool copied = false;   // out: no resize kernel ran, the request was the plain copy (of a window: its crop)
    // the optional parts, each read only where its flag is set and its `route` written once the launches are out
    bool tensor = false;   // tc: `out` holds element frames.  Crops: win is (0, 0, w, h) and tc.d_origin the origins
    bool source = false;   // sc: the frames at `in` lie in that layout
    bool dest = false;     // dc: the window is stored in that layout instead of tightly packed (bytes out only: never with tc)
    RsTensorCall tc;
    RsSourceCall sc;
    RsDestCall dc;
};

// What rs_route is asked: a request resolved, nothing of it on a device
struct RsRouteQuery {
    const lanczos_resize_desc* d = nullptr;   // the caller's descriptor
    const RsResolved* r = nullptr;
    RsWindow win;                             // the frame that is stored; of a crops request (0, 0, w, h)
    int frames = 1;
    int force = LANCZOS_RESIZE_AUTO;
    bool tensor = false, mapped = false, crops = false;
    int elem = 0;                             // bytes of a tensor element
    size_t extent_bytes = 0;                  // of one element frame
    const RsSource* src = nullptr;            // NULL: the call has no source
    const RsDest* dst = nullptr;              // NULL: the call has no destination
    const ResizeAxisHost *H = nullptr, *V = nullptr;   // the tables of r->inner's axes; read where both passes run
    bool norm = false;                        // a lanczos_tensor_norm request: wide samples, elements computed (tensor is set too)
};
enum RsMain { kRsMainFused, kRsMainNearest, kRsMainCopy, kRsMainCrop, kRsMainNone, kRsMainPassH, kRsMainPassV, kRsMainTwoPass,
              kRsMainVFirst };
enum RsFollower { kRsFollowNone, kRsFollowToTensor, kRsFollowCropsScratch, kRsFollowCropsDirect, kRsFollowToTensorNorm };
// Everything a call does, in the order it does it: pack, reduce, main, follower, unpack.  A scratch block of ResizeState that
// the call uses has its frame stride and size here; 0 bytes: not used
struct RsRoute {
    int err = LANCZOS_OK;   // the refusal; nothing else is set then
    bool reduce = false;    // k_reduce in front: r->fx x r->fy over r->rb into `reduced`, which the resize then reads
    bool pack = false;      // k_rs_pack_source in front of everything: the source gathered into `packed`
    RsMain main = kRsMainNone;
    int bps = 1, flags = 0;        // kRsMainFused: the instance rs_launch_fused<bps, flags>
    bool src_direct = false;       // ... reads the source as it lies
    bool dst_direct = false;       // ... stores the destination's layout itself
    RsWindow win;                  // the window the main step computes: the request's, or the whole output in front of a crops gather
    RsFusedPlan fp;                // kRsMainFused: its plan
    int mid_row0 = 0, mid_rows = 0;   // both passes run: the rows of the source the vertical taps of the window read
    RsFollower follower = kRsFollowNone;
    int tensor_route = 0, source_route = 0, dest_route = 0, kernel = 0;   // LANCZOS_TENSOR_* / SOURCE_* / DEST_* / KERNEL_*; 0: no such part
    struct Block {
        size_t fs = 0, bytes = 0;
    } packed, reduced, tensor_bytes, unpacked, scratch;
    bool follow_src = false;   // kRsFollowToTensorNorm behind kRsMainNone: the follower reads the source frames themselves
};
// The one decision.  Pure host code: no HIP call, no device state, no ResizeState
RsRoute rs_route(const RsRouteQuery& q);

// The entry points (ctx->mu held, device set).  resize_device resolves the request, asks rs_route and issues what it says.
int resize_device(ResizeState* st, RsRequest& q);
// host buffers, and for a tensor request a host table (tc.t.d_lut), host flips (tc.t.d_flip, or NULL) and host origins
// (tc.d_origin, or NULL); frames back to back (a source's or destination's extent, an element frame's tensor_extent_bytes
// apart); synchronous.  Element frames and a destination's go up before they come back, so that what the layout does not
// name keeps what it held.  q.in / q.out are left naming the staging blocks
int resize_host(ResizeState* st, RsRequest& q);

// Reduce by whole factors (lanczos_reduce.hip): Pillow's Image.reduce over an integer box, 8-bit.  Arguments validated by
// reduce_validate; the output rows are tightly packed.
int reduce_validate(int in_w, int in_h, int channels, int fx, int fy, const int32_t* box, int rb[4]);
hipError_t reduce_launch(const uint8_t* in, uint8_t* out, int in_w, int channels, int fx, int fy, const int rb[4], int frames,
                         size_t in_fs, size_t out_fs, RsIssue& is);
int reduce_device(ResizeState* st, int in_w, int in_h, int channels, int fx, int fy, const int32_t* box, const void* d_in,
                  void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride, hipStream_t stream, int* last_hip);
int reduce_host(ResizeState* st, int in_w, int in_h, int channels, int fx, int fy, const int32_t* box, const void* in,
                void* out, int frames, hipStream_t stream, int* last_hip);

// One request for the fused kernel, k_rs_fused<RsSample<BPS>, C, K, ALPHA, FLAGS> (lanczos_resize_fused.hpp): the instance
// is that of d's channels and alpha flag and of the plan's K.  Frame strides in bytes.  The kernel gets the tables from the
// window's first outputs on and the window's extent as its output size; the plan is that of the window.
struct RsFusedLaunch {
    const lanczos_resize_desc* d;
    RsWindow win;
    const RsFusedPlan* fp;
    const ResizeAxis *H, *V;
    const uint8_t* in;
    uint8_t* out;
    size_t in_fs, out_fs;
    int frames;
    const RsTensorCall* tc;   // a tensor request: `out` / `out_fs` are the element frames
    RsIssue& is;             // the stream, and the count the launches add to
    const RsSource* src = nullptr;   // NULL: packed interleaved rows.  A planar one runs the kRsPlanar instances
    const RsDest* dst = nullptr;     // NULL: packed output rows; else rows row_stride bytes apart.  A planar one runs the
                                     // kRsPlanarOut instances
};
// FLAGS of an instance.  Its low bits (kRsElemMask): bytes of a stored table element, 2 or 4; 0 where the samples themselves
// are stored.  + kRsMapped: through the channel map and the flips of the request (RsTensorOut::mapped)
constexpr int kRsElemMask = 7;
constexpr int kRsMapped = 8;
// + kRsCrops: a window origin per frame, read when the kernel runs (RsTensorCall::d_origin); the tables are the full axes'
constexpr int kRsCrops = 16;
// + kRsPlanar: the source is planar (RsSource::planar), staged through a byte transpose; with bytes out FLAGS is kRsPlanar alone
constexpr int kRsPlanar = 32;
// + kRsRowShift: LANCZOS_RESIZE_ALPHA over pitched interleaved rows whose pitch is no dword multiple: the staging shifts by the
// residue of each row.  As for kRsPlanar, bytes out is the flag alone and a tensor request runs the mapped instance
constexpr int kRsRowShift = 64;
// + kRsPlanarOut: the destination is planar (RsDest::planar, bytes out): the vertical pass stores one dword per plane
constexpr int kRsPlanarOut = 128;
// kRsNorm alone: wide samples (BPS 2 or 4) into computed elements, lanczos_tensor_norm; the element format is an argument
constexpr int kRsNorm = 256;
// The instances of rs_launch_fused<BPS, FLAGS> (each with its k_rs_fused kernels for every channel count, tap bucket and ALPHA),
// X(index, BPS, FLAGS).  This is the one list: the declarations, the cases of rs_launch_fused_any and rs_fused_instance_exists
// come from it, and lanczos_resize_fused_inst.hip is compiled once per index (-DLZ_RS_INST=<index>, the Makefile's RS_INSTS) into
// the instance of that entry and nothing else.  A new instance is a line here and one more index there.
//    0      8-bit, bytes out                          1, 2    8-bit into float / 16-bit elements through a table
//    3, 4   ... through a channel map and flips       5, 6    ... with a crop origin per frame
//    7..9   8-bit from a planar source: bytes, floats, 16-bit elements
//   10..12  ALPHA over rows pitched off a dword: the same three
//   13, 14  8-bit into a planar destination, from an interleaved and from a planar source
//   15, 16  16-bit and float samples                 17, 18   ... into computed elements (lanczos_tensor_norm)
#define LZ_RS_FUSED_INSTANCES(X)                                                             \
    X(0, 1, 0) X(1, 1, 4) X(2, 1, 2) X(3, 1, 4 + kRsMapped) X(4, 1, 2 + kRsMapped)           \
    X(5, 1, 4 + kRsMapped + kRsCrops) X(6, 1, 2 + kRsMapped + kRsCrops)                      \
    X(7, 1, kRsPlanar) X(8, 1, 4 + kRsMapped + kRsPlanar) X(9, 1, 2 + kRsMapped + kRsPlanar) \
    X(10, 1, kRsRowShift) X(11, 1, 4 + kRsMapped + kRsRowShift) X(12, 1, 2 + kRsMapped + kRsRowShift) \
    X(13, 1, kRsPlanarOut) X(14, 1, kRsPlanar + kRsPlanarOut)                                \
    X(15, 2, 0) X(16, 4, 0) X(17, 2, kRsNorm) X(18, 4, kRsNorm)
#define X(I, BPS, FLAGS) +1
constexpr int kRsFusedInstances = 0 LZ_RS_FUSED_INSTANCES(X);
#undef X
// whether rs_launch_fused<bps, flags> is one of them: what a route's (bps, flags) has to satisfy
constexpr bool rs_fused_instance_exists(int bps, int flags) {
#define X(I, BPS, FLAGS) || (bps == (BPS) && flags == (FLAGS))
    return false LZ_RS_FUSED_INSTANCES(X);
#undef X
}
template <int BPS, int FLAGS>
hipError_t rs_launch_fused(const RsFusedLaunch& c);

// LANCZOS_FILTER_NEAREST (lanczos_resize_nearest.hip): out[y][x] = in[vidx[y]][hidx[x]] for pixels of `channels` samples of
// `bps` bytes (1 or 4), one launch.  hidx / vidx are device tables of out_w / out_h source indices, all inside the source.
hipError_t rs_nearest_launch(const uint8_t* in, uint8_t* out, int in_w, int out_w, int out_h, int channels, int bps,
                             const int32_t* hidx, const int32_t* vidx, int frames, size_t in_fs, size_t out_fs,
                             RsIssue& is);
// The crop of a resize that changes neither axis (k_rs_crop, beside the gather): `rows` rows of `row_bytes` bytes from `in`
// (the window's first byte; rows in_pitch bytes apart) to tightly packed rows at `out`, every frame in one launch.
hipError_t rs_crop_launch(const uint8_t* in, uint8_t* out, size_t in_pitch, size_t row_bytes, int rows, int frames,
                          size_t in_fs, size_t out_fs, RsIssue& is);

// ---- YCbCr frames: lanczos_resize_ycc_* (8-bit frames into RGB bytes and tensor elements), lanczos_resize_ycc_out
// (into 8-bit YCbCr frames, from YCbCr or from RGB) and lanczos_resize_ycc16 (frames of 16-bit words into any of these) are one
// request and one composition.  Nothing of it resizes: every plane is a one-channel request of B-byte samples through
// resize_device with a pitched source and a pitched destination, a split in front of interleaved chroma, a join behind
// interleaved chroma out, and behind the planes the merge into RGB or elements (lanczos_resize_ycc.hip; the merge of words in
// lanczos_resize_ycc16.hip).  From RGB bytes it is the three-channel request into context scratch and k_rs_ycc_encode behind it
// (lanczos_resize_ycc_out.hip).  What needs no device -- the layouts, the descriptor check, the standard tables and matrices --
// is in lanczos_resize_ycc_layout.cpp and lanczos_resize_route.cpp.
// A lanczos_ycc_source or lanczos_ycc_dest resolved by ycc_layout_resolve for a w x h luma frame of B-byte samples; everything in
// bytes:
struct YccLayout {
    int layout = 0, sx = 0, sy = 0;
    int cw = 0, ch = 0;                     // the chroma planes' size
    size_t y_rs = 0, c_rs = 0;              // row strides; c_rs of NV12 / NV21 is the interleaved rows'
    size_t cb_off = 0, cr_off = 0;          // NV12 / NV21: both the interleaved plane's
    size_t extent = 0;                      // of one frame, the default frame stride: the end of its last plane
    size_t named = 0;                       // from a frame's first byte to the last one the layout names, + 1
    bool interleaved() const { return layout != LANCZOS_YCC_PLANAR; }
};
// d validated for these entries: three channels, samples of B bytes (1 or 2), no alpha (lanczos_resize_route.cpp)
int ycc_desc_validate(const lanczos_resize_desc* d, int B);
// L: lanczos_ycc_source or lanczos_ycc_dest.  aligned_origin: refuse a window origin (x0, y0) that is no multiple of the
// subsampling (the rule of a destination filled from YCbCr frames).  Every refusal is LANCZOS_ERR_BAD_ARG
template <class L>
int ycc_layout_resolve(const L* l, int w, int h, int B, bool aligned_origin, int x0, int y0, YccLayout* s);
// the tight layout -- Y, then Cb, then Cr (or the interleaved plane), rows packed -- and its resolution: what the *_init entries do
template <class L>
int ycc_layout_init(L* l, int w, int h, int B, int layout, int sub_x, int sub_y);
bool ycc_table(int standard, int32_t* t);
bool ycc_table_forward(int standard, int32_t* t);
int ycc16_matrix_validate(const lanczos_ycc16_matrix* m);
bool ycc16_matrix_init(lanczos_ycc16_matrix* m, int standard, int depth, bool msb_aligned, bool full_range);
// clip8(sum >> 6) with the clamp in front of the shift: the sum held to [0, 255 * 64 + 63] and then shifted is the same byte.
// (Shift first and clamp after compiles, two pixels at a time, into v_ashr_pk_u8_i32, and on an MI355X the dword that
// instruction leaves did not have a clean upper half: OR-ed with pixels 2 and 3 it turned them into 255.)
__device__ __forceinline__ uint32_t ycc_clip8_shift6(int sum) { return (uint32_t)(sum < 0 ? 0 : sum > 16383 ? 16383 : sum) >> 6; }
// What a call stores, and what it launched: the superset of lanczos_ycc_info, lanczos_ycc_out_info and lanczos_ycc16_info
enum YccOut { kYccOutRgb, kYccOutElems, kYccOutYcc, kYccOutYccFromRgb };
struct YccInfo {
    int luma_kernel = 0, chroma_kernel = 0, split = 0, join = 0, merge = 0, encode = 0, launches = 0;
};
// One call of any of the three families, filled in by lanczos_api.hip
struct YccRequest {
    const lanczos_resize_desc* d = nullptr;       // validated (ycc_desc_validate with B)
    const lanczos_resize_opts* o = nullptr;
    const lanczos_resize_window* win = nullptr;
    int B = 1;                                    // bytes of a sample
    YccOut kind = kYccOutRgb;
    YccLayout s;                                  // resolved, where the frames are YCbCr (every kind but kYccOutYccFromRgb)
    const lanczos_ycc_dest* dst = nullptr;        // the YCbCr kinds: resolved by the entry points, which know the window
    const int32_t* table = nullptr;               // 8-bit RGB, elements and from RGB: [3][3][256], inverse or forward
    lanczos_ycc16_matrix m{};                     // 16-bit RGB and elements: validated
    RsTensorOut t;                                // kYccOutElems: validated (tensor_view_validate, of words tensor_norm_validate)
    const void* in = nullptr;
    void* out = nullptr;
    int frames = 0;
    size_t in_frame_stride = 0, out_frame_stride = 0;
    hipStream_t stream = nullptr;
    int* last_hip = nullptr;
    YccInfo info;                                 // out, on LANCZOS_OK
    bool tensor() const { return kind == kYccOutElems; }
    bool to_ycc() const { return kind == kYccOutYcc || kind == kYccOutYccFromRgb; }
};
// ctx->mu held, device set: device pointers, asynchronous
int resize_ycc_device(ResizeState* st, YccRequest& q);
// host buffers, a host table, and of an element request a host element table and host flips; frames back to back (a layout's
// extent, w * h * 3 samples, an element frame's extent apart: the frame strides must be 0); synchronous.  A destination's and a
// tensor's frames go up before they come back, so that what the layout does not name keeps what it held
int resize_ycc_host(ResizeState* st, YccRequest& q);
// the launchers the composition calls across units: the merges behind the three planes (`planes`: frames luma planes, then
// frames pairs Cb | Cr, every plane plane_bytes long) and the encode behind the RGB resize
hipError_t ycc_merge_launch(const uint8_t* planes, size_t plane_bytes, uint8_t* out, size_t out_fs, int w, int h,
                            const int32_t* table, const RsTensorOut* t, int frames, RsIssue& is);
hipError_t ycc16_merge_launch(const uint8_t* planes, size_t plane_bytes, uint8_t* out, size_t out_fs, int w, int h,
                              const lanczos_ycc16_matrix& m, const RsTensorOut* t, int frames, RsIssue& is);
hipError_t ycc_encode_launch(const uint8_t* in, size_t in_fs, uint8_t* out, size_t out_fs, const YccLayout& t, int w, int h,
                             const int32_t* table, int frames, RsIssue& is);

}  // namespace lz
