// Asks rs_route (csrc/lanczos_resize_route.cpp, compiled beside this file: no library, no kernel, no device) what requests of
// lanczos_tensor_norm launch, and holds the answers against the rule of include/lanczos_hip.h: LANCZOS_TENSOR_FUSED exactly when
// the sample request's route is the fused kernel and one element frame spans less than 2^31 bytes (and nothing is forced away
// from it), LANCZOS_TENSOR_CONVERTED with k_rs_to_tensor_norm behind the sample request's own main step otherwise.  Requests go
// through the resolvers and validators the library's entries call.  Prints one line per request and "ok <n>" at the end;
// any broken expectation prints BAD and the exit status is 1.
#include <cstdio>
#include <cstring>

#include "lanczos_resize.hpp"
using namespace lz;

static int g_bad = 0;
#define EXPECT(cond, ...)          \
    do {                           \
        if (!(cond)) {             \
            printf("BAD %s: ", #cond); \
            printf(__VA_ARGS__);   \
            printf("\n");          \
            g_bad++;               \
        }                          \
    } while (0)

struct Case {
    const char* name;
    int in_w, in_h, out_w, out_h, channels, flags, filter;   // flags: LANCZOS_RESIZE_U16 / _F32
    int format;
    long long cs, rs, ps;   // 0, 0, 0: tight CHW
    int force, frames;
    bool windowed;          // a window (1, 1, out_w - 2, out_h - 2)
    int want_route;         // LANCZOS_TENSOR_*, or a negative LANCZOS_ERR_*
    int want_main;          // RsMain of the expected route
};

int main() {
    const int U = LANCZOS_RESIZE_U16, F = LANCZOS_RESIZE_F32, L3 = LANCZOS_FILTER_LANCZOS, NN = LANCZOS_FILTER_NEAREST;
    const int f32 = LANCZOS_TENSOR_F32, bf = LANCZOS_TENSOR_BF16, h16 = LANCZOS_TENSOR_F16;
    const int AUTO = LANCZOS_RESIZE_AUTO, FUSED = LANCZOS_RESIZE_FUSED, TWO = LANCZOS_RESIZE_TWO_PASS, CONV = LANCZOS_RESIZE_CONVERT;
    const long long R23 = (1ll << 23) - 1;
    const Case cases[] = {
        {"fused u16 c3", 400, 140, 200, 70, 3, U, L3, f32, 0, 0, 0, AUTO, 2, false, LANCZOS_TENSOR_FUSED, kRsMainFused},
        {"fused f32 c1 bf16", 400, 140, 200, 70, 1, F, L3, bf, 0, 0, 0, AUTO, 2, false, LANCZOS_TENSOR_FUSED, kRsMainFused},
        {"fused f32 c4 f16 window", 400, 140, 200, 70, 4, F, L3, h16, 0, 0, 0, AUTO, 2, true, LANCZOS_TENSOR_FUSED, kRsMainFused},
        {"fused forced", 400, 140, 200, 70, 3, U, L3, f32, 0, 0, 0, FUSED, 2, false, LANCZOS_TENSOR_FUSED, kRsMainFused},
        {"forced two pass", 400, 140, 200, 70, 3, U, L3, f32, 0, 0, 0, TWO, 2, false, LANCZOS_TENSOR_CONVERTED, kRsMainTwoPass},
        {"forced convert", 400, 140, 200, 70, 3, U, L3, f32, 0, 0, 0, CONV, 2, false, LANCZOS_TENSOR_CONVERTED, kRsMainFused},
        {"horizontal only", 400, 70, 200, 70, 3, U, L3, f32, 0, 0, 0, AUTO, 2, false, LANCZOS_TENSOR_CONVERTED, kRsMainPassH},
        {"vertical only", 200, 140, 200, 70, 1, F, L3, bf, 0, 0, 0, AUTO, 2, false, LANCZOS_TENSOR_CONVERTED, kRsMainPassV},
        {"at size", 200, 70, 200, 70, 3, U, L3, h16, 0, 0, 0, AUTO, 2, false, LANCZOS_TENSOR_CONVERTED, kRsMainNone},
        {"at size window", 200, 70, 200, 70, 3, U, L3, f32, 0, 0, 0, AUTO, 2, true, LANCZOS_TENSOR_CONVERTED, kRsMainCrop},
        {"tall vertical first", 4, 900, 3, 300, 1, U, L3, f32, 0, 0, 0, AUTO, 1, false, LANCZOS_TENSOR_CONVERTED, kRsMainVFirst},
        {"nearest f32", 400, 140, 200, 70, 3, F, NN, f32, 0, 0, 0, AUTO, 2, false, LANCZOS_TENSOR_CONVERTED, kRsMainNearest},
        {"forced fused, one pass", 400, 70, 200, 70, 3, U, L3, f32, 0, 0, 0, FUSED, 2, false, -LANCZOS_ERR_UNSUPPORTED, 0},
        {"forced fused, wide taps", 4000, 1400, 100, 35, 3, U, L3, f32, 0, 0, 0, FUSED, 1, false, -LANCZOS_ERR_UNSUPPORTED, 0},
        {"wide taps", 4000, 1400, 100, 35, 3, U, L3, f32, 0, 0, 0, AUTO, 1, false, LANCZOS_TENSOR_CONVERTED, kRsMainTwoPass},
        // an element frame of 2^31 bytes: 64 * (2^23 - 1) + 63 + 1 = 2^29 float32 elements; one column less is 4 bytes below
        {"2^31 bytes", 128, 130, 64, 65, 1, U, L3, f32, 1, R23, 1, AUTO, 1, false, LANCZOS_TENSOR_CONVERTED, kRsMainFused},
        {"2^31 - 4 bytes", 126, 130, 63, 65, 1, U, L3, f32, 1, R23, 1, AUTO, 1, false, LANCZOS_TENSOR_FUSED, kRsMainFused},
        {"2^31 bytes, forced fused", 128, 130, 64, 65, 1, U, L3, f32, 1, R23, 1, FUSED, 1, false, -LANCZOS_ERR_UNSUPPORTED, 0},
        // ... and of 2^30 16-bit elements: 64 * (2^24 - 1) + 64 = 2^30
        {"2^31 bytes bf16", 128, 130, 64, 65, 1, F, L3, bf, 1, (1ll << 24) - 1, 1, AUTO, 1, false, LANCZOS_TENSOR_CONVERTED, kRsMainFused},
        {"2^31 - 2 bytes f16", 126, 130, 63, 65, 1, F, L3, h16, 1, (1ll << 24) - 1, 1, AUTO, 1, false, LANCZOS_TENSOR_FUSED, kRsMainFused},
    };
    int n = 0;
    for (const Case& c : cases) {
        lanczos_resize_desc d{};
        d.in_w = c.in_w, d.in_h = c.in_h, d.out_w = c.out_w, d.out_h = c.out_h, d.channels = c.channels, d.a = 3;
        d.reserved[0] = c.flags | LANCZOS_RESIZE_FILTER(c.filter);
        lanczos_resize_window win{1, 1, c.out_w - 2, c.out_h - 2, {0, 0, 0, 0}};
        const lanczos_resize_window* wp = c.windowed ? &win : nullptr;
        RsResolved r;
        RsRouteQuery q;
        int rc = resize_validate(&d);
        if (rc == LANCZOS_OK) rc = resize_resolve(&d, nullptr, &r);
        if (rc == LANCZOS_OK) rc = resize_window_resolve(&d, wp, &q.win);
        lanczos_tensor_norm tn{};
        for (int k = 0; k < 4; k++) tn.div[k] = 65535.0f, tn.mean[k] = 0.5f, tn.std[k] = 0.25f;
        tn.format = c.format, tn.out_channels = c.channels;
        for (int k = 0; k < c.channels; k++) tn.src_channel[k] = k;
        tn.chan_stride = c.cs ? c.cs : (long long)q.win.w * q.win.h, tn.row_stride = c.rs ? c.rs : q.win.w, tn.pix_stride = c.ps ? c.ps : 1;
        RsTensorOut lay;
        if (rc == LANCZOS_OK) rc = tensor_norm_validate(&d, wp, &tn, &lay);
        EXPECT(rc == LANCZOS_OK, "%s: refused with %d before the route", c.name, rc);
        if (rc != LANCZOS_OK) continue;
        EXPECT(lay.norm && lay.mapped == false && lay.elem == (c.format == f32 ? 4 : 2), "%s: the resolved layout", c.name);
        const bool f64 = true;
        ResizeAxisHost H, V;
        const bool both = resize_filter(&d) == NN && (r.need_h || r.need_v);
        if ((r.need_h || both) && !resize_build_axis(d.in_w, d.out_w, d.a, resize_filter(&d), r.h, &H, f64)) rc = LANCZOS_ERR_UNSUPPORTED;
        if ((r.need_v || both) && !resize_build_axis(d.in_h, d.out_h, d.a, resize_filter(&d), r.v, &V, f64)) rc = LANCZOS_ERR_UNSUPPORTED;
        EXPECT(rc == LANCZOS_OK, "%s: no tables", c.name);
        q.d = &d, q.r = &r, q.frames = c.frames, q.H = &H, q.V = &V;
        // the sample request first, under AUTO: what `fused` means in the rule
        const RsRoute plain = rs_route(q);
        const bool plan_fused = plain.err == LANCZOS_OK && plain.main == kRsMainFused;
        EXPECT(plain.flags == 0 && plain.tensor_route == 0 && plain.follower == kRsFollowNone, "%s: the sample request", c.name);
        q.force = c.force;
        q.tensor = q.norm = true, q.mapped = lay.mapped, q.elem = lay.elem;
        q.extent_bytes = tensor_extent_bytes(&d, q.win, lay);
        const RsRoute rt = rs_route(q);
        const int B = resize_bps(&d);
        const bool fits = q.extent_bytes < ((size_t)1 << 31);
        printf("NORM %-26s err %d route %d main %d bps %d flags %d follower %d from_src %d scratch %zu extent %zu\n", c.name, rt.err,
               rt.tensor_route, (int)rt.main, rt.bps, rt.flags, (int)rt.follower, (int)rt.follow_src, rt.tensor_bytes.fs, q.extent_bytes);
        n++;
        if (c.want_route < 0) {
            EXPECT(rt.err == -c.want_route, "%s: err %d", c.name, rt.err);
            EXPECT(!(plan_fused && fits), "%s: a refusal of a fusable request", c.name);
            continue;
        }
        EXPECT(rt.err == LANCZOS_OK, "%s: err %d", c.name, rt.err);
        EXPECT(rt.tensor_route == c.want_route && (int)rt.main == c.want_main, "%s: route %d main %d", c.name, rt.tensor_route, (int)rt.main);
        // the rule itself
        const bool want_fused = plan_fused && fits && c.force != TWO && c.force != CONV;
        EXPECT((rt.tensor_route == LANCZOS_TENSOR_FUSED) == want_fused, "%s: the rule says %d", c.name, (int)want_fused);
        if (rt.tensor_route == LANCZOS_TENSOR_FUSED) {
            EXPECT(rt.main == kRsMainFused && rt.flags == kRsNorm && rt.bps == B && rt.follower == kRsFollowNone && !rt.follow_src &&
                       rt.tensor_bytes.bytes == 0,
                   "%s: the fused route's parts", c.name);
            EXPECT(memcmp(&rt.fp, &plain.fp, sizeof(rt.fp)) == 0, "%s: another plan than the sample request's", c.name);
        } else {
            const size_t packed = (((size_t)q.win.w * q.win.h * c.channels * B) + 3) & ~(size_t)3;
            // (bps names the fused instance and is set where that runs: it then stores plain samples, to scratch)
            EXPECT(rt.follower == kRsFollowToTensorNorm && (rt.main != kRsMainFused || (rt.flags == 0 && rt.bps == B)), "%s: the converted route's parts", c.name);
            EXPECT(rt.follow_src == (rt.main == kRsMainNone), "%s: from the source exactly where nothing runs in front", c.name);
            EXPECT(rt.tensor_bytes.fs == (rt.follow_src ? 0 : packed) && rt.tensor_bytes.bytes == rt.tensor_bytes.fs * c.frames,
                   "%s: scratch %zu", c.name, rt.tensor_bytes.fs);
            // the main step is the sample request's own under the same force
            RsRouteQuery p = q;
            p.tensor = p.norm = false, p.elem = 0, p.extent_bytes = 0, p.force = c.force == CONV ? AUTO : c.force;
            const RsRoute same = rs_route(p);
            EXPECT(rt.main == kRsMainNone || (same.err == LANCZOS_OK && same.main == rt.main && same.scratch.fs == rt.scratch.fs),
                   "%s: another main step than the sample request's", c.name);
        }
        EXPECT(rt.kernel == (rt.main == kRsMainFused ? LANCZOS_KERNEL_RESIZE_FUSED : rt.main == kRsMainNearest ? LANCZOS_KERNEL_RESIZE_NEAREST
                                                                                                                  : LANCZOS_KERNEL_RESIZE_TWO_PASS),
               "%s: kernel %d", c.name, rt.kernel);
    }
    // an 8-bit query with the new field at its default is what it was: the existing matrix holds that against predict(); here
    // only that the default is off
    EXPECT(RsRouteQuery().norm == false && RsRoute().follow_src == false, "defaults");
    if (g_bad) return 1;
    printf("ok %d\n", n);
    return 0;
}
