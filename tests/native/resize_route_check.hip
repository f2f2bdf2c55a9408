// Asks rs_route (csrc/lanczos_resize_route.cpp, compiled beside this file: no library, no kernel, no device) what each request
// of a file launches, and prints it for tests/test_resize_matrix_cfg.py to hold against resize_matrix_cfg.predict.  The request
// goes through the resolvers the library's entries call: resize_resolve, resize_window_resolve, resize_source_resolve,
// resize_dest_resolve, tensor_extent_bytes, and the host tables of the axes that run.
// Input (argv[1]), one request per line:
//   in_w in_h out_w out_h channels a reserved0                 the descriptor (sample width, alpha and filter in reserved0)
//   has_opts box0 box1 box2 box3 gap                           lanczos_resize_opts
//   has_win x0 y0 w h  crops                                   the window; crops = 1: (w, h) is the crop size, x0 = y0 = 0
//   elem mapped chan_stride row_stride pix_stride out_channels the tensor part (elem 0: bytes out); mapped bit 1: the request is a
//                                                              lanczos_tensor_norm one (wide samples, no map)
//   has_src row_stride chan_stride pix_stride                  lanczos_resize_source
//   has_dst row_stride chan_stride pix_stride                  lanczos_resize_dest
//   force frames
// Output per line: ROUTE <line> <err> <reduce> <pack> <main> <bps> <flags> <follower> <tensor> <source> <dest> <kernel>
// and behind them the list this program was compiled with, INSTANCE <index> <bps> <flags> per entry of LZ_RS_FUSED_INSTANCES.  A
// fused route that names no entry (rs_fused_instance_exists) prints BAD and the exit status is 1.
#include <cstdio>

#include "lanczos_resize.hpp"
using namespace lz;

static const char* const kMain[] = {"fused", "nearest", "copy", "crop", "none", "pass_h_only", "pass_v_only", "two_pass", "v_first"};
static const char* const kFollower[] = {"none", "to_tensor", "crops_scratch", "crops_direct", "to_tensor_norm"};
static_assert(rs_fused_instance_exists(1, 0) && !rs_fused_instance_exists(2, 4), "the predicate is the list's, at compile time");

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) {
        printf("usage: %s requests.txt\n", argv[0]);
        return 2;
    }
    int line = 0, has_opts, has_win, crops, elem, mapped, oc, has_src, has_dst, force, frames, res0;
    lanczos_resize_desc d{};
    lanczos_resize_opts o{};
    lanczos_resize_window win{};
    lanczos_resize_source src{};
    lanczos_resize_dest dst{};
    long long tcs, trs, tps, s[3], t[3];
    while (fscanf(f, "%d %d %d %d %d %d %d %d %lf %lf %lf %lf %lf %d %d %d %d %d %d %d %d %lld %lld %lld %d %d %lld %lld %lld %d %lld %lld %lld %d %d",
                  &d.in_w, &d.in_h, &d.out_w, &d.out_h, &d.channels, &d.a, &res0, &has_opts, &o.box[0], &o.box[1], &o.box[2], &o.box[3],
                  &o.reducing_gap, &has_win, &win.x0, &win.y0, &win.w, &win.h, &crops, &elem, &mapped, &tcs, &trs, &tps, &oc, &has_src,
                  &s[0], &s[1], &s[2], &has_dst, &t[0], &t[1], &t[2], &force, &frames) == 35) {
        d.reserved[0] = res0;
        src.row_stride = s[0], src.chan_stride = s[1], src.pix_stride = (int32_t)s[2];
        dst.row_stride = t[0], dst.chan_stride = t[1], dst.pix_stride = (int32_t)t[2];
        RsResolved r;
        RsRouteQuery q;
        RsSource rs;
        RsDest rd;
        int rc = resize_validate(&d);
        if (rc == LANCZOS_OK) rc = resize_resolve(&d, has_opts ? &o : nullptr, &r);
        if (rc == LANCZOS_OK) rc = resize_window_resolve(&d, has_win ? &win : nullptr, &q.win);
        if (rc == LANCZOS_OK) rc = resize_source_resolve(&d, has_src ? &src : nullptr, &rs);
        if (rc == LANCZOS_OK) rc = resize_dest_resolve(&d, q.win, has_dst ? &dst : nullptr, &rd);
        if (rc != LANCZOS_OK) {
            printf("BAD line %d: a resolver refuses it with %d\n", line, rc);
            return 1;
        }
        const bool f64 = resize_bps(&d) > 1;
        ResizeAxisHost H, V;
        if (r.need_h && !resize_build_axis(r.inner.in_w, r.inner.out_w, d.a, resize_filter(&d), r.h, &H, f64)) rc = LANCZOS_ERR_UNSUPPORTED;
        if (r.need_v && !resize_build_axis(r.inner.in_h, r.inner.out_h, d.a, resize_filter(&d), r.v, &V, f64)) rc = LANCZOS_ERR_UNSUPPORTED;
        if (rc != LANCZOS_OK) {
            printf("BAD line %d: no tables\n", line);
            return 1;
        }
        q.d = &d, q.r = &r, q.frames = frames, q.force = force, q.H = &H, q.V = &V;
        if (elem) {
            RsTensorOut lay{nullptr, tcs, trs, tps, elem, oc};
            q.tensor = true, q.mapped = (mapped & 1) != 0, q.norm = (mapped & 2) != 0, q.crops = crops != 0, q.elem = elem;
            q.extent_bytes = tensor_extent_bytes(&d, q.win, lay);
        }
        q.src = has_src ? &rs : nullptr, q.dst = has_dst ? &rd : nullptr;
        const RsRoute rt = rs_route(q);
        printf("ROUTE %d %d %d %d %s %d %d %s %d %d %d %d\n", line, rt.err, (int)rt.reduce, (int)rt.pack, kMain[rt.main], rt.bps, rt.flags,
               kFollower[rt.follower], rt.tensor_route, rt.source_route, rt.dest_route, rt.kernel);
        if (rt.err == LANCZOS_OK && rt.main == kRsMainFused && !rs_fused_instance_exists(rt.bps, rt.flags)) {
            printf("BAD line %d: no fused instance <%d, %d>\n", line, rt.bps, rt.flags);
            return 1;
        }
        line++;
    }
    fclose(f);
    printf("done %d\n", line);
#define X(I, BPS, FLAGS) printf("INSTANCE %d %d %d\n", I, BPS, FLAGS);
    LZ_RS_FUSED_INSTANCES(X)
#undef X
    return 0;
}
