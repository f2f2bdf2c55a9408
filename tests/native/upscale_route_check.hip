// Asks up_route (csrc/lanczos_upscale_route.cpp, compiled beside this file with lanczos_taps.cpp: no library, no kernel, no device)
// what each request of a file does, and prints it for tests/test_upscale_route_cfg.py to hold against upscale_route_cfg.predict.
// The plan's facts are made as get_plan makes them (build_axis / build_axis_hls, prefix_info); what the kernel headers decide
// (fast_prepare, rat_prepare, ratp_prepare succeeded) and the marching instance's facts come with the request.
// Input (argv[1]), one request per line:
//   in_w in_h channels bytes_per_sample scale_n scale_d a mode out_row0 out_rows     the descriptor
//   frames in_frame_stride out_frame_stride in_base out_base force                  the call (strides as given: 0 = back to back)
//   fast_ok rat_ok ratp_ok  tile_kernel separate_prefix no_ratp                     the plan's facts, the environment switches
//   has_facts nt lds_bytes strip_out_px wg_per_cu cus                               MarchFacts (has_facts 0: no marching instance)
//   K M M2                                                                          the prefix handed to up_route instead of the plan's (K < 0: the plan's)
// Output per line: ROUTE <line> <err> <kernel> <main> <launches> then <count>x<frames>:<prefix> for the full launches of a split
// batch and for the last launch; after a refusal only <err>.
#include <cstdio>

#include "lanczos_upscale.hpp"
using namespace lz;

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) {
        printf("usage: %s requests.txt\n", argv[0]);
        return 2;
    }
    int line = 0, in_w, in_h, c, bps, sn, sd, a, mode, row0, rows, frames, force, fast_ok, rat_ok, ratp_ok, tile, sep, noratp, has_facts, pk, pm, pm2;
    long long in_stride, out_stride, in_base, out_base;
    MarchFacts mf{};
    while (fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %lld %lld %lld %lld %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &in_w, &in_h, &c, &bps,
                  &sn, &sd, &a, &mode, &row0, &rows, &frames, &in_stride, &out_stride, &in_base, &out_base, &force, &fast_ok, &rat_ok,
                  &ratp_ok, &tile, &sep, &noratp, &has_facts, &mf.nt, &mf.lds_bytes, &mf.strip_out_px, &mf.wg_per_cu, &mf.cus, &pk, &pm, &pm2) == 31) {
        lanczos_desc d{};
        d.in_w = in_w, d.in_h = in_h, d.channels = c, d.bytes_per_sample = bps, d.scale_n = sn, d.scale_d = sd, d.a = a, d.mode = mode;
        d.out_w = (int)((long long)in_w * sn / sd), d.out_h = (int)((long long)in_h * sn / sd);
        d.out_row0 = row0, d.out_rows = rows;
        if (validate(&d) != LANCZOS_OK || frames < 1) {
            printf("BAD line %d: the descriptor is refused before any route\n", line);
            return 1;
        }
        AxisTaps V;
        UpQuery q;
        if (mode == LANCZOS_MODE_HLS) {
            build_axis_hls(d.in_h, d.out_h, sn, sd, a, &V, d.reserved[0]);
        } else {
            build_axis(d.in_h, d.out_h, sn, sd, a, &V);
            q.prefix = prefix_info(V);
        }
        q.d = &d, q.frames = frames, q.in_frame_stride = (size_t)in_stride, q.out_frame_stride = (size_t)out_stride;
        q.in = (uintptr_t)in_base, q.out = (uintptr_t)out_base, q.force = force;
        q.fast_ok = fast_ok != 0, q.rat_ok = rat_ok != 0, q.ratp_ok = ratp_ok != 0, q.v_first = V.first.data();
        q.tile_kernel = tile != 0, q.separate_prefix = sep != 0, q.no_ratp = noratp != 0;
        q.facts = has_facts ? &mf : nullptr;
        if (pk >= 0) q.prefix.K = pk, q.prefix.M = pm, q.prefix.M2 = pm2;
        const UpRoute r = up_route(q);
        if (r.err != LANCZOS_OK) {
            printf("ROUTE %d %d\n", line, r.err);
        } else {
            printf("ROUTE %d 0 %d %d %d", line, r.kernel, r.main, r.n_launches);
            if (r.n_launches > 1) printf(" %dx%d:%d", r.n_launches - 1, r.body.frames, r.body.prefix);
            printf(" 1x%d:%d\n", r.tail.frames, r.tail.prefix);
        }
        line++;
    }
    fclose(f);
    printf("done %d\n", line);
    return 0;
}
