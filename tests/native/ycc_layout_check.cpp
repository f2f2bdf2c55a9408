// Runs ycc_layout_resolve (csrc/lanczos_resize_ycc_layout.cpp, compiled beside this file and nothing else: no library, no kernel,
// no device) over VALIDATE rows of tests/resize_ycc_layout_cfg.py and prints its return code per row, for
// tests/test_resize_ycc_layout_host.py to hold against the recorded codes.  The rows it is given have a legal descriptor and a
// window inside the output, so the resolver's answer is the entry's.  For every accepted row it also checks what a caller relies
// on: the planes lie inside [0, extent), named <= extent, and ycc_layout_init's tight layout of the same frame resolves and
// names every byte of its extent.
// Input (argv[1]), one row per line: B dest in_w in_h out_w out_h has_win x0 y0 w h y_row_stride c_row_stride cb_offset
// cr_offset layout sub_x sub_y reserved_index.  Output: one code per row, then `done <rows>`; BAD and exit status 1 on a broken
// invariant.  Built with -fsanitize=address,undefined it is the sanitizer run of the resolver.
#include <cstdio>

#include "lanczos_resize.hpp"
using namespace lz;

template <class L>
static int run(const long long* v, int w, int h, int x0, int y0, bool dest, int line) {
    const int B = (int)v[0];
    L l{};
    l.y_row_stride = v[11], l.c_row_stride = v[12], l.cb_offset = v[13], l.cr_offset = v[14];
    l.layout = (int32_t)v[15], l.sub_x = (int32_t)v[16], l.sub_y = (int32_t)v[17];
    if (v[18] >= 0) l.reserved[v[18]] = 1;
    YccLayout s;
    const int rc = ycc_layout_resolve(&l, w, h, B, dest, x0, y0, &s);
    printf("%d\n", rc);
    if (rc != LANCZOS_OK) return 0;
    const size_t c_row = (size_t)(s.interleaved() ? 2 : 1) * B * s.cw;
    const bool inside = (size_t)h * s.y_rs <= s.cb_off && (size_t)h * s.y_rs <= s.cr_off && s.cb_off + s.ch * s.c_rs <= s.extent &&
                        s.cr_off + s.ch * s.c_rs <= s.extent && s.named <= s.extent && s.y_rs >= (size_t)B * w && s.c_rs >= c_row;
    L tight;
    YccLayout ts;
    const int rc_init = ycc_layout_init(&tight, w, h, B, l.layout, l.sub_x, l.sub_y);
    const int rc_tight = ycc_layout_resolve(&tight, w, h, B, false, 0, 0, &ts);
    if (!inside || rc_init != LANCZOS_OK || rc_tight != LANCZOS_OK || ts.named != ts.extent || ts.cw != s.cw || ts.ch != s.ch) {
        printf("BAD line %d: inside %d init %d tight %d\n", line, (int)inside, rc_init, rc_tight);
        return 1;
    }
    return 0;
}

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) {
        printf("usage: %s rows.txt\n", argv[0]);
        return 2;
    }
    long long v[19];
    int line = 0;
    for (;; line++) {
        int n = 0;
        while (n < 19 && fscanf(f, "%lld", &v[n]) == 1) n++;
        if (n != 19) break;
        const bool dest = v[1] != 0, has_win = v[6] != 0;
        const int w = (int)(dest ? (has_win ? v[9] : v[4]) : v[2]), h = (int)(dest ? (has_win ? v[10] : v[5]) : v[3]);
        const int x0 = has_win ? (int)v[7] : 0, y0 = has_win ? (int)v[8] : 0;
        if (dest ? run<lanczos_ycc_dest>(v, w, h, x0, y0, true, line) : run<lanczos_ycc_source>(v, w, h, 0, 0, false, line)) return 1;
    }
    fclose(f);
    printf("done %d\n", line);
    return 0;
}
