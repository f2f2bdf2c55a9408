// tests/native/lsb1_eps_check.hip -- the V-pass error bound eps of every LANCZOS_MODE_LSB1 instance the GPU tests reach, against
// the tolerance of the per-sample LSB1 check (tests/lsb1_check.py: delta_for -- 2^-10 for 8-bit samples; 2^-5 for 16-bit ones,
// 2^-4 at integer scales with a = 4 and 2^-3 at rational scales, where the proven 16-bit bounds are wider).  Host code only
// (hipcc compiles it without a GPU).  The check explains a sample that differs from the reference only if the reference's f64
// sum v lies within delta below the stored value; the kernels store floor(sum + eps) with |sum - v| <= eps, so delta must be at
// least 2 eps of every instance.  eps comes from the library's own host preparation, with the tables it builds:
//   fast_prepare (k_march / k_fast: bias, and bias_p of the paired chain -- lanczos_march.hpp picks one per instance, both are
//                 checked), rat_prepare (k_rat), ratp_prepare (k_ratp, where an instance exists).
// Prints one line per (family, sample type, channels, scale, a, size) and "all instances ok" when every 2 eps <= delta.
#include <hip/hip_runtime.h>
#include <cstdio>
#include "lanczos_hip.h"
#include "lanczos_rational.hpp"
using namespace lz;

static int fails = 0, lines = 0;
static double worst[3] = {0, 0, 0};   // largest eps per sample size (index = bytes)

static lanczos_desc desc(int w, int h, int c, int bytes, int n, int dd, int a) {
    lanczos_desc d = {};
    const int g = gcd(n, dd);          // lanczos.h:110, as lanczos_desc_init
    d.in_w = w;
    d.in_h = h;
    d.scale_n = n / g;
    d.scale_d = dd / g;
    d.out_w = (int)((long long)w * d.scale_n / d.scale_d);
    d.out_h = (int)((long long)h * d.scale_n / d.scale_d);
    d.channels = c;
    d.bytes_per_sample = bytes;
    d.a = a;
    d.mode = LANCZOS_MODE_LSB1;
    return d;
}

// tests/lsb1_check.py delta_for, on the reduced scale
static double delta_for(const lanczos_desc& d) {
    if (d.bytes_per_sample == 1) return 1.0 / 1024;
    if (d.scale_d != 1) return 1.0 / 8;
    return d.a == 4 ? 1.0 / 16 : 1.0 / 32;
}

static void report(const char* fam, const lanczos_desc& d, double eps) {
    const double delta = delta_for(d);
    const bool ok = 2.0 * eps <= delta;
    if (eps > worst[d.bytes_per_sample]) worst[d.bytes_per_sample] = eps;
    printf("eps %s u%d C%d %d/%d a%d %dx%d: %.9g  delta %.9g  2eps/delta %.4f %s\n", fam, 8 * d.bytes_per_sample, d.channels,
           d.scale_n, d.scale_d, d.a, d.in_w, d.in_h, eps, delta, 2.0 * eps / delta, ok ? "ok" : "FAILED");
    lines++;
    if (!ok) fails++;
}

static void one(int w, int h, int c, int bytes, int n, int dd, int a) {
    const lanczos_desc d = desc(w, h, c, bytes, n, dd, a);
    if (d.out_w < 1 || d.out_h < 1) return;
    AxisTaps H, V;
    build_axis(d.in_w, d.out_w, d.scale_n, d.scale_d, d.a, &H);
    build_axis(d.in_h, d.out_h, d.scale_n, d.scale_d, d.a, &V);
    if (d.scale_d == 1) {
        FastConsts fc;
        if (fast_prepare(d, H, V, &fc)) report("fast", d, fc.bias > fc.bias_p ? fc.bias : fc.bias_p);
        return;
    }
    RatHost r;
    rat_prepare(d, H, V, &r);
    if (!r.ok) return;
    report("rat", d, r.bias);
    for (int c2 : {1, 3, 4}) {          // k_ratp instances exist per channel count; its eps does not depend on it
        lanczos_desc dc = d;
        dc.channels = c2;
        if (!ratp_has(dc)) continue;
        RatPHost p;
        ratp_prepare(dc, H, V, r, &p);
        if (p.ok) report("ratp", dc, p.bias);
    }
}

int main() {
    // integer scales 2-4: every (sample type, channels, a), at the test sizes and at the full-size configurations (eps carries
    // a term that grows with the axis length, lanczos_fast.hpp fast_prepare)
    for (int bytes = 1; bytes <= 2; bytes++)
        for (int c : {1, 3, 4})
            for (int s = 2; s <= 4; s++)
                for (int a = 2; a <= 4; a++) {
                    one(160, 45, c, bytes, s, 1, a);
                    one(3840, 2160, c, bytes, s, 1, a);
                }
    // rational scales the GPU tests use (periodic ones through k_ratp where an instance exists, all through k_rat), at the
    // sizes they use and at 1080p
    const int scales[][2] = {{4, 3}, {3, 2}, {5, 2}, {5, 3}, {7, 4}, {5, 4}, {9, 8}, {17, 16}, {33, 32}, {65, 64}, {257, 256}, {1025, 1024}};
    const int sizes[][2] = {{12, 5}, {12, 9}, {64, 300}, {300, 200}, {1200, 40}, {64, 1024}};
    for (int bytes = 1; bytes <= 2; bytes++)
        for (const auto& sc : scales)
            for (int a = 2; a <= 4; a++) {
                for (const auto& sz : sizes) one(sz[0], sz[1], 3, bytes, sc[0], sc[1], a);
                if (sc[1] <= 4) one(1920, 1080, 3, bytes, sc[0], sc[1], a);
            }
    printf("%d instances, largest eps: u8 %.9g, u16 %.9g\n", lines, worst[1], worst[2]);
    if (fails) {
        printf("%d instances FAILED: 2 eps > delta\n", fails);
        return 1;
    }
    printf("all instances ok\n");
    return 0;
}
