// tests/native/march_fixup_census.hip -- which samples of a frame the marching kernel k_march (lanczos_march.hpp) cannot decide in
// f32, and which of those would be WRONG if its fix-up paths lost them.  Host code only (hipcc compiles it without a GPU).  The
// tap tables and FastConsts are the library's own (build_axis, fast_prepare), the constants are MarchCfg's / FastCfg's own
// constexprs; the kernel's decisions are emulated with fmaf() -- the single-rounding FMA v_fma_f32 is -- in the kernel's tap
// order and with the kernel's biases.
//
//   census  <bps> <C> <S> <a> <exact 0|1> <in_w> <in_h> <frame.raw>
//     CONST name value ...        MarchCfg / FastCfg constexprs and the FastConsts the kernel gets
//     H r tx u im bim near n_int n_near bite_int bite_near past xlo xhi ulp
//                                 one line per H unit (input row r, strip tx, unit u; units past the right edge included: the H
//                                 pass runs them) that puts anything on the worklist.  im: the integer-phase candidate bits in the
//                                 kernel's layout (bit 8*SB*e + i <-> own input sample i*VEC + e: round e appends the set bits i), bim: those that bite;
//                                 near: the unit flag (NEAR_PER_SAMPLE: some sample flagged); n_int / n_near: list entries of both
//                                 kinds; bite_*: entries whose f32 store differs from the double chain of full_TB.h:58-63 (a lost
//                                 entry is a wrong sample); past: entries at xx >= out_w (flush() skips them); xlo / xhi: the
//                                 smallest / largest output pixel with a biting COMPUTED entry (-1: none); ulp: integer-phase
//                                 entries whose exact sum the LAST BIT of the centre weight decides (with 1 - 2^-53 for the 1 the chain
//                                 stores another value): they check the fix-up's arithmetic, not only that the entry is processed
//     V y tx wave kind lanes bite down
//                                 EXACT only, one line per output row y >= K and 64-dword-column V wave whose row is redone in f64:
//                                 kind 0 = integer-phase row, 1 = computed row; lanes: undecided lanes; bite: samples of the wave
//                                 whose f32 store differs from the reference's (the intermediate is the reference's own, in double);
//                                 down: lanes of an integer-phase row that are undecided through the row two BELOW alone
//     SUM ...                     totals
//   It FAILS (exit 1) if any sample the kernel would NOT flag differs from the double chain: the proven bound, on these contents,
//   and the emulation itself.
//   searchh <bps> <C> <S> <a> <exact> <seed> <tries>   period-P rows with a flagged AND biting computed sample: MOTIFH lines
//   searchv <bps> <C> <S> <a> <seed> <tries>           period-2a columns (as the V pass meets them in an integer-phase column of
//                                                      the intermediate, a copy of the input) with an undecided, biting row: MOTIFV
//   searche <bps> <C> <S> <a> <exact> <seed> <tries>   the last a - 1 pixels of a row such that the first unit PAST the right edge
//                                                      (its window still holds them) flags: MOTIFE lines
//   searchb <bps> <C> <S> <a> <in_w> <seed> <tries>    the first and the last P + a pixels of a row of width in_w such that a computed
//                                                      sample whose taps the frame edge cuts off (floor(x) < a - 1, floor(x) > in_w - 1 - a)
//                                                      is flagged and biting against the TABLE's weights of its index: MOTIFBL / MOTIFBR
//   searchi <bps> <C> <S> <a> <seed> <tries>           2a pixels around an integer-phase candidate (the centre at index a - 1) whose
//                                                      exact sum the last bit of the centre weight decides: MOTIFI
//   searchf <bps> <C> <S> <a> <exact>                  grey values whose every computed H sample is flagged and biting on a flat row: MOTIFF
//   enum22  <C>                                        8-bit 2x a = 2: all 511^2 pair-sum combinations of the paired chain
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "lanczos_hip.h"
#include "lanczos_march.hpp"
using namespace lz;

static float fractf_hw(float x) {   // v_fract_f32: x - floor(x), clamped below 1
    const float f = x - floorf(x);
    return f >= 1.0f ? 0x1.fffffep-1f : f;
}
static uint32_t fbits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static unsigned cvt_u8_rne(float a) {    // v_cvt_pk_u8_f32: round to nearest even, saturating
    if (!(a > 0.0f)) return 0;
    const float r = nearbyintf(a);
    return r > 255.0f ? 255u : (unsigned)r;
}
static unsigned cvt_u32_sat(float a) {   // v_cvt_u32_f32: truncating, negative -> 0
    if (!(a > 0.0f)) return 0;
    return a >= 4294967296.0f ? 0xffffffffu : (unsigned)a;
}
template <typename T>
static unsigned store_ref(double x) {    // store_convert<T> (full_TB.h:63)
    const double kMax = sizeof(T) == 1 ? 255.0 : 65535.0;
    if (x > kMax) return (unsigned)kMax;
    if (x < 0) return 0;
    return (unsigned)x;
}

struct Smp { unsigned store; bool flag; };

// one computed sample of the H pass (v: the 2a window samples, ascending taps) -- march_body: hpass
template <typename K>
static Smp h_sample(const FastConsts& fc, bool exact, int ph, const float* v) {
    constexpr int TAPS = K::TAPS, A = K::A;
    const bool split = K::SPLIT && (exact || LZ_MARCH_SPLIT_LSB1);
    if (split) {
        float ah = 0.0f;
        for (int k = 0; k < A; k++) ah = fmaf(fc.wsh[ph][k], v[k] + v[TAPS - 1 - k], ah);
        const float fh = fractf_hw(ah);
        float al = fh + fc.bias_s;
        for (int k = 0; k < A; k++) al = fmaf(fc.wsl[ph][k], v[k] + v[TAPS - 1 - k], al);
        const float jt = floorf(al), r = (ah - fh) + jt;
        const unsigned uv = cvt_u32_sat(r);
        return {uv < 65535u ? uv : 65535u, fmaxf(al - jt, 1.0f - r) < fc.near2_s};
    }
    float acc = K::RNE_H ? (K::SYM ? fc.vbias_rne_p : fc.vbias_rne) : (K::SYM ? fc.bias_p : fc.bias);
    if (K::SYM) {
        for (int k = 0; k < A; k++) acc = fmaf(fc.wf[ph][k], v[k] + v[TAPS - 1 - k], acc);
    } else {
        for (int j = 0; j < TAPS; j++) {
            const int k = f32_tap_order(j, TAPS);
            acc = fmaf(fc.wf[ph][k], v[k], acc);   // (S = 3: fast_prepare made wf[2][k] == wf[1][2a-1-k]: the kernel's mirror)
        }
    }
    const float near2 = K::SYM ? fc.near2_p : fc.near2;
    if (K::RNE_H) {
        const float g = fractf_hw(fabsf(acc)) - 0.5f;
        return {cvt_u8_rne(acc), fbits(g) < fbits(near2)};
    }
    const float m = fmaxf(acc, 0.5f);
    const unsigned uv = cvt_u32_sat(m);
    return {uv < 65535u ? uv : 65535u, fractf_hw(m) < near2};
}

// one computed sample of the EXACT V pass -- march_body: vpass (MIXV, the paired and the plain float window are the same roundings)
template <typename K>
static Smp v_sample(const FastConsts& fc, int ph, const float* v) {
    constexpr int TAPS = K::TAPS, A = K::A, SB = K::SB;
    if (K::SPLIT || SB == 1) return h_sample<K>(fc, true, ph, v);   // the H pass's arithmetic and test, sample for sample
    float acc = K::SYM ? fc.bias_p : fc.bias;
    for (int j = 0; j < TAPS; j++) {
        const int k = f32_tap_order(j, TAPS);
        acc = fmaf(fc.wf[ph][k], v[k], acc);
    }
    const float lo = 0.5f, hi = 65535.5f;
    const float xc = acc < lo ? lo : (acc > hi ? hi : acc);   // v_med3_f32
    const float fl = floorf(xc);
    return {(unsigned)fl, (xc - fl) < fc.near2};
}

// SWAR lane tests of the integer-phase candidates, per byte / halfword lane (no carries cross a lane: see the kernel)
template <int SB>
static bool lane_loose(unsigned x, int vlim) {
    const unsigned HALF = SB == 1 ? 0x80u : 0x8000u, LOWL = HALF - 1;
    const unsigned addc1 = (unsigned)vlim < HALF - 1 ? HALF - 1 - (unsigned)vlim : 0;
    const unsigned t7 = x & LOWL;
    return ((((t7 + LOWL) | x) & ~((t7 + addc1) | x)) & HALF) != 0;
}
template <int SB>
static bool lane_le2(unsigned x, unsigned n) {   // top bit of (c2 - (n & LOW)) & ~n: n <= 2 * x as the kernel decides it
    const unsigned HALF = SB == 1 ? 0x80u : 0x8000u, LOWL = HALF - 1, FULL = 2 * HALF - 1;
    const unsigned c2 = (((x & LOWL) << 1) | HALF) & FULL;
    return (((c2 - (n & LOWL)) & ~n) & HALF) != 0;
}

template <typename T, int C, int S, int A>
struct Inst {
    using K = MarchCfg<T, C, S, A>;
    using F = typename K::F;
    static constexpr int TAPS = 2 * A, SB = (int)sizeof(T);

    static bool prepare(int w, int h, bool exact, AxisTaps* H, AxisTaps* V, FastConsts* fc) {
        lanczos_desc d{};
        d.in_w = w, d.in_h = h, d.channels = C, d.bytes_per_sample = SB, d.scale_n = S, d.scale_d = 1, d.a = A;
        d.out_w = w * S, d.out_h = h * S, d.out_rows = d.out_h, d.mode = exact ? LANCZOS_MODE_EXACT : LANCZOS_MODE_LSB1;
        if (validate(&d) != LANCZOS_OK) return false;
        build_axis(w, w * S, S, 1, A, H);
        build_axis(h, h * S, S, 1, A, V);
        return fast_prepare(d, *H, *V, fc);
    }

    static void constants(const FastConsts& fc, bool exact) {
        const bool split = K::SPLIT && (exact || LZ_MARCH_SPLIT_LSB1);
        const bool mixv = LZ_MARCH_MIXV && SB == 1 && K::SYM && (exact || LZ_MARCH_MIXV_LSB1) && K::MIN_WAVES > 1;
        printf("CONST MS %d MRG %d NGRP %d UPR %d P %d NU %d NWAVES %d WLW %d WL_ROUND %d NNI %d UNIT_IN_DW %d UNIT_OUT_S %d VEC %d "
               "TWP_OUT %d RS %d RS_POW2 %d NEAR_PER_SAMPLE %d SPLIT %d MIXV %d SYM %d RNE_H %d NVT %d NVT_PAD %d TAPS %d\n",
               K::MS, K::MRG, K::NGRP, K::UPR, K::P, K::NU, K::NWAVES, K::WLW, K::WL_ROUND, K::NNI, F::UNIT_IN_DW, F::UNIT_OUT_S, F::VEC,
               F::TWP_OUT, K::RS, (int)K::RS_POW2, (int)(K::NEAR_PER_SAMPLE && !split), (int)split, (int)mixv, (int)K::SYM, (int)K::RNE_H,
               K::NVT, K::NVT_PAD, TAPS);
        printf("CONST near2 %.9g near2_p %.9g near2_s %.9g vlim %d tight %d skip_last %d phase_exact_h %d\n", (double)fc.near2,
               (double)fc.near2_p, (double)fc.near2_s, fc.vlim, fc.tight, fc.skip_last, fc.phase_exact_h);
    }

    // full_TB.h:58-63 / 71-75: ascending taps, separate multiply and add, the axis table's own weights
    // (nudged: a weight of exactly 1 -- the centre tap of an integer phase -- one ulp low)
    static double chain(const AxisTaps& ax, int o, const double* v, bool nudged = false) {
        double sum = 0;
        for (int k = 0; k < TAPS; k++) {
            double w = ax.w[(size_t)o * TAPS + k];
            if (nudged && w == 1.0) w = 0x1.fffffffffffffp-1;
            sum += v[k] * w;
        }
        return sum;
    }

    static int census(bool exact, int w, int h, const char* path) {
        AxisTaps H, V;
        FastConsts fc;
        if (!prepare(w, h, exact, &H, &V, &fc)) { printf("fast_prepare refused\n"); return 2; }
        std::vector<T> img((size_t)w * h * C);
        FILE* f = fopen(path, "rb");
        if (!f || fread(img.data(), sizeof(T), img.size(), f) != img.size()) { printf("cannot read %s\n", path); return 2; }
        fclose(f);
        constants(fc, exact);
        const int out_w = w * S, out_h = h * S, strips = (out_w + F::TWP_OUT - 1) / F::TWP_OUT;
        auto px = [&](int r, int x, int c) -> unsigned { return (x < 0 || x >= w) ? 0u : img[((size_t)r * w + x) * C + c]; };
        const bool per_sample = K::NEAR_PER_SAMPLE && !(K::SPLIT && (exact || LZ_MARCH_SPLIT_LSB1));
        long fails = 0, n_units = 0, t_int = 0, t_near = 0, t_bint = 0, t_bnear = 0;
        std::vector<T> Tm((size_t)h * out_w * C);   // the reference's truncated H intermediate
        // ---------------------------------------------------------------------------------------------------------------- H pass
        for (int r = 0; r < h; r++)
            for (int tx = 0; tx < strips; tx++)
                for (int u = 0; u < K::UPR; u++) {
                    const int x0 = tx * F::TWP_IN + u * K::P;
                    unsigned im = 0, bim = 0;
                    int n_int = 0, n_near = 0, b_int = 0, b_near = 0, past = 0, xlo = -1, xhi = -1, ulp = 0;
                    bool sflag[F::UNIT_OUT_S], sbite[F::UNIT_OUT_S];
                    bool near = false;
                    for (int q = 0; q < K::P * S; q++) {
                        const int p = q / S, ph = q % S, xx = (x0 + p) * S + ph;
                        for (int c = 0; c < C; c++) {
                            const int o = q * C + c;
                            float v[TAPS];
                            for (int k = 0; k < TAPS; k++) v[k] = (float)px(r, x0 + p - (A - 1) + k, c);
                            unsigned want = 0, want_nudged = 0;
                            if (xx < out_w) {
                                // the table's out-of-range taps are 0 and the reference clamps the index: the same sum
                                double vr[TAPS];
                                for (int k = 0; k < TAPS; k++) {
                                    int i = H.first[xx] + k;
                                    i = i < 0 ? 0 : (i > w - 1 ? w - 1 : i);
                                    vr[k] = (double)img[((size_t)r * w + i) * C + c];
                                }
                                want = store_ref<T>(chain(H, xx, vr));
                                want_nudged = store_ref<T>(chain(H, xx, vr, true));
                                Tm[((size_t)r * out_w + xx) * C + c] = (T)want;
                            }
                            sflag[o] = sbite[o] = false;
                            if (ph == 0) {
                                const unsigned v0 = px(r, x0 + p, c);
                                bool cand = false;
                                if (fc.vlim > 0) {
                                    cand = lane_loose<SB>(v0, fc.vlim);
                                    if (fc.tight)
                                        cand = cand && !(lane_le2<SB>(v0, px(r, x0 + p - 2, c)) && lane_le2<SB>(v0, px(r, x0 + p + 2, c)));
                                }
                                if (cand) {
                                    const int si = p * C + c, i = si / F::VEC, e = si % F::VEC;   // own input sample si = i * VEC + e
                                    im |= 1u << (8 * SB * e + i);
                                    n_int++;
                                    if (xx >= out_w) past++;
                                    else if (want != v0) b_int++, sbite[o] = true, bim |= 1u << (8 * SB * e + i);
                                    if (xx < out_w && want_nudged != want) ulp++;
                                } else if (xx < out_w && want != v0) {
                                    if (fails++ < 10) printf("UNFLAGGED H integer phase r %d xx %d c %d: copy %u reference %u\n", r, xx, c, v0, want);
                                }
                                continue;
                            }
                            const Smp s = h_sample<K>(fc, exact, ph, v);
                            sflag[o] = s.flag;
                            near = near || s.flag;
                            if (xx < out_w && s.store != want) sbite[o] = true;
                        }
                    }
                    // what goes on the list: the flagged samples (per-sample instances) or every computed sample of a flagged unit
                    for (int q = 0; q < K::P * S; q++)
                        for (int c = 0; c < C; c++) {
                            const int o = q * C + c, xx = (x0 + q / S) * S + q % S;
                            if (q % S == 0) continue;
                            const bool listed = per_sample ? sflag[o] : near;
                            if (listed) {
                                n_near++;
                                if (xx >= out_w) past++;
                                else if (sbite[o]) b_near++, xlo = xlo < 0 ? xx : xlo, xhi = xx;
                            } else if (sbite[o]) {
                                if (fails++ < 10) printf("UNFLAGGED H r %d xx %d c %d\n", r, xx, c);
                            }
                        }
                    n_units++;
                    if (im || near) {
                        printf("H %d %d %d %x %x %d %d %d %d %d %d %d %d %d\n", r, tx, u, im, bim, (int)near, n_int, n_near, b_int, b_near, past, xlo, xhi, ulp);
                        t_int += n_int, t_near += n_near, t_bint += b_int, t_bnear += b_near;
                    }
                }
        // ---------------------------------------------------------------------------------------------------------------- V pass
        long v_rows = 0, v_redo = 0, v_bite = 0;
        if (exact) {
            const PrefixInfo pi = prefix_info(V);
            printf("CONST K %d\n", pi.K);
            auto tm = [&](int r, int xs) -> unsigned { return (r < 0 || r >= h) ? 0u : Tm[(size_t)r * out_w * C + xs]; };
            const int row_s = out_w * C;
            for (int y = pi.K; y < out_h; y++) {
                const int m = y / S, ph = y % S;
                for (int tx = 0; tx < strips; tx++)
                    for (int wv = 0; wv * 64 < K::NVT; wv++) {
                        int lanes = 0, bite = 0, down = 0;
                        bool any_col = false;
                        for (int l = 0; l < 64; l++) {
                            const int col = wv * 64 + l, xs0 = tx * F::TWS_OUT + col * F::VEC;
                            if (col >= K::NVT || xs0 + F::VEC > row_s) continue;
                            any_col = true;
                            bool und = false, dn = false;
                            int lb = 0;
                            for (int e = 0; e < F::VEC; e++) {
                                const int xs = xs0 + e;
                                float v[TAPS];
                                for (int k = 0; k < TAPS; k++) v[k] = (float)tm(m - A + 1 + k, xs);
                                double vr[TAPS];
                                for (int k = 0; k < TAPS; k++) {
                                    int i = V.first[y] + k;
                                    i = i < 0 ? 0 : (i > h - 1 ? h - 1 : i);
                                    vr[k] = (double)Tm[(size_t)i * out_w * C + xs];
                                }
                                const unsigned want = store_ref<T>(chain(V, y, vr));
                                if (ph == 0) {
                                    const unsigned v0 = tm(m, xs);
                                    bool fl = false;
                                    if (fc.vlim > 0 && SB == 1 && A >= 3 && fc.tight) {
                                        fl = lane_loose<SB>(v0, fc.vlim) && !(lane_le2<SB>(v0, tm(m - 2, xs)) && lane_le2<SB>(v0, tm(m + 2, xs)));
                                        dn = dn || (lane_loose<SB>(v0, fc.vlim) && !lane_le2<SB>(v0, tm(m + 2, xs)));
                                    } else if (fc.vlim > 0) {
                                        const float c0 = (float)v0;
                                        fl = c0 >= 1.0f && c0 <= (float)fc.vlim;
                                        if (A >= 3 && fc.tight) dn = dn || (fl && (float)tm(m + 2, xs) > 2.0f * c0);
                                        if (A >= 3 && fc.tight) fl = fl && ((float)tm(m - 2, xs) > 2.0f * c0 || (float)tm(m + 2, xs) > 2.0f * c0);
                                    }
                                    und = und || fl;
                                    if (want != v0) lb++;
                                } else {
                                    const Smp s = v_sample<K>(fc, ph, v);
                                    und = und || s.flag;
                                    if (s.store != want) lb++;
                                }
                            }
                            if (und) lanes++;
                            if (dn) down++;
                            bite += lb;
                        }
                        if (!any_col) continue;
                        v_rows++;
                        if (lanes) {
                            printf("V %d %d %d %d %d %d %d\n", y, tx, wv, ph == 0 ? 0 : 1, lanes, bite, down);
                            v_redo++, v_bite += bite > 0;
                        } else if (bite) {
                            if (fails++ < 10) printf("UNFLAGGED V y %d tx %d wave %d: %d samples differ\n", y, tx, wv, bite);
                        }
                    }
            }
        }
        printf("SUM units %ld int %ld near %ld bite_int %ld bite_near %ld vwaves %ld vredo %ld vbite %ld unflagged_wrong %ld\n", n_units, t_int,
               t_near, t_bint, t_bnear, v_rows, v_redo, v_bite, fails);
        printf(fails ? "census: FAILED\n" : "census: ok\n");
        return fails ? 1 : 0;
    }

    // period-P rows (every unit of an interior row sees the same window) with a flagged and biting computed sample
    static int searchh(bool exact, unsigned seed, long tries) {
        AxisTaps H, V;
        FastConsts fc;
        const int w = 64 * K::P, h = 8 * A;
        if (!prepare(w, h, exact, &H, &V, &fc)) return 2;
        std::mt19937_64 rng(seed);
        const int maxv = SB == 1 ? 255 : 65535;
        long flagged = 0, biting = 0;
        int found = 0;
        for (long t = 0; t < tries && found < 4; t++) {
            unsigned pat[8][4];
            // a third of the tries dark, a third mid, a third full range: the flag windows scale with nothing, the sums do
            const int top = t % 3 == 0 ? maxv : (t % 3 == 1 ? maxv / 4 : maxv / 16);
            for (int p = 0; p < K::P; p++)
                for (int c = 0; c < C; c++) pat[p][c] = (unsigned)(rng() % (unsigned)(top + 1));
            bool hit = false;
            for (int p = 0; p < K::P && !hit; p++)
                for (int ph = 1; ph < S && !hit; ph++)
                    for (int c = 0; c < C && !hit; c++) {
                        float v[TAPS];
                        double vd[TAPS];
                        for (int k = 0; k < TAPS; k++) vd[k] = v[k] = (float)pat[((p - (A - 1) + k) % K::P + K::P) % K::P][c];
                        const Smp s = h_sample<K>(fc, exact, ph, v);
                        if (!s.flag) continue;
                        flagged++;
                        const int xx = (16 * K::P + p) * S + ph;   // an interior index of that phase
                        if (s.store != store_ref<T>(chain(H, xx, vd))) hit = true;
                    }
            if (hit) {
                biting++;
                found++;
                printf("MOTIFH");
                for (int p = 0; p < K::P; p++)
                    for (int c = 0; c < C; c++) printf(" %u", pat[p][c]);
                printf("\n");
            }
        }
        printf("SEARCHH seed %u tries %ld flagged %ld found %d\n", seed, tries, flagged, found);
        return 0;
    }

    // the last a - 1 in-image pixels of a row, as the first past-edge unit sees them: zeros to their right
    static int searche(bool exact, unsigned seed, long tries) {
        AxisTaps H, V;
        FastConsts fc;
        if (!prepare(64 * K::P, 8 * A, exact, &H, &V, &fc)) return 2;
        std::mt19937_64 rng(seed);
        const int maxv = SB == 1 ? 255 : 65535;
        int found = 0;
        for (long t = 0; t < tries && found < 4; t++) {
            unsigned pat[4][4] = {};
            const int top = t % 3 == 0 ? maxv : (t % 3 == 1 ? maxv / 4 : maxv / 16);
            for (int p = 0; p < A - 1; p++)
                for (int c = 0; c < C; c++) pat[p][c] = (unsigned)(rng() % (unsigned)(top + 1));
            bool hit = false;
            for (int p = 0; p < K::P && p < A - 1 && !hit; p++)      // own pixel p of the past-edge unit: window pixels p - (a-1) + k
                for (int ph = 1; ph < S && !hit; ph++)
                    for (int c = 0; c < C && !hit; c++) {
                        float v[TAPS];
                        for (int k = 0; k < TAPS; k++) {
                            const int x = p - (A - 1) + k;     // relative to the first past-edge pixel
                            v[k] = x < 0 ? (float)pat[x + A - 1][c] : 0.0f;
                        }
                        hit = h_sample<K>(fc, exact, ph, v).flag;
                    }
            if (hit) {
                found++;
                printf("MOTIFE");
                for (int p = 0; p < A - 1; p++)
                    for (int c = 0; c < C; c++) printf(" %u", pat[p][c]);
                printf("\n");
            }
        }
        printf("SEARCHE seed %u tries %ld found %d\n", seed, tries, found);
        return 0;
    }

    // rows that are black but for their first / last P + a pixels: the units at the frame edges, whose exact chain takes the
    // per-index table row (out-of-range taps zeroed) where phase_exact_h == 0
    static int searchb(int w, unsigned seed, long tries) {
        AxisTaps H, V;
        FastConsts fc;
        if (w % K::P != 0 || !prepare(w, 8 * A, true, &H, &V, &fc)) return 2;
        const int maxv = SB == 1 ? 255 : 65535, L = K::P + A;
        for (int side = 0; side < 2; side++) {
            std::mt19937_64 rng(seed + side);
            bool found = false;
            for (long t = 0; t < tries && !found; t++) {
                unsigned pat[16][4];
                const int top = t % 3 == 0 ? maxv : (t % 3 == 1 ? maxv / 4 : maxv / 16);
                for (int p = 0; p < L; p++)
                    for (int c = 0; c < C; c++) pat[p][c] = (unsigned)(rng() % (unsigned)(top + 1));
                auto px = [&](int x, int c) -> unsigned {   // the row: pat at its first (side 0) or last (side 1) L pixels
                    if (x < 0 || x >= w) return 0u;
                    if (side == 0) return x < L ? pat[x][c] : 0u;
                    return x >= w - L ? pat[x - (w - L)][c] : 0u;
                };
                for (int xi = side == 0 ? 0 : w - A; xi < (side == 0 ? A - 1 : w) && !found; xi++)
                    for (int ph = 1; ph < S && !found; ph++)
                        for (int c = 0; c < C && !found; c++) {
                            const int xx = xi * S + ph;
                            float v[TAPS];
                            double vr[TAPS];
                            for (int k = 0; k < TAPS; k++) {
                                v[k] = (float)px(xi - (A - 1) + k, c);
                                int i = H.first[xx] + k;
                                i = i < 0 ? 0 : (i > w - 1 ? w - 1 : i);
                                vr[k] = (double)px(i, c);
                            }
                            const Smp s = h_sample<K>(fc, true, ph, v);
                            found = s.flag && s.store != store_ref<T>(chain(H, xx, vr));
                        }
                if (found) {
                    printf(side == 0 ? "MOTIFBL" : "MOTIFBR");
                    for (int p = 0; p < L; p++)
                        for (int c = 0; c < C; c++) printf(" %u", pat[p][c]);
                    printf("\n");
                }
            }
            printf("SEARCHB side %d seed %u tries %ld found %d\n", side, seed + side, tries, (int)found);
        }
        return 0;
    }

    static int searchi(unsigned seed, long tries) {
        AxisTaps H, V;
        FastConsts fc;
        if (!prepare(64 * K::P, 8 * A, true, &H, &V, &fc)) return 2;
        if (fc.vlim <= 0) tries = 0;   // no integer-phase sample is ever a candidate
        std::mt19937_64 rng(seed);
        const int maxv = SB == 1 ? 255 : 65535, xx = 16 * K::P * S;   // an interior integer-phase index
        int found = 0;
        for (long t = 0; t < tries && found < 1; t++) {
            double v[TAPS];
            for (int k = 0; k < TAPS; k++) v[k] = (double)(rng() % (unsigned)(maxv + 1));
            const unsigned v0 = 1u + (unsigned)(rng() % (unsigned)fc.vlim);
            v[A - 1] = v0;
            if (A < 3) continue;
            const bool cand = lane_loose<SB>(v0, fc.vlim) &&
                              (!fc.tight || !(lane_le2<SB>(v0, (unsigned)v[A - 3]) && lane_le2<SB>(v0, (unsigned)v[A + 1])));
            if (!cand || store_ref<T>(chain(H, xx, v)) == store_ref<T>(chain(H, xx, v, true))) continue;
            found++;
            printf("MOTIFI");
            for (int k = 0; k < TAPS; k++) printf(" %u", (unsigned)v[k]);
            printf("\n");
        }
        printf("SEARCHI seed %u tries %ld found %d\n", seed, tries, found);
        return 0;
    }

    static int searchf(bool exact) {
        AxisTaps H, V;
        FastConsts fc;
        if (!prepare(64 * K::P, 8 * A, exact, &H, &V, &fc)) return 2;
        int found = 0;
        for (int g = 1; g <= (SB == 1 ? 255 : 65535) && found < 4; g++) {
            bool all = true;
            for (int ph = 1; ph < S && all; ph++) {
                float v[TAPS];
                double vd[TAPS];
                for (int k = 0; k < TAPS; k++) vd[k] = v[k] = (float)g;
                const Smp s = h_sample<K>(fc, exact, ph, v);
                all = s.flag && s.store != store_ref<T>(chain(H, 16 * K::P * S + ph, vd));
            }
            if (all) found++, printf("MOTIFF %d\n", g);
        }
        printf("SEARCHF found %d\n", found);
        return 0;
    }

    // a column of period 2a
    static int searchv(unsigned seed, long tries) {
        AxisTaps H, V;
        FastConsts fc;
        const int w = 64 * K::P, h = 16 * A;
        if (!prepare(w, h, true, &H, &V, &fc)) return 2;
        std::mt19937_64 rng(seed);
        const int maxv = SB == 1 ? 255 : 65535;
        int found = 0;
        long flagged = 0;
        for (long t = 0; t < tries && found < 4; t++) {
            unsigned pat[TAPS];
            // values above vlim: whatever stands beside such a column, the H stage's integer-phase sample is the input sample
            for (int k = 0; k < TAPS; k++) pat[k] = (unsigned)fc.vlim + 1u + (unsigned)(rng() % (unsigned)(maxv - fc.vlim));
            bool hit = false;
            {   // integer-phase COLUMNS of the intermediate: copies of the input
                for (int r = 0; r < TAPS && !hit; r++)
                    for (int ph = S - 1; ph < S && !hit; ph++) {   // the LAST phase: the top bit of a V group's redo mask
                        float v[TAPS];
                        double vd[TAPS];
                        for (int k = 0; k < TAPS; k++) vd[k] = v[k] = (float)pat[(r + k) % TAPS];
                        const Smp s = v_sample<K>(fc, ph, v);
                        if (!s.flag) continue;
                        flagged++;
                        const int y = (4 * A + TAPS + r + A - 1) * S + ph;   // an interior row of that phase
                        if (s.store != store_ref<T>(chain(V, y, vd))) hit = true;
                    }
            }
            if (hit) {
                found++;
                printf("MOTIFV");
                for (int k = 0; k < TAPS; k++) printf(" %u", pat[k]);
                printf("\n");
            }
        }
        printf("SEARCHV seed %u tries %ld flagged %ld found %d\n", seed, tries, flagged, found);
        return 0;
    }
};

// 8-bit 2x a = 2: the paired chain sees two pair sums; every one of the 511^2 combinations, none may flag
template <int C>
static int enum22() {
    using I = Inst<uint8_t, C, 2, 2>;
    AxisTaps H, V;
    FastConsts fc;
    if (!I::prepare(256, 64, true, &H, &V, &fc)) return 2;
    long flagged = 0;
    double closest = 1;
    for (int s0 = 0; s0 <= 510; s0++)
        for (int s1 = 0; s1 <= 510; s1++) {
            float acc = fc.vbias_rne_p;
            acc = fmaf(fc.wf[1][0], (float)s0, acc);
            acc = fmaf(fc.wf[1][1], (float)s1, acc);
            const float g = fractf_hw(fabsf(acc)) - 0.5f;
            if (fbits(g) < fbits(fc.near2_p)) flagged++;
            const double sum = (double)fc.wd[1][0] * s0 + (double)fc.wd[1][1] * s1;
            const double d = std::fabs(sum - std::nearbyint(sum));
            if (sum >= 0.5 && d > 0 && d < closest) closest = d;
        }
    printf("ENUM22 C %d combinations %d flagged %ld vlim %d near2_p %.9g closest_to_an_integer %.9g\n", C, 511 * 511, flagged, fc.vlim,
           (double)fc.near2_p, closest);
    return flagged == 0 && fc.vlim == 0 ? 0 : 1;
}

int main(int argc, char** argv) {
    if (argc >= 3 && !strcmp(argv[1], "enum22")) {
        const int c = atoi(argv[2]);
        return c == 1 ? enum22<1>() : (c == 3 ? enum22<3>() : (c == 4 ? enum22<4>() : 2));
    }
    if (argc < 6) {
        printf("usage: %s census|searchh|searchv|searche|searchb|searchi|searchf|enum22 ... (see the head of the source)\n", argv[0]);
        return 2;
    }
    const int bps = atoi(argv[2]), c = atoi(argv[3]), s = atoi(argv[4]), a = atoi(argv[5]);
#define X(T, C, S, A)                                                                                                       \
    if (bps == (int)sizeof(T) && c == C && s == S && a == A) {                                                              \
        if (!strcmp(argv[1], "census") && argc == 10) return Inst<T, C, S, A>::census(atoi(argv[6]) != 0, atoi(argv[7]), atoi(argv[8]), argv[9]); \
        if (!strcmp(argv[1], "searchh") && argc == 9) return Inst<T, C, S, A>::searchh(atoi(argv[6]) != 0, (unsigned)atoi(argv[7]), atol(argv[8])); \
        if (!strcmp(argv[1], "searche") && argc == 9) return Inst<T, C, S, A>::searche(atoi(argv[6]) != 0, (unsigned)atoi(argv[7]), atol(argv[8])); \
        if (!strcmp(argv[1], "searchb") && argc == 9) return Inst<T, C, S, A>::searchb(atoi(argv[6]), (unsigned)atoi(argv[7]), atol(argv[8])); \
        if (!strcmp(argv[1], "searchi") && argc == 8) return Inst<T, C, S, A>::searchi((unsigned)atoi(argv[6]), atol(argv[7])); \
        if (!strcmp(argv[1], "searchf") && argc == 7) return Inst<T, C, S, A>::searchf(atoi(argv[6]) != 0); \
        if (!strcmp(argv[1], "searchv") && argc == 8) return Inst<T, C, S, A>::searchv((unsigned)atoi(argv[6]), atol(argv[7])); \
        return 2;                                                                                                           \
    }
    LZ_FAST_CONFIGS(X)
#undef X
    printf("no such instance\n");
    return 2;
}
