// lanczos_upscale_route.cpp -- the upscale entry's decision (lanczos_upscale.hpp): no kernel, no HIP call, no
// device state, no context and no environment read.  up_route says what a call of lanczos_resample_device does;
// resample_device_locked (lanczos_api.hip) issues it, and a host program can link this file with lanczos_taps.cpp alone
// (tests/native/upscale_route_check.hip holds it against tests/upscale_route_cfg.py for every kind of call).
#include "lanczos_upscale.hpp"

namespace lz {

bool fast_supports(const lanczos_desc& d, const UpGeom& g) {
    if (d.scale_d != 1) return false;
    if (g.out_pitch % 4 != 0 || (((uintptr_t)g.out) & 3) != 0 || (g.out_frame_stride & 3) != 0) return false;
    if ((size_t)g.out_pitch * g.out_rows >= (1ull << 31) || (size_t)g.in_pitch >= (1ull << 30)) return false;
#define X(T, C, S, A) \
    if (d.bytes_per_sample == (int)sizeof(T) && d.channels == C && d.scale_n == S && d.a == A) return true;
    LZ_FAST_CONFIGS(X)
#undef X
    return false;
}

bool rat_supports(const lanczos_desc& d, const UpGeom& g) {
    if (d.scale_d == 1) return false;                       // integer scales: the marching / tile kernels
    if (g.out_pitch % 4 != 0 || (((uintptr_t)g.out) & 3) != 0 || (g.out_frame_stride & 3) != 0) return false;
    // tile window bounds assume scale > 1: input span of a tile <= its output span + 2a
    return d.scale_n > d.scale_d && g.frames <= 65535;
}

// the marching kernel moves whole 16-byte chunks: rows, frames and the base must be 16-byte multiples
bool march_supports(const UpGeom& g) {
    return g.in_pitch % 16 == 0 && (((uintptr_t)g.in) & 15) == 0 && (g.in_frame_stride & 15) == 0 &&
           (size_t)g.in_pitch * g.in_rows < (1ull << 30);  // (the hoisted load offsets' out-of-range markers need the two top bits)
}

// k_prefix_reg<T, S, A> unrolls the recurrence of an unclipped frame: the plan's prefix must be that one
bool prefix_reg_supports(const lanczos_desc& d, const PrefixInfo& pi) {
#define X(T, S, A)                                                                                             \
    if (d.bytes_per_sample == (int)sizeof(T) && d.scale_n == S && d.a == A && pi.K == prefix_K(S, A) &&        \
        pi.M == prefix_M(S, A) && pi.M2 == prefix_M2(S, A))                                                    \
        return true;
    LZ_PREFIX_REG_CONFIGS(X)
#undef X
    return false;
}

void strip_input_rows(const int32_t* v_first, int a, int in_h, int row0, int rows, const PrefixInfo& pi, int* in_row0, int* in_rows) {
    int lo = v_first[row0];
    int hi = v_first[row0 + rows - 1] + 2 * a - 1;
    if (row0 < pi.K && pi.M2 - 1 > hi) hi = pi.M2 - 1;  // the in-place prefix reads a little deeper
    if (lo < 0) lo = 0;
    if (hi > in_h - 1) hi = in_h - 1;
    *in_row0 = lo;
    *in_rows = hi - lo + 1;
}

UpStrip up_strip(const lanczos_desc& d, const int32_t* v_first, const PrefixInfo& pi) {
    UpStrip s{};
    s.row0 = d.out_rows == 0 ? 0 : d.out_row0;
    s.rows = d.out_rows == 0 ? d.out_h : d.out_rows;
    strip_input_rows(v_first, d.a, d.in_h, s.row0, s.rows, pi, &s.in_row0, &s.in_rows);
    return s;
}

namespace {

UpRoute refuse(int err) {
    UpRoute r;
    r.err = err;
    return r;
}

}  // namespace

UpRoute up_route(const UpQuery& q) {
    const lanczos_desc& d = *q.d;
    const PrefixInfo& pi = q.prefix;
    UpRoute r;
    r.strip = up_strip(d, q.v_first, pi);
    const int row0 = r.strip.row0, rows = r.strip.rows;
    const bool has_prefix = row0 < pi.K;
    // the prefix recurrence needs rows [0,M) of the output and [0,M2) of the H pass in one place
    // (any depth runs: prefixes too deep for k_prefix's row arrays take the streaming form of the recurrence, k_prefix_stream)
    if (has_prefix && row0 != 0) return refuse(LANCZOS_ERR_UNSUPPORTED);

    UpGeom g{};
    g.in = q.in, g.out = q.out;
    g.in_pitch = d.in_w * d.channels * d.bytes_per_sample;
    g.out_pitch = d.out_w * d.channels * d.bytes_per_sample;
    g.in_frame_stride = r.in_frame_stride = q.in_frame_stride ? q.in_frame_stride : (size_t)g.in_pitch * r.strip.in_rows;
    g.out_frame_stride = r.out_frame_stride = q.out_frame_stride ? q.out_frame_stride : (size_t)g.out_pitch * rows;
    g.in_rows = r.strip.in_rows, g.out_rows = rows, g.frames = q.frames;

    const bool hls = d.mode == LANCZOS_MODE_HLS;
    if (hls) {
        if (q.force == LANCZOS_KERNEL_FAST || q.force == LANCZOS_KERNEL_GENERIC) return refuse(LANCZOS_ERR_UNSUPPORTED);
        if (d.channels > 4 || 2 * d.a > 2 * kMaxA) return refuse(LANCZOS_ERR_UNSUPPORTED);
        if (q.frames > 65535) return refuse(LANCZOS_ERR_UNSUPPORTED);
    }
    const bool use_fast = q.fast_ok && q.force != LANCZOS_KERNEL_GENERIC && fast_supports(d, g);
    const bool use_rat = !use_fast && q.rat_ok && q.force != LANCZOS_KERNEL_GENERIC && rat_supports(d, g);
    if (q.force == LANCZOS_KERNEL_FAST && !use_fast && !use_rat) return refuse(LANCZOS_ERR_UNSUPPORTED);

    r.n_launches = 1;
    r.tail = UpLaunch{q.frames, LANCZOS_ROUTE_PREFIX_NONE};
    if (hls) {
        r.kernel = LANCZOS_KERNEL_HLS, r.main = LANCZOS_ROUTE_MAIN_HLS;
        return r;
    }
    // LANCZOS_TILE_KERNEL=1: the tile-per-workgroup kernel (A/B measurements)
    const bool march = use_fast && !q.tile_kernel && march_supports(g);
    if (march && !q.facts) return refuse(LANCZOS_ERR_BAD_ARG);   // (fast_supports and march_facts read the same instance list)
    r.kernel = use_fast || use_rat ? LANCZOS_KERNEL_FAST : LANCZOS_KERNEL_GENERIC;
    const int skip_rows = has_prefix ? pi.K : 0;
    if (march) r.main = row0 + rows <= skip_rows ? LANCZOS_ROUTE_MAIN_NONE : LANCZOS_ROUTE_MAIN_MARCH;
    else if (use_fast) r.main = LANCZOS_ROUTE_MAIN_TILE;
    else if (use_rat && q.ratp_ok && !q.no_ratp) r.main = LANCZOS_ROUTE_MAIN_RATP;
    else r.main = use_rat ? LANCZOS_ROUTE_MAIN_RAT : LANCZOS_ROUTE_MAIN_GENERIC;

    // behind / streamed.  Columns per block: the row arrays (M + M2 rows) must fit 60 KB of LDS; deep prefixes (scales close to
    // 1) get fewer.  Deeper still (S = 1: the whole frame; S -> 1): rings of 24 rows instead of M + M2 row arrays
    int bw = 128;
    while (bw > 32 && (size_t)(pi.M + pi.M2) * bw * d.bytes_per_sample > 60 * 1024) bw >>= 1;
    const bool streamed = (size_t)(pi.M + pi.M2) * bw * d.bytes_per_sample > 60 * 1024;
    if (streamed) bw = 128;
    // How the prefix rows of a launch of nf frames are produced.  Riding on k_march (extra workgroups behind the marching ones)
    // needs a main launch at all and the row arrays to fit the workgroup's LDS; past about one prefix workgroup per CU they slow
    // the march down more than the launch they replace (config 2, ms per step riding / separate: 1 frame 0.0198 / 0.0253,
    // 8: 0.0687 / 0.0729, 16: 0.117-0.120 / 0.114-0.116, 32: 0.232 / 0.218 -- profiles/
    // round3a_ab_prefix_riding_and_ldsdma_placement.txt).  Then the register-only kernel goes out in FRONT, on the same stream,
    // where it has an instance and the frame is tall enough that no tap of the recurrence is clipped.
    auto prefix_of = [&](int nf) {
        if (!has_prefix) return LANCZOS_ROUTE_PREFIX_NONE;
        if (march && !q.separate_prefix) {
            const MarchFacts& f = *q.facts;
            const int blocks_per_frame = (d.out_w * d.channels + f.nt - 1) / f.nt;
            if ((size_t)(pi.M + pi.M2) * f.nt * d.bytes_per_sample <= (size_t)f.lds_bytes && r.main != LANCZOS_ROUTE_MAIN_NONE &&
                blocks_per_frame * nf <= f.cus)
                return LANCZOS_ROUTE_PREFIX_RIDING;
            if (d.scale_d == 1 && d.in_h >= pi.M2 && prefix_reg_supports(d, pi)) return LANCZOS_ROUTE_PREFIX_FRONT;
        }
        return streamed ? LANCZOS_ROUTE_PREFIX_STREAMED : LANCZOS_ROUTE_PREFIX_BEHIND;
    };
    if (march) {
        // A batch of twice the kernel's preferred size or more goes out as launches of that size (two chunks per (strip, frame)
        // pair, rank-aware shares: the fastest shape this kernel has) followed by the rest.  The four-workgroups-per-CU instances
        // already split at one and a half times that size: their one-workgroup-per-slot table degrades quickly (config 2, 48
        // frames: 400 us in one launch, 333 us as 32 + 16; 40 frames: 289 us either way), that of the two-workgroups-per-CU
        // instances does not (config 3, 40 frames: 251 us in one launch, 272 us as 24 + 16) --
        // profiles/round4y_ab_oversized_batch_split_rule.txt.
        const MarchFacts& f = *q.facts;
        const int strips = (d.out_w + f.strip_out_px - 1) / f.strip_out_px;
        int pf = (f.wg_per_cu * f.cus) / (2 * strips);
        while (pf > 0 && (2 * strips * pf) % 16 != 0) pf--;   // every XCD gets whole pairs of chunks (march_build_table: balanced)
        const bool split = q.frames >= 2 * pf || (LZ_SPLIT_RULE && f.wg_per_cu >= 4 && q.frames >= pf + pf / 2);
        if (pf >= 8 && split) {
            r.n_launches = (q.frames + pf - 1) / pf;
            r.body = UpLaunch{pf, prefix_of(pf)};
            r.tail.frames = q.frames - (r.n_launches - 1) * pf;
        }
    }
    r.tail.prefix = prefix_of(r.tail.frames);
    r.bw = bw;
    r.prefix_lds = streamed ? 0 : (size_t)(pi.M + pi.M2) * bw * d.bytes_per_sample;
    return r;
}

}  // namespace lz
