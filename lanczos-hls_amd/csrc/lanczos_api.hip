// lanczos_api.hip -- the extern "C" boundary (include/lanczos_hip.h) over the HIP kernels.
//
// Replaces, for the resample path only: lanczos() (lanczos.cpp:86-98) with its strip scheduler
// process_channel (lanczos.cpp:68-83), the Col/Row workers (worker.cpp:134-284), the weight ROM
// (kernel.cpp:40-67) and the cyclic line buffer (cyclic_buffer.h).  Here: host-tabulated taps that stay
// resident on the device, one fused H+V kernel launch per batch of frames, and a tiny launch IN FRONT of it (same
// stream) for the in-place prefix rows of large batches; small batches carry those rows inside the main launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/lanczos_hip.h"
#include "lanczos_env.hpp"
#include "lanczos_fast.hpp"
#include "lanczos_layout.hpp"
#include "lanczos_march.hpp"
#include "lanczos_generic.hpp"
#include "lanczos_hls.hpp"
#include "lanczos_rational.hpp"
#include "lanczos_resize.hpp"
#include "lanczos_kernels_common.hpp"
#include "lanczos_taps.hpp"
#include "lanczos_upscale.hpp"

namespace {

struct PlanKey {
    int in_w, in_h, out_w, out_h, channels, bps, sn, sd, a, hls;
};

struct Plan {
    lz::AxisTaps H, V;
    lz::PrefixInfo prefix;
    lz::TapTables dev{};       // device copies: pointers into the cache item's one block
    lz::FastConsts fast{};      // phase weights etc. for the specialised kernels
    bool fast_ok = false;
    lz::RatHost rat;            // rational scales: per-index f32 weights, integer-phase flags (k_rat)
    lz::RatTables rat_dev{};
    lz::RatPHost ratp;          // exactly periodic rational scales: per-phase weights (k_ratp)
    lz::RatTables ratp_dev{};
    const float* ratp_w_dev = nullptr;
};
using PlanCache = lz::UploadCache<PlanKey, Plan>;

}  // namespace

static constexpr size_t kMaxPlans = 32;

struct lanczos_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    lz::Lifetime life;                    // where every replaced device block of the context goes (lanczos_cache.hpp)
    PlanCache plans{&life, kMaxPlans};    // tap tables, one block per shape
    lz::WgTabCache wg_tabs{&life};        // k_march's workgroup tables, one per launch shape
    std::mutex mu;
    int last_kernel = LANCZOS_KERNEL_NONE;
    int last_tensor_route = 0;   // lanczos_last_tensor_route: LANCZOS_TENSOR_* of the last call, 0 unless it was a tensor call
    int last_source_route = 0;   // lanczos_last_source_route: LANCZOS_SOURCE_* of the last call that had a source layout
    int last_dest_route = 0;     // lanczos_last_dest_route: LANCZOS_DEST_* of the last call that had a destination layout
    lanczos_ycc_info last_ycc{};  // lanczos_last_ycc_info: what the last successful lanczos_resize_ycc_* call launched
    lanczos_ycc_out_info last_ycc_out{};  // lanczos_last_ycc_out_info: ... lanczos_resize_ycc_out call launched
    lanczos_ycc16_info last_ycc16{};  // lanczos_last_ycc16_info: ... lanczos_resize_ycc16 call launched
    int last_route = 0;      // lanczos_last_route: main kernel, prefix route and launch count of the last upscale call
    int route_launches = 0;  // launches of the call in flight (reset by the entry points, counted where a launch is issued)
    int route_seen = 0;      // prefix routes of those launches, one bit each
    int last_hip = 0;
    int force = LANCZOS_KERNEL_NONE;
    lz::ScratchBlock stage_in, stage_out;   // staging for lanczos_resample_host
    // timing: event triples (start, middle, end) around a call's kernels; ev_prefix_first[i]: the in-place prefix kernel ran
    // in FRONT of the main kernel (start..middle = prefix, middle..end = main) instead of behind it
    bool timing = false;
    std::vector<hipEvent_t> ev;
    std::vector<char> ev_prefix_first;
    int ev_used = 0;
    int launches = 0;
    double main_ms = 0, prefix_ms = 0;
#ifdef LZ_PROFILE_BITS
    void* stamp_buf = nullptr;   // diagnostic builds: per-wave cycle sums + residency census of k_march (lanczos_diag_report)
#endif
    hipStream_t copy_in = nullptr, copy_out = nullptr;  // lanczos_resample_host pipeline
    std::vector<hipEvent_t> pipe_ev;
    lz::ScratchBlock planar_in, planar_out;   // interleaved scratch frames of lanczos_resample_planar_device
    lz::ResizeState* resize = nullptr;   // lanczos_resize_* (lanczos_resize.hip), created on first use
};
#ifdef LZ_PROFILE_BITS
static constexpr size_t kStampBytes = 16384 * 8 * 6 * 8;
#endif

namespace {

#define LZ_HIP(ctx, call)                                  \
    do {                                                   \
        hipError_t e_ = (call);                            \
        if (e_ != hipSuccess) {                            \
            (ctx)->last_hip = (int)e_;                     \
            return LANCZOS_ERR_HIP;                        \
        }                                                  \
    } while (0)

// lanczos_last_route: an upscale entry point starts a call with route_begin; every launch of the call reports itself with
// route_launch at the point where it is issued
void route_begin(lanczos_ctx* ctx) {
    ctx->last_route = ctx->route_launches = ctx->route_seen = ctx->last_tensor_route = 0;
    ctx->wg_tabs.last_valid = false;   // lanczos_last_march_table: no k_march launch in this call yet
}
void route_launch(lanczos_ctx* ctx, int main_kernel, int prefix_route) {
    if (ctx->route_launches < 0x7fff) ctx->route_launches++;
    ctx->route_seen |= 1 << prefix_route;
    ctx->last_route = main_kernel | prefix_route << 4 | ctx->route_seen << 8 | ctx->route_launches << 16;
}

// The plan of a shape: tap tables built on the host and uploaded ONCE, on the stream of the first call that needs them (the
// entry points stay asynchronous on the caller's stream).  Upload, ordering of other streams, capture, eviction and release are
// the upload cache's (lanczos_cache.hpp); here are the key, the host-side preparation and the layout of the block.
int get_plan(lanczos_ctx* ctx, const lanczos_desc* d, hipStream_t stream, Plan** out) {
    PlanKey key;
    memset(&key, 0, sizeof(key));
    const bool hls = d->mode == LANCZOS_MODE_HLS;
    key = PlanKey{d->in_w, d->in_h, d->out_w, d->out_h, d->channels, d->bytes_per_sample,
                  d->scale_n, d->scale_d, d->a, hls ? 1 + d->reserved[0] : 0};
    if (PlanCache::Item* it = ctx->plans.find(key)) {
        LZ_HIP(ctx, ctx->plans.use(it, stream));
        *out = it;
        return LANCZOS_OK;
    }
    Plan plan, *p = &plan;
    if (hls) {  // ROM weights, exact stepping, no in-place prefix (lanczos_hls.hpp)
        lz::build_axis_hls(d->in_w, d->out_w, d->scale_n, d->scale_d, d->a, &p->H, d->reserved[0]);
        lz::build_axis_hls(d->in_h, d->out_h, d->scale_n, d->scale_d, d->a, &p->V, d->reserved[0]);
    } else {
        lz::build_axis(d->in_w, d->out_w, d->scale_n, d->scale_d, d->a, &p->H);
        lz::build_axis(d->in_h, d->out_h, d->scale_n, d->scale_d, d->a, &p->V);
        p->prefix = lz::prefix_info(p->V);
    }
    const int taps = 2 * d->a;
    // one device block: h_first | v_first | h_w | v_w  (8-byte aligned sections)
    size_t off_hf = 0;
    size_t off_vf = off_hf + (((size_t)d->out_w * 4 + 7) & ~(size_t)7);
    size_t off_hw = off_vf + (((size_t)d->out_h * 4 + 7) & ~(size_t)7);
    size_t off_vw = off_hw + (size_t)d->out_w * taps * 8;
    size_t off_xw = off_vw + (size_t)d->out_h * taps * 8;
    size_t total = off_xw + (size_t)lz::kFastMaxS * lz::kMaxTaps * 8;
    p->fast_ok = !hls && lz::fast_prepare(*d, p->H, p->V, &p->fast);
    if (!hls && d->scale_d != 1) lz::rat_prepare(*d, p->H, p->V, &p->rat);
    size_t off_hwf = 0, off_vwf = 0, off_hint = 0, off_vint = 0;
    if (p->rat.ok) {  // appended sections: f32 weights and integer-phase flags of both axes
        off_hwf = total;
        off_vwf = off_hwf + (size_t)d->out_w * taps * 4;
        off_hint = off_vwf + (size_t)d->out_h * taps * 4;
        off_vint = off_hint + (((size_t)d->out_w + 7) & ~(size_t)7);
        total = off_vint + (((size_t)d->out_h + 7) & ~(size_t)7);
    }
    size_t off_pw = 0;
    if (p->rat.ok && lz::ratp_has(*d)) lz::ratp_prepare(*d, p->H, p->V, p->rat, &p->ratp);
    if (p->ratp.ok) {
        off_pw = total;
        total += sizeof(p->ratp.phase_w);
    }
    std::vector<uint8_t> block(total, 0);
    uint8_t* const host = block.data();
    if (p->rat.ok) {
        memcpy(host + off_hwf, p->rat.h_wf.data(), p->rat.h_wf.size() * 4);
        memcpy(host + off_vwf, p->rat.v_wf.data(), p->rat.v_wf.size() * 4);
        memcpy(host + off_hint, p->rat.h_int.data(), p->rat.h_int.size());
        memcpy(host + off_vint, p->rat.v_int.data(), p->rat.v_int.size());
    }
    if (p->ratp.ok) memcpy(host + off_pw, p->ratp.phase_w, sizeof(p->ratp.phase_w));
    if (p->fast_ok) {  // row 0: integer phase, row ph: phase ph
        memcpy(host + off_xw, p->fast.wi, lz::kMaxTaps * 8);
        for (int ph = 1; ph < lz::kFastMaxS; ph++)
            memcpy(host + off_xw + (size_t)ph * lz::kMaxTaps * 8, p->fast.wd[ph], lz::kMaxTaps * 8);
    }
    memcpy(host + off_hf, p->H.first.data(), (size_t)d->out_w * 4);
    memcpy(host + off_vf, p->V.first.data(), (size_t)d->out_h * 4);
    memcpy(host + off_hw, p->H.w.data(), (size_t)d->out_w * taps * 8);
    memcpy(host + off_vw, p->V.w.data(), (size_t)d->out_h * taps * 8);
    hipError_t e = hipSuccess;
    PlanCache::Item* const it = ctx->plans.insert(key, std::move(plan), host, total, stream, lz::Upload::on_stream, &e);
    if (!it) {
        ctx->last_hip = (int)e;
        return LANCZOS_ERR_HIP;
    }
    p = it;   // the payload has moved into the item: what follows points its tables into the item's block
    uint8_t* b = (uint8_t*)it->dev_block;
    p->dev.h_first = (const int32_t*)(b + off_hf);
    p->dev.v_first = (const int32_t*)(b + off_vf);
    p->dev.h_w = (const double*)(b + off_hw);
    p->dev.v_w = (const double*)(b + off_vw);
    p->dev.x_w = (const double*)(b + off_xw);
    if (p->rat.ok) {
        p->rat_dev.h_wf = (const float*)(b + off_hwf);
        p->rat_dev.v_wf = (const float*)(b + off_vwf);
        p->rat_dev.h_int = b + off_hint;
        p->rat_dev.v_int = b + off_vint;
        p->rat_dev.bias = p->rat.bias;
        p->rat_dev.vbias_rne = p->rat.vbias_rne;
        p->rat_dev.near2 = p->rat.near2;
        p->rat_dev.vlim = p->rat.vlim;
        p->rat_dev.tight = p->rat.tight;
    }
    if (p->ratp.ok) {
        p->ratp_dev = p->rat_dev;
        p->ratp_dev.bias = p->ratp.bias;
        p->ratp_dev.vbias_rne = p->ratp.vbias_rne;
        p->ratp_dev.near2 = p->ratp.near2;
        p->ratp_w_dev = (const float*)(b + off_pw);
    }
    *out = p;
    return LANCZOS_OK;
}

}  // namespace

extern "C" {

const char* lanczos_version(void) {
#ifdef LZ_PROFILE_BITS
    return "lanczos-hls_amd 0.1 (gfx950) +profile-bits";   // diagnostic build: ablation bits, stamps (scripts/ablate*.sh check for this)
#else
    return "lanczos-hls_amd 0.1 (gfx950)";
#endif
}

const char* lanczos_strerror(int code) {
    switch (code) {
        case LANCZOS_OK: return "ok";
        case LANCZOS_ERR_BAD_ARG: return "bad argument (null pointer, size, channels, a, or out != in*N/D)";
        case LANCZOS_ERR_UNSUPPORTED: return "unsupported configuration (scale < 1, or a strip that cuts the in-place prefix rows)";
        case LANCZOS_ERR_NO_DEVICE: return "no HIP device";
        case LANCZOS_ERR_HIP: return "HIP runtime error";
        case LANCZOS_ERR_NOMEM: return "out of memory";
        case LANCZOS_ERR_RCCL: return "RCCL call failed (lanczos_multi_last_error)";
        default: return "unknown error";
    }
}

int lanczos_desc_init(lanczos_desc* d, int in_w, int in_h, int channels, int bytes_per_sample, int scale_n,
                      int scale_d, int a) {
    if (!d) return LANCZOS_ERR_BAD_ARG;
    memset(d, 0, sizeof(*d));
    if (scale_n <= 0 || scale_d <= 0) return LANCZOS_ERR_BAD_ARG;
    const int g = lz::gcd(scale_n, scale_d);  // lanczos.h:110: the reference reduces N/D by their gcd
    d->in_w = in_w;
    d->in_h = in_h;
    d->scale_n = scale_n / g;
    d->scale_d = scale_d / g;
    d->out_w = (int)((long long)in_w * d->scale_n / d->scale_d);
    d->out_h = (int)((long long)in_h * d->scale_n / d->scale_d);
    d->channels = channels;
    d->bytes_per_sample = bytes_per_sample;
    d->a = a;
    d->mode = LANCZOS_MODE_LSB1;
    return lz::validate(d);
}

int lanczos_validate(const lanczos_desc* d) { return lz::validate(d); }

int lanczos_inplace_rows(const lanczos_desc* d) {
    if (lz::validate(d) != LANCZOS_OK) return -1;
    if (d->mode == LANCZOS_MODE_HLS) return 0;  // the HLS pipeline has no in-place pass
    lz::AxisTaps V;
    lz::build_axis(d->in_h, d->out_h, d->scale_n, d->scale_d, d->a, &V);
    return lz::prefix_info(V).K;
}

int lanczos_strip_input_rows(const lanczos_desc* d, int out_row0, int out_rows, int* in_row0, int* in_rows) {
    int rc = lz::validate(d);
    if (rc != LANCZOS_OK) return rc;
    if (!in_row0 || !in_rows || out_row0 < 0 || out_rows <= 0 || out_row0 + out_rows > d->out_h)
        return LANCZOS_ERR_BAD_ARG;
    lz::AxisTaps V;
    if (d->mode == LANCZOS_MODE_HLS) {
        lz::build_axis_hls(d->in_h, d->out_h, d->scale_n, d->scale_d, d->a, &V, d->reserved[0]);  // (the fixed-point stepper moves the window)
        lz::strip_input_rows(V.first.data(), d->a, d->in_h, out_row0, out_rows, lz::PrefixInfo(), in_row0, in_rows);
        return LANCZOS_OK;
    }
    lz::build_axis(d->in_h, d->out_h, d->scale_n, d->scale_d, d->a, &V);
    lz::strip_input_rows(V.first.data(), d->a, d->in_h, out_row0, out_rows, lz::prefix_info(V), in_row0, in_rows);
    return LANCZOS_OK;
}

size_t lanczos_in_frame_bytes(const lanczos_desc* d) {
    return d ? (size_t)d->in_w * d->in_h * d->channels * d->bytes_per_sample : 0;
}
size_t lanczos_out_frame_bytes(const lanczos_desc* d) {
    return d ? (size_t)d->out_w * d->out_h * d->channels * d->bytes_per_sample : 0;
}

double lanczos_kernel(double x, int a) { return lz::kernel(x, a); }

double lanczos_kernel_idx(int in_idx, int out_idx, int scale_n, int scale_d, int a) {
    // the software model's argument for (output index, input index): x - i with x = out / SCALE
    // (full_TB.h:57,60).  The HLS twin looks up |out*SCALE_D - in*SCALE_N| / SCALE_N (kernel.cpp:56-58),
    // the same point up to the rounding of the division.
    const double SCALE = (double)scale_n / scale_d;
    const double x = (double)out_idx / SCALE;
    return lz::kernel(x - in_idx, a);
}

int lanczos_taps_host(const lanczos_desc* d, int axis, int32_t* first, double* weights) {
    int rc = lz::validate(d);
    if (rc != LANCZOS_OK) return rc;
    if (!first || !weights || (axis != 0 && axis != 1)) return LANCZOS_ERR_BAD_ARG;
    lz::AxisTaps t;
    if (d->mode == LANCZOS_MODE_HLS)
        lz::build_axis_hls(axis == 0 ? d->in_w : d->in_h, axis == 0 ? d->out_w : d->out_h, d->scale_n, d->scale_d, d->a, &t, d->reserved[0]);
    else if (axis == 0)
        lz::build_axis(d->in_w, d->out_w, d->scale_n, d->scale_d, d->a, &t);
    else
        lz::build_axis(d->in_h, d->out_h, d->scale_n, d->scale_d, d->a, &t);
    memcpy(first, t.first.data(), t.first.size() * sizeof(int32_t));
    memcpy(weights, t.w.data(), t.w.size() * sizeof(double));
    return LANCZOS_OK;
}

int lanczos_create(lanczos_ctx** out, int device) {
    if (!out) return LANCZOS_ERR_BAD_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return LANCZOS_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return LANCZOS_ERR_NO_DEVICE;
    (void)lz::env();  // every environment switch is read here, once per process (lanczos_env.hpp)
    lanczos_ctx* ctx = new (std::nothrow) lanczos_ctx();
    if (!ctx) return LANCZOS_ERR_NOMEM;
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return LANCZOS_ERR_HIP;
    }
    *out = ctx;
    return LANCZOS_OK;
}

#ifdef LZ_PROFILE_BITS
// Diagnostic builds only (make variant EXTRA=-DLZ_PROFILE_BITS): where a wave of k_march<u8,3,2,3> spends its cycles and when /
// where every workgroup ran, from the stamps of the last LANCZOS_STAMP=1 launch.  Not part of the C ABI of include/lanczos_hip.h.
static void diag_report(lanczos_ctx* ctx, FILE* out) {
    if (!ctx->stamp_buf) return;
    {
        std::vector<unsigned long long> h(kStampBytes / 8);
        if (hipMemcpy(h.data(), ctx->stamp_buf, kStampBytes, hipMemcpyDeviceToHost) == hipSuccess) {
            double sum[5] = {0, 0, 0, 0, 0}, ticks = 0;
            long n = 0;
            for (size_t i = 0; i + 5 < (size_t)16384 * 8 * 3; i += 6)
                if (h[i + 5]) {
                    for (int k = 0; k < 5; k++) sum[k] += (double)h[i + k];
                    ticks += (double)h[i + 5];
                    n++;
                }
            {   // residency census: per CU, time-averaged and peak number of co-resident workgroups
                std::map<unsigned long long, std::vector<std::pair<unsigned long long, int>>> ev;
                const size_t off = (size_t)16384 * 8 * 3;
                long wgs = 0;
                unsigned long long tmin = ~0ull, tmax = 0;
                for (size_t i = off; i + 2 < h.size(); i += 3) {
                    if (!h[i + 1]) continue;
                    const unsigned hw = (unsigned)h[i + 2];
                    const unsigned long long key = ((h[i + 2] >> 32) << 16) | (((hw >> 13) & 7) << 8) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 15);
                    ev[key].push_back({h[i], +1});
                    ev[key].push_back({h[i + 1], -1});
                    if (h[i] < tmin) tmin = h[i];
                    if (h[i + 1] > tmax) tmax = h[i + 1];
                    wgs++;
                }
                double avg = 0;
                int peak = 0;
                for (auto& kv : ev) {
                    std::sort(kv.second.begin(), kv.second.end());
                    int cur = 0;
                    unsigned long long last = tmin, area = 0;
                    for (auto& e : kv.second) {
                        area += (unsigned long long)cur * (e.first - last);
                        last = e.first;
                        cur += e.second;
                        if (cur > peak) peak = cur;
                    }
                    avg += (double)area / (double)(tmax - tmin ? tmax - tmin : 1);
                }
                {   // spread of start times and lifetimes (100 MHz ticks -> us)
                    std::vector<double> st, life;
                    for (size_t i = off; i + 2 < h.size(); i += 3)
                        if (h[i + 1]) {
                            st.push_back((h[i] - tmin) / 100.0);
                            life.push_back((h[i + 1] - h[i]) / 100.0);
                        }
                    std::sort(st.begin(), st.end());
                    std::sort(life.begin(), life.end());
                    if (!st.empty())
                        fprintf(out, "CENSUS start us: p50=%.1f p90=%.1f max=%.1f | lifetime us: min=%.1f p10=%.1f p50=%.1f p90=%.1f max=%.1f\n",
                                st[st.size() / 2], st[st.size() * 9 / 10], st.back(), life.front(), life[life.size() / 10],
                                life[life.size() / 2], life[life.size() * 9 / 10], life.back());
                }
                if (!lz::env().census_dump.empty()) {  // raw records for offline correlation: wg index, start, end, xcc, hw_id
                    FILE* df = fopen(lz::env().census_dump.c_str(), "w");
                    if (df) {
                        for (size_t i = off, k = 0; i + 2 < h.size(); i += 3, k++)
                            if (h[i + 1])
                                fprintf(df, "%zu %llu %llu %u %u\n", k, h[i] - tmin, h[i + 1] - tmin, (unsigned)(h[i + 2] >> 32),
                                        (unsigned)h[i + 2]);
                        fclose(df);
                    }
                }
                if (wgs)
                    fprintf(out, "CENSUS wgs=%ld distinct_cus=%zu span=%.1f us avg_resident_wgs_per_cu=%.2f peak=%d\n", wgs,
                            ev.size(), (tmax - tmin) / 100.0, avg / ev.size(), peak);
            }
            if (n)
                fprintf(out, "STAMP waves=%ld ticks/wave=%.1f cycles/tick: issue=%.0f hpass=%.0f commit=%.0f vpass=%.0f barrier=%.0f\n",
                        n, ticks / n, sum[0] / ticks, sum[1] / ticks, sum[2] / ticks, sum[3] / ticks, sum[4] / ticks);
            for (int w = 0; w < 6; w++) {  // the same by wave index inside the workgroup (k_march<u8,3,2,3>: 6 waves; 0-2 run the H pass)
                double s6[5] = {0, 0, 0, 0, 0}, tk = 0;
                for (size_t i = (size_t)w * 6; i + 5 < (size_t)16384 * 8 * 3; i += 36)
                    if (h[i + 5]) {
                        for (int k = 0; k < 5; k++) s6[k] += (double)h[i + k];
                        tk += (double)h[i + 5];
                    }
                if (tk > 0)
                    fprintf(out, "STAMP wave %d: issue=%.0f hpass=%.0f commit=%.0f vpass=%.0f barrier=%.0f\n", w, s6[0] / tk, s6[1] / tk,
                            s6[2] / tk, s6[3] / tk, s6[4] / tk);
            }
        }
    }
}
#endif

int lanczos_destroy(lanczos_ctx* ctx) {
    if (!ctx) return LANCZOS_ERR_BAD_ARG;
    (void)hipSetDevice(ctx->device);
    // Launches of this context may still be running on the caller's streams: the device is drained before anything they read
    // is freed (the only device-wide wait of the library, at the one point where it is owed).
    (void)hipDeviceSynchronize();
    ctx->plans.release_all();
    ctx->wg_tabs.release_all();
    delete ctx->resize;
    ctx->life.release_all();   // (before the context's streams go; the scratch blocks free themselves with the context)
#ifdef LZ_PROFILE_BITS
    if (ctx->stamp_buf) {
        diag_report(ctx, stderr);
        (void)hipFree(ctx->stamp_buf);
    }
#endif
    for (hipEvent_t e : ctx->ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->pipe_ev) (void)hipEventDestroy(e);
    if (ctx->copy_in) (void)hipStreamDestroy(ctx->copy_in);
    if (ctx->copy_out) (void)hipStreamDestroy(ctx->copy_out);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return LANCZOS_OK;
}

int lanczos_timing_enable(lanczos_ctx* ctx, int on) {
    if (!ctx) return LANCZOS_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->timing = on != 0;
    return LANCZOS_OK;
}

static int timing_flush(lanczos_ctx* ctx) {
    const int used = ctx->ev_used;
    ctx->ev_used = 0;  // whatever happens below, the next call starts from a clean slate
    for (int i = 0; i + 2 < used; i += 3) {
        float a = 0, b = 0;
        LZ_HIP(ctx, hipEventSynchronize(ctx->ev[i + 2]));
        LZ_HIP(ctx, hipEventElapsedTime(&a, ctx->ev[i], ctx->ev[i + 1]));
        LZ_HIP(ctx, hipEventElapsedTime(&b, ctx->ev[i + 1], ctx->ev[i + 2]));
        const bool prefix_first = ctx->ev_prefix_first[i / 3] != 0;  // start..middle = the prefix kernel in front of the main one
        ctx->main_ms += prefix_first ? b : a;
        ctx->prefix_ms += prefix_first ? a : b;
        ctx->launches++;
    }
    return LANCZOS_OK;
}

int lanczos_timing_read(lanczos_ctx* ctx, int* launches, double* main_kernel_ms, double* prefix_kernel_ms) {
    if (!ctx) return LANCZOS_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    (void)hipSetDevice(ctx->device);
    int rc = timing_flush(ctx);
    if (rc != LANCZOS_OK) return rc;
    if (launches) *launches = ctx->launches;
    if (main_kernel_ms) *main_kernel_ms = ctx->main_ms;
    if (prefix_kernel_ms) *prefix_kernel_ms = ctx->prefix_ms;
    ctx->launches = 0;
    ctx->main_ms = ctx->prefix_ms = 0;
    return LANCZOS_OK;
}

int lanczos_last_kernel(const lanczos_ctx* ctx) { return ctx ? ctx->last_kernel : LANCZOS_KERNEL_NONE; }
int lanczos_last_route(const lanczos_ctx* ctx) { return ctx ? ctx->last_route : 0; }
int lanczos_last_hip_error(const lanczos_ctx* ctx) { return ctx ? ctx->last_hip : 0; }

// Host data only (the item's page-locked source block): no stream, no device.  Like the other last_* reports it is read between
// the context's calls, by the thread that made them.
int lanczos_last_march_table(const lanczos_ctx* ctx, lanczos_march_table_info* info, int32_t* entries, int capacity) {
    if (!ctx || !info || capacity < 0) return -LANCZOS_ERR_BAD_ARG;
    memset(info, 0, sizeof(*info));
    const lz::WgTabCache::Item* it = ctx->wg_tabs.last();
    if (!it) return 0;
    info->workgroups = it->n;
    info->segs = it->segs;
    info->mode = it->mode_a ? LANCZOS_MARCH_TABLE_A : LANCZOS_MARCH_TABLE_B;
    info->rank_aware = it->balanced ? 1 : 0;
    const long long* const k = it->key.k;
    info->strips = (int32_t)k[1], info->frames = (int32_t)k[2];
    info->m_lo = (int32_t)k[3], info->m_hi = (int32_t)k[4];
    info->wg_per_cu = (int32_t)k[5], info->cus = (int32_t)k[6];
    const int total = it->n * it->segs;
    if (entries) {
        static_assert(sizeof(lz::WgEntry) == 4 * sizeof(int32_t), "a table entry is four int32");
        memcpy(entries, it->host_block, sizeof(lz::WgEntry) * (size_t)(capacity < total ? capacity : total));
    }
    return total;
}

int lanczos_force_kernel(lanczos_ctx* ctx, int family) {
    if (!ctx || family < LANCZOS_KERNEL_NONE || family > LANCZOS_KERNEL_FAST) return LANCZOS_ERR_BAD_ARG;  // (_HLS follows the mode)
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->force = family;
    return LANCZOS_OK;
}

// (bytes per sample, a) -> <T, TAPS>: the instance ladder of k_rat, k_prefix and k_prefix_stream.  f(T(), integral_constant<TAPS>())
extern "C++" {
template <typename F>
static void with_sample_taps(int bytes_per_sample, int a, F&& f) {
    auto taps = [&](auto t) {
        if (a == 2) f(t, std::integral_constant<int, 4>());
        else if (a == 3) f(t, std::integral_constant<int, 6>());
        else f(t, std::integral_constant<int, 8>());
    };
    if (bytes_per_sample == 1) taps(uint8_t());
    else taps(uint16_t());
}
}

// In-place prefix rows of an integer scale as a register-only kernel (k_prefix_reg) on `stream`, in FRONT of the marching kernel
// (5 us by events of a 210 us step).  A fork / join onto a side stream so that it overlaps the march was measured and dropped
// (the two event dependencies cost 14 us per step).  up_route sends a launch here only where prefix_reg_supports.
static hipError_t launch_prefix_front(const lanczos_desc* d, const lz::FrameGeom& g, const Plan* p, hipStream_t stream) {
    const int samples_w = d->out_w * d->channels;
    dim3 grid((samples_w + 127) / 128, g.frames);
#define X(T, S, A)                                                                                  \
    if (d->bytes_per_sample == (int)sizeof(T) && d->scale_n == S && d->a == A)                      \
        hipLaunchKernelGGL((lz::k_prefix_reg<T, S, A>), grid, dim3(128), 0, stream, g, p->dev);
    LZ_PREFIX_REG_CONFIGS(X)
#undef X
    return hipGetLastError();
}

// The event triple (start, middle, end) around one launch of a call, where timing is on.  begin() reserves it -- only once
// nothing but a HIP failure can stop the call -- and records the start; commit() records the end and counts the triple
// (ev_used += 3) after all three records succeeded, so timing_flush never meets an unrecorded event.
struct LaunchTimer {
    lanczos_ctx* ctx;
    hipStream_t stream;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    int begin() {
        if (!ctx->timing) return LANCZOS_OK;
        if (ctx->ev_used + 3 > 3 * 4096) {
            const int rc = timing_flush(ctx);
            if (rc != LANCZOS_OK) return rc;
        }
        while ((int)ctx->ev.size() < ctx->ev_used + 3) {
            hipEvent_t e;
            LZ_HIP(ctx, hipEventCreate(&e));
            ctx->ev.push_back(e);
        }
        ctx->ev_prefix_first.resize(ctx->ev.size() / 3 + 1, 0);
        LZ_HIP(ctx, hipEventRecord(ctx->ev[ctx->ev_used], stream));
        for (int i = 0; i < 3; i++) ev[i] = ctx->ev[ctx->ev_used + i];
        return LANCZOS_OK;
    }
    int middle() {   // start..middle: the main kernel, or the prefix kernel that went in front of it
        if (ev[0]) LZ_HIP(ctx, hipEventRecord(ev[1], stream));
        return LANCZOS_OK;
    }
    int commit(bool prefix_first) {
        if (!ev[0]) return LANCZOS_OK;
        LZ_HIP(ctx, hipEventRecord(ev[2], stream));
        ctx->ev_prefix_first[ctx->ev_used / 3] = prefix_first ? 1 : 0;
        ctx->ev_used += 3;
        return LANCZOS_OK;
    }
};

// one launch of a route: the prefix rows in front, the main kernel, the prefix rows behind it, as the route lists them
static int issue_launch(lanczos_ctx* ctx, const lanczos_desc* d, const Plan* p, const lz::UpRoute& rt, const lz::UpLaunch& launch,
                        const lz::MarchFacts& facts, const lz::FrameGeom& g, hipStream_t stream) {
    const int rows = rt.strip.rows, frames = launch.frames;
    const bool front = launch.prefix == LANCZOS_ROUTE_PREFIX_FRONT;
    LaunchTimer timer{ctx, stream};
    int rc = timer.begin();
    if (rc != LANCZOS_OK) return rc;
    if (front) {
        LZ_HIP(ctx, launch_prefix_front(d, g, p, stream));
        if ((rc = timer.middle()) != LANCZOS_OK) return rc;
    }
    switch (rt.main) {
        case LANCZOS_ROUTE_MAIN_HLS: {
            const int tiles_x = (d->out_w + lz::kHlsTileW - 1) / lz::kHlsTileW;
            const int tiles_y = (rows + lz::kHlsTileH - 1) / lz::kHlsTileH;
            dim3 grid(tiles_x * tiles_y, frames);
            if (d->bytes_per_sample == 1)
                hipLaunchKernelGGL(lz::k_hls<uint8_t>, grid, dim3(lz::kHlsThreads), 0, stream, g, p->dev);
            else
                hipLaunchKernelGGL(lz::k_hls<uint16_t>, grid, dim3(lz::kHlsThreads), 0, stream, g, p->dev);
            LZ_HIP(ctx, hipGetLastError());
            break;
        }
        case LANCZOS_ROUTE_MAIN_MARCH: {
            lz::FrameGeom gm = g;
            const bool riding = launch.prefix == LANCZOS_ROUTE_PREFIX_RIDING;
            if (riding) gm.prefix_K = p->prefix.K, gm.prefix_M = p->prefix.M, gm.prefix_M2 = p->prefix.M2;
            LZ_HIP(ctx, lz::march_issue(*d, gm, p->dev, p->fast, stream, riding, facts, &ctx->wg_tabs));
            break;
        }
        case LANCZOS_ROUTE_MAIN_NONE: break;   // a strip that ends inside the prefix rows: nothing marches
        case LANCZOS_ROUTE_MAIN_TILE: LZ_HIP(ctx, lz::fast_launch(*d, g, p->dev, p->fast, stream)); break;
        case LANCZOS_ROUTE_MAIN_RATP: LZ_HIP(ctx, lz::ratp_launch(*d, g, p->dev, p->ratp_dev, p->ratp_w_dev, stream)); break;
        case LANCZOS_ROUTE_MAIN_RAT: {
            const int row_bytes = d->out_w * d->channels * d->bytes_per_sample;
            const int tiles_x = (row_bytes + lz::kRatTileRowBytes - 1) / lz::kRatTileRowBytes;
            const int tiles_y = (rows + lz::kRatTileH - 1) / lz::kRatTileH;
            dim3 grid(tiles_x * tiles_y, frames);
            const bool ex = d->mode == LANCZOS_MODE_EXACT;
            with_sample_taps(d->bytes_per_sample, d->a, [&](auto t, auto taps) {
                using T = decltype(t);
                constexpr int TAPS = decltype(taps)::value;
                if (ex) hipLaunchKernelGGL((lz::k_rat<T, TAPS, true>), grid, dim3(lz::kRatThreads), 0, stream, g, p->dev, p->rat_dev);
                else hipLaunchKernelGGL((lz::k_rat<T, TAPS, false>), grid, dim3(lz::kRatThreads), 0, stream, g, p->dev, p->rat_dev);
            });
            LZ_HIP(ctx, hipGetLastError());
            break;
        }
        default: {
            const int samples_w = d->out_w * d->channels;
            const int tiles_x = (samples_w + lz::kGenTileW - 1) / lz::kGenTileW;
            const int tiles_y = (rows + lz::kGenTileH - 1) / lz::kGenTileH;
            dim3 grid(tiles_x * tiles_y, frames);
            if (d->bytes_per_sample == 1)
                hipLaunchKernelGGL(lz::k_generic<uint8_t>, grid, dim3(lz::kGenTileW), 0, stream, g, p->dev);
            else
                hipLaunchKernelGGL(lz::k_generic<uint16_t>, grid, dim3(lz::kGenTileW), 0, stream, g, p->dev);
            LZ_HIP(ctx, hipGetLastError());
        }
    }
    ctx->last_kernel = rt.kernel;
    if (!front && (rc = timer.middle()) != LANCZOS_OK) return rc;
    if (launch.prefix == LANCZOS_ROUTE_PREFIX_BEHIND || launch.prefix == LANCZOS_ROUTE_PREFIX_STREAMED) {
        const int samples_w = d->out_w * d->channels, bw = rt.bw;
        dim3 grid((samples_w + bw - 1) / bw, frames);
        const int K = p->prefix.K, M = p->prefix.M, M2 = p->prefix.M2;
        with_sample_taps(d->bytes_per_sample, d->a, [&](auto t, auto taps) {
            using T = decltype(t);
            constexpr int TAPS = decltype(taps)::value;
            if (launch.prefix == LANCZOS_ROUTE_PREFIX_STREAMED)
                hipLaunchKernelGGL((lz::k_prefix_stream<T, TAPS>), grid, dim3(128), 0, stream, g, p->dev, K, M);
            else
                hipLaunchKernelGGL((lz::k_prefix<T, TAPS>), grid, dim3(bw), rt.prefix_lds, stream, g, p->dev, K, M, M2);
        });
        LZ_HIP(ctx, hipGetLastError());
    }
    route_launch(ctx, rt.main, launch.prefix);
    return timer.commit(front);
}

// the resample proper; ctx->mu is held by the caller.  The plan's facts and the marching instance's go to up_route
// (lanczos_upscale.hpp), which decides everything the call does; what it lists is issued here.
static int resample_device_locked(lanczos_ctx* ctx, const lanczos_desc* d, const void* d_in, void* d_out, int frames,
                                  size_t in_frame_stride, size_t out_frame_stride, void* stream_v) {
    LZ_HIP(ctx, hipSetDevice(ctx->device));
    // NULL is the NULL (legacy default) stream -- NOT the context's private stream: a caller whose producers run
    // on the default stream (torch's default stream is handle 0) must be ordered behind them
    hipStream_t stream = (hipStream_t)stream_v;
    Plan* p = nullptr;
    const int rc = get_plan(ctx, d, stream, &p);
    if (rc != LANCZOS_OK) return rc;
    lz::MarchFacts facts{};
    const hipError_t fe = p->fast_ok ? lz::march_facts(*d, &facts) : hipErrorNotSupported;
    if (fe != hipSuccess && fe != hipErrorNotSupported) LZ_HIP(ctx, fe);

    lz::UpQuery q;
    q.d = d, q.frames = frames;
    q.in_frame_stride = in_frame_stride, q.out_frame_stride = out_frame_stride;
    q.in = (uintptr_t)d_in, q.out = (uintptr_t)d_out;
    q.force = ctx->force;
    q.fast_ok = p->fast_ok, q.rat_ok = p->rat.ok, q.ratp_ok = p->ratp.ok;
    q.prefix = p->prefix, q.v_first = p->V.first.data();
    q.tile_kernel = lz::env().tile_kernel, q.separate_prefix = lz::env().separate_prefix, q.no_ratp = lz::env().no_ratp;
    q.facts = fe == hipSuccess ? &facts : nullptr;
    const lz::UpRoute rt = lz::up_route(q);
    if (rt.err != LANCZOS_OK) return rt.err;

    lz::FrameGeom g{};
    g.in_pitch = d->in_w * d->channels * d->bytes_per_sample;
    g.out_pitch = d->out_w * d->channels * d->bytes_per_sample;
    g.in_frame_stride = rt.in_frame_stride;
    g.out_frame_stride = rt.out_frame_stride;
    g.in_w = d->in_w;
    g.in_h = d->in_h;
    g.out_w = d->out_w;
    g.out_h = d->out_h;
    g.channels = d->channels;
    g.a = d->a;
    g.in_row0 = rt.strip.in_row0;
    g.in_rows = rt.strip.in_rows;
    g.out_row0 = rt.strip.row0;
    g.out_rows = rt.strip.rows;
    g.skip_rows = rt.strip.row0 < p->prefix.K ? p->prefix.K : 0;
    g.hls_bp = d->mode == LANCZOS_MODE_HLS ? d->reserved[0] : 0;
    g.debug_skip = 0;
    g.stamps = nullptr;
#ifdef LZ_PROFILE_BITS
    // diagnostic builds only: ablation bits, and (LANCZOS_STAMP=1) the kernel instance that sums s_memtime deltas per phase
    // and records when / where every workgroup ran; reported by diag_report() when the context is destroyed
    g.debug_skip = lz::env().debug_skip;
    if (lz::env().stamp) {
        if (!ctx->stamp_buf) (void)hipMalloc(&ctx->stamp_buf, kStampBytes), (void)hipMemset(ctx->stamp_buf, 0, kStampBytes);
        g.stamps = (unsigned long long*)ctx->stamp_buf;
    }
#endif
    // (with timing on, every launch of a split batch commits its own event triple: what is timed is what is shipped)
    for (int i = 0, f0 = 0; i < rt.n_launches; i++) {
        const lz::UpLaunch launch = rt.launch(i);
        g.in = (const uint8_t*)d_in + (size_t)f0 * g.in_frame_stride;
        g.out = (uint8_t*)d_out + (size_t)f0 * g.out_frame_stride;
        g.frames = launch.frames;
        const int lrc = issue_launch(ctx, d, p, rt, launch, facts, g, stream);
        if (lrc != LANCZOS_OK) return lrc;
        f0 += launch.frames;
    }
    return LANCZOS_OK;
}

int lanczos_resample_device(lanczos_ctx* ctx, const lanczos_desc* d, const void* d_in, void* d_out, int frames,
                            size_t in_frame_stride, size_t out_frame_stride, void* stream_v) {
    if (!ctx || !d_in || !d_out || frames <= 0) return LANCZOS_ERR_BAD_ARG;
    int rc = lz::validate(d);
    if (rc != LANCZOS_OK) return rc;
    std::lock_guard<std::mutex> lock(ctx->mu);
    route_begin(ctx);
    return resample_device_locked(ctx, d, d_in, d_out, frames, in_frame_stride, out_frame_stride, stream_v);
}

int lanczos_host_alloc(void** p, size_t bytes) {
    if (!p || bytes == 0) return LANCZOS_ERR_BAD_ARG;
    *p = nullptr;
    return hipHostMalloc(p, bytes, hipHostMallocDefault) == hipSuccess ? LANCZOS_OK : LANCZOS_ERR_NOMEM;
}

int lanczos_host_free(void* p) {
    if (!p) return LANCZOS_OK;
    return hipHostFree(p) == hipSuccess ? LANCZOS_OK : LANCZOS_ERR_HIP;
}

// Host buffers in, host buffers out.  Frames are pushed through in groups on three streams (copy-in, resample,
// copy-out) chained by events, so with page-locked buffers (lanczos_host_alloc, or the caller's own registered
// memory) the PCIe copies of neighbouring groups overlap each other and the kernels; with pageable memory the
// runtime stages the copies and the calls degrade to the serial order -- same results either way.
int lanczos_resample_host(lanczos_ctx* ctx, const lanczos_desc* d, const void* in, void* out, int frames) {
    if (!ctx || !in || !out || frames <= 0) return LANCZOS_ERR_BAD_ARG;
    int rc = lz::validate(d);
    if (rc != LANCZOS_OK) return rc;
    // The staging buffers, the two copy streams and the pipeline events belong to the context: the lock is held
    // for the whole call (calls on one context are serialised; use one context per host thread to overlap them).
    std::lock_guard<std::mutex> lock(ctx->mu);
    LZ_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->stream) return LANCZOS_ERR_HIP;
    route_begin(ctx);
    Plan* p = nullptr;
    rc = get_plan(ctx, d, ctx->stream, &p);   // (the pipeline's resample calls run on the context's stream)
    if (rc != LANCZOS_OK) return rc;
    const lz::UpStrip strip = lz::up_strip(*d, p->V.first.data(), p->prefix);
    const size_t in_frame = (size_t)d->in_w * d->channels * d->bytes_per_sample * strip.in_rows;
    const size_t out_frame = (size_t)d->out_w * d->channels * d->bytes_per_sample * strip.rows;
    if (!ctx->copy_in) LZ_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_in, hipStreamNonBlocking));
    if (!ctx->copy_out) LZ_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_out, hipStreamNonBlocking));
    // (the context's own streams: never captured.  The copy streams touch one block each, the kernels both)
    LZ_HIP(ctx, ctx->stage_in.reserve(&ctx->life, in_frame * frames, ctx->copy_in, false));
    LZ_HIP(ctx, ctx->stage_out.reserve(&ctx->life, out_frame * frames, ctx->copy_out, false));
    ctx->stage_in.note(ctx->stream, false), ctx->stage_out.note(ctx->stream, false);
    // groups of at most 4 frames, at most 64 groups in flight per call
    int group = frames >= 8 ? 4 : (frames >= 2 ? (frames + 1) / 2 : 1);
    if ((frames + group - 1) / group > 64) group = (frames + 63) / 64;
    const int ngroups = (frames + group - 1) / group;
    while ((int)ctx->pipe_ev.size() < 2 * ngroups) {
        hipEvent_t e;
        LZ_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->pipe_ev.push_back(e);
    }
    // One failing step must not leave copies in flight on the caller's buffers: whatever the outcome, all three
    // streams are drained before the call returns.
    auto pipeline = [&]() -> int {
        for (int gi = 0; gi < ngroups; gi++) {
            const int f0 = gi * group, nf = (f0 + group <= frames) ? group : frames - f0;
            const uint8_t* hin = (const uint8_t*)in + (size_t)f0 * in_frame;
            uint8_t* din = (uint8_t*)ctx->stage_in.p + (size_t)f0 * in_frame;
            uint8_t* dout = (uint8_t*)ctx->stage_out.p + (size_t)f0 * out_frame;
            uint8_t* hout = (uint8_t*)out + (size_t)f0 * out_frame;
            LZ_HIP(ctx, hipMemcpyAsync(din, hin, in_frame * nf, hipMemcpyHostToDevice, ctx->copy_in));
            LZ_HIP(ctx, hipEventRecord(ctx->pipe_ev[2 * gi], ctx->copy_in));
            LZ_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->pipe_ev[2 * gi], 0));
            const int rc2 = resample_device_locked(ctx, d, din, dout, nf, 0, 0, ctx->stream);
            if (rc2 != LANCZOS_OK) return rc2;
            LZ_HIP(ctx, hipEventRecord(ctx->pipe_ev[2 * gi + 1], ctx->stream));
            LZ_HIP(ctx, hipStreamWaitEvent(ctx->copy_out, ctx->pipe_ev[2 * gi + 1], 0));
            LZ_HIP(ctx, hipMemcpyAsync(hout, dout, out_frame * nf, hipMemcpyDeviceToHost, ctx->copy_out));
        }
        return LANCZOS_OK;
    };
    rc = pipeline();
    const hipError_t e_in = hipStreamSynchronize(ctx->copy_in);
    const hipError_t e_k = hipStreamSynchronize(ctx->stream);
    const hipError_t e_out = hipStreamSynchronize(ctx->copy_out);
    if (rc != LANCZOS_OK) return rc;
    for (hipError_t e : {e_in, e_k, e_out})
        if (e != hipSuccess) {
            ctx->last_hip = (int)e;
            return LANCZOS_ERR_HIP;
        }
    return LANCZOS_OK;
}

// ---- planar <-> interleaved (full_TB.h:127-138, 146-165) --------------------------------------------------------
static int layout_check(const void* src, const void* dst, int w, int h, int channels, int bytes_per_sample, int frames) {
    if (!src || !dst || w <= 0 || h <= 0 || frames <= 0) return LANCZOS_ERR_BAD_ARG;
    if ((channels != 1 && channels != 3 && channels != 4) || (bytes_per_sample != 1 && bytes_per_sample != 2))
        return LANCZOS_ERR_BAD_ARG;
    if (h > 65535 || frames > 65535) return LANCZOS_ERR_UNSUPPORTED;
    return LANCZOS_OK;
}

static int layout_call(lanczos_ctx* ctx, bool to_interleaved, const void* src, void* dst, int w, int h, int channels,
                       int bytes_per_sample, int frames, void* stream) {
    if (!ctx) return LANCZOS_ERR_BAD_ARG;
    const int rc = layout_check(src, dst, w, h, channels, bytes_per_sample, frames);
    if (rc != LANCZOS_OK) return rc;
    std::lock_guard<std::mutex> lock(ctx->mu);
    LZ_HIP(ctx, hipSetDevice(ctx->device));
    route_begin(ctx);
    LZ_HIP(ctx, lz::layout_launch(to_interleaved, src, dst, w, h, channels, bytes_per_sample, frames, (hipStream_t)stream));
    return LANCZOS_OK;
}

int lanczos_planar_to_interleaved_device(lanczos_ctx* ctx, const void* d_planar, void* d_interleaved, int w, int h,
                                         int channels, int bytes_per_sample, int frames, void* stream) {
    return layout_call(ctx, true, d_planar, d_interleaved, w, h, channels, bytes_per_sample, frames, stream);
}

int lanczos_interleaved_to_planar_device(lanczos_ctx* ctx, const void* d_interleaved, void* d_planar, int w, int h,
                                         int channels, int bytes_per_sample, int frames, void* stream) {
    return layout_call(ctx, false, d_interleaved, d_planar, w, h, channels, bytes_per_sample, frames, stream);
}

// img_in[C][IN_H][IN_W] -> img_out[C][OUT_H][OUT_W], the arrays lanczos_expected() works on (full_TB.h:20-21,79-96).
// Whole frames only.  The interleaved scratch frames belong to the context: calls on one context must follow each
// other in stream order (one stream at a time).  The lock is held from the growth of the scratch frames to the last of the
// three launches: a second thread's call on the same context and stream can neither replace the frames nor write its own
// pixels into them between this call's launches.
int lanczos_resample_planar_device(lanczos_ctx* ctx, const lanczos_desc* d, const void* d_in_planar, void* d_out_planar,
                                   int frames, void* stream) {
    if (!ctx || !d_in_planar || !d_out_planar || frames <= 0) return LANCZOS_ERR_BAD_ARG;
    int rc = lz::validate(d);
    if (rc != LANCZOS_OK) return rc;
    if (d->out_rows != 0 && !(d->out_row0 == 0 && d->out_rows == d->out_h)) return LANCZOS_ERR_UNSUPPORTED;
    rc = layout_check(d_in_planar, d_out_planar, d->in_w, d->in_h, d->channels, d->bytes_per_sample, frames);
    if (rc == LANCZOS_OK) rc = layout_check(d_in_planar, d_out_planar, d->out_w, d->out_h, d->channels, d->bytes_per_sample, frames);
    if (rc != LANCZOS_OK) return rc;
    const size_t in_bytes = lanczos_in_frame_bytes(d) * frames, out_bytes = lanczos_out_frame_bytes(d) * frames;
    std::lock_guard<std::mutex> lock(ctx->mu);
    LZ_HIP(ctx, hipSetDevice(ctx->device));
    route_begin(ctx);
    const bool capturing = lz::stream_capturing((hipStream_t)stream);
    LZ_HIP(ctx, ctx->planar_in.reserve(&ctx->life, in_bytes, (hipStream_t)stream, capturing));
    LZ_HIP(ctx, ctx->planar_out.reserve(&ctx->life, out_bytes, (hipStream_t)stream, capturing));
    LZ_HIP(ctx, lz::layout_launch(true, d_in_planar, ctx->planar_in.p, d->in_w, d->in_h, d->channels, d->bytes_per_sample, frames,
                                  (hipStream_t)stream));
    lanczos_desc whole = *d;
    whole.out_row0 = 0;
    whole.out_rows = 0;
    rc = resample_device_locked(ctx, &whole, ctx->planar_in.p, ctx->planar_out.p, frames, 0, 0, stream);
    if (rc != LANCZOS_OK) return rc;
    // (the report of the call is that of its resample: the layout launches add nothing to it)
    const hipError_t e = lz::layout_launch(false, ctx->planar_out.p, d_out_planar, d->out_w, d->out_h, d->channels, d->bytes_per_sample,
                                           frames, (hipStream_t)stream);
    if (e != hipSuccess) {
        route_begin(ctx);
        ctx->last_hip = (int)e;
        return LANCZOS_ERR_HIP;
    }
    return LANCZOS_OK;
}

// ---- resize to any size (Pillow's contract; lanczos_resize.hip) ------------------------------------------------------
int lanczos_resize_desc_init(lanczos_resize_desc* d, int in_w, int in_h, int out_w, int out_h, int channels, int a) {
    if (!d) return LANCZOS_ERR_BAD_ARG;
    memset(d, 0, sizeof(*d));
    d->in_w = in_w, d->in_h = in_h, d->out_w = out_w, d->out_h = out_h, d->channels = channels, d->a = a;
    return lz::resize_validate(d);
}

int lanczos_resize_desc_init_ex(lanczos_resize_desc* d, int in_w, int in_h, int out_w, int out_h, int channels, int a,
                                int flags) {
    if (!d) return LANCZOS_ERR_BAD_ARG;
    memset(d, 0, sizeof(*d));
    d->in_w = in_w, d->in_h = in_h, d->out_w = out_w, d->out_h = out_h, d->channels = channels, d->a = a;
    d->reserved[0] = flags;
    return lz::resize_validate(d);
}

int lanczos_resize_desc_init_filter(lanczos_resize_desc* d, int in_w, int in_h, int out_w, int out_h, int channels,
                                    int filter, int flags) {
    if (!d) return LANCZOS_ERR_BAD_ARG;
    memset(d, 0, sizeof(*d));
    d->in_w = in_w, d->in_h = in_h, d->out_w = out_w, d->out_h = out_h, d->channels = channels, d->a = 3;
    if (filter < 0 || filter > 15 || (flags & LANCZOS_RESIZE_FILTER(15)) != 0) return LANCZOS_ERR_BAD_ARG;
    d->reserved[0] = flags | LANCZOS_RESIZE_FILTER(filter);
    return lz::resize_validate(d);
}

int lanczos_resize_validate(const lanczos_resize_desc* d) { return lz::resize_validate(d); }

int lanczos_resize_opts_init(lanczos_resize_opts* o, const lanczos_resize_desc* d) {
    if (!o) return LANCZOS_ERR_BAD_ARG;
    memset(o, 0, sizeof(*o));
    int rc = lz::resize_validate(d);
    if (rc != LANCZOS_OK) return rc;
    o->box[2] = d->in_w, o->box[3] = d->in_h;
    return LANCZOS_OK;
}

// the tables of one axis of the resize that remains once the options are resolved
static int resize_taps_any(const lanczos_resize_desc* d, const lanczos_resize_opts* o, int axis, int32_t* first,
                           int32_t* count, void* coeffs, int* ksize, bool f64) {
    int rc = lz::resize_validate(d);
    if (rc != LANCZOS_OK) return rc;
    if (!ksize || (axis != 0 && axis != 1)) return LANCZOS_ERR_BAD_ARG;
    lz::RsResolved r;
    if ((rc = lz::resize_resolve(d, o, &r)) != LANCZOS_OK) return rc;
    const int in_n = axis == 0 ? r.inner.in_w : r.inner.in_h, out_n = axis == 0 ? d->out_w : d->out_h;
    const lz::RsSpan span = axis == 0 ? r.h : r.v;
    const int filter = lz::resize_filter(d);
    *ksize = lz::resize_ksize(in_n, out_n, d->a, filter, span);
    if (!first && !count && !coeffs) return LANCZOS_OK;
    if (!first || !count || !coeffs) return LANCZOS_ERR_BAD_ARG;
    lz::ResizeAxisHost t;
    if (!lz::resize_build_axis(in_n, out_n, d->a, filter, span, &t, f64)) return LANCZOS_ERR_UNSUPPORTED;
    memcpy(first, t.first.data(), t.first.size() * sizeof(int32_t));
    memcpy(count, t.count.data(), t.count.size() * sizeof(int32_t));
    if (f64) memcpy(coeffs, t.coeffs64.data(), t.coeffs64.size() * sizeof(double));
    else memcpy(coeffs, t.coeffs.data(), t.coeffs.size() * sizeof(int32_t));
    return LANCZOS_OK;
}

int lanczos_resize_taps_host_ex(const lanczos_resize_desc* d, const lanczos_resize_opts* o, int axis, int32_t* first,
                                int32_t* count, int32_t* coeffs, int* ksize) {
    return resize_taps_any(d, o, axis, first, count, coeffs, ksize, false);
}

int lanczos_resize_taps_f64_host_ex(const lanczos_resize_desc* d, const lanczos_resize_opts* o, int axis, int32_t* first,
                                    int32_t* count, double* coeffs, int* ksize) {
    return resize_taps_any(d, o, axis, first, count, coeffs, ksize, true);
}

int lanczos_resize_taps_host(const lanczos_resize_desc* d, int axis, int32_t* first, int32_t* count, int32_t* coeffs,
                             int* ksize) {
    return lanczos_resize_taps_host_ex(d, nullptr, axis, first, count, coeffs, ksize);
}

int lanczos_resize_taps_f64_host(const lanczos_resize_desc* d, int axis, int32_t* first, int32_t* count, double* coeffs,
                                 int* ksize) {
    return lanczos_resize_taps_f64_host_ex(d, nullptr, axis, first, count, coeffs, ksize);
}

int lanczos_resize_window_plan_host(const lanczos_resize_desc* d, const lanczos_resize_opts* o, const lanczos_resize_window* win,
                                    int frames, lanczos_resize_plan_ex* out) {
    int rc = lz::resize_validate(d);
    if (rc != LANCZOS_OK) return rc;
    if (frames < 1 || !out) return LANCZOS_ERR_BAD_ARG;
    return lz::resize_plan_host(d, o, win, frames, out, nullptr);
}

int lanczos_resize_plan_host_ex(const lanczos_resize_desc* d, const lanczos_resize_opts* o, int frames,
                                lanczos_resize_plan_ex* out) {
    return lanczos_resize_window_plan_host(d, o, nullptr, frames, out);
}

int lanczos_resize_window_init(lanczos_resize_window* win, const lanczos_resize_desc* d) {
    if (!win) return LANCZOS_ERR_BAD_ARG;
    memset(win, 0, sizeof(*win));
    const int rc = lz::resize_validate(d);
    if (rc != LANCZOS_OK) return rc;
    win->w = d->out_w, win->h = d->out_h;
    return LANCZOS_OK;
}

int lanczos_resize_window_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win) {
    const int rc = lz::resize_validate(d);
    if (rc != LANCZOS_OK) return rc;
    lz::RsWindow w;
    return lz::resize_window_resolve(d, win, &w);
}

int lanczos_resize_window_source(const lanczos_resize_desc* d, const lanczos_resize_opts* o, const lanczos_resize_window* win,
                                 int32_t rect[4]) {
    const int rc = lz::resize_validate(d);
    if (rc != LANCZOS_OK) return rc;
    if (!rect) return LANCZOS_ERR_BAD_ARG;
    return lz::resize_window_source(d, o, win, rect);
}

int lanczos_resize_plan_host(const lanczos_resize_desc* d, int frames, lanczos_resize_plan* out) {
    if (!out) return LANCZOS_ERR_BAD_ARG;
    lanczos_resize_plan_ex ex;
    const int rc = lanczos_resize_plan_host_ex(d, nullptr, frames, &ex);
    if (rc == LANCZOS_OK) *out = ex.inner;
    else memset(out, 0, sizeof(*out));
    return rc;
}

static int resize_state(lanczos_ctx* ctx) {
    if (!ctx->resize) ctx->resize = new (std::nothrow) lz::ResizeState(&ctx->life);
    return ctx->resize ? LANCZOS_OK : LANCZOS_ERR_NOMEM;
}

// Every lanczos_resize_*_device / _host entry is: null checks, its validators, fill the request, resize_run.
extern "C++" {
// the buffers of an entry.  Device: NULL stream = the legacy default stream, as lanczos_resample_device.  Host: the context's
struct ResizeBufs {
    const void* in;
    void* out;
    int frames;
    size_t in_frame_stride, out_frame_stride;
    void* stream;
    bool host;
    bool null() const { return !in || !out || frames <= 0; }
};
static ResizeBufs host_bufs(const void* in, void* out, int frames) { return ResizeBufs{in, out, frames, 0, 0, nullptr, true}; }

static lz::RsRequest resize_request(const lanczos_resize_desc* d, const lanczos_resize_opts* o, const lanczos_resize_window* win,
                                    const ResizeBufs& b) {
    lz::RsRequest q;
    q.d = d, q.o = o, q.win = win;
    q.in = b.in, q.out = b.out, q.frames = b.frames;
    q.in_frame_stride = b.in_frame_stride, q.out_frame_stride = b.out_frame_stride, q.stream = (hipStream_t)b.stream;
    return q;
}

// what follows the validation of every resize: the context's lock, its device, its state, the call, the routes it took
static int resize_run(lanczos_ctx* ctx, lz::RsRequest& q, bool host) {
    std::lock_guard<std::mutex> lock(ctx->mu);
    LZ_HIP(ctx, hipSetDevice(ctx->device));
    if (host && !ctx->stream) return LANCZOS_ERR_HIP;
    int rc = resize_state(ctx);
    if (rc != LANCZOS_OK) return rc;
    route_begin(ctx);
    if (host) q.stream = ctx->stream;
    q.last_kernel = &ctx->last_kernel, q.last_hip = &ctx->last_hip;
    rc = host ? lz::resize_host(ctx->resize, q) : lz::resize_device(ctx->resize, q);
    if (q.tensor) ctx->last_tensor_route = q.tc.route;   // also of a call that failed once its launches were out
    if (rc == LANCZOS_OK && q.source && q.sc.route) ctx->last_source_route = q.sc.route;   // a refused or failed call leaves them
    if (rc == LANCZOS_OK && q.dest && q.dc.route) ctx->last_dest_route = q.dc.route;
    return rc;
}

// bytes out.  src / dst NULL: the entry without that parameter
static int resize_bytes(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* o, const lanczos_resize_window* win,
                        const lanczos_resize_source* src, const lanczos_resize_dest* dst, const ResizeBufs& b) {
    if (!ctx || b.null()) return LANCZOS_ERR_BAD_ARG;
    lz::RsRequest q = resize_request(d, o, win, b);
    q.source = src != nullptr, q.dest = dst != nullptr;
    int rc = lz::resize_validate(d);
    lz::RsWindow w;   // a destination is resolved for the window
    if (rc == LANCZOS_OK && dst) rc = lz::resize_window_resolve(d, win, &w);
    if (rc == LANCZOS_OK && src) rc = lz::resize_source_resolve(d, src, &q.sc.s);
    if (rc == LANCZOS_OK && dst) rc = lz::resize_dest_resolve(d, w, dst, &q.dc.s);
    return rc != LANCZOS_OK ? rc : resize_run(ctx, q, b.host);
}

// The float and the 16-bit tensor entries are one request (lz::RsTensorOut) with another element width
template <class T>
static int resize_tensor(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* o, const lanczos_resize_window* win,
                         const T* t, int elem, const ResizeBufs& b) {
    if (!ctx || b.null()) return LANCZOS_ERR_BAD_ARG;
    lz::RsRequest q = resize_request(d, o, win, b);
    q.tensor = true;
    const int rc = lz::tensor_validate(d, win, t, elem, &q.tc.t);
    return rc != LANCZOS_OK ? rc : resize_run(ctx, q, b.host);
}

// a crops request is a view whose frame is the window (0, 0, w, h): validated as one, *win filled
static int tensor_crops_validate(const lanczos_resize_desc* d, const lanczos_resize_crops* crops, const lanczos_tensor_view* v,
                                 lanczos_resize_window* win, lz::RsTensorOut* lay) {
    const int rc = lz::resize_crops_validate(d, crops);
    if (rc != LANCZOS_OK) return rc;
    *win = lanczos_resize_window{0, 0, crops->w, crops->h, {0, 0, 0, 0}};
    return lz::tensor_view_validate(d, win, v, lay);
}

// ... and so are the entries of a view, with a window or with crops (not both), with or without a source.  cropped: the entry
// takes crops (NULL is then refused), not a window
static int resize_view(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* o, const lanczos_resize_window* win,
                       const lanczos_resize_crops* crops, bool cropped, const lanczos_resize_source* src, const lanczos_tensor_view* v,
                       const ResizeBufs& b) {
    if (win && crops) return LANCZOS_ERR_BAD_ARG;
    if (!ctx || b.null()) return LANCZOS_ERR_BAD_ARG;
    lanczos_resize_window cw;
    lz::RsRequest q = resize_request(d, o, cropped ? &cw : win, b);
    q.tensor = true, q.source = src != nullptr;
    int rc = cropped ? tensor_crops_validate(d, crops, v, &cw, &q.tc.t) : lz::tensor_view_validate(d, win, v, &q.tc.t);
    if (rc == LANCZOS_OK && src) rc = lz::resize_source_resolve(d, src, &q.sc.s);
    if (rc != LANCZOS_OK) return rc;
    if (crops) q.tc.d_origin = crops->d_origin;
    for (int f = 0; crops && b.host && f < b.frames; f++) {   // a host array can be validated: nothing is clamped here
        const int32_t x0 = crops->d_origin[2 * f], y0 = crops->d_origin[2 * f + 1];
        if (x0 < 0 || x0 > d->out_w - crops->w || y0 < 0 || y0 > d->out_h - crops->h) return LANCZOS_ERR_BAD_ARG;
    }
    return resize_run(ctx, q, b.host);
}
}   // extern "C++"

int lanczos_resize_window_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* o,
                                 const lanczos_resize_window* win, const void* d_in, void* d_out, int frames,
                                 size_t in_frame_stride, size_t out_frame_stride, void* stream) {
    return resize_bytes(ctx, d, o, win, nullptr, nullptr, {d_in, d_out, frames, in_frame_stride, out_frame_stride, stream, false});
}

int lanczos_resize_device_ex(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* o, const void* d_in,
                             void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride, void* stream) {
    return lanczos_resize_window_device(ctx, d, o, nullptr, d_in, d_out, frames, in_frame_stride, out_frame_stride, stream);
}

int lanczos_resize_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const void* d_in, void* d_out, int frames,
                          size_t in_frame_stride, size_t out_frame_stride, void* stream) {
    return lanczos_resize_device_ex(ctx, d, nullptr, d_in, d_out, frames, in_frame_stride, out_frame_stride, stream);
}

int lanczos_resize_window_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* o,
                               const lanczos_resize_window* win, const void* in, void* out, int frames) {
    return resize_bytes(ctx, d, o, win, nullptr, nullptr, host_bufs(in, out, frames));
}

int lanczos_resize_host_ex(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* o, const void* in,
                           void* out, int frames) {
    return lanczos_resize_window_host(ctx, d, o, nullptr, in, out, frames);
}

int lanczos_resize_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const void* in, void* out, int frames) {
    return lanczos_resize_host_ex(ctx, d, nullptr, in, out, frames);
}

int lanczos_resize_tensor_window_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win,
                                          const lanczos_tensor_out* t) {
    lz::RsTensorOut lay;
    return lz::tensor_validate(d, win, t, 4, &lay);
}

int lanczos_resize_tensor_validate(const lanczos_resize_desc* d, const lanczos_tensor_out* t) {
    return lanczos_resize_tensor_window_validate(d, nullptr, t);
}

int lanczos_tensor_lut_normalize(int channels, const float* mean, const float* std, float* lut) {
    if ((channels != 1 && channels != 3 && channels != 4) || !lut) return LANCZOS_ERR_BAD_ARG;
    lz::tensor_lut_normalize(channels, mean, std, lut);
    return LANCZOS_OK;
}

int lanczos_resize_tensor_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                 const lanczos_tensor_out* t, const void* d_in, void* d_out, int frames,
                                 size_t in_frame_stride, size_t out_frame_stride, void* stream) {
    return resize_tensor(ctx, d, opts, nullptr, t, 4, {d_in, d_out, frames, in_frame_stride, out_frame_stride, stream, false});
}

int lanczos_resize_tensor_window_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                        const lanczos_resize_window* win, const lanczos_tensor_out* t, const void* d_in,
                                        void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride, void* stream) {
    return resize_tensor(ctx, d, opts, win, t, 4, {d_in, d_out, frames, in_frame_stride, out_frame_stride, stream, false});
}

int lanczos_resize_tensor_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                               const lanczos_tensor_out* t, const void* in, void* out, int frames) {
    return resize_tensor(ctx, d, opts, nullptr, t, 4, host_bufs(in, out, frames));
}

int lanczos_resize_tensor_window_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                      const lanczos_resize_window* win, const lanczos_tensor_out* t, const void* in, void* out,
                                      int frames) {
    return resize_tensor(ctx, d, opts, win, t, 4, host_bufs(in, out, frames));
}

int lanczos_resize_tensor16_window_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win,
                                            const lanczos_tensor16_out* t) {
    lz::RsTensorOut lay;
    return lz::tensor_validate(d, win, t, 2, &lay);
}

int lanczos_resize_tensor16_validate(const lanczos_resize_desc* d, const lanczos_tensor16_out* t) {
    return lanczos_resize_tensor16_window_validate(d, nullptr, t);
}

int lanczos_tensor_lut_convert16(const float* in, int n, int format, uint16_t* out) {
    if (!in || !out || n < 0) return LANCZOS_ERR_BAD_ARG;
    return lz::tensor_lut_convert16(in, n, format, out) ? LANCZOS_OK : LANCZOS_ERR_BAD_ARG;
}

int lanczos_tensor16_lut_normalize(int channels, const float* mean, const float* std, int format, uint16_t* lut) {
    float f[4 * 256];
    const int rc = lanczos_tensor_lut_normalize(channels, mean, std, lut ? f : nullptr);
    return rc != LANCZOS_OK ? rc : lanczos_tensor_lut_convert16(f, channels * 256, format, lut);
}

int lanczos_resize_tensor16_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                   const lanczos_tensor16_out* t, const void* d_in, void* d_out, int frames,
                                   size_t in_frame_stride, size_t out_frame_stride, void* stream) {
    return resize_tensor(ctx, d, opts, nullptr, t, 2, {d_in, d_out, frames, in_frame_stride, out_frame_stride, stream, false});
}

int lanczos_resize_tensor16_window_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                          const lanczos_resize_window* win, const lanczos_tensor16_out* t, const void* d_in,
                                          void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride,
                                          void* stream) {
    return resize_tensor(ctx, d, opts, win, t, 2, {d_in, d_out, frames, in_frame_stride, out_frame_stride, stream, false});
}

int lanczos_resize_tensor16_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                 const lanczos_tensor16_out* t, const void* in, void* out, int frames) {
    return resize_tensor(ctx, d, opts, nullptr, t, 2, host_bufs(in, out, frames));
}

int lanczos_resize_tensor16_window_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                        const lanczos_resize_window* win, const lanczos_tensor16_out* t, const void* in,
                                        void* out, int frames) {
    return resize_tensor(ctx, d, opts, win, t, 2, host_bufs(in, out, frames));
}

int lanczos_tensor_view_init(lanczos_tensor_view* v, const lanczos_resize_desc* d, int elem_bytes) {
    if (!v || (elem_bytes != 2 && elem_bytes != 4)) return LANCZOS_ERR_BAD_ARG;
    const int rc = lz::resize_validate(d);
    if (rc != LANCZOS_OK) return rc;
    *v = lanczos_tensor_view{};
    v->chan_stride = (int64_t)d->out_h * d->out_w, v->row_stride = d->out_w, v->pix_stride = 1;
    v->elem_bytes = elem_bytes, v->out_channels = d->channels;
    for (int c = 0; c < d->channels; c++) v->src_channel[c] = c;
    return LANCZOS_OK;
}

int lanczos_resize_tensor_view_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win,
                                        const lanczos_tensor_view* v) {
    lz::RsTensorOut lay;
    return lz::tensor_view_validate(d, win, v, &lay);
}

int lanczos_resize_tensor_view_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                      const lanczos_resize_window* win, const lanczos_tensor_view* v, const void* d_in,
                                      void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride, void* stream) {
    return resize_view(ctx, d, opts, win, nullptr, false, nullptr, v, {d_in, d_out, frames, in_frame_stride, out_frame_stride, stream, false});
}

int lanczos_resize_tensor_view_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                    const lanczos_resize_window* win, const lanczos_tensor_view* v, const void* in, void* out,
                                    int frames) {
    return resize_view(ctx, d, opts, win, nullptr, false, nullptr, v, host_bufs(in, out, frames));
}

int lanczos_resize_crops_validate(const lanczos_resize_desc* d, const lanczos_resize_crops* crops) {
    return lz::resize_crops_validate(d, crops);
}

int lanczos_resize_crops_plan_host(const lanczos_resize_desc* d, const lanczos_resize_opts* o, const lanczos_resize_crops* crops,
                                   int frames, lanczos_resize_plan_ex* out) {
    const int rc = lz::resize_crops_validate(d, crops);
    if (rc != LANCZOS_OK) return rc;
    if (frames < 1 || !out) return LANCZOS_ERR_BAD_ARG;
    return lz::resize_plan_host(d, o, nullptr, frames, out, crops);
}

int lanczos_resize_tensor_crops_validate(const lanczos_resize_desc* d, const lanczos_resize_crops* crops,
                                         const lanczos_tensor_view* v) {
    lanczos_resize_window win;
    lz::RsTensorOut lay;
    return tensor_crops_validate(d, crops, v, &win, &lay);
}

int lanczos_resize_tensor_crops_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                       const lanczos_resize_crops* crops, const lanczos_tensor_view* v, const void* d_in,
                                       void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride, void* stream) {
    return resize_view(ctx, d, opts, nullptr, crops, true, nullptr, v, {d_in, d_out, frames, in_frame_stride, out_frame_stride, stream, false});
}

int lanczos_resize_tensor_crops_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                     const lanczos_resize_crops* crops, const lanczos_tensor_view* v, const void* in, void* out,
                                     int frames) {
    return resize_view(ctx, d, opts, nullptr, crops, true, nullptr, v, host_bufs(in, out, frames));
}

int lanczos_last_tensor_route(const lanczos_ctx* ctx) { return ctx ? ctx->last_tensor_route : 0; }

// ---- 16-bit and float frames into normalised tensors (lanczos_resize_tensor_norm.hip) -----------------------------------

int lanczos_tensor_norm_init(lanczos_tensor_norm* n, const lanczos_resize_desc* d, int format, int layout) {
    if (!n || (format != LANCZOS_TENSOR_F32 && format != LANCZOS_TENSOR_BF16 && format != LANCZOS_TENSOR_F16)) return LANCZOS_ERR_BAD_ARG;
    if (layout != LANCZOS_TENSOR_CHW && layout != LANCZOS_TENSOR_HWC) return LANCZOS_ERR_BAD_ARG;
    const int rc = lz::resize_validate(d);
    if (rc != LANCZOS_OK) return rc;
    *n = lanczos_tensor_norm{};
    for (int c = 0; c < 4; c++) n->div[c] = 1.0f, n->std[c] = 1.0f;
    if (layout == LANCZOS_TENSOR_CHW) n->chan_stride = (int64_t)d->out_h * d->out_w, n->row_stride = d->out_w, n->pix_stride = 1;
    else n->chan_stride = 1, n->row_stride = (int64_t)d->out_w * d->channels, n->pix_stride = d->channels;
    n->format = format, n->out_channels = d->channels;
    for (int c = 0; c < d->channels; c++) n->src_channel[c] = c;
    return LANCZOS_OK;
}

int lanczos_resize_tensor_norm_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win,
                                        const lanczos_tensor_norm* n) {
    lz::RsTensorOut lay;
    return lz::tensor_norm_validate(d, win, n, &lay);
}

extern "C++" {
static int resize_norm(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* o, const lanczos_resize_window* win,
                       const lanczos_resize_source* src, const lanczos_tensor_norm* n, const ResizeBufs& b) {
    if (!ctx || b.null()) return LANCZOS_ERR_BAD_ARG;
    lz::RsRequest q = resize_request(d, o, win, b);
    q.tensor = true, q.source = src != nullptr;
    int rc = lz::tensor_norm_validate(d, win, n, &q.tc.t);
    if (rc == LANCZOS_OK && src) rc = lz::resize_source_resolve(d, src, &q.sc.s);
    return rc != LANCZOS_OK ? rc : resize_run(ctx, q, b.host);
}
}   // extern "C++"

int lanczos_resize_tensor_norm_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                      const lanczos_resize_window* win, const lanczos_resize_source* src,
                                      const lanczos_tensor_norm* n, const void* d_in, void* d_out, int frames,
                                      size_t in_frame_stride, size_t out_frame_stride, void* stream) {
    return resize_norm(ctx, d, opts, win, src, n, {d_in, d_out, frames, in_frame_stride, out_frame_stride, stream, false});
}

int lanczos_resize_tensor_norm_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                    const lanczos_resize_window* win, const lanczos_resize_source* src,
                                    const lanczos_tensor_norm* n, const void* in, void* out, int frames) {
    return resize_norm(ctx, d, opts, win, src, n, host_bufs(in, out, frames));
}

// ---- a source layout beside the descriptor (lanczos_resize_source.hip) -------------------------------------------------
int lanczos_resize_source_init(lanczos_resize_source* src, const lanczos_resize_desc* d, int layout) {
    if (!src || (layout != LANCZOS_SOURCE_INTERLEAVED && layout != LANCZOS_SOURCE_PLANAR)) return LANCZOS_ERR_BAD_ARG;
    const int rc = lz::resize_validate(d);
    if (rc != LANCZOS_OK) return rc;
    const int64_t B = lz::resize_bps(d);
    *src = lanczos_resize_source{};
    if (layout == LANCZOS_SOURCE_PLANAR) {
        if (B != 1) return LANCZOS_ERR_UNSUPPORTED;
        src->row_stride = d->in_w, src->chan_stride = (int64_t)d->in_w * d->in_h, src->pix_stride = 1;
    } else {
        src->row_stride = (int64_t)d->in_w * d->channels * B, src->chan_stride = B, src->pix_stride = (int32_t)(d->channels * B);
    }
    return LANCZOS_OK;
}

int lanczos_resize_source_validate(const lanczos_resize_desc* d, const lanczos_resize_source* src) {
    const int rc = lz::resize_validate(d);
    if (rc != LANCZOS_OK) return rc;
    lz::RsSource s;
    return lz::resize_source_resolve(d, src, &s);
}

int lanczos_resize_source_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* o,
                                 const lanczos_resize_window* win, const lanczos_resize_source* src, const void* d_in,
                                 void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride, void* stream) {
    return resize_bytes(ctx, d, o, win, src, nullptr, {d_in, d_out, frames, in_frame_stride, out_frame_stride, stream, false});
}

int lanczos_resize_source_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* o,
                               const lanczos_resize_window* win, const lanczos_resize_source* src, const void* in, void* out,
                               int frames) {
    return resize_bytes(ctx, d, o, win, src, nullptr, host_bufs(in, out, frames));
}

int lanczos_resize_tensor_source_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                        const lanczos_resize_window* win, const lanczos_resize_crops* crops,
                                        const lanczos_resize_source* src, const lanczos_tensor_view* v, const void* d_in,
                                        void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride, void* stream) {
    return resize_view(ctx, d, opts, win, crops, crops != nullptr, src, v, {d_in, d_out, frames, in_frame_stride, out_frame_stride, stream, false});
}

int lanczos_resize_tensor_source_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                      const lanczos_resize_window* win, const lanczos_resize_crops* crops,
                                      const lanczos_resize_source* src, const lanczos_tensor_view* v, const void* in, void* out,
                                      int frames) {
    return resize_view(ctx, d, opts, win, crops, crops != nullptr, src, v, host_bufs(in, out, frames));
}

int lanczos_last_source_route(const lanczos_ctx* ctx) { return ctx ? ctx->last_source_route : 0; }

// ---- a destination layout beside the descriptor (lanczos_resize_dest.hip) ------------------------------------------------
int lanczos_resize_dest_init(lanczos_resize_dest* dst, const lanczos_resize_desc* d, const lanczos_resize_window* win, int layout) {
    if (!dst || (layout != LANCZOS_DEST_INTERLEAVED && layout != LANCZOS_DEST_PLANAR)) return LANCZOS_ERR_BAD_ARG;
    int rc = lz::resize_validate(d);
    lz::RsWindow w;
    if (rc == LANCZOS_OK) rc = lz::resize_window_resolve(d, win, &w);
    if (rc != LANCZOS_OK) return rc;
    const int64_t B = lz::resize_bps(d);
    *dst = lanczos_resize_dest{};
    if (layout == LANCZOS_DEST_PLANAR) {
        if (B != 1) return LANCZOS_ERR_UNSUPPORTED;
        dst->row_stride = w.w, dst->chan_stride = (int64_t)w.w * w.h, dst->pix_stride = 1;
    } else {
        dst->row_stride = (int64_t)w.w * d->channels * B, dst->chan_stride = B, dst->pix_stride = (int32_t)(d->channels * B);
    }
    return LANCZOS_OK;
}

int lanczos_resize_dest_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win, const lanczos_resize_dest* dst) {
    int rc = lz::resize_validate(d);
    lz::RsWindow w;
    if (rc == LANCZOS_OK) rc = lz::resize_window_resolve(d, win, &w);
    if (rc != LANCZOS_OK) return rc;
    lz::RsDest s;
    return lz::resize_dest_resolve(d, w, dst, &s);
}

int lanczos_resize_dest_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* o,
                               const lanczos_resize_window* win, const lanczos_resize_source* src, const lanczos_resize_dest* dst,
                               const void* d_in, void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride,
                               void* stream) {
    return resize_bytes(ctx, d, o, win, src, dst, {d_in, d_out, frames, in_frame_stride, out_frame_stride, stream, false});
}

int lanczos_resize_dest_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* o,
                             const lanczos_resize_window* win, const lanczos_resize_source* src, const lanczos_resize_dest* dst,
                             const void* in, void* out, int frames) {
    return resize_bytes(ctx, d, o, win, src, dst, host_bufs(in, out, frames));
}

int lanczos_last_dest_route(const lanczos_ctx* ctx) { return ctx ? ctx->last_dest_route : 0; }

// ---- YCbCr frames (lanczos_resize_ycc.hip): lanczos_resize_ycc_*, lanczos_resize_ycc_out and lanczos_resize_ycc16 fill one ----
// request, lz::YccRequest, with the bytes of a sample (B: 1, or 2 for the ycc16 entries) and what is stored
extern "C++" {
static int ycc_source_init(lanczos_ycc_source* src, const lanczos_resize_desc* d, int B, int layout, int sub_x, int sub_y) {
    if (!src) return LANCZOS_ERR_BAD_ARG;
    const int rc = lz::ycc_desc_validate(d, B);
    if (rc != LANCZOS_OK) return rc;
    return lz::ycc_layout_init(src, d->in_w, d->in_h, B, layout, sub_x, sub_y);
}

static int ycc_source_resolve(const lanczos_resize_desc* d, const lanczos_ycc_source* src, int B, lz::YccLayout* s) {
    const int rc = lz::ycc_desc_validate(d, B);
    if (rc != LANCZOS_OK) return rc;
    return lz::ycc_layout_resolve(src, d->in_w, d->in_h, B, false, 0, 0, s);
}

static int ycc_dest_init(lanczos_ycc_dest* dst, const lanczos_resize_desc* d, const lanczos_resize_window* win, int B, int layout,
                         int sub_x, int sub_y) {
    if (!dst) return LANCZOS_ERR_BAD_ARG;
    int rc = lz::ycc_desc_validate(d, B);
    lz::RsWindow w;
    if (rc == LANCZOS_OK) rc = lz::resize_window_resolve(d, win, &w);
    if (rc != LANCZOS_OK) return rc;
    return lz::ycc_layout_init(dst, w.w, w.h, B, layout, sub_x, sub_y);
}

static int ycc_dest_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win, const lanczos_ycc_dest* dst, int B) {
    int rc = lz::ycc_desc_validate(d, B);
    lz::RsWindow w;
    if (rc == LANCZOS_OK) rc = lz::resize_window_resolve(d, win, &w);
    if (rc != LANCZOS_OK) return rc;
    lz::YccLayout s;
    return lz::ycc_layout_resolve(dst, w.w, w.h, B, true, w.x0, w.y0, &s);
}

// What the launching entries share once q is resolved: the lock, the device, the resize state, the context's stream for host
// buffers, the call, and on LANCZOS_OK last_kernel and `store`, which copies q.info into the entry's public info struct
template <class Store>
static int ycc_run(lanczos_ctx* ctx, lz::YccRequest& q, bool host, Store&& store) {
    std::lock_guard<std::mutex> lock(ctx->mu);
    LZ_HIP(ctx, hipSetDevice(ctx->device));
    if (host && !ctx->stream) return LANCZOS_ERR_HIP;
    int rc = resize_state(ctx);
    if (rc != LANCZOS_OK) return rc;
    route_begin(ctx);
    if (host) q.stream = ctx->stream;
    q.last_hip = &ctx->last_hip;
    rc = host ? lz::resize_ycc_host(ctx->resize, q) : lz::resize_ycc_device(ctx->resize, q);
    if (rc == LANCZOS_OK) ctx->last_kernel = q.info.luma_kernel, store(q.info);
    return rc;
}

// every lanczos_resize_ycc_* entry: v NULL stores RGB bytes
static int resize_ycc(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* o, const lanczos_resize_window* win,
                      const lanczos_ycc_source* src, const int32_t* table, const lanczos_tensor_view* v, bool tensor,
                      const ResizeBufs& b) {
    if (!ctx || b.null() || !table) return LANCZOS_ERR_BAD_ARG;
    lz::YccRequest q;
    q.d = d, q.o = o, q.win = win, q.table = table, q.B = 1, q.kind = tensor ? lz::kYccOutElems : lz::kYccOutRgb;
    q.in = b.in, q.out = b.out, q.frames = b.frames;
    q.in_frame_stride = b.in_frame_stride, q.out_frame_stride = b.out_frame_stride, q.stream = (hipStream_t)b.stream;
    int rc = ycc_source_resolve(d, src, 1, &q.s);
    if (rc == LANCZOS_OK && tensor) rc = lz::tensor_view_validate(d, win, v, &q.t);
    if (rc != LANCZOS_OK) return rc;
    return ycc_run(ctx, q, b.host, [&](const lz::YccInfo& i) {
        ctx->last_ycc = lanczos_ycc_info{i.luma_kernel, i.chroma_kernel, i.split, i.launches, {}};
    });
}
}   // extern "C++"

int lanczos_ycc_source_init(lanczos_ycc_source* src, const lanczos_resize_desc* d, int layout, int sub_x, int sub_y) {
    return ycc_source_init(src, d, 1, layout, sub_x, sub_y);
}

int lanczos_ycc_source_validate(const lanczos_resize_desc* d, const lanczos_ycc_source* src) {
    lz::YccLayout s;
    return ycc_source_resolve(d, src, 1, &s);
}

int lanczos_ycc_table(int standard, int32_t* t) { return t && lz::ycc_table(standard, t) ? LANCZOS_OK : LANCZOS_ERR_BAD_ARG; }

int lanczos_last_ycc_info(const lanczos_ctx* ctx, lanczos_ycc_info* info) {
    if (!ctx || !info) return LANCZOS_ERR_BAD_ARG;
    *info = ctx->last_ycc;
    return LANCZOS_OK;
}

int lanczos_resize_ycc_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                              const lanczos_resize_window* win, const lanczos_ycc_source* src, const int32_t* d_table,
                              const void* d_in, void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride,
                              void* stream) {
    return resize_ycc(ctx, d, opts, win, src, d_table, nullptr, false, {d_in, d_out, frames, in_frame_stride, out_frame_stride, stream, false});
}

int lanczos_resize_ycc_tensor_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                     const lanczos_resize_window* win, const lanczos_ycc_source* src, const int32_t* d_table,
                                     const lanczos_tensor_view* v, const void* d_in, void* d_out, int frames,
                                     size_t in_frame_stride, size_t out_frame_stride, void* stream) {
    return resize_ycc(ctx, d, opts, win, src, d_table, v, true, {d_in, d_out, frames, in_frame_stride, out_frame_stride, stream, false});
}

int lanczos_resize_ycc_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                            const lanczos_resize_window* win, const lanczos_ycc_source* src, const int32_t* table, const void* in,
                            void* out, int frames) {
    return resize_ycc(ctx, d, opts, win, src, table, nullptr, false, host_bufs(in, out, frames));
}

int lanczos_resize_ycc_tensor_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                   const lanczos_resize_window* win, const lanczos_ycc_source* src, const int32_t* table,
                                   const lanczos_tensor_view* v, const void* in, void* out, int frames) {
    return resize_ycc(ctx, d, opts, win, src, table, v, true, host_bufs(in, out, frames));
}

// ---- into YCbCr frames -------------------------------------------------------------------------------------------------------
int lanczos_ycc_dest_init(lanczos_ycc_dest* dst, const lanczos_resize_desc* d, const lanczos_resize_window* win, int layout,
                          int sub_x, int sub_y) {
    return ycc_dest_init(dst, d, win, 1, layout, sub_x, sub_y);
}

int lanczos_ycc_dest_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win, const lanczos_ycc_dest* dst) {
    return ycc_dest_validate(d, win, dst, 1);
}

int lanczos_ycc_table_forward(int standard, int32_t* t) {
    return t && lz::ycc_table_forward(standard, t) ? LANCZOS_OK : LANCZOS_ERR_BAD_ARG;
}

int lanczos_last_ycc_out_info(const lanczos_ctx* ctx, lanczos_ycc_out_info* info) {
    if (!ctx || !info) return LANCZOS_ERR_BAD_ARG;
    *info = ctx->last_ycc_out;
    return LANCZOS_OK;
}

int lanczos_resize_ycc_out(lanczos_ctx* ctx, const lanczos_ycc_out_request* rq) {
    if (!ctx || !rq || !rq->in || !rq->out || !rq->dst || rq->frames <= 0) return LANCZOS_ERR_BAD_ARG;
    if (rq->memory != LANCZOS_MEM_DEVICE && rq->memory != LANCZOS_MEM_HOST) return LANCZOS_ERR_BAD_ARG;
    for (int32_t r : rq->reserved)
        if (r != 0) return LANCZOS_ERR_BAD_ARG;
    const bool from_rgb = rq->src == nullptr;
    lz::YccRequest q;
    q.d = rq->d, q.o = rq->opts, q.win = rq->win, q.dst = rq->dst, q.table = rq->table;
    q.B = 1, q.kind = from_rgb ? lz::kYccOutYccFromRgb : lz::kYccOutYcc;
    q.in = rq->in, q.out = rq->out, q.frames = rq->frames;
    q.in_frame_stride = rq->in_frame_stride, q.out_frame_stride = rq->out_frame_stride, q.stream = (hipStream_t)rq->stream;
    int rc = lz::ycc_desc_validate(rq->d, 1);
    if (rc != LANCZOS_OK) return rc;
    if (from_rgb ? !rq->table : rq->table != nullptr) return LANCZOS_ERR_BAD_ARG;   // the table belongs to RGB frames, and only to them
    if (!from_rgb && (rc = ycc_source_resolve(rq->d, rq->src, 1, &q.s)) != LANCZOS_OK) return rc;
    return ycc_run(ctx, q, rq->memory == LANCZOS_MEM_HOST, [&](const lz::YccInfo& i) {
        ctx->last_ycc_out = lanczos_ycc_out_info{i.luma_kernel, i.chroma_kernel, i.split, i.join, i.encode, i.launches, {}};
    });
}

// ---- YCbCr frames of 16-bit words --------------------------------------------------------------------------------------------
int lanczos_ycc16_matrix_init(lanczos_ycc16_matrix* m, int standard, int depth, int msb_aligned, int full_range) {
    return m && lz::ycc16_matrix_init(m, standard, depth, msb_aligned != 0, full_range != 0) ? LANCZOS_OK : LANCZOS_ERR_BAD_ARG;
}

int lanczos_ycc16_matrix_validate(const lanczos_ycc16_matrix* m) { return lz::ycc16_matrix_validate(m); }

int lanczos_ycc16_source_init(lanczos_ycc_source* src, const lanczos_resize_desc* d, int layout, int sub_x, int sub_y) {
    return ycc_source_init(src, d, 2, layout, sub_x, sub_y);
}

int lanczos_ycc16_source_validate(const lanczos_resize_desc* d, const lanczos_ycc_source* src) {
    lz::YccLayout s;
    return ycc_source_resolve(d, src, 2, &s);
}

int lanczos_ycc16_dest_init(lanczos_ycc_dest* dst, const lanczos_resize_desc* d, const lanczos_resize_window* win, int layout,
                            int sub_x, int sub_y) {
    return ycc_dest_init(dst, d, win, 2, layout, sub_x, sub_y);
}

int lanczos_ycc16_dest_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win, const lanczos_ycc_dest* dst) {
    return ycc_dest_validate(d, win, dst, 2);
}

int lanczos_last_ycc16_info(const lanczos_ctx* ctx, lanczos_ycc16_info* info) {
    if (!ctx || !info) return LANCZOS_ERR_BAD_ARG;
    *info = ctx->last_ycc16;
    return LANCZOS_OK;
}

extern "C++" {
// everything lanczos_resize_ycc16 refuses from the request alone; on LANCZOS_OK q holds the request, resolved
static int ycc16_request_resolve(const lanczos_ycc16_request* rq, lz::YccRequest& q) {
    if (!rq || !rq->in || !rq->out || !rq->src || rq->frames <= 0) return LANCZOS_ERR_BAD_ARG;
    if (rq->memory != LANCZOS_MEM_DEVICE && rq->memory != LANCZOS_MEM_HOST) return LANCZOS_ERR_BAD_ARG;
    for (int32_t r : rq->reserved)
        if (r != 0) return LANCZOS_ERR_BAD_ARG;
    const bool host = rq->memory == LANCZOS_MEM_HOST;
    q.d = rq->d, q.o = rq->opts, q.win = rq->win, q.dst = rq->dst, q.B = 2;
    q.kind = rq->dst ? lz::kYccOutYcc : rq->norm ? lz::kYccOutElems : lz::kYccOutRgb;
    q.in = rq->in, q.out = rq->out, q.frames = rq->frames;
    q.in_frame_stride = rq->in_frame_stride, q.out_frame_stride = rq->out_frame_stride, q.stream = (hipStream_t)rq->stream;
    int rc = lz::ycc_desc_validate(rq->d, 2);
    if (rc != LANCZOS_OK) return rc;
    // the output kind: dst alone, matrix alone, or matrix and norm
    if ((rq->dst != nullptr) == (rq->matrix != nullptr) || (rq->norm && !rq->matrix)) return LANCZOS_ERR_BAD_ARG;
    if ((rc = ycc_source_resolve(rq->d, rq->src, 2, &q.s)) != LANCZOS_OK) return rc;
    lz::RsResolved r;
    lz::RsWindow w;
    if ((rc = lz::resize_resolve(rq->d, rq->opts, &r)) != LANCZOS_OK) return rc;   // (a reducing_gap on words: LANCZOS_ERR_BAD_ARG)
    if ((rc = lz::resize_window_resolve(rq->d, rq->win, &w)) != LANCZOS_OK) return rc;
    lz::YccLayout t;
    if (rq->dst && (rc = lz::ycc_layout_resolve(rq->dst, w.w, w.h, 2, true, w.x0, w.y0, &t)) != LANCZOS_OK) return rc;
    if (rq->matrix) {
        if ((rc = lz::ycc16_matrix_validate(rq->matrix)) != LANCZOS_OK) return rc;
        q.m = *rq->matrix;
    }
    if (rq->norm && (rc = lz::tensor_norm_validate(rq->d, rq->win, rq->norm, &q.t)) != LANCZOS_OK) return rc;
    // bases and frame strides: words on words, RGB frames on dwords, elements on elements
    const size_t out_mask = rq->dst ? 1 : rq->norm ? (size_t)(q.t.elem - 1) : host ? 1 : 3;
    if ((((uintptr_t)rq->in | rq->in_frame_stride) & 1) != 0 || (((uintptr_t)rq->out | rq->out_frame_stride) & out_mask) != 0)
        return LANCZOS_ERR_BAD_ARG;
    if (host && (rq->in_frame_stride || rq->out_frame_stride)) return LANCZOS_ERR_BAD_ARG;
    return LANCZOS_OK;
}
}   // extern "C++"

int lanczos_ycc16_request_validate(const lanczos_ycc16_request* rq) {
    lz::YccRequest q;
    return ycc16_request_resolve(rq, q);
}

int lanczos_resize_ycc16(lanczos_ctx* ctx, const lanczos_ycc16_request* rq) {
    if (!ctx) return LANCZOS_ERR_BAD_ARG;
    lz::YccRequest q;
    const int rc = ycc16_request_resolve(rq, q);
    if (rc != LANCZOS_OK) return rc;
    return ycc_run(ctx, q, rq->memory == LANCZOS_MEM_HOST, [&](const lz::YccInfo& i) {
        ctx->last_ycc16 = lanczos_ycc16_info{i.luma_kernel, i.chroma_kernel, i.split, i.join, i.merge, i.launches, {}};
    });
}

int lanczos_reduce_size(int in_w, int in_h, int fx, int fy, const int32_t* box, int* out_w, int* out_h) {
    if (!out_w || !out_h) return LANCZOS_ERR_BAD_ARG;
    int rb[4];
    const int rc = lz::reduce_validate(in_w, in_h, 1, fx, fy, box, rb);
    if (rc != LANCZOS_OK) return rc;
    *out_w = (rb[2] - rb[0] + fx - 1) / fx, *out_h = (rb[3] - rb[1] + fy - 1) / fy;
    return LANCZOS_OK;
}

int lanczos_reduce_device(lanczos_ctx* ctx, int in_w, int in_h, int channels, int fx, int fy, const int32_t* box,
                          const void* d_in, void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride,
                          void* stream) {
    if (!ctx || !d_in || !d_out || frames <= 0) return LANCZOS_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    LZ_HIP(ctx, hipSetDevice(ctx->device));
    int rc = resize_state(ctx);
    if (rc != LANCZOS_OK) return rc;
    route_begin(ctx);
    return lz::reduce_device(ctx->resize, in_w, in_h, channels, fx, fy, box, d_in, d_out, frames, in_frame_stride,
                             out_frame_stride, (hipStream_t)stream, &ctx->last_hip);
}

int lanczos_reduce_host(lanczos_ctx* ctx, int in_w, int in_h, int channels, int fx, int fy, const int32_t* box,
                        const void* in, void* out, int frames) {
    if (!ctx || !in || !out || frames <= 0) return LANCZOS_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    LZ_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->stream) return LANCZOS_ERR_HIP;
    int rc = resize_state(ctx);
    if (rc != LANCZOS_OK) return rc;
    route_begin(ctx);
    return lz::reduce_host(ctx->resize, in_w, in_h, channels, fx, fy, box, in, out, frames, ctx->stream, &ctx->last_hip);
}

int lanczos_resize_force(lanczos_ctx* ctx, int path) {
    if (!ctx || path < LANCZOS_RESIZE_AUTO || path > LANCZOS_RESIZE_CONVERT) return LANCZOS_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(ctx->mu);
    int rc = resize_state(ctx);
    if (rc != LANCZOS_OK) return rc;
    ctx->resize->force = path;
    return LANCZOS_OK;
}

int lanczos_u8(lanczos_ctx* ctx, const uint8_t* in, int in_w, int in_h, int channels, uint8_t* out, int out_w,
               int out_h, int a) {
    if (in_w <= 0 || in_h <= 0 || out_w <= 0 || out_h <= 0) return LANCZOS_ERR_BAD_ARG;
    lanczos_desc d;
    // SCALE_N/SCALE_D = OUT_WIDTH/IN_WIDTH reduced (lanczos.h:110-114)
    int rc = lanczos_desc_init(&d, in_w, in_h, channels, 1, out_w, in_w, a);
    if (rc != LANCZOS_OK) return rc;
    if (d.out_w != out_w || d.out_h != out_h) return LANCZOS_ERR_BAD_ARG;  // full_TB.h:115-118
    // the reference-shaped single-frame entry point returns lanczos_expected()'s bytes, bit for bit; the batch and
    // device entry points default to LANCZOS_MODE_LSB1 (lanczos_desc_init)
    d.mode = LANCZOS_MODE_EXACT;
    return lanczos_resample_host(ctx, &d, in, out, 1);
}

}  // extern "C"
