// lanczos_upscale.hpp -- what the upscale entry (lanczos_resample_device) decides, without a kernel and without a device
// (DESIGN.md 4.2).  up_route (lanczos_upscale_route.cpp) is one pure function from the facts of a call -- the descriptor, the
// buffers' alignment, the plan's facts, three environment switches and the marching instance's MarchFacts -- to everything the
// call does: the refusal, the strip geometry, the main kernel and the launches it goes out as, each with the route of its in-place
// prefix rows.  resample_device_locked (lanczos_api.hip) issues what it lists; a host program can link the route unit alone
// (tests/native/upscale_route_check.hip).  The instance lists and the predicates over them live here so that both sides see them.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/lanczos_hip.h"
#include "lanczos_taps.hpp"

// The instantiated configurations: (sample type, channels, scale, a) -- every integer scale 2..4 of the reference's params.h
// space (lanczos.h:9-31: NUM_CHANNELS 1 / 3 / 4, LANCZOS_A 2..4) for 8-bit samples, scales 2 and 3 with a = 3, 4 for 16-bit ones.
// Four groups = four translation units (csrc/lanczos_inst.hip compiled with -DLZ_INST_GROUP=0..3, in parallel).
#define LZ_FAST_CONFIGS_G0(X) /* 8-bit, 2x */ \
    X(uint8_t, 3, 2, 3) X(uint8_t, 3, 2, 2) X(uint8_t, 3, 2, 4) X(uint8_t, 4, 2, 2) X(uint8_t, 4, 2, 3) X(uint8_t, 4, 2, 4) \
    X(uint8_t, 1, 2, 2) X(uint8_t, 1, 2, 3) X(uint8_t, 1, 2, 4)
#define LZ_FAST_CONFIGS_G1(X) /* 8-bit, 3x */ \
    X(uint8_t, 3, 3, 3) X(uint8_t, 3, 3, 2) X(uint8_t, 3, 3, 4) X(uint8_t, 4, 3, 2) X(uint8_t, 4, 3, 3) X(uint8_t, 4, 3, 4) \
    X(uint8_t, 1, 3, 2) X(uint8_t, 1, 3, 3) X(uint8_t, 1, 3, 4)
#define LZ_FAST_CONFIGS_G2(X) /* 8-bit, 4x */ \
    X(uint8_t, 3, 4, 3) X(uint8_t, 3, 4, 2) X(uint8_t, 3, 4, 4) X(uint8_t, 4, 4, 2) X(uint8_t, 4, 4, 3) X(uint8_t, 4, 4, 4) \
    X(uint8_t, 1, 4, 2) X(uint8_t, 1, 4, 3) X(uint8_t, 1, 4, 4)
#define LZ_FAST_CONFIGS_G3(X) /* 16-bit */ \
    X(uint16_t, 4, 2, 4) X(uint16_t, 3, 2, 3) X(uint16_t, 4, 2, 3) X(uint16_t, 3, 2, 4) \
    X(uint16_t, 3, 3, 3) X(uint16_t, 3, 3, 4) X(uint16_t, 4, 3, 3) X(uint16_t, 4, 3, 4)
#define LZ_FAST_CONFIGS(X) LZ_FAST_CONFIGS_G0(X) LZ_FAST_CONFIGS_G1(X) LZ_FAST_CONFIGS_G2(X) LZ_FAST_CONFIGS_G3(X)

// the instances of the register-only prefix kernel k_prefix_reg<T, S, A> (lanczos_generic.hpp): (sample type, scale, a)
#define LZ_PREFIX_REG_CONFIGS(X)                                                                                        \
    X(uint8_t, 2, 2) X(uint8_t, 2, 3) X(uint8_t, 2, 4) X(uint8_t, 3, 2) X(uint8_t, 3, 3) X(uint8_t, 3, 4) X(uint8_t, 4, 2) \
    X(uint8_t, 4, 3) X(uint8_t, 4, 4) X(uint16_t, 2, 3) X(uint16_t, 2, 4) X(uint16_t, 3, 3) X(uint16_t, 3, 4)

#ifndef LZ_SPLIT_RULE   // A/B builds only (0): the four-per-CU instances split at twice the preferred size like the others
#define LZ_SPLIT_RULE 1
#endif

namespace lz {

// K, M, M2 of the in-place prefix of an integer scale on a frame tall enough that no tap is clipped: the tap rows are known at
// compile time (first = floor(y / S) - A + 1), which is what k_prefix_reg unrolls
constexpr int prefix_last_tap(int o, int S, int A) { return o / S + A; }
constexpr int prefix_K(int S, int A) {
    int k = 0;
    for (int o = 0; o < 4 * A * S + 8; o++)
        if (prefix_last_tap(o, S, A) > o) k = o + 1;
    return k;
}
constexpr int prefix_M(int S, int A) {
    int m = prefix_K(S, A);
    for (int o = 0; o < prefix_K(S, A); o++)
        if (prefix_last_tap(o, S, A) + 1 > m) m = prefix_last_tap(o, S, A) + 1;
    return m;
}
constexpr int prefix_M2(int S, int A) {
    int m2 = 0;
    for (int o = 0; o < prefix_M(S, A); o++)
        if (prefix_last_tap(o, S, A) + 1 > m2) m2 = prefix_last_tap(o, S, A) + 1;
    return m2;
}

// What the decision reads of a marching instance on a device: MarchCfg's NT and LDS_BYTES and its strip width F::TWP_OUT, the
// resident workgroups per CU and the CU count (march_facts, lanczos_march.hpp)
struct MarchFacts {
    int nt, lds_bytes, strip_out_px, wg_per_cu, cus;
};

// the fields of FrameGeom (lanczos_kernels_common.hpp) the predicates below read, under FrameGeom's names
struct UpGeom {
    uintptr_t in, out;
    unsigned long long in_frame_stride, out_frame_stride;   // resolved: never 0
    int in_pitch, out_pitch, in_rows, out_rows, frames;
};

bool fast_supports(const lanczos_desc& d, const UpGeom& g);    // an instance of LZ_FAST_CONFIGS serves the call
bool rat_supports(const lanczos_desc& d, const UpGeom& g);     // k_rat / k_ratp serve it
bool march_supports(const UpGeom& g);                          // k_march serves it (else the tile kernel k_fast)
bool prefix_reg_supports(const lanczos_desc& d, const PrefixInfo& pi);   // an instance of LZ_PREFIX_REG_CONFIGS with this prefix

// the rows of a call: the whole frame (out_rows == 0) or the strip, and the input rows [in_row0, in_row0 + in_rows) it reads
struct UpStrip {
    int row0, rows, in_row0, in_rows;
};
void strip_input_rows(const int32_t* v_first, int a, int in_h, int row0, int rows, const PrefixInfo& pi, int* in_row0, int* in_rows);
UpStrip up_strip(const lanczos_desc& d, const int32_t* v_first, const PrefixInfo& pi);

struct UpQuery {
    const lanczos_desc* d = nullptr;
    int frames = 0;
    size_t in_frame_stride = 0, out_frame_stride = 0;   // as given: 0 = back to back
    uintptr_t in = 0, out = 0;                          // the base pointers (their low bits decide)
    int force = LANCZOS_KERNEL_NONE;                    // lanczos_force_kernel
    bool fast_ok = false, rat_ok = false, ratp_ok = false;   // the plan's: fast_prepare, rat_prepare, ratp_prepare succeeded
    PrefixInfo prefix;                                  // the plan's (all 0 in LANCZOS_MODE_HLS)
    const int32_t* v_first = nullptr;                   // the plan's vertical first[out_h]
    bool tile_kernel = false, separate_prefix = false, no_ratp = false;   // lanczos_env.hpp
    const MarchFacts* facts = nullptr;                  // NULL: the descriptor has no marching instance
};

struct UpLaunch {
    int frames, prefix;   // LANCZOS_ROUTE_PREFIX_* of this launch
};

struct UpRoute {
    int err = LANCZOS_OK;   // the refusal; nothing else is set when it is not LANCZOS_OK
    UpStrip strip{};
    size_t in_frame_stride = 0, out_frame_stride = 0;   // resolved
    int kernel = LANCZOS_KERNEL_NONE;                   // lanczos_last_kernel's family
    int main = LANCZOS_ROUTE_MAIN_NONE;                 // NONE: a strip that ends inside the prefix rows (k_march only)
    // The launches: one unless the batch is split; then n_launches - 1 of the preferred size (`body`) and the rest (`tail`), each
    // decided on its own frame count (the smaller last launch may ride where the full ones send their prefix rows in front).
    int n_launches = 0;
    UpLaunch body{}, tail{};
    UpLaunch launch(int i) const { return i + 1 < n_launches ? body : tail; }
    // behind / streamed: columns per block of k_prefix / k_prefix_stream, and k_prefix's dynamic LDS (0: streamed)
    int bw = 0;
    size_t prefix_lds = 0;
};

UpRoute up_route(const UpQuery& q);

}  // namespace lz
