// lanczos_resize_fused.hpp -- the resize kernels, written once for the three sample widths (lanczos_resize.hip describes the
// two paths):
//
//   RsSample<BPS>   what a sample width brings: its types, Pillow's multiply-add and store.  These are the specification of
//                   the bytes; everything below only moves samples around.
//   k_rs_pass_h/_v  the two-pass kernels, one thread per output sample (instantiated in lanczos_resize.hip).
//   k_rs_fused      the fused kernel, and rs_launch_fused, which fills its arguments and picks the instance.  The instances
//                   are those of LZ_RS_FUSED_INSTANCES (lanczos_resize.hpp), which also says which unit compiles them.
#pragma once
#include "lanczos_alpha.hpp"
#include "lanczos_resize.hpp"

#include <algorithm>
#include <type_traits>

namespace lz {

// ---- the sample policies ---------------------------------------------------------------------------------------------
//
// elem_t: a sample in memory; word_t: the unsigned type of its width; coeff_t / acc_t: a coefficient and a running sum;
// kAcc0: the sum before the first tap; SPD: samples per dword; kPassUnroll: the tap loop's unroll factor in the two-pass
// kernels; get(w, i): sample i of a dword; mad(sample, k, acc): one tap; store(acc): the sample Pillow stores, in the low
// bits of a word.
template <int BPS>
struct RsSample;

// 8-bit: acc = 2^21 + sum(sample * coeff) in int32 with 24-bit multiplies (|coeff| < 2^23 and 255 * sum|coeff| + 2^21 < 2^31,
// checked when a table is built), result clamp(acc >> 22, 0, 255).  Integer sums: tap order and zero-padded taps change nothing.
template <>
struct RsSample<1> {
    using elem_t = uint8_t;
    using word_t = uint8_t;
    using coeff_t = int32_t;
    using acc_t = int;
    static constexpr int BPS = 1, SPD = 4, kPassUnroll = 8;
    static constexpr int kAcc0 = 1 << (kResizePrecision - 1);
    static __device__ __forceinline__ int get(uint32_t w, int i) { return (int)((w >> (8 * i)) & 255u); }
    static __device__ __forceinline__ int mad(int sample, int coeff, int acc) { return __mul24(sample, coeff) + acc; }
    static __device__ __forceinline__ uint32_t store(int acc) { return (uint32_t)min(max(acc >> kResizePrecision, 0), 255); }
};

// 16-bit (Pillow's I;16) accumulates in double, tap by tap: ss = ss + (double)sample * k.  The bytes follow from three
// things.  (1) The multiply and the add round separately: every tap goes through mad, spelled with __dmul_rn / __dadd_rn,
// which the compiler never contracts (the build also passes -ffp-contract=off); the ISA of the wide-sample kernels holds no
// v_fma_f64.  (2) One chain per sample in ascending tap order: no tree, no split sums.  (3) A padded tap multiplies a finite
// sample by 0.0 and adds +0.0, which leaves the sum and its rounding as they were.  u16 -> f64 is exact.
template <>
struct RsSample<2> {
    using elem_t = uint16_t;
    using word_t = uint16_t;
    using coeff_t = double;
    using acc_t = double;
    static constexpr int BPS = 2, SPD = 2, kPassUnroll = 4;
    static constexpr double kAcc0 = 0.0;
    static __device__ __forceinline__ uint32_t get(uint32_t w, int i) { return (w >> (16 * i)) & 0xffffu; }
    static __device__ __forceinline__ double mad(uint32_t sample, double k, double ss) {
        return __dadd_rn(ss, __dmul_rn((double)sample, k));
    }
    // Pillow's ROUND_UP and its two CLIP8 stores: v < 0 stores 0, v > 65535 stores 0xFF00 | (v & 255) -- the low byte wraps
    static __device__ __forceinline__ uint32_t store(double ss) {
        const int v = (int)(ss < 0.0 ? __dadd_rn(ss, -0.5) : __dadd_rn(ss, 0.5));
        return v < 0 ? 0u : (uint32_t)(min(v >> 8, 255) << 8 | (v & 255));
    }
};

// float (Pillow's mode F) accumulates in double like 16-bit and stores (float)ss.  The bits follow from four things.  (1) and
// (2) as above.  (3) Exactly `count` taps are multiplied.  A float next to the window may be inf or NaN, and inf * 0.0 is
// NaN, so the 16-bit padding (a neighbouring sample times +0.0) is not harmless here: the unrolled horizontal loop of the fused
// kernel selects on tap < count -- never on the coefficient, since a zero weight inside Pillow's window is multiplied there
// too -- and every other loop runs to count.  Staged dwords beyond the frame read as 0 and are never multiplied either.
// (4) Denormals survive: samples travel as dwords, and float <-> double conversions and the double arithmetic run with the
// kernel mode's denormal bits set (FP_DENORM = 3 for both fields of the MODE register, the compiler's default: the build
// passes no flush flag).
template <>
struct RsSample<4> {
    using elem_t = float;
    using word_t = uint32_t;
    using coeff_t = double;
    using acc_t = double;
    static constexpr int BPS = 4, SPD = 1, kPassUnroll = 4;
    static constexpr double kAcc0 = 0.0;
    static __device__ __forceinline__ float get(uint32_t w, int) { return __uint_as_float(w); }
    static __device__ __forceinline__ double mad(float sample, double k, double ss) {
        return __dadd_rn(ss, __dmul_rn((double)sample, k));
    }
    static __device__ __forceinline__ uint32_t store(double ss) { return __float_as_uint(__double2float_rn(ss)); }
};

// ---- the element of a lanczos_tensor_norm request -----------------------------------------------------------------------
//
// cvt(((float)P / div - mean) / std) for one stored sample, in the words of `format` (LANCZOS_TENSOR_*; uniform over a launch).
// Three IEEE operations, each rounded on its own: the build passes -ffp-contract=off and no fast-math flag, so `/` is the
// correctly rounded division (v_div_scale / v_div_fmas / v_div_fixup) and nothing is folded, and the kernel mode keeps
// denormals.  bfloat16 is rounded on the bits as tensor_lut_convert16 rounds it; float16 by the conversion instruction, which is
// round to nearest even with subnormals kept and overflow to inf, as that function is.
__device__ __forceinline__ uint32_t rs_norm_elem(float v, float div, float mean, float std, int format) {
    const float e = ((v / div) - mean) / std;
    const uint32_t b = __float_as_uint(e);
    if (format == LANCZOS_TENSOR_F32) return b;
    if (format == LANCZOS_TENSOR_BF16) {
        if ((b & 0x7fffffffu) > 0x7f800000u) return (b >> 16) | 0x7fc0u;
        return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
    }
    const _Float16 h = (_Float16)e;
    return (uint32_t)__builtin_bit_cast(unsigned short, h);
}
// one of four launch arguments by a lane's channel
__device__ __forceinline__ float rs_norm_pick(const float (&p)[4], int c) { return c == 0 ? p[0] : c == 1 ? p[1] : c == 2 ? p[2] : p[3]; }
// the float a stored sample is: exact for 16 bits, the sample itself for a float
template <int BPS>
__device__ __forceinline__ float rs_norm_sample(uint32_t stored) {
    if constexpr (BPS == 4) return __uint_as_float(stored);
    else return (float)stored;
}

// ---- two-pass path ---------------------------------------------------------------------------------------------------

// one pass: `n_cols` samples per output row, `rows` output rows, frames in blockIdx.z
template <class KT>
struct RsPass {
    const uint8_t* src;
    uint8_t* dst;
    unsigned long long src_fs, dst_fs;         // frame strides (bytes)
    unsigned long long src_pitch, dst_pitch;   // row pitches (samples)
    int n_cols, channels;
    const int32_t *first, *count;
    const KT* coeffs;
    int ksize;
};

// horizontal: output sample x = o * C + c of row blockIdx.y
template <class S>
__global__ __launch_bounds__(kRsThreads) void k_rs_pass_h(RsPass<typename S::coeff_t> p) {
    const int x = blockIdx.x * kRsThreads + threadIdx.x;
    if (x >= p.n_cols) return;
    const int o = x / p.channels, c = x - o * p.channels;
    const typename S::elem_t* src = (const typename S::elem_t*)(p.src + blockIdx.z * p.src_fs) + blockIdx.y * p.src_pitch + c;
    const int f = p.first[o], n = p.count[o];
    const typename S::coeff_t* k = p.coeffs + (size_t)o * p.ksize;
    typename S::acc_t acc = S::kAcc0;
#pragma unroll S::kPassUnroll
    for (int i = 0; i < n; i++) acc = S::mad(src[(size_t)(f + i) * p.channels], k[i], acc);
    ((typename S::word_t*)(p.dst + blockIdx.z * p.dst_fs))[blockIdx.y * p.dst_pitch + x] = (typename S::word_t)S::store(acc);
}

// vertical: output row o = blockIdx.y, sample column x (coefficients uniform over the workgroup)
template <class S>
__global__ __launch_bounds__(kRsThreads) void k_rs_pass_v(RsPass<typename S::coeff_t> p) {
    const int x = blockIdx.x * kRsThreads + threadIdx.x;
    if (x >= p.n_cols) return;
    const int o = blockIdx.y;
    const int f = p.first[o], n = p.count[o];
    const typename S::coeff_t* k = p.coeffs + (size_t)o * p.ksize;
    const typename S::elem_t* src = (const typename S::elem_t*)(p.src + blockIdx.z * p.src_fs) + (size_t)f * p.src_pitch + x;
    typename S::acc_t acc = S::kAcc0;
#pragma unroll S::kPassUnroll
    for (int i = 0; i < n; i++) acc = S::mad(src[(size_t)i * p.src_pitch], k[i], acc);
    ((typename S::word_t*)(p.dst + blockIdx.z * p.dst_fs))[o * p.dst_pitch + x] = (typename S::word_t)S::store(acc);
}

// ---- fused path ------------------------------------------------------------------------------------------------------

template <class KT>
struct RsFused {
    const uint8_t* in;
    uint8_t* out;
    unsigned long long in_fs, out_fs;
    int in_pitch, out_pitch, in_h, out_w, out_h;   // pitches in bytes
    const int32_t *hf, *hc;
    const KT* hk;
    int hks;
    const int32_t *vf, *vc;
    const KT* vk;
    int vks;
    int strips, rows_per_chunk;   // grid.x = strips * chunks, grid.y = frames
    int ring_rows, stage_rows, stage_dw;
};
// tensor instances: `out` / `out_fs` of RsFused are the element frames and their stride in bytes
struct RsFusedTensor : RsFused<int32_t> {
    const uint32_t* lut;     // [C][256] words of EB bytes each, read when the kernel runs
    int cs, rs, ps;          // channel, row and pixel strides in elements
    unsigned extent_bytes;   // of one element frame, below 2^31
};
// ... + kRsMapped: lut is [out_channels][256], indexed by the output channel.  A struct of its own: with these fields behind
// RsFusedTensor's the argument loads of the instances without a map were merged otherwise, and their registers moved
struct RsFusedTensorMap : RsFusedTensor {
    unsigned dst;            // byte c: the output channel of source channel c, 255 where it is dropped
    int flip;                // bit 0: mirror x, bit 1: mirror y
    const uint8_t* d_flip;   // NULL, or one byte per frame of the launch, XORed with flip; read when the kernel runs
};
// ... + kRsCrops: the tables are those of the full axes and every frame has a window origin of its own.  Again a struct of its
// own, for the reason above
struct RsFusedTensorCrops : RsFusedTensorMap {
    const int32_t* d_origin;   // a pair (x0, y0) per frame of the launch, in output pixels of the full request; read when the
                               // kernel runs and clamped to [0, max_x0] x [0, max_y0]
    int max_x0, max_y0;        // the full output's size less the window's
};
// kRsNorm (wide samples into computed elements, lanczos_tensor_norm): `out` / `out_fs` are the element frames; always mapped
template <class KT>
struct RsFusedNorm : RsFused<KT> {
    int cs, rs, ps;          // channel, row and pixel strides in elements
    unsigned extent_bytes;   // of one element frame, below 2^31
    unsigned dst;            // byte c: the output channel of source channel c, 255 where it is dropped
    int flip;                // bit 0: mirror x, bit 1: mirror y
    const uint8_t* d_flip;   // NULL, or one byte per frame of the launch, XORed with flip; read when the kernel runs
    int format;              // LANCZOS_TENSOR_F32 / _BF16 / _F16
    float div[4], mean[4], std[4];   // by SOURCE channel: those of the output channel it goes to
};
// ... + kRsPlanar: the source is planar.  in_pitch is then the pitch of a plane row; behind the fields of the instance without it
template <class Base>
struct RsFusedPlanar : Base {
    int chan_stride;      // bytes between the planes of a frame
    unsigned src_bytes;   // from the frame's first byte to the last one the layout names, below 2^31
};
// ... + kRsPlanarOut: the destination is planar (RsDest::planar).  out_pitch is then the pitch of a plane row; behind the fields of
// the instance without it, for the reason RsFusedTensorMap gives
template <class Base>
struct RsFusedPlanarOut : Base {
    int out_chan_stride;   // bytes between the planes of a frame
    unsigned dst_bytes;    // from the frame's first byte to the last one the layout names + 1, below 2^31
};
// the argument of k_rs_fused<..., FLAGS> for coefficients KT
template <int FLAGS, class KT>
using RsFusedArgsPacked = std::conditional_t<
    (FLAGS & kRsNorm) != 0, RsFusedNorm<KT>,
    std::conditional_t<
    (FLAGS & kRsCrops) != 0, RsFusedTensorCrops,
    std::conditional_t<(FLAGS & kRsMapped) != 0, RsFusedTensorMap, std::conditional_t<FLAGS != 0, RsFusedTensor, RsFused<KT>>>>>;
template <int FLAGS, class KT>
using RsFusedArgsIn = std::conditional_t<(FLAGS & kRsPlanar) != 0, RsFusedPlanar<RsFusedArgsPacked<(FLAGS & ~kRsPlanar), KT>>,
                                         RsFusedArgsPacked<(FLAGS & ~kRsRowShift), KT>>;
template <int FLAGS, class KT>
using RsFusedArgs = std::conditional_t<(FLAGS & kRsPlanarOut) != 0, RsFusedPlanarOut<RsFusedArgsIn<(FLAGS & ~kRsPlanarOut), KT>>,
                                       RsFusedArgsIn<FLAGS, KT>>;

// The byte transpose of the planar staging and of k_rs_pack_source: p[c] holds bytes x .. x + 3 of plane c, o[] the C dwords of
// those four pixels interleaved.  v_perm_b32 picks byte sel[k] of the eight bytes {a : b} (b the low four) for result byte k
template <int C>
__device__ __forceinline__ void rs_interleave4(const uint32_t (&p)[C], uint32_t (&o)[C]) {
    static_assert(C == 3 || C == 4, "three or four planes");
    if constexpr (C == 4) {
        const uint32_t lo01 = __builtin_amdgcn_perm(p[1], p[0], 0x05010400u), hi01 = __builtin_amdgcn_perm(p[1], p[0], 0x07030602u);
        const uint32_t lo23 = __builtin_amdgcn_perm(p[3], p[2], 0x05010400u), hi23 = __builtin_amdgcn_perm(p[3], p[2], 0x07030602u);
        o[0] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u), o[1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
        o[2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u), o[3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
    } else {   // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
        o[0] = __builtin_amdgcn_perm(p[2], __builtin_amdgcn_perm(p[1], p[0], 0x010c0400u), 0x03040100u);
        o[1] = __builtin_amdgcn_perm(p[2], __builtin_amdgcn_perm(p[1], p[0], 0x06020c05u), 0x03020500u);
        o[2] = __builtin_amdgcn_perm(p[2], __builtin_amdgcn_perm(p[1], p[0], 0x0c07030cu), 0x07020106u);
    }
}
// the dword at any byte address, put together from the two aligned ones around it (k_rs_pack_source, k_rs_unpack_dest)
__device__ __forceinline__ uint32_t rs_load_dword_at(const uint8_t* p) {
    const unsigned sh = (unsigned)((uintptr_t)p & 3);
    const uint32_t* q = (const uint32_t*)(p - sh);
    const uint32_t lo = q[0];
    const uint32_t up = sh != 0 ? q[1] : 0u;
    return __builtin_amdgcn_alignbyte(up, lo, sh);
}
// One row segment of a destination: n bytes from `row` on, which starts at any byte.  A lane holds bytes 4 i .. 4 i + 3 of it in v
// (those below n; `have`: there is at least one); the lane LS below it holds group i - 1 and the lane LS above group i + 1, NL
// lanes of the wave taking part (LS = 1: neighbouring lanes; LS = C: the lanes of one plane where the planes alternate lane by
// lane).  Every lane of the wave calls.  Dwords are stored at dword-aligned addresses only and cover bytes of the segment only:
// where the segment starts r bytes into a dword, a lane stores the aligned dword that ends inside its group, put together from
// the previous group's upper r bytes and its own lower 4 - r (v_alignbyte).  What that leaves goes out as bytes: the lower bytes
// of the chain's first group, the upper r bytes of the chain's or the segment's last group, and a dword that would cross the
// segment's end.
template <int LS, int NL = 64>
__device__ __forceinline__ void rs_store_segment(uint8_t* row, unsigned i, unsigned n, uint32_t v, bool have) {
    const unsigned r = (unsigned)((uintptr_t)row & 3);
    const unsigned lane = threadIdx.x & 63;
    const uint32_t prev = (uint32_t)__shfl_up((int)v, LS, 64);
    if (!have) return;
    const unsigned p0 = 4 * i;
    if (r == 0) {
        if (p0 + 4 <= n) {
            *(uint32_t*)(row + p0) = v;
        } else {
            for (unsigned j = 0; p0 + j < n; j++) row[p0 + j] = (uint8_t)(v >> (8 * j));
        }
        return;
    }
    // bytes p0 - r .. p0 - r + 3 of the segment: byte j is the previous group's byte 4 - r + j for j < r, this group's j - r beyond
    const uint32_t m = __builtin_amdgcn_alignbyte(v, prev, 4 - r);
    uint8_t* const at = row + p0 - r;   // dword-aligned
    const bool first = lane < LS;       // no previous group in this wave: the lane that holds it stores those bytes itself, below
    if (!first && p0 + 4 <= n + r) {
        *(uint32_t*)at = m;
    } else {   // ... or a dword across the segment's end, cut there
        for (unsigned j = first ? r : 0u; j < 4; j++)
            if (p0 + j < n + r) at[j] = (uint8_t)(m >> (8 * j));
    }
    // this group's upper r bytes ride in the next group's dword; without a next group in this wave: bytes
    const bool next_has = lane + LS < NL && p0 + 4 < n;
    if (!next_has)
        for (unsigned j = 4 - r; j < 4; j++)
            if (p0 + j < n) row[p0 + j] = (uint8_t)(v >> (8 * j));
}
// the range of a planar frame's buffer resource: from its base rounded down to a dword to the last byte the layout names
template <bool PLANAR, class Args>
__device__ __forceinline__ unsigned rs_planar_range(const Args& g, int delta) {
    if constexpr (PLANAR) return ((unsigned)delta + g.src_bytes + 3u) & ~3u;
    else return 0u;
}
constexpr int kRsPlanarBatch = 4;   // groups of four pixels a thread of the planar staging has in flight: up to 2 C loads each

template <int C, int BPS>
struct RsStrip {
    static constexpr int SW = rs_strip_width(C, BPS);   // output pixels per strip
    static constexpr int RL = kRsThreads / SW;          // input rows per horizontal round
    static constexpr int RDW = SW * C * BPS / 4;        // ring row in dwords
    static constexpr int WPR = RDW / 64;                // waves per ring row in the vertical pass
};

// The march.  Input rows are staged in LDS as the dwords they come in; the horizontal pass turns them into rows of an LDS
// ring, stored as Pillow stores the intermediate; the vertical pass reads the ring, a lane owning one dword of the row (S::SPD
// samples).  A thread keeps one output column and its K coefficients in registers for the whole march (2 VGPRs per tap where
// they are doubles); the vertical coefficients are workgroup-uniform scalar loads.
//
// Float frames start on a dword and have dword pitches (checked by the caller), so a staged dword is a sample: there is no
// `delta`, no shift, and the window is read tap by tap with the select RsSample<4> asks for.
//
// ALPHA (LANCZOS_RESIZE_ALPHA, C == 4, 8-bit): the staging loads premultiply, once per staged pixel and not once per window
// that reads it, and the vertical pass divides alpha out where it packs its dword, which for four channels is one pixel.  For
// that the staged dwords are pixels: a frame base that is no dword multiple (every row then starts `delta` bytes into a
// dword, the row pitch being one) is shifted out while staging, and the horizontal pass reads its window unshifted.
//
// A table element (FLAGS & kRsElemMask; lanczos_tensor_out, 8-bit): the vertical pass stores lut[c][byte] as a float at c * cs + y * rs + x * ps of the float
// frame instead of the byte.  A lane holds four consecutive samples of the interleaved row, so a store of them as they lie would
// put 16 bytes between neighbouring lanes; the wave's 64 dwords are exchanged instead (four ds_bpermute) so that in round r
// lane i has sample 64 r + i of the wave's 256: neighbouring lanes store neighbouring samples, whole 256-byte runs where the
// layout is interleaved or has one channel, runs of every C-th lane per plane where it is planar.  The table is read from
// global memory through the vector cache (1 to 4 KiB, resident after the first rows): LDS and the plan stay the byte kernel's.
// Those bits are the width of the stored element in bytes: 4 (floats, lanczos_tensor_out), 2 (bfloat16 or float16 words,
// lanczos_tensor16_out: the table is of 16-bit words and the store a 16-bit one, everything else the same), 0: bytes out.
//
// + kRsMapped (lanczos_tensor_view with a channel map or flips; instances of their own, the ones above are as they
// were): the lane's channel c becomes dst[c], four byte fields of one scalar, and a channel no output names stores nothing.  A
// flip negates a stride and moves the base to the matching corner of the frame -- both computed once per workgroup from one
// uniform byte load -- so every offset stays inside [0, extent) and the buffer resource is the same.
//
// + kRsMapped + kRsCrops (lanczos_resize_crops; instances of their own again): out_w x out_h is the crop every frame
// stores and the tables are the full axes'.  A workgroup loads its frame's origin with two uniform loads, clamps it so that the
// crop lies inside the full output -- device memory cannot be validated, and the tables end there -- and moves its six table
// pointers by it: from there on it is the kernel of the window at that origin.  The plan is the largest over every origin
// (rs_fused_plan_crops), so staging rows and ring hold whichever the frame has.
//
// FLAGS = kRsNorm (lanczos_tensor_norm, 16-bit and float samples; instances of their own,
// the wide instances that store samples are as they were): only the epilogue differs.  After the vertical chain a lane holds
// SPD sums of consecutive samples of the strip's row; each is turned into the sample Pillow stores (S::store), then into the
// element by three float operations and a rounding (rs_norm_elem), and stored at oc * cs + y * rs + x * ps through the channel
// map and the flips, which every instance has (the identity view runs the identity map).  The element format is a launch
// argument, uniform over the wave, not a template parameter: one instance per (width, C, K) and a third of the build.
//
// FLAGS with kRsPlanar (a planar source, 8-bit, C = 3 or 4; instances of their own once more): only
// the staging loads differ.  A thread takes four pixels of a staged row: one dword from each of the C plane rows, transposed into
// C interleaved dwords (rs_interleave4) and written to LDS as dwords.  A plane row starts at any byte, another residue per plane
// and per row where the strides are odd, so each of those dwords is put together from the two aligned ones around it
// (v_alignbyte, the second loaded only where the residue is not 0).  The staged rows then hold interleaved pixels from the
// strip's first one on, premultiplied for ALPHA, and the horizontal pass reads its window unshifted, as it does for ALPHA.
// Loads go through a buffer resource over [frame base rounded down to a dword, last named byte rounded up to one): nothing
// outside it is read, and whatever lies in the padding of a row is only ever multiplied by a zero coefficient.
//
// FLAGS with kRsRowShift (ALPHA over interleaved rows whose pitch is no dword multiple; instances beside the planar ones): the
// ALPHA staging shifts every pixel by the residue of its own row instead of the frame's.
//
// FLAGS with kRsPlanarOut (a planar destination, bytes out, 8-bit, C = 3 or 4; instances of their own):
// only the epilogue differs.  The wave's 64 dwords are exchanged as the tensor epilogue exchanges them, so that in round r lane i
// has sample 64 r + i of the wave's 256, and every sample goes out as one byte store to c * chan_stride + y * row_stride + x of
// the frame: every C-th lane continues one plane row, and only bytes the layout names are ever stored.  The other form, one
// dword store per lane, is built by LZ_RS_PLANAR_OUT_DWORDS: the lane's dword is exchanged so that a lane holds four pixels of
// ONE plane (C = 4: within the quad; C = 3: the row goes out in four slots of 16 groups, 48 lanes each), and rs_store_segment
// stores it -- dwords at dword-aligned addresses only, realigned with the neighbouring group's dword where the plane row
// starts off one, bytes at the ends of the strip's segment.  It measured slower than the byte stores on every workload.
template <class S, int C, int K, bool ALPHA = false, int FLAGS = 0>
__global__ __launch_bounds__(kRsThreads) void k_rs_fused(
    RsFusedArgs<FLAGS, typename S::coeff_t> g) {
    constexpr int EB = FLAGS & kRsElemMask;         // bytes of a stored table element
    constexpr bool NORM = (FLAGS & kRsNorm) != 0;   // wide samples into computed elements: its own epilogue, nothing else differs
    static_assert(!NORM || (FLAGS == kRsNorm && S::BPS > 1), "norm: 16-bit or float samples, no other flag");
    constexpr bool PLANAR = (FLAGS & kRsPlanar) != 0;
    constexpr bool ROWSHIFT = (FLAGS & kRsRowShift) != 0;
    constexpr bool PLANAR_OUT = (FLAGS & kRsPlanarOut) != 0;
    static_assert(!PLANAR_OUT || (EB == 0 && S::BPS == 1 && C >= 3 && !ROWSHIFT && FLAGS < 2 * kRsPlanarOut),
                  "planar destinations: bytes out, 3 or 4 channels");
    // The planar epilogue has two forms: the tensor epilogue's exchange with a byte store per sample, and one dword store per
    // lane (C = 4: after a transpose within the quad; C = 3: the row walked in four slots of 16 groups of four pixels, 48 lanes,
    // instead of three waves, so that no group straddles a wave).  The byte form measured faster on every workload and is what
    // is built; the dword form stays for the A/B (DESIGN.md 4.5 has both numbers)
#ifdef LZ_RS_PLANAR_OUT_DWORDS
    constexpr bool kPlanarOutBytes = false;
#else
    constexpr bool kPlanarOutBytes = true;
#endif
    constexpr bool kSlots = PLANAR_OUT && C == 3 && !kPlanarOutBytes;
    static_assert(!ROWSHIFT || (ALPHA && !PLANAR && !(FLAGS & kRsCrops)), "a shift per row: the ALPHA staging of pitched rows");
    static_assert(!PLANAR || (S::BPS == 1 && C >= 3 && !(FLAGS & kRsCrops)), "planar sources: 8-bit, 3 or 4 channels, no crops");
    constexpr bool kPixelStage = ALPHA || PLANAR;         // a staged row starts at the strip's first pixel, whatever the address
    constexpr bool kNoShift = kPixelStage && C == 4;      // ... and a staged dword is a pixel: the horizontal pass shifts nothing
    constexpr bool MAPPED = (FLAGS & kRsMapped) != 0;
    constexpr bool CROPS = (FLAGS & kRsCrops) != 0;
    static_assert((EB == 0 && !MAPPED) || EB == 2 || EB == 4, "bytes, 16-bit elements or floats out");
    static_assert(!CROPS || MAPPED, "a crop origin per frame comes with the mapped epilogue");
    static_assert(!ALPHA || C == 4, "alpha is the fourth of four channels");
    static_assert((!ALPHA && !EB) || S::BPS == 1, "alpha and tensor output are 8-bit");
    using acc_t = typename S::acc_t;
    using word_t = typename S::word_t;
    using St = RsStrip<C, S::BPS>;
    constexpr int SW = St::SW, RL = St::RL, RDW = St::RDW, WPR = St::WPR;
    constexpr int BPS = S::BPS, SPD = S::SPD;
    constexpr int CB = C * BPS;                        // bytes per pixel
    constexpr int NE = (K * C + SPD - 1) / SPD;        // dwords of one horizontal window
    constexpr bool kDwordSamples = BPS == 4;           // a sample is a dword: nothing to align
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* ring = lds;                        // [ring_rows][RDW]
    uint32_t* stage = lds + g.ring_rows * RDW;   // [stage_rows][stage_dw]

    const int tid = threadIdx.x;
    if constexpr (CROPS) {   // the frame's origin, clamped: the tables from there on are the window's
        const int ox = __builtin_amdgcn_readfirstlane(g.d_origin[2 * blockIdx.y]);
        const int oy = __builtin_amdgcn_readfirstlane(g.d_origin[2 * blockIdx.y + 1]);
        const int cx = min(max(ox, 0), g.max_x0), cy = min(max(oy, 0), g.max_y0);
        g.hf += cx, g.hc += cx, g.hk += (size_t)cx * g.hks;
        g.vf += cy, g.vc += cy, g.vk += (size_t)cy * g.vks;
    }
    const int strip = blockIdx.x % g.strips, chunk = blockIdx.x / g.strips;
    const int x0 = strip * SW;
    const int sw = min(SW, g.out_w - x0);
    const int xs = g.hf[x0];   // first input pixel of the strip's span

    // horizontal: this thread's output column for the whole march, its coefficients in registers; nh taps are its window
    const int px = tid % SW, rl = tid / SW;
    typename S::coeff_t kh[K];
    int hoff, nh;   // the window's offset into the strip's span: bytes, dwords where a sample is one
    {
        const int p = x0 + min(px, sw - 1);
        nh = px < sw ? g.hc[p] : 0;
        hoff = (g.hf[p] - xs) * (kDwordSamples ? C : CB);
#pragma unroll
        for (int k = 0; k < K; k++) kh[k] = k < nh ? g.hk[(size_t)p * g.hks + k] : 0;
    }

    const uint8_t* fin = g.in + blockIdx.y * g.in_fs;
    // dword-aligned base and range: the bytes in front of the frame and behind its end that share a dword with it (same
    // page) are read but only ever multiplied by zero coefficients; everything further out reads as 0
    const int delta = kDwordSamples ? 0 : (int)((uintptr_t)fin & 3);
    const __amdgpu_buffer_rsrc_t irsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t*>(fin - delta), 0,
        PLANAR          ? rs_planar_range<PLANAR>(g, delta)
        : kDwordSamples ? (unsigned)(g.in_h * g.in_pitch) : (unsigned)((delta + g.in_h * g.in_pitch + 3) & ~3), 0x00020000);
    uint8_t* fout = g.out + blockIdx.y * g.out_fs;
    unsigned out_bytes = (unsigned)(g.out_h * g.out_pitch);
    if constexpr (EB != 0) out_bytes = g.extent_bytes;
    if constexpr (PLANAR_OUT) out_bytes = g.dst_bytes;
    if constexpr (NORM) out_bytes = g.extent_bytes;
    const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(fout, 0, out_bytes, 0x00020000);
    const bool out_aligned = (((uintptr_t)fout | (unsigned)g.out_pitch | (unsigned)(x0 * CB)) & 3) == 0;
    const int valid_bytes = sw * (kDwordSamples ? C : CB);   // of the strip's row; dwords where a sample is one
    // MAPPED: the frame's flips turned into a base and two signed strides (elements)
    [[maybe_unused]] int t_base = 0, t_rs = 0, t_ps = 0;
    if constexpr (MAPPED || NORM) {
        const int m = g.flip ^ (g.d_flip ? __builtin_amdgcn_readfirstlane((int)g.d_flip[blockIdx.y]) : 0);
        t_rs = (m & 2) ? -g.rs : g.rs, t_ps = (m & 1) ? -g.ps : g.ps;
        t_base = ((m & 2) ? (g.out_h - 1) * g.rs : 0) + ((m & 1) ? (g.out_w - 1) * g.ps : 0);
    }

    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int o_begin = chunk * g.rows_per_chunk;
    const int o_end = min(o_begin + g.rows_per_chunk, g.out_h);
    const float inv_sd = 1.0f / (float)g.stage_dw;
    int hi = g.vf[o_begin];   // next input row to produce
    for (int o0 = o_begin; o0 < o_end; o0 += kRsOB) {
        const int nob = min(kRsOB, o_end - o0);
        const int lo = g.vf[o0];
        const int need = g.vf[o0 + nob - 1] + g.vc[o0 + nob - 1];
        if (hi < lo) hi = lo;
        while (hi < need) {
            const int nr = min(g.stage_rows, need - hi);
            // kRsLoadBatch loads in flight per thread before the first LDS write (one HBM latency per batch, not per dword)
            const int total = nr * g.stage_dw;
            if constexpr (PLANAR) {
                // a unit is four pixels of a staged row, C dwords of it; ngr of them cover a row
                const int ngr = (g.stage_dw + C - 1) / C;
                const int units = nr * ngr;
                const float inv_ngr = 1.0f / (float)ngr;
                for (int u0 = tid; u0 < units; u0 += kRsPlanarBatch * kRsThreads) {
                    uint32_t pl[kRsPlanarBatch][C];
#pragma unroll
                    for (int b = 0; b < kRsPlanarBatch; b++) {
                        const int u = u0 + b * kRsThreads;
                        int r = (int)((float)u * inv_ngr);   // u / ngr, corrected below (u < 2^20)
                        r -= r * ngr > u;
                        r += (r + 1) * ngr <= u;
                        const int off0 = delta + (hi + r) * g.in_pitch + xs + 4 * (u - r * ngr);
#pragma unroll
                        for (int c = 0; c < C; c++) {
                            const int off = off0 + c * g.chan_stride;
#ifdef LZ_RS_PLANAR_BYTE_LOADS   // the A/B of the aligned loads: four byte loads per plane dword (DESIGN.md 4.5 has both numbers)
                            uint32_t bytes = 0u;
#pragma unroll
                            for (int k = 0; k < 4; k++)
                                bytes |= (u < units ? (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(irsrc, off + k, 0, 0) : 0u) << (8 * k);
                            pl[b][c] = bytes;
                            continue;
#endif
                            const unsigned sh = (unsigned)off & 3u;
                            const uint32_t lo = u < units ? __builtin_amdgcn_raw_buffer_load_b32(irsrc, off & ~3, 0, 0) : 0u;
                            const uint32_t up = sh != 0 && u < units ? __builtin_amdgcn_raw_buffer_load_b32(irsrc, (off & ~3) + 4, 0, 0) : 0u;
                            pl[b][c] = __builtin_amdgcn_alignbyte(up, lo, sh);
                        }
                    }
#pragma unroll
                    for (int b = 0; b < kRsPlanarBatch; b++) {
                        const int u = u0 + b * kRsThreads;
                        if (u < units) {
                            int r = (int)((float)u * inv_ngr);
                            r -= r * ngr > u;
                            r += (r + 1) * ngr <= u;
                            const int d0 = (u - r * ngr) * C;   // the unit's first dword of its row
                            uint32_t px[C];
                            rs_interleave4<C>(pl[b], px);
#pragma unroll
                            for (int c = 0; c < C; c++)
                                if (d0 + c < g.stage_dw) stage[r * g.stage_dw + d0 + c] = ALPHA ? rs_premul_px(px[c]) : px[c];
                        }
                    }
                }
            } else
            for (int u0 = tid; u0 < total; u0 += kRsLoadBatch * kRsThreads) {
                uint32_t v[kRsLoadBatch];
                uint32_t vn[ALPHA ? kRsLoadBatch : 1];   // ALPHA, delta != 0: the dword behind v[b], the rest of its pixel
                (void)vn;
                [[maybe_unused]] unsigned rsh[ROWSHIFT ? kRsLoadBatch : 1];   // ROWSHIFT: the residue of the load's row
#pragma unroll
                for (int b = 0; b < kRsLoadBatch; b++) {
                    const int u = u0 + b * kRsThreads;
                    int r = (int)((float)u * inv_sd);   // u / stage_dw, corrected below (u < 2^20)
                    r -= r * g.stage_dw > u;
                    r += (r + 1) * g.stage_dw <= u;
                    int at;
                    if constexpr (kDwordSamples) {
                        at = (hi + r) * g.in_pitch + 4 * (xs * C + u - r * g.stage_dw);
                    } else {
                        const int off = delta + (hi + r) * g.in_pitch + xs * CB;
                        at = (off & ~3) + 4 * (u - r * g.stage_dw);
                        if constexpr (ROWSHIFT) rsh[b] = (unsigned)off & 3u;
                    }
                    v[b] = u < total ? __builtin_amdgcn_raw_buffer_load_b32(irsrc, at, 0, 0) : 0u;
                    if constexpr (ROWSHIFT)
                        vn[b] = rsh[b] != 0 && u < total ? __builtin_amdgcn_raw_buffer_load_b32(irsrc, at + 4, 0, 0) : 0u;
                    else if constexpr (ALPHA)
                        vn[b] = delta != 0 && u < total ? __builtin_amdgcn_raw_buffer_load_b32(irsrc, at + 4, 0, 0) : 0u;
                }
#pragma unroll
                for (int b = 0; b < kRsLoadBatch; b++)
                    if (u0 + b * kRsThreads < total) {
                        if constexpr (ROWSHIFT)
                            stage[u0 + b * kRsThreads] = rs_premul_px(__builtin_amdgcn_alignbyte(vn[b], v[b], rsh[b]));
                        else if constexpr (ALPHA)
                            stage[u0 + b * kRsThreads] = rs_premul_px(__builtin_amdgcn_alignbyte(vn[b], v[b], (unsigned)delta));
                        else
                            stage[u0 + b * kRsThreads] = v[b];
                    }
            }
            __syncthreads();
            for (int j = rl; j < nr; j += RL) {
                acc_t acc[C];
#pragma unroll
                for (int c = 0; c < C; c++) acc[c] = S::kAcc0;
                if constexpr (kDwordSamples) {
                    const uint32_t* srow = stage + j * g.stage_dw + hoff;
#pragma unroll
                    for (int k = 0; k < K; k++) {
#pragma unroll
                        for (int c = 0; c < C; c++) {
                            const acc_t ss = S::mad(S::get(srow[k * C + c], 0), kh[k], acc[c]);
                            acc[c] = k < nh ? ss : acc[c];   // a select on the tap count: the sum of a tap past it is dropped
                        }
                    }
                } else {
                    const int pos = (kPixelStage ? 0 : (delta + (hi + j) * g.in_pitch + xs * CB) & 3) + hoff;
                    const uint32_t* srow = stage + j * g.stage_dw + (pos >> 2);
                    const unsigned sh = kNoShift ? 0u : pos & 3;   // ALPHA: the staged dwords are pixels
                    uint32_t dw[NE + 1];
#pragma unroll
                    for (int t = 0; t <= NE; t++) dw[t] = !kNoShift || t < NE ? srow[t] : 0u;
#pragma unroll
                    for (int t = 0; t < NE; t++) {
                        const uint32_t e = __builtin_amdgcn_alignbyte(dw[t + 1], dw[t], sh);
#pragma unroll
                        for (int b = 0; b < SPD; b++) {
                            const int idx = t * SPD + b;   // sample of the window: tap idx / C of channel idx % C, ascending
                            if (idx < K * C) acc[idx % C] = S::mad(S::get(e, b), kh[idx / C], acc[idx % C]);
                        }
                    }
                }
                word_t* rrow = (word_t*)ring + ((hi + j) % g.ring_rows) * (RDW * SPD) + px * C;
#pragma unroll
                for (int c = 0; c < C; c++) rrow[c] = (word_t)S::store(acc[c]);
            }
            __syncthreads();
            hi += nr;
        }
        // vertical: one output row per wave (WPR waves per row), coefficients uniform, SPD samples per lane
        constexpr int VPR = kSlots ? 4 : WPR;   // wave iterations per output row
        for (int q = wave; q < nob * VPR; q += kRsThreads / 64) {
            const int r = q / VPR;
            const int o = o0 + r;
            int dcol;
            if constexpr (kSlots) dcol = (q - r * VPR) * 48 + min(lane, 47);   // lanes 48 .. 63 idle along with lane 47
            else dcol = (q - r * WPR) * 64 + lane;
            const int f = g.vf[o], n = g.vc[o];
            const typename S::coeff_t* kv = g.vk + (size_t)o * g.vks;
            int slot = f % g.ring_rows;
            // SPD of the four sums are used.  Named sums and the packing below written out per width, not an array and
            // loops over it: from those the compiler orders the sums' registers otherwise, and for 8-bit it then packs with
            // the v_ashr_pk_u8_i32 that the table-element branch speaks of.  With the array, and the 8-bit pack kept from that
            // instruction by hand, every instance had the same registers and occupancy but another schedule, and the 4K
            // workloads measured 0.25 to 0.5 % slower (8-bit and float, three channels, halving and doubling)
            [[maybe_unused]] acc_t a0 = S::kAcc0, a1 = a0, a2 = a0, a3 = a0;
#pragma unroll 4
            for (int i = 0; i < n; i++) {
                const typename S::coeff_t k = kv[i];
                const uint32_t w = ring[slot * RDW + dcol];
                a0 = S::mad(S::get(w, 0), k, a0);
                if constexpr (SPD > 1) a1 = S::mad(S::get(w, 1), k, a1);
                if constexpr (SPD > 2) a2 = S::mad(S::get(w, 2), k, a2), a3 = S::mad(S::get(w, 3), k, a3);
                if (++slot == g.ring_rows) slot = 0;
            }
            const int b0 = kDwordSamples ? dcol : dcol * 4;   // the lane's place in the strip's row, as valid_bytes counts
            if constexpr (NORM) {
                // the lane's SPD sums are consecutive samples of the strip's row: each becomes the sample Pillow stores, then the
                // element, and goes out on its own -- no exchange, a lane already holds whole samples
#pragma unroll
                for (int s = 0; s < SPD; s++) {
                    const int j = dcol * SPD + s;
                    if (j < sw * C) {
                        const int xo = j / C, c = j - xo * C;
                        const int oc = (int)((g.dst >> (8 * c)) & 255u);
                        if (oc < 4) {
                            const float v = rs_norm_sample<BPS>(S::store(s == 0 ? a0 : a1));
                            const uint32_t e = rs_norm_elem(v, rs_norm_pick(g.div, c), rs_norm_pick(g.mean, c), rs_norm_pick(g.std, c), g.format);
                            const int to = t_base + oc * g.cs + o * t_rs + (x0 + xo) * t_ps;
                            if (g.format == LANCZOS_TENSOR_F32) __builtin_amdgcn_raw_buffer_store_b32(e, orsrc, to * 4, 0, 0);
                            else __builtin_amdgcn_raw_buffer_store_b16((uint16_t)e, orsrc, to * 2, 0, 0);
                        }
                    }
                }
            } else if constexpr (EB != 0) {
                // the dword is put together with v_perm_b32, not with shifts: followed by the exchange below, the shifted form
                // is compiled to v_ashr_pk_u8_i32, whose 16-bit result leaves the upper half of its register as it was while
                // the code behind it takes that half for zero (seen on the device: bytes 2 and 3 with bits of a0 in them)
                uint32_t packed = __builtin_amdgcn_perm(S::store(a1), S::store(a0), 0x0c0c0400u) |
                                  __builtin_amdgcn_perm(S::store(a3), S::store(a2), 0x04000c0cu);
                if constexpr (ALPHA) packed = rs_unpremul_px(packed);
                const int wb = b0 - lane * 4;   // the wave's first sample of the strip's row
#pragma unroll
                for (int rr = 0; rr < 4; rr++) {
                    const uint32_t w = (uint32_t)__shfl((int)packed, 16 * rr + (lane >> 2), 64);
                    const int j = wb + 64 * rr + lane;
                    if (j < valid_bytes) {
                        const int xo = j / C, c = j - xo * C;
                        if constexpr (MAPPED) {
                            const int oc = (int)((g.dst >> (8 * c)) & 255u);
                            if (oc < 4) {
                                const int at = oc * 256 + (int)((w >> (8 * (lane & 3))) & 255u);
                                const int to = t_base + oc * g.cs + o * t_rs + (x0 + xo) * t_ps;
                                if constexpr (EB == 2)
                                    __builtin_amdgcn_raw_buffer_store_b16(((const uint16_t*)g.lut)[at], orsrc, to * 2, 0, 0);
                                else
                                    __builtin_amdgcn_raw_buffer_store_b32(g.lut[at], orsrc, to * 4, 0, 0);
                            }
                        } else {
                            const int at = c * 256 + (int)((w >> (8 * (lane & 3))) & 255u);
                            const int to = c * g.cs + o * g.rs + (x0 + xo) * g.ps;
                            if constexpr (EB == 2)
                                __builtin_amdgcn_raw_buffer_store_b16(((const uint16_t*)g.lut)[at], orsrc, to * 2, 0, 0);
                            else
                                __builtin_amdgcn_raw_buffer_store_b32(g.lut[at], orsrc, to * 4, 0, 0);
                        }
                    }
                }
            } else if constexpr (PLANAR_OUT) {
                // (packed with v_perm_b32 for the reason above: an exchange follows)
                uint32_t packed = __builtin_amdgcn_perm(S::store(a1), S::store(a0), 0x0c0c0400u) |
                                  __builtin_amdgcn_perm(S::store(a3), S::store(a2), 0x04000c0cu);
                if constexpr (ALPHA) packed = rs_unpremul_px(packed);
                if constexpr (kPlanarOutBytes) {
                    const int wb = b0 - lane * 4;   // the wave's first sample of the strip's row
#pragma unroll
                    for (int rr = 0; rr < 4; rr++) {
                        const uint32_t w = (uint32_t)__shfl((int)packed, 16 * rr + (lane >> 2), 64);
                        const int j = wb + 64 * rr + lane;
                        if (j < valid_bytes) {
                            const int xo = j / C, c = j - xo * C;
                            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(w >> (8 * (lane & 3))), orsrc,
                                                                 c * g.out_chan_stride + o * g.out_pitch + x0 + xo, 0, 0);
                        }
                    }
                } else if constexpr (C == 4) {
                    // a lane is a pixel: the quad transposes its 4 x 4 bytes, and lane 4 i + c has plane c of pixels 4 i .. 4 i + 3
                    const int c = lane & 3;
                    uint32_t pl = 0u;
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        pl |= (((uint32_t)__shfl((int)packed, (lane & ~3) + k, 64) >> (8 * c)) & 255u) << (8 * k);
                    uint8_t* const row = fout + (size_t)c * (size_t)g.out_chan_stride + (size_t)o * (size_t)g.out_pitch + x0;
                    rs_store_segment<4>(row, (unsigned)(lane >> 2), (unsigned)sw, pl, (lane & ~3) < sw);
                } else {
                    // three lanes are four pixels (R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3): lane 3 j + c gets plane c of them
                    const int l = min(lane, 47), j3 = l / 3, c = l - 3 * j3;
                    const uint32_t d0 = (uint32_t)__shfl((int)packed, 3 * j3, 64), d1 = (uint32_t)__shfl((int)packed, 3 * j3 + 1, 64),
                                   d2 = (uint32_t)__shfl((int)packed, 3 * j3 + 2, 64);
                    const int f0 = 8 * c, f1 = 8 * ((c + 3) & 3), f2 = 8 * ((c + 2) & 3), f3 = 8 * ((c + 1) & 3);
                    // sample c of pixel k is byte 3 k + c of the twelve: pixel 0 in d0; pixel 1 in d0 (c = 0) or d1; pixel 2 in d1
                    // (c < 2) or d2; pixel 3 in d2
                    const uint32_t p1 = c == 0 ? d0 : d1, p2 = c < 2 ? d1 : d2;
                    const uint32_t pl = ((d0 >> f0) & 255u) | (((p1 >> f1) & 255u) << 8) | (((p2 >> f2) & 255u) << 16) |
                                        (((d2 >> f3) & 255u) << 24);
                    const unsigned grp = (unsigned)((q - r * VPR) * 16 + j3);   // the group of four pixels in the strip
                    uint8_t* const row = fout + (size_t)c * (size_t)g.out_chan_stride + (size_t)o * (size_t)g.out_pitch + x0;
                    rs_store_segment<3, 48>(row, grp, (unsigned)sw, pl, lane < 48 && (int)(4 * grp) < sw);
                }
            } else if (b0 < valid_bytes) {
                const int row_off = o * g.out_pitch + (kDwordSamples ? 4 * (x0 * C + dcol) : x0 * CB + b0);
                uint32_t packed;   // the dword of the lane's stored samples
                if constexpr (SPD == 4) packed = S::store(a0) | (S::store(a1) << 8) | (S::store(a2) << 16) | (S::store(a3) << 24);
                else if constexpr (SPD == 2) packed = S::store(a0) | (S::store(a1) << 16);
                else packed = S::store(a0);
                if constexpr (ALPHA) packed = rs_unpremul_px(packed);
                if (kDwordSamples || (out_aligned && b0 + 4 <= valid_bytes)) {
                    __builtin_amdgcn_raw_buffer_store_b32(packed, orsrc, row_off, 0, 0);
                } else if constexpr (BPS == 1) {
                    for (int b = 0; b < 4 && b0 + b < valid_bytes; b++)
                        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(packed >> (8 * b)), orsrc, row_off + b, 0, 0);
                } else if constexpr (BPS == 2) {
                    __builtin_amdgcn_raw_buffer_store_b16((uint16_t)S::store(a0), orsrc, row_off, 0, 0);
                    if (b0 + 2 < valid_bytes) __builtin_amdgcn_raw_buffer_store_b16((uint16_t)S::store(a1), orsrc, row_off + 2, 0, 0);
                }
            }
        }
    }
}

// f(C, K, ALPHA) as std::integral_constants for the instance of a request; false: there is none
template <class F>
bool rs_dispatch_instance(int channels, int K, bool alpha, F&& f) {
    auto with_k = [&](auto kb) {
        if (channels == 1) f(std::integral_constant<int, 1>(), kb, std::false_type());
        else if (channels == 3) f(std::integral_constant<int, 3>(), kb, std::false_type());
        else if (alpha) f(std::integral_constant<int, 4>(), kb, std::true_type());
        else f(std::integral_constant<int, 4>(), kb, std::false_type());
    };
#define X(KB)                                          \
    if (K == KB) {                                     \
        with_k(std::integral_constant<int, KB>());     \
        return true;                                   \
    }
    LZ_RS_BUCKETS(X)
#undef X
    return false;
}

// the launch arguments of a request, all but the frame pointers
template <class KT>
void rs_fill_fused(RsFused<KT>* g, const RsFusedLaunch& c) {
    const lanczos_resize_desc* d = c.d;
    const RsWindow& w = c.win;   // the kernel's output is the window: its tables start at the window's first outputs
    g->in_pitch = c.src ? (int)c.src->row_stride : d->in_w * d->channels * resize_bps(d);   // below 2^31 (the plan)
    g->out_pitch = c.dst ? (int)c.dst->row_stride : w.w * d->channels * resize_bps(d);   // below 2^31 (rs_route)
    g->in_h = d->in_h, g->out_w = w.w, g->out_h = w.h;
    g->in_fs = c.in_fs, g->out_fs = c.out_fs;
    g->hks = c.H->host.ksize, g->vks = c.V->host.ksize;
    g->hf = c.H->first() + w.x0, g->hc = c.H->count() + w.x0, g->hk = c.H->coeffs<KT>() + (size_t)w.x0 * g->hks;
    g->vf = c.V->first() + w.y0, g->vc = c.V->count() + w.y0, g->vk = c.V->coeffs<KT>() + (size_t)w.y0 * g->vks;
    g->strips = c.fp->strips, g->rows_per_chunk = c.fp->rows_per_chunk;
    g->ring_rows = c.fp->ring_rows, g->stage_rows = c.fp->stage_rows, g->stage_dw = c.fp->stage_dw;
}

template <int BPS, int FLAGS>
hipError_t rs_launch_fused(const RsFusedLaunch& c) {
    using S = RsSample<BPS>;
    const bool alpha = (c.d->reserved[0] & LANCZOS_RESIZE_ALPHA) != 0;
    const RsFusedPlan& fp = *c.fp;
    constexpr bool PLANAR = (FLAGS & kRsPlanar) != 0;
    RsFusedArgs<FLAGS, typename S::coeff_t> g{};
    rs_fill_fused(&g, c);
    constexpr bool ROWSHIFT = (FLAGS & kRsRowShift) != 0;
    constexpr bool PLANAR_OUT = (FLAGS & kRsPlanarOut) != 0;
    if ((c.src && c.src->planar) != PLANAR) return hipErrorInvalidValue;
    if ((c.dst && c.dst->planar) != PLANAR_OUT) return hipErrorInvalidValue;
    if constexpr (PLANAR_OUT) g.out_chan_stride = (int)c.dst->chan_stride, g.dst_bytes = (unsigned)c.dst->named;
    if constexpr (PLANAR) {
        g.chan_stride = (int)c.src->chan_stride;
        g.src_bytes = (unsigned)((c.d->channels - 1) * c.src->chan_stride + (c.d->in_h - 1) * c.src->row_stride + c.d->in_w);
    }
    constexpr bool NORM = (FLAGS & kRsNorm) != 0;
    if constexpr (NORM) {
        const RsTensorOut& t = c.tc->t;
        g.cs = (int)t.chan_stride, g.rs = (int)t.row_stride, g.ps = (int)t.pix_stride;   // extent below 2^31 bytes
        g.extent_bytes = (unsigned)c.tc->extent_bytes;
        g.dst = t.dst_of_src(), g.flip = t.flip & 3, g.format = t.format;
        for (int oc = 0; oc < t.out_channels; oc++) {
            const int sc = t.src_channel[oc];
            g.div[sc] = t.div[oc], g.mean[sc] = t.mean[oc], g.std[sc] = t.std[oc];
        }
    }
    if constexpr ((FLAGS & kRsElemMask) != 0) {
        g.lut = (const uint32_t*)c.tc->t.d_lut;
        g.cs = (int)c.tc->t.chan_stride, g.rs = (int)c.tc->t.row_stride, g.ps = (int)c.tc->t.pix_stride;   // extent below 2^31 bytes
        g.extent_bytes = (unsigned)c.tc->extent_bytes;
    }
    if constexpr ((FLAGS & kRsMapped) != 0) g.dst = c.tc->t.dst_of_src(), g.flip = c.tc->t.flip & 3;
    if constexpr ((FLAGS & kRsCrops) != 0) g.max_x0 = c.d->out_w - c.win.w, g.max_y0 = c.d->out_h - c.win.h;
    void (*kern)(decltype(g)) = nullptr;
    rs_dispatch_instance(c.d->channels, fp.K, alpha, [&](auto ch, auto k, auto a) {
        // alpha is 8-bit only (resize_validate); a planar source of one channel is the interleaved one
        if constexpr ((!decltype(a)::value || BPS == 1) && (!(PLANAR || PLANAR_OUT) || decltype(ch)::value >= 3) &&
                      (!ROWSHIFT || decltype(a)::value))
            kern = k_rs_fused<S, decltype(ch)::value, decltype(k)::value, decltype(a)::value, FLAGS>;
    });
    if (!kern) return c.frames > 0 ? hipErrorInvalidValue : hipSuccess;   // no frame, no launch to miss
    return rs_for_frame_groups(c.is, c.frames, [&](int f0, int nf) {
        g.in = c.in + (size_t)f0 * c.in_fs;
        g.out = c.out + (size_t)f0 * c.out_fs;
        if constexpr ((FLAGS & kRsMapped) != 0 || NORM) g.d_flip = c.tc->t.d_flip ? c.tc->t.d_flip + f0 : nullptr;   // a byte per frame
        if constexpr ((FLAGS & kRsCrops) != 0) g.d_origin = c.tc->d_origin + 2 * (size_t)f0;                  // a pair per frame
        hipLaunchKernelGGL(kern, dim3(fp.strips * fp.chunks, nf), dim3(kRsThreads), fp.lds, c.is.stream, g);
    });
}
// each is instantiated, with its kernels, by lanczos_resize_fused_inst.hip
#define X(I, BPS, FLAGS) extern template hipError_t rs_launch_fused<BPS, FLAGS>(const RsFusedLaunch&);
LZ_RS_FUSED_INSTANCES(X)
#undef X

}  // namespace lz
