// lanczos_resize_fused.hpp -- k_rs_fused, the fused kernel of 8-bit resizes (lanczos_resize.hip describes the march), as a
// template two translation units instantiate: lanczos_resize.hip the instances that store bytes, lanczos_resize_tensor.hip
// those whose vertical pass stores floats through a table instead (TENSOR; include/lanczos_hip.h, lanczos_tensor_out).
#pragma once
#include "lanczos_alpha.hpp"
#include "lanczos_resize.hpp"

namespace lz {

__device__ __forceinline__ int rs_mad(int sample, int coeff, int acc) { return __mul24(sample, coeff) + acc; }
__device__ __forceinline__ uint32_t rs_clip8(int acc) { return (uint32_t)min(max(acc >> kResizePrecision, 0), 255); }

struct RsFused {
    const uint8_t* in;
    uint8_t* out;
    unsigned long long in_fs, out_fs;
    int in_pitch, out_pitch, in_h, out_w, out_h;
    const int32_t *hf, *hc, *hk;
    int hks;
    const int32_t *vf, *vc, *vk;
    int vks;
    int strips, rows_per_chunk;   // grid.x = strips * chunks, grid.y = frames
    int ring_rows, stage_rows, stage_dw;
};
// TENSOR instances: `out` / `out_fs` of RsFused are the float frames and their stride in bytes
struct RsFusedTensor : RsFused {
    const uint32_t* lut;     // [C][256] words, read when the kernel runs
    int cs, rs, ps;          // channel, row and pixel strides in floats
    unsigned extent_bytes;   // of one float frame, below 2^31
};
template <bool TENSOR>
struct RsFusedArg {
    using type = RsFused;
};
template <>
struct RsFusedArg<true> {
    using type = RsFusedTensor;
};

template <int C>
struct RsStrip {
    static constexpr int SW = rs_strip_width(C, 1);   // output pixels per strip
    static constexpr int RL = kRsThreads / SW;    // input rows per horizontal round
    static constexpr int RDW = SW * C / 4;        // ring row in dwords
    static constexpr int WPR = RDW / 64;          // waves per ring row in the vertical pass
};

// ALPHA (LANCZOS_RESIZE_ALPHA, C == 4): the staging loads premultiply, once per staged pixel and not once per window that
// reads it, and the vertical pass divides alpha out where it packs its dword, which for four channels is one pixel.  For
// that the staged dwords are pixels: a frame base that is no dword multiple (every row then starts `delta` bytes into a
// dword, the row pitch being one) is shifted out while staging, and the horizontal pass reads its window unshifted.
//
// TENSOR (lanczos_tensor_out): the vertical pass stores lut[c][byte] as a float at c * cs + y * rs + x * ps of the float frame
// instead of the byte.  A lane holds four consecutive samples of the interleaved row, so a store of them as they lie would
// put 16 bytes between neighbouring lanes; the wave's 64 dwords are exchanged instead (four ds_bpermute) so that in round r
// lane i has sample 64 r + i of the wave's 256: neighbouring lanes store neighbouring samples, whole 256-byte runs where the
// layout is interleaved or has one channel, runs of every C-th lane per plane where it is planar.  The table is read from
// global memory through the vector cache (1 to 4 KiB, resident after the first rows): LDS and the plan stay the byte kernel's.
template <int C, int K, bool ALPHA = false, bool TENSOR = false>
__global__ __launch_bounds__(kRsThreads) void k_rs_fused(typename RsFusedArg<TENSOR>::type g) {
    static_assert(!ALPHA || C == 4, "alpha is the fourth of four channels");
    using S = RsStrip<C>;
    constexpr int SW = S::SW, RL = S::RL, RDW = S::RDW, WPR = S::WPR;
    constexpr int NE = (K * C + 3) / 4;   // dwords of one horizontal window
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* ring = lds;                        // [ring_rows][RDW]
    uint32_t* stage = lds + g.ring_rows * RDW;   // [stage_rows][stage_dw]
    uint8_t* ring8 = (uint8_t*)ring;

    const int tid = threadIdx.x;
    const int strip = blockIdx.x % g.strips, chunk = blockIdx.x / g.strips;
    const int x0 = strip * SW;
    const int sw = min(SW, g.out_w - x0);
    const int xs = g.hf[x0];   // first input pixel of the strip's span

    // horizontal: this thread's output column for the whole march, its coefficients in registers
    const int px = tid % SW, rl = tid / SW;
    int kh[K];
    int hoffb;
    {
        const int p = x0 + min(px, sw - 1);
        const int n = px < sw ? g.hc[p] : 0;
        hoffb = (g.hf[p] - xs) * C;
#pragma unroll
        for (int k = 0; k < K; k++) kh[k] = k < n ? g.hk[(size_t)p * g.hks + k] : 0;
    }

    const uint8_t* fin = g.in + blockIdx.y * g.in_fs;
    // dword-aligned base and range: the bytes in front of the frame and behind its end that share a dword with it (same
    // page) are read but only ever multiplied by zero coefficients; everything further out reads as 0
    const int delta = (int)((uintptr_t)fin & 3);
    const __amdgpu_buffer_rsrc_t irsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t*>(fin - delta), 0, (unsigned)((delta + g.in_h * g.in_pitch + 3) & ~3), 0x00020000);
    uint8_t* fout = g.out + blockIdx.y * g.out_fs;
    unsigned out_bytes = (unsigned)(g.out_h * g.out_pitch);
    if constexpr (TENSOR) out_bytes = g.extent_bytes;
    const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(fout, 0, out_bytes, 0x00020000);
    const bool out_aligned = (((uintptr_t)fout | (unsigned)g.out_pitch | (unsigned)(x0 * C)) & 3) == 0;
    const int valid_bytes = sw * C;

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
            for (int u0 = tid; u0 < total; u0 += kRsLoadBatch * kRsThreads) {
                uint32_t v[kRsLoadBatch];
                uint32_t vn[ALPHA ? kRsLoadBatch : 1];   // ALPHA, delta != 0: the dword behind v[b], the rest of its pixel
                (void)vn;
#pragma unroll
                for (int b = 0; b < kRsLoadBatch; b++) {
                    const int u = u0 + b * kRsThreads;
                    int r = (int)((float)u * inv_sd);   // u / stage_dw, corrected below (u < 2^20)
                    r -= r * g.stage_dw > u;
                    r += (r + 1) * g.stage_dw <= u;
                    const int off = delta + (hi + r) * g.in_pitch + xs * C;
                    const int at = (off & ~3) + 4 * (u - r * g.stage_dw);
                    v[b] = u < total ? __builtin_amdgcn_raw_buffer_load_b32(irsrc, at, 0, 0) : 0u;
                    if constexpr (ALPHA)
                        vn[b] = delta != 0 && u < total ? __builtin_amdgcn_raw_buffer_load_b32(irsrc, at + 4, 0, 0) : 0u;
                }
#pragma unroll
                for (int b = 0; b < kRsLoadBatch; b++)
                    if (u0 + b * kRsThreads < total) {
                        if constexpr (ALPHA)
                            stage[u0 + b * kRsThreads] = rs_premul_px(__builtin_amdgcn_alignbyte(vn[b], v[b], (unsigned)delta));
                        else
                            stage[u0 + b * kRsThreads] = v[b];
                    }
            }
            __syncthreads();
            for (int j = rl; j < nr; j += RL) {
                const int pos = (ALPHA ? 0 : (delta + (hi + j) * g.in_pitch + xs * C) & 3) + hoffb;
                const uint32_t* srow = stage + j * g.stage_dw + (pos >> 2);
                const unsigned sh = ALPHA ? 0u : pos & 3;   // ALPHA: the staged dwords are pixels
                uint32_t dw[NE + 1];
#pragma unroll
                for (int t = 0; t <= NE; t++) dw[t] = !ALPHA || t < NE ? srow[t] : 0u;
                int acc[C];
#pragma unroll
                for (int c = 0; c < C; c++) acc[c] = 1 << (kResizePrecision - 1);
#pragma unroll
                for (int t = 0; t < NE; t++) {
                    const uint32_t e = __builtin_amdgcn_alignbyte(dw[t + 1], dw[t], sh);
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        const int idx = t * 4 + b;
                        if (idx < K * C) acc[idx % C] = rs_mad((int)((e >> (8 * b)) & 255u), kh[idx / C], acc[idx % C]);
                    }
                }
                uint8_t* rrow = ring8 + ((hi + j) % g.ring_rows) * (RDW * 4) + px * C;
#pragma unroll
                for (int c = 0; c < C; c++) rrow[c] = (uint8_t)rs_clip8(acc[c]);
            }
            __syncthreads();
            hi += nr;
        }
        // vertical: one output row per wave (WPR waves per row), coefficients uniform
        for (int q = wave; q < nob * WPR; q += kRsThreads / 64) {
            const int r = q / WPR;
            const int o = o0 + r;
            const int dcol = (q - r * WPR) * 64 + lane;
            const int f = g.vf[o], n = g.vc[o];
            const int32_t* kv = g.vk + (size_t)o * g.vks;
            int slot = f % g.ring_rows;
            int a0 = 1 << (kResizePrecision - 1), a1 = a0, a2 = a0, a3 = a0;
#pragma unroll 4
            for (int i = 0; i < n; i++) {
                const int k = kv[i];
                const uint32_t w = ring[slot * RDW + dcol];
                a0 = rs_mad((int)(w & 255u), k, a0);
                a1 = rs_mad((int)((w >> 8) & 255u), k, a1);
                a2 = rs_mad((int)((w >> 16) & 255u), k, a2);
                a3 = rs_mad((int)(w >> 24), k, a3);
                if (++slot == g.ring_rows) slot = 0;
            }
            const int b0 = dcol * 4;
            if constexpr (TENSOR) {
                // the dword is put together with v_perm_b32, not with shifts: followed by the exchange below, the shifted form
                // is compiled to v_ashr_pk_u8_i32, whose 16-bit result leaves the upper half of its register as it was while
                // the code behind it takes that half for zero (seen on the device: bytes 2 and 3 with bits of a0 in them)
                uint32_t packed = __builtin_amdgcn_perm(rs_clip8(a1), rs_clip8(a0), 0x0c0c0400u) |
                                  __builtin_amdgcn_perm(rs_clip8(a3), rs_clip8(a2), 0x04000c0cu);
                if constexpr (ALPHA) packed = rs_unpremul_px(packed);
                const int wb = b0 - lane * 4;   // the wave's first sample of the strip's row
#pragma unroll
                for (int rr = 0; rr < 4; rr++) {
                    const uint32_t w = (uint32_t)__shfl((int)packed, 16 * rr + (lane >> 2), 64);
                    const int j = wb + 64 * rr + lane;
                    if (j < valid_bytes) {
                        const int xo = j / C, c = j - xo * C;
                        const uint32_t v = g.lut[c * 256 + (int)((w >> (8 * (lane & 3))) & 255u)];
                        __builtin_amdgcn_raw_buffer_store_b32(v, orsrc, (c * g.cs + o * g.rs + (x0 + xo) * g.ps) * 4, 0, 0);
                    }
                }
            } else if (b0 < valid_bytes) {
                const int row_off = o * g.out_pitch + x0 * C + b0;
                uint32_t packed = rs_clip8(a0) | (rs_clip8(a1) << 8) | (rs_clip8(a2) << 16) | (rs_clip8(a3) << 24);
                if constexpr (ALPHA) packed = rs_unpremul_px(packed);
                if (out_aligned && b0 + 4 <= valid_bytes) {
                    __builtin_amdgcn_raw_buffer_store_b32(packed, orsrc, row_off, 0, 0);
                } else {
                    for (int b = 0; b < 4 && b0 + b < valid_bytes; b++)
                        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(packed >> (8 * b)), orsrc, row_off + b, 0, 0);
                }
            }
        }
    }
}

// horizontal tap counts with a fused instance (a request runs on the smallest one >= its ksize, zero-padded).  3 and 5 serve
// the upscales of the short filters (box and bilinear: ksize 3, bicubic: 5) and only them: a Lanczos request keeps the
// instance it always had (a = 2 upscales, ksize 5, run on 7).  LANCZOS_RS_NO_SMALL_BUCKETS=1 pads the short filters to 7 too
#define LZ_RS_BUCKETS(X) X(3) X(5) X(7) X(9) X(11) X(13) X(17) X(25)

}  // namespace lz
