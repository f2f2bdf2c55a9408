// lanczos_resize16.hip -- the kernels of LANCZOS_RESIZE_U16: 16-bit samples resized as Pillow resizes mode I;16
// (include/lanczos_hip.h).  Tables, cache, planning and dispatch are in lanczos_resize.hip; the two kernel
// paths mirror the 8-bit ones:
//
//   fused     k_rs16_fused: the march of k_rs_fused with 2-byte samples -- input rows staged in LDS as the dwords they
//             come in, horizontal pass into an LDS ring of u16 rows stored as Pillow stores them, vertical pass from the
//             ring.  A thread keeps one output column and its K double coefficients in registers (2 VGPRs per tap) for the
//             whole march; the vertical coefficients are workgroup-uniform scalar loads; a lane of the vertical pass owns a
//             dword of the row, two samples.
//   two-pass  k_rs16_h into the u16 intermediate in context scratch, k_rs16_v from it: any tap count, and the only kernel
//             when one axis keeps its size.
//
// Pillow accumulates in double, tap by tap: ss = ss + (double)sample * k.  The bytes follow from three things.  (1) The
// multiply and the add round separately: every tap goes through rs16_mad, spelled with __dmul_rn / __dadd_rn, which the
// compiler never contracts (the build also passes -ffp-contract=off); the ISA of this file holds no v_fma_f64.  (2) One
// chain per sample in ascending tap order: no tree, no split sums.  (3) A padded tap multiplies a finite sample by 0.0 and
// adds +0.0, which leaves the sum and its rounding as they were.  u16 -> f64 is exact.
#include "lanczos_resize.hpp"

#include "lanczos_env.hpp"

#include <algorithm>

namespace lz {

__device__ __forceinline__ double rs16_mad(uint32_t sample, double k, double ss) {
    return __dadd_rn(ss, __dmul_rn((double)sample, k));
}

// Pillow's ROUND_UP and its two CLIP8 stores: v < 0 stores 0, v > 65535 stores 0xFF00 | (v & 255) -- the low byte wraps
__device__ __forceinline__ uint32_t rs16_store(double ss) {
    const int v = (int)(ss < 0.0 ? __dadd_rn(ss, -0.5) : __dadd_rn(ss, 0.5));
    return v < 0 ? 0u : (uint32_t)(min(v >> 8, 255) << 8 | (v & 255));
}

// one pass of the two-pass path: `n_cols` samples per output row, frames in blockIdx.z; pitches in samples
struct Rs16Pass {
    const uint8_t* src;
    uint8_t* dst;
    unsigned long long src_fs, dst_fs;   // frame strides (bytes)
    unsigned long long src_pitch, dst_pitch;
    int n_cols, channels;
    const int32_t *first, *count;
    const double* coeffs;
    int ksize;
};

// horizontal: output sample x = o * C + c of row blockIdx.y
__global__ __launch_bounds__(kRsThreads) void k_rs16_h(Rs16Pass p) {
    const int x = blockIdx.x * kRsThreads + threadIdx.x;
    if (x >= p.n_cols) return;
    const int o = x / p.channels, c = x - o * p.channels;
    const uint16_t* src = (const uint16_t*)(p.src + blockIdx.z * p.src_fs) + blockIdx.y * p.src_pitch + c;
    const int f = p.first[o], n = p.count[o];
    const double* k = p.coeffs + (size_t)o * p.ksize;
    double ss = 0.0;
#pragma unroll 4
    for (int i = 0; i < n; i++) ss = rs16_mad(src[(size_t)(f + i) * p.channels], k[i], ss);
    ((uint16_t*)(p.dst + blockIdx.z * p.dst_fs))[blockIdx.y * p.dst_pitch + x] = (uint16_t)rs16_store(ss);
}

// vertical: output row o = blockIdx.y, sample column x (coefficients uniform over the workgroup)
__global__ __launch_bounds__(kRsThreads) void k_rs16_v(Rs16Pass p) {
    const int x = blockIdx.x * kRsThreads + threadIdx.x;
    if (x >= p.n_cols) return;
    const int o = blockIdx.y;
    const int f = p.first[o], n = p.count[o];
    const double* k = p.coeffs + (size_t)o * p.ksize;
    const uint16_t* src = (const uint16_t*)(p.src + blockIdx.z * p.src_fs) + (size_t)f * p.src_pitch + x;
    double ss = 0.0;
#pragma unroll 4
    for (int i = 0; i < n; i++) ss = rs16_mad(src[(size_t)i * p.src_pitch], k[i], ss);
    ((uint16_t*)(p.dst + blockIdx.z * p.dst_fs))[o * p.dst_pitch + x] = (uint16_t)rs16_store(ss);
}

struct Rs16Fused {
    const uint8_t* in;
    uint8_t* out;
    unsigned long long in_fs, out_fs;
    int in_pitch, out_pitch, in_h, out_w, out_h;   // pitches in bytes
    const int32_t *hf, *hc;
    const double* hk;
    int hks;
    const int32_t *vf, *vc;
    const double* vk;
    int vks;
    int strips, rows_per_chunk;   // grid.x = strips * chunks, grid.y = frames
    int ring_rows, stage_rows, stage_dw;
};

template <int C>
struct Rs16Strip {
    static constexpr int SW = rs_strip_width(C, 2);   // output pixels per strip
    static constexpr int RL = kRsThreads / SW;           // input rows per horizontal round
    static constexpr int RDW = SW * C / 2;               // ring row in dwords (two samples each)
    static constexpr int WPR = RDW / 64;                 // waves per ring row in the vertical pass
};

template <int C, int K>
__global__ __launch_bounds__(kRsThreads) void k_rs16_fused(Rs16Fused g) {
    using S = Rs16Strip<C>;
    constexpr int SW = S::SW, RL = S::RL, RDW = S::RDW, WPR = S::WPR;
    constexpr int NE = (K * C + 1) / 2;   // dwords of one horizontal window
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* ring = lds;                        // [ring_rows][RDW]
    uint32_t* stage = lds + g.ring_rows * RDW;   // [stage_rows][stage_dw]
    uint16_t* ring16 = (uint16_t*)ring;

    const int tid = threadIdx.x;
    const int strip = blockIdx.x % g.strips, chunk = blockIdx.x / g.strips;
    const int x0 = strip * SW;
    const int sw = min(SW, g.out_w - x0);
    const int xs = g.hf[x0];   // first input pixel of the strip's span

    // horizontal: this thread's output column for the whole march, its coefficients in registers
    const int px = tid % SW, rl = tid / SW;
    double kh[K];
    int hoffb;
    {
        const int p = x0 + min(px, sw - 1);
        const int n = px < sw ? g.hc[p] : 0;
        hoffb = (g.hf[p] - xs) * C * 2;
#pragma unroll
        for (int k = 0; k < K; k++) kh[k] = k < n ? g.hk[(size_t)p * g.hks + k] : 0.0;
    }

    const uint8_t* fin = g.in + blockIdx.y * g.in_fs;
    // dword-aligned base and range: a frame that starts two bytes into a dword shares it with the sample in front of it,
    // which is read (same page) but only ever multiplied by a zero coefficient; everything further out reads as 0
    const int delta = (int)((uintptr_t)fin & 3);
    const __amdgpu_buffer_rsrc_t irsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t*>(fin - delta), 0, (unsigned)((delta + g.in_h * g.in_pitch + 3) & ~3), 0x00020000);
    uint8_t* fout = g.out + blockIdx.y * g.out_fs;
    const __amdgpu_buffer_rsrc_t orsrc =
        __builtin_amdgcn_make_buffer_rsrc(fout, 0, (unsigned)(g.out_h * g.out_pitch), 0x00020000);
    const bool out_aligned = (((uintptr_t)fout | (unsigned)g.out_pitch | (unsigned)(x0 * C * 2)) & 3) == 0;
    const int valid_bytes = sw * C * 2;

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
#pragma unroll
                for (int b = 0; b < kRsLoadBatch; b++) {
                    const int u = u0 + b * kRsThreads;
                    int r = (int)((float)u * inv_sd);   // u / stage_dw, corrected below (u < 2^20)
                    r -= r * g.stage_dw > u;
                    r += (r + 1) * g.stage_dw <= u;
                    const int off = delta + (hi + r) * g.in_pitch + xs * C * 2;
                    const int at = (off & ~3) + 4 * (u - r * g.stage_dw);
                    v[b] = u < total ? __builtin_amdgcn_raw_buffer_load_b32(irsrc, at, 0, 0) : 0u;
                }
#pragma unroll
                for (int b = 0; b < kRsLoadBatch; b++)
                    if (u0 + b * kRsThreads < total) stage[u0 + b * kRsThreads] = v[b];
            }
            __syncthreads();
            for (int j = rl; j < nr; j += RL) {
                const int pos = ((delta + (hi + j) * g.in_pitch + xs * C * 2) & 3) + hoffb;   // even
                const uint32_t* srow = stage + j * g.stage_dw + (pos >> 2);
                const unsigned sh = pos & 3;   // 0 or 2
                uint32_t dw[NE + 1];
#pragma unroll
                for (int t = 0; t <= NE; t++) dw[t] = srow[t];
                double acc[C];
#pragma unroll
                for (int c = 0; c < C; c++) acc[c] = 0.0;
#pragma unroll
                for (int t = 0; t < NE; t++) {
                    const uint32_t e = __builtin_amdgcn_alignbyte(dw[t + 1], dw[t], sh);
#pragma unroll
                    for (int b = 0; b < 2; b++) {
                        const int idx = t * 2 + b;   // sample of the window: tap idx / C of channel idx % C, ascending
                        if (idx < K * C) acc[idx % C] = rs16_mad((e >> (16 * b)) & 0xffffu, kh[idx / C], acc[idx % C]);
                    }
                }
                uint16_t* rrow = ring16 + ((hi + j) % g.ring_rows) * (RDW * 2) + px * C;
#pragma unroll
                for (int c = 0; c < C; c++) rrow[c] = (uint16_t)rs16_store(acc[c]);
            }
            __syncthreads();
            hi += nr;
        }
        // vertical: one output row per wave (WPR waves per row), coefficients uniform, two samples per lane
        for (int q = wave; q < nob * WPR; q += kRsThreads / 64) {
            const int r = q / WPR;
            const int o = o0 + r;
            const int dcol = (q - r * WPR) * 64 + lane;
            const int f = g.vf[o], n = g.vc[o];
            const double* kv = g.vk + (size_t)o * g.vks;
            int slot = f % g.ring_rows;
            double a0 = 0.0, a1 = 0.0;
#pragma unroll 4
            for (int i = 0; i < n; i++) {
                const double k = kv[i];
                const uint32_t w = ring[slot * RDW + dcol];
                a0 = rs16_mad(w & 0xffffu, k, a0);
                a1 = rs16_mad(w >> 16, k, a1);
                if (++slot == g.ring_rows) slot = 0;
            }
            const int b0 = dcol * 4;
            if (b0 < valid_bytes) {
                const int row_off = o * g.out_pitch + x0 * C * 2 + b0;
                const uint32_t s0 = rs16_store(a0), s1 = rs16_store(a1);
                if (out_aligned && b0 + 4 <= valid_bytes) {
                    __builtin_amdgcn_raw_buffer_store_b32(s0 | (s1 << 16), orsrc, row_off, 0, 0);
                } else {
                    __builtin_amdgcn_raw_buffer_store_b16((uint16_t)s0, orsrc, row_off, 0, 0);
                    if (b0 + 2 < valid_bytes) __builtin_amdgcn_raw_buffer_store_b16((uint16_t)s1, orsrc, row_off + 2, 0, 0);
                }
            }
        }
    }
}

// horizontal tap counts with a fused instance (a request runs on the smallest one >= its ksize, zero-padded)
#define LZ_RS16_BUCKETS(X) X(3) X(5) X(7) X(9) X(11) X(13) X(17) X(25)

int rs16_bucket(int ksize, bool small) {
    int k = 0;
    if ((!small || env().rs_no_small_buckets) && ksize < 7) ksize = 7;   // 3 and 5: the short filters only (lanczos_resize.hip)
#define X(KB) \
    if (!k && ksize <= KB) k = KB;
    LZ_RS16_BUCKETS(X)
#undef X
    return k;
}

hipError_t rs16_launch_fused(const lanczos_resize_desc* d, const RsFusedPlan& fp, const ResizeAxis* H, const ResizeAxis* V,
                             const uint8_t* in, uint8_t* out, size_t in_fs, size_t out_fs, int frames, hipStream_t stream) {
    Rs16Fused g{};
    g.in_pitch = d->in_w * d->channels * 2;
    g.out_pitch = d->out_w * d->channels * 2;
    g.in_h = d->in_h, g.out_w = d->out_w, g.out_h = d->out_h;
    g.in_fs = in_fs, g.out_fs = out_fs;
    g.hf = H->first(), g.hc = H->count(), g.hk = H->coeffs64(), g.hks = H->host.ksize;
    g.vf = V->first(), g.vc = V->count(), g.vk = V->coeffs64(), g.vks = V->host.ksize;
    g.strips = fp.strips, g.rows_per_chunk = fp.rows_per_chunk;
    g.ring_rows = fp.ring_rows, g.stage_rows = fp.stage_rows, g.stage_dw = fp.stage_dw;
    for (int f0 = 0; f0 < frames; f0 += 65535) {
        const int nf = std::min(65535, frames - f0);
        g.in = in + (size_t)f0 * in_fs;
        g.out = out + (size_t)f0 * out_fs;
        const dim3 grid(fp.strips * fp.chunks, nf);
        bool launched = false;
#define X(KB)                                                                                                           \
    if (!launched && fp.K == KB) {                                                                                      \
        if (d->channels == 1) hipLaunchKernelGGL((k_rs16_fused<1, KB>), grid, dim3(kRsThreads), fp.lds, stream, g);     \
        else if (d->channels == 3) hipLaunchKernelGGL((k_rs16_fused<3, KB>), grid, dim3(kRsThreads), fp.lds, stream, g); \
        else hipLaunchKernelGGL((k_rs16_fused<4, KB>), grid, dim3(kRsThreads), fp.lds, stream, g);                      \
        launched = true;                                                                                                \
    }
        LZ_RS16_BUCKETS(X)
#undef X
        if (!launched) return hipErrorInvalidValue;
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t rs16_launch_pass(bool horizontal, const ResizeAxis* ax, int channels, const uint8_t* src, size_t src_fs,
                            size_t src_pitch, uint8_t* dst, size_t dst_fs, size_t dst_pitch, int n_cols, int rows, int frames,
                            hipStream_t stream) {
    Rs16Pass p{};
    p.src_fs = src_fs, p.dst_fs = dst_fs, p.src_pitch = src_pitch, p.dst_pitch = dst_pitch;
    p.n_cols = n_cols, p.channels = channels;
    p.first = ax->first(), p.count = ax->count(), p.coeffs = ax->coeffs64(), p.ksize = ax->host.ksize;
    for (int f0 = 0; f0 < frames; f0 += 65535) {
        const int nf = std::min(65535, frames - f0);
        p.src = src + (size_t)f0 * src_fs;
        p.dst = dst + (size_t)f0 * dst_fs;
        const dim3 grid((n_cols + kRsThreads - 1) / kRsThreads, rows, nf);
        if (horizontal) hipLaunchKernelGGL(k_rs16_h, grid, dim3(kRsThreads), 0, stream, p);
        else hipLaunchKernelGGL(k_rs16_v, grid, dim3(kRsThreads), 0, stream, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace lz
