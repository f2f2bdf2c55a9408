// lanczos_resize32.hip -- the kernels of LANCZOS_RESIZE_F32: float samples resized as Pillow resizes mode F
// (include/lanczos_hip.h).  Tables (the double ones of the 16-bit path), cache, planning and dispatch are in
// lanczos_resize.hip; the two kernel paths mirror those of lanczos_resize16.hip with 4-byte samples:
//
//   fused     k_rs32_fused: input rows staged in LDS as the dwords they are, horizontal pass into an LDS ring of float rows,
//             vertical pass from the ring.  A thread keeps one output column and its K double coefficients in registers for
//             the whole march; the vertical coefficients are workgroup-uniform scalar loads; a lane of the vertical pass owns
//             one sample of the row.
//   two-pass  k_rs32_h into the float intermediate in context scratch, k_rs32_v from it: any tap count, and the only kernel
//             when one axis keeps its size.
//
// Pillow accumulates in double, tap by tap: ss = ss + (double)sample * k, and stores (float)ss.  The bits follow from four
// things.  (1) The multiply and the add round separately: every tap goes through rs32_mad, spelled with __dmul_rn /
// __dadd_rn, which the compiler never contracts (the build also passes -ffp-contract=off).  (2) One chain per sample in
// ascending tap order.  (3) Exactly `count` taps are multiplied.  A float next to the window may be inf or NaN, and
// inf * 0.0 is NaN, so the 16-bit kernels' padding (a neighbouring sample times +0.0) is not harmless here: the unrolled
// horizontal loop of the fused kernel selects on tap < count -- never on the coefficient, since a zero weight inside Pillow's
// window is multiplied there too -- and every other loop runs to count.  Staged dwords beyond the frame read as 0 and are
// never multiplied either.  (4) Denormals survive: samples travel as dwords, and float <-> double conversions and the
// double arithmetic run with the kernel mode's denormal bits set (FP_DENORM = 3 for both fields of the MODE register, the
// compiler's default: the build passes no flush flag).
#include "lanczos_resize.hpp"

#include <algorithm>

namespace lz {

__device__ __forceinline__ double rs32_mad(float sample, double k, double ss) {
    return __dadd_rn(ss, __dmul_rn((double)sample, k));
}

// one pass of the two-pass path: `n_cols` samples per output row, frames in blockIdx.z; pitches in samples
struct Rs32Pass {
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
__global__ __launch_bounds__(kRsThreads) void k_rs32_h(Rs32Pass p) {
    const int x = blockIdx.x * kRsThreads + threadIdx.x;
    if (x >= p.n_cols) return;
    const int o = x / p.channels, c = x - o * p.channels;
    const float* src = (const float*)(p.src + blockIdx.z * p.src_fs) + blockIdx.y * p.src_pitch + c;
    const int f = p.first[o], n = p.count[o];
    const double* k = p.coeffs + (size_t)o * p.ksize;
    double ss = 0.0;
#pragma unroll 4
    for (int i = 0; i < n; i++) ss = rs32_mad(src[(size_t)(f + i) * p.channels], k[i], ss);
    ((float*)(p.dst + blockIdx.z * p.dst_fs))[blockIdx.y * p.dst_pitch + x] = __double2float_rn(ss);
}

// vertical: output row o = blockIdx.y, sample column x (coefficients uniform over the workgroup)
__global__ __launch_bounds__(kRsThreads) void k_rs32_v(Rs32Pass p) {
    const int x = blockIdx.x * kRsThreads + threadIdx.x;
    if (x >= p.n_cols) return;
    const int o = blockIdx.y;
    const int f = p.first[o], n = p.count[o];
    const double* k = p.coeffs + (size_t)o * p.ksize;
    const float* src = (const float*)(p.src + blockIdx.z * p.src_fs) + (size_t)f * p.src_pitch + x;
    double ss = 0.0;
#pragma unroll 4
    for (int i = 0; i < n; i++) ss = rs32_mad(src[(size_t)i * p.src_pitch], k[i], ss);
    ((float*)(p.dst + blockIdx.z * p.dst_fs))[o * p.dst_pitch + x] = __double2float_rn(ss);
}

struct Rs32Fused {
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
struct Rs32Strip {
    static constexpr int SW = rs_strip_width(C, 4);   // output pixels per strip
    static constexpr int RL = kRsThreads / SW;        // input rows per horizontal round
    static constexpr int RDW = SW * C;                // ring row in dwords (one sample each)
    static constexpr int WPR = RDW / 64;              // waves per ring row in the vertical pass
};

template <int C, int K>
__global__ __launch_bounds__(kRsThreads) void k_rs32_fused(Rs32Fused g) {
    using S = Rs32Strip<C>;
    constexpr int SW = S::SW, RL = S::RL, RDW = S::RDW, WPR = S::WPR;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* ring = lds;                        // [ring_rows][RDW]
    uint32_t* stage = lds + g.ring_rows * RDW;   // [stage_rows][stage_dw]

    const int tid = threadIdx.x;
    const int strip = blockIdx.x % g.strips, chunk = blockIdx.x / g.strips;
    const int x0 = strip * SW;
    const int sw = min(SW, g.out_w - x0);
    const int xs = g.hf[x0];   // first input pixel of the strip's span

    // horizontal: this thread's output column for the whole march, its coefficients in registers; nh taps are multiplied
    const int px = tid % SW, rl = tid / SW;
    double kh[K];
    int hoff, nh;
    {
        const int p = x0 + min(px, sw - 1);
        nh = px < sw ? g.hc[p] : 0;
        hoff = (g.hf[p] - xs) * C;   // dwords
#pragma unroll
        for (int k = 0; k < K; k++) kh[k] = k < nh ? g.hk[(size_t)p * g.hks + k] : 0.0;
    }

    // frames start on a dword and have dword pitches (checked by the caller): a staged dword is a sample.  Dwords beyond
    // the frame read as 0; like the samples of a row behind a window's last tap they are staged but never multiplied
    const uint8_t* fin = g.in + blockIdx.y * g.in_fs;
    const __amdgpu_buffer_rsrc_t irsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(fin), 0, (unsigned)(g.in_h * g.in_pitch), 0x00020000);
    uint8_t* fout = g.out + blockIdx.y * g.out_fs;
    const __amdgpu_buffer_rsrc_t orsrc =
        __builtin_amdgcn_make_buffer_rsrc(fout, 0, (unsigned)(g.out_h * g.out_pitch), 0x00020000);
    const int valid_dw = sw * C;

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
                    const int at = (hi + r) * g.in_pitch + 4 * (xs * C + u - r * g.stage_dw);
                    v[b] = u < total ? __builtin_amdgcn_raw_buffer_load_b32(irsrc, at, 0, 0) : 0u;
                }
#pragma unroll
                for (int b = 0; b < kRsLoadBatch; b++)
                    if (u0 + b * kRsThreads < total) stage[u0 + b * kRsThreads] = v[b];
            }
            __syncthreads();
            for (int j = rl; j < nr; j += RL) {
                const uint32_t* srow = stage + j * g.stage_dw + hoff;
                double acc[C];
#pragma unroll
                for (int c = 0; c < C; c++) acc[c] = 0.0;
#pragma unroll
                for (int k = 0; k < K; k++) {
#pragma unroll
                    for (int c = 0; c < C; c++) {
                        const double ss = rs32_mad(__uint_as_float(srow[k * C + c]), kh[k], acc[c]);
                        acc[c] = k < nh ? ss : acc[c];   // a select on the tap count: the sum of a tap past it is dropped
                    }
                }
                uint32_t* rrow = ring + ((hi + j) % g.ring_rows) * RDW + px * C;
#pragma unroll
                for (int c = 0; c < C; c++) rrow[c] = __float_as_uint(__double2float_rn(acc[c]));
            }
            __syncthreads();
            hi += nr;
        }
        // vertical: one output row per wave (WPR waves per row), coefficients uniform, one sample per lane
        for (int q = wave; q < nob * WPR; q += kRsThreads / 64) {
            const int r = q / WPR;
            const int o = o0 + r;
            const int dcol = (q - r * WPR) * 64 + lane;
            const int f = g.vf[o], n = g.vc[o];
            const double* kv = g.vk + (size_t)o * g.vks;
            int slot = f % g.ring_rows;
            double a0 = 0.0;
#pragma unroll 4
            for (int i = 0; i < n; i++) {
                a0 = rs32_mad(__uint_as_float(ring[slot * RDW + dcol]), kv[i], a0);
                if (++slot == g.ring_rows) slot = 0;
            }
            if (dcol < valid_dw)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(__double2float_rn(a0)), orsrc,
                                                      o * g.out_pitch + 4 * (x0 * C + dcol), 0, 0);
        }
    }
}

hipError_t rs32_launch_fused(const lanczos_resize_desc* d, const RsFusedPlan& fp, const ResizeAxis* H, const ResizeAxis* V,
                             const uint8_t* in, uint8_t* out, size_t in_fs, size_t out_fs, int frames, hipStream_t stream) {
    Rs32Fused g{};
    g.in_pitch = d->in_w * d->channels * 4;
    g.out_pitch = d->out_w * d->channels * 4;
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
        if (d->channels == 1) hipLaunchKernelGGL((k_rs32_fused<1, KB>), grid, dim3(kRsThreads), fp.lds, stream, g);     \
        else if (d->channels == 3) hipLaunchKernelGGL((k_rs32_fused<3, KB>), grid, dim3(kRsThreads), fp.lds, stream, g); \
        else hipLaunchKernelGGL((k_rs32_fused<4, KB>), grid, dim3(kRsThreads), fp.lds, stream, g);                      \
        launched = true;                                                                                                \
    }
        X(3) X(5) X(7) X(9) X(11) X(13) X(17) X(25)   // the buckets of rs16_bucket
#undef X
        if (!launched) return hipErrorInvalidValue;
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t rs32_launch_pass(bool horizontal, const ResizeAxis* ax, int channels, const uint8_t* src, size_t src_fs,
                            size_t src_pitch, uint8_t* dst, size_t dst_fs, size_t dst_pitch, int n_cols, int rows, int frames,
                            hipStream_t stream) {
    Rs32Pass p{};
    p.src_fs = src_fs, p.dst_fs = dst_fs, p.src_pitch = src_pitch, p.dst_pitch = dst_pitch;
    p.n_cols = n_cols, p.channels = channels;
    p.first = ax->first(), p.count = ax->count(), p.coeffs = ax->coeffs64(), p.ksize = ax->host.ksize;
    for (int f0 = 0; f0 < frames; f0 += 65535) {
        const int nf = std::min(65535, frames - f0);
        p.src = src + (size_t)f0 * src_fs;
        p.dst = dst + (size_t)f0 * dst_fs;
        const dim3 grid((n_cols + kRsThreads - 1) / kRsThreads, rows, nf);
        if (horizontal) hipLaunchKernelGGL(k_rs32_h, grid, dim3(kRsThreads), 0, stream, p);
        else hipLaunchKernelGGL(k_rs32_v, grid, dim3(kRsThreads), 0, stream, p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace lz
