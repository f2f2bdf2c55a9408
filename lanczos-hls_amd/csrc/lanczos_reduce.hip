// lanczos_reduce.hip -- reduce by whole factors: Pillow's Image.reduce((fx, fy), box) on 8-bit frames of 1, 3 or 4
// interleaved channels (include/lanczos_hip.h, lanczos_reduce_*).  It stands on its own and in front of the
// resize of a request with reducing_gap.
//
// A pure streaming kernel: every source byte inside the box is read once, the output is 1 / (fx * fy) of it.
//
//   k_reduce<C>  a workgroup owns one output row of one frame and a tile of its output pixels whose source span is at most
//                kRdSpan bytes of a source row.  Phase 1 walks the block's fy source rows: thread t loads dwords t, t + 256,
//                ... of the span, whatever fx and the pixel size are, so a wave reads 256 contiguous bytes per load and a
//                thread has kRdRows x kRdDw loads in flight; it keeps one uint32 column sum per byte.  A row whose span does
//                not start on a dword (odd pitch, odd base, odd box) is read as aligned dwords and shifted with alignbyte.
//                Phase 2 goes through LDS: the column sums are written out, and a thread gathers the fx sums of each of the
//                four samples of one output dword, divides and stores the packed dword (bytes at a ragged or misaligned end).
//   k_reduce_wide  fx * C > kRdSpan, a block row wider than a tile: one workgroup per output pixel, a plain strided sum
//                and an LDS tree.  Slow and rare (fx above 1024); present so that every supported factor runs.
//
// Arithmetic is Pillow's: out = ((sum + d / 2) * m(d)) >> 24 in uint32 with d the pixels the block really covers and
// m(d) = floor(2^24 / d); the four divisors of a launch (interior, ragged right, ragged bottom, the corner) come from the host.
#include "lanczos_resize.hpp"

#include <algorithm>

namespace lz {

constexpr int kRdDw = 4;                            // dwords of the span per thread
constexpr int kRdRows = 4;                          // source rows per batch of loads: kRdRows * kRdDw loads in flight
constexpr int kRdSpan = kRdDw * kRsThreads * 4;     // bytes of a source row per tile

struct RdArgs {
    const uint8_t* in;
    uint8_t* out;
    unsigned long long in_fs, out_fs;
    int in_pitch, in_bytes;        // bytes of a source row, of a source frame
    int x0, y0, bw, bh;            // the box: origin, extent in pixels
    int fx, fy, ow, oh;
    int tile_ow;                   // output pixels per tile
    uint32_t mul[2][2], half[2][2];   // [ragged bottom][ragged right]: m(d), d / 2
    int last_w, last_h;            // columns / rows of the last block column / row
};

template <int C>
__global__ __launch_bounds__(kRsThreads) void k_reduce(RdArgs g) {
    __shared__ __attribute__((aligned(16))) uint32_t col[kRdSpan];
    const int tid = threadIdx.x;
    const int oy = blockIdx.y;
    const int ox0 = blockIdx.x * g.tile_ow;
    const int now = min(g.tile_ow, g.ow - ox0);                 // output pixels of this tile
    const int px0 = ox0 * g.fx;                                 // first box column of the tile
    const int span = (min(px0 + now * g.fx, g.bw) - px0) * C;   // source bytes per row
    const int ndw = (span + 3) >> 2;
    const int nrows = oy == g.oh - 1 ? g.last_h : g.fy;

    const uint8_t* fin = g.in + blockIdx.z * g.in_fs;
    // dword-aligned base and range, as the fused resize: bytes that share a dword with the frame's ends are read and never
    // used, everything further out reads as 0
    const int delta = (int)((uintptr_t)fin & 3);
    const __amdgpu_buffer_rsrc_t irsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(fin - delta), 0,
                                                                           (unsigned)((delta + g.in_bytes + 3) & ~3), 0x00020000);
    uint32_t acc[kRdDw][4];
#pragma unroll
    for (int j = 0; j < kRdDw; j++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[j][b] = 0u;

    const int row_off = delta + (g.y0 + oy * g.fy) * g.in_pitch + (g.x0 + px0) * C;
    for (int r0 = 0; r0 < nrows; r0 += kRdRows) {
        uint32_t v[kRdRows][kRdDw];
#pragma unroll
        for (int r = 0; r < kRdRows; r++) {
            const int off = row_off + (r0 + r) * g.in_pitch;
            const int at = (off & ~3) + 4 * tid;
            const unsigned sh = (unsigned)off & 3u;
            const bool row_ok = r0 + r < nrows;
            if (sh == 0) {   // uniform over the workgroup
#pragma unroll
                for (int j = 0; j < kRdDw; j++)
                    v[r][j] = row_ok && tid + j * kRsThreads < ndw
                                  ? __builtin_amdgcn_raw_buffer_load_b32(irsrc, at + j * kRsThreads * 4, 0, 0)
                                  : 0u;
            } else {
#pragma unroll
                for (int j = 0; j < kRdDw; j++) {
                    const bool ok = row_ok && tid + j * kRsThreads < ndw;
                    const uint32_t lo = ok ? __builtin_amdgcn_raw_buffer_load_b32(irsrc, at + j * kRsThreads * 4, 0, 0) : 0u;
                    const uint32_t hi = ok ? __builtin_amdgcn_raw_buffer_load_b32(irsrc, at + j * kRsThreads * 4 + 4, 0, 0) : 0u;
                    v[r][j] = __builtin_amdgcn_alignbyte(hi, lo, sh);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kRdRows; r++)
#pragma unroll
            for (int j = 0; j < kRdDw; j++)
#pragma unroll
                for (int b = 0; b < 4; b++) acc[j][b] += (v[r][j] >> (8 * b)) & 255u;
    }
#pragma unroll
    for (int j = 0; j < kRdDw; j++) {
        const int u = tid + j * kRsThreads;
        if (u < ndw) *(uint4*)&col[4 * u] = make_uint4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
    }
    __syncthreads();

    // phase 2: a thread per dword of the output address grid
    uint8_t* orow = g.out + blockIdx.z * g.out_fs + ((size_t)oy * g.ow + ox0) * C;
    const int a0 = (int)((uintptr_t)orow & 3);
    const int nbytes = now * C;
    const int ry = oy == g.oh - 1;
    for (int q = tid; q * 4 - a0 < nbytes; q += kRsThreads) {
        uint32_t packed = 0u;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int s = q * 4 - a0 + b;   // sample of the tile
            if (s < 0 || s >= nbytes) continue;
            const int oxl = s / C, c = s - oxl * C;
            const int rx = ox0 + oxl == g.ow - 1;
            const int w = rx ? g.last_w : g.fx;
            const uint32_t* cp = col + oxl * g.fx * C + c;
            uint32_t sum = 0u;
            for (int i = 0; i < w; i++) sum += cp[i * C];
            packed |= (((sum + g.half[ry][rx]) * g.mul[ry][rx]) >> 24) << (8 * b);
        }
        const int s0 = q * 4 - a0;
        if (s0 >= 0 && s0 + 4 <= nbytes) {
            *(uint32_t*)(orow + s0) = packed;
        } else {
            for (int b = 0; b < 4; b++)
                if (s0 + b >= 0 && s0 + b < nbytes) orow[s0 + b] = (uint8_t)(packed >> (8 * b));
        }
    }
}

// one workgroup per output pixel: a block row wider than a tile
template <int C>
__global__ __launch_bounds__(kRsThreads) void k_reduce_wide(RdArgs g) {
    __shared__ uint32_t part[kRsThreads][C];
    const int tid = threadIdx.x;
    const int ox = blockIdx.x, oy = blockIdx.y;
    const int rx = ox == g.ow - 1, ry = oy == g.oh - 1;
    const int w = rx ? g.last_w : g.fx, h = ry ? g.last_h : g.fy;
    const uint8_t* src = g.in + blockIdx.z * g.in_fs + (size_t)(g.y0 + oy * g.fy) * g.in_pitch + (size_t)(g.x0 + ox * g.fx) * C;
    uint32_t sum[C];
#pragma unroll
    for (int c = 0; c < C; c++) sum[c] = 0u;
    for (int y = 0; y < h; y++) {
        const uint8_t* row = src + (size_t)y * g.in_pitch;
        for (int x = tid; x < w; x += kRsThreads)
#pragma unroll
            for (int c = 0; c < C; c++) sum[c] += row[x * C + c];
    }
#pragma unroll
    for (int c = 0; c < C; c++) part[tid][c] = sum[c];
    __syncthreads();
    for (int n = kRsThreads / 2; n > 0; n >>= 1) {
        if (tid < n)
#pragma unroll
            for (int c = 0; c < C; c++) part[tid][c] += part[tid + n][c];
        __syncthreads();
    }
    if (tid < C)
        g.out[blockIdx.z * g.out_fs + ((size_t)oy * g.ow + ox) * C + tid] =
            (uint8_t)(((part[0][tid] + g.half[ry][rx]) * g.mul[ry][rx]) >> 24);
}

int reduce_validate(int in_w, int in_h, int channels, int fx, int fy, const int32_t* box, int rb[4]) {
    if (in_w < 1 || in_w > kResizeMaxSize || in_h < 1 || in_h > kResizeMaxSize) return LANCZOS_ERR_BAD_ARG;
    if (channels != 1 && channels != 3 && channels != 4) return LANCZOS_ERR_BAD_ARG;
    if (fx < 1 || fy < 1) return LANCZOS_ERR_BAD_ARG;
    rb[0] = box ? box[0] : 0, rb[1] = box ? box[1] : 0, rb[2] = box ? box[2] : in_w, rb[3] = box ? box[3] : in_h;
    if (rb[0] < 0 || rb[0] >= rb[2] || rb[2] > in_w || rb[1] < 0 || rb[1] >= rb[3] || rb[3] > in_h) return LANCZOS_ERR_BAD_ARG;
    if ((long long)fx * fy >= 65536) return LANCZOS_ERR_UNSUPPORTED;           // the divisor table and the uint32 sums
    // 32-bit buffer offsets, the rows of the last batch that are computed but not loaded included
    if ((long long)in_w * ((long long)in_h + kRdRows) * channels + 8 >= (1ll << 31)) return LANCZOS_ERR_UNSUPPORTED;
    return LANCZOS_OK;
}

hipError_t reduce_launch(const uint8_t* in, uint8_t* out, int in_w, int channels, int fx, int fy, const int rb[4], int frames,
                         size_t in_fs, size_t out_fs, RsIssue& is) {
    RdArgs g{};
    g.in_fs = in_fs, g.out_fs = out_fs;
    g.in_pitch = in_w * channels;
    g.in_bytes = (int)std::min<size_t>(in_fs, (size_t)rb[3] * g.in_pitch);   // nothing below the box is read
    g.x0 = rb[0], g.y0 = rb[1], g.bw = rb[2] - rb[0], g.bh = rb[3] - rb[1];
    g.fx = fx, g.fy = fy;
    g.ow = (g.bw + fx - 1) / fx, g.oh = (g.bh + fy - 1) / fy;
    g.last_w = g.bw - (g.ow - 1) * fx, g.last_h = g.bh - (g.oh - 1) * fy;
    for (int ry = 0; ry < 2; ry++)
        for (int rx = 0; rx < 2; rx++) {
            const uint32_t d = (uint32_t)(rx ? g.last_w : fx) * (uint32_t)(ry ? g.last_h : fy);
            g.mul[ry][rx] = (1u << 24) / d, g.half[ry][rx] = d / 2;
        }
    const bool wide = fx * channels > kRdSpan;
    g.tile_ow = wide ? 1 : kRdSpan / (fx * channels);
    const int tiles = wide ? g.ow : (g.ow + g.tile_ow - 1) / g.tile_ow;
    void (*kern)(RdArgs);
    if (wide) kern = channels == 1 ? k_reduce_wide<1> : channels == 3 ? k_reduce_wide<3> : k_reduce_wide<4>;
    else kern = channels == 1 ? k_reduce<1> : channels == 3 ? k_reduce<3> : k_reduce<4>;
    return rs_for_frame_groups(is, frames, [&](int f0, int nf) {
        g.in = in + (size_t)f0 * in_fs;
        g.out = out + (size_t)f0 * out_fs;
        hipLaunchKernelGGL(kern, dim3(tiles, g.oh, nf), dim3(kRsThreads), 0, is.stream, g);
    });
}

}  // namespace lz
