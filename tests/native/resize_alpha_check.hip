// resize_alpha_check.hip -- the two per-pixel conversions of LANCZOS_RESIZE_ALPHA as the resize kernels use them
// (lanczos_alpha.hpp: rs_premul_px, rs_unpremul_px), run on the device over every (value, alpha) pair and compared on the
// host with the literal integer formulas of the contract:
//   premultiply      t = c * A + 128, c' = ((t >> 8) + t) >> 8
//   un-premultiply   A == 0 or A == 255: c = c'; otherwise c = min(255, 255 * c' / A), truncating
// The un-premultiply divides through an f32 reciprocal; this run is what proves it exact.  Each pair sits in all three
// colour bytes of a pixel in turn (the other two hold other values), so every byte lane of the helpers is covered.
// Prints "all 65536 pairs exact" twice and exits 0, or the first mismatches and exits 1.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "lanczos_alpha.hpp"

__global__ void k_convert(const uint32_t* px, uint32_t* pre, uint32_t* un, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    pre[i] = lz::rs_premul_px(px[i]);
    un[i] = lz::rs_unpremul_px(px[i]);
}

static uint32_t premul_ref(uint32_t c, uint32_t A) {
    const uint32_t t = c * A + 128;
    return ((t >> 8) + t) >> 8;
}
static uint32_t unpremul_ref(uint32_t c, uint32_t A) {
    if (A == 0 || A == 255) return c;
    const uint32_t q = (255 * c) / A;
    return q < 255 ? q : 255;
}

#define CHECK(x)                                                                     \
    do {                                                                             \
        hipError_t e_ = (x);                                                         \
        if (e_ != hipSuccess) {                                                      \
            printf("%s: %s\n", #x, hipGetErrorString(e_));                           \
            return 2;                                                                \
        }                                                                            \
    } while (0)

int main() {
    const int pairs = 65536, n = pairs * 3;
    std::vector<uint32_t> px(n), pre(n), un(n);
    for (int lane = 0; lane < 3; lane++)
        for (int i = 0; i < pairs; i++) {
            const uint32_t v = i & 255, A = i >> 8;
            const uint32_t o1 = (v * 7 + 13) & 255, o2 = 255 - v;   // the other two colour bytes
            const uint32_t c[3] = {lane == 0 ? v : o1, lane == 1 ? v : (lane == 0 ? o1 : o2), lane == 2 ? v : o2};
            px[lane * pairs + i] = c[0] | (c[1] << 8) | (c[2] << 16) | (A << 24);
        }
    uint32_t *d_px, *d_pre, *d_un;
    CHECK(hipMalloc((void**)&d_px, n * 4));
    CHECK(hipMalloc((void**)&d_pre, n * 4));
    CHECK(hipMalloc((void**)&d_un, n * 4));
    CHECK(hipMemcpy(d_px, px.data(), n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_convert, dim3((n + 255) / 256), dim3(256), 0, 0, d_px, d_pre, d_un, n);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(pre.data(), d_pre, n * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(un.data(), d_un, n * 4, hipMemcpyDeviceToHost));
    int bad_pre = 0, bad_un = 0;
    bool seen[2][65536] = {};
    for (int i = 0; i < n; i++) {
        const uint32_t p = px[i], A = p >> 24;
        uint32_t want_pre = A << 24, want_un = A << 24;
        for (int b = 0; b < 3; b++) {
            const uint32_t c = (p >> (8 * b)) & 255;
            want_pre |= premul_ref(c, A) << (8 * b);
            want_un |= unpremul_ref(c, A) << (8 * b);
            seen[0][(A << 8) | c] = seen[1][(A << 8) | c] = true;
        }
        if (pre[i] != want_pre && bad_pre++ < 8) printf("premultiply %08x: got %08x, want %08x\n", p, pre[i], want_pre);
        if (un[i] != want_un && bad_un++ < 8) printf("un-premultiply %08x: got %08x, want %08x\n", p, un[i], want_un);
    }
    int covered = 0;
    for (int i = 0; i < 65536; i++) covered += seen[0][i] && seen[1][i];
    if (covered != 65536) {
        printf("only %d of 65536 pairs covered\n", covered);
        return 1;
    }
    if (!bad_pre) printf("premultiply: all %d pairs exact\n", covered);
    if (!bad_un) printf("un-premultiply: all %d pairs exact\n", covered);
    (void)hipFree(d_px), (void)hipFree(d_pre), (void)hipFree(d_un);
    return bad_pre || bad_un ? 1 : 0;
}
