/*
 * include/lanczos_hip.h -- C ABI of the MI355X (gfx950) Lanczos-a resampler.
 *
 * This is the drop-in boundary for the reference's resample path.  Plain pointers and sizes only;
 * no C++/torch types.  What each entry point replaces in /root/reference/LanczosUpscaler:
 *
 *   lanczos_resample_host / lanczos_u8     <- void lanczos(stream_t, stream_t)   lanczos.h:121-126,
 *                                             lanczos.cpp:86-98 (called at full_TB.h:140); results are
 *                                             those of the software model lanczos_expected(),
 *                                             full_TB.h:79-96, on the stb interleaved layout of
 *                                             full_TB.h:107 (R | G<<8 | B<<16, worker.cpp:35-43):
 *                                             bit-identical with LANCZOS_MODE_EXACT (what lanczos_u8 and
 *                                             hls_compat.hpp's lanczos() use), within +-1 LSB per sample
 *                                             with LANCZOS_MODE_LSB1 (what lanczos_desc_init sets: the
 *                                             faster default of the batch / device entry points)
 *   lanczos_resample_device                <- the same, for callers that already hold device memory
 *                                             (batches of frames, row strips of one frame)
 *   lanczos_kernel / lanczos_kernel_idx    <- double lanczos_kernel(double)      full_TB.h:51-53 and
 *                                             kernel_t lanczos_kernel(input_idx_t, output_idx_t, scale_t)
 *                                             kernel.h:6, kernel.cpp:61-67
 *   lanczos_desc                           <- the compile-time macros of params.h (lanczos.h:9-31):
 *                                             IN_WIDTH, IN_HEIGHT, OUT_WIDTH, OUT_HEIGHT, NUM_CHANNELS,
 *                                             LANCZOS_A, SCALE_N, SCALE_D -- here run-time arguments
 *   error codes                            <- the EXIT_FAILURE checks of full_TB.h:110-123
 *
 * Semantics (all verified against the reference's compiled software path, tests/):
 *   horizontal pass then vertical pass; taps floor(x)-a+1 .. floor(x)+a with x = out/((double)N/D);
 *   out-of-range taps dropped, no renormalisation; every store clamps to [0,max] and TRUNCATES; the
 *   horizontal result is stored as a truncated integer before the vertical pass; the vertical pass is
 *   IN PLACE bottom-to-top, so the first K output rows read already-written output rows
 *   (full_TB.h:67-77; K = lanczos_inplace_rows()).
 */
#ifndef LANCZOS_HIP_H
#define LANCZOS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LANCZOS_OK 0
#define LANCZOS_ERR_BAD_ARG 1      /* null pointer, non-positive size, out != in*N/D, a or channels unsupported */
#define LANCZOS_ERR_UNSUPPORTED 2  /* valid request this build cannot run (scale < 1; a row strip that starts inside the in-place prefix rows).
                                     Resizes to any size, downscaling included: lanczos_resize_* below */
#define LANCZOS_ERR_NO_DEVICE 3    /* no HIP device / device index out of range */
#define LANCZOS_ERR_HIP 4          /* a HIP runtime call failed; see lanczos_last_hip_error() */
#define LANCZOS_ERR_NOMEM 5
#define LANCZOS_ERR_RCCL 6         /* an RCCL call of the root exchange failed; see lanczos_multi_last_error() */

/* parity modes (lanczos_desc.mode) */
#define LANCZOS_MODE_LSB1 0   /* default: horizontal pass bit-exact, vertical pass f32 accumulators;
                                 every output sample within +-1 LSB of the reference software path */
#define LANCZOS_MODE_EXACT 1  /* every output sample bit-identical to the reference software path */
#define LANCZOS_MODE_HLS 2    /* the semantics of the reference's HLS pipeline instead (lanczos.cpp:86-98): vertical pass
                                 first (lanczos.cpp:21-51), ROM weights L(|o*D - i*N| / N) (kernel.cpp:40-59), zero rows /
                                 samples above and left of the image, the last row / sample repeated below and right of it
                                 (worker.cpp:147-153,176-188,244,256-265), each pass's sum clamped to [min,max] of its two
                                 centre taps -- the de-ringing of README.md:4 (worker.cpp:66-74,103-111) -- a real-valued
                                 intermediate, truncating final store (worker.cpp:118-130).  Computed in f64 with exact phase
                                 stepping; the hardware's ap_fixed arithmetic is NOT emulated.  Parity unpinned by the
                                 reference (the HLS path cannot be built without Xilinx headers); checked against
                                 oracle/lanczos_hls_model.c.  No in-place prefix: lanczos_inplace_rows() is 0. */

/* which kernel family served the last call (lanczos_last_kernel) */
#define LANCZOS_KERNEL_NONE 0
#define LANCZOS_KERNEL_GENERIC 1  /* table-driven, any rational scale > 1, f64 throughout (always exact) */
#define LANCZOS_KERNEL_FAST 2     /* specialised: integer scale, LDS-staged tiles, f32 taps + exact fallback */
#define LANCZOS_KERNEL_HLS 3      /* LANCZOS_MODE_HLS: V-then-H with de-ringing clamps, f64 */
#define LANCZOS_KERNEL_RESIZE_FUSED 4     /* lanczos_resize_*: one launch, H pass into an LDS row ring, V pass from it */
#define LANCZOS_KERNEL_RESIZE_TWO_PASS 5  /* lanczos_resize_*: H kernel into scratch, V kernel from it (any tap count);
                                             also a resize that changes one axis only, or none */
#define LANCZOS_KERNEL_RESIZE_NEAREST 6   /* lanczos_resize_* with LANCZOS_FILTER_NEAREST: one gather launch, no tables of weights */

typedef struct lanczos_ctx lanczos_ctx; /* opaque: device, stream, cached tap tables, staging buffers */

typedef struct lanczos_desc {
    int32_t in_w, in_h;         /* IN_WIDTH, IN_HEIGHT  (pixels, FULL frame)                     */
    int32_t out_w, out_h;       /* OUT_WIDTH, OUT_HEIGHT (pixels, FULL frame) = in * N / D         */
    int32_t channels;           /* NUM_CHANNELS: 1, 3 or 4, interleaved                            */
    int32_t bytes_per_sample;   /* 1 (u8, the reference) or 2 (u16 generalisation, clamp 65535)    */
    int32_t scale_n, scale_d;   /* SCALE_N / SCALE_D >= 1 (1/1 included: DESIGN.md 1) */
    int32_t a;                  /* LANCZOS_A: 2, 3 or 4                                            */
    int32_t mode;               /* LANCZOS_MODE_*                                                  */
    /* Row strip of the frame to produce (multi-GPU tile sharding).  out_rows == 0 means the whole
     * frame.  With a strip, `in` points at input row lanczos_strip_input_rows().in_row0 and `out`
     * at output row out_row0; both keep the full-frame row pitch. */
    int32_t out_row0, out_rows;
    /* reserved[0] = BIT_PRECISION (params.h; lanczos.h:74-81) of LANCZOS_MODE_HLS's fixed-point emulation: 0 = ideal arithmetic
     * (default), 1..20 = weights cut to BP fractional bits (kernel_t = ap_fixed<8+BP,8>) and the horizontal accumulator cut
     * to BP fractional bits after every tap (num_el_t = ap_fixed<10+BP,10>), AP_TRN / AP_WRAP as the declarations default to.
     * 8-bit samples, HLS mode only.  Parity unpinned (the hardware's ROM comes out of hls::sinpi).  reserved[1..2]: 0. */
    int32_t reserved[3];
} lanczos_desc;

/* ---- descriptor helpers (host only, no GPU needed) ---- */
/* Fill a descriptor for a whole frame; out dims = in * n / d (integer division, as OUT_WIDTH = IN_WIDTH*3). */
int lanczos_desc_init(lanczos_desc* d, int in_w, int in_h, int channels, int bytes_per_sample,
                      int scale_n, int scale_d, int a);
int lanczos_validate(const lanczos_desc* d);
/* K: output rows [0,K) depend on already-written output rows (in-place vertical pass). */
int lanczos_inplace_rows(const lanczos_desc* d);
/* Input rows [*in_row0, *in_row0 + *in_rows) needed to produce output rows [out_row0, out_row0+out_rows). */
int lanczos_strip_input_rows(const lanczos_desc* d, int out_row0, int out_rows, int* in_row0, int* in_rows);
size_t lanczos_in_frame_bytes(const lanczos_desc* d);   /* full frame */
size_t lanczos_out_frame_bytes(const lanczos_desc* d);  /* full frame */

/* ---- weights (host, double) ---- */
double lanczos_kernel(double x, int a);                                                /* full_TB.h:51-53 */
double lanczos_kernel_idx(int in_idx, int out_idx, int scale_n, int scale_d, int a);   /* kernel.h:6     */
/* Tap table of one axis (0 = horizontal, 1 = vertical): for every output index o, first[o] =
 * floor(x)-a+1 and weights[o*2a + k] = L(x - (first[o]+k)), zero where the tap is out of range. */
int lanczos_taps_host(const lanczos_desc* d, int axis, int32_t* first, double* weights);

/* ---- context ---- */
int lanczos_create(lanczos_ctx** ctx, int device);
int lanczos_destroy(lanczos_ctx* ctx);

/* Page-locked host memory for lanczos_resample_host callers that want the copies overlapped. */
int lanczos_host_alloc(void** p, size_t bytes);
int lanczos_host_free(void* p);

/* ---- the resample ---- */
/* Host buffers (what stbi_load returned / what stbi_write_png takes), `frames` frames back to back.
 * Synchronous for the caller; inside, groups of frames are pipelined over copy-in / resample / copy-out
 * streams, which overlaps the PCIe copies when the buffers are page-locked (lanczos_host_alloc). */
int lanczos_resample_host(lanczos_ctx* ctx, const lanczos_desc* d, const void* in, void* out, int frames);
/* Device buffers, asynchronous on `stream` (a hipStream_t; NULL = the default stream, so work queued there
 * by the caller is ordered before the resample).
 * Frame f starts at in + f*in_frame_stride / out + f*out_frame_stride (bytes; 0 = tightly packed). */
int lanczos_resample_device(lanczos_ctx* ctx, const lanczos_desc* d, const void* d_in, void* d_out,
                            int frames, size_t in_frame_stride, size_t out_frame_stride, void* stream);
/* ---- planar frames ----
 * The reference's software model and testbench hold PLANAR frames, byte img_in[NUM_CHANNELS][IN_HEIGHT][IN_WIDTH] /
 * img_out_ex[NUM_CHANNELS][OUT_HEIGHT][OUT_WIDTH] (full_TB.h:20-21), and convert from/to the interleaved stb buffer with
 * host loops (full_TB.h:127-138, 146-165).  The same three steps on the device, asynchronous on `stream`
 * (NULL = default stream); `frames` frames back to back, each [channels][h][w]: */
int lanczos_planar_to_interleaved_device(lanczos_ctx* ctx, const void* d_planar, void* d_interleaved, int w, int h,
                                         int channels, int bytes_per_sample, int frames, void* stream);
int lanczos_interleaved_to_planar_device(lanczos_ctx* ctx, const void* d_interleaved, void* d_planar, int w, int h,
                                         int channels, int bytes_per_sample, int frames, void* stream);
/* img_in[C][IN_H][IN_W] -> img_out[C][OUT_H][OUT_W]: what lanczos_expected(img_in, img_out_ex) computes (full_TB.h:79-96).
 * Whole frames only; the interleaved scratch frames live in the context (one stream at a time per context). */
int lanczos_resample_planar_device(lanczos_ctx* ctx, const lanczos_desc* d, const void* d_in_planar, void* d_out_planar,
                                   int frames, void* stream);
/* The reference's call shape: sizes as plain ints, RGB8 in/out, scale = out_w/in_w reduced.
 * Always LANCZOS_MODE_EXACT: the bytes are those of lanczos_expected() (full_TB.h:79-96). */
int lanczos_u8(lanczos_ctx* ctx, const uint8_t* in, int in_w, int in_h, int channels,
               uint8_t* out, int out_w, int out_h, int a);

/* ---- several devices of one node (lanczos_multi.hip) ----
 * The reference has no parallelism beyond HLS unrolling (ROW_WORKERS, lanczos.cpp:72-82); this is the north star's
 * multi-GPU scheduler.  The resample shards with no data-path collective: */
#define LANCZOS_SPLIT_FRAMES 0  /* a batch of frames in per-device blocks (BASELINE config 4) */
#define LANCZOS_SPLIT_ROWS 1    /* every frame in output row strips + input halo (BASELINE config 5) */
typedef struct lanczos_multi lanczos_multi; /* opaque: one lanczos_ctx per device (+ RCCL communicators for the root path) */
/* partition arithmetic (host only, no GPU): part `part` of `parts` */
int lanczos_partition_frames(int frames, int parts, int part, int* first, int* count);
int lanczos_partition_rows(const lanczos_desc* d, int parts, int part, int* out_row0, int* out_rows, int* in_row0,
                           int* in_rows);
int lanczos_multi_create(lanczos_multi** m, const int* devices, int n_devices);
int lanczos_multi_destroy(lanczos_multi* m);
int lanczos_multi_devices(const lanczos_multi* m);
/* Host buffers (`frames` whole frames back to back): one host thread per device, every device copies only its share over
 * its own PCIe link.  Results are those of lanczos_resample_host on one device. */
int lanczos_resample_multi_host(lanczos_multi* m, const lanczos_desc* d, const void* in, void* out, int frames, int split);
/* Frames resident on the ROOT device (devices[0]): scatter (RCCL ncclSend/ncclRecv group over xGMI) -> resample on every
 * device -> gather.  Synchronous.  compute_ms / total_ms may be NULL.  librccl is loaded on first use (n_devices > 1).
 * EXPERIMENTAL with more than one device: the exchange has not run on multi-GPU hardware yet (no such node was
 * available to the builders).  What is checked without it: the message lists (lanczos_multi_exchange_plan, below) against the
 * partition functions, and the group handling -- every ncclSend / ncclRecv code looked at, an opened group always closed, the
 * first failure reported as LANCZOS_ERR_RCCL with lanczos_multi_last_error().  The caller's current HIP device is preserved. */
int lanczos_resample_multi_root(lanczos_multi* m, const lanczos_desc* d, const void* d_in_root, void* d_out_root, int frames,
                                int split, double* compute_ms, double* total_ms);
/* What the last lanczos_resample_multi_root call saw: the HIP error, the ncclResult_t of the first failing RCCL call and which
 * message of the list it was (-1: ncclGroupStart / ncclCommInitAll, list size: ncclGroupEnd).  Pointers may be NULL. */
int lanczos_multi_last_error(const lanczos_multi* m, int* hip_error, int* rccl_error, int* rccl_message);
/* The root exchange as data (host only, no GPU): message k moves `bytes` from rank `src`'s buffer at src_off to rank `dst`'s
 * buffer at dst_off.  Rank 0's buffers are the caller's root buffers (all frames), a peer's buffer is its shard (split by
 * frames: its frames back to back; split by rows: its strip of every frame, frame after frame).  phase 0 = scatter of the inputs,
 * 1 = gather of the outputs.  Returns the number of messages (call with cap = 0 to size `out`), or -LANCZOS_ERR_*. */
typedef struct lanczos_xfer {
    int src, dst;
    size_t src_off, dst_off, bytes;
} lanczos_xfer;
int lanczos_multi_exchange_plan(const lanczos_desc* d, int frames, int split, int n_devices, int phase, lanczos_xfer* out, int cap);
/* What a ONE-GPU machine can execute of the RCCL path: loads librccl, builds a one-rank communicator on the context's first
 * device and moves `messages` self messages of `bytes` bytes each between two device buffers through the same group executor and
 * send / recv adapter as lanczos_resample_multi_root; the bytes are compared.  fail_at >= 0 makes message `fail_at` name a peer
 * that does not exist: the call then returns LANCZOS_ERR_RCCL and lanczos_multi_last_error() names that message (the group is
 * closed, the communicator proven usable afterwards).  LANCZOS_ERR_UNSUPPORTED: no librccl on this system.  (rccl.h:700,722) */
int lanczos_multi_exchange_selftest(lanczos_multi* m, int messages, size_t bytes, int fail_at);
/* Device memory for plain-C callers that do not include the HIP headers (host/main.c --root). */
int lanczos_device_alloc(int device, void** p, size_t bytes);
int lanczos_device_free(int device, void* p);
int lanczos_device_copy(int device, void* dst, const void* src, size_t bytes, int to_device);

/* ---- resize to any size (Pillow's contract, NOT the reference's) ----
 * lanczos_desc above follows the reference's software model and only upscales by one N/D on both axes.  The resize entry
 * points below take any output size per axis, downscaling included, and produce what Pillow's
 * Image.resize((out_w, out_h), Image.LANCZOS) produces, byte for byte (a = 3 is Pillow's LANCZOS; a = 2 and 4 use the same
 * recipe with that a).  Per axis, with scale = in / out, fs = max(scale, 1), support = a * fs:
 *   output o reads inputs [first, first + count) around centre (o + 0.5) * scale with weights L((i - centre + 0.5) / fs),
 *   L(x) = sinc(x) sinc(x / a) on [-a, a), normalised to sum 1 and rounded to 22-bit fixed point (host, double);
 *   acc = 2^21 + sum(sample * coeff) in int32, result = clamp(acc >> 22, 0, 255).
 * The horizontal pass runs first into an 8-bit intermediate; a pass whose axis keeps its size is skipped (as Pillow does).
 * The order is Pillow 12.2.0's (Image.resize), for every sample type, weighted filter and option below: where both passes
 * run and the frame the resize reads -- the reduced one under a reducing_gap -- has in_h > 100 * in_w and out_h < in_h, the
 * VERTICAL pass runs first, over the full width, into an intermediate of out_h rows stored in the same way, and the
 * horizontal pass runs on that; with LANCZOS_RESIZE_ALPHA the first pass premultiplies and the last one divides alpha out,
 * whichever axis it is.  Such a request never runs the fused kernel: lanczos_resize_plan_host and its _ex, window and crops
 * forms report fused = 0, forced LANCZOS_RESIZE_FUSED is LANCZOS_ERR_UNSUPPORTED, lanczos_last_kernel reports
 * LANCZOS_KERNEL_RESIZE_TWO_PASS, a tensor request takes LANCZOS_TENSOR_CONVERTED and a source layout LANCZOS_SOURCE_PACKED.
 * Windows, tensor outputs, views, crops and sources stay slices and maps of that result.
 * Channels are independent: 8-bit interleaved samples, 1, 3 or 4 channels.  Four channels give Pillow's result on RGBX /
 * RGBa data.  With LANCZOS_RESIZE_ALPHA in the flag word they give Pillow's result in mode RGBA instead (channel 3 is
 * straight alpha), byte for byte, inside the same kernels -- no extra launch and no extra pass over memory:
 *   every input pixel is premultiplied: t = c * A + 128, c' = ((t >> 8) + t) >> 8 for its three colour samples c, alpha A
 *   as it is; both passes run on the premultiplied four channels, alpha filtered like any other channel; every output
 *   pixel with resized alpha A keeps its colour samples if A is 0 or 255 and otherwise gets c = min(255, 255 * c' / A)
 *   (truncating; c' > A occurs where the filter rings).  A resize that changes neither axis is a plain copy, flag or not.
 *
 * With LANCZOS_RESIZE_U16 in the flag word the samples are native-endian uint16_t (1, 3 or 4 interleaved channels) and the
 * result is what Pillow produces in mode I;16, byte for byte, every channel resized as an independent I;16 plane.  Pillow
 * does not use the fixed-point recipe there.  The tap geometry (first, count, the weights and their normalisation) is the
 * one above, but the coefficients stay double and one pass computes, per output sample,
 *   ss = 0.0; for i ascending: ss = ss + (double)sample[first + i] * k[i]    -- an IEEE multiply and an IEEE add, no FMA;
 *   v = (int)(ss < 0 ? ss - 0.5 : ss + 0.5)                                  -- truncating;
 *   stored = lo | hi << 8 with lo = clip8(v % 256) (C's %: the sign of v) and hi = clip8(v >> 8), clip8 to 0 .. 255.
 * That store is Pillow's, quirk included: a negative v stores 0, but a v above 65535 stores 0xFF00 | (v & 255), NOT 65535:
 * the low byte wraps.  It is no corner: Lanczos overshoots at every hard edge of a full-range image.  The horizontal pass
 * runs first into a 16-bit intermediate stored that way; a pass whose axis keeps its size is skipped, a resize that changes
 * neither axis is a plain copy.  The bytes are those of a Pillow build whose compiler does not contract the multiply and
 * the add into an FMA (the x86-64 wheels; checked against 12.2.0).  Frame strides stay in bytes; base pointers and strides
 * of a 16-bit request must be even.  Pillow has no 16-bit RGBA: LANCZOS_RESIZE_U16 | LANCZOS_RESIZE_ALPHA is refused.
 *
 * With LANCZOS_RESIZE_F32 in the flag word the samples are IEEE float (1, 3 or 4 interleaved channels) and the result is what
 * Pillow produces in mode F, bit for bit, every channel resized as an independent F plane.  Tap geometry and coefficients
 * are exactly those of the 16-bit path (lanczos_resize_taps_f64_host / _ex), and one pass computes, per output sample,
 *   ss = 0.0; for i = 0 .. count - 1 ascending: ss = ss + (double)sample[first + i] * k[i]   -- IEEE multiply, IEEE add, no FMA;
 *   stored = (float)ss, rounded to nearest even.
 * No clamp and no rounding to integer: a sum beyond FLT_MAX stores +-inf, a sum in the float denormal range stores the
 * denormal (nothing is flushed, on load or on store), a tiny negative sum stores -0.0.  Exactly `count` taps are multiplied:
 * a tap inside the window whose weight happens to be 0.0 is multiplied (a non-finite sample there gives NaN, as in Pillow),
 * a sample outside the window never is, however the kernels pad their loops.  Output NaNs sit exactly where Pillow's sit;
 * their sign and payload are not part of the contract (x86 and the GPU produce different default NaNs).  The horizontal pass
 * runs first into a float intermediate stored that way; a pass whose axis keeps its size (idle box) is skipped, and a
 * request with no pass is a plain copy.  There is no float alpha: the flag combines with no other flag.  Base pointers and
 * frame strides (still in bytes) must be multiples of 4.  A source box works; reducing_gap does not (LANCZOS_ERR_BAD_ARG), and
 * lanczos_reduce_* takes no floats: Pillow does reduce mode F, but its float box average is no double sum in row-major order
 * and its summation order has not been pinned down -- not built rather than guessed. */
typedef struct lanczos_resize_desc {
    int32_t in_w, in_h;     /* 1..65535 each */
    int32_t out_w, out_h;   /* 1..65535 each, independent of the input size and of each other */
    int32_t channels;       /* 1, 3 or 4, interleaved; 8-bit samples, 16-bit with LANCZOS_RESIZE_U16, float with LANCZOS_RESIZE_F32 */
    int32_t a;              /* 2, 3 or 4 (3 = Pillow's LANCZOS); 3 with any filter other than LANCZOS_FILTER_LANCZOS */
    int32_t reserved[2];    /* reserved[0]: flags, 0 or one of LANCZOS_RESIZE_ALPHA / _U16 / _F32, and the filter in bits
                               8..11 (LANCZOS_RESIZE_FILTER); reserved[1]: must be 0 */
} lanczos_resize_desc;

/* flag of lanczos_resize_desc.reserved[0]: channel 3 is straight alpha (Pillow's RGBA mode); channels must be 4 */
#define LANCZOS_RESIZE_ALPHA 1
/* flag of lanczos_resize_desc.reserved[0]: samples are native-endian uint16_t (Pillow's I;16 arithmetic, see above); not
 * together with LANCZOS_RESIZE_ALPHA */
#define LANCZOS_RESIZE_U16 4
/* flag of lanczos_resize_desc.reserved[0]: samples are float (Pillow's mode F arithmetic, see above); with no other flag */
#define LANCZOS_RESIZE_F32 16

/* The filter (Image.resize's `resample` argument) sits in bits 8..11 of lanczos_resize_desc.reserved[0] and combines with the
 * flags above exactly as those combine with each other.  0 is Lanczos with the descriptor's a; every other filter needs
 * a == 3 (one canonical descriptor per request), values 6..15 are LANCZOS_ERR_BAD_ARG.
 *
 * The weighted filters change two things of the recipe above and nothing else: the support S that stands where a stands
 * (support = S * fs, ksize = 2 * ceil(support) + 1, the safe box of reducing_gap uses S - 0.5) and the weight w(x) of the
 * argument x = (i + first - centre + 0.5) / fs, all in double without contraction, Pillow's functions as they are written:
 *   BOX       S = 0.5  w = 1 if -0.5 < x <= 0.5 (on the signed x: the interval is not symmetric), else 0
 *   BILINEAR  S = 1    x = |x|; w = 1 - x if x < 1, else 0
 *   HAMMING   S = 1    x = |x|; w = 1 if x == 0, 0 if x >= 1, else with x = x * pi: sin(x) / x * (0.54f + 0.46f * cos(x)) --
 *                      the two constants are FLOAT literals widened to double (0.54000002145767211914..., not 0.54)
 *   BICUBIC   S = 2    x = |x|; with a = -0.5: ((a + 2) x - (a + 3)) x x + 1 if x < 1, (((x - 5) x + 8) x - 4) a if x < 2, else 0
 * Normalisation, the 22-bit rounding, the double tables of 16-bit and float requests, pass skipping, the premultiplied alpha
 * path, the I;16 store and the float rule that exactly `count` taps are multiplied are those of Lanczos.
 *
 * LANCZOS_FILTER_NEAREST has no weights.  Per axis, with the span (b0f, b1f) rounded to float as above,
 *   step = (double)(float)(b1f - b0f) / out;  xo = (double)b0f + step * 0.5;
 *   for o = 0 .. out - 1 in order: idx[o] = (int)xo; xo += step          -- a RUNNING SUM, not b0f + (o + 0.5) * step
 * and out[y][x] = in[idx_v[y]][idx_h[x]], whole pixels: with LANCZOS_RESIZE_ALPHA nothing is premultiplied.  One launch
 * gathers both axes (LANCZOS_KERNEL_RESIZE_NEAREST; no intermediate, no context scratch); equal sizes with the full box are the
 * plain copy.  The tables functions report *ksize = 1, count = 1, first = idx and the coefficient 1.0 (2^22 in fixed point);
 * the plan reports fused = 0.  Pillow ignores reducing_gap for NEAREST: a non-zero gap is LANCZOS_ERR_BAD_ARG.  An index
 * outside the source (it cannot happen for a box inside the frame) is LANCZOS_ERR_UNSUPPORTED.
 * LANCZOS_FILTER_NEAREST | LANCZOS_RESIZE_U16 is LANCZOS_ERR_UNSUPPORTED: Pillow sends I;16 through its generic transform, whose
 * indices are computed by direct multiplication and differ from the running sum's (8-bit and float frames take the path
 * above, checked against Pillow 12.2.0). */
#define LANCZOS_FILTER_LANCZOS 0
#define LANCZOS_FILTER_BOX 1
#define LANCZOS_FILTER_BILINEAR 2
#define LANCZOS_FILTER_HAMMING 3
#define LANCZOS_FILTER_BICUBIC 4
#define LANCZOS_FILTER_NEAREST 5
#define LANCZOS_RESIZE_FILTER(f) ((f) << 8)
#define LANCZOS_RESIZE_FILTER_OF(flags) (((flags) >> 8) & 15)

/* forced path of lanczos_resize_force (tests and A/B runs only) */
#define LANCZOS_RESIZE_AUTO 0
#define LANCZOS_RESIZE_FUSED 1     /* LANCZOS_ERR_UNSUPPORTED where the fused kernel cannot run the shape, and for a tensor
                                      request whose float frame spans 2^31 bytes or more */
#define LANCZOS_RESIZE_TWO_PASS 2
#define LANCZOS_RESIZE_CONVERT 3   /* the resize as AUTO plans it; a source layout takes LANCZOS_SOURCE_PACKED (the A/B of the direct
                                    * staging), a destination layout LANCZOS_DEST_UNPACKED (the A/B of the direct stores)
                                    * and a tensor request takes the converted route (the A/B of the
                                      fused tensor epilogue); a byte request runs as under AUTO */

/* host only, no GPU needed */
int lanczos_resize_desc_init(lanczos_resize_desc* d, int in_w, int in_h, int out_w, int out_h, int channels, int a);
/* the same with the flag word (lanczos_resize_desc_init gives 0) */
int lanczos_resize_desc_init_ex(lanczos_resize_desc* d, int in_w, int in_h, int out_w, int out_h, int channels, int a,
                                int flags);
/* the same with a filter: a = 3, reserved[0] = flags | LANCZOS_RESIZE_FILTER(filter); `flags` carries no filter bits */
int lanczos_resize_desc_init_filter(lanczos_resize_desc* d, int in_w, int in_h, int out_w, int out_h, int channels,
                                    int filter, int flags);
/* LANCZOS_ERR_BAD_ARG: size, channels, a, a flag word whose flags are other than 0, LANCZOS_RESIZE_ALPHA, LANCZOS_RESIZE_U16 or
 * LANCZOS_RESIZE_F32, LANCZOS_RESIZE_ALPHA without four channels, a filter above LANCZOS_FILTER_NEAREST, a != 3 with a filter
 * other than LANCZOS_FILTER_LANCZOS.  LANCZOS_ERR_UNSUPPORTED: LANCZOS_FILTER_NEAREST with LANCZOS_RESIZE_U16 */
int lanczos_resize_validate(const lanczos_resize_desc* d);
/* Fixed-point tables of one axis (0 = horizontal, 1 = vertical): output o reads inputs first[o] .. first[o] + count[o] - 1
 * with coeffs[o * ksize + i] (i < count[o]; zero beyond).  *ksize = 2 * ceil(support) + 1.  With first, count and coeffs all
 * NULL only *ksize is returned; otherwise all three must hold out (and out * ksize) elements. */
int lanczos_resize_taps_host(const lanczos_resize_desc* d, int axis, int32_t* first, int32_t* count, int32_t* coeffs,
                             int* ksize);
/* The double tables of the 16-bit and float paths, same shapes and rules: first and count are those of
 * lanczos_resize_taps_host, coeffs[o * ksize + i] is the normalised weight itself.  Neither function looks at
 * LANCZOS_RESIZE_U16 or LANCZOS_RESIZE_F32. */
int lanczos_resize_taps_f64_host(const lanczos_resize_desc* d, int axis, int32_t* first, int32_t* count, double* coeffs,
                                 int* ksize);
/* Diagnostic: what lanczos_resize_device would launch for this request and `frames` frames under LANCZOS_RESIZE_AUTO (the
 * launch itself plans with the same function).  fused = 0: the two-pass path (one axis keeps its size, more horizontal
 * taps than the widest fused instance has, the LDS row ring does not fit 80 KiB, or a frame of 2^31 bytes or more); the
 * other fields are then 0.  fused = 1: the fused kernel instance with K horizontal taps on a grid of strips x chunks
 * workgroups per frame; a workgroup marches down rows_per_chunk output rows in blocks of 8 with an LDS ring of ring_rows
 * rows and a staging area of stage_rows input rows of stage_dw dwords; lds_bytes is their sum.  A 16-bit request has ring
 * and staging rows of 2-byte samples and narrower strips, so it meets the 80 KiB condition at smaller reductions; a float
 * request has rows of 4-byte samples in strips of 128 (one channel) or 64 pixels and meets it at smaller ones still. */
typedef struct lanczos_resize_plan {
    int32_t fused;
    int32_t K, strips, rows_per_chunk, chunks, ring_rows, stage_rows, stage_dw, lds_bytes;
} lanczos_resize_plan;
int lanczos_resize_plan_host(const lanczos_resize_desc* d, int frames, lanczos_resize_plan* out);
/* Device buffers, asynchronous on `stream` (NULL = the default stream), frames at d_in + f * in_frame_stride and
 * d_out + f * out_frame_stride (bytes; 0 = tightly packed), as lanczos_resample_device.  The first call of an axis shape
 * builds its tables and uploads them before it returns (a blocking copy on a private stream, so that the cached tables are
 * valid whether or not the caller's stream is being captured into a graph and whether or not that graph is ever replayed).
 * The two-pass path keeps its intermediate in context scratch: one stream at a time per context, and a captured graph
 * must not outlive its context. */
int lanczos_resize_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const void* d_in, void* d_out, int frames,
                          size_t in_frame_stride, size_t out_frame_stride, void* stream);
/* Host buffers, `frames` frames back to back; synchronous (copy in -> resize -> copy out on the context's stream). */
int lanczos_resize_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const void* in, void* out, int frames);
/* LANCZOS_RESIZE_AUTO / _FUSED / _TWO_PASS / _CONVERT: tests and A/B runs only (lanczos_force_kernel does not affect resizes).
 * LANCZOS_FILTER_NEAREST has one path: forced _FUSED is LANCZOS_ERR_UNSUPPORTED for it, forced _TWO_PASS changes nothing. */
int lanczos_resize_force(lanczos_ctx* ctx, int path);

/* ---- resize from a source box and with reducing_gap (the other two arguments of Pillow's Image.resize) ----
 * The _ex entry points take a lanczos_resize_opts beside the descriptor; NULL is the call without it, and the entry points
 * above forward to them with NULL.
 *
 * box = (x0, y0, x1, y1) in source pixels, fractions allowed, 0 <= x0 < x1 <= in_w and 0 <= y0 < y1 <= in_h.  Per axis with
 * (b0, b1): both are rounded to float (Pillow's C takes float box[4]) and their difference is taken in float,
 *   scale = (double)(float)(b1f - b0f) / out,  centre = (double)b0f + (o + 0.5) * scale,
 * and everything else -- fs, support, ksize, first = max(int(centre - support + 0.5), 0), the end min(int(centre + support
 * + 0.5), in), weights, normalisation, the 22-bit rounding or the double tables of 16-bit requests -- is the recipe above.
 * first indexes the WHOLE source axis and is clipped to the whole source, not to the box: pixels outside the box contribute
 * near its edges.  A pass runs iff out != in || b0f != 0 || b1f != in, so a sub-pixel shift at equal size runs the pass; with
 * both axes idle the call is the plain copy.  Every sample type takes a box (8-bit, LANCZOS_RESIZE_ALPHA, _U16, _F32).
 * The two-pass path produces only the intermediate rows the vertical taps read, and sizes its scratch by them.
 *
 * reducing_gap = g (0 = none, otherwise g >= 1; below 1 or NaN: LANCZOS_ERR_BAD_ARG), as Image.resize(..., reducing_gap=g):
 * all in double on the caller's box, before anything is rounded to float,
 *   fx = int((x1 - x0) / out_w / g) or 1, fy likewise; both 1: the plain box resize.  Otherwise, with s = a - 0.5,
 *   sx = s * (x1 - x0) / out_w, sy likewise, the safe box is
 *   rb = (max(0, int(x0 - sx)), max(0, int(y0 - sy)), min(in_w, ceil(x1 + sx)), min(in_h, ceil(y1 + sy)));
 *   the source is reduced by (fx, fy) over rb (lanczos_reduce_*, below) and the REDUCED frame is resized with the box
 *   ((x0 - rb0) / fx, (y0 - rb1) / fy, (x1 - rb0) / fx, (y1 - rb1) / fy) (divided in double, rounded to float after).
 * The result is Pillow's for the same arguments; it is NOT the resize without a gap (it differs from it in general).
 * Pillow silently drops reducing_gap in mode RGBA and raises for I;16, so neither has an oracle: a gap together with
 * LANCZOS_RESIZE_ALPHA or LANCZOS_RESIZE_U16 is LANCZOS_ERR_BAD_ARG, and so is one with LANCZOS_RESIZE_F32 (not built, see
 * above).  fx * fy >= 65536: LANCZOS_ERR_UNSUPPORTED.
 * The reduced frames live in context scratch under the rules of the two-pass intermediate (one stream at a time per context;
 * a captured launch pins the block; a captured graph must not outlive its context). */
typedef struct lanczos_resize_opts {
    double box[4];        /* x0, y0, x1, y1 */
    double reducing_gap;  /* 0 = none */
    int32_t reserved[4];  /* must be 0 */
} lanczos_resize_opts;
/* the full box of `d` and no gap: the request without options */
int lanczos_resize_opts_init(lanczos_resize_opts* o, const lanczos_resize_desc* d);
/* as lanczos_resize_taps_host / _taps_f64_host.  With a gap that reduces, the tables are those of the inner resize (of the
 * reduced frame with the box after reduction): *ksize and the first[] range follow the reduced axis. */
int lanczos_resize_taps_host_ex(const lanczos_resize_desc* d, const lanczos_resize_opts* o, int axis, int32_t* first,
                                int32_t* count, int32_t* coeffs, int* ksize);
int lanczos_resize_taps_f64_host_ex(const lanczos_resize_desc* d, const lanczos_resize_opts* o, int axis, int32_t* first,
                                    int32_t* count, double* coeffs, int* ksize);
/* Diagnostic: how a request with options resolves (the launch resolves with the same function).  fx = fy = 1: no reduction;
 * safe_box is then (0, 0, in_w, in_h), the reduced size the source's and inner_box the caller's box.  pass_h / pass_v: whether
 * the inner resize runs that pass.  mid_row0 / mid_rows: the rows of the (reduced) source the horizontal pass of the two-pass
 * path produces, which is what its scratch holds per frame (mid_rows x out_w pixels); 0 / 0 unless both passes run.  (A
 * request that runs vertical first, see above, reads those source rows too, but its scratch holds out_h x reduced_w pixels.)  inner:
 * the plan of the inner resize, as lanczos_resize_plan_host reports it. */
typedef struct lanczos_resize_plan_ex {
    int32_t fx, fy;
    int32_t safe_box[4];
    int32_t reduced_w, reduced_h;
    int32_t pass_h, pass_v;
    int32_t mid_row0, mid_rows;
    double inner_box[4];
    lanczos_resize_plan inner;
} lanczos_resize_plan_ex;
int lanczos_resize_plan_host_ex(const lanczos_resize_desc* d, const lanczos_resize_opts* o, int frames,
                                lanczos_resize_plan_ex* out);
int lanczos_resize_device_ex(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* o, const void* d_in,
                             void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride, void* stream);
int lanczos_resize_host_ex(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* o, const void* in,
                           void* out, int frames);

/* ---- resize 8-bit frames straight into a float tensor (PIL.Image.resize -> ToTensor() -> Normalize(mean, std)) ----
 * A tensor request is the byte request plus a table and an output layout:
 *   out[f][c * chan_stride + y * row_stride + x * pix_stride] = lut[c * 256 + P(f, y, x, c)]
 * where P(f, y, x, c) is exactly the byte lanczos_resize_device_ex stores for the same descriptor and options: every filter,
 * box, reducing_gap, LANCZOS_RESIZE_ALPHA, and the plain copy where no pass runs.  out is float, strides count floats, frame f
 * starts out_frame_stride BYTES behind frame f - 1.  CHW is (out_h * out_w, out_w, 1), HWC is (1, out_w * channels, channels);
 * padded rows or planes and a slice of a larger tensor are larger strides.  Floats the contract does not name are not written.
 * Table entries are copied as 32-bit words and nothing is computed on them: NaN payloads and -0.0 arrive unchanged.  An 8-bit
 * sample has 256 values, so any per-channel pointwise map is such a table, and one built with IEEE float operations repeats
 * torch's result bit for bit: lanczos_tensor_lut_normalize builds that of ToTensor() + Normalize().
 * d_lut is a device pointer to channels * 256 floats which the caller owns.  The kernels read it WHEN THEY RUN, not when the
 * call is made: it must stay allocated until they have run, and a replayed graph sees the table's contents of that moment.
 * Routes (lanczos_last_tensor_route): where the byte request runs the fused kernel and a float frame spans less than 2^31
 * bytes, the fused kernel's vertical pass stores the floats itself (LANCZOS_TENSOR_FUSED; LANCZOS_RESIZE_ALPHA included) --
 * a tensor request is fused exactly when lanczos_resize_plan_host(_ex) says the byte request is, on the same plan.  Every
 * other request (two passes, one pass, LANCZOS_FILTER_NEAREST, the plain copy, forced LANCZOS_RESIZE_TWO_PASS, larger float
 * frames) writes its bytes to context scratch and one conversion launch follows (LANCZOS_TENSOR_CONVERTED); that scratch
 * lives under the rules of the two-pass intermediate (one stream at a time per context; a captured launch pins the block; a
 * captured graph must not outlive its context).  lanczos_last_kernel reports the resize kernel as for the byte request. */
typedef struct lanczos_tensor_out {
    const float* d_lut;     /* device: channels * 256 floats, lut[c * 256 + v]; read when the kernels run */
    int64_t chan_stride, row_stride, pix_stride;   /* in floats, each > 0 */
    int32_t reserved[4];    /* must be 0 */
} lanczos_tensor_out;
#define LANCZOS_TENSOR_FUSED 1      /* the resize kernel wrote the floats itself */
#define LANCZOS_TENSOR_CONVERTED 2  /* the bytes went to context scratch and a conversion launch followed */
/* LANCZOS_ERR_BAD_ARG: what lanczos_resize_validate refuses, a null t or table, a stride <= 0 (or above 2^40), non-zero
 * reserved words, strides under which two (c, y, x) share an address -- sorted by stride, each stride must be at least the
 * previous stride times its extent (an axis of extent 1 takes no part).  LANCZOS_ERR_UNSUPPORTED: LANCZOS_RESIZE_U16 or
 * LANCZOS_RESIZE_F32 (no table per 16-bit value or for a float: those frames have lanczos_resize_tensor_norm_* below). */
int lanczos_resize_tensor_validate(const lanczos_resize_desc* d, const lanczos_tensor_out* t);
/* Host only: lut[c * 256 + v] = ((float)v / 255.0f - mean[c]) / std[c], in float with IEEE division and no contraction --
 * bit for bit torch's uint8.to(float32).div(255).sub(mean).div(std).  mean == NULL is 0 and std == NULL is 1, so NULL, NULL is
 * plain ToTensor().  channels: 1, 3 or 4. */
int lanczos_tensor_lut_normalize(int channels, const float* mean, const float* std, float* lut);
/* As lanczos_resize_device_ex (opts may be NULL) with float frames at d_out.  Further LANCZOS_ERR_BAD_ARG: d_out or
 * out_frame_stride no multiple of 4, out_frame_stride (bytes; 0 = the frame's extent) smaller than the frame's extent
 * ((channels - 1) * chan_stride + (out_h - 1) * row_stride + (out_w - 1) * pix_stride + 1 floats). */
int lanczos_resize_tensor_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                 const lanczos_tensor_out* t, const void* d_in, void* d_out, int frames,
                                 size_t in_frame_stride, size_t out_frame_stride, void* stream);
/* Host buffers and a HOST table in t->d_lut; `frames` input frames back to back, float frames one extent apart; synchronous.
 * Floats of `out` the strides do not name keep their contents. */
int lanczos_resize_tensor_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                               const lanczos_tensor_out* t, const void* in, void* out, int frames);
/* 0 if the last call on the context was no tensor call (or failed before its launches), else LANCZOS_TENSOR_FUSED or
 * LANCZOS_TENSOR_CONVERTED */
int lanczos_last_tensor_route(const lanczos_ctx* ctx);

/* ---- ... into a bfloat16 or float16 tensor (the pipeline above followed by .to(torch.bfloat16) / .to(torch.float16)) ----
 * lanczos_resize_tensor_*'s contract with "float" read as "16-bit element":
 *   out[f][c * chan_stride + y * row_stride + x * pix_stride] = lut[c * 256 + P(f, y, x, c)]
 * with out and lut of 16-bit words, strides in ELEMENTS (2 bytes) and P the byte of the byte request.  The words are moved and
 * never computed on, so one entry serves bfloat16, float16 and any other 16-bit pointwise map of an 8-bit sample; zeros,
 * subnormals, NaN and inf patterns arrive unchanged.  A table of float32 entries rounded to nearest-even
 * (lanczos_tensor_lut_convert16) gives what torch's cast of the float32 tensor gives, bit for bit.  Elements the strides do not
 * name are not written: a 16-bit neighbour of a stored element keeps its contents.  The table's lifetime, the overlap rule,
 * the stride cap, the routes (fused where the byte request is and an element frame spans less than 2^31 bytes, else converted),
 * lanczos_last_tensor_route, lanczos_last_kernel, lanczos_resize_force and the scratch and capture rules are the float
 * entry's.  The element width has a struct of its own since lanczos_tensor_out's reserved words must be 0. */
typedef struct lanczos_tensor16_out {
    const uint16_t* d_lut;  /* device: channels * 256 16-bit words, lut[c * 256 + v]; read when the kernels run */
    int64_t chan_stride, row_stride, pix_stride;   /* in ELEMENTS (2 bytes), each > 0 */
    int32_t reserved[4];    /* must be 0 */
} lanczos_tensor16_out;
#define LANCZOS_TENSOR_BF16 1   /* formats of the two table functions; a request carries none */
#define LANCZOS_TENSOR_F16 2
/* as lanczos_resize_tensor_validate */
int lanczos_resize_tensor16_validate(const lanczos_resize_desc* d, const lanczos_tensor16_out* t);
/* Host only: n float32 values to words of `format`, round to nearest, ties to even, as torch's CPU cast.  bfloat16:
 * (bits + 0x7FFF + ((bits >> 16) & 1)) >> 16.  float16: IEEE binary16, subnormals kept, overflow to +-inf.  A NaN becomes
 * some NaN of the format.  LANCZOS_ERR_BAD_ARG: a NULL pointer, n < 0, an unknown format. */
int lanczos_tensor_lut_convert16(const float* in, int n, int format, uint16_t* out);
/* Host only: lanczos_tensor_lut_normalize followed by lanczos_tensor_lut_convert16 --
 * uint8.to(float32).div(255).sub(mean).div(std).to(bfloat16 or float16), bit for bit. */
int lanczos_tensor16_lut_normalize(int channels, const float* mean, const float* std, int format, uint16_t* lut);
/* As lanczos_resize_tensor_device with 16-bit frames at d_out: d_out and out_frame_stride (bytes) are multiples of 2, the
 * frame's extent is ((channels - 1) * chan_stride + (out_h - 1) * row_stride + (out_w - 1) * pix_stride + 1) * 2 bytes. */
int lanczos_resize_tensor16_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                   const lanczos_tensor16_out* t, const void* d_in, void* d_out, int frames,
                                   size_t in_frame_stride, size_t out_frame_stride, void* stream);
/* As lanczos_resize_tensor_host: a HOST table in t->d_lut, 16-bit frames one extent apart; synchronous.  Elements of `out` the
 * strides do not name keep their contents. */
int lanczos_resize_tensor16_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                 const lanczos_tensor16_out* t, const void* in, void* out, int frames);

/* ---- resize and crop in one call: compute only a window of the output (Image.resize(...).crop(window)) ----
 * A window is (x0, y0, w, h) in OUTPUT pixels of the full request (descriptor and options): 0 <= x0, 1 <= w, x0 + w <= out_w
 * and the same for y.  A windowed call stores a tightly packed w x h frame whose sample (x, y, c) is exactly what the same
 * call without a window stores at (x0 + x, y0 + y, c) -- every sample type (8-bit, LANCZOS_RESIZE_ALPHA, _U16, _F32), every
 * filter (LANCZOS_FILTER_NEAREST included), every source box, reducing_gap, and both tensor element widths.  Nothing outside
 * that frame is written, and the result depends only on the source pixels the window's outputs read
 * (lanczos_resize_window_source; a kernel may load a few more inside the frame and drop them).  It
 * is exact by construction: the kernels of the full request run on slices of its tables (first, count and coeffs from output x0
 * or y0 on), which stay cached under the full axes -- a centre crop and the full resize of one shape share their tables.
 * The source `box` is no substitute: its corners are rounded to float and `first` is clipped against the source, not against
 * the output grid, so a box over "the same region" gives other bytes than the crop of the full resize.
 * Whether an axis runs its pass is decided by the FULL request, as without a window: an axis that keeps its size is only
 * cropped, and with both axes idle the call is a crop copy (one launch for any frame count; RGBA is not premultiplied, as in
 * the plain copy).  A NULL window, or the whole output, is the call without one: same route, same bytes -- the entry points
 * without a window forward with NULL.  One window per call, the same for every frame of the batch.
 * Planning follows the window: the fused plan is that of a w x h output (a window the fused kernel cannot run -- see
 * lanczos_resize_plan -- takes the two-pass path, and forced LANCZOS_RESIZE_FUSED is then LANCZOS_ERR_UNSUPPORTED); the
 * two-pass path computes only the intermediate rows the window's vertical taps read, w pixels wide; a horizontal pass alone
 * runs the window's h rows, a vertical pass alone the window's w columns.  lanczos_last_kernel and lanczos_last_tensor_route
 * report as for the full request's route family.  The capture and scratch rules are those of the call without a window.
 * With a reducing_gap that reduces, the reduction still covers the whole safe box (restricting it to the window is not built):
 * the window only applies to the resize of the reduced frames.
 * Tensor calls: the strides describe the window's C x h x w frame -- the overlap rule, the frame's extent, the minimum of
 * out_frame_stride and the 2^31-byte limit of the fused tensor route all use w and h, not out_w and out_h. */
typedef struct lanczos_resize_window {
    int32_t x0, y0, w, h;
    int32_t reserved[4];  /* must be 0 */
} lanczos_resize_window;
/* the whole output of `d` */
int lanczos_resize_window_init(lanczos_resize_window* win, const lanczos_resize_desc* d);
/* Host only.  LANCZOS_ERR_BAD_ARG: what lanczos_resize_validate refuses, a window outside the output, w or h below 1, non-zero
 * reserved words.  win NULL = the whole output. */
int lanczos_resize_window_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win);
/* Host only: rect = (x0, y0, x1, y1), integers, half open -- the source rectangle the windowed request's result depends on.  Per axis: one
 * that runs reads the union of [first[o], first[o] + count[o]) over the window's outputs o (lanczos_resize_taps_host_ex; for
 * LANCZOS_FILTER_NEAREST the smallest index to the largest + 1); an idle axis reads the window's own range.  With a reducing_gap
 * that reduces, rect is the safe box (lanczos_resize_plan_ex.safe_box) whatever the window. */
int lanczos_resize_window_source(const lanczos_resize_desc* d, const lanczos_resize_opts* o, const lanczos_resize_window* win,
                                 int32_t rect[4]);
/* lanczos_resize_plan_host_ex for the windowed request: mid_row0 / mid_rows are the rows the window's vertical taps read, and
 * inner is the fused plan of a w x h output.  The whole output gives what lanczos_resize_plan_host_ex gives. */
int lanczos_resize_window_plan_host(const lanczos_resize_desc* d, const lanczos_resize_opts* o, const lanczos_resize_window* win,
                                    int frames, lanczos_resize_plan_ex* out);
/* As lanczos_resize_device_ex / lanczos_resize_host_ex (o and win may be NULL) with output frames of w x h pixels:
 * out_frame_stride 0 is w * h * channels samples, a smaller one is LANCZOS_ERR_BAD_ARG. */
int lanczos_resize_window_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* o,
                                 const lanczos_resize_window* win, const void* d_in, void* d_out, int frames,
                                 size_t in_frame_stride, size_t out_frame_stride, void* stream);
int lanczos_resize_window_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* o,
                               const lanczos_resize_window* win, const void* in, void* out, int frames);
/* as lanczos_resize_tensor_validate / lanczos_resize_tensor16_validate for a frame of the window's extent */
int lanczos_resize_tensor_window_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win,
                                          const lanczos_tensor_out* t);
int lanczos_resize_tensor16_window_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win,
                                            const lanczos_tensor16_out* t);
/* as the tensor entry points above, element frames of the window's extent:
 * ((channels - 1) * chan_stride + (h - 1) * row_stride + (w - 1) * pix_stride + 1) elements */
int lanczos_resize_tensor_window_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                        const lanczos_resize_window* win, const lanczos_tensor_out* t, const void* d_in,
                                        void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride, void* stream);
int lanczos_resize_tensor_window_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                      const lanczos_resize_window* win, const lanczos_tensor_out* t, const void* in, void* out,
                                      int frames);
int lanczos_resize_tensor16_window_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                          const lanczos_resize_window* win, const lanczos_tensor16_out* t, const void* d_in,
                                          void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride,
                                          void* stream);
int lanczos_resize_tensor16_window_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                        const lanczos_resize_window* win, const lanczos_tensor16_out* t, const void* in,
                                        void* out, int frames);

/* ---- tensor outputs with a channel map and per-frame flips (BGR -> RGB, RGBA -> RGB, RandomHorizontalFlip) ----
 * One entry point for every tensor request: the element width is a field and the window an optional argument.  With (w, h)
 * the extent of the window (of the whole output when win is NULL), P(f, y, x, c) the byte lanczos_resize_window_device stores
 * for the same descriptor, options and window, and m_f = (flip ^ d_flip[f]) & 3 (d_flip NULL: flip & 3):
 *   out[f][oc * chan_stride + Y * row_stride + X * pix_stride] = lut[oc * 256 + P(f, y, x, src_channel[oc])]
 *   X = (m_f & 1) ? w - 1 - x : x        Y = (m_f & 2) ? h - 1 - y : y
 * The table is indexed by the OUTPUT channel: mean / std of lanczos_tensor_lut_normalize are given in output order.  The map is
 * injective: it reorders and drops channels and cannot replicate them (a stride-0 expand on the caller's side does that).  A
 * source channel that no oc names is not stored anywhere.  With LANCZOS_RESIZE_ALPHA the colour samples are un-premultiplied
 * as in the byte request whether or not alpha itself is kept: RGBA -> RGB with alpha is Pillow's resize in mode RGBA followed
 * by .convert("RGB").  Flips mirror inside the frame: the set of addresses written per frame does not depend on them.
 * The overlap rule, the frame's extent, the minimum out_frame_stride and the 2^31-byte limit of the fused route are those of
 * the tensor entries above with `channels` read as out_channels and "element" as elem_bytes: the extent is
 * (out_channels - 1) * chan_stride + (h - 1) * row_stride + (w - 1) * pix_stride + 1 elements.  Elements the strides do not
 * name are not written, 16-bit neighbours included; words are moved and never computed on.  d_lut and d_flip live as d_lut
 * does above: both are read WHEN THE KERNELS RUN, and a replayed graph sees their contents of that moment.  Bits 2..7 of a
 * d_flip byte are ignored (device memory cannot be validated).
 * A view with elem_bytes 4, out_channels == channels, the identity in src_channel, flip 0 and d_flip NULL is
 * lanczos_resize_tensor_window_device: the same words on the same route and the same kernels; with elem_bytes 2 it is
 * lanczos_resize_tensor16_window_device.  Routes: a view is LANCZOS_TENSOR_FUSED exactly when
 * lanczos_resize_window_plan_host says the byte request is fused and the element frame spans less than 2^31 bytes, else
 * LANCZOS_TENSOR_CONVERTED; lanczos_last_tensor_route, lanczos_last_kernel and lanczos_resize_force (LANCZOS_RESIZE_CONVERT
 * included) apply as above.  Byte, 16-bit-sample and float-sample outputs have no map and no flips. */
typedef struct lanczos_tensor_view {
    const void* d_lut;        /* out_channels * 256 elements of elem_bytes each, lut[oc * 256 + v]; read when the kernels run */
    int64_t chan_stride, row_stride, pix_stride;   /* in elements, each > 0 */
    int32_t elem_bytes;       /* 4 (float32 words) or 2 (bfloat16 / float16 words) */
    int32_t out_channels;     /* 1 .. d->channels */
    int32_t src_channel[4];   /* src_channel[oc] < d->channels for oc < out_channels, pairwise distinct; the rest must be 0 */
    int32_t flip;             /* bit 0: mirror x, bit 1: mirror y -- applied to every frame */
    const uint8_t* d_flip;    /* NULL, or one byte per frame (same bits), XORed with `flip`; read when the kernels run */
    int32_t reserved[4];      /* must be 0 */
} lanczos_tensor_view;
/* the identity over every channel, CHW strides of d's whole output, no flips, d_lut NULL.  LANCZOS_ERR_BAD_ARG: a null v, what
 * lanczos_resize_validate refuses, elem_bytes other than 2 or 4 */
int lanczos_tensor_view_init(lanczos_tensor_view* v, const lanczos_resize_desc* d, int elem_bytes);
/* Host only.  LANCZOS_ERR_BAD_ARG: everything lanczos_resize_tensor_window_validate refuses (the overlap rule under the
 * out_channels extents), elem_bytes other than 2 or 4, out_channels outside 1 .. channels, a src_channel out of range, a
 * duplicate or a non-zero one beyond out_channels, flip outside 0 .. 3, non-zero reserved words.  LANCZOS_ERR_UNSUPPORTED:
 * LANCZOS_RESIZE_U16 or LANCZOS_RESIZE_F32 (those frames have lanczos_resize_tensor_norm_* below). */
int lanczos_resize_tensor_view_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win,
                                        const lanczos_tensor_view* v);
/* As lanczos_resize_tensor_window_device (opts and win may be NULL): d_lut and d_flip are device pointers.  Further
 * LANCZOS_ERR_BAD_ARG: d_out or out_frame_stride (bytes; 0 = the frame's extent) no multiple of elem_bytes, a frame stride
 * below the extent. */
int lanczos_resize_tensor_view_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                      const lanczos_resize_window* win, const lanczos_tensor_view* v, const void* d_in,
                                      void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride, void* stream);
/* Host buffers, a HOST table in v->d_lut and a HOST flip array (`frames` bytes, or NULL) in v->d_flip; element frames one
 * extent apart; synchronous.  Elements of `out` the strides do not name keep their contents. */
int lanczos_resize_tensor_view_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                    const lanczos_resize_window* win, const lanczos_tensor_view* v, const void* in, void* out,
                                    int frames);

/* ---- tensor outputs with a crop origin per frame (Resize -> RandomCrop -> RandomHorizontalFlip -> ToTensor -> Normalize) ----
 * A tensor view whose window has one size (w, h) for the whole batch and an origin per frame, read from device memory when the
 * kernels run.  With P_full(f, y, x, c) the byte lanczos_resize_device_ex stores for the same descriptor and options WITHOUT a
 * window, m_f the flip bits of lanczos_tensor_view and (x0_f, y0_f) frame f's origin after clamping:
 *   out[f][oc * chan_stride + Y * row_stride + X * pix_stride] = lut[oc * 256 + P_full(f, y0_f + y, x0_f + x, src_channel[oc])]
 *   X = (m_f & 1) ? w - 1 - x : x        Y = (m_f & 2) ? h - 1 - y : y                            0 <= x < w, 0 <= y < h
 *   x0_f = min(max(d_origin[2 f], 0), out_w - w)        y0_f = min(max(d_origin[2 f + 1], 0), out_h - h)
 * Exact by construction, as a window is.  Everything else is lanczos_tensor_view's contract with (w, h) as the frame: every
 * filter, box and reducing_gap, LANCZOS_RESIZE_ALPHA, both element widths, the overlap rule, the extent, elements the strides
 * do not name left untouched, the 2^31-byte limit of the fused route.  d_origin lives as d_lut and d_flip do: it is read WHEN
 * THE KERNELS RUN, and a replayed graph follows its contents of that moment.  THE CLAMP IS PART OF THE CONTRACT and of the
 * kernels: device memory cannot be validated, and an origin outside the output would index the tap tables out of range.
 * Routes: LANCZOS_TENSOR_FUSED exactly when lanczos_resize_crops_plan_host says fused -- its plan holds for every origin, which
 * the plan of the window at one origin does not -- and the element frame spans less than 2^31 bytes.  Every other request
 * (two passes, one pass, LANCZOS_FILTER_NEAREST, a plan that does not fit, forced LANCZOS_RESIZE_TWO_PASS / _CONVERT) is
 * LANCZOS_TENSOR_CONVERTED: the bytes of the WHOLE output go to context scratch and one launch gathers every frame's window
 * from it; a request that changes neither axis gathers from the caller's frames, with no scratch and no copy (RandomCrop +
 * flip + ToTensor + Normalize of frames already at size).  Forced LANCZOS_RESIZE_FUSED is LANCZOS_ERR_UNSUPPORTED where the
 * crops plan is not fused.  lanczos_last_tensor_route and lanczos_last_kernel report as for a view. */
typedef struct lanczos_resize_crops {
    int32_t w, h;               /* 1..out_w, 1..out_h: the size of every frame's window */
    const int32_t* d_origin;    /* `frames` pairs (x0, y0) in output pixels of the full request; 4-byte aligned */
    int32_t reserved[4];        /* must be 0 */
} lanczos_resize_crops;
/* Host only; d_origin is not read.  LANCZOS_ERR_BAD_ARG: what lanczos_resize_validate refuses, a null struct, w or h below 1
 * or above the output, a null or misaligned d_origin, non-zero reserved words. */
int lanczos_resize_crops_validate(const lanczos_resize_desc* d, const lanczos_resize_crops* crops);
/* lanczos_resize_plan_host_ex for a crops request; d_origin is not read.  inner.ring_rows and inner.stage_dw are the largest
 * lanczos_resize_window_plan_host reports for the window (x0, y0, w, h) over every legal origin, stage_rows and lds_bytes
 * follow from them, and K, strips, rows_per_chunk and chunks are the window's at any origin.  fused = 0 where those maxima do
 * not fit, even if the window at some origins would.  mid_row0 / mid_rows are the whole output's. */
int lanczos_resize_crops_plan_host(const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                   const lanczos_resize_crops* crops, int frames, lanczos_resize_plan_ex* out);
/* Host only: lanczos_resize_crops_validate, then lanczos_resize_tensor_view_validate with (w, h) as the frame. */
int lanczos_resize_tensor_crops_validate(const lanczos_resize_desc* d, const lanczos_resize_crops* crops,
                                         const lanczos_tensor_view* v);
/* As lanczos_resize_tensor_view_device with (w, h) as the frame; d_lut, d_flip and d_origin are device pointers. */
int lanczos_resize_tensor_crops_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                       const lanczos_resize_crops* crops, const lanczos_tensor_view* v, const void* d_in,
                                       void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride, void* stream);
/* Host buffers, a HOST table, a HOST flip array and HOST origins (`frames` pairs in crops->d_origin); synchronous.  An origin
 * outside [0, out_w - w] x [0, out_h - h] is LANCZOS_ERR_BAD_ARG here: the host array can be validated, so it is not clamped. */
int lanczos_resize_tensor_crops_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                     const lanczos_resize_crops* crops, const lanczos_tensor_view* v, const void* in, void* out,
                                     int frames);

/* ---- resize from planar (CHW) and row-pitched sources without a repack ----
 * Every entry above reads `channels` interleaved samples with tightly packed rows.  A source layout beside the descriptor says
 * where the samples lie instead: sample (y, x, c) of frame f is at byte
 *   f * in_frame_stride + c * chan_stride + y * row_stride + x * pix_stride
 * of d_in (B = bytes per sample, C = channels).  Two shapes are accepted:
 *   interleaved, pitched   pix_stride = C * B, chan_stride = B, row_stride >= in_w * C * B and a multiple of B.  Every sample
 *                          type (8-bit, LANCZOS_RESIZE_ALPHA, _U16, _F32); a float source keeps its multiple-of-4 rule for base
 *                          and strides, a 16-bit one its multiple-of-2 rule.
 *   planar                 pix_stride = 1, row_stride >= in_w, chan_stride >= (in_h - 1) * row_stride + in_w.  8-bit samples
 *                          only, LANCZOS_RESIZE_ALPHA included; base and strides may have any residue.  One channel, planar,
 *                          is the interleaved shape.  A planar _U16 or _F32 source is LANCZOS_ERR_UNSUPPORTED: those types
 *                          resize every channel as an independent plane, so such a source already is frames * C one-channel
 *                          frames (channels = 1, in_frame_stride = chan_stride) for the entries above.
 * Everything else, and a non-zero reserved word, is LANCZOS_ERR_BAD_ARG: no negative strides, no layout per frame.
 * in_frame_stride = 0 is the layout's own extent: in_h * row_stride (interleaved), channels * chan_stride (planar); a non-zero
 * stride below that extent is LANCZOS_ERR_BAD_ARG.
 * THE CONTRACT: the result is what the entry without a source stores for the same descriptor, options, window, view and crops
 * when it is given the tightly packed interleaved copy of the source -- byte for byte, word for word, nothing else written.
 * The same tables and arithmetic run; only the place a source byte is fetched from changes.  No byte outside [frame base
 * rounded down to a dword, frame end rounded up to a dword) is read, and bytes the layout does not name never reach a result.
 * The frame END is: planar, the last byte the layout names (the padding behind the last row of the last plane is never read);
 * interleaved, base + in_h * row_stride -- the fused kernel's range check covers whole pitched rows, so EVERY frame, the last
 * one included, must hold its full in_h * row_stride bytes.  A region that starts x0 pixels into the rows of a larger surface and
 * ends in the surface's last row passes the surface's end by x0 * C * B bytes: the allocation has to cover them (they never
 * reach a result).
 * Routes (lanczos_last_source_route): LANCZOS_SOURCE_DIRECT, the resize kernel reads the caller's memory -- the fused kernel,
 * for a pitched interleaved source of any sample type (with a window, a view or crops) and for a planar 8-bit source of 3 or 4
 * channels (bytes out or a tensor; planar instances of their own); a tightly packed interleaved
 * source is DIRECT on every route, being the call without a source.  LANCZOS_SOURCE_PACKED, everything else: the two-pass
 * kernels, one pass, LANCZOS_FILTER_NEAREST, the copies, reducing_gap, oversize frames, a planar source with crops (and a
 * LANCZOS_RESIZE_ALPHA one whose row pitch is no multiple of 4 with crops), forced LANCZOS_RESIZE_TWO_PASS, and any source that
 * is not tightly packed under forced LANCZOS_RESIZE_CONVERT (the A/B of the direct staging): one streaming
 * launch (k_rs_pack_source) gathers the frames tightly packed into context scratch and the request runs on that block.  The
 * block lives as the other scratch of a context does: one stream at a time per context, and a captured launch pins it. */
typedef struct lanczos_resize_source {
    int64_t row_stride, chan_stride;   /* bytes */
    int32_t pix_stride;                /* bytes */
    int32_t reserved[3];               /* must be 0 */
} lanczos_resize_source;
#define LANCZOS_SOURCE_INTERLEAVED 0
#define LANCZOS_SOURCE_PLANAR 1
#define LANCZOS_SOURCE_DIRECT 1
#define LANCZOS_SOURCE_PACKED 2
/* Host only: the tight layout of that kind for d's source frame. */
int lanczos_resize_source_init(lanczos_resize_source* src, const lanczos_resize_desc* d, int layout);
/* Host only.  NULL validates as the call without a source does. */
int lanczos_resize_source_validate(const lanczos_resize_desc* d, const lanczos_resize_source* src);
/* lanczos_resize_window_device with a source layout (src NULL: exactly that call). */
int lanczos_resize_source_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                 const lanczos_resize_window* win, const lanczos_resize_source* src, const void* d_in,
                                 void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride, void* stream);
/* lanczos_resize_tensor_view_device (crops NULL) or lanczos_resize_tensor_crops_device (win NULL) with a source layout; win
 * together with crops is LANCZOS_ERR_BAD_ARG.  src NULL: exactly those calls. */
int lanczos_resize_tensor_source_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                        const lanczos_resize_window* win, const lanczos_resize_crops* crops,
                                        const lanczos_resize_source* src, const lanczos_tensor_view* v, const void* d_in,
                                        void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride, void* stream);
/* Host buffers: `frames` frames back to back in the described layout (the layout's own extent apart); synchronous.  Otherwise as
 * lanczos_resize_window_host and lanczos_resize_tensor_view_host / lanczos_resize_tensor_crops_host. */
int lanczos_resize_source_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                               const lanczos_resize_window* win, const lanczos_resize_source* src, const void* in, void* out,
                               int frames);
int lanczos_resize_tensor_source_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                      const lanczos_resize_window* win, const lanczos_resize_crops* crops,
                                      const lanczos_resize_source* src, const lanczos_tensor_view* v, const void* in, void* out,
                                      int frames);
/* LANCZOS_SOURCE_DIRECT / LANCZOS_SOURCE_PACKED of the last call that had a source and returned LANCZOS_OK, 0 before any. */
int lanczos_last_source_route(const lanczos_ctx* ctx);

/* ---- resize into planar (CHW) and row-pitched destinations without a repack ----
 * The byte, 16-bit-sample and float-sample entries above store `channels` interleaved samples with tightly packed rows.  A
 * destination layout beside the descriptor says where the samples go instead, the mirror of lanczos_resize_source.  With (w, h)
 * the window's extent (win NULL: the whole output), sample (y, x, c) of frame f goes to byte
 *   f * out_frame_stride + c * chan_stride + y * row_stride + x * pix_stride
 * of d_out (B = bytes per sample, C = channels).  Two shapes are accepted:
 *   interleaved, pitched   pix_stride = C * B, chan_stride = B, row_stride >= w * C * B and a multiple of B.  Every sample type
 *                          (8-bit, LANCZOS_RESIZE_ALPHA, _U16, _F32); floats keep their multiple-of-4 rule for base and strides,
 *                          16-bit samples their multiple-of-2 rule.
 *   planar                 pix_stride = 1, row_stride >= w, chan_stride >= (h - 1) * row_stride + w.  8-bit samples only,
 *                          LANCZOS_RESIZE_ALPHA included; base, strides and frame stride may have any residue.  One channel,
 *                          planar, is the interleaved shape.  Planar _U16 / _F32 is LANCZOS_ERR_UNSUPPORTED, for the reason the
 *                          source gives: the caller already has frames * C one-channel frames.
 * Everything else, and a non-zero reserved word, is LANCZOS_ERR_BAD_ARG.  out_frame_stride = 0 is the layout's own extent:
 * h * row_stride (interleaved), C * chan_stride (planar); a non-zero stride below the last named byte + 1 is LANCZOS_ERR_BAD_ARG.
 * dst NULL is exactly lanczos_resize_source_device; a tightly packed interleaved dst resolves to no destination, as a tight
 * source does.
 * THE CONTRACT: the named bytes are, byte for byte and word for word, what lanczos_resize_source_device stores for the same
 * descriptor, options, window and source into a tightly packed interleaved frame.  EVERY BYTE THE LAYOUT DOES NOT NAME KEEPS ITS
 * CONTENTS: row padding, plane padding, the gaps between frames and the bytes around the buffer.  The padding behind the last
 * row need not be allocated.  Every dword store of the destination's own code goes to a dword-aligned address and covers named
 * bytes only; the partial dwords at the ends of a row go out as bytes.
 * Routes (lanczos_last_dest_route): LANCZOS_DEST_DIRECT, the resize kernel stored into the caller's layout itself -- the fused
 * kernel, into pitched interleaved rows of every sample type (the pitch is an argument every instance already has) and into
 * planes of 3 or 4 8-bit channels (planar-out instances of their own), with a window and from an
 * interleaved, pitched or planar source; a tightly packed interleaved destination is DIRECT on every route, being the call
 * without one.  LANCZOS_DEST_UNPACKED, everything else: the two-pass kernels, one pass, LANCZOS_FILTER_NEAREST, the copies,
 * reducing_gap, frames whose named span is 2^31 bytes or more, a planar destination from LANCZOS_RESIZE_ALPHA rows whose pitch
 * is no multiple of 4, forced LANCZOS_RESIZE_TWO_PASS, and any destination that is not tightly packed under forced
 * LANCZOS_RESIZE_CONVERT (the A/B of the direct stores).  The request then stores its tightly packed result in a scratch block of the context, and one streaming launch
 * (k_rs_unpack_dest) scatters it.  The block lives as the other scratch of a context does.  There is no tensor form (a tensor
 * view carries strides already), no channel map, no flips and no crop origins here. */
typedef struct lanczos_resize_dest {
    int64_t row_stride, chan_stride;   /* bytes */
    int32_t pix_stride;                /* bytes */
    int32_t reserved[3];               /* must be 0 */
} lanczos_resize_dest;
#define LANCZOS_DEST_INTERLEAVED 0
#define LANCZOS_DEST_PLANAR 1
#define LANCZOS_DEST_DIRECT 1     /* the resize kernel stored into the caller's layout itself */
#define LANCZOS_DEST_UNPACKED 2   /* packed result in context scratch, then one scatter launch */
/* Host only: the tight layout of that kind for the window's frame (win NULL: d's whole output). */
int lanczos_resize_dest_init(lanczos_resize_dest* dst, const lanczos_resize_desc* d, const lanczos_resize_window* win, int layout);
/* Host only.  NULL validates as the call without a destination does. */
int lanczos_resize_dest_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win, const lanczos_resize_dest* dst);
/* lanczos_resize_source_device with a destination layout (dst NULL: exactly that call; src may be NULL). */
int lanczos_resize_dest_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                               const lanczos_resize_window* win, const lanczos_resize_source* src, const lanczos_resize_dest* dst,
                               const void* d_in, void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride,
                               void* stream);
/* Host buffers; synchronous.  `out` holds `frames` frames the layout's own extent apart, the last one up to its last named byte;
 * the bytes of `out` the layout does not name keep their contents. */
int lanczos_resize_dest_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                             const lanczos_resize_window* win, const lanczos_resize_source* src, const lanczos_resize_dest* dst,
                             const void* in, void* out, int frames);
/* LANCZOS_DEST_DIRECT / LANCZOS_DEST_UNPACKED of the last call that had a destination and returned LANCZOS_OK, 0 before any. */
int lanczos_last_dest_route(const lanczos_ctx* ctx);

/* ---- resize 16-bit and float frames straight into normalised tensors ----
 * The tensor entries above are 8-bit only: their table has an entry per sample value.  LANCZOS_RESIZE_U16 (Pillow's I;16) and
 * LANCZOS_RESIZE_F32 (mode F) frames have this entry instead, which computes the normalisation where the sample is stored.  With
 * P(f, y, x, c) the sample lanczos_resize_window_device stores for the same descriptor, options and window (a uint16 or a float),
 * (w, h) the window's extent and m_f = (flip ^ d_flip[f]) & 3:
 *   out[f][oc * chan_stride + Y * row_stride + X * pix_stride] =
 *       cvt( ((float)P(f, y, x, src_channel[oc]) / div[oc] - mean[oc]) / std[oc] )
 *   X = (m_f & 1) ? w - 1 - x : x        Y = (m_f & 2) ? h - 1 - y : y
 * (float)P is exact for a 16-bit sample and the identity for a float one.  The division, the subtraction and the division are
 * three separately rounded IEEE binary32 operations, round to nearest, denormals kept: no fused multiply-add, no reciprocal, no
 * folded scale -- those differ from the three operations on most 16-bit values.  cvt is the identity for LANCZOS_TENSOR_F32 and
 * what lanczos_tensor_lut_convert16 computes for LANCZOS_TENSOR_BF16 / _F16: round to nearest even, float16 subnormals kept,
 * overflow to +-inf, a NaN to some NaN.  With `resized` Pillow's own output this is, bit for bit, torch's
 * torch.from_numpy(resized).permute(...).float().div(div).sub(mean).div(std)[.to(dtype)] on the CPU.
 * div, mean and std are indexed by the OUTPUT channel and passed by value: a captured call bakes them in.  They are not
 * inspected -- the arithmetic is defined for every float.  The channel map, the flips, the strides (in elements), the overlap
 * rule, the extent, the minimum out_frame_stride and d_flip's lifetime are lanczos_tensor_view's; elements the strides do not
 * name are not written.
 * opts: a box; a reducing_gap stays refused for wide samples.  win: optional.  src: optional, a row-pitched interleaved source;
 * a planar source of wide samples stays LANCZOS_ERR_UNSUPPORTED.  No crop origins.  LANCZOS_FILTER_NEAREST with _U16 stays
 * LANCZOS_ERR_UNSUPPORTED.
 * Routes (lanczos_last_tensor_route): LANCZOS_TENSOR_FUSED exactly when lanczos_resize_window_plan_host says the sample request
 * is fused and one element frame spans less than 2^31 bytes: the fused kernel's vertical pass applies the operations to the sum
 * it holds and stores the element.  Everything else (two passes, one pass, tall frames, LANCZOS_FILTER_NEAREST on floats, the
 * plain copy, forced LANCZOS_RESIZE_TWO_PASS / _CONVERT, larger element frames) is LANCZOS_TENSOR_CONVERTED: the samples go
 * tightly packed to context scratch and one streaming launch (k_rs_to_tensor_norm) follows; a request that changes neither axis
 * and has no window converts straight from the caller's frames.  lanczos_last_kernel and lanczos_resize_force apply as for the
 * other tensor entries. */
#define LANCZOS_TENSOR_F32 3   /* an element format beside LANCZOS_TENSOR_BF16 / LANCZOS_TENSOR_F16 */
#define LANCZOS_TENSOR_CHW 0   /* the layouts of lanczos_tensor_norm_init */
#define LANCZOS_TENSOR_HWC 1
typedef struct lanczos_tensor_norm {
    float div[4], mean[4], std[4];                 /* per output channel; entries beyond out_channels are not read */
    int64_t chan_stride, row_stride, pix_stride;   /* in elements, each > 0 */
    int32_t format;           /* LANCZOS_TENSOR_F32, LANCZOS_TENSOR_BF16 or LANCZOS_TENSOR_F16 */
    int32_t out_channels;     /* 1 .. d->channels */
    int32_t src_channel[4];   /* as lanczos_tensor_view */
    int32_t flip;             /* bit 0: mirror x, bit 1: mirror y -- applied to every frame */
    const uint8_t* d_flip;    /* NULL, or one byte per frame (same bits), XORed with `flip`; read when the kernels run */
    int32_t reserved[4];      /* must be 0 */
} lanczos_tensor_norm;
/* Host only: the identity over every channel, the tight LANCZOS_TENSOR_CHW or _HWC strides of d's whole output, no flips,
 * div = 1, mean = 0, std = 1.  LANCZOS_ERR_BAD_ARG: a null n, what lanczos_resize_validate refuses, an unknown format or layout. */
int lanczos_tensor_norm_init(lanczos_tensor_norm* n, const lanczos_resize_desc* d, int format, int layout);
/* Host only.  LANCZOS_ERR_UNSUPPORTED: an 8-bit descriptor (the table entries above serve those).  LANCZOS_ERR_BAD_ARG: an
 * unknown format and everything lanczos_resize_tensor_view_validate refuses, the table pointer aside. */
int lanczos_resize_tensor_norm_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win,
                                        const lanczos_tensor_norm* n);
/* Device buffers, asynchronous on `stream`: d_in and in_frame_stride are multiples of the sample width, d_out and
 * out_frame_stride (bytes; 0 = the frame's extent) multiples of the element width. */
int lanczos_resize_tensor_norm_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                      const lanczos_resize_window* win, const lanczos_resize_source* src,
                                      const lanczos_tensor_norm* n, const void* d_in, void* d_out, int frames,
                                      size_t in_frame_stride, size_t out_frame_stride, void* stream);
/* Host buffers and a HOST flip array (`frames` bytes, or NULL); source frames the layout's extent apart, element frames one
 * extent apart; synchronous.  Elements of `out` the strides do not name keep their contents. */
int lanczos_resize_tensor_norm_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                    const lanczos_resize_window* win, const lanczos_resize_source* src,
                                    const lanczos_tensor_norm* n, const void* in, void* out, int frames);

/* ---- resize YCbCr frames (I420, 4:2:2, 4:4:4 planes, NV12, NV21) straight into RGB bytes and tensors ----
 * A frame holds in_w x in_h luma samples and two chroma planes subsampled by 2^sub_x x 2^sub_y (sub_x, sub_y 0 or 1) of
 * cw x ch samples, cw = (in_w + sub_x) >> sub_x, ch = (in_h + sub_y) >> sub_y: centre siting (JPEG, MPEG-1), the full chroma
 * plane covers the full luma plane, odd sizes included.  THE CONTRACT is a composition of Pillow calls, byte for byte:
 *   Yo  = Image.fromarray(Y,  "L").resize((out_w, out_h), filt, box=bl, reducing_gap=g)
 *   Cbo = Image.fromarray(Cb, "L").resize((out_w, out_h), filt, box=bc, reducing_gap=g)
 *   Cro = Image.fromarray(Cr, "L").resize((out_w, out_h), filt, box=bc, reducing_gap=g)
 *   rgb = Image.merge("YCbCr", (Yo, Cbo, Cro)).convert("RGB")
 * bl is the request's box in luma pixels (opts NULL: the whole frame) and bc is bl with x times 2^-sub_x and y times 2^-sub_y,
 * computed on the doubles of bl, so exactly.  Every plane obeys the rules of a one-channel resize on its own: an axis of a plane
 * that keeps its size over the whole axis skips its pass (4:2:0 with out == in copies luma and still resizes chroma), and a
 * reducing_gap reduces each plane as Pillow would reduce that plane.  The window is the same output rectangle for the three
 * planes.  Left-sited chroma (MPEG-2) would need a negative box offset, which Pillow refuses: it is not expressed here.
 * The descriptor describes the RGB result: channels = 3, in_w x in_h the luma size, every filter (LANCZOS_FILTER_NEAREST
 * included) and every a.  LANCZOS_RESIZE_ALPHA, _U16 or _F32 in its flag word is LANCZOS_ERR_UNSUPPORTED (wide chroma, P010 /
 * P016 and planes of 16-bit words, has an entry of its own: lanczos_resize_ycc16, below).  There is no crop origin per frame
 * and no lanczos_resize_dest on these entries.
 * The colour conversion is a table the caller passes, int32 t[3][3][256]:
 *   out[c] = clip8((t[c][0][y] + t[c][1][cb] + t[c][2][cr]) >> 6)           (>> arithmetic, clip8 to 0 .. 255)
 * Its indices are bytes, so no content can address out of bounds; entries must keep the sum inside int32.  lanczos_ycc_table fills
 * it for three standards.  LANCZOS_YCC_JFIF is Pillow's convert("RGB") exactly: t[c][0][y] = 64 y and
 * T(k, i) = (int)(k * (i - 128) * 64 + 0.5) (double, truncation toward zero) with k = 1.402 (R from Cr), -0.34414 and -0.71414
 * (G from Cb, Cr), 1.772 (B from Cb).  LANCZOS_YCC_BT601 / _BT709 are the limited-range matrices: ky = 255/219, kc = 255/224,
 * (Kr, Kb) = (0.299, 0.114) / (0.2126, 0.0722), Kg = 1 - Kr - Kb; luma entries (int)(ky (i - 16) 64 + 0.5) + 32 (the shift
 * then rounds), chroma entries (int)(k (i - 128) 64 + 0.5) with k = 2 (1 - Kr) kc (R from Cr), -2 (1 - Kb) Kb / Kg kc and
 * -2 (1 - Kr) Kr / Kg kc (G from Cb, Cr), 2 (1 - Kb) kc (B from Cb).  Their result is within 1 of the float64 matrix result
 * rounded to nearest and clipped.  Any other matrix or channel order (full-range BT.709, BGR rows) is the caller's own table.
 * Routes: the planes are resized by the one-channel requests of lanczos_resize_source_device (same routes, same kernels:
 * lanczos_resize_window_plan_host of the one-channel request of a plane says which) into context scratch, and one streaming
 * launch (k_rs_ycc_merge) converts the three planes into RGB bytes or tensor elements.  The chroma of a planar layout takes two
 * resize calls; the interleaved chroma of NV12 / NV21 is split into planes by one streaming launch (k_rs_ycc_split) and then
 * takes one.  lanczos_resize_force applies to every plane.  The scratch lives as the other scratch of a context does: one stream
 * at a time per context, a captured launch pins its block, a captured graph must not outlive its context. */
#define LANCZOS_YCC_PLANAR 0   /* three planes: Y at the frame base, Cb at cb_offset, Cr at cr_offset */
#define LANCZOS_YCC_NV12 1     /* Y plane, then one plane of interleaved (Cb, Cr) pairs at cb_offset; sub_x must be 1 */
#define LANCZOS_YCC_NV21 2     /* ... of (Cr, Cb) pairs */
#define LANCZOS_YCC_JFIF 0     /* the standards of lanczos_ycc_table */
#define LANCZOS_YCC_BT601 1
#define LANCZOS_YCC_BT709 2
typedef struct lanczos_ycc_source {
    int64_t y_row_stride, c_row_stride;   /* bytes; of NV12 / NV21 c_row_stride is that of the interleaved rows (>= 2 cw) */
    int64_t cb_offset, cr_offset;         /* bytes from the frame base to the first chroma sample; NV12 / NV21: both the same */
    int32_t layout, sub_x, sub_y;
    int32_t reserved[5];                  /* must be 0 */
} lanczos_ycc_source;
/* Host only: the tight layout -- Y, then Cb, then Cr (or the interleaved plane), rows packed.  LANCZOS_ERR_BAD_ARG as validate. */
int lanczos_ycc_source_init(lanczos_ycc_source* src, const lanczos_resize_desc* d, int layout, int sub_x, int sub_y);
/* Host only.  LANCZOS_ERR_UNSUPPORTED: LANCZOS_RESIZE_ALPHA, _U16 or _F32 in d.  LANCZOS_ERR_BAD_ARG: a null pointer, what
 * lanczos_resize_validate refuses, channels other than 3, an unknown layout, a subsampling other than 0 or 1, NV12 / NV21 with
 * sub_x != 1 or with two different offsets, a row stride below a plane's row (or above 2^40), a negative offset, planes that
 * overlap (a plane is its rows times its row stride: every plane must hold its full pitched rows), a non-zero reserved word.
 * The frame's extent is the end of its last plane: in_frame_stride 0 stands for it, a smaller one is LANCZOS_ERR_BAD_ARG. */
int lanczos_ycc_source_validate(const lanczos_resize_desc* d, const lanczos_ycc_source* src);
/* Host only: t[3][3][256] of a standard (above).  LANCZOS_ERR_BAD_ARG: a null t, an unknown standard. */
int lanczos_ycc_table(int standard, int32_t* t);
/* Device buffers, asynchronous on `stream`.  d_table: device, 3 * 3 * 256 int32, read WHEN THE KERNELS RUN.  d_in: any byte
 * address, frames in_frame_stride bytes apart (any residue).  d_out: tightly packed interleaved RGB bytes of the window (win NULL:
 * the whole output), w * h * 3 per frame; d_out and out_frame_stride (0 = w * h * 3 rounded up to a multiple of 4) must be
 * multiples of 4, else LANCZOS_ERR_BAD_ARG.  Nothing is written past a frame's w * h * 3 bytes.  opts and win may be NULL. */
int lanczos_resize_ycc_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                              const lanczos_resize_window* win, const lanczos_ycc_source* src, const int32_t* d_table,
                              const void* d_in, void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride,
                              void* stream);
/* ... into tensor elements: with (R, G, B) the bytes above as source channels 0, 1, 2, everything is lanczos_tensor_view's
 * contract and lanczos_resize_tensor_view_device's rules (table by output channel, strides in elements, channel map, flip and
 * d_flip, the overlap rule, the extent, elements the strides do not name left untouched). */
int lanczos_resize_ycc_tensor_device(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                     const lanczos_resize_window* win, const lanczos_ycc_source* src, const int32_t* d_table,
                                     const lanczos_tensor_view* v, const void* d_in, void* d_out, int frames,
                                     size_t in_frame_stride, size_t out_frame_stride, void* stream);
/* Host buffers, a HOST table (and for the tensor form a HOST element table and HOST flips in v); synchronous.  Frames lie back
 * to back: the source's extent apart, w * h * 3 bytes apart (no padding), element frames one extent apart.  Elements of `out` the
 * strides do not name keep their contents. */
int lanczos_resize_ycc_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                            const lanczos_resize_window* win, const lanczos_ycc_source* src, const int32_t* table, const void* in,
                            void* out, int frames);
int lanczos_resize_ycc_tensor_host(lanczos_ctx* ctx, const lanczos_resize_desc* d, const lanczos_resize_opts* opts,
                                   const lanczos_resize_window* win, const lanczos_ycc_source* src, const int32_t* table,
                                   const lanczos_tensor_view* v, const void* in, void* out, int frames);
/* What the last successful lanczos_resize_ycc_* call on the context launched: the LANCZOS_KERNEL_* of the luma resize and of
 * the chroma resize (LANCZOS_KERNEL_NONE: a plain copy), whether k_rs_ycc_split ran, and the number of launches (resize
 * kernels, copies, split and merge).  All zero before any.  LANCZOS_ERR_BAD_ARG: a null pointer. */
typedef struct lanczos_ycc_info {
    int32_t luma_kernel, chroma_kernel, split, launches;
    int32_t reserved[4];
} lanczos_ycc_info;
int lanczos_last_ycc_info(const lanczos_ctx* ctx, lanczos_ycc_info* info);

/* ---- resize INTO YCbCr frames (I420, 4:2:2, 4:4:4 planes, NV12, NV21) from YCbCr frames or from packed RGB bytes ----
 * The mirror of the section above: a lanczos_ycc_dest says where the planes of a result frame go.  The stored frame is the
 * window (win NULL: the whole output) of w x h luma samples; its chroma planes hold ocw x och samples, ocw = (w + sub_x) >> sub_x,
 * och = (h + sub_y) >> sub_y, with the destination's subsampling.  THE CONTRACT is a composition of Pillow calls, byte for byte.
 * FROM YCbCr (src given): no colour conversion and no table, the planes are resized plane by plane,
 *   Yo  = Image.fromarray(Y,  "L").resize((out_w, out_h), filt, box=bl, reducing_gap=g)
 *   Cbo = Image.fromarray(Cb, "L").resize((OCW, OCH), filt, box=bc, reducing_gap=g)             (Cr likewise)
 * with OCW = (out_w + sub_x) >> sub_x, OCH = (out_h + sub_y) >> sub_y the full output's chroma size under the DESTINATION's
 * subsampling, and bl, bc the boxes of the section above: bc is bl scaled by the SOURCE's subsampling on the doubles.  Source and
 * destination subsampling and layout are independent (4:2:0 -> 4:4:4, NV12 -> I420, NV21 -> NV12 are all requests).  Every plane
 * obeys the one-channel rules on its own: an axis that keeps its size over its whole span is not filtered, so NV12 -> I420 at the
 * same size is a pure re-layout.  A window (x0, y0, w, h) is in luma output pixels; x0 must be a multiple of 2^sub_x and y0 of
 * 2^sub_y of the destination, else LANCZOS_ERR_BAD_ARG; the chroma window is (x0 >> sub_x, y0 >> sub_y, ocw, och), which then lies
 * inside the full chroma plane for every w and h.
 * FROM RGB (src NULL): the frames at `in` are tightly packed interleaved 8-bit RGB, as lanczos_resize_window_device takes them,
 *   rgb = Image.fromarray(x, "RGB").resize((out_w, out_h), filt, box=b, reducing_gap=g)[.crop(window)]
 *   Y, Cb, Cr = rgb.convert("YCbCr").split()
 *   Cb, Cr = Cb.reduce((1 << sub_x, 1 << sub_y)), Cr.reduce((1 << sub_x, 1 << sub_y))          (only where sub_x or sub_y is 1)
 * The window is cut first, so any origin is legal, and the chroma blocks are those of the windowed frame.  The conversion is a
 * table the caller passes, of the form of the table above, int32 t[3][3][256]:
 *   out[c] = clip8((t[c][0][R] + t[c][1][G] + t[c][2][B]) >> 6),  c = Y, Cb, Cr        (>> arithmetic, clip8 to 0 .. 255)
 * and the chroma average is lanczos_reduce_*'s rule, ((sum + d / 2) * floor(2^24 / d)) >> 24, where d counts the 1, 2 or 4
 * converted bytes a block really holds: the last column and row of blocks of an odd frame are ragged.
 * lanczos_ycc_table_forward fills the table for the standards.  LANCZOS_YCC_JFIF is Pillow's convert("YCbCr") exactly: entries
 * (int)(k * i * 64 + 0.5) (double, truncation toward zero) with k = 0.299, 0.587, 0.114 (Y), -0.16874, -0.33126, 0.5 (Cb),
 * 0.5, -0.41869, -0.08131 (Cr), and 128 * 64 added to the R entry of Cb and of Cr (+ 128 behind the shift).  LANCZOS_YCC_BT601 /
 * _BT709 are the limited-range forward matrices with the same entry rule: Y rows k = K * 219/255, chroma rows
 * -Kr/(2(1-Kb)), -Kg/(2(1-Kb)), 1/2 (Cb) and 1/2, -Kg/(2(1-Kr)), -Kb/(2(1-Kr)) (Cr) times 224/255; the offsets 16 * 64 + 32 (Y)
 * and 128 * 64 + 32 (Cb, Cr) are folded into the R entries, so the shift rounds.  Their result is within 1 of the float64 matrix
 * result rounded to nearest and clipped.
 * A request that resizes nothing (out == in, no box, no gap, no window) is a colour conversion: k_rs_ycc_encode reads the caller's
 * frames, nothing copies them.
 * UNNAMED BYTES: every byte of the destination that the layout does not name -- row padding, gaps between planes and frames,
 * bytes around the buffer -- keeps its contents, in device and in host memory.
 * Routes.  From YCbCr, luma and planar chroma are the one-channel requests of lanczos_resize_dest_device with a pitched source and
 * a pitched destination: where the plan is fused the kernel stores into the caller's planes (LANCZOS_DEST_DIRECT), no scratch
 * and no extra pass.  For NV12 / NV21 out the two chroma planes go tight into context scratch and one streaming launch
 * (k_rs_ycc_join) interleaves them into the pitched rows; interleaved chroma in is split as above.  Fused 4:2:0 planar -> planar
 * is three launches, NV -> NV four (luma, split, one chroma call of 2 * frames frames, join).  From RGB, the resize stores tight RGB into context scratch and one
 * launch (k_rs_ycc_encode) converts, averages and stores the planes or the interleaved rows.  lanczos_resize_force applies to every
 * plane; the scratch lives as the other scratch of a context does. */
typedef struct lanczos_ycc_dest {
    int64_t y_row_stride, c_row_stride;   /* bytes; of NV12 / NV21 c_row_stride is that of the interleaved rows (>= 2 ocw) */
    int64_t cb_offset, cr_offset;         /* bytes from the frame base to the first chroma sample; NV12 / NV21: both the same */
    int32_t layout, sub_x, sub_y;         /* LANCZOS_YCC_PLANAR / _NV12 / _NV21; 0 or 1 */
    int32_t reserved[5];                  /* must be 0 */
} lanczos_ycc_dest;
/* Host only: the tight layout of the stored frame (win NULL: the whole output) -- Y, then Cb, then Cr (or the interleaved
 * plane), rows packed.  Only the window's size is read, not its origin.  LANCZOS_ERR_BAD_ARG as validate otherwise. */
int lanczos_ycc_dest_init(lanczos_ycc_dest* dst, const lanczos_resize_desc* d, const lanczos_resize_window* win, int layout,
                          int sub_x, int sub_y);
/* Host only: the rules of lanczos_ycc_source_validate, mirrored.  LANCZOS_ERR_UNSUPPORTED: LANCZOS_RESIZE_ALPHA, _U16 or _F32
 * in d.  LANCZOS_ERR_BAD_ARG: a null pointer, what lanczos_resize_validate or lanczos_resize_window_validate refuses, channels
 * other than 3, an unknown layout, a subsampling other than 0 or 1, NV12 / NV21 with sub_x != 1 or with two different offsets, a
 * row stride below a plane's row (or above 2^40), a negative offset, planes that overlap (a plane is its rows times its row
 * stride), a window origin that is no multiple of the subsampling (the rule of a YCbCr source; lanczos_resize_ycc_out does not
 * apply it to RGB frames), a non-zero reserved word.  Planes may lie at any byte address with any pitch.  The frame's extent is
 * the end of its last plane: out_frame_stride 0 stands for it; a stride need only clear the last byte the layout names. */
int lanczos_ycc_dest_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win, const lanczos_ycc_dest* dst);
/* Host only: the forward table t[3][3][256] of a standard (above).  LANCZOS_ERR_BAD_ARG: a null t, an unknown standard. */
int lanczos_ycc_table_forward(int standard, int32_t* t);
#define LANCZOS_MEM_DEVICE 0   /* in, out and table are device pointers; asynchronous on `stream` */
#define LANCZOS_MEM_HOST 1     /* ... host pointers; synchronous; frames lie one extent apart (the frame strides must be 0) */
typedef struct lanczos_ycc_out_request {
    const lanczos_resize_desc* d;      /* channels = 3; in_w x in_h the luma or RGB size.  _ALPHA, _U16, _F32: UNSUPPORTED */
    const lanczos_resize_opts* opts;   /* may be NULL */
    const lanczos_resize_window* win;  /* may be NULL */
    const lanczos_ycc_source* src;     /* NULL: the frames at `in` are packed RGB */
    const lanczos_ycc_dest* dst;
    const int32_t* table;              /* from RGB: the forward table, read WHEN THE KERNELS RUN; from YCbCr it must be NULL */
    const void* in;                    /* any byte address */
    void* out;                         /* any byte address */
    int32_t frames;
    int32_t memory;                    /* LANCZOS_MEM_DEVICE or LANCZOS_MEM_HOST */
    size_t in_frame_stride;            /* bytes, any residue; 0: the source's extent, or in_w * in_h * 3 */
    size_t out_frame_stride;           /* bytes, any residue; 0: the destination's extent */
    void* stream;                      /* LANCZOS_MEM_DEVICE only */
    int32_t reserved[4];               /* must be 0 */
} lanczos_ycc_out_request;
/* The one launching entry.  LANCZOS_ERR_BAD_ARG: a null request, d, dst, in or out, frames < 1, an unknown memory, a table with
 * src or none without, a table off a dword, what the validations above refuse, frame strides below the layouts' needs. */
int lanczos_resize_ycc_out(lanczos_ctx* ctx, const lanczos_ycc_out_request* rq);
/* What the last successful lanczos_resize_ycc_out on the context launched.  From YCbCr: the LANCZOS_KERNEL_* of the luma and of
 * the chroma resize (LANCZOS_KERNEL_NONE: a copy), whether k_rs_ycc_split and k_rs_ycc_join ran; from RGB: luma_kernel is the
 * kernel of the RGB resize (LANCZOS_KERNEL_NONE: a copy, a crop, or nothing at all), chroma_kernel LANCZOS_KERNEL_NONE, encode 1.
 * launches counts everything: resize kernels, copies, split, join, encode.  All zero before any call. */
typedef struct lanczos_ycc_out_info {
    int32_t luma_kernel, chroma_kernel, split, join, encode, launches;
    int32_t reserved[2];
} lanczos_ycc_out_info;
int lanczos_last_ycc_out_info(const lanczos_ctx* ctx, lanczos_ycc_out_info* info);

/* ---- resize YCbCr frames of 16-bit words (P010, P016, P210, planar 10 / 12 / 16-bit) into YCbCr, RGB words and tensors ----
 * The two sections above are 8-bit.  This one entry serves frames whose samples are uint16 words holding any depth from 8 to 16
 * bits, LSB-aligned (yuv420p10le) or MSB-aligned (P010): 4:2:0, 4:2:2 and 4:4:4 planes, and interleaved chroma of word pairs in
 * either order.  The descriptor has channels = 3 and LANCZOS_RESIZE_U16; in_w x in_h is the luma size.  THE CONTRACT for the
 * planes is Pillow's mode I;16 on the raw words, plane by plane:
 *   Yo  = Image.fromarray(Y,  "I;16").resize((out_w, out_h), filt, box=bl)
 *   Cbo = Image.fromarray(Cb, "I;16").resize((CW, CH), filt, box=bc)                            (Cr likewise)
 * bl is the request's box in luma pixels and bc is bl scaled by the SOURCE's subsampling on its doubles (centre siting, odd sizes
 * included), the rule of the 8-bit entries.  (CW, CH) is (out_w, out_h) for RGB and tensor output and the full output's chroma
 * size under the DESTINATION's subsampling for YCbCr output, whose window rule is lanczos_ycc_dest_validate's: origins are
 * multiples of the destination's subsampling.  An axis that keeps its size over its whole span is not filtered: P010 -> planar at
 * the same even size is a pure re-layout and runs no resize kernel.
 * THE I;16 STORE IS PART OF THE CONTRACT: a rounded sum below 0 stores 0, and one above 65535 stores 0xFF00 | low byte -- not
 * 65535.  MSB-aligned full-range content (words near 65535 beside words near 0) hits this at every hard edge, exactly as Pillow
 * does; limited-range and LSB-aligned content stays clear of it.
 * What wide requests refuse stays refused: a reducing_gap is LANCZOS_ERR_BAD_ARG (Pillow's reduce refuses I;16) and
 * LANCZOS_FILTER_NEAREST is LANCZOS_ERR_UNSUPPORTED.
 * THE OUTPUT KIND is decided by which pointers of the request are set:
 *   dst alone          wide YCbCr frames in dst's layout; no colour conversion.
 *   matrix alone       packed RGB of 16-bit samples, w * h * 3 words per frame (the window's; win NULL: the whole output); `out`
 *                      and out_frame_stride (0 = w * h * 6 rounded up to a multiple of 4) must be multiples of 4.
 *   matrix and norm    tensor elements: cvt(((float)RGB16[src_channel[oc]] / div[oc] - mean[oc]) / std[oc]), lanczos_tensor_norm's
 *                      contract with (R, G, B) the words above as source channels 0, 1, 2 -- the channel map, flips, d_flip,
 *                      strides (in elements), the overlap rule and the extent all apply; elements the strides do not name are
 *                      left untouched.
 * Every other combination is LANCZOS_ERR_BAD_ARG.
 * THE COLOUR CONVERSION is an integer matrix passed by value (a table over words would hold 3 * 3 * 65536 entries):
 *   out[c] = clamp((k[c][0] * (y - sub[0]) + k[c][1] * (cb - sub[1]) + k[c][2] * (cr - sub[2]) + rnd) >> shift, 0, max)
 * with the sum in int64, >> an arithmetic shift and rnd = shift ? 1 << (shift - 1) : 0.  |k| < 2^24, sub and max in 0 .. 65535,
 * shift in 0 .. 30: within these bounds no content can overflow the sum.  lanczos_ycc16_matrix_init fills it for a standard
 * (LANCZOS_YCC_JFIF and _BT601: the BT.601 constants; _BT709; _BT2020: Kr 0.2627, Kb 0.0593), a depth of 8 .. 16 bits, either
 * alignment and either range, scaled to max = 65535: with unit = 2^(16 - depth) for MSB-aligned words and 1 otherwise,
 *   ky = 65535 / (luma range in words),    luma range   = (full ? 2^depth - 1 : 219 << (depth - 8)) * unit
 *   kc = 65535 / (chroma range in words),  chroma range = (full ? 2^depth - 1 : 224 << (depth - 8)) * unit
 *   sub = ((full ? 0 : 16 << (depth - 8)) * unit, 2^(depth - 1) * unit, 2^(depth - 1) * unit)
 *   R = ky y' + 2 (1 - Kr) kc cr',  G = ky y' - 2 (1 - Kb) Kb / Kg kc cb' - 2 (1 - Kr) Kr / Kg kc cr',  B = ky y' + 2 (1 - Kb) kc cb'
 * shift is the largest value <= 30 for which every entry, rounded to nearest, stays below 2^23 in magnitude, and k the real
 * coefficient times 2^shift rounded to nearest.  The unrounded integer sum then differs from the real one by at most
 * sum_j 0.5 |v_j - sub_j| / 2^shift < 0.5, so results are within 1 of the float64 matrix rounded to nearest.  Any other matrix (a
 * full-range BT.709 to 10-bit RGB, BGR rows, a pass-through) is the caller's own struct.
 * LAYOUTS are lanczos_ycc_source and lanczos_ycc_dest with every stride and offset in BYTES, validated by the functions below,
 * which mirror the 8-bit rules with these differences: the descriptor must have LANCZOS_RESIZE_U16 (else
 * LANCZOS_ERR_UNSUPPORTED; _ALPHA and _F32 too); a luma or planar chroma row is 2 w bytes, an interleaved row 4 cw bytes; every
 * stride, offset, base pointer and frame stride must be a multiple of 2, else LANCZOS_ERR_BAD_ARG.  Bytes of a destination the
 * layout does not name keep their contents, in device and in host memory.
 * Routes.  The planes are one-channel LANCZOS_RESIZE_U16 requests of lanczos_resize_dest_device with a pitched source, for YCbCr
 * output with a pitched destination too, so a fused plan stores into the caller's planes.  Interleaved chroma in is split into
 * two tight word planes by one streaming launch (k_rs_ycc_split16); interleaved chroma out is joined from two tight planes by one
 * (k_rs_ycc_join16); RGB words and elements come from one launch over the three resized planes (k_rs_ycc16_merge).  Fused 4:2:0
 * planar -> planar is 3 launches; P010 -> P010 is 4 (luma, split, one chroma call of 2 * frames frames, join); P010 -> tensor is 4
 * (luma, split, chroma, merge).  lanczos_resize_force applies to every plane; the scratch lives as the other scratch of a
 * context does.  Not here: RGB words into wide YCbCr, crop origins per frame, left-sited chroma. */
#define LANCZOS_YCC_BT2020 3   /* a standard of lanczos_ycc16_matrix_init beside LANCZOS_YCC_JFIF / _BT601 / _BT709 */
typedef struct lanczos_ycc16_matrix {
    int32_t k[3][3];      /* |k| < 2^24; rows R, G, B over (y, cb, cr) */
    int32_t sub[3];       /* 0 .. 65535, subtracted from (y, cb, cr) */
    int32_t shift;        /* 0 .. 30 */
    int32_t max;          /* 0 .. 65535 */
    int32_t reserved[4];  /* must be 0 */
} lanczos_ycc16_matrix;
/* Host only.  LANCZOS_ERR_BAD_ARG: a null m, an unknown standard, a depth outside 8 .. 16. */
int lanczos_ycc16_matrix_init(lanczos_ycc16_matrix* m, int standard, int depth, int msb_aligned, int full_range);
/* Host only.  LANCZOS_ERR_BAD_ARG: a null m, |k| >= 2^24, a sub, shift or max outside its range, a non-zero reserved word. */
int lanczos_ycc16_matrix_validate(const lanczos_ycc16_matrix* m);
/* Host only: the tight layouts in bytes, as lanczos_ycc_source_init / lanczos_ycc_dest_init give them for 8-bit frames. */
int lanczos_ycc16_source_init(lanczos_ycc_source* src, const lanczos_resize_desc* d, int layout, int sub_x, int sub_y);
int lanczos_ycc16_dest_init(lanczos_ycc_dest* dst, const lanczos_resize_desc* d, const lanczos_resize_window* win, int layout,
                            int sub_x, int sub_y);
/* Host only: the rules of lanczos_ycc_source_validate / lanczos_ycc_dest_validate with the differences above. */
int lanczos_ycc16_source_validate(const lanczos_resize_desc* d, const lanczos_ycc_source* src);
int lanczos_ycc16_dest_validate(const lanczos_resize_desc* d, const lanczos_resize_window* win, const lanczos_ycc_dest* dst);
typedef struct lanczos_ycc16_request {
    const lanczos_resize_desc* d;        /* channels = 3 with LANCZOS_RESIZE_U16; in_w x in_h the luma size */
    const lanczos_resize_opts* opts;     /* may be NULL; a box only */
    const lanczos_resize_window* win;    /* may be NULL */
    const lanczos_ycc_source* src;       /* required */
    const lanczos_ycc_dest* dst;         /* wide YCbCr out */
    const lanczos_ycc16_matrix* matrix;  /* RGB words or, with norm, tensor elements out; read when the call is made */
    const lanczos_tensor_norm* norm;     /* LANCZOS_MEM_HOST: d_flip is a host array */
    const void* in;                      /* a multiple of 2 */
    void* out;                           /* a multiple of 2 (YCbCr), of 4 (RGB words), of the element (tensor) */
    int32_t frames;
    int32_t memory;                      /* LANCZOS_MEM_DEVICE or LANCZOS_MEM_HOST */
    size_t in_frame_stride;              /* bytes, a multiple of 2; 0: the source's extent */
    size_t out_frame_stride;             /* bytes; 0: the destination's extent, w * h * 6 rounded up to 4, the elements' extent */
    void* stream;                        /* LANCZOS_MEM_DEVICE only */
    int32_t reserved[4];                 /* must be 0 */
} lanczos_ycc16_request;
/* Host only: everything lanczos_resize_ycc16 refuses from the request alone, by the code it would return -- a null request, d,
 * src, in or out, frames < 1, an unknown memory, a non-zero reserved word, an illegal combination of dst / matrix / norm, what the
 * validations above and lanczos_resize_tensor_norm_validate refuse, a reducing_gap, a base or frame stride off its multiple, a
 * frame stride with LANCZOS_MEM_HOST. */
int lanczos_ycc16_request_validate(const lanczos_ycc16_request* rq);
/* The one launching entry.  LANCZOS_MEM_HOST: synchronous, frames one extent apart (RGB words back to back). */
int lanczos_resize_ycc16(lanczos_ctx* ctx, const lanczos_ycc16_request* rq);
/* What the last successful lanczos_resize_ycc16 on the context launched: the LANCZOS_KERNEL_* of the luma and of the chroma
 * resize (LANCZOS_KERNEL_NONE: a copy), whether k_rs_ycc_split16, k_rs_ycc_join16 and k_rs_ycc16_merge ran, and the number of
 * launches (resize kernels, copies, split, join, merge).  All zero before any call. */
typedef struct lanczos_ycc16_info {
    int32_t luma_kernel, chroma_kernel, split, join, merge, launches;
    int32_t reserved[2];
} lanczos_ycc16_info;
int lanczos_last_ycc16_info(const lanczos_ctx* ctx, lanczos_ycc16_info* info);

/* ---- reduce by whole factors (Pillow's Image.reduce((fx, fy), box), an exact integer box average) ----
 * 8-bit, 1, 3 or 4 independent interleaved channels.  box = (x0, y0, x1, y1), integers with 0 <= x0 < x1 <= in_w and the same
 * for y; NULL = the whole frame.  The output is ceil((x1 - x0) / fx) x ceil((y1 - y0) / fy) pixels, tightly packed rows.
 * Output pixel (ox, oy) covers source columns x0 + ox * fx .. min(x0 + (ox + 1) * fx, x1) - 1 and the rows likewise: the last
 * column and row of blocks may be ragged and then divide by their own pixel count d, in uint32:
 *   out = ((sum + d / 2) * m(d)) >> 24,  m(d) = floor(2^24 / d)
 * (what Pillow's single-precision 4294967296.0f / (256 * d) gives for every d < 65536).  fx * fy >= 65536 and frames of 2^31
 * bytes or more: LANCZOS_ERR_UNSUPPORTED.  Pillow refuses I;16 here; there is no 16-bit, no float and no alpha-aware reduce. */
int lanczos_reduce_size(int in_w, int in_h, int fx, int fy, const int32_t* box, int* out_w, int* out_h);   /* host only */
/* Device buffers, asynchronous on `stream`; frame strides in bytes, 0 = tightly packed; the base may be any byte address. */
int lanczos_reduce_device(lanczos_ctx* ctx, int in_w, int in_h, int channels, int fx, int fy, const int32_t* box,
                          const void* d_in, void* d_out, int frames, size_t in_frame_stride, size_t out_frame_stride,
                          void* stream);
/* Host buffers, `frames` frames back to back; synchronous. */
int lanczos_reduce_host(lanczos_ctx* ctx, int in_w, int in_h, int channels, int fx, int fy, const int32_t* box,
                        const void* in, void* out, int frames);

/* ---- measurement / introspection ---- */
/* When enabled, every lanczos_resample_device call brackets its main kernel with HIP events on the
 * launch stream. lanczos_timing_read synchronises, returns and resets the sums. */
int lanczos_timing_enable(lanczos_ctx* ctx, int on);
int lanczos_timing_read(lanczos_ctx* ctx, int* launches, double* main_kernel_ms, double* prefix_kernel_ms);
int lanczos_last_kernel(const lanczos_ctx* ctx);
/* How the last upscale call (lanczos_resample_device / _host / _planar_device) on the context was launched -- finer than the
 * family of lanczos_last_kernel, for tests and A/B runs.  One int: LANCZOS_ROUTE_MAIN(r) is the main kernel,
 * LANCZOS_ROUTE_PREFIX(r) how the in-place prefix rows [0, K) were produced, LANCZOS_ROUTE_LAUNCHES(r) the number of launches the
 * call went out as (1 unless lanczos_resample_device split an oversized batch; lanczos_resample_host counts the launches of its
 * pipeline's groups).  Main kernel and prefix route are those of the LAST launch; LANCZOS_ROUTE_PREFIX_SEEN(r) has bit
 * (1 << route) set for every prefix route any launch of the call took.  0 (all fields "none") after a resize, reduce or layout
 * call, after a call that failed before its first launch, and on a new context. */
int lanczos_last_route(const lanczos_ctx* ctx);
#define LANCZOS_ROUTE_MAIN(r) ((r) & 0xf)
#define LANCZOS_ROUTE_PREFIX(r) (((r) >> 4) & 0xf)
#define LANCZOS_ROUTE_PREFIX_SEEN(r) (((r) >> 8) & 0xff)
#define LANCZOS_ROUTE_LAUNCHES(r) (((r) >> 16) & 0x7fff)
#define LANCZOS_ROUTE_MAIN_NONE 0     /* no main launch: a strip from row 0 that ends inside the prefix rows (k_march only) */
#define LANCZOS_ROUTE_MAIN_MARCH 1    /* k_march: integer scales, rows and frame strides 16-byte multiples */
#define LANCZOS_ROUTE_MAIN_TILE 2     /* k_fast, the tile-per-workgroup kernel: the other integer scales, LANCZOS_TILE_KERNEL=1 */
#define LANCZOS_ROUTE_MAIN_RATP 3     /* k_ratp: exactly periodic rational scales */
#define LANCZOS_ROUTE_MAIN_RAT 4      /* k_rat: the other rational scales, LANCZOS_NO_RATP=1 */
#define LANCZOS_ROUTE_MAIN_GENERIC 5  /* k_generic */
#define LANCZOS_ROUTE_MAIN_HLS 6      /* k_hls */
#define LANCZOS_ROUTE_PREFIX_NONE 0      /* no prefix rows in the call: K = 0, a strip below them, LANCZOS_MODE_HLS */
#define LANCZOS_ROUTE_PREFIX_RIDING 1    /* extra workgroups at the end of the k_march grid */
#define LANCZOS_ROUTE_PREFIX_FRONT 2     /* k_prefix_reg (registers only) in front of k_march */
#define LANCZOS_ROUTE_PREFIX_BEHIND 3    /* k_prefix (LDS row arrays) behind the main kernel */
#define LANCZOS_ROUTE_PREFIX_STREAMED 4  /* k_prefix_stream (LDS rings, any depth) behind the main kernel */
int lanczos_last_hip_error(const lanczos_ctx* ctx);
/* The workgroup table of the last k_march launch of the last upscale call on the context (the table decides which rows of which
 * (strip, frame) pair every marching workgroup computes; for tests and A/B runs).  `entries`, if not NULL, receives up to
 * `capacity` int32 quadruples (frame, strip, m_b, m_e) in table order -- workgroup-major, info->segs entries per workgroup,
 * m_b >= m_e: an empty segment -- where [m_b, m_e) are the input rows m = floor(y / scale) whose output rows the segment stores.
 * Returns the number of quadruples the table holds (info->workgroups * info->segs), or a negative LANCZOS_ERR_*.  All of `info`
 * is zero and 0 is returned where the last call launched no k_march, after a resize, reduce or layout call and on a new
 * context, as for lanczos_last_route.  Host data only: the call touches neither a stream nor the device. */
typedef struct lanczos_march_table_info {
    int32_t workgroups;   /* marching workgroups of the launch (riding prefix workgroups not counted) */
    int32_t segs;         /* table entries per workgroup */
    int32_t mode;         /* LANCZOS_MARCH_TABLE_* : which branch of the builder made the table */
    int32_t rank_aware;   /* 1: shares weighted by the slots' speeds, 0: equal chunks */
    int32_t strips, frames;
    int32_t m_lo, m_hi;   /* the rows the table shares out */
    int32_t wg_per_cu;    /* resident marching workgroups per CU the table was laid out for */
    int32_t cus;
    int32_t reserved[6];
} lanczos_march_table_info;
#define LANCZOS_MARCH_TABLE_NONE 0
#define LANCZOS_MARCH_TABLE_A 1   /* one workgroup per CU slot, a share may run across (strip, frame) pairs */
#define LANCZOS_MARCH_TABLE_B 2   /* whole chunks of one pair, one segment per workgroup */
int lanczos_last_march_table(const lanczos_ctx* ctx, lanczos_march_table_info* info, int32_t* entries, int capacity);
/* Force a kernel family for A/B tests: LANCZOS_KERNEL_NONE (auto), _GENERIC or _FAST. */
int lanczos_force_kernel(lanczos_ctx* ctx, int family);
const char* lanczos_strerror(int code);
const char* lanczos_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LANCZOS_HIP_H */
