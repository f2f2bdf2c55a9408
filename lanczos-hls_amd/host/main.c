/*
 * main.c -- the harness: what main.cpp:15-19 + sim_tb (full_TB.h:99-180) do around the resample entry point,
 * with the reference's compile-time parameters (params.h) turned into command-line arguments.
 *
 *   lanczos_upscale <in.(png|ppm|pgm)> <out.(png|ppm|pgm)> [--scale N[/D]] [--a A] [--channels C]
 *                   [--exact | --hls] [--device D] [--repeat K]
 *   lanczos_upscale <in> <out> --size WxH [--filter box|bilinear|hamming|bicubic|nearest|lanczos] [--box x0,y0,x1,y1]
 *                   [--reducing-gap G] [--window x0,y0,w,h] [--a A] [--channels C | --alpha] [--device D] [--repeat K]
 *                   (resize to any size, downscaling included, through lanczos_resize_host: Pillow's Image.resize with
 *                   LANCZOS, not the reference's model; refuses --scale, --exact, --hls and the multi-device flags.
 *                   --alpha: four channels, the fourth straight alpha, resized as Pillow's mode RGBA and written as an
 *                   RGBA PNG; needs --size, --channels 4 if --channels is given, and a .png output.
 *                   --box: resize that region of the source (source pixels, fractions allowed), Image.resize's box;
 *                   --reducing-gap G >= 1: reduce by whole factors first, Image.resize's reducing_gap; not with --alpha;
 *                   --filter: Image.resize's resample, default lanczos; every other filter needs a = 3, nearest takes no
 *                   --reducing-gap;
 *                   --window: compute and write only that window of the WxH output (output pixels), a w x h image:
 *                   Image.resize(...).crop((x0, y0, x0 + w, y0 + h)) through lanczos_resize_window_host)
 *                   [--devices 0-7 | 0,2,5] [--frames F] [--split frames|rows] [--root]   (several GPUs of one node, plain C:
 *                   the image is replicated into a batch of F frames and the batch -- or every frame's rows -- is split
 *                   over the devices by lanczos_resample_multi_host; the first result frame is written.  --root: the batch
 *                   is resident on the first device instead and travels by one RCCL scatter / gather over xGMI
 *                   (lanczos_resample_multi_root); compute-only and exchange-inclusive rates are printed separately,
 *                   SURVEY.md 8e "Reporting")
 *
 * load (interleaved u8 HWC, like stbi_load, full_TB.h:107) -> checks with the reference's messages and
 * EXIT_FAILURE (full_TB.h:110-123) -> "Scale:%d/%d, WIDTHS %d -> %d" (full_TB.h:124) -> the resample, through
 * the C ABI (include/lanczos_hip.h; replaces lanczos(stream_in, stream_out), full_TB.h:140) -> write the image
 * (like stbi_write_png, full_TB.h:172).  Host code is plain C; everything GPU is behind the extern "C" shim.
 * There is no software fallback: without a GPU the program reports the error and fails.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "../../include/lanczos_hip.h"
#include "image_io.h"

static int ends_with(const char* s, const char* suf) {
    size_t n = strlen(s), m = strlen(suf);
    return n >= m && strcmp(s + n - m, suf) == 0;
}

static double ms_since(const struct timespec* t0) {
    struct timespec t1;
    clock_gettime(CLOCK_MONOTONIC, &t1);
    return (t1.tv_sec - t0->tv_sec) * 1e3 + (t1.tv_nsec - t0->tv_nsec) / 1e6;
}

static const char* const filter_names[6] = {"lanczos", "box", "bilinear", "hamming", "bicubic", "nearest"}; /* LANCZOS_FILTER_* */

/* --size WxH: one frame through lanczos_resize_host */
static int resize_main(const char* out_path, const uint8_t* img, int width, int height, int channels, int out_w, int out_h,
                       int a, int alpha, int filter, int device, int repeat, const double* box, double gap, const int* window) {
    lanczos_resize_desc d;
    lanczos_resize_opts o;
    lanczos_resize_window win;
    lanczos_resize_plan_ex plan;
    int rc = lanczos_resize_desc_init_ex(&d, width, height, out_w, out_h, channels, a,
                                         (alpha ? LANCZOS_RESIZE_ALPHA : 0) | LANCZOS_RESIZE_FILTER(filter));
    if (rc == LANCZOS_OK) rc = lanczos_resize_opts_init(&o, &d);
    if (rc == LANCZOS_OK) {
        if (box) memcpy(o.box, box, sizeof(o.box));
        o.reducing_gap = gap;
        rc = lanczos_resize_window_init(&win, &d);
    }
    if (rc == LANCZOS_OK) {
        if (window) win.x0 = window[0], win.y0 = window[1], win.w = window[2], win.h = window[3];
        rc = lanczos_resize_window_plan_host(&d, &o, &win, 1, &plan); /* validates the box, the gap and the window */
    }
    if (rc != LANCZOS_OK) {
        printf("Cannot resize %i x %i to %i x %i: %s.\n", width, height, out_w, out_h, lanczos_strerror(rc));
        return EXIT_FAILURE;
    }
    printf("Resize %d x %d -> %d x %d, a = %d%s\n", width, height, out_w, out_h, a, alpha ? ", straight alpha" : "");
    if (filter != LANCZOS_FILTER_LANCZOS) printf("Filter %s\n", filter_names[filter]);
    if (box) printf("Box %g,%g,%g,%g\n", o.box[0], o.box[1], o.box[2], o.box[3]);
    if (plan.fx > 1 || plan.fy > 1)
        printf("Reduce by %d x %d over %d,%d,%d,%d to %d x %d first\n", plan.fx, plan.fy, plan.safe_box[0], plan.safe_box[1],
               plan.safe_box[2], plan.safe_box[3], plan.reduced_w, plan.reduced_h);
    if (window) {
        int32_t rect[4] = {0, 0, 0, 0};
        (void)lanczos_resize_window_source(&d, &o, &win, rect);
        printf("Window %d,%d,%d,%d of the output, from source pixels %d,%d to %d,%d\n", win.x0, win.y0, win.w, win.h, rect[0],
               rect[1], rect[2], rect[3]);
    }
    uint8_t* out = (uint8_t*)malloc((size_t)win.w * win.h * channels);
    lanczos_ctx* ctx = NULL;
    rc = lanczos_create(&ctx, device);
    if (rc != LANCZOS_OK || !out) {
        printf("Cannot use the GPU: %s\n", lanczos_strerror(rc));
        return EXIT_FAILURE;
    }
    struct timespec t0;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (int k = 0; k < repeat && rc == LANCZOS_OK; k++) rc = lanczos_resize_window_host(ctx, &d, &o, &win, img, out, 1);
    if (rc != LANCZOS_OK) {
        printf("lanczos_resize failed: %s (hip error %d)\n", lanczos_strerror(rc), lanczos_last_hip_error(ctx));
        return EXIT_FAILURE;
    }
    const double ms = ms_since(&t0) / repeat;
    printf("%dx%d->%dx%d_%d: %.3f ms per frame incl. PCIe copies (%.1f Mpix/s), kernel family %d\n", width, height, out_w,
           out_h, a, ms, win.w * (double)win.h / ms / 1e3, lanczos_last_kernel(ctx));
    const int ok = ends_with(out_path, ".png") ? lz_image_write_png(out_path, win.w, win.h, channels, out, win.w * channels)
                                               : lz_image_write_pnm(out_path, win.w, win.h, channels, out, win.w * channels);
    lanczos_destroy(ctx);
    free(out);
    if (!ok) {
        printf("Could not write %s\n", out_path);
        return EXIT_FAILURE;
    }
    return 0;
}

int main(int argc, char* argv[]) {
    const char *in_path = NULL, *out_path = NULL;
    int scale_n = 2, scale_d = 1, a = 3, want_channels = 3, exact = 0, hls = 0, device = 0, repeat = 1;
    int devices[64], n_devices = 0, frames = 1, split = LANCZOS_SPLIT_FRAMES, root = 0;
    int size_w = 0, size_h = 0, have_size = 0, upscale_only = 0; /* upscale_only: a flag --size cannot go with */
    int alpha = 0, have_channels = 0, have_box = 0, have_gap = 0, filter = LANCZOS_FILTER_LANCZOS, have_filter = 0;
    double box[4] = {0, 0, 0, 0}, gap = 0.0;
    int window[4] = {0, 0, 0, 0}, have_window = 0;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--size") && i + 1 < argc) {
            have_size = 1;
            if (sscanf(argv[++i], "%dx%d", &size_w, &size_h) != 2) size_w = size_h = 0;
        } else if (!strcmp(argv[i], "--box") && i + 1 < argc) {
            char tail;
            have_box = sscanf(argv[++i], "%lf,%lf,%lf,%lf%c", &box[0], &box[1], &box[2], &box[3], &tail) == 4 ? 1 : -1;
        } else if (!strcmp(argv[i], "--window") && i + 1 < argc) {
            char tail;
            have_window = sscanf(argv[++i], "%d,%d,%d,%d%c", &window[0], &window[1], &window[2], &window[3], &tail) == 4 ? 1 : -1;
        } else if (!strcmp(argv[i], "--reducing-gap") && i + 1 < argc) {
            char tail;
            have_gap = sscanf(argv[++i], "%lf%c", &gap, &tail) == 1 && gap >= 1.0 ? 1 : -1;
        } else if (!strcmp(argv[i], "--filter") && i + 1 < argc) {
            have_filter = -1;
            i++;
            for (int f = 0; f < 6; f++)
                if (!strcmp(argv[i], filter_names[f])) filter = f, have_filter = 1;
        } else if (!strcmp(argv[i], "--scale") && i + 1 < argc) {
            upscale_only = 1;
            scale_d = 1;
            if (sscanf(argv[++i], "%d/%d", &scale_n, &scale_d) < 1) scale_n = 0;
        } else if (!strcmp(argv[i], "--a") && i + 1 < argc) {
            a = atoi(argv[++i]);
        } else if (!strcmp(argv[i], "--channels") && i + 1 < argc) {
            want_channels = atoi(argv[++i]);
            have_channels = 1;
        } else if (!strcmp(argv[i], "--alpha")) {
            alpha = 1;
        } else if (!strcmp(argv[i], "--device") && i + 1 < argc) {
            device = atoi(argv[++i]);
        } else if (!strcmp(argv[i], "--repeat") && i + 1 < argc) {
            repeat = atoi(argv[++i]);
        } else if (!strcmp(argv[i], "--exact")) {
            exact = 1;
            upscale_only = 1;
        } else if (!strcmp(argv[i], "--hls")) {
            hls = 1;
            upscale_only = 1;
        } else if (!strcmp(argv[i], "--root")) {
            root = 1;
            upscale_only = 1;
        } else if (!strcmp(argv[i], "--frames") && i + 1 < argc) {
            upscale_only = 1;
            frames = atoi(argv[++i]);
        } else if (!strcmp(argv[i], "--split") && i + 1 < argc) {
            upscale_only = 1;
            split = !strcmp(argv[++i], "rows") ? LANCZOS_SPLIT_ROWS : LANCZOS_SPLIT_FRAMES;
        } else if (!strcmp(argv[i], "--devices") && i + 1 < argc) { /* "0-7" or "0,2,5" */
            upscale_only = 1;
            const char* p = argv[++i];
            int lo, hi;
            if (sscanf(p, "%d-%d", &lo, &hi) == 2) {
                for (int v = lo; v <= hi && n_devices < 64; v++) devices[n_devices++] = v;
            } else {
                while (*p && n_devices < 64) {
                    devices[n_devices++] = atoi(p);
                    while (*p && *p != ',') p++;
                    if (*p == ',') p++;
                }
            }
        } else if (!in_path) {
            in_path = argv[i];
        } else if (!out_path) {
            out_path = argv[i];
        }
    }
    if (!in_path || !out_path) {
        fprintf(stderr, "usage: %s <in.png|ppm> <out.png|ppm> [--scale N[/D]] [--a A] [--channels C] [--exact|--hls] "
                        "[--device D] [--repeat K] [--devices 0-7|0,2,5] [--frames F] [--split frames|rows] [--root]\n"
                        "       %s <in.png|ppm> <out.png|ppm> --size WxH [--filter box|bilinear|hamming|bicubic|nearest|lanczos] "
                        "[--box x0,y0,x1,y1] [--reducing-gap G] [--window x0,y0,w,h] [--a A] "
                        "[--channels C | --alpha] [--device D] [--repeat K]\n",
                argv[0], argv[0]);
        return EXIT_FAILURE;
    }
    if (have_size && upscale_only) {
        fprintf(stderr, "--size cannot be combined with --scale, --exact, --hls, --devices, --frames, --split or --root\n");
        return EXIT_FAILURE;
    }
    if (have_box < 0) {
        fprintf(stderr, "--box takes four numbers, x0,y0,x1,y1 in source pixels\n");
        return EXIT_FAILURE;
    }
    if (have_gap < 0) {
        fprintf(stderr, "--reducing-gap takes a number of at least 1\n");
        return EXIT_FAILURE;
    }
    if ((have_box || have_gap) && !have_size) {
        fprintf(stderr, "--box and --reducing-gap need --size\n");
        return EXIT_FAILURE;
    }
    if (have_window < 0 || (have_window && !have_size)) {
        fprintf(stderr, "--window takes four integers, x0,y0,w,h in pixels of the --size output, and needs --size\n");
        return EXIT_FAILURE;
    }
    if (have_filter < 0 || (have_filter && !have_size)) {
        fprintf(stderr, "--filter takes box, bilinear, hamming, bicubic, nearest or lanczos, and needs --size\n");
        return EXIT_FAILURE;
    }
    if (alpha) {
        if (!have_size || (have_channels && want_channels != 4) || !ends_with(out_path, ".png")) {
            fprintf(stderr, "--alpha needs --size, four channels (no --channels other than 4) and a .png output\n");
            return EXIT_FAILURE;
        }
        want_channels = 4;
    }
    if (repeat < 1) repeat = 1;
    printf("Running full TB (%s)\n", lanczos_version());  /* main.cpp:16 */

    int width = 0, height = 0, channels = 0;
    uint8_t* img = lz_image_load(in_path, &width, &height, &channels, want_channels);
    if (img == NULL) { /* full_TB.h:110-113 */
        printf("Image was not loaded successfully.\n");
        return EXIT_FAILURE;
    }
    if (have_size) {
        const int rc = resize_main(out_path, img, width, height, want_channels, size_w, size_h, a, alpha, filter, device, repeat,
                                   have_box ? box : NULL, have_gap ? gap : 0.0, have_window ? window : NULL);
        lz_image_free(img);
        return rc;
    }
    lanczos_desc d;
    int rc = lanczos_desc_init(&d, width, height, want_channels, 1, scale_n, scale_d, a);
    if (rc != LANCZOS_OK) { /* the reference rejects what its compiled-in parameters do not cover (full_TB.h:115-123) */
        printf("Image has wrong dimensions (%i x %i) or parameters: %s.\n", width, height, lanczos_strerror(rc));
        return EXIT_FAILURE;
    }
    d.mode = hls ? LANCZOS_MODE_HLS : (exact ? LANCZOS_MODE_EXACT : LANCZOS_MODE_LSB1);
    if (frames < 1) frames = 1;
    printf("Scale:%d/%d, WIDTHS %d -> %d\n", d.scale_n, d.scale_d, d.in_w, d.out_w); /* full_TB.h:124 */

    struct timespec t0, t1;
    uint8_t* out = NULL;
    lanczos_ctx* ctx = NULL;
    if (n_devices > 0) {
        /* several devices, still plain C: a batch of `frames` copies of the image, split by frames or by rows */
        const size_t in_fb = lanczos_in_frame_bytes(&d), out_fb = lanczos_out_frame_bytes(&d);
        uint8_t* batch_in = (uint8_t*)malloc(in_fb * frames);
        out = (uint8_t*)malloc(out_fb * frames);
        lanczos_multi* m = NULL;
        rc = lanczos_multi_create(&m, devices, n_devices);
        if (rc != LANCZOS_OK || !out || !batch_in) {
            printf("Cannot use the GPUs: %s\n", lanczos_strerror(rc));
            return EXIT_FAILURE;
        }
        for (int f = 0; f < frames; f++) memcpy(batch_in + (size_t)f * in_fb, img, in_fb);
        if (root) {
            /* the batch lives on the FIRST device; the other devices get their shares by one RCCL scatter and return them by one
             * gather (over xGMI).  Two rates, never mixed: the resample step alone and the whole call. */
            void *d_in = NULL, *d_out = NULL;
            double cms = 0, tms = 0, cms_sum = 0, tms_sum = 0;
            rc = lanczos_device_alloc(devices[0], &d_in, in_fb * frames);
            if (rc == LANCZOS_OK) rc = lanczos_device_alloc(devices[0], &d_out, out_fb * frames);
            if (rc == LANCZOS_OK) rc = lanczos_device_copy(devices[0], d_in, batch_in, in_fb * frames, 1);
            if (rc == LANCZOS_OK) rc = lanczos_resample_multi_root(m, &d, d_in, d_out, frames, split, &cms, &tms); /* warm-up */
            for (int k = 0; k < repeat && rc == LANCZOS_OK; k++) {
                rc = lanczos_resample_multi_root(m, &d, d_in, d_out, frames, split, &cms, &tms);
                cms_sum += cms;
                tms_sum += tms;
            }
            if (rc == LANCZOS_OK) rc = lanczos_device_copy(devices[0], out, d_out, out_fb * frames, 0);
            if (rc != LANCZOS_OK) {
                int he = 0, re = 0, at = 0;
                lanczos_multi_last_error(m, &he, &re, &at);
                printf("lanczos failed: %s (hip error %d, rccl error %d at message %d)\n", lanczos_strerror(rc), he, re, at);
                return EXIT_FAILURE;
            }
            const double mpix = frames * d.out_w * (double)d.out_h / 1e6;
            printf("%dx%d->%dx%d_%d|%d_%d: %d frames resident on device %d, %d device(s), split by %s:\n"
                   "  compute only            %.3f ms per batch (%.1f Mpix/s)\n"
                   "  root scatter + gather   %.3f ms per batch (%.1f Mpix/s)\n", d.in_w, d.in_h, d.out_w, d.out_h, d.scale_n,
                   d.scale_d, d.a, frames, devices[0], lanczos_multi_devices(m), split == LANCZOS_SPLIT_ROWS ? "rows" : "frames",
                   cms_sum / repeat, mpix / (cms_sum / repeat) * 1e3, tms_sum / repeat, mpix / (tms_sum / repeat) * 1e3);
            lanczos_device_free(devices[0], d_in);
            lanczos_device_free(devices[0], d_out);
            goto multi_done;
        }
        rc = lanczos_resample_multi_host(m, &d, batch_in, out, frames, split); /* warm-up: plans, staging buffers */
        clock_gettime(CLOCK_MONOTONIC, &t0);
        for (int k = 0; k < repeat && rc == LANCZOS_OK; k++) rc = lanczos_resample_multi_host(m, &d, batch_in, out, frames, split);
        clock_gettime(CLOCK_MONOTONIC, &t1);
        if (rc != LANCZOS_OK) {
            printf("lanczos failed: %s\n", lanczos_strerror(rc));
            return EXIT_FAILURE;
        }
        const double ms = ((t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) / 1e6) / repeat;
        printf("%dx%d->%dx%d_%d|%d_%d: %d frames over %d device(s), split by %s: %.3f ms per batch incl. PCIe copies "
               "(%.1f Mpix/s)\n", d.in_w, d.in_h, d.out_w, d.out_h, d.scale_n, d.scale_d, d.a, frames,
               lanczos_multi_devices(m), split == LANCZOS_SPLIT_ROWS ? "rows" : "frames", ms,
               frames * d.out_w * (double)d.out_h / ms / 1e3);
    multi_done:
        for (int f = 1; f < frames; f++)
            if (memcmp(out, out + (size_t)f * out_fb, out_fb) != 0) {
                printf("frame %d differs from frame 0\n", f);
                return EXIT_FAILURE;
            }
        lanczos_multi_destroy(m);
        free(batch_in);
    } else {
        out = (uint8_t*)malloc(lanczos_out_frame_bytes(&d));
        rc = lanczos_create(&ctx, device);
        if (rc != LANCZOS_OK || !out) {
            printf("Cannot use the GPU: %s\n", lanczos_strerror(rc));
            return EXIT_FAILURE;
        }
        clock_gettime(CLOCK_MONOTONIC, &t0);
        for (int k = 0; k < repeat && rc == LANCZOS_OK; k++) rc = lanczos_resample_host(ctx, &d, img, out, 1);
        clock_gettime(CLOCK_MONOTONIC, &t1);
        if (rc != LANCZOS_OK) {
            printf("lanczos failed: %s (hip error %d)\n", lanczos_strerror(rc), lanczos_last_hip_error(ctx));
            return EXIT_FAILURE;
        }
        const double ms = ((t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) / 1e6) / repeat;
        printf("%dx%d->%dx%d_%d|%d_%d: %.3f ms per frame incl. PCIe copies (%.1f Mpix/s), kernel family %d\n", d.in_w,
               d.in_h, d.out_w, d.out_h, d.scale_n, d.scale_d, d.a, ms, d.out_w * (double)d.out_h / ms / 1e3,
               lanczos_last_kernel(ctx));
    }

    int ok = ends_with(out_path, ".png") ? lz_image_write_png(out_path, d.out_w, d.out_h, want_channels, out,
                                                              d.out_w * want_channels)
                                         : lz_image_write_pnm(out_path, d.out_w, d.out_h, want_channels, out,
                                                              d.out_w * want_channels);
    if (!ok) {
        printf("Could not write %s\n", out_path);
        return EXIT_FAILURE;
    }
    if (ctx) lanczos_destroy(ctx);
    lz_image_free(img);
    free(out);
    return 0;
}
