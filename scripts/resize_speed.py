#!/usr/bin/env python3
"""resize_speed.py -- speed of the resize-to-any-size entry (lanczos_resize_device) on one MI355X.

    python scripts/resize_speed.py [--steps K] [--warmup W] [--rounds R] [--only W1,W3,A1,U1,F1,WIN1,RC1] [--routes rgbx,three_step]
                                   [--pillow] [--parent-lib PATH]

One JSON line per (workload, path).  Discipline as bench.py's: the frames are resident in HBM and the steps cycle through
enough input / output sets that the inputs of one cycle exceed twice the 256 MiB Infinity Cache (no step finds its input
there); W untimed warm-up steps per path; device-event timing of K steps per region; the paths (auto, fused, two-pass)
alternate region by region and every path's figure is the median over its R regions.  Before timing, the frame-0 outputs
of all paths are compared byte for byte.

  us_per_step    device time of one call over F frames (median region / K)
  mpix_per_s     output pixels per second
  hbm_frac       compulsory bytes (F * (input + output frame bytes)) / step time / 8 TB/s
  kernel         family that served the call (lanczos_last_kernel: 4 fused, 5 two-pass)

A1 and A4 are W1's and W4's shapes with four channels, straight alpha in the last (Pillow's mode RGBA).  They time three
routes under RESIZE_AUTO, alternating region by region like the paths above:
  rgbx        the four channels filtered independently (no alpha semantics: the floor of what the kernel costs)
  alpha       LANCZOS_RESIZE_ALPHA: premultiply and un-premultiply inside the resize kernel
  three_step  what a caller had to do without the flag: premultiply with torch elementwise operations, the rgbx resize,
              un-premultiply with torch elementwise operations, the same integer formulas, all on the same stream
Before timing, frame 0 of `alpha` and of `three_step` are compared byte for byte.  --routes selects routes (a build without
the flag runs rgbx,three_step).

U1 and U4 are W1's and W4's shapes with 16-bit samples (LANCZOS_RESIZE_U16, Pillow's mode I;16): the same three paths, the
same discipline, twice the compulsory bytes.

C1, C4 (bicubic), L1, L4 (bilinear) and N1, N4 (nearest) are W1's and W4's shapes with Pillow's other filters (--only C1,C4,...;
a build with LANCZOS_RESIZE_FILTER).  LANCZOS_RS_NO_SMALL_BUCKETS=1 in the environment pads the short filters' upscales to the
7-tap fused instance (the A/B of the 3- and 5-tap instances).  N1 and N4 also time a device-to-device copy of the output's
bytes on the same stream and print the ratio.

F1 and F4 are W1's and W4's shapes with float samples (LANCZOS_RESIZE_F32, Pillow's mode F; uniform [0, 1) inputs): the same
three paths, four times the compulsory bytes.  They run on request (--only F1,F4) and need a build with the flag.

R5 is W5's shape (3840x2160 -> 160x90, 32 frames) with reducing_gap: routes `plain` (W5 as it is: two-pass, 145 vertical
taps), `gap2` and `gap3` (reduce 12x12 / 8x8 into context scratch, then the fused kernel), `reduce12` (lanczos_reduce_device
12x12 alone) and `copy` (a device-to-device copy of the same source bytes, which moves twice what the reduction moves),
alternating region by region.  The bytes of gap2 / gap3 are NOT those of plain: they are Pillow's for that gap.

B1 / B2 are a fractional 1280x720-ish box out of 7680x4320 (8 frames) to 1920x1080 / 640x360: `boxed_auto` and
`boxed_two_pass` on the whole frames against `tight_auto` and `tight_two_pass`, the same resize of a tightly packed copy of
the crop region padded by the support (its box is the boxed one shifted by whole pixels; a float rounds the two
differently, so the bytes are compared between the paths of each, not between boxed and tight).  R5, B1 and B2 run on
request (--only R5,B1,B2); they need a build with lanczos_resize_device_ex.

T1, T2, T4 and TP are tensor workloads (lanczos_resize_tensor_device: 8-bit frames resized straight into normalised float
tensors; --only T1,T2,T4,TP; a build with the entry): T1 is W1's shape to CHW, T2 the same to HWC, T4 W4's shape to CHW, TP a
preprocessing shape, 256 frames of 500x375 -> 224x224 from a centred 375x375 box, to CHW.  Routes, alternating region by region:
  fused         the tensor call under RESIZE_AUTO: the fused kernel stores the floats
  converted     the same call under RESIZE_CONVERT: the same byte resize into context scratch, then k_rs_to_tensor
  bytes_torch   the byte resize, then uint8 -> .permute().float().div(255).sub(mean).div(std) with torch on the same stream
  bytes         the byte resize alone
  parent_bytes  the byte resize alone on another build of the library (--parent-lib PATH: the parent commit's)
  copy          a device-to-device copy of one step's float output: the floor of what the extra bytes cost
Frame 0 of fused and converted are compared bit for bit before timing; a last line gives the ratios.

T1h, T2h, T4h and TPh are T1, T2, T4 and TP to bfloat16 (lanczos_resize_tensor16_device; --only T1h,T2h,T4h,TPh).  Routes:
  fused         the 16-bit tensor call under RESIZE_AUTO: the fused kernel stores the bfloat16 words
  converted     the same call under RESIZE_CONVERT: the byte resize into context scratch, then k_rs_to_tensor16
  f32_cast      the float32 tensor call (fused) followed by torch's .to(torch.bfloat16) on the same stream: what the 16-bit
                entry replaces
  f32           the float32 tensor call alone
Frame 0 of fused, converted and f32_cast are compared bit for bit before timing; a last line gives the ratios.

N16, N16h, N32 and NP16 are normalised-tensor workloads of wide samples (lanczos_resize_tensor_norm_device: uint16 or float32
frames resized straight into normalised tensors; --only N16,N16h,N32,NP16; a build with the entry).  N16: 32 frames of
3840x2160 -> 1920x1080, three 16-bit channels, to CHW float32; N16h the same to bfloat16; N32 the same shape with float samples;
NP16: 256 one-channel 16-bit frames of 512x512 -> 224x224 to float32.  Routes, alternating region by region:
  fused          the call under RESIZE_AUTO: the fused kernel computes and stores the elements
  converted      the same call under RESIZE_CONVERT: the same sample resize into context scratch, then k_rs_to_tensor_norm
  samples_torch  the sample resize, then .permute().float().div(div).sub(mean).div(std)[.to(bfloat16)] with torch on the same
                 stream, div / mean / std given as tensors so that torch divides
  samples        the sample resize alone
  parent_samples the sample resize alone on another build of the library (--parent-lib PATH: the parent commit's)
  copy           a device-to-device copy of one step's element output
Frame 0 of fused, converted and samples_torch are compared bit for bit before timing; a last line gives the ratios.

WIN1, WIN1h, WIN2 and WINC are resize-and-crop workloads (a window of the output, lanczos_resize_window_device; --only
WIN1,WIN1h,WIN2,WINC; a build with the entry).  WIN1: 256 frames of 500x375 RGB8 -> 341x256, window center_window(341, 256, 224, 224), bytes out.  WIN1h:
the same into normalised bfloat16 CHW.  WIN2: 32 frames of 3840x2160 -> 1920x1080, window the centre 1280x720.  WINC: 256 frames of 341x256 at their own size (neither
axis runs: the full call is the plain copy, the windowed one the crop copy k_rs_crop), window the centre 224x224.  Routes:
  windowed      the call with the window: only the window's pixels are computed and stored
  full_slice    the full call, then torch's slice of the window and .contiguous() on the same stream: what the window replaces
  full          the full call alone
  parent_full   the full call alone on another build of the library (--parent-lib PATH: the parent commit's)
Frame 0 of windowed and full_slice are compared byte for byte before timing; a last line gives the ratios and the two plans.

V1, V1h, VW and VWh are tensor views (a channel map and per-frame flips, lanczos_resize_tensor_view_device; --only V1,V1h,VW,VWh;
a build with the entry), all to normalised CHW with the table in output order.  V1: T1's shape, BGR -> RGB, every other frame
mirrored horizontally through d_flip, float32; V1h: the same to bfloat16.  VW: 256 RGBA frames (alpha set) of 500x375 -> 341x256,
window center_window(341, 256, 224, 224), alpha dropped, float32; VWh: the same to bfloat16.  Routes:
  view            the view under RESIZE_AUTO: the mapped fused instances store the elements
  view_converted  the view under RESIZE_CONVERT: the byte resize into context scratch, then k_rs_to_tensor_map
  tensor_torch    the tensor call without a map, then torch's t[:, [2, 1, 0]] / t[:, :3], torch.where(flip, t.flip(-1), t) and
                  .contiguous() on the same stream: what the view replaces
  tensor          the tensor call without a map alone
Frame 0 of view, view_converted and tensor_torch are compared bit for bit before timing; a last line gives the ratios.

RC1, RC1h and RCC are crops workloads (a tensor view with a crop origin per frame, lanczos_resize_tensor_crops_device; --only
RC1,RC1h,RCC; a build with the entry): Resize -> RandomCrop(224) -> RandomHorizontalFlip -> ToTensor -> Normalize in one call, to
normalised CHW.  RC1: 256 frames of 500x375 RGB8 -> 341x256, a seeded random 224x224 origin per frame, every other frame mirrored,
float32; RC1h: the same to bfloat16.  RCC: 256 frames of 256x256 kept at size (no pass runs: the gather reads the caller's
frames), random 224x224 crops, float32.  Routes:
  crops            the call under RESIZE_AUTO
  crops_converted  the call under RESIZE_CONVERT: the byte resize of the whole output into context scratch, then
                   k_rs_to_tensor_crops (RCC: the same launch as `crops`)
  full_gather      what the call replaces: the view call on the FULL output, then torch's gather of every frame's window with the
                   mirror folded into its column indices (index tensors built outside the timed region).  The gather is the
                   fastest of four that were timed on RC1's tensors (float32 / bfloat16 µs): rows by index_select then columns by
                   torch.gather 299 / 250, torch.gather over rows then over columns with expanded indices 312 / 235 -- the first
                   is used for float32, the second for bfloat16 --, one advanced-indexing expression t[f, c, y, x] 598 / 578, a
                   loop of 256 slice copies 2 818 / 2 784
  window_center    the view call with the centred uniform window and the same flips: the same pixel count on the existing
                   kernels, the floor
Frame 0 of crops, crops_converted and full_gather are compared bit for bit before timing; a last line gives the ratios.

SRC1, SRC1h, SRCP and SRCW are source-layout workloads (lanczos_resize_source: planar or row-pitched frames read as they lie;
--only SRC1,SRC1h,SRCP,SRCW; a build with the entry), RGB8.  SRC1: 32 planar frames of 3840x2160 -> 1920x1080, bytes out; SRC1h:
the same to normalised bfloat16 CHW; SRCP: 256 planar frames of 500x375 -> 341x256, the centre 224x224 window, normalised float32
CHW; SRCW: 32 interleaved frames of 1920x1080 whose rows are pitched to a multiple of 256 bytes -> 3840x2160, bytes out.  SRCA
and SRCAh (--only SRCA,SRCAh): 256 interleaved RGBA frames of 500x375 with LANCZOS_RESIZE_ALPHA and rows of 2006 bytes (no dword
multiple: every row another residue) -> 341x256, bytes out and normalised bfloat16 CHW.  Routes:
  direct        the call under RESIZE_FUSED: the fused kernel stages the caller's planes or pitched rows itself
  packed        the call under RESIZE_CONVERT: k_rs_pack_source into context scratch, then the request as it always ran
  auto          the call under RESIZE_AUTO (the summary line names the route it took)
  torch_repack  what the call replaces: torch's permute(0, 2, 3, 1).contiguous() (SRCW: the slice's .contiguous()) on the same
                stream, then the call without a source
  floor         the call without a source alone, on frames that are already packed
Frame 0 of all five is compared bit for bit before timing; a last line gives the ratios.

DST1, DSTP, DSTPW and DSTW are destination-layout workloads (lanczos_resize_dest: planes or pitched rows stored by the library;
--only DST1,DSTP,DSTPW,DSTW; a build with the entry), RGB8, bytes out.  DST1: 32 interleaved frames of 3840x2160 -> 1920x1080 into
planes; DSTP: 256 planar frames of 500x375 -> 341x256 into planes (an odd width: three plane rows in four start off a dword);
DSTPW: the same with the centre 224x224 window; DSTW: 32 frames of 1920x1080 -> 3840x2160 into rows pitched to a multiple of 256
bytes that is not the tight pitch (11776); DSTA and DST4 (--only DSTA,DST4): DSTP with four channels and alpha, DST1 with four
channels.  Routes: direct, unpacked, auto, torch_repack and floor (run_dest); the dword form of the planar epilogue is the direct
route of a library built with EXTRA=-DLZ_RS_PLANAR_OUT_DWORDS and loaded through LANCZOS_LIB.

--pillow adds Pillow's single-core time of one frame of each workload (if Pillow imports; else "not available"); for U1 and
U4 that is the time of one I;16 plane (a frame has three), for F1 and F4 that of one F plane.

YC1, YC2 and YC3 (--only YC1,YC2,YC3) are YCbCr frames (lanczos_resize_ycc_*): 32 NV12 frames 3840x2160 -> 1920x1080 to
normalised bfloat16 CHW, 256 I420 frames 500x375 -> 341x256 with the centre 224x224 window to float32 CHW, 32 NV12 frames
1920x1080 -> 3840x2160 to RGB bytes.  Routes, alternating region by region: `ycc`, the one call; `torch_convert`, what it
replaces (repeat_interleave of the chroma, the float matrix, round, clamp, cast, repack, then the existing RGB call);
`rgb_floor`, the existing RGB call alone on frames converted beforehand (--parent-lib: on that build); `luma_only`, the luma
plane's one-channel resize alone.  A summary line carries the ratios, the kernels and the launch count of the call.

YO1, YO2 and YO3 (--only YO1,YO2,YO3) resize INTO YCbCr frames (lanczos_resize_ycc_out): 32 NV12 frames 3840x2160 -> 1920x1080
NV12; 32 RGB frames 1920x1080 kept at size -> NV12 under BT.709; 32 RGB frames 3840x2160 -> 1280x720 I420.  Routes: `ycc_out`,
the one call; `pipeline`, what it replaces (from NV12 the chroma split in torch, three one-channel resize calls and the
re-interleave in torch; from RGB the RGB resize, then the float matrix, avg_pool2d, round, clamp, cast and repack in torch);
`floor`, the luma call alone, or the RGB resize alone (--parent-lib: on that build).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import lanczos_hls_amd as L  # noqa: E402

HBM_BPS = 8e12
WORKLOADS = {   # name: (in_w, in_h, out_w, out_h, channels, a, frames)
    "W1": (3840, 2160, 1920, 1080, 3, 3, 32),
    "W2": (1920, 1080, 1280, 720, 3, 3, 32),
    "W3": (7680, 4320, 1920, 1080, 3, 3, 8),
    "W4": (1920, 1080, 3840, 2160, 3, 3, 32),
    "W5": (3840, 2160, 160, 90, 3, 3, 32),
}
U16_WORKLOADS = {   # W1's and W4's shapes, 16-bit samples
    "U1": (3840, 2160, 1920, 1080, 3, 3, 32),
    "U4": (1920, 1080, 3840, 2160, 3, 3, 32),
}
F32_WORKLOADS = {   # W1's and W4's shapes, float samples
    "F1": (3840, 2160, 1920, 1080, 3, 3, 32),
    "F4": (1920, 1080, 3840, 2160, 3, 3, 32),
}
RGBA_WORKLOADS = {   # W1's and W4's shapes, four channels
    "A1": (3840, 2160, 1920, 1080, 4, 3, 32),
    "A4": (1920, 1080, 3840, 2160, 4, 3, 32),
}
FILTER_WORKLOADS = {   # W1's and W4's shapes with Pillow's other filters: name: (workload, filter)
    "C1": ("W1", "bicubic"), "C4": ("W4", "bicubic"), "L1": ("W1", "bilinear"), "L4": ("W4", "bilinear"),
    "N4": ("W4", "nearest"), "N1": ("W1", "nearest"),   # nearest: also timed against a device-to-device copy of the output
}
ROUTES = ("rgbx", "alpha", "three_step")
PATHS = {"auto": L.RESIZE_AUTO, "fused": L.RESIZE_FUSED, "two_pass": L.RESIZE_TWO_PASS}


def run(name, spec, args, ctx, torch, bits=8, filt="lanczos"):
    iw, ih, ow, oh, c, a, f = spec
    in_fb, out_fb = iw * ih * c * bits // 8, ow * oh * c * bits // 8   # frame bytes
    step_in = f * in_fb
    sets = max(2, -(-2 * 256 * 2 ** 20 // step_in) + 1)
    gen = torch.Generator(device="cuda").manual_seed(7)
    if bits == 32:
        xs = [torch.rand(f * in_fb // 4, dtype=torch.float32, device="cuda", generator=gen).view(torch.uint8)
              for _ in range(sets)]
        d = L.resize_desc(iw, ih, ow, oh, c, a, f32=True)
    else:
        xs = [torch.randint(0, 256, (f * in_fb,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(sets)]
        d = L.resize_desc(iw, ih, ow, oh, c, a, bits=bits, filter=filt)
    ys = [torch.empty(f * out_fb, dtype=torch.uint8, device="cuda") for _ in range(sets)]
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    paths, ref = {}, None
    for pname, p in PATHS.items():   # which paths can run this shape, and do they agree
        ctx.resize_force(p)
        try:
            ctx.resize_device(d, xs[0].data_ptr(), ys[0].data_ptr(), f, 0, 0, s)
        except L.LanczosError as e:
            if e.code != L.ERR_UNSUPPORTED:
                raise
            continue
        torch.cuda.synchronize()
        out0 = ys[0][:out_fb].cpu().numpy()
        if ref is None:
            ref = out0
        elif not np.array_equal(out0, ref):
            raise SystemExit(f"{name}: path {pname} differs from the first path")
        paths[pname] = (p, ctx.last_kernel())
    times = {pn: [] for pn in paths}
    for pn, (p, _) in paths.items():
        ctx.resize_force(p)
        for k in range(args.warmup):
            ctx.resize_device(d, xs[k % sets].data_ptr(), ys[k % sets].data_ptr(), f, 0, 0, s)
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for pn, (p, _) in paths.items():
            ctx.resize_force(p)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for k in range(args.steps):
                i = (r * args.steps + k) % sets
                ctx.resize_device(d, xs[i].data_ptr(), ys[i].data_ptr(), f, 0, 0, s)
            e1.record(stream)
            e1.synchronize()
            times[pn].append(e0.elapsed_time(e1) * 1e3 / args.steps)
    ctx.resize_force(L.RESIZE_AUTO)
    if filt == "nearest":   # the yardstick of a gather: hipMemcpyAsync device to device of the output's bytes, same stream
        paths = {"auto": paths["auto"]}   # one kernel whatever is forced
        copies = []
        for r in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for k in range(args.steps):
                ys[(k + 1) % sets].copy_(ys[k % sets], non_blocking=True)
            e1.record(stream)
            e1.synchronize()
            copies.append(e0.elapsed_time(e1) * 1e3 / args.steps)
        print(json.dumps({"workload": name, "d2d_copy_of_output_us": round(statistics.median(copies), 2),
                          "nearest_over_copy": round(statistics.median(times["auto"]) / statistics.median(copies), 3),
                          "bytes": f * out_fb, "measured": True}), flush=True)
    for pn, (p, fam) in paths.items():
        us = statistics.median(times[pn])
        line = {"workload": name, "shape": f"{iw}x{ih}->{ow}x{oh} C{c} a{a} u{bits}" + ("" if filt == "lanczos" else " " + filt),
                "frames": f, "path": pn, "kernel": fam, "small_buckets": os.environ.get("LANCZOS_RS_NO_SMALL_BUCKETS", "0") in ("", "0"),
                "us_per_step": round(us, 2), "us_all_regions": [round(v, 2) for v in times[pn]],
                "mpix_per_s": round(f * ow * oh / us, 1), "hbm_frac": round(f * (in_fb + out_fb) / (us * 1e-6) / HBM_BPS, 4),
                "compulsory_bytes": f * (in_fb + out_fb), "input_sets_cycled": sets, "steps": args.steps,
                "rounds": args.rounds, "lib": os.path.basename(L.LIB_PATH), "measured": True}
        print(json.dumps(line), flush=True)
    if args.pillow:
        key = {8: "pillow_single_core_ms_per_frame", 16: "pillow_single_core_ms_per_I16_plane",
               32: "pillow_single_core_ms_per_F_plane"}[bits]
        try:
            from PIL import Image
            raw = xs[0][:in_fb].cpu().numpy()
            if bits == 8:
                img = Image.frombytes("RGB", (iw, ih), raw.tobytes())
            else:
                img = Image.fromarray(np.ascontiguousarray(raw.view(np.uint16 if bits == 16 else np.float32)
                                                           .reshape(ih, iw, c)[:, :, 0]))
            img.resize((ow, oh), Image.LANCZOS)
            t0 = time.perf_counter()
            img.resize((ow, oh), Image.LANCZOS)
            ms = (time.perf_counter() - t0) * 1e3
            print(json.dumps({"workload": name, key: round(ms, 2), "measured": True}))
        except ImportError:
            print(json.dumps({"workload": name, key: "not available"}))
    del xs, ys
    torch.cuda.empty_cache()


def premultiply(torch, x):
    """x: uint8 [N][4], straight alpha -> premultiplied (t = c * A + 128, c' = ((t >> 8) + t) >> 8)."""
    v = x.to(torch.int32)
    t = v[:, :3] * v[:, 3:] + 128
    out = x.clone()
    out[:, :3] = ((t >> 8) + t) >> 8
    return out


def unpremultiply(torch, y, out):
    """y: uint8 [N][4] premultiplied -> `out` with straight alpha (A in {0, 255}: copy; else min(255, 255 * c' // A))."""
    v = y.to(torch.int32)
    c, a = v[:, :3], v[:, 3:]
    q = torch.clamp(torch.div(255 * c, a.clamp(min=1), rounding_mode="floor"), max=255)
    out.copy_(y)
    out[:, :3] = torch.where((a == 0) | (a == 255), c, q)
    return out


def run_rgba(name, spec, args, ctx, torch):
    iw, ih, ow, oh, c, a, f = spec
    in_fb, out_fb = iw * ih * c, ow * oh * c
    sets = max(2, -(-2 * 256 * 2 ** 20 // (f * in_fb)) + 1)
    gen = torch.Generator(device="cuda").manual_seed(7)
    xs = [torch.randint(0, 256, (f * in_fb,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(sets)]
    ys = [torch.empty(f * out_fb, dtype=torch.uint8, device="cuda") for _ in range(sets)]
    tmp = torch.empty(f * out_fb, dtype=torch.uint8, device="cuda")   # three_step: the premultiplied result
    routes = [r for r in ROUTES if r in args.routes.split(",")]
    d_rgbx = L.resize_desc(iw, ih, ow, oh, c, a)
    d_alpha = L.resize_desc(iw, ih, ow, oh, c, a, alpha=True) if "alpha" in routes else None
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    ctx.resize_force(L.RESIZE_AUTO)

    def step(route, i):
        if route == "rgbx":
            ctx.resize_device(d_rgbx, xs[i].data_ptr(), ys[i].data_ptr(), f, 0, 0, s)
        elif route == "alpha":
            ctx.resize_device(d_alpha, xs[i].data_ptr(), ys[i].data_ptr(), f, 0, 0, s)
        else:
            pre = premultiply(torch, xs[i].view(-1, 4))
            ctx.resize_device(d_rgbx, pre.data_ptr(), tmp.data_ptr(), f, 0, 0, s)
            unpremultiply(torch, tmp.view(-1, 4), ys[i].view(-1, 4))

    first = {}
    for route in routes:
        step(route, 0)
        torch.cuda.synchronize()
        first[route] = (ys[0][:out_fb].cpu().numpy(), ctx.last_kernel())
    if "alpha" in first and "three_step" in first and not np.array_equal(first["alpha"][0], first["three_step"][0]):
        raise SystemExit(f"{name}: the alpha route differs from the three-step route")
    times = {r: [] for r in routes}
    for route in routes:
        for k in range(args.warmup):
            step(route, k % sets)
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for route in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for k in range(args.steps):
                step(route, (r * args.steps + k) % sets)
            e1.record(stream)
            e1.synchronize()
            times[route].append(e0.elapsed_time(e1) * 1e3 / args.steps)
    for route in routes:
        us = statistics.median(times[route])
        line = {"workload": name, "shape": f"{iw}x{ih}->{ow}x{oh} C{c} a{a}", "frames": f, "route": route,
                "kernel": first[route][1], "us_per_step": round(us, 2),
                "us_all_regions": [round(v, 2) for v in times[route]], "mpix_per_s": round(f * ow * oh / us, 1),
                "hbm_frac": round(f * (in_fb + out_fb) / (us * 1e-6) / HBM_BPS, 4), "compulsory_bytes": f * (in_fb + out_fb),
                "input_sets_cycled": sets, "steps": args.steps, "rounds": args.rounds, "lib": os.path.basename(L.LIB_PATH),
                "measured": True}
        print(json.dumps(line), flush=True)
    del xs, ys, tmp
    torch.cuda.empty_cache()


def run_routes(name, shape, f, routes, in_bytes, out_bytes, args, ctx, torch, check=()):
    """routes: {route: step(i)} alternating region by region; check: pairs of routes whose frame-0 outputs must agree
    (each step(i) returns the tensor it wrote)."""
    stream = torch.cuda.current_stream()
    first = {}
    for rn, step in routes.items():
        y = step(0)
        torch.cuda.synchronize()
        first[rn] = (y.cpu().numpy().copy(), ctx.last_kernel())
    for a, b in check:
        if not np.array_equal(first[a][0], first[b][0]):
            raise SystemExit(f"{name}: route {a} differs from route {b}")
    times = {rn: [] for rn in routes}
    for rn, step in routes.items():
        for k in range(args.warmup):
            step(k)
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for rn, step in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for k in range(args.steps):
                step(r * args.steps + k)
            e1.record(stream)
            e1.synchronize()
            times[rn].append(e0.elapsed_time(e1) * 1e3 / args.steps)
    for rn in routes:
        us = statistics.median(times[rn])
        line = {"workload": name, "shape": shape, "frames": f, "route": rn, "kernel": first[rn][1],
                "us_per_step": round(us, 2), "us_all_regions": [round(v, 2) for v in times[rn]],
                "hbm_frac": round((in_bytes[rn] + out_bytes[rn]) / (us * 1e-6) / HBM_BPS, 4),
                "compulsory_bytes": in_bytes[rn] + out_bytes[rn], "steps": args.steps, "rounds": args.rounds,
                "lib": os.path.basename(L.LIB_PATH), "measured": True}
        print(json.dumps(line), flush=True)
    return {rn: statistics.median(times[rn]) for rn in routes}


TENSOR_WORKLOADS = {   # name: (in_w, in_h, out_w, out_h, channels, frames, layout, box)
    "T1": (3840, 2160, 1920, 1080, 3, 32, "chw", None),
    "T2": (3840, 2160, 1920, 1080, 3, 32, "hwc", None),
    "T4": (1920, 1080, 3840, 2160, 3, 32, "chw", None),
    "TP": (500, 375, 224, 224, 3, 256, "chw", (62.5, 0.0, 437.5, 375.0)),
}
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


class ParentLib:
    """The byte resize of another build of the C ABI (the parent commit's), loaded beside this one."""

    def __init__(self, path):
        import ctypes
        self.lib = ctypes.CDLL(path)
        self.h = ctypes.c_void_p()
        self.lib.lanczos_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
        self.lib.lanczos_resize_device_ex.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t,
                                                      ctypes.c_void_p]
        if hasattr(self.lib, "lanczos_resize_tensor16_device"):
            self.lib.lanczos_resize_tensor16_device.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int, ctypes.c_size_t,
                                                                                        ctypes.c_size_t, ctypes.c_void_p]
        self.lib.lanczos_destroy.argtypes = [ctypes.c_void_p]
        if self.lib.lanczos_create(ctypes.byref(self.h), 0) != 0:
            raise SystemExit(f"{path}: lanczos_create failed")
        self.byref = ctypes.byref

    def resize_tensor16_device(self, d, t, d_in, d_out, frames, stream):
        rc = self.lib.lanczos_resize_tensor16_device(self.h, self.byref(d), None, self.byref(t), d_in, d_out, frames, 0, 0, stream)
        if rc != 0:
            raise SystemExit(f"parent lanczos_resize_tensor16_device: {rc}")

    def resize_device(self, d, d_in, d_out, frames, stream, opts=None):
        rc = self.lib.lanczos_resize_device_ex(self.h, self.byref(d), self.byref(opts) if opts is not None else None, d_in,
                                               d_out, frames, 0, 0, stream)
        if rc != 0:
            raise SystemExit(f"parent lanczos_resize_device_ex: {rc}")

    def window_device(self, entry, d, window, t, d_in, d_out, frames, in_fs, out_fs, stream):
        """lanczos_resize_window_device (t None) or lanczos_resize_tensor[16]_window_device of the other build"""
        import ctypes
        fn = getattr(self.lib, entry)
        fn.argtypes = [ctypes.c_void_p] * (6 if t is None else 7) + [ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
        win = self.byref(L.resize_window(d, window)) if window is not None else None
        head = (self.h, self.byref(d), None, win) + (() if t is None else (self.byref(t),))
        rc = fn(*head, d_in, d_out, frames, in_fs, out_fs, stream)
        if rc != 0:
            raise SystemExit(f"parent {entry}: {rc}")

    def close(self):
        self.lib.lanczos_destroy(self.h)


def run_tensor(name, args, ctx, torch, parent):
    iw, ih, ow, oh, c, f, layout, box = TENSOR_WORKLOADS[name]
    in_fb, out_fb = iw * ih * c, ow * oh * c
    sets = max(2, -(-2 * 256 * 2 ** 20 // (f * in_fb)) + 1)
    gen = torch.Generator(device="cuda").manual_seed(7)
    xs = [torch.randint(0, 256, (f * in_fb,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(sets)]
    ys = [torch.empty(f * out_fb, dtype=torch.float32, device="cuda") for _ in range(sets)]
    tmp = torch.empty(f * out_fb, dtype=torch.uint8, device="cuda")
    d = L.resize_desc(iw, ih, ow, oh, c)
    opts = L.resize_opts(d, box=box) if box else None
    lut = torch.from_numpy(L.normalize_lut(c, IMAGENET_MEAN, IMAGENET_STD)).cuda()
    st = L.tensor_strides(layout, ow, oh, c)
    shape = (1, c, 1, 1) if layout == "chw" else (1, 1, 1, c)
    mean = torch.tensor(IMAGENET_MEAN, device="cuda").view(shape)
    std = torch.tensor(IMAGENET_STD, device="cuda").view(shape)
    s = torch.cuda.current_stream().cuda_stream
    seen = {}

    def tensor(path):
        def step(i):
            ctx.resize_force(path)
            ctx.resize_tensor_device(d, xs[i % sets].data_ptr(), ys[i % sets].data_ptr(), f, lut.data_ptr(), st, stream=s,
                                     opts=opts)
            seen[path] = ctx.last_tensor_route()
            return ys[i % sets][:out_fb].view(torch.int32)
        return step

    def bytes_(i):
        ctx.resize_force(L.RESIZE_AUTO)
        ctx.resize_device(d, xs[i % sets].data_ptr(), tmp.data_ptr(), f, 0, 0, s, opts=opts)
        return tmp[:out_fb]

    def bytes_torch(i):
        bytes_(i)
        t = tmp.view(f, oh, ow, c)
        t = t.permute(0, 3, 1, 2) if layout == "chw" else t
        return t.float().div(255).sub(mean).div(std).contiguous().view(-1)[:out_fb].view(torch.int32)

    def parent_bytes(i):
        parent.resize_device(d, xs[i % sets].data_ptr(), tmp.data_ptr(), f, s, opts)
        return tmp[:out_fb]

    def copy(i):
        ys[(i + 1) % sets].copy_(ys[i % sets], non_blocking=True)
        return ys[(i + 1) % sets][:out_fb].view(torch.int32)

    routes = {"fused": tensor(L.RESIZE_AUTO), "converted": tensor(L.RESIZE_CONVERT), "bytes_torch": bytes_torch, "bytes": bytes_}
    if parent is not None:
        routes["parent_bytes"] = parent_bytes
    routes["copy"] = copy
    inb = {rn: f * in_fb for rn in routes}
    outb = {rn: 4 * f * out_fb for rn in routes}
    outb["bytes"] = outb["parent_bytes"] = f * out_fb
    inb["copy"] = 4 * f * out_fb
    us = run_routes(name, f"{iw}x{ih}->{ow}x{oh} C{c} {layout}" + (f" box {box}" if box else ""), f, routes, inb, outb, args,
                    ctx, torch, check=(("fused", "converted"),))
    ctx.resize_force(L.RESIZE_AUTO)
    if (seen[L.RESIZE_AUTO], seen[L.RESIZE_CONVERT]) != (L.TENSOR_FUSED, L.TENSOR_CONVERTED):
        raise SystemExit(f"{name}: routes {seen}")
    base = us.get("parent_bytes", us["bytes"])
    print(json.dumps({"workload": name, "fused_over_converted": round(us["fused"] / us["converted"], 3),
                      "fused_over_bytes_torch": round(us["fused"] / us["bytes_torch"], 3),
                      "fused_minus_byte_resize_us": round(us["fused"] - base, 2), "byte_resize": "parent" if parent else "this build",
                      "copy_of_float_output_us": round(us["copy"], 2), "measured": True}), flush=True)
    del xs, ys, tmp
    torch.cuda.empty_cache()


def run_tensor16(name, args, ctx, torch):
    iw, ih, ow, oh, c, f, layout, box = TENSOR_WORKLOADS[name[:-1]]
    in_fb, out_fb = iw * ih * c, ow * oh * c
    sets = max(2, -(-2 * 256 * 2 ** 20 // (f * in_fb)) + 1)
    gen = torch.Generator(device="cuda").manual_seed(7)
    xs = [torch.randint(0, 256, (f * in_fb,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(sets)]
    ys = [torch.empty(f * out_fb, dtype=torch.bfloat16, device="cuda") for _ in range(sets)]
    wide = [torch.empty(f * out_fb, dtype=torch.float32, device="cuda") for _ in range(sets)]
    d = L.resize_desc(iw, ih, ow, oh, c)
    opts = L.resize_opts(d, box=box) if box else None
    lut = torch.from_numpy(L.normalize_lut(c, IMAGENET_MEAN, IMAGENET_STD)).cuda()
    lut16 = torch.from_numpy(L.normalize_lut(c, IMAGENET_MEAN, IMAGENET_STD, dtype="bfloat16").view(np.int16)).cuda()
    st = L.tensor_strides(layout, ow, oh, c)
    s = torch.cuda.current_stream().cuda_stream
    seen = {}

    def tensor16(path):
        def step(i):
            ctx.resize_force(path)
            ctx.resize_tensor_device(d, xs[i % sets].data_ptr(), ys[i % sets].data_ptr(), f, lut16.data_ptr(), st, stream=s,
                                     opts=opts, dtype="bfloat16")
            seen[path] = ctx.last_tensor_route()
            return ys[i % sets][:out_fb].view(torch.int16)
        return step

    def f32(i):
        ctx.resize_force(L.RESIZE_AUTO)
        ctx.resize_tensor_device(d, xs[i % sets].data_ptr(), wide[i % sets].data_ptr(), f, lut.data_ptr(), st, stream=s,
                                 opts=opts)
        return wide[i % sets][:out_fb].view(torch.int32)

    def f32_cast(i):
        f32(i)
        return wide[i % sets].to(torch.bfloat16)[:out_fb].view(torch.int16)

    routes = {"fused": tensor16(L.RESIZE_AUTO), "converted": tensor16(L.RESIZE_CONVERT), "f32_cast": f32_cast, "f32": f32}
    inb = {rn: f * in_fb for rn in routes}
    outb = {rn: 2 * f * out_fb for rn in routes}
    outb["f32"] = 4 * f * out_fb
    us = run_routes(name, f"{iw}x{ih}->{ow}x{oh} C{c} {layout} bfloat16" + (f" box {box}" if box else ""), f, routes, inb, outb,
                    args, ctx, torch, check=(("fused", "converted"), ("fused", "f32_cast")))
    ctx.resize_force(L.RESIZE_AUTO)
    if (seen[L.RESIZE_AUTO], seen[L.RESIZE_CONVERT]) != (L.TENSOR_FUSED, L.TENSOR_CONVERTED):
        raise SystemExit(f"{name}: routes {seen}")
    print(json.dumps({"workload": name, "fused_over_f32_cast": round(us["fused"] / us["f32_cast"], 3),
                      "converted_over_f32_cast": round(us["converted"] / us["f32_cast"], 3),
                      "fused_over_converted": round(us["fused"] / us["converted"], 3),
                      "fused_over_f32": round(us["fused"] / us["f32"], 3), "measured": True}), flush=True)
    del xs, ys, wide
    torch.cuda.empty_cache()


NORM_WORKLOADS = {   # name: (in_w, in_h, out_w, out_h, channels, frames, sample bits, element dtype)
    "N16": (3840, 2160, 1920, 1080, 3, 32, 16, "float32"),
    "N16h": (3840, 2160, 1920, 1080, 3, 32, 16, "bfloat16"),
    "N32": (3840, 2160, 1920, 1080, 3, 32, 32, "float32"),
    "NP16": (512, 512, 224, 224, 1, 256, 16, "float32"),
}


def run_norm(name, args, ctx, torch, parent):
    iw, ih, ow, oh, c, f, bits, dtype = NORM_WORKLOADS[name]
    B, E = bits // 8, 4 if dtype == "float32" else 2
    in_fb, out_fb = iw * ih * c, ow * oh * c   # samples / elements of a frame
    sets = max(2, -(-2 * 256 * 2 ** 20 // (f * in_fb * B)) + 1)
    gen = torch.Generator(device="cuda").manual_seed(7)
    if bits == 16:   # every 16-bit pattern, held as int16 and read as uint16
        xs = [torch.randint(-32768, 32768, (f * in_fb,), dtype=torch.int16, device="cuda", generator=gen) for _ in range(sets)]
    else:
        xs = [torch.rand(f * in_fb, dtype=torch.float32, device="cuda", generator=gen) for _ in range(sets)]
    edt = torch.float32 if E == 4 else torch.bfloat16
    bits_t = torch.int32 if E == 4 else torch.int16
    ys = [torch.empty(f * out_fb, dtype=edt, device="cuda") for _ in range(sets)]
    tmp = torch.empty(f * out_fb, dtype=torch.uint16 if bits == 16 else torch.float32, device="cuda")
    d = L.resize_desc(iw, ih, ow, oh, c, bits=16 if bits == 16 else 8, f32=bits == 32)
    div = (65535.0,) * c if bits == 16 else (1.0,) * c
    mean_v, std_v = IMAGENET_MEAN[:c], IMAGENET_STD[:c]
    nrm = L.tensor_norm(L.tensor_strides("chw", ow, oh, c), div, mean_v, std_v, dtype, tuple(range(c)))
    shape = (1, c, 1, 1)
    t_div = torch.tensor(div, device="cuda").view(shape)
    t_mean = torch.tensor(mean_v, device="cuda").view(shape)
    t_std = torch.tensor(std_v, device="cuda").view(shape)
    s = torch.cuda.current_stream().cuda_stream
    seen = {}

    def norm(path):
        def step(i):
            ctx.resize_force(path)
            ctx.resize_tensor_norm_device(d, xs[i % sets].data_ptr(), ys[i % sets].data_ptr(), f, nrm, stream=s)
            seen[path] = ctx.last_tensor_route()
            return ys[i % sets][:out_fb].view(bits_t)
        return step

    def samples(i):
        ctx.resize_force(L.RESIZE_AUTO)
        ctx.resize_device(d, xs[i % sets].data_ptr(), tmp.data_ptr(), f, 0, 0, s)
        return tmp[:out_fb].view(torch.int16 if bits == 16 else torch.int32)

    def samples_torch(i):
        samples(i)
        t = tmp.view(f, oh, ow, c).permute(0, 3, 1, 2).float().div(t_div).sub(t_mean).div(t_std)
        t = t if E == 4 else t.to(torch.bfloat16)
        return t.contiguous().view(-1)[:out_fb].view(bits_t)

    def parent_samples(i):
        parent.resize_device(d, xs[i % sets].data_ptr(), tmp.data_ptr(), f, s)
        return tmp[:out_fb].view(torch.int16 if bits == 16 else torch.int32)

    def copy(i):
        ys[(i + 1) % sets].copy_(ys[i % sets], non_blocking=True)
        return ys[(i + 1) % sets][:out_fb].view(bits_t)

    routes = {"fused": norm(L.RESIZE_AUTO), "converted": norm(L.RESIZE_CONVERT), "samples_torch": samples_torch, "samples": samples}
    if parent is not None:
        routes["parent_samples"] = parent_samples
    routes["copy"] = copy
    inb = {rn: B * f * in_fb for rn in routes}
    outb = {rn: E * f * out_fb for rn in routes}
    outb["samples"] = outb["parent_samples"] = B * f * out_fb
    inb["copy"] = E * f * out_fb
    us = run_routes(name, f"{iw}x{ih}->{ow}x{oh} C{c} {'u16' if bits == 16 else 'f32'} -> {dtype} chw", f, routes, inb, outb, args, ctx, torch,
                    check=(("fused", "converted"), ("fused", "samples_torch")))
    ctx.resize_force(L.RESIZE_AUTO)
    if (seen[L.RESIZE_AUTO], seen[L.RESIZE_CONVERT]) != (L.TENSOR_FUSED, L.TENSOR_CONVERTED):
        raise SystemExit(f"{name}: routes {seen}")
    base = us.get("parent_samples", us["samples"])
    print(json.dumps({"workload": name, "fused_over_converted": round(us["fused"] / us["converted"], 3),
                      "fused_over_samples_torch": round(us["fused"] / us["samples_torch"], 3),
                      "fused_minus_sample_resize_us": round(us["fused"] - base, 2), "sample_resize": "parent" if parent else "this build",
                      "torch_stages_us": round(us["samples_torch"] - us["samples"], 2),
                      "copy_of_element_output_us": round(us["copy"], 2), "measured": True}), flush=True)
    del xs, ys, tmp
    torch.cuda.empty_cache()


WINDOW_WORKLOADS = {   # name: (in_w, in_h, out_w, out_h, channels, frames, crop (w, h) taken from the centre, bfloat16 CHW out)
    "WIN1": (500, 375, 341, 256, 3, 256, (224, 224), False),
    "WIN1h": (500, 375, 341, 256, 3, 256, (224, 224), True),
    "WIN2": (3840, 2160, 1920, 1080, 3, 32, (1280, 720), False),
    "WINC": (341, 256, 341, 256, 3, 256, (224, 224), False),   # neither axis runs: the crop copy against torch's slice
}


def run_window(name, args, ctx, torch, parent):
    iw, ih, ow, oh, c, f, crop, half = WINDOW_WORKLOADS[name]
    window = L.center_window(ow, oh, *crop)
    x0, y0, w, h = window
    in_fb, out_fb, win_fb = iw * ih * c, ow * oh * c, w * h * c
    sets = max(2, -(-2 * 256 * 2 ** 20 // (f * in_fb)) + 1)
    gen = torch.Generator(device="cuda").manual_seed(7)
    dt = torch.bfloat16 if half else torch.uint8
    xs = [torch.randint(0, 256, (f * in_fb,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(sets)]
    ys = [torch.empty(f * win_fb, dtype=dt, device="cuda") for _ in range(sets)]      # windowed results
    fulls = [torch.empty(f * out_fb, dtype=dt, device="cuda") for _ in range(sets)]   # full results
    d = L.resize_desc(iw, ih, ow, oh, c)
    win = L.resize_window(d, window)
    s = torch.cuda.current_stream().cuda_stream
    ctx.resize_force(L.RESIZE_AUTO)
    if half:
        lut16 = torch.from_numpy(L.normalize_lut(c, IMAGENET_MEAN, IMAGENET_STD, dtype="bfloat16").view(np.int16)).cuda()
        t_win = L.tensor16_out(lut16.data_ptr(), L.tensor_strides("chw", w, h, c))
        t_full = L.tensor16_out(lut16.data_ptr(), L.tensor_strides("chw", ow, oh, c))
    bits = (lambda y: y.view(torch.int16)) if half else (lambda y: y)

    def windowed(i):
        if half:
            ctx.resize_tensor_device(d, xs[i % sets].data_ptr(), ys[i % sets].data_ptr(), f, None, t_win, stream=s, window=win)
        else:
            ctx.resize_device(d, xs[i % sets].data_ptr(), ys[i % sets].data_ptr(), f, 0, 0, s, window=win)
        return bits(ys[i % sets][:win_fb])

    def full(i):
        if half:
            ctx.resize_tensor_device(d, xs[i % sets].data_ptr(), fulls[i % sets].data_ptr(), f, None, t_full, stream=s)
        else:
            ctx.resize_device(d, xs[i % sets].data_ptr(), fulls[i % sets].data_ptr(), f, 0, 0, s)
        return bits(fulls[i % sets][:out_fb])

    def full_slice(i):
        full(i)
        if half:
            t = fulls[i % sets].view(f, c, oh, ow)[:, :, y0:y0 + h, x0:x0 + w]
        else:
            t = fulls[i % sets].view(f, oh, ow, c)[:, y0:y0 + h, x0:x0 + w]
        return bits(t.contiguous().view(-1)[:win_fb])

    def parent_full(i):
        if half:
            parent.resize_tensor16_device(d, t_full, xs[i % sets].data_ptr(), fulls[i % sets].data_ptr(), f, s)
        else:
            parent.resize_device(d, xs[i % sets].data_ptr(), fulls[i % sets].data_ptr(), f, s)
        return bits(fulls[i % sets][:out_fb])

    routes = {"windowed": windowed, "full_slice": full_slice, "full": full}
    if parent is not None:
        routes["parent_full"] = parent_full
    e = 2 if half else 1
    rect = L.resize_window_source(d, win)
    inb = {rn: f * in_fb for rn in routes}
    inb["windowed"] = f * (rect[2] - rect[0]) * (rect[3] - rect[1]) * c
    outb = {rn: e * f * out_fb for rn in routes}
    outb["windowed"] = e * f * win_fb
    outb["full_slice"] = e * f * (out_fb + 2 * win_fb)
    us = run_routes(name, f"{iw}x{ih}->{ow}x{oh} C{c} window {window}" + (" bfloat16 chw" if half else ""), f, routes, inb, outb,
                    args, ctx, torch, check=(("windowed", "full_slice"),))
    pw, pf = L.resize_window_plan_host(d, win, f), L.resize_window_plan_host(d, None, f)
    plan = lambda p: {"fused": p.inner.fused, "K": p.inner.K, "strips": p.inner.strips, "chunks": p.inner.chunks,
                      "rows_per_chunk": p.inner.rows_per_chunk, "mid_rows": p.mid_rows}
    print(json.dumps({"workload": name, "windowed_over_full_slice": round(us["windowed"] / us["full_slice"], 3),
                      "windowed_over_full": round(us["windowed"] / us["full"], 3),
                      "windowed_over_parent_full": round(us["windowed"] / us["parent_full"], 3) if parent else None,
                      "full_over_parent_full": round(us["full"] / us["parent_full"], 3) if parent else None,
                      "pixels_full_over_window": round(ow * oh / (w * h), 3), "source_rect": rect,
                      "plan_windowed": plan(pw), "plan_full": plan(pf), "measured": True}), flush=True)
    del xs, ys, fulls
    torch.cuda.empty_cache()


VIEW_WORKLOADS = {   # name: (in_w, in_h, out_w, out_h, channels, alpha, frames, crop (w, h) from the centre or None, channels_out, per-frame flips, bfloat16)
    "V1": (3840, 2160, 1920, 1080, 3, False, 32, None, (2, 1, 0), True, False),      # T1's shape, BGR -> RGB, every other frame mirrored
    "V1h": (3840, 2160, 1920, 1080, 3, False, 32, None, (2, 1, 0), True, True),
    "VW": (500, 375, 341, 256, 4, True, 256, (224, 224), (0, 1, 2), False, False),   # WIN1's shape on RGBA frames, alpha dropped
    "VWh": (500, 375, 341, 256, 4, True, 256, (224, 224), (0, 1, 2), False, True),
}


def run_view(name, args, ctx, torch):
    """A tensor view (channel map, per-frame flips) against what it replaces -- the tensor call without one followed by torch's
    index / where(flip) / .contiguous() on the same stream -- and against that tensor call alone.  CHW, the ImageNet table in
    output order."""
    iw, ih, ow, oh, c, alpha, f, crop, src, flips, half = VIEW_WORKLOADS[name]
    window = L.center_window(ow, oh, *crop) if crop else None
    w, h = (window[2], window[3]) if window else (ow, oh)
    oc = len(src)
    in_fb, full_fb, view_fb = iw * ih * c, w * h * c, w * h * oc
    sets = max(2, -(-2 * 256 * 2 ** 20 // (f * in_fb)) + 1)
    gen = torch.Generator(device="cuda").manual_seed(7)
    dt = torch.bfloat16 if half else torch.float32
    dtype = "bfloat16" if half else "float32"
    xs = [torch.randint(0, 256, (f * in_fb,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(sets)]
    ys = [torch.empty(f * view_fb, dtype=dt, device="cuda") for _ in range(sets)]    # the view's results
    fulls = [torch.empty(f * full_fb, dtype=dt, device="cuda") for _ in range(sets)]   # every source channel, unflipped
    d = L.resize_desc(iw, ih, ow, oh, c, alpha=alpha)
    win = L.resize_window(d, window) if window else None
    # the table in output order, and the same rows in source order for the call without a map (a dropped channel gets zeros)
    lut_out = L.normalize_lut(oc, IMAGENET_MEAN[:oc], IMAGENET_STD[:oc], dtype=dtype)
    lut_src = np.zeros((c, 256), dtype=lut_out.dtype)
    for o, sc in enumerate(src):
        lut_src[sc] = lut_out[o]
    as_dev = lambda a: torch.from_numpy(a.view(np.int16) if half else a).cuda()
    d_out, d_src = as_dev(lut_out), as_dev(lut_src)
    fl = np.array([k & 1 for k in range(f)], dtype=np.uint8) if flips else None
    d_flip = torch.from_numpy(fl).cuda() if flips else None
    mask = torch.from_numpy(fl.astype(bool)).cuda().view(f, 1, 1, 1) if flips else None
    index = torch.tensor(src, device="cuda")
    st_view, st_full = L.tensor_strides("chw", w, h, oc), L.tensor_strides("chw", w, h, c)
    s = torch.cuda.current_stream().cuda_stream
    bits = (lambda y: y.view(torch.int16)) if half else (lambda y: y.view(torch.int32))
    seen = {}

    def view(path):
        def step(i):
            ctx.resize_force(path)
            ctx.resize_tensor_device(d, xs[i % sets].data_ptr(), ys[i % sets].data_ptr(), f, d_out.data_ptr(), st_view, stream=s,
                                     dtype=dtype, window=win, channels_out=src, d_flip=d_flip.data_ptr() if flips else None)
            seen[path] = ctx.last_tensor_route()
            return bits(ys[i % sets][:view_fb])
        return step

    def tensor(i):
        ctx.resize_force(L.RESIZE_AUTO)
        ctx.resize_tensor_device(d, xs[i % sets].data_ptr(), fulls[i % sets].data_ptr(), f, d_src.data_ptr(), st_full, stream=s,
                                 dtype=dtype, window=win)
        return bits(fulls[i % sets][:full_fb])

    def tensor_torch(i):
        tensor(i)
        t = fulls[i % sets].view(f, c, h, w)
        t = t[:, :oc] if src == tuple(range(oc)) else t[:, index]
        if flips:
            t = torch.where(mask, t.flip(-1), t)
        return bits(t.contiguous().view(-1)[:view_fb])

    routes = {"view": view(L.RESIZE_AUTO), "view_converted": view(L.RESIZE_CONVERT), "tensor_torch": tensor_torch, "tensor": tensor}
    e = 2 if half else 4
    inb = {rn: f * in_fb for rn in routes}
    outb = {rn: e * f * view_fb for rn in routes}
    outb["tensor"] = e * f * full_fb
    us = run_routes(name, f"{iw}x{ih}->{ow}x{oh} C{c}{' alpha' if alpha else ''} -> channels {src}" +
                    (f" window {window}" if window else "") + (" flips 0,1,0,1.." if flips else "") + f" chw {dtype}", f, routes,
                    inb, outb, args, ctx, torch, check=(("view", "view_converted"), ("view", "tensor_torch")))
    ctx.resize_force(L.RESIZE_AUTO)
    if (seen[L.RESIZE_AUTO], seen[L.RESIZE_CONVERT]) != (L.TENSOR_FUSED, L.TENSOR_CONVERTED):
        raise SystemExit(f"{name}: routes {seen}")
    print(json.dumps({"workload": name, "view_over_tensor_torch": round(us["view"] / us["tensor_torch"], 3),
                      "view_over_tensor": round(us["view"] / us["tensor"], 3),
                      "view_over_view_converted": round(us["view"] / us["view_converted"], 3), "measured": True}), flush=True)
    del xs, ys, fulls
    torch.cuda.empty_cache()


CROPS_WORKLOADS = {   # name: (in_w, in_h, out_w, out_h, channels, frames, crop (w, h), bfloat16)
    "RC1": (500, 375, 341, 256, 3, 256, (224, 224), False),
    "RC1h": (500, 375, 341, 256, 3, 256, (224, 224), True),
    "RCC": (256, 256, 256, 256, 3, 256, (224, 224), False),
}


def run_crops(name, args, ctx, torch):
    """A crop origin per frame against the view call on the full output plus torch's gather, against the centred uniform window
    (the floor) and against its own converted route."""
    iw, ih, ow, oh, c, f, (w, h), half = CROPS_WORKLOADS[name]
    in_fb, full_fb, crop_fb = iw * ih * c, ow * oh * c, w * h * c
    sets = max(2, -(-2 * 256 * 2 ** 20 // (f * in_fb)) + 1)
    gen = torch.Generator(device="cuda").manual_seed(7)
    dt = torch.bfloat16 if half else torch.float32
    dtype = "bfloat16" if half else "float32"
    xs = [torch.randint(0, 256, (f * in_fb,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(sets)]
    ys = [torch.empty(f * crop_fb, dtype=dt, device="cuda") for _ in range(sets)]
    fulls = [torch.empty(f * full_fb, dtype=dt, device="cuda") for _ in range(sets)]
    d = L.resize_desc(iw, ih, ow, oh, c)
    lut = L.normalize_lut(c, IMAGENET_MEAN[:c], IMAGENET_STD[:c], dtype=dtype)
    d_lut = torch.from_numpy(lut.view(np.int16) if half else lut).cuda()
    rng = np.random.default_rng(11)
    org = np.stack([rng.integers(0, ow - w + 1, f), rng.integers(0, oh - h + 1, f)], axis=1).astype(np.int32)
    fl = np.array([k & 1 for k in range(f)], dtype=np.uint8)
    d_org, d_flip = torch.from_numpy(org).cuda(), torch.from_numpy(fl).cuda()
    # the gather's index tensors: the rows of every frame and its (mirrored where the frame is) columns
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cols = org[:, :1] + np.where(fl[:, None] == 1, np.arange(w)[::-1][None], np.arange(w)[None])
    rows = org[:, 1:] + np.arange(h)[None]
    g_y, g_x = dev(rows).view(f, 1, h, 1).expand(f, c, h, ow), dev(cols).view(f, 1, 1, w).expand(f, c, h, w)
    row_of = dev((np.arange(f)[:, None, None] * c + np.arange(c)[None, :, None]) * oh + rows[:, None, :]).view(-1)
    g_x2 = g_x.reshape(f * c * h, w)
    win = L.resize_window(d, L.center_window(ow, oh, w, h))
    st_crop, st_full = L.tensor_strides("chw", w, h, c), L.tensor_strides("chw", ow, oh, c)
    s = torch.cuda.current_stream().cuda_stream
    bits = (lambda y: y.view(torch.int16)) if half else (lambda y: y.view(torch.int32))
    src = tuple(range(c))
    seen = {}

    def crops(path):
        def step(i):
            ctx.resize_force(path)
            ctx.resize_tensor_device(d, xs[i % sets].data_ptr(), ys[i % sets].data_ptr(), f, d_lut.data_ptr(), st_crop, stream=s,
                                     dtype=dtype, channels_out=src, d_flip=d_flip.data_ptr(), crop=(w, h), d_origin=d_org.data_ptr())
            seen[path] = ctx.last_tensor_route()
            return bits(ys[i % sets][:crop_fb])
        return step

    def full_gather(i):
        ctx.resize_force(L.RESIZE_AUTO)
        ctx.resize_tensor_device(d, xs[i % sets].data_ptr(), fulls[i % sets].data_ptr(), f, d_lut.data_ptr(), st_full, stream=s,
                                 dtype=dtype, channels_out=src)
        if half:
            t = fulls[i % sets].view(f, c, oh, ow).gather(2, g_y).gather(3, g_x)
        else:
            t = fulls[i % sets].view(f * c * oh, ow).index_select(0, row_of).gather(1, g_x2)
        return bits(t.view(-1)[:crop_fb])

    def window_center(i):
        ctx.resize_force(L.RESIZE_AUTO)
        ctx.resize_tensor_device(d, xs[i % sets].data_ptr(), ys[i % sets].data_ptr(), f, d_lut.data_ptr(), st_crop, stream=s,
                                 dtype=dtype, window=win, channels_out=src, d_flip=d_flip.data_ptr())
        return bits(ys[i % sets][:crop_fb])

    routes = {"crops": crops(L.RESIZE_AUTO), "crops_converted": crops(L.RESIZE_CONVERT), "full_gather": full_gather,
              "window_center": window_center}
    e = 2 if half else 4
    inb = {rn: f * in_fb for rn in routes}
    outb = {rn: e * f * crop_fb for rn in routes}
    us = run_routes(name, f"{iw}x{ih}->{ow}x{oh} C{c} random {w}x{h} crops, flips 0,1,0,1.. chw {dtype}", f, routes, inb, outb,
                    args, ctx, torch, check=(("crops", "crops_converted"), ("crops", "full_gather")))
    ctx.resize_force(L.RESIZE_AUTO)
    plan = L.resize_crops_plan_host(d, (w, h), f).inner
    if seen[L.RESIZE_CONVERT] != L.TENSOR_CONVERTED or seen[L.RESIZE_AUTO] != (L.TENSOR_FUSED if plan.fused else L.TENSOR_CONVERTED):
        raise SystemExit(f"{name}: routes {seen}")
    print(json.dumps({"workload": name, "crops_over_full_gather": round(us["crops"] / us["full_gather"], 3),
                      "crops_over_window_center": round(us["crops"] / us["window_center"], 3),
                      "crops_over_crops_converted": round(us["crops"] / us["crops_converted"], 3),
                      "auto_route": seen[L.RESIZE_AUTO],
                      "plan": {k: getattr(plan, k) for k in ("fused", "K", "strips", "chunks", "ring_rows", "stage_rows", "stage_dw",
                                                             "lds_bytes")}, "measured": True}), flush=True)
    del xs, ys, fulls
    torch.cuda.empty_cache()


SOURCE_WORKLOADS = {   # name: (in_w, in_h, out_w, out_h, frames, planar, row alignment or -padding (bytes), crop (w, h) from the centre, tensor dtype or None, channels, alpha)
    "SRC1": (3840, 2160, 1920, 1080, 32, True, 1, None, None, 3, False),
    "SRC1h": (3840, 2160, 1920, 1080, 32, True, 1, None, "bfloat16", 3, False),
    "SRCP": (500, 375, 341, 256, 256, True, 1, (224, 224), "float32", 3, False),
    "SRCW": (1920, 1080, 3840, 2160, 32, False, 256, None, None, 3, False),
    "SRCA": (500, 375, 341, 256, 256, False, -6, None, None, 4, True),      # RGBA rows of 2006 bytes: the row-shift ALPHA instances
    "SRCAh": (500, 375, 341, 256, 256, False, -6, None, "bfloat16", 4, True),
}


def run_source(name, args, ctx, torch):
    """A source layout (lanczos_resize_source) against what it replaces: direct (the kernel reads the planar or pitched frames),
    packed (the same request under RESIZE_CONVERT: k_rs_pack_source first), torch_repack (permute(0, 2, 3, 1).contiguous(), or
    the slice's .contiguous(), then the call without a source) and floor (that call alone on frames already packed).  RGB8;
    tensors are normalised CHW."""
    iw, ih, ow, oh, f, planar, align, crop, dtype, c, alpha = SOURCE_WORKLOADS[name]
    window = L.center_window(ow, oh, *crop) if crop else None
    w, h = (window[2], window[3]) if window else (ow, oh)
    d = L.resize_desc(iw, ih, ow, oh, c, alpha=alpha)
    win = L.resize_window(d, window) if window else None
    pitch = iw * c - align if align < 0 else -(-iw * c // align) * align
    src = L.resize_source(d, "planar") if planar else L.resize_source(d, "interleaved", row_stride=pitch)
    L.resize_source_validate(d, src)
    src_fb = iw * ih * c if planar else ih * pitch          # bytes of a frame as the caller holds it
    in_fb = iw * ih * c
    elem = {None: 1, "float32": 4, "bfloat16": 2}[dtype]
    out_fb = w * h * c
    sets = max(2, -(-2 * 256 * 2 ** 20 // (f * src_fb)) + 1)
    gen = torch.Generator(device="cuda").manual_seed(11)
    xs = [torch.randint(0, 256, (f * src_fb,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(sets)]
    # the same frames already packed, for the floor
    if planar:
        packed = [x.view(f, c, ih, iw).permute(0, 2, 3, 1).contiguous() for x in xs]
    else:
        packed = [x.view(f, ih, pitch)[:, :, :iw * c].contiguous() for x in xs]
    odt = {None: torch.uint8, "float32": torch.float32, "bfloat16": torch.bfloat16}[dtype]
    ys = [torch.empty(f * out_fb, dtype=odt, device="cuda") for _ in range(sets)]
    bits = {1: (lambda y: y), 4: (lambda y: y.view(torch.int32)), 2: (lambda y: y.view(torch.int16))}[elem]
    d_lut = None
    if dtype:
        lut = L.normalize_lut(c, (IMAGENET_MEAN + (0.5,))[:c], (IMAGENET_STD + (0.25,))[:c], dtype=dtype)
        d_lut = torch.from_numpy(lut.view(np.int16) if elem == 2 else lut).cuda()
    st = L.tensor_strides("chw", w, h, c)
    s = torch.cuda.current_stream().cuda_stream
    seen = {}

    def call(x_ptr, y, source):
        if dtype:
            ctx.resize_tensor_device(d, x_ptr, y.data_ptr(), f, d_lut.data_ptr(), st, stream=s, dtype=dtype, window=win, source=source)
        else:
            ctx.resize_device(d, x_ptr, y.data_ptr(), f, stream=s, window=win, source=source)

    def with_source(path):
        def step(i):
            ctx.resize_force(path)
            call(xs[i % sets].data_ptr(), ys[i % sets], src)
            seen[path] = ctx.last_source_route()
            return bits(ys[i % sets][:out_fb])
        return step

    def torch_repack(i):
        ctx.resize_force(L.RESIZE_AUTO)
        x = xs[i % sets]
        t = x.view(f, c, ih, iw).permute(0, 2, 3, 1).contiguous() if planar else x.view(f, ih, pitch)[:, :, :iw * c].contiguous()
        call(t.data_ptr(), ys[i % sets], None)
        return bits(ys[i % sets][:out_fb])

    def floor(i):
        ctx.resize_force(L.RESIZE_AUTO)
        call(packed[i % sets].data_ptr(), ys[i % sets], None)
        return bits(ys[i % sets][:out_fb])

    routes = {"direct": with_source(L.RESIZE_FUSED), "packed": with_source(L.RESIZE_CONVERT), "auto": with_source(L.RESIZE_AUTO),
              "torch_repack": torch_repack, "floor": floor}
    inb = {rn: f * in_fb for rn in routes}
    outb = {rn: elem * f * out_fb for rn in routes}
    us = run_routes(name, f"{iw}x{ih}->{ow}x{oh} C{c}{' alpha' if alpha else ''} {'planar' if planar else f'rows pitched to {pitch}'}" +
                    (f" window {window}" if window else "") + (f" chw {dtype}" if dtype else " bytes"), f, routes, inb, outb, args,
                    ctx, torch, check=(("direct", "packed"), ("direct", "torch_repack"), ("direct", "floor"), ("direct", "auto")))
    ctx.resize_force(L.RESIZE_AUTO)
    if (seen[L.RESIZE_FUSED], seen[L.RESIZE_CONVERT]) != (L.SOURCE_DIRECT, L.SOURCE_PACKED):
        raise SystemExit(f"{name}: routes {seen}")
    print(json.dumps({"workload": name, "auto_route": {L.SOURCE_DIRECT: "direct", L.SOURCE_PACKED: "packed"}[seen[L.RESIZE_AUTO]],
                      "direct_over_packed": round(us["direct"] / us["packed"], 3),
                      "direct_over_torch_repack": round(us["direct"] / us["torch_repack"], 3),
                      "packed_over_torch_repack": round(us["packed"] / us["torch_repack"], 3),
                      "direct_over_floor": round(us["direct"] / us["floor"], 3), "measured": True}), flush=True)
    del xs, ys, packed
    torch.cuda.empty_cache()


DEST_WORKLOADS = {   # name: (in_w, in_h, out_w, out_h, frames, planar source, planar destination, row alignment (bytes), crop (w, h) from the centre, channels, alpha)
    "DST1": (3840, 2160, 1920, 1080, 32, False, True, 1, None, 3, False),
    "DSTP": (500, 375, 341, 256, 256, True, True, 1, None, 3, False),          # an odd width: three plane rows in four start off a dword
    "DSTPW": (500, 375, 341, 256, 256, True, True, 1, (224, 224), 3, False),
    "DSTW": (1920, 1080, 3840, 2160, 32, False, False, 256, None, 3, False),   # interleaved rows pitched to a multiple of 256 bytes
    "DSTA": (500, 375, 341, 256, 256, True, True, 1, None, 4, True),           # DSTP with four channels and LANCZOS_RESIZE_ALPHA
    "DST4": (3840, 2160, 1920, 1080, 32, False, True, 1, None, 4, False),      # DST1 with four channels
}


def run_dest(name, args, ctx, torch):
    """A destination layout (lanczos_resize_dest) against what it replaces: direct (the fused kernel stores the planes or pitched
    rows itself; with a library built with -DLZ_RS_PLANAR_OUT_DWORDS, loaded through LANCZOS_LIB, this is the dword form of the
    planar epilogue), unpacked (the same request under RESIZE_CONVERT: k_rs_unpack_dest last), auto, torch_repack
    (the call without a destination, then permute(0, 3, 1, 2).contiguous(), or the copy into the pitched rows) and floor (that
    call alone).  RGB8, bytes out."""
    iw, ih, ow, oh, f, planar_in, planar_out, align, crop, c, alpha = DEST_WORKLOADS[name]
    window = L.center_window(ow, oh, *crop) if crop else None
    w, h = (window[2], window[3]) if window else (ow, oh)
    d = L.resize_desc(iw, ih, ow, oh, c, alpha=alpha)
    win = L.resize_window(d, window) if window else None
    pitch = -(-w * c // align) * align
    if not planar_out and pitch == w * c:     # already a multiple: one more unit, or the destination would be the tight one
        pitch += align
    dst = L.resize_dest(d, "planar", window=window) if planar_out else L.resize_dest(d, "interleaved", row_stride=pitch, window=window)
    L.resize_dest_validate(d, dst, window=window)
    src = L.resize_source(d, "planar") if planar_in else None
    in_fb, out_fb = iw * ih * c, w * h * c
    dst_fb = out_fb if planar_out else h * pitch            # bytes of a frame as the caller holds it
    sets = max(2, -(-2 * 256 * 2 ** 20 // (f * in_fb)) + 1)
    gen = torch.Generator(device="cuda").manual_seed(12)
    xs = [torch.randint(0, 256, (f * in_fb,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(sets)]
    if planar_in:   # the same frames interleaved, for the call without a layout
        packed = [x.view(f, c, ih, iw).permute(0, 2, 3, 1).contiguous() for x in xs]
    else:
        packed = xs
    ys = [torch.zeros(f * dst_fb, dtype=torch.uint8, device="cuda") for _ in range(sets)]
    tmp = torch.empty(f * out_fb, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    seen = {}

    def named(y):   # the bytes of frame 0 in one order, whatever the layout
        if planar_out:
            return y[:out_fb].view(c, h, w).permute(1, 2, 0).contiguous()
        return y[:dst_fb].view(h, pitch)[:, :w * c].contiguous().view(h, w, c)

    def with_dest(path):
        def step(i):
            ctx.resize_force(path)
            ctx.resize_device(d, xs[i % sets].data_ptr(), ys[i % sets].data_ptr(), f, stream=s, window=win, source=src, dest=dst)
            seen[path] = ctx.last_dest_route()
            return named(ys[i % sets])
        return step

    def torch_repack(i):
        ctx.resize_force(L.RESIZE_AUTO)
        ctx.resize_device(d, xs[i % sets].data_ptr(), tmp.data_ptr(), f, stream=s, window=win, source=src)
        y = ys[i % sets]
        if planar_out:
            y.view(f, c, h, w).copy_(tmp.view(f, h, w, c).permute(0, 3, 1, 2))
        else:
            y.view(f, h, pitch)[:, :, :w * c].copy_(tmp.view(f, h, w * c))
        return named(y)

    def floor(i):
        ctx.resize_force(L.RESIZE_AUTO)
        ctx.resize_device(d, packed[i % sets].data_ptr(), tmp.data_ptr(), f, stream=s, window=win)
        return tmp[:out_fb].view(h, w, c)

    routes = {"direct": with_dest(L.RESIZE_FUSED), "unpacked": with_dest(L.RESIZE_CONVERT), "auto": with_dest(L.RESIZE_AUTO),
              "torch_repack": torch_repack, "floor": floor}
    inb = {rn: f * in_fb for rn in routes}
    outb = {rn: f * out_fb for rn in routes}
    us = run_routes(name, f"{iw}x{ih}->{ow}x{oh} C{c}{' alpha' if alpha else ''} {'planar' if planar_in else 'interleaved'} in, " +
                    ("planar out" if planar_out else f"rows pitched to {pitch} out") + (f" window {window}" if window else ""), f, routes,
                    inb, outb, args, ctx, torch, check=(("direct", "unpacked"), ("direct", "torch_repack"), ("direct", "floor"), ("direct", "auto")))
    ctx.resize_force(L.RESIZE_AUTO)
    if (seen[L.RESIZE_FUSED], seen[L.RESIZE_CONVERT]) != (L.DEST_DIRECT, L.DEST_UNPACKED):
        raise SystemExit(f"{name}: routes {seen}")
    print(json.dumps({"workload": name, "auto_route": {L.DEST_DIRECT: "direct", L.DEST_UNPACKED: "unpacked"}[seen[L.RESIZE_AUTO]],
                      "direct_over_unpacked": round(us["direct"] / us["unpacked"], 3),
                      "direct_over_torch_repack": round(us["direct"] / us["torch_repack"], 3),
                      "unpacked_over_torch_repack": round(us["unpacked"] / us["torch_repack"], 3),
                      "direct_over_floor": round(us["direct"] / us["floor"], 3), "measured": True}), flush=True)
    del xs, ys, packed, tmp
    torch.cuda.empty_cache()


def run_gap(name, args, ctx, torch):
    iw, ih, ow, oh, c, a, f = WORKLOADS["W5"]
    in_fb, out_fb = iw * ih * c, ow * oh * c
    sets = max(2, -(-2 * 256 * 2 ** 20 // (f * in_fb)) + 1)
    gen = torch.Generator(device="cuda").manual_seed(7)
    xs = [torch.randint(0, 256, (f * in_fb,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(sets)]
    ys = [torch.empty(f * out_fb, dtype=torch.uint8, device="cuda") for _ in range(sets)]
    rw, rh = L.reduce_size(iw, ih, 12)
    red = torch.empty(f * rw * rh * c, dtype=torch.uint8, device="cuda")
    cp = torch.empty(f * in_fb, dtype=torch.uint8, device="cuda")
    d = L.resize_desc(iw, ih, ow, oh, c, a)
    opts = {g: L.resize_opts(d, reducing_gap=g) for g in (2.0, 3.0)}
    s = torch.cuda.current_stream().cuda_stream
    ctx.resize_force(L.RESIZE_AUTO)

    def resize(o):
        def step(i):
            ctx.resize_device(d, xs[i % sets].data_ptr(), ys[i % sets].data_ptr(), f, 0, 0, s, opts=o)
            return ys[i % sets][:out_fb]
        return step

    def reduce12(i):
        ctx.reduce_device(iw, ih, c, 12, xs[i % sets].data_ptr(), red.data_ptr(), f, stream=s)
        return red[:rw * rh * c]

    def copy(i):
        cp.copy_(xs[i % sets])
        return cp[:out_fb]

    routes = {"plain": resize(None), "gap2": resize(opts[2.0]), "gap3": resize(opts[3.0]), "reduce12": reduce12, "copy": copy}
    inb = {rn: f * in_fb for rn in routes}
    outb = {"plain": f * out_fb, "gap2": f * out_fb, "gap3": f * out_fb, "reduce12": f * rw * rh * c, "copy": f * in_fb}
    run_routes(name, f"{iw}x{ih}->{ow}x{oh} C{c} a{a}", f, routes, inb, outb, args, ctx, torch)
    del xs, ys, red, cp
    torch.cuda.empty_cache()


def run_box(name, out, args, ctx, torch):
    iw, ih, c, a, f = 7680, 4320, 3, 3, 8
    ow, oh = out
    box = (3000.3, 1700.6, 4281.1, 2420.2)
    padx, pady = int(a * max(1.0, (box[2] - box[0]) / ow)) + 2, int(a * max(1.0, (box[3] - box[1]) / oh)) + 2
    cx0, cy0 = int(box[0]) - padx, int(box[1]) - pady
    cx1, cy1 = int(box[2]) + 1 + padx, int(box[3]) + 1 + pady
    cw, ch = cx1 - cx0, cy1 - cy0
    tbox = (box[0] - cx0, box[1] - cy0, box[2] - cx0, box[3] - cy0)
    in_fb, out_fb, crop_fb = iw * ih * c, ow * oh * c, cw * ch * c
    sets = 3   # 8 frames of 8K are 796 MB: every step's source region is far behind the Infinity Cache by its next use
    gen = torch.Generator(device="cuda").manual_seed(7)
    xs = [torch.randint(0, 256, (f, ih, iw, c), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(sets)]
    ts = [x[:, cy0:cy1, cx0:cx1].contiguous() for x in xs]
    ys = [torch.empty(f * out_fb, dtype=torch.uint8, device="cuda") for _ in range(sets)]
    d, dt = L.resize_desc(iw, ih, ow, oh, c, a), L.resize_desc(cw, ch, ow, oh, c, a)
    o, ot = L.resize_opts(d, box=box), L.resize_opts(dt, box=tbox)
    s = torch.cuda.current_stream().cuda_stream

    def mk(desc, opt, src, path):
        def step(i):
            ctx.resize_force(path)
            ctx.resize_device(desc, src[i % sets].data_ptr(), ys[i % sets].data_ptr(), f, 0, 0, s, opts=opt)
            return ys[i % sets][:out_fb]
        return step

    routes = {"boxed_auto": mk(d, o, xs, L.RESIZE_AUTO), "tight_auto": mk(dt, ot, ts, L.RESIZE_AUTO),
              "boxed_two_pass": mk(d, o, xs, L.RESIZE_TWO_PASS), "tight_two_pass": mk(dt, ot, ts, L.RESIZE_TWO_PASS)}
    inb = {rn: f * crop_fb for rn in routes}
    outb = {rn: f * out_fb for rn in routes}
    # the tight box is the boxed one shifted by whole pixels, which a float rounds differently: bytes are compared between
    # the two paths of each, not between boxed and tight
    run_routes(name, f"box {box} of {iw}x{ih}->{ow}x{oh} C{c} a{a}; tight {cw}x{ch}", f, routes, inb, outb, args, ctx, torch,
               check=(("boxed_auto", "boxed_two_pass"), ("tight_auto", "tight_two_pass")))
    ctx.resize_force(L.RESIZE_AUTO)
    del xs, ts, ys
    torch.cuda.empty_cache()


YCC_WORKLOADS = {   # name: (in_w, in_h, out_w, out_h, frames, layout, crop (w, h) from the centre or None, tensor dtype or None)
    "YC1": (3840, 2160, 1920, 1080, 32, "nv12", None, "bfloat16"),
    "YC2": (500, 375, 341, 256, 256, "i420", (224, 224), "float32"),
    "YC3": (1920, 1080, 3840, 2160, 32, "nv12", None, None),
}


def run_ycc(name, args, ctx, torch, parent):
    """YCbCr frames: (a) `ycc`, the one call; (b) `torch_convert`, what it replaces -- chroma replicated to luma size
    (repeat_interleave), the float matrix, round, clamp, cast and repack in torch, then the existing RGB call; (c) `rgb_floor`, the
    existing RGB call alone on frames converted beforehand, on the parent's build where --parent-lib is given.  `luma_only` is the
    luma plane's resize on its own (a one-channel call into scratch-sized memory): what (a) spends beyond it is chroma, the
    split and the merge.  (b)'s chroma is nearest-replicated and its matrix is float, so its numbers differ from (a)'s by design:
    only (a) is Pillow's composition; no route is checked against another."""
    iw, ih, ow, oh, f, layout, crop, dtype = YCC_WORKLOADS[name]
    d = L.resize_desc(iw, ih, ow, oh, 3)
    src = L.ycc_source(d, layout)
    in_fb = L.ycc_frame_bytes(d, src)
    cw, chh = L.ycc_chroma_size(d, src)
    win = L.center_window(ow, oh, *crop) if crop else None
    w, h = (win[2], win[3]) if win else (ow, oh)
    elem = {None: 1, "float32": 4, "bfloat16": 2}[dtype]
    rgb_fs = (w * h * 3 + 3) // 4 * 4
    out_fb = rgb_fs if dtype is None else w * h * 3 * elem
    sets = max(2, -(-2 * 256 * 2 ** 20 // (f * in_fb)) + 1)
    gen = torch.Generator(device="cuda").manual_seed(7)
    xs = [torch.randint(0, 256, (f, in_fb), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(sets)]
    ys = [torch.empty(f * out_fb, dtype=torch.uint8, device="cuda") for _ in range(sets)]
    table = torch.from_numpy(L.ycc_table("jfif")).cuda()
    s = torch.cuda.current_stream().cuda_stream
    st = L.tensor_strides("chw", w, h, 3)
    lut = None if dtype is None else torch.from_numpy(
        L.normalize_lut(3, IMAGENET_MEAN, IMAGENET_STD, dtype).view(np.int32 if elem == 4 else np.int16)).cuda()

    def to_rgb(x):
        yy = x[:, :iw * ih].view(f, ih, iw).float()
        if layout == "nv12":
            c2 = x[:, iw * ih:].view(f, chh, cw, 2)
            cb, cr = c2[..., 0], c2[..., 1]
        else:
            cb = x[:, iw * ih:iw * ih + cw * chh].view(f, chh, cw)
            cr = x[:, iw * ih + cw * chh:].view(f, chh, cw)
        up = lambda p: p.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :ih, :iw].float().sub(128.0)
        u, v = up(cb), up(cr)
        rgb = torch.stack([yy + 1.402 * v, yy - 0.34414 * u - 0.71414 * v, yy + 1.772 * u], -1)
        return rgb.round().clamp(0, 255).to(torch.uint8).contiguous()

    rgbs = [to_rgb(xs[k]) for k in range(min(sets, 2))]           # (c)'s inputs, converted beforehand
    tmp1 = torch.empty(f * ((w * h + 3) // 4 * 4), dtype=torch.uint8, device="cuda")
    d1 = L.resize_desc(iw, ih, ow, oh, 1)

    def rgb_call(c, x_ptr, y):
        if dtype is None:
            c.resize_device(d, x_ptr, y.data_ptr(), f, 0, rgb_fs, s, window=win)
        else:
            c.resize_tensor_device(d, x_ptr, y.data_ptr(), f, lut.data_ptr(), st, stream=s, dtype=dtype, window=win)

    def ycc(i):
        y = ys[i % sets]
        if dtype is None:
            ctx.resize_ycc_device(d, src, table.data_ptr(), xs[i % sets].data_ptr(), y.data_ptr(), f, stream=s, window=win)
        else:
            ctx.resize_ycc_tensor_device(d, src, table.data_ptr(), xs[i % sets].data_ptr(), y.data_ptr(), f, lut.data_ptr(), st,
                                         stream=s, dtype=dtype, window=win)
        return y[:out_fb]

    def torch_convert(i):
        rgb = to_rgb(xs[i % sets])
        rgb_call(ctx, rgb.data_ptr(), ys[i % sets])
        return ys[i % sets][:out_fb]

    def rgb_floor(i):
        y = ys[i % sets]
        x_ptr = rgbs[i % len(rgbs)].data_ptr()
        if parent is None:
            rgb_call(ctx, x_ptr, y)
        elif dtype is None:
            parent.window_device("lanczos_resize_window_device", d, win, None, x_ptr, y.data_ptr(), f, 0, rgb_fs, s)
        else:
            t = L.tensor_out(lut.data_ptr(), st) if elem == 4 else L.tensor16_out(lut.data_ptr(), st)
            parent.window_device("lanczos_resize_tensor_window_device" if elem == 4 else "lanczos_resize_tensor16_window_device",
                                 d, win, t, x_ptr, y.data_ptr(), f, 0, 0, s)
        return y[:out_fb]

    def luma_only(i):
        ctx.resize_device(d1, xs[i % sets].data_ptr(), tmp1.data_ptr(), f, in_fb, tmp1.numel() // f, s, window=win)
        return tmp1[:w * h]

    ycc(0)
    info = ctx.last_ycc_info()
    routes = {"ycc": ycc, "torch_convert": torch_convert, "rgb_floor": rgb_floor, "luma_only": luma_only}
    inb = {"ycc": f * in_fb, "torch_convert": f * in_fb, "rgb_floor": f * iw * ih * 3, "luma_only": f * iw * ih}
    outb = {rn: f * w * h * 3 * elem for rn in routes}
    outb["luma_only"] = f * w * h
    us = run_routes(name, f"{layout} {iw}x{ih}->{ow}x{oh}" + (f" window {win}" if win else "") + f" {dtype or 'rgb bytes'}", f,
                    routes, inb, outb, args, ctx, torch)
    print(json.dumps({"workload": name, "ycc_over_torch_convert": round(us["ycc"] / us["torch_convert"], 3),
                      "ycc_over_rgb_floor": round(us["ycc"] / us["rgb_floor"], 3), "rgb_floor": "parent" if parent else "this build",
                      "ycc_minus_luma_only_us": round(us["ycc"] - us["luma_only"], 2), "luma_kernel": info.luma_kernel,
                      "chroma_kernel": info.chroma_kernel, "split": info.split, "launches": info.launches,
                      "scratch_round_trip_bytes": 2 * 3 * f * w * h, "measured": True}), flush=True)
    del xs, ys, rgbs, tmp1
    torch.cuda.empty_cache()


YCC_OUT_WORKLOADS = {   # name: (in_w, in_h, out_w, out_h, frames, source layout or None for RGB frames, destination layout, standard)
    "YO1": (3840, 2160, 1920, 1080, 32, "nv12", "nv12", None),
    "YO2": (1920, 1080, 1920, 1080, 32, None, "nv12", "bt709"),
    "YO3": (3840, 2160, 1280, 720, 32, None, "i420", "jfif"),
}


def run_ycc_out(name, args, ctx, torch, parent):
    """Into YCbCr frames (lanczos_resize_ycc_out): (a) `ycc_out`, the one call; (b) `pipeline`, what it replaces, built from the
    other entries and torch -- from NV12: the chroma split in torch, three one-channel resize calls (luma straight into the
    result's luma plane), the re-interleave in torch; from RGB: the RGB resize, then the float matrix, avg_pool2d, round, clamp,
    cast and repack in torch; (c) `floor`: the luma call alone, or the RGB resize alone (--parent-lib: on that build).  (b)'s
    matrix and average are float, so its bytes differ from (a)'s by design from RGB; from NV12 they are checked to agree."""
    iw, ih, ow, oh, f, layout, out_layout, standard = YCC_OUT_WORKLOADS[name]
    d = L.resize_desc(iw, ih, ow, oh, 3)
    dst = L.ycc_dest(d, out_layout)
    out_fb = L.ycc_dest_frame_bytes(d, dst)
    ocw, och = L.ycc_dest_chroma_size(d, dst)
    src = L.ycc_source(d, layout) if layout else None
    in_fb = L.ycc_frame_bytes(d, src) if layout else iw * ih * 3
    sets = max(2, -(-2 * 256 * 2 ** 20 // (f * in_fb)) + 1)
    gen = torch.Generator(device="cuda").manual_seed(7)
    xs = [torch.randint(0, 256, (f, in_fb), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(sets)]
    ys = [torch.empty((f, out_fb), dtype=torch.uint8, device="cuda") for _ in range(sets)]
    s = torch.cuda.current_stream().cuda_stream
    table = torch.from_numpy(L.ycc_table_forward(standard)).cuda() if standard else None
    d1 = L.resize_desc(iw, ih, ow, oh, 1)

    def ycc_out(i):
        y = ys[i % sets]
        if layout:
            ctx.resize_ycc_to_ycc_device(d, src, dst, xs[i % sets].data_ptr(), y.data_ptr(), f, stream=s)
        else:
            ctx.resize_rgb_to_ycc_device(d, dst, table.data_ptr(), xs[i % sets].data_ptr(), y.data_ptr(), f, stream=s)
        return y[0]

    def put_chroma(y, cb, cr):
        if out_layout == "nv12":
            c2 = y[:, ow * oh:].view(f, och, ocw, 2)
            c2[..., 0], c2[..., 1] = cb, cr
        else:
            y[:, ow * oh:ow * oh + ocw * och] = cb.reshape(f, -1)
            y[:, ow * oh + ocw * och:] = cr.reshape(f, -1)

    if layout:
        cw, chh = L.ycc_chroma_size(d, src)
        dc = L.resize_desc(cw, chh, ocw, och, 1)
        tmp = torch.empty((2, f, och, ocw), dtype=torch.uint8, device="cuda")

        def pipeline(i):
            x, y = xs[i % sets], ys[i % sets]
            c2 = x[:, iw * ih:].view(f, chh, cw, 2)
            cb, cr = c2[..., 0].contiguous(), c2[..., 1].contiguous()
            ctx.resize_device(d1, x.data_ptr(), y.data_ptr(), f, in_fb, out_fb, s)
            ctx.resize_device(dc, cb.data_ptr(), tmp[0].data_ptr(), f, 0, 0, s)
            ctx.resize_device(dc, cr.data_ptr(), tmp[1].data_ptr(), f, 0, 0, s)
            put_chroma(y, tmp[0], tmp[1])
            return y[0]

        def floor(i):
            ctx.resize_device(d1, xs[i % sets].data_ptr(), ys[i % sets].data_ptr(), f, in_fb, out_fb, s)
            return ys[i % sets][0, :ow * oh]
        floor_in, floor_out = f * iw * ih, f * ow * oh
    else:
        rgb = torch.empty((f, oh, ow, 3), dtype=torch.uint8, device="cuda")
        kr, kb = (0.299, 0.114) if standard != "bt709" else (0.2126, 0.0722)
        kg = 1.0 - kr - kb
        sy, sc, y0 = (1.0, 1.0, 0.0) if standard == "jfif" else (219.0 / 255.0, 224.0 / 255.0, 16.0)
        m = torch.tensor([[kr * sy, kg * sy, kb * sy], [-kr / (2 * (1 - kb)) * sc, -kg / (2 * (1 - kb)) * sc, 0.5 * sc],
                          [0.5 * sc, -kg / (2 * (1 - kr)) * sc, -kb / (2 * (1 - kr)) * sc]], dtype=torch.float32, device="cuda")
        off = torch.tensor([y0, 128.0, 128.0], dtype=torch.float32, device="cuda")
        q = lambda p: p.round().clamp(0, 255).to(torch.uint8)

        def rgb_resize(c, i):
            if c is None:
                ctx.resize_device(d, xs[i % sets].data_ptr(), rgb.data_ptr(), f, 0, 0, s)
            else:
                c.resize_device(d, xs[i % sets].data_ptr(), rgb.data_ptr(), f, s)

        def pipeline(i):
            y = ys[i % sets]
            rgb_resize(None, i)
            ycc = rgb.float() @ m.t() + off
            y[:, :ow * oh] = q(ycc[..., 0]).view(f, -1)
            c = torch.nn.functional.avg_pool2d(ycc[..., 1:].permute(0, 3, 1, 2), 2)
            put_chroma(y, q(c[:, 0]), q(c[:, 1]))
            return y[0]

        def floor(i):
            rgb_resize(parent, i)
            return rgb[0]
        floor_in, floor_out = f * in_fb, f * ow * oh * 3

    ycc_out(0)
    info = ctx.last_ycc_out_info()
    routes = {"ycc_out": ycc_out, "pipeline": pipeline, "floor": floor}
    inb = {"ycc_out": f * in_fb, "pipeline": f * in_fb, "floor": floor_in}
    outb = {"ycc_out": f * out_fb, "pipeline": f * out_fb, "floor": floor_out}
    us = run_routes(name, f"{layout or 'rgb'} {iw}x{ih}->{ow}x{oh} {out_layout}" + (f" {standard}" if standard else ""), f, routes, inb,
                    outb, args, ctx, torch, check=(("ycc_out", "pipeline"),) if layout else ())
    print(json.dumps({"workload": name, "ycc_out_over_pipeline": round(us["ycc_out"] / us["pipeline"], 3),
                      "ycc_out_over_floor": round(us["ycc_out"] / us["floor"], 3),
                      "floor": ("luma call" if layout else "rgb resize") + (", parent" if parent and not layout else ", this build"),
                      "luma_kernel": info.luma_kernel, "chroma_kernel": info.chroma_kernel, "split": info.split, "join": info.join,
                      "encode": info.encode, "launches": info.launches, "measured": True}), flush=True)
    del xs, ys
    torch.cuda.empty_cache()


YCC16_WORKLOADS = {   # name: (in_w, in_h, out_w, out_h, frames, layout, crop (w, h) from the centre or None, tensor dtype or None: YCbCr out)
    "YW1": (3840, 2160, 1920, 1080, 32, "p010", None, None),
    "YW2": (3840, 2160, 1920, 1080, 32, "p010", None, "bfloat16"),
    "YW3": (500, 375, 341, 256, 256, "i420", (224, 224), "float32"),
}


def run_ycc16(name, args, ctx, torch, parent):
    """YCbCr frames of 16-bit words (lanczos_resize_ycc16), 10-bit samples: MSB-aligned in P010, LSB-aligned in planes.
    YW1, P010 -> P010: (a) `ycc16`, the one call; (b) `pipeline`, what it replaces -- torch's split of the chroma pairs, three
    one-channel uint16 calls (luma straight into the result), torch's re-interleave; (c) `floor`, the luma call alone.  (a) and
    (b) are checked to agree.  YW2 / YW3, into normalised tensors under BT.2020: (b) `pipeline` is torch's chroma replication,
    float matrix, round, clamp and cast to RGB words, then resize_tensor_norm; (c) `floor` is resize_tensor_norm alone on frames
    converted beforehand (--parent-lib: on that build); `luma_only` the luma plane's call.  (b) replicates chroma and its matrix
    is float, so only (a) is Pillow's composition there and no route is checked against another."""
    import ctypes
    iw, ih, ow, oh, f, layout, crop, dtype = YCC16_WORKLOADS[name]
    msb = layout == "p010"
    d = L.resize_desc(iw, ih, ow, oh, 3, bits=16)
    src = L.ycc16_source(d, layout)
    in_fb = L.ycc_frame_bytes(d, src)
    cw, chh = L.ycc_chroma_size(d, src)
    win = L.center_window(ow, oh, *crop) if crop else None
    w, h = (win[2], win[3]) if win else (ow, oh)
    s = torch.cuda.current_stream().cuda_stream
    sets = max(2, -(-2 * 256 * 2 ** 20 // (f * in_fb)) + 1)
    gen = torch.Generator(device="cuda").manual_seed(7)
    words = lambda n: (torch.randint(64, 941, (f, n), dtype=torch.int32, device="cuda", generator=gen) << (6 if msb else 0)).to(torch.int16)
    xs = [words(in_fb // 2) for _ in range(sets)]
    d1 = L.resize_desc(iw, ih, ow, oh, 1, bits=16)
    unsigned = lambda t: t.to(torch.int32) & 0xFFFF

    def split(x):
        if layout == "p010":
            c2 = x[:, iw * ih:].view(f, chh, cw, 2)
            return c2[..., 0], c2[..., 1]
        return x[:, iw * ih:iw * ih + cw * chh].view(f, chh, cw), x[:, iw * ih + cw * chh:].view(f, chh, cw)

    if dtype is None:
        dst = L.ycc16_dest(d, layout)
        out_fb = L.ycc_dest_frame_bytes(d, dst)
        ocw, och = L.ycc_dest_chroma_size(d, dst)
        ys = [torch.empty((f, out_fb // 2), dtype=torch.int16, device="cuda") for _ in range(sets)]
        dc = L.resize_desc(cw, chh, ocw, och, 1, bits=16)
        tmp = torch.empty((2, f, och, ocw), dtype=torch.int16, device="cuda")

        def ycc16(i):
            ctx.resize_ycc16_to_ycc_device(d, src, dst, xs[i % sets].data_ptr(), ys[i % sets].data_ptr(), f, stream=s)
            return ys[i % sets][0]

        def pipeline(i):
            x, y = xs[i % sets], ys[i % sets]
            cb, cr = (p.contiguous() for p in split(x))
            ctx.resize_device(d1, x.data_ptr(), y.data_ptr(), f, in_fb, out_fb, s)
            ctx.resize_device(dc, cb.data_ptr(), tmp[0].data_ptr(), f, 0, 0, s)
            ctx.resize_device(dc, cr.data_ptr(), tmp[1].data_ptr(), f, 0, 0, s)
            c2 = y[:, ow * oh:].view(f, och, ocw, 2)
            c2[..., 0], c2[..., 1] = tmp[0], tmp[1]
            return y[0]

        def floor(i):
            ctx.resize_device(d1, xs[i % sets].data_ptr(), ys[i % sets].data_ptr(), f, in_fb, out_fb, s)
            return ys[i % sets][0, :ow * oh]
        routes = {"ycc16": ycc16, "pipeline": pipeline, "floor": floor}
        inb = {"ycc16": f * in_fb, "pipeline": f * in_fb, "floor": f * iw * ih * 2}
        outb = {"ycc16": f * out_fb, "pipeline": f * out_fb, "floor": f * ow * oh * 2}
        check, floor_on = (("ycc16", "pipeline"),), "luma call, this build"
    else:
        elem = 4 if dtype == "float32" else 2
        m = L.ycc16_matrix("bt2020", 10, msb, False)
        st = L.tensor_strides("chw", w, h, 3)
        n = L.tensor_norm(st, 65535.0, IMAGENET_MEAN, IMAGENET_STD, dtype)
        ys = [torch.empty(f * w * h * 3 * elem, dtype=torch.uint8, device="cuda") for _ in range(sets)]
        d3 = L.resize_desc(iw, ih, ow, oh, 3, bits=16)
        kr, kb = 0.2627, 0.0593
        kg, unit = 1.0 - kr - kb, (64.0 if msb else 1.0)
        ky, kc = 65535.0 / (876.0 * unit), 65535.0 / (896.0 * unit)

        def to_rgb(x):
            yy = (unsigned(x[:, :iw * ih]).view(f, ih, iw).float() - 64.0 * unit) * ky
            up = lambda p: (unsigned(p).repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :ih, :iw].float() - 512.0 * unit) * kc
            cb, cr = split(x)
            u, v = up(cb), up(cr)
            rgb = torch.stack([yy + 2 * (1 - kr) * v, yy - 2 * (1 - kb) * kb / kg * u - 2 * (1 - kr) * kr / kg * v, yy + 2 * (1 - kb) * u], -1)
            return rgb.round().clamp(0, 65535).to(torch.int32).to(torch.int16).contiguous()

        rgbs = [to_rgb(xs[k]) for k in range(min(sets, 2))]           # the floor's inputs, converted beforehand
        tmp1 = torch.empty(f * w * h + 1, dtype=torch.int16, device="cuda")

        def ycc16(i):
            y = ys[i % sets]
            ctx.resize_ycc16_tensor_device(d, src, m, n, xs[i % sets].data_ptr(), y.data_ptr(), f, stream=s, window=win)
            return y[:w * h * 3 * elem]

        def pipeline(i):
            y = ys[i % sets]
            rgb = to_rgb(xs[i % sets])
            ctx.resize_tensor_norm_device(d3, rgb.data_ptr(), y.data_ptr(), f, n, stream=s, window=win)
            return y[:w * h * 3 * elem]

        if parent is not None:
            fn = parent.lib.lanczos_resize_tensor_norm_device
            fn.argtypes = [ctypes.c_void_p] * 8 + [ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
            pwin = L.resize_window(d3, win) if win else None

        def floor(i):
            y, x_ptr = ys[i % sets], rgbs[i % len(rgbs)].data_ptr()
            if parent is None:
                ctx.resize_tensor_norm_device(d3, x_ptr, y.data_ptr(), f, n, stream=s, window=win)
            else:
                rc = fn(parent.h, ctypes.byref(d3), None, ctypes.byref(pwin) if pwin is not None else None, None, ctypes.byref(n), x_ptr,
                        y.data_ptr(), f, 0, 0, s)
                if rc != 0:
                    raise SystemExit(f"parent lanczos_resize_tensor_norm_device: {rc}")
            return y[:w * h * 3 * elem]

        def luma_only(i):
            ctx.resize_device(d1, xs[i % sets].data_ptr(), tmp1.data_ptr(), f, in_fb, 2 * w * h, s, window=win)
            return tmp1[:w * h]
        routes = {"ycc16": ycc16, "pipeline": pipeline, "floor": floor, "luma_only": luma_only}
        inb = {"ycc16": f * in_fb, "pipeline": f * in_fb, "floor": f * iw * ih * 6, "luma_only": f * iw * ih * 2}
        outb = {rn: f * w * h * 3 * elem for rn in routes}
        outb["luma_only"] = f * w * h * 2
        check, floor_on = (), "resize_tensor_norm on RGB words, " + ("parent" if parent else "this build")

    ycc16(0)
    info = ctx.last_ycc16_info()
    us = run_routes(name, f"{layout} {iw}x{ih}->{ow}x{oh}" + (f" window {win}" if win else "") + f" {dtype or layout}", f, routes, inb,
                    outb, args, ctx, torch, check=check)
    print(json.dumps({"workload": name, "ycc16_over_pipeline": round(us["ycc16"] / us["pipeline"], 3),
                      "ycc16_over_floor": round(us["ycc16"] / us["floor"], 3), "floor": floor_on,
                      "luma_kernel": info.luma_kernel, "chroma_kernel": info.chroma_kernel, "split": info.split, "join": info.join,
                      "merge": info.merge, "launches": info.launches, "measured": True}), flush=True)
    del xs, ys
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="W1,W2,W3,W4,W5,A1,A4,U1,U4")
    ap.add_argument("--routes", default=",".join(ROUTES))
    ap.add_argument("--pillow", action="store_true")
    ap.add_argument("--parent-lib", default=None,
                    help="another build of liblanczos_hip.so for the parent_bytes route of T*, the parent_samples route of N*, the parent_full route of WIN* and the rgb_floor route of YC*")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("resize_speed.py needs a GPU")
    ctx = L.Context(0)
    parent = ParentLib(args.parent_lib) if args.parent_lib else None
    for name in args.only.split(","):
        if name in YCC16_WORKLOADS:
            run_ycc16(name, args, ctx, torch, parent)
        elif name in YCC_OUT_WORKLOADS:
            run_ycc_out(name, args, ctx, torch, parent)
        elif name in YCC_WORKLOADS:
            run_ycc(name, args, ctx, torch, parent)
        elif name in NORM_WORKLOADS:
            run_norm(name, args, ctx, torch, parent)
        elif name in WINDOW_WORKLOADS:
            run_window(name, args, ctx, torch, parent)
        elif name in CROPS_WORKLOADS:
            run_crops(name, args, ctx, torch)
        elif name in SOURCE_WORKLOADS:
            run_source(name, args, ctx, torch)
        elif name in DEST_WORKLOADS:
            run_dest(name, args, ctx, torch)
        elif name in VIEW_WORKLOADS:
            run_view(name, args, ctx, torch)
        elif name in TENSOR_WORKLOADS:
            run_tensor(name, args, ctx, torch, parent)
        elif name.endswith("h") and name[:-1] in TENSOR_WORKLOADS:
            run_tensor16(name, args, ctx, torch)
        elif name == "R5":
            run_gap(name, args, ctx, torch)
        elif name in ("B1", "B2"):
            run_box(name, (1920, 1080) if name == "B1" else (640, 360), args, ctx, torch)
        elif name in RGBA_WORKLOADS:
            run_rgba(name, RGBA_WORKLOADS[name], args, ctx, torch)
        elif name in U16_WORKLOADS:
            run(name, U16_WORKLOADS[name], args, ctx, torch, bits=16)
        elif name in F32_WORKLOADS:
            run(name, F32_WORKLOADS[name], args, ctx, torch, bits=32)
        elif name in FILTER_WORKLOADS:
            run(name, WORKLOADS[FILTER_WORKLOADS[name][0]], args, ctx, torch, filt=FILTER_WORKLOADS[name][1])
        else:
            run(name, WORKLOADS[name], args, ctx, torch)
    if parent is not None:
        parent.close()
    ctx.close()


if __name__ == "__main__":
    main()
