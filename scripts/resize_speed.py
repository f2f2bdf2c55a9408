#!/usr/bin/env python3
"""resize_speed.py -- speed of the resize-to-any-size entry (lanczos_resize_device) on one MI355X.

    python scripts/resize_speed.py [--steps K] [--warmup W] [--rounds R] [--only W1,W3] [--pillow]

One JSON line per (workload, path).  Discipline as bench.py's: the frames are resident in HBM and the steps cycle through
enough input / output sets that the inputs of one cycle exceed twice the 256 MiB Infinity Cache (no step finds its input
there); W untimed warm-up steps per path; device-event timing of K steps per region; the paths (auto, fused, two-pass)
alternate region by region and every path's figure is the median over its R regions.  Before timing, the frame-0 outputs
of all paths are compared byte for byte.

  us_per_step    device time of one call over F frames (median region / K)
  mpix_per_s     output pixels per second
  hbm_frac       compulsory bytes (F * (input + output frame bytes)) / step time / 8 TB/s
  kernel         family that served the call (lanczos_last_kernel: 4 fused, 5 two-pass)

--pillow adds Pillow's single-core time of one frame of each workload (if Pillow imports; else "not available").
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
PATHS = {"auto": L.RESIZE_AUTO, "fused": L.RESIZE_FUSED, "two_pass": L.RESIZE_TWO_PASS}


def run(name, spec, args, ctx, torch):
    iw, ih, ow, oh, c, a, f = spec
    in_fb, out_fb = iw * ih * c, ow * oh * c
    step_in = f * in_fb
    sets = max(2, -(-2 * 256 * 2 ** 20 // step_in) + 1)
    gen = torch.Generator(device="cuda").manual_seed(7)
    xs = [torch.randint(0, 256, (f * in_fb,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(sets)]
    ys = [torch.empty(f * out_fb, dtype=torch.uint8, device="cuda") for _ in range(sets)]
    d = L.resize_desc(iw, ih, ow, oh, c, a)
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
    for pn, (p, fam) in paths.items():
        us = statistics.median(times[pn])
        line = {"workload": name, "shape": f"{iw}x{ih}->{ow}x{oh} C{c} a{a}", "frames": f, "path": pn, "kernel": fam,
                "us_per_step": round(us, 2), "us_all_regions": [round(v, 2) for v in times[pn]],
                "mpix_per_s": round(f * ow * oh / us, 1), "hbm_frac": round(f * (in_fb + out_fb) / (us * 1e-6) / HBM_BPS, 4),
                "compulsory_bytes": f * (in_fb + out_fb), "input_sets_cycled": sets, "steps": args.steps,
                "rounds": args.rounds, "measured": True}
        print(json.dumps(line), flush=True)
    if args.pillow:
        try:
            from PIL import Image
            img = Image.frombytes("RGB", (iw, ih), xs[0][:in_fb].cpu().numpy().tobytes())
            img.resize((ow, oh), Image.LANCZOS)
            t0 = time.perf_counter()
            img.resize((ow, oh), Image.LANCZOS)
            ms = (time.perf_counter() - t0) * 1e3
            print(json.dumps({"workload": name, "pillow_single_core_ms_per_frame": round(ms, 2), "measured": True}))
        except ImportError:
            print(json.dumps({"workload": name, "pillow_single_core_ms_per_frame": "not available"}))
    del xs, ys
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="W1,W2,W3,W4,W5")
    ap.add_argument("--pillow", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("resize_speed.py needs a GPU")
    ctx = L.Context(0)
    for name in args.only.split(","):
        run(name, WORKLOADS[name], args, ctx, torch)
    ctx.close()


if __name__ == "__main__":
    main()
