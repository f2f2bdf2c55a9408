#!/usr/bin/env python3
"""Host time per call of lanczos_resample_device: the wall time the calling thread spends inside the C ABI.

    python scripts/upscale_host_time.py [--other PATH] [--rounds 7]

With --other (another build of the library, e.g. the parent commit's) both are loaded into this one process and their rounds
alternate, so that both see the same core, clocks and neighbours: between processes the figure moves by a third on a shared
machine, which hides any difference between two builds.  Five requests, 8-bit RGB, Lanczos-3:
  riding    one 48 x 8 frame, 2x: k_march with the prefix rows riding
  bench     32 frames of 1920 x 1080, 2x: bench.py's shape and batch (front prefix kernel + k_march)
  split     64 frames of 1920 x 16, 2x: twice the preferred batch of a four-per-CU instance, two launches of each kernel
  rational  one 48 x 16 frame, 3/2: k_ratp and k_prefix
  generic   one 48 x 8 frame, 2x, LANCZOS_KERNEL_GENERIC forced: k_generic and k_prefix
Every round issues the request's calls on one stream through the ctypes function itself (no wrapper in between); the clock stops
when the last call has returned, and the stream is synchronised outside it (few enough calls that the queue never fills).  One JSON
line: per request and library the microseconds per call of every round, their median, and the route the call reported."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lanczos_hls_amd as L  # noqa: E402

# name -> (in_w, in_h, scale_n, scale_d, frames, forced family, calls per round)
REQUESTS = {
    "riding": (48, 8, 2, 1, 1, L.KERNEL_NONE, 1000),
    "bench": (1920, 1080, 2, 1, 32, L.KERNEL_NONE, 40),
    "split": (1920, 16, 2, 1, 64, L.KERNEL_NONE, 200),
    "rational": (48, 16, 3, 2, 1, L.KERNEL_NONE, 1000),
    "generic": (48, 8, 2, 1, 1, L.KERNEL_GENERIC, 1000),
}


class Build:
    """A build of the library loaded by path, with a context of its own: the entry points this script calls, declared here"""

    def __init__(self, path):
        self.path, self.lib = path, ctypes.CDLL(path)
        vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
        self.lib.lanczos_create.argtypes = [ctypes.POINTER(vp), ci]
        self.lib.lanczos_destroy.argtypes = [vp]
        self.lib.lanczos_force_kernel.argtypes = [vp, ci]
        self.lib.lanczos_last_route.argtypes = [vp]
        self.lib.lanczos_resample_device.argtypes = [vp, vp, vp, vp, ci, sz, sz, vp]
        self.ctx = vp()
        if self.lib.lanczos_create(ctypes.byref(self.ctx), 0) != L.OK:
            raise SystemExit(f"lanczos_create failed in {path}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="a second build to measure in alternation with this one")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch
    builds = {"this": Build(L.LIB_PATH)}
    if args.other:
        builds["other"] = Build(os.path.abspath(args.other))
    stream = torch.cuda.Stream()
    s = ctypes.c_void_p(stream.cuda_stream)
    out = {"libs": {k: b.path for k, b in builds.items()}}
    for name, (w, h, sn, sd, frames, force, calls) in REQUESTS.items():
        d = L.make_desc(w, h, 3, sn, sd, 3, 1, L.MODE_LSB1)
        x = torch.randint(0, 256, (frames, h * w * 3), dtype=torch.uint8, device="cuda")
        y = torch.zeros((frames, d.out_h * d.out_w * 3), dtype=torch.uint8, device="cuda")
        pd, px, py = ctypes.cast(ctypes.byref(d), ctypes.c_void_p), x.data_ptr(), y.data_ptr()
        rounds = {k: [] for k in builds}
        for r in range(args.rounds + 1):   # the first round warms up: tables, code objects
            for k, b in builds.items():
                b.lib.lanczos_force_kernel(b.ctx, force)
                call, ctx = b.lib.lanczos_resample_device, b.ctx
                t0 = time.perf_counter()
                for _ in range(calls):
                    rc = call(ctx, pd, px, py, frames, 0, 0, s)
                t1 = time.perf_counter()
                stream.synchronize()
                if rc != L.OK:
                    raise SystemExit(f"{name}, {k}: code {rc}")
                if r:
                    rounds[k].append(round((t1 - t0) / calls * 1e6, 3))
        out[name] = {k: {"us_per_call": v, "median_us": statistics.median(v), "route": hex(builds[k].lib.lanczos_last_route(builds[k].ctx))}
                     for k, v in rounds.items()}
        out[name]["calls"] = calls
        del x, y
    for b in builds.values():
        b.lib.lanczos_destroy(b.ctx)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
