#!/usr/bin/env python3
"""Host time per resize call: the wall time of one call of the C ABI on a request so small that the launch dominates, for a
build of the library (LANCZOS_LIB=PATH names another one, e.g. the parent commit's; run the two alternately, a process each).

    python scripts/resize_host_time.py [--calls 5000] [--rounds 5]

Six requests, one frame each, 16 x 16 -> 8 x 8, AUTO:
  bytes    lanczos_resize_device, RGB
  crops    lanczos_resize_tensor_crops_device, RGB into a 4 x 4 float32 CHW crop
  planar   lanczos_resize_dest_device, RGB planes in, RGB planes out
  ycc      lanczos_resize_ycc_device, NV12 into RGB bytes (four launches a call)
  ycc_out  lanczos_resize_ycc_out, NV12 into NV12 (four launches)
  ycc16    lanczos_resize_ycc16, P010 into P010 (four launches)
Every round issues --calls calls on one stream through the ctypes function itself (no wrapper in between) and synchronises once
at the end.  One JSON line: microseconds per call of every round, and their median, per request."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lanczos_hls_amd as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    lib, ctx = L._lib(), L.Context()
    d = L.resize_desc(16, 16, 8, 8, 3, 3)
    x = torch.randint(0, 256, (16 * 16 * 3,), dtype=torch.uint8, device="cuda")
    y = torch.zeros(8 * 8 * 3 * 4, dtype=torch.uint8, device="cuda")
    lut = torch.arange(3 * 256, dtype=torch.float32, device="cuda")
    origin = torch.tensor([2, 3], dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    s = ctypes.c_void_p(stream.cuda_stream)
    view = L.tensor_view(lut.data_ptr(), (16, 4, 1), 4, (0, 1, 2))
    crops = L.resize_crops(4, 4, origin.data_ptr())
    src, dst = L.resize_source(d, "planar"), L.resize_dest(d, "planar")
    h, pd, px, py = ctx._h, ctypes.byref(d), x.data_ptr(), y.data_ptr()
    requests = {
        "bytes": lambda: lib.lanczos_resize_device(h, pd, px, py, 1, 0, 0, s),
        "crops": lambda: lib.lanczos_resize_tensor_crops_device(h, pd, None, ctypes.byref(crops), ctypes.byref(view), px, py, 1, 0, 0, s),
        "planar": lambda: lib.lanczos_resize_dest_device(h, pd, None, None, ctypes.byref(src), ctypes.byref(dst), px, py, 1, 0, 0, s),
    }
    # one call of each YCbCr entry: luma, split, one chroma call, then merge or join
    table = torch.from_numpy(L.ycc_table("jfif")).cuda()
    nv12, nv12_out = L.ycc_source(d, "nv12"), L.ycc_dest(d, "nv12")
    d16 = L.resize_desc(16, 16, 8, 8, 3, 3, bits=16)
    rq_out = L.ycc_out_request(d, nv12_out, px, py, 1, source=nv12, stream=stream.cuda_stream)
    rq16 = L.ycc16_request(d16, L.ycc16_source(d16, "p010"), px, py, 1, dest=L.ycc16_dest(d16, "p010"), stream=stream.cuda_stream)
    requests.update({
        "ycc": lambda: lib.lanczos_resize_ycc_device(h, pd, None, None, ctypes.byref(nv12), table.data_ptr(), px, py, 1, 0, 0, s),
        "ycc_out": lambda: lib.lanczos_resize_ycc_out(h, ctypes.byref(rq_out)),
        "ycc16": lambda: lib.lanczos_resize_ycc16(h, ctypes.byref(rq16)),
    })
    out = {"lib": L.LIB_PATH, "calls": args.calls}
    for name, call in requests.items():
        rounds = []
        for r in range(args.rounds + 1):   # the first round warms up: tables, scratch, code objects
            t0 = time.perf_counter()
            for _ in range(args.calls):
                rc = call()
            stream.synchronize()
            if rc != L.OK:
                raise SystemExit(f"{name}: code {rc}")
            if r:
                rounds.append(round((time.perf_counter() - t0) / args.calls * 1e6, 3))
        out[name] = {"us_per_call": rounds, "median_us": statistics.median(rounds)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
