#!/usr/bin/env python3
"""Host time per resize call THROUGH THE PYTHON BINDING: the requests of scripts/resize_host_time.py, issued through
Context.resize_device / Context.resize_tensor_device instead of the ctypes function, so that the figure holds what the wrapper
adds (the entry choice, byref, the return-code check).

    python scripts/binding_host_time.py [--root DIR] [--fake] [--calls 5000] [--rounds 5]

--root DIR  import lanczos-hls_amd/__init__.py from that tree (e.g. a worktree of the parent commit) against THIS tree's library;
            run the two alternately, a process each.
--fake      the recorder of tests/binding_calls_cfg.py stands in for the library: launching entries return OK at once, so the
            figure is binding time alone and needs no GPU.

Three requests, one frame each, 16 x 16 -> 8 x 8 RGB:
  bytes    resize_device(desc, in, out, 1, stream=)
  crops    resize_tensor_device(..., a ready TensorView, crop=a ready ResizeCrops), a 4 x 4 float32 CHW crop
  planar   resize_device(..., source=planes, dest=planes)
Every round issues --calls calls on one stream and synchronises once at the end.  One JSON line: microseconds per call of every
round, and their median, per request."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--fake", action="store_true")
    ap.add_argument("--calls", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    if root != ROOT:
        os.environ.setdefault("LANCZOS_LIB", os.path.join(ROOT, "lanczos-hls_amd", "liblanczos_hip.so"))
    if not args.fake:
        import torch   # before the library loads, so that both share one HIP runtime
    import binding_calls_cfg as B
    L = B.load_module(root)
    real = L._lib()
    if args.fake:
        L._LIB = B.Recorder(real, B.launching(L), keep=False)
        px, py, p_lut, p_origin, s = B.D_IN, B.D_OUT, B.D_LUT, B.D_ORIGIN, ctypes.c_void_p(B.STREAM)
        sync = lambda: None
    else:
        x = torch.randint(0, 256, (16 * 16 * 3,), dtype=torch.uint8, device="cuda")
        y = torch.zeros(8 * 8 * 3 * 4, dtype=torch.uint8, device="cuda")
        lut = torch.arange(3 * 256, dtype=torch.float32, device="cuda")
        origin = torch.tensor([2, 3], dtype=torch.int32, device="cuda")
        stream = torch.cuda.Stream()
        px, py, p_lut, p_origin, s = x.data_ptr(), y.data_ptr(), lut.data_ptr(), origin.data_ptr(), ctypes.c_void_p(stream.cuda_stream)
        sync = stream.synchronize
    ctx = L.Context()
    d = L.resize_desc(16, 16, 8, 8, 3, 3)
    view = L.tensor_view(p_lut, (16, 4, 1), 4, (0, 1, 2))
    crops = L.resize_crops(4, 4, p_origin)
    src, dst = L.resize_source(d, "planar"), L.resize_dest(d, "planar")
    requests = {
        "bytes": lambda: ctx.resize_device(d, px, py, 1, stream=s),
        "crops": lambda: ctx.resize_tensor_device(d, px, py, 1, None, view, stream=s, crop=crops),
        "planar": lambda: ctx.resize_device(d, px, py, 1, stream=s, source=src, dest=dst),
    }
    out = {"root": root, "lib": L.LIB_PATH, "fake": args.fake, "calls": args.calls}
    for name, call in requests.items():
        rounds = []
        for r in range(args.rounds + 1):   # the first round warms up: tables, scratch, code objects
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call()   # raises LanczosError on any code but OK
            sync()
            if r:
                rounds.append(round((time.perf_counter() - t0) / args.calls * 1e6, 3))
        out[name] = {"us_per_call": rounds, "median_us": statistics.median(rounds)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
