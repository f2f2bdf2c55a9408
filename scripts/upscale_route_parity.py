#!/usr/bin/env python3
"""Do two builds of the library decide and compute the same for the upscale entry?

    python scripts/upscale_route_parity.py --other lanczos-hls_amd/build/liblanczos_hip_parent.so [--random 300] [--seed 1]

The requests of tests/test_upscale_route_gpu.py and --random seeded random ones at tiny sizes (every kind of scale, mode, force,
strip, frame stride and batch size) go through lanczos_resample_device of both libraries, one child process per library
(LANCZOS_LIB names the other one).  Per request the children report the return code, lanczos_last_kernel, lanczos_last_route,
the march-table info with a checksum of its entries, and a checksum of the output; the parent process compares them and prints
one JSON line with the counts.  Exit status 1 if anything differs."""
import argparse
import json
import os
import random
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def requests(n_random, seed, cus):
    import fast_cfg as F
    import upscale_route_cfg as U
    from test_upscale_route_gpu import _requests
    out = [q for _, q, _ in _requests(cus)]
    rng = random.Random(seed)
    insts = sorted(F.FAST_INSTANCES)
    while len(out) < len(_requests(cus)) + n_random:
        if rng.random() < 0.6:
            bps, c, sn, a = rng.choice(insts)
            sd = 1
        else:
            sn, sd = rng.choice([(3, 2), (4, 3), (5, 2), (5, 3), (5, 1), (9, 8), (1, 1)])
            bps, c, a = rng.choice((1, 2)), rng.choice((1, 3, 4)), rng.choice((2, 3, 4))
        w = sd * rng.randint(16 // sd + 1, 64 // sd)
        if sd == 1 and rng.random() < 0.7:   # rows that are 16-byte multiples: k_march
            w = 16 * rng.randint(1, 4)
        K, Mm, M2 = U._prefix_rows(sn, a) if sd == 1 and sn > 1 else (0, 0, 12)
        h = sd * max(1, rng.choice((M2 - 1, M2, M2 + 5, 2, 24)) // sd)
        frames = rng.choice((1, 1, 2, 3, 5, 8, 33, cus // 2 + 1, cus + 1, 2 * cus + 3, 4 * cus + 3))
        mode = rng.choice((U.MODE_LSB1, U.MODE_EXACT, U.MODE_EXACT, U.MODE_HLS))
        force = rng.choice((U.KERNEL_NONE, U.KERNEL_NONE, U.KERNEL_NONE, U.KERNEL_GENERIC, U.KERNEL_FAST))
        out_h = h * sn // sd
        row0 = rows = 0
        if rng.random() < 0.3 and out_h > 2:
            row0 = rng.choice((0, 0, min(K, out_h - 1), rng.randint(0, out_h - 1)))
            rows = rng.randint(1, out_h - row0)
        pad_in, pad_out = rng.choice((0, 0, 0, 16, 32, 8)), rng.choice((0, 0, 0, 16, 4, 2))
        out.append(U.request(w, h, c, bps, sn, sd, a, mode, row0, rows, frames, pad_in, pad_out, 0, 0, force))
    return out


def child(args):
    import numpy as np
    import torch
    import lanczos_hls_amd as L
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ctx = L.Context(0)
    for i, q in enumerate(requests(args.random, args.seed, cus)):
        d = L.make_desc(q.in_w, q.in_h, q.c, q.sn, q.sd, q.a, q.bps, q.mode, q.row0, q.rows)
        in_rows = L.strip_input_rows(d, q.row0, q.rows)[1] if q.rows else q.in_h
        # (in_stride / out_stride of a random request: padding bytes behind every frame)
        in_fb = in_rows * q.in_w * q.c * q.bps + q.in_stride
        out_fb = (q.rows or d.out_h) * d.out_w * q.c * q.bps + q.out_stride
        x = torch.from_numpy(np.random.default_rng(i).integers(0, 256, (q.frames, in_fb), dtype=np.uint8)).cuda()
        y = torch.full((q.frames, out_fb), 0x5A, dtype=torch.uint8, device="cuda")
        ctx.force_kernel(q.force)
        rc = L.OK
        try:
            ctx.resample_device(d, x.data_ptr(), y.data_ptr(), q.frames, in_fb if q.in_stride else 0, out_fb if q.out_stride else 0,
                                torch.cuda.current_stream().cuda_stream)
        except L.LanczosError as e:
            rc = e.code
        torch.cuda.synchronize()
        info, tab = ctx.last_march_table()
        r = ctx.last_route()
        print(json.dumps({"i": i, "rc": rc, "kernel": ctx.last_kernel() if rc == 0 else None,
                          "route": [r.main, r.prefix, r.launches, sorted(r.prefix_seen)], "table": list(info),
                          "entries": zlib.crc32(tab.tobytes()), "out": zlib.crc32(y.cpu().numpy().tobytes())}), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="the library to compare this build with")
    ap.add_argument("--random", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = []
    for lib in (None, os.path.abspath(args.other)):
        env = {k: v for k, v in os.environ.items() if k != "LANCZOS_LIB"}
        if lib:
            env["LANCZOS_LIB"] = lib
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--random", str(args.random), "--seed", str(args.seed)],
                           env=env, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            raise SystemExit(f"child for {lib or 'this build'} ended with {p.returncode}: {p.stderr[-2000:]}")
        runs.append([json.loads(line) for line in p.stdout.split("\n") if line.startswith("{")])
    a, b = runs
    fields = ("rc", "kernel", "route", "table", "entries", "out")
    differ = {f: sum(x[f] != y[f] for x, y in zip(a, b)) for f in fields}
    for x, y in zip(a, b):
        if x != y:
            print("DIFFERS", json.dumps(x), json.dumps(y))
    routes = sorted({(x["route"][0], x["route"][1]) for x in a if x["rc"] == 0})
    print(json.dumps({"requests": len(a), "other_requests": len(b), "refused": sum(x["rc"] != 0 for x in a),
                      "split": sum(x["route"][2] > 1 for x in a), "marched": sum(x["table"][0] > 0 for x in a),
                      "main_prefix_pairs": routes, "differing": differ}))
    sys.exit(1 if len(a) != len(b) or any(differ.values()) else 0)


if __name__ == "__main__":
    main()
