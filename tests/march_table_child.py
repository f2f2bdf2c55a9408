"""Child process of test_march_table_gpu.py::test_production_switches_reshape_the_table (not collected by pytest): the library
reads its environment switches once per process (csrc/lanczos_env.hpp), so every setting gets a fresh process.  Runs the two
small config 2 batches of REQUESTS in both parity modes through lanczos_resample_device and writes, per request and mode, the
route, the reported workgroup table, the first occurrence of every base frame and whether every later frame equals the first
one of its base frame to the .npz named on the command line."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import lanczos_hls_amd as L  # noqa: E402
import march_table_cfg as M  # noqa: E402
import patterns as P  # noqa: E402

INSTANCE = "u8-c3-2x-a3"
# name -> candidates (in_w, in_h, frames): the first whose launch is ONE k_march launch with a table of the wanted mode is kept
#   slots:  the per-slot batches.  Under LANCZOS_MARCH_SEGS=1 with very uneven LANCZOS_RANK_WEIGHTS the shares of the slow slots
#           shrink to segments of exactly min_seg rows (or to nothing) next to shares of three segments
#   chunks: a taller frame than the equal goal's: LANCZOS_MARCH_WGS=63 cuts its 21 pairs into three chunks of 55 / 55 / 28 rows
#           where the default is five of 31 / 31 / 31 / 31 / 14
REQUESTS = {"slots": M.CANDIDATES[(INSTANCE, "per-slot")], "chunks": [(272, 140, 7)]}
SEED = {"slots": 6100, "chunks": 6200}


def base_frames(name, w, h):
    s = SEED[name]
    return [P.noise(h, w, 3, seed=s), P.dark_noise(h, w, 3, seed=s + 1), P.noise(h, w, 3, seed=s + 2), P.dark_noise(h, w, 3, seed=s + 3),
            P.noise(h, w, 3, seed=s + 4)]


def run(ctx, name, cand, mode):
    """One lanczos_resample_device call on device blocks of the library's own (lanczos_device_alloc / _copy: a child process
    does not count on torch seeing the device)."""
    import ctypes
    lib = L._lib()
    lib.lanczos_device_alloc.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    lib.lanczos_device_free.argtypes = [ctypes.c_int, ctypes.c_void_p]
    lib.lanczos_device_copy.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    bps, c, s, a = M.INSTANCES[INSTANCE]
    w, h, frames = cand
    d = L.make_desc(w, h, c, s, 1, a, bps, mode)
    idx = np.arange(frames) % 5
    x = np.ascontiguousarray(np.stack(base_frames(name, w, h))[idx])
    y = np.zeros((frames, h * s, w * s, c), np.uint8)
    dx, dy = ctypes.c_void_p(), ctypes.c_void_p()
    try:
        for ptr, arr in ((dx, x), (dy, y)):
            rc = lib.lanczos_device_alloc(0, ctypes.byref(ptr), arr.nbytes)
            assert rc == L.OK, f"lanczos_device_alloc: {rc}"
        rc = lib.lanczos_device_copy(0, dx, x.ctypes.data, x.nbytes, 1)
        assert rc == L.OK, f"lanczos_device_copy to the device: {rc}"
        ctx.resample_device(d, dx, dy, frames, 0, 0, None)   # the NULL stream: the blocking copy below is ordered behind it
        r = ctx.last_route()
        info, tab = ctx.last_march_table()
        rc = lib.lanczos_device_copy(0, y.ctypes.data, dy, y.nbytes, 0)
        assert rc == L.OK, f"lanczos_device_copy from the device: {rc}"
    finally:
        lib.lanczos_device_free(0, dx)
        lib.lanczos_device_free(0, dy)
    recur = bool(np.array_equal(y, y[:5][idx]))
    return r, info, tab, y[:5].copy(), recur


def main(out_path, want_mode_slots, forced=None):
    """forced: the "slots" batches the default run chose, {"exact": .., "lsb1": ..} (the runs under a switch take the same ones:
    their bytes are compared)."""
    ctx = L.Context(0)
    res = {}
    try:
        for name, cands in REQUESTS.items():
            for mode, tag in ((L.MODE_EXACT, "exact"), (L.MODE_LSB1, "lsb1")):
                for cand in ([forced[tag]] if name == "slots" and forced else cands):
                    r, info, tab, first, recur = run(ctx, name, cand, mode)
                    if (r.main, r.launches) == (L.ROUTE_MAIN_MARCH, 1) and (name != "slots" or info.mode == want_mode_slots):
                        break
                res[f"{name}:{tag}:cand"] = np.array(cand)
                res[f"{name}:{tag}:route"] = np.array([r.main, r.prefix, r.launches])
                res[f"{name}:{tag}:info"] = np.array(info)
                res[f"{name}:{tag}:table"] = tab
                res[f"{name}:{tag}:first"] = first
                res[f"{name}:{tag}:recur"] = np.array(recur)
    finally:
        ctx.close()
    np.savez(out_path, **res)
    return 0


if __name__ == "__main__":
    forced = None
    if len(sys.argv) > 3:   # "w,h,frames/w,h,frames": EXACT / LSB1
        forced = dict(zip(("exact", "lsb1"), (tuple(int(v) for v in part.split(",")) for part in sys.argv[3].split("/"))))
    sys.exit(main(sys.argv[1], int(sys.argv[2]), forced))
