"""Child process of test_parity_gpu.py::test_production_switches_change_no_result (not collected by pytest): the library reads
its environment switches once per process (csrc/lanczos_env.hpp), so every switch is tried in a fresh process.  Runs the
requests of SWITCH_REQUESTS in both parity modes and writes the outputs, the routes and the reported k_march workgroup tables to the
.npz named on the command line."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import lanczos_hls_amd as L  # noqa: E402
import patterns as P  # noqa: E402

# name -> (frames, sn, sd, a): a config 2 batch (k_march, prefix rows riding or in front), a periodic rational scale (k_ratp;
# k_rat under LANCZOS_NO_RATP) and a deep in-place prefix (K = 67: k_prefix behind k_rat)
SWITCH_REQUESTS = {
    "config2_batch": (lambda: np.stack([P.noise(1080, 1920, 3, seed=1), P.dark_noise(1080, 1920, 3, seed=2)]), 2, 1, 3),
    "rational_3_2": (lambda: P.noise(270, 480, 3, seed=3)[None], 3, 2, 3),
    "deep_prefix_33_32": (lambda: P.noise(160, 128, 3, seed=31)[None], 33, 32, 3),
}


def main(out_path):
    ctx = L.Context(0)
    res = {}
    try:
        for name, (gen, sn, sd, a) in SWITCH_REQUESTS.items():
            frames = gen()
            for mode, tag in ((L.MODE_EXACT, "exact"), (L.MODE_LSB1, "lsb1")):
                res[f"{name}:{tag}"] = ctx.resample(frames, sn, sd, a, mode)
                res[f"{name}:{tag}:kernel"] = np.array(ctx.last_kernel())
                r = ctx.last_route()
                res[f"{name}:{tag}:route"] = np.array([r.main, r.prefix, r.launches])
                info, tab = ctx.last_march_table()   # of the call's last launch; all zero where that was no k_march
                res[f"{name}:{tag}:table_info"] = np.array(info)
                res[f"{name}:{tag}:table"] = tab
    finally:
        ctx.close()
    np.savez(out_path, **res)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
