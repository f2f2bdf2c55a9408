"""The upscale entry's decision held against its restatement, without a GPU: up_route (csrc/lanczos_upscale_route.cpp), run on the
host by tests/native/upscale_route_check.hip, says for every request of a cross product what upscale_route_cfg.predict says --
the refusal, the kernel family, the main kernel, and the frame count and prefix route of every launch.  A census asserts that the
product reaches every (main, prefix) pair tests/test_upscale_routes_gpu.py reaches on a device, every refusal, and a split batch
whose smaller last launch rides behind launches that send their prefix rows in front.

What each of four single changes to the route unit fails here (each was made, alone, and the file run):
  `>=` -> `>` in the 2 * pf split rule                test_the_route_is_the_prediction (frames = 2 * pf: one launch, not two)
  the riding cap `> cus` -> `>= cus`                  test_the_route_is_the_prediction (blocks * frames == cus: front, not riding)
  `in_h >= M2` dropped from the front conditions      test_the_route_is_the_prediction (in_h = M2 - 1 asked with the unclipped prefix,
                                                      large batch: front, not behind -- the plan's own prefix of such a frame is
                                                      clipped, so prefix_reg_supports refuses it as well)
  the forced-FAST refusal dropped / moved behind HLS  test_the_route_is_the_prediction (forced FAST without an instance: generic runs)
"""
import itertools
import os
import shutil
import subprocess

import pytest

import fast_cfg as F
import march_fixup_cfg as MF
import march_table_cfg as M
import upscale_route_cfg as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lanczos-hls_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

DEVICES = [(1, 256), (2, 256), (3, 256), (4, 256), (4, 8)]   # (resident workgroups per CU, CUs)
FORCES = (U.KERNEL_NONE, U.KERNEL_GENERIC, U.KERNEL_FAST)
SWITCHES = ({}, {"tile_kernel": 1}, {"separate_prefix": 1}, {"no_ratp": 1})


def _hipcc(tmp, name, sources):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    path = str(tmp / name)
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, *sources, "-o", path], check=True, timeout=600)
    return path


@pytest.fixture(scope="module")
def route_exe(tmp_path_factory):
    """tests/native/upscale_route_check.hip with the two host-only translation units: no library load, no kernel, no GPU"""
    return _hipcc(tmp_path_factory.mktemp("upscale_route"), "upscale_route_check",
                  [os.path.join(ROOT, "tests", "native", "upscale_route_check.hip"), os.path.join(CSRC, "lanczos_upscale_route.cpp"),
                   os.path.join(CSRC, "lanczos_taps.cpp")])


def _frame_counts(pf, cus):
    return sorted({n for n in (1, 5, 8, pf - 1, pf, pf + pf // 2 - 1, pf + pf // 2, 2 * pf - 1, 2 * pf, 2 * pf + 3, cus + 1, 65536) if n >= 1})


def _width(inst, aligned, near):
    bps, c, s, a = inst
    return next(w for w in range(near, near + 64) if ((w * c * bps) % 16 == 0) == aligned and (w * s * c * bps) % 4 == 0)


def cases():
    """[(Request, Facts or None)]: the cross product of the module docstring, frames of 16 to 64 input pixels"""
    out = []
    for inst in sorted(F.FAST_INSTANCES):
        bps, c, s, a = inst
        K, Mm, M2 = U._prefix_rows(s, a)
        w = _width(inst, True, 48)
        for nb, cus in DEVICES:
            f = U.facts(inst, nb, cus)
            pf = M.preferred_frames(nb, cus, -(-w * s // f.strip_out_px))
            for frames in _frame_counts(pf, cus):
                for h in (M2 - 1, M2):
                    for force, sw in itertools.product(FORCES, SWITCHES):
                        if force != U.KERNEL_NONE and (sw or h != M2):
                            continue
                        out.append((U.request(w, h, c, bps, s, 1, a, frames=frames, force=force, **sw), f))
                # strips: from row 0 ending inside the prefix rows, across K, wholly below K, row0 > 0 inside the prefix rows
                for row0, rows in ((0, K - 1), (0, K), (0, K + 3), (K, 4), (K + 2, 3), (1, K + 2)):
                    out.append((U.request(w, M2 + 4, c, bps, s, 1, a, row0=row0, rows=rows, frames=frames), f))
            # alignment of the input (march or tile) and of the output (an instance or k_generic)
            in_pitch, out_pitch = w * c * bps, w * s * c * bps
            for frames in (1, cus + 1):
                for kw in ({"in_base": 8}, {"in_stride": in_pitch * M2 + 8}, {"in_stride": in_pitch * M2 + 32}, {"out_base": 1}, {"out_base": 2},
                           {"out_stride": out_pitch * M2 * s + 2}, {"out_stride": out_pitch * M2 * s + 64}):
                    out.append((U.request(w, M2, c, bps, s, 1, a, frames=frames, **kw), f))
                wt = _width(inst, False, 16)
                out.append((U.request(wt, M2, c, bps, s, 1, a, frames=frames), f))
                if (17 * s * c * bps) % 4 != 0:   # output rows that are no dword multiples
                    out.append((U.request(17, M2, c, bps, s, 1, a, frames=frames), f))
                    out.append((U.request(17, M2, c, bps, s, 1, a, frames=frames, force=U.KERNEL_FAST), f))
        # a prefix whose row arrays do not fit the instance's LDS: MarchFacts of a smaller workgroup memory
        small = U.facts(inst, 2, 256)._replace(lds_bytes=(Mm + M2) * U.facts(inst, 2, 256).nt * bps - 1)
        out.append((U.request(w, M2, c, bps, s, 1, a, frames=1), small))
        out.append((U.request(w, M2, c, bps, s, 1, a, frames=1), small._replace(lds_bytes=small.lds_bytes + 1)))
        # the front kernel does not clamp rows beyond the frame: a frame one row short of M2 is refused it whatever prefix the query
        # holds (the plan's prefix of such a frame is clipped and differs from the instance's anyway: asked with the unclipped one)
        for h in (M2 - 1, M2):
            out.append((U.request(w, h, c, bps, s, 1, a, frames=257, prefix=(K, Mm, M2)), U.facts(inst, 4, 256)))
    # rational scales, periodic and not; an integer scale without an instance; deep prefixes (behind, then streamed); the HLS mode
    others = [(3, 2), (4, 3), (5, 2), (5, 3), (5, 1), (9, 8), (1, 1)]
    for (sn, sd), c, bps, a in itertools.product(others, (1, 3, 4), (1, 2), (2, 3)):
        w = 16 * sd
        for mode, force, frames, sw in itertools.product((U.MODE_LSB1, U.MODE_EXACT, U.MODE_HLS), FORCES, (1, 5, 65535, 65536), SWITCHES):
            if sw and force != U.KERNEL_NONE:
                continue
            out.append((U.request(w, 8 * sd, c, bps, sn, sd, a, mode=mode, frames=frames, force=force, **sw), None))
        out.append((U.request(w + 1, 8 * sd, c, bps, sn, sd, a, out_base=2), None))
    for mode, force in itertools.product((U.MODE_LSB1, U.MODE_HLS), FORCES):   # HLS on a descriptor that has an instance
        out.append((U.request(48, 12, 3, 1, 2, 1, 3, mode=mode, frames=3, force=force), U.facts((1, 3, 2, 3), 4, 256)))
    out.append((U.request(32, 600, 4, 2, 257, 256, 3, frames=3), None))   # K = 515: streamed
    out.append((U.request(24, 1000, 1, 1, 1, 1, 3, frames=3), None))      # S = 1: the whole height is prefix
    return out


def _routes(exe, tmp_path, lines):
    path = str(tmp_path / "requests.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[len(lines)] == "done %d" % len(lines), out[-3:]
    routes = []
    for i, text in enumerate(out[:len(lines)]):
        t = text.split(None, 2)
        assert t[0] == "ROUTE" and int(t[1]) == i, text
        routes.append(U.parse_route(t[2]))
    return routes


def test_the_route_is_the_prediction(route_exe, tmp_path):
    todo = cases()
    assert len(todo) > 20000
    routes = _routes(route_exe, tmp_path, [U.route_line(q, f) for q, f in todo])
    pairs, refusals, split_ride_behind_front = set(), set(), 0
    for (q, f), got in zip(todo, routes):
        want = U.predict(q, f)
        assert got == want, f"{q} {f}: up_route says {got}, predicted {want}"
        if got.err:
            refusals.add("row0" if q.row0 else "hls-force" if q.mode == U.MODE_HLS and q.force else "hls-frames" if q.mode == U.MODE_HLS
                         else "forced-fast")
            continue
        pairs |= {(got.main, p) for _, p in got.launches}
        if len(got.launches) > 1 and got.launches[0][1] == U.PREFIX_FRONT and got.launches[-1][1] == U.PREFIX_RIDING:
            split_ride_behind_front += 1
    # every pair tests/test_upscale_routes_gpu.py reaches on a device
    assert pairs >= {(U.MAIN_MARCH, U.PREFIX_RIDING), (U.MAIN_MARCH, U.PREFIX_FRONT), (U.MAIN_MARCH, U.PREFIX_BEHIND), (U.MAIN_MARCH, U.PREFIX_NONE),
                     (U.MAIN_NONE, U.PREFIX_FRONT), (U.MAIN_TILE, U.PREFIX_BEHIND), (U.MAIN_RATP, U.PREFIX_BEHIND), (U.MAIN_RAT, U.PREFIX_BEHIND),
                     (U.MAIN_RAT, U.PREFIX_STREAMED), (U.MAIN_GENERIC, U.PREFIX_STREAMED), (U.MAIN_GENERIC, U.PREFIX_BEHIND),
                     (U.MAIN_HLS, U.PREFIX_NONE)}, pairs
    assert refusals == {"row0", "hls-force", "hls-frames", "forced-fast"}, refusals
    assert split_ride_behind_front, "no split batch whose last launch rides behind launches with the prefix in front"


def test_the_restated_instance_constants(tmp_path):
    """MarchFacts' nt, lds_bytes and strip_out_px as upscale_route_cfg.facts restates them are MarchCfg's own, for all 35 instances"""
    src = tmp_path / "march_consts.hip"
    src.write_text('#include <hip/hip_runtime.h>\n#include <cstdio>\n#include "lanczos_hip.h"\n#include "lanczos_march.hpp"\n'
                   'int main() {\n#define X(T, C, S, A) printf("%d %d %d %d %d %d %d\\n", (int)sizeof(T), C, S, A, lz::MarchCfg<T, C, S, A>::NT, '
                   'lz::MarchCfg<T, C, S, A>::LDS_BYTES, lz::MarchCfg<T, C, S, A>::F::TWP_OUT);\n    LZ_FAST_CONFIGS(X)\n    return 0;\n}\n')
    exe = _hipcc(tmp_path, "march_consts", [str(src)])
    rows = [tuple(int(v) for v in line.split()) for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n") if line]
    assert len(rows) == 35 and {r[:4] for r in rows} == set(F.FAST_INSTANCES)
    for r in rows:
        f = U.facts(r[:4], 1, 256)
        assert (f.nt, f.lds_bytes, f.strip_out_px) == r[4:], (r, f)
