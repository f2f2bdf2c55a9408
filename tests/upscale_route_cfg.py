"""What a call of lanczos_resample_device does, predicted in plain Python -- TEST INFRASTRUCTURE ONLY.

up_route (csrc/lanczos_upscale_route.cpp) decides the refusal, the kernel family, the main kernel and the launches a call goes
out as, each with the route of its in-place prefix rows.  predict() restates that decision from the library's documents and
sources, not from its answers; tests/test_upscale_route_cfg.py holds the two against each other on the host over a cross product
of requests, tests/test_upscale_route_gpu.py on a device with the facts the device reports.  The instance constants, the
preferred batch size and the split rule are march_table_cfg's and march_fixup_cfg's.
"""
import collections
import math

import fast_cfg as F
import march_fixup_cfg as MF
import march_table_cfg as M
import ratp_cfg as R

OK, ERR_BAD_ARG, ERR_UNSUPPORTED = 0, 1, 2
MODE_LSB1, MODE_EXACT, MODE_HLS = 0, 1, 2
KERNEL_NONE, KERNEL_GENERIC, KERNEL_FAST, KERNEL_HLS = 0, 1, 2, 3
MAIN_NONE, MAIN_MARCH, MAIN_TILE, MAIN_RATP, MAIN_RAT, MAIN_GENERIC, MAIN_HLS = range(7)
PREFIX_NONE, PREFIX_RIDING, PREFIX_FRONT, PREFIX_BEHIND, PREFIX_STREAMED = range(5)

# the instances of k_prefix_reg: (bytes per sample, S, a)
PREFIX_REG_INSTANCES = {(1, s, a) for s in (2, 3, 4) for a in (2, 3, 4)} | {(2, s, a) for s in (2, 3) for a in (3, 4)}

Request = collections.namedtuple("Request", "in_w in_h c bps sn sd a mode row0 rows frames in_stride out_stride in_base out_base force "
                                            "tile_kernel separate_prefix no_ratp prefix")
Facts = collections.namedtuple("Facts", "nt lds_bytes strip_out_px wg_per_cu cus")
Route = collections.namedtuple("Route", "err kernel main launches")   # launches: ((frames, prefix), ...)


def request(in_w, in_h, c, bps, sn, sd, a, mode=MODE_LSB1, row0=0, rows=0, frames=1, in_stride=0, out_stride=0, in_base=0, out_base=0,
            force=KERNEL_NONE, tile_kernel=0, separate_prefix=0, no_ratp=0, prefix=None):
    """prefix: (K, M, M2) handed to the decision instead of the plan's (up_route is a function of its query: any facts may be asked)"""
    return Request(in_w, in_h, c, bps, sn, sd, a, mode, row0, rows, frames, in_stride, out_stride, in_base, out_base, force,
                   tile_kernel, separate_prefix, no_ratp, prefix)


def _prefix_rows(s, a):
    """K, M, M2 of an integer scale on a frame tall enough that no tap is clipped (csrc/lanczos_upscale.hpp prefix_K / _M / _M2
    restated): output row o reads rows up to o // s + a; K = rows that read a row below themselves, M = output rows the
    recurrence holds, M2 = H-pass rows it reads -- the smallest input height the front kernel admits."""
    last = lambda o: o // s + a
    K = max(o + 1 for o in range(4 * a * s + 8) if last(o) > o)
    M = max([K] + [last(o) + 1 for o in range(K)])
    M2 = max(last(o) + 1 for o in range(M))
    return K, M, M2


def v_first(in_h, sn, sd, a, hls=False):
    """first[] of the vertical axis (lanczos_taps.cpp: build_axis, build_axis_hls)"""
    out_h = in_h * sn // sd
    if hls:
        return [o * sd // sn - a + 1 for o in range(out_h)]
    scale = sn / sd
    return [int(math.floor(o / scale)) - a + 1 for o in range(out_h)]


def prefix_info(first, in_h, a):
    """K, M, M2 of a frame (lanczos_taps.cpp: prefix_info): taps clipped to the frame"""
    last = lambda o: min(first[o] + 2 * a - 1, in_h - 1)
    K = max([o + 1 for o in range(len(first)) if last(o) > o], default=0)
    Mm = max([K] + [last(o) + 1 for o in range(K)])
    M2 = max([last(o) + 1 for o in range(min(Mm, len(first)))], default=0)
    return K, Mm, M2


def strip_input_rows(first, a, in_h, row0, rows, K, M2):
    hi = first[row0 + rows - 1] + 2 * a - 1
    if row0 < K:
        hi = max(hi, M2 - 1)
    lo, hi = max(first[row0], 0), min(hi, in_h - 1)
    return lo, hi - lo + 1


def instance(q):
    """(bps, c, S, a) if the descriptor has an instance of the integer-scale kernels (LZ_FAST_CONFIGS), else None"""
    inst = (q.bps, q.c, q.sn, q.a)
    return inst if q.sd == 1 and inst in F.FAST_INSTANCES else None


def march_lds_bytes(inst):
    """MarchCfg::LDS_BYTES (csrc/lanczos_march.hpp): two input tiles of a tick, the H ring, the worklists, the phase weights"""
    k, f = MF.march_cfg(inst), F.fast_cfg(inst)
    load_it = -(-(k.MS * (f.IN_PITCH // 16)) // k.NT)
    return 2 * load_it * k.NT * 16 + k.RS * f.H_PITCH + -(-k.NU // 64) * k.WLW * 2 + 4 * 8 * 8


def facts(inst, wg_per_cu, cus):
    """MarchFacts of an instance on a device with these two figures"""
    k = MF.march_cfg(inst)
    return Facts(k.NT, march_lds_bytes(inst), k.TWP_OUT, wg_per_cu, cus)


def plan_facts(q):
    """(fast_ok, rat_ok, ratp_ok): what the plan of the descriptor holds (fast_prepare / rat_prepare / ratp_prepare succeed for
    every shape of the product: small frames, eps far below their limits)"""
    if q.mode == MODE_HLS:
        return 0, 0, 0
    rat = q.sd != 1
    periodic = (q.sn, q.sd) in ((3, 2), (4, 3), (5, 2))   # 5/3: x = o / SCALE rounds, not periodic
    return int(instance(q) is not None), int(rat), int(rat and periodic and (q.bps, q.c, q.sn, q.sd, q.a) in R.RATP_INSTANCES)


def predict(q, f=None):
    """The Route of request q; f: the Facts of its marching instance on the device (None: it has none)."""
    out_w, out_h = q.in_w * q.sn // q.sd, q.in_h * q.sn // q.sd
    hls = q.mode == MODE_HLS
    first = v_first(q.in_h, q.sn, q.sd, q.a, hls)
    K, Mm, M2 = (0, 0, 0) if hls else (q.prefix or prefix_info(first, q.in_h, q.a))
    row0, rows = (q.row0, q.rows) if q.rows else (0, out_h)
    has_prefix = row0 < K
    refused = Route(ERR_UNSUPPORTED, 0, 0, ())
    if has_prefix and row0 != 0:
        return refused
    in_row0, in_rows = strip_input_rows(first, q.a, q.in_h, row0, rows, K, M2)
    in_pitch, out_pitch = q.in_w * q.c * q.bps, out_w * q.c * q.bps
    in_stride, out_stride = q.in_stride or in_pitch * in_rows, q.out_stride or out_pitch * rows
    if hls:
        if q.force in (KERNEL_FAST, KERNEL_GENERIC) or q.frames > 65535:
            return refused
        return Route(OK, KERNEL_HLS, MAIN_HLS, ((q.frames, PREFIX_NONE),))
    fast_ok, rat_ok, ratp_ok = plan_facts(q)
    out_aligned = out_pitch % 4 == 0 and q.out_base % 4 == 0 and out_stride % 4 == 0
    use_fast = bool(fast_ok) and q.force != KERNEL_GENERIC and out_aligned
    use_rat = not use_fast and bool(rat_ok) and q.force != KERNEL_GENERIC and out_aligned and q.sn > q.sd and q.frames <= 65535
    if q.force == KERNEL_FAST and not use_fast and not use_rat:
        return refused
    march = use_fast and not q.tile_kernel and in_pitch % 16 == 0 and q.in_base % 16 == 0 and in_stride % 16 == 0
    kernel = KERNEL_FAST if use_fast or use_rat else KERNEL_GENERIC
    if march:
        main = MAIN_NONE if row0 + rows <= (K if has_prefix else 0) else MAIN_MARCH
    elif use_fast:
        main = MAIN_TILE
    elif use_rat:
        main = MAIN_RATP if ratp_ok and not q.no_ratp else MAIN_RAT
    else:
        main = MAIN_GENERIC
    bw = 128
    while bw > 32 and (Mm + M2) * bw * q.bps > 60 * 1024:
        bw //= 2
    streamed = (Mm + M2) * bw * q.bps > 60 * 1024

    def prefix_of(nf):
        if not has_prefix:
            return PREFIX_NONE
        if march and not q.separate_prefix:
            blocks = -(-out_w * q.c // f.nt)
            if (Mm + M2) * f.nt * q.bps <= f.lds_bytes and main != MAIN_NONE and blocks * nf <= f.cus:
                return PREFIX_RIDING
            if q.sd == 1 and q.in_h >= M2 and (q.bps, q.sn, q.a) in PREFIX_REG_INSTANCES and (K, Mm, M2) == _prefix_rows(q.sn, q.a):
                return PREFIX_FRONT
        return PREFIX_STREAMED if streamed else PREFIX_BEHIND

    sizes = [q.frames]
    if march:
        n_strips = -(-out_w // f.strip_out_px)
        if not M.single_launch(f.wg_per_cu, f.cus, n_strips, q.frames):
            pf = M.preferred_frames(f.wg_per_cu, f.cus, n_strips)
            sizes = [pf] * ((q.frames - 1) // pf) + [q.frames - (q.frames - 1) // pf * pf]
    return Route(OK, kernel, main, tuple((n, prefix_of(n)) for n in sizes))


def route_line(q, f=None):
    """The request as tests/native/upscale_route_check.hip reads it"""
    return " ".join(str(int(v)) for v in (q.in_w, q.in_h, q.c, q.bps, q.sn, q.sd, q.a, q.mode, q.row0, q.rows, q.frames, q.in_stride,
                                          q.out_stride, q.in_base, q.out_base, q.force, *plan_facts(q), q.tile_kernel,
                                          q.separate_prefix, q.no_ratp, f is not None, *(f or (0, 0, 0, 0, 0)),
                                          *(q.prefix or (-1, 0, 0))))


def parse_route(text):
    """A ROUTE line of upscale_route_check's output (without its line number) as a Route"""
    t = text.split()
    if int(t[0]) != OK:
        return Route(int(t[0]), 0, 0, ())
    launches = []
    for item in t[4:]:
        count, rest = item.split("x")
        frames, prefix = rest.split(":")
        launches += [(int(frames), int(prefix))] * int(count)
    assert len(launches) == int(t[3]), text
    return Route(OK, int(t[1]), int(t[2]), tuple(launches))
