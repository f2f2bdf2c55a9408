"""The instances of the periodic rational-scale kernel k_ratp, their tile constants and the frames that test them -- TEST
INFRASTRUCTURE ONLY.

RATP_INSTANCES restates LZ_RATP_CONFIGS of csrc/lanczos_rational.hpp as (bytes per sample, channels, N, D, a); ratp_cfg()
restates the constants of RatPCfg<T, C, N, D, A>; RATP_SHAPES names, per instance, the smallest input frame at which the
instance has two tiles each way, a last tile that ends inside a unit, a last period cut by the frame, output rows that are
dword multiples and -- where C * SB allows -- input rows that are not (the byte-load branch of the LOAD step), plus the
height of about twice that at which there are three tile rows.  tests/test_rational_instances.py keeps all three honest
against the header without a GPU; tests/test_rational_instances_gpu.py runs them.
"""
import collections
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lanczos-hls_amd", "csrc", "lanczos_rational.hpp")

# (bytes per sample, channels, N, D, a)
RATP_INSTANCES = {(1, 3, 4, 3, 3), (1, 3, 3, 2, 3), (1, 3, 5, 2, 3), (1, 3, 5, 4, 3), (1, 4, 4, 3, 3), (1, 4, 3, 2, 3), (1, 1, 4, 3, 3),
                  (1, 1, 3, 2, 3), (1, 3, 4, 3, 2), (1, 3, 3, 2, 2), (2, 4, 3, 2, 3)}

# instance -> (in_w, in_h, tall in_h)
RATP_SHAPES = {
    (1, 3, 4, 3, 3): (159, 44, 88),
    (1, 3, 3, 2, 3): (115, 41, 83),
    (1, 3, 5, 2, 3): (101, 27, 55),
    (1, 3, 5, 4, 3): (199, 45, 90),
    (1, 4, 4, 3, 3): (40, 44, 88),
    (1, 4, 3, 2, 3): (41, 41, 83),
    (1, 1, 4, 3, 3): (159, 44, 88),
    (1, 1, 3, 2, 3): (115, 41, 83),
    (1, 3, 4, 3, 2): (171, 44, 88),
    (1, 3, 3, 2, 2): (123, 41, 83),
    (2, 4, 3, 2, 3): (41, 41, 83),
}

RatPCfg = collections.namedtuple("RatPCfg", "SB C N D A TAPS VEC UP P_IN P_OUT UOD NT TP TH NR NVG NUW NVT WIN_PX LPB IN_PITCH MIS NW "
                                            "WIN_DW0 UNIT_IN_B H_PITCH LDS_BYTES")


def header_text():
    with open(HEADER) as f:
        return f.read()


def header_instances(text=None):
    """The entries of LZ_RATP_CONFIGS, in the header's order, as (bytes per sample, channels, N, D, a)."""
    text = header_text() if text is None else text
    m = re.search(r"#define LZ_RATP_CONFIGS\(X\)((?:\s*\\\n\s*X\([^)]*\))+)", text)
    assert m, "LZ_RATP_CONFIGS not found in lanczos_rational.hpp"
    out = []
    for t, c, n, d, a in re.findall(r"X\((\w+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+)\)", m.group(1)):
        out.append(({"uint8_t": 1, "uint16_t": 2}[t], int(c), int(n), int(d), int(a)))
    return out


def header_constant(name, text=None):
    """The default of a `#define NAME value` / `constexpr int NAME = value;` of the header."""
    text = header_text() if text is None else text
    m = re.search(r"#define %s (\d+)" % name, text) or re.search(r"constexpr int %s = (\d+);" % name, text)
    assert m, name
    return int(m.group(1))


def ratp_cfg(inst, rows=48, nvg=3, nt=512):
    """RatPCfg<T, C, N, D, A> of csrc/lanczos_rational.hpp, formula by formula (rows = LZ_RATP_ROWS, nvg = LZ_RATP_NVG, nt = NT)."""
    SB, C, N, D, A = inst
    TAPS, VEC = 2 * A, 4 // SB
    UP = next((u for u in range(1, 5) if (u * N * C * SB) % 4 == 0 and (u * D * C * SB) % 4 == 0), 4)
    P_IN, P_OUT = UP * D, UP * N
    UOD = P_OUT * C * SB // 4
    TP = max(rows // N, 1)
    TH = TP * N
    NR = TP * D + TAPS - 1
    NVG = nvg if TP % nvg == 0 else (2 if TP % 2 == 0 else 1)
    NUW = nt // NR
    while NUW > 1 and NUW * UOD * NVG > nt:
        NUW -= 1
    NUW = max(NUW, 1)
    NVT = NUW * UOD
    WIN_PX = P_IN + TAPS - 1
    LPB = ((A - 1) * C * SB + 15) // 16 * 16
    IN_PITCH = (LPB + NUW * P_IN * C * SB + A * C * SB + 15) // 16 * 16
    MIS = (LPB - (A - 1) * C * SB) % 4
    NW = (MIS + WIN_PX * C * SB + 3) // 4
    WIN_DW0 = (LPB - (A - 1) * C * SB - MIS) // 4
    UNIT_IN_B = P_IN * C * SB
    H_PITCH = NVT * 4
    return RatPCfg(SB, C, N, D, A, TAPS, VEC, UP, P_IN, P_OUT, UOD, nt, TP, TH, NR, NVG, NUW, NVT, WIN_PX, LPB, IN_PITCH, MIS, NW,
                   WIN_DW0, UNIT_IN_B, H_PITCH, NR * IN_PITCH + NR * H_PITCH)


def prefix_rows(N, D, a):
    """K of a frame tall enough that no tap is clipped: output row o reads input rows up to first(o) + 2a - 1 with
    first(o) = D * (o // N) + (o % N) * D // N - a + 1 (what ratp_prepare checks index by index); the in-place vertical pass
    (full_TB.h:67-77) reads rows already written for every o whose last row lies below o itself."""
    last = lambda o: D * (o // N) + (o % N) * D // N + a
    return max(o + 1 for o in range(8 * a * N) if last(o) > o)


def shape_facts(inst, in_w, in_h, **kw):
    """What a frame gives an instance: out size, tiles each way, whether the last tile ends inside a unit / a period ..."""
    k = ratp_cfg(inst, **kw)
    out_w, out_h = in_w * k.N // k.D, in_h * k.N // k.D
    tile_w = k.NUW * k.P_OUT
    return {
        "out_w": out_w, "out_h": out_h, "tile_w": tile_w, "tile_h": k.TH,
        "tiles_x": -(-out_w // tile_w), "tiles_y": -(-out_h // k.TH),
        "partial_unit": out_w % k.P_OUT != 0, "partial_period": out_h % k.N != 0,
        "out_rows_dwords": (out_w * k.C * k.SB) % 4 == 0, "in_rows_dwords": (in_w * k.C * k.SB) % 4 == 0,
        # ratp_prepare's condition on one axis (lanczos_rational.hpp: ref_ax)
        "periodic_axis": any(o > k.N * (k.A + 2) and i > 2 * k.A + k.D + 2 for o, i in ((out_w, in_w), (out_h, in_h))),
        "K": prefix_rows(k.N, k.D, k.A),
    }


def strip_cuts(inst, out_h, **kw):
    """Row boundaries that cut an output of out_h rows into strips none of which starts on a tile row or a period:
    0, c1, TH - 1, TH + N + 1, TH + 2N - 1, 2 TH - 2, out_h.  The first strip starts inside the in-place prefix rows and c1 is
    the first row >= max(7, K) that is no multiple of N (a strip that starts at 0 < row < K is refused by the entry point:
    the prefix recurrence needs rows [0, M) in one place); the strip [TH + N + 1, TH + 2N - 1) is narrower than a period."""
    k = ratp_cfg(inst, **kw)
    K = prefix_rows(k.N, k.D, k.A)
    c1 = max(7, K)
    while c1 % k.N == 0:
        c1 += 1
    return [0, c1, k.TH - 1, k.TH + k.N + 1, k.TH + 2 * k.N - 1, 2 * k.TH - 2, out_h]


def handover_frames(inst):
    """The three frames either side of ratp_prepare's `out_n > N * (a + 2) and in_n > 2a + D + 2`, with output rows that are
    dword multiples (rat_supports): [(in_w, in_h, True if an axis qualifies)] -- the largest frame where both axes fail, the
    smallest where only the width qualifies, the smallest where only the height does."""
    SB, C, N, D, A = inst
    ok = lambda n: n * N // D > N * (A + 2) and n > 2 * A + D + 2
    dword = lambda w: (w * N // D * C * SB) % 4 == 0
    n_q = next(n for n in range(1, 1000) if ok(n))
    assert not ok(n_q - 1) and all(ok(n) for n in range(n_q, n_q + 50))
    w_fail = next(w for w in range(n_q - 1, 0, -1) if dword(w))
    w_q = next(w for w in range(n_q, 1000) if dword(w))
    return [(w_fail, n_q - 1, False), (w_q, n_q - 1, True), (w_fail, n_q, True)]


def rat_frame(c, sb, sn, sd, tile_row_bytes=512, tile_h=32):
    """The smallest input frame (at least 100 x 50) whose sn/sd output spans two k_rat tiles each way (kRatTileRowBytes x
    kRatTileH) with ragged right and bottom edges and rows that are dword multiples (rat_supports); input rows that are no
    dword multiples where the sample size allows (the byte-load branch of k_rat's LOAD step)."""
    def fits(w):
        row = w * sn // sd * c * sb
        return row % 4 == 0 and row > tile_row_bytes and row % tile_row_bytes != 0
    cands = [w for w in range(100, 2000) if fits(w)]
    w = next((w for w in cands[:8] if (w * c * sb) % 4 != 0), cands[0])
    h = next(h for h in range(50, 200) if h * sn // sd > tile_h and (h * sn // sd) % tile_h != 0)
    return w, h
