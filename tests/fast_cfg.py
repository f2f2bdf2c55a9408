"""The instances of the tile-per-workgroup integer-scale kernel k_fast, their tile constants, the frames that test them and
the two contents that steer its worklist -- TEST INFRASTRUCTURE ONLY.

FAST_INSTANCES restates LZ_FAST_CONFIGS_G0..G3 of csrc/lanczos_fast.hpp as (bytes per sample, channels, S, a); fast_cfg()
restates FastShape<T, C, S, A> and FastCfg<T, C, S, A> formula by formula; FAST_SHAPES names, per instance, the smallest input
frame that reaches the tile kernel by a plain call (input rows that are no 16-byte multiples, output rows that are dword
multiples) with two tiles across, a partial last tile that holds one whole unit and ends inside the next (on a unit boundary
where the dword condition forces in_w % P == 0), and 2 MR + a input rows: three tile rows, a ragged last one, and every LDS row
of the middle tile row -- both halo rows included -- inside the image.  FAST_SHAPES16 is the same frame at the smallest such
width whose rows ARE 16-byte multiples (the uint4 branch of the LOAD step; only a frame stride keeps k_march away).

sparse_flips() and dense_flips() are frames that decide which branch of the FIXUP step a tile takes: the worklist of a tile is
at most sparse_bound() long whatever eps is (<= WL_CAP / 2: the list branch) and at least dense_count() long under any
vlim >= 1 (> WL_CAP in the middle tile row: the redo-everything branch).

tests/test_fast_instances.py keeps all of this honest against the header and the oracle without a GPU;
tests/test_fast_instances_gpu.py runs it.
"""
import collections
import os
import re

import numpy as np

from ratp_cfg import prefix_rows

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lanczos-hls_amd", "csrc", "lanczos_fast.hpp")
GENERIC_HEADER = os.path.join(os.path.dirname(HEADER), "lanczos_generic.hpp")

# (bytes per sample, channels, S, a)
FAST_INSTANCES = ({(1, c, s, a) for c in (1, 3, 4) for s in (2, 3, 4) for a in (2, 3, 4)} |
                  {(2, c, s, a) for c in (3, 4) for s in (2, 3) for a in (3, 4)})

# instance -> (in_w, in_h)
FAST_SHAPES = {
    (1, 1, 2, 2): (266, 62), (1, 1, 2, 3): (266, 63), (1, 1, 2, 4): (266, 64),
    (1, 1, 3, 2): (268, 42), (1, 1, 3, 3): (268, 43), (1, 1, 3, 4): (268, 44),
    (1, 1, 4, 2): (265, 32), (1, 1, 4, 3): (265, 33), (1, 1, 4, 4): (265, 34),
    (1, 3, 2, 2): (134, 62), (1, 3, 2, 3): (134, 63), (1, 3, 2, 4): (134, 64),
    (1, 3, 3, 2): (136, 42), (1, 3, 3, 3): (136, 43), (1, 3, 3, 4): (136, 44),
    (1, 3, 4, 2): (133, 32), (1, 3, 4, 3): (133, 33), (1, 3, 4, 4): (133, 34),
    (1, 4, 2, 2): (133, 62), (1, 4, 2, 3): (133, 63), (1, 4, 2, 4): (133, 64),
    (1, 4, 3, 2): (133, 42), (1, 4, 3, 3): (133, 43), (1, 4, 3, 4): (133, 44),
    (1, 4, 4, 2): (133, 32), (1, 4, 4, 3): (133, 33), (1, 4, 4, 4): (133, 34),
    (2, 3, 2, 3): (67, 63), (2, 3, 2, 4): (67, 64),
    (2, 3, 3, 3): (68, 43), (2, 3, 3, 4): (68, 44),
    (2, 4, 2, 3): (67, 63), (2, 4, 2, 4): (67, 64),
    (2, 4, 3, 3): (67, 43), (2, 4, 3, 4): (67, 44),
}

# instance -> in_w of the frame whose rows are 16-byte multiples (the height is FAST_SHAPES')
FAST_SHAPES16 = {
    (1, 1, 2, 2): 272, (1, 1, 2, 3): 272, (1, 1, 2, 4): 272, (1, 1, 3, 2): 272, (1, 1, 3, 3): 272, (1, 1, 3, 4): 272,
    (1, 1, 4, 2): 272, (1, 1, 4, 3): 272, (1, 1, 4, 4): 272,
    (1, 3, 2, 2): 144, (1, 3, 2, 3): 144, (1, 3, 2, 4): 144, (1, 3, 3, 2): 144, (1, 3, 3, 3): 144, (1, 3, 3, 4): 144,
    (1, 3, 4, 2): 144, (1, 3, 4, 3): 144, (1, 3, 4, 4): 144,
    (1, 4, 2, 2): 136, (1, 4, 2, 3): 136, (1, 4, 2, 4): 136, (1, 4, 3, 2): 136, (1, 4, 3, 3): 136, (1, 4, 3, 4): 136,
    (1, 4, 4, 2): 136, (1, 4, 4, 3): 136, (1, 4, 4, 4): 136,
    (2, 3, 2, 3): 72, (2, 3, 2, 4): 72, (2, 3, 3, 3): 72, (2, 3, 3, 4): 72,
    (2, 4, 2, 3): 68, (2, 4, 2, 4): 68, (2, 4, 3, 3): 68, (2, 4, 3, 4): 68,
}

# Output samples a test frame may hold.  Two tiles across and three tile rows with the middle one's halo rows in the image are
# more than that for 8-bit RGB at 4x and RGBA at 3x and 4x (129 px x S x C samples x (2 MR + a) S rows: 201 000 to 290 000), so
# those nine get what they need.
MAX_OUT_SAMPLES = 200000
MAX_OUT_SAMPLES_BIG = 300000

# instances whose frame may hold up to MAX_OUT_SAMPLES_BIG samples
BIG_FRAMES = {(1, c, s, a) for (c, s) in ((3, 4), (4, 3), (4, 4)) for a in (2, 3, 4)}

FastCfg = collections.namedtuple("FastCfg", "SB C S A TAPS P UPR TWP_IN TWP_OUT TWS_OUT TWB_OUT VEC NVT NGRP NT MR MRG TH NR LPB "
                                            "IN_PITCH H_PITCH WIN_PX MIS NW UNIT_IN_DW UNIT_OUT_S UNIT_OUT_DW WIN_DW0 WL_CAP "
                                            "WL_ROW_BITS WL_SMP_BITS LDS_BYTES")


def inst_id(i):
    """u8-c3-2x-a3"""
    return f"u{8 * i[0]}-c{i[1]}-{i[2]}x-a{i[3]}"


def header_text():
    """lanczos_upscale.hpp (the instance lists LZ_FAST_CONFIGS_G0..G3) followed by lanczos_fast.hpp (the shapes)"""
    with open(os.path.join(os.path.dirname(HEADER), "lanczos_upscale.hpp")) as f, open(HEADER) as g:
        return f.read() + g.read()


def header_instances(text=None):
    """The entries of LZ_FAST_CONFIGS_G0..G3, in the header's order, as (bytes per sample, channels, S, a)."""
    text = header_text() if text is None else text
    out = []
    for g in range(4):
        m = re.search(r"#define LZ_FAST_CONFIGS_G%d\(X\)[^\n]*\\\n((?:[^\n]*\\\n)*[^\n]*)\n" % g, text)
        assert m, "LZ_FAST_CONFIGS_G%d not found in lanczos_upscale.hpp" % g
        found = re.findall(r"X\((\w+),\s*(\d+),\s*(\d+),\s*(\d+)\)", m.group(1))
        assert found, "LZ_FAST_CONFIGS_G%d has no entries" % g
        out += [({"uint8_t": 1, "uint16_t": 2}[t], int(c), int(s), int(a)) for t, c, s, a in found]
    assert re.search(r"#define LZ_FAST_CONFIGS\(X\) LZ_FAST_CONFIGS_G0\(X\) LZ_FAST_CONFIGS_G1\(X\) LZ_FAST_CONFIGS_G2\(X\) "
                     r"LZ_FAST_CONFIGS_G3\(X\)\n", text), "LZ_FAST_CONFIGS is no longer the four groups"
    return out


def header_shape(text=None):
    """FastShape of the header: {"mr": {S: MR}, "ngrp": {S: NGRP}, "wl_cap": WL_CAP, "upr": UPR}."""
    text = header_text() if text is None else text
    m = re.search(r"int MR = S == 2 \? (\d+) : \(S == 3 \? (\d+) : (\d+)\);", text)
    n = re.search(r"int NGRP = S == 2 \? (\d+) : (\d+);", text)
    w = re.search(r"constexpr int WL_CAP = (\d+);", text)
    u = re.search(r"int UPR = UPR_ > 0 \? UPR_ : (\d+);", text)
    assert m and n and w and u, "FastShape / WL_CAP / UPR not found in lanczos_fast.hpp"
    return {"mr": {2: int(m.group(1)), 3: int(m.group(2)), 4: int(m.group(3))},
            "ngrp": {2: int(n.group(1)), 3: int(n.group(2)), 4: int(n.group(2))}, "wl_cap": int(w.group(1)), "upr": int(u.group(1))}


def generic_tile(text=None):
    """(kGenTileW, kGenTileH) of csrc/lanczos_generic.hpp."""
    if text is None:
        with open(GENERIC_HEADER) as f:
            text = f.read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % n, text).group(1)) for n in ("kGenTileW", "kGenTileH"))


_SHAPE = None


def fast_cfg(inst, shape=None):
    """FastCfg<T, C, S, A> of csrc/lanczos_fast.hpp, formula by formula; `shape` = header_shape() (read once by default)."""
    global _SHAPE
    if shape is None:
        _SHAPE = _SHAPE or header_shape()
        shape = _SHAPE
    SB, C, S, A = inst
    TAPS = 2 * A
    P = (8 if C == 1 else 4) if SB == 1 else 2
    UPR = shape["upr"]
    TWP_IN = P * UPR
    TWP_OUT = TWP_IN * S
    TWS_OUT = TWP_OUT * C
    TWB_OUT = TWS_OUT * SB
    VEC = 4 // SB
    NVT = TWB_OUT // 4
    NGRP = shape["ngrp"][S]
    NT = (NVT * NGRP + 63) // 64 * 64
    MR = shape["mr"][S]
    MRG = MR // NGRP
    TH = MR * S
    NR = MR + TAPS - 1
    LPB = ((A - 1) * C * SB + 15) // 16 * 16
    IN_PITCH = (LPB + TWP_IN * C * SB + A * C * SB + 15) // 16 * 16
    H_PITCH = TWB_OUT
    WIN_PX = P + TAPS - 1
    MIS = (LPB - (A - 1) * C * SB) % 4
    NW = (MIS + WIN_PX * C * SB + 3) // 4
    UNIT_IN_DW = P * C * SB // 4
    UNIT_OUT_S = P * S * C
    UNIT_OUT_DW = UNIT_OUT_S * SB // 4
    WIN_DW0 = (LPB - (A - 1) * C * SB - MIS) // 4
    WL_CAP = shape["wl_cap"]
    WL_ROW_BITS = 5 if NR <= 32 else 6
    WL_SMP_BITS = 16 - WL_ROW_BITS
    LDS_BYTES = NR * IN_PITCH + NR * H_PITCH + WL_CAP * 2 + 16
    return FastCfg(SB, C, S, A, TAPS, P, UPR, TWP_IN, TWP_OUT, TWS_OUT, TWB_OUT, VEC, NVT, NGRP, NT, MR, MRG, TH, NR, LPB, IN_PITCH,
                   H_PITCH, WIN_PX, MIS, NW, UNIT_IN_DW, UNIT_OUT_S, UNIT_OUT_DW, WIN_DW0, WL_CAP, WL_ROW_BITS, WL_SMP_BITS, LDS_BYTES)


def static_assert_errors(k):
    """The static_asserts of FastCfg and k_fast on a restated configuration: the ones that fail, as text."""
    bad = []
    if (k.P * k.C * k.SB) % 4 != 0:
        bad.append("unit must cover whole dwords")
    if k.UNIT_OUT_S > 64:
        bad.append("flag mask is 64 bits")
    if k.MR % k.NGRP != 0:
        bad.append("V groups split the tile evenly")
    if not (k.NR <= 64 and k.TWS_OUT <= (1 << k.WL_SMP_BITS)):
        bad.append("worklist entry packs row | sample in 16 bits")
    if not (k.H_PITCH % 4 == 0 and k.IN_PITCH % 16 == 0):
        bad.append("LDS pitches")
    if (k.MIS + (k.A - 1) * k.C * k.SB) % 4 != 0:
        bad.append("own pixels start on a dword")
    if not (k.NGRP == 1 or k.NVT % 64 == 0):
        bad.append("V groups must be whole waves")
    if k.WIN_DW0 * 4 + (k.UPR - 1) * k.UNIT_IN_DW * 4 + k.NW * 4 > k.IN_PITCH:
        bad.append("a unit's window leaves its LDS row")
    return bad


def prefix_K(S, a):
    """K of an integer scale (lanczos_generic.hpp: prefix_K): output row o reads input rows up to o / S + a."""
    return prefix_rows(S, 1, a)


def shape_facts(inst, in_w, in_h, shape=None):
    """What a frame gives an instance."""
    k = fast_cfg(inst, shape)
    out_w, out_h = in_w * k.S, in_h * k.S
    tiles_x, tiles_y = -(-in_w // k.TWP_IN), -(-out_h // k.TH)
    return {
        "out_w": out_w, "out_h": out_h, "tiles_x": tiles_x, "tiles_y": tiles_y,
        "in_rows_16": (in_w * k.C * k.SB) % 16 == 0, "out_rows_dwords": (out_w * k.C * k.SB) % 4 == 0,
        "partial_tile": in_w % k.TWP_IN != 0, "partial_unit": in_w % k.P != 0,
        "whole_unit_in_last_tile": in_w % k.TWP_IN > k.P,
        "ragged_bottom": out_h % k.TH != 0,
        # LDS rows of tile row 1: input rows MR - a + 1 .. 2 MR + a - 1
        "middle_halo_in_image": k.MR - k.A + 1 >= 0 and 2 * k.MR + k.A - 1 <= in_h - 1,
        "out_samples": out_w * out_h * k.C, "K": prefix_K(k.S, k.A),
    }


def _width_ok(k, w, rows16, partial_unit):
    return ((w * k.C * k.SB) % 16 == 0) == rows16 and (w * k.S * k.C * k.SB) % 4 == 0 and w % k.TWP_IN > k.P and \
        (w % k.P != 0) == partial_unit


def partial_unit_possible(inst, shape=None):
    """Can a frame whose output rows are dword multiples end inside a unit?  Not where the dword condition forces
    in_w % P == 0: 8-bit RGB at 3x (9 in_w bytes a row: in_w % 4 == 0 == P) and 16-bit RGB at 3x (18 in_w: in_w even, P = 2)."""
    k = fast_cfg(inst, shape)
    return any(_width_ok(k, w, False, True) for w in range(k.TWP_IN, 2 * k.TWP_IN))


def smallest_frame(inst, shape=None):
    """The FAST_SHAPES entry of an instance, searched: the narrowest width past one tile + one unit with the properties of the
    module docstring, 2 MR + a rows."""
    k = fast_cfg(inst, shape)
    pu = partial_unit_possible(inst, shape)
    w = next(w for w in range(k.TWP_IN + 1, 2 * k.TWP_IN) if _width_ok(k, w, False, pu))
    return w, 2 * k.MR + k.A


def smallest_width16(inst, shape=None):
    k = fast_cfg(inst, shape)
    return next(w for w in range(k.TWP_IN + 1, 2 * k.TWP_IN) if _width_ok(k, w, True, False) or _width_ok(k, w, True, True))


def _off(c, n):
    """The first row >= c that is no multiple of any of n."""
    while any(c % m == 0 for m in n):
        c += 1
    return c


def strip_cuts(inst, out_h, shape=None):
    """Row boundaries that cut an output of out_h rows into strips: 0, c1, c2, c3, out_h - 1, out_h.  c1 is the first row
    >= max(7, K) that is no multiple of S (a strip that starts at 0 < row < K is refused: the prefix recurrence needs rows [0, M)
    in one place); no interior cut is a multiple of TH or of S, so every strip but the first starts inside a tile row (y_tile <
    y_begin) and off an integer phase; [c1, c2) lies inside tile row 0, [c2, c3) spans tile rows 0 and 1, [c3, out_h - 1) tile
    rows 1 and 2; the last strip is a single row (at S = 2 the only place for one: two odd cuts are never neighbours)."""
    k = fast_cfg(inst, shape)
    n = (k.S, k.TH)
    c1 = _off(max(7, prefix_K(k.S, k.A)), n)
    c2 = _off(max(c1 + 1, k.TH - k.S - 1), n)
    c3 = _off(k.TH + k.S + 1, n)
    return [0, c1, c2, c3, out_h - 1, out_h]


def cut_errors(inst, cuts, out_h, shape=None):
    """What strip_cuts promises, checked: the promises that do not hold, as text."""
    k = fast_cfg(inst, shape)
    K = prefix_K(k.S, k.A)
    bad = []
    if not (cuts == sorted(set(cuts)) and cuts[0] == 0 and cuts[-1] == out_h):
        bad.append("not ascending from 0 to out_h")
    c1 = cuts[1]
    if not (c1 >= max(7, K) and c1 % k.S != 0 and all(r % k.S == 0 for r in range(max(7, K), c1))):
        bad.append("first cut is not the first row >= max(7, K) off a multiple of S")
    if any(c % k.TH == 0 or c % k.S == 0 for c in cuts[1:-1]):
        bad.append("an interior cut on a multiple of TH or S")
    strips = list(zip(cuts, cuts[1:]))
    if not any(b - a == 1 for a, b in strips):
        bad.append("no single-row strip")
    if not any(a > 0 and a // k.TH == (b - 1) // k.TH and b - a > 1 for a, b in strips):
        bad.append("no strip inside one tile row")
    if not any((b - 1) // k.TH - a // k.TH == 1 for a, b in strips):
        bad.append("no strip that spans two tile rows")
    return bad


# ---- contents ---------------------------------------------------------------------------------------------------------------------
def _dtype_max(sb):
    return (np.uint8, 255) if sb == 1 else (np.uint16, 65535)


def _tile_rows(k, ty, h):
    """LDS rows of tile row ty as input rows [r_lo, r_lo + NR - 1] (r_lo = ty MR - a + 1), and their part inside the image."""
    r_lo = ty * k.MR - k.A + 1
    return r_lo, r_lo + k.NR - 1, max(r_lo, 0), min(r_lo + k.NR - 1, h - 1)


def sparse_motifs(inst, h, w, shape=None):
    """The (row, pixel) of the `1` of every motif of sparse_flips, sorted.  Two per full tile (tx, ty): in the tile's first LDS
    row at the first pixel of its first unit, and in its last LDS row at the last pixel of its last unit -- both rows are halo
    rows of the tile (clipped to the image at the top and bottom) and own rows of the tile row above / below, so every motif is
    met by two tile rows.  At tx = 0 the 1 sits at pixel 2, the first with a pixel two to its left (the second unit where
    P = 2).  The partial last tile has its motif at the last in-image column, in its first LDS row -- and in its last LDS row
    too where no tap of that 1 reaches the motif of the tile to its left (it does in the 16-bit frames, three pixels past the
    tile boundary: a max beside a 1 pushes the sum back up, and the motif would be no flip)."""
    k = fast_cfg(inst, shape)
    tiles_x = -(-w // k.TWP_IN)
    out = set()
    for ty in range(-(-h * k.S // k.TH)):
        _, _, ra, rb = _tile_rows(k, ty, h)
        for tx in range(tiles_x):
            p0 = tx * k.TWP_IN
            if p0 + k.TWP_IN <= w:
                out.add((ra, max(p0, 2)))
                out.add((rb, p0 + k.TWP_IN - 1))
            else:
                out.add((ra, w - 1))
                if tx == 0 or w - 3 > p0 - 1 + k.A:
                    out.add((rb, w - 1))
    return sorted(out)


def sparse_flips(inst, h, w, shape=None):
    """All zeros except the motifs `max at pixel x - 2, 1 at pixel x`, in every channel, at sparse_motifs().  The reference's
    double chain at the integer phase of such a 1 is (max * L(2) + 0) + 1 with L(2) ~ -1e-17 (a >= 3): one ulp below 1, stored
    as 0 -- the sample the FIXUP step exists for."""
    k = fast_cfg(inst, shape)
    dt, mx = _dtype_max(k.SB)
    img = np.zeros((h, w, k.C), dt)
    for (y, x) in sparse_motifs(inst, h, w, shape):
        assert x >= 2 and not img[y, x - 2:x + 1].any(), (inst, y, x)
        img[y, x - 2] = mx
        img[y, x] = 1
    return img


def dense_n(inst, shape=None):
    """n of dense_flips: 8, doubled until a full tile's NR x TWP_IN window holds more than WL_CAP samples equal to 1 (16 for
    8-bit one-channel 4x a = 2: 18 rows x 256 samples)."""
    k = fast_cfg(inst, shape)
    n = 8
    while k.NR * k.TWP_IN * k.C * (n - 1) // n <= k.WL_CAP + k.NR * k.C and n < 1024:
        n *= 2
    return n


def dense_flips(inst, h, w, shape=None):
    """Every sample 1, except that pixel (y, x) is max wherever (x + 3 y) % n == 0, n = dense_n().  A sample equal to 1 is queued
    under any vlim >= 1, so a tile's worklist is at least dense_count() long."""
    k = fast_cfg(inst, shape)
    dt, mx = _dtype_max(k.SB)
    img = np.ones((h, w, k.C), dt)
    yy, xx = np.mgrid[0:h, 0:w]
    img[(xx + 3 * yy) % dense_n(inst, shape) == 0] = mx
    return img


def _tiles(k, h, w):
    return [(tx, ty) for ty in range(-(-h * k.S // k.TH)) for tx in range(-(-w // k.TWP_IN))]


def sparse_bound(inst, img, shape=None):
    """{(tx, ty): upper bound of the tile's worklist length}: a unit whose WIN_PX window is all zero queues nothing (its sums
    are 0 + eps, clamped to 0.5: decided; no own sample is >= 1), every other unit at most its UNIT_OUT_S samples.  All UPR
    units of all NR rows count, those past the right edge included (the H pass runs them)."""
    k = fast_cfg(inst, shape)
    h, w, _ = img.shape
    nz = np.zeros((h, w + 2 * k.TWP_IN + 2 * k.TAPS), bool)        # pixel holds a nonzero sample; columns shifted by TAPS
    nz[:, k.TAPS:k.TAPS + w] = img.any(axis=2)
    csum = np.concatenate([np.zeros((h, 1), np.int64), np.cumsum(nz, axis=1)], axis=1)
    out = {}
    for (tx, ty) in _tiles(k, h, w):
        _, _, ra, rb = _tile_rows(k, ty, h)
        units = 0
        for u in range(k.UPR):
            x0 = tx * k.TWP_IN + u * k.P - (k.A - 1) + k.TAPS          # first window pixel (shifted)
            units += int(np.count_nonzero(csum[ra:rb + 1, x0 + k.WIN_PX] - csum[ra:rb + 1, x0]))
        out[tx, ty] = units * k.UNIT_OUT_S
    return out


def motifs_per_tile(inst, h, w, shape=None):
    """{(tx, ty): motifs of sparse_flips with a pixel in the tile's NR x (TWP_IN + 2a - 1) window}."""
    k = fast_cfg(inst, shape)
    mot = sparse_motifs(inst, h, w, shape)
    out = {}
    for (tx, ty) in _tiles(k, h, w):
        _, _, ra, rb = _tile_rows(k, ty, h)
        x_lo, x_hi = tx * k.TWP_IN - (k.A - 1), tx * k.TWP_IN + k.TWP_IN - 1 + k.A
        out[tx, ty] = sum(1 for (y, x) in mot if ra <= y <= rb and x >= x_lo and x - 2 <= x_hi)
    return out


def dense_count(inst, img, shape=None):
    """{(tx, ty): in-image samples equal to 1 among the tile's NR rows x TWP_IN own pixels}: a lower bound of its worklist
    length under any vlim >= 1."""
    k = fast_cfg(inst, shape)
    h, w, _ = img.shape
    out = {}
    for (tx, ty) in _tiles(k, h, w):
        _, _, ra, rb = _tile_rows(k, ty, h)
        out[tx, ty] = int(np.count_nonzero(img[ra:rb + 1, tx * k.TWP_IN:(tx + 1) * k.TWP_IN] == 1))
    return out


def integer_phase_flips(img, want, s):
    """[h][w][C] bool: the oracle's output at the integer phase of an input sample differs from the sample."""
    return want[::s, ::s] != img


# ---- k_generic ----------------------------------------------------------------------------------------------------------------------
def generic_frame(c, sb, sn, sd, a, ragged, tile=(256, 32)):
    """The smallest input frame whose sn/sd output spans two k_generic tiles each way (kGenTileW sample columns x kGenTileH
    rows), ragged both ways, with more than kGenTileH rows at and below K; output rows that are dword multiples (ragged =
    False: only force_kernel(KERNEL_GENERIC) reaches k_generic) or that are not (True: a plain call does).  None where no such
    width exists: C = 4, and 16-bit samples at an even scale (the row is an even number of 2-byte samples)."""
    tw, th = tile
    def fits(w):
        n = w * sn // sd * c
        return tw < n < 2 * tw and ((n * sb) % 4 != 0) == ragged
    w = next((w for w in range(8, 4 * tw) if fits(w)), None)
    if w is None:
        return None
    K = prefix_rows(sn, sd, a)
    h = next(h for h in range(8, 400) if h * sn // sd > K + th and (h * sn // sd) % th != 0 and h * sn // sd > th)
    return w, h


def generic_cuts(sn, sd, a, out_h):
    """Three strips with arbitrary cuts: [0, K + 5), [K + 5, K + 22), [K + 22, out_h)."""
    K = prefix_rows(sn, sd, a)
    return [0, K + 5, K + 22, out_h]
