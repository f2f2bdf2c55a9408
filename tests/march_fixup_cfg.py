"""Contents that steer the marching kernel's fix-up paths, and what they must reach -- TEST INFRASTRUCTURE ONLY.

k_march (csrc/lanczos_march.hpp) is exact only through two content-dependent mechanisms: the H pass's wave-private worklist
(integer-phase candidates by ballot rounds with a mid-loop flush; near-integer units written by the first NNI lanes with an
in-loop flush; the per-sample path of the 16-bit non-split instances) and, in EXACT mode, the V pass's redo mask.  Noise reaches
them once in 10^3 to 10^4 units.  This module restates MarchCfg (march_cfg), names per instance a frame of two full column strips
and a partial one and 4 MS + 2a + 3 rows (frame_shape), builds the steering contents (content) and evaluates, on the output of
tests/native/march_fixup_census.hip, which paths a content reaches with at least one BITING sample on them -- a sample whose f32
store differs from the reference's, so that losing its list entry is a wrong byte (goal_states).

Alignment.  Which two rows share an H wave is decided by the parity of a chunk's first row, which the device's workgroup table
chooses: an H goal counts as reached only if a wave of either parity reaches it (rows are identical or come in pairs an odd
distance apart).  Where a V group starts is the table's choice as well, and no content can make every start reach a redo mask
with bit 0 and the top bit (an integer-phase row is undecided only below a brighter row two away: the brightest row of a period
never is); v_mask therefore counts the group starts that reach it here, and tests/test_march_fixup_gpu.py checks on the table
the launch REPORTS that one of them ran.

MOTIFS_* were found by the tool's seeded search modes (searchh / searchv / searche / searchb / searchi / searchf, seed and tries in SEARCH);
tests/test_march_fixup_cfg.py re-runs the census on every content and pins the outcome.
"""
import collections
import os
import re

import numpy as np

import fast_cfg as F

MARCH_HEADER = os.path.join(os.path.dirname(F.HEADER), "lanczos_march.hpp")
INSTANCES = sorted(F.FAST_INSTANCES)
inst_id = F.inst_id

MarchCfg = collections.namedtuple("MarchCfg", "SB C S A TAPS P UPR NGRP MS MRG NVT NU NVT_PAD NT NWAVES RS RS_POW2 WL_ROUND WLW NNI "
                                              "UNIT_IN_DW UNIT_OUT_S VEC TWP_IN TWP_OUT SYM RNE_H SPLIT")


def header_march_shape(text=None):
    """MarchShape of the header: (default NGRP, the specialisation's (type, C, S), its NGRP, its MS)."""
    if text is None:
        with open(MARCH_HEADER) as f:
            text = f.read()
    d = re.search(r"struct MarchShape \{\s*static constexpr int NGRP = (\d+);[^\n]*\n\s*static constexpr int MS = 2 \* A \* NGRP;", text)
    s = re.search(r"struct MarchShape<(\w+), (\d+), (\d+), A> \{[^\n]*\n\s*static constexpr int NGRP = (\d+);\s*static constexpr int MS = (\d+);", text)
    assert d and s, "MarchShape not found in lanczos_march.hpp"
    return int(d.group(1)), ({"uint8_t": 1, "uint16_t": 2}[s.group(1)], int(s.group(2)), int(s.group(3))), int(s.group(4)), int(s.group(5))


_MSHAPE = None


def march_cfg(inst):
    """MarchCfg<T, C, S, A> of csrc/lanczos_march.hpp, formula by formula (the H-unit geometry is FastCfg's: fast_cfg.fast_cfg)."""
    global _MSHAPE
    _MSHAPE = _MSHAPE or header_march_shape()
    ngrp_default, special, ngrp_s, ms_s = _MSHAPE
    k = F.fast_cfg(inst)
    SB, C, S, A = inst
    NGRP, MS = (ngrp_s, ms_s) if (SB, C, S) == special else (ngrp_default, 2 * A * ngrp_default)
    NVT = k.TWB_OUT // 4
    NU = MS * k.UPR
    NVT_PAD = NVT if NGRP == 1 else -(-NVT // 64) * 64
    NT = -(-max(NVT_PAD * NGRP, NU) // 64) * 64
    RS = 32 if 2 * MS + k.TAPS - 1 <= 32 else -(-(2 * MS + k.TAPS - 1) // 8) * 8
    WL_ROUND = 64 * k.UNIT_IN_DW
    return MarchCfg(SB, C, S, A, k.TAPS, k.P, k.UPR, NGRP, MS, MS // NGRP, NVT, NU, NVT_PAD, NT, NT // 64, RS, int(RS & (RS - 1) == 0),
                    WL_ROUND, WL_ROUND + 96, k.UNIT_OUT_S - k.P * C, k.UNIT_IN_DW, k.UNIT_OUT_S, k.VEC, k.TWP_IN, k.TWP_OUT,
                    int(S == 2), int(SB == 1), int(SB == 2 and S == 2))


def frame_shape(inst):
    """(in_w, in_h): the narrowest row of a 16-byte multiple that gives two full strips and a partial one with at least two
    whole units; 4 MS + 2a + 3 rows, one more where that is a multiple of MS."""
    k = march_cfg(inst)
    w = next(w for w in range(2 * k.TWP_IN + 2 * k.P, 3 * k.TWP_IN) if (w * k.C * k.SB) % 16 == 0)
    h = 4 * k.MS + 2 * k.A + 3
    return w, h + (h % k.MS == 0)


def modes(inst):
    """The H pass is the same kernel code in both modes except for the 16-bit 2x instances (EXACT: the split-weight chain and a
    unit flag; LSB1: the single chain and per-sample flags): those are censused in both, every other instance as EXACT."""
    return (1, 0) if inst[0] == 2 and inst[2] == 2 else (1,)


# ---- motifs (tests/native/march_fixup_census.hip search modes; SEARCH = (seed, tries) of every search) ----------------------------
SEARCH = (20261019, 3000000)
# instance -> P * C samples of a period-P row with a flagged and biting computed sample (EXACT-mode H pass)
MOTIFS_H = {
    (1, 1, 2, 3): (173, 185, 74, 224, 60, 1, 161, 153),
    (1, 1, 2, 4): (2, 6, 2, 14, 15, 11, 6, 3),
    (1, 1, 3, 2): (36, 40, 20, 17, 23, 22, 55, 22),
    (1, 1, 3, 3): (4, 6, 8, 2, 0, 9, 9, 1),
    (1, 1, 3, 4): (15, 15, 15, 13, 12, 5, 6, 12),
    (1, 1, 4, 2): (12, 1, 12, 0, 4, 12, 6, 12),
    (1, 1, 4, 3): (4, 14, 9, 4, 1, 2, 15, 15),
    (1, 1, 4, 4): (14, 83, 151, 185, 95, 119, 208, 96),
    (1, 3, 2, 3): (183, 124, 217, 21, 174, 234, 209, 53, 154, 9, 230, 33),
    (1, 3, 2, 4): (199, 177, 206, 83, 91, 5, 75, 1, 72, 203, 30, 72),
    (1, 3, 3, 2): (63, 56, 61, 50, 4, 51, 21, 31, 48, 51, 17, 40),
    (1, 3, 3, 3): (8, 1, 8, 5, 10, 12, 9, 5, 3, 0, 9, 14),
    (1, 3, 3, 4): (238, 130, 79, 225, 91, 210, 67, 34, 107, 155, 60, 27),
    (1, 3, 4, 2): (14, 9, 1, 13, 9, 0, 4, 14, 6, 15, 5, 7),
    (1, 3, 4, 3): (63, 12, 0, 23, 45, 63, 60, 28, 50, 34, 26, 61),
    (1, 3, 4, 4): (175, 245, 35, 236, 152, 130, 217, 129, 36, 194, 240, 24),
    (1, 4, 2, 3): (253, 132, 187, 3, 121, 4, 119, 185, 157, 73, 229, 85, 121, 241, 67, 44),
    (1, 4, 2, 4): (91, 202, 177, 152, 81, 63, 127, 72, 38, 53, 214, 237, 166, 197, 95, 142),
    (1, 4, 3, 2): (29, 48, 63, 49, 40, 32, 27, 51, 58, 61, 48, 17, 28, 30, 47, 52),
    (1, 4, 3, 3): (1, 1, 8, 13, 3, 3, 8, 8, 15, 14, 9, 13, 4, 3, 9, 4),
    (1, 4, 3, 4): (92, 113, 209, 244, 138, 98, 44, 188, 235, 165, 169, 164, 70, 85, 156, 199),
    (1, 4, 4, 2): (97, 161, 254, 110, 5, 133, 21, 77, 211, 127, 124, 127, 173, 164, 136, 17),
    (1, 4, 4, 3): (7, 9, 13, 12, 6, 1, 14, 7, 15, 6, 1, 7, 12, 4, 5, 10),
    (1, 4, 4, 4): (135, 30, 27, 177, 193, 113, 112, 136, 252, 48, 24, 81, 18, 130, 36, 111),
    (2, 3, 2, 3): (55731, 54086, 54427, 55633, 50975, 57028),
    (2, 3, 2, 4): (46507, 27206, 7920, 23800, 47634, 54971),
    (2, 3, 3, 3): (6263, 24204, 45312, 49938, 25203, 33173),
    (2, 3, 3, 4): (6263, 24204, 45312, 49938, 25203, 33173),
    (2, 4, 2, 3): (58324, 20019, 46789, 38770, 2954, 11775, 46094, 19987),
    (2, 4, 2, 4): (2250, 12812, 14377, 15445, 221, 2441, 2476, 11332),
    (2, 4, 3, 3): (10049, 8851, 3357, 2124, 15519, 1440, 11707, 3216),
    (2, 4, 3, 4): (217, 2493, 8057, 6934, 15805, 12900, 14252, 11931),
}
# 16-bit 2x: the same for the LSB1 H pass (single chain, per-sample flags)
MOTIFS_H_LSB1 = {
    (2, 3, 2, 3): (4071, 1221, 3833, 2126, 309, 3360),
    (2, 3, 2, 4): (38098, 3248, 39763, 8008, 42369, 62638),
    (2, 4, 2, 3): (41698, 15989, 17210, 1941, 38795, 2423, 505, 38265),
    (2, 4, 2, 4): (15458, 2884, 2289, 4437, 6327, 1743, 6793, 12480),
}
# instance -> 2a grey values: rows r of value pat[r % 2a] hold an undecided and biting computed V sample behind the exact H stage
MOTIFS_V = {
    (1, 1, 2, 3): (230, 88, 241, 88, 139, 83),
    (1, 1, 2, 4): (217, 185, 210, 112, 104, 101, 90, 235),
    (1, 1, 3, 2): (111, 239, 108, 9),
    (1, 1, 3, 3): (212, 220, 253, 88, 231, 190),
    (1, 1, 3, 4): (106, 69, 230, 210, 139, 215, 102, 210),
    (1, 1, 4, 2): (180, 174, 2, 221),
    (1, 1, 4, 3): (88, 153, 147, 70, 206, 169),
    (1, 1, 4, 4): (227, 182, 223, 111, 94, 185, 66, 95),
    (1, 3, 2, 3): (230, 88, 241, 88, 139, 83),
    (1, 3, 2, 4): (217, 185, 210, 112, 104, 101, 90, 235),
    (1, 3, 3, 2): (111, 239, 108, 9),
    (1, 3, 3, 3): (212, 220, 253, 88, 231, 190),
    (1, 3, 3, 4): (106, 69, 230, 210, 139, 215, 102, 210),
    (1, 3, 4, 2): (180, 174, 2, 221),
    (1, 3, 4, 3): (88, 153, 147, 70, 206, 169),
    (1, 3, 4, 4): (227, 182, 223, 111, 94, 185, 66, 95),
    (1, 4, 2, 3): (230, 88, 241, 88, 139, 83),
    (1, 4, 2, 4): (217, 185, 210, 112, 104, 101, 90, 235),
    (1, 4, 3, 2): (111, 239, 108, 9),
    (1, 4, 3, 3): (212, 220, 253, 88, 231, 190),
    (1, 4, 3, 4): (106, 69, 230, 210, 139, 215, 102, 210),
    (1, 4, 4, 2): (180, 174, 2, 221),
    (1, 4, 4, 3): (88, 153, 147, 70, 206, 169),
    (1, 4, 4, 4): (227, 182, 223, 111, 94, 185, 66, 95),
    (2, 3, 2, 3): (46688, 47758, 33214, 16884, 17794, 56564),
    (2, 3, 2, 4): (39765, 24191, 16792, 59391, 16603, 22525, 28014, 40043),
    (2, 3, 3, 3): (43708, 55060, 63612, 23193, 57199, 45844),
    (2, 3, 3, 4): (47104, 40894, 41311, 29343, 47009, 32433, 49557, 47256),
    (2, 4, 2, 3): (46688, 47758, 33214, 16884, 17794, 56564),
    (2, 4, 2, 4): (39765, 24191, 16792, 59391, 16603, 22525, 28014, 40043),
    (2, 4, 3, 3): (43708, 55060, 63612, 23193, 57199, 45844),
    (2, 4, 3, 4): (47104, 40894, 41311, 29343, 47009, 32433, 49557, 47256),
}
# instance -> (a - 1) * C samples: the last pixels of a row under which the first unit past the right edge flags
MOTIFS_E = {
    (1, 1, 2, 3): (182, 166),
    (1, 1, 2, 4): (43, 186, 56),
    (1, 1, 3, 3): (10, 153),
    (1, 1, 3, 4): (58, 19, 3),
    (1, 1, 4, 3): (23, 32),
    (1, 1, 4, 4): (49, 10, 33),
    (1, 3, 2, 3): (131, 109, 132, 154, 131, 157),
    (1, 3, 2, 4): (79, 178, 243, 111, 135, 76, 23, 40, 93),
    (1, 3, 3, 3): (52, 2, 60, 54, 21, 0),
    (1, 3, 3, 4): (43, 40, 53, 2, 34, 1, 26, 44, 39),
    (1, 3, 4, 3): (37, 23, 134, 117, 32, 178),
    (1, 3, 4, 4): (215, 212, 236, 96, 59, 224, 231, 33, 60),
    (1, 4, 2, 3): (97, 94, 74, 182, 241, 99, 122, 166),
    (1, 4, 2, 4): (172, 176, 92, 213, 164, 39, 166, 134, 76, 118, 197, 142),
    (1, 4, 3, 3): (28, 2, 36, 55, 29, 21, 54, 44),
    (1, 4, 3, 4): (158, 134, 56, 133, 13, 0, 77, 98, 4, 63, 171, 22),
    (1, 4, 4, 3): (192, 214, 5, 157, 142, 2, 248, 43),
    (1, 4, 4, 4): (60, 32, 38, 3, 8, 26, 27, 45, 54, 62, 31, 34),
    (2, 3, 2, 3): (11790, 13651, 11415, 9913, 8799, 9335),
    (2, 3, 2, 4): (3047, 193, 1375, 391, 2621, 3763, 3421, 2308, 2390),
    (2, 3, 3, 3): (6263, 24204, 45312, 49938, 25203, 33173),
    (2, 3, 3, 4): (44805, 39142, 37651, 46277, 21592, 22655, 42290, 27368, 46710),
    (2, 4, 2, 3): (15200, 47766, 59121, 18939, 62343, 41478, 10718, 31791),
    (2, 4, 2, 4): (7490, 1620, 11998, 15692, 7373, 14525, 9899, 14197, 12606, 3103, 15414, 12578),
    (2, 4, 3, 3): (40, 3346, 1690, 978, 790, 1856, 2778, 3769),
    (2, 4, 3, 4): (22257, 50811, 61927, 49732, 59280, 13831, 38457, 42656, 58026, 39832, 42776, 32895),
}
# 16-bit instances -> a grey value whose every computed H sample is flagged (and biting) on a flat frame
# instance -> 2a pixels (every channel) around an integer-phase candidate, the centre at index a - 1, whose exact sum the last bit
# of the centre weight decides (searchi): a fix-up that processes the entry with slightly wrong arithmetic stores another value
MOTIFS_I = {
    (1, 1, 2, 3): (241, 123, 58, 68, 144, 7),
    (1, 1, 2, 4): (119, 140, 0, 62, 115, 149, 129, 46),
    (1, 1, 3, 3): (241, 123, 58, 68, 144, 7),
    (1, 1, 3, 4): (119, 140, 0, 62, 115, 149, 129, 46),
    (1, 1, 4, 3): (241, 123, 58, 68, 144, 7),
    (1, 1, 4, 4): (119, 140, 0, 62, 115, 149, 129, 46),
    (1, 3, 2, 3): (241, 123, 58, 68, 144, 7),
    (1, 3, 2, 4): (119, 140, 0, 62, 115, 149, 129, 46),
    (1, 3, 3, 3): (241, 123, 58, 68, 144, 7),
    (1, 3, 3, 4): (119, 140, 0, 62, 115, 149, 129, 46),
    (1, 3, 4, 3): (241, 123, 58, 68, 144, 7),
    (1, 3, 4, 4): (119, 140, 0, 62, 115, 149, 129, 46),
    (1, 4, 2, 3): (241, 123, 58, 68, 144, 7),
    (1, 4, 2, 4): (119, 140, 0, 62, 115, 149, 129, 46),
    (1, 4, 3, 3): (241, 123, 58, 68, 144, 7),
    (1, 4, 3, 4): (119, 140, 0, 62, 115, 149, 129, 46),
    (1, 4, 4, 3): (241, 123, 58, 68, 144, 7),
    (1, 4, 4, 4): (119, 140, 0, 62, 115, 149, 129, 46),
    (2, 3, 2, 3): (37651, 46277, 13943, 22655, 42290, 27368),
    (2, 3, 2, 4): (39832, 42776, 32895, 12288, 3912, 33494, 55183, 17162),
    (2, 3, 3, 3): (37651, 46277, 13943, 22655, 42290, 27368),
    (2, 3, 3, 4): (39832, 42776, 32895, 12288, 3912, 33494, 55183, 17162),
    (2, 4, 2, 3): (37651, 46277, 13943, 22655, 42290, 27368),
    (2, 4, 2, 4): (39832, 42776, 32895, 12288, 3912, 33494, 55183, 17162),
    (2, 4, 3, 3): (37651, 46277, 13943, 22655, 42290, 27368),
    (2, 4, 3, 4): (39832, 42776, 32895, 12288, 3912, 33494, 55183, 17162),
}
# 3x instances -> (first, last) P + a pixels of a row with a biting computed sample whose taps the frame edge cuts off (searchb,
# at frame_shape's width)
MOTIFS_B = {
    (1, 1, 3, 2): ((6, 10, 5, 10, 5, 12, 5, 4, 11, 14), (12, 4, 6, 13, 14, 9, 4, 5, 10, 6)),
    (1, 1, 3, 3): ((1, 3, 3, 11, 4, 2, 10, 3, 2, 1, 11), (6, 5, 10, 11, 13, 4, 3, 13, 4, 0, 13)),
    (1, 1, 3, 4): ((5, 10, 8, 5, 4, 6, 5, 14, 13, 1, 8, 13), (3, 3, 8, 15, 7, 0, 5, 12, 11, 7, 4, 1)),
    (1, 3, 3, 2): ((53, 6, 57, 14, 1, 57, 52, 41, 53, 20, 48, 59, 43, 3, 26, 54, 49, 42), (64, 178, 7, 250, 12, 73, 63, 72,
        65, 34, 240, 20, 211, 90, 97, 105, 246, 92)),
    (1, 3, 3, 3): ((115, 218, 74, 3, 6, 114, 240, 151, 135, 181, 58, 248, 206, 57, 92, 22, 227, 27, 61, 113, 234), (242, 178,
        160, 142, 143, 105, 147, 86, 107, 159, 29, 100, 6, 209, 105, 47, 46, 83, 236, 162, 114)),
    (1, 3, 3, 4): ((43, 42, 6, 60, 18, 12, 21, 12, 34, 43, 8, 18, 23, 35, 39, 59, 56, 40, 49, 59, 12, 32, 10, 43), (15, 13, 3,
        13, 10, 0, 14, 2, 2, 8, 6, 15, 2, 11, 7, 10, 7, 6, 13, 3, 13, 2, 7, 7)),
    (1, 4, 3, 2): ((8, 6, 7, 2, 9, 10, 5, 7, 6, 5, 0, 2, 10, 8, 15, 8, 4, 8, 9, 9, 2, 0, 6, 13), (9, 0, 8, 9, 5, 2, 0, 14, 15,
        2, 15, 8, 0, 6, 0, 5, 7, 6, 13, 10, 14, 0, 3, 6)),
    (1, 4, 3, 3): ((36, 35, 55, 4, 47, 12, 5, 61, 47, 44, 18, 60, 39, 44, 61, 11, 9, 41, 34, 21, 40, 62, 56, 61, 39, 29, 50,
        25), (8, 8, 15, 0, 0, 1, 7, 14, 4, 0, 5, 13, 14, 8, 4, 7, 0, 7, 4, 13, 6, 2, 0, 1, 6, 8, 13, 13)),
    (1, 4, 3, 4): ((14, 6, 55, 21, 11, 42, 10, 39, 28, 38, 43, 30, 0, 55, 59, 34, 63, 30, 8, 37, 53, 30, 22, 37, 11, 11, 35,
        19, 58, 11, 13, 43), (116, 192, 221, 254, 160, 195, 186, 148, 60, 166, 44, 231, 2, 189, 196, 87, 183, 217, 148, 23,
        119, 254, 163, 219, 120, 48, 67, 35, 12, 74, 138, 122)),
    (2, 3, 3, 3): ((7740, 22688, 54324, 24012, 60406, 58220, 12449, 5648, 32990, 33498, 59172, 64430, 56373, 36524, 13048),
        (10343, 12349, 14164, 3107, 13279, 8997, 4441, 13278, 1766, 1404, 6998, 15534, 1125, 14921, 14457)),
    (2, 3, 3, 4): ((22257, 50811, 61927, 49732, 59280, 13831, 38457, 42656, 58026, 39832, 42776, 32895, 46916, 3912, 33494,
        55183, 17162, 28671), (62959, 58136, 8896, 6967, 16191, 13398, 21984, 18010, 56778, 25142, 7933, 24563, 153, 19142,
        11624, 10343, 61501, 63316)),
    (2, 4, 3, 3): ((40, 3346, 1690, 978, 790, 1856, 2778, 3769, 3372, 3561, 1219, 3396, 2331, 2658, 3845, 2278, 787, 1221,
        1112, 2175), (3568, 349, 979, 1037, 2294, 1363, 568, 1778, 51, 3380, 921, 2633, 2233, 79, 1946, 3546, 1435, 2651,
        2589, 422)),
    (2, 4, 3, 4): ((22257, 50811, 61927, 49732, 59280, 13831, 38457, 42656, 58026, 39832, 42776, 32895, 46916, 3912, 33494,
        55183, 17162, 28671, 6263, 24204, 45312, 49938, 25203, 33173), (1404, 6998, 15534, 1125, 14921, 14457, 10866, 10215,
        554, 10227, 3441, 12264, 7424, 656, 5737, 4673, 3053, 2398, 10762, 170, 12023, 10856, 13568, 5447)),
}
MOTIFS_F = {
    (2, 3, 2, 3): 1,
    (2, 3, 2, 4): 406,
    (2, 3, 3, 3): 1,
    (2, 3, 3, 4): 526,
    (2, 4, 2, 3): 1,
    (2, 4, 2, 4): 406,
    (2, 4, 3, 3): 1,
    (2, 4, 3, 4): 526,
}

CONTENTS = ("int_h", "int_v", "int_lone", "near_h", "near_v", "near_one", "near_edge", "near_rim", "int_ulp", "mixed", "mixed_v", "near_col", "near_flat")


def _dt(inst):
    return (np.uint8, 255) if inst[0] == 1 else (np.uint16, 65535)


def _tile_h(inst, motif, w):
    k = march_cfg(inst)
    row = np.array(motif, dtype=np.int64).reshape(k.P, k.C)
    return np.tile(row, (-(-w // k.P), 1))[:w]


def one_positions(inst, w=None):
    """near_one: (row, first pixel) of the three lone units -- unit 0 of strip 1, unit 17 of strip 0, the last in-image unit --
    each on two rows three apart (one of either wave parity), the bands MS rows apart."""
    k = march_cfg(inst)
    w = w or frame_shape(inst)[0]
    xs = (k.TWP_IN, 17 * k.P, (w - 1) // k.P * k.P)
    return [(k.A + 2 + b * k.MS + d, x) for b, x in enumerate(xs) for d in (0, 3)]


def content(inst, name, lsb1=False, width=None):
    """The frame [h][w][C] of an instance and content (at another width: the same construction), or None where the content needs
    a motif the search did not find."""
    k = march_cfg(inst)
    w, h = frame_shape(inst)
    w = width or w
    dt, mx = _dt(inst)
    mh = (MOTIFS_H_LSB1 if lsb1 and inst in MOTIFS_H_LSB1 else MOTIFS_H).get(inst)
    img = np.zeros((h, w, k.C), np.int64)
    # 1, 1, max, max, 1, 1: every 1 next to the max pair is a tight candidate (a brighter sample two away).  (The period-4 row
    # 1, 1, max, max does not leave 1 at a = 3 -- the census finds no biting entry away from the frame edges -- and puts exactly
    # WLW - WL_ROUND entries, one short of a flush, into a round of the 16-bit RGB instances.)
    ipat = np.array([1, 1, mx, mx, 1, 1])
    n = len(ipat)
    if name == "int_h":       # identical rows
        img[:] = ipat[np.arange(w) % n][None, :, None]
    elif name == "int_v":     # the transpose
        img[:] = ipat[np.arange(h) % n][:, None, None]
    elif name == "int_lone":
        # isolated `max at x -+ 2, 1 at x`: columns 0 and 1 and w - 2 and w - 1 (a +-2 neighbour outside the image), two in the
        # interior; on rows three apart.  And one pixel column of 1, 1, max, max downwards in the partial last strip, channel 0
        for r in range(1, h - 1, 3):
            for x, nb in ((0, 2), (1, 3), (w - 1, w - 3), (w - 2, w - 4), (k.TWP_IN + 9, k.TWP_IN + 7), (k.TWP_IN - 1, k.TWP_IN + 1)):
                if (r // 3) % 3 == (x + nb) % 3:
                    img[r, x], img[r, nb] = 1, mx
        img[:, 2 * k.TWP_IN + k.P, 0] = ipat[np.arange(h) % n]
    elif name == "near_h":
        if mh is None:
            return None
        img[:] = _tile_h(inst, mh, w)[None]
    elif name == "near_v":
        if inst not in MOTIFS_V:
            return None
        img[:] = np.array(MOTIFS_V[inst])[np.arange(h) % k.TAPS][:, None, None]
    elif name == "near_one":
        if mh is None:
            return None
        t = _tile_h(inst, mh, w + 4 * k.P)
        for r, x in one_positions(inst, w):
            lo, hi = max(x - (k.A - 1), 0), min(x + k.P + k.A, w)      # the unit's whole window
            img[r, lo:hi] = t[lo:hi]
    elif name == "near_edge":
        if inst not in MOTIFS_E:
            return None
        e = np.array(MOTIFS_E[inst]).reshape(k.A - 1, k.C)
        img[:, w - (k.A - 1):] = e[None]
    elif name == "mixed":     # int_h and near_h in the same rows, 16 units each in turn: both kinds in every wave
        if mh is None:
            return None
        near = (np.arange(w) // (16 * k.P)) % 2 == 1
        img[:] = np.where(near[:, None], _tile_h(inst, mh, w), ipat[np.arange(w) % n][:, None])[None]
    elif name == "mixed_v":
        # even pixel columns: the int_v column, odd ones: the near_v column, each shifted down by x // 2 rows -- a V wave spans at
        # least 16 input pixels, so every row is an undecided integer-phase row in some lane and an undecided computed row in another
        if inst not in MOTIFS_V:
            return None
        yy, xx = np.mgrid[0:h, 0:w]
        cv = np.array(MOTIFS_V[inst])
        img[:] = np.where(xx % 2 == 1, cv[(yy + xx // 2) % k.TAPS], ipat[(yy + xx // 2) % n])[:, :, None]
    elif name == "near_col":  # one pixel column of the near_v motif, channel 0, in the partial last strip
        if inst not in MOTIFS_V:
            return None
        img[:, 2 * k.TWP_IN + k.P, 0] = np.array(MOTIFS_V[inst])[np.arange(h) % k.TAPS]
    elif name == "int_ulp":   # the searchi window, alone on black, in the first, a middle and the last unit of a row; rows three apart
        if inst not in MOTIFS_I:
            return None
        for r in range(2, h - 1, 3):
            for x in (k.A - 1, k.TWP_IN + 5 * k.P + 1, w - k.A - 1):
                img[r, x - (k.A - 1):x + k.A + 1] = np.array(MOTIFS_I[inst])[:, None]
    elif name == "near_rim":  # black rows but for their first and last P + a pixels: computed samples whose taps the frame edge cuts off
        if inst not in MOTIFS_B:
            return None
        left, right = (np.array(m).reshape(k.P + k.A, k.C) for m in MOTIFS_B[inst])
        img[:, :k.P + k.A] = left[None]
        img[:, w - (k.P + k.A):] = right[None]
    elif name == "near_flat":
        if inst not in MOTIFS_F:
            return None
        img[:] = MOTIFS_F[inst]
    else:
        raise ValueError(name)
    return np.ascontiguousarray(img.astype(dt))


# ---- the census -----------------------------------------------------------------------------------------------------------------------
Census = collections.namedtuple("Census", "const H V summary ok")


def parse_census(text, returncode=0):
    const, H, V, summary = {}, [], [], {}
    for line in text.split("\n"):
        t = line.split()
        if not t:
            continue
        if t[0] == "CONST":
            const.update({t[i]: float(t[i + 1]) if "." in t[i + 1] or "e" in t[i + 1] else int(t[i + 1]) for i in range(1, len(t), 2)})
        elif t[0] == "H":
            H.append([int(t[1]), int(t[2]), int(t[3]), int(t[4], 16), int(t[5], 16)] + [int(x) for x in t[6:]])
        elif t[0] == "V":
            V.append([int(x) for x in t[1:]])
        elif t[0] == "SUM":
            summary = {t[i]: int(t[i + 1]) for i in range(1, len(t), 2)}
    return Census(const, np.array(H, dtype=np.int64).reshape(-1, 14), np.array(V, dtype=np.int64).reshape(-1, 7), summary,
                  returncode == 0 and "census: ok" in text)


# columns of Census.H / Census.V
H_R, H_TX, H_U, H_IM, H_BIM, H_NEAR, H_NINT, H_NNEAR, H_BINT, H_BNEAR, H_PAST, H_XLO, H_XHI, H_ULP = range(14)
V_Y, V_TX, V_WAVE, V_KIND, V_LANES, V_BITE, V_DOWN = range(7)

H_GOALS = ("int_final", "int_mid", "near_one", "near_loop", "per_sample", "int_and_near", "past_edge", "edge_bites", "int_ulp")
V_GOALS = ("v_int", "v_comp", "v_mask", "v_one_lane")
GOALS = H_GOALS + V_GOALS


def _popcount(x):
    return bin(int(x)).count("1")


def wave_events(k, units, per_sample):
    """What one H wave does with its units (rows of Census.H in lane order): the set of goals it reaches.  Follows hpass's list
    code: integer rounds e = 0 .. VEC - 1 with a flush when cnt > WLW - WL_ROUND, then the near path."""
    got = set()
    mask = (1 << k.UNIT_IN_DW) - 1
    cnt = flushes = 0
    bite_before = bite_after = entries_after = 0
    any_int = any(u[H_IM] for u in units)
    for e in range(k.VEC):
        n = sum(_popcount((u[H_IM] >> (8 * k.SB * e)) & mask) for u in units)
        b = sum(_popcount((u[H_BIM] >> (8 * k.SB * e)) & mask) for u in units)
        if flushes:
            entries_after += n
            bite_after += b
        else:
            bite_before += b
        cnt += n
        if cnt > k.WLW - k.WL_ROUND and e < k.VEC - 1:
            flushes, cnt = flushes + 1, 0
    if any_int and not flushes and bite_before:
        got.add("int_final")
    if flushes and entries_after and bite_before and bite_after:
        got.add("int_mid")
    near = [u for u in units if u[H_NEAR]]
    if near:
        if per_sample:
            # a round adds at most 64 entries and the list is flushed at cnt > WLW - 64: more than WLW entries are a flush inside
            # the loop and entries behind it
            if sum(u[H_NNEAR] for u in near) > k.WLW and near[0][H_BNEAR] and near[-1][H_BNEAR]:
                got.add("per_sample")
        else:
            if len(near) == 1 and near[0][H_BNEAR]:
                got.add("near_one")
            first_flush = -(-(k.WLW - k.NNI + 1) // k.NNI)
            if len(near) > first_flush and near[0][H_BNEAR] and near[-1][H_BNEAR]:
                got.add("near_loop")
        if any_int and any(u[H_BINT] for u in units) and any(u[H_BNEAR] for u in near):
            got.add("int_and_near")
    if any(u[H_PAST] for u in units):
        got.add("past_edge")
    return got


def h_goal_parities(inst, cen):
    """goal -> set of wave parities (first row of the pair mod 2) at which some wave reaches it."""
    k = march_cfg(inst)
    per_sample = bool(cen.const["NEAR_PER_SAMPLE"])
    by_row = collections.defaultdict(list)
    for u in cen.H:
        by_row[(int(u[H_R]), int(u[H_TX]))].append(u)
    out = collections.defaultdict(set)
    rows = sorted({r for r, _ in by_row})
    for r0 in sorted({r for r in rows} | {r - 1 for r in rows}):
        for tx in sorted({t for _, t in by_row}):
            units = sorted(by_row.get((r0, tx), []), key=lambda u: u[H_U]) + sorted(by_row.get((r0 + 1, tx), []), key=lambda u: u[H_U])
            if units:
                for g in wave_events(k, units, per_sample):
                    out[g].add(r0 % 2)
    return out


def v_redo_rows(cen):
    """(tx, wave) -> {output row y: (kind, lanes, bite, down)} of the rows the EXACT V pass redoes."""
    out = collections.defaultdict(dict)
    for v in cen.V:
        out[(int(v[V_TX]), int(v[V_WAVE]))][int(v[V_Y])] = (int(v[V_KIND]), int(v[V_LANES]), int(v[V_BITE]), int(v[V_DOWN]))
    return out


def mask_starts(inst, cen, m_lo, m_hi):
    """The V group starts m_g (whole group inside [m_lo, m_hi)) at which some wave's redo mask holds bit 0 and the top bit
    MRG S - 1, both biting; and how many starts there are."""
    k = march_cfg(inst)
    redo = v_redo_rows(cen)
    good = set()
    for m_g in range(m_lo, m_hi - k.MRG + 1):
        y0, y1 = m_g * k.S, (m_g + k.MRG) * k.S - 1
        if any(y0 in rows and y1 in rows and rows[y0][2] and rows[y1][2] for rows in redo.values()):
            good.add(m_g)
    return good, max(m_hi - k.MRG + 1 - m_lo, 0)


def edge_bite_rows(inst, cen):
    """(row parities with a biting computed entry at an output pixel x with floor(x / S) < a - 1, the same for floor(x / S) >
    in_w - 1 - a): the samples whose taps the frame edge cuts off -- where phase_exact_h == 0 flush() takes their weights from the
    per-index table, whose out-of-range taps are zero, not from the phase weights."""
    k = march_cfg(inst)
    w = frame_shape(inst)[0]
    bit = cen.H[cen.H[:, H_BNEAR] > 0]
    left = {int(u[H_R]) % 2 for u in bit if u[H_XLO] // k.S < k.A - 1}
    right = {int(u[H_R]) % 2 for u in bit if u[H_XHI] // k.S > w - 1 - k.A}
    return left, right


def goal_states(inst, censuses, m_lo, m_hi):
    """censuses: {(content, exact): Census}.  goal -> the contents that reach it (H goals: at both wave parities)."""
    k = march_cfg(inst)
    strips = -(-frame_shape(inst)[0] // k.TWP_IN)
    out = {g: [] for g in GOALS}
    for (name, exact), cen in sorted(censuses.items()):
        tag = name if exact else name + ":lsb1"
        for g, par in h_goal_parities(inst, cen).items():
            if par == {0, 1}:
                out[g].append(tag)
        if {int(u[H_R]) % 2 for u in cen.H if u[H_ULP]} == {0, 1}:
            out["int_ulp"].append(tag)
        if not cen.const["phase_exact_h"] and edge_bite_rows(inst, cen) == ({0, 1}, {0, 1}):
            out["edge_bites"].append(tag)
        if not exact:
            continue
        if any(v[V_KIND] == 0 and v[V_BITE] for v in cen.V):
            out["v_int"].append(tag)
        if any(v[V_KIND] == 1 and v[V_BITE] for v in cen.V):
            out["v_comp"].append(tag)
        if mask_starts(inst, cen, m_lo, m_hi)[0]:
            out["v_mask"].append(tag)
        if any(v[V_TX] == strips - 1 and v[V_LANES] == 1 and v[V_BITE] for v in cen.V):
            out["v_one_lane"].append(tag)
    return out


INT_GOALS = ("int_final", "int_mid", "int_and_near", "int_ulp", "v_int", "v_mask")   # need an integer-phase candidate: vlim >= 1


def unreachable_reason(inst, goal, consts):
    """Why no content can reach a goal, or None.  consts: the census constants of every mode of modes(inst).  Each reason names
    its proof, which tests/test_march_fixup_cfg.py carries out: "enumeration" (the tool's enum22 mode), "vlim == 0", "not
    compiled" and "phase_exact_h == 1" (the census's constants), "searched" (the tool's searche mode, SEARCH tries, found nothing)."""
    if inst[0] == 1 and inst[2] == 2 and inst[3] == 2:
        return "enumeration: none of the 511^2 pair sums of the paired 2-tap chain flags, and vlim == 0"
    if goal in INT_GOALS and all(c["vlim"] == 0 for c in consts):
        return "vlim == 0"
    if goal == "per_sample" and not any(c["NEAR_PER_SAMPLE"] for c in consts):
        return "not compiled: no mode of this instance flags per sample"
    if goal in ("near_one", "near_loop") and all(c["NEAR_PER_SAMPLE"] for c in consts):
        return "not compiled: every mode of this instance flags per sample"
    if goal == "edge_bites" and all(c["phase_exact_h"] for c in consts):
        return "phase_exact_h == 1: the exact chain never reads the per-index table"
    if goal == "past_edge" and inst not in MOTIFS_E:
        return "searched: %d tries, seed %d: no past-edge unit flags" % (SEARCH[1], SEARCH[0])
    return None


def v_variant(const):
    """The arithmetic of an instance's computed rows in the EXACT V pass, by the census's constants."""
    if const["SPLIT"]:
        return "split"
    if const["MIXV"]:
        return "mixv"
    if const["RNE_H"]:
        return "paired" if const["SYM"] else "plain"
    return "fmed3"


# ---- the reported table -------------------------------------------------------------------------------------------------------------
def table_groups(inst, seg, y_lo, y_hi):
    """The V groups of one table segment (m_b, m_e) as (m_g, interior): march_body's vpass."""
    k = march_cfg(inst)
    m_b, m_e = seg
    ticks = -(-(m_e - m_b + k.TAPS - 1) // k.MS)
    out = []
    for t in range(ticks):
        for g in range(k.NGRP):
            m_g = m_b - (k.TAPS - 1) + t * k.MS + g * k.MRG
            if m_g + k.MRG <= m_b or m_g >= m_e:
                continue
            out.append((m_g, m_g >= m_b and m_g + k.MRG <= m_e and m_g * k.S >= y_lo and (m_g + k.MRG) * k.S <= y_hi))
    return out


def table_coverage(inst, cen, segments, y_lo, y_hi):
    """What the redo rows of a census met under a reported table: segments = [(strip, m_b, m_e)] of ONE frame.  Returns counts:
    biting redo rows stored from an interior group and from a CHECKED (chunk-edge) group; groups whose mask holds bit 0 and the
    top bit, both biting; and integer-phase redo rows DROPPED by the redo loop: the row m_b - 1 just above a chunk, which the
    chunk's first group (rows m_b - 2a + 1 .. m_b) tests like any other and which is not the chunk's to store.  Of that row's
    window the ring holds every row from m_b - a + 1 down: at a = 4 all three rows of the test (m - 2, m, m + 2) are real, at
    a = 3 the row m - 2 is not, so only lanes that are undecided through the row two below alone (`down`) count there."""
    k = march_cfg(inst)
    redo = v_redo_rows(cen)
    n = {"interior": 0, "checked": 0, "discarded": 0, "mask": 0}
    for (tx, m_b, m_e) in segments:
        waves = [rows for (t, _), rows in redo.items() if t == tx]
        for m_g, interior in table_groups(inst, (m_b, m_e), y_lo, y_hi):
            for rows in waves:
                ys = [y for y in rows if m_g <= y // k.S < m_g + k.MRG and rows[y][2]]
                stored = [y for y in ys if m_b <= y // k.S < m_e and y_lo <= y < y_hi]
                n["interior" if interior else "checked"] += len(stored)
                y = (m_b - 1) * k.S
                if m_g < m_b and y in rows and rows[y][0] == 0 and (k.A >= 4 or (k.A == 3 and rows[y][3] > 0)):
                    n["discarded"] += 1
                if m_g * k.S in ys and (m_g + k.MRG) * k.S - 1 in ys and m_g >= m_b and m_g + k.MRG <= m_e:
                    n["mask"] += 1
    return n


def tile_width(inst):
    """The frame one pixel group wider: the narrowest width past frame_shape's whose input rows are no 16-byte multiples while
    the output rows stay dword multiples -- the tile kernel k_fast takes it."""
    k = march_cfg(inst)
    w0 = frame_shape(inst)[0]
    return next(w for w in range(w0 + 1, w0 + 64) if (w * k.C * k.SB) % 16 != 0 and (w * k.S * k.C * k.SB) % 4 == 0)


def out_samples(inst):
    w, h = frame_shape(inst)
    return w * h * inst[1] * inst[2] ** 2
