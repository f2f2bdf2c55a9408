"""The workgroup-table shapes of the marching kernel k_march and the batches that reach them -- TEST INFRASTRUCTURE ONLY.

What a k_march workgroup computes is decided by a host-built table (csrc/lanczos_march.hpp: march_build_table) with three
shapes; GOALS names them as predicates over the table a launch reports (Context.last_march_table()).  INSTANCES are the four
kernel instances the table tests run, CANDIDATES the batches (in_w, in_h, frames) that reach each goal: which one does depends
on the resident workgroups per CU (nb) and the CU count, which only the device knows, so every (instance, goal) has a short
list.  tests/test_march_table_cfg.py proves without a GPU (on the host-built table, 256 CUs, nb 1..4) that the list serves every
nb; tests/test_march_table_gpu.py takes the first candidate that serves the device.

Everything about the table is restated here from the library's sources, not read from them: strips(), rows(), single_launch()
(the split rule of lanczos_upscale_route.cpp: up_route), partition_errors() and the goal predicates.
"""
import collections

import numpy as np

MODE_A, MODE_B = 1, 2   # lanczos_march_table_info.mode

# name -> (bytes per sample, channels, scale, a)
INSTANCES = {
    "u8-c3-2x-a3": (1, 3, 2, 3),    # config 2: two V groups, 12 input rows per tick
    "u8-c3-3x-a3": (1, 3, 3, 3),    # config 3: the one-V-group specialisation
    "u16-c4-2x-a4": (2, 4, 2, 4),   # config 5: 16 rows per tick, the 40-row ring with the modulo slot
    "u8-c1-4x-a2": (1, 1, 4, 2),
}
GOALS = ("equal", "rank-aware", "per-slot")

Info = collections.namedtuple("Info", "workgroups segs mode rank_aware strips frames m_lo m_hi wg_per_cu cus")


def strip_in_px(inst):
    """Input pixels per column strip: MarchCfg::F::TWP_IN = P * 32 (csrc/lanczos_fast.hpp: FastCfg)."""
    bps, c, s, a = inst
    return (2 if bps == 2 else (8 if c == 1 else 4)) * 32


def ms_taps(inst):
    """MS (input rows per tick) and TAPS of MarchCfg / MarchShape."""
    bps, c, s, a = inst
    ngrp = 1 if (bps, c, s) == (1, 3, 3) else 2
    return (12 if ngrp == 1 else 2 * a * ngrp), 2 * a


def strips(inst, in_w):
    return -(-in_w // strip_in_px(inst))


def prefix_rows(s, a):
    """K of an integer scale on a frame tall enough that no tap is clipped: output rows [0, K) read a row below themselves."""
    return max(o + 1 for o in range(4 * a * s + 8) if o // s + a > o)


def rows(inst, in_h, out_row0=0, out_rows=0):
    """[m_lo, m_hi) of a launch (march_issue_t): the input rows m = y // s of the output rows k_march stores, which start behind
    the in-place prefix rows [0, K)."""
    bps, c, s, a = inst
    y_lo = max(out_row0, prefix_rows(s, a) if out_row0 < prefix_rows(s, a) else 0)
    y_hi = out_row0 + out_rows if out_rows else in_h * s
    return y_lo // s, (y_hi - 1) // s + 1


def preferred_frames(nb, cus, n_strips):
    pf = nb * cus // (2 * n_strips)
    while pf > 0 and (2 * n_strips * pf) % 16 != 0:
        pf -= 1
    return pf


def single_launch(nb, cus, n_strips, frames):
    """up_route's split rule (csrc/lanczos_upscale_route.cpp): a batch of twice the preferred size pf goes out as launches of pf frames, one of one
    and a half times pf already where four workgroups are resident per CU; batches are split only where pf >= 8."""
    pf = preferred_frames(nb, cus, n_strips)
    return not (pf >= 8 and (frames >= 2 * pf or (nb >= 4 and frames >= pf + pf // 2)))


def in_width_ok(inst, in_w):
    """march_supports: input rows are 16-byte multiples; at least two strips, the last one ragged."""
    bps, c, s, a = inst
    return (in_w * c * bps) % 16 == 0 and in_w > strip_in_px(inst) and in_w % strip_in_px(inst) != 0


# (instance, goal) -> [(in_w, in_h, frames), ...], tried in this order.  Found by a search over the host-built table (256 CUs,
# nb 1..4).  Input rows are 16-byte multiples (march_supports), two or three strips with a ragged last one, frame counts that are
# no multiples of five.  Per-slot (mode A) needs pairs * ticks_pair >= 10 * slots in ONE launch: these are the smallest batches
# the conditions leave.
CANDIDATES = {
    # three chunks of three ticks and a last chunk of 5 to 8 rows (less than one tick with its window), at every nb: 7 frames
    # of three strips are far fewer workgroups than slots, and the XCDs do not all get whole pairs, so the shares stay equal
    ("u8-c3-2x-a3", "equal"): [(272, 70, 7), (144, 100, 7)],
    ("u8-c3-3x-a3", "equal"): [(272, 70, 7), (144, 100, 7)],
    ("u16-c4-2x-a4", "equal"): [(130, 90, 7), (66, 100, 7)],
    ("u8-c1-4x-a2", "equal"): [(528, 50, 7), (272, 70, 7)],
    # pairs a multiple of 8 (every XCD gets whole pairs), three chunks per pair cut by slot speed: heights like 31 / 19 / 28; then a
    # two-chunk batch.  Unreachable where every slot speed is 1 (rank_aware_reachable)
    ("u8-c3-2x-a3", "rank-aware"): [(272, 80, 8), (144, 50, 12)],
    ("u8-c3-3x-a3", "rank-aware"): [(272, 70, 8), (144, 70, 12), (144, 40, 12)],
    ("u16-c4-2x-a4", "rank-aware"): [(130, 100, 8), (66, 60, 12)],
    ("u8-c1-4x-a2", "rank-aware"): [(528, 50, 8), (272, 40, 12)],
    # one entry per nb, smallest first (nb 1, 2, 3, 4): two strips, 60 to 130 MB of input and output together at nb 2 to 4
    ("u8-c3-2x-a3", "per-slot"): [(144, 160, 92), (144, 120, 233), (144, 120, 351), (144, 160, 366)],
    ("u8-c3-3x-a3", "per-slot"): [(144, 160, 92), (144, 120, 233), (144, 120, 351), (144, 160, 366)],
    ("u16-c4-2x-a4", "per-slot"): [(66, 160, 124), (66, 160, 233), (66, 160, 351), (66, 240, 321)],
    ("u8-c1-4x-a2", "per-slot"): [(272, 80, 124), (272, 80, 233), (272, 80, 351), (272, 120, 321)],
}


def threads(inst):
    """MarchCfg::NT: the V pass wants one thread per output dword column and V group, the H pass one per unit of a tick."""
    bps, c, s, a = inst
    ms, _ = ms_taps(inst)
    ngrp = 1 if (bps, c, s) == (1, 3, 3) else 2
    nvt = strip_in_px(inst) * s * c * bps // 4
    nvt_pad = nvt if ngrp == 1 else -(-nvt // 64) * 64
    return -(-max(nvt_pad * ngrp, ms * 32) // 64) * 64


def rank_aware_reachable(inst, nb):
    """march_slot_speed: the slots of a CU differ in speed only with three or four resident workgroups, or with two whose wave
    count is no multiple of four; everywhere else every speed is 1 and march_build_table never weighs the shares."""
    return nb in (3, 4) or (nb == 2 and (threads(inst) // 64) % 4 != 0)


def segments(tab):
    """The non-empty segments of a table [workgroups][segs][4] as rows (workgroup, frame, strip, m_b, m_e)."""
    tab = np.asarray(tab).reshape(len(tab), -1, 4)
    wg = np.repeat(np.arange(tab.shape[0]), tab.shape[1])
    flat = tab.reshape(-1, 4)
    keep = flat[:, 2] < flat[:, 3]
    return np.column_stack([wg[keep], flat[keep]])


def partition_errors(info, tab):
    """[] if every entry is in range and every (frame, strip, row of [m_lo, m_hi)) lies in exactly one non-empty segment."""
    tab = np.asarray(tab)
    if tab.shape != (info.workgroups, info.segs, 4):
        return [f"table shape {tab.shape} for {info.workgroups} workgroups x {info.segs} segments"]
    if not (info.workgroups > 0 and info.segs > 0 and info.m_lo < info.m_hi):
        return [f"empty table: {info}"]
    sg = segments(tab)
    bad = ((sg[:, 1] < 0) | (sg[:, 1] >= info.frames) | (sg[:, 2] < 0) | (sg[:, 2] >= info.strips) | (sg[:, 3] < info.m_lo) |
           (sg[:, 4] > info.m_hi))
    if bad.any():
        return [f"entry out of range: workgroup {r[0]}: frame {r[1]} strip {r[2]} rows [{r[3]}, {r[4]})" for r in sg[bad][:4]]
    m_rows = info.m_hi - info.m_lo
    cover = np.zeros(info.frames * info.strips * m_rows + 1, np.int64)
    base = (sg[:, 1] * info.strips + sg[:, 2]) * m_rows - info.m_lo
    np.add.at(cover, base + sg[:, 3], 1)
    np.add.at(cover, base + sg[:, 4], -1)
    cover = np.cumsum(cover)[:-1]
    wrong = np.nonzero(cover != 1)[0]
    out = []
    for i in wrong[:4]:
        pair, m = divmod(int(i), m_rows)
        out.append(f"frame {pair // info.strips} strip {pair % info.strips} row {m + info.m_lo} lies in {cover[i]} segments")
    return out


def summary(info, tab):
    """The figures the goals and the reports are about."""
    sg = segments(tab)
    per_wg = np.bincount(sg[:, 0], minlength=info.workgroups)
    nxt = (sg[1:, 0] == sg[:-1, 0])                      # consecutive non-empty segments of one workgroup
    frame_changes = int((nxt & (sg[1:, 1] != sg[:-1, 1])).sum())
    strip_changes = int((nxt & (sg[1:, 1] == sg[:-1, 1]) & (sg[1:, 2] != sg[:-1, 2])).sum())
    heights = {}
    for r in sg[np.lexsort((sg[:, 3], sg[:, 2], sg[:, 1]))]:
        heights.setdefault((int(r[1]), int(r[2])), []).append(int(r[4] - r[3]))
    return {
        "two_segment_wgs": int((per_wg == 2).sum()), "three_segment_wgs": int((per_wg >= 3).sum()), "idle_wgs": int((per_wg == 0).sum()),
        "frame_changes": frame_changes, "strip_changes": strip_changes, "shortest_segment": int((sg[:, 4] - sg[:, 3]).min()),
        "longest_segment": int((sg[:, 4] - sg[:, 3]).max()), "pair_heights": heights,
    }


def meets(goal, info, tab):
    """The goal's predicate over a reported table."""
    s = summary(info, tab)
    hs = list(s["pair_heights"].values())
    if goal == "equal":    # mode B, equal chunks, at least 3 per pair, the last one shorter than the others
        return info.mode == MODE_B and not info.rank_aware and info.segs == 1 and \
            all(len(h) >= 3 and len(set(h[:-1])) == 1 and h[-1] < h[0] for h in hs)
    if goal == "rank-aware":   # mode B, shares by slot speed: two different chunk heights within one pair
        return info.mode == MODE_B and bool(info.rank_aware) and info.segs == 1 and any(len(set(h)) >= 2 for h in hs)
    if goal == "per-slot":     # mode A: a share that runs into the next frame, and one that runs into the next strip of its frame
        return info.mode == MODE_A and s["frame_changes"] >= 1 and s["strip_changes"] >= 1
    raise ValueError(goal)


def describe(info, tab):
    s = summary(info, tab)
    return (f"mode {'-AB'[info.mode]} {'rank-aware' if info.rank_aware else 'equal'}, {info.workgroups} workgroups x {info.segs} segment(s), "
            f"{info.strips} strips x {info.frames} frames, rows [{info.m_lo}, {info.m_hi}), nb {info.wg_per_cu}, {info.cus} CUs: "
            f"{s['two_segment_wgs']} two-segment and {s['three_segment_wgs']} three-segment workgroups, {s['frame_changes']} frame changes, "
            f"{s['strip_changes']} strip changes, segments of {s['shortest_segment']}..{s['longest_segment']} rows")
