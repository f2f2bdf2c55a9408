"""tests/march_table_cfg.py kept honest without a GPU: march_build_table (host code of csrc/lanczos_march.hpp, compiled here with
hipcc) builds the table of every candidate batch for 256 CUs and 1 to 4 resident workgroups per CU, and the goal predicates and
the partition check of march_table_cfg -- the ones tests/test_march_table_gpu.py applies to the table a device reports -- run
on it.  For every nb at least one candidate of every (instance, goal) must go out as one launch and meet its goal; where the
builder cannot make rank-aware shares at all (every slot speed is 1) that is asserted instead."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import march_table_cfg as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS, NBS = 256, (1, 2, 3, 4)

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


def host_tables(exe, batches, env=None):
    """batches: [(instance, in_w, in_h, frames, nb, cus)] -> [(Info, table [workgroups][segs][4], (MS, TAPS, NWAVES, TWP_OUT))]"""
    path = exe + ".in"
    with open(path, "w") as f:
        for inst, w, h, frames, nb, cus in batches:
            f.write("%d %d %d %d %d %d %d %d %d %d\n" % (*inst, w, *M.rows(inst, h), frames, nb, cus))
    base = {k: v for k, v in os.environ.items() if not k.startswith("LANCZOS_")}
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300, env=dict(base, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert lines[2 * len(batches)] == "done %d" % len(batches), lines[-3:]
    out = []
    for i in range(len(batches)):
        t = [int(x) for x in lines[2 * i].split()[1:]]
        assert lines[2 * i].startswith("TAB ") and t[0] == i and lines[2 * i + 1].startswith("ENT ")
        info = M.Info(workgroups=t[3], segs=t[4], mode=t[1], rank_aware=t[2], strips=t[5], frames=t[6], m_lo=t[7], m_hi=t[8],
                      wg_per_cu=t[9], cus=t[10])
        tab = np.array(lines[2 * i + 1].split()[1:], dtype=np.int32).reshape(info.workgroups, info.segs, 4)
        out.append((info, tab, tuple(t[11:15])))
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    path = str(tmp_path_factory.mktemp("march_table_cfg") / "march_table_cfg_check")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "lanczos-hls_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "march_table_cfg_check.hip"), "-o", path], check=True, timeout=600)
    return path


@pytest.fixture(scope="module")
def tables(exe):
    """(instance name, goal) -> nb -> [(candidate, Info, table)] in the candidates' order"""
    keys = [(name, goal, cand, nb) for (name, goal), cands in M.CANDIDATES.items() for cand in cands for nb in NBS]
    res = host_tables(exe, [(M.INSTANCES[name], *cand, nb, CUS) for (name, goal, cand, nb) in keys])
    out = {}
    for (name, goal, cand, nb), (info, tab, consts) in zip(keys, res):
        inst = M.INSTANCES[name]
        # the restated constants are MarchCfg's own
        assert consts == (*M.ms_taps(inst), M.threads(inst) // 64, M.strip_in_px(inst) * inst[2]), (name, consts)
        assert (info.strips, info.frames) == (M.strips(inst, cand[0]), cand[2])
        out.setdefault((name, goal), {}).setdefault(nb, []).append((cand, info, tab))
    return out


def test_every_instance_and_goal_has_candidates():
    assert set(M.CANDIDATES) == {(name, goal) for name in M.INSTANCES for goal in M.GOALS}
    for (name, goal), cands in M.CANDIDATES.items():
        inst = M.INSTANCES[name]
        assert cands, (name, goal)
        for (w, h, frames) in cands:
            assert M.in_width_ok(inst, w), (name, goal, w)
            assert frames % 5 != 0 and frames > 5, (name, goal, frames)   # five base frames cycled: every one recurs, out of step
            assert h >= 4 * inst[3] + 4, (name, goal, h)                   # tall enough that no prefix tap is clipped


@pytest.mark.parametrize("goal", M.GOALS)
@pytest.mark.parametrize("name", list(M.INSTANCES))
def test_a_candidate_reaches_the_goal_at_every_nb(tables, name, goal):
    inst = M.INSTANCES[name]
    for nb in NBS:
        serving = []
        for cand, info, tab in tables[(name, goal)][nb]:
            errs = M.partition_errors(info, tab)
            assert not errs, f"{name} {cand} nb {nb}: {errs}"
            if M.single_launch(nb, CUS, info.strips, info.frames) and M.meets(goal, info, tab):
                serving.append(cand)
        print(f"{name} {goal} nb {nb}: {serving}")
        if goal == "rank-aware" and not M.rank_aware_reachable(inst, nb):
            assert not any(info.rank_aware for _, info, _ in tables[(name, goal)][nb]), f"{name} nb {nb}: rank-aware shares after all"
            continue
        assert serving, f"{name} {goal}: no candidate of {M.CANDIDATES[(name, goal)]} is one launch that meets the goal at nb {nb}: " + \
            "; ".join(f"{c}: {M.describe(i, t)}" for c, i, t in tables[(name, goal)][nb])


def test_per_slot_candidates_reach_the_shortest_segment(tables):
    """Mode A's cuts leave no segment under min_seg = 3 MS - (2a - 1) rows, and the candidates have segments of exactly that."""
    for name, inst in M.INSTANCES.items():
        ms, taps = M.ms_taps(inst)
        for nb in NBS:
            got = [M.summary(i, t)["shortest_segment"] for c, i, t in tables[(name, "per-slot")][nb] if i.mode == M.MODE_A]
            assert got and min(got) == 3 * ms - (taps - 1), (name, nb, got)


def test_the_checks_notice_a_broken_table(tables):
    cand, info, tab = next(x for x in tables[("u8-c3-2x-a3", "per-slot")][4] if x[1].mode == M.MODE_A)
    assert M.meets("per-slot", info, tab) and not M.meets("equal", info, tab) and not M.meets("rank-aware", info, tab)
    two = np.nonzero((tab[:, :, 2] < tab[:, :, 3]).sum(1) == 2)[0][0]
    for seg, col, delta, word in ((1, 3, -1, "0 segments"), (0, 2, -1, "2 segments"), (0, 3, +1, "out of range"), (1, 0, +1, "0 segments"),
                                  (1, 1, info.strips, "out of range")):
        t = tab.copy()
        t[two, seg, col] += delta
        errs = M.partition_errors(info, t)
        assert errs and any(word in e for e in errs), (seg, col, delta, errs)
    t = tab.copy()
    t[two, 1, 2] = t[two, 1, 3]   # the second segment of a share dropped
    assert M.partition_errors(info, t)
    cand, info, tab = tables[("u8-c3-2x-a3", "equal")][4][0]
    assert M.meets("equal", info, tab) and not M.meets("per-slot", info, tab) and not M.meets("rank-aware", info, tab)
    assert not M.meets("equal", info._replace(rank_aware=1), tab) and not M.meets("equal", info._replace(mode=M.MODE_A), tab)
    cand, info, tab = tables[("u8-c3-2x-a3", "rank-aware")][4][0]
    assert M.meets("rank-aware", info, tab) and not M.meets("equal", info, tab)


def test_split_rule_restated():
    """config 2 at 1080p (15 strips, four per CU, 256 CUs): 32 frames preferred, split from 48; config 3 at 720p (10 strips, two per
    CU): 24 preferred, split from 48 (tests/test_upscale_routes_gpu.py: 73 = 32 + 32 + 9, 81 = 3 x 24 + 9)."""
    assert M.preferred_frames(4, 256, 15) == 32 and M.single_launch(4, 256, 15, 47) and not M.single_launch(4, 256, 15, 48)
    assert M.preferred_frames(2, 256, 10) == 24 and M.single_launch(2, 256, 10, 47) and not M.single_launch(2, 256, 10, 48)
    assert M.single_launch(1, 256, 60, 100)   # fewer than eight frames preferred: never split
