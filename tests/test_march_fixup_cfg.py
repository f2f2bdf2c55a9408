"""tests/march_fixup_cfg.py kept honest without a GPU, and its outcome pinned.

tests/native/march_fixup_census.hip (host code only: hipcc compiles it without a GPU) emulates, with the library's own tap tables
and FastConsts and MarchCfg's own constexprs, which samples of a frame k_march cannot decide in f32 and which of them BITE (the
f32 store differs from the reference's double chain, so a lost worklist entry or a lost redo row is a wrong sample).  It fails on
any sample that the kernel would not flag and that differs all the same: the proven bound on these contents, and the emulation.

For all 35 instances every (instance, goal) pair of march_fixup_cfg.GOALS is either REACHED on a committed content, with a
biting sample on that path (H goals: in a wave of either row parity), or proven UNREACHABLE -- by the enumeration of the 8-bit 2x
a = 2 chain, by vlim == 0, by phase_exact_h == 1, by a variant the instance does not compile, or by a seeded search of stated size that found nothing.
There is no third state.  EXPECT pins the outcome per instance: (arithmetic of the computed rows in the EXACT V pass, (V group
starts whose redo mask holds bit 0 and the top bit on mixed_v, group starts there are), goal -> the contents that reach it or the
reason none can).  A change to MarchCfg, to fast_prepare or to a content shows as a diff of this table.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fast_cfg as F
import march_fixup_cfg as M
import march_table_cfg as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

ENUM = "unreachable: enumeration: none of the 511^2 pair sums of the paired 2-tap chain flags, and vlim == 0"
VLIM0 = "unreachable: vlim == 0"
NO_PS = "unreachable: not compiled: no mode of this instance flags per sample"
ALL_PS = "unreachable: not compiled: every mode of this instance flags per sample"
PHASE_EXACT = "unreachable: phase_exact_h == 1: the exact chain never reads the per-index table"
SEARCHED = "unreachable: searched: %d tries, seed %d: no past-edge unit flags" % (M.SEARCH[1], M.SEARCH[0])

EXPECT = {
    "u8-c1-2x-a2": ("paired", (0, 0), {
        "int_final": ENUM, "int_mid": ENUM, "near_one": ENUM, "near_loop": ENUM, "per_sample": ENUM, "int_and_near": ENUM,
        "past_edge": ENUM, "edge_bites": ENUM, "int_ulp": ENUM, "v_int": ENUM, "v_comp": ENUM, "v_mask": ENUM, "v_one_lane":
        ENUM
    }),
    "u8-c1-2x-a3": ("mixv", (46, 50), {
        "int_final": "int_h,int_lone,mixed,mixed_v", "int_mid": "int_h,mixed", "near_one": "near_one", "near_loop":
        "mixed,near_h", "per_sample": NO_PS, "int_and_near": "mixed", "past_edge": "near_edge", "edge_bites": PHASE_EXACT,
        "int_ulp": "int_ulp", "v_int": "int_lone,int_v,mixed_v", "v_comp": "mixed_v,near_col,near_v", "v_mask": "mixed_v",
        "v_one_lane": "int_lone,mixed_v,near_col"
    }),
    "u8-c1-2x-a4": ("mixv", (60, 65), {
        "int_final": "int_h,int_lone,mixed,mixed_v", "int_mid": "int_h,mixed", "near_one": "near_one", "near_loop":
        "mixed,near_h", "per_sample": NO_PS, "int_and_near": "mixed", "past_edge": "near_edge", "edge_bites": PHASE_EXACT,
        "int_ulp": "int_ulp,mixed,near_h,near_one", "v_int": "int_lone,int_v,mixed_v,near_col", "v_comp":
        "mixed_v,near_col,near_v", "v_mask": "mixed_v", "v_one_lane": "int_lone,mixed_v,near_col"
    }),
    "u8-c1-3x-a2": ("plain", (0, 36), {
        "int_final": VLIM0, "int_mid": VLIM0, "near_one": "near_one,near_rim", "near_loop": "mixed,near_h", "per_sample":
        NO_PS, "int_and_near": VLIM0, "past_edge": SEARCHED, "edge_bites": "near_rim", "int_ulp": VLIM0, "v_int": VLIM0,
        "v_comp": "mixed_v,near_col,near_v", "v_mask": VLIM0, "v_one_lane": "near_col"
    }),
    "u8-c1-3x-a3": ("plain", (47, 51), {
        "int_final": "int_h,int_lone,mixed,near_h,near_one,near_rim", "int_mid": "int_h,mixed", "near_one":
        "near_h,near_one,near_rim", "near_loop": "mixed,near_h", "per_sample": NO_PS, "int_and_near":
        "mixed,near_h,near_one,near_rim", "past_edge": "near_edge", "edge_bites": "near_rim", "int_ulp":
        "int_ulp,mixed,near_h,near_one,near_rim", "v_int": "int_lone,int_v,mixed_v", "v_comp": "mixed_v,near_col,near_v",
        "v_mask": "mixed_v", "v_one_lane": "int_lone,mixed_v,near_col"
    }),
    "u8-c1-3x-a4": ("plain", (62, 67), {
        "int_final": "int_h,int_lone,mixed,mixed_v,near_edge", "int_mid": "int_h,mixed", "near_one": "near_one,near_rim",
        "near_loop": "mixed,near_h", "per_sample": NO_PS, "int_and_near": "mixed", "past_edge": "near_edge", "edge_bites":
        "near_rim", "int_ulp": "int_ulp,mixed,near_h,near_one,near_rim", "v_int": "int_lone,int_v,mixed_v,near_col", "v_comp":
        "mixed_v,near_col,near_v", "v_mask": "mixed_v", "v_one_lane": "int_lone,mixed_v,near_col"
    }),
    "u8-c1-4x-a2": ("plain", (0, 36), {
        "int_final": VLIM0, "int_mid": VLIM0, "near_one": "near_one", "near_loop": "mixed,near_h", "per_sample": NO_PS,
        "int_and_near": VLIM0, "past_edge": SEARCHED, "edge_bites": PHASE_EXACT, "int_ulp": VLIM0, "v_int": VLIM0, "v_comp":
        "mixed_v,near_col,near_v", "v_mask": VLIM0, "v_one_lane": "near_col"
    }),
    "u8-c1-4x-a3": ("plain", (48, 52), {
        "int_final": "int_h,int_lone,mixed,near_h,near_one", "int_mid": "int_h,mixed", "near_one": "near_h,near_one",
        "near_loop": "mixed,near_h", "per_sample": NO_PS, "int_and_near": "mixed,near_h,near_one", "past_edge": "near_edge",
        "edge_bites": PHASE_EXACT, "int_ulp": "int_ulp,mixed,near_h,near_one", "v_int": "int_lone,int_v,mixed_v", "v_comp":
        "mixed_v,near_col,near_v", "v_mask": "mixed_v", "v_one_lane": "int_lone,mixed_v,near_col"
    }),
    "u8-c1-4x-a4": ("plain", (62, 67), {
        "int_final": "int_h,int_lone,mixed,mixed_v", "int_mid": "int_h,mixed", "near_one": "near_one", "near_loop":
        "mixed,near_h", "per_sample": NO_PS, "int_and_near": "mixed", "past_edge": "near_edge", "edge_bites": PHASE_EXACT,
        "int_ulp": "int_ulp", "v_int": "int_lone,int_v,mixed_v,near_col,near_v", "v_comp": "mixed_v,near_col,near_v",
        "v_mask": "mixed_v", "v_one_lane": "int_lone,mixed_v,near_col"
    }),
    "u8-c3-2x-a2": ("paired", (0, 0), {
        "int_final": ENUM, "int_mid": ENUM, "near_one": ENUM, "near_loop": ENUM, "per_sample": ENUM, "int_and_near": ENUM,
        "past_edge": ENUM, "edge_bites": ENUM, "int_ulp": ENUM, "v_int": ENUM, "v_comp": ENUM, "v_mask": ENUM, "v_one_lane":
        ENUM
    }),
    "u8-c3-2x-a3": ("mixv", (46, 50), {
        "int_final": "int_h,int_lone,mixed", "int_mid": "int_h,mixed", "near_one": "near_one", "near_loop": "mixed,near_h",
        "per_sample": NO_PS, "int_and_near": "mixed", "past_edge": "near_edge", "edge_bites": PHASE_EXACT, "int_ulp":
        "int_ulp,mixed,near_h,near_one", "v_int": "int_lone,int_v,mixed_v", "v_comp": "mixed_v,near_col,near_v", "v_mask":
        "mixed_v", "v_one_lane": "int_lone,near_col"
    }),
    "u8-c3-2x-a4": ("mixv", (60, 65), {
        "int_final": "int_h,int_lone,mixed,near_h,near_one", "int_mid": "int_h,mixed", "near_one": "near_one", "near_loop":
        "mixed,near_h", "per_sample": NO_PS, "int_and_near": "mixed,near_h,near_one", "past_edge": "near_edge", "edge_bites":
        PHASE_EXACT, "int_ulp": "int_ulp,mixed,near_edge,near_h,near_one", "v_int": "int_lone,int_v,mixed_v,near_col",
        "v_comp": "mixed_v,near_col,near_v", "v_mask": "mixed_v", "v_one_lane": "int_lone,near_col"
    }),
    "u8-c3-3x-a2": ("plain", (0, 44), {
        "int_final": VLIM0, "int_mid": VLIM0, "near_one": "near_one,near_rim", "near_loop": "mixed,near_h", "per_sample":
        NO_PS, "int_and_near": VLIM0, "past_edge": SEARCHED, "edge_bites": "near_rim", "int_ulp": VLIM0, "v_int": VLIM0,
        "v_comp": "mixed_v,near_col,near_v", "v_mask": VLIM0, "v_one_lane": "near_col"
    }),
    "u8-c3-3x-a3": ("plain", (41, 45), {
        "int_final": "int_h,int_lone,mixed", "int_mid": "int_h,mixed", "near_one": "near_one,near_rim", "near_loop":
        "mixed,near_h", "per_sample": NO_PS, "int_and_near": "mixed", "past_edge": "near_edge", "edge_bites": "near_rim",
        "int_ulp": "int_ulp,near_rim", "v_int": "int_lone,int_v,mixed_v", "v_comp": "mixed_v,near_col,near_v", "v_mask":
        "mixed_v", "v_one_lane": "int_lone,mixed_v,near_col"
    }),
    "u8-c3-3x-a4": ("plain", (42, 47), {
        "int_final": "int_h,int_lone,mixed,near_rim", "int_mid": "int_h,mixed", "near_one": "near_one,near_rim", "near_loop":
        "mixed,near_h", "per_sample": NO_PS, "int_and_near": "mixed,near_rim", "past_edge": "near_edge", "edge_bites":
        "near_rim", "int_ulp": "int_ulp,mixed,near_h,near_one,near_rim", "v_int": "int_lone,int_v,mixed_v,near_col", "v_comp":
        "mixed_v,near_col,near_v", "v_mask": "mixed_v,near_col", "v_one_lane": "int_lone,mixed_v,near_col"
    }),
    "u8-c3-4x-a2": ("plain", (0, 36), {
        "int_final": VLIM0, "int_mid": VLIM0, "near_one": "near_one", "near_loop": "mixed,near_h", "per_sample": NO_PS,
        "int_and_near": VLIM0, "past_edge": SEARCHED, "edge_bites": PHASE_EXACT, "int_ulp": VLIM0, "v_int": VLIM0, "v_comp":
        "mixed_v,near_col,near_v", "v_mask": VLIM0, "v_one_lane": "near_col"
    }),
    "u8-c3-4x-a3": ("plain", (48, 52), {
        "int_final": "int_h,int_lone,mixed", "int_mid": "int_h,mixed", "near_one": "near_one", "near_loop": "mixed,near_h",
        "per_sample": NO_PS, "int_and_near": "mixed", "past_edge": "near_edge", "edge_bites": PHASE_EXACT, "int_ulp":
        "int_ulp,mixed", "v_int": "int_lone,int_v,mixed_v", "v_comp": "mixed_v,near_col,near_v", "v_mask": "mixed_v",
        "v_one_lane": "int_lone,mixed_v,near_col"
    }),
    "u8-c3-4x-a4": ("plain", (62, 67), {
        "int_final": "int_h,int_lone,mixed,near_h,near_one", "int_mid": "int_h,mixed", "near_one": "near_one", "near_loop":
        "mixed,near_h", "per_sample": NO_PS, "int_and_near": "mixed,near_h,near_one", "past_edge": "near_edge", "edge_bites":
        PHASE_EXACT, "int_ulp": "int_ulp,mixed,near_edge,near_h,near_one", "v_int": "int_lone,int_v,mixed_v,near_col,near_v",
        "v_comp": "mixed_v,near_col,near_v", "v_mask": "mixed_v", "v_one_lane": "int_lone,mixed_v,near_col"
    }),
    "u8-c4-2x-a2": ("paired", (0, 0), {
        "int_final": ENUM, "int_mid": ENUM, "near_one": ENUM, "near_loop": ENUM, "per_sample": ENUM, "int_and_near": ENUM,
        "past_edge": ENUM, "edge_bites": ENUM, "int_ulp": ENUM, "v_int": ENUM, "v_comp": ENUM, "v_mask": ENUM, "v_one_lane":
        ENUM
    }),
    "u8-c4-2x-a3": ("paired", (46, 50), {
        "int_final": "int_h,int_lone,mixed,near_h,near_one", "int_mid": "int_h,mixed,mixed_v", "near_one": "near_one",
        "near_loop": "mixed,near_h", "per_sample": NO_PS, "int_and_near": "mixed,near_h,near_one", "past_edge": "near_edge",
        "edge_bites": PHASE_EXACT, "int_ulp": "int_ulp,mixed,near_h,near_one", "v_int": "int_lone,int_v,mixed_v", "v_comp":
        "mixed_v,near_col,near_v", "v_mask": "mixed_v", "v_one_lane": "int_lone,mixed_v,near_col"
    }),
    "u8-c4-2x-a4": ("paired", (60, 65), {
        "int_final": "int_h,int_lone,mixed,near_h,near_one", "int_mid": "int_h,mixed,mixed_v", "near_one": "near_h,near_one",
        "near_loop": "mixed,near_h", "per_sample": NO_PS, "int_and_near": "mixed,near_h,near_one", "past_edge": "near_edge",
        "edge_bites": PHASE_EXACT, "int_ulp": "int_ulp,mixed,near_h,near_one", "v_int": "int_lone,int_v,mixed_v,near_col",
        "v_comp": "mixed_v,near_col,near_v", "v_mask": "mixed_v", "v_one_lane": "int_lone,mixed_v,near_col"
    }),
    "u8-c4-3x-a2": ("plain", (0, 36), {
        "int_final": VLIM0, "int_mid": VLIM0, "near_one": "near_h,near_one,near_rim", "near_loop": "mixed,near_h",
        "per_sample": NO_PS, "int_and_near": VLIM0, "past_edge": SEARCHED, "edge_bites": "near_rim", "int_ulp": VLIM0,
        "v_int": VLIM0, "v_comp": "mixed_v,near_col,near_v", "v_mask": VLIM0, "v_one_lane": "mixed_v,near_col"
    }),
    "u8-c4-3x-a3": ("plain", (47, 51), {
        "int_final": "int_h,int_lone,mixed,near_h,near_one", "int_mid": "int_h,mixed", "near_one": "near_h,near_one,near_rim",
        "near_loop": "mixed,near_h", "per_sample": NO_PS, "int_and_near": "mixed,near_h,near_one", "past_edge": "near_edge",
        "edge_bites": "near_rim", "int_ulp": "int_ulp,mixed,near_rim", "v_int": "int_lone,int_v,mixed_v", "v_comp":
        "mixed_v,near_col,near_v", "v_mask": "mixed_v", "v_one_lane": "int_lone,mixed_v,near_col"
    }),
    "u8-c4-3x-a4": ("plain", (62, 67), {
        "int_final": "int_h,int_lone,mixed,near_edge,near_rim", "int_mid": "int_h,mixed,mixed_v", "near_one":
        "near_h,near_one,near_rim", "near_loop": "mixed,near_h", "per_sample": NO_PS, "int_and_near": "mixed,near_rim",
        "past_edge": "near_edge", "edge_bites": "near_rim", "int_ulp": "int_ulp,mixed,near_edge,near_one,near_rim", "v_int":
        "int_lone,int_v,mixed_v,near_col", "v_comp": "mixed_v,near_col,near_v", "v_mask": "mixed_v", "v_one_lane":
        "int_lone,mixed_v,near_col"
    }),
    "u8-c4-4x-a2": ("plain", (0, 36), {
        "int_final": VLIM0, "int_mid": VLIM0, "near_one": "near_one", "near_loop": "mixed,near_h", "per_sample": NO_PS,
        "int_and_near": VLIM0, "past_edge": SEARCHED, "edge_bites": PHASE_EXACT, "int_ulp": VLIM0, "v_int": VLIM0, "v_comp":
        "mixed_v,near_col,near_v", "v_mask": VLIM0, "v_one_lane": "mixed_v,near_col"
    }),
    "u8-c4-4x-a3": ("plain", (48, 52), {
        "int_final": "int_h,int_lone,mixed", "int_mid": "int_h,mixed", "near_one": "near_h,near_one", "near_loop":
        "mixed,near_h", "per_sample": NO_PS, "int_and_near": "mixed", "past_edge": "near_edge", "edge_bites": PHASE_EXACT,
        "int_ulp": "int_ulp,mixed,near_h,near_one", "v_int": "int_lone,int_v,mixed_v", "v_comp": "mixed_v,near_col,near_v",
        "v_mask": "mixed_v", "v_one_lane": "int_lone,mixed_v,near_col"
    }),
    "u8-c4-4x-a4": ("plain", (62, 67), {
        "int_final": "int_h,int_lone,mixed", "int_mid": "int_h,mixed,mixed_v", "near_one": "near_h,near_one", "near_loop":
        "mixed,near_h", "per_sample": NO_PS, "int_and_near": "mixed", "past_edge": "near_edge", "edge_bites": PHASE_EXACT,
        "int_ulp": "int_ulp,mixed,near_h,near_one", "v_int": "int_lone,int_v,mixed_v,near_col,near_v", "v_comp":
        "mixed_v,near_col,near_v", "v_mask": "mixed_v", "v_one_lane": "int_lone,mixed_v,near_col"
    }),
    "u16-c3-2x-a3": ("split", (46, 50), {
        "int_final": "int_h:lsb1,int_h,int_lone:lsb1,int_lone,mixed:lsb1,mixed", "int_mid": "int_h:lsb1,int_h", "near_one":
        "near_one", "near_loop": "near_h", "per_sample": "int_v:lsb1,near_flat:lsb1", "int_and_near": "mixed:lsb1,mixed",
        "past_edge": "near_edge:lsb1,near_edge", "edge_bites": PHASE_EXACT, "int_ulp": "int_ulp:lsb1,int_ulp", "v_int":
        "int_lone,int_v,mixed_v", "v_comp": "mixed_v,near_col,near_v", "v_mask": "mixed_v", "v_one_lane": "int_lone,near_col"
    }),
    "u16-c3-2x-a4": ("split", (60, 65), {
        "int_final": "int_h:lsb1,int_h,int_lone:lsb1,int_lone,mixed:lsb1,mixed,mixed_v:lsb1,mixed_v", "int_mid":
        "int_h:lsb1,int_h", "near_one": "near_one", "near_loop": "near_h", "per_sample": "near_flat:lsb1", "int_and_near":
        "mixed:lsb1,mixed,mixed_v:lsb1", "past_edge": "near_edge:lsb1,near_edge,near_v:lsb1", "edge_bites": PHASE_EXACT,
        "int_ulp": "int_ulp:lsb1,int_ulp", "v_int": "int_lone,int_v,mixed_v,near_col", "v_comp": "mixed_v,near_col,near_v",
        "v_mask": "mixed_v,near_col", "v_one_lane": "int_lone,near_col"
    }),
    "u16-c3-3x-a3": ("fmed3", (47, 51), {
        "int_final": "int_h,int_lone,mixed", "int_mid": "int_h", "near_one": ALL_PS, "near_loop": ALL_PS, "per_sample":
        "int_v,near_flat", "int_and_near": "mixed", "past_edge": "mixed_v,near_edge,near_h,near_one,near_v", "edge_bites":
        "near_rim", "int_ulp": "int_ulp,near_rim", "v_int": "int_lone,int_v,mixed_v", "v_comp":
        "int_h,int_lone,mixed,mixed_v,near_col,near_edge,near_flat,near_h,near_one,near_rim,near_v", "v_mask":
        "int_lone,mixed_v", "v_one_lane": "int_lone,mixed,near_col,near_edge,near_rim"
    }),
    "u16-c3-3x-a4": ("fmed3", (66, 67), {
        "int_final": "int_h,int_lone,mixed,mixed_v,near_rim", "int_mid": "int_h", "near_one": ALL_PS, "near_loop": ALL_PS,
        "per_sample": "near_flat", "int_and_near": "int_lone,mixed,mixed_v,near_rim", "past_edge": "mixed_v,near_edge,near_v",
        "edge_bites": "int_lone,int_v,near_rim", "int_ulp": "int_ulp,near_rim", "v_int": "int_lone,int_v,mixed_v", "v_comp":
        "int_h,int_lone,int_ulp,mixed,mixed_v,near_col,near_edge,near_flat,near_h,near_one,near_rim,near_v", "v_mask":
        "int_lone,mixed_v", "v_one_lane": "int_lone,near_col,near_edge,near_h,near_rim"
    }),
    "u16-c4-2x-a3": ("split", (46, 50), {
        "int_final": "int_h:lsb1,int_h,int_lone:lsb1,int_lone,mixed:lsb1,mixed", "int_mid": "int_h:lsb1,int_h", "near_one":
        "near_h,near_one", "near_loop": "near_h", "per_sample": "int_v:lsb1,near_flat:lsb1", "int_and_near":
        "mixed:lsb1,mixed", "past_edge": "near_edge:lsb1,near_edge", "edge_bites": PHASE_EXACT, "int_ulp":
        "int_ulp:lsb1,int_ulp,mixed", "v_int": "int_lone,int_v,mixed_v", "v_comp": "mixed,mixed_v,near_col,near_v", "v_mask":
        "mixed_v", "v_one_lane": "int_lone,near_col"
    }),
    "u16-c4-2x-a4": ("split", (60, 65), {
        "int_final": "int_h:lsb1,int_h,int_lone:lsb1,int_lone,mixed:lsb1,mixed,mixed_v:lsb1,mixed_v", "int_mid":
        "int_h:lsb1,int_h", "near_one": "near_one", "near_loop": "near_h", "per_sample": "near_flat:lsb1", "int_and_near":
        "mixed:lsb1,mixed,mixed_v:lsb1", "past_edge": "near_col:lsb1,near_col,near_edge:lsb1,near_edge,near_v:lsb1",
        "edge_bites": PHASE_EXACT, "int_ulp": "int_ulp:lsb1,int_ulp,mixed:lsb1,mixed", "v_int":
        "int_lone,int_v,mixed_v,near_col", "v_comp": "mixed_v,near_col,near_v", "v_mask": "mixed_v,near_col", "v_one_lane":
        "int_lone,near_col"
    }),
    "u16-c4-3x-a3": ("fmed3", (47, 51), {
        "int_final": "int_h,int_lone,mixed,near_rim", "int_mid": "int_h", "near_one": ALL_PS, "near_loop": ALL_PS,
        "per_sample": "int_v,near_flat", "int_and_near": "mixed,near_rim", "past_edge": "mixed_v,near_col,near_edge,near_v",
        "edge_bites": "near_rim", "int_ulp": "int_ulp,mixed,near_rim", "v_int": "int_lone,int_v,mixed_v", "v_comp":
        "int_h,int_lone,mixed,mixed_v,near_col,near_edge,near_flat,near_h,near_one,near_rim,near_v", "v_mask":
        "int_lone,mixed_v", "v_one_lane": "int_lone,mixed,near_col,near_edge,near_h,near_one,near_rim"
    }),
    "u16-c4-3x-a4": ("fmed3", (66, 67), {
        "int_final": "int_h,int_lone,mixed,mixed_v,near_rim", "int_mid": "int_h", "near_one": ALL_PS, "near_loop": ALL_PS,
        "per_sample": "near_flat", "int_and_near": "int_lone,mixed,mixed_v,near_rim", "past_edge":
        "mixed_v,near_col,near_edge,near_v", "edge_bites": "int_lone,int_v,near_h,near_rim", "int_ulp":
        "int_ulp,mixed,near_rim", "v_int": "int_lone,int_v,mixed_v", "v_comp":
        "int_h,int_lone,int_ulp,mixed,mixed_v,near_col,near_edge,near_flat,near_h,near_one,near_rim,near_v", "v_mask":
        "mixed_v", "v_one_lane": "int_lone,mixed,near_col,near_edge,near_h"
    }),
}


def build_census(directory):
    """Compile tests/native/march_fixup_census.hip (with lanczos_taps.cpp, no GPU code) into `directory`; returns the program."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "lanczos-hls_amd", "csrc")
    exe = os.path.join(str(directory), "march_fixup_census")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function",
                    "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "native", "march_fixup_census.hip"),
                    os.path.join(csrc, "lanczos_taps.cpp"), "-o", exe], check=True, timeout=900)
    return exe


def run_census(exe, inst, img, exact, directory):
    """The census of one frame: the parsed output, the tool's verdict included."""
    path = os.path.join(str(directory), "frame.raw")
    np.ascontiguousarray(img).tofile(path)
    h, w, _ = img.shape
    r = subprocess.run([exe, "census", *(str(v) for v in inst), str(int(exact)), str(w), str(h), path], capture_output=True, text=True, timeout=120)
    return M.parse_census(r.stdout, r.returncode), r.stdout[-1500:] + r.stderr[-500:]


def _tool(exe, *args):
    r = subprocess.run([exe, *(str(a) for a in args)], capture_output=True, text=True, timeout=300)
    return r.returncode, r.stdout


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_census(tmp_path_factory.mktemp("march_fixup_census"))


_CENSUS = {}


def _censuses(exe, inst, tmp):
    """{(content, exact): Census} of an instance's frame under every content it has, computed once."""
    if inst not in _CENSUS:
        out = {}
        for name in M.CONTENTS:
            for exact in M.modes(inst):
                img = M.content(inst, name, lsb1=not exact)
                if img is None:
                    continue
                cen, tail = run_census(exe, inst, img, exact, tmp)
                assert cen.ok, f"{M.inst_id(inst)} {name} exact {exact}: a sample the kernel would not flag differs from the double chain\n{tail}"
                out[(name, exact)] = cen
        _CENSUS[inst] = out
    return _CENSUS[inst]


def test_instances_and_table():
    assert M.INSTANCES == sorted(F.header_instances()) and len(M.INSTANCES) == 35
    assert set(EXPECT) == {M.inst_id(i) for i in M.INSTANCES}
    for v in EXPECT.values():
        assert set(v[2]) == set(M.GOALS)


def test_frames():
    """Two full column strips and a partial one that holds whole units, rows that are 16-byte multiples (march_supports), about
    4 MS + 2a + 3 rows and no multiple of MS; the tile-kernel twin one pixel group wider.  OVER_CAP: with that geometry the
    output of these instances holds more than fast_cfg.MAX_OUT_SAMPLES_BIG samples (three strips of 8-bit RGBA at 4x are 4 160
    samples a row); the geometry is what the goals need, so it is kept and the frames that exceed the figure are pinned, and so
    is the largest of them: 8-bit RGBA 4x a = 4, 264 x 75 -> 1 056 x 300 x 4 = 1 267 200 samples."""
    over = []
    for inst in M.INSTANCES:
        k = M.march_cfg(inst)
        w, h = M.frame_shape(inst)
        assert (w * k.C * k.SB) % 16 == 0 and 2 * k.TWP_IN + 2 * k.P <= w < 3 * k.TWP_IN and w % k.P == 0, (inst, w)
        assert h % k.MS != 0 and 4 * k.MS + 2 * k.A + 3 <= h <= 4 * k.MS + 2 * k.A + 4, (inst, h)
        wt = M.tile_width(inst)
        assert (wt * k.C * k.SB) % 16 != 0 and (wt * k.S * k.C * k.SB) % 4 == 0 and w < wt <= w + 4 * k.P
        if M.out_samples(inst) > F.MAX_OUT_SAMPLES_BIG:
            over.append(M.inst_id(inst))
    assert over == OVER_CAP, over
    assert max((M.out_samples(i), M.inst_id(i)) for i in M.INSTANCES) == (1267200, "u8-c4-4x-a4")


OVER_CAP = ["u8-c1-3x-a4", "u8-c1-4x-a2", "u8-c1-4x-a3", "u8-c1-4x-a4", "u8-c3-3x-a2", "u8-c3-3x-a3", "u8-c3-3x-a4", "u8-c3-4x-a2",
            "u8-c3-4x-a3", "u8-c3-4x-a4", "u8-c4-2x-a4", "u8-c4-3x-a2", "u8-c4-3x-a3", "u8-c4-3x-a4", "u8-c4-4x-a2", "u8-c4-4x-a3",
            "u8-c4-4x-a4", "u16-c4-3x-a4"]


@pytest.mark.parametrize("inst", M.INSTANCES, ids=[M.inst_id(i) for i in M.INSTANCES])
def test_constants_are_the_headers(exe, inst, tmp_path):
    """The tool prints MarchCfg's and FastCfg's own constexprs; march_cfg() restates them from the header's MarchShape."""
    k = M.march_cfg(inst)
    for exact in M.modes(inst):
        c = _censuses(exe, inst, tmp_path)[("int_h", exact)].const
        for name in ("MS", "MRG", "NGRP", "UPR", "P", "NU", "NWAVES", "WLW", "WL_ROUND", "NNI", "UNIT_IN_DW", "UNIT_OUT_S", "VEC", "TWP_OUT",
                     "RS", "RS_POW2", "SYM", "RNE_H", "NVT", "NVT_PAD", "TAPS"):
            assert c[name] == getattr(k, name), (inst, name, c[name], getattr(k, name))
        assert c["SPLIT"] == (k.SPLIT and exact) and c["NEAR_PER_SAMPLE"] == (k.SB == 2 and not c["SPLIT"])
        assert c["WLW"] == 64 * c["UNIT_IN_DW"] + 96 and c["NNI"] == k.P * k.C * (k.S - 1)
        assert (c["vlim"] == 0) == (k.A == 2) and c["phase_exact_h"] == (k.S != 3), (inst, c)
        if exact:
            assert c["K"] == T.prefix_rows(k.S, k.A)


@pytest.mark.parametrize("inst", M.INSTANCES, ids=[M.inst_id(i) for i in M.INSTANCES])
def test_every_goal_is_reached_or_proven_unreachable(exe, inst, tmp_path):
    cens = _censuses(exe, inst, tmp_path)
    k = M.march_cfg(inst)
    m_lo, m_hi = T.rows(inst, M.frame_shape(inst)[1])
    consts = [cens[("int_h", e)].const for e in M.modes(inst)]
    reached = M.goal_states(inst, cens, m_lo, m_hi)
    got = {}
    for g in M.GOALS:
        if reached[g]:
            got[g] = ",".join(reached[g])
            continue
        why = M.unreachable_reason(inst, g, consts)
        assert why is not None, f"{M.inst_id(inst)}: goal {g} is neither reached on a content nor proven unreachable"
        got[g] = "unreachable: " + why
        if why.startswith("enumeration"):
            rc, out = _tool(exe, "enum22", k.C)
            assert rc == 0 and " flagged 0 " in out and " vlim 0 " in out, out
            assert all(c.summary["int"] == c.summary["near"] == c.summary["vredo"] == 0 for c in cens.values())
        elif why.startswith("vlim"):
            assert all(c["vlim"] == 0 for c in consts) and all(c.summary["int"] == 0 for c in cens.values())
        elif why.startswith("searched"):
            rc, out = _tool(exe, "searche", *inst, 1, *M.SEARCH)
            assert rc == 0 and "MOTIFE" not in out and "SEARCHE seed %d tries %d found 0" % M.SEARCH in out, out
        elif why.startswith("phase_exact_h"):
            assert all(c["phase_exact_h"] == 1 for c in consts) and k.S != 3
        else:
            assert why.startswith("not compiled") and len({bool(c["NEAR_PER_SAMPLE"]) for c in consts}) == 1
    variant, starts, want = EXPECT[M.inst_id(inst)]
    good, total = M.mask_starts(inst, cens[("mixed_v", 1)], m_lo, m_hi) if ("mixed_v", 1) in cens else (set(), 0)
    assert (M.v_variant(consts[0]), (len(good), total), got) == (variant, starts, want)


def test_the_motif_tables_are_what_the_searches_find(exe):
    """MOTIFS_* are the first hit of the tool's search modes under SEARCH, instance by instance; an instance without an entry
    is one the search found nothing for."""
    for inst in M.INSTANCES:
        for table, args in ((M.MOTIFS_H, ("searchh", *inst, 1, *M.SEARCH)), (M.MOTIFS_V, ("searchv", *inst, *M.SEARCH)),
                            (M.MOTIFS_I, ("searchi", *inst, *M.SEARCH)),
                            (M.MOTIFS_E, ("searche", *inst, 1, *M.SEARCH))) + \
                (((M.MOTIFS_H_LSB1, ("searchh", *inst, 0, *M.SEARCH)),) if len(M.modes(inst)) == 2 else ()) + \
                (((M.MOTIFS_F, ("searchf", *inst, 0)),) if inst[0] == 2 else ()) + \
                (((M.MOTIFS_B, ("searchb", *inst, M.frame_shape(inst)[0], *M.SEARCH)),) if inst[2] == 3 else ()):
            rc, out = _tool(exe, *args)
            hits = [tuple(int(v) for v in line.split()[1:]) for line in out.split("\n") if line.startswith("MOTIF")]
            first = hits[0] if hits else None
            if first is not None and args[0] == "searchf":
                first = first[0]
            if args[0] == "searchb":
                first = tuple(hits) if len(hits) == 2 else None
            assert rc == 0 and table.get(inst) == first, (inst, args[0], table.get(inst), first)


def test_the_wave_model_on_hand_made_waves():
    """march_fixup_cfg.wave_events -- hpass's list code restated -- on waves written out by hand (config 2: WLW 288, WL_ROUND 192,
    NNI 12): what reaches a goal, and that a wave without a biting entry reaches none."""
    k = M.march_cfg((1, 3, 2, 3))
    unit = lambda u, im=0, bim=0, near=0, nnear=0, bnear=0, past=0: [0, 0, u, im, bim, near, 0, nnear, 0, bnear, past, -1, -1]
    # 64 units with three candidates in round 0 (192 > WLW - WL_ROUND = 96: a flush) and one biting candidate in round 1
    wave = [unit(u, im=0x107, bim=0x101) for u in range(64)]
    assert M.wave_events(k, wave, False) == {"int_mid"}
    assert M.wave_events(k, [unit(3, im=0x1, bim=0x1)], False) == {"int_final"}
    assert M.wave_events(k, [unit(3, im=0x1)], False) == set()                      # nothing bites: nothing is reached
    assert M.wave_events(k, [unit(5, near=1, nnear=12, bnear=1)], False) == {"near_one"}
    full = [unit(u, near=1, nnear=12, bnear=1) for u in range(24)]
    assert M.wave_events(k, full, False) == set() and "near_loop" in M.wave_events(k, full + [unit(30, near=1, nnear=12, bnear=1)], False)
    assert M.wave_events(k, [unit(31, near=1, nnear=12, past=12)], False) == {"past_edge"}
