"""k_march under every shape of its workgroup table, with the shape asserted.

What a marching workgroup computes is decided by a host-built table (csrc/lanczos_march.hpp: march_build_table):

  equal        mode B, equal chunks of a (strip, frame) pair's rows: a chunk that starts deep in the frame (the ring primed from real
               rows whose results are never stored) and a last chunk shorter than a tick
  rank-aware   mode B, the chunks of a pair cut by the speed of their CU slots: unequal ticks per workgroup, boundaries off the middle
  per-slot     mode A, one workgroup per CU slot, a share runs from the end of one pair into the next: the segment loop -- a new
               strip or a new frame (both buffer descriptors rebuilt) inside one workgroup, the ring and the prefetch restarted

Which batch reaches which shape depends on the workgroups resident per CU and the CU count, which only the device knows:
tests/march_table_cfg.py lists candidates per (instance, goal), the first one whose launch REPORTS (Context.last_march_table)
k_march, one launch and a table that meets the goal is taken, and finding none fails the test.  One exception, asserted, not
assumed: where the device holds one workgroup per CU, or two of eight waves, every slot speed is 1 and the builder has no
rank-aware shares (march_table_cfg.rank_aware_reachable); the batch then runs under the equal table it got, and the rank-aware
shape of that instance is reached in test_production_switches_reshape_the_table's manner only (LANCZOS_RANK_WEIGHTS).

Checked per case: the reported table partitions the launch (every frame, strip and row in exactly one non-empty segment, entries
in range) on the device's own nb and CUs; the bytes -- five distinct base frames cycled over a frame count that is no multiple of
five, the first occurrence of each against the CPU oracle (EXACT: bit-identical; LSB1: test_parity_gpu._cmp, i.e. within 1 LSB
and lsb1_check.check), every later frame byte for byte against the first of its base frame on the device: the same input at
other cut rows, in other segments; and the sentinel in the padding between the output frames."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import lanczos_hls_amd as L
import march_table_cfg as M
from test_parity_gpu import _cmp
from test_upscale_routes_gpu import _base_frames, _dev, _host, _oracle

pytestmark = pytest.mark.gpu

MODES = (L.MODE_EXACT, L.MODE_LSB1)
MODE_IDS = {L.MODE_EXACT: "exact", L.MODE_LSB1: "lsb1"}
PAD_IN, PAD_OUT = 48, 80   # bytes between frames (16-byte multiples: march_supports), poisoned


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _dt(inst):
    return np.uint16 if inst[0] == 2 else np.uint8


_BASES, _WANTS = {}, {}


def _bases(name, w, h):
    """The five base frames of a shape and, computed once for both modes and every test that uses the shape, their oracle results."""
    inst = M.INSTANCES[name]
    key = (name, w, h)
    if key not in _BASES:
        _BASES[key] = _base_frames(h, w, inst[1], _dt(inst), seed=7000 + 97 * list(M.INSTANCES).index(name) + h)
    return _BASES[key]


def _wants(name, w, h):
    inst = M.INSTANCES[name]
    key = (name, w, h)
    if key not in _WANTS:
        _WANTS[key] = [_oracle(b, inst[2], 1, inst[3])[0] for b in _bases(name, w, h)]
    return _WANTS[key]


def _launch(ctx, name, cand, mode, out_row0=0, out_rows=0):
    """One lanczos_resample_device call on `frames` frames (the base frames cycled), padded strides.  Returns the output frames
    [frames][rows][out_w][c] on the device (padding checked and cut off), the route and the reported table."""
    import torch
    bps, c, s, a = inst = M.INSTANCES[name]
    w, h, frames = cand
    dt = _dt(inst)
    d = L.make_desc(w, h, c, s, 1, a, bps, mode, out_row0, out_rows)
    r0, in_rows = L.strip_input_rows(d, out_row0, out_rows) if out_rows else (0, h)
    rows = out_rows or d.out_h
    in_fb, out_fb = in_rows * w * c * bps, rows * d.out_w * c * bps
    idx = torch.arange(frames, device="cuda") % 5
    src = _dev(np.stack([b[r0:r0 + in_rows] for b in _bases(name, w, h)]).reshape(5, in_fb // bps))
    x = torch.full((frames, (in_fb + PAD_IN) // bps), 0xA5A5 - 65536 if bps == 2 else 0xA5, dtype=src.dtype, device="cuda")
    x[:, :in_fb // bps] = src[idx]
    poison = 0x5A5A if bps == 2 else 0x5A
    y = torch.full((frames, (out_fb + PAD_OUT) // bps), poison, dtype=src.dtype, device="cuda")
    ctx.resample_device(d, x.data_ptr(), y.data_ptr(), frames, in_fb + PAD_IN, out_fb + PAD_OUT, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    route = ctx.last_route()
    info, tab = ctx.last_march_table()
    assert bool((y[:, out_fb // bps:] == poison).all()), f"{name} {cand}: the padding between the output frames was written"
    return y[:, :out_fb // bps].reshape(frames, rows, d.out_w, c), route, info, tab


def _pick(ctx, name, goal, mode):
    """The first candidate of (instance, goal) whose launch reports k_march, one launch and a table that meets the goal, with the
    result of that launch.  reached = False: the asserted exception of the module docstring."""
    inst = M.INSTANCES[name]
    tried = []
    for cand in M.CANDIDATES[(name, goal)]:
        y, route, info, tab = _launch(ctx, name, cand, mode)
        ok = (route.main, route.launches) == (L.ROUTE_MAIN_MARCH, 1)
        tried.append((cand, route, info, tab, ok))
        if ok and M.meets(goal, info, tab):
            return cand, y, info, tab, True
        del y
    nbs = {t[2].wg_per_cu for t in tried if t[2].workgroups}
    if goal == "rank-aware" and len(nbs) == 1 and not M.rank_aware_reachable(inst, nbs.pop()):
        assert not any(t[2].rank_aware for t in tried), f"{name}: rank-aware shares where every slot speed is 1"
        cand, route, info, tab, ok = next(t for t in tried if t[4])
        return cand, _launch(ctx, name, cand, mode)[0], info, tab, False
    raise AssertionError(f"{name} {goal} mode {MODE_IDS[mode]}: no candidate reaches the goal in one k_march launch -- " +
                         " | ".join(f"{t[0]}: {t[1]}; {M.describe(t[2], t[3]) if t[2].workgroups else 'no table'}" for t in tried))


def _check_bytes(ctx, name, cand, mode, y, what, wants=None, row0=0):
    """y [frames][rows][out_w][c] on the device against the oracle results of the base frames (rows [row0, row0 + rows) of them)."""
    import torch
    inst = M.INSTANCES[name]
    w, h, frames = cand
    rows = y.shape[1]
    wants = _wants(name, w, h) if wants is None else wants
    idx = torch.arange(frames, device="cuda") % 5
    bad = (y != y[:5][idx]).flatten(1).any(1).nonzero().flatten().tolist()
    assert not bad, f"{what}: frames {bad[:8]} (of {len(bad)}) differ from the first frame with the same content"
    for b in range(5):
        got, want = _host(y[b], _dt(inst)), wants[b][row0:row0 + rows]
        if mode == L.MODE_EXACT or rows == wants[b].shape[0]:
            _cmp(got, want, mode, f"{what}, frame {b}", (_bases(name, w, h)[b], inst[2], 1, inst[3], ctx.last_kernel()))
        else:   # (lsb1_check.check wants a whole frame)
            assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1, f"{what}, frame {b}: more than 1 LSB"


@pytest.mark.parametrize("mode", MODES, ids=[MODE_IDS[m] for m in MODES])
@pytest.mark.parametrize("goal", M.GOALS)
@pytest.mark.parametrize("name", list(M.INSTANCES))
def test_every_table_shape(ctx, name, goal, mode):
    import torch
    inst = M.INSTANCES[name]
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    cand, y, info, tab, reached = _pick(ctx, name, goal, mode)
    what = f"{name} {goal} {cand} mode {MODE_IDS[mode]}"
    print(f"\n{what}: nb {info.wg_per_cu}, {info.cus} CUs; {M.describe(info, tab)}" + ("" if reached else
          " -- every slot speed is 1 at this nb: no rank-aware shares, the equal table runs"))
    # the reported table, on the device's own nb and CUs
    assert not M.partition_errors(info, tab), f"{what}: {M.partition_errors(info, tab)}"
    assert (info.strips, info.frames) == (M.strips(inst, cand[0]), cand[2]) and (info.m_lo, info.m_hi) == M.rows(inst, cand[1]), f"{what}: {info}"
    assert info.mode != M.MODE_A or info.workgroups == info.wg_per_cu * info.cus, f"{what}: {info}"
    assert M.single_launch(info.wg_per_cu, info.cus, info.strips, info.frames), f"{what}: the split rule as restated would have cut this batch"
    _check_bytes(ctx, name, cand, mode, y, what)
    print(f"{what}: {time.time() - t0:.2f} s, peak device memory {torch.cuda.max_memory_allocated() / 2**20:.0f} MiB")


@pytest.mark.parametrize("mode", MODES, ids=[MODE_IDS[m] for m in MODES])
def test_a_row_strip_of_a_batch(ctx, mode):
    """Config 2, seven frames of 272 x 140, output rows [61, 198) from the input rows lanczos_strip_input_rows names: the strip's
    69 input rows go out as equal chunks of 31 / 31 / 7 that start at row 30 of the frame, not at its top.  Compared with the
    same rows of the whole-frame oracle result and, byte for byte in both modes, of the whole-frame run of the same batch."""
    name, cand, row0, rows = "u8-c3-2x-a3", (272, 140, 7), 61, 137
    inst = M.INSTANCES[name]
    whole, route, _, _ = _launch(ctx, name, cand, mode)
    assert (route.main, route.launches) == (L.ROUTE_MAIN_MARCH, 1), str(route)
    _check_bytes(ctx, name, cand, mode, whole, f"{name} {cand} mode {MODE_IDS[mode]}")
    y, route, info, tab = _launch(ctx, name, cand, mode, row0, rows)
    what = f"{name} rows [{row0}, {row0 + rows}) of {cand} mode {MODE_IDS[mode]}"
    print(f"\n{what}: {M.describe(info, tab)}")
    assert (route.main, route.prefix, route.launches) == (L.ROUTE_MAIN_MARCH, L.ROUTE_PREFIX_NONE, 1), f"{what}: {route}"
    assert (info.m_lo, info.m_hi) == M.rows(inst, cand[1], row0, rows) == (30, 99), f"{what}: {info}"
    assert not M.partition_errors(info, tab) and M.meets("equal", info, tab), f"{what}: {M.describe(info, tab)} {M.partition_errors(info, tab)}"
    _check_bytes(ctx, name, cand, mode, y, what, row0=row0)
    assert bool((y == whole[:, row0:row0 + rows]).all()), f"{what}: differs from the same rows of the whole-frame run"


def _child(tmp_path, tag, env_extra, want_mode, forced=None):
    out = str(tmp_path / f"{tag}.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LANCZOS_") or k == "LANCZOS_LIB"}
    env.update(env_extra)
    args = [sys.executable, os.path.join(os.path.dirname(__file__), "march_table_child.py"), out, str(want_mode)]
    if forced:
        args.append(forced)
    r = subprocess.run(args, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"{tag}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    return np.load(out)


def test_production_switches_reshape_the_table(tmp_path):
    """LANCZOS_MARCH_SEGS=1 with LANCZOS_RANK_WEIGHTS="4:1:1:0.25/4:1:0.25" (mode A wherever its conditions hold, very uneven
    shares: segments of exactly min_seg rows, idle workgroups and shares of three segments next to long ones) and
    LANCZOS_MARCH_WGS=63 (three chunks per pair where the default is five), each in a fresh child process on small config 2
    frames: the reported table partitions the launch and has the shape the switch asks for, EXACT equals the oracle, and the
    LSB1 bytes are those of the default run (the switches re-partition the work and change no sample)."""
    import march_table_child as E
    name = E.INSTANCE
    inst = M.INSTANCES[name]
    ms, taps = M.ms_taps(inst)
    base = _child(tmp_path, "default", {}, M.MODE_A)
    forced = "/".join(",".join(str(v) for v in base[f"slots:{t}:cand"]) for t in ("exact", "lsb1"))
    runs = {"default": base,
            "segs": _child(tmp_path, "segs", {"LANCZOS_MARCH_SEGS": "1", "LANCZOS_RANK_WEIGHTS": "4:1:1:0.25/4:1:0.25"}, M.MODE_A, forced),
            "wgs": _child(tmp_path, "wgs", {"LANCZOS_MARCH_WGS": "63"}, M.MODE_A, forced)}
    for run, res in runs.items():
        for req in E.REQUESTS:
            for tag, mode in (("exact", L.MODE_EXACT), ("lsb1", L.MODE_LSB1)):
                what = f"{run} {req} {tag}"
                cand = tuple(int(v) for v in res[f"{req}:{tag}:cand"])
                info, tab = M.Info(*(int(v) for v in res[f"{req}:{tag}:info"])), res[f"{req}:{tag}:table"]
                sm = M.summary(info, tab)
                print(f"\n{what} {cand}: {M.describe(info, tab)}, {sm['idle_wgs']} idle workgroups")
                assert tuple(res[f"{req}:{tag}:route"][[0, 2]]) == (L.ROUTE_MAIN_MARCH, 1), f"{what}: route {res[f'{req}:{tag}:route']}"
                assert not M.partition_errors(info, tab), f"{what}: {M.partition_errors(info, tab)}"
                assert (info.strips, info.frames) == (M.strips(inst, cand[0]), cand[2]) and (info.m_lo, info.m_hi) == M.rows(inst, cand[1])
                if req == "slots" and run != "wgs":   # (LANCZOS_MARCH_WGS leaves mode A to its own conditions)
                    assert M.meets("per-slot", info, tab), f"{what}: {M.describe(info, tab)}"
                    assert sm["shortest_segment"] == 3 * ms - (taps - 1), f"{what}: {M.describe(info, tab)}"
                if req == "slots" and run == "segs":
                    sg = M.segments(tab)
                    n_min = int(((sg[:, 4] - sg[:, 3]) == 3 * ms - (taps - 1)).sum())
                    print(f"{what}: {n_min} segments of exactly {3 * ms - (taps - 1)} rows")
                    assert n_min >= 8 and sm["longest_segment"] >= 3 * (3 * ms - (taps - 1)), f"{what}: {M.describe(info, tab)}"
                if req == "chunks":
                    assert M.meets("equal", info, tab), f"{what}: {M.describe(info, tab)}"
                    heights = sm["pair_heights"][(0, 0)]
                    assert heights == ([55, 55, 28] if run == "wgs" else [31, 31, 31, 31, 14]), f"{what}: chunks of {heights} rows"
                assert bool(res[f"{req}:{tag}:recur"]), f"{what}: a later frame differs from the first one with the same content"
                assert cand == tuple(int(v) for v in base[f"{req}:{tag}:cand"]), f"{what}: batch {cand}, the default run took another"
                first = res[f"{req}:{tag}:first"]
                if mode == L.MODE_EXACT:
                    wants = [_oracle(b, inst[2], 1, inst[3])[0] for b in E.base_frames(req, cand[0], cand[1])]
                    for b in range(5):
                        assert np.array_equal(first[b], wants[b]), f"{what}: frame {b} differs from the oracle"
                else:
                    assert np.array_equal(first, base[f"{req}:{tag}:first"]), f"{what}: LSB1 bytes differ from the default run"
                    exact = res[f"{req}:exact:first"]
                    if exact.shape == first.shape:
                        assert np.abs(first.astype(int) - exact.astype(int)).max() <= 1, f"{what}: more than 1 LSB from EXACT"


def test_table_report_of_the_other_calls(ctx):
    """The report follows lanczos_last_route: all zero on a new context, after a call that launched no k_march (the tile kernel,
    a strip inside the prefix rows), after a resize, a reduce and a layout call; the planar entry reports its resample; a split
    batch reports its LAST launch; and a short `entries` buffer is filled up to its capacity only."""
    import ctypes
    import torch
    import patterns as P
    fresh = L.Context(0)
    try:
        info, tab = fresh.last_march_table()
        assert tuple(info) == (0,) * 10 and tab.size == 0
    finally:
        fresh.close()
    img = P.noise(40, 64, 3, seed=9)
    ctx.resample(img, 2, 1, 3, L.MODE_EXACT)
    info, tab = ctx.last_march_table()
    assert ctx.last_route().main == L.ROUTE_MAIN_MARCH and info.mode == M.MODE_B and info.segs == 1 and (info.strips, info.frames) == (1, 1)
    assert (info.m_lo, info.m_hi) == (2, 40) and tab.shape == (info.workgroups, 1, 4) and not M.partition_errors(M.Info(*info), tab)
    # capacity: only that many quadruples are written, the return value is the table's size
    buf = np.full((info.workgroups + 1, 4), -7, np.int32)
    raw = L.MarchTableInfoC()
    n = L._lib().lanczos_last_march_table(ctx._h, ctypes.byref(raw), buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1)
    assert n == info.workgroups and np.array_equal(buf[0], tab[0, 0]) and (buf[1:] == -7).all() and raw.workgroups == info.workgroups
    assert L._lib().lanczos_last_march_table(ctx._h, None, None, 0) < 0
    for call in (lambda: ctx.resize(img, 32, 20), lambda: ctx.reduce(img, 2), lambda: ctx.resample(P.noise(40, 67, 3, seed=9), 2, 1, 3),
                 lambda: ctx.resample(img, 3, 2, 3)):
        ctx.resample(img, 2, 1, 3)
        assert ctx.last_march_table()[0].workgroups > 0
        call()
        info, tab = ctx.last_march_table()
        assert tuple(info) == (0,) * 10 and tab.size == 0, (info, ctx.last_route())
    d = L.make_desc(64, 40, 3, 2, 1, 3, 1, L.MODE_EXACT)
    x = _dev(np.ascontiguousarray(img.transpose(2, 0, 1)))
    y = torch.zeros((3, 80, 128), dtype=torch.uint8, device="cuda")
    ctx.resample_planar_device(d, x.data_ptr(), y.data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ctx.last_march_table()[0].workgroups > 0 and ctx.last_march_table()[0].frames == 1
    ctx.planar_to_interleaved_device(x.data_ptr(), y.data_ptr(), 64, 40, 3, 1, 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ctx.last_march_table()[0].workgroups == 0
    # a strip [0, 3) ends inside the prefix rows: no k_march launch
    ds = L.make_desc(64, 40, 3, 2, 1, 3, 1, L.MODE_EXACT, out_row0=0, out_rows=3)
    r0, n = L.strip_input_rows(ds, 0, 3)
    ctx.resample_strip(img[r0:r0 + n], ds)
    assert ctx.last_route().main == L.ROUTE_MAIN_NONE and ctx.last_march_table()[0].workgroups == 0
    # 9 frames through the host entry go out as groups of 4, 4 and 1: the report is the last launch's
    ctx.resample(np.stack([img] * 9), 2, 1, 3, L.MODE_EXACT)
    assert ctx.last_route().launches == 3 and ctx.last_march_table()[0].frames == 1
