"""k_march's fix-up worklist and f64 redo paths on contents that steer them: every instance x every content of
tests/march_fixup_cfg.py x EXACT and LSB1, against the CPU oracle.

What the contents reach -- the integer-phase rounds with and without a mid-loop flush, the near-integer path with one unit and
with an in-loop flush, the per-sample path, entries past the right edge, entries whose taps the frame edge cuts off, undecided integer-phase and computed rows on every
arithmetic variant of the V pass, a single undecided lane in the partial last strip, each with samples whose f32 store is NOT the
reference's -- is established without a GPU by tests/test_march_fixup_cfg.py.  Here the kernels run:

  single frame   route march + riding, one launch, asserted; EXACT bit-identical to the oracle, LSB1 by test_parity_gpu._cmp
                 (within 1 LSB and lsb1_check.check)
  batch          the instance's contents cycled over the smallest batch that sends the prefix rows somewhere else than riding
                 (more prefix workgroups than CUs: the non-riding instantiation of k_march), route asserted.  Where the split rule
                 of lanczos_resample_device cuts that batch into launches small enough to ride again (asserted on the reported
                 workgroups per CU), the non-riding instantiation is reached by a row strip that starts behind the prefix rows
  the table      after the EXACT calls the table the launch reports (Context.last_march_table) is held against the census: a
                 biting redo row stored from an interior V group and one from a chunk-edge (CHECKED) group, an integer-phase redo
                 row just above a chunk (set in the mask of the chunk's first group, dropped by the redo loop) and a group whose mask holds bit 0 and the top
                 bit must all have run -- a table without an interior group fails with the advice to raise the frame height
  k_fast         near_h, near_v and mixed one pixel group wider (rows no 16-byte multiples): route tile, asserted

The census tool is compiled once per module (host code only)."""
import numpy as np
import pytest

import lanczos_hls_amd as L
import march_fixup_cfg as M
import march_table_cfg as T
from test_march_fixup_cfg import build_census, run_census
from test_parity_gpu import _cmp, _oracle

pytestmark = pytest.mark.gpu

MODES = (L.MODE_EXACT, L.MODE_LSB1)
MODE_IDS = {L.MODE_EXACT: "exact", L.MODE_LSB1: "lsb1"}
MARCH, TILE = L.ROUTE_MAIN_MARCH, L.ROUTE_MAIN_TILE
RIDING, BEHIND, NONE = L.ROUTE_PREFIX_RIDING, L.ROUTE_PREFIX_BEHIND, L.ROUTE_PREFIX_NONE
_IDS = [M.inst_id(i) for i in M.INSTANCES]


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_census(tmp_path_factory.mktemp("march_fixup_census"))


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _frames(inst):
    """[(content, frame, oracle output)] of an instance: every content it has (the 16-bit 2x instances: near_h with the LSB1
    motif as well), computed once per item."""
    out = []
    for name in M.CONTENTS:
        for lsb1 in (False, True) if name in ("near_h", "mixed", "near_one") and inst in M.MOTIFS_H_LSB1 else (False,):
            img = M.content(inst, name, lsb1=lsb1)
            if img is not None:
                out.append((name + (":lsb1" if lsb1 else ""), img, _oracle(img, inst[2], 1, inst[3])))
    return out


def _segments(tab, frame=0):
    """[(strip, m_b, m_e)] of one frame of a reported table."""
    return [(int(r[2]), int(r[3]), int(r[4])) for r in T.segments(tab) if r[1] == frame]


def _device_batch(ctx, inst, imgs, frames, mode, out_row0=0, out_rows=0):
    """`frames` frames (imgs cycled) through lanczos_resample_device; returns the output [frames][rows][out_w][c] on the host."""
    import torch
    bps, c, s, a = inst
    h, w, _ = imgs[0].shape
    d = L.make_desc(w, h, c, s, 1, a, bps, mode, out_row0, out_rows)
    r0, in_rows = L.strip_input_rows(d, out_row0, out_rows) if out_rows else (0, h)
    rows = out_rows or d.out_h
    src = np.stack([imgs[f % len(imgs)][r0:r0 + in_rows] for f in range(frames)])
    x = torch.from_numpy(src.view(np.uint8).reshape(frames, -1)).cuda()
    y = torch.full((frames, rows * d.out_w * c * bps), 0x5A, dtype=torch.uint8, device="cuda")
    assert x.data_ptr() % 16 == 0 and x.shape[1] % 16 == 0
    ctx.resample_device(d, x.data_ptr(), y.data_ptr(), frames, 0, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return y.cpu().numpy().view(imgs[0].dtype).reshape(frames, rows, d.out_w, c)


@pytest.mark.parametrize("inst", M.INSTANCES, ids=_IDS)
def test_fixup_paths_of_every_instance(ctx, exe, cus, inst, tmp_path):
    bps, c, s, a = inst
    k = M.march_cfg(inst)
    w, h = M.frame_shape(inst)
    K = T.prefix_rows(s, a)
    y_lo, y_hi = K, h * s
    frames = _frames(inst)
    assert len(frames) >= (3 if a == 2 and s == 2 and bps == 1 else 9), [f[0] for f in frames]
    cover = {"interior": 0, "checked": 0, "discarded": 0, "mask": 0}
    any_redo = False
    # ---- single frames: march + riding, one launch
    for name, img, want in frames:
        for mode in MODES:
            what = f"{M.inst_id(inst)} {w}x{h} {name} mode {MODE_IDS[mode]}"
            got = ctx.resample(img, s, 1, a, mode)
            r = ctx.last_route()
            assert (r.main, r.prefix, r.launches) == (MARCH, RIDING, 1), f"{what}: route {r}, built to reach march+riding in one launch"
            n = _cmp(got, want, mode, what, (img, s, 1, a, ctx.last_kernel()))
            assert mode != L.MODE_EXACT or n == 0
            if mode == L.MODE_EXACT and ":" not in name:
                info, tab = ctx.last_march_table()
                assert not T.partition_errors(T.Info(*info), tab) and (info.m_lo, info.m_hi) == T.rows(inst, h), f"{what}: {info}"
                segs = _segments(tab)
                assert any(inner for (_, m_b, m_e) in segs for (_, inner) in M.table_groups(inst, (m_b, m_e), y_lo, y_hi)), \
                    f"{what}: the reported table {segs} leaves no interior V group -- raise the frame height in march_fixup_cfg.frame_shape"
                cen, tail = run_census(exe, inst, img, True, tmp_path)
                assert cen.ok, f"{what}: {tail}"
                any_redo = any_redo or len(cen.V) > 0
                for key, v in M.table_coverage(inst, cen, segs, y_lo, y_hi).items():
                    cover[key] += v
    # ---- what the reported tables let the redo rows meet
    what = f"{M.inst_id(inst)} {w}x{h}"
    print(f"\n{what}: biting redo rows stored from interior groups {cover['interior']}, from chunk-edge groups {cover['checked']}; "
          f"integer-phase redo rows dropped above a chunk {cover['discarded']}; groups with mask bit 0 and the top bit {cover['mask']}")
    if bps == 1 and s == 2 and a == 2:
        assert not any_redo, f"{what}: the census finds redo rows where the enumeration proves there are none"
    else:
        assert cover["interior"] > 0 and cover["checked"] > 0, f"{what}: {cover}"
        if a >= 3:   # (a = 2: vlim == 0, no integer-phase row is ever undecided; a computed row outside a chunk reads ring rows
            #          that were never produced, which the census cannot predict)
            assert cover["discarded"] > 0 and cover["mask"] > 0, f"{what}: {cover}"
    # ---- the non-riding instantiation: a batch with more prefix workgroups than CUs, the contents cycled
    imgs, wants = [f[1] for f in frames], [f[2] for f in frames]
    blocks = -(-(w * s * c) // k.NT)
    n = max(cus // blocks + 1, len(frames))
    for mode in MODES:
        what = f"{M.inst_id(inst)} {w}x{h} x{n} mode {MODE_IDS[mode]}"
        got = _device_batch(ctx, inst, imgs, n, mode)
        r = ctx.last_route()
        info, tab = ctx.last_march_table()
        assert r.main == MARCH, f"{what}: route {r}"
        for f in range(n):
            j = f % len(frames)
            if f < len(frames):
                _cmp(got[f], wants[j], mode, f"{what} frame {f} ({frames[j][0]})", (imgs[j], s, 1, a, ctx.last_kernel()))
            else:
                assert np.array_equal(got[f], got[j]), f"{what}: frame {f} differs from frame {j} with the same content"
        if RIDING not in r.prefix_seen:
            assert r.launches == 1 and r.prefix in (L.ROUTE_PREFIX_FRONT, BEHIND), f"{what}: route {r}"
            continue
        # the split rule cut the batch into launches that ride again: asserted, and the non-riding kernel runs on a row strip
        assert r.launches > 1 and not T.single_launch(info.wg_per_cu, info.cus, -(-w // k.TWP_IN), n), f"{what}: route {r}, {info}"
        r0 = K + 1
        got = _device_batch(ctx, inst, imgs, len(frames), mode, r0, h * s - r0)
        r = ctx.last_route()
        assert (r.main, r.prefix, r.launches) == (MARCH, NONE, 1), f"{what} rows [{r0}, {h * s}): route {r}"
        for f in range(len(frames)):
            # (lsb1_check.check wants a whole frame: the strip's rows under the oracle's rows [0, r0), which pass it by themselves)
            whole = np.concatenate([wants[f][:r0], got[f]])
            _cmp(whole, wants[f], mode, f"{what} rows [{r0}, {h * s}) frame {f} ({frames[f][0]})", (imgs[f], s, 1, a, ctx.last_kernel()))
    # ---- the tile kernel on the same contents, one pixel group wider
    wt = M.tile_width(inst)
    for name in ("near_h", "near_v", "mixed"):
        img = M.content(inst, name, width=wt)
        if img is None:
            continue
        want = _oracle(img, s, 1, a)
        for mode in MODES:
            what = f"{M.inst_id(inst)} {wt}x{h} {name} mode {MODE_IDS[mode]} (k_fast)"
            got = ctx.resample(img, s, 1, a, mode)
            r = ctx.last_route()
            assert (r.main, r.prefix, r.launches) == (TILE, BEHIND, 1), f"{what}: route {r}"
            _cmp(got, want, mode, what, (img, s, 1, a, ctx.last_kernel()))
