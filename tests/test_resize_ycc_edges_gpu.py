"""GPU checks of the two hand-written kernels of lanczos_resize_ycc_* past the shapes of tests/test_resize_ycc_gpu.py:
k_rs_ycc_split on rows of more than one workgroup and of fewer bytes than the way to the next dword, k_rs_ycc_merge_bytes and
k_rs_ycc_merge_tensor<E> on frames of more than one workgroup (1024 pixels) and over every (y, cb, cr), under the standard
tables and under callers' tables at the edge of what the contract allows, the 65 535-frame chunking of both launchers, and the
layouts the header allows and nothing ran (NV16 / NV61, YV12).

Two constructions isolate a kernel, both from the routing contract (an axis that keeps its size over the whole axis skips its
pass; LANCZOS_KERNEL_NONE is a plain copy), and both assert the route they rely on:

    merge alone   a 4:4:4 frame with out == in and the whole box: the three planes are copies, the merge sees the caller's
                  triples.  luma_kernel == chroma_kernel == KERNEL_NONE.
    split alone   NV12 / NV21 with even in_w, in_h and out = (in_w / 2, in_h / 2): the chroma box is the chroma plane, so chroma
                  is a copy of what the split wrote, and under Y.passthrough_table() (R = cb, G = y, B = cr) the output's R and B
                  are the split's bytes one to one.  chroma_kernel == KERNEL_NONE and info.split.

Every comparison is byte for byte or bit for bit against tests/resize_ycc_model.py (compose, convert, the tables) and
resize_tensor_view_model.scatter; tests/test_resize_ycc_host.py pins each of these shapes and tables without a GPU (the model
against the installed Pillow, the tables' sums in int64).  Outputs lie between sentinels, and every sentinel is checked.

Not run: the branch of k_rs_ycc_merge_tensor for g.n > 0xffffffff.  It cannot be taken: a side is at most kResizeMaxSize =
65535 pixels and 65535^2 < 2^32."""
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_tensor16_model as T16
import resize_tensor_model as T32
import resize_tensor_view_model as V
import resize_ycc_model as Y
from resize_ycc_run import GUARD, _bytes, _desc, _eq, _source, _tensor

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MERGE_BLOCK = 1024                                              # pixels of a workgroup of the merge kernels
NV = pytest.mark.parametrize("layout", [Y.NV12, Y.NV21], ids=["nv12", "nv21"])


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.resize_force(L.RESIZE_AUTO)
    c.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "resize_pillow_ycc.npz"))


TABLES = {"jfif": lambda: Y.table(Y.JFIF), "bt601": lambda: Y.table(Y.BT601), "bt709": lambda: Y.table(Y.BT709),
          "boundary": Y.boundary_table, "wide": Y.wide_table, "passthrough": Y.passthrough_table}


@pytest.fixture(scope="module")
def tables():
    """name -> (the table, its copy on the device)"""
    import torch
    return {k: (t, torch.from_numpy(t).cuda()) for k, t in ((k, make()) for k, make in TABLES.items())}


def _case(shape, name="edge"):
    return Y.Case(name, shape.sx, shape.sy, shape.in_w, shape.in_h, shape.out_w, shape.out_h, shape.filt, None, None, "noise")


# ---- the split ------------------------------------------------------------------------------------------------------------------
# A row of 2 cw bytes at residue r = address & 3 has head = min(-r & 3, 2 cw) bytes in front of its first aligned dword, nd =
# (2 cw - head) >> 2 dwords and rest bytes behind them; work item k < nd moves dword k, items nd .. nd + head + rest - 1 the
# bytes, 256 items to a workgroup (Y.split_cover restates this).  So, per width and residue, (head, nd, rest) and the items:
#   cw  511 (1022 B)  r = 0: (0, 255, 2)  dwords 0 .. 254, bytes 255, 256            -> a tail byte in workgroup 1
#                     r = 2: (2, 255, 0)  bytes 255, 256                             -> a head byte in workgroup 1
#                     r = 1, 3: (3, 254, 3) / (1, 255, 1)  bytes 254 .. 259 / 255, 256
#   cw  512 (1024 B)  r = 0: (0, 256, 0)  dwords 0 .. 255: exactly workgroup 0, nothing behind
#                     r = 1, 2, 3: nd = 255, bytes from item 255 on                  -> bytes in workgroup 1, no dword
#   cw  513 (1026 B)  r = 0: (0, 256, 2)  dwords fill workgroup 0, bytes 256, 257    -> only the byte tail in workgroup 1
#                     r = 2: (2, 256, 0)  the same with head bytes; r = 1, 3: nd = 255, bytes 255 .. 260 / 255 .. 258
#   cw  516 (1032 B)  r = 0: (0, 258, 0)  dwords 256, 257                            -> whole dwords in workgroup 1
#                     r = 1, 2, 3: nd = 257, dword 256 and bytes from 257 on
#   cw 1030 (2060 B)  every r: nd = 514 or 515, dwords 512 .. and the bytes behind   -> dwords and bytes in workgroup 2
SPLIT_WIDE_WORK = {511: {("byte", 1)}, 512: {("byte", 1)}, 513: {("byte", 1)}, 516: {("dword", 1), ("byte", 1)},
                   1030: {("dword", 2), ("byte", 2)}}


def _rows_cover(s, frames, cw, ch):
    """the residues of the interleaved rows of the frames `s`, and the (kind, workgroup) pairs with work over all of them"""
    res, who = set(), set()
    for f in range(frames):
        for r in range(ch):
            addr = s.at + f * s.frame_stride + s.cb_offset + r * s.c_row_stride      # from a dword-aligned base (asserted in _bytes)
            res.add(addr % 4)
            who |= Y.split_cover(addr, cw)[1]
    return res, who


def test_the_wide_rows_reach_the_second_and_third_workgroup():
    """plain arithmetic on the row cover, no kernel: the chosen widths put a dword and a tail byte into workgroup 1 and work
    into workgroup 2; at cw = 513 on an aligned row nothing but the byte tail is there"""
    assert set(Y.SPLIT_WIDE_CW) == set(SPLIT_WIDE_WORK)
    seen = set()
    for cw in Y.SPLIT_WIDE_CW:
        who = set().union(*(Y.split_cover(r, cw)[1] for r in range(4)))
        assert SPLIT_WIDE_WORK[cw] <= who, (cw, who)
        seen |= who
    assert {("dword", 1), ("byte", 1), ("dword", 2), ("byte", 2)} <= seen
    assert Y.split_cover(0, 513)[1] == {("dword", 0), ("byte", 1)} and Y.split_cover(0, 516)[1] == {("dword", 0), ("dword", 1)}
    assert all(who == {("dword", 0), ("byte", 0)} or who == {("dword", 0)} or who == {("byte", 0)}
               for cw in range(1, 42) for r in range(4) for who in (Y.split_cover(r, cw)[1],))   # the sibling file's widths: workgroup 0 only


@NV
@pytest.mark.parametrize("cw", Y.SPLIT_WIDE_CW)
def test_split_alone_on_wide_rows(ctx, tables, layout, cw):
    """the split-alone construction at 2 cw x 4, two frames a byte apart, the frame base at every residue, a tight and an odd
    chroma pitch: R and B are the chroma planes themselves, G is the model's luma.  The chroma differs from call to call, so
    that no byte the split left out can be right by what the call before left in the scratch"""
    shape = Y.split_alone_shape(cw)
    case, frames = _case(shape), 2
    y, cb, cr = Y.noise_planes(shape, frames, seed=2)
    want = Y.compose_shape(shape, y, cb, cr, t=tables["passthrough"][0])
    assert np.array_equal(want[..., 0], cb) and np.array_equal(want[..., 2], cr)       # the construction, in the model
    res, who = set(), set()
    cb0, cr0 = cb, cr
    for base in range(4):
        for crs in (2 * cw, 2 * cw + 1):
            cb, cr = cb0 ^ np.uint8(1 + 29 * base + 7 * (crs & 1)), cr0 ^ np.uint8(2 + 31 * base + 11 * (crs & 1))
            s = Y.build(y, cb, cr, layout, c_row_stride=crs, base=base, frame_gap=1, seed=3 + base)
            r1, w1 = _rows_cover(s, frames, cw, 2)
            res, who = res | r1, who | w1
            got = _bytes(ctx, case, s, frames, tables["passthrough"][1])
            info = ctx.last_ycc_info()
            assert info.split and info.chroma_kernel == L.KERNEL_NONE and info.luma_kernel != L.KERNEL_NONE, info
            what = f"layout {layout} cw {cw} base {base} pitch {crs}"
            _eq(got[..., 0], cb, what + ": Cb")
            _eq(got[..., 2], cr, what + ": Cr")
            _eq(got[..., 1], want[..., 1], what + ": luma")
    assert res == {0, 1, 2, 3} and SPLIT_WIDE_WORK[cw] <= who, (res, who)


@NV
def test_split_on_an_odd_wide_row_then_the_chroma_pass(ctx, tables, layout):
    """1031 x 3: cw = 516 and ch = 2 from odd sizes, so the chroma planes the split wrote go through a resize pass"""
    shape = Y.SPLIT_ODD_WIDE
    for base in range(4):
        y, cb, cr = Y.noise_planes(shape, 2, seed=3 + base)     # other planes every call: nothing is right by the scratch's leftovers
        want = Y.compose_shape(shape, y, cb, cr)
        s = Y.build(y, cb, cr, layout, c_row_stride=2 * 516 + 1, base=base, frame_gap=1)
        assert ("dword", 1) in _rows_cover(s, 2, 516, 2)[1]
        _eq(_bytes(ctx, _case(shape), s, 2, tables["jfif"][1]), want, f"layout {layout} base {base}")
        info = ctx.last_ycc_info()
        assert info.split and info.chroma_kernel != L.KERNEL_NONE and info.luma_kernel != L.KERNEL_NONE, info


@NV
def test_split_on_narrow_rows(ctx, tables, layout):
    """in_w 1 .. 9 x in_h 1 .. 3 (rows of 1 .. 5 pairs) at every base residue with an odd chroma pitch, to 3 x 2 and to the same
    size: head = min(to_dword, len), nd == 0 and rest in every combination"""
    covers = set()
    for shape in Y.narrow_shapes():
        cw, ch = Y.chroma_size(shape.in_w, shape.in_h, 1, 1)
        for base in range(4):
            y, cb, cr = Y.noise_planes(shape, 2, seed=4 + base)                        # other planes every call
            want = Y.compose_shape(shape, y, cb, cr)
            s = Y.build(y, cb, cr, layout, c_row_stride=2 * cw + 1, base=base, seed=5 + base)
            covers |= {(cw,) + Y.split_cover(s.at + f * s.frame_stride + s.cb_offset + r * s.c_row_stride, cw)[0]
                       for f in range(2) for r in range(ch)}
            _eq(_bytes(ctx, _case(shape), s, 2, tables["jfif"][1]), want, f"layout {layout} {shape} base {base}")
            assert ctx.last_ycc_info().split
    # every (cw, head, nd, rest) a row of 1 .. 5 pairs can have: 4 residues each
    assert covers == {(cw,) + Y.split_cover(r, cw)[0] for cw in range(1, 6) for r in range(4)}
    assert {(1, 2, 0, 0), (1, 1, 0, 1), (1, 0, 0, 2), (2, 3, 0, 1)} <= covers          # no dword at all: the row ends before or at the next one


def test_nv16_nv61_and_yv12(ctx, golden, tables):
    """NV12 / NV21 with sub_y = 0 (4:2:2 with interleaved chroma) against Pillow's 4:2:2 fixture, and planar frames with Cr in
    front of Cb against the 4:2:0 one"""
    d_jfif = tables["jfif"][1]
    case = Y.CASE["i422_down"]
    y, cb, cr = Y.make_planes(case, 2)
    for layout in (Y.NV12, Y.NV21):
        for base in range(4):
            s = Y.build(y, cb, cr, layout, c_row_stride=2 * 17 + 1, base=base, gap=base, frame_gap=1)
            _eq(_bytes(ctx, case, s, 2, d_jfif), golden["i422_down_out"], f"4:2:2 layout {layout} base {base}")
            info = ctx.last_ycc_info()
            assert info.split and info.launches == 4, info
    case = Y.CASE["i420_down"]
    y, cb, cr = Y.make_planes(case, 2)
    for kw in (dict(), dict(c_row_stride=21, gap=3, base=1, frame_gap=2)):
        s = Y.build(y, cb, cr, Y.PLANAR, cr_first=True, **kw)
        assert s.cr_offset < s.cb_offset
        _eq(_bytes(ctx, case, s, 2, d_jfif), golden["i420_down_out"], f"YV12 {kw}")
        assert not ctx.last_ycc_info().split


# ---- the merge over every (y, cb, cr) ------------------------------------------------------------------------------------------
ALL = Y.Case("all_triples", 0, 0, 4096, 4096, 4096, 4096, "lanczos", None, None, "")


@pytest.fixture(scope="module")
def triples():
    """the 4:4:4 frame of Y.all_triples() as it lies in memory, between noise"""
    y, cb, cr = Y.all_triples()
    rng = np.random.default_rng(6)
    edge = lambda: rng.integers(0, 256, Y.MARGIN, dtype=np.uint8)
    buf = np.concatenate([edge(), y.ravel(), cb.ravel(), cr.ravel(), edge()])
    n = 1 << 24
    return (y, cb, cr), Y.Frames(buf, Y.MARGIN, 3 * n, 4096, 4096, n, 2 * n, Y.PLANAR)


def _first_triple(diff_hw, what, got, want):
    i = int(np.flatnonzero(diff_hw.ravel())[0])
    raise AssertionError(f"{what}: {int(diff_hw.sum())} triples differ, first (y, cb, cr) = ({i >> 16}, {(i >> 8) & 255}, {i & 255}): "
                         f"{got(i)} != {want(i)}")


@pytest.mark.parametrize("name", ["jfif", "bt601", "bt709", "boundary", "wide"])
def test_merge_bytes_over_all_triples(ctx, tables, triples, name):
    """merge alone, every triple once, under the three standard tables, the boundary table (sums at both ends of int32 and at
    every step of clip8(sum >> 6)) and the wide one"""
    (y, cb, cr), s = triples
    t, dt = tables[name]
    got = _bytes(ctx, ALL, s, 1, dt)[0]
    info = ctx.last_ycc_info()
    assert info.luma_kernel == info.chroma_kernel == L.KERNEL_NONE and not info.split, info
    assert info.launches == 4, info                             # three copies and the merge
    want = Y.convert(t, y, cb, cr)                              # in int64
    if not np.array_equal(got, want):
        g, w = got.reshape(-1, 3), want.reshape(-1, 3)
        _first_triple((got != want).any(-1), f"table {name}", lambda i: g[i], lambda i: w[i])


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_merge_tensor_over_all_triples(ctx, tables, triples, dtype):
    """the same frame through k_rs_ycc_merge_tensor<uint32_t> and <uint16_t>: CHW, the reversing map and both flips, the
    identity element tables, so that every byte value of every channel goes through the wave's exchange and is named"""
    import torch
    (y, cb, cr), s = triples
    t, dt = tables["jfif"]
    src, flip, n = (2, 1, 0), 3, 1 << 24
    elem, word, signed, SENT, lut = ((4, np.uint32, np.int32, 0xA5A5A5A5, T32.identity_lut(3)) if dtype == "float32" else
                                     (2, np.uint16, np.int16, 0xA5A5, T16.identity_lut16(3)))
    yb = torch.from_numpy(np.full(GUARD + 3 * n + GUARD, SENT, dtype=word).view(signed)).cuda()
    x = torch.from_numpy(s.buf).cuda()
    dl = torch.from_numpy(V.words(lut).view(signed)).cuda()
    d = _desc(ALL)
    ctx.resize_ycc_tensor_device(d, _source(d, ALL, s), dt.data_ptr(), x.data_ptr() + s.at, yb.data_ptr() + elem * GUARD, 1,
                                 dl.data_ptr(), V.strides("chw", 4096, 4096, 3), in_frame_stride=s.frame_stride,
                                 stream=torch.cuda.current_stream().cuda_stream, dtype=dtype, channels_out=src, flip=flip)
    torch.cuda.synchronize()
    info = ctx.last_ycc_info()
    assert info.luma_kernel == info.chroma_kernel == L.KERNEL_NONE and info.launches == 4, info
    raw = yb.cpu().numpy().view(word)
    assert (raw[:GUARD] == SENT).all() and (raw[GUARD + 3 * n:] == SENT).all(), "a word outside the frame was written"
    got = raw[GUARD:GUARD + 3 * n].reshape(3, 4096, 4096)
    want = Y.chw_words(Y.convert(t, y, cb, cr), lut, src, flip)
    for oc in range(3):
        if not np.array_equal(got[oc], want[oc]):
            g, w = got[oc][::-1, ::-1].ravel(), want[oc][::-1, ::-1].ravel()         # flip 3 undone: pixel i is triple i
            _first_triple(g != w, f"{dtype} output channel {oc}", lambda i: hex(g[i]), lambda i: hex(w[i]))


def test_boundary_table_behind_a_resize_pass(ctx, tables):
    """the clamp in front of the shift also where the planes come out of a resize pass: NV12 at i420_edges_down (ringing
    edges in all three planes), whole and through a window that starts at an odd pixel, under the boundary table"""
    case = Y.CASE["i420_edges_down"]
    y, cb, cr = Y.make_planes(case, 2)
    t, dt = tables["boundary"]
    s = Y.build(y, cb, cr, Y.NV12, y_row_stride=case.in_w + 3, base=1)
    for win in (None, (3, 1, 13, 9)):
        want = Y.compose(y, cb, cr, 1, 1, case.out_w, case.out_h, window=win, t=t)
        _eq(_bytes(ctx, case, s, 2, dt, window=win), want, f"window {win}")
        info = ctx.last_ycc_info()
        assert info.split and info.luma_kernel != L.KERNEL_NONE and info.chroma_kernel != L.KERNEL_NONE, info


# ---- the merge past one workgroup ----------------------------------------------------------------------------------------------
# name -> (w, h, window): 61 x 40 is 2440 pixels, two full workgroups and a third of 392 whose second wave is partial; its
# windows start at an odd pixel, cover more than a workgroup and leave tails of 3, 2 and 1 pixels in the second workgroup
PAST = {"61x40": (61, 40, None), "1x1500": (1, 1500, None), "2500x1": (2500, 1, None), "1100x3": (1100, 3, None),
        "61x40 window 55x37": (61, 40, (3, 1, 55, 37)), "61x40 window 54x37": (61, 40, (3, 1, 54, 37)),
        "61x40 window 53x37": (61, 40, (3, 1, 53, 37))}
PAST_TENSOR = ("61x40", "1x1500", "2500x1", "1100x3", "61x40 window 55x37")


def _past_one_workgroup(name, golden, frames=4):
    """(case, the frames as they lie in memory, the RGB bytes [F][h][w][3], the window) of an entry of PAST: the 61 x 40
    ones are Pillow's fixture i420_up_bicubic from NV12 frames, the others 4:4:4 frames that keep their size (merge alone)"""
    w, h, win = PAST[name]
    if (w, h) == (61, 40):
        case = Y.CASE["i420_up_bicubic"]
        pick = [0, 1, 1, 0][:frames]
        y, cb, cr = (p[pick] for p in Y.make_planes(case, 2))
        ref = golden["i420_up_bicubic_out"][pick]
        if win is not None:
            ref = ref[:, win[1]:win[1] + win[3], win[0]:win[0] + win[2]]
        return case, Y.build(y, cb, cr, Y.NV12, y_row_stride=case.in_w + 1, base=1), ref, win, False
    shape = Y.Shape(0, 0, w, h, w, h, "lanczos")
    y, cb, cr = Y.noise_planes(shape, frames, seed=6)
    return _case(shape), Y.build(y, cb, cr, Y.PLANAR, base=1, gap=1), Y.convert(Y.table(Y.JFIF), y, cb, cr), None, True


def _assert_route(ctx, merge_alone):
    info = ctx.last_ycc_info()
    if merge_alone:
        assert info.luma_kernel == info.chroma_kernel == L.KERNEL_NONE and not info.split, info
    else:
        assert info.split and info.luma_kernel != L.KERNEL_NONE and info.chroma_kernel != L.KERNEL_NONE, info


def test_the_outputs_past_one_workgroup_are_what_they_are_for():
    px = {k: (w * h if win is None else win[2] * win[3]) for k, (w, h, win) in PAST.items()}
    assert all(n > MERGE_BLOCK for n in px.values())
    assert {n % 4 for n in px.values()} == {0, 1, 2, 3}                                # the byte kernel's tails, none in workgroup 0
    assert all(n // 4 * 4 >= MERGE_BLOCK for n in px.values())
    assert px["61x40"] == 2 * MERGE_BLOCK + 392 and 256 < 392 < 512                   # a third workgroup whose second wave is partial
    w, h, _ = PAST["1100x3"]
    assert w > MERGE_BLOCK and MERGE_BLOCK % w != 0 and (2 * MERGE_BLOCK) // w != (3 * MERGE_BLOCK - 1) // w   # rem0 != 0; dy changes inside
    assert PAST["1x1500"][0] == 1 and PAST["2500x1"][1] == 1 and PAST["2500x1"][0] > 2 * MERGE_BLOCK
    assert all(PAST[k][2][0] % 2 == 1 for k in PAST if PAST[k][2] is not None)


@pytest.mark.parametrize("name", PAST_TENSOR)
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_tensor_outputs_past_one_workgroup(ctx, golden, tables, dtype, name):
    """CHW and HWC, tight and gapped, the identity, the reversing and a two-channel map, flips 0 .. 3 per frame from d_flip and
    one flip from the struct, on frames whose pixels span workgroups: base, y0, rem0 and dy of k_rs_ycc_merge_tensor"""
    frames = 4
    lut_of = (lambda oc: T32.identity_lut(oc)) if dtype == "float32" else (lambda oc: T16.identity_lut16(oc))
    case, s, ref, win, merge_alone = _past_one_workgroup(name, golden, frames)
    _, h, w, _ = ref.shape
    dt = tables["jfif"][1]
    for src in ((0, 1, 2), (2, 1, 0), (2, 0)):
        oc = len(src)
        layouts = {"chw": V.strides("chw", w, h, oc), "hwc": V.strides("hwc", w, h, oc),
                   "chw padded": (h * (w + 3) + 5, w + 3, 1), "hwc gaps": (1, w * (oc + 2) + 1, oc + 2)}
        for st in layouts.values():
            _tensor(ctx, case, s, frames, dt, ref, lut_of(oc), src, [0, 1, 2, 3], st, dtype, window=win)
            _assert_route(ctx, merge_alone)
    m = 1 + PAST_TENSOR.index(name) % 3                          # a flip for every frame, from the host struct alone
    _tensor(ctx, case, s, frames, dt, ref, lut_of(3), (0, 1, 2), [m] * frames, V.strides("chw", w, h, 3), dtype, window=win,
            host_flip=m)


@pytest.mark.parametrize("name", list(PAST))
def test_bytes_past_one_workgroup_with_a_padded_frame_stride(ctx, golden, tables, name):
    """k_rs_ycc_merge_bytes on the same outputs, three frames a padded stride apart: the tails of 0 .. 3 pixels lie in a later
    workgroup than the first"""
    case, s, ref, win, merge_alone = _past_one_workgroup(name, golden, 3)
    _eq(_bytes(ctx, case, s, 3, tables["jfif"][1], window=win, pad=2), ref, name)
    _assert_route(ctx, merge_alone)


# ---- more than 65 535 frames ---------------------------------------------------------------------------------------------------
def _groups(frames):
    return (frames + 65534) // 65535                            # a launch takes at most 65 535 frames


def _plane_launches(in_w, in_h, out_w, out_h, frames):
    """the launches of one one-channel resize call, from lanczos_resize_window_plan_host and the header: no pass is one copy;
    the fused kernel or a single pass is one kernel, two passes are two, each once per group of frames"""
    p = L.resize_window_plan_host(L.resize_desc(in_w, in_h, out_w, out_h, 1), None, frames, box=(0, 0, in_w, in_h))
    if not (p.pass_h or p.pass_v):
        return 1
    return (1 if p.inner.fused or not (p.pass_h and p.pass_v) else 2) * _groups(frames)


@pytest.mark.parametrize("layout", [Y.PLANAR, Y.NV12], ids=["i420", "nv12"])
def test_more_than_65535_frames_in_one_call(ctx, tables, layout):
    """ycc_split_launch and ycc_merge_launch go out in groups of 65 535 frames and re-base g.in, g.out, g.y, g.c and
    g.d_flip: 65 537 frames of 4 x 2 cycled from 8, four further ones at 0, 65534, 65535 and 65536, every frame compared"""
    import torch
    shape, F = Y.MANY_FRAMES, 65537
    case = _case(shape)
    y, cb, cr = Y.noise_planes(shape, 12, seed=7)
    ref12 = Y.compose_shape(shape, y, cb, cr)
    assert len({r.tobytes() for r in ref12}) == 12
    idx = np.arange(F) % 8
    idx[[0, 65534, 65535, 65536]] = [8, 9, 10, 11]
    tight = Y.tight(y, cb, cr, layout)
    assert tight.shape == (12, 12)
    rng = np.random.default_rng(8)
    buf = np.concatenate([rng.integers(0, 256, Y.MARGIN + 1, dtype=np.uint8), tight[idx].ravel(),
                          rng.integers(0, 256, Y.MARGIN, dtype=np.uint8)])
    s = (Y.Frames(buf, Y.MARGIN + 1, 12, 4, 2, 8, 10, layout) if layout == Y.PLANAR else
         Y.Frames(buf, Y.MARGIN + 1, 12, 4, 4, 8, 8, layout))
    dt = tables["jfif"][1]
    # the count the header defines (resize kernels, copies, split and merge): luma and the merge once per group of frames, the
    # planar chroma as two calls of F frames, the split once per group and its planes as one call of 2 F frames
    k_luma = _plane_launches(4, 2, 3, 2, F)
    if layout == Y.PLANAR:
        launches = k_luma + 2 * _plane_launches(2, 1, 3, 2, F) + _groups(F)
    else:
        launches = k_luma + _groups(F) + _plane_launches(2, 1, 3, 2, 2 * F) + _groups(F)
    assert _groups(F) == 2 and _groups(2 * F) == 3
    got = _bytes(ctx, case, s, F, dt)
    info = ctx.last_ycc_info()
    _eq(got, ref12[idx], f"layout {layout}: bytes")
    assert info.split == (layout == Y.NV12) and info.launches == launches, (info, launches)
    # float32 CHW with a flip per frame; the flips of the second group's first frames differ from those an un-rebased d_flip has
    flips = (np.arange(F) & 3).astype(np.uint8)
    flips[65535], flips[65536] = 2, 3
    assert flips[65535] != flips[0] and flips[65536] != flips[1]
    lut = T32.identity_lut(3)
    views = np.stack([np.stack([V.view(ref12[k], lut, None, m) for m in range(4)]) for k in range(12)])   # [12][4][3][2][3]
    assert not np.array_equal(views[idx[65535], flips[65535]], views[idx[65535], flips[0]])
    assert not np.array_equal(views[idx[65536], flips[65536]], views[idx[65536], flips[1]])
    n, SENT = 18, 0xA5A5A5A5
    fs = n + 5
    total = GUARD + (F - 1) * fs + n + GUARD
    want = np.full(total, SENT, dtype=np.uint32)
    want[(GUARD + fs * np.arange(F))[:, None] + np.arange(n)[None, :]] = views[idx, flips].reshape(F, n)
    yb = torch.from_numpy(np.full(total, SENT, dtype=np.uint32).view(np.int32)).cuda()
    x = torch.from_numpy(s.buf).cuda()
    dl = torch.from_numpy(lut.view(np.int32)).cuda()
    df = torch.from_numpy(flips).cuda()
    d = _desc(case)
    ctx.resize_ycc_tensor_device(d, _source(d, case, s), dt.data_ptr(), x.data_ptr() + s.at, yb.data_ptr() + 4 * GUARD, F,
                                 dl.data_ptr(), V.strides("chw", 3, 2, 3), in_frame_stride=12, out_frame_stride=4 * fs,
                                 stream=torch.cuda.current_stream().cuda_stream, d_flip=df.data_ptr())
    torch.cuda.synchronize()
    assert ctx.last_ycc_info().launches == launches
    got = yb.cpu().numpy().view(np.uint32)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        at = int(bad[0]) - GUARD
        raise AssertionError(f"layout {layout}: {len(bad)} words differ, first in frame {at // fs} at word {at % fs}: "
                             f"{int(got[bad[0]]):#x} != {int(want[bad[0]]):#x}")


def test_more_than_65535_frames_cropped_in_one_call(ctx, tables):
    """65 537 frames of a 4 x 2 4:4:4 source kept at size, of which the window 2 x 2 at (2, 0) is stored: no pass runs and the
    window is not the frame, so every plane is rs_route's kRsMainCrop, and k_rs_crop takes the whole batch in ONE launch (it
    strides over the frames with gridDim.z) where every other step goes out once per 65 535 frames.  Every frame is compared
    with the slice of its source, and the count is the launches that went out: one per plane and the merge in two groups"""
    shape, F, win = Y.Shape(0, 0, 4, 2, 4, 2, "lanczos"), 65537, (2, 0, 2, 2)
    case = _case(shape)
    p = L.resize_window_plan_host(L.resize_desc(4, 2, 4, 2, 1), win, F, box=(0, 0, 4, 2))
    assert not (p.pass_h or p.pass_v)                           # a copy of a window: the crop
    y, cb, cr = Y.noise_planes(shape, 12, seed=9)
    ref12 = Y.convert(Y.table(Y.JFIF), y, cb, cr)[:, win[1]:win[1] + win[3], win[0]:win[0] + win[2]]
    assert len({r.tobytes() for r in ref12}) == 12
    idx = np.arange(F) % 8
    idx[[0, 65534, 65535, 65536]] = [8, 9, 10, 11]
    tight = Y.tight(y, cb, cr, Y.PLANAR)
    assert tight.shape == (12, 24)
    rng = np.random.default_rng(10)
    buf = np.concatenate([rng.integers(0, 256, Y.MARGIN + 1, dtype=np.uint8), tight[idx].ravel(),
                          rng.integers(0, 256, Y.MARGIN, dtype=np.uint8)])
    s = Y.Frames(buf, Y.MARGIN + 1, 24, 4, 4, 8, 16, Y.PLANAR)
    got = _bytes(ctx, case, s, F, tables["jfif"][1], window=win)
    info = ctx.last_ycc_info()
    _eq(got, ref12[idx], "65537 cropped frames")
    assert info.luma_kernel == info.chroma_kernel == L.KERNEL_NONE and not info.split, info
    assert _groups(F) == 2 and info.launches == 3 * 1 + _groups(F), info


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_not_yet_exercised(ctx, tables):
    """a d_table off a dword, and an interleaved 4:2:2 layout with two different offsets: ERR_BAD_ARG from both device entries,
    and the report of the last good call stays"""
    import torch
    case = Y.CASE["i422_down"]
    d = _desc(case)
    y, cb, cr = Y.make_planes(case, 2)
    fr = torch.from_numpy(np.concatenate([Y.tight(y, cb, cr, Y.NV12).ravel(), np.zeros(64, np.uint8)])).cuda()
    n = case.out_w * case.out_h * 3
    out = torch.zeros(2 * n + 64, dtype=torch.uint8, device="cuda")
    t = torch.zeros(2 * n + 64, dtype=torch.float32, device="cuda")
    dl = torch.from_numpy(T32.identity_lut(3)).cuda()
    st = V.strides("chw", case.out_w, case.out_h, 3)
    src = L.ycc_source(d, L.YCC_NV12, 1, 0)
    table = torch.zeros(9 * 256 + 1, dtype=torch.int32, device="cuda")            # room for the table at any residue
    table[:9 * 256] = tables["jfif"][1].reshape(-1)
    ctx.resize_ycc_device(d, src, table.data_ptr(), fr.data_ptr(), out.data_ptr(), 2)
    torch.cuda.synchronize()
    before = ctx.last_ycc_info()
    assert before.split and before.launches == 4

    def both(s=src, tp=table.data_ptr()):
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_ycc_device(d, s, tp, fr.data_ptr(), out.data_ptr(), 2)
        assert e.value.code == L.ERR_BAD_ARG, e.value.code
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_ycc_tensor_device(d, s, tp, fr.data_ptr(), t.data_ptr(), 2, dl.data_ptr(), st)
        assert e.value.code == L.ERR_BAD_ARG, e.value.code
    assert table.data_ptr() % 4 == 0
    for off in (1, 2, 3):
        both(tp=table.data_ptr() + off)
    for layout in (L.YCC_NV12, L.YCC_NV21):
        nv = L.ycc_source(d, layout, 1, 0)
        assert (nv.sub_x, nv.sub_y) == (1, 0) and nv.cb_offset == nv.cr_offset
        nv.cr_offset += 1
        both(s=nv)
        nv.cr_offset -= 2
        both(s=nv)
    torch.cuda.synchronize()
    assert ctx.last_ycc_info() == before
    assert not out[2 * n:].any() and not t.view(torch.int32).any()              # and nothing was stored by a refused call
