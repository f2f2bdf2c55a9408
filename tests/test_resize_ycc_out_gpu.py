"""GPU checks of lanczos_resize_ycc_out: resize INTO YCbCr frames (I420, 4:2:2, 4:4:4, NV12, NV21) from YCbCr frames and from
packed RGB bytes.  The yardsticks are Pillow's committed fixture (tests/golden/resize_pillow_ycc_out.npz), the numpy model that
reproduces it (tests/resize_ycc_out_model.py) and, from YCbCr, three Context.resize calls on the planes.  Every call writes into
a whole buffer with noise in every byte the destination does not name and around the frames; the whole buffer is compared, so
a byte written outside the named ones fails the test that wrote it.

Launch counts: planar -> planar 3, NV -> planar 4 (the split), planar -> NV 4 (the join), NV -> NV 4: luma, split, one chroma call
of 2 * frames frames, join, and nothing else."""
import ctypes
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_ycc_model as Y
import resize_ycc_out_model as M
from resize_ycc_run import _eq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("i420", "i422", "i444", "nv12", "nv21")
FRAMES = M.FRAMES


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.resize_force(L.RESIZE_AUTO)
    c.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "resize_pillow_ycc_out.npz"))


@pytest.fixture(scope="module")
def d_tables():
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(t)).cuda() for k, t in
            (("jfif", L.ycc_table_forward("jfif")), ("bt709", L.ycc_table_forward("bt709")), ("clip", M.clip_table()))}


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _src_struct(d, layout, s):
    code, sx, sy = L.YCC_LAYOUTS[layout]
    return L.ycc_source(d, code, sx, sy, y_row_stride=s.y_row_stride, c_row_stride=s.c_row_stride, cb_offset=s.cb_offset,
                        cr_offset=s.cr_offset)


def _dst_struct(d, layout, s, window=None, aligned=True):
    code, sx, sy = L.YCC_LAYOUTS[layout]
    return L.ycc_dest(d, code, window, sx, sy, y_row_stride=s.y_row_stride, c_row_stride=s.c_row_stride, cb_offset=s.cb_offset,
                      cr_offset=s.cr_offset, aligned=aligned)


def _planes_of(golden, name, sub=None):
    if sub is None:
        return tuple(golden[f"{name}_{k}"] for k in ("y", "cb", "cr"))
    return golden[f"{name}_y"], golden[f"{name}_{sub}_cb"], golden[f"{name}_{sub}_cr"]


def _ycc(ctx, d, src_layout, s, dst_layout, before, window=None, box=None, gap=None, path=L.RESIZE_AUTO, frames=FRAMES):
    """YCbCr frames of Frames `s` into the buffer of Frames `before`: the whole buffer afterwards, and the call's info"""
    import torch
    x, o = torch.from_numpy(s.buf).cuda(), torch.from_numpy(before.buf).cuda()
    ctx.resize_force(path)
    try:
        ctx.resize_ycc_to_ycc_device(d, _src_struct(d, src_layout, s), _dst_struct(d, dst_layout, before, window), x.data_ptr() + s.at,
                                     o.data_ptr() + before.at, frames, in_frame_stride=s.frame_stride,
                                     out_frame_stride=before.frame_stride, stream=_stream(), box=box, reducing_gap=gap, window=window)
        torch.cuda.synchronize()
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    return o.cpu().numpy(), ctx.last_ycc_out_info()


def _rgb(ctx, d, x_np, at, fs, dst_layout, before, d_table, window=None, path=L.RESIZE_AUTO, frames=FRAMES):
    """RGB frames at byte `at` of x_np, `fs` bytes apart, into the buffer of Frames `before`"""
    import torch
    x, o = torch.from_numpy(x_np).cuda(), torch.from_numpy(before.buf).cuda()
    ctx.resize_force(path)
    try:
        ctx.resize_rgb_to_ycc_device(d, _dst_struct(d, dst_layout, before, window, aligned=False), d_table.data_ptr(), x.data_ptr() + at,
                                     o.data_ptr() + before.at, frames, in_frame_stride=fs, out_frame_stride=before.frame_stride,
                                     stream=_stream(), window=window)
        torch.cuda.synchronize()
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    return o.cpu().numpy(), ctx.last_ycc_out_info()


def _planned_kernel(in_w, in_h, out_w, out_h, filt, box, gap, frames, window=None, channels=1):
    """the kernel lanczos_resize_window_plan_host predicts for a plane (or an RGB frame) under AUTO (KERNEL_NONE: no pass runs)"""
    d = L.resize_desc(in_w, in_h, out_w, out_h, channels, filter=filt)
    p = L.resize_window_plan_host(d, window, frames, box=box if box is not None else (0, 0, in_w, in_h), reducing_gap=gap)
    if not (p.pass_h or p.pass_v):
        return L.KERNEL_NONE
    if filt == "nearest":
        return L.KERNEL_RESIZE_NEAREST
    return L.KERNEL_RESIZE_FUSED if p.inner.fused else L.KERNEL_RESIZE_TWO_PASS


def _pitched(planes, layout, seed=5, pad=3):
    """before / expected in a pitched layout: rows `pad` bytes longer than tight, the base off a dword, gaps in front of the
    chroma planes and one byte between frames"""
    w, cw = planes[0].shape[-1], planes[1].shape[-1]
    crow = cw if M.layout_code(layout) == M.PLANAR else 2 * cw
    return M.before_and_expected(planes, layout, seed=seed, y_row_stride=w + pad, c_row_stride=crow + pad - 1, base=1, gap=1, frame_gap=1)


_three = {}


def _three_resizes(ctx, case, planes):
    """three Context.resize calls on the planes: the composition the contract names (cached per case)"""
    if case.name not in _three:
        y, cb, cr = planes
        ocw, och = M.out_chroma_size(case.out_w, case.out_h, case.dsx, case.dsy)
        bc = Y.chroma_box(case.box, case.in_w, case.in_h, case.ssx, case.ssy)
        kw = dict(reducing_gap=case.gap, filter=case.filt)
        _three[case.name] = (ctx.resize(y[..., None], case.out_w, case.out_h, box=case.box, **kw)[..., 0],
                             ctx.resize(cb[..., None], ocw, och, box=bc, **kw)[..., 0], ctx.resize(cr[..., None], ocw, och, box=bc, **kw)[..., 0])
    return _three[case.name]


@pytest.mark.parametrize("dst", NAMES)
@pytest.mark.parametrize("src", NAMES)
def test_every_pair_of_layouts(ctx, golden, src, dst):
    """{i420, i422, i444, nv12, nv21} squared at 37 x 23 -> 22 x 14 and -> 50 x 31, pitched on both sides: Pillow's planes, the
    three resizes', the kernels the plan predicts, split only from NV, join only to NV, the launch counts of fused plans"""
    ssub, dsub = M.sub_of(src), M.sub_of(dst)
    for size in ("down", "up"):
        case = M.CASE[f"{M.SUB_NAME[ssub]}_to_{M.SUB_NAME[dsub]}_{size}"]
        planes = M.make_planes(case)
        d = L.resize_desc(case.in_w, case.in_h, case.out_w, case.out_h, 3)
        s = Y.build(*planes, M.layout_code(src), y_row_stride=case.in_w + 3, base=1, gap=2, frame_gap=1, seed=3)
        want_planes = _planes_of(golden, case.name)
        before, want = _pitched(want_planes, dst)
        got, info = _ycc(ctx, d, src, s, dst, before)
        _eq(got, want.buf, f"{src} -> {dst} {size}: the whole buffer against Pillow")
        for g, w in zip(_three_resizes(ctx, case, planes), want_planes):
            _eq(g, w, f"{case.name}: three resizes against Pillow")
        cw, ch = Y.chroma_size(case.in_w, case.in_h, *ssub)
        ocw, och = M.out_chroma_size(case.out_w, case.out_h, *dsub)
        src_nv, dst_nv = src.startswith("nv"), dst.startswith("nv")
        k_luma = _planned_kernel(case.in_w, case.in_h, case.out_w, case.out_h, case.filt, None, None, FRAMES)
        k_chroma = _planned_kernel(cw, ch, ocw, och, case.filt, Y.chroma_box(None, case.in_w, case.in_h, *ssub), None,
                                   2 * FRAMES if src_nv and dst_nv else FRAMES)
        assert (info.luma_kernel, info.chroma_kernel) == (k_luma, k_chroma), (info, k_luma, k_chroma)
        assert info.split == src_nv and info.join == dst_nv and not info.encode, info
        if k_luma == k_chroma == L.KERNEL_RESIZE_FUSED:
            assert info.launches == {(False, False): 3, (True, False): 4, (False, True): 4, (True, True): 4}[(src_nv, dst_nv)], info


@pytest.mark.parametrize("name,path", [("420_to_420_down", L.RESIZE_TWO_PASS), ("444_to_420_up", L.RESIZE_TWO_PASS),
                                       ("420_to_420_gap2", L.RESIZE_AUTO), ("420_to_420_nearest", L.RESIZE_AUTO),
                                       ("420_to_444_box", L.RESIZE_AUTO), ("420_to_444_box", L.RESIZE_TWO_PASS)])
def test_forced_two_pass_gap_nearest_and_box(ctx, golden, name, path):
    case = M.CASE[name]
    planes = M.make_planes(case)
    d = L.resize_desc(case.in_w, case.in_h, case.out_w, case.out_h, 3, filter=case.filt)
    want_planes = _planes_of(golden, name)
    pairs = [(s, t) for s in NAMES for t in NAMES if M.sub_of(s) == (case.ssx, case.ssy) and M.sub_of(t) == (case.dsx, case.dsy)]
    assert pairs
    for src, dst in pairs:
        s = Y.build(*planes, M.layout_code(src), c_row_stride=2 * planes[1].shape[-1] + 3, base=3, gap=1)
        before, want = _pitched(want_planes, dst)
        got, info = _ycc(ctx, d, src, s, dst, before, box=case.box, gap=case.gap, path=path)
        _eq(got, want.buf, f"{name} {src} -> {dst} path {path}")
        if path == L.RESIZE_TWO_PASS:
            assert L.KERNEL_RESIZE_FUSED not in (info.luma_kernel, info.chroma_kernel), info
        if case.filt == "nearest":
            assert info.luma_kernel == info.chroma_kernel == L.KERNEL_RESIZE_NEAREST, info


def test_same_size_is_a_pure_relayout(ctx, golden):
    """NV12 -> I420 (and every other 4:2:0 pair) at the same even size: no resize kernel runs, the planes are the source's.  At
    an odd size the chroma box is half a sample short of the plane: luma is a copy, chroma is filtered, as Pillow filters it"""
    for name, relayout in (("420_to_420_same", True), ("420_to_420_same_odd", False)):
        case = M.CASE[name]
        planes = M.make_planes(case)
        want_planes = _planes_of(golden, name)
        assert all(np.array_equal(w, p) for w, p in zip(want_planes, planes)) == relayout and np.array_equal(want_planes[0], planes[0])
        d = L.resize_desc(case.in_w, case.in_h, case.out_w, case.out_h, 3)
        for src, dst in (("nv12", "i420"), ("nv21", "nv12"), ("i420", "nv21"), ("i420", "i420")):
            s = Y.build(*planes, M.layout_code(src), y_row_stride=41, base=1, gap=3)
            before, want = _pitched(want_planes, dst)
            got, info = _ycc(ctx, d, src, s, dst, before)
            _eq(got, want.buf, f"{name} {src} -> {dst}")
            assert info.luma_kernel == L.KERNEL_NONE and (info.chroma_kernel == L.KERNEL_NONE) == relayout, info
            assert info.split == src.startswith("nv") and info.join == dst.startswith("nv"), info


@pytest.mark.parametrize("dst", ["nv12", "nv21"])
def test_join_at_every_residue(ctx, golden, dst):
    """NV12 / NV21 destinations at 37 x 23 -> 22 x 14: bases 0 .. 3, c_row_stride 25 (odd), a gap of 0 .. 3 bytes in front of the
    chroma plane and one byte between frames: the interleaved rows start at every residue"""
    case = M.CASE["420_to_420_down"]
    planes = M.make_planes(case)
    d = L.resize_desc(case.in_w, case.in_h, case.out_w, case.out_h, 3)
    s = Y.build(*planes, Y.PLANAR)
    want_planes = _planes_of(golden, case.name)
    rows = set()
    for base in range(4):
        for gap in range(4):
            before, want = M.before_and_expected(want_planes, dst, seed=base + 4 * gap, y_row_stride=23, c_row_stride=25, base=base, gap=gap,
                                                 frame_gap=1)
            got, info = _ycc(ctx, d, "i420", s, dst, before)
            _eq(got, want.buf, f"{dst} base {base} gap {gap}")
            assert info.join and not info.split
            rows |= {(want.at + f * want.frame_stride + want.cb_offset + r * 25) % 4 for f in range(FRAMES) for r in range(7)}
    assert rows == {0, 1, 2, 3}


def test_past_one_workgroup_of_the_join(ctx, golden):
    """2058 x 6 NV12 -> 1029 x 3 NV12: 515 chroma pairs = 1030 bytes per row, more than 256 dwords"""
    case = M.CASE["420_to_420_wide"]
    planes = M.make_planes(case)
    d = L.resize_desc(case.in_w, case.in_h, case.out_w, case.out_h, 3)
    want_planes = _planes_of(golden, case.name)
    assert want_planes[1].shape[-1] == 515
    for src, dst, base in (("nv12", "nv12", 0), ("nv21", "nv12", 1), ("i420", "nv21", 2), ("nv12", "nv12", 3)):
        s = Y.build(*planes, M.layout_code(src))
        before, want = M.before_and_expected(want_planes, dst, c_row_stride=1033, base=base, gap=1)
        got, info = _ycc(ctx, d, src, s, dst, before)
        _eq(got, want.buf, f"wide {src} -> {dst} base {base}")
        assert info.join


def test_past_65535_frames(ctx):
    """65537 I420 frames of 4 x 2 kept at size -> NV12: every kernel and copy of the call goes out in two groups"""
    import torch
    n = 65537
    rng = np.random.default_rng(77)
    y, cb, cr = rng.integers(0, 256, (n, 8), dtype=np.uint8), rng.integers(0, 256, (n, 2), dtype=np.uint8), rng.integers(0, 256, (n, 2), dtype=np.uint8)
    src = np.concatenate([y, cb, cr], axis=1)                       # I420, tight: 12 bytes a frame
    guard = 64
    want = rng.integers(0, 256, guard + 12 * n + guard, dtype=np.uint8)
    before = want.copy()
    body = want[guard:guard + 12 * n].reshape(n, 12)
    body[:, :8], body[:, 8:12:2], body[:, 9:12:2] = y, cb, cr       # NV12, tight
    before[guard:guard + 12 * n] ^= 0xFF
    d = L.resize_desc(4, 2, 4, 2, 3)
    x, o = torch.from_numpy(src.reshape(-1)).cuda(), torch.from_numpy(before).cuda()
    ctx.resize_ycc_to_ycc_device(d, L.ycc_source(d, "i420"), L.ycc_dest(d, "nv12"), x.data_ptr(), o.data_ptr() + guard, n, stream=_stream())
    torch.cuda.synchronize()
    info = ctx.last_ycc_out_info()
    _eq(o.cpu().numpy(), want, "65537 frames")
    assert info.join and not info.split and (info.luma_kernel, info.chroma_kernel) == (L.KERNEL_NONE, L.KERNEL_NONE), info
    assert info.launches == 1 + 1 + 1 + 2, info                     # three plane copies (one call each) and the join in two groups


def test_windows_from_ycc(ctx):
    """aligned origins with odd w and h, touching the right and the bottom edge, equal the slice of the full call; an odd
    origin is BAD_ARG for a subsampled destination and fine for 4:4:4"""
    in_w, in_h, out_w, out_h = 37, 23, 51, 31
    rng = np.random.default_rng(31)
    for src, dst in (("nv12", "nv12"), ("i420", "i422"), ("i444", "i420"), ("nv21", "i444")):
        ssub, (dsx, dsy) = M.sub_of(src), M.sub_of(dst)
        cw, ch = Y.chroma_size(in_w, in_h, *ssub)
        planes = tuple(rng.integers(0, 256, sh, dtype=np.uint8) for sh in ((FRAMES, in_h, in_w), (FRAMES, ch, cw), (FRAMES, ch, cw)))
        d = L.resize_desc(in_w, in_h, out_w, out_h, 3)
        s = Y.build(*planes, M.layout_code(src), base=1)
        ocw, och = M.out_chroma_size(out_w, out_h, dsx, dsy)
        zero = (np.zeros((FRAMES, out_h, out_w), np.uint8), np.zeros((FRAMES, och, ocw), np.uint8), np.zeros((FRAMES, och, ocw), np.uint8))
        full_b = M.build(zero, dst, seed=9)
        got, _ = _ycc(ctx, d, src, s, dst, full_b)
        full = []                                                   # the full call's planes, read back out of its buffer
        for f in range(FRAMES):
            o = full_b.at + f * full_b.frame_stride
            yo = np.stack([got[o + r * full_b.y_row_stride:][:out_w] for r in range(out_h)])
            if dst.startswith("nv"):
                rows = np.stack([got[o + full_b.cb_offset + r * full_b.c_row_stride:][:2 * ocw] for r in range(och)])
                first, second = rows[:, 0::2], rows[:, 1::2]
                cbo, cro = (first, second) if dst == "nv12" else (second, first)
            else:
                cbo = np.stack([got[o + full_b.cb_offset + r * full_b.c_row_stride:][:ocw] for r in range(och)])
                cro = np.stack([got[o + full_b.cr_offset + r * full_b.c_row_stride:][:ocw] for r in range(och)])
            full.append((yo, cbo, cro))
        full = tuple(np.stack([f[k] for f in full]) for k in range(3))
        _eq(full[0], M.ycc_to_ycc(*planes, *ssub, dsx, dsy, out_w, out_h)[0], "the full call's luma against the model")
        for win in ((2, 2, 49, 29), (0, 0, 51, 31), (4, 6, 7, 5), (50, 30, 1, 1), (48, 28, 3, 3)) + (() if dsx or dsy else ((3, 1, 5, 5),)):
            x0, y0, w, h = win
            wcw, wch = M.out_chroma_size(w, h, dsx, dsy)
            want_planes = (full[0][:, y0:y0 + h, x0:x0 + w], full[1][:, y0 >> dsy:(y0 >> dsy) + wch, x0 >> dsx:(x0 >> dsx) + wcw],
                           full[2][:, y0 >> dsy:(y0 >> dsy) + wch, x0 >> dsx:(x0 >> dsx) + wcw])
            before, want = _pitched(want_planes, dst, seed=2)
            got_w, _ = _ycc(ctx, d, src, s, dst, before, window=win)
            _eq(got_w, want.buf, f"{src} -> {dst} window {win}")
        if dsx or dsy:                                              # an odd origin: refused before anything is launched
            import torch
            odd = L.resize_window(d, (3, 1, 5, 5))
            xb, ob = torch.from_numpy(s.buf).cuda(), torch.from_numpy(full_b.buf).cuda()
            rq = L.ycc_out_request(d, L.ycc_dest(d, dst, odd, aligned=False), xb.data_ptr() + s.at, ob.data_ptr() + full_b.at, FRAMES,
                                   _src_struct(d, src, s), window=odd, in_frame_stride=s.frame_stride)
            assert L._lib().lanczos_resize_ycc_out(ctx._h, ctypes.byref(rq)) == L.ERR_BAD_ARG, dst
            torch.cuda.synchronize()
            _eq(ob.cpu().numpy(), full_b.buf, "a refused call writes nothing")


@pytest.mark.parametrize("dst", NAMES)
def test_rgb_into_every_layout(ctx, golden, d_tables, dst):
    """37 x 23 -> 22 x 14, -> 51 x 31, kept at size, 1 x 1, 2 x 1, 1 x 2 (ragged blocks of 1, 2 and 4 bytes) and one frame
    row past one workgroup of the encode (2053 x 5): Pillow's bytes in the whole buffer; kept at size, one launch"""
    sub = M.SUB_NAME[M.sub_of(dst)]
    for case in M.RGB_CASES:
        x = M.make_rgb(case)
        d = L.resize_desc(case.in_w, case.in_h, case.out_w, case.out_h, 3)
        before, want = _pitched(_planes_of(golden, case.name, sub), dst)
        same = (case.in_w, case.in_h) == (case.out_w, case.out_h)
        # frames that are read where they lie start off a dword and lie an odd stride apart
        n = case.in_w * case.in_h * 3
        fs = n + (1 if n % 2 == 0 else 2)
        raw = np.random.default_rng(1).integers(0, 256, 1 + FRAMES * fs, dtype=np.uint8)
        for f in range(FRAMES):
            raw[1 + f * fs:1 + f * fs + n] = x[f].reshape(-1)
        got, info = _rgb(ctx, d, raw, 1, fs, dst, before, d_tables["jfif"])
        _eq(got, want.buf, f"{case.name} -> {dst}")
        assert info.encode and not info.split and not info.join and info.chroma_kernel == L.KERNEL_NONE, info
        if same:
            assert info.luma_kernel == L.KERNEL_NONE and info.launches == 1, info   # no resize and no copy launch
        else:
            k = _planned_kernel(case.in_w, case.in_h, case.out_w, case.out_h, case.filt, None, None, FRAMES, channels=3)
            assert info.luma_kernel == k == L.KERNEL_RESIZE_FUSED and info.launches == 2, info


def test_rgb_clip_table_bt709_and_odd_windows(ctx, d_tables):
    """a caller's table whose sums leave [0, 16383] on both sides, in dwords whose first two pixels clip and whose next two do
    not, and the reverse; BT.709; windows at odd origins equal the model on the cropped frame; forced TWO_PASS"""
    x = M.clip_frames()
    t = M.clip_table()
    d = L.resize_desc(37, 23, 37, 23, 3)
    raw = np.ascontiguousarray(x).reshape(-1)
    for dst in NAMES:
        dsx, dsy = M.sub_of(dst)
        before, want = _pitched(M.rgb_to_ycc(x, dsx, dsy, 37, 23, t=t), dst, pad=4)   # (pad 4: luma and 4:4:4 rows on dwords)
        got, info = _rgb(ctx, d, raw, 0, 37 * 23 * 3, dst, before, d_tables["clip"])
        _eq(got, want.buf, f"clip table -> {dst}")
        assert info.launches == 1
    case = M.RGB_CASE["rgb_down"]
    x = M.make_rgb(case)
    raw = np.ascontiguousarray(x).reshape(-1)
    d = L.resize_desc(case.in_w, case.in_h, case.out_w, case.out_h, 3)
    t709 = M.forward_table(M.BT709)
    for dst in ("nv12", "i444", "i422"):
        dsx, dsy = M.sub_of(dst)
        before, want = _pitched(M.rgb_to_ycc(x, dsx, dsy, case.out_w, case.out_h, t=t709), dst)
        for path in (L.RESIZE_AUTO, L.RESIZE_TWO_PASS):
            _eq(_rgb(ctx, d, raw, 0, 0, dst, before, d_tables["bt709"], path=path)[0], want.buf, f"BT.709 -> {dst} path {path}")
        for win in ((1, 1, 9, 7), (3, 2, 4, 4), (21, 13, 1, 1), (5, 3, 17, 11)):
            before, want = _pitched(M.rgb_to_ycc(x, dsx, dsy, case.out_w, case.out_h, window=win), dst, seed=8)
            _eq(_rgb(ctx, d, raw, 0, 0, dst, before, d_tables["jfif"], window=win)[0], want.buf, f"window {win} -> {dst}")
    # kept at size with a window: a crop in front of the encode, no resize kernel
    d = L.resize_desc(37, 23, 37, 23, 3)
    x = M.make_rgb(M.RGB_CASE["rgb_same"])
    before, want = _pitched(M.rgb_to_ycc(x, 1, 1, 37, 23, window=(3, 5, 11, 9)), "nv21")
    got, info = _rgb(ctx, d, np.ascontiguousarray(x).reshape(-1), 0, 0, "nv21", before, d_tables["jfif"], window=(3, 5, 11, 9))
    _eq(got, want.buf, "a window of frames kept at size")
    assert info.luma_kernel == L.KERNEL_NONE and info.launches == 2, info


def test_host_memory_keeps_unnamed_bytes(ctx, golden):
    """the fixture's cases through memory = HOST into pitched layouts: the whole host buffer is the expected one"""
    for name, src, dst in (("420_to_420_down", "nv12", "nv12"), ("422_to_444_up", "i422", "i444"), ("444_to_420_down", "i444", "i420"),
                           ("420_to_420_same", "nv21", "i420"), ("420_to_420_same_odd", "i420", "nv12")):
        case = M.CASE[name]
        planes = M.make_planes(case)
        before, want = M.before_and_expected(_planes_of(golden, name), dst, y_row_stride=case.out_w + 3,
                                             c_row_stride=2 * _planes_of(golden, name)[1].shape[-1] + 1, base=1, gap=2)
        d = L.resize_desc(case.in_w, case.in_h, case.out_w, case.out_h, 3)
        t = _dst_struct(d, dst, before)
        n = before.frame_stride
        assert n == L.ycc_dest_frame_bytes(d, t)
        buf = before.buf.copy()
        out = buf[before.at:before.at + FRAMES * n].reshape(FRAMES, n)
        res = ctx.resize_ycc_to_ycc(M.tight(planes, src), case.in_w, case.in_h, case.out_w, case.out_h, layout=src, dest=t, out=out)
        assert res is out
        _eq(buf, want.buf, f"host {name} {src} -> {dst}")
    for cname, dst in (("rgb_down", "nv12"), ("rgb_same", "i420"), ("rgb_up", "i444"), ("rgb_1x2", "nv21")):
        case = M.RGB_CASE[cname]
        wp = _planes_of(golden, cname, M.SUB_NAME[M.sub_of(dst)])
        before, want = M.before_and_expected(wp, dst, y_row_stride=case.out_w + 1, c_row_stride=2 * wp[1].shape[-1] + 3, base=3, gap=1)
        d = L.resize_desc(case.in_w, case.in_h, case.out_w, case.out_h, 3)
        t = _dst_struct(d, dst, before)
        buf = before.buf.copy()
        out = buf[before.at:before.at + FRAMES * before.frame_stride].reshape(FRAMES, before.frame_stride)
        ctx.resize_rgb_to_ycc(M.make_rgb(case), case.out_w, case.out_h, dest=t, out=out)
        _eq(buf, want.buf, f"host {cname} -> {dst}")
    # the tight defaults: the planes back to back, nothing else
    case = M.CASE["420_to_420_down"]
    got = ctx.resize_ycc_to_ycc(M.tight(M.make_planes(case), "nv12"), case.in_w, case.in_h, case.out_w, case.out_h, "nv12", "i420")
    _eq(got, M.tight(_planes_of(golden, case.name), "i420"), "host, tight")
    got = ctx.resize_rgb_to_ycc(M.make_rgb(M.RGB_CASE["rgb_down"])[0], 22, 14, "nv12")
    _eq(got, M.tight(_planes_of(golden, "rgb_down", "420"), "nv12")[0], "host, tight, one RGB image")


def test_entry_refusals(ctx, d_tables):
    import torch
    d = L.resize_desc(37, 23, 22, 14, 3)
    t, s = L.ycc_dest(d, "nv12"), L.ycc_source(d, "nv12")
    x, o = torch.zeros(4096, dtype=torch.uint8, device="cuda"), torch.zeros(4096, dtype=torch.uint8, device="cuda")
    tab = d_tables["jfif"].data_ptr()
    call = lambda rq: L._lib().lanczos_resize_ycc_out(ctx._h, ctypes.byref(rq))
    mk = lambda dd=d, tt=t, **kw: L.ycc_out_request(dd, tt, x.data_ptr(), o.data_ptr(), 1, **kw)
    assert call(mk(source=s, table=tab)) == L.ERR_BAD_ARG           # a table from YCbCr
    assert call(mk()) == L.ERR_BAD_ARG                              # none from RGB
    assert call(mk(table=tab + 2)) == L.ERR_BAD_ARG                 # off a dword
    assert call(mk(source=s, memory=2)) == L.ERR_BAD_ARG
    assert call(mk(source=s, out_frame_stride=10)) == L.ERR_BAD_ARG and call(mk(source=s, in_frame_stride=10)) == L.ERR_BAD_ARG
    assert call(mk(source=s, memory=L.MEM_HOST, out_frame_stride=4096)) == L.ERR_BAD_ARG
    rq = mk(source=s)
    rq.reserved[2] = 1
    assert call(rq) == L.ERR_BAD_ARG
    rq = mk(source=s)
    rq.frames = 0
    assert call(rq) == L.ERR_BAD_ARG
    rq = mk(source=s)
    rq.dst = None
    assert call(rq) == L.ERR_BAD_ARG
    for kw in ({"bits": 16}, {"f32": True}):
        assert call(mk(L.resize_desc(37, 23, 22, 14, 3, **kw), source=s)) == L.ERR_UNSUPPORTED
    da = L.resize_desc(37, 23, 22, 14, 3)
    da.reserved[0] |= L.RESIZE_ALPHA
    assert call(mk(da, source=s)) == L.ERR_UNSUPPORTED
    assert call(mk(L.resize_desc(37, 23, 22, 14, 1), source=s)) == L.ERR_BAD_ARG
    bad = L.ycc_dest(d, "nv12")
    bad.c_row_stride = 21
    assert call(mk(tt=bad, source=s)) == L.ERR_BAD_ARG
    c2 = L.Context(0)
    try:
        assert c2.last_ycc_out_info() == (0, 0, False, False, False, 0)   # all zero before any call
    finally:
        c2.close()
    assert call(mk(source=s)) == L.OK
    torch.cuda.synchronize()


def test_capture_and_replay(golden):
    """one NV12 -> NV12 call and one RGB -> NV12 call captured on a context that has not seen the shapes; each replayed twice
    with rewritten inputs, an eager call of another shape in between: all outputs are the model's"""
    import torch
    case, rcase = M.CASE["420_to_420_down"], M.RGB_CASE["rgb_down"]
    c = L.Context(0)
    try:
        d = L.resize_desc(case.in_w, case.in_h, case.out_w, case.out_h, 3)
        p1, p2 = M.make_planes(case), M.make_planes(case, seed=3)
        r1, r2 = M.make_rgb(rcase), M.make_rgb(rcase, seed=3)
        want = {1: M.compose_case(case, p1), 2: M.compose_case(case, p2), 3: M.rgb_to_ycc(r1, 1, 1, 22, 14), 4: M.rgb_to_ycc(r2, 1, 1, 22, 14)}
        _eq(np.stack(want[1][1]), golden[f"{case.name}_cb"], "the model is the fixture's")
        s1, s2 = (Y.build(*p, Y.NV12, y_row_stride=40, c_row_stride=41, base=1, seed=4) for p in (p1, p2))
        bufs = {k: _pitched(v, "nv12", seed=k) for k, v in want.items()}
        x = torch.from_numpy(s1.buf).cuda()
        xr = torch.from_numpy(np.ascontiguousarray(r1).reshape(-1)).cuda()
        o = torch.from_numpy(bufs[1][0].buf).cuda()
        orgb = torch.from_numpy(bufs[3][0].buf).cuda()
        dt = torch.from_numpy(L.ycc_table_forward("jfif")).cuda()
        b = bufs[1][0]
        g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.graph(g1, stream=stream, capture_error_mode="relaxed"):
            c.resize_ycc_to_ycc_device(d, _src_struct(d, "nv12", s1), _dst_struct(d, "nv12", b), x.data_ptr() + s1.at, o.data_ptr() + b.at,
                                       FRAMES, in_frame_stride=s1.frame_stride, out_frame_stride=b.frame_stride,
                                       stream=torch.cuda.current_stream().cuda_stream)
        info = c.last_ycc_out_info()
        assert info.split and info.join and info.launches == 4, info
        with torch.cuda.graph(g2, stream=stream, capture_error_mode="relaxed"):
            c.resize_rgb_to_ycc_device(d, _dst_struct(d, "nv12", b), dt.data_ptr(), xr.data_ptr(), orgb.data_ptr() + b.at, FRAMES,
                                       out_frame_stride=b.frame_stride, stream=torch.cuda.current_stream().cuda_stream)
        info = c.last_ycc_out_info()
        assert info.encode and info.launches == 2, info
        torch.cuda.synchronize()
        _eq(o.cpu().numpy(), bufs[1][0].buf, "captured, not run")

        def replay(graph, dev, key):
            dev.copy_(torch.from_numpy(bufs[key][0].buf))
            graph.replay()
            torch.cuda.synchronize()
            _eq(dev.cpu().numpy(), bufs[key][1].buf, f"replay {key}")
        replay(g1, o, 1)
        replay(g2, orgb, 3)
        big = M.CASE["420_to_420_gap2"]                               # eager, larger planes: the scratch blocks are replaced
        pb = M.make_planes(big)
        _eq(c.resize_ycc_to_ycc(M.tight(pb, "nv12"), big.in_w, big.in_h, 60, 40, "nv12", "nv12"),
            M.tight(M.ycc_to_ycc(*pb, 1, 1, 1, 1, 60, 40), "nv12"), "eager after the capture")
        _eq(c.resize_rgb_to_ycc(M.make_rgb(M.RGB_CASE["rgb_up"]), 60, 40, "i420"),
            M.tight(M.rgb_to_ycc(M.make_rgb(M.RGB_CASE["rgb_up"]), 1, 1, 60, 40), "i420"), "eager RGB after the capture")
        x.copy_(torch.from_numpy(s2.buf))
        xr.copy_(torch.from_numpy(np.ascontiguousarray(r2).reshape(-1)))
        replay(g1, o, 2)
        replay(g2, orgb, 4)
        del g1, g2
    finally:
        c.close()
