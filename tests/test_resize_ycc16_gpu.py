"""GPU checks of lanczos_resize_ycc16: YCbCr frames of 16-bit words (P010 / P016 / P210-shaped pairs in either order, planes of
4:2:0, 4:2:2 and 4:4:4) into wide YCbCr frames, packed RGB words and normalised tensor elements.  The yardsticks are Pillow's
committed fixture (tests/golden/resize_pillow_ycc16.npz: every plane resized as mode I;16), the numpy model that reproduces it
(tests/resize_ycc16_model.py) and three Context.resize calls on the planes.  Every call writes into a whole buffer with noise
or sentinels in everything it must not write; the whole buffer is compared.

Launch counts of fused plans: planar -> planar 3, pairs -> planar 4 (the split), planar -> pairs 4 (the join), pairs -> pairs 4
(luma, split, one chroma call of 2 * frames frames, join); into RGB words or elements planar 4 (three planes and the merge),
pairs 4 (luma, split, one chroma call, merge)."""
import ctypes
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_tensor_norm_model as TN
import resize_ycc16_model as M
import resize_ycc16_run as R
from resize_ycc16_run import eq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = M.FRAMES
NAMES = [c.name for c in M.CASES]
BT2020_10 = M.matrix(M.BT2020, 10, True, False)


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.resize_force(L.RESIZE_AUTO)
    c.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "resize_pillow_ycc16.npz"))


def _layouts(sub):
    """the layouts of a subsampling: planes, and where chroma is halved across, pairs in either order"""
    return [M.SUB_PLANAR[sub]] + ([M.SUB_PAIRS[sub], M.SUB_PAIRS_SWAPPED[sub]] if sub[0] else [])


def _pairs(name):
    return M.layout_code(name) != M.PLANAR


def _source(case, planes, layout, k=0):
    """pitched source frames: a luma pitch of odd words (2 mod 4 bytes), the base at residue 0 or 2 mod 4 in turn"""
    cw = planes[1].shape[-1]
    crow = 2 * cw if _pairs(layout) else cw
    return M.build(*planes, M.layout_code(layout), y_row_stride=(case.in_w + 3) | 1, c_row_stride=crow + 1 + (k & 1), base=k & 1,
                   gap=1 + (k & 1), frame_gap=1, seed=3 + k)


def _dest(want_planes, layout, k=0, seed=5):
    w, cw = want_planes[0].shape[-1], want_planes[1].shape[-1]
    crow = 2 * cw if _pairs(layout) else cw
    return M.expected_dest(want_planes, layout, seed=seed, y_row_stride=(w + 2) | 1, c_row_stride=crow + 2 - (k & 1), base=(k + 1) & 1,
                           gap=1, frame_gap=1)


def _chroma_kernels(case, src, dst, window, frames=FRAMES):
    """(luma, chroma) kernels the plan predicts for a case into YCbCr (dst a layout) or into RGB (dst None)"""
    cw, ch = M.chroma_size(case.in_w, case.in_h, case.ssx, case.ssy)
    bc = M.chroma_box(case.box, case.in_w, case.in_h, case.ssx, case.ssy)
    k_luma = R.planned_kernel(case.in_w, case.in_h, case.out_w, case.out_h, case.filt, case.box, frames, window)
    if dst is None:
        ocw, och, cwin, one_call = case.out_w, case.out_h, window, _pairs(src)
    else:
        dsx, dsy = M.sub_of(dst)
        ocw, och = M.out_chroma_size(case.out_w, case.out_h, dsx, dsy)
        cwin = None
        if window is not None:
            x0, y0, w, h = window
            cwin = (x0 >> dsx, y0 >> dsy) + M.out_chroma_size(w, h, dsx, dsy)
        one_call = _pairs(src) and _pairs(dst)
    return k_luma, R.planned_kernel(cw, ch, ocw, och, case.filt, bc, 2 * frames if one_call else frames, cwin)


_three = {}


def _three_resizes(ctx, case, planes):
    """three Context.resize calls on one-channel uint16 planes, composed in numpy: (Yo, Cbo, Cro, dCbo, dCro), uncut"""
    if case.name not in _three:
        y, cb, cr = planes
        bc = M.chroma_box(case.box, case.in_w, case.in_h, case.ssx, case.ssy)
        ocw, och = M.out_chroma_size(case.out_w, case.out_h, case.dsx, case.dsy)
        one = lambda p, ow, oh, b: ctx.resize(p[..., None], ow, oh, box=b, filter=case.filt)[..., 0]
        _three[case.name] = (one(y, case.out_w, case.out_h, case.box), one(cb, case.out_w, case.out_h, bc), one(cr, case.out_w, case.out_h, bc),
                             one(cb, ocw, och, bc), one(cr, ocw, och, bc))
    return _three[case.name]


@pytest.mark.parametrize("name", NAMES)
def test_every_case_into_ycc(ctx, golden, name):
    """every fixture case from every layout of its subsampling into every layout of the destination's: Pillow's planes in the
    whole buffer, the kernels the plan predicts, split only from pairs, join only into pairs, the launch counts of fused plans"""
    case = M.CASE[name]
    planes = M.make_planes(case)
    want_planes = M.golden_planes(golden, case, "ycc")
    d = R.desc(case.in_w, case.in_h, case.out_w, case.out_h, case.filt)
    k = 0
    for src in _layouts((case.ssx, case.ssy)):
        for dst in _layouts((case.dsx, case.dsy)):
            s = _source(case, planes, src, k)
            before, want = _dest(want_planes, dst, k)
            got, info = R.to_ycc(ctx, d, src, s, dst, before, window=case.window, box=case.box)
            eq(got, want.buf, f"{name} {src} -> {dst}: the whole buffer against Pillow")
            k_luma, k_chroma = _chroma_kernels(case, src, dst, case.window)
            assert (info.luma_kernel, info.chroma_kernel) == (k_luma, k_chroma), (src, dst, info, k_luma, k_chroma)
            assert info.split == _pairs(src) and info.join == _pairs(dst) and not info.merge, (src, dst, info)
            if k_luma == k_chroma == L.KERNEL_RESIZE_FUSED:
                assert info.launches == (4 if _pairs(src) or _pairs(dst) else 3), (src, dst, info)
            k += 1
    uncut = _three_resizes(ctx, case, planes)
    for g, key in zip(uncut, ("y", "cb", "cr", "dcb", "dcr")):
        eq(g, golden[f"{name}_{key}"], f"{name}: three uint16 resizes against Pillow ({key})")


@pytest.mark.parametrize("name", NAMES)
def test_every_case_into_rgb_and_tensor(ctx, golden, name):
    """... into packed RGB words and into float32 CHW elements, through the BT.2020 10-bit matrix: the model's conversion of
    Pillow's planes, in whole buffers"""
    case = M.CASE[name]
    planes = M.make_planes(case)
    rgb = M.rgb16(BT2020_10, M.golden_planes(golden, case, "rgb"))
    d = R.desc(case.in_w, case.in_h, case.out_w, case.out_h, case.filt)
    for k, src in enumerate(_layouts((case.ssx, case.ssy))):
        s = _source(case, planes, src, k)
        got, want, info = R.to_rgb(ctx, d, src, s, BT2020_10, rgb, window=case.window, box=case.box)
        eq(got, want, f"{name} {src} -> RGB words")
        kernels = _chroma_kernels(case, src, None, case.window)
        assert (info.luma_kernel, info.chroma_kernel) == kernels and info.split == _pairs(src) and info.merge and not info.join, (src, info, kernels)
        if kernels == (L.KERNEL_RESIZE_FUSED, L.KERNEL_RESIZE_FUSED):
            assert info.launches == 4, (src, info)       # planes: 3 + merge; pairs: luma, split, one chroma call, merge
        got, want, info2 = R.to_tensor(ctx, d, src, s, BT2020_10, rgb, mean=(0.4, 0.5, 0.3), std=(0.2, 0.25, 0.3), window=case.window,
                                       box=case.box)
        eq(got, want, f"{name} {src} -> float32 CHW")
        assert info2 == info, (info, info2)


@pytest.mark.parametrize("name,path", [("420_down_odd", L.RESIZE_TWO_PASS), ("444_up", L.RESIZE_TWO_PASS), ("420_box", L.RESIZE_TWO_PASS),
                                       ("420_window", L.RESIZE_TWO_PASS), ("420_to_444", L.RESIZE_CONVERT)])
def test_forced_paths(ctx, golden, name, path):
    case = M.CASE[name]
    planes = M.make_planes(case)
    d = R.desc(case.in_w, case.in_h, case.out_w, case.out_h, case.filt)
    src, dst = _layouts((case.ssx, case.ssy))[-1], _layouts((case.dsx, case.dsy))[-1]
    s = _source(case, planes, src, 1)
    before, want = _dest(M.golden_planes(golden, case, "ycc"), dst, 0)
    got, info = R.to_ycc(ctx, d, src, s, dst, before, window=case.window, box=case.box, path=path)
    eq(got, want.buf, f"{name} {src} -> {dst} path {path}")
    if path == L.RESIZE_TWO_PASS:
        assert L.KERNEL_RESIZE_FUSED not in (info.luma_kernel, info.chroma_kernel), info
    rgb = M.rgb16(BT2020_10, M.golden_planes(golden, case, "rgb"))
    got, want, info = R.to_tensor(ctx, d, src, s, BT2020_10, rgb, dtype="bfloat16", window=case.window, box=case.box, path=path)
    eq(got, want, f"{name} {src} -> bfloat16 path {path}")
    if path == L.RESIZE_TWO_PASS:
        assert L.KERNEL_RESIZE_FUSED not in (info.luma_kernel, info.chroma_kernel) and info.merge, info


def test_five_frames_at_an_odd_word_stride(ctx):
    """five P010-shaped frames whose stride is an odd multiple of 2 bytes on both sides, into pairs and into planes"""
    case = M.CASE["420_down_odd"]
    planes = M.make_planes(case, frames=5, seed=2)
    want_planes = M.case_planes_ycc(case, planes)
    d = R.desc(case.in_w, case.in_h, case.out_w, case.out_h)
    for src, dst in (("p010", "p016"), ("nv21", "i420"), ("i420", "nv21")):
        s = M.build(*planes, M.layout_code(src), y_row_stride=case.in_w + 2, base=1, frame_gap=0)
        s = s if s.frame_stride & 1 else M.build(*planes, M.layout_code(src), y_row_stride=case.in_w + 2, base=1, frame_gap=1)
        before, want = M.expected_dest(want_planes, dst, y_row_stride=case.out_w + 1, frame_gap=0)
        if not before.frame_stride & 1:
            before, want = M.expected_dest(want_planes, dst, y_row_stride=case.out_w + 1, frame_gap=1)
        assert s.frame_stride & 1 and before.frame_stride & 1
        got, info = R.to_ycc(ctx, d, src, s, dst, before, frames=5)
        eq(got, want.buf, f"five frames {src} -> {dst}")
        assert info.split == _pairs(src) and info.join == _pairs(dst)
    rgb = M.rgb16(BT2020_10, M.case_planes_rgb(case, planes))
    s = M.build(*planes, M.NV12, y_row_stride=case.in_w + 2, base=1, frame_gap=0)
    s = s if s.frame_stride & 1 else M.build(*planes, M.NV12, y_row_stride=case.in_w + 2, base=1, frame_gap=1)
    got, want, _ = R.to_rgb(ctx, d, "p010", s, BT2020_10, rgb)
    eq(got, want, "five frames -> RGB words (741 words a frame: a tail of one pixel and a noise word behind it)")
    got, want, _ = R.to_tensor(ctx, d, "p010", s, BT2020_10, rgb, flips=[0, 1, 2, 3, 1])
    eq(got, want, "five frames -> elements, a flip per frame")


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_elements_maps_flips_and_sentinels(ctx, golden, dtype, layout):
    """float32 / bfloat16 / float16, CHW / HWC with a sentinel between any two elements, a reversing map and a two-channel map,
    flips from the struct and from d_flip: the three float operations on the RGB words, bit for bit"""
    case = M.CASE["420_up_bicubic"]
    planes = M.make_planes(case)
    rgb = M.rgb16(BT2020_10, M.golden_planes(golden, case, "rgb"))
    d = R.desc(case.in_w, case.in_h, case.out_w, case.out_h, case.filt)
    s = _source(case, planes, "p010", 1)
    h, w = rgb.shape[1:3]
    for src, flip, flips in (((0, 1, 2), 0, None), ((2, 1, 0), 1, None), ((2, 0), 2, [1, 2]), ((1,), 3, [3, 0])):
        c = len(src)
        st = ((2 * w + 1) * h + 5, 2 * w + 1, 2) if layout == "chw" else (1, (w + 1) * (c + 1), c + 1)   # gaps everywhere
        got, want, info = R.to_tensor(ctx, d, "p010", s, BT2020_10, rgb, div=(65535.0, 1023.0, 255.0)[:c], mean=(0.485, 0.456, 0.406)[:c],
                                      std=(0.229, 0.224, 0.225)[:c], dtype=dtype, src=src, flip=flip, flips=flips, strides=st)
        eq(got, want, f"{dtype} {layout} map {src} flip {flip} d_flip {flips}")
        assert info.merge and info.split and info.launches == 4, info
        assert (want == R.SENTINEL[dtype]).sum() >= want.size // 5      # kept sentinels: at least one beside every HWC pixel of 3


def test_host_memory_all_three_kinds(ctx, golden):
    """memory = HOST through the array forms: tight frames in, tight frames / RGB words / elements out; a caller's destination
    buffer keeps its unnamed words"""
    case = M.CASE["420_down_odd"]
    planes = M.make_planes(case)
    for src, dst in (("p010", "p010"), ("i420", "nv21"), ("nv21", "i420")):
        got = ctx.resize_ycc16_to_ycc(M.tight(*planes, src), case.in_w, case.in_h, case.out_w, case.out_h, src, dst)
        eq(got, M.tight(*M.golden_planes(golden, case, "ycc"), dst), f"host {src} -> {dst}")
    info = ctx.last_ycc16_info()
    assert info.split and not info.join and not info.merge, info
    rgb = M.rgb16(M.matrix(M.BT709, 10, True, False), M.golden_planes(golden, case, "rgb"))
    got = ctx.resize_ycc16_rgb(M.tight(*planes, "p010"), case.in_w, case.in_h, case.out_w, case.out_h)   # the default matrix: BT.709, P010
    eq(got, rgb, "host -> RGB words (19 x 13: frames of an odd number of words, back to back)")
    got = ctx.resize_ycc16_rgb(M.tight(*planes, "p010")[0], case.in_w, case.in_h, case.out_w, case.out_h)
    eq(got, rgb[0], "host, one frame")
    for dtype in ("float32", "bfloat16", "float16"):
        got = ctx.resize_ycc16_tensor(M.tight(*planes, "i420"), case.in_w, case.in_h, case.out_w, case.out_h, "i420", mean=0.45, std=0.225,
                                      dtype=dtype, tensor_layout="hwc", channels_out=(2, 1, 0), flip=[1, 2])
        want = TN.norm(rgb, 65535.0, 0.45, 0.225, dtype, (2, 1, 0), [1, 2], "hwc")
        assert TN.same_bits(got, want, dtype), dtype
    # a pitched destination in host memory: the whole buffer
    want_planes = M.golden_planes(golden, case, "ycc")
    before, want = M.expected_dest(want_planes, "p010", y_row_stride=case.out_w + 2, c_row_stride=2 * want_planes[1].shape[-1] + 1, base=1,
                                   gap=1)                              # (host frames lie one extent apart: no gap between them)
    d = R.desc(case.in_w, case.in_h, case.out_w, case.out_h)
    t = R.dst_struct(d, "p010", before)
    n = before.frame_stride
    assert 2 * n == L.ycc_dest_frame_bytes(d, t)
    buf = before.buf.copy()
    out = buf[before.at:before.at + FRAMES * n].reshape(FRAMES, n)
    assert ctx.resize_ycc16_to_ycc(M.tight(*planes, "i420"), case.in_w, case.in_h, case.out_w, case.out_h, "i420", dest=t, out=out) is out
    eq(buf, want.buf, "host, a pitched destination")


def test_entry_refusals_write_nothing(ctx):
    import torch
    d = R.desc(37, 23, 19, 13)
    s, t, m = L.ycc16_source(d, "p010"), L.ycc16_dest(d, "p010"), L.ycc16_matrix()
    x, o = torch.zeros(8192, dtype=torch.int16, device="cuda"), torch.full((8192,), 77, dtype=torch.int16, device="cuda")
    call = lambda rq: L._lib().lanczos_resize_ycc16(ctx._h, ctypes.byref(rq))
    mk = lambda dd=d, **kw: L.ycc16_request(dd, s, x.data_ptr(), o.data_ptr(), 1, **kw)
    n = L.tensor_norm(TN.strides("chw", 19, 13, 3))
    assert call(mk()) == L.ERR_BAD_ARG and call(mk(dest=t, matrix=m)) == L.ERR_BAD_ARG and call(mk(dest=t, norm=n)) == L.ERR_BAD_ARG
    assert call(mk(norm=n)) == L.ERR_BAD_ARG
    assert call(mk(dest=t, in_frame_stride=10)) == L.ERR_BAD_ARG and call(mk(dest=t, out_frame_stride=10)) == L.ERR_BAD_ARG
    assert call(mk(dest=t, out_frame_stride=2 * 4096 + 1)) == L.ERR_BAD_ARG and call(mk(matrix=m, out_frame_stride=2 * 4096 + 2)) == L.ERR_BAD_ARG
    rq = mk(dest=t)
    rq.out = o.data_ptr() + 1
    assert call(rq) == L.ERR_BAD_ARG
    rq = mk(matrix=m)
    rq.out = o.data_ptr() + 2
    assert call(rq) == L.ERR_BAD_ARG
    assert call(mk(L.resize_desc(37, 23, 19, 13, 3), dest=t)) == L.ERR_UNSUPPORTED                   # no LANCZOS_RESIZE_U16
    assert call(mk(dest=t, opts=L.resize_opts(L.resize_desc(37, 23, 19, 13, 3), None, 2.0))) == L.ERR_BAD_ARG   # a reducing_gap
    torch.cuda.synchronize()
    assert bool((o == 77).all()), "a refused call writes nothing"
    c2 = L.Context(0)
    try:
        assert c2.last_ycc16_info() == (0, 0, False, False, False, 0)
    finally:
        c2.close()
    assert call(mk(dest=t)) == L.OK
    torch.cuda.synchronize()


def test_capture_and_replay_with_rewritten_input_and_flips(golden):
    """one P010 -> bfloat16 CHW call captured on a context that has not seen the shape, replayed with rewritten frames and
    rewritten d_flip bytes, an eager call of another shape in between"""
    import torch
    case = M.CASE["420_down_odd"]
    c = L.Context(0)
    try:
        d = R.desc(case.in_w, case.in_h, case.out_w, case.out_h)
        p1, p2 = M.make_planes(case), M.make_planes(case, seed=3)
        rgb1 = M.rgb16(BT2020_10, M.golden_planes(golden, case, "rgb"))
        rgb2 = M.rgb16(BT2020_10, M.case_planes_rgb(case, p2))
        s1, s2 = (M.build(*p, M.NV12, y_row_stride=39, c_row_stride=41, base=1, seed=4) for p in (p1, p2))
        st = TN.strides("chw", case.out_w, case.out_h, 3)
        f1, f2 = [0, 3], [2, 1]
        b1 = R.tensor_buffers(rgb1, 65535.0, 0.5, 0.25, "bfloat16", (0, 1, 2), f1, st)
        b2 = R.tensor_buffers(rgb2, 65535.0, 0.5, 0.25, "bfloat16", (0, 1, 2), f2, st)
        x, o = R.dev(s1.buf), R.dev(b1[0])
        flips = torch.tensor(f1, dtype=torch.uint8, device="cuda")
        n = L.tensor_norm(st, 65535.0, 0.5, 0.25, "bfloat16", (0, 1, 2), 0, flips.data_ptr())
        g = torch.cuda.CUDAGraph()
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="relaxed"):
            c.resize_ycc16_tensor_device(d, R.src_struct(d, "p010", s1), M.matrix_struct(L, BT2020_10), n, x.data_ptr() + 2 * s1.at,
                                         o.data_ptr() + 2 * b1[2], FRAMES, in_frame_stride=2 * s1.frame_stride, out_frame_stride=2 * b1[3],
                                         stream=torch.cuda.current_stream().cuda_stream)
        info = c.last_ycc16_info()
        assert info.split and info.merge and info.launches == 4, info
        torch.cuda.synchronize()
        eq(R.back(o, np.uint16), b1[0], "captured, not run")
        g.replay()
        torch.cuda.synchronize()
        eq(R.back(o, np.uint16), b1[1], "first replay")
        big = M.CASE["444_up"]                                      # eager, larger planes: the scratch blocks are replaced
        pb = M.make_planes(big)
        eq(c.resize_ycc16_to_ycc(M.tight(*pb, "i444"), big.in_w, big.in_h, 80, 48, "i444", "i444"),
           M.tight(*M.planes_ycc(*pb, 0, 0, 0, 0, 80, 48), "i444"), "eager after the capture")
        x.copy_(R.dev(s2.buf))
        flips.copy_(torch.tensor(f2, dtype=torch.uint8))
        o.copy_(R.dev(b2[0]))
        g.replay()
        torch.cuda.synchronize()
        eq(R.back(o, np.uint16), b2[1], "second replay: rewritten frames and flips")
        del g
    finally:
        c.close()
