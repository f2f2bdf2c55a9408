"""GPU checks of lanczos_resize_ycc_* (YCbCr frames with subsampled chroma into RGB bytes and tensors).  The yardsticks are
Pillow's committed fixture (tests/golden/resize_pillow_ycc.npz: three "L" resizes, Image.merge("YCbCr") and convert("RGB")), the
numpy model that reproduces it (tests/resize_ycc_model.py), and the composition the contract names: three Context.resize calls
on the planes (themselves pinned to Pillow) merged in numpy.  Everything is compared as bytes or bit patterns; the frames come
from the model's builders with noise in every byte a layout does not name, and the outputs lie between sentinels."""
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_tensor16_model as T16
import resize_tensor_model as T32
import resize_tensor_view_model as V
import resize_ycc_model as Y
from resize_ycc_run import _bytes, _desc, _eq, _source, _tensor

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.resize_force(L.RESIZE_AUTO)
    c.close()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "resize_pillow_ycc.npz"))


@pytest.fixture(scope="module")
def d_jfif():
    import torch
    return torch.from_numpy(L.ycc_table("jfif")).cuda()


def _three_resizes(ctx, case, y, cb, cr, window=None, path=L.RESIZE_AUTO):
    """the composition the contract names: three Context.resize calls on the planes, merged in numpy.  Returns the RGB bytes
    and the kernels the luma and the chroma call ran"""
    bc = Y.chroma_box(case.box, case.in_w, case.in_h, case.sx, case.sy)
    ctx.resize_force(path)
    try:
        kw = dict(reducing_gap=case.gap, filter=case.filt, window=window)
        yo = ctx.resize(y[..., None], case.out_w, case.out_h, box=case.box, **kw)[..., 0]
        k_luma = ctx.last_kernel()
        cbo = ctx.resize(cb[..., None], case.out_w, case.out_h, box=bc, **kw)[..., 0]
        cro = ctx.resize(cr[..., None], case.out_w, case.out_h, box=bc, **kw)[..., 0]
        k_chroma = ctx.last_kernel()
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    return Y.convert(Y.table(Y.JFIF), yo, cbo, cro), k_luma, k_chroma


def _planned_kernel(in_w, in_h, out_w, out_h, filt, box, gap, frames, window=None):
    """the kernel lanczos_resize_window_plan_host predicts for a one-channel plane under AUTO (None: no pass runs)"""
    d = L.resize_desc(in_w, in_h, out_w, out_h, 1, filter=filt)
    p = L.resize_window_plan_host(d, window, frames, box=box if box is not None else (0, 0, in_w, in_h), reducing_gap=gap)
    if not (p.pass_h or p.pass_v):
        return None
    if filt == "nearest":
        return L.KERNEL_RESIZE_NEAREST
    return L.KERNEL_RESIZE_FUSED if p.inner.fused else L.KERNEL_RESIZE_TWO_PASS


@pytest.mark.parametrize("case", Y.CASES, ids=[c.name for c in Y.CASES])
def test_planar_frames_against_pillow_and_the_composition(ctx, golden, d_jfif, case):
    """every case of the fixture as tight planes (I420 / 4:2:2 / 4:4:4): Pillow's bytes, the model's, the three resizes';
    the kernels per plane are those the plan predicts; forced TWO_PASS gives the same bytes"""
    frames = 2
    y, cb, cr = Y.make_planes(case, frames)
    want = golden[f"{case.name}_out"]
    assert np.array_equal(Y.compose(y, cb, cr, case.sx, case.sy, case.out_w, case.out_h, case.filt, case.box, case.gap), want)
    s = Y.build(y, cb, cr, Y.PLANAR)
    got = _bytes(ctx, case, s, frames, d_jfif)
    info = ctx.last_ycc_info()
    _eq(got, want, f"{case.name} against Pillow")
    comp, k_luma, k_chroma = _three_resizes(ctx, case, y, cb, cr)
    _eq(got, comp, f"{case.name} against three resizes")
    # routes: no split for planes; per plane the kernel of the one-channel request, which is the plan's
    cw, ch = Y.chroma_size(case.in_w, case.in_h, case.sx, case.sy)
    bc = Y.chroma_box(case.box, case.in_w, case.in_h, case.sx, case.sy)
    p_luma = _planned_kernel(case.in_w, case.in_h, case.out_w, case.out_h, case.filt, case.box, case.gap, frames)
    p_chroma = _planned_kernel(cw, ch, case.out_w, case.out_h, case.filt, bc, case.gap, frames)
    # (a plane no pass runs on is a plain copy: the report names no kernel for it, KERNEL_NONE)
    want_k = tuple(L.KERNEL_NONE if p is None else k for p, k in ((p_luma, k_luma), (p_chroma, k_chroma)))
    assert not info.split and (info.luma_kernel, info.chroma_kernel) == want_k, (info, k_luma, k_chroma)
    assert (p_luma or L.KERNEL_NONE) == info.luma_kernel and (p_chroma or L.KERNEL_NONE) == info.chroma_kernel, (info, p_luma, p_chroma)
    if case.name == "i420_same":
        assert p_luma is None and p_chroma is not None          # luma is a copy, chroma still resizes
    if case.name == "i444_up":
        assert p_luma == p_chroma == L.KERNEL_RESIZE_FUSED      # the upscale runs the fused kernel
    if p_luma == p_chroma == L.KERNEL_RESIZE_FUSED and case.gap is None:
        assert info.launches == 4, info                         # three tight planes, one launch each, and the merge
    assert info.launches >= 3
    if case.filt != "nearest":
        _eq(_bytes(ctx, case, s, frames, d_jfif, path=L.RESIZE_TWO_PASS), want, f"{case.name} forced TWO_PASS")
        forced = ctx.last_ycc_info()
        assert forced.luma_kernel != L.KERNEL_RESIZE_FUSED and forced.chroma_kernel != L.KERNEL_RESIZE_FUSED, forced


@pytest.mark.parametrize("layout", [Y.NV12, Y.NV21], ids=["nv12", "nv21"])
def test_interleaved_chroma_pitched_at_every_residue(ctx, golden, d_jfif, layout):
    """NV12 / NV21 at 37 x 23 with y_row_stride 48 and c_row_stride 44, the frame base at residues 0 .. 3, gaps of 0 .. 3 bytes
    in front of the chroma plane and one byte between frames: the split reads rows that start at every residue; noise in every byte the
    layout does not name, of two kinds, which must not reach the result"""
    case = Y.CASE["i420_down"]
    frames = 2
    y, cb, cr = Y.make_planes(case, frames)
    want = golden["i420_down_out"]
    rows = set()
    for base in range(4):
        for seed in (1, 2):
            s = Y.build(y, cb, cr, layout, y_row_stride=48, c_row_stride=44, base=base, gap=(base + 1) % 4, frame_gap=1,
                        seed=seed)
            rows |= {(s.at + f * s.frame_stride + s.cb_offset + r * 44) % 4 for f in range(frames) for r in range(12)}
            _eq(_bytes(ctx, case, s, frames, d_jfif), want, f"layout {layout} base {base} seed {seed}")
            info = ctx.last_ycc_info()
            assert info.split and info.luma_kernel == info.chroma_kernel == L.KERNEL_RESIZE_FUSED, info
            assert info.launches == 4, info                      # luma, split, both chroma planes in one call, merge
    assert rows == {0, 1, 2, 3}
    # a tight NV frame with an odd chroma width: rows of 38 bytes, every second one off a dword
    s = Y.build(y, cb, cr, layout)
    _eq(_bytes(ctx, case, s, frames, d_jfif), want, f"layout {layout} tight")
    # the other fixture cases with 4:2:0 chroma, split: the upscale, the box, NEAREST and the gap
    for name in ("i420_up_bicubic", "i420_box", "i420_nearest", "i420_gap2_both", "i420_same", "i420_1x1"):
        c2 = Y.CASE[name]
        p = Y.make_planes(c2, frames)
        _eq(_bytes(ctx, c2, Y.build(*p, layout, c_row_stride=2 * ((c2.in_w + 1) // 2) + 3, base=1, gap=2), frames, d_jfif),
            golden[f"{name}_out"], f"layout {layout} {name}")
        assert ctx.last_ycc_info().split


def test_window_that_starts_at_an_odd_pixel(ctx, golden, d_jfif):
    for name, win in (("i420_down", (3, 1, 13, 9)), ("i444_up", (7, 5, 21, 17)), ("i420_same", (1, 3, 35, 19)),
                      ("i420_nearest", (5, 1, 9, 11)), ("i420_down", (18, 12, 1, 1))):
        case = Y.CASE[name]
        y, cb, cr = Y.make_planes(case, 2)
        x0, y0, w, h = win
        want = golden[f"{name}_out"][:, y0:y0 + h, x0:x0 + w]
        for layout in (Y.PLANAR, Y.NV12) if case.sx else (Y.PLANAR,):
            s = Y.build(y, cb, cr, layout, y_row_stride=case.in_w + 3, base=3)
            got = _bytes(ctx, case, s, 2, d_jfif, window=win)
            _eq(got, want, f"{name} window {win} layout {layout}")
            _eq(got, _three_resizes(ctx, case, y, cb, cr, window=win)[0], f"{name} window {win}: three resizes")


def test_batch_with_an_odd_frame_stride(ctx, d_jfif):
    """five frames whose stride on the input side is no dword multiple, so that every frame has another residue"""
    case = Y.CASE["i420_down"]
    frames = 5
    y, cb, cr = Y.make_planes(case, frames, seed=3)
    want = Y.compose(y, cb, cr, 1, 1, case.out_w, case.out_h)
    for layout in (Y.PLANAR, Y.NV12, Y.NV21):
        s = Y.build(y, cb, cr, layout, y_row_stride=case.in_w + 2, frame_gap=0 if layout == Y.PLANAR else 2, base=2)
        assert s.frame_stride % 4 and len({(s.at + f * s.frame_stride) % 4 for f in range(frames)}) == 4
        got = _bytes(ctx, case, s, frames, d_jfif, pad=1)
        _eq(got, want, f"layout {layout}")
        _eq(got, _three_resizes(ctx, case, y, cb, cr)[0], f"layout {layout}: three resizes")


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_tensor_outputs(ctx, golden, d_jfif, dtype):
    """CHW and HWC, tight and with gaps between rows, planes and elements; a reversing and a two-channel map; flips 0 .. 3 per
    frame from d_flip, and one flip for every frame from the struct; on a tail of 3 pixels, a window and an upscale"""
    frames = 4
    lut_of = (lambda oc: T32.identity_lut(oc)) if dtype == "float32" else (lambda oc: T16.identity_lut16(oc))
    for name, win in (("i420_down", None), ("i420_down", (3, 1, 13, 9)), ("i444_up", None)):
        case = Y.CASE[name]
        y, cb, cr = Y.make_planes(case, frames, seed=5)
        ref = Y.compose(y, cb, cr, case.sx, case.sy, case.out_w, case.out_h, case.filt, case.box, case.gap, window=win)
        _, h, w, _ = ref.shape
        s = Y.build(y, cb, cr, Y.NV12 if case.sx else Y.PLANAR, y_row_stride=case.in_w + 1, base=1)
        for src in ((0, 1, 2), (2, 1, 0), (2, 0)):
            oc = len(src)
            layouts = {"chw": V.strides("chw", w, h, oc), "hwc": V.strides("hwc", w, h, oc),
                       "chw padded": (h * (w + 3) + 5, w + 3, 1), "hwc gaps": (1, w * (oc + 2) + 1, oc + 2)}
            for lname, st in layouts.items():
                _tensor(ctx, case, s, frames, d_jfif, ref, lut_of(oc), src, [0, 1, 2, 3], st, dtype, window=win)
        for m in (1, 2, 3):      # a flip for every frame, from the host struct alone
            _tensor(ctx, case, s, frames, d_jfif, ref, lut_of(3), (0, 1, 2), [m] * frames, V.strides("chw", w, h, 3), dtype,
                    window=win, host_flip=m)
    # Pillow's bytes through the table, directly
    case = Y.CASE["i420_edges_down"]
    y, cb, cr = Y.make_planes(case, 2)
    _tensor(ctx, case, Y.build(y, cb, cr), 2, d_jfif, golden["i420_edges_down_out"], lut_of(3), (0, 1, 2), [0, 3],
            V.strides("chw", case.out_w, case.out_h, 3), dtype)


def test_host_entries_and_standards(ctx, golden):
    """Context.resize_ycc / resize_ycc_tensor on tight frames of every named layout, and the limited-range tables"""
    for name, layouts in (("i420_down", ("i420", "nv12", "nv21")), ("i422_down", ("i422",)), ("i444_up", ("i444",)),
                          ("i420_gap2_luma", ("i420", "nv12")), ("i420_box", ("nv12",))):
        case = Y.CASE[name]
        y, cb, cr = Y.make_planes(case, 2)
        want = golden[f"{name}_out"]
        for lay in layouts:
            code = {"nv12": Y.NV12, "nv21": Y.NV21}.get(lay, Y.PLANAR)
            fr = Y.tight(y, cb, cr, code)
            kw = dict(layout=lay, filter=case.filt, box=case.box, reducing_gap=case.gap)
            _eq(ctx.resize_ycc(fr, case.in_w, case.in_h, case.out_w, case.out_h, **kw), want, f"host {name} {lay}")
            _eq(ctx.resize_ycc(fr[1], case.in_w, case.in_h, case.out_w, case.out_h, **kw), want[1], f"host {name} {lay}: one frame")
            assert ctx.last_ycc_info().split == (lay in ("nv12", "nv21"))
    case = Y.CASE["i420_down"]
    y, cb, cr = Y.make_planes(case, 3, seed=2)
    fr = Y.tight(y, cb, cr, Y.NV12)
    planes = Y.resize_planes(y, cb, cr, 1, 1, case.out_w, case.out_h)
    for std, code in (("bt601", Y.BT601), ("bt709", Y.BT709)):
        _eq(ctx.resize_ycc(fr, case.in_w, case.in_h, case.out_w, case.out_h, standard=std), Y.convert(Y.table(code), *planes), std)
    bgr = np.ascontiguousarray(L.ycc_table("jfif")[::-1])                   # the caller's own table: BGR rows
    _eq(ctx.resize_ycc(fr, case.in_w, case.in_h, case.out_w, case.out_h, table=bgr), Y.convert(Y.table(Y.JFIF), *planes)[..., ::-1], "bgr")
    ref = Y.convert(Y.table(Y.JFIF), *planes)
    win = (3, 1, 13, 9)
    refw = ref[:, 1:10, 3:16]
    for dt in ("float32", "float16"):
        for kw, r in (({}, ref), ({"channels_out": (2, 0), "flip": [1, 2, 3]}, ref), ({"window": win, "tensor_layout": "hwc", "flip": "h"}, refw)):
            mean, std = ((0.4, 0.5), (0.2, 0.3)) if "channels_out" in kw else ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
            got = ctx.resize_ycc_tensor(fr, case.in_w, case.in_h, case.out_w, case.out_h, mean=mean, std=std, dtype=dt, **kw)
            lut = (L.normalize_lut(3, mean, std, dt) if len(mean) == 3 else
                   np.concatenate([L.normalize_lut(1, mean[k], std[k], dt) for k in range(2)]))
            want = V.view(r, lut, kw.get("channels_out"), kw.get("flip") if not isinstance(kw.get("flip"), str) else 1,
                          kw.get("tensor_layout", "chw"))
            _eq(V.words(got), want, f"tensor host {dt} {kw}")


def test_refusals_on_the_device_entries(ctx, d_jfif):
    import torch
    case = Y.CASE["i420_down"]
    d = _desc(case)
    y, cb, cr = Y.make_planes(case, 2)
    fr = torch.from_numpy(Y.tight(y, cb, cr)).cuda()
    n = case.out_w * case.out_h * 3
    out = torch.zeros(2 * n + 64, dtype=torch.uint8, device="cuda")
    t = torch.zeros(2 * n + 64, dtype=torch.float32, device="cuda")
    dl = torch.from_numpy(T32.identity_lut(3)).cuda()
    src = L.ycc_source(d, "i420")
    ext = L.ycc_frame_bytes(d, src)
    st = V.strides("chw", case.out_w, case.out_h, 3)
    ctx.resize_ycc_device(d, src, d_jfif.data_ptr(), fr.data_ptr(), out.data_ptr(), 2, out_frame_stride=n + 3)
    torch.cuda.synchronize()
    before = ctx.last_ycc_info()
    assert before.launches == 4

    def both(code, dd=d, s=src, table=d_jfif.data_ptr(), x=fr.data_ptr(), o=None, frames=2, **kw):
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_ycc_device(dd, s, table, x, out.data_ptr() if o is None else o, frames, **kw)
        assert e.value.code == code, (kw, e.value.code)
        kw.pop("out_frame_stride", None)
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_ycc_tensor_device(dd, s, table, x, t.data_ptr(), frames, dl.data_ptr(), st, **kw)
        assert e.value.code == code, (kw, e.value.code)
    both(L.ERR_BAD_ARG, s=None)
    both(L.ERR_BAD_ARG, table=None)
    both(L.ERR_BAD_ARG, x=None)
    both(L.ERR_BAD_ARG, frames=0)
    both(L.ERR_BAD_ARG, in_frame_stride=ext - 1)
    both(L.ERR_BAD_ARG, window=L.ResizeWindow(0, 0, case.out_w + 1, 1))
    both(L.ERR_BAD_ARG, box=(0, 0, case.in_w + 1, case.in_h))
    bad = L.ycc_source(d, "i420")
    bad.reserved[2] = 1
    both(L.ERR_BAD_ARG, s=bad)
    nv = L.ycc_source(d, "nv12")
    nv.sub_x = 0
    both(L.ERR_BAD_ARG, s=nv)
    for kw in ({"bits": 16}, {"f32": True}):
        both(L.ERR_UNSUPPORTED, dd=L.resize_desc(case.in_w, case.in_h, case.out_w, case.out_h, 3, **kw))
    da = _desc(case)
    da.reserved[0] |= L.RESIZE_ALPHA
    both(L.ERR_UNSUPPORTED, dd=da)
    both(L.ERR_BAD_ARG, dd=L.resize_desc(case.in_w, case.in_h, case.out_w, case.out_h, 1))
    both(L.ERR_BAD_ARG, dd=L.resize_desc(case.in_w, case.in_h, case.out_w, case.out_h, 4))
    # RGB frames are stored by dwords: the base and the stride are dword multiples, and the stride clears the frame
    for kw in (dict(o=out.data_ptr() + 1), dict(out_frame_stride=n), dict(out_frame_stride=n + 2), dict(out_frame_stride=n - 1)):
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_ycc_device(d, src, d_jfif.data_ptr(), fr.data_ptr(), kw.pop("o", out.data_ptr()), 2, **kw)
        assert e.value.code == L.ERR_BAD_ARG, kw
    assert n % 4 and (n + 3) % 4 == 0
    # element frames on multiples of their element; the view's own rules are lanczos_tensor_view's
    with pytest.raises(L.LanczosError) as e:
        ctx.resize_ycc_tensor_device(d, src, d_jfif.data_ptr(), fr.data_ptr(), t.data_ptr() + 2, 2, dl.data_ptr(), st)
    assert e.value.code == L.ERR_BAD_ARG
    with pytest.raises(L.LanczosError) as e:
        ctx.resize_ycc_tensor_device(d, src, d_jfif.data_ptr(), fr.data_ptr(), t.data_ptr(), 2, dl.data_ptr(), (1, 1, 1))
    assert e.value.code == L.ERR_BAD_ARG
    with pytest.raises(L.LanczosError) as e:
        ctx.resize_ycc_tensor_device(d, src, d_jfif.data_ptr(), fr.data_ptr(), t.data_ptr(), 2, dl.data_ptr(), st, channels_out=(0, 3))
    assert e.value.code == L.ERR_BAD_ARG
    torch.cuda.synchronize()
    assert ctx.last_ycc_info() == before                       # a refused call leaves the report of the last good one
    # two-channel frames stay refused
    with pytest.raises(L.LanczosError):
        L.resize_desc(case.in_w, case.in_h, case.out_w, case.out_h, 2)


def test_capture_and_replay_on_one_stream(golden):
    """one linear capture of an NV12 tensor call on a single stream (luma, split, chroma, merge; both scratch blocks grown
    inside the capture), replayed, then replayed with the input and the flips rewritten; an eager call of a larger shape on the
    same context afterwards leaves the graph's blocks alive"""
    import torch
    case = Y.CASE["i420_down"]
    frames = 3
    c = L.Context(0)                                            # a context that has not seen the shape
    try:
        d = _desc(case)
        p1, p2 = Y.make_planes(case, frames, seed=11), Y.make_planes(case, frames, seed=12)
        ref1 = Y.compose(*p1, 1, 1, case.out_w, case.out_h)
        ref2 = Y.compose(*p2, 1, 1, case.out_w, case.out_h)
        s1, s2 = (Y.build(*p, Y.NV12, y_row_stride=48, c_row_stride=44, base=1, seed=4) for p in (p1, p2))
        src = _source(d, case, s1)
        lut = T32.identity_lut(3)
        st = V.strides("chw", case.out_w, case.out_h, 3)
        x = torch.from_numpy(s1.buf).cuda()
        dt = torch.from_numpy(L.ycc_table("jfif")).cuda()
        dl = torch.from_numpy(lut).cuda()
        df = torch.tensor([0, 1, 2], dtype=torch.uint8, device="cuda")
        out = torch.zeros((frames, 3, case.out_h, case.out_w), dtype=torch.float32, device="cuda")
        g = torch.cuda.CUDAGraph()
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="relaxed"):
            c.resize_ycc_tensor_device(d, src, dt.data_ptr(), x.data_ptr() + s1.at, out.data_ptr(), frames, dl.data_ptr(), st,
                                       in_frame_stride=s1.frame_stride, stream=torch.cuda.current_stream().cuda_stream,
                                       d_flip=df.data_ptr())
        info = c.last_ycc_info()
        assert info.split and info.launches == 4
        torch.cuda.synchronize()
        assert not out.view(torch.int32).any()                  # captured, not run
        g.replay()
        torch.cuda.synchronize()
        _eq(V.words(out.cpu().numpy()), V.view(ref1, lut, None, [0, 1, 2]), "first replay")
        x.copy_(torch.from_numpy(s2.buf))
        df.copy_(torch.tensor([3, 0, 1], dtype=torch.uint8))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        _eq(V.words(out.cpu().numpy()), V.view(ref2, lut, None, [3, 0, 1]), "replay after the input and the flips changed")
        big = Y.CASE["i420_gap2_both"]                          # eager, larger planes: the scratch blocks are replaced
        pb = Y.make_planes(big, 2)
        _eq(c.resize_ycc(Y.tight(*pb, Y.NV12), big.in_w, big.in_h, 60, 40), Y.compose(*pb, 1, 1, 60, 40), "eager after the capture")
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        _eq(V.words(out.cpu().numpy()), V.view(ref2, lut, None, [3, 0, 1]), "replay after the eager call")
        del g
    finally:
        c.close()
