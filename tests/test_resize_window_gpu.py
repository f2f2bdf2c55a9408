"""GPU checks of the window of the output (lanczos_resize_window_*, lanczos_resize_tensor*_window_*): a windowed call stores
exactly the slice of what the same call without a window stores -- compared byte for byte, floats and 16-bit words as bit
patterns -- on every route: the fused kernel (every sample type, forced and planned), two passes, one pass of either axis,
the gather of NEAREST, the crop copy where neither axis runs, with a source box and a reducing gap, into float and bfloat16
tensors, and in a batch.  For the committed fixture the expected bytes are Pillow's Image.resize(...).crop(window).

Every device call writes into a buffer prefilled with a sentinel whose frames lie further apart than a frame is long: the guards
around the frames and the gaps between them must keep the sentinel, which a launch that still wrote full-size rows would not."""
import importlib.util
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_tensor16_model as T16
import resize_tensor_model as T32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xA5
ALL_PATHS = (L.RESIZE_AUTO, L.RESIZE_TWO_PASS, L.RESIZE_FUSED)


def _gen():
    spec = importlib.util.spec_from_file_location("make_resize_window_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_resize_window_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.resize_force(L.RESIZE_AUTO)
    c.close()


def _frame(dtype, h, w, c, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        return (rng.standard_normal((h, w, c)) * 100).astype(np.float32)
    x = rng.integers(0, np.iinfo(dtype).max + 1, (h, w, c), dtype=dtype)
    if dtype == np.uint8 and c == 4:                               # every kind of alpha
        x[..., 3][rng.random((h, w)) < 0.25] = 0
        x[..., 3][rng.random((h, w)) < 0.25] = 255
    return x


def _desc(imgs, ow, oh, a=3, alpha=False, filter="lanczos"):
    f, ih, iw, c = imgs.shape
    return L.resize_desc(iw, ih, ow, oh, c, a, alpha, 16 if imgs.dtype == np.uint16 else 8, imgs.dtype == np.float32, filter)


def _device(ctx, imgs, ow, oh, window=None, path=L.RESIZE_AUTO, lead=0, in_gap=0, guard=64, out_gap=None, a=3, alpha=False,
            filter="lanczos", box=None, gap=None):
    """One device call on [F][H][W][C] frames.  The input frames start `lead` bytes into their buffer, in_gap bytes apart;
    the output frames `guard` bytes into a buffer of sentinels, out_gap bytes apart (never 0: the frame stride is larger than
    the frame).  Returns (frames [F][h][w][C], last_kernel) after checking that nothing but the frames was written."""
    import torch
    f, ih, iw, c = imgs.shape
    B = imgs.dtype.itemsize
    d = _desc(imgs, ow, oh, a, alpha, filter)
    x0, y0, w, h = window if window is not None else (0, 0, ow, oh)
    in_fb, out_fb = ih * iw * c * B, h * w * c * B
    in_fs = in_fb + in_gap
    out_gap = 7 * B if out_gap is None else out_gap
    assert out_gap > 0 and out_gap % B == 0 and guard % B == 0 and lead % B == 0 and in_gap % B == 0
    out_fs = out_fb + out_gap
    xb = np.full(lead + f * in_fs + 8, 0x5A, dtype=np.uint8)
    xb[lead:lead + f * in_fs].reshape(f, in_fs)[:, :in_fb] = np.ascontiguousarray(imgs).reshape(f, -1).view(np.uint8)
    x = torch.from_numpy(xb).cuda()
    total = guard + f * out_fs + guard
    y = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    ctx.resize_force(path)
    try:
        ctx.resize_device(d, x.data_ptr() + lead, y.data_ptr() + guard, f, in_frame_stride=in_fs if in_gap else 0,
                          out_frame_stride=out_fs, stream=torch.cuda.current_stream().cuda_stream, box=box, reducing_gap=gap,
                          window=window)
        torch.cuda.synchronize()
        kernel = ctx.last_kernel()
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    got = y.cpu().numpy()
    body = got[guard:guard + f * out_fs].reshape(f, out_fs)
    assert (got[:guard] == SENTINEL).all() and (got[guard + f * out_fs:] == SENTINEL).all(), "a guard was written"
    assert (body[:, out_fb:] == SENTINEL).all(), "the gap between two frames was written"
    return np.ascontiguousarray(body[:, :out_fb]).view(imgs.dtype).reshape(f, h, w, c), kernel


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    g, w = np.frombuffer(got.tobytes(), np.uint8), np.frombuffer(want.tobytes(), np.uint8)
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at byte {int(bad[0])} of {g.size}")


def _windows_equal_the_slice(ctx, imgs, ow, oh, windows, paths, what, kernel=None, **kw):
    """each window on each path against the slice of the AUTO call without a window (computed once)"""
    full, full_kernel = _device(ctx, imgs, ow, oh, None, **kw)
    if kernel is not None:
        assert full_kernel == kernel, (what, full_kernel)
    for window in windows:
        x0, y0, w, h = window
        want = np.ascontiguousarray(full[:, y0:y0 + h, x0:x0 + w])
        for path in paths:
            got, k = _device(ctx, imgs, ow, oh, window, path, **kw)
            _same(got, want, f"{what} window {window} path {path}")
            if path == L.RESIZE_AUTO:
                assert k == full_kernel, (what, window, k)         # the route family of the full request
            elif kernel in (L.KERNEL_RESIZE_FUSED, L.KERNEL_RESIZE_TWO_PASS) and path != L.RESIZE_AUTO:
                assert k == (L.KERNEL_RESIZE_FUSED if path == L.RESIZE_FUSED else L.KERNEL_RESIZE_TWO_PASS)
    return full


# ---- the fused kernel -------------------------------------------------------------------------------------------------

RGB8_WINDOWS = [(250, 5, 300, 37),   # off the 256-pixel strip grid, 37 rows (no multiple of 8), two strips of its own
                (0, 0, 17, 9),       # an odd width: rows of 51 bytes, the unaligned stores
                (583, 61, 17, 9),    # the right and bottom edges
                (299, 33, 1, 1),
                (249, 0, 301, 70),   # an odd width over two strips, every row
                (0, 0, 600, 70)]     # the whole output


def test_fused_rgb8_windows_on_every_route(ctx):
    imgs = _frame(np.uint8, 163, 211, 3, 1)[None]
    d = _desc(imgs, 600, 70)
    for window in RGB8_WINDOWS:
        assert L.resize_window_plan_host(d, window, 1).inner.fused, window   # forced FUSED runs on each
    _windows_equal_the_slice(ctx, imgs, 600, 70, RGB8_WINDOWS, ALL_PATHS, "rgb8 211x163 -> 600x70", L.KERNEL_RESIZE_FUSED)


def test_the_whole_window_is_the_plain_call(ctx):
    """same bytes and the same kernel as the entry without a window, through the host entry as well"""
    img = _frame(np.uint8, 163, 211, 3, 1)
    plain = ctx.resize(img, 600, 70)
    k = ctx.last_kernel()
    whole = ctx.resize(img, 600, 70, window=(0, 0, 600, 70))
    assert ctx.last_kernel() == k == L.KERNEL_RESIZE_FUSED
    _same(whole, plain, "whole window, host entry")
    part = ctx.resize(img, 600, 70, window=(250, 5, 300, 37))
    _same(part, np.ascontiguousarray(plain[5:42, 250:550]), "window, host entry")
    grey = ctx.resize(img[..., 0].copy(), 600, 70, window=(250, 5, 300, 37))
    assert grey.shape == (37, 300)
    batch = ctx.resize(np.stack([img, img[::-1]]), 600, 70, window=(583, 61, 17, 9))
    assert batch.shape == (2, 9, 17, 3)
    _same(batch[0], np.ascontiguousarray(plain[61:, 583:]), "window of a batch, host entry")


FUSED_INSTANCES = [
    # (what, dtype, channels, in_w, in_h, out_w, out_h, keywords, window)
    ("one channel", np.uint8, 1, 211, 163, 600, 70, {}, (250, 5, 300, 37)),
    ("four channels", np.uint8, 4, 111, 83, 200, 70, {}, (59, 5, 75, 37)),             # strips of 64: three of its own
    ("alpha", np.uint8, 4, 111, 83, 200, 70, {"alpha": True}, (59, 5, 75, 37)),
    ("uint16 x 3", np.uint16, 3, 111, 83, 300, 70, {}, (121, 5, 141, 37)),             # strips of 128
    ("float x 1", np.float32, 1, 111, 83, 300, 70, {}, (121, 5, 141, 37)),             # strips of 128
    ("float x 3", np.float32, 3, 111, 83, 200, 70, {}, (59, 5, 75, 37)),               # strips of 64
    ("downscale", np.uint8, 3, 300, 200, 97, 61, {}, (30, 20, 41, 21)),
    ("bicubic", np.uint8, 3, 211, 163, 600, 70, {"filter": "bicubic"}, (250, 5, 300, 37)),
    ("a = 2", np.uint8, 3, 211, 163, 600, 70, {"a": 2}, (250, 5, 301, 37)),
]


@pytest.mark.parametrize("case", FUSED_INSTANCES, ids=[c[0] for c in FUSED_INSTANCES])
def test_the_other_fused_instances(ctx, case):
    what, dtype, c, iw, ih, ow, oh, kw, window = case
    imgs = _frame(dtype, ih, iw, c, 2)[None]
    d = _desc(imgs, ow, oh, **kw)
    assert L.resize_plan_host(d, 1).fused and L.resize_window_plan_host(d, window, 1).inner.fused, what
    _windows_equal_the_slice(ctx, imgs, ow, oh, [window], ALL_PATHS, what, L.KERNEL_RESIZE_FUSED, **kw)


def test_forced_fused_is_refused_where_the_windowed_plan_cannot_fuse(ctx):
    """a reduction by 40: the full request and a window of the same columns run two passes (more horizontal taps than the
    widest fused instance), forced FUSED is LANCZOS_ERR_UNSUPPORTED, and the window still equals the slice"""
    imgs = _frame(np.uint8, 90, 2000, 3, 3)[None]
    d = _desc(imgs, 50, 45)
    window = (10, 7, 21, 11)
    assert not L.resize_plan_host(d, 1).fused and not L.resize_window_plan_host(d, window, 1).inner.fused
    _windows_equal_the_slice(ctx, imgs, 50, 45, [window], (L.RESIZE_AUTO, L.RESIZE_TWO_PASS), "40:1", L.KERNEL_RESIZE_TWO_PASS)
    ctx.resize_force(L.RESIZE_FUSED)
    try:
        with pytest.raises(L.LanczosError) as e:
            ctx.resize(imgs[0], 50, 45, window=window)
        assert e.value.code == L.ERR_UNSUPPORTED
    finally:
        ctx.resize_force(L.RESIZE_AUTO)


# ---- one pass, nearest, the crop copy ---------------------------------------------------------------------------------

ONE_PASS = [
    ("h only", np.uint8, 3, 97, 41, 55, 41, {}),
    ("h only, upscale", np.uint8, 1, 97, 41, 300, 41, {}),
    ("h only, alpha", np.uint8, 4, 97, 41, 55, 41, {"alpha": True}),
    ("h only, uint16", np.uint16, 3, 97, 41, 55, 41, {}),
    ("v only", np.uint8, 3, 97, 41, 97, 90, {}),
    ("v only, alpha", np.uint8, 4, 97, 41, 97, 19, {"alpha": True}),
    ("v only, float", np.float32, 3, 97, 41, 97, 90, {}),
]


@pytest.mark.parametrize("case", ONE_PASS, ids=[c[0] for c in ONE_PASS])
def test_one_pass_routes_crop_both_axes(ctx, case):
    what, dtype, c, iw, ih, ow, oh, kw = case
    imgs = _frame(dtype, ih, iw, c, 4)[None]
    d = _desc(imgs, ow, oh, **kw)
    p = L.resize_window_plan_host(d, None, 1)
    assert p.pass_h + p.pass_v == 1 and not p.inner.fused
    windows = [(13, 5, 31, 11), (0, 0, 7, 3), (ow - 9, oh - 4, 9, 4), (ow // 2, oh // 2, 1, 1)]
    _windows_equal_the_slice(ctx, imgs, ow, oh, windows, (L.RESIZE_AUTO, L.RESIZE_TWO_PASS), what, L.KERNEL_RESIZE_TWO_PASS, **kw)


@pytest.mark.parametrize("dtype,c", [(np.uint8, 3), (np.uint8, 4), (np.uint8, 1), (np.float32, 3), (np.float32, 1)])
def test_nearest(ctx, dtype, c):
    imgs = _frame(dtype, 61, 83, c, 5)[None]
    for ow, oh in ((131, 40), (83, 40), (300, 61)):                # both axes, and either one the identity
        windows = [(17, 9, 61, 23), (0, 0, 5, 3), (ow - 7, oh - 5, 7, 5), (ow - 1, 0, 1, 1)]
        _windows_equal_the_slice(ctx, imgs, ow, oh, windows, (L.RESIZE_AUTO,), f"nearest {ow}x{oh}", L.KERNEL_RESIZE_NEAREST,
                                 filter="nearest", lead=imgs.dtype.itemsize, guard=64 + imgs.dtype.itemsize)


CROP_COPY = [
    # (what, dtype, channels, keywords of _device): the base offsets choose the copy's unit
    ("bytes at odd bases", np.uint8, 3, {"lead": 1, "guard": 65}),
    ("bytes, dword aligned", np.uint8, 4, {"out_gap": 8}),
    ("bytes, an even base", np.uint8, 1, {"lead": 2, "guard": 66, "out_gap": 6}),
    ("uint16", np.uint16, 3, {"lead": 2, "guard": 66}),
    ("uint16, dword aligned", np.uint16, 1, {"out_gap": 8}),
    ("float", np.float32, 3, {}),
    ("rgba, alpha flag", np.uint8, 4, {"alpha": True}),
]


@pytest.mark.parametrize("case", CROP_COPY, ids=[c[0] for c in CROP_COPY])
def test_both_axes_idle_is_a_crop_copy(ctx, case):
    """the source's own samples, RGBA not premultiplied (a partial alpha would change the colours); also for NEAREST, which
    with both axes idle is the copy too"""
    what, dtype, c, kw = case
    imgs = np.stack([_frame(dtype, 30, 40, c, 6 + k) for k in range(2)])
    windows = [(11, 5, 23, 19), (0, 0, 1, 1), (39, 29, 1, 1), (0, 7, 40, 2), (12, 0, 8, 30), (1, 1, 38, 28)]
    for window in windows:
        x0, y0, w, h = window
        want = np.ascontiguousarray(imgs[:, y0:y0 + h, x0:x0 + w])
        for filt in ("lanczos", "nearest"):
            if filt == "nearest" and dtype == np.uint16:
                continue                                           # no NEAREST for uint16 frames
            got, k = _device(ctx, imgs, 40, 30, window, in_gap=4 * imgs.dtype.itemsize, filter=filt, **kw)
            _same(got, want, f"{what} window {window} {filt}")
            assert k == L.KERNEL_RESIZE_TWO_PASS                   # as the plain copy reports
    whole, k = _device(ctx, imgs, 40, 30, (0, 0, 40, 30), **kw)
    _same(whole, imgs, what + " whole")


def test_a_crop_copy_of_many_frames_is_one_call(ctx):
    """70000 frames of 3 x 2 pixels: more than a grid is deep, so the kernel walks the frames"""
    imgs = np.arange(70000 * 6, dtype=np.uint32).astype(np.uint8).reshape(70000, 2, 3, 1)
    got, _ = _device(ctx, imgs, 3, 2, (1, 0, 2, 2), out_gap=3)
    _same(got, np.ascontiguousarray(imgs[:, :, 1:3]), "70000 frames")


# ---- options ----------------------------------------------------------------------------------------------------------

def test_a_source_box_and_a_reducing_gap_with_a_window(ctx):
    imgs = _frame(np.uint8, 163, 211, 3, 7)[None]
    box = (7.3, 5.6, 201.2, 157.75)
    _windows_equal_the_slice(ctx, imgs, 600, 70, [(250, 5, 300, 37), (583, 61, 17, 9)], ALL_PATHS, "box", L.KERNEL_RESIZE_FUSED,
                             box=box)
    _windows_equal_the_slice(ctx, imgs, 211, 163, [(100, 50, 37, 21)], (L.RESIZE_AUTO, L.RESIZE_TWO_PASS), "shifted box, equal size",
                             box=(0.5, 0.25, 211, 163))
    imgs = _frame(np.uint8, 300, 400, 3, 8)[None]
    p = L.resize_plan_host(_desc(imgs, 50, 38), 1, reducing_gap=2.0)
    assert (p.fx, p.fy) == (4, 3)
    _windows_equal_the_slice(ctx, imgs, 50, 38, [(13, 9, 24, 20), (0, 0, 50, 1), (49, 37, 1, 1)], ALL_PATHS, "gap 2", gap=2.0)
    f32 = _frame(np.float32, 83, 111, 1, 9)[None]
    _windows_equal_the_slice(ctx, f32, 300, 70, [(121, 5, 141, 37)], ALL_PATHS, "float box", box=(3.25, 0.0, 100.5, 80.0))


# ---- batches ----------------------------------------------------------------------------------------------------------

def test_a_batch_of_five_frames_with_padded_strides(ctx):
    imgs = np.stack([_frame(np.uint8, 163, 211, 3, 20 + k) for k in range(5)])
    _windows_equal_the_slice(ctx, imgs, 600, 70, [(250, 5, 301, 37)], ALL_PATHS, "batch", L.KERNEL_RESIZE_FUSED, lead=1, in_gap=13,
                             guard=67, out_gap=11)
    one = _frame(np.uint8, 41, 97, 4, 30)
    imgs = np.stack([one, one[::-1].copy(), one[:, ::-1].copy(), one, one[::-1, ::-1].copy()])
    _windows_equal_the_slice(ctx, imgs, 97, 19, [(13, 5, 31, 11)], (L.RESIZE_AUTO,), "batch v only alpha", lead=3, in_gap=5,
                             guard=65, out_gap=9, alpha=True)


# ---- tensor calls -----------------------------------------------------------------------------------------------------

def _tensor_device(ctx, imgs, ow, oh, window, st, dtype, path, lut, frame_gap, alpha=False):
    """A tensor call into a buffer of sentinel elements, frames frame_gap elements further apart than their extent: returns
    (all elements as words, the expected words, route)"""
    import torch
    f, ih, iw, c = imgs.shape
    T, word, tdt = (T32, np.uint32, np.int32) if dtype == "float32" else (T16, np.uint16, np.int16)
    d = _desc(imgs, ow, oh, alpha=alpha)
    x0, y0, w, h = window
    ctx.resize_force(L.RESIZE_AUTO)
    ref = ctx.resize(imgs, ow, oh, alpha=alpha, window=window)
    n = T.extent(w, h, c, st)
    fs = n + frame_gap
    guard = 33
    sentinel = word(0xA5A5A5A5 & np.iinfo(word).max)
    want = np.full(guard + (f - 1) * fs + n + guard, sentinel, dtype=word)
    assert T.scatter(want, guard, ref, lut, st, fs) == f * c * h * w
    x = torch.from_numpy(np.ascontiguousarray(imgs).reshape(-1)).cuda()
    y = torch.from_numpy(np.full(want.size, sentinel, dtype=word).view(tdt)).cuda()
    dl = torch.from_numpy(np.ascontiguousarray(lut).view(word).view(tdt)).cuda()
    ctx.resize_force(path)
    try:
        ctx.resize_tensor_device(d, x.data_ptr(), y.data_ptr() + guard * word().itemsize, f, dl.data_ptr(), st,
                                 out_frame_stride=fs * word().itemsize, stream=torch.cuda.current_stream().cuda_stream,
                                 dtype=dtype, window=window)
        torch.cuda.synchronize()
        route = ctx.last_tensor_route()
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    return y.cpu().numpy().view(word), want, route


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("layout", ["chw", "hwc", "padded chw"])
def test_tensor_calls_with_a_window(ctx, dtype, layout):
    """a fused shape: TENSOR_FUSED under AUTO, the converted route under forced CONVERT and TWO_PASS; the table applied to the
    windowed bytes, and every element the strides do not name keeps the sentinel.  The strides are the WINDOW's: tightly
    packed for 301 x 37 they would overlap for 600 x 70"""
    imgs = np.stack([_frame(np.uint8, 163, 211, 3, 40 + k) for k in range(2)])
    window = (249, 5, 301, 37)
    x0, y0, w, h = window
    T = T32 if dtype == "float32" else T16
    lut = T32.identity_lut(3) if dtype == "float32" else T16.identity_lut16(3)
    st = T.strides(layout, w, h, 3) if layout != "padded chw" else (h * (w + 3) + 5, w + 3, 1)
    d = _desc(imgs, 600, 70)
    assert L.resize_window_plan_host(d, window, 2).inner.fused
    for path, route in ((L.RESIZE_AUTO, L.TENSOR_FUSED), (L.RESIZE_CONVERT, L.TENSOR_CONVERTED),
                        (L.RESIZE_TWO_PASS, L.TENSOR_CONVERTED)):
        got, want, r = _tensor_device(ctx, imgs, 600, 70, window, st, dtype, path, lut, 10)
        assert r == route, (layout, path, r)
        assert np.array_equal(got, want), f"{dtype} {layout} path {path}: {int((got != want).sum())} words differ"


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_resize_tensor_with_a_window(ctx, dtype):
    """Context.resize_tensor(window=): the table of ToTensor() + Normalize() over the windowed bytes, CHW and HWC; alpha; the
    routes that are never fused (nearest, one pass, the crop copy)"""
    mean, std = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)
    T = (lambda b, lut, layout: T32.tensor(b, lut, layout)) if dtype == "float32" else T16.tensor16
    bits = T32.bits if dtype == "float32" else T16.words
    cases = [(3, 211, 163, 600, 70, (250, 5, 300, 37), {}, L.TENSOR_FUSED),
             (4, 111, 83, 200, 70, (59, 5, 75, 37), {"alpha": True}, L.TENSOR_FUSED),
             (3, 83, 61, 131, 40, (17, 9, 61, 23), {"filter": "nearest"}, L.TENSOR_CONVERTED),
             (1, 97, 41, 55, 41, (13, 5, 31, 11), {}, L.TENSOR_CONVERTED),
             (3, 40, 30, 40, 30, (11, 5, 23, 19), {}, L.TENSOR_CONVERTED)]
    for c, iw, ih, ow, oh, window, kw, route in cases:
        img = _frame(np.uint8, ih, iw, c, 50 + c)
        ref = ctx.resize(img, ow, oh, window=window, **kw)
        lut = L.normalize_lut(c, mean[:c], std[:c], dtype)
        for layout in ("chw", "hwc"):
            got = ctx.resize_tensor(img, ow, oh, mean=mean[:c], std=std[:c], layout=layout, dtype=dtype, window=window, **kw)
            x0, y0, w, h = window
            assert got.shape == ((c, h, w) if layout == "chw" else (h, w, c))
            assert ctx.last_tensor_route() == route, (c, ow, oh, layout)
            assert np.array_equal(bits(got), T(ref, lut, layout)), (c, ow, oh, layout, dtype)


def test_device_argument_checks(ctx):
    """the minimum of out_frame_stride is the window's frame, for bytes and for tensors; a refused call launches nothing"""
    import torch
    d = L.resize_desc(211, 163, 600, 70, 3)
    window = (250, 5, 300, 37)
    x = torch.zeros(211 * 163 * 3, dtype=torch.uint8, device="cuda")
    y = torch.full((2 * 300 * 37 * 3 * 4 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    ok = 300 * 37 * 3
    for stride, code in ((ok - 1, L.ERR_BAD_ARG), (ok, L.OK), (ok + 1, L.OK)):
        try:
            ctx.resize_device(d, x.data_ptr(), y.data_ptr(), 2, out_frame_stride=stride, window=window)
            got = L.OK
        except L.LanczosError as e:
            got = e.code
        assert got == code, stride
    for bad in ((250, 5, 400, 37), (0, 0, 0, 1)):
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_device(d, x.data_ptr(), y.data_ptr(), 1, window=bad)
        assert e.value.code == L.ERR_BAD_ARG
    dl = torch.zeros(3 * 256, dtype=torch.float32, device="cuda")
    st = L.tensor_strides("chw", 300, 37, 3)
    ctx.resize_tensor_device(d, x.data_ptr(), y.data_ptr(), 2, dl.data_ptr(), st, out_frame_stride=4 * ok, window=window)
    torch.cuda.synchronize()
    assert ctx.last_tensor_route() == L.TENSOR_FUSED
    with pytest.raises(L.LanczosError) as e:
        ctx.resize_tensor_device(d, x.data_ptr(), y.data_ptr(), 2, dl.data_ptr(), st, out_frame_stride=4 * ok - 4, window=window)
    assert e.value.code == L.ERR_BAD_ARG and ctx.last_tensor_route() == 0
    with pytest.raises(L.LanczosError) as e:                       # the window's strides overlap for the whole output
        ctx.resize_tensor_device(d, x.data_ptr(), y.data_ptr(), 1, dl.data_ptr(), st)
    assert e.value.code == L.ERR_BAD_ARG


# ---- Pillow's bytes ---------------------------------------------------------------------------------------------------

def test_pillow_resize_then_crop(ctx):
    G = _gen()
    cases = G.load()
    assert len(cases) >= 12
    for name, (case, img, out) in cases.items():
        _, mode, filt, iw, ih, ow, oh, box, gap, window = case
        if mode == "F":
            got = ctx.resize_f32(img, ow, oh, box=box, filter=filt, window=window)
        else:
            got = ctx.resize(img, ow, oh, alpha=mode == "RGBA", box=box, reducing_gap=gap, filter=filt, window=window)
        _same(got, out, name)
    # the pipeline the window is for: CenterCrop through center_window, on both forced routes too
    case, img, out = cases["RGB_center"]
    assert L.center_window(case[5], case[6], 44, 44) == case[9]
    for path in (L.RESIZE_FUSED, L.RESIZE_TWO_PASS):
        ctx.resize_force(path)
        try:
            _same(ctx.resize(img, case[5], case[6], window=L.center_window(case[5], case[6], 44, 44)), out, f"center path {path}")
        finally:
            ctx.resize_force(L.RESIZE_AUTO)
