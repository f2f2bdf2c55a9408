"""GPU checks of the normalised-tensor entry for 16-bit and float samples (lanczos_resize_tensor_norm_*): uint16 / float32 frames
resized straight into float32, bfloat16 or float16 tensors, cvt(((float)P / div - mean) / std) computed where the sample is
stored.  Everything is compared as bit patterns, never within a tolerance: against the numpy model of the three operations
(tests/resize_tensor_norm_model.py, held to torch's CPU pipeline by tests/test_resize_tensor_norm_host.py) over the samples the
existing Context.resize / Context.resize_f32 return for the same request, which are pinned to Pillow elsewhere, and for Pillow's
own fixtures over Pillow's outputs.  Every fused instance runs once, with the set reached asserted; the route is asserted
wherever it is named; the device cases compare the whole guarded buffer, so nothing the strides do not name is touched."""
import importlib.util
import itertools
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_tensor_norm_model as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ("float32", "bfloat16", "float16")
BUCKETS = (3, 5, 7, 9, 11, 13, 17, 25)                       # LZ_RS_BUCKETS
# (div, mean, std) of tests/test_resize_tensor_norm_host.py: ImageNet-like, 12 bits with float16 subnormals, float16 overflow
PARAMS = [(65535.0, 0.485, 0.229), (4095.0, 0.0, 256.0), (1.0, -3.5, 0.5)]
DIV, MEAN, STD = (65535.0, 4095.0, 1023.0, 255.0), (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.25)
SENTINEL = {4: 0xA5A5A5A5, 2: 0xA5A5}


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.resize_force(L.RESIZE_AUTO)
    c.close()


def _noise(shape, dtype, seed):
    """uint16: every value equally likely.  float32: finite, both signs, magnitudes over twelve decades (no sum overflows)"""
    rng = np.random.default_rng(seed)
    if dtype == np.uint16:
        return rng.integers(0, 65536, shape, dtype=np.uint16)
    return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-6, 6, shape)).astype(np.float32)


def _samples(ctx, imgs, ow, oh, **kw):
    """the samples the existing entries store for the request (AUTO): not under test here"""
    ctx.resize_force(L.RESIZE_AUTO)
    return ctx.resize(imgs, ow, oh, **kw) if imgs.dtype == np.uint16 else ctx.resize_f32(imgs, ow, oh, **kw)


def _eq(got, want, what):
    got, want = N.patterns(got), N.patterns(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ, first at {tuple(bad[0])}: "
                             f"{int(got[tuple(bad[0])]):#x} != {int(want[tuple(bad[0])]):#x}")


def _device_case(ctx, imgs, ow, oh, dtype, st, what, div=DIV, mean=MEAN, std=STD, src=None, flips=None, flip=0, window=None,
                 frame_gap=0, in_gap=0, pitch_pad=0, path=L.RESIZE_AUTO, a=3, filter="lanczos", want_route=None):
    """One device call into a guarded buffer of sentinels: frames `frame_gap` elements further apart than their extent, source
    frames `in_gap` samples further apart (rows `pitch_pad` samples longer: a pitched source), the first element frame an odd
    number of elements into the buffer.  The whole buffer is compared with the model scattered over the same sentinels."""
    import torch
    f, ih, iw, c = imgs.shape
    u16 = imgs.dtype == np.uint16
    B = imgs.dtype.itemsize
    src = tuple(range(c)) if src is None else tuple(src)
    oc = len(src)
    d = L.resize_desc(iw, ih, ow, oh, c, a, bits=16 if u16 else 8, f32=not u16, filter=filter)
    kw = {"a": a, "filter": filter}
    if window is not None:
        kw["window"] = window
    ref = _samples(ctx, imgs, ow, oh, **kw)
    w, h = ref.shape[2], ref.shape[1]
    E = 4 if dtype == "float32" else 2
    et = np.uint32 if E == 4 else np.uint16
    n = N.extent(w, h, oc, st)
    fs = n + frame_gap
    GUARD = 33
    total = GUARD + (f - 1) * fs + n + GUARD
    want = np.full(total, SENTINEL[E], dtype=et)
    mflips = flip if flips is None else [flip ^ int(m) for m in flips]
    assert N.scatter(want, GUARD, ref, div[:oc], mean[:oc], std[:oc], dtype, src, mflips, st, fs) == f * oc * h * w
    y = torch.from_numpy(np.full(total, SENTINEL[E], dtype=et).view(np.int32 if E == 4 else np.int16)).cuda()
    # the source, pitched and gapped where asked, sentinels (a finite pattern) in between
    row = iw * c + pitch_pad
    in_fs = ih * row + in_gap
    xs = np.full(f * in_fs + 8, 0x3C3C if u16 else 1.0, dtype=imgs.dtype)
    for k in range(f):
        xs[k * in_fs:k * in_fs + ih * row].reshape(ih, row)[:, :iw * c] = imgs[k].reshape(ih, iw * c)
    x = torch.from_numpy(xs.view(np.int16) if u16 else xs).cuda()
    df = torch.from_numpy(np.asarray(flips, dtype=np.uint8)).cuda() if flips is not None else None
    nrm = L.tensor_norm(st, div[:oc], mean[:oc], std[:oc], dtype, src, flip, df.data_ptr() if df is not None else None)
    source = L.resize_source(d, "interleaved", row_stride=row * B) if pitch_pad else None
    ctx.resize_force(path)
    try:
        ctx.resize_tensor_norm_device(d, x.data_ptr(), y.data_ptr() + E * GUARD, f, nrm, in_frame_stride=in_fs * B if (in_gap or pitch_pad) else 0,
                                      out_frame_stride=E * fs if frame_gap else 0, stream=torch.cuda.current_stream().cuda_stream,
                                      window=window, source=source)
        torch.cuda.synchronize()
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    route, kernel = ctx.last_tensor_route(), ctx.last_kernel()
    _eq(y.cpu().numpy().view(et), want, what)
    if want_route is not None:
        assert route == want_route, (what, route)
        if want_route == L.TENSOR_FUSED:
            assert kernel == L.KERNEL_RESIZE_FUSED, (what, kernel)
    return route


def _instance_shape(bps, c, K):
    """(filter, a, in_w, out_w): out_w is a strip and 37 pixels, in_w makes the horizontal tap count fall into bucket K"""
    sw = {2: {1: 128, 3: 128, 4: 64}, 4: {1: 128, 3: 64, 4: 64}}[bps][c]     # rs_strip_width
    ow = sw + 37
    if K in (3, 5):
        return ("bilinear" if K == 3 else "bicubic"), 3, ow // 2 + 3, ow
    a, ratio = {7: (3, 0.8), 9: (4, 0.8), 11: (3, 1.5), 13: (3, 1.9), 17: (4, 1.9), 25: (3, 3.9)}[K]
    return "lanczos", a, int(ow * ratio), ow


REACHED = set()


@pytest.mark.parametrize("K", BUCKETS)
@pytest.mark.parametrize("bps", [2, 4])
def test_every_fused_instance(ctx, bps, K):
    """k_rs_fused<RsSample<bps>, C, K, false, kRsNorm> for C = 1, 3, 4: two strips, the second ragged, three chunks, 70 output
    rows, two frames with a frame stride that is not tight, the three element formats over CHW, HWC and a gapped layout"""
    sdt = np.uint16 if bps == 2 else np.float32
    layouts = itertools.cycle(["chw", "hwc", "gapped"])
    for c in (1, 3, 4):
        filt, a, iw, ow = _instance_shape(bps, c, K)
        ih, oh, frames = 53, 70, 2
        d = L.resize_desc(iw, ih, ow, oh, c, a, bits=16 if bps == 2 else 8, f32=bps == 4, filter=filt)
        p = L.resize_plan_host(d, frames)
        sw = ow - 37
        assert p.fused and p.K == K and p.strips == 2 and ow % sw and p.chunks >= 2, (bps, c, K, p.fused, p.K, p.strips, p.chunks)
        imgs = _noise((frames, ih, iw, c), sdt, 100 * K + 10 * c + bps)
        for dtype in DTYPES:
            name = next(layouts)
            st = (oh * (ow + 3) + 5, ow + 3, 1) if name == "gapped" else N.strides(name, ow, oh, c)
            _device_case(ctx, imgs, ow, oh, dtype, st, f"bps={bps} C={c} K={K} {dtype} {name}", a=a, filter=filt, frame_gap=7,
                         in_gap=6, want_route=L.TENSOR_FUSED)
        REACHED.add((bps, c, K))


def test_every_fused_instance_was_reached():
    assert REACHED == set(itertools.product((2, 4), (1, 3, 4), BUCKETS)), sorted(set(itertools.product((2, 4), (1, 3, 4), BUCKETS)) - REACHED)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_16_bit_value_through_both_kernels(ctx, dtype):
    """a 256 x 256 frame of all 65 536 values: kept at size it is the converted kernel's input as it lies; resized to 200 x 70 the
    fused epilogue sees what Context.resize stores"""
    img = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    rng = np.random.default_rng(1)
    shuffled = rng.permutation(65536).astype(np.uint16).reshape(256, 256)
    small = ctx.resize(shuffled, 200, 70)
    assert L.resize_plan_host(L.resize_desc(256, 256, 200, 70, 1, bits=16), 1).fused
    for div, mean, std in PARAMS:
        got = ctx.resize_tensor_norm(img, 256, 256, div, mean, std, dtype)
        assert ctx.last_tensor_route() == L.TENSOR_CONVERTED
        _eq(got, N.norm(img, div, mean, std, dtype), f"at size {dtype} {div}")
        got = ctx.resize_tensor_norm(shuffled, 200, 70, div, mean, std, dtype)
        assert ctx.last_tensor_route() == L.TENSOR_FUSED and ctx.last_kernel() == L.KERNEL_RESIZE_FUSED
        _eq(got, N.norm(small, div, mean, std, dtype), f"resized {dtype} {div}")
    if dtype == "float16":
        sub = N.norm(img, *PARAMS[1], dtype)
        assert ((sub & 0x7C00) == 0).sum() > 4 and (N.norm(img, *PARAMS[2], dtype) == 0x7C00).any()


def _golden(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_float_fixtures_of_pillow(ctx):
    """Pillow's mode F outputs (denormal, overflowing, tiny negative, non-finite): with div 1, mean 0, std 1 to float32 the result
    is Pillow's bits; with a normalisation and every format it is the model over Pillow's outputs.  NaN positions coincide"""
    g = _golden("make_resize32_golden")
    cases = g.load(os.path.join(ROOT, "tests", "golden", "resize_pillow_f32.npz"))
    routes = set()
    for si, kind in g.CASES:
        iw, ih, ow, oh, box = g.SHAPES[si]
        img, out = cases[g.case_name(si, kind)]
        got = ctx.resize_tensor_norm(img, ow, oh, box=box)
        routes.add(ctx.last_tensor_route())
        assert got.shape == (1, oh, ow) and got.dtype == np.float32
        assert N.same_bits(got[0], out, "float32"), (si, kind)
        for dtype in DTYPES:
            got = ctx.resize_tensor_norm(img, ow, oh, 3.0, 0.25, 0.5, dtype, box=box)
            assert N.same_bits(got, N.norm(out, 3.0, 0.25, 0.5, dtype), dtype), (si, kind, dtype)
    assert routes == {L.TENSOR_FUSED, L.TENSOR_CONVERTED}


def test_16_bit_fixtures_of_pillow(ctx):
    g = _golden("make_resize16_golden")
    cases = g.load(os.path.join(ROOT, "tests", "golden", "resize_pillow_u16.npz"))
    routes = set()
    for si, (iw, ih, ow, oh) in enumerate(g.SHAPES):
        for pattern in g.PATTERNS:
            img, out = cases[g.case_name(si, pattern)]
            for dtype in DTYPES:
                got = ctx.resize_tensor_norm(img, ow, oh, None, 0.485, 0.229, dtype, layout="hwc")
                _eq(got, N.norm(out, 65535.0, 0.485, 0.229, dtype, layout="hwc"), f"s{si} {pattern} {dtype}")
            routes.add(ctx.last_tensor_route())
    assert routes == {L.TENSOR_FUSED, L.TENSOR_CONVERTED}


ROUTES = [
    # name, sample type, (iw, ih, ow, oh), C, filter, forced path, expected route (None: refused), expected kernel
    ("horizontal only", np.uint16, (90, 41, 61, 41), 3, "lanczos", L.RESIZE_AUTO, L.TENSOR_CONVERTED, L.KERNEL_RESIZE_TWO_PASS),
    ("vertical only", np.float32, (61, 90, 61, 41), 3, "lanczos", L.RESIZE_AUTO, L.TENSOR_CONVERTED, L.KERNEL_RESIZE_TWO_PASS),
    ("at size", np.uint16, (61, 41, 61, 41), 3, "lanczos", L.RESIZE_AUTO, L.TENSOR_CONVERTED, L.KERNEL_RESIZE_TWO_PASS),
    ("at size, odd count", np.uint16, (7, 9, 7, 9), 1, "lanczos", L.RESIZE_AUTO, L.TENSOR_CONVERTED, L.KERNEL_RESIZE_TWO_PASS),
    ("odd count", np.uint16, (20, 41, 7, 9), 1, "lanczos", L.RESIZE_TWO_PASS, L.TENSOR_CONVERTED, L.KERNEL_RESIZE_TWO_PASS),
    ("tall, vertical first", np.uint16, (4, 900, 3, 300), 3, "lanczos", L.RESIZE_AUTO, L.TENSOR_CONVERTED, L.KERNEL_RESIZE_TWO_PASS),
    ("nearest on float", np.float32, (90, 41, 61, 35), 3, "nearest", L.RESIZE_AUTO, L.TENSOR_CONVERTED, L.KERNEL_RESIZE_NEAREST),
    ("forced two pass", np.uint16, (90, 41, 61, 35), 3, "lanczos", L.RESIZE_TWO_PASS, L.TENSOR_CONVERTED, L.KERNEL_RESIZE_TWO_PASS),
    ("forced convert", np.float32, (90, 41, 61, 35), 4, "lanczos", L.RESIZE_CONVERT, L.TENSOR_CONVERTED, L.KERNEL_RESIZE_FUSED),
    ("auto", np.uint16, (90, 41, 61, 35), 4, "lanczos", L.RESIZE_AUTO, L.TENSOR_FUSED, L.KERNEL_RESIZE_FUSED),
    ("forced fused", np.float32, (90, 41, 61, 35), 1, "lanczos", L.RESIZE_FUSED, L.TENSOR_FUSED, L.KERNEL_RESIZE_FUSED),
    ("forced fused, one pass", np.uint16, (90, 41, 61, 41), 3, "lanczos", L.RESIZE_FUSED, None, 0),
]


@pytest.mark.parametrize("case", ROUTES, ids=[r[0] for r in ROUTES])
def test_routes(ctx, case):
    name, sdt, (iw, ih, ow, oh), c, filt, path, route, kernel = case
    imgs = _noise((2, ih, iw, c), sdt, 7 + iw + ih)
    st = N.strides("chw", ow, oh, c)
    if route is None:
        with pytest.raises(L.LanczosError) as e:
            _device_case(ctx, imgs, ow, oh, "float32", st, name, filter=filt, path=path)
        assert e.value.code == L.ERR_UNSUPPORTED
        return
    for dtype in DTYPES:
        _device_case(ctx, imgs, ow, oh, dtype, st, f"{name} {dtype}", filter=filt, path=path, want_route=route, frame_gap=3)
        assert ctx.last_kernel() == kernel, name
    if (iw * ih * c) % 2:   # the frames behind the first start off a dword and the last dword of each is half outside it
        assert sdt == np.uint16 and (ow * oh * c) % 2


VIEWS = [
    ("window", {"window": (5, 3, 47, 29)}, 3),
    ("reorder", {"src": (2, 1, 0)}, 3),
    ("drop a channel", {"src": (0, 1, 2)}, 4),
    ("drop and reorder", {"src": (3, 0)}, 4),
    ("flips per frame", {"flips": [0, 1, 2, 3], "flip": 1}, 3),
    ("pitched source", {"pitch_pad": 5}, 3),
    ("everything", {"window": (4, 2, 50, 30), "src": (2, 0), "flips": [3, 0, 1, 2], "pitch_pad": 2}, 3),
]


@pytest.mark.parametrize("path,route", [(L.RESIZE_AUTO, L.TENSOR_FUSED), (L.RESIZE_TWO_PASS, L.TENSOR_CONVERTED)])
@pytest.mark.parametrize("case", VIEWS, ids=[v[0] for v in VIEWS])
def test_the_view(ctx, case, path, route):
    """a window, a channel map, flips per frame and a pitched source, on both routes and for both sample widths; a dropped
    channel's plane does not exist in the layout and the sentinels around the frames stay"""
    name, kw, c = case
    for sdt, dtype in ((np.uint16, "float32"), (np.float32, "bfloat16"), (np.uint16, "float16")):
        imgs = _noise((4, 41, 90, c), sdt, 300 + c)
        w, h = kw["window"][2:] if "window" in kw else (61, 35)
        oc = len(kw.get("src", range(c)))
        for layout in ("chw", "hwc"):
            _device_case(ctx, imgs, 61, 35, dtype, N.strides(layout, w, h, oc), f"{name} {dtype} {layout}", path=path,
                         want_route=route, frame_gap=5, **kw)


def test_the_host_entry_and_python_arguments(ctx):
    """Context.resize_tensor_norm: defaults, shapes, torch-style indexing of the model"""
    img = _noise((2, 41, 90, 3), np.uint16, 5)
    ref = ctx.resize(img, 61, 35)
    got = ctx.resize_tensor_norm(img, 61, 35)
    assert got.shape == (2, 3, 35, 61) and got.dtype == np.float32
    _eq(got, N.norm(ref, 65535.0), "defaults")
    got = ctx.resize_tensor_norm(img, 61, 35, mean=MEAN[:2], std=STD[:2], dtype="bfloat16", layout="hwc", channels_out=(2, 0), flip=[1, 2])
    assert got.shape == (2, 35, 61, 2) and got.dtype == np.uint16
    _eq(got, N.norm(ref, 65535.0, MEAN[:2], STD[:2], "bfloat16", (2, 0), [1, 2], "hwc"), "map, flips, hwc")
    grey = _noise((41, 90), np.float32, 6)
    got = ctx.resize_tensor_norm(grey, 61, 35, dtype="float16", window=(3, 2, 40, 20))
    assert got.shape == (1, 20, 40) and got.dtype == np.float16
    _eq(got, N.norm(ctx.resize_f32(grey, 61, 35, window=(3, 2, 40, 20)), 1.0, dtype="float16"), "2-D float input, a window")
    for bad in (img.astype(np.uint8), img.astype(np.float64)):
        with pytest.raises(L.LanczosError):
            ctx.resize_tensor_norm(bad, 61, 35)
    with pytest.raises(L.LanczosError):
        ctx.resize_tensor_norm(img, 61, 35, dtype="int8")


def test_device_argument_checks(ctx):
    import torch
    d = L.resize_desc(90, 41, 61, 35, 3, bits=16)
    x = torch.zeros(90 * 41 * 3 + 4, dtype=torch.int16, device="cuda")
    y = torch.zeros(61 * 35 * 3 + 8, dtype=torch.float32, device="cuda")
    st = N.strides("chw", 61, 35, 3)
    n32, n16 = L.tensor_norm(st), L.tensor_norm(st, dtype="float16")
    for nrm, kw, xp, yp in ((n32, {}, x.data_ptr(), y.data_ptr() + 2), (n32, {"out_frame_stride": 4 * 61 * 35 * 3 + 2}, x.data_ptr(), y.data_ptr()),
                            (n32, {"out_frame_stride": 4 * 61 * 35 * 3 - 4}, x.data_ptr(), y.data_ptr()), (n16, {}, x.data_ptr(), y.data_ptr() + 1),
                            (n32, {}, x.data_ptr() + 1, y.data_ptr())):
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_tensor_norm_device(d, xp, yp, 1, nrm, **kw)
        assert e.value.code == L.ERR_BAD_ARG
        assert ctx.last_tensor_route() == 0
    with pytest.raises(L.LanczosError) as e:                                   # a reducing_gap stays refused for wide samples
        ctx.resize_tensor_norm_device(d, x.data_ptr(), y.data_ptr(), 1, n32, opts=L.resize_opts(L.resize_desc(90, 41, 61, 35, 3), None, 2.0))
    assert e.value.code == L.ERR_BAD_ARG
    planar = L.ResizeSource()
    planar.row_stride, planar.chan_stride, planar.pix_stride = 90 * 2, 90 * 41 * 2, 2
    with pytest.raises(L.LanczosError) as e:                                   # ... and so does a planar source of them
        ctx.resize_tensor_norm_device(d, x.data_ptr(), y.data_ptr(), 1, n32, source=planar)
    assert e.value.code == L.ERR_UNSUPPORTED
    ctx.resize_tensor_norm_device(d, x.data_ptr() + 2, y.data_ptr() + 2, 1, n16)   # 2 bytes past a dword, both sides
    torch.cuda.synchronize()
    assert ctx.last_tensor_route() == L.TENSOR_FUSED and ctx.last_kernel() == L.KERNEL_RESIZE_FUSED


@pytest.mark.parametrize("path", [L.RESIZE_FUSED, L.RESIZE_TWO_PASS])
def test_capture_replay_then_eager(path):
    """A captured call replays right, with the div / mean / std of the capture baked in and the flips read when the kernels run;
    an eager call on the same context afterwards is right as well"""
    import torch
    c = L.Context(0)
    try:
        ih, iw, oh, ow, frames = 95 + path, 141, 47, 63, 4          # shapes no other test of this module uses
        d = L.resize_desc(iw, ih, ow, oh, 3, bits=16)
        assert L.resize_plan_host(d, frames).fused
        imgs = _noise((frames, ih, iw, 3), np.uint16, 77)
        ref = c.resize(imgs, ow, oh)
        c.close()
        c = L.Context(0)                                            # a context that has not seen the shape
        c.resize_force(path)
        st = N.strides("chw", ow, oh, 3)
        flips, flips2 = np.array([0, 1, 2, 3], dtype=np.uint8), np.array([3, 3, 0, 1], dtype=np.uint8)
        x = torch.from_numpy(imgs.view(np.int16)).cuda()
        df = torch.from_numpy(flips).cuda()
        y = torch.zeros((frames, 3, oh, ow), dtype=torch.float32, device="cuda")
        nrm = L.tensor_norm(st, DIV[:3], MEAN[:3], STD[:3], "float32", (2, 1, 0), 0, df.data_ptr())
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            c.resize_tensor_norm_device(d, x.data_ptr(), y.data_ptr(), frames, nrm, stream=torch.cuda.current_stream().cuda_stream)
        assert c.last_tensor_route() == (L.TENSOR_FUSED if path == L.RESIZE_FUSED else L.TENSOR_CONVERTED)
        torch.cuda.synchronize()
        assert not y.view(torch.int32).any()                        # captured, not run
        for k in range(3):
            nrm.div[k], nrm.mean[k], nrm.std[k] = 1.0, 0.0, 1.0     # the struct travelled by value: the graph keeps the old ones
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), N.norm(ref, DIV[:3], MEAN[:3], STD[:3], "float32", (2, 1, 0), flips), "first replay")
        df.copy_(torch.from_numpy(flips2))
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), N.norm(ref, DIV[:3], MEAN[:3], STD[:3], "float32", (2, 1, 0), flips2), "replay after the flips changed")
        del g
        y.zero_()
        c.resize_tensor_norm_device(d, x.data_ptr(), y.data_ptr(), frames, nrm, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), N.norm(ref, 1.0, 0.0, 1.0, "float32", (2, 1, 0), flips2), "eager after the capture")
    finally:
        c.close()
