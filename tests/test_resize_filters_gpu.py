"""GPU checks of the resize filters (LANCZOS_RESIZE_FILTER: box, bilinear, Hamming, bicubic, nearest): every sample equal to
Pillow's fixture and to the numpy model of the contract (tests/resize_filters_model.py), never within a tolerance (float32:
NaN positions coincide, everything else as a 32-bit pattern).  The fixture on every path and sample type, every 3- and 5-tap
fused instance, 1-tap windows, the old instances on the new tables, non-finite neighbours of short float windows, the nearest
kernel (pixel sizes, ragged rows, odd bases, strided batches with guards, capture), and the cache key."""
import importlib.util
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_filters_model as FM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden():
    spec = importlib.util.spec_from_file_location("make_resize_filters_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_resize_filters_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    g = _golden()
    return g, g.load()


def _eq(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if FM.same(got, want):
        return
    bad = FM.M32.differs(got, want) if got.dtype == np.float32 else got != want
    at = tuple(np.argwhere(bad)[0])
    raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} samples differ, first at {at}: {got[at]!r} != {want[at]!r}")


def _img(h, w, c, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        return (rng.random((h, w, c), dtype=np.float32) * np.float32(4) - np.float32(1)).astype(np.float32)
    if dtype == np.uint16:
        x = rng.integers(0, 65536, (h, w, c)).astype(np.uint16)
        x[rng.random((h, w, c)) < 0.2] = 65535       # hard edges: the bicubic overshoots past 65535 (the wrapping store)
        x[rng.random((h, w, c)) < 0.2] = 0
        return x
    x = rng.integers(0, 256, (h, w, c)).astype(np.uint8)
    if c == 4:
        x[..., 3][rng.random((h, w)) < 0.25] = 0
        x[..., 3][rng.random((h, w)) < 0.25] = 255
    return x


def _run(ctx, img, filt, ow, oh, alpha=False, box=None, gap=None):
    if img.dtype == np.float32:
        return ctx.resize_f32(img, ow, oh, box=box, filter=filt)
    return ctx.resize(img, ow, oh, alpha=alpha, box=box, reducing_gap=gap, filter=filt)


def _plan(img, filt, ow, oh, alpha=False, box=None, gap=None):
    x = img if img.ndim == 3 else img[..., None]
    d = L.resize_desc(x.shape[1], x.shape[0], ow, oh, x.shape[2], alpha=alpha, bits=16 if img.dtype == np.uint16 else 8,
                      f32=img.dtype == np.float32, filter=filt)
    if box is None and gap is None:
        return L.resize_plan_host(d, 1)
    return L.resize_plan_host(d, 1, box=box, reducing_gap=gap).inner


def _all_paths(ctx, img, want, filt, what, alpha=False, box=None, gap=None):
    """AUTO, forced FUSED where the plan allows it (refused where not) and forced TWO_PASS against `want`; returns the plan"""
    oh, ow = want.shape[:2]
    p = _plan(img, filt, ow, oh, alpha, box, gap)
    nearest = L.filter_code(filt) == L.FILTER_NEAREST
    try:
        for path in (L.RESIZE_AUTO, L.RESIZE_FUSED, L.RESIZE_TWO_PASS):
            ctx.resize_force(path)
            if path == L.RESIZE_FUSED and not p.fused:
                with pytest.raises(L.LanczosError) as e:
                    _run(ctx, img, filt, ow, oh, alpha, box, gap)
                assert e.value.code == L.ERR_UNSUPPORTED, what
                continue
            _eq(_run(ctx, img, filt, ow, oh, alpha, box, gap), want, f"{what} path {path}")
            fused = p.fused and path != L.RESIZE_TWO_PASS
            idle = not FM.MB.axis_runs(img.shape[1], ow, *(box[0::2] if box else (0, img.shape[1]))) and \
                not FM.MB.axis_runs(img.shape[0], oh, *(box[1::2] if box else (0, img.shape[0])))
            expect = L.KERNEL_RESIZE_FUSED if fused else L.KERNEL_RESIZE_NEAREST if nearest and not idle else L.KERNEL_RESIZE_TWO_PASS
            assert ctx.last_kernel() == expect, (what, path, ctx.last_kernel())
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    return p


def test_pillow_fixture_all_paths(ctx, golden):
    """Pillow's own output for every filter x mode of the fixture, boxes and gaps included"""
    g, cases = golden
    fused = 0
    for name, (f, m, s, img, want) in cases.items():
        _, _, ow, oh, box, gap = g.SHAPES[s]
        p = _all_paths(ctx, img, want, f, name, alpha=m == "RGBA", box=box, gap=gap)
        fused += p.fused
        assert not (f == "nearest" and p.fused)
    assert fused >= 100, fused


SAMPLES = (("u8", np.uint8, False), ("alpha", np.uint8, True), ("u16", np.uint16, False), ("f32", np.float32, False))


@pytest.mark.parametrize("kind,dtype,alpha", SAMPLES, ids=[s[0] for s in SAMPLES])
@pytest.mark.parametrize("filt,K", [("bilinear", 3), ("bicubic", 5)])
def test_every_small_fused_instance(ctx, filt, K, kind, dtype, alpha):
    """K in {3, 5} x C in {1, 3, 4} x sample type against the model, each at a shape with more than one strip, a ragged last
    strip and a ragged last 8-row block; the plan's K is asserted."""
    for c in ((4,) if alpha else (1, 3, 4)):
        sw = 64 if c == 4 or (dtype == np.float32 and c == 3) else 128 if dtype != np.uint8 else 256
        iw, ih = (sw + sw // 3) // 2 + 2, 37
        ow, oh = sw + sw // 3 + 5, 75                       # two strips, the last ragged; 75 rows: a block of 3 at the end
        img = _img(ih, iw, c, dtype, seed=100 * K + c)
        want = FM.resize(img, FM.NAMES.index(filt), ow, oh, alpha=alpha)
        p = _all_paths(ctx, img, want, filt, f"{filt} {kind} C={c}", alpha=alpha)
        assert p.fused and p.K == K and p.strips == 2 and ow % sw and oh % 8, (c, p.K, p.strips)


def test_issue_shape_70x37_to_150x75(ctx):
    for filt, K in (("bilinear", 3), ("bicubic", 5), ("box", 3), ("hamming", 3)):
        img = _img(37, 70, 3, np.uint8, seed=7)
        p = _all_paths(ctx, img, FM.resize(img, FM.NAMES.index(filt), 150, 75), filt, filt)
        assert p.fused and p.K == K


def test_one_tap_windows_and_old_buckets(ctx):
    """A BOX upscale and BOX at out = in with a shifted box have 1-tap windows in both axes; bicubic downscales whose ksize
    lands in the old 7, 9 and 13 buckets run the old instances on the new tables."""
    for dtype in (np.uint8, np.uint16, np.float32):
        img = _img(45, 70, 3, dtype, seed=21)
        for ow, oh, box in ((150, 101, None), (70, 45, (0.5, 0.25, 70, 45))):
            b = box or (0, 0, 70, 45)
            for in_n, out_n, b0, b1 in ((70, ow, b[0], b[2]), (45, oh, b[1], b[3])):
                assert (FM.axis_tables(FM.BOX, in_n, out_n, b0, b1)[1] == 1).all()
            p = _all_paths(ctx, img, FM.resize(img, FM.BOX, ow, oh, box), "box", f"1-tap {dtype.__name__} {box}", box=box)
            assert p.fused and p.K == 3
    for iw, ow, K in ((90, 70, 7), (100, 60, 9), (150, 55, 13)):
        for c, dtype, alpha in ((3, np.uint8, False), (4, np.uint8, True), (1, np.uint16, False), (3, np.float32, False)):
            img = _img(61, iw, c, dtype, seed=K + c)
            assert FM.ksize(FM.BICUBIC, ow, 0, iw) == K
            p = _all_paths(ctx, img, FM.resize(img, FM.BICUBIC, ow, 40, alpha=alpha), "bicubic", f"bicubic K={K} C={c}",
                           alpha=alpha)
            assert p.fused and p.K == K, (p.K, K)


@pytest.mark.parametrize("filt", ["box", "bilinear", "bicubic"])
def test_f32_nonfinite_neighbours_of_short_windows(ctx, filt):
    """inf / NaN samples just outside 1- and 2-tap windows: the padded taps of the 3- and 5-tap instances must not read them
    into the sum.  Exactly `count` taps are multiplied (the model's rule), so a NaN spreads over Pillow's window only."""
    rng = np.random.default_rng(5)
    for c in (1, 3, 4):
        img = rng.random((37, 70, c), dtype=np.float32)
        flat = img.reshape(-1)
        for v in (np.inf, -np.inf, np.nan):
            flat[rng.choice(flat.size, 4, replace=False)] = np.float32(v)
        img[0, 0], img[-1, -1], img[0, -1] = np.inf, np.nan, -np.inf          # frame corners: windows cut by the edge
        want = FM.resize(img, FM.NAMES.index(filt), 150, 75)
        assert 0 < np.isnan(want).mean() < 0.2
        p = _all_paths(ctx, img, want, filt, f"{filt} C={c}")
        assert p.fused and p.K in (3, 5)


# ---- NEAREST -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c,dtype,alpha", [(1, np.uint8, False), (3, np.uint8, False), (4, np.uint8, False), (4, np.uint8, True),
                                           (1, np.float32, False), (3, np.float32, False), (4, np.float32, False)])
def test_nearest_every_pixel_size(ctx, c, dtype, alpha):
    """pixel sizes 1, 3, 4, 12 and 16 bytes; up, down, 1 -> N, out_w = 13 (row bytes no dword multiple), a sub-pixel box, more
    than one workgroup per row"""
    img = _img(29, 41, c, dtype, seed=c)
    for ow, oh, box in ((13, 7, None), (90, 61, None), (41, 29, (0.5, 0.25, 41, 29)), (23, 19, (5.3, 4.7, 36.1, 28.2)),
                        (41, 50, None), (1100, 3, None)):
        want = FM.resize(img, FM.NEAREST, ow, oh, box, alpha=alpha)
        _all_paths(ctx, img, want, "nearest", f"nearest C={c} {dtype.__name__} {ow}x{oh} {box}", alpha=alpha, box=box)
    one = img[:1, :1]
    _eq(_run(ctx, one, "nearest", 57, 5, alpha), FM.resize(one, FM.NEAREST, 57, 5, alpha=alpha), "1 -> N")
    assert ctx.last_kernel() == L.KERNEL_RESIZE_NEAREST
    _eq(_run(ctx, img, "nearest", 41, 29, alpha), img, "equal size, full box: a copy")
    assert ctx.last_kernel() == L.KERNEL_RESIZE_TWO_PASS


def test_nearest_u16_is_refused(ctx):
    with pytest.raises(L.LanczosError) as e:
        ctx.resize(np.zeros((8, 8), np.uint16), 5, 5, filter="nearest")
    assert e.value.code == L.ERR_UNSUPPORTED
    with pytest.raises(L.LanczosError) as e:
        ctx.resize(np.zeros((80, 80), np.uint8), 5, 5, filter="nearest", reducing_gap=2.0)
    assert e.value.code == L.ERR_BAD_ARG


@pytest.mark.parametrize("c,dtype", [(1, np.uint8), (3, np.uint8), (4, np.uint8), (3, np.float32)])
def test_nearest_strided_batches_odd_bases_and_guards(ctx, c, dtype):
    """frames at strides with gaps, 8-bit bases at odd byte offsets (float: 4 and 8), guard bytes in front, between and behind"""
    import torch
    f, ih, iw, ow, oh = 3, 23, 37, 13, 31
    B = np.dtype(dtype).itemsize
    frames = np.stack([_img(ih, iw, c, dtype, seed=60 + k) for k in range(f)])
    want = FM.resize(frames, FM.NEAREST, ow, oh)
    in_fb, out_fb = ih * iw * c * B, oh * ow * c * B
    in_fs, out_fs = in_fb + (5 if B == 1 else 12), out_fb + (7 if B == 1 else 20)
    d = L.resize_desc(iw, ih, ow, oh, c, f32=dtype == np.float32, filter="nearest")
    s = torch.cuda.Stream()
    for lead, out_lead in (((0, 0), (1, 3), (2, 1), (3, 2)) if B == 1 else ((0, 0), (4, 8))):
        x = torch.full((lead + f * in_fs + 64,), 201, dtype=torch.uint8, device="cuda")
        for k in range(f):
            x[lead + k * in_fs:lead + k * in_fs + in_fb] = torch.from_numpy(frames[k].reshape(-1).view(np.uint8)).cuda()
        y = torch.full((out_lead + f * out_fs + 64,), 77, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            ctx.resize_device(d, x.data_ptr() + lead, y.data_ptr() + out_lead, f, in_fs, out_fs, s.cuda_stream)
        s.synchronize()
        got = y.cpu().numpy()
        assert (got[:out_lead] == 77).all(), "wrote in front of the first frame"
        got = got[out_lead:]
        for k in range(f):
            _eq(got[k * out_fs:k * out_fs + out_fb].copy().view(dtype).reshape(oh, ow, c), want[k], f"frame {k} lead {lead}")
            assert (got[k * out_fs + out_fb:(k + 1) * out_fs] == 77).all(), "wrote into the gap between frames"
        assert (got[f * out_fs:] == 77).all()


def test_nearest_first_use_inside_capture_then_replay_and_eager():
    import torch
    c = L.Context(0)
    try:
        ih, iw, oh, ow = 85, 133, 49, 63
        img, img2 = _img(ih, iw, 3, np.uint8, 9), _img(ih, iw, 3, np.uint8, 10)
        d = L.resize_desc(iw, ih, ow, oh, 3, filter="nearest")
        x = torch.from_numpy(img).cuda()
        y = torch.zeros((oh, ow, 3), dtype=torch.uint8, device="cuda")
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            c.resize_device(d, x.data_ptr(), y.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert int(y.max()) == 0                                # captured, not run
        x.copy_(torch.from_numpy(img2))
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), FM.resize(img2, FM.NEAREST, ow, oh), "replay")
        x.copy_(torch.from_numpy(img))
        y2 = torch.zeros_like(y)
        c.resize_device(d, x.data_ptr(), y2.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _eq(y2.cpu().numpy(), FM.resize(img, FM.NEAREST, ow, oh), "eager call after the first replay")
        big = _img(150, 200, 3, np.uint8, 11)
        _eq(c.resize(big, 85, 60, filter="bicubic"), FM.resize(big, FM.BICUBIC, 85, 60), "other shape, other filter")
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), FM.resize(img, FM.NEAREST, ow, oh), "replay after other work")
        del g
    finally:
        c.close()


@pytest.mark.parametrize("order", [("lanczos", "bicubic", "nearest"), ("nearest", "bicubic", "lanczos")])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_filters_of_one_axis_shape_do_not_share_a_cache_entry(order, dtype):
    img = _img(61, 97, 3, dtype, seed=33)
    c = L.Context(0)
    try:
        for round_ in range(2):
            for filt in order:
                _eq(_run(c, img, filt, 45, 30), FM.resize(img, FM.NAMES.index(filt), 45, 30), f"{filt}, round {round_}")
    finally:
        c.close()
