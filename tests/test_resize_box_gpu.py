"""The source box, reduce and reducing_gap of the resize entry on the GPU (lanczos_resize_*_ex, lanczos_reduce_*): every
case of the Pillow fixture byte for byte through every path its plan admits, full-size frames against the numpy model
(tests/resize_box_model.py), frame strides and odd base addresses, and first use inside a captured graph."""
import importlib.util
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import patterns as P
import resize_box_model as BM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_pillow_box.npz")


def _gen():
    spec = importlib.util.spec_from_file_location("make_resize_box_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_resize_box_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _gen()


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _eq(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} samples differ, first at {tuple(bad[0])}: "
                             f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


def _bilevel(h, w, c, seed):
    """0 / 255 in 5 x 3 cells: block sums at both extremes and every mix between."""
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 2, (h // 3 + 1, w // 5 + 1, c), dtype=np.uint8) * 255
    return np.ascontiguousarray(np.repeat(np.repeat(cells, 3, axis=0), 5, axis=1)[:h, :w])


def _all_paths(ctx, img, ow, oh, want, what, box=None, gap=None, alpha=False, a=3):
    """AUTO and TWO_PASS always; FUSED where the plan admits it, and refused with ERR_UNSUPPORTED where it does not."""
    x = img if img.ndim == 3 else img[:, :, None]
    d = L.resize_desc(x.shape[1], x.shape[0], ow, oh, x.shape[2], a, alpha, 8 * img.dtype.itemsize)
    full = (0, 0, x.shape[1], x.shape[0])
    plan = L.resize_plan_host(d, 1, box=box if box is not None else full, reducing_gap=gap)
    fused = 0
    try:
        for path in (L.RESIZE_AUTO, L.RESIZE_TWO_PASS, L.RESIZE_FUSED):
            ctx.resize_force(path)
            if path == L.RESIZE_FUSED and not plan.inner.fused:
                with pytest.raises(L.LanczosError) as e:
                    ctx.resize(img, ow, oh, a, alpha, box=box, reducing_gap=gap)
                assert e.value.code == L.ERR_UNSUPPORTED, what
                continue
            _eq(ctx.resize(img, ow, oh, a, alpha, box=box, reducing_gap=gap), want, f"{what} path {path}")
            want_family = L.KERNEL_RESIZE_FUSED if plan.inner.fused and path != L.RESIZE_TWO_PASS else L.KERNEL_RESIZE_TWO_PASS
            assert ctx.last_kernel() == want_family, (what, path)
            fused += path == L.RESIZE_FUSED
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    return fused


def test_pillow_fixture_box_cases(ctx):
    z = np.load(GOLDEN)
    fused = 0
    for i, (name, iw, ih, ow, oh, mode, box) in enumerate(G.BOX_CASES):
        img = G.make_input(0, i, iw, ih, mode)
        fused += _all_paths(ctx, img, ow, oh, z[f"box_{name}"], name, box=box, alpha=mode == "RGBA")
    assert fused >= 10      # the fused kernels ran boxed tables of every sample type


def test_pillow_fixture_reduce_cases(ctx):
    z = np.load(GOLDEN)
    for i, (name, iw, ih, mode, factor, box) in enumerate(G.REDUCE_CASES):
        img = G.make_input(1, i, iw, ih, mode)
        _eq(ctx.reduce(img, factor, box), z[f"reduce_{name}"], name)
    _eq(ctx.reduce(G.make_input(1, 0, 64, 48, "RGB"), 2), z["reduce_sq2_RGB"], "int factor")


def test_pillow_fixture_gap_cases(ctx):
    z = np.load(GOLDEN)
    for i, (name, iw, ih, ow, oh, mode, box, gap) in enumerate(G.GAP_CASES):
        img = G.make_input(2, i, iw, ih, mode)
        _all_paths(ctx, img, ow, oh, z[f"gap_{name}"], name, box=box, gap=gap)


def test_gap_is_refused_for_alpha_and_16_bit_on_the_device_too(ctx):
    for img, alpha in ((P.noise(60, 80, 4, seed=1), True), (P.noise(60, 80, 1, seed=2)[..., 0].astype(np.uint16) * 257, False)):
        with pytest.raises(L.LanczosError) as e:
            ctx.resize(img, 10, 8, 3, alpha, reducing_gap=2.0)
        assert e.value.code == L.ERR_BAD_ARG
    with pytest.raises(L.LanczosError) as e:
        ctx.reduce(P.noise(60, 80, 1, seed=2)[..., 0].astype(np.uint16), 2)
    assert e.value.code == L.ERR_BAD_ARG


@pytest.mark.parametrize("gap", [2.0, 3.0])
def test_w5_with_a_gap_full_size(ctx, gap):
    """3840 x 2160 -> 160 x 90, the thumbnail that runs two-pass without a gap: reduced 12 x 12 (gap 2) or 8 x 8 (gap 3),
    then the fused kernel."""
    frames = np.stack([P.gradient_noise(2160, 3840, 3, seed=int(gap)), P.noise(2160, 3840, 3, seed=20 + int(gap))])
    got = ctx.resize(frames, 160, 90, 3, reducing_gap=gap)
    assert ctx.last_kernel() == L.KERNEL_RESIZE_FUSED
    _eq(got, BM.resize(frames, 160, 90, None, gap), f"W5 gap {gap}")
    assert not np.array_equal(got, ctx.resize(frames, 160, 90, 3))      # the gap is not the ungapped resize


@pytest.mark.parametrize("out", [(1920, 1080), (640, 360)])
def test_fractional_crop_out_of_8k(ctx, out):
    ow, oh = out
    img = P.gradient_noise(4320, 7680, 3, seed=ow)
    box = (3000.3, 1700.6, 4281.1, 2420.2)
    want = BM.resize_box(img, ow, oh, box)
    assert _all_paths(ctx, img, ow, oh, want, f"8k crop -> {out}", box=box) == 1


@pytest.mark.parametrize("sample", ["alpha", "u16"])
def test_boxed_alpha_and_16_bit_at_moderate_size(ctx, sample):
    if sample == "alpha":
        img = P.noise(600, 801, 4, seed=31)
    else:
        img = np.random.default_rng(32).integers(0, 65536, (600, 801, 3), dtype=np.uint16)
    for (ow, oh), box in (((517, 389), (10.3, 20.7, 790.1, 580.9)), ((300, 450), (200.5, 0, 500.25, 600)),
                          ((801, 600), (0.5, 0.25, 801, 600))):
        want = BM.resize_box(img, ow, oh, box, alpha=sample == "alpha")
        _all_paths(ctx, img, ow, oh, want, f"{sample} {ow}x{oh}", box=box, alpha=sample == "alpha")


@pytest.mark.parametrize("content", ["noise", "bilevel"])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_reduce_full_size(ctx, c, content):
    h, w = 2160, 3840
    img = P.noise(h, w, c, seed=c) if content == "noise" else _bilevel(h, w, c, seed=c)
    for factor in ((12, 12), (7, 5), (1, 4), (3, 1), (13, 11)):       # 13 x 11 leaves ragged edges on both axes
        _eq(ctx.reduce(img, factor), BM.reduce(img, factor), f"C={c} {content} {factor}")
    assert w % 13 and h % 11 and w % 7 and not h % 5
    box = (17, 9, 3801, 2150)
    _eq(ctx.reduce(img, (12, 12), box), BM.reduce(img, (12, 12), box), f"C={c} {content} boxed")


def test_reduce_wide_factors(ctx):
    """fx * C beyond a tile's span runs the one-workgroup-per-pixel kernel; just below it the tiled one with one pixel."""
    for c, fx, fy in ((4, 1025, 3), (4, 1024, 3), (1, 4097, 2), (3, 1366, 5), (3, 1365, 5)):
        img = P.noise(11, 2 * fx + 77, c, seed=fx)
        _eq(ctx.reduce(img, (fx, fy)), BM.reduce(img, (fx, fy)), f"C={c} {fx}x{fy}")


def test_frames_with_strides_and_an_odd_base(ctx):
    """Reduce, the boxed resize and the composite on several frames with non-tight frame strides and a base address that is
    no dword multiple; every byte around the frames is poison, and the gaps of the output stay untouched."""
    import torch
    f, ih, iw = 4, 271, 483
    s = torch.cuda.Stream()
    for c in (3, 1, 4):
        frames = np.stack([P.gradient_noise(ih, iw, c, seed=70 + k) for k in range(f)])
        in_fb = ih * iw * c
        in_fs = in_fb + 13
        box, rbox = (20.3, 10.7, 470.1, 260.9), (5, 3, 480, 269)
        jobs = [("reduce", BM.reduce(frames, (5, 4), rbox)), ("box", BM.resize_box(frames, 150, 100, box)),
                ("gap", BM.resize(frames, 40, 30, box, 2.0))]
        for lead in (1, 3):
            n = lead + f * in_fs + 64
            x = torch.from_numpy(np.random.default_rng(lead).integers(0, 256, n, dtype=np.uint8)).cuda()
            for k in range(f):
                x[lead + k * in_fs:lead + k * in_fs + in_fb] = torch.from_numpy(frames[k].reshape(-1)).cuda()
            for what, want in jobs:
                oh, ow = want.shape[1:3]
                out_fb = oh * ow * c
                out_fs = out_fb + 7
                for olead in (0, 1):
                    y = torch.full((olead + f * out_fs + 64,), 77, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    with torch.cuda.stream(s):
                        if what == "reduce":
                            ctx.reduce_device(iw, ih, c, (5, 4), x.data_ptr() + lead, y.data_ptr() + olead, f, rbox, in_fs,
                                              out_fs, s.cuda_stream)
                        else:
                            d = L.resize_desc(iw, ih, ow, oh, c)
                            ctx.resize_device(d, x.data_ptr() + lead, y.data_ptr() + olead, f, in_fs, out_fs, s.cuda_stream,
                                              box=box, reducing_gap=2.0 if what == "gap" else None)
                    s.synchronize()
                    got = y.cpu().numpy()
                    assert (got[:olead] == 77).all()
                    for k in range(f):
                        at = olead + k * out_fs
                        _eq(got[at:at + out_fb].reshape(oh, ow, c), want[k], f"{what} C={c} frame {k} lead {lead}/{olead}")
                        assert (got[at + out_fb:at + out_fs] == 77).all(), "wrote into the gap between frames"
                    assert (got[olead + f * out_fs:] == 77).all()


@pytest.mark.parametrize("path", [L.RESIZE_AUTO, L.RESIZE_TWO_PASS])
@pytest.mark.parametrize("order", ["capture_first", "eager_first"])
def test_composite_inside_a_captured_graph(path, order):
    """reduce -> context scratch -> box resize captured into a graph: first use inside the capture, replayed, then eager --
    and the other order.  The reduced frames and (two-pass) the intermediate are context scratch a live graph pins."""
    import torch
    c = L.Context(0)
    try:
        c.resize_force(path)
        ih, iw, oh, ow = 397 + path, 611, 23, 31        # shapes no other test of this module uses
        box, gap = (7.5, 3.25, 600.75, 390.5), 2.0
        img, img2 = P.gradient_noise(ih, iw, 3, seed=9), P.noise(ih, iw, 3, seed=10)
        want, want2 = BM.resize(img, ow, oh, box, gap), BM.resize(img2, ow, oh, box, gap)
        assert BM.gap_plan(iw, ih, ow, oh, box, gap)[:2] == (9, 8)
        d = L.resize_desc(iw, ih, ow, oh, 3)
        x = torch.from_numpy(img).cuda()
        y = torch.zeros((oh, ow, 3), dtype=torch.uint8, device="cuda")
        if order == "eager_first":
            _eq(c.resize(img, ow, oh, 3, box=box, reducing_gap=gap), want, "eager before the capture")
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            c.resize_device(d, x.data_ptr(), y.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream, box=box,
                            reducing_gap=gap)
        torch.cuda.synchronize()
        assert int(y.max()) == 0                          # captured, not run
        if order == "capture_first":
            g.replay()
            torch.cuda.synchronize()
            _eq(y.cpu().numpy(), want, "first replay")
        _eq(c.resize(img2, ow, oh, 3, box=box, reducing_gap=gap), want2, "eager after the capture")
        big = P.noise(900, 1300, 3, seed=11)              # a larger request: grows the reduced block and the scratch
        _eq(c.resize(big, 50, 40, 3, reducing_gap=1.0), BM.resize(big, 50, 40, None, 1.0), "larger request")
        x.copy_(torch.from_numpy(img2))
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), want2, "replay after other work")
        del g
    finally:
        c.close()
