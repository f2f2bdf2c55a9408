"""GPU checks of the 16-bit resize (LANCZOS_RESIZE_U16): every sample identical to Pillow's I;16 fixture and to the numpy
model of the contract (tests/resize16_model.py), never within a tolerance -- the fixture on all three paths and as 3- and
4-channel stacks, every fused instance, geometry edges, full-size frames, strided batches at bases that are no dword
multiple, first use inside stream capture in both orders, and 8-bit requests around a 16-bit one of the same axis shapes."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize16_model as M
import resize_model as M8

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_8BIT = os.path.join(ROOT, "tests", "golden", "resize_pillow.npz")
FUSED_K = (7, 9, 11, 13, 17, 25)


def _golden():
    spec = importlib.util.spec_from_file_location("make_resize16_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_resize16_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _noise(h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 65536, (h, w, c), dtype=np.uint16)


def _bilevel(h, w, c, seed):
    return (np.random.default_rng(seed).integers(0, 2, (h, w, c)) * 65535).astype(np.uint16)


def _eq(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} samples differ, first at {tuple(bad[0])}: "
                             f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


def _plan(iw, ih, ow, oh, c, a, frames=1):
    return L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, c, a, bits=16), frames)


def _hks(iw, ow, a):
    return L.resize_taps_f64_host(L.resize_desc(iw, 1, ow, 1, 1, a, bits=16), 0)[2].shape[1]


def _all_paths(ctx, img, want, a, what):
    """FUSED (refused exactly where the plan says two-pass), TWO_PASS and AUTO against `want`; returns the plan."""
    ih, iw, c = img.shape
    oh, ow = want.shape[:2]
    p = _plan(iw, ih, ow, oh, c, a)
    try:
        ctx.resize_force(L.RESIZE_FUSED)
        if p.fused:
            _eq(ctx.resize(img, ow, oh, a), want, f"{what} fused")
            assert ctx.last_kernel() == L.KERNEL_RESIZE_FUSED, what
        else:
            with pytest.raises(L.LanczosError) as e:
                ctx.resize(img, ow, oh, a)
            assert e.value.code == L.ERR_UNSUPPORTED, what
        ctx.resize_force(L.RESIZE_TWO_PASS)
        _eq(ctx.resize(img, ow, oh, a), want, f"{what} two-pass")
        assert ctx.last_kernel() == L.KERNEL_RESIZE_TWO_PASS, what
        ctx.resize_force(L.RESIZE_AUTO)
        _eq(ctx.resize(img, ow, oh, a), want, f"{what} auto")
        assert ctx.last_kernel() == (L.KERNEL_RESIZE_FUSED if p.fused else L.KERNEL_RESIZE_TWO_PASS), what
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    return p


def test_pillow_fixture_all_paths_and_channel_stacks(ctx):
    """Pillow's own I;16 output: every plane alone (C = 1, also as a 2-D array), and the planes of a shape stacked to 3 and
    4 interleaved channels, every channel being an independent I;16 plane."""
    g = _golden()
    cases = g.load()
    fused = two_pass = 0
    for si, (iw, ih, ow, oh) in enumerate(g.SHAPES):
        planes = [cases[g.case_name(si, p)] for p in g.PATTERNS]
        for pattern, (img, want) in zip(g.PATTERNS, planes):
            p = _all_paths(ctx, img[..., None], want[..., None], 3, f"shape {si} {pattern}")
            fused += p.fused
            two_pass += not p.fused
            _eq(ctx.resize(img, ow, oh, 3), want, f"shape {si} {pattern} 2-D")
        for order in ((0, 1, 2), (3, 2, 1, 0)):
            img = np.stack([planes[k][0] for k in order], axis=2)
            want = np.stack([planes[k][1] for k in order], axis=2)
            _all_paths(ctx, img, want, 3, f"shape {si} C={len(order)}")
    assert fused >= 16 and two_pass >= 12, (fused, two_pass)   # 4 shapes fuse; 2 change one axis only, 1 has 135 taps


# horizontal ksize -> (a, in_w) at out_w = 261: two whole strips and a ragged one of 5 (four of 64 and 5 with four channels)
H_KSIZE = {5: (2, 200), 7: (3, 200), 9: (4, 200), 11: (3, 392), 13: (3, 496), 15: (3, 574), 17: (4, 496), 19: (3, 757),
           25: (3, 1018)}


def test_every_fused_instance(ctx):
    """k_rs_fused<RsSample<2>, C, K> for every C in {1, 3, 4} and K in {7, 9, 11, 13, 17, 25}, at both edges of the buckets, a = 2, 3, 4,
    each with a vertical upscale and a vertical reduction, against the model on all three paths."""
    ow, ih = 261, 60
    seen = set()
    for c in (1, 3, 4):
        for hk, (a, iw) in H_KSIZE.items():
            assert _hks(iw, ow, a) == hk                       # from the public query, not recomputed
            k = next(b for b in FUSED_K if b >= hk)
            img = (_noise if hk % 4 == 1 else _bilevel)(ih, iw, c, seed=hk * 8 + c)
            for oh in (67, 23):
                p = _all_paths(ctx, img, M.resize(img, ow, oh, a), a, f"C={c} hk={hk} a={a} oh={oh}")
                assert p.fused and p.K == k, (c, hk, p.K)
                assert p.strips == (5 if c == 4 else 3)
                seen.add((c, p.K, a))
    assert {(c, k) for c, k, _ in seen} == {(C, K) for C in (1, 3, 4) for K in FUSED_K}
    assert {a for _, _, a in seen} == {2, 3, 4}


def _edge_cases(c):
    sw = 64 if c == 4 else 128
    cases = []
    for ow in (1, 2, 3, sw - 1, sw, sw + 1, 2 * sw + 1):
        cases.append((f"out_w={ow}", max(2, (ow * 17 + 9) // 10), 40, ow, 23, 3))
    for oh in (1, 7, 8, 9, 33, 65):
        cases.append((f"out_h={oh}", 50, max(2, (oh * 17 + 9) // 10), 37, oh, 3))
    cases += [("in_w=1", 1, 20, 7, 13, 3), ("in_h=1", 20, 1, 13, 7, 3), ("in=1x1", 1, 1, 5, 4, 3), ("out=1x1", 41, 37, 1, 1, 3),
              ("w 2->600", 2, 30, 600, 17, 4), ("h 2->600", 30, 2, 17, 600, 2),
              ("w 600->2", 600, 30, 2, 17, 3), ("h 600->2", 30, 600, 17, 2, 3),
              ("h only down", 77, 90, 77, 31, 3), ("h only up", 77, 31, 77, 90, 2),
              ("w only down", 90, 77, 31, 77, 4), ("w only up", 31, 77, 90, 77, 3),
              ("identity", 31, 17, 31, 17, 3),
              ("ksize 27", 1100, 24, 261, 23, 3), ("staging capped", 1017, 200, 261, 29, 3)]
    return cases


@pytest.mark.parametrize("c", [1, 3, 4])
def test_geometry_edges(ctx, c):
    """1-pixel inputs and outputs, ragged last strips, march blocks of fewer than 8 rows, one-axis-only resizes in each
    direction (one kernel of the two-pass path), the plain copy, and what the fused kernel cannot take."""
    for name, iw, ih, ow, oh, a in _edge_cases(c):
        img = _noise(ih, iw, c, seed=iw + 3 * oh + c) if (iw + oh) % 2 else _bilevel(ih, iw, c, seed=iw + 3 * oh + c)
        p = _all_paths(ctx, img, M.resize(img, ow, oh, a), a, f"C={c} {name} {iw}x{ih}->{ow}x{oh}")
        one_axis = iw == ow or ih == oh
        if one_axis or name in ("ksize 27", "w 600->2", "h 600->2", "out=1x1"):
            assert not p.fused, name
        elif name != "staging capped":
            assert p.fused, name
        if name == "identity":
            _eq(ctx.resize(img, ow, oh, a), img, "identity is a copy")


@pytest.mark.parametrize("shape", [(3840, 2160, 1920, 1080), (1920, 1080, 3840, 2160)])
@pytest.mark.parametrize("pattern", ["noise", "bilevel"])
def test_full_size_frames(ctx, shape, pattern):
    """One frame each of the two speed workloads' shapes (scripts/resize_speed.py U1, U4), three channels."""
    iw, ih, ow, oh = shape
    img = (_noise if pattern == "noise" else _bilevel)(ih, iw, 3, seed=iw + len(pattern))
    want = M.resize(img, ow, oh, 3)
    assert _plan(iw, ih, ow, oh, 3, 3).fused
    _all_paths(ctx, img, want, 3, f"{shape} {pattern}")
    if pattern == "bilevel":   # the wrap is live: stores above 0xFF00 that are not 65535, and zeros from negative sums
        assert ((want >= 0xFF00) & (want != 65535)).any() and (want == 0).any()


def test_strided_batches_at_2_byte_offsets_with_guards(ctx):
    """Frame strides larger than a frame, a base two bytes into a dword, poison in every gap; the bytes around every output
    frame stay as they were."""
    import torch
    for c in (3, 1, 4):
        f, ih, iw, ow, oh = 4, 135, 241, 150, 75
        frames = np.stack([_noise(ih, iw, c, seed=50 + k) if k % 2 else _bilevel(ih, iw, c, seed=50 + k) for k in range(f)])
        want = M.resize(frames, ow, oh, 3)
        in_fb, out_fb = ih * iw * c * 2, oh * ow * c * 2
        in_fs, out_fs = in_fb + 14, out_fb + 6            # even; with the leads below every frame is met at both dword alignments
        s = torch.cuda.Stream()
        d = L.resize_desc(iw, ih, ow, oh, c, 3, bits=16)
        for lead, out_lead in ((0, 0), (2, 0), (2, 2), (0, 2)):
            n = lead + f * in_fs + 64
            x = torch.from_numpy(np.random.default_rng(lead).integers(0, 256, n, dtype=np.uint8)).cuda()   # poison
            for k in range(f):
                x[lead + k * in_fs:lead + k * in_fs + in_fb] = torch.from_numpy(frames[k].reshape(-1).view(np.uint8)).cuda()
            for path in (L.RESIZE_AUTO, L.RESIZE_TWO_PASS, L.RESIZE_FUSED):
                ctx.resize_force(path)
                y = torch.full((out_lead + f * out_fs + 64,), 77, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                with torch.cuda.stream(s):
                    ctx.resize_device(d, x.data_ptr() + lead, y.data_ptr() + out_lead, f, in_fs, out_fs, s.cuda_stream)
                s.synchronize()
                got = y.cpu().numpy()
                assert (got[:out_lead] == 77).all(), "wrote in front of the first frame"
                got = got[out_lead:]
                for k in range(f):
                    _eq(got[k * out_fs:k * out_fs + out_fb].view(np.uint16).reshape(oh, ow, c), want[k],
                        f"C={c} frame {k} path {path} lead {lead}/{out_lead}")
                    assert (got[k * out_fs + out_fb:(k + 1) * out_fs] == 77).all(), "wrote into the gap between frames"
                assert (got[f * out_fs:] == 77).all()
    ctx.resize_force(L.RESIZE_AUTO)


def test_odd_bases_and_strides_are_refused(ctx):
    import torch
    iw, ih, ow, oh, c = 40, 30, 21, 17, 3
    d = L.resize_desc(iw, ih, ow, oh, c, 3, bits=16)
    x = torch.zeros(2 * iw * ih * c * 2 + 64, dtype=torch.uint8, device="cuda")
    y = torch.full((2 * ow * oh * c * 2 + 64,), 77, dtype=torch.uint8, device="cuda")
    lib = L._lib()

    def code(in_off=0, out_off=0, in_fs=0, out_fs=0, frames=1):
        return lib.lanczos_resize_device(ctx._h, ctypes.byref(d), x.data_ptr() + in_off, y.data_ptr() + out_off, frames,
                                         in_fs, out_fs, None)
    assert code(in_off=1) == L.ERR_BAD_ARG and code(out_off=1) == L.ERR_BAD_ARG
    assert code(in_fs=iw * ih * c * 2 + 1, frames=2) == L.ERR_BAD_ARG
    assert code(out_fs=ow * oh * c * 2 + 3, frames=2) == L.ERR_BAD_ARG
    torch.cuda.synchronize()
    assert int(y.min()) == 77                                   # nothing ran
    assert code(in_off=2, out_off=2, in_fs=iw * ih * c * 2 + 2, out_fs=ow * oh * c * 2 + 2, frames=2) == L.OK
    torch.cuda.synchronize()
    # the same odd addresses are fine for 8-bit samples
    d8 = L.resize_desc(iw, ih, ow, oh, c, 3)
    assert lib.lanczos_resize_device(ctx._h, ctypes.byref(d8), x.data_ptr() + 1, y.data_ptr() + 1, 2, iw * ih * c + 1,
                                     ow * oh * c + 1, None) == L.OK
    torch.cuda.synchronize()
    with pytest.raises(L.LanczosError) as e:
        ctx.resize(np.zeros((8, 8, 4), np.uint16), 4, 4, alpha=True)
    assert e.value.code == L.ERR_BAD_ARG
    for dtype in (np.int16, np.float32):
        with pytest.raises(L.LanczosError):
            ctx.resize(np.zeros((8, 8, 3), dtype), 4, 4)


@pytest.mark.parametrize("order", ["replay_then_eager", "eager_before_replay"])
@pytest.mark.parametrize("path", [L.RESIZE_FUSED, L.RESIZE_TWO_PASS])
def test_first_use_inside_capture(path, order):
    """The double tables of a shape first used inside stream capture are uploaded at once: the graph replays right, and an
    eager call gives the right samples whether it comes after the first replay or before any."""
    import torch
    c = L.Context(0)
    try:
        c.resize_force(path)
        ih, iw, oh, ow = 85 + path, 133, 49, 63
        img, img2 = _noise(ih, iw, 3, seed=9), _bilevel(ih, iw, 3, seed=10)
        d = L.resize_desc(iw, ih, ow, oh, 3, 3, bits=16)
        x = torch.from_numpy(img.view(np.int16)).cuda()
        y = torch.zeros((oh, ow, 3), dtype=torch.int16, device="cuda")
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            c.resize_device(d, x.data_ptr(), y.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert int(y.abs().max()) == 0                          # captured, not run

        def eager(what):
            y2 = torch.zeros_like(y)
            c.resize_device(d, x.data_ptr(), y2.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            _eq(y2.cpu().numpy().view(np.uint16), M.resize(img, ow, oh, 3), what)

        if order == "eager_before_replay":
            eager("eager call before any replay")
            assert int(y.abs().max()) == 0
        x.copy_(torch.from_numpy(img2.view(np.int16)))
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy().view(np.uint16), M.resize(img2, ow, oh, 3), "replay")
        x.copy_(torch.from_numpy(img.view(np.int16)))
        if order == "replay_then_eager":
            eager("eager call after the first replay")
        big = _noise(150, 200, 3, seed=11)                      # another shape: may grow the two-pass scratch
        _eq(c.resize(big, 85, 60, 3), M.resize(big, 85, 60, 3), "other shape")
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy().view(np.uint16), M.resize(img, ow, oh, 3), "replay after other work")
        del g
    finally:
        c.close()


@pytest.mark.parametrize("path", [L.RESIZE_AUTO, L.RESIZE_TWO_PASS])
def test_8bit_and_16bit_tables_of_one_axis_shape_do_not_collide(path):
    """One context, one pair of axis shapes: an 8-bit request (Pillow's fixture), the 16-bit request, the 8-bit one again,
    the 16-bit one again.  An axis cache keyed without the sample width would hand one of them the other's tables."""
    z = np.load(GOLDEN_8BIT)
    img8, want8 = z["down_RGB_in"], z["down_RGB_out"]
    ih, iw, c = img8.shape
    oh, ow = want8.shape[:2]
    img16 = _noise(ih, iw, c, seed=77)
    want16 = M.resize(img16, ow, oh, 3)
    ctx = L.Context(0)
    try:
        ctx.resize_force(path)
        for round_ in range(2):
            _eq(ctx.resize(img8, ow, oh, 3), want8, f"8-bit, round {round_}")
            _eq(ctx.resize(img16, ow, oh, 3), want16, f"16-bit, round {round_}")
        _eq(ctx.resize(img8, ow, oh, 3), M8.resize(img8, ow, oh, 3), "8-bit against its model")
    finally:
        ctx.close()
    ctx = L.Context(0)                                          # and with the 16-bit request first
    try:
        ctx.resize_force(path)
        _eq(ctx.resize(img16, ow, oh, 3), want16, "16-bit first")
        _eq(ctx.resize(img8, ow, oh, 3), want8, "8-bit after 16-bit")
    finally:
        ctx.close()
