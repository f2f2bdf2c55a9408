"""GPU checks of the float resize (LANCZOS_RESIZE_F32): every sample bit for bit Pillow's mode F fixture and the numpy model
of the contract (tests/resize32_model.py) -- NaN positions coincide, everything else is compared as a 32-bit pattern, never
within a tolerance.  The fixture on all three paths and as 3- and 4-channel stacks, every fused instance, non-finite and
denormal frames on both paths, strided batches at bases 4 and 8 bytes into an allocation with guards, misaligned requests,
first use inside stream capture, a 16-bit and a float request sharing their axis tables, and boxed resizes."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize16_model as M16
import resize32_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED_K = (7, 9, 11, 13, 17, 25)
PATHS = (L.RESIZE_FUSED, L.RESIZE_TWO_PASS)


def _golden():
    spec = importlib.util.spec_from_file_location("make_resize32_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_resize32_golden.py"))
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


def _noise(h, w, c, seed):
    return np.random.default_rng(seed).random((h, w, c), dtype=np.float32)


def _decades(h, w, c, seed):
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], (h, w, c)) * 10.0 ** rng.uniform(-30, 30, (h, w, c))).astype(np.float32)


def _hostile(h, w, c, seed):
    """unit noise with inf, -inf, NaN, denormals and near-FLT_MAX samples sprinkled in (about one sample in 2000 each)"""
    rng = np.random.default_rng(seed)
    x = rng.random((h, w, c), dtype=np.float32)
    flat = x.reshape(-1)
    n = max(1, flat.size // 2000)
    for v in (np.inf, -np.inf, np.nan, 1e-41, -3e-39, 3.3e38):
        flat[rng.choice(flat.size, n, replace=False)] = np.float32(v)
    return x


def _eq(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype)
    bad = M.differs(got, want)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} samples differ, first at {at}: "
                             f"{got[at]!r} != {want[at]!r}")


def _plan(iw, ih, ow, oh, c, a, box=None):
    p = L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, c, a, f32=True), 1, box=box)
    return p.inner if box is not None else p


def _all_paths(ctx, img, want, a, what, box=None):
    """FUSED (refused exactly where the plan says two-pass), TWO_PASS and AUTO against `want`; returns the plan."""
    ih, iw, c = img.shape
    oh, ow = want.shape[:2]
    p = _plan(iw, ih, ow, oh, c, a, box)
    try:
        ctx.resize_force(L.RESIZE_FUSED)
        if p.fused:
            _eq(ctx.resize_f32(img, ow, oh, a, box), want, f"{what} fused")
            assert ctx.last_kernel() == L.KERNEL_RESIZE_FUSED, what
        else:
            with pytest.raises(L.LanczosError) as e:
                ctx.resize_f32(img, ow, oh, a, box)
            assert e.value.code == L.ERR_UNSUPPORTED, what
        ctx.resize_force(L.RESIZE_TWO_PASS)
        _eq(ctx.resize_f32(img, ow, oh, a, box), want, f"{what} two-pass")
        assert ctx.last_kernel() == L.KERNEL_RESIZE_TWO_PASS, what
        ctx.resize_force(L.RESIZE_AUTO)
        _eq(ctx.resize_f32(img, ow, oh, a, box), want, f"{what} auto")
        assert ctx.last_kernel() == (L.KERNEL_RESIZE_FUSED if p.fused else L.KERNEL_RESIZE_TWO_PASS), what
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    return p


def test_pillow_fixture_all_paths(ctx, golden):
    """Pillow's own mode F output, every plane alone (C = 1, also as a 2-D array), boxes included."""
    g, cases = golden
    fused = two_pass = 0
    for si, kind in g.CASES:
        iw, ih, ow, oh, box = g.SHAPES[si]
        img, want = cases[g.case_name(si, kind)]
        p = _all_paths(ctx, img[..., None], want[..., None], 3, f"shape {si} {kind}", box)
        fused += p.fused
        two_pass += not p.fused
        _eq(ctx.resize_f32(img, ow, oh, 3, box), want, f"shape {si} {kind} 2-D")
    assert fused >= 20 and two_pass >= 5, (fused, two_pass)   # shapes 3 and 4 change one axis only


def test_pillow_fixture_as_channel_stacks(ctx, golden):
    """The planes of a shape stacked to 3 and 4 interleaved channels, every channel an independent F plane: a NaN or an inf
    of one channel stays in that channel."""
    g, cases = golden
    for si, (iw, ih, ow, oh, box) in enumerate(g.SHAPES):
        planes = [cases[g.case_name(s, k)] for s, k in g.CASES if s == si]
        assert len(planes) >= 2
        for c in (3, 4):
            pick = [planes[(j * 2 + c) % len(planes)] for j in range(c)]
            img = np.stack([p[0] for p in pick], axis=2)
            want = np.stack([p[1] for p in pick], axis=2)
            _all_paths(ctx, img, want, 3, f"shape {si} C={c}", box)


# horizontal ksize -> (a, in_w) at out_w = 261: whole strips and a ragged one of 5 (two of 128 with one channel, four of 64
# with three or four)
H_KSIZE = {5: (2, 200), 7: (3, 200), 9: (4, 200), 11: (3, 392), 13: (3, 496), 15: (3, 574), 17: (4, 496), 19: (3, 757),
           25: (3, 1018)}


def _hks(iw, ow, a):
    return L.resize_taps_f64_host(L.resize_desc(iw, 1, ow, 1, 1, a, f32=True), 0)[2].shape[1]


def test_every_fused_instance(ctx):
    """k_rs_fused<RsSample<4>, C, K> for every C in {1, 3, 4} and K in {7, 9, 11, 13, 17, 25}, at both edges of the buckets, a = 2, 3, 4,
    each with a vertical upscale (67 rows: more than one chunk of 32, ragged 8-row steps) and a vertical reduction, against
    the model on all three paths.  Below a bucket's K the padded taps meet real neighbours: the frames carry inf and NaN."""
    ow, ih = 261, 60
    seen = set()
    for c in (1, 3, 4):
        for hk, (a, iw) in H_KSIZE.items():
            assert _hks(iw, ow, a) == hk                       # from the public query, not recomputed
            k = next(b for b in FUSED_K if b >= hk)
            img = (_hostile if hk < k or hk % 4 == 1 else _decades)(ih, iw, c, seed=hk * 8 + c)
            for oh in (67, 23):
                p = _all_paths(ctx, img, M.resize(img, ow, oh, a), a, f"C={c} hk={hk} a={a} oh={oh}")
                assert p.fused and p.K == k, (c, hk, p.K)
                assert p.strips == (3 if c == 1 else 5)
                assert p.chunks > 1 or oh < 32
                seen.add((c, p.K, a))
    assert {(c, k) for c, k, _ in seen} == {(C, K) for C in (1, 3, 4) for K in FUSED_K}
    assert {a for _, _, a in seen} == {2, 3, 4}


@pytest.mark.parametrize("c", [1, 3, 4])
def test_geometry_edges_and_one_axis(ctx, c):
    """1-pixel inputs and outputs, ragged strips, one-axis-only resizes (one kernel of the two-pass path), the plain copy --
    bits kept, NaN payloads included -- and what the fused kernel cannot take."""
    sw = 128 if c == 1 else 64
    cases = [(f"out_w={ow}", max(2, (ow * 17 + 9) // 10), 40, ow, 23, 3) for ow in (1, sw - 1, sw, sw + 1)]
    cases += [(f"out_h={oh}", 50, max(2, (oh * 17 + 9) // 10), 37, oh, 3) for oh in (1, 8, 9, 33)]
    cases += [("in=1x1", 1, 1, 5, 4, 3), ("w 2->300", 2, 30, 300, 17, 4), ("h 300->2", 30, 300, 17, 2, 3),
              ("h only down", 77, 90, 77, 31, 3), ("w only up", 31, 77, 90, 77, 2), ("ksize 27", 1100, 24, 261, 23, 3)]
    for name, iw, ih, ow, oh, a in cases:
        img = _hostile(ih, iw, c, seed=iw + 3 * oh + c)
        p = _all_paths(ctx, img, M.resize(img, ow, oh, a), a, f"C={c} {name} {iw}x{ih}->{ow}x{oh}")
        if iw == ow or ih == oh or name in ("ksize 27", "h 300->2"):
            assert not p.fused, name
    img = _hostile(17, 31, c, seed=5)
    img.reshape(-1).view(np.uint32)[3] = 0x7FC12345            # a NaN with a payload
    got = ctx.resize_f32(img, 31, 17)
    assert np.array_equal(got.view(np.uint32), img.view(np.uint32)), "no pass is a copy"


@pytest.mark.parametrize("kind", ["nonfinite", "denormal", "overflow", "tinyneg"])
def test_nonfinite_and_denormal_frames_on_both_paths(ctx, golden, kind):
    """Larger frames of the fixture's hostile kinds against the model on both paths: several strips, chunks and staging
    rounds, down and up."""
    g, _ = golden
    for iw, ih, ow, oh in ((300, 170, 157, 75), (90, 70, 290, 200)):
        img = np.stack([g.make_input(1 + j, kind, iw, ih) for j in range(3)], axis=2)
        want = M.resize(img, ow, oh, 3)
        if kind == "denormal":
            assert ((np.abs(want) < M.FLT_MIN) & (want != 0)).mean() > 0.5
        if kind == "tinyneg":
            assert (want.view(np.uint32) == 0x80000000).any()
        if kind == "overflow":
            assert np.isinf(want).any()
        p = _all_paths(ctx, img, want, 3, f"{kind} {iw}x{ih}->{ow}x{oh}")
        assert p.fused


def test_strided_batches_at_4_and_8_byte_offsets_with_guards(ctx):
    """Frame strides larger than a frame, bases 4 and 8 bytes into an allocation, NaN poison in every gap and in front of
    the first frame (a kernel that multiplied it, even by 0.0, would show); the bytes around every output frame stay."""
    import torch
    for c in (3, 1, 4):
        f, ih, iw, ow, oh = 4, 135, 241, 150, 75
        frames = np.stack([_noise(ih, iw, c, seed=50 + k) if k % 2 else _hostile(ih, iw, c, seed=50 + k) for k in range(f)])
        want = M.resize(frames, ow, oh, 3)
        in_fb, out_fb = ih * iw * c * 4, oh * ow * c * 4
        in_fs, out_fs = in_fb + 12, out_fb + 20
        s = torch.cuda.Stream()
        d = L.resize_desc(iw, ih, ow, oh, c, 3, f32=True)
        for lead, out_lead in ((0, 0), (4, 8), (8, 4)):
            n = lead + f * in_fs + 64
            x = torch.from_numpy(np.full(n // 4 + 1, np.nan, np.float32).view(np.uint8)[:n].copy()).cuda()   # poison
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
                    _eq(got[k * out_fs:k * out_fs + out_fb].copy().view(np.float32).reshape(oh, ow, c), want[k],
                        f"C={c} frame {k} path {path} lead {lead}/{out_lead}")
                    assert (got[k * out_fs + out_fb:(k + 1) * out_fs] == 77).all(), "wrote into the gap between frames"
                assert (got[f * out_fs:] == 77).all()
    ctx.resize_force(L.RESIZE_AUTO)


def test_misaligned_bases_and_strides_are_refused(ctx):
    import torch
    iw, ih, ow, oh, c = 40, 30, 21, 17, 3
    d = L.resize_desc(iw, ih, ow, oh, c, 3, f32=True)
    x = torch.zeros(2 * iw * ih * c * 4 + 64, dtype=torch.uint8, device="cuda")
    y = torch.full((2 * ow * oh * c * 4 + 64,), 77, dtype=torch.uint8, device="cuda")
    lib = L._lib()

    def code(in_off=0, out_off=0, in_fs=0, out_fs=0, frames=1):
        return lib.lanczos_resize_device(ctx._h, ctypes.byref(d), x.data_ptr() + in_off, y.data_ptr() + out_off, frames,
                                         in_fs, out_fs, None)
    for off in (1, 2, 3):
        assert code(in_off=off) == L.ERR_BAD_ARG and code(out_off=off) == L.ERR_BAD_ARG
    assert code(in_fs=iw * ih * c * 4 + 2, frames=2) == L.ERR_BAD_ARG
    assert code(out_fs=ow * oh * c * 4 + 6, frames=2) == L.ERR_BAD_ARG
    assert lib.lanczos_resize_device_ex(ctx._h, ctypes.byref(d), ctypes.byref(L.resize_opts(d, reducing_gap=2.0)),
                                        x.data_ptr(), y.data_ptr(), 1, 0, 0, None) == L.ERR_BAD_ARG
    torch.cuda.synchronize()
    assert int(y.min()) == 77                                   # nothing ran
    assert code(in_off=4, out_off=8, in_fs=iw * ih * c * 4 + 4, out_fs=ow * oh * c * 4 + 8, frames=2) == L.OK
    torch.cuda.synchronize()
    for dtype in (np.float64, np.uint8):
        with pytest.raises(L.LanczosError):
            ctx.resize_f32(np.zeros((8, 8, 3), dtype), 4, 4)
    with pytest.raises(L.LanczosError):
        ctx.resize(np.zeros((8, 8, 3), np.float32), 4, 4)


@pytest.mark.parametrize("path", PATHS)
def test_first_use_inside_capture_then_replay_and_eager(path):
    """The tables of a shape first used inside stream capture are uploaded at once: the graph replays right, and an eager
    call after it gives the right samples."""
    import torch
    c = L.Context(0)
    try:
        c.resize_force(path)
        ih, iw, oh, ow = 85 + path, 133, 49, 63
        img, img2 = _noise(ih, iw, 3, seed=9), _hostile(ih, iw, 3, seed=10)
        d = L.resize_desc(iw, ih, ow, oh, 3, 3, f32=True)
        x = torch.from_numpy(img).cuda()
        y = torch.zeros((oh, ow, 3), dtype=torch.float32, device="cuda")
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            c.resize_device(d, x.data_ptr(), y.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert int(y.view(torch.int32).abs().max()) == 0        # captured, not run
        x.copy_(torch.from_numpy(img2))
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), M.resize(img2, ow, oh, 3), "replay")
        x.copy_(torch.from_numpy(img))
        y2 = torch.zeros_like(y)
        c.resize_device(d, x.data_ptr(), y2.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _eq(y2.cpu().numpy(), M.resize(img, ow, oh, 3), "eager call after the first replay")
        big = _noise(150, 200, 3, seed=11)                      # another shape: may grow the two-pass scratch
        _eq(c.resize_f32(big, 85, 60, 3), M.resize(big, 85, 60, 3), "other shape")
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        _eq(y.cpu().numpy(), M.resize(img, ow, oh, 3), "replay after other work")
        del g
    finally:
        c.close()


@pytest.mark.parametrize("first", ["u16", "f32"])
@pytest.mark.parametrize("path", [L.RESIZE_AUTO, L.RESIZE_TWO_PASS])
def test_16bit_and_float_requests_share_one_axis_shape(path, first):
    """One context, one pair of axis shapes, a 16-bit and a float request in either order and again: both run on the same
    cached double tables, and neither disturbs the other."""
    ih, iw, oh, ow, c = 97, 141, 45, 60, 3
    img16 = np.random.default_rng(77).integers(0, 65536, (ih, iw, c), dtype=np.uint16)
    img32 = _hostile(ih, iw, c, seed=78)
    want16, want32 = M16.resize(img16, ow, oh, 3), M.resize(img32, ow, oh, 3)
    ctx = L.Context(0)
    try:
        ctx.resize_force(path)
        for round_ in range(2):
            for which in (("u16", "f32") if first == "u16" else ("f32", "u16")):
                if which == "u16":
                    assert np.array_equal(ctx.resize(img16, ow, oh, 3), want16), f"16-bit, round {round_}"
                else:
                    _eq(ctx.resize_f32(img32, ow, oh, 3), want32, f"float, round {round_}")
    finally:
        ctx.close()


@pytest.mark.parametrize("c", [1, 3])
def test_boxed_resize_on_both_paths(ctx, c):
    """A fractional box, a fractional shift at equal size, and whole-pixel columns with reduced rows (zero weights at the
    end of every horizontal window, next to NaN and inf samples), against the model."""
    iw, ih = 150, 110
    img = _hostile(ih, iw, c, seed=90 + c)
    for ow, oh, box in ((71, 64, (10.3, 7.7, 140.1, 101.2)), (120, 90, (13.5, 9.25, 133.5, 99.25)),
                        (120, 64, (13, 0, 133, 110)), (200, 170, (20.5, 11, 99.75, 80))):
        want = M.resize(img, ow, oh, 3, box)
        p = _all_paths(ctx, img, want, 3, f"C={c} box {box}", box)
        assert p.fused
    # a box that leaves one axis idle runs one pass
    want = M.resize(img, iw, 64, 3, (0, 3.5, iw, 100))
    _all_paths(ctx, img, want, 3, "vertical box only", (0, 3.5, iw, 100))
