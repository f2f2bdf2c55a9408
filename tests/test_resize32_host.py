"""CPU-only checks of the float resize (LANCZOS_RESIZE_F32, Pillow's mode F): the numpy model equals the committed Pillow
fixture bit for bit and the fixture tells the contract from its near misses, the model equals Pillow where Pillow imports,
descriptor validation, the plans of float requests, the tables a float descriptor runs on, and the dtype check of
Context.resize_f32.  No GPU needed."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize32_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_pillow_f32.npz")
GOLDEN_8BIT = os.path.join(ROOT, "tests", "golden", "resize_pillow.npz")


def golden_module():
    spec = importlib.util.spec_from_file_location("make_resize32_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_resize32_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixture():
    g = golden_module()
    return g, g.load(GOLDEN)


def test_fixture_equals_model(fixture):
    g, cases = fixture
    assert len(cases) == len(g.CASES) == 33
    assert os.path.getsize(GOLDEN) <= os.path.getsize(GOLDEN_8BIT)
    for si, kind in g.CASES:
        iw, ih, ow, oh, box = g.SHAPES[si]
        img, want = cases[g.case_name(si, kind)]
        assert img.shape == (ih, iw) and want.shape == (oh, ow) and want.dtype == np.float32
        got = M.resize(img, ow, oh, 3, box)
        assert M.same(got, want), (si, kind, int(M.differs(got, want).sum()))
        assert np.isnan(want).mean() <= 0.15, (si, kind)


def test_fixture_tells_the_near_misses_apart(fixture):
    """The conditions the generator refuses to write a fixture without, checked on the committed file."""
    g, cases = fixture
    zero_weight_guard = 0
    for si, kind in g.CASES:
        iw, ih, ow, oh, box = g.SHAPES[si]
        img, want = cases[g.case_name(si, kind)]

        def share(**kw):
            return float(M.differs(M.resize(img, ow, oh, 3, box, **kw), want).mean())
        x0, y0, x1, y1 = box if box is not None else (0, 0, iw, ih)
        both = M.MB.axis_runs(iw, ow, x0, x1) and M.MB.axis_runs(ih, oh, y0, y1)
        if kind == "noise":
            assert share(acc32=True) >= 0.10, si
            if both:
                assert share(mid64=True) >= 0.10, si
        elif kind == "denormal":
            assert (np.abs(img) < M.FLT_MIN).all() and (img != 0).all()
            assert share(flush=True) == 1.0, si
        elif kind == "overflow":
            assert np.isinf(want).any(), si
        elif kind == "tinyneg":
            assert (want.view(np.uint32) == 0x80000000).any(), si       # -0.0 stored
        elif kind == "nonfinite":
            assert np.isnan(want).any() and np.isinf(want).any(), si
            assert share(pad_to=M.bucket) > 0, si
            if g.zero_weight_taps(si, M) and share(skip_zero_k=True) > 0:
                zero_weight_guard += 1
    assert zero_weight_guard >= 1                                         # a k == 0 guard is told from a count guard
    kinds = {k for _, k in g.CASES}
    assert kinds == {"noise", "decades", "denormal", "overflow", "tinyneg", "nonfinite"}


def test_model_equals_pillow_where_pillow_imports():
    pytest.importorskip("PIL")
    g = golden_module()
    rng = np.random.default_rng(32)
    for k in range(12):
        iw, ih, ow, oh = (int(v) for v in rng.integers(1, 70, 4))
        img = rng.random((ih, iw), dtype=np.float32) if k % 2 else \
            (rng.choice([-1.0, 1.0], (ih, iw)) * 10.0 ** rng.uniform(-30, 30, (ih, iw))).astype(np.float32)
        if k % 3 == 0:
            img.reshape(-1)[rng.integers(0, img.size)] = [np.inf, -np.inf, np.nan, 1e-42][k // 3]
        box = None
        if k >= 8:
            x0, y0 = rng.uniform(0, iw / 3), rng.uniform(0, ih / 3)
            box = (x0, y0, rng.uniform(x0 + iw / 3, iw), rng.uniform(y0 + ih / 3, ih))
        got, want = M.resize(img, ow, oh, 3, box), g.pillow_resize(img, ow, oh, box)
        assert M.same(got, want), (iw, ih, ow, oh, box)


def test_validation_of_the_flag_word():
    lib = L._lib()
    assert L.RESIZE_F32 == 16

    def code(flags, channels=3):
        dd = L.ResizeDesc()
        return lib.lanczos_resize_desc_init_ex(ctypes.byref(dd), 64, 48, 20, 100, channels, 3, flags)

    for channels in (1, 3, 4):
        assert code(16, channels) == L.OK
    assert code(16, 2) == L.ERR_BAD_ARG
    for flags in (17, 20, 21, 16 | 2, 16 | 8, 16 | 32, 16 | 1 << 16):
        for channels in (3, 4):
            assert code(flags, channels) == L.ERR_BAD_ARG, (flags, channels)
    d = L.resize_desc(64, 48, 20, 100, 3, 3, f32=True)
    assert d.reserved[0] == 16 and d.reserved[1] == 0
    for kw in ({"alpha": True}, {"bits": 16}):
        with pytest.raises(L.LanczosError) as e:
            L.resize_desc(64, 48, 20, 100, 4, 3, f32=True, **kw)
        assert e.value.code == L.ERR_BAD_ARG
    # a gap is refused for floats, a box is not
    with pytest.raises(L.LanczosError) as e:
        L.resize_plan_host(d, 1, reducing_gap=2.0)
    assert e.value.code == L.ERR_BAD_ARG
    with pytest.raises(L.LanczosError):
        L.resize_taps_f64_host(d, 0, reducing_gap=1.0)
    assert L.resize_plan_host(d, 1, box=(1.5, 2, 60, 40.25)).pass_h == 1
    # misaligned bases and strides are refused before anything is launched (here: without a context at all, which is
    # refused as well; tests/test_resize32_gpu.py checks the same calls with a live context)
    fb = 64 * 48 * 3 * 4
    assert lib.lanczos_resize_device(None, ctypes.byref(d), 4, 8, 2, fb + 2, 0, None) == L.ERR_BAD_ARG
    assert lib.lanczos_resize_device(None, ctypes.byref(d), 6, 8, 1, 0, 0, None) == L.ERR_BAD_ARG


def test_plan_of_float_requests():
    fits = [(3840, 2160, 1920, 1080), (1920, 1080, 3840, 2160), (1920, 1080, 1280, 720), (640, 480, 1000, 700),
            (64, 48, 31, 17), (97, 53, 33, 200)]
    for c in (1, 3, 4):
        sw = 128 if c == 1 else 64
        for (iw, ih, ow, oh) in fits:
            p = L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, c, 3, f32=True), 4)
            assert p.fused == 1, (iw, ih, ow, oh, c)
            assert p.K >= M.M16.ksize(iw, ow, 3) and p.K in M.FUSED_K
            assert p.strips == -(-ow // sw)
            assert p.rows_per_chunk % 8 == 0 and p.chunks == -(-oh // p.rows_per_chunk)
            _, vc, _ = M.M16.axis_tables(ih, oh, 3)
            hf, _, _ = M.M16.axis_tables(iw, ow, 3)
            assert p.ring_rows >= int(vc.max())
            # a staged row holds every window of the widest strip: K * C dwords from the last column's first tap on
            span = max(int(hf[min(ow, x0 + sw) - 1] - hf[x0]) for x0 in range(0, ow, sw))
            assert p.stage_dw >= span * c + p.K * c
            assert p.lds_bytes == p.ring_rows * sw * c * 4 + p.stage_rows * p.stage_dw * 4   # 4-byte ring samples
            assert 0 < p.lds_bytes <= 80 * 1024
            # the 8-bit and 16-bit plans of the same shape are what they were
            p8 = L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, c, 3), 4)
            sw8 = 64 if c == 4 else 256
            assert p8.fused == 1 and p8.lds_bytes == p8.ring_rows * sw8 * c + p8.stage_rows * p8.stage_dw * 4
            p16 = L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, c, 3, bits=16), 4)
            sw16 = 64 if c == 4 else 128
            assert p16.fused == 1 and p16.lds_bytes == p16.ring_rows * sw16 * c * 2 + p16.stage_rows * p16.stage_dw * 4
    # two-pass: more horizontal taps than the widest instance / one axis only
    for (iw, ih, ow, oh) in [(3840, 2160, 160, 90), (3840, 2160, 3840, 1080), (3840, 2160, 1920, 2160)]:
        p = L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, 3, 3, f32=True), 1)
        assert p.fused == 0 and p.lds_bytes == 0 and p.K == 0
    # the flip at the LDS limit, on shapes that fuse with 8-bit and with 16-bit samples (ring rows of 256 bytes there).  One
    # channel, ring rows of 128 floats = 512 bytes; a vertical reduction by r needs a ring of 13 r rows.  r = 11: 143 rows are
    # 73 216 bytes and the staging rows fit beside them under 80 KiB; r = 12: 156 rows are 79 872 bytes and not even the
    # smallest staging area (4 rows of more than 256 dwords) fits
    p11 = L.resize_plan_host(L.resize_desc(1024, 4400, 512, 400, 1, 3, f32=True), 1)
    p12 = L.resize_plan_host(L.resize_desc(1024, 4800, 512, 400, 1, 3, f32=True), 1)
    assert p11.fused == 1 and p11.ring_rows == 143 and p11.stage_rows >= 4
    assert p11.ring_rows * 512 + p11.stage_rows * p11.stage_dw * 4 == p11.lds_bytes <= 80 * 1024
    assert p12.fused == 0 and 156 * 512 + 4 * 256 * 4 > 80 * 1024
    for kw in ({}, {"bits": 16}):
        q = L.resize_plan_host(L.resize_desc(1024, 4800, 512, 400, 1, 3, **kw), 1)
        assert q.fused == 1 and q.ring_rows == 156
    # four channels: a reduction by 12 (156 ring rows) fuses with 8-bit samples, not with 16-bit ones and not with floats
    assert L.resize_plan_host(L.resize_desc(1024, 4800, 512, 400, 4, 3), 1).fused == 1
    assert L.resize_plan_host(L.resize_desc(1024, 4800, 512, 400, 4, 3, f32=True), 1).fused == 0


def test_tables_of_a_float_descriptor_are_the_16bit_ones():
    for (iw, ih, ow, oh) in [(97, 53, 33, 200), (64, 48, 128, 31), (1920, 1080, 1280, 720)]:
        d32 = L.resize_desc(iw, ih, ow, oh, 3, 3, f32=True)
        d16 = L.resize_desc(iw, ih, ow, oh, 3, 3, bits=16)
        for axis in (0, 1):
            for kw in ({}, {"box": (1.25, 2.5, iw - 3.0, ih - 0.75)}):
                f, c, k = L.resize_taps_f64_host(d32, axis, **kw)
                f16, c16, k16 = L.resize_taps_f64_host(d16, axis, **kw)
                assert np.array_equal(f, f16) and np.array_equal(c, c16)
                assert np.array_equal(k.view(np.uint64), k16.view(np.uint64))
            mf, mc, mk = M.tables(iw if axis == 0 else ih, ow if axis == 0 else oh, 3)
            f, c, k = L.resize_taps_f64_host(d32, axis)
            assert np.array_equal(f, mf) and np.array_equal(c, mc) and np.array_equal(k.view(np.uint64), mk.view(np.uint64))


def test_resize_f32_dtype_check_needs_no_gpu():
    # the dtype is looked at before anything touches the device
    ctx = L.Context.__new__(L.Context)
    ctx._h = ctypes.c_void_p()
    for dtype in (np.float64, np.float16, np.uint8, np.uint16, np.int32):
        with pytest.raises(L.LanczosError) as e:
            ctx.resize_f32(np.zeros((8, 8, 3), dtype), 4, 4)
        assert e.value.code == L.ERR_BAD_ARG
        assert "float32" in str(e.value)
    with pytest.raises(L.LanczosError) as e:
        ctx.resize_f32(np.zeros(8, np.float32), 4, 4)
    assert e.value.code == L.ERR_BAD_ARG
    # and Context.resize goes on refusing floats
    with pytest.raises(L.LanczosError) as e:
        ctx.resize(np.zeros((8, 8, 3), np.float32), 4, 4)
    assert e.value.code == L.ERR_BAD_ARG and "uint16" in str(e.value)
