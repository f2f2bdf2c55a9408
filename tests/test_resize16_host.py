"""CPU-only checks of the 16-bit resize (LANCZOS_RESIZE_U16, Pillow's mode I;16): the numpy model equals the committed
Pillow fixture byte for byte and the fixture exercises the wrapping store, the library's double tables equal the model's
bit for bit, descriptor validation, the plan of 16-bit requests, and the dtypes Context.resize refuses.  No GPU needed."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize16_model as M
import resize_model as M8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_pillow_u16.npz")
GOLDEN_8BIT = os.path.join(ROOT, "tests", "golden", "resize_pillow.npz")


def golden_module():
    spec = importlib.util.spec_from_file_location("make_resize16_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_resize16_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_equals_model_and_exercises_the_wrap():
    g = golden_module()
    cases = g.load(GOLDEN)
    assert len(cases) == len(g.SHAPES) * len(g.PATTERNS) == 28
    assert os.path.getsize(GOLDEN) <= os.path.getsize(GOLDEN_8BIT)
    total = differs_saturating = 0
    stats = {}
    for si, (iw, ih, ow, oh) in enumerate(g.SHAPES):
        for pattern in g.PATTERNS:
            img, want = cases[g.case_name(si, pattern)]
            assert img.shape == (ih, iw) and want.shape == (oh, ow) and want.dtype == np.uint16
            assert np.array_equal(M.resize(img, ow, oh, 3, stats=stats), want), (si, pattern)
            total += want.size
            differs_saturating += int((M.resize(img, ow, oh, 3, saturate=True) != want).sum())
    # a condition on the fixture: a kernel that saturates to 65535 instead of storing as Pillow does cannot pass on it
    assert differs_saturating * 10 >= total, (differs_saturating, total)
    assert stats["vmin"] < 0 and stats["vmax"] > 65535, stats


def test_model_equals_pillow_where_pillow_imports():
    pytest.importorskip("PIL")
    g = golden_module()
    rng = np.random.default_rng(16)
    for k in range(12):
        iw, ih, ow, oh = (int(v) for v in rng.integers(1, 70, 4))
        img = rng.integers(0, 65536, (ih, iw), dtype=np.uint16) if k % 2 else \
            (rng.integers(0, 2, (ih, iw)) * 65535).astype(np.uint16)
        assert np.array_equal(M.resize(img, ow, oh, 3), g.pillow_resize(img, ow, oh)), (iw, ih, ow, oh)


def test_store_is_pillows():
    v = np.array([-70000, -257, -256, -1, 0, 1, 255, 256, 65535, 65536, 65537, 65791, 65792, 83297, 200000], np.int64)
    want = [0, 0, 0, 0, 0, 1, 255, 256, 65535, 0xFF00, 0xFF01, 0xFFFF, 0xFF00, 0xFF00 | (83297 & 255), 0xFF00 | (200000 & 255)]
    assert M.store(v).tolist() == want


SWEEP = [1, 2, 3, 5, 7, 16, 17, 40, 97, 160, 333, 1000, 1080, 1920, 3840]


@pytest.mark.parametrize("a", [2, 3, 4])
def test_f64_tables_equal_the_model_bit_for_bit(a):
    pairs = [(i, o) for i in SWEEP for o in SWEEP if i * o <= 1_000_000]
    assert any(i > o for i, o in pairs) and any(i < o for i, o in pairs)
    for in_n, out_n in pairs:
        for axis in (0, 1):
            # neither table function looks at the sample width of the descriptor
            d = L.resize_desc(in_n if axis == 0 else 3, in_n if axis == 1 else 3,
                              out_n if axis == 0 else 3, out_n if axis == 1 else 3, 3, a, bits=16 if axis == 0 else 8)
            f, c, k = L.resize_taps_f64_host(d, axis)
            f8, c8, _ = L.resize_taps_host(d, axis)
            mf, mc, mk = M.axis_tables(in_n, out_n, a)
            assert k.shape == (out_n, M.ksize(in_n, out_n, a)) and k.dtype == np.float64
            assert np.array_equal(k.view(np.uint64), mk.view(np.uint64)), (in_n, out_n, a, axis)
            assert np.array_equal(f, mf) and np.array_equal(c, mc)
            assert np.array_equal(f, f8) and np.array_equal(c, c8)
            ks = np.arange(k.shape[1])[None, :]
            assert (k.view(np.uint64)[ks >= c[:, None]] == 0).all()      # padded taps are +0.0


def test_f64_tables_geometry_is_the_8bit_one():
    for in_n, out_n in [(97, 40), (40, 97), (3840, 1920), (1080, 2160), (1, 9), (160, 7)]:
        mf, mc, _ = M.axis_tables(in_n, out_n, 3)
        f8, c8, _ = M8.axis_tables(in_n, out_n, 3)
        assert np.array_equal(mf, f8) and np.array_equal(mc, c8)


def test_ksize_query_and_argument_checks_of_the_f64_tables():
    lib = L._lib()
    d = L.resize_desc(3840, 2160, 160, 90, 3, 3, bits=16)
    ks = ctypes.c_int()
    assert lib.lanczos_resize_taps_f64_host(ctypes.byref(d), 1, None, None, None, ctypes.byref(ks)) == L.OK
    assert ks.value == 145
    assert lib.lanczos_resize_taps_f64_host(ctypes.byref(d), 2, None, None, None, ctypes.byref(ks)) == L.ERR_BAD_ARG
    assert lib.lanczos_resize_taps_f64_host(ctypes.byref(d), 0, None, None, None, None) == L.ERR_BAD_ARG
    buf = np.zeros(160, np.int32)
    assert lib.lanczos_resize_taps_f64_host(ctypes.byref(d), 0, buf.ctypes.data, None, None,
                                            ctypes.byref(ks)) == L.ERR_BAD_ARG


def test_validation_of_the_flag_word():
    lib = L._lib()
    assert L.RESIZE_U16 == 4

    def code(flags, channels=3, r1=0):
        dd = L.ResizeDesc()
        rc = lib.lanczos_resize_desc_init_ex(ctypes.byref(dd), 64, 48, 20, 100, channels, 3, flags)
        dd.reserved[1] = r1
        return rc if r1 == 0 else lib.lanczos_resize_validate(ctypes.byref(dd))

    for channels in (1, 3, 4):
        assert code(4, channels) == L.OK
        assert code(0, channels) == L.OK
    assert code(1, 4) == L.OK
    assert code(4, 2) == L.ERR_BAD_ARG
    for flags in (5, 6, 2, 3, 7, 8, 12, -1, 1 << 16, 4 | 1 << 16):
        for channels in (3, 4):
            assert code(flags, channels) == L.ERR_BAD_ARG, (flags, channels)
    assert code(4, 3, r1=1) == L.ERR_BAD_ARG
    d = L.resize_desc(64, 48, 20, 100, 3, 3, bits=16)
    assert d.reserved[0] == 4 and d.reserved[1] == 0
    assert L.resize_desc(64, 48, 20, 100, 4, 3, alpha=True).reserved[0] == 1
    with pytest.raises(L.LanczosError) as e:
        L.resize_desc(64, 48, 20, 100, 4, 3, alpha=True, bits=16)
    assert e.value.code == L.ERR_BAD_ARG
    with pytest.raises(L.LanczosError):
        L.resize_desc(64, 48, 20, 100, 3, 3, bits=12)
    # odd strides / bases of a 16-bit request are refused before anything is launched (here: without a context at all,
    # which is refused as well; tests/test_resize16_gpu.py checks the same calls with a live context)
    assert lib.lanczos_resize_device(None, ctypes.byref(d), 2, 4, 1, 64 * 48 * 6 + 1, 0, None) == L.ERR_BAD_ARG


def test_plan_of_16bit_requests():
    fits = [(3840, 2160, 1920, 1080), (1920, 1080, 3840, 2160), (1920, 1080, 1280, 720), (640, 480, 1000, 700),
            (64, 48, 31, 17), (97, 53, 33, 200)]
    for c in (1, 3, 4):
        for (iw, ih, ow, oh) in fits:
            d16 = L.resize_desc(iw, ih, ow, oh, c, 3, bits=16)
            p = L.resize_plan_host(d16, 4)
            sw = 64 if c == 4 else 128
            assert p.fused == 1, (iw, ih, ow, oh, c)
            assert p.K >= M.ksize(iw, ow, 3) and p.K in (7, 9, 11, 13, 17, 25)
            assert p.strips == -(-ow // sw)
            assert p.rows_per_chunk % 8 == 0 and p.chunks == -(-oh // p.rows_per_chunk)
            _, vc, _ = M.axis_tables(ih, oh, 3)
            assert p.ring_rows >= int(vc.max())
            assert p.stage_rows >= 1
            assert p.lds_bytes == p.ring_rows * sw * c * 2 + p.stage_rows * p.stage_dw * 4   # 2-byte ring samples
            assert 0 < p.lds_bytes <= 80 * 1024
            # the 8-bit plan of the same shape is what it was: 1-byte ring rows of its own strip width
            p8 = L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, c, 3), 4)
            sw8 = 64 if c == 4 else 256
            assert p8.fused == 1 and p8.lds_bytes == p8.ring_rows * sw8 * c + p8.stage_rows * p8.stage_dw * 4
    # two-pass: more horizontal taps than the widest instance / a ring beyond 80 KiB / one axis only
    for (iw, ih, ow, oh) in [(3840, 2160, 160, 90), (3840, 2160, 3840, 1080), (3840, 2160, 1920, 2160)]:
        p = L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, 3, 3, bits=16), 1)
        assert p.fused == 0 and p.lds_bytes == 0 and p.K == 0
    # four channels keep their strip width, so ring and staging rows are twice as large: a reduction by 12 (156 ring rows
    # of 256 bytes) still fuses with 8-bit samples and falls to two passes with 16-bit ones (156 rows of 512 bytes leave no
    # room for the staging rows within 80 KiB)
    p8 = L.resize_plan_host(L.resize_desc(1024, 4800, 512, 400, 4, 3), 1)
    p16 = L.resize_plan_host(L.resize_desc(1024, 4800, 512, 400, 4, 3, bits=16), 1)
    assert p8.fused == 1 and p8.ring_rows == 156 and p16.fused == 0


def test_context_resize_dtype_check_needs_no_gpu():
    # the dtype is looked at before anything touches the device
    ctx = L.Context.__new__(L.Context)
    ctx._h = ctypes.c_void_p()
    for dtype in (np.int16, np.float32, np.int32, np.float64):
        with pytest.raises(L.LanczosError) as e:
            ctx.resize(np.zeros((8, 8, 3), dtype), 4, 4)
        assert e.value.code == L.ERR_BAD_ARG
        assert "uint16" in str(e.value)
