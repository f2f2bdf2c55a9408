"""CPU-only checks of the resize-to-any-size entry (lanczos_resize_*, Pillow's contract): the numpy model equals Pillow,
the committed fixture equals the model, the library's host tables equal the model's bit for bit, the fixed-point ranges
the kernels rely on hold, descriptor validation, and the CLI's argument checks.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_pillow.npz")
CHANNELS = {"L": 1, "RGB": 3, "RGBX": 4}


def _cases():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_resize_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_resize_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _pillow(img, out_w, out_h, mode):
    from PIL import Image
    h, w, c = img.shape
    r = Image.frombytes(mode, (w, h), img.tobytes()).resize((out_w, out_h), Image.LANCZOS)
    return np.frombuffer(r.tobytes(), np.uint8).reshape(out_h, out_w, c)


def test_model_equals_pillow_on_the_fixture_shapes():
    pytest.importorskip("PIL")
    g = _cases()
    for i, (name, iw, ih, ow, oh, mode) in enumerate(g.CASES):
        img = g.make_input(i, iw, ih, CHANNELS[mode])
        assert np.array_equal(M.resize(img, ow, oh, 3), _pillow(img, ow, oh, mode)), name


def test_model_equals_pillow_on_random_sizes():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(2024)
    for k in range(24):
        iw, ih, ow, oh = (int(v) for v in rng.integers(1, 90, 4))
        mode = ("L", "RGB", "RGBX")[k % 3]
        img = rng.integers(0, 256, (ih, iw, CHANNELS[mode]), dtype=np.uint8)
        assert np.array_equal(M.resize(img, ow, oh, 3), _pillow(img, ow, oh, mode)), (iw, ih, ow, oh, mode)


def test_fixture_equals_model():
    z = np.load(GOLDEN)
    g = _cases()
    assert os.path.getsize(GOLDEN) < 200 * 1024
    for i, (name, iw, ih, ow, oh, mode) in enumerate(g.CASES):
        img = z[f"{name}_in"]
        assert img.shape == (ih, iw, CHANNELS[mode])
        assert np.array_equal(img, g.make_input(i, iw, ih, CHANNELS[mode])), name
        assert np.array_equal(M.resize(img, ow, oh, 3), z[f"{name}_out"]), name


SWEEP = [1, 2, 3, 5, 7, 16, 17, 40, 97, 160, 333, 1000, 1080, 1920, 3840]


@pytest.mark.parametrize("a", [2, 3, 4])
def test_host_tables_equal_the_model(a):
    pairs = [(i, o) for i in SWEEP for o in SWEEP if i * o <= 4_000_000]
    for in_n, out_n in pairs:
        for axis in (0, 1):
            d = L.resize_desc(in_n if axis == 0 else 3, in_n if axis == 1 else 3,
                              out_n if axis == 0 else 3, out_n if axis == 1 else 3, 3, a)
            f, c, k = L.resize_taps_host(d, axis)
            mf, mc, mk = M.axis_tables(in_n, out_n, a)
            assert k.shape == (out_n, M.ksize(in_n, out_n, a))
            assert np.array_equal(f, mf) and np.array_equal(c, mc) and np.array_equal(k, mk), (in_n, out_n, a, axis)
            assert (f >= 0).all() and (f + c <= in_n).all() and (c >= 1).all()
            ks = np.arange(k.shape[1])[None, :]
            assert (k[ks >= c[:, None]] == 0).all()


@pytest.mark.parametrize("a", [2, 3, 4])
def test_coefficient_and_accumulator_bounds(a):
    """Every coefficient fits a signed 24-bit operand (the kernels multiply with v_mad_i32_i24) and the int32 accumulator
    cannot overflow: 255 * sum|k| + 2^21 < 2^31.  All in, out <= 40."""
    kmin, kmax, accmax = 0, 0, 0
    for in_n in range(1, 41):
        for out_n in range(1, 41):
            d = L.resize_desc(in_n, 1, out_n, 1, 1, a)
            _, _, k = L.resize_taps_host(d, 0)
            kmin, kmax = min(kmin, int(k.min())), max(kmax, int(k.max()))
            accmax = max(accmax, int((255 * np.abs(k.astype(np.int64)).sum(axis=1)).max()) + (1 << 21))
    assert -(1 << 23) < kmin and kmax < (1 << 23), (kmin, kmax)
    assert accmax < (1 << 31), accmax
    assert kmax < 1.36 * (1 << 22) and kmin > -0.36 * (1 << 22)   # what the contract's sweep found


def test_ksize_query_and_validation():
    lib = L._lib()
    d = L.resize_desc(3840, 2160, 160, 90, 3, 3)
    ks = ctypes.c_int()
    assert lib.lanczos_resize_taps_host(ctypes.byref(d), 1, None, None, None, ctypes.byref(ks)) == L.OK
    assert ks.value == 145                       # the thumbnail case of the two-pass path
    assert lib.lanczos_resize_taps_host(ctypes.byref(d), 2, None, None, None, ctypes.byref(ks)) == L.ERR_BAD_ARG
    buf = np.zeros(160, np.int32)
    assert lib.lanczos_resize_taps_host(ctypes.byref(d), 0, buf.ctypes.data, None, None, ctypes.byref(ks)) == L.ERR_BAD_ARG

    def code(**kw):
        args = dict(in_w=64, in_h=48, out_w=20, out_h=100, channels=3, a=3)
        args.update(kw)
        dd = L.ResizeDesc()
        return lib.lanczos_resize_desc_init(ctypes.byref(dd), args["in_w"], args["in_h"], args["out_w"], args["out_h"],
                                            args["channels"], args["a"])

    assert code() == L.OK
    assert code(in_w=65535, out_h=1) == L.OK
    for kw in (dict(in_w=0), dict(in_h=0), dict(out_w=0), dict(out_h=0), dict(in_w=65536), dict(out_h=65536),
               dict(out_w=-3), dict(channels=2), dict(channels=0), dict(channels=5), dict(a=1), dict(a=5)):
        assert code(**kw) == L.ERR_BAD_ARG, kw
    for i in (0, 1):
        dd = L.resize_desc(64, 48, 20, 100, 3, 3)
        dd.reserved[i] = 7
        assert lib.lanczos_resize_validate(ctypes.byref(dd)) == L.ERR_BAD_ARG
    assert lib.lanczos_resize_validate(None) == L.ERR_BAD_ARG
    assert lib.lanczos_resize_device(None, ctypes.byref(d), None, None, 1, 0, 0, None) == L.ERR_BAD_ARG
    assert lib.lanczos_resize_force(None, L.RESIZE_FUSED) == L.ERR_BAD_ARG


def test_the_scale_descriptor_still_refuses_downscaling():
    lib = L._lib()
    dd = L.Desc()
    assert lib.lanczos_desc_init(ctypes.byref(dd), 64, 48, 3, 1, 2, 3, 3) == L.ERR_UNSUPPORTED
    assert lib.lanczos_desc_init(ctypes.byref(dd), 64, 48, 3, 1, 1, 2, 3) == L.ERR_UNSUPPORTED


def test_cli_refuses_size_with_upscale_only_flags(tmp_path):
    exe = os.path.join(ROOT, "lanczos-hls_amd", "lanczos_upscale")
    if not os.path.exists(exe):
        L.build()
    for extra in (["--scale", "2"], ["--exact"], ["--hls"], ["--devices", "0-1"], ["--frames", "4"], ["--split", "rows"],
                  ["--root"]):
        r = subprocess.run([exe, "in.png", str(tmp_path / "o.png"), "--size", "10x10"] + extra, capture_output=True,
                           text=True, timeout=60)
        assert r.returncode != 0 and "--size cannot be combined" in r.stderr, extra
