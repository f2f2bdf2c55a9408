"""CPU-only checks of LANCZOS_RESIZE_ALPHA (four channels with straight alpha, Pillow's mode RGBA): the numpy model
(tests/resize_alpha_model.py) reproduces the committed Pillow fixture byte for byte and, where Pillow imports, Pillow still
does; the two conversions of the model equal Pillow's convert("RGBa") / convert("RGBA") on every (value, alpha) pair; the
flag word of the descriptor is validated; the launch plan does not depend on the flag.  No GPU needed."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_alpha_model as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_pillow_alpha.npz")
KINDS = {"noise", "low", "extremes", "opaque", "disc"}


def _cases():
    spec = importlib.util.spec_from_file_location(
        "make_resize_alpha_golden", os.path.join(ROOT, "tests", "golden", "make_resize_alpha_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_equals_model():
    z = np.load(GOLDEN)
    g = _cases()
    assert os.path.getsize(GOLDEN) < 300 * 1024
    assert {c[5] for c in g.CASES} == KINDS
    shapes = {"down": 0, "up": 0, "mixed": 0, "h_only": 0, "v_only": 0, "identity": 0, "to_1x1": 0, "large_reduction": 0}
    clamped = 0
    for i, (name, iw, ih, ow, oh, kind) in enumerate(g.CASES):
        img, want = z[f"{name}_in"], z[f"{name}_out"]
        assert img.shape == (ih, iw, 4) and want.shape == (oh, ow, 4), name
        assert np.array_equal(img, g.make_input(i, iw, ih, kind)), name
        assert np.array_equal(A.resize(img, ow, oh, 3), want), name
        clamped += A.clamp_hits(img, ow, oh, 3)
        for s in shapes:
            shapes[s] += name.startswith(s)
    assert all(shapes.values()), shapes
    assert clamped > 0                                    # c' > A at the output: the min() of the contract is live
    # what the kinds promise
    assert set(np.unique(z["mixed_low_in"][..., 3])) <= {0, 1, 2, 3}
    assert set(np.unique(z["down_extremes_in"][..., 3])) == {0, 1, 254, 255}
    assert (z["down_opaque_in"][..., 3] == 255).all()
    disc = z["down_disc_in"][..., 3]
    assert disc.min() == 0 and disc.max() == 255 and ((disc > 0) & (disc < 255)).any()
    assert np.array_equal(z["identity_noise_out"], z["identity_noise_in"])   # rule 4: a copy, no round trip
    assert not np.array_equal(A.unpremultiply(A.premultiply(z["identity_noise_in"])), z["identity_noise_in"])


def test_pillow_still_reproduces_the_fixture():
    pytest.importorskip("PIL")
    z = np.load(GOLDEN)
    g = _cases()
    for name, iw, ih, ow, oh, kind in g.CASES:
        assert np.array_equal(g.pillow_resize(z[f"{name}_in"], ow, oh), z[f"{name}_out"]), name


def test_conversions_equal_pillow_on_every_pair():
    pytest.importorskip("PIL")
    from PIL import Image
    v, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    px = np.stack([v, 255 - v, v ^ 0x55, a], axis=-1)                       # [256][256][4]: every (value, alpha) pair
    pre = np.frombuffer(Image.frombytes("RGBA", (256, 256), px.tobytes()).convert("RGBa").tobytes(), np.uint8)
    assert np.array_equal(A.premultiply(px).reshape(-1), pre)
    un = np.frombuffer(Image.frombytes("RGBa", (256, 256), px.tobytes()).convert("RGBA").tobytes(), np.uint8)
    assert np.array_equal(A.unpremultiply(px).reshape(-1), un)             # pairs with value > alpha included


def test_flag_word_validation():
    lib = L._lib()
    assert L.RESIZE_ALPHA == 1

    def code(channels, flags):
        d = L.ResizeDesc()
        rc = lib.lanczos_resize_desc_init_ex(ctypes.byref(d), 64, 48, 20, 100, channels, 3, flags)
        if rc == L.OK:
            assert (d.in_w, d.in_h, d.out_w, d.out_h, d.channels, d.a) == (64, 48, 20, 100, channels, 3)
            assert d.reserved[0] == flags and d.reserved[1] == 0
            assert lib.lanczos_resize_validate(ctypes.byref(d)) == L.OK
        return rc

    assert code(4, L.RESIZE_ALPHA) == L.OK                 # the feature: refused before it existed
    assert code(4, 0) == L.OK and code(3, 0) == L.OK and code(1, 0) == L.OK
    assert code(1, L.RESIZE_ALPHA) == L.ERR_BAD_ARG
    assert code(3, L.RESIZE_ALPHA) == L.ERR_BAD_ARG
    assert code(2, L.RESIZE_ALPHA) == L.ERR_BAD_ARG        # LA is not part of the ABI
    for flags in (2, 3, 7, -1, 1 << 16):
        assert code(4, flags) == L.ERR_BAD_ARG, flags
    d = L.resize_desc(64, 48, 20, 100, 4, 3, alpha=True)
    assert d.reserved[0] == L.RESIZE_ALPHA
    d.reserved[1] = 1
    assert lib.lanczos_resize_validate(ctypes.byref(d)) == L.ERR_BAD_ARG
    d = L.ResizeDesc()
    assert lib.lanczos_resize_desc_init(ctypes.byref(d), 64, 48, 20, 100, 4, 3) == L.OK
    assert d.reserved[0] == 0 and d.reserved[1] == 0       # the plain initialiser still gives flag 0
    assert L.resize_desc(64, 48, 20, 100, 4, 3).reserved[0] == 0
    assert lib.lanczos_resize_desc_init_ex(None, 64, 48, 20, 100, 4, 3, 1) == L.ERR_BAD_ARG
    for c in (1, 3):
        with pytest.raises(L.LanczosError) as e:
            L.resize_desc(64, 48, 20, 100, c, 3, alpha=True)
        assert e.value.code == L.ERR_BAD_ARG


def test_alpha_with_other_channel_counts_raises_before_any_gpu_work():
    class NoGpu(L.Context):
        def __init__(self):                                 # no lanczos_create: resize() must fail at the descriptor
            self._h = ctypes.c_void_p()
    for shape in ((5, 6), (5, 6, 1), (5, 6, 3), (2, 5, 6, 3)):
        with pytest.raises(L.LanczosError) as e:
            NoGpu().resize(np.zeros(shape, np.uint8), 3, 4, alpha=True)
        assert e.value.code == L.ERR_BAD_ARG, shape


def test_plan_does_not_depend_on_the_flag():
    fields = [n for n, _ in L.ResizePlan._fields_]
    fused = two_pass = 0
    for iw, ih, ow, oh, a, frames in ((3840, 2160, 1920, 1080, 3, 1), (1920, 1080, 3840, 2160, 3, 32), (801, 600, 517, 389, 4, 1),
                                      (1018, 120, 261, 31, 3, 5), (200, 120, 261, 131, 2, 1), (3840, 2160, 160, 90, 3, 1),
                                      (1920, 1080, 1920, 540, 3, 1), (64, 64, 64, 64, 3, 1), (1100, 40, 261, 23, 3, 1)):
        p0 = L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, 4, a), frames)
        p1 = L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, 4, a, alpha=True), frames)
        assert [getattr(p0, n) for n in fields] == [getattr(p1, n) for n in fields], (iw, ih, ow, oh)
        fused += p0.fused
        two_pass += not p0.fused
        for axis in (0, 1):                                 # the tables do not know the flag either
            t0 = L.resize_taps_host(L.resize_desc(iw, ih, ow, oh, 4, a), axis)
            t1 = L.resize_taps_host(L.resize_desc(iw, ih, ow, oh, 4, a, alpha=True), axis)
            assert all(np.array_equal(x, y) for x, y in zip(t0, t1))
    assert fused >= 4 and two_pass >= 3
