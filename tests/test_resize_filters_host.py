"""CPU-only checks of the resize filters (LANCZOS_RESIZE_FILTER: box, bilinear, Hamming, bicubic, nearest): the numpy model
(tests/resize_filters_model.py) equals the committed Pillow fixture and the fixture tells the contract from its near misses,
the library's tables equal the model's as integer and 64-bit patterns, descriptor validation, filter 0 is what the old
initialisers give, coefficient bounds, and the plans of short filters.  No GPU needed."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_box_model as MB
import resize_filters_model as FM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_pillow_filters.npz")
NEW = (FM.BOX, FM.BILINEAR, FM.HAMMING, FM.BICUBIC, FM.NEAREST)
FLAGS = {"L": 0, "RGB": 0, "RGBX": 0, "RGBA": L.RESIZE_ALPHA, "I;16": L.RESIZE_U16, "F": L.RESIZE_F32}


def golden_module():
    spec = importlib.util.spec_from_file_location("make_resize_filters_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_resize_filters_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixture():
    g = golden_module()
    return g, g.load(GOLDEN)


def _init_filter(iw, ih, ow, oh, c, filt, flags=0):
    d = L.ResizeDesc()
    return L._lib().lanczos_resize_desc_init_filter(ctypes.byref(d), iw, ih, ow, oh, c, filt, flags), d


def test_fixture_equals_model(fixture):
    """byte for byte; mode F bit for bit with NaN positions coinciding (FM.same)"""
    g, cases = fixture
    assert len(cases) == len(g.cases()) == 220
    assert os.path.getsize(GOLDEN) < 1 << 20
    seen = set()
    for f, m, s, img, want in cases.values():
        iw, ih, ow, oh, box, gap = g.SHAPES[s]
        assert max(iw, ih, ow, oh) <= 101 or (f == "nearest" and ih == oh == 1), (f, m, s)
        got = FM.resize(img, FM.NAMES.index(f), ow, oh, box, gap, alpha=m == "RGBA")
        assert FM.same(got, want), (f, m, s)
        seen.add((f, m))
    assert seen == {(f, m) for f in g.FILTERS for m in g.MODES} - {("nearest", "I;16")}


def test_fixture_tells_the_near_misses_apart(fixture):
    """The conditions the generator refuses to write a fixture without, checked on the committed file: each near miss
    differs from Pillow in at least one sample of at least one case."""
    g, cases = fixture
    variants = {"hamming_double": ("hamming", dict(hamming_double=True)), "box_symmetric": ("box", dict(box_symmetric=True)),
                "nearest_direct": ("nearest", dict(nearest_direct=True)), "nearest_premul": ("nearest", dict(nearest_premul=True)),
                "bicubic_a": ("bicubic", dict(bicubic_a=-0.75))}
    for v, (filt, kw) in variants.items():
        told = 0
        for f, m, s, img, want in cases.values():
            if f != filt or (v == "nearest_premul" and m != "RGBA"):
                continue
            iw, ih, ow, oh, box, gap = g.SHAPES[s]
            told += not FM.same(FM.resize(img, FM.NAMES.index(f), ow, oh, box, gap, alpha=m == "RGBA", **kw), want)
        assert told >= 1, v


AXES = [(97, 41, None), (41, 97, None), (200, 7, None), (23, 50, None), (24, 24, (1.5, 24)), (40, 17, (5.3, 36.1)),
        (101, 6, (0.5, 94.5)), (1, 57, None), (8, 204, None), (2999, 1777, None)]


@pytest.mark.parametrize("filt", NEW)
def test_tables_equal_the_model(filt):
    """_taps_host / _taps_f64_host (and _ex with a box) hand out the filter's tables: integer and 64-bit patterns"""
    for in_n, out_n, span in AXES:
        if in_n > 300 and filt != FM.NEAREST:
            continue
        for axis in (0, 1):
            dims = (in_n, 5, out_n, 5) if axis == 0 else (5, in_n, 5, out_n)
            rc, d = _init_filter(*dims, 1, filt)
            assert rc == L.OK
            box = None
            if span is not None:
                box = (span[0], 0, span[1], 5) if axis == 0 else (0, span[0], 5, span[1])
            b0, b1 = span if span is not None else (0, in_n)
            f, c, k = L.resize_taps_host(d, axis, box=box)
            mf, mc, mk = FM.axis_tables(filt, in_n, out_n, b0, b1)
            assert k.shape[1] == FM.ksize(filt, out_n, b0, b1) == mk.shape[1], (filt, in_n, out_n, span)
            assert np.array_equal(f, mf) and np.array_equal(c, mc) and np.array_equal(k, mk), (filt, in_n, out_n, span, axis)
            f, c, k = L.resize_taps_f64_host(d, axis, box=box)
            mf, mc, mk = FM.axis_tables(filt, in_n, out_n, b0, b1, f64=True)
            assert np.array_equal(f, mf) and np.array_equal(c, mc), (filt, in_n, out_n, span, axis)
            assert np.array_equal(k.view(np.uint64), mk.view(np.uint64)), (filt, in_n, out_n, span, axis)
            if filt == FM.NEAREST:
                assert k.shape[1] == 1 and (c == 1).all() and (k == 1.0).all() and f.min() >= 0 and f.max() < in_n


def test_gap_tables_use_the_filters_support():
    """reducing_gap: the safe box is S - 0.5 source steps wide where Lanczos has a - 0.5"""
    for filt in FM.WEIGHTED[1:]:
        rc, d = _init_filter(101, 97, 12, 11, 3, filt)
        assert rc == L.OK
        for box in (None, (7.5, 3.25, 99, 90)):
            p = L.resize_plan_host(d, 1, box=box, reducing_gap=1.5)
            fx, fy, rb, (rw, rh), inner = FM.gap_plan(filt, 101, 97, 12, 11, box, 1.5)
            assert (p.fx, p.fy) == (fx, fy) and fx > 1 and tuple(p.safe_box) == tuple(rb), (filt, box)
            assert (p.reduced_w, p.reduced_h) == (rw, rh) and tuple(p.inner_box) == tuple(inner), (filt, box)
            f, c, k = L.resize_taps_host(d, 0, box=box, reducing_gap=1.5)
            mf, mc, mk = FM.axis_tables(filt, rw, 12, inner[0], inner[2])
            assert np.array_equal(f, mf) and np.array_equal(c, mc) and np.array_equal(k, mk), (filt, box)


def test_flag_validation():
    for filt in range(16):
        rc, d = _init_filter(20, 20, 30, 10, 3, filt)
        assert rc == (L.OK if filt <= 5 else L.ERR_BAD_ARG), filt
        if filt <= 5:
            assert d.reserved[0] == filt << 8 and d.a == 3 and d.reserved[1] == 0
            assert L._lib().lanczos_resize_validate(ctypes.byref(d)) == L.OK
    for filt in range(1, 6):
        for a in (2, 4):
            d = L.ResizeDesc(20, 20, 30, 10, 3, a)
            d.reserved[0] = filt << 8
            assert L._lib().lanczos_resize_validate(ctypes.byref(d)) == L.ERR_BAD_ARG, (filt, a)
            with pytest.raises(L.LanczosError) as e:
                L.resize_desc(20, 20, 30, 10, 3, a, filter=filt)
            assert e.value.code == L.ERR_BAD_ARG
    # the filter combines with the flags as they combine with each other
    for filt in range(1, 5):
        assert _init_filter(20, 20, 30, 10, 4, filt, L.RESIZE_ALPHA)[0] == L.OK
        assert _init_filter(20, 20, 30, 10, 3, filt, L.RESIZE_ALPHA)[0] == L.ERR_BAD_ARG
        assert _init_filter(20, 20, 30, 10, 3, filt, L.RESIZE_U16)[0] == L.OK
        assert _init_filter(20, 20, 30, 10, 3, filt, L.RESIZE_F32)[0] == L.OK
        assert _init_filter(20, 20, 30, 10, 4, filt, L.RESIZE_U16 | L.RESIZE_ALPHA)[0] == L.ERR_BAD_ARG
        assert _init_filter(20, 20, 30, 10, 4, filt, L.RESIZE_F32 | L.RESIZE_ALPHA)[0] == L.ERR_BAD_ARG
    assert _init_filter(20, 20, 30, 10, 4, L.FILTER_NEAREST, L.RESIZE_ALPHA)[0] == L.OK
    assert _init_filter(20, 20, 30, 10, 1, L.FILTER_NEAREST, L.RESIZE_F32)[0] == L.OK
    # Pillow's I;16 NEAREST is its generic transform, not the running-sum gather: refused
    assert _init_filter(20, 20, 30, 10, 1, L.FILTER_NEAREST, L.RESIZE_U16)[0] == L.ERR_UNSUPPORTED
    assert _init_filter(20, 20, 30, 10, 3, 1, 1 << 8)[0] == L.ERR_BAD_ARG   # filter bits in `flags`
    # NEAREST with a gap: Pillow drops it silently, the library refuses
    d = L.resize_desc(100, 100, 10, 10, 3, filter="nearest")
    p = L.ResizePlanEx()
    o = L.resize_opts(d, None, 2.0)
    assert L._lib().lanczos_resize_plan_host_ex(ctypes.byref(d), ctypes.byref(o), 1, ctypes.byref(p)) == L.ERR_BAD_ARG
    assert L.resize_plan_host(d, 1, box=(1, 1, 50, 50)).inner.fused == 0
    assert L.resize_plan_host(d, 1).fused == 0
    with pytest.raises(L.LanczosError):
        L.resize_desc(20, 20, 30, 10, 3, filter="cubic")
    assert [L.filter_code(n) for n in L.FILTER_NAMES] == list(range(6)) and L.filter_code("BICUBIC") == L.FILTER_BICUBIC


def test_filter_0_is_the_old_request():
    """descriptors, tables and plans of LANCZOS_FILTER_LANCZOS are bit-identical to those of the old initialisers"""
    for flags, c in ((0, 3), (L.RESIZE_ALPHA, 4), (L.RESIZE_U16, 1), (L.RESIZE_F32, 3)):
        rc, d0 = _init_filter(70, 37, 150, 75, c, L.FILTER_LANCZOS, flags)
        assert rc == L.OK
        d1 = L.ResizeDesc()
        assert L._lib().lanczos_resize_desc_init_ex(ctypes.byref(d1), 70, 37, 150, 75, c, 3, flags) == L.OK
        assert bytes(d0) == bytes(d1)
    for a in (2, 3, 4):
        for iw, ow in ((70, 150), (97, 41)):
            d = L.resize_desc(iw, 37, ow, 75, 3, a)
            dn = L.resize_desc(iw, 37, ow, 75, 3, a, filter="lanczos")
            assert bytes(d) == bytes(dn)
            f, c, k = L.resize_taps_host(d, 0)
            mf, mc, mk = MB.axis_tables(iw, ow, a, 0, iw)
            assert np.array_equal(f, mf) and np.array_equal(c, mc) and np.array_equal(k, mk)
            p = L.resize_plan_host(d, 1)
            assert p.fused and p.K == next(b for b in (7, 9, 11, 13, 17, 25) if b >= k.shape[1])   # never the 3- or 5-tap instance


@pytest.mark.parametrize("filt", FM.WEIGHTED[1:])
def test_coefficient_bounds(filt):
    """what the kernels rely on: signed 24-bit coefficients and 255 * sum|k| + 2^21 < 2^31, over in, out <= 40"""
    for in_n in range(1, 41):
        for out_n in range(1, 41):
            _, _, k = FM.axis_tables(filt, in_n, out_n)
            k = k.astype(np.int64)
            assert np.abs(k).max() < 1 << 23, (filt, in_n, out_n)
            assert 255 * np.abs(k).sum(axis=1).max() + (1 << 21) < 1 << 31, (filt, in_n, out_n)
    # the library builds the same tables (test_tables_equal_the_model) and accepts them
    rc, d = _init_filter(40, 40, 1, 1, 1, filt)
    assert rc == L.OK and L.resize_taps_host(d, 0)[2].shape == (1, FM.ksize(filt, 1, 0, 40))


def test_plans_of_short_filters():
    """ksize 3 (box, bilinear, Hamming upscales) runs on the 3-tap instance, ksize 5 (bicubic) on the 5-tap one, for every
    sample type; 1-tap vertical windows (BOX upscale, BOX at out = in with a shifted box) chunk like any other and stay
    inside 80 KiB"""
    for filt, K in ((FM.BOX, 3), (FM.BILINEAR, 3), (FM.HAMMING, 3), (FM.BICUBIC, 5)):
        for flags, c in ((0, 1), (0, 3), (0, 4), (L.RESIZE_ALPHA, 4), (L.RESIZE_U16, 3), (L.RESIZE_F32, 4)):
            rc, d = _init_filter(70, 37, 150, 75, c, filt, flags)
            assert rc == L.OK
            p = L.resize_plan_host(d, 1)
            assert p.fused == 1 and p.K == K and p.strips >= 1 and p.lds_bytes <= 80 * 1024, (filt, flags, c, p.K)
    for iw, ih, ow, oh, box in ((70, 37, 150, 75, None), (64, 600, 64, 600, (0.5, 0.25, 64, 600)), (500, 300, 1100, 2100, None)):
        rc, d = _init_filter(iw, ih, ow, oh, 3, FM.BOX)
        pe = L.resize_plan_host(d, 4, box=box if box is not None else (0, 0, iw, ih))
        p = pe.inner
        b = box if box is not None else (0, 0, iw, ih)
        vf, vc, _ = FM.axis_tables(FM.BOX, ih, oh, b[1], b[3])
        assert (vc == 1).all() and pe.pass_h and pe.pass_v
        assert p.fused == 1 and p.K == 3 and p.lds_bytes <= 80 * 1024
        assert p.rows_per_chunk % 8 == 0 and p.chunks == -(-oh // p.rows_per_chunk)
        ring = max(int(vf[min(o + 8, oh) - 1] + 1 - vf[o]) for o in range(0, oh, 8))
        assert p.ring_rows == ring and 1 <= p.stage_rows <= 16
        assert p.lds_bytes == p.ring_rows * 256 * 3 + p.stage_rows * p.stage_dw * 4   # ring rows of a 256-pixel RGB strip
