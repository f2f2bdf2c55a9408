"""CPU-only checks of the source box, reduce and reducing_gap of the resize entry (lanczos_resize_*_ex, lanczos_reduce_*;
Pillow's Image.resize(size, LANCZOS, box, reducing_gap) and Image.reduce): the committed fixture equals the numpy model
and, where Pillow imports, Pillow; the library's host tables and plans equal the model's; every refusal returns its code;
the old entry points and the _ex ones with NULL agree.  No GPU needed."""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_box_model as BM
import resize_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_pillow_box.npz")


def _gen():
    spec = importlib.util.spec_from_file_location("make_resize_box_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_resize_box_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _gen()


def test_fixture_is_small_and_its_inputs_are_reproducible():
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 200 * 1024
    name, iw, ih, _, _, mode, _ = G.BOX_CASES[0]
    assert np.array_equal(z["input_check"], G.make_input(0, 0, iw, ih, mode))
    assert len(z.files) == len(G.BOX_CASES) + len(G.REDUCE_CASES) + len(G.GAP_CASES) + 1


def test_fixture_covers_what_it_has_to():
    modes = {c[5] for c in G.BOX_CASES}
    assert modes == {"L", "RGB", "RGBX", "RGBA", "I;16"}
    assert any(c[1:3] == c[3:5] for c in G.BOX_CASES)                                 # equal size, sub-pixel shift
    assert any(all(float(v).is_integer() for v in c[6]) for c in G.BOX_CASES)         # integer box
    assert any(c[4][0] == 1 for c in G.REDUCE_CASES) and any(c[4][1] == 1 for c in G.REDUCE_CASES)
    assert any(c[5] is not None for c in G.REDUCE_CASES)
    assert {c[7] for c in G.GAP_CASES} == {1.0, 1.1, 2.0, 3.0}
    plans = [BM.gap_plan(c[1], c[2], c[3], c[4], c[6], c[7])[:2] for c in G.GAP_CASES]
    assert all(fx > 1 or fy > 1 for fx, fy in plans)
    assert any(fx > 1 and fy == 1 for fx, fy in plans) and any(fx == 1 and fy > 1 for fx, fy in plans)
    assert any(c[6] is not None for c in G.GAP_CASES) and any(c[6] is None for c in G.GAP_CASES)


def test_fixture_tells_the_contract_from_its_near_misses():
    """What the generator checks before it writes: a double box, a ragged edge divided by fx * fy and a dropped gap would
    each change bytes of the fixture (the gap check against the model's ungapped resize here, Pillow's there)."""
    z = np.load(GOLDEN)
    double_box = ragged = 0
    for i, (name, iw, ih, ow, oh, mode, box) in enumerate(G.BOX_CASES):
        if mode in ("L", "RGB", "RGBX"):
            img = G.make_input(0, i, iw, ih, mode)
            double_box += not np.array_equal(BM.resize_box(img, ow, oh, box, float_box=False), z[f"box_{name}"])
    for i, (name, iw, ih, mode, factor, box) in enumerate(G.REDUCE_CASES):
        img = G.make_input(1, i, iw, ih, mode)
        ragged += not np.array_equal(BM.reduce(img, factor, box, own_divisor=False), z[f"reduce_{name}"])
    assert double_box >= 1 and ragged >= 1
    for i, (name, iw, ih, ow, oh, mode, box, gap) in enumerate(G.GAP_CASES):
        img = G.make_input(2, i, iw, ih, mode)
        assert not np.array_equal(BM.resize(img, ow, oh, box, None), z[f"gap_{name}"]), name


def test_fixture_equals_model():
    z = np.load(GOLDEN)
    for i, (name, iw, ih, ow, oh, mode, box) in enumerate(G.BOX_CASES):
        img = G.make_input(0, i, iw, ih, mode)
        assert np.array_equal(BM.resize(img, ow, oh, box, alpha=mode == "RGBA"), z[f"box_{name}"]), name
    for i, (name, iw, ih, mode, factor, box) in enumerate(G.REDUCE_CASES):
        img = G.make_input(1, i, iw, ih, mode)
        want = z[f"reduce_{name}"]
        assert want.shape[:2] == BM.reduce_size(iw, ih, factor, box)[::-1], name
        assert np.array_equal(BM.reduce(img, factor, box), want), name
    for i, (name, iw, ih, ow, oh, mode, box, gap) in enumerate(G.GAP_CASES):
        img = G.make_input(2, i, iw, ih, mode)
        assert np.array_equal(BM.resize(img, ow, oh, box, gap), z[f"gap_{name}"]), name


def test_pillow_still_equals_the_fixture():
    pytest.importorskip("PIL")
    z = np.load(GOLDEN)
    for i, (name, iw, ih, ow, oh, mode, box) in enumerate(G.BOX_CASES):
        assert np.array_equal(G.pillow_resize(G.make_input(0, i, iw, ih, mode), ow, oh, mode, box), z[f"box_{name}"]), name
    for i, (name, iw, ih, mode, factor, box) in enumerate(G.REDUCE_CASES):
        assert np.array_equal(G.pillow_reduce(G.make_input(1, i, iw, ih, mode), mode, factor, box), z[f"reduce_{name}"]), name
    for i, (name, iw, ih, ow, oh, mode, box, gap) in enumerate(G.GAP_CASES):
        assert np.array_equal(G.pillow_resize(G.make_input(2, i, iw, ih, mode), ow, oh, mode, box, gap), z[f"gap_{name}"]), name


def test_model_equals_pillow_on_random_boxes_factors_and_gaps():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(515)
    for k in range(16):
        iw, ih = (int(v) for v in rng.integers(20, 120, 2))
        ow, oh = (int(v) for v in rng.integers(1, 60, 2))
        mode = ("L", "RGB", "RGBX")[k % 3]
        img = rng.integers(0, 256, (ih, iw, G.CHANNELS[mode]), dtype=np.uint8)
        x0, x1 = sorted(rng.uniform(0, iw, 2))
        y0, y1 = sorted(rng.uniform(0, ih, 2))
        box = (float(x0), float(y0), float(x1) if x1 - x0 > 1 else float(iw), float(y1) if y1 - y0 > 1 else float(ih))
        gap = (None, 1.0, 1.5, 2.0)[k % 4]
        assert np.array_equal(BM.resize(img, ow, oh, box, gap), G.pillow_resize(img, ow, oh, mode, box, gap)), (k, box, gap)
        fx, fy = (int(v) for v in rng.integers(1, 15, 2))
        ib = (int(x0), int(y0), max(int(x0) + 1, int(x1)), max(int(y0) + 1, int(y1)))
        assert np.array_equal(BM.reduce(img, (fx, fy), ib), G.pillow_reduce(img, mode, (fx, fy), ib)), (k, fx, fy, ib)


def _axes_of_fixture():
    """(in_n, out_n, b0, b1) of every axis a fixture case resizes, the inner resizes of the gapped cases included."""
    out = []
    for name, iw, ih, ow, oh, mode, box in G.BOX_CASES:
        out += [(iw, ow, box[0], box[2], (iw, ih, ow, oh, box, None, 0)), (ih, oh, box[1], box[3], (iw, ih, ow, oh, box, None, 1))]
    for name, iw, ih, ow, oh, mode, box, gap in G.GAP_CASES:
        _, _, _, (rw, rh), inner = BM.gap_plan(iw, ih, ow, oh, box, gap)
        out += [(rw, ow, inner[0], inner[2], (iw, ih, ow, oh, box, gap, 0)), (rh, oh, inner[1], inner[3], (iw, ih, ow, oh, box, gap, 1))]
    return out


def test_host_tables_equal_the_model_on_every_fixture_axis():
    for in_n, out_n, b0, b1, (iw, ih, ow, oh, box, gap, axis) in _axes_of_fixture():
        d = L.resize_desc(iw, ih, ow, oh, 3)
        f, c, k = L.resize_taps_host(d, axis, box=box, reducing_gap=gap)
        mf, mc, mk = BM.axis_tables(in_n, out_n, 3, b0, b1)
        assert k.shape == (out_n, BM.ksize(out_n, 3, b0, b1)), (iw, ih, ow, oh, box, gap, axis)
        assert np.array_equal(f, mf) and np.array_equal(c, mc) and np.array_equal(k, mk), (iw, ih, ow, oh, box, gap, axis)
        assert (f >= 0).all() and (f + c <= in_n).all() and (c >= 1).all()
        f6, c6, k6 = L.resize_taps_f64_host(d, axis, box=box, reducing_gap=gap)
        _, _, mk6 = BM.axis_tables(in_n, out_n, 3, b0, b1, f64=True)
        assert np.array_equal(f6, mf) and np.array_equal(c6, mc)
        assert np.array_equal(k6.view(np.uint64), mk6.view(np.uint64)), (iw, ih, ow, oh, box, gap, axis)


@pytest.mark.parametrize("a", [2, 3, 4])
def test_boxed_tables_keep_the_coefficient_and_accumulator_bounds(a):
    """The ranges the kernels rely on (|coeff| < 2^23, 255 * sum|coeff| + 2^21 < 2^31) hold for boxed tables too: every
    in, out <= 24 with boxes at fractional offsets, touching and not touching the ends."""
    kmin = kmax = accmax = 0
    for in_n in range(2, 25):
        boxes = [(0.0, in_n), (0.3, in_n), (0.0, in_n - 0.7), (in_n * 0.25, in_n * 0.8), (0.5, 1.75), (in_n - 1.1, in_n)]
        for out_n in range(1, 25):
            for b0, b1 in boxes:
                d = L.resize_desc(in_n, 1, out_n, 1, 1, a)
                f, c, k = L.resize_taps_host(d, 0, box=(b0, 0, b1, 1))
                mf, mc, mk = BM.axis_tables(in_n, out_n, a, b0, b1)
                assert np.array_equal(f, mf) and np.array_equal(c, mc) and np.array_equal(k, mk), (in_n, out_n, b0, b1)
                kmin, kmax = min(kmin, int(k.min())), max(kmax, int(k.max()))
                accmax = max(accmax, int((255 * np.abs(k.astype(np.int64)).sum(axis=1)).max()) + (1 << 21))
    assert -(1 << 23) < kmin and kmax < (1 << 23), (kmin, kmax)
    assert accmax < (1 << 31), accmax


def test_old_entry_points_and_ex_with_null_agree():
    lib = L._lib()
    for iw, ih, ow, oh in ((3840, 2160, 160, 90), (97, 61, 40, 23), (40, 30, 97, 71), (33, 77, 20, 77), (31, 17, 31, 17)):
        d = L.resize_desc(iw, ih, ow, oh, 3)
        full = L.resize_opts(d)
        assert list(full.box) == [0, 0, iw, ih] and full.reducing_gap == 0 and list(full.reserved) == [0] * 4
        for axis in (0, 1):
            old = L.resize_taps_host(d, axis)
            mf, mc, mk = M.axis_tables(iw if axis == 0 else ih, ow if axis == 0 else oh, 3)
            assert np.array_equal(old[2], mk)
            ks = ctypes.c_int()
            n = ow if axis == 0 else oh
            for ref in (None, ctypes.byref(full)):
                f, c = np.empty(n, np.int32), np.empty(n, np.int32)
                k = np.empty(old[2].shape, np.int32)
                assert lib.lanczos_resize_taps_host_ex(ctypes.byref(d), ref, axis, f.ctypes.data, c.ctypes.data,
                                                       k.ctypes.data, ctypes.byref(ks)) == L.OK
                assert ks.value == old[2].shape[1]
                assert np.array_equal(f, old[0]) and np.array_equal(c, old[1]) and np.array_equal(k, old[2])
            o6 = L.resize_taps_f64_host(d, axis)
            n6 = L.resize_taps_f64_host(d, axis, opts=full)
            assert np.array_equal(o6[2].view(np.uint64), n6[2].view(np.uint64))
        for frames in (1, 32):
            p = L.resize_plan_host(d, frames)
            for ref in (None, ctypes.byref(full)):
                pe = L.ResizePlanEx()
                assert lib.lanczos_resize_plan_host_ex(ctypes.byref(d), ref, frames, ctypes.byref(pe)) == L.OK
                assert bytes(pe.inner) == bytes(p)
                assert (pe.fx, pe.fy, list(pe.safe_box), pe.reduced_w, pe.reduced_h) == (1, 1, [0, 0, iw, ih], iw, ih)
                assert list(pe.inner_box) == [0, 0, iw, ih]
                assert (pe.pass_h, pe.pass_v) == (int(iw != ow), int(ih != oh))


def test_w5_with_a_gap_plans_the_fused_kernel():
    d = L.resize_desc(3840, 2160, 160, 90, 3)
    assert L.resize_plan_host(d, 32).fused == 0                    # W5 as it is: two-pass, 145 vertical taps
    p = L.resize_plan_host(d, 32, reducing_gap=2.0)
    assert (p.fx, p.fy) == (12, 12) and (p.reduced_w, p.reduced_h) == (320, 180)
    assert list(p.safe_box) == [0, 0, 3840, 2160] and list(p.inner_box) == [0, 0, 320, 180]
    assert p.inner.fused == 1 and (p.pass_h, p.pass_v) == (1, 1)
    p = L.resize_plan_host(d, 32, reducing_gap=3.0)
    assert (p.fx, p.fy) == (8, 8) and (p.reduced_w, p.reduced_h) == (480, 270) and p.inner.fused == 1


def test_plans_equal_the_model_over_sizes_boxes_and_gaps():
    rng = np.random.default_rng(99)
    seen_reduced = seen_plain = 0
    for k in range(400):
        iw, ih = (int(v) for v in rng.integers(8, 5000, 2))
        ow, oh = (int(v) for v in rng.integers(1, 400, 2))
        if k % 3:
            x0, x1 = sorted(rng.uniform(0, iw, 2))
            y0, y1 = sorted(rng.uniform(0, ih, 2))
            if x1 - x0 < 1e-3 or y1 - y0 < 1e-3:
                continue
            box = (float(x0), float(y0), float(x1), float(y1)) if k % 2 else (int(x0), int(y0), int(x0) + max(1, int(x1 - x0)),
                                                                            int(y0) + max(1, int(y1 - y0)))
        else:
            box = None
        gap = (None, 1.0, 1.1, 2.0, 3.0)[k % 5]
        a = (3, 2, 4)[k % 3]
        fx, fy, rb, (rw, rh), inner = BM.gap_plan(iw, ih, ow, oh, box, gap, a)
        if fx * fy >= 65536:
            continue
        d = L.resize_desc(iw, ih, ow, oh, 3, a)
        p = L.resize_plan_host(d, 4, box=box if box is not None else (0, 0, iw, ih), reducing_gap=gap)
        assert (p.fx, p.fy) == (fx, fy), (k, iw, ih, ow, oh, box, gap)
        assert tuple(p.safe_box) == tuple(rb) and (p.reduced_w, p.reduced_h) == (rw, rh), (k, iw, ih, ow, oh, box, gap)
        assert tuple(p.inner_box) == tuple(float(v) for v in inner), (k, iw, ih, ow, oh, box, gap)
        assert p.pass_h == int(BM.axis_runs(rw, ow, inner[0], inner[2])) and p.pass_v == int(BM.axis_runs(rh, oh, inner[1], inner[3]))
        if fx > 1 or fy > 1:
            seen_reduced += 1
            assert L.reduce_size(iw, ih, (fx, fy), rb) == (rw, rh)
        else:
            seen_plain += 1
    assert seen_reduced > 50 and seen_plain > 50


def test_two_pass_intermediate_is_bounded_by_the_box():
    """A 1280 x 720 crop out of 7680 x 4320 must not pay for 4320 rows: the horizontal pass produces the rows the vertical
    taps read, first_v[0] .. first_v[-1] + count_v[-1], and the scratch holds those."""
    d = L.resize_desc(7680, 4320, 640, 360, 3)
    box = (3000.25, 1700.5, 4280.75, 2420.25)
    p = L.resize_plan_host(d, 1, box=box)
    f, c, _ = BM.axis_tables(4320, 360, 3, box[1], box[3])
    assert (p.mid_row0, p.mid_rows) == (int(f[0]), int(f[-1] + c[-1] - f[0]))
    assert 1700 - 8 <= p.mid_row0 <= 1700 and 720 <= p.mid_rows <= 720 + 16
    full = L.resize_plan_host(d, 1, box=(0, 0, 7680, 4320))
    assert (full.mid_row0, full.mid_rows) == (0, 4320)
    h_only = L.resize_plan_host(L.resize_desc(7680, 4320, 640, 4320, 3), 1, box=(3000.25, 0, 4280.75, 4320))
    assert (h_only.pass_h, h_only.pass_v, h_only.mid_rows) == (1, 0, 0)


def test_pass_rule():
    d = L.resize_desc(40, 30, 40, 30, 3)
    for box, want in (((0, 0, 40, 30), (0, 0)), ((0.5, 0, 40, 30), (1, 0)), ((0, 0, 40, 29.5), (0, 1)),
                      ((0.25, 0.25, 39.5, 30), (1, 1)), ((0, 0, 40 - 1e-9, 30), (0, 0))):   # the last rounds to 40.0f
        p = L.resize_plan_host(d, 1, box=box)
        assert (p.pass_h, p.pass_v) == want, box


def test_refusals():
    lib = L._lib()
    d = L.resize_desc(200, 150, 20, 15, 3)

    def code(desc=d, box=None, gap=None, reserved=None):
        o = L.resize_opts(desc)
        if box is not None:
            for i in range(4):
                o.box[i] = box[i]
        if gap is not None:
            o.reducing_gap = gap
        if reserved is not None:
            o.reserved[reserved] = 1
        p = L.ResizePlanEx()
        rc = lib.lanczos_resize_plan_host_ex(ctypes.byref(desc), ctypes.byref(o), 1, ctypes.byref(p))
        ks = ctypes.c_int()
        assert lib.lanczos_resize_taps_host_ex(ctypes.byref(desc), ctypes.byref(o), 0, None, None, None, ctypes.byref(ks)) == rc
        return rc

    assert code() == L.OK and code(gap=1.0) == L.OK and code(box=(0.5, 0.5, 199.5, 149.5), gap=2.5) == L.OK
    for box in ((-0.1, 0, 200, 150), (0, -1, 200, 150), (0, 0, 200.5, 150), (0, 0, 200, 151), (50, 0, 50, 150),
                (60, 0, 50, 150), (0, 70, 200, 70), (float("nan"), 0, 200, 150), (0, 0, float("inf"), 150)):
        assert code(box=box) == L.ERR_BAD_ARG, box
    for gap in (0.5, 0.999, -1.0, float("nan")):
        assert code(gap=gap) == L.ERR_BAD_ARG, gap
    for i in range(4):
        assert code(reserved=i) == L.ERR_BAD_ARG
    # Pillow drops the gap for RGBA and raises for I;16: no oracle, so both are refused -- with a gap only
    for desc in (L.resize_desc(200, 150, 20, 15, 4, alpha=True), L.resize_desc(200, 150, 20, 15, 1, bits=16)):
        assert code(desc) == L.OK and code(desc, box=(1.5, 2.5, 100, 100)) == L.OK
        assert code(desc, gap=2.0) == L.ERR_BAD_ARG and code(desc, gap=1.0) == L.ERR_BAD_ARG
    # fx * fy >= 65536
    assert code(L.resize_desc(65535, 65535, 100, 100, 1), gap=1.0) == L.ERR_UNSUPPORTED
    assert code(L.resize_desc(25500, 25500, 100, 100, 1), gap=1.0) == L.OK          # 255 * 255
    assert lib.lanczos_resize_opts_init(None, ctypes.byref(d)) == L.ERR_BAD_ARG
    assert lib.lanczos_resize_device_ex(None, ctypes.byref(d), None, None, None, 1, 0, 0, None) == L.ERR_BAD_ARG
    assert lib.lanczos_resize_host_ex(None, ctypes.byref(d), None, None, None, 1) == L.ERR_BAD_ARG
    with pytest.raises(L.LanczosError):
        L.resize_opts(d, box=(0, 0, 1))

    # reduce
    w, h = ctypes.c_int(), ctypes.c_int()

    def rcode(iw=100, ih=80, fx=3, fy=2, box=None):
        b = (ctypes.c_int32 * 4)(*box) if box is not None else None
        return lib.lanczos_reduce_size(iw, ih, fx, fy, b, ctypes.byref(w), ctypes.byref(h))

    assert rcode() == L.OK and (w.value, h.value) == (34, 40)
    assert rcode(box=(1, 2, 99, 79)) == L.OK and (w.value, h.value) == (33, 39)
    assert rcode(fx=255, fy=257) == L.OK and rcode(fx=256, fy=256) == L.ERR_UNSUPPORTED
    for kw in (dict(fx=0), dict(fy=0), dict(fx=-2), dict(iw=0), dict(ih=65536), dict(box=(5, 0, 5, 80)), dict(box=(0, 0, 101, 80)),
               dict(box=(-1, 0, 100, 80)), dict(box=(0, 9, 100, 8))):
        assert rcode(**kw) == L.ERR_BAD_ARG, kw
    assert lib.lanczos_reduce_size(100, 80, 2, 2, None, None, None) == L.ERR_BAD_ARG
    assert lib.lanczos_reduce_device(None, 100, 80, 3, 2, 2, None, None, None, 1, 0, 0, None) == L.ERR_BAD_ARG
    assert lib.lanczos_reduce_host(None, 100, 80, 3, 2, 2, None, None, None, 1) == L.ERR_BAD_ARG
    with pytest.raises(L.LanczosError) as e:     # Pillow: "image has wrong mode"
        L.Context.reduce(None, np.zeros((4, 4), np.uint16), 2)
    assert e.value.code == L.ERR_BAD_ARG


def test_cli_checks_box_and_gap_arguments(tmp_path):
    exe = os.path.join(ROOT, "lanczos-hls_amd", "lanczos_upscale")
    if not os.path.exists(exe):
        L.build()
    for extra, msg in ((["--box", "1,2,3"], "--box"), (["--box", "1,2,3,x"], "--box"), (["--reducing-gap", "0.5"], "--reducing-gap"),
                       (["--reducing-gap", "abc"], "--reducing-gap")):
        r = subprocess.run([exe, "in.png", str(tmp_path / "o.png"), "--size", "10x10"] + extra, capture_output=True, text=True,
                           timeout=60)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    for extra in (["--box", "0,0,4,4"], ["--reducing-gap", "2"]):
        r = subprocess.run([exe, "in.png", str(tmp_path / "o.png")] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "need --size" in r.stderr, (extra, r.stderr)
