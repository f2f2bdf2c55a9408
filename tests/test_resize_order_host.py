"""CPU-only checks of the pass order (Pillow 12.2.0's Image.resize runs a frame with height > 100 * width that shrinks in
height vertical first; resize_model.pillow_vertical_first): a live differential sweep of the numpy models against the
installed Pillow over about 2000 seeded requests with sides up to 1200, and the committed fixture of tall frames
(tests/golden/resize_pillow_tall.npz) against the model, the horizontal-first near miss and the library's host tables and
plans.  No GPU needed."""
import collections
import importlib.util
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_box_model as MB
import resize_filters_model as FM
import resize_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_pillow_tall.npz")
MODES = ("L", "RGB", "RGBX", "RGBA", "I;16", "F")
MAX_PIXELS = 600_000


def golden_module():
    spec = importlib.util.spec_from_file_location("make_resize_tall_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_resize_tall_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixture():
    g = golden_module()
    return g, g.load(GOLDEN)


def test_the_rule():
    assert not M.pillow_vertical_first(3, 300, 40) and M.pillow_vertical_first(3, 301, 40)
    assert M.pillow_vertical_first(3, 400, 399) and not M.pillow_vertical_first(3, 400, 400)
    assert not M.pillow_vertical_first(3, 400, 401)
    assert M.pillow_vertical_first(655, 65535, 1000) and not M.pillow_vertical_first(656, 65535, 1000)
    assert M.pass_order(3, 301, 40) == (1, 2) and M.pass_order(3, 301, 40, "h_first") == (2, 1) == M.pass_order(3, 300, 40)


# ---- the live sweep ------------------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "mode filt in_w in_h out_w out_h box gap stratum")
SIDES = ((1, 8), (1, 200), (200, 1200))


def _side(rng):
    lo, hi = SIDES[int(rng.integers(0, 3))]
    return int(rng.integers(lo, hi + 1))


def _box(rng, in_w, in_h, fractional):
    """a legal box: it starts in the first 40 % of each axis and ends in the last 40 %"""
    if fractional:   # eighths of a pixel: exact in float32, never empty
        x0, y0 = (round(float(rng.uniform(0, 0.4 * n)) * 8) / 8 for n in (in_w, in_h))
        x1, y1 = (n - round(float(rng.uniform(0, 0.4 * n)) * 8) / 8 for n in (in_w, in_h))
    else:
        x0, y0 = (int(rng.integers(0, int(0.4 * n) + 1)) for n in (in_w, in_h))
        x1, y1 = (n - int(rng.integers(0, int(0.4 * n) + 1)) for n in (in_w, in_h))
    assert 0 <= x0 < x1 <= in_w and 0 <= y0 < y1 <= in_h
    return (x0, y0, x1, y1)


def _gap_ok(mode, filt):
    """where a reducing_gap has a contract: 8-bit without alpha, a weighted filter"""
    return mode in ("L", "RGB", "RGBX") and filt != FM.NEAREST


def _reduced(c):
    """(reduced_w, reduced_h) -- the frame the resize reads -- and whether both of its passes run"""
    rw, rh, b = c.in_w, c.in_h, c.box if c.box is not None else (0, 0, c.in_w, c.in_h)
    if c.gap is not None:
        fx, fy, _, (w, h), inner = FM.gap_plan(c.filt, c.in_w, c.in_h, c.out_w, c.out_h, c.box, c.gap)
        if fx > 1 or fy > 1:
            rw, rh, b = w, h, inner
    return rw, rh, MB.axis_runs(rw, c.out_w, b[0], b[2]) and MB.axis_runs(rh, c.out_h, b[1], b[3])


def _combos():
    return [(m, f) for m in MODES for f in range(6) if not (m == "I;16" and f == FM.NEAREST)]


def _draw_cases():
    rng = np.random.default_rng(20261020)
    cases = []
    # any shape: the three size classes per side, half with a box, 40 % of the eligible with a gap
    for mode, filt in _combos():
        for _ in range(30):
            while True:
                iw, ih, ow, oh = _side(rng), _side(rng), _side(rng), _side(rng)
                if iw * ih <= MAX_PIXELS and ow * oh <= MAX_PIXELS:
                    break
            box = _box(rng, iw, ih, rng.random() < 0.7) if rng.random() < 0.5 else None
            gap = float(rng.choice([1.0, 1.5, 2.0, 3.0])) if _gap_ok(mode, filt) and rng.random() < 0.4 else None
            cases.append(Case(mode, filt, iw, ih, ow, oh, box, gap, "any"))
    # tall by construction: at most 11 wide (100 * 11 + 1 <= 1200), shrinking in height; the width changes most of the time.
    # Where the horizontal pass copies samples exactly the two orders are one function and no test can tell them apart: a
    # frame one pixel wide (every window is that pixel with weight 1.0) and a BOX upscale across (single pixels).  Those
    # keep to the cases whose width stays (one pass) and to the "any" stratum; here BOX always shrinks across.
    for mode, filt in _combos():
        for _ in range(24):
            iw = int(rng.integers(2, 12))
            ih = int(rng.integers(100 * iw + 1, 1201))
            oh = int(rng.integers(1, ih))
            if rng.random() < 0.1:
                iw = ow = int(rng.integers(1, 12))
                ih = max(ih, 100 * iw + 1)
            else:
                ow = int(rng.integers(1, iw)) if filt == FM.BOX else int(rng.integers(1, 41))
            box = _box(rng, iw, ih, rng.random() < 0.7) if rng.random() < 0.5 else None
            gap = None
            if _gap_ok(mode, filt) and rng.random() < 0.4:   # a gap that keeps the reduced frame tall: fy of 1..3, fx = 1
                gap = float(rng.choice([1.0, 1.5, 2.0]))
            cases.append(Case(mode, filt, iw, ih, ow, oh, box, gap, "tall"))
    # the reduction moves the frame across the rule
    gap_combos = [(m, f) for m, f in _combos() if _gap_ok(m, f)]
    for k in range(30):   # wide enough not to be tall, reduced across by fx: 3 or 4 columns of 700..1200 rows remain, one more
        mode, filt = gap_combos[k % len(gap_combos)]             # than the output has, so that the horizontal pass runs
        ow = int(rng.integers(2, 4))
        fx = int(rng.integers(5, 9))
        iw, ih = ow * fx + int(rng.integers(1, ow)), int(rng.integers(700, 1201))
        oh = int(rng.integers(ih // 2 + 1, ih))
        cases.append(Case(mode, filt, iw, ih, ow, oh, None, 1.0, "into"))
    for k in range(30):   # tall, reduced down by a large fy: a few dozen rows remain
        mode, filt = gap_combos[(7 * k) % len(gap_combos)]
        iw = int(rng.integers(2, 9))
        ih = int(rng.integers(100 * iw + 1, 1201))
        oh = int(rng.integers(2, 9))
        ow = int(rng.integers(1, 41))
        cases.append(Case(mode, filt, iw, ih, ow, oh, None, 1.0, "outof"))
    return cases


def test_models_equal_live_pillow_over_a_stratified_sweep():
    """Every case is legal by construction: Pillow raises on none and none is skipped.  The counts of every stratum are
    asserted, and so is that the models with order="h_first" (what they computed before the rule) miss Pillow on at least
    80 % of the tall cases with a weighted filter whose passes both run: this sweep would have caught the defect."""
    pytest.importorskip("PIL")
    g = golden_module()
    cases = _draw_cases()
    assert 1900 <= len(cases) <= 2100
    n = collections.Counter()
    per_combo = collections.Counter()
    compared = 0
    mismatches, h_first_eligible, h_first_differs = [], 0, 0
    for i, c in enumerate(cases):
        assert c.in_w * c.in_h <= MAX_PIXELS and c.out_w * c.out_h <= MAX_PIXELS
        rw, rh, both = _reduced(c)
        tall = M.pillow_vertical_first(rw, rh, c.out_h)
        tall_request = M.pillow_vertical_first(c.in_w, c.in_h, c.out_h)
        fractional = c.box is not None and any(float(v) != int(v) for v in c.box)
        per_combo[(c.mode, c.filt)] += 1
        n["tall"] += tall
        n["tall_fractional_box"] += tall and fractional
        n["tall_gap"] += tall and c.gap is not None
        n["tall_only_reduced"] += tall and not tall_request
        n["tall_only_request"] += tall_request and not tall
        n["box"] += c.box is not None
        n["gap"] += c.gap is not None
        for s in range(3):
            n[f"side{s}"] += any(SIDES[s][0] <= v <= SIDES[s][1] for v in (c.in_w, c.in_h, c.out_w, c.out_h))
        img = g.make_plane(np.random.default_rng(5000 + i), c.mode, c.in_w, c.in_h)
        want = g.pillow_resize(img, c.mode, FM.NAMES[c.filt], c.out_w, c.out_h, c.box, c.gap)   # raises: the test fails
        got = FM.resize(img, c.filt, c.out_w, c.out_h, c.box, c.gap, alpha=c.mode == "RGBA")
        compared += 1
        if not FM.same(got, want):
            mismatches.append(c)
        if tall and both and c.filt != FM.NEAREST:
            h_first_eligible += 1
            old = FM.resize(img, c.filt, c.out_w, c.out_h, c.box, c.gap, alpha=c.mode == "RGBA", order="h_first")
            h_first_differs += not FM.same(old, want)
    print(f"{len(cases)} cases, {dict(n)}; h_first differs on {h_first_differs} of {h_first_eligible}; "
          f"{len(mismatches)} mismatches")
    assert compared == len(cases)   # none skipped
    assert set(per_combo) == set(_combos()) and min(per_combo.values()) >= 20, per_combo
    assert n["tall"] >= 300 and n["tall_fractional_box"] >= 60 and n["tall_gap"] >= 40, n
    assert n["tall_only_reduced"] >= 10 and n["tall_only_request"] >= 10, n
    assert min(n["side0"], n["side1"], n["side2"]) >= 300, n
    assert not mismatches, (len(mismatches), mismatches[:5])
    assert h_first_eligible >= 200 and h_first_differs >= 0.8 * h_first_eligible, (h_first_differs, h_first_eligible)


# ---- the committed fixture -------------------------------------------------------------------------------------------------

def _tall(g, case):
    return g.vertical_first(*g.reduced_size(FM, case[:8]), case[5])


def test_fixture_equals_model(fixture):
    g, cases = fixture
    assert len(cases) == len(g.all_cases()) == 171 and os.path.getsize(GOLDEN) < 1 << 20
    seen = collections.Counter()
    for name, case in cases.items():
        f, m, iw, ih, ow, oh, box, gap, img, want = case
        assert g.vertical_first(iw, ih, oh) == M.pillow_vertical_first(iw, ih, oh)
        got = FM.resize(img, FM.NAMES.index(f), ow, oh, box, gap, alpha=m == "RGBA")
        assert FM.same(got, want), name
        if _tall(g, case):
            seen[(f, m, "box" if box is not None else "full")] += 1
    weighted = {(f, m, b) for f in g.FILTERS[:5] for m in g.MODES for b in ("box", "full")}
    nearest = {("nearest", m, b) for m in ("L", "RGBA", "F") for b in ("box", "full")}
    assert set(seen) >= weighted | nearest


def test_fixture_sits_on_both_sides_of_every_edge(fixture):
    g, cases = fixture
    side = {name: _tall(g, case) for name, case in cases.items()}
    request = {name: g.vertical_first(case[2], case[3], case[5]) for name, case in cases.items()}
    for f in ("lanczos", "bilinear"):
        for m in ("L", "RGBA", "I16", "F"):
            t = f"_{f}_{m}"
            assert not side["h100_at" + t] and side["h100_over" + t]
            assert side["shrink_by1" + t] and not side["shrink_by0" + t] and not side["shrink_grow" + t]
            assert side["onepass_w4" + t] and side["onepass_w1" + t]
            for s in ("shrink_by0", "shrink_by1", "shrink_grow", "h100_at", "h100_over"):
                assert g.both_run(MB, FM, cases[s + t][:8]), s + t
            for s in ("onepass_w4", "onepass_w1"):
                assert not g.both_run(MB, FM, cases[s + t][:8]), s + t
    for f in ("lanczos", "bicubic"):
        for m in ("L", "RGB"):
            t = f"_{f}_{m}"
            assert side["gap_into" + t] and not request["gap_into" + t]
            assert not side["gap_outof" + t] and request["gap_outof" + t]
            assert side["gap_stays" + t] and request["gap_stays" + t]
            assert side["gap_unit" + t]
            c = cases["gap_unit" + t]
            assert FM.gap_plan(FM.NAMES.index(f), *c[2:8])[:2] == (1, 1)
            c = cases["gap_stays" + t]
            assert FM.gap_plan(FM.NAMES.index(f), *c[2:8])[:2] == (1, 3)
            for s in ("gap_into", "gap_outof", "gap_stays", "gap_unit"):
                assert g.both_run(MB, FM, cases[s + t][:8]), s + t


def test_fixture_tells_the_two_orders_apart(fixture):
    """what the generator refuses to write a fixture without, on the committed file: no tall case with a weighted filter
    whose passes both run is reproduced by the horizontal-first model; every other case is (the order does not matter there)"""
    g, cases = fixture
    told = 0
    for name, case in cases.items():
        f, m, iw, ih, ow, oh, box, gap, img, want = case
        old = FM.resize(img, FM.NAMES.index(f), ow, oh, box, gap, alpha=m == "RGBA", order="h_first")
        if g.tells_the_orders_apart(MB, FM, case[:8]):
            assert not FM.same(old, want), name
            told += 1
        else:
            assert FM.same(old, want), name
    assert told == 118


def test_host_tables_of_both_calls_equal_the_model(fixture):
    """a tall request runs the tables of its two axes in the other order, not other tables: for every fixture case whose
    filter is weighted the library's host tables of both axes equal the model's, over the reduced frame under a gap"""
    g, cases = fixture
    checked = 0
    for name, case in cases.items():
        f, m, iw, ih, ow, oh, box, gap, img, want = case
        if f == "nearest":
            continue
        filt = FM.NAMES.index(f)
        wide = m in ("I;16", "F")
        d = L.resize_desc(iw, ih, ow, oh, g.channels(m), alpha=m == "RGBA", bits=16 if m == "I;16" else 8, f32=m == "F", filter=f)
        rw, rh = g.reduced_size(FM, case[:8])
        b = box if box is not None else (0, 0, iw, ih)
        if (rw, rh) != (iw, ih):
            b = FM.gap_plan(filt, iw, ih, ow, oh, box, gap)[4]
        for axis, in_n, out_n, b0, b1 in ((0, rw, ow, b[0], b[2]), (1, rh, oh, b[1], b[3])):
            if not MB.axis_runs(in_n, out_n, b0, b1):
                continue
            taps = L.resize_taps_f64_host if wide else L.resize_taps_host
            lf, lc, lk = taps(d, axis, box=box if box is not None or gap is not None else (0, 0, iw, ih), reducing_gap=gap)
            mf, mc, mk = FM.axis_tables(filt, in_n, out_n, b0, b1, f64=wide)
            assert np.array_equal(lf, mf) and np.array_equal(lc, mc), (name, axis)
            assert lk.tobytes() == mk.tobytes(), (name, axis)
            checked += 1
    assert checked >= 250


def test_plans_of_the_fixture_cases(fixture):
    """the planner reports fused = 0 for a request that runs vertical first, and goes on planning the twins on the other side
    of each edge as it did (these small frames all fit the fused kernel)"""
    g, cases = fixture
    for name, case in cases.items():
        f, m, iw, ih, ow, oh, box, gap, img, want = case
        if f == "nearest":
            continue
        d = L.resize_desc(iw, ih, ow, oh, g.channels(m), alpha=m == "RGBA", bits=16 if m == "I;16" else 8, f32=m == "F", filter=f)
        p = L.resize_plan_host(d, 1, box=box if box is not None else (0, 0, iw, ih), reducing_gap=gap)
        both = g.both_run(MB, FM, case[:8])
        assert (bool(p.pass_h) and bool(p.pass_v)) == both, name
        assert (p.reduced_w, p.reduced_h) == tuple(g.reduced_size(FM, case[:8])), name
        assert p.inner.fused == (1 if both and not _tall(g, case) else 0), name
        if box is None and gap is None:
            assert L.resize_plan_host(d, 1).fused == p.inner.fused, name
        w = L.resize_window_plan_host(d, (0, 0, ow, max(1, oh // 2)), 1, box=box, reducing_gap=gap)
        assert w.inner.fused == p.inner.fused, name
        if m in ("L", "RGB", "RGBX"):
            cp = L.resize_crops_plan_host(d, (ow, max(1, oh // 2)), 1, box=box, reducing_gap=gap)
            assert cp.inner.fused == p.inner.fused, name
