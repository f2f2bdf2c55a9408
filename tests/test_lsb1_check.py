"""The per-sample LSB1 check (tests/lsb1_check.py, oracle_explain_hwc_*) proven on the CPU before the GPU tests rely on it:
  * the oracle's own output is explained everywhere with no +1, and the classification's store(v) IS the reference (the
    threaded restatement and the reference's recorded outputs in tests/golden/golden_small.npz);
  * a numpy model of the LSB1 vertical pass (T from the oracle, f32 weights, an f32 chain, floor(sum + eps), integer-phase
    rows copied, prefix rows from the oracle) passes and produces +1s -- the check admits what the kernels legitimately do;
  * four wrong variants of it are caught: f16 weights, round-to-nearest instead of the biased floor, one integer-phase H sample
    off by one in a dark region (what a broken fix-up list would do), a +1 where the reference's sum is far from a boundary;
  * delta covers 2 eps of every instance the GPU tests reach (tests/native/lsb1_eps_check.hip, built with hipcc, no GPU)."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import lsb1_check as LC
import oracle_lib as O
import patterns as P
from test_parity_gpu import RATIONAL_SHAPES, SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(img, sn, sd, a):
    h, w, c = img.shape
    return O.cfg(w, h, w * sn // sd, h * sn // sd, c, a, sn, sd)


def _expected(img, sn, sd, a, threads=4):
    c = _cfg(img, sn, sd, a)
    return O.expected_hwc_u8(c, img, threads) if img.dtype == np.uint8 else O.expected_hwc_u16(c, img, threads)


def _self_check(img, sn, sd, a, what):
    """The oracle's own output: every sample equal to store(v) (no copy rule: the reference itself does not copy the
    integer-phase rows), the classification's reference output identical to the restatement's."""
    want = _expected(img, sn, sd, a)
    st, ref = O.explain_hwc(_cfg(img, sn, sd, a), img, want, LC.delta_for(img.dtype, sn, sd, a), False, 4, want_ref=True)
    assert np.array_equal(ref, want), what
    assert st.unexplained == 0 and st.plus1 == 0 and st.equal == st.samples == want.size, (what, st.unexplained, st.plus1)
    return st


@pytest.mark.parametrize("pattern", ["noise", "dark"])
def test_oracle_output_is_explained_medium_shapes(pattern):
    for (w, h, c, sn, sd, a) in SHAPES + RATIONAL_SHAPES:
        _self_check(P.ALL_U8[pattern](h, w, c), sn, sd, a, f"{pattern} {w}x{h}x{c} {sn}/{sd} a={a}")


def test_oracle_output_is_explained_u16_prefix_and_tiny():
    cases = []
    for (w, h, c, sn, sd, a) in [(96, 64, 4, 2, 1, 4), (80, 50, 3, 2, 1, 3), (64, 48, 1, 3, 1, 2), (96, 60, 4, 3, 2, 3),
                                 (148, 37, 3, 3, 1, 3), (160, 45, 4, 2, 1, 4)]:
        cases.append((P.noise(h, w, c, seed=9, dtype=np.uint16), sn, sd, a, f"u16 {w}x{h}x{c} {sn}/{sd} a={a}"))
    for (w, h, c, sn, sd, a) in [(128, 96, 3, 9, 8, 3), (128, 160, 3, 33, 32, 3), (64, 1024, 3, 1025, 1024, 3)]:
        cases.append((P.noise(h, w, c, seed=31), sn, sd, a, f"deep prefix {sn}/{sd}"))
    for (w, h, c, a) in [(64, 48, 3, 3), (40, 200, 1, 3)]:
        cases.append((P.dark_noise(h, w, c, seed=5), 1, 1, a, f"S=1 dark {w}x{h}x{c}"))
    rng = np.random.default_rng(11)
    for (w, h, c, sn, sd, a) in [(1, 1, 3, 2, 1, 3), (2, 3, 1, 2, 1, 4), (3, 2, 4, 3, 1, 3), (5, 4, 3, 2, 1, 2),
                                 (4, 7, 3, 3, 2, 3), (7, 1, 3, 2, 1, 3), (1, 9, 4, 4, 1, 2)]:
        cases.append((rng.integers(0, 256, (h, w, c), dtype=np.uint8), sn, sd, a, f"tiny {w}x{h}x{c}"))
    for img, sn, sd, a, what in cases:
        st = _self_check(img, sn, sd, a, what)
        if what.startswith("deep") or what.startswith("S=1"):
            assert st.inplace_rows > 2 * a, what       # the prefix rows (delta 0) are a large part of these frames


def test_reference_outputs_in_golden_fixtures_are_explained():
    """tests/golden/golden_small.npz holds outputs of the reference's own compiled lines: each one is store(v) everywhere."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "golden_small.npz"))
    keys = sorted({k.rsplit(":", 1)[0] for k in z.files})
    assert len(keys) >= 20
    for k in keys:
        dims, out, sc, a, c = k.split(":")[0].split("_")
        sn, sd = (int(v) for v in sc.split("-"))
        img = np.ascontiguousarray(z[k + ":in"].transpose(1, 2, 0))
        want = np.ascontiguousarray(z[k + ":out"].transpose(1, 2, 0))
        st, ref = O.explain_hwc(_cfg(img, sn, sd, int(a[1:])), img, want, LC.DELTA_U8, False, 2, want_ref=True)
        assert np.array_equal(ref, want), k
        assert st.unexplained == 0 and st.equal == st.samples, k


# ------------------------------------------------------------------------------------- a numpy model of the LSB1 V pass
def _f32_eps(wrows, maxv):
    """A bound on |f32 chain - f64 sum| for the model below (weights rounded to f32, product and add rounded separately)."""
    u = 2.0 ** -24
    eps = 0.0
    for w in wrows:
        s = np.abs(w) * maxv
        e = float(np.sum(s)) * u * 2                          # weight rounding + product rounding
        e += sum(float(np.sum(s[:k + 1])) * u * 1.01 for k in range(len(w)))   # each add (|acc| <= running sum of |terms|)
        eps = max(eps, e)
    return eps * 1.05 + 1e-9


def _lsb1_model(img, sn, sd, a, weights=np.float32, store="floor", T=None):
    """T from the oracle (bit-exact H pass), V pass in float32 from `weights`-precision weights, integer-phase rows copied
    from T, rows < K from the oracle; store: 'floor' = floor(sum + eps) (the kernels), 'nearest' = round(sum)."""
    c = _cfg(img, sn, sd, a)
    if T is None:
        T = O.hpass_hwc(c, img)
    maxv = 255.0 if img.dtype == np.uint8 else 65535.0
    out = _expected(img, sn, sd, a).copy()          # rows < K stay the oracle's
    K = O.inplace_rows(c)
    scale = sn / sd
    kern = O.lib().oracle_lanczos_kernel
    rows = []
    for o in range(K, c.out_h):
        x = o / scale
        lo, hi = max(0, math.floor(x) - a + 1), min(c.in_h - 1, math.floor(x) + a)
        rows.append((o, x, lo, hi, np.array([kern(x - i, a) for i in range(lo, hi + 1)])))
    eps = np.float32(_f32_eps([r[4] for r in rows], maxv))
    Tf = T.astype(np.float32)
    for (o, x, lo, hi, w) in rows:
        if x == math.floor(x):
            out[o] = T[int(x)]
            continue
        wq = w.astype(weights).astype(np.float32)
        acc = np.full(Tf.shape[1:], eps if store == "floor" else 0, np.float32)
        for k, i in enumerate(range(lo, hi + 1)):
            acc = (acc + np.float32(wq[k]) * Tf[i]).astype(np.float32)
        v = np.floor(acc) if store == "floor" else np.rint(acc)
        out[o] = np.clip(v, 0, maxv).astype(img.dtype)
    return out, float(eps)


MODEL_CASES = [(P.noise(45, 160, 3, seed=4), 2, 1, 3), (P.dark_noise(45, 160, 3, seed=3), 2, 1, 3),
               (P.noise(37, 148, 1, seed=4), 3, 1, 4), (P.gradient_noise(40, 96, 4, seed=2), 4, 1, 2),
               (P.noise(60, 90, 3, seed=5), 4, 3, 3)]


def test_model_of_the_lsb1_vertical_pass_is_explained():
    plus1 = 0
    for (img, sn, sd, a) in MODEL_CASES:
        got, eps = _lsb1_model(img, sn, sd, a)
        assert 2 * eps <= LC.delta_for(img.dtype, sn, sd, a)
        r = LC.check(img, sn, sd, a, got, LC.FAMILY_FAST, f"model {img.dtype} {sn}/{sd} a={a}", threads=4)
        assert r["int_row_samples"] > 0
        assert r["max_plus1_gap"] <= 2 * eps
        plus1 += r["plus1"]
    assert plus1 > 0      # the check admits the +1s the biased floor makes, not only identical bytes


def test_negative_control_f16_weights():
    bad = 0
    for (img, sn, sd, a) in MODEL_CASES:
        got, _ = _lsb1_model(img, sn, sd, a, weights=np.float16)
        d = np.abs(got.astype(int) - _expected(img, sn, sd, a).astype(int))
        st = LC.explain(img, sn, sd, a, got)
        assert st.unexplained > 0, (sn, sd, a, d.max())
        bad += st.unexplained
    print(f"f16 weights: {bad} unexplained samples")


def test_negative_control_round_to_nearest():
    for (img, sn, sd, a) in MODEL_CASES:
        got, _ = _lsb1_model(img, sn, sd, a, store="nearest")
        st = LC.explain(img, sn, sd, a, got)
        assert st.unexplained > 0 and st.first_kind == 1, (sn, sd, a)
        with pytest.raises(AssertionError, match="unexplained by the LSB1 contract"):
            LC.check(img, sn, sd, a, got, LC.FAMILY_FAST, "round to nearest", threads=4)


@pytest.mark.parametrize("off", [1, -1])
def test_negative_control_integer_phase_h_sample_off_by_one(off):
    """One H sample on an integer phase (a byte copy or a fix-up of the kernels) wrong by one LSB in a dark region: every output
    still within 1 LSB of the reference -- and reported."""
    img = P.dark_noise(45, 160, 3, seed=3)
    sn, sd, a = 2, 1, 3
    c = _cfg(img, sn, sd, a)
    T = O.hpass_hwc(c, img)
    r, ch = 20, 1
    xx = next(2 * ix for ix in range(20, 80) if 1 <= T[r, 2 * ix, ch] <= 30)   # x = xx / 2 an integer, away from the edges
    T[r, xx, ch] = int(T[r, xx, ch]) + off
    got, _ = _lsb1_model(img, sn, sd, a, T=T)
    assert np.abs(got.astype(int) - _expected(img, sn, sd, a).astype(int)).max() <= 1
    st = LC.explain(img, sn, sd, a, got)
    assert st.unexplained > 0, off
    assert st.first_x == xx and st.first_c == ch and abs(st.first_o - 2 * r) <= 2 * a, (st.first_o, st.first_x, st.first_c)


def test_negative_control_plus_one_far_from_a_boundary():
    img = P.noise(45, 160, 3, seed=4)
    sn, sd, a = 2, 1, 3
    c = _cfg(img, sn, sd, a)
    want = _expected(img, sn, sd, a)
    T = O.hpass_hwc(c, img).astype(np.float64)
    kern = O.lib().oracle_lanczos_kernel
    o, ch = 41, 0                                    # a non-integer-phase row >= K
    x = o / 2
    lo, hi = max(0, math.floor(x) - a + 1), min(c.in_h - 1, math.floor(x) + a)
    for col in range(10, c.out_w):
        v = 0.0
        for i in range(lo, hi + 1):                  # the reference's f64 sum, full_TB.h:72-74
            v += T[i, col, ch] * kern(x - i, a)
        if 1 <= v < 250 and v - math.floor(v) < 0.5:  # margin to the next store boundary > 0.5 >> delta
            break
    got = want.copy()
    got[o, col, ch] += 1
    st = LC.explain(img, sn, sd, a, got, copies_int_rows=False)     # (the oracle's own rows: no copy rule)
    assert st.unexplained == 1 and (st.first_o, st.first_x, st.first_c, st.first_kind) == (o, col, ch, 1)
    assert st.first_got == int(want[o, col, ch]) + 1 and abs(st.first_v - v) < 1e-9
    # the same +1 on the oracle's output passes the old +-1 comparison
    assert np.abs(got.astype(int) - want.astype(int)).max() == 1


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_delta_covers_twice_eps_of_every_instance(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "lsb1_eps_check")
    csrc = os.path.join(ROOT, "lanczos-hls_amd", "csrc")
    subprocess.run([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function",
                    "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "native", "lsb1_eps_check.hip"),
                    os.path.join(csrc, "lanczos_taps.cpp"), "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    assert "all instances ok" in r.stdout
    pat = re.compile(r"^eps (\w+) u(\d+) C(\d) (\d+)/(\d+) a(\d) (\d+)x(\d+): (\S+)  delta (\S+)", re.M)
    seen = set()
    for fam, bits, c, sn, sd, a, w, h, eps, delta in pat.findall(r.stdout):
        dt = np.uint8 if bits == "8" else np.uint16
        assert float(delta) == LC.delta_for(dt, int(sn), int(sd), int(a))       # the harness and the helper agree
        assert 2 * float(eps) <= float(delta), (fam, bits, c, sn, sd, a, w, h, eps)
        seen.add((fam, bits, int(c), int(sn), int(sd), int(a)))
    # every integer-scale instance (8-bit C {1,3,4} x S {2,3,4} x a {2,3,4}, 16-bit C {3,4} x S {2,3} x a {3,4}), k_rat at every
    # rational scale of the GPU tests, k_ratp where it has instances
    for c in (1, 3, 4):
        for s in (2, 3, 4):
            for a in (2, 3, 4):
                assert ("fast", "8", c, s, 1, a) in seen
    for c in (3, 4):
        for s in (2, 3):
            for a in (3, 4):
                assert ("fast", "16", c, s, 1, a) in seen
    for (_, _, _, sn, sd, a) in RATIONAL_SHAPES:
        g = math.gcd(sn, sd)
        assert ("rat", "8", 3, sn // g, sd // g, a) in seen
    assert ("rat", "16", 3, 3, 2, 3) in seen and ("ratp", "16", 4, 3, 2, 3) in seen
    assert any(k[0] == "ratp" and k[1] == "8" for k in seen)
