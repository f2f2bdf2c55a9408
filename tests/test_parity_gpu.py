"""GPU parity: the HIP path, called through the C ABI, against the CPU checker.

  * golden fixtures (reference outputs) and known-answer digests: bit-exact in EXACT mode
  * oracle on seeded synthetic frames (noise / dark / gradient / blocks): EXACT mode bit-exact;
    default LSB1 mode within +-1 LSB per sample (the tolerance BASELINE.json's north_star states) AND per sample within the
    mode's stated contract (tests/lsb1_check.py: +1 only where the reference's f64 sum lies within delta below a store
    boundary, integer-phase rows copies of the H intermediate, prefix rows and k_generic bit-exact)
  * edge cases the reference's loop bounds imply: tiny images (every tap range clipped), a = 2/3/4,
    1/3/4 channels, non-integer scales, the in-place prefix rows, strips, batches, u16
  * per-instance coverage lives in modules of its own: every k_ratp / k_rat instance in tests/test_rational_instances_gpu.py, every
    k_fast tile-kernel instance (whole on contents that steer its FIXUP worklist, in row strips, in batches with strides off
    16 bytes) and both k_generic kernels (in strips and strided batches, 16-bit samples forced) in
    tests/test_fast_instances_gpu.py, every k_march instance on contents that steer its fix-up worklist and its f64 redo rows in
    tests/test_march_fixup_gpu.py (what each content reaches: tests/test_march_fixup_cfg.py, no GPU);
    test_every_integer_scale_instance below stays as the one-frame pass over both the marching and the tile kernel
"""
import json
import os

import numpy as np
import pytest

import lanczos_hls_amd as L
import lsb1_check as LC
import oracle_lib as O
import patterns as P

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _parse(key):
    dims, out, sc, a, c = key.split("_")
    iw, ih = (int(v) for v in dims.split("x"))
    ow, oh = (int(v) for v in out.split("x"))
    sn, sd = (int(v) for v in sc.split("-"))
    return iw, ih, ow, oh, sn, sd, int(a[1:]), int(c[1:])


def _oracle(img, sn, sd, a, threads=8):
    h, w, c = img.shape
    cfg = O.cfg(w, h, w * sn // sd, h * sn // sd, c, a, sn, sd)
    if img.dtype == np.uint16:
        return O.expected_hwc_u16(cfg, img, threads)
    return O.expected_hwc_u8(cfg, img, threads)


def _cmp(got, want, mode, what, req=None):
    """EXACT: bit-identical.  LSB1: within 1 LSB, and `req` = (img, sn, sd, a, kernel family) must be given: the sample-by-sample
    contract of tests/lsb1_check.py is checked on top."""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    if mode == L.MODE_EXACT:
        assert diff.max() == 0, f"{what}: {np.count_nonzero(diff)} samples differ, max {diff.max()}"
    else:
        assert diff.max() <= 1, f"{what}: max |diff| {diff.max()} > 1 LSB"
        assert req is not None, f"{what}: an LSB1 comparison needs the request for the per-sample check"
        img, sn, sd, a, family = req
        LC.check(img, sn, sd, a, got, family, what)
    return int(np.count_nonzero(diff))


def _req(ctx, img, sn, sd, a):
    """The request of the last call on ctx, with the kernel family that served it."""
    return (img, sn, sd, a, ctx.last_kernel())


@pytest.mark.parametrize("family", [L.KERNEL_GENERIC, L.KERNEL_NONE])
@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_LSB1])
def test_golden_fixtures(ctx, family, mode):
    """Reference outputs committed under tests/golden (made by the reference's own compiled lines)."""
    z = np.load(os.path.join(GOLD, "golden_small.npz"))
    keys = sorted({k.rsplit(":", 1)[0] for k in z.files})
    ctx.force_kernel(family)
    try:
        for k in keys:
            shape, pname = k.split(":")
            iw, ih, ow, oh, sn, sd, a, c = _parse(shape)
            img = np.ascontiguousarray(z[k + ":in"].transpose(1, 2, 0))      # planar -> stb layout
            want = np.ascontiguousarray(z[k + ":out"].transpose(1, 2, 0))
            got = ctx.resample(img, sn, sd, a, mode)
            fam = ctx.last_kernel()
            if family == L.KERNEL_GENERIC:
                assert fam == L.KERNEL_GENERIC, k
                _cmp(got, want, L.MODE_EXACT, k + " (k_generic: bit-exact in every mode)")
            _cmp(got, want, mode, k, (img, sn, sd, a, fam))
    finally:
        ctx.force_kernel(L.KERNEL_NONE)


def test_known_answer_digests_full_size(ctx):
    """BASELINE configs 2 and 3 at full size: FNV-1a-64 of the planar output equals the reference's
    digest -- no CPU work needed on the box."""
    with open(os.path.join(GOLD, "kat_digests.json")) as f:
        kat = json.load(f)
    for shape in ("1920x1080_3840x2160_2-1_a3_c3", "1280x720_3840x2160_3-1_a3_c3",
                  "256x256_512x512_2-1_a2_c3", "480x270_960x540_2-1_a4_c4", "300x200_400x266_4-3_a3_c3"):
        iw, ih, ow, oh, sn, sd, a, c = _parse(shape)
        planar = O.lcg_u8(c * ih * iw, 12345).reshape(c, ih, iw)
        got = ctx.resample(np.ascontiguousarray(planar.transpose(1, 2, 0)), sn, sd, a, L.MODE_EXACT)
        assert got.shape == (oh, ow, c)
        dig = O.fnv1a64(np.ascontiguousarray(got.transpose(2, 0, 1)))
        assert f"{dig:016x}" == kat["survey_8c"][shape], shape


SHAPES = [
    # (in_w, in_h, channels, sn, sd, a)
    (200, 120, 3, 2, 1, 3), (160, 90, 3, 3, 1, 3), (128, 96, 3, 2, 1, 2), (96, 64, 4, 2, 1, 4),
    (150, 100, 3, 4, 3, 3), (120, 80, 1, 2, 1, 3), (90, 60, 4, 3, 1, 2), (100, 75, 3, 3, 2, 3),
    (64, 33, 1, 5, 2, 4), (515, 131, 3, 2, 1, 3), (333, 77, 3, 3, 1, 3),
    # served by the specialised kernels: several tiles wide/tall, ragged right and bottom edges
    (514, 131, 3, 2, 1, 3), (320, 99, 3, 3, 1, 3), (700, 50, 3, 2, 1, 3), (130, 300, 3, 2, 1, 3),
    (260, 200, 4, 2, 1, 4), (260, 200, 1, 2, 1, 3), (258, 70, 3, 2, 1, 2), (258, 70, 3, 2, 1, 4),
    (200, 90, 4, 2, 1, 3),
    # rows that are 16-byte multiples -> the marching kernel (ragged strips, several chunks, tiny heights)
    (208, 131, 3, 2, 1, 3), (144, 77, 3, 3, 1, 3), (400, 50, 3, 2, 1, 3), (64, 300, 3, 2, 1, 3),
    (256, 200, 1, 2, 1, 3), (272, 9, 3, 2, 1, 3), (16, 40, 3, 2, 1, 4), (48, 30, 3, 2, 1, 2),
]


def _fast_expected(w, c, sn, sd, bps=1):
    """Which kernel family must serve a shape: the specialised kernels take every integer scale 2..4 (round 3: all of
    C in {1,3,4} x a in {2,3,4}, the reference's params.h space lanczos.h:9-31) and the periodic / per-index rational kernels
    every other scale, whenever the output rows are dword multiples; only ragged rows fall to the f64 generic kernel."""
    return (w * sn // sd * c * bps) % 4 == 0 and (sd != 1 or sn <= 4)


@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_LSB1])
@pytest.mark.parametrize("pattern", ["noise", "dark", "gradient", "blocks"])
def test_oracle_parity_medium(ctx, pattern, mode):
    for (w, h, c, sn, sd, a) in SHAPES:
        img = P.ALL_U8[pattern](h, w, c)
        want = _oracle(img, sn, sd, a)
        got = ctx.resample(img, sn, sd, a, mode)
        _cmp(got, want, mode, f"{pattern} {w}x{h}x{c} {sn}/{sd} a={a}", _req(ctx, img, sn, sd, a))
        want_family = L.KERNEL_FAST if _fast_expected(w, c, sn, sd) else L.KERNEL_GENERIC
        assert ctx.last_kernel() == want_family, (w, h, c, sn, sd, a, ctx.last_kernel())


@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_LSB1])
def test_every_integer_scale_instance(ctx, mode):
    """Every instantiated (sample type, channels, scale, a) of the integer-scale kernels (lanczos_fast.hpp LZ_FAST_CONFIGS:
    8-bit C in {1,3,4} x S in {2,3,4} x a in {2,3,4}; 16-bit C in {3,4} x S in {2,3} x a in {3,4}) against the oracle, once
    with rows that are 16-byte multiples (the marching kernel) and once ragged (the tile kernel), dark noise (integer-phase
    fix-ups everywhere) and plain noise.  16-bit: parity unpinned by the reference (checker = the templated restatement)."""
    cases = [(np.uint8, c, s, a) for c in (1, 3, 4) for s in (2, 3, 4) for a in (2, 3, 4)]
    cases += [(np.uint16, c, s, a) for c in (3, 4) for s in (2, 3) for a in (3, 4)]
    for (dt, c, s, a) in cases:
        bps = np.dtype(dt).itemsize
        # 160*c*bps is a 16-byte multiple for every case; 148 is not for 1 and 3 channels, 149 is not for 4 (dword rows all)
        for (w, h) in ((160, 45), (149 if c == 4 else 148, 37)):
            assert ((w * c * bps) % 16 == 0) == (w == 160) and (w * s * c * bps) % 4 == 0
            for pat, seed in (("dark", 3), ("noise", 4)):
                img = (P.dark_noise(h, w, c, seed=seed) if pat == "dark" else P.noise(h, w, c, seed=seed)) if dt == np.uint8 else \
                      (P.noise(h, w, c, seed=seed, dtype=np.uint16) >> (8 if pat == "dark" else 0)).astype(np.uint16)
                want = _oracle(img, s, 1, a)
                got = ctx.resample(img, s, 1, a, mode)
                _cmp(got, want, mode, f"{dt.__name__} c={c} {s}x a={a} {w}x{h} {pat}", _req(ctx, img, s, 1, a))
                assert ctx.last_kernel() == L.KERNEL_FAST, (dt.__name__, c, s, a, w)
                r = ctx.last_route()   # one frame: the prefix rows ride on k_march; behind the tile kernel they are k_prefix's
                assert (r.main, r.prefix, r.launches) == ((L.ROUTE_MAIN_MARCH, L.ROUTE_PREFIX_RIDING, 1) if w == 160 else
                                                          (L.ROUTE_MAIN_TILE, L.ROUTE_PREFIX_BEHIND, 1)), (dt.__name__, c, s, a, w, str(r))


def test_sixteen_bit_exact_mode_split_weight_chains(ctx):
    """The EXACT instances of the 16-bit 2x kernels run split-weight chains in both passes (lanczos_march.hpp: SPLIT -- an exactly
    summing coarse half plus a small remainder; tests/test_split_chain.py proves the arithmetic on the CPU).  Content chosen for
    what that arithmetic has to get right: empty channels and black regions (sums exactly 0: exempt from the undecided flag),
    saturated edges (overshoot above 65535 and below 0: the saturating converts), flat areas (every sample of a row on the same
    fraction), a smooth ramp with noise, plain noise.  Bit-identical to the checker; 16-bit: parity unpinned by the reference."""
    h, w = 70, 320
    yy, xx = np.mgrid[0:h, 0:w]
    for c in (3, 4):
        cc = np.arange(c)[None, None, :]
        blocks = (((yy // 16 + xx // 16)[..., None] + cc) % 5 * 15000).astype(np.uint16)           # one channel in five is 0
        edges = np.where(((xx // 24 + yy // 10) % 2 == 0)[..., None], 65535, 0).astype(np.uint16).repeat(c, 2)
        edges[..., 0] = 0                                                                          # an empty channel
        ramp = np.clip(((yy * 900 + xx * 190)[..., None] + P.noise(h, w, c, seed=5, dtype=np.uint16) // 64), 0, 65535).astype(np.uint16)
        flat = np.full((h, w, c), 40000, np.uint16)
        flat[:, w // 2:] = 12345
        for a in (3, 4):
            for name, img in (("blocks", blocks), ("edges", edges), ("ramp", ramp), ("flat", flat),
                              ("noise", P.noise(h, w, c, seed=6, dtype=np.uint16))):
                img = np.ascontiguousarray(img)
                want = _oracle(img, 2, 1, a)
                for mode in (L.MODE_EXACT, L.MODE_LSB1):
                    got = ctx.resample(img, 2, 1, a, mode)
                    _cmp(got, want, mode, f"uint16 c={c} a={a} {name}", _req(ctx, img, 2, 1, a))
                    assert ctx.last_kernel() == L.KERNEL_FAST


RATIONAL_SHAPES = [
    # (in_w, in_h, channels, sn, sd, a) -- output rows are dword multiples: served by k_rat
    (300, 200, 3, 4, 3, 3), (256, 120, 3, 3, 2, 3), (400, 90, 4, 3, 2, 2), (128, 77, 1, 5, 2, 4), (240, 131, 3, 5, 3, 3),
    (96, 64, 4, 7, 4, 4), (12, 9, 4, 4, 3, 3), (64, 300, 1, 3, 2, 3), (1200, 40, 3, 4, 3, 3), (12, 5, 3, 4, 3, 2),
]


# the instances of k_ratp (lanczos_rational.hpp LZ_RATP_CONFIGS) as (bytes per sample, channels, N, D, a): tests/ratp_cfg.py
# holds the one list, tests/test_rational_instances.py compares it with the header
from ratp_cfg import RATP_INSTANCES  # noqa: E402


@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_LSB1])
@pytest.mark.parametrize("pattern", ["noise", "dark", "gradient", "blocks"])
def test_rational_scales_fast_kernel(ctx, pattern, mode):
    """4/3, 3/2, 5/2, 5/3, 7/4: the reference reduces SCALE_N/SCALE_D with gcd (lanczos.h:108-114) and evaluates
    x = xx / SCALE in double; k_rat follows its per-index taps, k_ratp serves the frames the host found periodic.
    Of k_ratp's 11 instances these shapes reach three -- (u8, C, N, D, a) = (3, 4, 3, 3) at 300 x 200 and 1200 x 40, (3, 3, 2, 3)
    at 256 x 120, (1, 3, 2, 3) at 64 x 300 -- and the 16-bit tail a fourth, (u16, 4, 3, 2, 3); of k_rat's six (sample type, a)
    pairs they reach uint8 with a = 2, 3, 4.  Every instance of both families, in both modes, on multi-tile ragged frames, in
    strips and in strided batches: tests/test_rational_instances_gpu.py."""
    for (w, h, c, sn, sd, a) in RATIONAL_SHAPES:
        img = P.ALL_U8[pattern](h, w, c)
        want = _oracle(img, sn, sd, a)
        got = ctx.resample(img, sn, sd, a, mode)
        _cmp(got, want, mode, f"{pattern} {w}x{h}x{c} {sn}/{sd} a={a}", _req(ctx, img, sn, sd, a))
        assert ctx.last_kernel() == L.KERNEL_FAST, (w, h, c, sn, sd, a)
        assert ctx.last_route().main in (L.ROUTE_MAIN_RATP, L.ROUTE_MAIN_RAT), (w, h, c, sn, sd, a, str(ctx.last_route()))
        if (1, c, sn, sd, a) not in RATP_INSTANCES:       # no k_ratp instance: the per-index kernel
            assert ctx.last_route().main == L.ROUTE_MAIN_RAT, (w, h, c, sn, sd, a)
        elif min(w, h) >= 64:                             # (frames of a few periods only are left to k_rat)
            assert ctx.last_route().main == L.ROUTE_MAIN_RATP, (w, h, c, sn, sd, a)
    img16 = P.noise(60, 96, 4, seed=77, dtype=np.uint16)
    got = ctx.resample(img16, 3, 2, 3, mode)
    _cmp(got, _oracle(img16, 3, 2, 3), mode, "u16 3/2", _req(ctx, img16, 3, 2, 3))
    assert ctx.last_kernel() == L.KERNEL_FAST
    assert (2, 4, 3, 2, 3) in RATP_INSTANCES and ctx.last_route().main == L.ROUTE_MAIN_RATP   # (the one 16-bit instance)


def test_rational_fast_kernel_known_answer_and_speed(ctx):
    """SURVEY.md 8(c)'s 300x200 -> 400x266 (4/3) digest through the fast kernel, and the fast kernel against the f64
    generic kernel on a 4/3 and a 3/2 frame batch.  Measured (profiles/README.md, round 2): 4.6x at 4/3, 5.1-5.3x at 3/2,
    6.2x at 5/2; the asserted floors leave room for box-to-box spread."""
    import time
    import torch
    with open(os.path.join(GOLD, "kat_digests.json")) as f:
        kat = json.load(f)
    planar = O.lcg_u8(3 * 200 * 300, 12345).reshape(3, 200, 300)
    got = ctx.resample(np.ascontiguousarray(planar.transpose(1, 2, 0)), 4, 3, 3, L.MODE_EXACT)
    assert ctx.last_kernel() == L.KERNEL_FAST
    assert f"{O.fnv1a64(np.ascontiguousarray(got.transpose(2, 0, 1))):016x}" == kat["survey_8c"]["300x200_400x266_4-3_a3_c3"]
    for (sn, sd) in ((4, 3), (3, 2)):
        d = L.make_desc(1920, 1080, 3, sn, sd, 3)
        x = torch.from_numpy(np.stack([P.gradient_noise(1080, 1920, 3, seed=40 + i) for i in range(4)])).cuda()
        y = torch.empty((4, d.out_h, d.out_w, 3), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        times = {}
        outs = {}
        for fam in (L.KERNEL_GENERIC, L.KERNEL_NONE):
            ctx.force_kernel(fam)
            for _ in range(3):
                ctx.resample_device(d, x.data_ptr(), y.data_ptr(), 4, 0, 0, stream)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                ctx.resample_device(d, x.data_ptr(), y.data_ptr(), 4, 0, 0, stream)
            torch.cuda.synchronize()
            times[fam] = (time.perf_counter() - t0) / 10
            outs[fam] = y.clone()
        ctx.force_kernel(L.KERNEL_NONE)
        assert ctx.last_kernel() == L.KERNEL_FAST
        diff = (outs[L.KERNEL_GENERIC].to(torch.int16) - outs[L.KERNEL_NONE].to(torch.int16)).abs()
        assert int(diff.max()) <= 1                                   # LSB1 against the always-exact kernel
        _cmp(outs[L.KERNEL_NONE][0].cpu().numpy(), outs[L.KERNEL_GENERIC][0].cpu().numpy(), L.MODE_LSB1, f"rational {sn}/{sd} frame 0",
             (x[0].cpu().numpy(), sn, sd, 3, L.KERNEL_FAST))
        print(f"rational {sn}/{sd}: generic {times[L.KERNEL_GENERIC] * 1e6:.1f} us, fast {times[L.KERNEL_NONE] * 1e6:.1f} us per 4 frames")
        assert times[L.KERNEL_GENERIC] / times[L.KERNEL_NONE] >= (4.0 if (sn, sd) == (4, 3) else 4.6), (sn, sd, times)


def test_scales_close_to_one_deep_inplace_prefix(ctx):
    """S -> 1: the in-place vertical pass (full_TB.h:67-77) reads already-written rows for K ~ a*S/(S-1) output rows --
    27 rows at 9/8, 99 at 33/32, 195 at 65/64 (the cap of round 1 was 64).  Reduced N/D as lanczos.h:108-114 makes them."""
    for (w, h, c, sn, sd, a) in [(128, 96, 3, 9, 8, 3), (128, 160, 3, 33, 32, 3), (64, 256, 1, 65, 64, 3), (64, 192, 4, 17, 16, 4)]:
        img = P.noise(h, w, c, seed=31)
        d = L.make_desc(w, h, c, sn, sd, a)
        K = L.inplace_rows(d)
        assert K == (a - 1) * sn // (sn - sd) + 1
        want = _oracle(img, sn, sd, a)
        for mode in (L.MODE_EXACT, L.MODE_LSB1):
            got = ctx.resample(img, sn, sd, a, mode)
            _cmp(got, want, mode, f"deep prefix {sn}/{sd} K={K}", _req(ctx, img, sn, sd, a))
            r = ctx.last_route()   # M + M2 rows of 32 columns or more fit the LDS at all four depths: k_prefix, behind k_rat
            main = L.ROUTE_MAIN_RAT if (d.out_w * c) % 4 == 0 else L.ROUTE_MAIN_GENERIC   # (65 samples per row: k_generic)
            assert (r.main, r.prefix) == (main, L.ROUTE_PREFIX_BEHIND), (sn, sd, str(r))
    # S = 1: every sample on an integer phase, the in-place pass one recurrence over the whole height per column
    # (full_TB.h:67-77) -- the output is the input except where the double noise of the ~1e-17 taps flips a dark sample
    for (w, h, c, a, gen) in [(64, 48, 3, 3, P.dark_noise), (40, 200, 1, 3, P.dark_noise), (33, 21, 4, 4, P.noise), (96, 64, 3, 2, P.noise)]:
        img = gen(h, w, c, seed=5)
        want = _oracle(img, 4, 4, a)                # reduced to 1/1 by the gcd, like lanczos.h:110
        assert want.shape == img.shape
        for mode in (L.MODE_EXACT, L.MODE_LSB1):
            got = ctx.resample(img, 4, 4, a, mode)
            _cmp(got, want, mode, f"S=1 {w}x{h}x{c} a={a}", _req(ctx, img, 4, 4, a))
            r = ctx.last_route()
            assert (r.main, r.prefix) == (L.ROUTE_MAIN_GENERIC, L.ROUTE_PREFIX_BEHIND), (w, h, str(r))
    assert (_oracle(P.dark_noise(48, 64, 3, seed=5), 1, 1, 3) != P.dark_noise(48, 64, 3, seed=5)).any()   # (the quirk is exercised)
    # Deeper than the row arrays of k_prefix: the streaming form of the recurrence (k_prefix_stream, rings of 24 rows).  S = 1 at 4K
    # height and 1025/1024 (K = 2 * 1025 + 1 > the frame height: every output row reads written rows) -- both shapes have
    # reference builds of their own (oracle/ref_configs.txt, digests in tests/golden/kat_digests.json pin the oracle used here);
    # plus 16-bit samples, a = 4, and 257/256 with a main kernel below the prefix
    for (w, h, c, sn, sd, a, gen, dt) in [(24, 2160, 1, 1, 1, 3, P.dark_noise, np.uint8), (64, 1024, 3, 1025, 1024, 3, P.noise, np.uint8),
                                          (16, 1500, 4, 1, 1, 4, P.noise, np.uint16), (32, 1200, 3, 257, 256, 3, P.dark_noise, np.uint8)]:
        img = gen(h, w, c, seed=8) if dt == np.uint8 else P.noise(h, w, c, seed=8, dtype=np.uint16)
        d = L.make_desc(w, h, c, sn, sd, a, img.dtype.itemsize)
        want = _oracle(img, sn, sd, a)
        assert want.shape == (d.out_h, d.out_w, c)
        for mode in (L.MODE_EXACT, L.MODE_LSB1):
            got = ctx.resample(img, sn, sd, a, mode)
            _cmp(got, want, mode, f"streamed prefix {sn}/{sd} {w}x{h}x{c} a={a} K={L.inplace_rows(d)}", _req(ctx, img, sn, sd, a))
            r = ctx.last_route()   # (257/256 at 1200 rows of 8-bit samples: 1040 rows of 32 columns still fit, k_prefix serves it)
            assert r.main == (L.ROUTE_MAIN_GENERIC if sn == sd else L.ROUTE_MAIN_RAT), (sn, sd, str(r))
            assert r.prefix == (L.ROUTE_PREFIX_BEHIND if (sn, sd) == (257, 256) else L.ROUTE_PREFIX_STREAMED), (sn, sd, str(r))
    with pytest.raises(L.LanczosError) as e:       # S < 1: refused (the reference itself is out of bounds there)
        ctx.resample(P.noise(16, 16, 3), 3, 4, 3)
    assert e.value.code == L.ERR_UNSUPPORTED


def test_tiny_images_all_taps_clipped(ctx):
    """Images narrower/shorter than the 2a tap window: every loop bound of full_TB.h:59,72 clips."""
    rng = np.random.default_rng(11)
    for (w, h, c, sn, sd, a) in [(1, 1, 3, 2, 1, 3), (2, 3, 1, 2, 1, 4), (3, 2, 4, 3, 1, 3), (5, 4, 3, 2, 1, 2),
                                 (4, 7, 3, 3, 2, 3), (7, 1, 3, 2, 1, 3), (1, 9, 4, 4, 1, 2)]:
        img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        want = _oracle(img, sn, sd, a, threads=1)
        for mode in (L.MODE_EXACT, L.MODE_LSB1):
            got = ctx.resample(img, sn, sd, a, mode)
            _cmp(got, want, mode, f"tiny {w}x{h}x{c} {sn}/{sd} a={a}", _req(ctx, img, sn, sd, a))


def test_extreme_values_saturate_like_the_reference(ctx):
    """All-255 overshoots (phase-1/2 weight sum 1.019 at a=2, no renormalisation) -> clamp at 255;
    checkerboards drive sums negative -> clamp at 0 (full_TB.h:29-37)."""
    for a in (2, 3, 4):
        full = np.full((40, 56, 3), 255, np.uint8)
        chk = ((np.add.outer(np.arange(40), np.arange(56)) % 2) * 255).astype(np.uint8)[..., None].repeat(3, 2)
        for img in (full, chk, np.zeros((40, 56, 3), np.uint8)):
            want = _oracle(img, 2, 1, a)
            got = ctx.resample(img, 2, 1, a, L.MODE_EXACT)
            _cmp(got, want, L.MODE_EXACT, f"extreme a={a}")


def test_inplace_prefix_rows_follow_the_reference(ctx):
    """Rows < K must equal the in-place result (full_TB.h:67-77), which differs from a clean V pass."""
    img = P.noise(64, 80, 3, seed=5)
    for (sn, sd, a) in [(2, 1, 3), (3, 1, 3), (2, 1, 4), (4, 3, 3), (2, 1, 2)]:
        d = L.make_desc(80, 64, 3, sn, sd, a)
        K = L.inplace_rows(d)
        cfg = O.cfg(80, 64, d.out_w, d.out_h, 3, a, sn, sd)
        inplace = O.expected_hwc_u8(cfg, img)
        clean = O.outofplace_hwc_u8(cfg, img)
        got = ctx.resample(img, sn, sd, a, L.MODE_EXACT)
        assert np.array_equal(got, inplace)
        assert not np.array_equal(got[:K], clean[:K])


def test_batch_of_frames(ctx):
    frames = np.stack([P.noise(72, 96, 3, seed=100 + i) for i in range(5)])
    got = ctx.resample(frames, 2, 1, 3, L.MODE_EXACT)
    for i in range(5):
        assert np.array_equal(got[i], _oracle(frames[i], 2, 1, 3))


def test_oversized_batch_goes_out_as_several_launches(ctx):
    """A device batch of twice the marching kernel's preferred size or more (1920-wide RGB8 2x: 32 frames; one and a half times
    for the four-workgroups-per-CU instances) is split into launches of that size inside lanczos_resample_device; 70 frames =
    32 + 32 + 6, every frame against the oracle's frame
    (the frames are short, the width is config 2's: 15 strips)."""
    import torch
    w, h, f = 1920, 20, 70
    base = [P.noise(h, w, 3, seed=900 + i) for i in range(3)]
    frames = np.stack([base[i % 3] for i in range(f)])
    frames[:, 0, 0, 0] = np.arange(f, dtype=np.uint8)          # every frame differs somewhere
    d = L.make_desc(w, h, 3, 2, 1, 3, 1, L.MODE_EXACT)
    x = torch.from_numpy(frames).cuda()
    y = torch.zeros((f, d.out_h, d.out_w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.resample_device(d, x.data_ptr(), y.data_ptr(), f, 0, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    for i in (0, 1, 31, 32, 33, 63, 64, 69):
        assert np.array_equal(got[i], _oracle(frames[i], 2, 1, 3)), i
    one = ctx.resample(frames[:40], 2, 1, 3, L.MODE_EXACT)       # below one and a half times the preferred size: one launch, same bytes
    assert np.array_equal(one, got[:40])
    mid = ctx.resample(frames[:50], 2, 1, 3, L.MODE_EXACT)       # 48 <= frames < 64: 32 + 18 (round 4: the four-per-CU instances split earlier)
    assert np.array_equal(mid, got[:50])


def test_bounded_caches_survive_many_shapes():
    """The plan cache (32 shapes) and the marching kernel's table cache (64 launch shapes) retire their oldest entries by
    event instead of growing: 40 frame shapes and 70 batch sizes through ONE context, results still the oracle's, and the
    context tears down cleanly with retired entries pending."""
    import torch
    c = L.Context(0)
    try:
        first = None
        for i in range(40):                                  # 40 plans > kMaxPlans
            w, h = 64 + 16 * i, 24 + (i % 5)
            img = P.noise(h, w, 3, seed=300 + i)
            got = c.resample(img, 2, 1, 3, L.MODE_EXACT)
            if i in (0, 17, 39):
                assert np.array_equal(got, _oracle(img, 2, 1, 3)), i
            if i == 0:
                first = (img, got)
        assert np.array_equal(c.resample(first[0], 2, 1, 3, L.MODE_EXACT), first[1])   # the retired plan is rebuilt
        d = L.make_desc(208, 40, 3, 2, 1, 3, 1, L.MODE_EXACT)
        frames = np.stack([P.noise(40, 208, 3, seed=77)] * 70)
        x = torch.from_numpy(frames).cuda()
        y = torch.zeros((70, d.out_h, d.out_w, 3), dtype=torch.uint8, device="cuda")
        want = _oracle(frames[0], 2, 1, 3)
        st = torch.cuda.current_stream().cuda_stream
        for f in range(1, 71):                               # 70 launch shapes > 64 tables; no sync in between
            c.resample_device(d, x.data_ptr(), y.data_ptr(), f, 0, 0, st)
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        for f in (0, 35, 69):
            assert np.array_equal(got[f], want), f
    finally:
        c.close()


def test_row_strips_reassemble_to_the_whole_frame(ctx):
    """BASELINE config 5's sharding: output row strips with an input halo, no other exchange."""
    for (w, h, c, sn, sd, a, dtype) in [(96, 128, 4, 2, 1, 4, np.uint16), (120, 96, 3, 3, 1, 3, np.uint8),
                                        (90, 64, 3, 4, 3, 3, np.uint8)]:
        img = P.noise(h, w, c, seed=21, dtype=dtype)
        want = _oracle(img, sn, sd, a)
        oh = h * sn // sd
        parts = 4
        bounds = [oh * i // parts for i in range(parts + 1)]
        out = []
        for i in range(parts):
            d = L.make_desc(w, h, c, sn, sd, a, img.dtype.itemsize, L.MODE_EXACT,
                            out_row0=bounds[i], out_rows=bounds[i + 1] - bounds[i])
            r0, n = L.strip_input_rows(d, d.out_row0, d.out_rows)
            out.append(ctx.resample_strip(img[r0:r0 + n], d))
        assert np.array_equal(np.concatenate(out), want)


def test_u16_matches_the_templated_checker(ctx):
    """parity unpinned by the reference (no 16-bit path, full_TB.h:18,30): checked against the same
    restatement templated on the sample type (clamp 65535, truncation)."""
    for (w, h, c, sn, sd, a) in [(96, 64, 4, 2, 1, 4), (80, 50, 3, 2, 1, 3), (64, 48, 1, 3, 1, 2)]:
        img = P.noise(h, w, c, seed=9, dtype=np.uint16)
        want = _oracle(img, sn, sd, a)
        got = ctx.resample(img, sn, sd, a, L.MODE_EXACT)
        _cmp(got, want, L.MODE_EXACT, f"u16 {w}x{h}x{c}")
        got = ctx.resample(img, sn, sd, a, L.MODE_LSB1)
        _cmp(got, want, L.MODE_LSB1, f"u16 {w}x{h}x{c}", _req(ctx, img, sn, sd, a))


def test_reference_call_shape_and_errors(ctx):
    img = P.gradient_noise(48, 64, 3)
    got = ctx.u8(img, 128, 96, 3)       # the reference-shaped entry point is always bit-exact
    _cmp(got, _oracle(img, 2, 1, 3), L.MODE_EXACT, "lanczos_u8")
    with pytest.raises(L.LanczosError) as e:
        ctx.u8(img, 130, 96, 3)          # wrong output size: full_TB.h:115-118
    assert e.value.code == L.ERR_BAD_ARG
    same = ctx.u8(img, 64, 48, 3)        # scale 1 (round 3): the reference's identity-scale result, not an error
    _cmp(same, _oracle(img, 1, 1, 3), L.MODE_EXACT, "lanczos_u8 1/1")
    with pytest.raises(L.LanczosError) as e:
        ctx.u8(np.ascontiguousarray(img[:, :60]), 40, 32, 3)   # scale 2/3: the reference is out of bounds there (full_TB.h:85)
    assert e.value.code == L.ERR_UNSUPPORTED
    with pytest.raises(L.LanczosError):
        ctx.resample(np.zeros((4, 4, 2), np.uint8), 2, 1, 3)   # 2 channels


def test_full_size_properties(ctx):
    """BASELINE config 2 at full size without the CPU checker: determinism, frame independence inside a
    batch, and constant frames map to the analytically known constant."""
    f0 = P.noise(1080, 1920, 3, seed=1)
    f1 = P.gradient_noise(1080, 1920, 3)
    both = ctx.resample(np.stack([f0, f1]), 2, 1, 3)
    assert np.array_equal(both[0], ctx.resample(f0, 2, 1, 3))
    assert np.array_equal(both[1], ctx.resample(f1, 2, 1, 3))
    flat = np.full((1080, 1920, 3), 100, np.uint8)
    out = ctx.resample(flat, 2, 1, 3, L.MODE_EXACT)
    small = _oracle(np.full((40, 40, 3), 100, np.uint8), 2, 1, 3)
    assert np.array_equal(out[20:60, 20:60], small[20:60, 20:60])
    assert np.array_equal(out[:40, :40], small[:40, :40])          # top-left corner incl. prefix rows


@pytest.mark.parametrize("pattern", ["gradient", "blocks", "dark"])
def test_full_size_config2_against_oracle(ctx, pattern):
    """BASELINE config 2 at full size, the non-noise generators, every sample against the CPU checker
    (the noise generator at full size is covered by the known-answer digests)."""
    img = P.ALL_U8[pattern](1080, 1920, 3)
    want = _oracle(img, 2, 1, 3, threads=32)
    for mode in (L.MODE_LSB1, L.MODE_EXACT):
        got = ctx.resample(img, 2, 1, 3, mode)
        _cmp(got, want, mode, f"full-size {pattern}", _req(ctx, img, 2, 1, 3))
    # the same frames inside a batch of 3 on the device-pointer path the benchmark uses
    batch = np.stack([img, P.noise(1080, 1920, 3, seed=3), img[::-1].copy()])
    got = ctx.resample(batch, 2, 1, 3, L.MODE_LSB1)
    _cmp(got[0], want, L.MODE_LSB1, f"full-size {pattern} in a batch", _req(ctx, img, 2, 1, 3))


@pytest.mark.parametrize("shape", [(1920, 1080, 3, 2, 1, 3, 16), (1920, 1080, 3, 2, 1, 3, 32), (1920, 1080, 3, 2, 1, 3, 24),
                                   (1280, 720, 3, 3, 1, 3, 16), (1280, 720, 3, 3, 1, 3, 32)])
def test_benchmark_batches_every_frame(ctx, shape):
    """The launch shapes bench.py times (BASELINE configs 2 / 3 as batches of 16-32 frames): the marching kernel cuts them
    into one workgroup per CU slot with RANK-AWARE shares (unequal chunks per strip, lanczos_march.hpp: march_build_table).
    Every frame of the batch is the same picture, so every frame must equal frame 0 -- any gap or overlap in the partition
    shows -- and frame 0 must carry the reference's known-answer digest in EXACT mode / stay within 1 LSB
    of it in the default mode."""
    iw, ih, c, sn, sd, a, frames = shape
    with open(os.path.join(GOLD, "kat_digests.json")) as f:
        kat = json.load(f)
    planar = O.lcg_u8(c * ih * iw, 12345).reshape(c, ih, iw)
    img = np.ascontiguousarray(planar.transpose(1, 2, 0))
    batch = np.ascontiguousarray(np.broadcast_to(img, (frames,) + img.shape))
    exact = ctx.resample(batch, sn, sd, a, L.MODE_EXACT)
    dig = O.fnv1a64(np.ascontiguousarray(exact[0].transpose(2, 0, 1)))
    assert f"{dig:016x}" == kat["survey_8c"][f"{iw}x{ih}_{iw * sn // sd}x{ih * sn // sd}_{sn}-{sd}_a{a}_c{c}"]
    for i in range(1, frames):
        assert np.array_equal(exact[i], exact[0]), f"EXACT: frame {i} of {frames} differs from frame 0"
    fast = ctx.resample(batch, sn, sd, a, L.MODE_LSB1)
    _cmp(fast[0], exact[0], L.MODE_LSB1, f"batch of {frames}, frame 0", _req(ctx, img, sn, sd, a))
    for i in range(1, frames):
        assert np.array_equal(fast[i], fast[0]), f"LSB1: frame {i} of {frames} differs from frame 0"


# ---------------------------------------------------------------------------------------------------------------
# BASELINE config 5 at FULL size: 3840x2160x4 uint16 -> 7680x4320, a = 4.  PARITY UNPINNED BY THE REFERENCE (it has no
# 16-bit path, full_TB.h:18,30): the checker is the restatement templated on the sample type (clamp 65535).

C5 = (3840, 2160, 4, 2, 1, 4)


def _c5_frame():
    w, h, c = C5[:3]
    return O.lcg_u16(h * w * c, 12345).reshape(h, w, c)


def test_full_size_config5_digest(ctx):
    """EXACT mode at full size against the committed FNV-1a-64 of the u16 restatement's output
    (tests/golden/make_golden_u16.py) -- no CPU resample on the box."""
    with open(os.path.join(GOLD, "kat_digests_u16.json")) as f:
        kat = json.load(f)["digests"]
    w, h, c, sn, sd, a = C5
    got = ctx.resample(_c5_frame(), sn, sd, a, L.MODE_EXACT)
    assert got.shape == (h * 2, w * 2, c) and got.dtype == np.uint16
    assert ctx.last_kernel() == L.KERNEL_FAST
    assert f"{O.fnv1a64(got):016x}" == kat["3840x2160_7680x4320_2-1_a4_c4"]
    for shape in ("480x270_960x540_2-1_a4_c4", "320x180_640x360_2-1_a3_c3", "150x100_200x133_4-3_a3_c3"):
        iw, ih, ow, oh, sn2, sd2, a2, c2 = _parse(shape)
        img = O.lcg_u16(ih * iw * c2, 12345).reshape(ih, iw, c2)
        got = ctx.resample(img, sn2, sd2, a2, L.MODE_EXACT)
        assert f"{O.fnv1a64(got):016x}" == kat[shape], shape


def test_full_size_config5_batch_every_frame(ctx):
    """Config 5 as a batch of 4 identical frames (PARITY UNPINNED BY THE REFERENCE, as above): the host entry sends them out as two
    launches of two frames, and this launch shape (120 (strip, frame) pairs, two 8-wave workgroups per CU: no rank-aware
    shares) takes the marching kernel's table mode A -- one workgroup per CU slot, shares that run from one pair into the next
    (lanczos_march.hpp: march_build_table) -- which the reported table must confirm in both modes.  Every frame must equal
    frame 0 and frame 0 the committed digest."""
    import march_table_cfg as M
    with open(os.path.join(GOLD, "kat_digests_u16.json")) as f:
        kat = json.load(f)["digests"]
    w, h, c, sn, sd, a = C5
    frame = _c5_frame()
    batch = np.ascontiguousarray(np.broadcast_to(frame, (4,) + frame.shape))
    def mode_a(tag):
        info, tab = ctx.last_march_table()
        assert info.mode == L.MARCH_TABLE_A and info.workgroups == info.wg_per_cu * info.cus, f"{tag}: {info}"
        assert not M.partition_errors(info, tab), f"{tag}: {M.partition_errors(info, tab)}"
        sm = M.summary(info, tab)
        assert sm["strip_changes"] >= 1, f"{tag}: no share runs from one strip into the next: {M.describe(info, tab)}"
    got = ctx.resample(batch, sn, sd, a, L.MODE_EXACT)
    mode_a("EXACT")
    assert f"{O.fnv1a64(got[0]):016x}" == kat["3840x2160_7680x4320_2-1_a4_c4"]
    for i in range(1, 4):
        assert np.array_equal(got[i], got[0]), f"EXACT: frame {i} differs from frame 0"
    fast = ctx.resample(batch, sn, sd, a, L.MODE_LSB1)
    mode_a("LSB1")
    _cmp(fast[0], got[0], L.MODE_LSB1, "config 5 batch, frame 0", _req(ctx, frame, sn, sd, a))
    for i in range(1, 4):
        assert np.array_equal(fast[i], fast[0]), f"LSB1: frame {i} differs from frame 0"


def test_full_size_config5_against_oracle(ctx):
    """Both parity modes at full size, every sample against the threaded checker; gradient-like u16 content
    (the LCG noise frame is covered by the digest test)."""
    w, h, c, sn, sd, a = C5
    y, x = np.mgrid[0:h, 0:w]
    base = ((x * 65535 // w + y * 65535 // h) // 2).astype(np.int64)
    nz = (O.lcg_u16(h * w * c, 99).reshape(h, w, c) >> 6).astype(np.int64)
    img = np.clip(base[..., None] + nz, 0, 65535).astype(np.uint16)
    want = _oracle(img, sn, sd, a, threads=min(os.cpu_count() or 8, 64))
    for mode in (L.MODE_EXACT, L.MODE_LSB1):
        got = ctx.resample(img, sn, sd, a, mode)
        _cmp(got, want, mode, "full-size config 5", _req(ctx, img, sn, sd, a))
        assert ctx.last_kernel() == L.KERNEL_FAST


def test_full_size_config5_as_8_row_strips(ctx):
    """Config 5's tile sharding on one GPU: the frame as 8 output row strips of 540 rows, each from its input rows +
    halo (lanczos_strip_input_rows), through the DEVICE path each rank of bench.py --shard strips uses; the strips
    reassemble to the whole-frame result, bit for bit, in both modes."""
    import torch
    w, h, c, sn, sd, a = C5
    img = _c5_frame()
    x = torch.from_numpy(img.view(np.int16)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for mode in (L.MODE_EXACT, L.MODE_LSB1):
        full = L.make_desc(w, h, c, sn, sd, a, 2, mode)
        y_whole = torch.zeros((full.out_h, full.out_w, c), dtype=torch.int16, device="cuda")
        ctx.resample_device(full, x.data_ptr(), y_whole.data_ptr(), 1, 0, 0, stream)
        y_strips = torch.zeros_like(y_whole)
        for i in range(8):
            d = L.make_desc(w, h, c, sn, sd, a, 2, mode, out_row0=540 * i, out_rows=540)
            r0, n = L.strip_input_rows(d, d.out_row0, d.out_rows)
            assert r0 == max(0, 270 * i - 3) and r0 + n - 1 == min(h - 1, 270 * i + 269 + 4)
            xin = x[r0:r0 + n].contiguous()
            yout = torch.zeros((540, full.out_w, c), dtype=torch.int16, device="cuda")
            ctx.resample_device(d, xin.data_ptr(), yout.data_ptr(), 1, 0, 0, stream)
            y_strips[540 * i:540 * (i + 1)] = yout
        torch.cuda.synchronize()
        assert torch.equal(y_strips, y_whole), f"mode {mode}: strips differ from the whole frame"
        if mode == L.MODE_LSB1:   # (EXACT: the digest test pins the whole-frame bytes)
            whole = y_whole.cpu().numpy().view(np.uint16)
            LC.check(img, sn, sd, a, whole, L.KERNEL_FAST, "config 5 as 8 row strips, LSB1", threads=16)


def test_full_size_config3_against_oracle(ctx):
    """BASELINE config 3 (1280x720 -> 3840x2160, 3x) at full size, gradient content, both modes."""
    img = P.gradient_noise(720, 1280, 3)
    want = _oracle(img, 3, 1, 3, threads=32)
    for mode in (L.MODE_LSB1, L.MODE_EXACT):
        got = ctx.resample(img, 3, 1, 3, mode)
        _cmp(got, want, mode, "full-size config 3", _req(ctx, img, 3, 1, 3))


def test_device_path_is_ordered_behind_the_default_stream(ctx):
    """lanczos_resample_device(stream=NULL) runs on the default stream: frames produced there by asynchronous
    device work (a slow generator, as bench.py's does) must be complete before the resample reads them."""
    import torch
    dev = torch.device("cuda", 0)
    d = L.make_desc(960, 540, 3, 2, 1, 3)
    cfg = O.cfg(960, 540, d.out_w, d.out_h, 3, 3, 2, 1)
    for rep in range(3):
        yy = torch.arange(540, device=dev).view(1, 540, 1, 1) // 16
        xx = torch.arange(960, device=dev).view(1, 1, 960, 1) // 16
        cc = torch.arange(3, device=dev).view(1, 1, 1, 3)
        ff = torch.arange(8, device=dev).view(8, 1, 1, 1)
        x = (((yy + xx + cc + ff + rep) % 5) * 60).to(torch.uint8).contiguous()   # big int64 temporaries: slow
        y = torch.zeros((8, d.out_h, d.out_w, 3), device=dev, dtype=torch.uint8)
        ctx.resample_device(d, x.data_ptr(), y.data_ptr(), 8, 0, 0, None)
        torch.cuda.synchronize()
        for f in (0, 7):
            want = O.expected_hwc_u8(cfg, x[f].cpu().numpy(), 8)
            _cmp(y[f].cpu().numpy(), want, L.MODE_LSB1, f"default-stream ordering rep {rep} frame {f}",
                 _req(ctx, x[f].cpu().numpy(), 2, 1, 3))


def test_host_path_pipeline_with_pinned_buffers(ctx):
    """lanczos_resample_host pushes groups of frames through copy-in / resample / copy-out streams; with
    page-locked buffers (lanczos_host_alloc) the copies overlap.  Results must not depend on the grouping."""
    n = 9   # -> groups of 4, 4, 1
    pin_in = L.PinnedArray((n, 120, 208, 3), np.uint8)
    pin_out = L.PinnedArray((n, 240, 416, 3), np.uint8)
    for i in range(n):
        pin_in.array[i] = P.noise(120, 208, 3, seed=300 + i)
    got = ctx.resample(pin_in.array, 2, 1, 3, L.MODE_EXACT, out=pin_out.array)
    for i in range(n):
        assert np.array_equal(got[i], _oracle(pin_in.array[i], 2, 1, 3)), i
    pageable = ctx.resample(np.array(pin_in.array), 2, 1, 3, L.MODE_EXACT)
    assert np.array_equal(pageable, got)
    pin_in.close()
    pin_out.close()


# ---------------------------------------------------------------------------------------------------------------
# planar frames: the reference's img_in[C][H][W] / img_out_ex[C][OUT_H][OUT_W] arrays (full_TB.h:20-21) on the device


@pytest.mark.parametrize("w,h,c,dtype", [(64, 8, 3, np.uint8), (67, 5, 3, np.uint8), (130, 9, 4, np.uint8),
                                          (33, 7, 1, np.uint8), (62, 4, 3, np.uint16), (65, 3, 4, np.uint16),
                                          (1920, 16, 3, np.uint8)])
def test_planar_interleaved_conversions_match_numpy(ctx, w, h, c, dtype):
    """full_TB.h:127-138 / 146-165 on the device: bit-exact against numpy transposes, ragged widths included."""
    import torch
    frames = 3
    rng = np.random.default_rng(w * 131 + h)
    planar = rng.integers(0, np.iinfo(dtype).max + 1, size=(frames, c, h, w)).astype(dtype)
    tdt = torch.uint8 if dtype == np.uint8 else torch.int16
    d_pl = torch.from_numpy(planar.view(np.uint8 if dtype == np.uint8 else np.int16)).cuda()
    d_il = torch.zeros((frames, h, w, c), dtype=tdt, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.planar_to_interleaved_device(d_pl.data_ptr(), d_il.data_ptr(), w, h, c, planar.itemsize, frames, stream)
    torch.cuda.synchronize()
    got = d_il.cpu().numpy().view(dtype)
    assert np.array_equal(got, planar.transpose(0, 2, 3, 1))
    d_back = torch.zeros_like(d_pl)
    ctx.interleaved_to_planar_device(d_il.data_ptr(), d_back.data_ptr(), w, h, c, planar.itemsize, frames, stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_back.cpu().numpy().view(dtype), planar)


def test_planar_resample_matches_the_reference_digests(ctx):
    """lanczos_resample_planar_device on the LCG frames of SURVEY.md 8(c): the FNV-1a-64 of the PLANAR device result is
    the reference's digest -- no host-side layout change anywhere."""
    import torch
    with open(os.path.join(GOLD, "kat_digests.json")) as f:
        kat = json.load(f)
    for shape in ("1920x1080_3840x2160_2-1_a3_c3", "480x270_960x540_2-1_a4_c4", "300x200_400x266_4-3_a3_c3"):
        iw, ih, ow, oh, sn, sd, a, c = _parse(shape)
        planar = O.lcg_u8(c * ih * iw, 12345).reshape(1, c, ih, iw)
        d = L.make_desc(iw, ih, c, sn, sd, a, 1, L.MODE_EXACT)
        d_in = torch.from_numpy(planar).cuda()
        d_out = torch.zeros((1, c, oh, ow), dtype=torch.uint8, device="cuda")
        ctx.resample_planar_device(d, d_in.data_ptr(), d_out.data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        dig = O.fnv1a64(d_out.cpu().numpy())
        assert f"{dig:016x}" == kat["survey_8c"][shape], shape


def test_planar_call_shape_errors(ctx):
    import torch
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    with pytest.raises(L.LanczosError) as e:
        ctx.planar_to_interleaved_device(buf.data_ptr(), buf.data_ptr(), 16, 16, 2, 1, 1)   # channels = 2
    assert e.value.code == L.ERR_BAD_ARG
    with pytest.raises(L.LanczosError) as e:
        ctx.interleaved_to_planar_device(0, buf.data_ptr(), 16, 16, 3, 1, 1)               # null pointer
    assert e.value.code == L.ERR_BAD_ARG
    d = L.make_desc(64, 64, 3, 2, 1, 3, 1, L.MODE_LSB1)
    d.out_row0, d.out_rows = 16, 32                                                        # strips: not for planar
    with pytest.raises(L.LanczosError) as e:
        ctx.resample_planar_device(d, buf.data_ptr(), buf.data_ptr(), 1)
    assert e.value.code == L.ERR_UNSUPPORTED


@pytest.mark.parametrize("pad_in,pad_out", [(0, 0), (4096, 8192), (48, 80), (20, 12)])
def test_frame_strides_and_kernel_families(ctx, pad_in, pad_out):
    """Frames that are not tightly packed (in/out frame strides): 16-byte multiples keep the marching kernel, other
    strides fall back to the tile kernel -- same results either way, and the padding stays untouched."""
    import torch
    w, h, c, sn, a, frames = 208, 96, 3, 2, 3, 5
    d = L.make_desc(w, h, c, sn, 1, a, 1, L.MODE_EXACT)
    imgs = [P.gradient_noise(h, w, c, seed=70 + f) for f in range(frames)]
    cfg = O.cfg(w, h, d.out_w, d.out_h, c, a, sn, 1)
    want = [O.expected_hwc_u8(cfg, im) for im in imgs]
    in_fb, out_fb = w * h * c, d.out_w * d.out_h * c
    in_stride, out_stride = in_fb + pad_in, out_fb + pad_out
    host_in = np.full(frames * in_stride, 0xA5, dtype=np.uint8)
    for f in range(frames):
        host_in[f * in_stride:f * in_stride + in_fb] = imgs[f].reshape(-1)
    d_in = torch.from_numpy(host_in).cuda()
    d_out = torch.full((frames * out_stride,), 0x5A, dtype=torch.uint8, device="cuda")
    for mode in (L.MODE_EXACT, L.MODE_LSB1):
        d.mode = mode
        d_out.fill_(0x5A)
        ctx.resample_device(d, d_in.data_ptr(), d_out.data_ptr(), frames, in_stride, out_stride,
                            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        r = ctx.last_route()   # five frames: the prefix rows ride on k_march, k_prefix runs behind the tile kernel
        assert (r.main, r.prefix) == ((L.ROUTE_MAIN_MARCH, L.ROUTE_PREFIX_RIDING) if in_stride % 16 == 0 else
                                      (L.ROUTE_MAIN_TILE, L.ROUTE_PREFIX_BEHIND)), (pad_in, pad_out, str(r))
        got = d_out.cpu().numpy()
        for f in range(frames):
            g = got[f * out_stride:f * out_stride + out_fb].reshape(d.out_h, d.out_w, c)
            _cmp(g, want[f], mode, f"frame {f} pads {pad_in}/{pad_out}", _req(ctx, imgs[f], sn, 1, a))
            assert np.all(got[f * out_stride + out_fb:(f + 1) * out_stride] == 0x5A), "padding between frames was written"


def test_prefix_rows_ride_or_run_separately(ctx):
    """The in-place prefix rows (output rows < K) either ride on the marching launch (small batches) or run as the
    separate k_prefix launch (more than about one prefix workgroup per CU): both must give the reference's rows."""
    import torch
    w, h, c, sn, a = 208, 96, 3, 2, 3
    img = P.gradient_noise(h, w, c, seed=5)
    cfg = O.cfg(w, h, w * sn, h * sn, c, a, sn, 1)
    want = O.expected_hwc_u8(cfg, img)
    d = L.make_desc(w, h, c, sn, 1, a, 1, L.MODE_EXACT)
    k = L._lib().lanczos_inplace_rows(__import__("ctypes").byref(d))
    assert k >= 1
    for frames in (1, 7, 96):   # 96 frames x 4 prefix workgroups each > 256 CUs: the separate launch
        x = torch.from_numpy(np.repeat(img[None], frames, axis=0)).cuda()
        y = torch.zeros((frames, h * sn, w * sn, c), dtype=torch.uint8, device="cuda")
        for mode in (L.MODE_EXACT, L.MODE_LSB1):
            d.mode = mode
            y.zero_()
            ctx.resample_device(d, x.data_ptr(), y.data_ptr(), frames, 0, 0, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            r = ctx.last_route()
            assert (r.main, r.prefix, r.launches) == (L.ROUTE_MAIN_MARCH, L.ROUTE_PREFIX_FRONT if frames == 96 else L.ROUTE_PREFIX_RIDING, 1), \
                (frames, str(r))
            got = y.cpu().numpy()
            for f in (0, frames // 2, frames - 1):
                _cmp(got[f], want, mode, f"{frames} frames, frame {f}", _req(ctx, img, sn, 1, a))
                assert np.array_equal(got[f][:k], want[:k])      # the prefix kernels are f64 in every mode


def test_first_use_of_a_shape_inside_stream_capture():
    """The entry points are asynchronous on the caller's stream from the FIRST call of a shape on: the tap tables and the workgroup
    table go up with hipMemcpyAsync from page-locked blocks on that stream (no blocking copy, no device-wide wait), so the first
    call can be captured into a graph (relaxed capture mode: the call allocates) and replayed -- round-3 verdict, item 6."""
    import torch
    c = L.Context(0)
    try:
        img = P.gradient_noise(72, 112, 3, seed=5)            # (72 x 112: a shape no other test of this module uses)
        img2 = P.noise(72, 112, 3, seed=6)
        x = torch.from_numpy(img).cuda()
        y = torch.zeros((144, 224, 3), dtype=torch.uint8, device="cuda")
        for mode in (L.MODE_EXACT, L.MODE_LSB1):
            d = L.make_desc(112, 72, 3, 2, 1, 3, 1, mode)
            if mode == L.MODE_LSB1:
                d = L.make_desc(112, 72, 3, 2, 1, 2, 1, mode)  # a = 2: another plan, first used under capture as well
            want = _oracle(img, 2, 1, d.a)
            y.zero_()
            x.copy_(torch.from_numpy(img))
            s = torch.cuda.Stream()
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
                c.resample_device(d, x.data_ptr(), y.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert int(y.max()) == 0                          # captured, not run
            g.replay()
            torch.cuda.synchronize()
            _cmp(y.cpu().numpy(), want, mode, f"graph replay, mode {mode}", (img, 2, 1, d.a, c.last_kernel()))
            x.copy_(torch.from_numpy(img2))                   # the graph holds pointers, not data
            g.replay()
            torch.cuda.synchronize()
            _cmp(y.cpu().numpy(), _oracle(img2, 2, 1, d.a), mode, f"second replay, mode {mode}", (img2, 2, 1, d.a, c.last_kernel()))
            # and the plan / table the capture created serve an ordinary call afterwards
            y.zero_()
            c.resample_device(d, x.data_ptr(), y.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            _cmp(y.cpu().numpy(), _oracle(img2, 2, 1, d.a), mode, f"plain call after capture, mode {mode}", _req(c, img2, 2, 1, d.a))
            del g
    finally:
        c.close()


def test_planar_scratch_grows_after_capture():
    """lanczos_resample_planar_device captured at 32 x 16, then called eagerly at 64 x 48: both interleaved scratch frames of the
    context grow, and the blocks the graph names must stay (kept, not freed) -- the replay still gives the oracle's frame."""
    import torch
    c = L.Context(0)
    try:
        small, big = P.gradient_noise(16, 32, 1, seed=21), P.noise(48, 64, 1, seed=22)   # HWC with one channel: planar as it lies
        ds, db = L.make_desc(32, 16, 1, 2, 1, 3, 1, L.MODE_EXACT), L.make_desc(64, 48, 1, 2, 1, 3, 1, L.MODE_EXACT)
        xs, xb = torch.from_numpy(small).cuda(), torch.from_numpy(big).cuda()
        ys = torch.zeros((32, 64, 1), dtype=torch.uint8, device="cuda")
        yb = torch.zeros((96, 128, 1), dtype=torch.uint8, device="cuda")
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            c.resample_planar_device(ds, xs.data_ptr(), ys.data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert int(ys.max()) == 0                             # captured, not run
        c.resample_planar_device(db, xb.data_ptr(), yb.data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _cmp(yb.cpu().numpy(), _oracle(big, 2, 1, 3), L.MODE_EXACT, "eager call at the larger size")
        g.replay()
        torch.cuda.synchronize()
        _cmp(ys.cpu().numpy(), _oracle(small, 2, 1, 3), L.MODE_EXACT, "replay after the scratch frames grew")
        del g
    finally:
        c.close()


@pytest.mark.parametrize("mode", [L.MODE_EXACT, L.MODE_LSB1])
@pytest.mark.parametrize("sn,sd", [(2, 1), (3, 2)])
def test_first_use_inside_capture_then_eager_before_replay(sn, sd, mode):
    """The tap tables and the workgroup table of a shape first used inside stream capture are valid at once (they go up
    eagerly on a private stream; a copy queued on the capturing stream would run only at a replay): an eager call BEFORE any
    replay gives the right samples, the graph replays afterwards, also after an eager call of another shape, and a graph
    that is dropped without ever being replayed leaves a usable plan behind.  2/1 is served by k_march, 3/2 by k_ratp."""
    import torch
    c = L.Context(0)
    try:
        w, h, a = 128, 76 + 2 * mode + sd, 3                 # shapes no other test of this module uses; 16-byte rows: k_march
        img, img2 = P.gradient_noise(h, w, 3, seed=15), P.noise(h, w, 3, seed=16)
        d = L.make_desc(w, h, 3, sn, sd, a, 1, mode)
        x = torch.from_numpy(img).cuda()
        y = torch.zeros((d.out_h, d.out_w, 3), dtype=torch.uint8, device="cuda")
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            c.resample_device(d, x.data_ptr(), y.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert int(y.max()) == 0                              # captured, not run
        y2 = torch.zeros_like(y)
        c.resample_device(d, x.data_ptr(), y2.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert c.last_kernel() == L.KERNEL_FAST
        r = c.last_route()
        assert (r.main, r.prefix) == ((L.ROUTE_MAIN_MARCH, L.ROUTE_PREFIX_RIDING) if sd == 1 else (L.ROUTE_MAIN_RATP, L.ROUTE_PREFIX_BEHIND)), str(r)
        _cmp(y2.cpu().numpy(), _oracle(img, sn, sd, a), mode, "eager call before any replay", _req(c, img, sn, sd, a))
        assert int(y.max()) == 0
        x.copy_(torch.from_numpy(img2))
        g.replay()
        torch.cuda.synchronize()
        _cmp(y.cpu().numpy(), _oracle(img2, sn, sd, a), mode, "replay", _req(c, img2, sn, sd, a))
        other = P.noise(50, 88, 3, seed=17)                   # another shape, eagerly
        _cmp(c.resample(other, sn, sd, a, mode), _oracle(other, sn, sd, a), mode, "other shape", _req(c, other, sn, sd, a))
        x.copy_(torch.from_numpy(img))
        y.zero_()
        g.replay()
        torch.cuda.synchronize()
        _cmp(y.cpu().numpy(), _oracle(img, sn, sd, a), mode, "replay after other work", _req(c, img, sn, sd, a))
        del g
        # a graph that is never replayed
        img3 = P.gradient_noise(h + 2, w, 3, seed=18)
        d3 = L.make_desc(w, h + 2, 3, sn, sd, a, 1, mode)
        x3 = torch.from_numpy(img3).cuda()
        y3 = torch.zeros((d3.out_h, d3.out_w, 3), dtype=torch.uint8, device="cuda")
        g3 = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g3, stream=s, capture_error_mode="relaxed"):
            c.resample_device(d3, x3.data_ptr(), y3.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        del g3
        c.resample_device(d3, x3.data_ptr(), y3.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _cmp(y3.cpu().numpy(), _oracle(img3, sn, sd, a), mode, "eager call after a dropped graph", _req(c, img3, sn, sd, a))
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------
# The LSB1 contract at full size (tests/lsb1_check.py), with coverage asserted: the window population (samples whose reference
# sum lies within delta of a store boundary: where the biased floor decides) and the integer-phase flips of the H pass (where
# the fix-up lists decide) must be clearly non-zero, so that the check was exercised and not passed over.


def _c5_gradient():
    w, h, c = C5[:3]
    y, x = np.mgrid[0:h, 0:w]
    base = ((x * 65535 // w + y * 65535 // h) // 2).astype(np.int64)
    nz = (O.lcg_u16(h * w * c, 99).reshape(h, w, c) >> 6).astype(np.int64)
    return np.clip(base[..., None] + nz, 0, 65535).astype(np.uint16)


FULL_LSB1 = {
    "config2": ((1920, 1080, 3, 2, 3), {"noise": lambda: P.noise(1080, 1920, 3, seed=1), "dark": lambda: P.dark_noise(1080, 1920, 3),
                                        "gradient": lambda: P.gradient_noise(1080, 1920, 3)}),
    "config3": ((1280, 720, 3, 3, 3), {"noise": lambda: P.noise(720, 1280, 3, seed=1), "dark": lambda: P.dark_noise(720, 1280, 3),
                                       "gradient": lambda: P.gradient_noise(720, 1280, 3)}),
    "config5": ((3840, 2160, 4, 2, 4), {"noise": _c5_frame, "gradient": _c5_gradient}),
}


@pytest.mark.parametrize("config,pattern", [(k, p) for k, (_, gens) in FULL_LSB1.items() for p in gens])
def test_full_size_lsb1_contract(ctx, config, pattern):
    (w, h, c, s, a), gens = FULL_LSB1[config]
    img = gens[pattern]()
    got = ctx.resample(img, s, 1, a, L.MODE_LSB1)
    assert ctx.last_kernel() == L.KERNEL_FAST
    r = LC.check(img, s, 1, a, got, L.KERNEL_FAST, f"{config} {pattern} LSB1")
    print(f"{config} {pattern}: +1 fraction {r['plus1_fraction']:.3e} ({r['plus1']} of {r['samples']}), window {r['window']}, "
          f"integer-phase flips {r['int_flips']}, integer-row samples {r['int_row_samples']}, largest +1 gap "
          f"{r['max_plus1_gap']:.3g} (delta {r['delta']:g})")
    assert r["window"] >= 1000 and r["int_row_samples"] >= w * c * 100
    if pattern != "gradient":
        assert r["int_flips"] >= 100


def _run_switch_child(tmp_path, name, env_extra):
    import subprocess
    import sys
    out = str(tmp_path / f"{name}.npz")
    env = dict(os.environ)
    for k in ("LANCZOS_TILE_KERNEL", "LANCZOS_NO_RATP", "LANCZOS_SEPARATE_PREFIX", "LANCZOS_MARCH_SEGS", "LANCZOS_MARCH_WGS",
              "LANCZOS_RANK_WEIGHTS"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "lsb1_env_child.py"), out], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    return np.load(out)


def test_production_switches_change_no_result(tmp_path):
    """none of the production switches changes a result.  Each in a fresh child process (the environment is
    read once per process), one at a time: EXACT identical to the reference, LSB1 within its contract, and the switches that
    only re-partition the work give LSB1 bytes identical to the default run.  The workgroup table every run reports for the
    config 2 batch partitions its launch and has the shape the switch asks for.  The two 1080p frames go out as two launches of
    one frame, 15 (strip, frame) pairs each: mode A needs 64 pairs, so LANCZOS_MARCH_SEGS=1 cannot reach it here and every run
    reports mode B (tests/test_march_table_gpu.py forces mode A on batches that admit it)."""
    import lsb1_env_child as E
    import march_table_cfg as M
    reqs = {name: (gen(), sn, sd, a) for name, (gen, sn, sd, a) in E.SWITCH_REQUESTS.items()}
    want = {name: [_oracle(f, sn, sd, a, threads=16) for f in frames] for name, (frames, sn, sd, a) in reqs.items()}
    base = _run_switch_child(tmp_path, "default", {})
    partition_only = {"LANCZOS_SEPARATE_PREFIX", "LANCZOS_MARCH_SEGS", "LANCZOS_MARCH_WGS", "LANCZOS_RANK_WEIGHTS"}
    for var, val in [("LANCZOS_TILE_KERNEL", "1"), ("LANCZOS_NO_RATP", "1"), ("LANCZOS_SEPARATE_PREFIX", "1"),
                     ("LANCZOS_MARCH_SEGS", "0"), ("LANCZOS_MARCH_SEGS", "1"), ("LANCZOS_MARCH_WGS", "7"),
                     ("LANCZOS_RANK_WEIGHTS", "0"), (None, None)]:
        res = base if var is None else _run_switch_child(tmp_path, f"{var}_{val}", {var: val})
        tag = "default" if var is None else f"{var}={val}"
        for name, (frames, sn, sd, a) in reqs.items():
            exact, lsb1 = res[f"{name}:exact"], res[f"{name}:lsb1"]
            fam = int(res[f"{name}:lsb1:kernel"])
            for mtag in ("exact", "lsb1"):   # what each switch changed, and nothing else
                main, prefix = (int(v) for v in res[f"{name}:{mtag}:route"][:2])
                want_route = {"config2_batch": (L.ROUTE_MAIN_MARCH, L.ROUTE_PREFIX_RIDING), "rational_3_2": (L.ROUTE_MAIN_RATP, L.ROUTE_PREFIX_BEHIND),
                              "deep_prefix_33_32": (L.ROUTE_MAIN_RAT, L.ROUTE_PREFIX_BEHIND)}[name]
                if var == "LANCZOS_TILE_KERNEL" and name == "config2_batch":
                    want_route = (L.ROUTE_MAIN_TILE, L.ROUTE_PREFIX_BEHIND)
                if var == "LANCZOS_NO_RATP" and name == "rational_3_2":
                    want_route = (L.ROUTE_MAIN_RAT, L.ROUTE_PREFIX_BEHIND)
                if var == "LANCZOS_SEPARATE_PREFIX" and name == "config2_batch":
                    want_route = (L.ROUTE_MAIN_MARCH, L.ROUTE_PREFIX_BEHIND)
                assert (main, prefix) == want_route, f"{tag} {name} {mtag}: route {main}+{prefix}, expected {want_route}"
                info, tab = M.Info(*(int(v) for v in res[f"{name}:{mtag}:table_info"])), res[f"{name}:{mtag}:table"]
                if main != L.ROUTE_MAIN_MARCH:
                    assert tuple(info) == (0,) * 10 and tab.size == 0, f"{tag} {name} {mtag}: a table reported without k_march: {info}"
                    continue
                assert not M.partition_errors(info, tab), f"{tag} {name} {mtag}: {M.partition_errors(info, tab)}"
                assert (info.mode, info.segs, info.strips, info.frames, info.m_lo, info.m_hi) == (L.MARCH_TABLE_B, 1, 15, 1, 2, 1080), \
                    f"{tag} {name} {mtag}: {M.describe(info, tab)}"
                if tag == "LANCZOS_MARCH_WGS=7":      # seven workgroups for 15 pairs: one chunk per pair
                    assert info.workgroups == 15 and not info.rank_aware, f"{tag} {name} {mtag}: {M.describe(info, tab)}"
                if tag == "LANCZOS_RANK_WEIGHTS=0":
                    assert not info.rank_aware, f"{tag} {name} {mtag}: {M.describe(info, tab)}"
            for i in range(len(frames)):
                _cmp(exact[i], want[name][i], L.MODE_EXACT, f"{tag} {name} frame {i}")
                _cmp(lsb1[i], want[name][i], L.MODE_LSB1, f"{tag} {name} frame {i}", (frames[i], sn, sd, a, fam))
            if var in partition_only:
                assert np.array_equal(lsb1, base[f"{name}:lsb1"]), f"{tag}: {name} LSB1 bytes differ from the default run"
