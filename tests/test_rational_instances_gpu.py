"""Every instance of the two rational-scale kernel families (csrc/lanczos_rational.hpp), launched on purpose, route asserted,
against the CPU oracle.

  k_ratp<T, C, N, D, A, EXACT>   the periodic ratios: the 11 entries of LZ_RATP_CONFIGS x {EXACT, LSB1} = 22 kernels
  k_rat<T, TAPS, EXACT>          every other ratio: {uint8, uint16} x a in {2, 3, 4} x {EXACT, LSB1} = 12 kernels

Every constant of RatPCfg changes with (C, N, D, a, sample size) -- UP, MIS, NVG / TP / TH, the mirrored phases, the D-row slide
of the V window, NW -- so a wrong shift in wsample, a window slot off by one or a wrong mirror index would be specific to one
instance.  The frames of tests/ratp_cfg.py RATP_SHAPES (checked against the header without a GPU by
tests/test_rational_instances.py) give each instance two tiles across, three tile rows, a last tile that ends inside a unit, a
last period cut by the frame, and -- for C = 1 and 3 -- input rows that are no dword multiples (the byte-load branch of LOAD);
the batches below start frames off a dword for C = 4 as well.

No comparison machinery of its own: EXACT is bit-identical to the oracle, LSB1 goes through test_parity_gpu._cmp (+-1 LSB and
the per-sample contract of lsb1_check.check), 16-bit samples use the templated checker (parity unpinned by the reference).
The oracle runs once per (instance, content); all tests of an instance share the result.
"""
import numpy as np
import pytest

import lanczos_hls_amd as L
import patterns as P
import ratp_cfg as R
from test_parity_gpu import _cmp, _oracle, _req

pytestmark = pytest.mark.gpu

RATP, RAT, BEHIND, NONE = L.ROUTE_MAIN_RATP, L.ROUTE_MAIN_RAT, L.ROUTE_PREFIX_BEHIND, L.ROUTE_PREFIX_NONE
MODES = (L.MODE_EXACT, L.MODE_LSB1)
INSTANCES = sorted(R.RATP_INSTANCES)
_ID = lambda i: f"u{8 * i[0]}-c{i[1]}-{i[2]}_{i[3]}-a{i[4]}"
_IDS = [_ID(i) for i in INSTANCES]


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _content(name, h, w, c, sb, seed):
    """noise / dark noise (where the integer-phase vlim / tight exact chains fire) / a 0-max checker (sums below 0 and above
    max: fmed3, cvt_pk_u8_f32 and store_convert all saturate) / all max."""
    dt, mx = (np.uint8, 255) if sb == 1 else (np.uint16, 65535)
    if name == "noise":
        return P.noise(h, w, c, seed=seed, dtype=dt)
    if name == "dark":
        return P.dark_noise(h, w, c, seed=seed) if sb == 1 else (P.noise(h, w, c, seed=seed, dtype=dt) >> 8).astype(dt)
    if name == "checker":
        return np.ascontiguousarray(((np.add.outer(np.arange(h), np.arange(w)) % 2) * mx).astype(dt)[..., None].repeat(c, 2))
    assert name == "max"
    return np.full((h, w, c), mx, dt)


CONTENTS = ("noise", "dark", "checker", "max")
_FRAMES = {}


def _frame(inst, name):
    """(frame, oracle output) of an instance's tall RATP_SHAPES frame with content `name`: computed once, never written to."""
    if (inst, name) not in _FRAMES:
        sb, c, n, d, a = inst
        w, _, h = R.RATP_SHAPES[inst]
        img = _content(name, h, w, c, sb, seed=500 + 7 * INSTANCES.index(inst) + CONTENTS.index(name))
        want = _oracle(img, n, d, a)
        img.setflags(write=False)
        want.setflags(write=False)
        _FRAMES[inst, name] = (img, want)
    return _FRAMES[inst, name]


def _want_route(ctx, main, prefix, what):
    r = ctx.last_route()
    assert ctx.last_kernel() == L.KERNEL_FAST, f"{what}: kernel family {ctx.last_kernel()}"
    assert (r.main, r.prefix, r.launches) == (main, prefix, 1), \
        f"{what}: route {r}, built to reach {L.ROUTE_MAIN_NAMES[main]}+{L.ROUTE_PREFIX_NAMES[prefix]} in one launch"


# ---- 1. every k_ratp instance, both modes, multi-tile ragged frames ----------------------------------------------------------------
@pytest.mark.parametrize("inst", INSTANCES, ids=_IDS)
def test_every_ratp_instance(ctx, inst):
    """k_ratp<T, C, N, D, A, true> (EXACT) and <..., false> (LSB1) of one LZ_RATP_CONFIGS entry on its RATP_SHAPES frame at the
    tall height (2 x 3 or 2 x 4 tiles, partial last unit and period), four contents.  Route: ratp, k_prefix behind it, one
    launch; rows [0, K) bit-identical in both modes (the prefix kernels are f64 in every mode)."""
    sb, c, n, d, a = inst
    w, _, h = R.RATP_SHAPES[inst]
    K = L.inplace_rows(L.make_desc(w, h, c, n, d, a, sb))
    assert K == R.prefix_rows(n, d, a)
    for name in CONTENTS:
        img, want = _frame(inst, name)
        for mode in MODES:
            what = f"{_ID(inst)} {w}x{h} {name} mode {mode}"
            got = ctx.resample(img, n, d, a, mode)
            _want_route(ctx, RATP, BEHIND, what)
            _cmp(got, want, mode, what, _req(ctx, img, n, d, a))
            assert np.array_equal(got[:K], want[:K]), f"{what}: prefix rows [0, {K}) differ from the reference"


# ---- 2. every k_rat instance -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [2, 3, 4])
@pytest.mark.parametrize("dt", [np.uint8, np.uint16], ids=["uint8", "uint16"])
def test_every_rat_instance(ctx, dt, a):
    """k_rat<T, TAPS, EXACT>: the case [dt-a] launches k_rat<dt, 2a, true> (its EXACT calls) and k_rat<dt, 2a, false> (its LSB1
    calls) -- [uint8-2] <uint8_t, 4, *>, [uint8-3] <uint8_t, 6, *>, [uint8-4] <uint8_t, 8, *>, [uint16-2] <uint16_t, 4, *>,
    [uint16-3] <uint16_t, 6, *>, [uint16-4] <uint16_t, 8, *>: all 12.  Two ratios without a k_ratp instance: 5/3 (x = o / SCALE
    rounds, the frame is not periodic) and 7/4 (periodic, but no instance), C = 1, 3, 4, noise and dark noise, on frames of two
    k_rat tiles each way with ragged right and bottom edges (ratp_cfg.rat_frame)."""
    sb = np.dtype(dt).itemsize
    for (sn, sd) in ((5, 3), (7, 4)):
        for c in (1, 3, 4):
            assert (sb, c, sn, sd, a) not in R.RATP_INSTANCES
            w, h = R.rat_frame(c, sb, sn, sd)
            for name in ("noise", "dark"):
                img = _content(name, h, w, c, sb, seed=900 + 10 * sn + c + a)
                want = _oracle(img, sn, sd, a)
                for mode in MODES:
                    what = f"{np.dtype(dt).name} c={c} {sn}/{sd} a={a} {w}x{h} {name} mode {mode}"
                    got = ctx.resample(img, sn, sd, a, mode)
                    _want_route(ctx, RAT, BEHIND, what)
                    _cmp(got, want, mode, what, _req(ctx, img, sn, sd, a))


# ---- 3. strips through every k_ratp instance ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", INSTANCES, ids=_IDS)
def test_strips_through_every_ratp_instance(ctx, inst):
    """The tall frame as row strips cut at ratp_cfg.strip_cuts: no boundary on a tile row (TH) or a period (N), so every strip
    starts inside a tile and inside a period (y_tile, y_first, gr_min / gr_max, in_row0); the first strip starts inside the
    prefix rows and ends at row K or past it, one strip is narrower than a period.  Each strip from the input rows
    lanczos_strip_input_rows names.  A strip that starts at 0 < row < K is refused (ERR_UNSUPPORTED: the prefix recurrence
    needs rows [0, M) in one place), which is asserted; so the only strip that starts inside the prefix rows starts at row 0."""
    sb, c, n, d, a = inst
    w, _, h = R.RATP_SHAPES[inst]
    img, want = _frame(inst, "noise")
    K = R.prefix_rows(n, d, a)
    cuts = R.strip_cuts(inst, want.shape[0])
    for mode in MODES:
        parts = []
        for r0, r1 in zip(cuts, cuts[1:]):
            what = f"{_ID(inst)} strip [{r0}, {r1}) mode {mode} (K = {K})"
            desc = L.make_desc(w, h, c, n, d, a, sb, mode, out_row0=r0, out_rows=r1 - r0)
            i0, rows = L.strip_input_rows(desc, r0, r1 - r0)
            parts.append(ctx.resample_strip(img[i0:i0 + rows], desc))
            if r1 > K:
                _want_route(ctx, RATP, BEHIND if r0 < K else NONE, what)
        got = np.concatenate(parts)
        if mode == L.MODE_EXACT:
            assert np.array_equal(got, want), f"{_ID(inst)}: EXACT strips differ from the whole-frame reference"
        else:
            _cmp(got, want, mode, f"{_ID(inst)} strips, LSB1", (img, n, d, a, L.KERNEL_FAST))
    desc = L.make_desc(w, h, c, n, d, a, sb, L.MODE_EXACT, out_row0=K - 1, out_rows=K + 3)
    i0, rows = L.strip_input_rows(desc, K - 1, K + 3)
    with pytest.raises(L.LanczosError) as e:
        ctx.resample_strip(img[i0:i0 + rows], desc)
    assert e.value.code == L.ERR_UNSUPPORTED and K - 1 > 0


# ---- 4. batches, frame strides, frames that start off a dword ------------------------------------------------------------------------
@pytest.mark.parametrize("inst", INSTANCES, ids=_IDS)
def test_batches_with_strides_off_a_dword(ctx, inst):
    """Three frames of different content through lanczos_resample_device with an input frame stride of the frame + 5 bytes
    (+ 6 for 16-bit samples) and an output frame stride of the frame + 12.  RGBA frames are dword multiples: 8-bit frames 1 and
    2 then start 1 and 2 bytes off a dword, which takes the byte-load branch of LOAD for C = 4 as well; 16-bit: frame 1 starts
    2 bytes off, frame 2 on a dword again.  (C = 1 and 3: the rows are no dword multiples to begin with.)  Both buffers are
    filled with guard bytes first; every frame against the oracle, every pad byte of the output still the guard value."""
    import torch
    sb, c, n, d, a = inst
    w, _, h = R.RATP_SHAPES[inst]
    frames = [_frame(inst, name) for name in ("noise", "dark", "checker")]
    desc = L.make_desc(w, h, c, n, d, a, sb)
    in_fb, out_fb = w * h * c * sb, desc.out_w * desc.out_h * c * sb
    in_stride, out_stride = in_fb + (5 if sb == 1 else 6), out_fb + 12
    host_in = np.full(3 * in_stride, 0xA5, dtype=np.uint8)
    for f, (img, _) in enumerate(frames):
        host_in[f * in_stride:f * in_stride + in_fb] = img.reshape(-1).view(np.uint8)
    d_in = torch.from_numpy(host_in).cuda()
    d_out = torch.empty(3 * out_stride, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 4 == 0 and (c != 4 or in_stride % 4 != 0)
    for mode in MODES:
        desc.mode = mode
        d_out.fill_(0x5A)
        ctx.resample_device(desc, d_in.data_ptr(), d_out.data_ptr(), 3, in_stride, out_stride, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _want_route(ctx, RATP, BEHIND, f"{_ID(inst)} batch mode {mode}")
        got = d_out.cpu().numpy()
        for f, (img, want) in enumerate(frames):
            g = got[f * out_stride:f * out_stride + out_fb].copy().view(want.dtype).reshape(want.shape)
            _cmp(g, want, mode, f"{_ID(inst)} batch frame {f} mode {mode}", _req(ctx, img, n, d, a))
            assert np.all(got[f * out_stride + out_fb:(f + 1) * out_stride] == 0x5A), f"{_ID(inst)}: the padding behind frame {f} was written"


# ---- 5. the hand-over between k_ratp and k_rat -------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", [(1, 3, 4, 3, 3), (1, 4, 3, 2, 3)], ids=_ID)
def test_handover_between_ratp_and_rat(ctx, inst):
    """ratp_prepare wants one axis with out_n > N (a + 2) and in_n > 2a + D + 2.  The largest frame where both axes fail goes
    to k_rat; the smallest where only the width qualifies and the smallest where only the height does go to k_ratp, whose other
    axis then has a few periods only (4/3, a = 3, RGB: 15 x 15, 18 x 15, 15 x 16).  Noise and dark noise, both modes."""
    sb, c, n, d, a = inst
    cases = R.handover_frames(inst)
    if inst == (1, 3, 4, 3, 3):
        assert cases == [(15, 15, False), (18, 15, True), (15, 16, True)]
    for (w, h, periodic) in cases:
        for name in ("noise", "dark"):
            img = _content(name, h, w, c, sb, seed=70 + w + h)
            want = _oracle(img, n, d, a, threads=1)
            for mode in MODES:
                what = f"{_ID(inst)} {w}x{h} {name} mode {mode}"
                got = ctx.resample(img, n, d, a, mode)
                _want_route(ctx, RATP if periodic else RAT, BEHIND, what)
                _cmp(got, want, mode, what, _req(ctx, img, n, d, a))
