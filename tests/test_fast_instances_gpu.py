"""Every instance of the tile-per-workgroup integer-scale kernel (csrc/lanczos_fast.hpp) and both instances of the f64 fallback
(csrc/lanczos_generic.hpp), launched on purpose, route asserted, against the CPU oracle.

  k_fast<T, C, S, A, EXACT>   the 35 entries of LZ_FAST_CONFIGS_G0..G3 x {EXACT, LSB1} = 70 kernels
  k_generic<T>                uint8_t and uint16_t, with k_prefix<T, 2a> behind them

k_fast serves every integer scale whose input rows, base or frame stride are no 16-byte multiples (k_march takes the others).
Every constant of FastCfg changes with (sample size, C, S, a) -- P, TWP_IN, NR, LPB, MIS, NW, WIN_DW0, NGRP, NVT, the v_perm_b32
selectors, the width of the worklist's row field -- so a wrong shift or a window slot off by one would be specific to one
instance and show only where tiles are ragged or where raw and computed bytes meet.  The frames of tests/fast_cfg.py FAST_SHAPES
(checked against the header and the oracle without a GPU by tests/test_fast_instances.py) give each instance two tiles across
with a partial last tile that ends inside a unit, three tile rows with a ragged last one and the middle one's halo rows in the
image; sparse_flips and dense_flips put every tile on the list branch and the middle tile row on the redo-everything branch of
the FIXUP step, with content in which the reference's double chain really lands below v0.

No comparison machinery of its own: EXACT is bit-identical to the oracle, LSB1 goes through test_parity_gpu._cmp (+-1 LSB and
the per-sample contract of lsb1_check.check), rows [0, K) are bit-identical in both modes; 16-bit samples use the templated
checker (parity unpinned by the reference).  The oracle runs once per (instance, width, content); all tests of an instance
share the result, read-only.
"""
import numpy as np
import pytest

import fast_cfg as F
import lanczos_hls_amd as L
from test_parity_gpu import _cmp, _oracle, _req
from test_rational_instances_gpu import _content

pytestmark = pytest.mark.gpu

TILE, GENERIC, BEHIND, NONE = L.ROUTE_MAIN_TILE, L.ROUTE_MAIN_GENERIC, L.ROUTE_PREFIX_BEHIND, L.ROUTE_PREFIX_NONE
MODES = (L.MODE_EXACT, L.MODE_LSB1)
INSTANCES = sorted(F.FAST_INSTANCES)
_IDS = [F.inst_id(i) for i in INSTANCES]
CONTENTS = ("noise", "dark", "checker", "max", "sparse_flips", "dense_flips")
GUARD_IN, GUARD_OUT = 0xA5, 0x5A


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


_FRAMES = {}


def _frame(inst, name, w=None):
    """(frame, oracle output) of an instance's FAST_SHAPES frame (or the same at width w) with content `name`: computed once,
    never written to."""
    sb, c, s, a = inst
    w0, h = F.FAST_SHAPES[inst]
    w = w0 if w is None else w
    if (inst, name, w) not in _FRAMES:
        if name == "sparse_flips":
            img = F.sparse_flips(inst, h, w)
        elif name == "dense_flips":
            img = F.dense_flips(inst, h, w)
        else:
            img = _content(name, h, w, c, sb, seed=1300 + 7 * INSTANCES.index(inst) + CONTENTS.index(name))
        img = np.ascontiguousarray(img)
        want = _oracle(img, s, 1, a)
        img.setflags(write=False)
        want.setflags(write=False)
        _FRAMES[inst, name, w] = (img, want)
    return _FRAMES[inst, name, w]


def _want_route(ctx, main, prefix, what, family=L.KERNEL_FAST):
    r = ctx.last_route()
    assert ctx.last_kernel() == family, f"{what}: kernel family {ctx.last_kernel()}"
    assert (r.main, r.prefix, r.launches) == (main, prefix, 1), \
        f"{what}: route {r}, built to reach {L.ROUTE_MAIN_NAMES[main]}+{L.ROUTE_PREFIX_NAMES[prefix]} in one launch"


def _batch(ctx, desc, frames, in_pad, out_pad, what, main, family, exact_only=False):
    """Frames [(img, want)] through lanczos_resample_device with frame strides of the frame + in_pad / + out_pad bytes, both
    buffers filled with guard bytes first.  Route asserted, every frame compared (bit-identical where exact_only, else by mode),
    every pad byte of the output still the guard value.  desc.mode is set by the caller."""
    import torch
    n = len(frames)
    sb = desc.bytes_per_sample
    in_fb = desc.in_w * desc.in_h * desc.channels * sb
    out_fb = desc.out_w * desc.out_h * desc.channels * sb
    in_stride, out_stride = in_fb + in_pad, out_fb + out_pad
    host_in = np.full(n * in_stride, GUARD_IN, dtype=np.uint8)
    for f, (img, _) in enumerate(frames):
        host_in[f * in_stride:f * in_stride + in_fb] = img.reshape(-1).view(np.uint8)
    d_in = torch.from_numpy(host_in).cuda()
    d_out = torch.full((n * out_stride,), GUARD_OUT, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    ctx.resample_device(desc, d_in.data_ptr(), d_out.data_ptr(), n, in_stride, out_stride, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _want_route(ctx, main, BEHIND, what, family)
    got = d_out.cpu().numpy()
    for f, (img, want) in enumerate(frames):
        g = got[f * out_stride:f * out_stride + out_fb].copy().view(want.dtype).reshape(want.shape)
        _cmp(g, want, L.MODE_EXACT if exact_only else desc.mode, f"{what} frame {f}",
             (img, desc.scale_n, desc.scale_d, desc.a, family))
        assert np.all(got[f * out_stride + out_fb:(f + 1) * out_stride] == GUARD_OUT), f"{what}: the padding behind frame {f} was written"


# ---- 1. every k_fast instance, both modes, six contents ----------------------------------------------------------------------------
@pytest.mark.parametrize("inst", INSTANCES, ids=_IDS)
def test_every_tile_instance(ctx, inst):
    """k_fast<T, C, S, A, true> (EXACT) and <..., false> (LSB1) of one LZ_FAST_CONFIGS entry on its FAST_SHAPES frame (2 x 3
    tiles, partial last unit, ragged last tile row), six contents: noise, dark noise (integer-phase fix-ups everywhere), a 0-max
    checker (sums below 0 and above max: fmed3, cvt_pk_u8_f32 and store_convert all saturate), all max, sparse_flips (every
    tile's worklist short: the list branch of FIXUP, entries in the first and last unit, the first and last LDS row, the last
    column) and dense_flips (the middle tile row's worklist over WL_CAP: every sample of the tile redone exactly).  Route: tile,
    k_prefix behind it, one launch; rows [0, K) bit-identical in both modes (the prefix kernels are f64 in every mode)."""
    sb, c, s, a = inst
    w, h = F.FAST_SHAPES[inst]
    K = L.inplace_rows(L.make_desc(w, h, c, s, 1, a, sb))
    assert K == F.prefix_K(s, a)
    for name in CONTENTS:
        img, want = _frame(inst, name)
        for mode in MODES:
            what = f"{F.inst_id(inst)} {w}x{h} {name} mode {mode}"
            got = ctx.resample(img, s, 1, a, mode)
            _want_route(ctx, TILE, BEHIND, what)
            _cmp(got, want, mode, what, _req(ctx, img, s, 1, a))
            assert np.array_equal(got[:K], want[:K]), f"{what}: prefix rows [0, {K}) differ from the reference"


# ---- 2. strips through every k_fast instance ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("inst", INSTANCES, ids=_IDS)
def test_strips_through_every_tile_instance(ctx, inst):
    """The noise frame and the dense_flips frame as row strips cut at fast_cfg.strip_cuts: no interior boundary on a tile row
    (TH) or an integer phase (S), so every strip but the first starts inside a tile (y_tile < y_begin, y_first, gr_min / gr_max);
    one strip lies inside one tile row, two span two, the last is a single row.  Each strip from the input rows
    lanczos_strip_input_rows names.  Then a strip [0, r) with r <= K through the device entry point into a guarded buffer:
    every tile of k_fast returns early (y_end <= y_first), only k_prefix writes -- the rows are the oracle's and nothing else
    is touched.  A strip that starts at 0 < row < K is refused (ERR_UNSUPPORTED: the prefix recurrence needs rows [0, M) in one
    place), so the only strip that starts inside the prefix rows starts at row 0."""
    import torch
    sb, c, s, a = inst
    w, h = F.FAST_SHAPES[inst]
    K = F.prefix_K(s, a)
    for name in ("noise", "dense_flips"):
        img, want = _frame(inst, name)
        cuts = F.strip_cuts(inst, want.shape[0])
        for mode in MODES:
            parts = []
            for r0, r1 in zip(cuts, cuts[1:]):
                what = f"{F.inst_id(inst)} {name} strip [{r0}, {r1}) mode {mode} (K = {K})"
                desc = L.make_desc(w, h, c, s, 1, a, sb, mode, out_row0=r0, out_rows=r1 - r0)
                i0, rows = L.strip_input_rows(desc, r0, r1 - r0)
                parts.append(ctx.resample_strip(img[i0:i0 + rows], desc))
                _want_route(ctx, TILE, BEHIND if r0 < K else NONE, what)
            got = np.concatenate(parts)
            what = f"{F.inst_id(inst)} {name} strips mode {mode}"
            _cmp(got, want, mode, what, (img, s, 1, a, L.KERNEL_FAST))
            assert np.array_equal(got[:K], want[:K]), f"{what}: prefix rows [0, {K}) differ from the reference"
    # [0, r), r <= K: k_fast launches, every tile returns early, k_prefix writes r rows
    img, want = _frame(inst, "noise")
    r = max(1, K - 1)
    row_b, pad = w * s * c * sb, 256
    for mode in MODES:
        desc = L.make_desc(w, h, c, s, 1, a, sb, mode, out_row0=0, out_rows=r)
        i0, rows = L.strip_input_rows(desc, 0, r)
        assert i0 == 0
        d_in = torch.from_numpy(img[:rows].copy().reshape(-1).view(np.uint8)).cuda()
        d_out = torch.full((pad + r * row_b + pad,), GUARD_OUT, dtype=torch.uint8, device="cuda")
        ctx.resample_device(desc, d_in.data_ptr(), d_out.data_ptr() + pad, 1, 0, 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        what = f"{F.inst_id(inst)} strip [0, {r}) inside the prefix rows (K = {K}) mode {mode}"
        _want_route(ctx, TILE, BEHIND, what)
        got = d_out.cpu().numpy()
        assert np.array_equal(got[pad:pad + r * row_b].view(want.dtype).reshape(r, w * s, c), want[:r]), f"{what}: rows differ from the reference"
        assert np.all(got[:pad] == GUARD_OUT) and np.all(got[pad + r * row_b:] == GUARD_OUT), f"{what}: bytes outside the strip were written"
    assert K - 1 > 0
    desc = L.make_desc(w, h, c, s, 1, a, sb, L.MODE_EXACT, out_row0=K - 1, out_rows=K + 3)
    i0, rows = L.strip_input_rows(desc, K - 1, K + 3)
    with pytest.raises(L.LanczosError) as e:
        ctx.resample_strip(img[i0:i0 + rows], desc)
    assert e.value.code == L.ERR_UNSUPPORTED


# ---- 3. batches, frame strides, frames that start off 16 bytes -----------------------------------------------------------------------
@pytest.mark.parametrize("inst", INSTANCES, ids=_IDS)
def test_batches_with_strides_off_16_bytes(ctx, inst):
    """Three frames (sparse_flips, dense_flips, noise) through lanczos_resample_device with an input frame stride of the frame
    + 5 bytes (+ 6 for 16-bit samples) and an output frame stride of the frame + 12: frames 1 and 2 start 5 and 10 (6 and 12)
    bytes further off a 16-byte boundary than frame 0, so the bytewise branch of the LOAD step runs for C = 4 and for 16-bit
    samples as well.  Then the FAST_SHAPES16 width -- rows that are 16-byte multiples, a 16-byte-aligned base -- with an input
    stride of the frame + 20: frame 0 takes the uint4 load for every interior chunk, frames 1 and 2 the bytewise one, and only
    the stride keeps k_march away, which the route asserts.  Guard bytes in both buffers; every pad byte of the output must
    still be the guard value."""
    sb, c, s, a = inst
    w, h = F.FAST_SHAPES[inst]
    w16 = F.FAST_SHAPES16[inst]
    assert (w * c * sb) % 16 != 0 and (w16 * c * sb) % 16 == 0
    for (width, in_pad) in ((w, 5 if sb == 1 else 6), (w16, 20)):
        frames = [_frame(inst, name, width) for name in ("sparse_flips", "dense_flips", "noise")]
        for mode in MODES:
            desc = L.make_desc(width, h, c, s, 1, a, sb, mode)
            _batch(ctx, desc, frames, in_pad, 12, f"{F.inst_id(inst)} batch of {width}x{h}, in stride + {in_pad}, mode {mode}", TILE, L.KERNEL_FAST)


# ---- 4. k_generic in strips and batches ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.uint8, np.uint16], ids=["uint8", "uint16"])
def test_generic_in_strips_and_batches(ctx, dt):
    """k_generic<T> and k_prefix<T, 2a> behind it: C in {1, 3, 4} x a in {2, 3, 4} at 2/1, 7/5 and 9/8 on frames of two k_generic
    tiles each way, ragged, with more than a tile's rows below K (fast_cfg.generic_frame).  Reached once through
    force_kernel(KERNEL_GENERIC) on a width whose output rows are dword multiples (a plain call would take a fast kernel) and
    once by a plain call on a width whose rows are not (none exists for C = 4, nor for 16-bit samples at 2/1).  Each: whole, in
    three strips (the first ends five rows past K), and as a batch of three frames with input and output frame strides of the
    frame + 5 bytes (+ 6 for 16-bit samples) in guarded buffers.  Bit-identical to the oracle in both modes (f64 throughout);
    route generic, k_prefix behind it for whatever starts at row 0 (M + M2 rows of 32 columns fit the LDS at 9/8 too: never
    the streamed form), no prefix kernel for a strip that starts at or past K.  16-bit: parity unpinned by the reference."""
    sb = np.dtype(dt).itemsize
    try:
        for (sn, sd) in ((2, 1), (7, 5), (9, 8)):
            for c in (1, 3, 4):
                for a in (2, 3, 4):
                    for ragged in (False, True):
                        fr = F.generic_frame(c, sb, sn, sd, a, ragged)
                        if fr is None:
                            assert ragged and (c == 4 or (sb == 2 and sn % 2 == 0))
                            continue
                        w, h = fr
                        ctx.force_kernel(L.KERNEL_NONE if ragged else L.KERNEL_GENERIC)
                        tag = f"{np.dtype(dt).name} c={c} {sn}/{sd} a={a} {w}x{h} {'plain call' if ragged else 'forced'}"
                        frames = []
                        for i, name in enumerate(("noise", "dark", "checker")):
                            img = _content(name, h, w, c, sb, seed=1700 + 10 * sn + 3 * c + a + i)
                            frames.append((img, _oracle(img, sn, sd, a, threads=2)))
                        img, want = frames[0]
                        K = L.inplace_rows(L.make_desc(w, h, c, sn, sd, a, sb))
                        cuts = F.generic_cuts(sn, sd, a, want.shape[0])
                        for mode in MODES:
                            what = f"{tag} mode {mode}"
                            got = ctx.resample(img, sn, sd, a, mode)
                            _want_route(ctx, GENERIC, BEHIND, what, L.KERNEL_GENERIC)
                            _cmp(got, want, L.MODE_EXACT, what)
                            parts = []
                            for r0, r1 in zip(cuts, cuts[1:]):
                                desc = L.make_desc(w, h, c, sn, sd, a, sb, mode, out_row0=r0, out_rows=r1 - r0)
                                i0, rows = L.strip_input_rows(desc, r0, r1 - r0)
                                parts.append(ctx.resample_strip(img[i0:i0 + rows], desc))
                                _want_route(ctx, GENERIC, BEHIND if r0 < K else NONE, f"{what} strip [{r0}, {r1})", L.KERNEL_GENERIC)
                            _cmp(np.concatenate(parts), want, L.MODE_EXACT, f"{what} strips {cuts}")
                            desc = L.make_desc(w, h, c, sn, sd, a, sb, mode)
                            _batch(ctx, desc, frames, 5 if sb == 1 else 6, 5 if sb == 1 else 6, f"{what} batch", GENERIC,
                                   L.KERNEL_GENERIC, exact_only=True)
    finally:
        ctx.force_kernel(L.KERNEL_NONE)
