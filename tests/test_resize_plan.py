"""CPU-only checks of the fused resize kernel's launch plan (lanczos_resize_plan_host, the same function the launch uses).

The invariants are written from the axis tables (lanczos_resize_taps_host, pinned to the numpy model and to Pillow by
tests/test_resize_host.py) and from the march the kernel documents (csrc/lanczos_resize.hip), not from the planner's
formulas:

  * a workgroup owns a strip of SW output columns (256; 64 for four channels) and a chunk of `rows_per_chunk` output rows,
    and marches down the chunk in blocks of 8 rows.  The rows a block's vertical taps read, first[o0] ..
    first[last] + count[last] - 1, live in an LDS ring of `ring_rows` rows, slot = row % ring_rows;
  * input rows are staged `stage_rows` at a time, `stage_dw` dwords each, from the dword that holds the strip's first
    input byte; a thread reads NE + 1 dwords, NE = (K * C + 3) / 4, from dword (align + (first[p] - first[x0]) * C) >> 2 of
    the staged row, align = the byte offset of the strip's first input byte in its dword (0..3);
  * K is the smallest horizontal tap count with an instance that is >= ksize; LDS = ring + staging <= 80 KiB.
"""
import numpy as np
import pytest

import lanczos_hls_amd as L

SWEEP = [1, 2, 3, 5, 7, 16, 17, 40, 97, 160, 333, 1000, 1080, 1920, 3840]   # tests/test_resize_host.py's
BUCKETS = (7, 9, 11, 13, 17, 25)
LDS_MAX = 80 * 1024
OB = 8                       # output rows per march block
BIG = (65535, 32768, 60000, 30000)   # 3 and 4 channels: a frame of 2^31 bytes or more

_TABLES = {}


def tables(in_n, out_n, a):
    """(first, count, ksize) of one axis from the library's host tables."""
    key = (in_n, out_n, a)
    if key not in _TABLES:
        d = L.resize_desc(in_n, 1, out_n, 1, 1, a)
        f, c, k = L.resize_taps_host(d, 0)
        _TABLES[key] = (f.astype(np.int64), c.astype(np.int64), k.shape[1])
    return _TABLES[key]


def strip_width(channels):
    return 64 if channels == 4 else 256


def min_ring_rows(vf, vc, out_h):
    """The most input rows any block of 8 output rows (from row 0) reads."""
    o0 = np.arange(0, out_h, OB)
    last = np.minimum(o0 + OB, out_h) - 1
    return int((vf[last] + vc[last] - vf[o0]).max())


def min_stage_dw(hf, out_w, channels, k):
    """Dwords of a staged row that the widest strip reads at the worst alignment: last index + 1."""
    sw = strip_width(channels)
    ne = (k * channels + 3) // 4
    x0 = np.arange(0, out_w, sw)
    x1 = np.minimum(x0 + sw, out_w) - 1
    return int((((3 + (hf[x1] - hf[x0]) * channels) >> 2) + ne).max()) + 1


def two_pass_reasons(in_w, in_h, out_w, out_h, channels, a):
    """Why the fused kernel cannot run a request (csrc/lanczos_resize.hip), each computed from the request and
    its tables alone: [] means it can."""
    reasons = []
    if in_w == out_w or in_h == out_h:
        return ["axis"]                       # one pass only (or a copy): nothing to fuse, and no table for that axis
    if in_h > 100 * in_w and out_h < in_h:
        reasons.append("order")               # Pillow runs such a frame vertical first: the pass kernels in that order
    if in_w * in_h * channels + 4 >= 2 ** 31 or out_w * out_h * channels >= 2 ** 31:
        reasons.append("bytes")               # 32-bit buffer offsets
    hf, hc, hks = tables(in_w, out_w, a)
    vf, vc, _ = tables(in_h, out_h, a)
    k = next((b for b in BUCKETS if b >= hks), 0)
    if not k:
        reasons.append("bucket")              # no instance with that many horizontal taps
    else:
        ring = min_ring_rows(vf, vc, out_h) * strip_width(channels) * channels
        if ring + 4 * min_stage_dw(hf, out_w, channels, k) * 4 > LDS_MAX:
            reasons.append("lds")             # the ring and the smallest staging (4 rows) do not fit
    return reasons


def check_plan(shape, channels, a, frames):
    """Asserts every invariant of the plan of one request; returns 'fused' or the first reason for two-pass."""
    in_w, in_h, out_w, out_h = shape
    what = (shape, channels, a, frames)
    p = L.resize_plan_host(L.resize_desc(in_w, in_h, out_w, out_h, channels, a), frames)
    reasons = two_pass_reasons(in_w, in_h, out_w, out_h, channels, a)
    if not p.fused:
        assert reasons, what
        assert (p.K, p.strips, p.rows_per_chunk, p.chunks, p.ring_rows, p.stage_rows, p.stage_dw, p.lds_bytes) == (0,) * 8
        return reasons[0]
    assert not reasons or reasons == ["lds"] and p.stage_rows < 4, (what, reasons)
    assert in_w != out_w and in_h != out_h, what
    hf, hc, hks = tables(in_w, out_w, a)
    vf, vc, _ = tables(in_h, out_h, a)
    sw = strip_width(channels)
    assert p.K >= hks and p.K in BUCKETS and not any(hks <= b < p.K for b in BUCKETS), (what, p.K, hks)
    assert (hc <= p.K).all(), what
    assert p.strips == -(-out_w // sw), what
    assert p.lds_bytes == p.ring_rows * sw * channels + p.stage_rows * p.stage_dw * 4, what
    assert p.lds_bytes <= LDS_MAX, what
    # chunks
    rpc = p.rows_per_chunk
    assert rpc > 0 and rpc % OB == 0, (what, rpc)
    assert p.chunks * rpc >= out_h and (p.chunks - 1) * rpc < out_h, (what, rpc, p.chunks)
    # ring: every block of every chunk.  The tables must be monotone for the block's first and last row to bound it.
    assert (np.diff(vf) >= 0).all() and (np.diff(vf + vc) >= 0).all(), what
    for c in range(p.chunks):
        o_end = min((c + 1) * rpc, out_h)
        o0 = np.arange(c * rpc, o_end, OB)
        last = np.minimum(o0 + OB, o_end) - 1
        span = vf[last] + vc[last] - vf[o0]
        assert int(span.max()) <= p.ring_rows, (what, c, int(span.max()), p.ring_rows)
    # staging: every strip, every output column of it, every alignment
    assert (np.diff(hf) >= 0).all(), what
    ne = (p.K * channels + 3) // 4
    x = np.arange(out_w)
    hoffb = (hf - hf[x // sw * sw]) * channels
    for align in range(4):
        last_dw = ((align + hoffb) >> 2) + ne
        assert int(last_dw.max()) < p.stage_dw, (what, align, int(last_dw.max()), p.stage_dw)
    assert p.stage_rows >= 1, what
    assert p.stage_rows * p.stage_dw + 16 * 256 < 2 ** 20, what   # the staging loop's float division is exact below 2^20
    return "fused"


def sweep_shapes():
    """Every (in, out) pair of SWEEP x SWEEP as the horizontal axis and as the vertical axis, each with three partners."""
    pairs = [(i, o) for i in SWEEP for o in SWEEP if i * o <= 4_000_000]
    n = len(pairs)
    shapes = []
    for k, (iw, ow) in enumerate(pairs):
        for step in (1, 71, 149):
            ih, oh = pairs[(k * step + 5 * step) % n]
            shapes.append((iw, ih, ow, oh))
    shapes.append(BIG)
    return shapes


@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("a", [2, 3, 4])
def test_plan_invariants_over_the_sweep(channels, a):
    """661 shapes (every SWEEP x SWEEP pair as the horizontal and as the vertical axis, and one frame of 2^31 bytes or more)
    x frames in {1, 32}: 1322 plans per (channels, a).  How they plan (first reason that holds, in the order axis, order,
    bytes, bucket, lds; `order` is a frame more than 100 times as tall as wide that shrinks in height, which runs the pass
    kernels vertical first as Pillow does -- 1 x 160 .. 3840, 2 x 333 .. 3840, 3 x 333 .. 3840, ... in this sweep):

        C a | fused  axis  order  bytes  bucket  lds
        1 2 |   614   164     80      0     384   80
        1 3 |   582   164     80      0     418   78
        1 4 |   544   164     80      0     464   70
        3 2 |   574   164     80      2     384  118
        3 3 |   544   164     80      2     418  114
        3 4 |   510   164     80      2     464  102
        4 2 |   612   164     80      2     384   80
        4 3 |   580   164     80      2     418   78
        4 4 |   542   164     80      2     464   70

    (one channel: 65535 x 32768 stays below 2^31 bytes, so `bytes` does not occur there in this sweep.  It can occur: at
    65535 x 32769, which test_frames_at_the_2_gib_edge plans.)  Every outcome must occur, so that no branch of the planner
    leaves the sweep unnoticed."""
    shapes = sweep_shapes()
    hs = {(s[0], s[2]) for s in shapes}
    vs = {(s[1], s[3]) for s in shapes}
    want = {(i, o) for i in SWEEP for o in SWEEP if i * o <= 4_000_000}
    assert want <= hs and want <= vs
    counts = {}
    for shape in shapes:
        for frames in (1, 32):
            r = check_plan(shape, channels, a, frames)
            counts[r] = counts.get(r, 0) + 1
    print(f"C={channels} a={a}: {counts}")
    outcomes = {"fused", "axis", "order", "bucket", "lds"} | ({"bytes"} if channels > 1 else set())
    assert set(counts) == outcomes, counts


def test_plan_query_validation():
    import ctypes
    lib = L._lib()
    p = L.ResizePlan()
    d = L.resize_desc(64, 48, 20, 100, 3, 3)
    assert lib.lanczos_resize_plan_host(ctypes.byref(d), 1, ctypes.byref(p)) == L.OK and p.fused == 1
    assert lib.lanczos_resize_plan_host(ctypes.byref(d), 0, ctypes.byref(p)) == L.ERR_BAD_ARG
    assert lib.lanczos_resize_plan_host(ctypes.byref(d), 1, None) == L.ERR_BAD_ARG
    assert lib.lanczos_resize_plan_host(None, 1, ctypes.byref(p)) == L.ERR_BAD_ARG
    d.channels = 2
    assert lib.lanczos_resize_plan_host(ctypes.byref(d), 1, ctypes.byref(p)) == L.ERR_BAD_ARG


# horizontal ksize -> (filter, a, in_w) at out_w = 261 (tests/test_resize*_gpu.py's instance shapes), and the tap count of the
# fused instance it runs on (0: two passes).  A box or bilinear upscale has 3 taps and a bicubic one 5, and only they run on
# the instances of 3 and 5; a Lanczos request pads to 7 at least, and 27 taps are more than any instance holds.
H_KSIZE_K = [(3, "box", 3, 200, 3), (3, "bilinear", 3, 200, 3), (5, "bicubic", 3, 200, 5), (5, "lanczos", 2, 200, 7),
             (7, "lanczos", 3, 200, 7), (9, "lanczos", 4, 200, 9), (11, "lanczos", 3, 392, 11), (13, "lanczos", 3, 496, 13),
             (15, "lanczos", 3, 574, 17), (17, "lanczos", 4, 496, 17), (19, "lanczos", 3, 757, 25), (21, "lanczos", 3, 835, 25),
             (23, "lanczos", 3, 913, 25), (25, "lanczos", 3, 1018, 25), (27, "lanczos", 3, 1100, 0)]


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_one_bucket_list_for_every_sample_width(channels):
    """The 8-bit, LANCZOS_RESIZE_U16 and LANCZOS_RESIZE_F32 descriptor of one shape run on the fused instance of the same tap
    count, or all three on two passes: horizontal ksize 3, 5, ..., 27 over the filters that reach them."""
    assert [r[0] for r in H_KSIZE_K if r[1] == "lanczos"] == list(range(5, 28, 2))
    ow, ih, oh = 261, 60, 67
    for hk, filt, a, iw, want in H_KSIZE_K:
        widths = {"u8": dict(), "u16": dict(bits=16), "f32": dict(f32=True)}
        assert L.resize_taps_host(L.resize_desc(iw, 1, ow, 1, 1, a, filter=filt), 0)[2].shape[1] == hk   # the public query
        got = {}
        for name, kw in widths.items():
            p = L.resize_plan_host(L.resize_desc(iw, ih, ow, oh, channels, a, filter=filt, **kw))
            got[name] = p.K if p.fused else 0
        assert got == {"u8": want, "u16": want, "f32": want}, (hk, filt, a, got)


# ---- the 2^31-byte edge, beyond the sweep -----------------------------------------------------------------------------------
# (name, in_w, in_h, channels, descriptor keywords, bytes per sample): frames of 2^31 bytes or more, two of them through the
# sample width alone.  tests/test_resize_wide_addresses_gpu.py runs them.
FRAMES_2GIB = [("u8c1", 65535, 32769, 1, {}, 1), ("u8c4", 32768, 16385, 4, {}, 1), ("rgba", 32768, 16385, 4, {"alpha": True}, 1),
               ("u16c3", 32768, 10923, 3, {"bits": 16}, 2), ("f32c3", 16384, 10923, 3, {"f32": True}, 4)]
OUT_EDGE = (173, 131)


def corner_box(in_w, in_h):
    """about 197 x 149 source pixels in the bottom-right corner, fractional on every side"""
    return (in_w - 200.25, in_h - 150.5, in_w - 3.0, in_h - 1.75)


def largest_fused_frame(bytes_per_pixel):
    """(in_w, in_h) with the most bytes the fused kernel admits (in_w * in_h * bytes_per_pixel + 4 < 2^31), both sides in
    1024 .. 65535: a short search over the heights."""
    limit = (2 ** 31 - 5) // bytes_per_pixel
    best = (0, 0, 0)
    for h in range(1024, 65536):
        w = min(65535, limit // h)
        if w >= 1024 and w * h > best[0]:
            best = (w * h, w, h)
    return best[1], best[2]


def frames_below_2gib():
    """(name, in_w, in_h, channels, descriptor keywords, bytes per sample) of the largest frames the fused kernel accepts"""
    return [("u8c4", 32766, 16385, 4, {}, 1), ("rgba", 32766, 16385, 4, {"alpha": True}, 1), ("u8c1", 65535, 32768, 1, {}, 1),
            ("u16c3",) + largest_fused_frame(6) + (3, {"bits": 16}, 2), ("f32c3",) + largest_fused_frame(12) + (3, {"f32": True}, 4)]


def bytes_reason(in_w, in_h, out_w, out_h, channels, bps):
    """the `bytes` reason of two_pass_reasons for any sample width"""
    return in_w * in_h * channels * bps + 4 >= 2 ** 31 or out_w * out_h * channels * bps >= 2 ** 31


def test_frames_at_the_2_gib_edge():
    """What the sweep cannot reach.  A frame of 2^31 bytes or more plans two passes for the `bytes` reason and no other: with
    the corner box the taps are few and the ring small, and the largest frame below the limit -- the same request but for a
    row, a column or a few of them -- plans fused.  That holds for one channel too (65535 x 32769, as input and as output), and
    for 16-bit and float frames, which cross 2^31 bytes through the sample width."""
    ow, oh = OUT_EDGE
    for name, iw, ih, c, kw, bps in FRAMES_2GIB:
        d = L.resize_desc(iw, ih, ow, oh, c, **kw)
        assert iw * ih * c * bps >= 2 ** 31 and bytes_reason(iw, ih, ow, oh, c, bps), name
        p = L.resize_plan_host(d, 1, box=corner_box(iw, ih))
        assert p.pass_h and p.pass_v and not p.inner.fused and p.mid_rows == 153, (name, p.mid_rows)
        assert (p.inner.K, p.inner.strips, p.inner.lds_bytes) == (0, 0, 0), name
    for name, iw, ih, c, kw, bps in frames_below_2gib():
        assert 2 ** 31 - 32768 <= iw * ih * c * bps <= 2 ** 31 - 5 and not bytes_reason(iw, ih, ow, oh, c, bps), (name, iw, ih)
        for w in (ow, 261):
            d = L.resize_desc(iw, ih, w, oh, c, **kw)
            p = L.resize_plan_host(d, 1, box=corner_box(iw, ih))
            hks = L.resize_taps_host(d, 0, box=corner_box(iw, ih))[2].shape[1]      # 9 taps down to 173, 7 up to 261
            assert hks == (9 if w == ow else 7)
            assert p.pass_h and p.pass_v and p.inner.fused and p.inner.K == hks, (name, w, p.inner.K)
    assert largest_fused_frame(6) == (57404, 6235) and largest_fused_frame(12) == (54610, 3277)
    # the whole frame, no box: 65535 x 32769 as a one-channel input, through check_plan like the sweep's shapes
    assert "bytes" in two_pass_reasons(65535, 32769, 60000, 30000, 1, 3)
    assert not L.resize_plan_host(L.resize_desc(65535, 32769, 60000, 30000, 1, 3), 1).fused
    assert check_plan((65535, 32768, 60000, 30000), 1, 3, 1) == "fused"
    # ... and as a one-channel output: an upscale of 7 taps whose ring is a few rows -- `bytes` is the only reason
    assert two_pass_reasons(40, 30, 65535, 32769, 1, 3) == ["bytes"]
    assert check_plan((40, 30, 65535, 32769), 1, 3, 1) == "bytes"
    assert check_plan((40, 30, 65535, 32768), 1, 3, 1) == "fused"
