"""Every launch route of the upscale entry, reached on purpose and checked against the CPU oracle.

lanczos_last_kernel() names a family only.  Which kernel produced the main rows and how the in-place prefix rows [0, K) were
produced (full_TB.h:67-77: the rows whose vertical taps read rows already written) is what lanczos_last_route() reports, and
every case here asserts the route it was built to reach before it compares samples:

  main kernel    none (a strip that ends inside the prefix rows) / march / tile / ratp / rat / generic
  prefix route   riding (extra workgroups of the k_march grid) / front (k_prefix_reg<T, S, A>, one unrolled instance per
                 (sample type, S, a), 13 of them) / behind (k_prefix) / streamed (k_prefix_stream)

EXACT mode: bit-identical to the oracle.  LSB1 mode: test_parity_gpu._cmp's contract (within 1 LSB and lsb1_check.check), and
the prefix rows bit-identical in both modes (the prefix kernels are f64 in every mode).

Batches are five distinct base frames cycled over a frame count that is no multiple of five: the oracle runs five times per
shape, and every frame of the batch is compared with its base frame's result on the device (a wrong frame index shows).
The front route needs more prefix workgroups than CUs in ONE launch, but lanczos_resample_device cuts a batch of twice the
instance's preferred size (one and a half times for the four-per-CU instances) into launches of that size, and for an instance
with one or two resident workgroups per CU those launches are small enough to ride again (8-bit RGBA 3x a = 4, 160 wide: 257
frames go out as five riding launches).  The window between the two sizes depends on the instance's workgroup size and
residency, which only the device knows, so _front_frames() finds the batch size by asking: CUs + 1, CUs // 2 + 1, ... until
one reports march + front in every launch.  Where no size does at 160 pixels (16-bit RGBA 3x a = 4: one workgroup per CU, as
many prefix workgroups per frame as strips -- the window is empty at every width that splits) the frames are 1040 wide: so many
strips that the preferred size falls below the eight frames from which batches are split at all.  Finding none fails the test.
"""
import numpy as np
import pytest

import lanczos_hls_amd as L
import oracle_lib as O
import patterns as P
from test_parity_gpu import _cmp
from upscale_route_cfg import _prefix_rows

pytestmark = pytest.mark.gpu

MARCH, TILE, RATP, RAT, GENERIC = L.ROUTE_MAIN_MARCH, L.ROUTE_MAIN_TILE, L.ROUTE_MAIN_RATP, L.ROUTE_MAIN_RAT, L.ROUTE_MAIN_GENERIC
NONE, RIDING, FRONT, BEHIND, STREAMED = (L.ROUTE_PREFIX_NONE, L.ROUTE_PREFIX_RIDING, L.ROUTE_PREFIX_FRONT, L.ROUTE_PREFIX_BEHIND,
                                         L.ROUTE_PREFIX_STREAMED)
MODES = (L.MODE_EXACT, L.MODE_LSB1)

# the 13 instances of k_prefix_reg (lanczos_upscale.hpp LZ_PREFIX_REG_CONFIGS) with the channel counts the integer-scale kernels have
INSTANCES = [(np.uint8, s, a) for s in (2, 3, 4) for a in (2, 3, 4)] + [(np.uint16, s, a) for s in (2, 3) for a in (3, 4)]
_IDS = [f"{np.dtype(dt).name}-{s}x-a{a}" for (dt, s, a) in INSTANCES]


def _channels(dt):
    return (1, 3, 4) if dt == np.uint8 else (3, 4)


def _width(c, bps, s, marching, block_multiple=None, near=160):
    """An input width near 160 (or `near`) whose rows are 16-byte multiples (march_supports) or not (the tile kernel; output rows stay
    dword multiples so that a specialised kernel serves), with out_w * c a multiple of the prefix kernels' 128-column block
    or not (a ragged last block: the j >= samples_w exit)."""
    for w in list(range(near, near + 100)) + list(range(near - 1, near - 60, -1)):
        if ((w * c * bps) % 16 == 0) != marching or (w * s * c * bps) % 4 != 0:
            continue
        if block_multiple is not None and ((w * s * c) % 128 == 0) != block_multiple:
            continue
        return w
    raise AssertionError((c, bps, s, marching, block_multiple))


def _base_frames(h, w, c, dt, seed):
    """Five distinct frames: noise and dark noise; 16-bit: full-range noise (overshoot saturates at 65535) and dark noise."""
    if dt == np.uint8:
        return [P.noise(h, w, c, seed=seed), P.dark_noise(h, w, c, seed=seed + 1), P.noise(h, w, c, seed=seed + 2),
                P.dark_noise(h, w, c, seed=seed + 3), P.noise(h, w, c, seed=seed + 4)]
    full = [P.noise(h, w, c, seed=seed + i, dtype=np.uint16) for i in range(5)]
    full[1] = (full[1] >> 8).astype(np.uint16)
    full[3] = (full[3] >> 6).astype(np.uint16)
    return full


def _oracle(img, sn, sd, a):
    h, w, c = img.shape
    cfg = O.cfg(w, h, w * sn // sd, h * sn // sd, c, a, sn, sd)
    fn = O.expected_hwc_u16 if img.dtype == np.uint16 else O.expected_hwc_u8
    return fn(cfg, img, 16), O.inplace_rows(cfg)


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev(arr):
    import torch
    arr = np.ascontiguousarray(arr)
    return torch.from_numpy(arr.view(np.int16) if arr.dtype == np.uint16 else arr).cuda()


def _host(t, dt):
    a = t.cpu().numpy()
    return a.view(np.uint16) if dt == np.uint16 else a


def _want_route(r, main, prefix, what, one_launch=True):
    """Exactly this route in every launch of the call (one_launch=False: a large batch, which may go out as several)."""
    assert r.main == main and r.prefix == prefix and r.prefix_seen == {prefix} and (r.launches == 1 or not one_launch), \
        f"{what}: route {r}, built to reach {L.ROUTE_MAIN_NAMES[main]}+{L.ROUTE_PREFIX_NAMES[prefix]}"


def _want_front(r, what):
    _want_route(r, MARCH, FRONT, what, one_launch=False)


_FRONT_FRAMES = {}


def _front_frames(ctx, cus, dt, c, s, a, w):
    """The batch size (no multiple of 5) at which frames of width w send k_prefix_reg<dt, s, a> ahead of every launch: the
    largest of CUs // k + 1 that does (see the module docstring); the same size with in_h < M2 must then report behind."""
    key = (np.dtype(dt).name, c, s, a, w)
    if key not in _FRONT_FRAMES:
        bases = _base_frames(_prefix_rows(s, a)[2], w, c, dt, seed=77)
        tried = []
        for k in range(1, 17):
            n = cus // k + 1
            while n % 5 == 0:
                n += 1
            _run_batch(ctx, bases, n, s, 1, a, L.MODE_EXACT)
            r = ctx.last_route()
            tried.append(f"{n} frames: {r}")
            if (r.main, r.prefix, r.prefix_seen) == (MARCH, FRONT, {FRONT}):
                _FRONT_FRAMES[key] = n
                break
        else:
            _FRONT_FRAMES[key] = "; ".join(tried)
    return _FRONT_FRAMES[key]


def _front_case(ctx, cus, dt, c, s, a, block_multiple):
    """(input width, batch size) at which the instance reaches march + front: about 160 wide, 1040 where that cannot."""
    tried = []
    for near in (160, 1040):
        w = _width(c, np.dtype(dt).itemsize, s, True, block_multiple, near)
        n = _front_frames(ctx, cus, dt, c, s, a, w)
        if isinstance(n, int):
            return w, n
        tried.append(f"{w} wide: {n}")
    raise AssertionError(f"{np.dtype(dt).name} c={c} {s}x a={a}: no batch size reaches march+front -- " + " | ".join(tried))


def _run_batch(ctx, bases, frames, sn, sd, a, mode, in_pad=0, out_pad=0, rows=None):
    """`frames` frames (the base frames cycled) through lanczos_resample_device; rows: a strip [0, rows) from the input rows
    lanczos_strip_input_rows names.  Returns the device result [frames][out rows][out_w][c] (padding cut off, checked)."""
    import torch
    h, w, c = bases[0].shape
    dt = bases[0].dtype.type
    bps = bases[0].dtype.itemsize
    d = L.make_desc(w, h, c, sn, sd, a, bps, mode, 0, rows or 0)
    in_rows = h
    if rows:
        r0, in_rows = L.strip_input_rows(d, 0, rows)
        assert r0 == 0
    out_rows = rows or d.out_h
    in_fb, out_fb = in_rows * w * c * bps, out_rows * d.out_w * c * bps
    src = np.stack([b[:in_rows] for b in bases]).reshape(5, in_fb // bps)
    xin = np.full((frames, (in_fb + in_pad) // bps), 0xA5A5 if bps == 2 else 0xA5, dtype=dt)
    xin[:, :in_fb // bps] = src[np.arange(frames) % 5]
    x = _dev(xin)
    y = torch.full((frames, (out_fb + out_pad) // bps), 0x5A5A if bps == 2 else 0x5A, dtype=x.dtype, device="cuda")
    ctx.resample_device(d, x.data_ptr(), y.data_ptr(), frames, in_fb + in_pad if in_pad else 0, out_fb + out_pad if out_pad else 0,
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if out_pad:
        assert bool((y[:, out_fb // bps:] == (0x5A5A if bps == 2 else 0x5A)).all()), "the padding between output frames was written"
    return y[:, :out_fb // bps].reshape(frames, out_rows, d.out_w, c)


def _check_batch(ctx, y, bases, wants, K, sn, sd, a, mode, what):
    """Every frame of the device result y against the oracle output of its base frame (wants: whole frames; y may be a strip
    from row 0).  LSB1: every frame equals the first frame of its base byte for byte (on the device), those five carry the
    contract -- checked on whole frames only, the contract check wants one."""
    import torch
    frames, rows = y.shape[0], y.shape[1]
    idx = torch.arange(frames, device="cuda") % 5
    dt = bases[0].dtype.type
    W = _dev(np.stack([wt[:rows] for wt in wants]))
    k = min(K, rows)
    bad = (y[:, :k] != W[idx][:, :k]).flatten(1).any(1).nonzero().flatten().tolist()
    assert not bad, f"{what}: prefix rows [0, {k}) differ from the reference in frames {bad[:8]} (of {len(bad)})"
    if mode == L.MODE_EXACT:
        bad = (y != W[idx]).flatten(1).any(1).nonzero().flatten().tolist()
        assert not bad, f"{what}: EXACT output differs from the reference in frames {bad[:8]} (of {len(bad)})"
        return
    if frames > 5:
        bad = (y != y[:5][idx]).flatten(1).any(1).nonzero().flatten().tolist()
        assert not bad, f"{what}: frames {bad[:8]} differ from the first frame with the same content"
    fam = ctx.last_kernel()
    for b in range(min(frames, 5)):
        got = _host(y[b], dt)
        if rows == wants[b].shape[0]:
            _cmp(got, wants[b], mode, f"{what}, frame {b}", (bases[b], sn, sd, a, fam))
        else:
            diff = np.abs(got.astype(np.int64) - wants[b][:rows].astype(np.int64))
            assert diff.max() <= 1, f"{what}, frame {b}: max |diff| {diff.max()} > 1 LSB"


def _shapes_of(ctx, cus, dt, s, a):
    """(channels, input width, input height, batch size) of an instance's cases: both widths x both heights."""
    m2 = _prefix_rows(s, a)[2]
    for c in _channels(dt):
        for block_multiple in (True, False):
            w, frames = _front_case(ctx, cus, dt, c, s, a, block_multiple)
            for h in (m2, m2 + 5):
                yield c, w, h, frames


# ---- a. every k_prefix_reg instance -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,s,a", INSTANCES, ids=_IDS)
def test_every_front_prefix_instance(ctx, cus, dt, s, a):
    """k_prefix_reg<T, S, A> in front of k_march, for every instance: more prefix workgroups than CUs, input heights M2 (the smallest the
    kernel admits: it does not clamp rows beyond the frame) and M2 + 5, a width whose sample columns fill the 128-column blocks
    and one with a ragged last block."""
    K, M, M2 = _prefix_rows(s, a)
    for c, w, h, frames in _shapes_of(ctx, cus, dt, s, a):
        assert frames % 5 != 0
        bases = _base_frames(h, w, c, dt, seed=1000 + 16 * s + a)
        res = [_oracle(b, s, 1, a) for b in bases]
        wants = [r[0] for r in res]
        assert res[0][1] == K and L.inplace_rows(L.make_desc(w, h, c, s, 1, a, bases[0].dtype.itemsize)) == K
        for mode in MODES:
            what = f"{np.dtype(dt).name} c={c} {s}x a={a} {w}x{h} x{frames} mode {mode}"
            y = _run_batch(ctx, bases, frames, s, 1, a, mode)
            _want_front(ctx.last_route(), what)
            _check_batch(ctx, y, bases, wants, K, s, 1, a, mode, what)


# ---- b. one step either side of each routing threshold ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt,s,a", INSTANCES, ids=_IDS)
def test_one_step_either_side_of_each_threshold(ctx, cus, dt, s, a):
    """The shapes of the test above with one condition of the front route taken away at a time:
    one frame -> the prefix rows ride (also with in_h < M2, where the riding workgroups clamp the rows beyond the frame);
    in_h = M2 - 1 and in_h = 2 with the large batch -> k_prefix behind k_march (the front kernel does not clamp and is refused);
    in_h = 1 -> no output row reads a row below itself: K = 0, no prefix route at all;
    the large batch at a width whose rows are no 16-byte multiples -> the tile kernel, k_prefix behind it."""
    K, M, M2 = _prefix_rows(s, a)
    bps = np.dtype(dt).itemsize
    for c in _channels(dt):
        wm, large = _front_case(ctx, cus, dt, c, s, a, False)   # the width and batch that go in front at in_h = M2
        wt = _width(c, bps, s, False)
        cases = [(wm, M2, 1, MARCH, RIDING), (wm, M2 + 5, 1, MARCH, RIDING), (wm, M2 - 1, 1, MARCH, RIDING), (wm, 1, 1, MARCH, NONE),
                 (wm, M2 - 1, large, MARCH, BEHIND), (wm, 2, large, MARCH, BEHIND), (wm, 1, large, MARCH, NONE),
                 (wt, M2, large, TILE, BEHIND), (wt, M2 + 5, large, TILE, BEHIND)]
        for (w, h, frames, main, prefix) in cases:
            bases = _base_frames(h, w, c, dt, seed=2000 + 16 * s + a)
            res = [_oracle(b, s, 1, a) for b in bases]
            k = res[0][1]
            assert (k > 0) == (prefix != NONE) and k <= K and (h < M2 or k == K), (h, k, K)
            for mode in MODES:
                what = f"{np.dtype(dt).name} c={c} {s}x a={a} {w}x{h} x{frames} mode {mode}"
                y = _run_batch(ctx, bases, frames, s, 1, a, mode)
                r = ctx.last_route()
                # (a large batch may be split: every launch of it must take the same route)
                _want_route(r, main, prefix, what, one_launch=frames == 1)
                _check_batch(ctx, y, bases, [x[0] for x in res], k, s, 1, a, mode, what)


# ---- c. strips from row 0 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,c,s,a", [(np.uint8, 3, 2, 3), (np.uint16, 4, 2, 4)], ids=["uint8-rgb-2x-a3", "uint16-rgba-2x-a4"])
def test_strips_from_row_0_into_and_past_the_prefix(ctx, cus, dt, c, s, a):
    """A strip [0, rows) with rows <= K has no main rows: nothing marches, and with no marching grid to ride on the prefix rows
    come from the front kernel whatever the batch size.  One and nine rows past K: riding for one frame, front for a large
    batch.  Input rows are those lanczos_strip_input_rows names; results are the same rows of the whole-frame reference."""
    K, M, M2 = _prefix_rows(s, a)
    (w, large), h = _front_case(ctx, cus, dt, c, s, a, False), 24
    bases = _base_frames(h, w, c, dt, seed=3000)
    res = [_oracle(b, s, 1, a) for b in bases]
    assert res[0][1] == K
    for frames in (1, large):
        for rows in (1, K - 1, K, K + 1, K + 9):
            for mode in MODES:
                what = f"{np.dtype(dt).name} strip [0, {rows}) of {w}x{h} x{frames} mode {mode} (K = {K})"
                y = _run_batch(ctx, bases, frames, s, 1, a, mode, rows=rows)
                r = ctx.last_route()
                if rows <= K:
                    _want_route(r, L.ROUTE_MAIN_NONE, FRONT, what, one_launch=frames == 1)
                elif frames == 1:
                    _want_route(r, MARCH, RIDING, what)
                else:
                    _want_front(r, what)
                _check_batch(ctx, y, bases, [x[0] for x in res], K, s, 1, a, mode, what)


# ---- d. the front route with padded frames ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,c,s,a,pad_in,pad_out", [(np.uint8, 3, 3, 2, 48, 80), (np.uint8, 1, 4, 4, 4096, 16), (np.uint16, 3, 3, 3, 32, 4112)])
def test_front_route_with_padded_frames(ctx, cus, dt, c, s, a, pad_in, pad_out):
    """In and out frame strides that are 16-byte multiples larger than the frames: k_march keeps the batch, k_prefix_reg goes
    in front with the same strides.  The padding is poisoned on both sides; that of the output must stay as it was."""
    K, M, M2 = _prefix_rows(s, a)
    (w, frames), h = _front_case(ctx, cus, dt, c, s, a, False), M2 + 2
    bases = _base_frames(h, w, c, dt, seed=4000)
    res = [_oracle(b, s, 1, a) for b in bases]
    for mode in MODES:
        what = f"{np.dtype(dt).name} c={c} {s}x a={a} {w}x{h} x{frames} pads {pad_in}/{pad_out} mode {mode}"
        y = _run_batch(ctx, bases, frames, s, 1, a, mode, in_pad=pad_in, out_pad=pad_out)
        _want_front(ctx.last_route(), what)
        _check_batch(ctx, y, bases, [x[0] for x in res], K, s, 1, a, mode, what)


# ---- e. the front route inside a split batch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,s,frames", [(1920, 2, 73), (1280, 3, 81)], ids=["four-per-cu-1920-2x", "two-per-cu-1280-3x"])
def test_front_route_inside_a_split_batch(ctx, w, s, frames):
    """An oversized batch goes out as several launches (resample_device_locked): 1920-wide RGB8 2x, the four-workgroups-per-CU
    instance, prefers 32 frames (73 = 32 + 32 + 9), 1280-wide RGB8 3x, a two-per-CU instance, 24 (81 = 3 x 24 + 9); each
    launch sends its own front kernel ahead, on its own frames, the last nine included (nine frames of 30 prefix
    workgroups are more than the CUs).  Short frames; EVERY frame is compared, so both sides of every cut are, wherever
    the cuts fall."""
    a, c, h = 3, 3, 20
    K = _prefix_rows(s, a)[0]
    bases = _base_frames(h, w, c, np.uint8, seed=5000 + s)
    res = [_oracle(b, s, 1, a) for b in bases]
    for mode in MODES:
        what = f"{w}x{h} {s}x x{frames} mode {mode}"
        y = _run_batch(ctx, bases, frames, s, 1, a, mode)
        r = ctx.last_route()
        assert r.launches > 1, f"{what}: route {r}, built to be split"
        assert r.main == MARCH and r.prefix_seen == {FRONT}, f"{what}: route {r}, built to reach march+front in every launch"
        _check_batch(ctx, y, bases, [x[0] for x in res], K, s, 1, a, mode, what)


# ---- f. deep prefixes and the rational kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,c,sn,sd,a,dt,main,prefix", [
    (128, 96, 3, 9, 8, 3, np.uint8, RAT, BEHIND),        # K = 19: a few dozen rows in LDS
    (128, 144, 1, 33, 32, 3, np.uint8, RAT, BEHIND),     # K = 67
    (64, 200, 4, 65, 64, 4, np.uint8, RAT, BEHIND),      # K = 196
    (32, 600, 4, 257, 256, 3, np.uint16, RAT, STREAMED), # K = 515: M + M2 rows of 32 16-bit columns are more than 60 KB
    (24, 1000, 1, 1, 1, 3, np.uint8, GENERIC, STREAMED), # S = 1: the whole height is prefix
    (96, 60, 3, 3, 2, 3, np.uint8, RATP, BEHIND),        # a periodic scale: k_ratp
    (96, 60, 3, 5, 3, 3, np.uint8, RAT, BEHIND),         # 5/3: x = o / SCALE rounds, not periodic: k_rat
    (96, 60, 3, 4, 3, 3, np.uint8, RATP, BEHIND),
])
def test_deep_prefixes_behind_and_streamed(ctx, w, h, c, sn, sd, a, dt, main, prefix):
    """Scales close to 1: the prefix is K ~ a * S / (S - 1) rows deep.  k_prefix holds M + M2 rows of its columns in LDS;
    past 60 KB at 32 columns k_prefix_stream takes over.  The main kernel is k_rat (k_ratp has instances up to N = 7), k_generic
    at S = 1, and k_ratp / k_rat for the periodic / non-periodic small ratios."""
    img = P.noise(h, w, c, seed=31) if dt == np.uint8 else P.noise(h, w, c, seed=31, dtype=np.uint16)
    want, K = _oracle(img, sn, sd, a)
    assert K == L.inplace_rows(L.make_desc(w, h, c, sn, sd, a, img.dtype.itemsize)) and K > 0
    for frames in (1, 3):
        for mode in MODES:
            what = f"{sn}/{sd} {w}x{h}x{c} a={a} x{frames} mode {mode} (K = {K})"
            y = _run_batch(ctx, [img] * 5, frames, sn, sd, a, mode)
            _want_route(ctx.last_route(), main, prefix, what)
            _check_batch(ctx, y, [img] * 5, [want] * 5, K, sn, sd, a, mode, what)


def test_route_report_of_the_other_entry_points(ctx):
    """The host entry counts the launches of its pipeline's groups; the planar entry reports its resample; a resize, a reduce,
    a layout call and a refused call report none.  lanczos_last_kernel is what it was."""
    import torch
    img = P.noise(40, 64, 3, seed=9)
    got = ctx.resample(np.stack([img] * 9), 2, 1, 3, L.MODE_EXACT)       # groups of 4, 4, 1
    r = ctx.last_route()
    assert (r.main, r.prefix, r.launches) == (MARCH, RIDING, 3) and ctx.last_kernel() == L.KERNEL_FAST, str(r)
    want, K = _oracle(img, 2, 1, 3)
    assert all(np.array_equal(g, want) for g in got)
    ctx.resize(img, 32, 20)
    assert ctx.last_route() == L.Route(0, 0, 0, frozenset()) and ctx.last_kernel() in (L.KERNEL_RESIZE_FUSED, L.KERNEL_RESIZE_TWO_PASS)
    ctx.resample(img, 2, 1, 3, L.MODE_HLS)
    r = ctx.last_route()
    assert (r.main, r.prefix, r.launches) == (L.ROUTE_MAIN_HLS, NONE, 1) and ctx.last_kernel() == L.KERNEL_HLS
    ctx.reduce(img, 2)
    assert ctx.last_route().launches == 0
    d = L.make_desc(64, 40, 3, 2, 1, 3, 1, L.MODE_EXACT)
    x = _dev(np.ascontiguousarray(img.transpose(2, 0, 1)))
    y = torch.zeros((3, 80, 128), dtype=torch.uint8, device="cuda")
    ctx.resample_planar_device(d, x.data_ptr(), y.data_ptr(), 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    r = ctx.last_route()
    assert (r.main, r.prefix, r.launches) == (MARCH, RIDING, 1), str(r)
    assert np.array_equal(y.cpu().numpy().transpose(1, 2, 0), want)
    ctx.planar_to_interleaved_device(x.data_ptr(), y.data_ptr(), 64, 40, 3, 1, 1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ctx.last_route().launches == 0
    ctx.resample(img, 2, 1, 3)
    assert ctx.last_route().launches == 1
    d = L.make_desc(64, 40, 3, 2, 1, 3, 1, L.MODE_EXACT, out_row0=2, out_rows=8)   # a strip that cuts the prefix rows: refused
    r0, n = L.strip_input_rows(d, 2, 8)
    with pytest.raises(L.LanczosError) as e:
        ctx.resample_strip(img[r0:r0 + n], d)
    assert e.value.code == L.ERR_UNSUPPORTED and ctx.last_route().launches == 0
