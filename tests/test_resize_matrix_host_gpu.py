"""The host entries over the resize matrix (tests/resize_matrix_cfg.py): every legal case under RESIZE_AUTO, with the destination
cases, goes once through the host entry that takes it -- lanczos_resize_dest_host for bytes out (with or without a source and a
destination), lanczos_resize_tensor_source_host for every tensor output (a window or crops, with or without a source) -- called by
ctypes on numpy buffers.  The force changes nothing in the staging code (resize_host), and resize_device behind it is walked under
every force by tests/test_resize_matrix_gpu.py.
The buffers are the tight ones of the header: frames the layout's own extent apart, `out` exactly as long as it says
(cfg.host_out_bytes), prefilled with the sentinel and lying inside a larger array of sentinels, so that a copy-down that is too long
shows as a changed sentinel and not as heap damage.  The whole array is compared with cfg.expected_host: what the strides do not
name -- padded tensor rows and planes, destination padding -- has to come back as it went in.  The table, the flips and the origins
are host arrays; the origins are cfg.host_origins_of, since the host entry refuses an origin outside the output, and
cfg.origins_of itself is one refused request per crop output.  Every refused case a host entry can express returns its code and
leaves `out` untouched; after a legal case the kernel and the three routes the context reports are the predictions."""
import ctypes

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_matrix_cfg as M
import resize_tensor_view_model as V

pytestmark = pytest.mark.gpu

AROUND = 256   # sentinel bytes in front of `out` and behind it


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.resize_force(L.RESIZE_AUTO)
    c.close()


class _Host:
    """what a (kind, geometry) test keeps: the frames in every layout, the tables, the flips, the origins"""

    def __init__(self, kind, geo):
        k = M.KINDS[kind]
        self.tight = np.ascontiguousarray(M.frames_of(kind, geo)).view(np.uint8).reshape(-1).copy()
        self.src = {name: M.host_source_of(kind, geo, name) for name in ("pitched", "planar")
                    if name == "pitched" or (k.bps == 1 and k.channels > 1)}
        self.luts = {}
        self.flips = np.array(M.D_FLIP, dtype=np.uint8)
        self.origins = {True: M.host_origins_of(geo), False: np.ascontiguousarray(M.origins_of(geo))}

    def lut(self, case):
        key = (M.OUTPUTS[case.out].elem, len(M.out_channels(case)))
        if key not in self.luts:
            self.luts[key] = V.words(M.lut_of(case)).view(np.uint8).reshape(-1).copy()
        return self.luts[key].ctypes.data

    def input(self, case):
        """(host pointer, ResizeSource or None): the frames the layout's own extent apart"""
        if case.src == "none":
            return self.tight.ctypes.data, None
        if case.src in self.src:
            s = self.src[case.src]
            assert (s.buf.ctypes.data + s.at) % 4 == 0
            return s.buf.ctypes.data + s.at, M.source_struct(case, s)
        return self.tight.ctypes.data, M.source_struct(case)   # a layout the entry refuses before it reads a byte


def _call(ctx, host, case, dest, out_ptr, inside=True):
    """the host entry of a case; returns its code"""
    o = M.OUTPUTS[case.out]
    lib, d = L._lib(), M.desc_of(case)
    opts = None
    if case.opt != "none":   # the box defaults to the whole frame and the gap to 0, as lanczos_resize_opts_init leaves them
        o_ = L.ResizeOpts()
        o_.box[:] = [float(v) for v in (M.box_of(case) or (0, 0, d.in_w, d.in_h))]
        o_.reducing_gap = M.gap_of(case) or 0.0
        opts = ctypes.byref(o_)
    window = M.window_of(case)
    wref = None
    if window:   # written field by field: a refused descriptor has to reach the entry
        win = L.ResizeWindow()
        win.x0, win.y0, win.w, win.h = window
        wref = ctypes.byref(win)
    in_ptr, source = host.input(case)
    sref = ctypes.byref(source) if source is not None else None
    if not o.elem:
        dref = ctypes.byref(M.dest_struct(case, dest)) if dest else None
        return lib.lanczos_resize_dest_host(ctx._h, ctypes.byref(d), opts, wref, sref, dref, in_ptr, out_ptr, M.FRAMES)
    assert dest is None
    view = L.tensor_view(host.lut(case), M.tensor_strides(case), o.elem, M.out_channels(case), o.flip if o.mapped else 0,
                         host.flips.ctypes.data if o.mapped else None)
    crops = L.resize_crops(*M.crop_size(case.geo), host.origins[inside].ctypes.data) if o.crop else None
    cref = ctypes.byref(crops) if crops is not None else None
    return lib.lanczos_resize_tensor_source_host(ctx._h, ctypes.byref(d), opts, wref, cref, sref, ctypes.byref(view), in_ptr, out_ptr,
                                                 M.FRAMES)


def host_cases(kind, geo):
    """(case, dest or None, verdict, inside) of the host walk, in the order of the device walk: every legal case under AUTO and
    every refused one a host entry can express -- those of AUTO, and those only the forced FUSED refuses; behind every legal crop
    output the same request with origins_of() unclamped, which the host entry refuses"""
    for case in M.cases((kind,), (geo,)):
        verdict = M.legality(case)
        if verdict == M.NA or case.force not in (L.RESIZE_AUTO, L.RESIZE_FUSED):
            continue
        auto = case._replace(force=L.RESIZE_AUTO)
        if case.force == L.RESIZE_FUSED and not (verdict is not None and M.legality(auto) is None):
            continue
        yield case, None, verdict, True
        if verdict is None and M.OUTPUTS[case.out].crop and case.src == "none":
            yield case, None, L.ERR_BAD_ARG, False
        if case.out == "bytes":
            for dest in M.DESTS:
                dv = M.dest_legality(case, dest)
                if case.force == L.RESIZE_AUTO or (dv is not None and M.dest_legality(auto, dest) is None):
                    yield case, dest, dv, True


def _run(ctx, kind, geo):
    host = _Host(kind, geo)
    f32 = M.KINDS[kind].bps == 4
    legal = refused = 0
    failures = []
    routes = [ctx.last_source_route(), ctx.last_dest_route()]
    after_refusal = ""
    try:
        for case, dest, verdict, inside in host_cases(kind, geo):
            what = M.describe(case) + (f" -> {dest}" if dest else "") + ("" if inside else " (an origin outside)")
            n = M.host_out_bytes(case, dest)
            buf = np.full(AROUND + n + AROUND, M.SENTINEL, dtype=np.uint8)
            assert (buf.ctypes.data + AROUND) % 4 == 0
            ctx.resize_force(case.force)
            code = _call(ctx, host, case, dest, buf.ctypes.data + AROUND, inside)
            if verdict is not None:
                refused += 1
                if code != verdict:
                    failures.append(f"{what}: returned {code}, not {verdict}")
                if (buf != M.SENTINEL).any():
                    failures.append(f"{what}: a refused call wrote to the output")
                if [ctx.last_source_route(), ctx.last_dest_route()] != routes:
                    failures.append(f"{what}: a refused call changed the source or the destination route")
                    routes = [ctx.last_source_route(), ctx.last_dest_route()]
                after_refusal = " (after a refusal)"
                continue
            legal += 1
            if code != L.OK:
                failures.append(f"{what}: returned {code}")
                continue
            want = M.expected_host(case, dest)
            assert want.size == n
            pred = M.predict(case)
            word = np.uint32 if f32 else np.uint8           # whole floats, by the rule of resize32_model.same
            diff = M.first_difference(buf[AROUND:AROUND + n].view(word), want.view(word), f32)
            if diff is not None:
                failures.append(f"{what}{after_refusal}: first difference at {'word' if f32 else 'byte'} {diff[0] + M.GUARD} of "
                                f"`out` ({n} bytes): {diff[1]:#x} != {diff[2]:#x}; predicted {tuple(pred)}")
            if (buf[:AROUND] != M.SENTINEL).any() or (buf[AROUND + n:] != M.SENTINEL).any():
                failures.append(f"{what}: a byte in front of `out` or behind it was written")
            if pred.source_route is not None:
                routes[0] = pred.source_route
            if dest:
                routes[1] = M.predict_dest(case, dest)
            report = (ctx.last_kernel(), ctx.last_tensor_route(), ctx.last_source_route(), ctx.last_dest_route())
            if report != (pred.last_kernel, pred.tensor_route, *routes):
                failures.append(f"{what}: reported (kernel, tensor route, source route, destination route) {report}, predicted "
                                f"{(pred.last_kernel, pred.tensor_route, *routes)}")
                routes = list(report[2:])
            after_refusal = ""
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
    return legal, refused, failures


@pytest.mark.parametrize("geo", list(M.GEOMETRIES))
@pytest.mark.parametrize("kind", list(M.KINDS))
def test_matrix_host(ctx, kind, geo):
    legal, refused, failures = _run(ctx, kind, geo)
    assert not failures, f"{len(failures)} failures in {legal} legal and {refused} refused cases, the first: {failures[0]}"
    # the counts against the rules: every legal case and destination case of AUTO; every refused one of AUTO, every one that
    # only the forced FUSED refuses, and one request with an origin outside per legal crop output
    auto = [c for c in M.cases((kind,), (geo,)) if c.force == L.RESIZE_AUTO and M.legality(c) != M.NA]
    pairs = [(c, d) for c in auto if c.out == "bytes" for d in M.DESTS]
    fused = [c._replace(force=L.RESIZE_FUSED) for c in auto if M.legality(c) is None]
    want_legal = sum(M.legality(c) is None for c in auto) + sum(M.dest_legality(c, d) is None for c, d in pairs)
    want_refused = (sum(M.legality(c) is not None for c in auto) + sum(M.dest_legality(c, d) is not None for c, d in pairs) +
                    sum(M.legality(c) is not None for c in fused) +
                    sum(M.dest_legality(c, d) is not None for c in fused if c.out == "bytes" for d in M.DESTS
                        if M.dest_legality(c._replace(force=L.RESIZE_AUTO), d) is None) +
                    sum(M.legality(c) is None and M.OUTPUTS[c.out].crop and c.src == "none" for c in auto))
    assert legal == want_legal > 0 and refused == want_refused > 0, (legal, want_legal, refused, want_refused)
