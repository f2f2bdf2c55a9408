"""GPU run of the resize matrix (tests/resize_matrix_cfg.py): every combination of sample kind, geometry, filter, options, window,
output, source layout and forced path that is a request goes through the device entries once, on a side stream, into a buffer of
sentinels.  A legal case is compared element for element with the numpy models composed on the CPU (float samples by the rule of
resize32_model.same), and the kernel, tensor route and source route the context reports with cfg.predict; a refused case must
return its code and leave every sentinel, and the legal case after it on the same context must still be right.  One test per
(kind, geometry); the reference of a case is computed once and shared by its sources and forced paths.
The same test then walks the pair's destination cases (cfg.dest_cases: every bytes-out request into pitched rows and into planes)
through lanczos_resize_dest_device with the same context, stream and sentinels: the whole buffer -- named bytes, row and plane
padding, frame gaps and guards in one comparison -- against cfg.expected_dest, and the kernel, source route and destination route
the context reports against cfg.predict / cfg.predict_dest."""
import collections

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_matrix_cfg as M
import resize_tensor_view_model as V

pytestmark = pytest.mark.gpu

_WORD = {1: np.uint8, 2: np.uint16, 4: np.uint32}


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.resize_force(L.RESIZE_AUTO)
    c.close()


class _Device:
    """what a (kind, geometry) test keeps on the device: the frames in every layout, the tables, flips and origins, one output"""

    def __init__(self, kind, geo):
        import torch
        self.torch = torch
        k = M.KINDS[kind]
        x = M.frames_of(kind, geo)
        self.tight = torch.from_numpy(x.view(np.uint8).reshape(-1).copy()).cuda()
        self.src = {}
        for name in ("pitched", "planar"):
            if name == "planar" and (k.bps != 1 or k.channels == 1):
                continue
            s = M.source_of(kind, geo, name)
            self.src[name] = (s, torch.from_numpy(s.buf).cuda())
            assert self.src[name][1].data_ptr() % 4 == 0
        self.luts = {}
        self.flips = torch.tensor(M.D_FLIP, dtype=torch.uint8).cuda()
        self.origins = torch.from_numpy(M.origins_of(geo)).cuda()
        biggest = max(M.out_geometry(M.Case(kind, geo, "lanczos", "none", "whole", o, "none", 0))[3] * 4 for o in M.OUTPUTS)
        self.out = torch.empty(biggest, dtype=torch.uint8, device="cuda")
        assert self.out.data_ptr() % 4 == 0

    def lut(self, case):
        key = (M.OUTPUTS[case.out].elem, len(M.out_channels(case)))
        if key not in self.luts:
            self.luts[key] = self.torch.from_numpy(V.words(M.lut_of(case)).view(np.uint8).reshape(-1).copy()).cuda()
        return self.luts[key].data_ptr()

    def input(self, case):
        """(device pointer, frame stride, ResizeSource or None)"""
        if case.src == "none":
            return self.tight.data_ptr(), 0, None
        if case.src in self.src:
            s, buf = self.src[case.src]
            return buf.data_ptr() + s.at, s.frame_stride, M.source_struct(case, s)
        return self.tight.data_ptr(), 0, M.source_struct(case)   # a layout the entry refuses before it reads a byte


def _call(ctx, dev, case, stream):
    """the device entry of a case on dev.out, GUARD elements in"""
    o = M.OUTPUTS[case.out]
    d = M.desc_of(case)
    item, _, fs, _ = M.out_geometry(case)
    d_in, in_fs, source = dev.input(case)
    d_out = dev.out.data_ptr() + M.GUARD * item
    kw = dict(in_frame_stride=in_fs, out_frame_stride=fs * item, stream=stream, box=M.box_of(case), reducing_gap=M.gap_of(case),
              source=source)
    if not o.elem:
        ctx.resize_device(d, d_in, d_out, M.FRAMES, window=M.window_of(case), **kw)
        return
    if o.mapped:
        kw.update(channels_out=M.out_channels(case), flip=o.flip, d_flip=dev.flips.data_ptr())
    if o.crop:
        kw.update(crop=M.crop_size(case.geo), d_origin=dev.origins.data_ptr())
    else:
        kw.update(window=M.window_of(case))
    ctx.resize_tensor_device(d, d_in, d_out, M.FRAMES, dev.lut(case), M.tensor_strides(case),
                             dtype="float32" if o.elem == 4 else "bfloat16", **kw)


def _run(ctx, kind, geo):
    """every case of (kind, geo) that is a request, once; returns (legal, refused, failures).  A wrong result is noted and the walk
    goes on, so that a failing test says how many cases fail; an error of the library or the runtime ends it."""
    import torch
    dev = _Device(kind, geo)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()   # the uploads above ran on the default stream
    f32 = M.KINDS[kind].bps == 4
    legal = refused = 0
    failures = []
    source_route = ctx.last_source_route()
    after_refusal = ""
    try:
        with torch.cuda.stream(side):
            for case in M.cases((kind,), (geo,)):
                verdict = M.legality(case)
                if verdict == M.NA:
                    continue
                item, _, _, total = M.out_geometry(case)
                what = M.describe(case)
                dev.out.fill_(M.SENTINEL)
                ctx.resize_force(case.force)
                if verdict is not None:
                    refused += 1
                    try:
                        _call(ctx, dev, case, side.cuda_stream)
                        code = L.OK
                    except L.LanczosError as e:
                        code = e.code
                    if code != verdict:
                        failures.append(f"{what}: returned {code}, not {verdict}")
                    if bool((dev.out != M.SENTINEL).any()):
                        failures.append(f"{what}: a refused call wrote to the output")
                    if ctx.last_source_route() != source_route:
                        failures.append(f"{what}: a refused call changed the source route")
                        source_route = ctx.last_source_route()
                    after_refusal = " (after a refusal)"
                    continue
                legal += 1
                _call(ctx, dev, case, side.cuda_stream)
                got = dev.out[:total * item].cpu().numpy().view(_WORD[item])
                pred = M.predict(case)
                diff = M.first_difference(got, M.expected(case), f32)
                if diff is not None:
                    failures.append(f"{what}{after_refusal}: first difference at element {diff[0]} of the output: {diff[1]:#x} != "
                                    f"{diff[2]:#x}; predicted {tuple(pred)}")
                if not bool((dev.out[total * item:] == M.SENTINEL).all()):
                    failures.append(f"{what}: a byte behind the output was written")
                if pred.source_route is not None:
                    source_route = pred.source_route
                report = (ctx.last_kernel(), ctx.last_tensor_route(), ctx.last_source_route())
                if report != (pred.last_kernel, pred.tensor_route, source_route):
                    failures.append(f"{what}: reported (kernel, tensor route, source route) {report}, predicted {tuple(pred)}")
                    source_route = report[2]
                after_refusal = ""
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
        torch.cuda.synchronize()
    return legal, refused, failures


def _run_dest(ctx, kind, geo):
    """every destination case of (kind, geo), once, as _run walks the cases without one; returns (legal, refused, failures, the
    count of every (dest, reported route) of a legal case, the leaves of cfg.DEST_LEAVES whose case ran and reported as predicted)"""
    import torch
    dev = _Device(kind, geo)
    k = M.KINDS[kind]
    todo = list(M.dest_cases((kind,), (geo,)))
    biggest = max(M.dest_layout(c, d).buf.size for c, d in todo)
    out = torch.empty((biggest + 3) // 4 * 4 + 64, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 4 == 0
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    legal = refused = 0
    failures = []
    seen = collections.Counter()
    leaves = set()
    source_route, dest_route = ctx.last_source_route(), ctx.last_dest_route()
    after_refusal = ""
    try:
        with torch.cuda.stream(side):
            for case, dest in todo:
                verdict = M.dest_legality(case, dest)
                what = f"{M.describe(case)} -> {dest}"
                t = M.dest_layout(case, dest)
                d_in, in_fs, source = dev.input(case)
                out.fill_(M.SENTINEL)
                ctx.resize_force(case.force)

                def call():
                    ctx.resize_device(M.desc_of(case), d_in, out.data_ptr() + t.at, M.FRAMES, in_frame_stride=in_fs,
                                      out_frame_stride=t.frame_stride, stream=side.cuda_stream, box=M.box_of(case),
                                      reducing_gap=M.gap_of(case), window=M.window_of(case), source=source,
                                      dest=M.dest_struct(case, dest))
                if verdict is not None:
                    refused += 1
                    try:
                        call()
                        code = L.OK
                    except L.LanczosError as e:
                        code = e.code
                    if code != verdict:
                        failures.append(f"{what}: returned {code}, not {verdict}")
                    if bool((out != M.SENTINEL).any()):
                        failures.append(f"{what}: a refused call wrote to the output")
                    if (ctx.last_source_route(), ctx.last_dest_route()) != (source_route, dest_route):
                        failures.append(f"{what}: a refused call changed the source or the destination route")
                        source_route, dest_route = ctx.last_source_route(), ctx.last_dest_route()
                    after_refusal = " (after a refusal)"
                    continue
                legal += 1
                call()
                got = out.cpu().numpy()
                want = M.expected_dest(case, dest)
                pred, want_route = M.predict(case), M.predict_dest(case, dest)
                word = np.uint32 if k.bps == 4 else np.uint8        # whole floats, by the rule of resize32_model.same
                diff = M.first_difference(got[:want.size].view(word), want.view(word), k.bps == 4)
                if diff is not None:
                    failures.append(f"{what}{after_refusal}: first difference at {'word' if k.bps == 4 else 'byte'} "
                                    f"{diff[0] + M.GUARD} of the buffer (frame 0 starts at byte {t.at}): {diff[1]:#x} != {diff[2]:#x}; "
                                    f"predicted {tuple(pred)}, destination route {want_route}")
                if not (got[want.size:] == M.SENTINEL).all():
                    failures.append(f"{what}: a byte behind the buffer was written")
                if pred.source_route is not None:
                    source_route = pred.source_route
                dest_route = want_route
                report = (ctx.last_kernel(), ctx.last_source_route(), ctx.last_dest_route())
                seen[dest, report[2]] += 1
                if report != (pred.last_kernel, source_route, dest_route):
                    failures.append(f"{what}: reported (kernel, source route, destination route) {report}, predicted "
                                    f"{(pred.last_kernel, source_route, dest_route)}")
                    source_route, dest_route = report[1:]
                elif diff is None:
                    leaves.update(leaf for leaf in M.predict_dest_main(case, dest) if leaf in M.DEST_LEAVES)
                after_refusal = ""
    finally:
        ctx.resize_force(L.RESIZE_AUTO)
        torch.cuda.synchronize()
    return legal, refused, failures, seen, leaves


@pytest.mark.parametrize("geo", list(M.GEOMETRIES))
@pytest.mark.parametrize("kind", list(M.KINDS))
def test_matrix(ctx, kind, geo):
    legal, refused, failures = _run(ctx, kind, geo)
    assert not failures, f"{len(failures)} failures in {legal} legal and {refused} refused cases, the first: {failures[0]}"
    want = [M.legality(c) for c in M.cases((kind,), (geo,))]
    assert legal == sum(v is None for v in want) > 0 and refused == sum(v not in (None, M.NA) for v in want)
    # ... and the same requests with a destination, where they store bytes
    legal, refused, failures, seen, leaves = _run_dest(ctx, kind, geo)
    assert not failures, (f"{len(failures)} failures in {legal} legal and {refused} refused cases with a destination, the first: "
                          f"{failures[0]}")
    pairs = list(M.dest_cases((kind,), (geo,)))
    want = [M.dest_legality(c, d) for c, d in pairs]
    assert M.NA not in want and len(pairs) == 2 * sum(c.out == "bytes" and v != M.NA for c, v in
                                                       ((c, M.legality(c)) for c in M.cases((kind,), (geo,))))
    assert legal == sum(v is None for v in want) > 0 and refused == sum(v is not None for v in want) > 0
    # what the context reported, counted: every (dest, route) pair the rules predict for this geometry; where a fused plan
    # exists that is every pair the kind can reach -- all four for 8-bit samples, both routes of pitched rows for wide ones
    predicted = collections.Counter((d, M.predict_dest(c, d)) for (c, d), v in zip(pairs, want) if v is None)
    assert seen == predicted, (seen, predicted)
    k = M.KINDS[kind]
    if geo in ("down", "up", "wideK", "strips"):
        assert set(seen) == M.dest_pairs(kind) and len(seen) == (2 if k.bps != 1 and k.channels > 1 else 4), seen
        assert leaves == {leaf for leaf in M.DEST_LEAVES if kind in M.LEAVES[leaf]}, leaves
    else:   # no fused plan without a box: the pass kernels, the gather and the copies, every one of them unpacked
        assert leaves >= {leaf for leaf in M.UNPACKS if kind in M.LEAVES[leaf]}, leaves
