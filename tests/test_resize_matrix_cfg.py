"""CPU-only checks that keep tests/resize_matrix_cfg.py honest: its legality rules agree with the host validators both ways and
with the error code, the planner facts the geometries were chosen for still hold, every leaf of the dispatcher is reached by a
legal case of every kind that can reach it, the library's own route decision (rs_route, run on the host by
tests/native/resize_route_check.hip) is the prediction for every legal case, and the composition that makes the expected arrays
reproduces the committed Pillow fixtures.  The destination dimension has the same checks: DEST_RULES against the validators,
rs_route's destination route and fused instance against predict_dest() / predict_dest_main() for every legal pair, every
(dest, route) pair and every leaf of a destination reached, expected_dest() between its sentinels; and the tight buffers of the
host walk are what the header says.  No GPU needed."""
import collections
import ctypes
import functools
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import lanczos_hls_amd as L
import resize_filters_model as F
import resize_matrix_cfg as M
import resize_tensor16_model as T16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_DUMMY = (ctypes.c_int32 * 8)()   # a non-NULL, aligned address for the pointers the validators only test


def _gen(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _view(case):
    o = M.OUTPUTS[case.out]
    return L.tensor_view(ctypes.addressof(_DUMMY), M.tensor_strides(case), o.elem, M.out_channels(case), o.flip if o.mapped else 0,
                         ctypes.addressof(_DUMMY) if o.mapped else None)


@functools.lru_cache(maxsize=None)
def _validators(kind, geo, filt, opt, win, out, src):
    """(the code of the first host validator that refuses, in the order the entries call them; the plan's `fused`)"""
    case = M.Case(kind, geo, filt, opt, win, out, src, L.RESIZE_AUTO)
    o = M.OUTPUTS[out]
    lib, d = L._lib(), M.desc_of(case)
    window = M.window_of(case)
    rc = lib.lanczos_resize_validate(ctypes.byref(d))
    if rc == L.OK and o.crop:
        cr = L.resize_crops(*M.crop_size(geo), ctypes.addressof(_DUMMY))
        rc = lib.lanczos_resize_crops_validate(ctypes.byref(d), ctypes.byref(cr))
        if rc == L.OK:
            rc = lib.lanczos_resize_tensor_crops_validate(ctypes.byref(d), ctypes.byref(cr), ctypes.byref(_view(case)))
    elif rc == L.OK and o.elem:
        wref = ctypes.byref(L.resize_window(d, window)) if window else None
        rc = lib.lanczos_resize_tensor_view_validate(ctypes.byref(d), wref, ctypes.byref(_view(case)))
        if not o.mapped:   # the plain tensor validators say the same
            t = (L.tensor_out if o.elem == 4 else L.tensor16_out)(ctypes.addressof(_DUMMY), M.tensor_strides(case))
            fn = {(4, False): lib.lanczos_resize_tensor_validate, (2, False): lib.lanczos_resize_tensor16_validate,
                  (4, True): lib.lanczos_resize_tensor_window_validate, (2, True): lib.lanczos_resize_tensor16_window_validate}
            args = (ctypes.byref(d), wref, ctypes.byref(t)) if window else (ctypes.byref(d), ctypes.byref(t))
            assert fn[o.elem, bool(window)](*args) == rc, case
    if rc == L.OK and src != "none":
        rc = lib.lanczos_resize_source_validate(ctypes.byref(d), ctypes.byref(M.source_struct(case)))
    fused = False
    if rc == L.OK:
        p = L.ResizePlanEx()
        opts = L._opts_ref(d, M.box_of(case), M.gap_of(case), None)
        if o.crop:
            cr = L.resize_crops(*M.crop_size(geo), ctypes.addressof(_DUMMY))
            rc = lib.lanczos_resize_crops_plan_host(ctypes.byref(d), opts, ctypes.byref(cr), M.FRAMES, ctypes.byref(p))
        else:
            wref = ctypes.byref(L.resize_window(d, window)) if window else None
            rc = lib.lanczos_resize_window_plan_host(ctypes.byref(d), opts, wref, M.FRAMES, ctypes.byref(p))
        fused = bool(p.inner.fused)
    return rc, fused


def test_the_legality_rules_are_the_validators():
    """every case of the product that is a request: the rules refuse it exactly where a validator does, with its code"""
    verdicts = collections.Counter()
    for case in M.cases():
        said = M.legality(case)
        verdicts[said] += 1
        if said == M.NA:
            continue
        rc, fused = _validators(*case[:7])
        if rc == L.OK and case.force == L.RESIZE_FUSED and not fused:
            rc = L.ERR_UNSUPPORTED
        assert (said or L.OK) == rc, (M.describe(case), said, rc)
    assert set(verdicts) == {None, M.NA, L.ERR_BAD_ARG, L.ERR_UNSUPPORTED}
    assert verdicts[None] > 40000 and verdicts[L.ERR_UNSUPPORTED] > verdicts[L.ERR_BAD_ARG] > 1000, verdicts
    # what NA stands for: one plane is a pitched source to the validator, and the Python entry refuses a window with crops
    c = M.Case("u8x1", "down", "lanczos", "none", "whole", "bytes", "planar", L.RESIZE_AUTO)
    d = M.desc_of(c)
    s = L.ResizeSource()
    s.row_stride, s.chan_stride, s.pix_stride = 64, 64 * 47, 1
    assert M.legality(c) == M.NA and L._lib().lanczos_resize_source_validate(ctypes.byref(d), ctypes.byref(s)) == L.OK
    assert M.legality(c._replace(out="f32crop", src="none", win="sub")) == M.NA


def test_the_rules_name_each_reason():
    """every rule decides at least one case of the product, except the one no value of the output dimension can break"""
    hit = collections.Counter()
    for case in M.cases():
        k, o = M.KINDS[case.kind], M.OUTPUTS[case.out]
        for name, holds, _ in M.RULES:
            if holds(case, k, o):
                hit[name] += 1
                break
    assert [n for n, _, _ in M.RULES if not hit[n]] == ["crops need a tensor output"], hit


def _p(kind, geo, filt, opt="none", where="whole"):
    return M.plan(M.Case(kind, geo, filt, opt, "whole", "bytes", "none", L.RESIZE_AUTO), where)


def test_plan_facts():
    """what the geometries were chosen for, asked of the planners: a planner change that empties a leaf fails here"""
    for kind in M.KINDS:
        for filt, ks in (("lanczos", (11, 7, 13)), ("bicubic", (9, 5, None))):
            down, up, strips = (_p(kind, g, filt) for g in ("down", "up", "strips"))
            assert down.fused and up.fused and strips.fused, (kind, filt)
            assert down.K == ks[0] and up.K == ks[1] and up.chunks == 2, (kind, filt, down.K, up.K, up.chunks)
            if ks[2]:
                assert strips.K == ks[2], (kind, strips.K)
            for g in ("down", "up", "strips"):      # the sub-window and the crop keep `fused`
                assert _p(kind, g, filt, where="sub").fused and _p(kind, g, filt, where="crop").fused, (kind, g, filt)
            for g in ("h", "v", "none"):
                assert not _p(kind, g, filt).fused, (kind, g)
            # `tall` runs both passes, vertical first: no fused plan for the whole output, the sub-window or the crop, with or
            # without a box
            for opt in ("none", "fbox", "ibox"):
                for where in ("whole", "sub", "crop"):
                    t = _p(kind, "tall", filt, opt, where)
                    assert not t.fused and t.pass_h and t.pass_v and t.reduced == (7, 750), (kind, filt, opt, where)
            assert (_p(kind, "h", filt).pass_h, _p(kind, "h", filt).pass_v) == (True, False)
            assert (_p(kind, "v", filt).pass_h, _p(kind, "v", filt).pass_v) == (False, True)
            assert (_p(kind, "none", filt).pass_h, _p(kind, "none", filt).pass_v) == (False, False)
            # the integer box keeps a one-axis request one-axis (and starts the axis of `none`); the fractional one runs both
            assert (_p(kind, "h", filt, "ibox").pass_h, _p(kind, "h", filt, "ibox").pass_v) == (True, False)
            assert (_p(kind, "v", filt, "ibox").pass_h, _p(kind, "v", filt, "ibox").pass_v) == (False, True)
            assert (_p(kind, "none", filt, "ibox").pass_h, _p(kind, "none", filt, "ibox").pass_v) == (True, False)
            for g in ("h", "v", "none"):
                assert _p(kind, g, filt, "fbox").pass_h and _p(kind, g, filt, "fbox").pass_v, (kind, g)
        assert not _p(kind, "wideK", "lanczos").fused and _p(kind, "wideK", "bicubic").fused and _p(kind, "wideK", "bicubic").K == 25
        strips = {"u8x1": 2, "u8x3": 2, "u16x3": 3, "u8x4": 5, "rgba": 5, "u16x4": 5, "f32x3": 5, "f32x4": 5}
        assert _p(kind, "strips", "lanczos").strips == strips.get(kind, 3), kind   # (one 16-bit or float channel: 128 columns)
        assert _p(kind, "strips", "lanczos", where="sub").strips > 1, kind
    for kind in ("u8x1", "u8x3", "u8x4"):           # the gap reduces wideK by 2 x 1, and what remains is fused
        g = _p(kind, "wideK", "lanczos", "gap")
        assert g.factors == (2, 1) and g.reduces and g.fused, (kind, g)
        assert not _p(kind, "up", "lanczos", "gap").reduces
        t = _p(kind, "tall", "lanczos", "gap")      # ... and `tall` by 1 x 4 to 7 x 188, which is not tall and is fused
        assert t.factors == (1, 4) and t.reduced == (7, 188) and t.fused, (kind, t)
    assert (3, 0, 58, 47) == M.box_of(M.Case("u8x3", "h", "lanczos", "ibox", "whole", "bytes", "none", 0))
    # the sub-window: odd origin, odd size, inside the output; the origins: the far corner, one to clamp, one odd and inside
    for geo, (_, _, ow, oh) in M.GEOMETRIES.items():
        w, h = M.window_size(geo)
        assert w % 2 and h % 2 and 3 + w <= ow and 5 + h <= oh, geo
        org = M.origins_of(geo)
        assert tuple(org[0]) == (ow - w, oh - h) and (org[1][0] > ow - w and org[1][1] < 0) and org[2][0] % 2 and org[2][1] % 2
        assert 0 < org[2][0] < ow - w and 0 < org[2][1] < oh - h, geo
    assert M.window_size("strips")[0] > 256


def test_every_leaf_is_reached():
    """every leaf of the written list by at least one legal case, and by every kind that can reach it -- and by no other; the
    leaves of a destination (the unpack kernels, the planar-out families) by the destination cases, and every (dest, route) pair
    by every kind that can reach it"""
    assert len(M.FUSED_FAMILIES) == len(set(M.FUSED_FAMILIES)) == 15
    names = set(M.FUSED_FAMILIES) | set(M.MAINS) | set(M.ALPHA_LEAVES) | {"reduce"} | set(M.PACKS) | set(M.FOLLOWERS)
    assert len(names) + len(M.DEST_LEAVES) == len(M.LEAVES) and not names & set(M.DEST_LEAVES)
    names |= set(M.DEST_LEAVES)
    assert names == set(M.LEAVES) and len(M.MAINS) == 8 and len(M.PACKS) == 3 and len(M.FOLLOWERS) == 4
    assert len(M.UNPACKS) == 3 and M.PLANAR_OUT_FAMILIES == ("fused<1, 0 + planar_out>", "fused<1, 0 + planar + planar_out>")
    reached = collections.defaultdict(set)
    reports = set()
    for case in M.cases():
        if M.legality(case) is None:
            pred = M.predict(case)
            for leaf in M.leaves_of(pred):
                reached[leaf].add(case.kind)
            reports.add((pred.last_kernel, pred.tensor_route, pred.source_route))
    assert not set(reached) & set(M.DEST_LEAVES)     # no case without a destination reaches a leaf of one
    pairs = collections.defaultdict(set)
    dest_mains = collections.defaultdict(set)
    for case, dest in M.dest_cases():
        if M.dest_legality(case, dest) is None:
            main, unpack = M.predict_dest_main(case, dest)
            for leaf in (main, unpack):
                if leaf in M.DEST_LEAVES:
                    reached[leaf].add(case.kind)
            dest_mains[case.kind].add(main)
            pairs[case.kind].add((dest, M.predict_dest(case, dest)))
    for leaf, kinds in M.LEAVES.items():
        assert reached[leaf] == set(kinds), (leaf, sorted(reached[leaf]), sorted(kinds))
    assert set(reached) == set(M.LEAVES)
    for kind, k in M.KINDS.items():
        assert pairs[kind] == M.dest_pairs(kind), (kind, pairs[kind])
        assert len(M.dest_pairs(kind)) == (2 if k.bps != 1 and k.channels > 1 else 4)
        # every main kernel that stores bytes also stores them in front of a destination
        assert dest_mains[kind] - set(M.PLANAR_OUT_FAMILIES) == {m for m in M.MAINS + M.FUSED_FAMILIES
                                                                 if m != "none" and kind in M.LEAVES[m] and
                                                                 (m in M.MAINS or m in (M.family(k.bps, 0), M.family(1, 32), M.family(1, 64)))}, kind
    assert {r[0] for r in reports} == {L.KERNEL_RESIZE_FUSED, L.KERNEL_RESIZE_TWO_PASS, L.KERNEL_RESIZE_NEAREST}
    assert {r[1] for r in reports} == {0, L.TENSOR_FUSED, L.TENSOR_CONVERTED}
    assert {r[2] for r in reports} == {None, L.SOURCE_DIRECT, L.SOURCE_PACKED}


def test_the_dispatcher_cases_the_issue_names():
    """the cases of the route decision (rs_route) that are easy to get wrong, spelled out"""
    c = M.Case("u8x3", "down", "lanczos", "none", "whole", "bytes", "pitched", L.RESIZE_AUTO)
    assert M.predict(c)[:] == (M.family(1, 0), (), False, None, None, L.KERNEL_RESIZE_FUSED, 0, L.SOURCE_DIRECT)
    for force in (L.RESIZE_CONVERT, L.RESIZE_TWO_PASS):   # both drop the source to PACKED, also for byte output
        p = M.predict(c._replace(force=force))
        assert (p.pack, p.source_route) == ("pack_rows", L.SOURCE_PACKED), force
    assert M.predict(c._replace(force=L.RESIZE_CONVERT)).main == M.family(1, 0)
    assert M.predict(c._replace(src="none")).source_route is None
    p = M.predict(c._replace(src="planar", out="bf16crop_hwc"))                # planar with crops is PACKED
    assert (p.main, p.pack, p.source_route) == (M.family(1, 26), "pack<3>", L.SOURCE_PACKED)
    p = M.predict(c._replace(kind="rgba", out="bf16crop_hwc"))                 # ... and so is row-shift with crops
    assert (p.main, p.pack, p.source_route) == (M.family(1, 26), "pack_rows", L.SOURCE_PACKED)
    assert M.predict(c._replace(kind="rgba")).main == M.family(1, 64)
    p = M.predict(c._replace(geo="wideK", opt="gap", src="planar"))            # a gap packs first and reduces from the packed frames
    assert (p.reduce, p.pack, p.source_route, p.main) == (True, "pack<3>", L.SOURCE_PACKED, M.family(1, 0))
    p = M.predict(c._replace(out="f32crop", force=L.RESIZE_CONVERT))           # crops_gather replans the whole output
    assert (p.main, p.follower, p.tensor_route, p.source_route) == (M.family(1, 0), "crops_scratch", L.TENSOR_CONVERTED, L.SOURCE_PACKED)
    p = M.predict(c._replace(geo="none", out="f32crop", src="none"))
    assert (p.main, p.follower, p.last_kernel) == ("none", "crops_direct", L.KERNEL_RESIZE_TWO_PASS)
    p = M.predict(c._replace(kind="rgba", geo="v", win="sub", out="bf16map_hwc", filt="bicubic"))
    assert (p.main, p.alpha, p.pack, p.follower) == ("pass_v_only", ("v_alpha<true>",), "pack_rows", "to_tensor_map")
    p = M.predict(c._replace(kind="f32x3", geo="v", win="sub", force=L.RESIZE_TWO_PASS))
    assert (p.main, p.pack, p.source_route) == ("pass_v_only", "pack_rows", L.SOURCE_PACKED)
    # a frame Pillow resizes vertical first: the pass kernels in that order, whatever else the request asks for
    t = c._replace(geo="tall")
    assert M.legality(t._replace(force=L.RESIZE_FUSED)) == L.ERR_UNSUPPORTED and M.legality(t) is None
    assert M.predict(t._replace(kind="rgba"))[:] == ("v_first", ("v_alpha_first", "h_alpha_last"), False, "pack_rows", None,
                                                     L.KERNEL_RESIZE_TWO_PASS, 0, L.SOURCE_PACKED)
    assert M.predict(t._replace(src="planar", out="f32crop"))[:] == ("v_first", (), False, "pack<3>", "crops_scratch",
                                                                     L.KERNEL_RESIZE_TWO_PASS, L.TENSOR_CONVERTED, L.SOURCE_PACKED)
    assert M.predict(t._replace(src="none", win="sub", out="bf16map_hwc")).follower == "to_tensor_map"
    assert M.predict(t._replace(src="none", filt="nearest")).main == "nearest"
    assert M.predict(t._replace(src="none", opt="gap")).main == M.family(1, 0)     # reduced to 7 x 188, which is not tall


@pytest.fixture(scope="module")
def route_exe(tmp_path_factory):
    """tests/native/resize_route_check.hip with the library's host-only translation unit: no library load, no kernel, no GPU"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "lanczos-hls_amd", "csrc")
    path = str(tmp_path_factory.mktemp("resize_route") / "resize_route_check")
    subprocess.run([hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function", "-I" + csrc,
                    os.path.join(ROOT, "tests", "native", "resize_route_check.hip"), os.path.join(csrc, "lanczos_resize_route.cpp"),
                    "-o", path], check=True, timeout=600)
    return path


Route = collections.namedtuple("Route", "err reduce pack main bps flags follower tensor_route source_route dest_route last_kernel")


def _routes(exe, tmp_path, lines):
    """rs_route's answer to every line, from one run of the program, and the (bps, flags) of every entry of
    LZ_RS_FUSED_INSTANCES the program was compiled with; every fused route names one of them"""
    path = str(tmp_path / "requests.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.split("\n")
    assert out[len(lines)] == "done %d" % len(lines), out[-3:]
    inst = [text.split() for text in out[len(lines) + 1:] if text]
    assert inst and [w[:2] for w in inst] == [["INSTANCE", str(i)] for i in range(len(inst))], inst   # the indices are dense
    listed = {(int(w[2]), int(w[3])) for w in inst}
    assert len(listed) == len(inst), inst   # and no entry is there twice
    routes = []
    for i, text in enumerate(out[:len(lines)]):
        w = text.split()
        assert w[0] == "ROUTE" and int(w[1]) == i, text
        rt = Route(*(v if k in (5, 8) else int(v) for k, v in enumerate(w) if k >= 2))
        assert rt.main != "fused" or (rt.bps, rt.flags) in listed, (lines[i], rt, sorted(listed))
        routes.append(rt)
    return routes, listed


@pytest.fixture(scope="module")
def product_routes(route_exe, tmp_path_factory):
    """the walk over the cross product: its legal cases, those refused only because FUSED is forced, rs_route's answer to each
    (legal ones first), and the instance list"""
    legal, forced = [], []
    for case in M.cases():
        said = M.legality(case)
        if said is None:
            legal.append(case)
        elif said == L.ERR_UNSUPPORTED and case.force == L.RESIZE_FUSED and M.legality(case._replace(force=L.RESIZE_AUTO)) is None:
            forced.append(case)
    routes, listed = _routes(route_exe, tmp_path_factory.mktemp("product"), [M.route_line(c) for c in legal + forced])
    return legal, forced, routes, listed


@pytest.fixture(scope="module")
def dest_routes(route_exe, tmp_path_factory):
    """the walk over the destinations: every legal (case, dest) pair, rs_route's answer to each, and the instance list"""
    todo = [(case, dest) for case, dest in M.dest_cases() if M.dest_legality(case, dest) is None]
    routes, listed = _routes(route_exe, tmp_path_factory.mktemp("dest"), [M.route_line(c, dest) for c, dest in todo])
    return todo, routes, listed


def test_the_route_is_the_prediction(product_routes):
    """rs_route (csrc/lanczos_resize_route.cpp), asked on the host for every legal case of the product, launches what predict()
    says; a case refused only because FUSED is forced is refused by the route, with that code"""
    legal, forced, routes, _ = product_routes
    assert len(legal) > 40000 and forced
    compared = 0
    for case, rt in zip(legal, routes):
        p = M.predict(case)
        assert rt.err == L.OK, (M.describe(case), rt)
        main = M.family(rt.bps, rt.flags) if rt.main == "fused" else rt.main
        follower = {"none": None, "to_tensor": "to_tensor"}.get(rt.follower, rt.follower)
        want_follower = "to_tensor" if p.follower == "to_tensor_map" else p.follower
        assert (main, bool(rt.reduce), bool(rt.pack), follower, rt.last_kernel, rt.tensor_route, rt.source_route or None) == \
            (p.main, p.reduce, p.pack is not None, want_follower, p.last_kernel, p.tensor_route, p.source_route), (M.describe(case), rt, p)
        assert rt.dest_route == 0, (M.describe(case), rt)
        compared += 1
    assert compared == len(legal)
    for case, rt in zip(forced, routes[len(legal):]):
        assert rt.err == L.ERR_UNSUPPORTED, (M.describe(case), rt)


@functools.lru_cache(maxsize=None)
def _dest_validator(kind, geo, win, dest):
    case = M.Case(kind, geo, "lanczos", "none", win, "bytes", "none", L.RESIZE_AUTO)
    d = M.desc_of(case)
    window = M.window_of(case)
    s = M.dest_struct(case, dest)
    return L._lib().lanczos_resize_dest_validate(ctypes.byref(d), ctypes.byref(L.resize_window(d, window)) if window else None,
                                                 ctypes.byref(s))


def test_the_destination_rules_are_the_validators():
    """every (case, dest) pair: DEST_RULES refuse it exactly where the validators do in the order lanczos_resize_dest_device calls
    them (descriptor, source, destination, then the options and the plan), with that code; and nothing but the one new row tells
    a pair from its case"""
    verdicts = collections.Counter()
    for case, dest in M.dest_cases():
        said = M.dest_legality(case, dest)
        verdicts[said] += 1
        assert said != M.NA
        lib, d = L._lib(), M.desc_of(case)
        rc = lib.lanczos_resize_validate(ctypes.byref(d))
        if rc == L.OK and case.src != "none":
            rc = lib.lanczos_resize_source_validate(ctypes.byref(d), ctypes.byref(M.source_struct(case)))
        if rc == L.OK:
            rc = _dest_validator(case.kind, case.geo, case.win, dest)
        if rc == L.OK:
            rc, fused = _validators(*case[:7])
            if rc == L.OK and case.force == L.RESIZE_FUSED and not fused:
                rc = L.ERR_UNSUPPORTED
        assert (said or L.OK) == rc, (M.describe(case), dest, said, rc)
        k = M.KINDS[case.kind]
        wide_planes = dest == "planar" and k.bps != 1 and k.channels > 1
        if not wide_planes:
            assert said == M.legality(case), (M.describe(case), dest)
        elif M.legality(case) is None:
            assert said == L.ERR_UNSUPPORTED, (M.describe(case), dest)
    bytes_out = [c for c in M.cases() if c.out == "bytes" and M.legality(c) != M.NA]
    assert sum(verdicts.values()) == 2 * len(bytes_out)
    assert verdicts[None] > 19000 and verdicts[L.ERR_UNSUPPORTED] > verdicts[L.ERR_BAD_ARG] > 1000, verdicts
    names = [n for n, _, _ in M.DEST_RULES]
    assert names.index("planar destinations are 8-bit only") == names.index("planar sources are 8-bit only") + 1
    # one plane is the pitched shape, of wide samples too; a pitch off a dword wherever the sample width leaves one
    for kind, k in M.KINDS.items():
        c = M.Case(kind, "down", "lanczos", "none", "sub", "bytes", "none", L.RESIZE_AUTO)
        assert M.dest_legality(c, "planar") == (L.ERR_UNSUPPORTED if k.bps != 1 and k.channels > 1 else None)
        assert M.dest_shape(c, "planar") == ("planar" if k.channels > 1 else "interleaved")
        assert (M.dest_strides(c, "pitched")[0] % 4 != 0) == (k.bps != 4), kind


def test_the_destination_route(dest_routes):
    """every legal (case, dest) pair of every kind on every geometry, into pitched rows and -- where the validator takes them --
    into planes: the route's destination is predict_dest's, the fused instance is predict_dest_main's (a planar-out one exactly
    where planes are stored DIRECT), and nothing in front of the store differs from the case without a destination"""
    todo, routes, _ = dest_routes
    assert len(todo) > 19000 and {dest for _, dest in todo} == set(M.DESTS)
    seen = collections.Counter()
    for (case, dest), rt in zip(todo, routes):
        want = M.predict_dest(case, dest)
        assert rt.err == L.OK and rt.dest_route == want, (M.describe(case), dest, rt, want)
        planar_out = rt.main == "fused" and bool(rt.flags & M.PLANAR_OUT)
        assert planar_out == (M.dest_shape(case, dest) == "planar" and want == L.DEST_DIRECT), (M.describe(case), dest, rt)
        main = M.family(rt.bps, rt.flags) if rt.main == "fused" else rt.main
        assert main == M.predict_dest_main(case, dest)[0], (M.describe(case), dest, rt)
        p = M.predict(case)   # a destination changes nothing in front of the store
        assert (rt.main == "fused", bool(rt.reduce), bool(rt.pack), rt.source_route or None, rt.last_kernel, rt.tensor_route) == \
            (p.main.startswith("fused<"), p.reduce, p.pack is not None, p.source_route, p.last_kernel, 0), (M.describe(case), dest, rt, p)
        seen[case.kind, dest, want] += 1
    for kind in M.KINDS:
        assert {(d, r) for k, d, r in seen if k == kind} == M.dest_pairs(kind), kind
    assert min(seen.values()) > 50, seen


def test_every_listed_instance_is_named(route_exe, tmp_path, product_routes, dest_routes):
    """every entry of LZ_RS_FUSED_INSTANCES is the instance of at least one route: of the two walks, and -- the matrix has no
    lanczos_tensor_norm output -- of the smallest case of that kind for the kRsNorm entries: three 16-bit or float channels,
    halved, into tight CHW float32 elements"""
    listed = product_routes[3]
    assert dest_routes[2] == listed
    walked = {(rt.bps, rt.flags) for rt in product_routes[2] + dest_routes[1] if rt.main == "fused"}
    lines = []
    for kind in ("u16x3", "f32x3"):
        case = M.Case(kind, "down", "lanczos", "none", "whole", "bytes", "none", L.RESIZE_AUTO)
        f = M.route_line(case).split()
        w, h = M.frame_size(case)
        f[19:25] = [str(v) for v in (4, 2, w * h, w, 1, 3)]   # elem, mapped = 2: a norm request, the strides, out_channels
        lines.append(" ".join(f))
    norm, again = _routes(route_exe, tmp_path, lines)
    assert again == listed
    assert [(rt.err, rt.main, rt.bps, rt.flags, rt.tensor_route) for rt in norm] == \
        [(L.OK, "fused", 2, M.NORM, L.TENSOR_FUSED), (L.OK, "fused", 4, M.NORM, L.TENSOR_FUSED)], norm
    named = walked | {(rt.bps, rt.flags) for rt in norm}
    assert named == listed, (sorted(listed - named), sorted(named - listed))
    # the cross product alone reaches every entry but the kRsNorm ones
    assert listed - walked == {i for i in listed if i[1] == M.NORM}, sorted(listed - walked)


def test_expected_dest_arrays_are_between_sentinels():
    """the guard, the gap between the frames, row padding and plane padding of expected_dest hold the sentinel, the named bytes are
    frames * w * h * C * bps of them and hold the frames of expected(); the buffer ends GUARD elements behind the last named byte"""
    import resize_dest_model as DM
    for kind, geo, win in (("rgba", "down", "whole"), ("u8x3", "strips", "sub"), ("u8x1", "tall", "sub"), ("u16x3", "down", "sub"),
                           ("u16x1", "up", "whole"), ("f32x4", "wideK", "whole"), ("f32x1", "h", "sub")):
        k = M.KINDS[kind]
        case = M.Case(kind, geo, "bicubic", "fbox", win, "bytes", "none", L.RESIZE_AUTO)
        w, h = M.frame_size(case)
        shape = (M.FRAMES, h, w, k.channels)
        _, n, fs, _ = M.out_geometry(case)
        plain = M.expected(case)
        frames = np.stack([plain[M.GUARD + f * fs:M.GUARD + f * fs + n].reshape(h, w, k.channels) for f in range(M.FRAMES)])
        for dest in M.DESTS:
            if M.dest_legality(case, dest) is not None:
                continue
            t = M.dest_layout(case, dest)
            want = M.expected_dest(case, dest)
            named = DM.named_mask(t, shape, k.bps)
            assert int(named.sum()) == M.FRAMES * w * h * k.channels * k.bps
            assert want.dtype == np.uint8 and want.size == t.buf.size and (want[~named] == M.SENTINEL).all()
            assert (t.buf == M.SENTINEL).all()
            assert np.array_equal(DM.unpack(t, shape, frames.dtype, buf=want), frames)
            # the layout: residue, frame stride, guards, a buffer that ends behind the last named byte
            g = M.GUARD * k.bps
            assert t.at == g + (3 * k.bps) % 4 and t.frame_stride == t.extent + M.FRAME_GAP * k.bps
            first, last = int(np.argmax(named)), named.size - 1 - int(np.argmax(named[::-1]))
            assert first == t.at and last + 1 + g == named.size and t.at + 2 * t.frame_stride + t.named == last + 1
            assert t.named < t.extent                       # the padding behind the last row is not in the buffer
            for f in range(M.FRAMES - 1):
                assert not named[t.at + f * t.frame_stride + t.named:t.at + (f + 1) * t.frame_stride].any()
            rows = named[t.at:t.at + t.row_stride]
            assert rows[:w * k.bps].all() and not rows.all()   # row padding
            if t.layout == "planar":
                assert t.chan_stride > (h - 1) * t.row_stride + w + 3 and not named[t.at + t.chan_stride - 5:t.at + t.chan_stride].any()
            # the tight form of the host entry: the same frames, the layout's own extent apart, as long as the header says
            tt = M.dest_layout(case, dest, tight=True)
            host = M.expected_host(case, dest)
            assert (tt.at, tt.frame_stride) == (0, tt.extent) and host.size == M.host_out_bytes(case, dest) == 2 * tt.extent + tt.named
            assert np.array_equal(DM.unpack(tt, shape, frames.dtype, buf=host), frames)
            assert (host[~DM.named_mask(tt, shape, k.bps)] == M.SENTINEL).all()


def test_expected_host_arrays():
    """the tight buffers of the host walk: as long as the header says, the frames of expected() one extent apart, the sentinel
    wherever the strides name nothing; the origins of the host walk are those of the device walk after the clamp"""
    for out in M.OUTPUTS:
        case = M.Case("rgba", "down", "bicubic", "fbox", "whole", out, "none", L.RESIZE_AUTO)
        item, n, fs, _ = M.out_geometry(case)
        want, host = M.expected(case).view(np.uint8), M.expected_host(case)
        assert host.dtype == np.uint8 and host.size == M.host_out_bytes(case) == M.FRAMES * n * item
        for f in range(M.FRAMES):
            assert np.array_equal(host[f * n * item:(f + 1) * n * item], want[(M.GUARD + f * fs) * item:(M.GUARD + f * fs + n) * item])
        if M.OUTPUTS[out].layout == "chwp":
            assert (host.reshape(-1, item) == M.SENTINEL).all(axis=1).sum() > M.FRAMES * 5
    for geo, (_, _, ow, oh) in M.GEOMETRIES.items():
        w, h = M.crop_size(geo)
        org, inside = M.origins_of(geo), M.host_origins_of(geo)
        assert inside.dtype == np.int32 and (inside >= 0).all() and (inside[:, 0] <= ow - w).all() and (inside[:, 1] <= oh - h).all()
        assert tuple(inside[1]) == (ow - w, 0) and np.array_equal(inside[[0, 2]], org[[0, 2]])
    for kind, k in M.KINDS.items():
        for src in ("pitched", "planar"):
            if src == "planar" and (k.bps != 1 or k.channels == 1):
                continue
            s = M.host_source_of(kind, "down", src)
            assert s.frame_stride == s.extent and s.at % 4 == 0
            assert (s.row_stride, s.chan_stride, s.pix_stride) == M.source_strides(kind, "down", src)
            assert np.array_equal(M.SM.unpack(s, M.frames_of(kind, "down").shape, k.dtype).view(np.uint8),
                                  M.frames_of(kind, "down").view(np.uint8))


def test_the_sources_name_what_the_issue_asks():
    for kind, k in M.KINDS.items():
        s = M.source_of(kind, "down", "pitched")
        assert s.row_stride == (61 * k.channels + 7) * k.bps and s.at % 4 == (3 * k.bps) % 4 and s.frame_stride == s.extent + k.bps
        assert np.array_equal(M.SM.unpack(s, M.frames_of(kind, "down").shape, k.dtype).view(np.uint8),
                              M.frames_of(kind, "down").view(np.uint8))
        assert M.source_struct(M.Case(kind, "down", "lanczos", "none", "whole", "bytes", "pitched", 0), s).row_stride == s.row_stride
        if k.bps == 1 and k.channels > 1:
            s = M.source_of(kind, "down", "planar")
            assert s.row_stride % 2 and s.chan_stride % 2 and s.frame_stride > s.extent
    assert M.source_of("rgba", "down", "pitched").row_stride % 4          # the row-shift family
    x = M.frames_of("f32x3", "down")
    assert np.isinf(x).sum() == np.isnan(x).sum() == M.FRAMES and ((x != 0) & (np.abs(x) < 1e-38)).sum() == M.FRAMES


# ---- the composition against Pillow's fixtures ------------------------------------------------------------------------

def _samples(cut_shape, dtype, full, **kw):
    f = full.shape[0]
    n = int(np.prod(cut_shape))
    word = {1: np.uint8, 2: np.uint16, 4: np.uint32}[np.dtype(dtype).itemsize]
    out = np.zeros(f * (n + 3), dtype=word)
    assert M.compose(full, base=0, frame_stride=n + 3, out=out, **kw) == f * n
    return np.stack([out[k * (n + 3):k * (n + 3) + n].view(dtype).reshape(cut_shape) for k in range(f)])


def test_the_composition_reproduces_pillow():
    """resize_pillow.npz and resize_pillow_alpha.npz (the whole output), resize_pillow_window.npz (the window) and
    resize_pillow_crops.npz (crops, flips) for the filters the matrix uses: M.compose over the model's full bytes gives Pillow's"""
    seen = 0
    for fixture, alpha in (("resize_pillow.npz", False), ("resize_pillow_alpha.npz", True)):
        z = np.load(os.path.join(GOLDEN, fixture))
        for name in sorted(k[:-3] for k in z.files if k.endswith("_in")):
            img, out = z[f"{name}_in"], z[f"{name}_out"]
            img3, out3 = (img[..., None], out[..., None]) if img.ndim == 2 else (img, out)
            full = F.resize(img3[None], F.LANCZOS, out3.shape[1], out3.shape[0], alpha=alpha)
            assert np.array_equal(_samples(out3.shape, np.uint8, full)[0], out3), (fixture, name)
            seen += 1
    for name, (case, img, want) in _gen("make_resize_window_golden").load().items():
        _, mode, filt, _, _, ow, oh, box, gap, window = case
        if filt not in M.FILTERS:
            continue
        x = img[None, ..., None] if img.ndim == 2 else img[None]
        full = F.resize(x, F.NAMES.index(filt), ow, oh, box, gap, alpha=mode == "RGBA")
        w3 = want[..., None] if want.ndim == 2 else want
        got = _samples(w3.shape, w3.dtype, full, window=window)[0]
        assert F.same(got, w3), name
        seen += 1
    for name, (case, imgs, origins, flips, want) in _gen("make_resize_crops_golden").load().items():
        _, mode, filt, _, _, ow, oh, box, gap, (w, h) = case
        if filt not in M.FILTERS:
            continue
        x = imgs[..., None] if imgs.ndim == 3 else imgs
        c = x.shape[-1]
        full = F.resize(x, F.NAMES.index(filt), ow, oh, box, gap, alpha=mode == "RGBA")
        st = M.V.strides("hwc", w, h, c)
        n = M.V.extent(w, h, c, st)
        out = np.zeros(len(x) * n, dtype=np.uint16)
        assert M.compose(full, crop=(w, h), origins=origins, lut=T16.identity_lut16(c), src=tuple(range(c)), flips=flips, strides=st,
                         base=0, frame_stride=n, out=out) == out.size
        out = out.reshape(len(x), h, w, c)
        assert np.array_equal(out >> 8, np.broadcast_to(np.arange(c, dtype=np.uint16), out.shape)), name
        w4 = want[..., None] if want.ndim == 3 else want
        assert np.array_equal((out & 255).astype(np.uint8), w4), name
        seen += 1
    assert seen >= 40, seen


def test_expected_arrays_are_between_sentinels():
    """the guard in front, the gap between the frames and the padding inside a padded tensor frame hold the sentinel"""
    for out in M.OUTPUTS:
        case = M.Case("rgba", "down", "bicubic", "fbox", "whole", out, "none", L.RESIZE_AUTO)
        item, n, fs, total = M.out_geometry(case)
        want = M.expected(case)
        sent = int(np.full(1, M.SENTINEL, np.uint8).repeat(item).view(want.dtype)[0])
        assert want.size == total and fs == n + 7 and (want[:M.GUARD] == sent).all() and (want[-M.GUARD:] == sent).all()
        for f in range(M.FRAMES - 1):
            assert (want[M.GUARD + f * fs + n:M.GUARD + (f + 1) * fs] == sent).all()
        named = (want[M.GUARD:M.GUARD + n] != sent).sum()
        w, h = M.frame_size(case)
        if M.OUTPUTS[out].layout == "chwp":
            assert named == len(M.out_channels(case)) * w * h < n
        assert M.first_difference(want.copy(), want, False) is None
        bad = want.copy()
        bad[M.GUARD + 5] ^= 1
        assert M.first_difference(bad, want, False)[0] == 5
