"""The jobs of the concurrency tests (tests/test_concurrency_gpu.py, tests/concurrency_child.py): small requests, one per launch
route of the library, each with the entry point it goes through, the report it must leave on its context and the CPU model that
makes its expected bytes.  No GPU is needed to import this module or to compute an expected array (tests/test_concurrency_cfg.py).

TABLE    one job per route; every host thread of the per-thread test runs all of them on a context and a stream of its own, and
         the two-stream tests take their upscale jobs from it.  Frames are the smallest of the existing frame tables
         (march_table_cfg, fast_cfg, ratp_cfg, the resize modules' multi-strip shapes) at which the route is still taken with
         more than one workgroup; nothing is larger than 256 x 160 pixels.
SHARED   the entries that hold context scratch, in several sizes: four threads run them on ONE context and ONE stream.  The
         context is forced to the two-pass path once, before the threads start, so that a byte request uses the two-pass
         intermediate and a tensor request the converted route.  No two jobs need the same amount of any kind of scratch.
SHARED_HOST  the synchronous host entries of the resize family, which use the same scratch from the context's private stream:
         by the contract (one stream at a time per context) they follow the device entries only after the caller's stream has
         drained, so the shared test runs them in a second phase.

A job is a dict.  kind: upscale (lanczos_resample_device), planar, resize, tensor, reduce, host_resample, host_resize,
host_tensor.  report: kernel = LANCZOS_KERNEL_* (None: the entry leaves it alone), main / prefix = the route of an upscale
(launches 0 otherwise), tensor = lanczos_last_tensor_route.  check: "exact" -- bit for bit the model's bytes; "lsb1" -- within one
LSB of the oracle, lsb1_check.check, and byte equality with the same call made single-threaded in the same process."""
import numpy as np

import lanczos_hls_amd as L
import lsb1_check as LC
import oracle_lib as O
import patterns as P
import resize_box_model as MB
import resize_crops_model as MC
import resize_filters_model as FM
import resize_tensor16_model as T16
import resize_tensor_model as T32
import resize_tensor_view_model as TV

ROUTES = ("march-2x-exact", "march-2x-lsb1", "march-3x-exact", "march-3x-lsb1", "tile-pitch-off-16", "ratp-3/2", "rat", "generic",
          "hls", "prefix-behind", "prefix-front", "resize-fused", "resize-two-pass", "resize-alpha", "resize-u16", "resize-f32",
          "nearest", "reducing-gap", "window", "tensor-f32-fused", "tensor-f32-converted", "tensor16", "view", "crops", "reduce",
          "planar")
SCRATCH_KINDS = ("two-pass", "reduced", "tensor-bytes", "planar", "stage")

_NP = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
_MEAN, _STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _up(name, routes, w, h, c, sn, sd, a, mode, main, prefix, kernel=L.KERNEL_FAST, frames=2, rows=0, seed=0, kind="upscale"):
    return dict(name=name, routes=routes, kind=kind, w=w, h=h, c=c, sn=sn, sd=sd, a=a, mode=mode, frames=frames, rows=rows, seed=seed,
                check="lsb1" if mode == L.MODE_LSB1 else "exact",
                report=dict(kernel=kernel, main=main, prefix=prefix, tensor=0))


def _rs(name, routes, w, h, c, ow, oh, kernel, dtype="u8", alpha=False, filter="lanczos", box=None, gap=None, window=None,
        force=L.RESIZE_AUTO, frames=2, seed=0, kind="resize", **tensor):
    t = dict(tdtype=None, layout="chw", channels_out=None, flips=None, crop=None, origins=None, troute=0)
    t.update(tensor)
    return dict(name=name, routes=routes, kind=kind, w=w, h=h, c=c, ow=ow, oh=oh, dtype=dtype, alpha=alpha, filter=filter, box=box,
                gap=gap, window=window, force=force, frames=frames, seed=seed, check="exact",
                report=dict(kernel=kernel, main=0, prefix=0, tensor=t["troute"]), **t)


def _prefix_K(w, h, c, s, a):
    return L.inplace_rows(L.make_desc(w, h, c, s, 1, a, 1, L.MODE_EXACT))


MARCH, TILE, RATP, RAT, GENERIC, HLS = (L.ROUTE_MAIN_MARCH, L.ROUTE_MAIN_TILE, L.ROUTE_MAIN_RATP, L.ROUTE_MAIN_RAT,
                                        L.ROUTE_MAIN_GENERIC, L.ROUTE_MAIN_HLS)
RIDING, FRONT, BEHIND = L.ROUTE_PREFIX_RIDING, L.ROUTE_PREFIX_FRONT, L.ROUTE_PREFIX_BEHIND
FUSED, TWO_PASS, NEAREST = L.KERNEL_RESIZE_FUSED, L.KERNEL_RESIZE_TWO_PASS, L.KERNEL_RESIZE_NEAREST

TABLE = [
    # rows that are 16-byte multiples: k_march, the prefix rows riding (208 * 3 and 144 * 3 bytes)
    _up("march2-exact", ("march-2x-exact",), 208, 48, 3, 2, 1, 3, L.MODE_EXACT, MARCH, RIDING, seed=11),
    _up("march2-lsb1", ("march-2x-lsb1",), 208, 48, 3, 2, 1, 3, L.MODE_LSB1, MARCH, RIDING, seed=12),
    _up("march3-exact", ("march-3x-exact",), 144, 40, 3, 3, 1, 3, L.MODE_EXACT, MARCH, RIDING, seed=13),
    _up("march3-lsb1", ("march-3x-lsb1",), 144, 40, 3, 3, 1, 3, L.MODE_LSB1, MARCH, RIDING, seed=14),
    # 200 * 3 = 600 bytes a row, 8 off a 16-byte multiple: the tile kernel, k_prefix behind it
    _up("tile", ("tile-pitch-off-16", "prefix-behind"), 200, 40, 3, 2, 1, 3, L.MODE_LSB1, TILE, BEHIND, seed=15),
    _up("ratp", ("ratp-3/2", "prefix-behind"), 96, 60, 3, 3, 2, 3, L.MODE_EXACT, RATP, BEHIND, seed=16),
    _up("rat", ("rat", "prefix-behind"), 96, 60, 3, 5, 3, 3, L.MODE_EXACT, RAT, BEHIND, seed=17),
    # 67 * 2 * 3 = 402 bytes an output row, no dword multiple: k_generic
    _up("generic", ("generic", "prefix-behind"), 67, 40, 3, 2, 1, 3, L.MODE_EXACT, GENERIC, BEHIND, kernel=L.KERNEL_GENERIC, seed=18),
    _up("hls", ("hls",), 120, 64, 3, 2, 1, 3, L.MODE_HLS, HLS, L.ROUTE_PREFIX_NONE, kernel=L.KERNEL_HLS, seed=19),
    # a strip [0, K): no main rows, nothing to ride on -- the register-only prefix kernel in front, whatever the batch
    _up("front", ("prefix-front",), 160, 24, 3, 2, 1, 3, L.MODE_EXACT, L.ROUTE_MAIN_NONE, FRONT, rows=-1, seed=20),
    _up("planar", ("planar",), 208, 40, 3, 2, 1, 3, L.MODE_EXACT, MARCH, RIDING, seed=21, kind="planar"),
    # resizes: output widths of two or three strips of the fused kernels (256 / 64 / 128 / 128 pixels a strip)
    _rs("resize-fused", ("resize-fused",), 230, 150, 3, 300, 100, FUSED, seed=31),
    _rs("resize-two-pass", ("resize-two-pass",), 200, 120, 3, 90, 70, TWO_PASS, force=L.RESIZE_TWO_PASS, seed=32),
    _rs("resize-alpha", ("resize-alpha",), 120, 80, 4, 150, 60, FUSED, alpha=True, seed=33),
    _rs("resize-u16", ("resize-u16",), 150, 90, 3, 200, 60, FUSED, dtype="u16", seed=34),
    _rs("resize-f32", ("resize-f32",), 100, 70, 1, 160, 50, FUSED, dtype="f32", seed=35),
    _rs("nearest", ("nearest",), 130, 90, 3, 77, 51, NEAREST, filter="nearest", seed=36),
    _rs("gap", ("reducing-gap",), 256, 160, 3, 40, 25, FUSED, gap=2.0, seed=37),
    _rs("window", ("window",), 200, 120, 3, 320, 180, FUSED, window=(37, 21, 270, 100), seed=38),
    _rs("tensor-fused", ("tensor-f32-fused",), 160, 100, 3, 280, 64, FUSED, kind="tensor", tdtype="float32",
        troute=L.TENSOR_FUSED, seed=39),
    _rs("tensor-converted", ("tensor-f32-converted",), 150, 90, 3, 270, 60, FUSED, force=L.RESIZE_CONVERT, kind="tensor",
        tdtype="float32", troute=L.TENSOR_CONVERTED, seed=40),
    _rs("tensor16", ("tensor16",), 140, 90, 3, 260, 70, FUSED, kind="tensor", tdtype="bfloat16", layout="hwc",
        troute=L.TENSOR_FUSED, seed=41),
    _rs("view", ("view",), 120, 80, 4, 150, 60, FUSED, kind="tensor", tdtype="float32", channels_out=(2, 1, 0), flips=(1, 2, 3),
        frames=3, troute=L.TENSOR_FUSED, seed=42),
    _rs("crops", ("crops",), 160, 100, 3, 200, 120, FUSED, kind="tensor", tdtype="float32", crop=(96, 64),
        origins=((0, 0), (50, 30), (104, 56)), frames=3, troute=L.TENSOR_FUSED, seed=43),
    dict(name="reduce", routes=("reduce",), kind="reduce", w=250, h=150, c=3, factor=(2, 3), box=None, frames=2, seed=44, check="exact",
         report=dict(kernel=None, main=0, prefix=0, tensor=0)),
]

# one context, one stream, forced to the two-pass path: what each job holds of the context's scratch is in scratch()
SHARED = [
    _rs("two-pass-s", (), 120, 80, 3, 70, 50, TWO_PASS, frames=1, seed=51),
    _rs("two-pass-m", (), 200, 120, 3, 90, 70, TWO_PASS, seed=52),
    _rs("two-pass-l", (), 256, 160, 3, 150, 100, TWO_PASS, seed=53),
    _rs("gap-s", (), 200, 120, 3, 30, 20, TWO_PASS, gap=2.0, frames=1, seed=54),
    _rs("gap-l", (), 256, 160, 3, 40, 25, TWO_PASS, gap=2.0, seed=55),
    _rs("tensor-converted-s", (), 100, 60, 3, 140, 40, TWO_PASS, kind="tensor", tdtype="float32", frames=1,
        troute=L.TENSOR_CONVERTED, seed=56),
    _rs("tensor-converted-l", (), 160, 100, 3, 220, 70, TWO_PASS, kind="tensor", tdtype="float32", troute=L.TENSOR_CONVERTED, seed=57),
    _rs("crops-converted-s", (), 120, 80, 3, 150, 90, TWO_PASS, kind="tensor", tdtype="float32", crop=(64, 48),
        origins=((7, 5), (86, 42)), troute=L.TENSOR_CONVERTED, seed=58),
    _rs("crops-converted-l", (), 160, 100, 3, 200, 120, TWO_PASS, kind="tensor", tdtype="bfloat16", crop=(96, 64),
        origins=((0, 0), (50, 30), (104, 56)), frames=3, troute=L.TENSOR_CONVERTED, seed=59),
    _up("planar-s", (), 96, 24, 3, 2, 1, 3, L.MODE_EXACT, MARCH, RIDING, frames=1, seed=60, kind="planar"),
    _up("planar-l", (), 208, 40, 3, 2, 1, 3, L.MODE_EXACT, MARCH, RIDING, seed=61, kind="planar"),
    _up("host-resample-s", (), 200, 30, 3, 2, 1, 3, L.MODE_EXACT, TILE, BEHIND, frames=1, seed=62, kind="host_resample"),
    _up("host-resample-l", (), 144, 40, 3, 3, 1, 3, L.MODE_EXACT, MARCH, RIDING, frames=3, seed=63, kind="host_resample"),
]
SHARED_HOST = [
    _rs("host-resize-s", (), 130, 90, 3, 70, 50, TWO_PASS, frames=1, seed=71, kind="host_resize"),
    _rs("host-resize-l", (), 220, 140, 3, 120, 90, TWO_PASS, seed=72, kind="host_resize"),
    _rs("host-tensor-s", (), 110, 70, 3, 150, 50, TWO_PASS, frames=1, seed=73, kind="host_tensor", tdtype="float32",
        troute=L.TENSOR_CONVERTED),
    _rs("host-tensor-l", (), 180, 110, 3, 240, 80, TWO_PASS, seed=74, kind="host_tensor", tdtype="float32", troute=L.TENSOR_CONVERTED),
]
# what the fifth thread of the shared test writes while the others work: none of it changes a job's bytes -- every upscale job of
# SHARED is served by the specialised kernels under AUTO (its report says so), the resize force is the one the context already has
SHARED_SETTINGS = dict(force_kernel=(L.KERNEL_FAST, L.KERNEL_NONE), resize_force=L.RESIZE_TWO_PASS, timing=(True, False))

BY_NAME = {j["name"]: j for j in TABLE + SHARED + SHARED_HOST}
assert len(BY_NAME) == len(TABLE) + len(SHARED) + len(SHARED_HOST)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _rows(job):
    """(output rows, input rows) of an upscale job; rows = -1 stands for the strip [0, K) of the in-place prefix rows"""
    if not job["rows"]:
        return job["h"] * job["sn"] // job["sd"], job["h"]
    rows = _prefix_K(job["w"], job["h"], job["c"], job["sn"], job["a"]) if job["rows"] < 0 else job["rows"]
    d = L.make_desc(job["w"], job["h"], job["c"], job["sn"], job["sd"], job["a"], 1, job["mode"], 0, rows)
    r0, n = L.strip_input_rows(d, 0, rows)
    assert r0 == 0
    return rows, n


def _frames(job):
    """[F][H][W][C] of the job's sample type: noise, every other frame dark (8-bit: the integer-phase fix-ups of LSB1)"""
    f, h, w, c, s = job["frames"], job["h"], job["w"], job["c"], 1000 * job["seed"]
    dt = job.get("dtype", "u8")
    if dt == "u16":
        return np.stack([P.noise(h, w, c, seed=s + i, dtype=np.uint16) for i in range(f)])
    if dt == "f32":
        return np.stack([(P.noise(h, w, c, seed=s + i, dtype=np.uint16).astype(np.float32) / np.float32(257.0) - np.float32(100.0))
                         for i in range(f)])
    return np.stack([P.dark_noise(h, w, c, seed=s + i) if i % 2 else P.noise(h, w, c, seed=s + i) for i in range(f)])


def _out_channels(job):
    return len(job["channels_out"]) if job.get("channels_out") else job["c"]


def lut_of(job):
    dt = job["tdtype"]
    oc = _out_channels(job)
    return L.normalize_lut(oc, _MEAN[:oc], _STD[:oc], dt)


_INPUTS, _EXPECTED = {}, {}


def inputs(job):
    """name -> numpy array: what goes to the device (or into the host entry) for the job.  img is always there."""
    if job["name"] in _INPUTS:
        return _INPUTS[job["name"]]
    x = _frames(job)
    ins = {"full": x}
    k = job["kind"]
    if k in ("upscale", "host_resample"):
        ins["img"] = np.ascontiguousarray(x[:, :_rows(job)[1]])
    elif k == "planar":
        ins["img"] = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    else:
        ins["img"] = x
    if k in ("tensor", "host_tensor"):
        ins["lut"] = lut_of(job)
        if job["flips"] is not None:
            ins["flip"] = np.asarray(job["flips"], dtype=np.uint8)
        if job["origins"] is not None:
            ins["origin"] = np.asarray(job["origins"], dtype=np.int32)
    _INPUTS[job["name"]] = ins
    return ins


# ---- expected bytes -------------------------------------------------------------------------------------------------------------
def _oracle(job, img):
    h, w, c = img.shape
    cfg = O.cfg(w, h, w * job["sn"] // job["sd"], h * job["sn"] // job["sd"], c, job["a"], job["sn"], job["sd"])
    if job["mode"] == L.MODE_HLS:
        return O.hls_expected_hwc(cfg, img, 4)
    return O.expected_hwc_u8(cfg, img, 4)


def _resize_bytes(job, whole=False):
    x = inputs(job)["img"]
    y = FM.resize(x, FM.NAMES.index(job["filter"]), job["ow"], job["oh"], box=job["box"], reducing_gap=job["gap"], a=3,
                  alpha=job["alpha"])
    if job["window"] is not None and not whole:
        x0, y0, w, h = job["window"]
        y = np.ascontiguousarray(y[:, y0:y0 + h, x0:x0 + w])
    return y


def expected(job):
    """The job's output as the CPU models give it, shaped as out_spec() says.  Computed once; nothing may write into it."""
    if job["name"] in _EXPECTED:
        return _EXPECTED[job["name"]]
    k = job["kind"]
    if k in ("upscale", "host_resample", "planar"):
        rows = _rows(job)[0]
        y = np.stack([_oracle(job, f)[:rows] for f in inputs(job)["full"]])
        want = np.ascontiguousarray(y.transpose(0, 3, 1, 2)) if k == "planar" else y
    elif k in ("resize", "host_resize"):
        want = _resize_bytes(job)
    elif k in ("tensor", "host_tensor"):
        b, lut = _resize_bytes(job), inputs(job)["lut"]
        if job["crop"] is not None:
            want = MC.crops(b, lut, job["crop"][0], job["crop"][1], job["origins"], job["channels_out"], job["flips"], job["layout"])
        elif job["channels_out"] is not None or job["flips"] is not None:
            want = TV.view(b, lut, job["channels_out"], job["flips"], job["layout"])
        elif job["tdtype"] == "float32":
            want = T32.tensor(b, lut, job["layout"])
        else:
            want = T16.tensor16(b, lut, job["layout"])
    elif k == "reduce":
        want = MB.reduce(inputs(job)["img"], job["factor"], job["box"])
    else:
        raise AssertionError(k)
    want.setflags(write=False)
    _EXPECTED[job["name"]] = want
    return want


def out_spec(job):
    """(shape, numpy dtype) of the device output; tensor words are uint32 / uint16 patterns"""
    w = expected(job)
    return w.shape, w.dtype


# ---- what the library is expected to choose (checked without a GPU by tests/test_concurrency_cfg.py) --------------------------------
def resize_desc(job):
    return L.resize_desc(job["w"], job["h"], job["ow"], job["oh"], job["c"], 3, job["alpha"], 16 if job["dtype"] == "u16" else 8,
                         job["dtype"] == "f32", job["filter"])


def plan_ex(job):
    """the lanczos_resize_plan_ex of a resize or tensor job under AUTO"""
    d = resize_desc(job)
    if job["crop"] is not None:
        return L.resize_crops_plan_host(d, job["crop"], job["frames"], box=job["box"], reducing_gap=job["gap"])
    box = job["box"] if job["box"] is not None or job["gap"] is not None else (0, 0, job["w"], job["h"])
    if job["window"] is not None:
        return L.resize_window_plan_host(d, job["window"], job["frames"], box=box, reducing_gap=job["gap"])
    return L.resize_plan_host(d, job["frames"], box=box, reducing_gap=job["gap"])


def scratch(job):
    """kind -> bytes of context scratch the job needs on a context forced to the two-pass path (the blocks of rs_route,
    csrc/lanczos_resize_route.cpp, that resize_device grows, csrc/lanczos_resize.hip): what makes a block of that kind grow"""
    k, f = job["kind"], job["frames"]
    if k == "planar":
        return {"planar": f * job["w"] * job["h"] * job["c"] * (1 + job["sn"] * job["sn"])}
    if k == "host_resample":
        rows, in_rows = _rows(job)
        return {"stage": f * job["c"] * (job["w"] * in_rows + job["w"] * job["sn"] // job["sd"] * rows)}
    if k not in ("resize", "tensor", "host_resize", "host_tensor"):
        return {}
    c = job["c"]
    whole = dict(job, crop=None, window=None)   # the converted crops route resizes the whole output
    p = plan_ex(whole)
    s = {"two-pass": f * p.mid_rows * job["ow"] * c}
    if job["gap"] is not None:
        s["reduced"] = f * p.reduced_w * p.reduced_h * c
    if k in ("tensor", "host_tensor"):
        s["tensor-bytes"] = f * ((job["ow"] * job["oh"] * c + 3) & ~3)
    if k.startswith("host_"):
        s["stage"] = f * c * job["w"] * job["h"] + int(np.prod(out_spec(job)[0])) * out_spec(job)[1].itemsize
    return s


def ascending(jobs):
    return sorted(jobs, key=lambda j: (sum(scratch(j).values()), j["name"]))


# ---- launching (GPU) ------------------------------------------------------------------------------------------------------------
def to_device(arr):
    import torch
    arr = np.ascontiguousarray(arr)
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(arr.dtype)
    return torch.from_numpy(arr.view(view) if view else arr).cuda()


def device_inputs(job):
    return {k: to_device(v) for k, v in inputs(job).items() if k != "full"}


def device_output(job):
    import torch
    shape, dt = out_spec(job)
    tdt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.int16, np.dtype(np.uint32): torch.int32,
           np.dtype(np.float32): torch.float32}[dt]
    return torch.zeros(shape, dtype=tdt, device="cuda")


def to_host(job, t):
    return t.cpu().numpy().view(out_spec(job)[1])


def launch(job, ctx, dev, out, stream, set_force=True):
    """The job's device entry on `stream` (a raw handle); dev / out as device_inputs / device_output.  set_force: the job's
    lanczos_resize_force is set around the call (a context of the caller's own); False on a shared context."""
    k, f = job["kind"], job["frames"]
    if k in ("upscale", "planar"):
        rows = _rows(job)[0] if job["rows"] else 0
        d = L.make_desc(job["w"], job["h"], job["c"], job["sn"], job["sd"], job["a"], 1, job["mode"], 0, rows)
        if k == "planar":
            ctx.resample_planar_device(d, dev["img"].data_ptr(), out.data_ptr(), f, stream)
        else:
            ctx.resample_device(d, dev["img"].data_ptr(), out.data_ptr(), f, 0, 0, stream)
        return
    if k == "reduce":
        ctx.reduce_device(job["w"], job["h"], job["c"], job["factor"], dev["img"].data_ptr(), out.data_ptr(), f, box=job["box"],
                          stream=stream)
        return
    d = resize_desc(job)
    if set_force:
        ctx.resize_force(job["force"])
    try:
        if k == "resize":
            ctx.resize_device(d, dev["img"].data_ptr(), out.data_ptr(), f, stream=stream, box=job["box"], reducing_gap=job["gap"],
                              window=job["window"])
        else:
            assert k == "tensor", k
            oc = _out_channels(job)
            w, h = job["crop"] if job["crop"] is not None else (job["window"][2:] if job["window"] is not None else (job["ow"], job["oh"]))
            ctx.resize_tensor_device(d, dev["img"].data_ptr(), out.data_ptr(), f, dev["lut"].data_ptr(),
                                     L.tensor_strides(job["layout"], w, h, oc), stream=stream, box=job["box"], reducing_gap=job["gap"],
                                     dtype=job["tdtype"], window=job["window"], channels_out=job["channels_out"],
                                     d_flip=dev["flip"].data_ptr() if "flip" in dev else None, crop=job["crop"],
                                     d_origin=dev["origin"].data_ptr() if "origin" in dev else None)
    finally:
        if set_force:
            ctx.resize_force(L.RESIZE_AUTO)


def host_call(job, ctx):
    """The job's synchronous host entry; returns the result shaped and typed as expected()"""
    k, x = job["kind"], inputs(job)["img"]
    if k == "host_resample":
        return ctx.resample(x, job["sn"], job["sd"], job["a"], job["mode"])
    if k == "host_resize":
        return ctx.resize(x, job["ow"], job["oh"], box=job["box"], reducing_gap=job["gap"])
    assert k == "host_tensor", k
    got = ctx.resize_tensor(x, job["ow"], job["oh"], lut=inputs(job)["lut"], layout=job["layout"], dtype=job["tdtype"])
    return TV.words(got)


def report_errors(job, ctx):
    """what the context's last_* reports say against the job's, as a list of messages (empty: as named)"""
    r, want, bad = ctx.last_route(), job["report"], []
    if want["kernel"] is not None and ctx.last_kernel() != want["kernel"]:
        bad.append(f"last_kernel {ctx.last_kernel()}, not {want['kernel']}")
    if want["main"] or want["prefix"]:
        if (r.main, r.prefix, r.launches) != (want["main"], want["prefix"], 1):
            bad.append(f"route {r}, not {L.ROUTE_MAIN_NAMES[want['main']]}+{L.ROUTE_PREFIX_NAMES[want['prefix']]} x1")
    elif r.launches:
        bad.append(f"route {r} after a call that is no upscale")
    if ctx.last_tensor_route() != want["tensor"]:
        bad.append(f"last_tensor_route {ctx.last_tensor_route()}, not {want['tensor']}")
    return [f"{job['name']}: {b}" for b in bad]


def output_errors(job, got, what=""):
    """`got` (numpy, as to_host gives it) against the expected bytes: exact jobs bit for bit; LSB1 jobs within one LSB and, frame
    by frame, lsb1_check.check.  A list of messages."""
    want = expected(job)
    tag = f"{job['name']}{' ' + what if what else ''}"
    if got.shape != want.shape or got.dtype != want.dtype:
        return [f"{tag}: {got.dtype}{got.shape}, not {want.dtype}{want.shape}"]
    if job["check"] == "exact":
        n = int(np.count_nonzero(got != want))
        return [f"{tag}: {n} of {want.size} elements differ from the model"] if n else []
    bad = []
    for i, frame in enumerate(got):
        try:
            LC.check(inputs(job)["full"][i], job["sn"], job["sd"], job["a"], np.ascontiguousarray(frame), LC.FAMILY_FAST,
                     f"{tag}, frame {i}", threads=4)
        except AssertionError as e:
            bad.append(str(e))
    return bad
