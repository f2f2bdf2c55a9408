"""The job table of the concurrency tests (tests/concurrency_cfg.py), checked without a GPU: every expected array can be produced,
every route the tests promise to cover is named by a job -- and is the route the library's own host-side plans choose for the
job's request --, and the jobs that share one context all need different amounts of scratch, so that walking them in ascending
order makes every kind of scratch block grow."""
import numpy as np
import pytest

import concurrency_cfg as C
import lanczos_hls_amd as L


@pytest.mark.parametrize("job", C.TABLE + C.SHARED + C.SHARED_HOST, ids=lambda j: j["name"])
def test_expected_bytes_can_be_produced(job):
    ins, want = C.inputs(job), C.expected(job)
    shape, dt = C.out_spec(job)
    assert want.shape == shape and want.dtype == dt and want.size > 0 and not want.flags.writeable
    assert ins["img"].shape[0] == job["frames"] == want.shape[0]
    assert max(job["w"], job["h"]) <= 256 and min(job["w"], job["h"]) <= 160, "nothing needs more than about 256 x 160 input"
    assert C.expected(job) is want, "computed once and shared"
    if job["check"] == "lsb1":
        assert job["kind"] == "upscale" and not job["rows"], "lsb1_check.check wants whole frames"
        assert any("differ" in e or "LSB" in e for e in C.output_errors(job, np.array(want) ^ 4)), "the check sees a wrong sample"
    if job["kind"] in ("upscale", "planar", "host_resample"):
        # more than one workgroup: more than one 128-column block of the prefix kernels, and of every main kernel's tiles
        assert want[0].size // job["c"] > 128 * 8


def test_every_route_is_named():
    named = {r for j in C.TABLE for r in j["routes"]}
    assert named == set(C.ROUTES), (set(C.ROUTES) - named, named - set(C.ROUTES))
    assert all(j["routes"] for j in C.TABLE), "a job of the table stands for a route"
    names = [j["name"] for j in C.TABLE + C.SHARED + C.SHARED_HOST]
    assert len(set(names)) == len(names)


def test_upscale_jobs_reach_the_kernels_they_name():
    """What can be told on the host: 16-byte rows for k_march, rows off 16 bytes with dword output rows for the tile kernel, a
    periodic / non-periodic rational scale, ragged output rows for k_generic, and a front strip that ends at the last prefix row."""
    for j in C.TABLE + C.SHARED:
        if j["kind"] not in ("upscale", "planar", "host_resample"):
            continue
        in_pitch, out_pitch = j["w"] * j["c"], j["w"] * j["sn"] // j["sd"] * j["c"]
        main = j["report"]["main"]
        if main == C.MARCH or j["name"] == "front":
            assert in_pitch % 16 == 0 and j["sd"] == 1, j["name"]
        if main == C.TILE:
            assert in_pitch % 16 != 0 and out_pitch % 4 == 0 and j["sd"] == 1, j["name"]
        if main in (C.RATP, C.RAT):
            assert j["sd"] != 1 and out_pitch % 4 == 0, j["name"]
        if main == C.GENERIC:
            assert out_pitch % 4 != 0, j["name"]
        d = L.make_desc(j["w"], j["h"], j["c"], j["sn"], j["sd"], j["a"], 1, j["mode"])
        if j["report"]["prefix"] != L.ROUTE_PREFIX_NONE:
            assert L.inplace_rows(d) > 0, j["name"]
        if j["name"] == "front":
            rows, in_rows = C._rows(j)
            assert rows == L.inplace_rows(d) and 0 < in_rows <= j["h"], (rows, in_rows)
    assert C.BY_NAME["hls"]["report"]["prefix"] == L.ROUTE_PREFIX_NONE


def test_resize_jobs_are_planned_as_they_are_named():
    """lanczos_resize_plan_host and its siblings (no GPU) say what AUTO launches for a request: fused where the table says so,
    a reduction where the job has a gap, and a window / crops plan that fits the fused kernel."""
    for j in C.TABLE:
        if j["kind"] not in ("resize", "tensor"):
            continue
        if j["filter"] == "nearest":
            assert j["report"]["kernel"] == C.NEAREST and j["force"] == L.RESIZE_AUTO
            continue
        p = C.plan_ex(j)
        assert p.pass_h and p.pass_v, j["name"]
        forced_off = j["force"] == L.RESIZE_TWO_PASS
        assert j["report"]["kernel"] == (C.TWO_PASS if forced_off else C.FUSED), j["name"]
        assert p.inner.fused == 1, f"{j['name']}: AUTO would not fuse this request: {p.inner.fused}"
        assert p.inner.strips * p.inner.chunks * j["frames"] > 1, f"{j['name']}: one workgroup"
        if j["gap"] is not None:
            assert p.fx > 1 and p.fy > 1, j["name"]
        if j["kind"] == "tensor":
            converted = j["force"] in (L.RESIZE_TWO_PASS, L.RESIZE_CONVERT)
            assert j["report"]["tensor"] == (L.TENSOR_CONVERTED if converted else L.TENSOR_FUSED), j["name"]
    for j in C.SHARED + C.SHARED_HOST:   # forced to the two-pass path: both passes run, so the intermediate is used
        if j["kind"] in ("resize", "tensor", "host_resize", "host_tensor"):
            p = C.plan_ex(dict(j, crop=None))
            assert p.pass_h and p.pass_v and j["report"]["kernel"] == C.TWO_PASS, j["name"]
            assert j["report"]["tensor"] == (L.TENSOR_CONVERTED if "tensor" in j["kind"] else 0), j["name"]
            assert j["gap"] is None or (p.fx > 1 and p.fy > 1), j["name"]


@pytest.mark.parametrize("group", ["SHARED", "SHARED_HOST"])
def test_no_two_jobs_of_a_shared_context_need_the_same_scratch(group):
    jobs = getattr(C, group)
    sizes = {j["name"]: C.scratch(j) for j in jobs}
    assert all(sizes.values()), "every job of the group holds context scratch"
    for kind in C.SCRATCH_KINDS:
        of_kind = [(s[kind], n) for n, s in sizes.items() if kind in s]
        assert len({b for b, _ in of_kind}) == len(of_kind), f"{kind}: {sorted(of_kind)}"
        if group == "SHARED":
            assert len(of_kind) >= 2, f"{kind}: the block never grows"
    if group == "SHARED":
        assert {k for s in sizes.values() for k in s} == set(C.SCRATCH_KINDS)
    order = C.ascending(jobs)
    totals = [sum(C.scratch(j).values()) for j in order]
    assert totals == sorted(totals) and len(set(totals)) == len(totals)
    # walked in this order every kind of block is replaced at least once after its first allocation
    for kind in {k for s in sizes.values() for k in s}:
        seq = [C.scratch(j)[kind] for j in order if kind in C.scratch(j)]
        assert any(b > max(seq[:i]) for i, b in enumerate(seq) if i), f"{kind}: {seq}"


def test_the_fifth_threads_settings_change_no_bytes():
    """force_kernel(FAST) is what AUTO picks for every upscale job of the shared group; the resize force is the group's own."""
    for j in C.SHARED:
        if j["kind"] in ("planar", "host_resample"):
            assert j["report"]["kernel"] == L.KERNEL_FAST and j["mode"] != L.MODE_HLS, j["name"]
    assert set(C.SHARED_SETTINGS["force_kernel"]) == {L.KERNEL_FAST, L.KERNEL_NONE}
    assert C.SHARED_SETTINGS["resize_force"] == L.RESIZE_TWO_PASS
